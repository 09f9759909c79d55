"""The leg / stop / weight control of relay_kernel and relay4_kernel (feedback_gnn_amd/csrc/fgnn_legs.h): tests/leg_ctl_check.cpp walks
`LegCtl` as the kernels' step loops do, up to `attempt_step_bound`, and this compares every case with the leg loops of
`relay_reference.relay_decode`, restated on the plan "these tests (r, k) reproduce the syndrome, and test t weighs WEIGHTS[row][t]".
CPU only."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2**31 - 1
# as in leg_ctl_check.cpp: ties, a strictly smaller later weight, a larger later weight, a mix with zeros and negative weights
WEIGHTS = [[4] * 9, [9, 8, 7, 6, 5, 4, 3, 2, 1], [1, 2, 3, 4, 5, 6, 7, 8, 9], [3, 0, 3, -2, 0, 5, -2, 3, 0]]


def build_and_run(flags):
    src = os.path.join(ROOT, "tests", "leg_ctl_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "leg_ctl_check")
        cc = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-function"] + flags +
                            ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    return run.stdout.split("\n")[:-1]


def reference(pre_iter, leg_iter, num_legs, stop_nconv, passes, weight):
    """The leg loops of `relay_decode` for one sample whose tests in `passes` pass and whose test (r, k) weighs weight[r, k]: found,
    (weight, leg, k) of the output (the first solution, a later one only if strictly lighter; with none the last test made), the tests
    whose decisions became the output, in order, and the workgroup step of the last test (a leg's step k = 0 tests nothing, its test k
    is k steps later, and the next leg begins in the step after the leg's last test)."""
    found, best, last, written, step = 0, None, None, [], 0
    for r in range(num_legs):
        step += 1
        for k in range(1, (pre_iter if r == 0 else leg_iter) + 1):
            step += 1
            last = (weight[r, k], r, k)
            if (r, k) in passes:
                found += 1
                if found == 1 or last[0] < best[0]:
                    best = last
                    written.append((r, k))
                break
        if found >= stop_nconv:
            break
    if found == 0:
        best = last
        written.append(last[1:])
    return found, best, written, step


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_walk_of_the_header_is_the_leg_loops_of_the_restatement(flags):
    lines = build_and_run(flags)
    assert int(lines[0]) == INT_MAX - 1, "the bound saturates: pre_iter = leg_iter = num_legs = INT_MAX"
    want = [(p, i, n, s, plan, row) for p in range(1, 4) for i in range(1, 4) for n in range(1, 4) for s in range(1, 4)
            for plan in range(1 << (p + (n - 1) * i)) for row in range(4)]
    assert len(lines) == 1 + len(want)
    kinds = set()
    for line, (p, i, n, s, plan, row) in zip(lines[1:], want):
        case, stats, steps, out = (part.split() for part in line.split("|"))
        assert [int(x) for x in case] == [p, i, n, s, plan, row], line
        tests = [(r, k) for r in range(n) for k in range(1, (p if r == 0 else i) + 1)]
        passes = {t for j, t in enumerate(tests) if plan >> j & 1}
        weight = {t: WEIGHTS[row][j] for j, t in enumerate(tests)}
        found, best, written, last_step = reference(p, i, n, s, passes, weight)
        assert [int(x) for x in stats] == [found, *best], line
        assert [tuple(int(x) for x in w.split(".")) for w in out] == written, line
        finished, stats_at, seen, bound = (int(x) for x in steps)
        assert bound == p + 1 + (n - 1) * (i + 1) + 1 and finished == last_step <= bound - 1, line
        assert stats_at == seen == finished + 1, "the stats follow the settle of the last weight, in the step the loop ends: " + line
        if not passes:
            assert found == 0 and finished == bound - 1, "the bound is tight: " + line
        kinds.add("none" if found == 0 else "one" if found == 1 else "replaced" if len(written) > 1 else "first kept")
    assert kinds == {"none", "one", "replaced", "first kept"}
