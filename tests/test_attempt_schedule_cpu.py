"""The attempt schedule of mbp4_kernel, dsbp4_kernel and stbp4_kernel (feedback_gnn_amd/csrc/fgnn_attempts.h): tests/attempt_ctl_check.cpp
walks `AttemptCtl` as the kernels' step loop does, up to `attempt_step_bound`, and this compares every case with the nested loops of
`mbp4_reference.mbp4_decode`, restated on the plan "the decision first reproduces the syndrome at test (a, k)".  CPU only."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2**31 - 1


def build_and_run(flags):
    src = os.path.join(ROOT, "tests", "attempt_ctl_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attempt_ctl_check")
        cc = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function"] + flags +
                            ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    return run.stdout.split("\n")[:-1]


def reference(pre_iter, attempt_iter, attempts, restart, stop):
    """The loops of `mbp4_decode` for one sample whose test passes at stop = (a, k) and nowhere else (None: never): the stats words
    (found, the a of the last test, iterations, the k of the last test) and the attempts that began from zero messages."""
    stats, zeroed = [0, 0, 0, 0], []
    for a in range(attempts):
        T = pre_iter if a == 0 else attempt_iter
        if restart and a > 0:
            zeroed.append(a)
        for k in range(1, T + 1):
            stats = [0, a, stats[2] + 1, k]
            if stop == (a, k):
                stats[0] = 1
                return stats, zeroed
    return stats, zeroed


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_walk_of_the_header_is_the_loops_of_the_restatement(flags):
    lines = build_and_run(flags)
    assert int(lines[0]) == INT_MAX - 1, "the bound saturates: pre_iter = attempt_iter = INT_MAX, 64 attempts"
    want = [(p, i, A, rs, stop) for p in range(1, 5) for i in range(1, 5) for A in range(1, 5) for rs in (0, 1)
            for stop in [(a, k) for a in range(A) for k in range(1, (p if a == 0 else i) + 1)] + [None]]
    assert len(lines) == 1 + len(want) and sum(stop is None for *_, stop in want) == 4 * 4 * 4 * 2
    for line, (p, i, A, rs, stop) in zip(lines[1:], want):
        case, stats, steps, zeroed = (part.split() for part in line.split("|"))
        assert [int(x) for x in case] == [p, i, A, rs, *(stop or (-1, 0))], line
        assert "unused" not in zeroed, line
        finished, seen, bound = (int(x) for x in steps)
        ref_stats, ref_zeroed = reference(p, i, A, bool(rs), stop)
        assert [int(x) for x in stats] == ref_stats, line
        # attempt a begins at the step after the T + 1 steps of each attempt before it; its test k is its step k + 1
        first = [1 + sum((p if b == 0 else i) + 1 for b in range(a)) for a in range(A)]
        assert [int(x) for x in zeroed] == [first[a] for a in ref_zeroed], line
        assert bound == p + 1 + (A - 1) * (i + 1) + 1 and 1 <= finished <= bound - 1 and seen == finished + 1, line
        if stop is None:
            assert finished == bound - 1, "the bound is tight: " + line
        else:
            assert finished == first[stop[0]] + stop[1], line
