"""fgnn_math_ranged.h against fgnn_math.h, bit for bit, on the CPU (no GPU).

The BP4 kernels evaluate the log of a log-sum-exp with fg_log_1to2, which forms the exponent term of fg_log without the int -> float
conversion; that is only the same float if the argument stays in [1, 2].  tests/math_ranged_check.c walks every float of [1, 2] and a
grid of log-sum-exp argument pairs (equal arguments, |a - b| one ulp either side of the clamp at 20, zeros of both signs, magnitudes
to 1e4) and exits non-zero on the first differing bit pattern.  Compiled with the flags the oracle is compiled with.
"""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranged_log_and_lse2_equal_the_general_routines_bitwise():
    src = os.path.join(ROOT, "tests", "math_ranged_check.c")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "math_ranged_check")
        cc = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function", "-I" + inc, src,
                             "-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "log_1to2: 8388609 values, 0 mismatches" in run.stdout
    assert ", 0 mismatches" in run.stdout.splitlines()[-1] and run.stdout.splitlines()[-1].startswith("lse2:")
