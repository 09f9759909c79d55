"""fg_phi_med / fg_softplus_max of fgnn_math_ranged.h against fg_phi / fg_softplus of fgnn_math.h, bit for bit.

The BP4 kernels end a phi with a median (v_med3_f32) and a softplus with a maximum (v_max_f32) where fgnn_math.h, which the oracle
compiles, compares the argument with the softplus threshold and selects.  That is the same float only because the computed
log1p(exp(x)) is ordered against x and against S = log1p(exp(threshold)) the right way on every input, which is a property of the
rounded routines and not of the real functions: tests/math_select_check.c walks every float of phi's clip range (231 640 148), points and
sweeps outside it on both sides, and every finite float of both signs for the softplus (4 278 190 080), compiled with the flags the
oracle is compiled with and split over the host's threads with OpenMP.  On the device the two forms are other instructions than the
CPU's min / max composition: tests/math_selects_gpu.hip evaluates both forms there on the inputs where the selects switch.
"""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_median_and_maximum_forms_equal_the_selects_bitwise():
    src = os.path.join(ROOT, "tests", "math_select_check.c")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "math_select_check")
        cc = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-function", "-I" + inc,
                             src, "-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "phi clip range: 231640148 values, 0 mismatches" in run.stdout
    assert "softplus: 4278190080 values, 0 mismatches" in run.stdout
    assert "phi outside the clip range" in run.stdout and "mismatch at" not in run.stdout


@pytest.mark.gpu
def test_device_forms_equal_the_selects_on_the_select_bands():
    """v_med3_f32 / v_max_f32 against v_cmp + v_cndmask on the device: 0 differing bit patterns, and the CRC-32 of the device's outputs
    equals that of the host build's fg_phi / fg_softplus on the same inputs."""
    import __graft_entry__ as entry
    exe = entry.build_math_selects_gpu()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    lines = {l.split(":")[0]: l for l in res.stdout.splitlines() if ":" in l}
    for name in ("phi", "softplus"):
        assert ", 0 differences on the device" in lines[name], res.stdout
        crc = lines[name].rsplit("crc device ", 1)[1].split()
        assert crc[0] == crc[2], res.stdout
    # every float of [13.9, 14.8] (ulp 2^-20) and of |t| in [13.9, 16.3], [86.9, 87.1], both signs
    assert int(lines["phi"].split("(")[1].split()[0]) == 943720
    assert int(lines["softplus"].split("(")[1].split()[0]) == 4771024
