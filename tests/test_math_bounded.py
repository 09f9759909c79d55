"""The bounded routines of fgnn_math_ranged.h and the two bounds the BP4 launch proves their range from, on the CPU.

bp4_kernel's BND variant evaluates the qubit update's softplus and log-sum-exp without their range guards (fg_softplus_bounded,
fg_lse2_corr_bounded, fg_lse2_bounded): the min(d, 20) in front of the exponential and the clamp / flush below -87.  plan_bp4 picks it
only when the launch arguments keep every argument within FG_BOUNDED_MAX = 80, and that proof stands on two facts checked here:
  * no check-to-qubit message exceeds phi0 = 16.6355324 in magnitude before the factor: fg_phi_med <= phi0 on every float of its clip
    range, at 0 and above the clip (tests/math_bounded_check.c, exhaustive, with the bit comparison of the routines themselves:
    every float of [0, 80] for the log-sum-exp, of [-80, 80] for the softplus, and the slack up to 87);
  * no output of the shipped feedback GNN exceeds max_i (sum_j |W_out[j][i]| + |b_out[i]|) * (1 + 1e-5), the bound fgnn_weights_create
    records for the decoder that reads the output: restated here in NumPy and held against the CPU oracle's GNN on random inputs,
    LLRs of magnitude 100 among them, for every weight file the package ships and for a copy with W_out scaled by 30.
"""
import glob
import os
import subprocess
import tempfile

import numpy as np
import pytest

from feedback_gnn_amd.weights_io import read_weight_list
from helpers import oracle_library_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT_FILES = sorted(glob.glob(os.path.join(ROOT, "feedback_gnn_amd", "weights", "*.npz")))
BOUNDED_MAX_BITS = 0x42A00000  # 80.0f


def test_bounded_routines_equal_the_guarded_ones_bitwise_and_phi_is_bounded():
    src = os.path.join(ROOT, "tests", "math_bounded_check.c")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "math_bounded_check")
        cc = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-function", "-I" + inc,
                             src, "-o", exe, "-lm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "mismatch" not in run.stdout.replace("0 mismatches", "") and "violated" not in run.stdout
    # every float of [0, 80] is bits 0 .. 0x42A00000; [-80, 80] twice that (both zeros)
    assert f"lse2 [0, 80]: {BOUNDED_MAX_BITS + 1} values, 0 mismatches" in run.stdout
    assert f"softplus [-80, 80]: {2 * (BOUNDED_MAX_BITS + 1)} values, 0 mismatches" in run.stdout
    assert "phi <= phi0 on the clip range: 231640148 values, 0 violations" in run.stdout
    assert "phi <= phi0 outside the clip range" in run.stdout and "phi(0) = phi0 = 16.6355324" in run.stdout


def llr_out_bound(weights):
    """fgnn_weights_create's llr_out_bound restated: in double, 1e-5 of relative slack, rounded up to float32."""
    w_out, b_out = np.asarray(weights[0], np.float64), np.asarray(weights[1], np.float64)
    worst = float((np.abs(w_out).sum(axis=0) + np.abs(b_out)).max()) * (1.0 + 1e-5)
    f = np.float32(worst)
    return f if float(f) >= worst else np.nextafter(f, np.float32(np.inf))


def _gnn_inputs(og, B, seed):
    """B codewords of GNN inputs: ordinary marginals and soft syndromes for the first half, saturated ones (LLRs of +-100, soft
    syndromes at +-phi0) for the second, random syndromes."""
    rng = np.random.RandomState(seed)
    llr = rng.uniform(-8.0, 12.0, size=(B, 3, og.n))
    lhx = rng.uniform(-16.6355324, 16.6355324, size=(B, og.m_x))
    lhz = rng.uniform(-16.6355324, 16.6355324, size=(B, og.m_z))
    h = B // 2
    llr[h:] = np.where(rng.rand(B - h, 3, og.n) < 0.5, -100.0, 100.0) * rng.uniform(0.9, 1.0, size=(B - h, 3, og.n))
    lhx[h:] = np.where(rng.rand(B - h, og.m_x) < 0.5, -16.6355324, 16.6355324)
    lhz[h:] = np.where(rng.rand(B - h, og.m_z) < 0.5, -16.6355324, 16.6355324)
    sx = (rng.rand(B, og.m_x) < 0.3).astype(np.uint8)
    sz = (rng.rand(B, og.m_z) < 0.3).astype(np.uint8)
    return llr.astype(np.float32), lhx.astype(np.float32), lhz.astype(np.float32), sx, sz


@pytest.mark.parametrize("path", WEIGHT_FILES, ids=[os.path.basename(p)[:-4] for p in WEIGHT_FILES])
def test_gnn_output_stays_within_the_bound_of_its_weights(path):
    assert WEIGHT_FILES
    og = oracle_library_forms("ghp882" if "n882" in os.path.basename(path) else "ghp1270")
    w = read_weight_list(path)
    B = 8  # 8 x 3 x n outputs: a few thousand qubits' inputs
    args = _gnn_inputs(og, B, 11)
    for scale in (1.0, 30.0):
        ws = [a.copy() for a in w]
        ws[0] = (ws[0] * np.float32(scale)).astype(np.float32)
        bound = llr_out_bound(ws)
        out = og.feedback_gnn(ws, *args)
        worst = float(np.abs(out).max())
        print(f"{os.path.basename(path)} w_out x {scale}: bound {float(bound):.6f}, max |out| {worst:.6f}")
        assert np.isfinite(out).all() and worst <= float(bound)
    # the unscaled bounds keep the proof's totals under 80 at factor 1 (3 * phi0 + 2 * bound + 1), the scaled ones do not
    assert 3 * 16.6355324 + 2 * float(llr_out_bound(w)) + 1 <= 80.0
    assert 3 * 16.6355324 + 2 * float(bound) + 1 > 80.0
