"""The fixtures shared by tests/test_stpost_reference_cpu.py and tests/test_gpu_stpost.py (a plain module: tests import it, pytest does
not): seeded windows on the two codes, a short schedule and rates high enough that space-time BP4 leaves windows unsolved.

The tiny code is hypergraph_product(rep_code(3), hamming_code(3)): 27 qubits, 14 hx and 9 hz checks of several degrees, so the
runtime-degree loop runs with unequal sides and several windows share a workgroup.  ghp882 is [[882,24]], (3,3,6)-regular: min-sum
runs the packed-row instantiation.  Per case: code, rounds, windows, p, q, seed.  The CPU test checks, for every case, that the
restatement leaves at least a quarter of the windows unsolved and solves at least two (6 min-sum iterations at factor 0.8, one alpha,
gamma = log((1-q)/q), a perfect last read-out), and that LOW_CAP pivots leave LSD with found = 0 and found = 1 windows."""
import functools

import numpy as np

import mbp4_reference as MB
from feedback_gnn_amd import codes_q as cq
from helpers import code, llr_const
from stpost_reference import draw_windows

INF = float("inf")
Q = 0.03
NUM_ITER = 6

CASES = {
    "tiny_r1": ("tiny", 1, 24, 0.15, 0),
    "tiny_r2": ("tiny", 2, 24, 0.08, 0),
    "tiny_r3": ("tiny", 3, 24, 0.08, 0),
    "ghp_r1": ("ghp882", 1, 8, 0.04, 2),
    "ghp_r2": ("ghp882", 2, 8, 0.04, 1),
    "ghp_r3": ("ghp882", 3, 8, 0.03, 1),
    "ghp_r5": ("ghp882", 5, 8, 0.02, 2),
}
LOW_CAP = {"tiny_r1": 4, "tiny_r2": 4, "tiny_r3": 4, "ghp_r2": 55}


@functools.lru_cache(maxsize=None)
def tiny_code():
    return cq.hypergraph_product(cq.rep_code(3), cq.hamming_code(3))


def case_code(case):
    name = CASES[case][0]
    return tiny_code() if name == "tiny" else code(name)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(synd_x [B,R,m_x], synd_z [B,R,m_z]) uint8 of the case; read-only, shared between tests."""
    _, R, B, p, seed = CASES[case]
    sx, sz = draw_windows(case_code(case), R, B, p, Q, seed)
    sx.setflags(write=False)
    sz.setflags(write=False)
    return sx, sz


def gamma_of(q):
    """log((1-q)/q) in float32 arithmetic."""
    q = np.float32(q)
    return float(np.log((np.float32(1.0) - q) / q, dtype=np.float32))


def case_settings(case, alphas=(1.0,), cn_type="minsum", restart=True):
    """The keyword arguments of `stbp4_reference.stbp4_decode` for the case's base configuration."""
    factors, owns = MB.mbp4_tables(alphas, 0.8)
    g = gamma_of(Q)
    return dict(factors=factors, owns=owns, pre_iter=NUM_ITER, attempt_iter=NUM_ITER, cn_type=cn_type, restart=restart,
                llr_const=llr_const(CASES[case][3]), gamma_x=g, gamma_z=g, gamma_last_x=INF, gamma_last_z=INF)


@functools.lru_cache(maxsize=None)
def _variant_arrays(case):
    sx, sz = case_inputs(case)
    B, n = sx.shape[0], case_code(case).hx.shape[1]
    rng = np.random.default_rng(1000 + CASES[case][4])
    g = gamma_of(Q)
    dx, dz = 0.6 / sx.shape[2], 0.6 / sz.shape[2]  # a defect in about every other window and side
    out = dict(prev_x=(rng.random((B, sx.shape[2])) < dx).astype(np.uint8), prev_z=(rng.random((B, sz.shape[2])) < dz).astype(np.uint8),
               llr_ch=(llr_const(CASES[case][3]) + rng.normal(0.0, 0.1, (B, 3, n))).astype(np.float32),
               synd_llr_x=(g + rng.normal(0.0, 0.5, sx.shape)).astype(np.float32))
    out["synd_llr_x"][:, -1] = np.float32(INF)  # the last read-out is perfect, as in the base configuration
    for a in out.values():
        a.setflags(write=False)
    return out


def case_variant(case, alphas=(1.0, 0.8, 0.6), cn_type="minsum", restart=True):
    """The second configuration of a case: a sparse `prev` on both sides, per-qubit priors around the case's, per-check syndrome LLRs
    on the hx side (+inf in the last round) and the scalar gamma with gamma_last = +inf on the hz side, and an alpha sweep of 6 + 4 + 4 iterations."""
    kw = case_settings(case, alphas, cn_type, restart)
    kw.update(pre_iter=NUM_ITER, attempt_iter=4, **_variant_arrays(case))
    del kw["llr_const"]
    return kw
