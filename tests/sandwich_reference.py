"""Stage-by-stage restatement of Sandwich_BP_GNN_Evaluation_Model.call between the syndromes and the residual check
(feedback_gnn.py:321-340), and of the residual check itself (:343-361), as plain functions.

The decoders and the feedback GNNs are the CPU oracle's SINGLE stages (`og.bp4_decode`, `og.feedback_gnn`,
`og.feedback_gnn_general`); everything that joins them (the flag test, the `errors` mask, the masked merge, the round counter) is dense
NumPy written as the reference writes it: int64 matrix products followed by `% 2`, `np.where` for the scatter update.  None of these functions
calls `og.sandwich_decode` or the oracle's `syndrome` / `residual`, so a masking mistake shared by the library's driver and the oracle's driver
does not pass.
"""
import functools

import numpy as np


def _dense(mat):
    return np.asarray(mat).astype(np.int64)


def dense_syndrome(code, ex, ez):
    """syndrome_x = hx noise_z, syndrome_z = hz noise_x (feedback_gnn.py:305-309) as int64 products mod 2."""
    sx = (np.asarray(ez).astype(np.int64) @ _dense(code.hx).T) % 2
    sz = (np.asarray(ex).astype(np.int64) @ _dense(code.hz).T) % 2
    return sx.astype(np.uint8), sz.astype(np.uint8)


def dense_flagged(code, x_hat, z_hat, synd_x, synd_z):
    """new_errors of feedback_gnn.py:324-328: does the estimate fail to reproduce the syndrome?  (bool [B])"""
    x_hat, z_hat = np.asarray(x_hat).astype(np.int64), np.asarray(z_hat).astype(np.int64)
    bad_z = ((x_hat @ _dense(code.hz).T) % 2 != np.asarray(synd_z).astype(np.int64)).any(1)
    bad_x = ((z_hat @ _dense(code.hx).T) % 2 != np.asarray(synd_x).astype(np.int64)).any(1)
    return bad_z | bad_x


def dense_residual(code, ex, ez, x_hat, z_hat, rows_x=None, rows_z=None):
    """(s_hat [B, m_z + m_x], ls_hat, flags) of feedback_gnn.py:343-361; flags = any(s_hat) | any(ls_hat) << 1 (metrics.py:221-223).
    ``rows_x`` / ``rows_z``: the matrices applied to the x / z difference for ls_hat (default hx_perp / hz_perp; BP4_OSD_Model uses
    lz / lx)."""
    rows_x = code.hx_perp if rows_x is None else rows_x
    rows_z = code.hz_perp if rows_z is None else rows_z
    xd = (np.asarray(ex) ^ np.asarray(x_hat)).astype(np.int64) & 1
    zd = (np.asarray(ez) ^ np.asarray(z_hat)).astype(np.int64) & 1
    s_hat = np.concatenate([(xd @ _dense(code.hz).T) % 2, (zd @ _dense(code.hx).T) % 2], axis=1).astype(np.uint8)
    ls_hat = np.concatenate([(xd @ _dense(rows_x).T) % 2, (zd @ _dense(rows_z).T) % 2], axis=1).astype(np.uint8)
    flags = (s_hat.any(1).astype(np.uint8) | (ls_hat.any(1).astype(np.uint8) << 1)).astype(np.uint8)
    return s_hat, ls_hat, flags


def sandwich_reference(og, synd_x, synd_z, iters, weights_list, llr_const, factors=None, cn_types=None, gnn_cfgs=None):
    """The BP / GNN / BP ... stack on given syndromes.  ``og``: an OracleGraph (stage_one).  ``weights_list[i]``: the weight arrays of
    feedback GNN i; ``gnn_cfgs[i]`` (optional): its integer-coded constructor setting for `og.feedback_gnn_general`, None = the shipped
    architecture (`og.feedback_gnn`).  Returns dict(x_hat, z_hat, rounds, llr, llr_compact):
      llr          the marginals of the last decoder of the stack, for every sample (what the reference computes);
      llr_compact  sample b holds the marginals of decoder number rounds[b] — the last decoder that runs on it when every round is
                   restricted to the samples still in `errors`."""
    num_layers = len(iters)
    assert len(weights_list) == num_layers - 1
    factors = [1.0] * num_layers if factors is None else list(factors)
    cn_types = ["boxplus-phi"] * num_layers if cn_types is None else list(cn_types)
    gnn_cfgs = [None] * (num_layers - 1) if gnn_cfgs is None else list(gnn_cfgs)
    code = og.code
    synd_x = np.ascontiguousarray(synd_x, dtype=np.uint8)
    synd_z = np.ascontiguousarray(synd_z, dtype=np.uint8)
    B = synd_x.shape[0]
    o = og.bp4_decode(synd_x, synd_z, iters[0], cn_types[0], factors[0], llr_const=llr_const)  # decoders[0] (:321)
    x_hat, z_hat = o["x_hat"].copy(), o["z_hat"].copy()
    errors = np.ones(B, dtype=bool)  # (:322)
    rounds = np.zeros(B, dtype=np.int64)
    llrs = [o["llr"]]
    for i in range(1, num_layers):
        errors &= dense_flagged(code, x_hat, z_hat, synd_x, synd_z)  # (:324-330)
        rounds += errors
        # feedbacks[i-1]((h_vn, logit_hz_perp, logit_hx_perp, ...)) (:335): stage-one logit_hx = z_logit, logit_hz = x_logit
        if gnn_cfgs[i - 1] is None:
            new = og.feedback_gnn(weights_list[i - 1], o["llr"], o["z_logit"], o["x_logit"], synd_x, synd_z)
        else:
            new = og.feedback_gnn_general(gnn_cfgs[i - 1], weights_list[i - 1], o["llr"], o["z_logit"], o["x_logit"], synd_x, synd_z)
        o = og.bp4_decode(synd_x, synd_z, iters[i], cn_types[i], factors[i], llr_ch=new)  # (:336)
        x_hat = np.where(errors[:, None], o["x_hat"], x_hat)  # (:339-340)
        z_hat = np.where(errors[:, None], o["z_hat"], z_hat)
        llrs.append(o["llr"])
    llr_compact = np.stack(llrs)[rounds, np.arange(B)] if B else o["llr"].copy()
    return dict(x_hat=x_hat.astype(np.uint8), z_hat=z_hat.astype(np.uint8), rounds=rounds.astype(np.uint8), llr=o["llr"],
                llr_compact=np.ascontiguousarray(llr_compact))


# The shape table of the driver tests (tests/test_sandwich_reference_cpu.py, tests/test_gpu_sandwich_shapes.py): seed 0x5EED, first sample
# 31, llr_const(0.05), the shipped [[882,24]] weights in every feedback GNN, boxplus-phi at factor 1.0.  `hist` = np.bincount(rounds,
# minlength=4) of the CPU oracle: how many samples stop after 0, 1, 2, 3 feedback rounds.
SEED = 0x5EED
FIRST_SAMPLE = 31
CASES = {
    # name: (code, p, B, iters, hist)
    "rsurf5": ("rsurf5", 0.07, 70, [1, 2, 4, 8], [31, 7, 4, 28]),  # irregular, 32 threads x 8 codewords per workgroup
    "surf3": ("surf3", 0.07, 70, [1, 2, 4, 8], [41, 3, 14, 12]),  # irregular, m_x != n/2, 16 codewords per workgroup
    "rsurf3": ("rsurf3", 0.07, 70, [1, 1, 2, 12], [43, 4, 11, 12]),  # n = 9, 16 codewords per workgroup
    "gb48": ("gb48", 0.07, 70, [2, 3, 5, 8], [36, 0, 0, 34]),  # degree-4 regular kernels, 4 codewords per workgroup
    "hp_c7": ("hp_c7", 0.06, 45, [3, 3, 6, 12], [33, 0, 0, 12]),  # fused flag test at 128 threads per codeword
    "ghp882": ("ghp882", 0.09, 45, [16, 8, 8, 8], [21, 9, 4, 11]),  # default launch (fused) and set_launch(128, 2)
}
# rows in which the flagged list shrinks in every round (index2 != index in rounds 2 and 3)
SHRINKING = ("rsurf5", "surf3", "rsurf3", "ghp882")


def case_inputs(og, name):
    """(ex, ez, sx, sz) of one row of CASES on the oracle's Philox stream; the syndromes are the dense products."""
    _, p, B, _, _ = CASES[name]
    ex, ez = og.pauli_noise(SEED, p, FIRST_SAMPLE, B)
    sx, sz = dense_syndrome(og.code, ex, ez)
    return ex, ez, sx, sz


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """One row of CASES, computed once per session and shared by the tests (read-only arrays): dict(ex, ez, sx, sz, weights, ref) with
    ref = sandwich_reference(...) on the library-default oracle graph."""
    from feedback_gnn_amd.weights_io import read_weight_list
    from helpers import WEIGHTS_882, llr_const, oracle_library_forms
    cname, _, _, iters, _ = CASES[name]
    og = oracle_library_forms(cname)
    ex, ez, sx, sz = case_inputs(og, name)
    w = read_weight_list(WEIGHTS_882)
    ref = sandwich_reference(og, sx, sz, iters, [w] * (len(iters) - 1), llr_const(0.05))
    for a in (ex, ez, sx, sz, *ref.values()):
        a.setflags(write=False)
    return dict(ex=ex, ez=ez, sx=sx, sz=sz, weights=w, ref=ref)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """The oracle's own driver (`og.sandwich_decode`) on the same row: the second checker of the GPU tests, held to `case_reference`
    by tests/test_sandwich_reference_cpu.py."""
    from helpers import llr_const, oracle_library_forms
    cname, _, _, iters, _ = CASES[name]
    c = case_reference(name)
    o = oracle_library_forms(cname).sandwich_decode(c["sx"], c["sz"], iters, [c["weights"]] * (len(iters) - 1), llr_const(0.05),
                                                    return_llr=True)
    for a in o.values():
        a.setflags(write=False)
    return o
