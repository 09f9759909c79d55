"""The sandwich driver (fgnn_sandwich.hip) on the launch shapes no other test reaches: several codewords per workgroup with a partly
filled last workgroup, the non-fused flag path (`fill_u8` + `fgnn_flag_update`, with the previous round's index list from the second
compacted round on), the slot -> sample index in the packed BP4 / GNN kernels, the fused flag test below 256 threads per codeword, and
`return_llr` under compaction.

Every case is held to tests/sandwich_reference.py (the oracle's single stages joined by dense NumPy) and, where the oracle's own driver
takes the case, to `og.sandwich_decode`, by EXACT equality of x_hat, z_hat, rounds and the marginals: the kernels and the oracle share one
float32 operation sequence, so there is no tolerance.  Full mode returns the marginals of the last decoder of the stack; compacted mode
those of the last decoder that ran on each sample (`llr_compact` of the restatement).

The round histograms of the table are asserted on the reference before the GPU is looked at: rows listed in SHRINKING lose samples in
every round, so the compacted list of round i + 1 is a strict subset of round i's and the flag update of rounds 2 and 3 runs on an index
list that differs from the round's own.
"""
import numpy as np
import pytest
import torch

from helpers import GEN_CONFIGS, gen_cfg_codes, gen_weights, gpu_graph, llr_const, oracle_library_forms, to_gpu
from sandwich_reference import CASES, SHRINKING, case_oracle, case_reference, dense_residual, sandwich_reference

pytestmark = pytest.mark.gpu

L0 = llr_const(0.05)
# (threads per codeword, codewords per workgroup) the library's default launch gives each code of the table
DEFAULT_GEOMETRY = {"rsurf5": (32, 8), "surf3": (16, 16), "rsurf3": (16, 16), "gb48": (64, 4), "hp_c7": (128, 1), "ghp882": (256, 1)}


def _dev(a):
    return to_gpu(np.array(a))  # a copy: the shared reference arrays are read-only


def _decode(gg, sx, sz, iters, gws, compact, **kw):
    g = gg.sandwich_decode(_dev(sx), _dev(sz), iters, gws, L0, compact=compact, return_llr=True, return_rounds=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def _assert_driver(g, ref, compact, what, rows=None):
    """GPU result `g` against (the rows `rows` of) a restatement / oracle result: exact, every output."""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    for k in ("x_hat", "z_hat", "rounds"):
        assert np.array_equal(g[k], pick(ref[k])), (what, k, np.argwhere(g[k] != pick(ref[k]))[:4].tolist())
    want = pick(ref["llr_compact"] if compact else ref["llr"])
    bad = np.argwhere((g["llr"] != want).any(axis=(1, 2))).ravel()
    assert bad.size == 0, (what, "llr (compacted)" if compact else "llr", "samples", bad[:8].tolist(), "rounds", pick(ref["rounds"])[bad[:8]].tolist())


def _with_compact_llr(o, ref):
    """The oracle's driver returns the full-mode marginals only: its compacted ones are the restatement's."""
    return dict(o, llr_compact=ref["llr_compact"])


def _shipped_weights(gg, c, iters):
    from feedback_gnn_amd.graph import GnnWeights
    return [GnnWeights(c["weights"], gg.device)] * (len(iters) - 1)


TABLE = [(name, None) for name in CASES] + [("ghp882", (128, 2))]


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name,launch", TABLE, ids=[n if l is None else f"{n}-{l[0]}x{l[1]}" for n, l in TABLE])
def test_driver_equals_the_restatement_on_the_shape_table(name, launch, compact):
    """Every row of the table at the library's default launch, [[882,24]] also at 128 threads x 2 codewords: the driver against the
    restatement and against the oracle's driver, then the residual check on the GPU's estimates.  The graphs are the session's shared
    ones in the library's default forms (the gb48 row is what showed that test_gpu_api.py's option round trip left options 4 and 5 on)."""
    cname, p, B, iters, hist = CASES[name]
    c, o = case_reference(name), case_oracle(name)
    ref = c["ref"]
    # preconditions, on the reference alone
    assert np.bincount(ref["rounds"], minlength=4).tolist() == hist
    if name in SHRINKING:
        assert min(hist) > 0, "the flagged list must shrink in every round"
    for k in ("x_hat", "z_hat", "rounds", "llr"):
        assert np.array_equal(ref[k], o[k]), k
    og, gg = oracle_library_forms(cname), gpu_graph(cname)
    try:
        if launch is not None:
            gg.set_launch(*launch)
        info = gg.info()
        assert (info["threads_per_codeword"], info["codewords_per_block"]) == (launch or DEFAULT_GEOMETRY[name])
        assert B % info["codewords_per_block"] != 0 or info["codewords_per_block"] == 1, "the last workgroup must be partly filled"
        g = _decode(gg, c["sx"], c["sz"], iters, _shipped_weights(gg, c, iters), compact)
        what = f"{name} launch={launch} compact={compact}"
        _assert_driver(g, ref, compact, what + " vs restatement")
        _assert_driver(g, _with_compact_llr(o, ref), compact, what + " vs oracle driver")
        # the residual check on the GPU's estimates (feedback_gnn.py:343-361)
        s1, l1, f1 = (t.cpu().numpy() for t in gg.residual(_dev(c["ex"]), _dev(c["ez"]), _dev(g["x_hat"]), _dev(g["z_hat"])))
    finally:
        if launch is not None:
            gg.set_launch(0, 0)
    for want, who in ((og.residual(c["ex"], c["ez"], ref["x_hat"], ref["z_hat"]), "oracle"),
                      (dense_residual(og.code, c["ex"], c["ez"], ref["x_hat"], ref["z_hat"]), "dense")):
        assert np.array_equal(s1, want[0]) and np.array_equal(l1, want[1]) and np.array_equal(f1, want[2]), (name, who)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name,launch", [("rsurf5", None), ("ghp882", None), ("ghp882", (128, 2))],
                         ids=["rsurf5", "ghp882", "ghp882-128x2"])
def test_forced_runtime_degree_kernels_with_an_index(name, launch, compact):
    """force_generic: the runtime-degree BP4 kernel and `gnn_kernel` take the driver's index list (on [[882,24]] in place of the (3,3,6)
    kernels; at 128 x 2 packed, with the non-fused flag path)."""
    cname, p, B, iters, hist = CASES[name]
    c = case_reference(name)
    ref = c["ref"]
    assert min(np.bincount(ref["rounds"], minlength=4)) > 0
    gg = gpu_graph(cname)
    try:
        gg.force_generic(True)
        if launch is not None:
            gg.set_launch(*launch)
        g = _decode(gg, c["sx"], c["sz"], iters, _shipped_weights(gg, c, iters), compact)
    finally:
        gg.force_generic(False)
        if launch is not None:
            gg.set_launch(0, 0)
    _assert_driver(g, ref, compact, f"{name} generic launch={launch} compact={compact}")


# non-shipped Feedback_GNN settings on rsurf5 (GEN_CONFIGS[2] with the output bias raised so that the new channel LLRs stay in the
# decoder's range, GEN_CONFIGS[1] as it is): (config, weights, histogram of the restatement)
def _general_cases():
    w2 = gen_weights(GEN_CONFIGS[2])
    w2[1] = w2[1] + 3.0
    return {"sum-sigmoid-3-bias": (GEN_CONFIGS[2], w2, [31, 9, 4, 26]), "max-relu-1-nobias": (GEN_CONFIGS[1], gen_weights(GEN_CONFIGS[1]), [31, 24, 2, 13])}


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("which", ["sum-sigmoid-3-bias", "max-relu-1-nobias"])
def test_general_gnn_kernel_with_an_index_at_eight_codewords_per_workgroup(which, compact):
    """`gnn_general_kernel` inside the driver on rsurf5 (8 codewords per workgroup, 70 = 8 * 8 + 6): the oracle's driver takes the shipped
    architecture only, so the restatement with `og.feedback_gnn_general` is the checker."""
    from feedback_gnn_amd.graph import GnnWeights
    cfg, w, hist = _general_cases()[which]
    _, _, B, iters, _ = CASES["rsurf5"]
    c = case_reference("rsurf5")
    og, gg = oracle_library_forms("rsurf5"), gpu_graph("rsurf5")
    ref = sandwich_reference(og, c["sx"], c["sz"], iters, [w] * 3, L0, gnn_cfgs=[gen_cfg_codes(cfg)] * 3)
    assert np.bincount(ref["rounds"], minlength=4).tolist() == hist and min(hist) > 0
    assert np.isfinite(ref["llr"]).all()
    assert gg.info()["codewords_per_block"] == 8
    gw = GnnWeights(w, gg.device, cfg)
    assert gw.general
    g = _decode(gg, c["sx"], c["sz"], iters, [gw] * 3, compact)
    _assert_driver(g, ref, compact, f"rsurf5 {which} compact={compact}")


def _edge_rows():
    """Row selections of the B = 70 rsurf5 run (samples decode independently: a sub-batch equals the rows of the full one)."""
    r = case_reference("rsurf5")["ref"]["rounds"]
    stays = np.nonzero(r == 3)[0]
    conv = np.nonzero(r == 0)[0]
    return {
        "B1-converged": conv[:1],
        "B1-flagged": stays[:1],
        "B8": np.arange(8),  # exactly one workgroup
        "B9": np.arange(9),  # one full workgroup and one with a single codeword
        # one flagged sample (row 9: the second workgroup of the full launch) among converged ones: a compacted list of exactly one entry
        "one-flagged": np.concatenate([conv[:9], stays[:1], conv[9:12]]),
    }


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("which", ["B1-converged", "B1-flagged", "B8", "B9", "one-flagged"])
def test_batch_edges_on_rsurf5(which, compact):
    _, _, _, iters, _ = CASES["rsurf5"]
    c = case_reference("rsurf5")
    ref = c["ref"]
    rows = _edge_rows()[which]
    if which in ("B8", "B9"):
        assert 0 < int((ref["rounds"][rows] > 0).sum()) < len(rows)
        assert len(set(ref["rounds"][rows].tolist())) >= 3
    if which == "one-flagged":
        assert int((ref["rounds"][rows] > 0).sum()) == 1 and ref["rounds"][rows].max() == 3
    gg = gpu_graph("rsurf5")
    g = _decode(gg, c["sx"][rows], c["sz"][rows], iters, _shipped_weights(gg, c, iters), compact)
    assert g["x_hat"].shape == (len(rows), gg.n)
    _assert_driver(g, ref, compact, f"rsurf5 {which} compact={compact}", rows=rows)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name", ["rsurf5", "hp_c7"])
def test_nothing_flagged(name, compact):
    """Five all-zero syndromes: decoder 0 returns the zero estimate, nothing is flagged, and the compacted driver leaves its loop at
    nact == 0 in round 1 — `llr` is then decoder 0's marginals; the full driver runs every round on every sample and merges none."""
    cname, _, _, iters, _ = CASES[name]
    c = case_reference(name)
    og, gg = oracle_library_forms(cname), gpu_graph(cname)
    sx, sz = np.zeros((5, og.m_x), np.uint8), np.zeros((5, og.m_z), np.uint8)
    ref = sandwich_reference(og, sx, sz, iters, [c["weights"]] * 3, L0)
    d0 = og.bp4_decode(sx, sz, iters[0], llr_const=L0)
    assert not ref["rounds"].any() and not ref["x_hat"].any() and not ref["z_hat"].any()
    assert np.array_equal(ref["llr_compact"], d0["llr"]) and not np.array_equal(ref["llr"], d0["llr"])
    g = _decode(gg, sx, sz, iters, _shipped_weights(gg, c, iters), compact)
    assert not g["rounds"].any() and not g["x_hat"].any() and not g["z_hat"].any()
    _assert_driver(g, ref, compact, f"{name} zero syndromes compact={compact}")
    if compact:
        assert np.array_equal(g["llr"], d0["llr"])
