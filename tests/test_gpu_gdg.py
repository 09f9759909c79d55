"""BP-GDG on the GPU (fgnn_gdg_decode) at every gdg_kernel<DV, DC> instantiation, held to the NumPy float32 restatement
tests/gdg_reference.py bit for bit: hard decisions as bytes, stats and path_stats as int32, no tolerance anywhere.  The update uses only
IEEE float32 add, multiply, min, max, abs and compare in a fixed order, the pick is an integer extremum of a total order and the weight of
a decision is an integer, so nothing depends on a reduction order, on which paths share a workgroup or on the launch geometry.  Graph
makers and edge inputs come from the binary BP and Relay-BP tests.  Shapes stay at n <= 150, B <= 70 and 12 iterations per stage."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import gdg_reference as G
import relay_reference as R
from feedback_gnn_amd import _lib, gf2
from guarded import guarded
from helpers import code, to_gpu
from test_bp2_reference_cpu import _llr_const
from test_gpu_bp2_shapes import CASES, LDS_BUDGET, _bare, graphs, lds_hx, named
from test_gpu_relay import FUZZ, informed_edge_channel, instantiation, noise_syndromes, noisy

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
POISON_HARD, POISON_STATS = 0xEE, -7


def gdg_lds_bytes(E_x, n, cpb):
    """fgnn_gdg_decode: messages, posteriors and fix bytes per virtual codeword, each rounded up to 4 floats; per workgroup two 64-bit
    keys, stamp and wacc per codeword, and ndone."""
    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    return (r4(E_x) + r4(n) + r4((n + 3) // 4)) * 4 * cpb + 16 * cpb + r4(2 * cpb + 1) * 4


@functools.lru_cache(maxsize=None)
def _ref_graph(key):
    return R._Graph(_HX[key])


_HX = {}


def ref_graph(hx):
    key = (hx.shape, zlib.crc32(np.ascontiguousarray(hx, np.int64).tobytes()))
    _HX[key] = hx
    return _ref_graph(key)


def both(g, hx, synd, pre, rnd, R_, depth, tail, factor=0.8, decim=25.0, B=None, index=None, nact=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical hard_out, stats and path_stats (and, with an index list, that the
    rows of the other samples are left as they were); returns the restatement's (hard, stats, path_stats)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    Bn = synd.shape[0] if synd is not None else llr["llr_ch"].shape[0] if "llr_ch" in llr else B
    kw, out0, listed = {}, None, index
    if index is not None:
        out0 = (np.full((Bn, hx.shape[1]), POISON_HARD, np.uint8), np.full((Bn, 4), POISON_STATS, np.int32))
        index = np.asarray(index, np.int32)
        listed = index if nact is None else index[:nact]
        kw = dict(index=to_gpu(index) if len(index) else torch.zeros(0, dtype=torch.int32, device=g.device), nact=nact,
                  out=(to_gpu(out0[0]), to_gpu(out0[1])))
    hard, stats, ps = g.gdg_decode(None if synd is None else to_gpu(synd), pre, rnd, R_, depth, tail, decim, factor, B=B,
                                   want_path_stats=True, **gl, **kw)
    h0, s0, p0 = G.gdg_decode(ref_graph(hx), synd, pre, rnd, R_, depth, tail, decim, factor, B=B, index=listed, out=out0, **llr)
    assert stats.dtype == torch.int32 and hard.dtype == torch.uint8 and ps.dtype == torch.int32
    h1, s1, p1 = hard.cpu().numpy(), stats.cpu().numpy(), ps.cpu().numpy()
    print("depth", depth, tail, "found", s0[:, 0].tolist(), "path", s0[:, 2].tolist(), "fixed", s0[:, 3].tolist())
    assert p1.shape == p0.shape and np.array_equal(p0, p1), (np.argwhere(p0 != p1)[:4], p0[(p0 != p1).any((1, 2))][:2], p1[(p0 != p1).any((1, 2))][:2])
    assert np.array_equal(s0, s1), (np.nonzero((s0 != s1).any(1))[0], s0[(s0 != s1).any(1)], s1[(s0 != s1).any(1)])
    assert np.array_equal(h0, h1)
    return h0, s0, p0


def fuzz(g, hx, rng):
    """B in 1..70, pre_iter and round_iter <= 12, depth 0 / 1 / 3, both tail picks, three factors, two decimation LLRs, a constant logit
    and per-bit logits with the edge values of informed_edge_channel."""
    for depth, tail, factor, decim in ((0, "most", 1.0, 25.0), (1, "least", 0.8, 30.0), (3, "most", 0.625, 8.0)):
        B = max(1, int(rng.randint(1, 71)) >> depth)  # B * 2^depth virtual codewords: 70 at the most
        pre, rnd, R_ = int(rng.randint(1, 13)), int(rng.randint(1, 13 if depth < 3 else 6)), int(rng.randint(0, 9 if depth < 3 else 5))
        e, synd = noisy(hx, B, 0.06, int(rng.randint(1 << 30)))
        both(g, hx, synd, pre, rnd, R_, depth, tail, factor, decim, llr_const=-2.197)
        both(g, hx, synd, pre, rnd, R_, depth, tail, factor, decim, llr_ch=informed_edge_channel(hx, e, int(rng.randint(1 << 30))))


assert set(FUZZ.values()) == {(3, 6), (4, 8), (0, 8), (0, 16), (0, 0)}, "the cases must reach every gdg_kernel instantiation"


@pytest.mark.parametrize("key", list(FUZZ))
def test_every_instantiation(key):
    """gdg_kernel goes through bit_dispatch with min-sum, as relay_kernel does: the instantiation rule is the one of test_gpu_relay.py."""
    g, _, hx = graphs(key, dict(CASES)[key])
    assert instantiation(g, hx) == FUZZ[key]
    assert hx.shape[1] <= 150
    fuzz(g, hx, np.random.RandomState(zlib.crc32(key.encode()) ^ 0x6D6))


def test_force_generic_on_a_regular_graph():
    g, _, hx = named("gb48")
    assert instantiation(g, hx) == (4, 8) and instantiation(g, hx, force_generic=True) == (0, 8)
    g.force_generic(True)
    try:
        fuzz(g, hx, np.random.RandomState(17))
    finally:
        g.force_generic(False)


# ---- several virtual codewords per workgroup ---------------------------------------------------------------------------------------------
def test_paths_of_one_workgroup_stop_at_different_steps():
    g, _, hx = named("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    for B in (1, cpb - 1, cpb, cpb + 1):
        synd = noise_syndromes(hx, B, 0.15, 40)  # the same first rows for every B
        _, _, ps = both(g, hx, synd, 5, 3, 6, 0, "least", llr_const=_llr_const(0.15))
        if B >= cpb - 1:
            first = ps[:cpb, 0]  # the first workgroup: one path per sample
            assert (first[:, 2] == 0).any() and (first[:, 2] > 0).any(), "paths that stop before and after the first fix"
            assert len(set(map(tuple, first[:, 2:]))) >= 3, "the workgroup's paths must stop at different steps"
    # the paths of one sample on both sides of a workgroup edge: P = 64 paths over workgroups of cpb < 64 virtual codewords
    assert cpb < 64
    for B in (1, 3):
        both(g, hx, noise_syndromes(hx, B, 0.15, 40), 4, 2, 5, 6, "least", llr_const=_llr_const(0.15))
    # and with several samples in one workgroup: P = 2
    assert cpb % 2 == 0
    both(g, hx, noise_syndromes(hx, cpb // 2 + 1, 0.15, 40), 4, 2, 5, 1, "most", llr_const=_llr_const(0.15))


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (2, 32), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    """(1, 64) and (2, 32): the 8 paths of several samples in one workgroup; (64, 2): a sample's paths over four workgroups."""
    g, _, hx = named("rsurf5")
    synd = noise_syndromes(hx, 11, 0.15, 41)
    want = G.gdg_decode(ref_graph(hx), synd, 4, 3, 5, 3, "least", llr_const=_llr_const(0.15))
    g.set_launch(tpc, cpb)
    try:
        got = both(g, hx, synd, 4, 3, 5, 3, "least", llr_const=_llr_const(0.15))
        both(g, hx, synd[:cpb // 8 + 1], 4, 3, 5, 3, "most", llr_const=_llr_const(0.15))
    finally:
        g.set_launch(0, 0)
    for a, b in zip(want, got):
        assert np.array_equal(a, b), "nothing depends on the launch geometry"


# ---- depth, tail, rounds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", ["least", "most"])
@pytest.mark.parametrize("depth", [0, 1, 3, 6])
def test_depths_and_tail_picks(depth, tail):
    g, _, hx = named("rsurf5")
    e, synd = noisy(hx, 6, 0.15, 21)
    both(g, hx, synd, 4, 2, 6, depth, tail, llr_const=_llr_const(0.15))
    both(g, hx, synd, 4, 2, 6, depth, tail, llr_ch=informed_edge_channel(hx, e, 22))


@functools.lru_cache(maxsize=None)
def _tree_case(name):
    """A batch on which the depth-3 tree does everything it can do, from the restatement: (synd, llr, hard, stats, path_stats, d)."""
    hx = np.asarray(code(name).hx)
    synd = noise_syndromes(hx, 40, {"gb48": 0.08, "rsurf5": 0.2}[name], 33)
    llr = _llr_const(0.1)
    return (synd, llr) + G.gdg_decode(ref_graph(hx), synd, *TREE_ITERS[name], 3, "least", llr_const=llr, want_paths=True)


# pre_iter, round_iter, max_rounds: short enough that some samples stay unsolved on every path
TREE_ITERS = {"gb48": (3, 2, 4), "rsurf5": (2, 1, 3)}


@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_selection_none_some_other_path_and_ties(name):
    """The case set holds, by the restatement: a sample where no path finds a solution, one where between 1 and P - 1 do, one whose
    output is not path 0, and (on the surface code, whose degenerate errors of equal weight give them; gb48 gives none, and
    test_a_tie_in_w_that_only_the_path_index_breaks constructs one) a tie in w between paths with different decisions that the path
    index breaks."""
    g, _, hx = named(name)
    synd, llr, hard, stats, ps, d = _tree_case(name)
    P = 8
    nf = stats[:, 0]
    assert (nf == 0).any(), "no path finds a solution"
    assert ((nf >= 1) & (nf <= P - 1)).any(), "between 1 and P - 1 paths find one"
    assert (stats[:, 2] != 0).any(), "an output from a path other than 0"
    ties = 0
    for b in range(len(nf)):
        best = [p for p in range(P) if ps[b, p, 0] and ps[b, p, 1] == stats[b, 1]]
        if nf[b] and len(best) >= 2 and any(not np.array_equal(d[b, best[0]], d[b, p]) for p in best[1:]):
            assert stats[b, 2] == best[0] and np.array_equal(hard[b], d[b, best[0]])
            ties += 1
    assert ties or name != "rsurf5", "a tie in w between different decisions"
    h0, s0, p0 = both(g, hx, synd, *TREE_ITERS[name], 3, "least", llr_const=llr)
    assert np.array_equal(h0, hard) and np.array_equal(s0, stats)


def test_a_tie_in_w_that_only_the_path_index_breaks():
    """Constructed: on a repetition-like check matrix with two bits of equal prior in every check, both values of the first guess solve
    the syndrome with one flipped bit each, at the same weight: the output is path 0's decision, not path 1's."""
    hx = np.zeros((3, 6), np.int64)
    for c in range(3):
        hx[c, 2 * c] = hx[c, 2 * c + 1] = 1
    g, _, _ = graphs("pairs3", lambda: _bare(hx))
    synd = np.array([[1, 0, 0], [0, 1, 1], [1, 1, 1]], np.uint8)
    h0, s0, p0, d = G.gdg_decode(ref_graph(hx), synd, 1, 2, 3, 1, "least", llr_const=-2.0, want_paths=True)
    tied = (p0[:, 0, 0] == 1) & (p0[:, 1, 0] == 1) & (p0[:, 0, 1] == p0[:, 1, 1]) & (d[:, 0] != d[:, 1]).any(1)
    assert tied.any(), (p0.tolist(), d.tolist())
    assert (s0[tied, 2] == 0).all() and np.array_equal(h0[tied], d[tied, 0])
    both(g, hx, synd, 1, 2, 3, 1, "least", llr_const=-2.0)


def test_max_rounds_zero_and_beyond_n():
    g, _, hx = named("rsurf5")
    n = hx.shape[1]
    synd = noise_syndromes(hx, 9, 0.2, 3)
    for depth in (0, 2):
        _, s0, p0 = both(g, hx, synd, 6, 3, 0, depth, "least", llr_const=_llr_const(0.2))
        assert not p0[:, :, 2].any() and (p0[:, :, 3] <= 6).all() and (p0[p0[:, :, 0] == 0][:, 3] == 6).all()
        assert (p0 == p0[:, :1]).all(), "without a fix every path is the same run"
        assert np.array_equal(s0[:, 0], p0[:, 0, 0] << depth) and not s0[:, 2:].any()
    # R = min(max_rounds, n): a syndrome outside the column space of gb48's hx is never solved, every bit ends up fixed
    g, _, hx = named("gb48")
    n = hx.shape[1]
    left = np.asarray(gf2.kernel(np.asarray(hx, np.int64).T)[0], np.int64) % 2
    u = left[0]
    synd = noise_syndromes(hx, 3, 0.06, 2)
    flip = int(np.nonzero(u)[0][0])
    for b in range(3):
        if (synd[b].astype(np.int64) @ u) % 2 == 0:
            synd[b, flip] ^= 1
    for tail in ("least", "most"):
        _, s0, p0 = both(g, hx, synd, 2, 1, n + 20, 1, tail, llr_const=_llr_const(0.06))
        assert not s0[:, :3].any() and (s0[:, 3] == n).all() and (p0[:, :, 2] == n).all() and (p0[:, :, 3] == 2 + n).all()


# ---- syndromes and index lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, _, hx = named(name)
    B, n = 9, hx.shape[1]
    zero = np.zeros((B, hx.shape[0]), np.uint8)
    h0, s0, p0 = both(g, hx, zero, 6, 5, 3, 2, "least", llr_const=-2.0)
    assert not h0.any() and np.array_equal(s0, np.tile(np.array([4, 0, 0, 0], np.int32), (B, 1)))
    assert np.array_equal(p0, np.tile(np.array([1, 0, 0, 1], np.int32), (B, 4, 1)))
    hn, sn, pn = g.gdg_decode(None, 6, 5, 3, 2, llr_const=-2.0, B=B, want_path_stats=True)
    assert np.array_equal(hn.cpu().numpy(), h0) and np.array_equal(sn.cpu().numpy(), s0) and np.array_equal(pn.cpu().numpy(), p0)
    e = (np.random.RandomState(8).rand(B, n) < 0.1).astype(np.int64)
    both(g, hx, None, 6, 5, 3, 2, "most", llr_ch=informed_edge_channel(hx, e, 8))


@pytest.mark.parametrize("depth", [0, 2])
def test_index_lists(depth):
    g, _, hx = named("rsurf5")
    B = 13
    e, synd = noisy(hx, B, 0.15, 6)
    llr = informed_edge_channel(hx, e, 7)
    full = both(g, hx, synd, 4, 3, 4, depth, "least", llr_ch=llr)
    perm = [11, 2, 7, 0, 12, 5]
    h0, s0, p0 = both(g, hx, synd, 4, 3, 4, depth, "least", llr_ch=llr, index=perm)
    assert np.array_equal(h0[perm], full[0][perm]) and np.array_equal(s0[perm], full[1][perm]) and np.array_equal(p0, full[2][perm])
    rest = sorted(set(range(B)) - set(perm))
    assert (h0[rest] == POISON_HARD).all() and (s0[rest] == POISON_STATS).all()
    both(g, hx, synd, 4, 3, 4, depth, "least", llr_ch=llr, index=perm, nact=4)   # the first nact entries count
    for index, nact in (([], None), (perm, 0)):                                      # an empty list decodes nothing
        h0, s0, p0 = both(g, hx, synd, 4, 3, 4, depth, "least", llr_ch=llr, index=index, nact=nact)
        assert (h0 == POISON_HARD).all() and (s0 == POISON_STATS).all() and p0.shape == (0, 1 << depth, 4)
    hard, stats = g.gdg_decode(to_gpu(synd[:0]), 4, 3, 4, depth)                     # an empty batch
    assert tuple(hard.shape) == (0, hx.shape[1]) and tuple(stats.shape) == (0, 4)


# ---- anchors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ghp882", "irr_16"])
def test_depth_0_no_rounds_is_one_relay_leg_with_gamma_zero_on_the_gpu(name):
    g, _, hx = named(name) if name == "ghp882" else graphs(name, dict(CASES)[name])
    B, T, n = 19, 12, hx.shape[1]
    e, synd = noisy(hx, B, 0.03 if name == "ghp882" else 0.06, 5)
    gamma = torch.zeros((1, n), dtype=torch.float32, device=g.device)
    for llr in (dict(llr_const=_llr_const(0.03)), dict(llr_ch=to_gpu(informed_edge_channel(hx, e, 9)))):
        for factor in (1.0, 0.8):
            h0, s0 = g.relay_decode(to_gpu(synd), gamma, T, T, 1, factor, **llr)
            h1, s1, p1 = g.gdg_decode(to_gpu(synd), T, 5, 0, 0, "most", 25.0, factor, want_path_stats=True, **llr)
            found = s0[:, 0] > 0
            assert torch.equal(h0, h1) and torch.equal(s0[:, 0], s1[:, 0]) and torch.equal(s0[:, 0], p1[:, 0, 0])
            assert torch.equal(s0[found, 1], s1[found, 1]) and not s1[~found, 1].any() and torch.equal(s0[:, 3], p1[:, 0, 3])
    assert len(set(s0[:, 3].tolist())) >= 2


def test_a_shallower_tree_is_the_front_of_a_deeper_one():
    g, _, hx = named("rsurf5")
    synd = to_gpu(noise_syndromes(hx, 9, 0.12, 8))
    llr = _llr_const(0.12)
    _, _, p1 = g.gdg_decode(synd, 4, 3, 6, 1, "least", llr_const=llr, want_path_stats=True)
    _, _, p3 = g.gdg_decode(synd, 4, 3, 6, 3, "least", llr_const=llr, want_path_stats=True)
    assert torch.equal(p3[:, :2], p1)


# ---- the classes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,tail", [(3, "least"), (1, "most"), (0, "most")])
def test_prefilter_gives_the_same_decisions(depth, tail):
    import feedback_gnn_amd as F
    g, _, hx = named("gb48")
    n = hx.shape[1]
    B = 37
    e, synd = noisy(hx, B, 0.07, 14)
    llr = informed_edge_channel(hx, e, 15) if depth else np.full((B, n), _llr_const(0.07), F32)
    plain = F.GDGDecoder(hx, pre_iter=6, round_iter=3, max_rounds=5, depth=depth, tail=tail, prefilter=False, graph=g)
    pre = F.GDGDecoder(hx, pre_iter=6, round_iter=3, max_rounds=5, depth=depth, tail=tail, prefilter=True, graph=g)
    h0, s0 = plain.decode(to_gpu(synd), llr_ch=to_gpu(llr))
    h1, s1 = pre.decode(to_gpu(synd), llr_ch=to_gpu(llr))
    hr, sr, pr = G.gdg_decode(ref_graph(hx), synd, 6, 3, 5, depth, tail, llr_ch=llr)
    assert np.array_equal(h0.cpu().numpy(), hr) and np.array_equal(s0.cpu().numpy(), sr)
    assert torch.equal(h0, h1) and torch.equal(s0[:, 1:], s1[:, 1:]) and pre.last_stats is s1
    presolved = torch.from_numpy(pr[:, 0, 2] == 0).to(g.device) & (s0[:, 0] > 0)   # plain BP solved it: every path did, at no fix
    assert presolved.any() and not presolved.all()
    assert (s0[presolved, 0] == 1 << depth).all() and (s1[presolved, 0] == 1).all() and torch.equal(s0[~presolved, 0], s1[~presolved, 0])
    e_hat = pre((to_gpu(llr), to_gpu(synd.T.copy())))
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (B, n) and torch.equal(e_hat, h0.to(torch.float32))


def test_bp2_gdg_model():
    import feedback_gnn_amd as F
    c = code("gb126")
    hx, logical = np.asarray(c.hx), np.asarray(c.hz_perp)
    dec = F.GDGDecoder(hx, pre_iter=8, round_iter=3, max_rounds=6, depth=2, normalization_factor=0.8)
    model = F.BP2_GDG_Model(hx, logical, dec, seed=SEED)
    B, prob = 48, 0.07
    s_hat, ls_hat = model(B, prob)
    noise, est, stats = model.last_noise.cpu().numpy(), model.last_estimate.cpu().numpy(), model.last_stats.cpu().numpy()
    assert tuple(s_hat.shape) == (B, hx.shape[0]) and tuple(ls_hat.shape) == (B, logical.shape[0])
    synd = (noise.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    h0, s0, _ = G.gdg_decode(ref_graph(hx), synd, 8, 3, 6, 2, "least", 25.0, 0.8, llr_const=_llr_const(prob))
    assert np.array_equal(est, h0) and np.array_equal(stats[:, 1:], s0[:, 1:]) and np.array_equal(stats[:, 0] > 0, s0[:, 0] > 0)
    res = noise ^ est
    solved = stats[:, 0] > 0
    assert solved.any() and not solved.all(), "the batch must hold solved and unsolved samples"
    assert np.array_equal(s_hat.cpu().numpy(), res.astype(np.int64) @ hx.T.astype(np.int64) % 2)
    assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
    assert np.array_equal(ls_hat.cpu().numpy(), res.astype(np.int64) @ logical.T.astype(np.int64) % 2)
    assert model.last_num_unsolved == int((~solved).sum())
    model(B, prob)
    assert not np.array_equal(noise, model.last_noise.cpu().numpy()), "a second call draws the next samples"


# ---- LDS ---------------------------------------------------------------------------------------------------------------------------------
def test_lds_budget_both_sides():
    """The largest lds_hx graph whose per-path state fits, and the next one: the first decodes, the second is refused."""
    def size(E):
        return gdg_lds_bytes(E, lds_hx(E).shape[1], 1)
    E = 8 * (LDS_BUDGET // 42)
    while size(E) > LDS_BUDGET:
        E -= 8
    assert size(E) <= LDS_BUDGET < size(E + 8) and size(E) > LDS_BUDGET - 64
    hx = lds_hx(E)
    g, _, _ = graphs(("lds", E), lambda: _bare(hx))
    assert g.info()["codewords_per_block"] == 1 and int(hx.sum()) == E
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    hard, stats, ps = g.gdg_decode(synd, 2, 2, 3, 1, llr_const=-2.0, want_path_stats=True)
    assert not hard.any() and stats.tolist() == [[2, 0, 0, 0]] * 2 and ps.tolist() == [[[1, 0, 0, 1]] * 2] * 2
    over = lds_hx(E + 8)
    g2, _, _ = graphs(("lds", E + 8), lambda: _bare(over))
    assert g2.info()["codewords_per_block"] == 1
    synd = torch.zeros((2, over.shape[0]), dtype=torch.uint8, device=g2.device)
    with pytest.raises(ValueError, match=f"code too large for the LDS-resident BP-GDG kernel: {size(E + 8)} bytes"):
        g2.gdg_decode(synd, 2, 2, 3, 1, llr_const=-2.0)
    g2.relay_decode(synd, torch.zeros((1, over.shape[1]), dtype=torch.float32, device=g2.device), 2, 2, 1, 0.8, llr_const=-2.0)  # the fix marks count


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_write():
    g, _, hx = named("gb48")
    n, B = hx.shape[1], 3
    synd = torch.zeros((B, hx.shape[0]), dtype=torch.uint8, device=g.device)
    L = _lib.lib()
    with guarded(g) as h:
        hard, stats, ps = h.alloc((B, n), torch.uint8), h.alloc((B, 4), torch.int32), h.alloc((B, 2, 4), torch.int32)
        need = g.gdg_workspace_bytes(1, B)
        assert need == B * 2 * (16 + n)
        ws = h.alloc((need,), torch.uint8)
        index = to_gpu(np.arange(B, dtype=np.int32))

        def call(factor=0.8, pre=3, rnd=2, R_=4, depth=1, tail=1, decim=25.0, B_=B, index_=None, nact=0, hard_=hard, stats_=stats, ws_=ws,
                 ws_bytes=need):
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = L.fgnn_gdg_decode(g.handle, factor, pre, rnd, R_, depth, tail, decim, None, -2.0, p(synd), B_, p(index_), nact, p(hard_),
                                   p(stats_), p(ps), p(ws_), ws_bytes, None)
            return rc, L.fgnn_last_error().decode()

        for kw, message in ((dict(pre=0), "pre_iter and round_iter must be >= 1"), (dict(rnd=0), "pre_iter and round_iter must be >= 1"),
                            (dict(R_=-1), "max_rounds must be >= 0"), (dict(depth=-1), "depth must be in 0 .. 6"),
                            (dict(depth=7), "depth must be in 0 .. 6"), (dict(tail=2), "tail_pick must be"), (dict(tail=-1), "tail_pick must be"),
                            (dict(decim=0.0), "decim_llr must be > 0"), (dict(decim=-1.0), "decim_llr must be > 0"),
                            (dict(decim=float("nan")), "decim_llr must be > 0"), (dict(B_=-1), "B must be >= 0"),
                            (dict(index_=index, nact=-1), "nact must be in 0 .. B"), (dict(index_=index, nact=B + 1), "nact must be in 0 .. B"),
                            (dict(hard_=None), "no output buffer"), (dict(stats_=None), "no output buffer"),
                            (dict(ws_=None), f"needs {need} bytes"), (dict(ws_bytes=need - 1), f"needs {need} bytes"),
                            (dict(depth=2), f"needs {B * 4 * (16 + n)} bytes")):
            rc, msg = call(**kw)
            assert rc == -1 and message in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        for t, name in ((hard, "hard_out"), (stats, "stats"), (ps, "path_stats"), (ws, "workspace")):
            h.assert_untouched(t, name)
        assert call(B_=0, hard_=None, stats_=None, ws_=None, ws_bytes=0)[0] == 0       # an empty batch needs no buffers
        assert call(index_=index, nact=0, hard_=None, stats_=None, ws_=None, ws_bytes=0)[0] == 0
        torch.cuda.synchronize()
        for t, name in ((hard, "hard_out"), (stats, "stats"), (ps, "path_stats"), (ws, "workspace")):
            h.assert_untouched(t, name)
        assert call()[0] == 0                                                           # and the same call, unchanged, decodes
        torch.cuda.synchronize()
        for t, name in ((hard, "hard_out"), (stats, "stats"), (ps, "path_stats"), (ws, "workspace")):
            h.assert_written(t, name)
    size = C.c_size_t()
    assert L.fgnn_gdg_workspace_bytes(g.handle, 7, 1, C.byref(size)) == -1 and L.fgnn_gdg_workspace_bytes(g.handle, 1, -1, C.byref(size)) == -1
    assert L.fgnn_gdg_workspace_bytes(None, 1, 1, C.byref(size)) == -1 and L.fgnn_gdg_workspace_bytes(g.handle, 1, 1, None) == -1
    for kw in (dict(tail="middle"), dict(depth=7), dict(decim_llr=0.0)):
        with pytest.raises(ValueError):
            g.gdg_decode(synd, 3, 2, 4, **dict(dict(depth=1), **kw))
