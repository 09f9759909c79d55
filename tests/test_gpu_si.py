"""BP-SI on the GPU (fgnn_si_decode) at every si_kernel<DV, DC> instantiation, held to the NumPy float32 restatement
tests/si_reference.py bit for bit: hard decisions as bytes, all four stats columns as int32, no tolerance anywhere.  The update uses only
IEEE float32 add, multiply, min, max, abs and compare in a fixed order, the pick is an integer minimum of a total order and the solve is
GF(2) arithmetic, so nothing depends on a reduction order, on which codewords share a workgroup or on the launch geometry.

Every comparison runs inside the guarded, poisoned allocator of tests/guarded.py: hard_out and stats lie between two 64 KiB guards and
start out as 0xFF bytes; the guards must be intact, the rows of the decoded samples written in full (of stats the first three columns:
the fourth legitimately holds -1, which is the poison), and with an index list the rows of the other samples still poison.

Shapes stay at 24 to 32 samples and a dozen iterations per attempt; the samples of a batch span p from 0 to far past threshold, and half
of some batches carry flipped syndrome bits, which is what makes a solve fail: the syndrome is then outside the column space."""
import ctypes as C
import functools
import re
import zlib

import numpy as np
import pytest
import torch

import relay_reference as R
import si_reference as S
from guarded import guarded
from helpers import code, random_sparse_basis, to_gpu
from test_bp2_reference_cpu import _llr_const
from test_gpu_bp2_shapes import CASES, LDS_BUDGET, _bare, graphs, lds_hx, named
from test_gpu_relay import informed_edge_channel, instantiation

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED


def si_lds_bytes(E_x, n, m_x, m_z, cpb):
    """fgnn_si_decode: messages, posteriors, scores, inactive bytes and adjacent bytes per codeword, each rounded up to 4 floats; per
    workgroup four 64-bit words per codeword, stamp and wacc per codeword, and ndone."""
    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    return (r4(E_x) + r4(n) + r4(m_z) + r4((n + 3) // 4) + r4((m_x + 3) // 4)) * 4 * cpb + 32 * cpb + r4(2 * cpb + 1) * 4


@functools.lru_cache(maxsize=None)
def _ref_graph(key):
    return R._Graph(_HX[key])


_HX = {}


def ref_graph(hx):
    key = (hx.shape, zlib.crc32(np.ascontiguousarray(hx, np.int64).tobytes()))
    _HX[key] = hx
    return _ref_graph(key)


def span_noise(hx, B, pmax, seed, flip=0.0):
    """Sample b has BSC(p_b) noise, p_b rising from 0 to pmax over the batch; with `flip`, the second half of the batch also gets that
    share of its syndrome bits flipped.  Returns (e, synd)."""
    rng = np.random.RandomState(seed)
    e = (rng.rand(B, hx.shape[1]) < np.linspace(0.0, pmax, B)[:, None]).astype(np.int64)
    synd = (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)
    if flip:
        f = rng.rand(*synd.shape) < flip
        f[:B // 2] = False
        synd ^= f.astype(np.uint8)
    return e, synd


def both(g, hx, hz, synd, num_iter, si_iter, max_groups, factor=0.8, B=None, index=None, nact=None, **llr):
    """Kernel and restatement on the same inputs, the kernel between guards; asserts identical hard_out and stats (and, with an index
    list, that the rows of the other samples are left as they were); returns the restatement's (hard, stats, trace)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    Bn = synd.shape[0] if synd is not None else llr["llr_ch"].shape[0] if "llr_ch" in llr else B
    n = hx.shape[1]
    with guarded(g) as h:
        kw, listed = {}, None
        if index is not None:
            index = np.asarray(index, np.int32)
            listed = index if nact is None else index[:nact]
            kw = dict(index=to_gpu(index) if len(index) else torch.zeros(0, dtype=torch.int32, device=g.device), nact=nact,
                      out=(h.alloc((Bn, n), torch.uint8, "hard"), h.alloc((Bn, 4), torch.int32, "stats")))
        hard, stats = g.si_decode(None if synd is None else to_gpu(synd), num_iter, si_iter, max_groups, factor, B=B, **gl, **kw)
        h.check()
        assert [r.shape for r in h.records[:2]] == [(Bn, n), (Bn, 4)] and stats.dtype == torch.int32 and hard.dtype == torch.uint8
        rows = np.arange(Bn) if listed is None else np.asarray(listed, np.int64)
        rest = np.setdiff1d(np.arange(Bn), rows)
        h.assert_written(hard[rows], "hard_out of the decoded samples")
        h.assert_written(stats[rows][:, :3], "stats of the decoded samples")
        if index is not None:
            h.assert_untouched(hard[rest], "hard_out of the other samples")
            h.assert_untouched(stats[rest], "stats of the other samples")
        h1, s1 = hard.cpu().numpy(), stats.cpu().numpy()
    h0, s0, trace = S.si_decode(ref_graph(hx), hz, synd, num_iter, si_iter, max_groups, factor, B=B, index=listed, want_trace=True, **llr)
    print("found", s0[rows, 0].tolist(), "attempt", s0[rows, 1].tolist(), "k", s0[rows, 2].tolist(), "group", s0[rows, 3].tolist())
    bad = np.nonzero((s0[rows] != s1[rows]).any(1))[0]
    assert len(bad) == 0, (bad, s0[rows][bad], s1[rows][bad])
    assert np.array_equal(h0[rows], h1[rows]), np.nonzero((h0[rows] != h1[rows]).any(1))[0]
    return h0, s0, trace


def kinds(trace):
    return {t[2] for sample in trace for t in sample}


def occurrences(stats, trace):
    """What a batch held: rescues, failed solves, exhausted group lists."""
    out = set()
    if ((stats[:, 0] == 1) & (stats[:, 1] > 0)).any():
        out.add("rescue")
    if "unsolvable" in kinds(trace):
        out.add("failed solve")
    if ((stats[:, 0] == 0) & (stats[:, 1] > 0)).any():
        out.add("exhausted")
    return out


# ---- the named codes -------------------------------------------------------------------------------------------------------------------
# name: (instantiation, B, pmax, share of flipped syndrome bits, (num_iter, si_iter, max_groups))
NAMED = {
    "steane": ((0, 8), 24, 0.5, 0.0, (1, 2, 2)),     # plain BP is cut short: the Hamming code leaves it nothing to rescue otherwise
    "toric4": ((0, 8), 32, 0.4, 0.15, (4, 3, 6)),    # dependent rows: flipped syndromes make solves fail
    "ibm72": ((3, 6), 28, 0.25, 0.1, (6, 4, 5)),
    "ghp882": ((3, 6), 24, 0.12, 0.0, (12, 8, 4)),
    "gb126": ((0, 16), 26, 0.12, 0.0, (8, 6, 5)),    # check degree 10: the predicated instantiation
    "hp_c7": ((3, 6), 30, 0.25, 0.0, (6, 4, 5)),     # a hypergraph product; of circulants of weight 3, so (3,6)-regular all the same:
                                                     # the irregular graphs are those of test_groups_unrelated_to_h_with_an_empty_row
}


@pytest.mark.parametrize("name", list(NAMED))
def test_named_codes(name):
    inst, B, pmax, flip, iters = NAMED[name]
    g, _, hx = named(name)
    hz = np.asarray(code(name).hz)
    assert instantiation(g, hx) == inst
    e, synd = span_noise(hx, B, pmax, 1, flip)
    _, s0, t0 = both(g, hx, hz, synd, *iters, llr_const=_llr_const(0.05))
    _, s1, t1 = both(g, hx, hz, synd, *iters, llr_ch=informed_edge_channel(hx, e, 3))
    seen = occurrences(s0, t0) | occurrences(s1, t1)
    assert "rescue" in seen, "every code must have samples that inactivation rescues"
    assert (s0[:, 0] == 1).any() and ((s0[:, 1] == 0) & (s0[:, 0] == 1)).any(), "and samples that plain BP solves"
    if name == "toric4":
        assert seen == {"rescue", "failed solve", "exhausted"}, seen
    if name in ("ibm72", "ghp882", "hp_c7", "gb126"):
        assert "exhausted" in seen


def test_force_generic_on_a_regular_graph():
    g, _, hx = named("ibm72")
    hz = np.asarray(code("ibm72").hz)
    assert instantiation(g, hx) == (3, 6) and instantiation(g, hx, force_generic=True) == (0, 8)
    e, synd = span_noise(hx, 28, 0.25, 2, 0.1)
    g.force_generic(True)
    try:
        both(g, hx, hz, synd, 6, 4, 5, llr_const=_llr_const(0.05))
        both(g, hx, hz, synd, 5, 3, 7, 0.625, llr_ch=informed_edge_channel(hx, e, 4))
    finally:
        g.force_generic(False)


# ---- groups unrelated to H, on the loop and the predicated instantiations ---------------------------------------------------------------
def unrelated(key, rows=20, seed=4):
    """(graph, hx, groups): a case of the binary shape tests with a seeded random sparse group matrix, one row of it emptied."""
    hx = np.asarray(dict(CASES)[key]().hx)
    grp = random_sparse_basis(hx.shape[1], rows, seed)[0].astype(np.int64)
    grp[7] = 0
    g, _, _ = graphs(("si", key, rows, seed), lambda: _bare(hx, grp))
    return g, hx, grp


@pytest.mark.parametrize("key,inst", [("gb_rand_9", (0, 0)), ("irr_30", (0, 0)), ("irr_8", (0, 8)), ("gb_rand_4a", (0, 8)), ("irr_16", (0, 16))])
def test_groups_unrelated_to_h_with_an_empty_row(key, inst):
    """The group matrix need not commute with H, and a group without a bit is never picked; gb_rand_4a is (4,8)-regular, but the group
    side is not, so it has no packed rows and runs the predicated kernel."""
    g, hx, grp = unrelated(key)
    assert instantiation(g, hx) == inst and not grp[7].any() and grp.sum(1).max() <= 32
    e, synd = span_noise(hx, 28, 0.2, 5)
    seen = set()
    for iters, llr in (((6, 4, 30), dict(llr_const=_llr_const(0.05))), ((6, 4, 8), dict(llr_ch=informed_edge_channel(hx, e, 3))),
                       ((3, 1, 19), dict(llr_const=_llr_const(0.1)))):
        _, s0, t0 = both(g, hx, grp, synd, *iters, **llr)
        seen |= occurrences(s0, t0)
        assert (s0[:, 3] != 7).all(), "the empty group is never inactivated"
        assert (s0[s0[:, 0] == 0][:, 1] == min(iters[2], 19)).all(), "attempts made = min(max_groups, non-empty groups)"
    assert seen == {"rescue", "failed solve", "exhausted"}, seen


def test_the_regular_4_8_rows():
    g, _, hx = named("gb48")
    hz = np.asarray(code("gb48").hz)
    assert instantiation(g, hx) == (4, 8)
    e, synd = span_noise(hx, 30, 0.25, 6, 0.1)
    both(g, hx, hz, synd, 6, 4, 6, llr_const=_llr_const(0.05))
    both(g, hx, hz, synd, 6, 4, 6, 1.0, llr_ch=informed_edge_channel(hx, e, 8))


# ---- iteration and group counts ----------------------------------------------------------------------------------------------------------
def test_si_iter_one_and_max_groups_below_and_above_the_group_count():
    g, _, hx = named("toric4")
    hz = np.asarray(code("toric4").hz)
    m_z = hz.shape[0]
    e, synd = span_noise(hx, 32, 0.4, 7, 0.15)
    llr = informed_edge_channel(hx, e, 9)
    for si_iter, max_groups in ((1, 3), (1, m_z), (2, m_z + 5), (3, 1), (2, 1 << 30)):
        _, s0, _ = both(g, hx, hz, synd, 3, si_iter, max_groups, llr_const=_llr_const(0.1))
        both(g, hx, hz, synd, 3, si_iter, max_groups, llr_ch=llr)
        assert (s0[s0[:, 0] == 0][:, 1] == min(max_groups, m_z)).all() and (s0[:, 0] == 0).any()
        assert (s0[s0[:, 1] > 0][:, 2] <= si_iter).all()


@pytest.mark.parametrize("name", ["toric4", "gb48"])
def test_zero_and_null_syndrome(name):
    g, _, hx = named(name)
    hz = np.asarray(code(name).hz)
    B, n = 9, hx.shape[1]
    zero = np.zeros((B, hx.shape[0]), np.uint8)
    h0, s0, _ = both(g, hx, hz, zero, 6, 5, 3, llr_const=-2.0)
    assert not h0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 1, -1], np.int32), (B, 1)))
    hn, sn = g.si_decode(None, 6, 5, 3, llr_const=-2.0, B=B)
    assert np.array_equal(hn.cpu().numpy(), h0) and np.array_equal(sn.cpu().numpy(), s0)
    e = (np.random.RandomState(8).rand(B, n) < 0.15).astype(np.int64)
    both(g, hx, hz, None, 6, 5, 3, llr_ch=informed_edge_channel(hx, e, 8))   # priors that say "error" against the zero syndrome


# ---- several codewords per workgroup -------------------------------------------------------------------------------------------------------
def test_codewords_of_one_workgroup_finish_at_different_attempts():
    g, _, hx = named("toric4")
    hz = np.asarray(code("toric4").hz)
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    e, synd = span_noise(hx, 3 * cpb + 1, 0.4, 11, 0.1)
    order = np.random.RandomState(3).permutation(len(synd))   # easy and hard samples side by side
    e, synd = e[order], synd[order]
    for B in (1, cpb - 1, cpb, cpb + 1, 3 * cpb + 1):
        _, s0, _ = both(g, hx, hz, synd[:B], 4, 3, 6, llr_const=_llr_const(0.1))
        if B >= cpb:
            first = s0[:cpb]
            assert len(set(first[:, 1].tolist())) >= 3 and len(set(map(tuple, first[:, :3].tolist()))) >= 4, first.tolist()


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (2, 32), (16, 4), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, _, hx = named("toric4")
    hz = np.asarray(code("toric4").hz)
    e, synd = span_noise(hx, 32, 0.4, 12, 0.1)
    order = np.random.RandomState(6).permutation(len(synd))   # easy and hard samples side by side
    e, synd = e[order], synd[order]
    llr = informed_edge_channel(hx, e, 13)
    want = S.si_decode(ref_graph(hx), hz, synd, 4, 3, 6, llr_ch=llr)
    g.set_launch(tpc, cpb)
    try:
        got = both(g, hx, hz, synd, 4, 3, 6, llr_ch=llr)
        _, s0, _ = both(g, hx, hz, synd[:cpb // 2 + 1], 4, 3, 6, llr_const=_llr_const(0.1))
    finally:
        g.set_launch(0, 0)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), "nothing depends on the launch geometry"
    assert len(set(got[1][:min(cpb, 32), 1].tolist())) >= min(cpb, 3), "the first workgroup's codewords finish at different attempts"


# ---- index lists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toric4", "ibm72"])
def test_index_lists(name):
    g, _, hx = named(name)
    hz = np.asarray(code(name).hz)
    B = 13
    e, synd = span_noise(hx, B, 0.3, 6, 0.1)
    llr = informed_edge_channel(hx, e, 7)
    full = both(g, hx, hz, synd, 4, 3, 4, llr_ch=llr)
    perm = [11, 2, 7, 0, 12, 5]
    h0, s0, _ = both(g, hx, hz, synd, 4, 3, 4, llr_ch=llr, index=perm)        # both() asserts the poison on the other rows
    assert np.array_equal(h0[perm], full[0][perm]) and np.array_equal(s0[perm], full[1][perm])
    both(g, hx, hz, synd, 4, 3, 4, llr_ch=llr, index=perm, nact=4)            # the first nact entries count
    for index, nact in (([], None), (perm, 0)):                                # an empty list decodes nothing
        both(g, hx, hz, synd, 4, 3, 4, llr_ch=llr, index=index, nact=nact)
    hard, stats = g.si_decode(to_gpu(synd[:0]), 4, 3, 4)                       # an empty batch
    assert tuple(hard.shape) == (0, hx.shape[1]) and tuple(stats.shape) == (0, 4)


# ---- anchor --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ghp882", "gb126", "hp_c7"])
def test_no_groups_is_one_relay_leg_with_gamma_zero_on_the_gpu(name):
    g, _, hx = named(name)
    B, T, n = 19, 12, hx.shape[1]
    e, synd = span_noise(hx, B, 0.08, 5)
    gamma = torch.zeros((1, n), dtype=torch.float32, device=g.device)
    for llr in (dict(llr_const=_llr_const(0.03)), dict(llr_ch=to_gpu(informed_edge_channel(hx, e, 9)))):
        for factor in (1.0, 0.8):
            h0, s0 = g.relay_decode(to_gpu(synd), gamma, T, T, 1, factor, **llr)
            h1, s1 = g.si_decode(to_gpu(synd), T, 5, 0, factor, **llr)
            found = s0[:, 0] > 0
            assert torch.equal(h0, h1) and torch.equal(s0[:, 0], s1[:, 0]) and torch.equal(s0[found, 3], s1[found, 2])
            assert not s1[:, 1].any() and (s1[:, 3] == -1).all() and not s1[~found, 2].any()
    assert found.any() and not found.all() and len(set(s0[found, 3].tolist())) >= 2


# ---- the classes -----------------------------------------------------------------------------------------------------------------------------
def test_si_decoder_and_bp2_si_model():
    import feedback_gnn_amd as F
    c = code("hp_c7")
    hx, hz, logical = np.asarray(c.hx), np.asarray(c.hz), np.asarray(c.lx)
    dec = F.SIDecoder(hx, hz, num_iter=8, si_iter=4, max_groups=6, normalization_factor=0.8)
    model = F.BP2_SI_Model(hx, hz, logical, dec, seed=SEED)
    B, prob = 48, 0.09
    s_hat, ls_hat = model(B, prob)
    noise, est, stats = model.last_noise.cpu().numpy(), model.last_estimate.cpu().numpy(), model.last_stats.cpu().numpy()
    assert tuple(s_hat.shape) == (B, hx.shape[0]) and tuple(ls_hat.shape) == (B, logical.shape[0])
    synd = (noise.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    h0, s0 = S.si_decode(ref_graph(hx), hz, synd, 8, 4, 6, 0.8, llr_const=_llr_const(prob))
    assert np.array_equal(est, h0) and np.array_equal(stats, s0)
    res = noise ^ est
    solved = stats[:, 0] > 0
    assert solved.any() and not solved.all() and (stats[:, 1] > 0)[solved].any(), "solved, rescued and unsolved samples"
    assert np.array_equal(s_hat.cpu().numpy(), res.astype(np.int64) @ hx.T.astype(np.int64) % 2)
    assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
    assert np.array_equal(ls_hat.cpu().numpy(), res.astype(np.int64) @ logical.T.astype(np.int64) % 2)
    assert model.last_num_unsolved == int((~solved).sum())
    model(B, prob)
    assert not np.array_equal(noise, model.last_noise.cpu().numpy()), "a second call draws the next samples"
    llr = np.full((B, hx.shape[1]), _llr_const(prob), F32)
    e_hat = dec((to_gpu(llr), to_gpu(synd.T.copy())))
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (B, hx.shape[1]) and np.array_equal(e_hat.cpu().numpy(), h0.astype(F32))


def test_bp4_si_model():
    import feedback_gnn_amd as F
    c = code("hp_c7")
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    bp4 = F.QLDPCBPDecoder(code=c, num_iter=6, normalization_factor=0.8, cn_type="minsum", stage_one=True)
    dz = F.SIDecoder(hx, hz, num_iter=8, si_iter=4, max_groups=6)
    dx = F.SIDecoder(hz, hx, num_iter=8, si_iter=4, max_groups=6)
    model = F.BP4_SI_Model(c, bp4, dz, dx, seed=SEED)
    B, prob = 40, 0.12
    s_hat, ls_hat = model(B, prob)
    g = model.graph
    assert tuple(s_hat.shape) == (B, g.m_z + g.m_x) and tuple(ls_hat.shape) == (B, g.rows_lz + g.rows_lx)
    stats = model.last_stats.cpu().numpy()
    assert stats.shape == (2, B, 4) and 0 < model.last_num_si < B
    listed = (stats[:, :, 1] > 0).any(0) | (stats[:, :, 0] == 0).any(0)
    assert listed.sum() <= model.last_num_si and ((stats[:, :, 0] == 1) & (stats[:, :, 1] > 0)).any(), "some half was rescued"
    unsolved = (stats[:, :, 0] == 0).any(0)
    assert model.last_num_unsolved == int(unsolved.sum())
    assert np.array_equal(s_hat.cpu().numpy().any(1), unsolved), "the residual syndrome is non-zero exactly on the unsolved samples"


# ---- LDS -------------------------------------------------------------------------------------------------------------------------------------
def test_lds_budget_both_sides():
    """The largest lds_hx graph whose per-codeword state fits, and the next one: the first decodes, the second is refused with the bytes
    it would need."""
    def size(E):
        return si_lds_bytes(E, E // 4, E // 8, 1, 1)   # lds_hx(E) for E a multiple of 8: E / 4 bits, E / 8 checks
    E = 8 * (LDS_BUDGET // 42)
    while size(E) > LDS_BUDGET:
        E -= 8
    assert size(E) <= LDS_BUDGET < size(E + 8) and size(E) > LDS_BUDGET - 64
    hx = lds_hx(E)
    assert hx.shape == (E // 8, E // 4) and lds_hx(E + 8).shape == ((E + 8) // 8, (E + 8) // 4)
    g, _, _ = graphs(("lds", E), lambda: _bare(hx))
    assert g.info()["codewords_per_block"] == 1 and int(hx.sum()) == E
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    hard, stats = g.si_decode(synd, 2, 2, 3, llr_const=-2.0)
    assert not hard.any() and stats.tolist() == [[1, 0, 1, -1]] * 2
    over = lds_hx(E + 8)
    g2, _, _ = graphs(("lds", E + 8), lambda: _bare(over))
    assert g2.info()["codewords_per_block"] == 1
    synd = torch.zeros((2, over.shape[0]), dtype=torch.uint8, device=g2.device)
    with pytest.raises(ValueError, match=f"code too large for the LDS-resident BP-SI kernel: {size(E + 8)} bytes of LDS per workgroup, the limit "
                                         f"is {LDS_BUDGET}"):
        g2.si_decode(synd, 2, 2, 3, llr_const=-2.0)
    g2.relay_decode(synd, torch.zeros((1, over.shape[1]), dtype=torch.float32, device=g2.device), 2, 2, 1, 0.8, llr_const=-2.0)  # the marks count


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_write():
    from feedback_gnn_amd import _lib
    g, _, hx = named("gb48")
    n, B = hx.shape[1], 3
    synd = torch.zeros((B, hx.shape[0]), dtype=torch.uint8, device=g.device)
    L = _lib.lib()
    with guarded(g) as h:
        hard, stats = h.alloc((B, n), torch.uint8), h.alloc((B, 4), torch.int32)
        index = to_gpu(np.arange(B, dtype=np.int32))

        def call(graph=g.handle, factor=0.8, num_iter=3, si_iter=2, max_groups=4, B_=B, index_=None, nact=0, hard_=hard, stats_=stats):
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = L.fgnn_si_decode(graph, factor, num_iter, si_iter, max_groups, None, -2.0, p(synd), B_, p(index_), nact, p(hard_), p(stats_), None)
            return rc, L.fgnn_last_error().decode()

        for kw, message in ((dict(graph=None), "graph is NULL"), (dict(num_iter=0), "num_iter and si_iter must be >= 1"),
                            (dict(si_iter=0), "num_iter and si_iter must be >= 1"), (dict(max_groups=-1), "max_groups must be >= 0"),
                            (dict(B_=-1), "B must be >= 0"), (dict(index_=index, nact=-1), "nact must be in 0 .. B"),
                            (dict(index_=index, nact=B + 1), "nact must be in 0 .. B"), (dict(hard_=None), "no output buffer"),
                            (dict(stats_=None), "no output buffer")):
            rc, msg = call(**kw)
            assert rc == -1 and message in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        for t, name in ((hard, "hard_out"), (stats, "stats")):
            h.assert_untouched(t, name)
        assert call(B_=0, hard_=None, stats_=None)[0] == 0       # an empty batch needs no buffers
        assert call(index_=index, nact=0, hard_=None, stats_=None)[0] == 0
        torch.cuda.synchronize()
        for t, name in ((hard, "hard_out"), (stats, "stats")):
            h.assert_untouched(t, name)
        assert call()[0] == 0                                    # and the same call, unchanged, decodes
        torch.cuda.synchronize()
        h.assert_written(hard, "hard_out")
        h.assert_written(stats[:, :3], "stats")
    assert L.fgnn_version() == 2


def test_groups_beyond_the_solve_tables_are_refused_by_name():
    """A group of 33 bits, and a group of 32 bits whose 96 checks exceed the 64 the residual word holds; each is the second row of its
    group matrix, and the message says so.  The refusal holds for max_groups = 0 too and writes nothing."""
    n = 99
    hx = np.zeros((n, n), np.int64)   # bit v in checks v, v + 33, v + 66 (mod 99): three distinct checks per bit
    for k in (0, 33, 66):
        hx[(np.arange(n) + k) % n, np.arange(n)] = 1
    wide = np.zeros((3, n), np.int64)
    wide[0, :4] = wide[2, 50:52] = 1
    wide[1, 10:43] = 1               # 33 bits
    many = np.zeros((3, n), np.int64)
    many[0, :4] = many[2, 50:52] = 1
    many[1, :32] = 1                 # 32 bits in 32 + 32 + 32 distinct checks
    assert len(set(np.nonzero(hx[:, :32].any(1))[0])) == 96
    for key, grp, message in (("wide", wide, "group 1 (row 1 of side 1) has 33 bits: stabilizer inactivation takes groups of up to 32"),
                              ("many", many, "group 1 (row 1 of side 1) has 96 adjacent checks: the solve tables of stabilizer inactivation hold 64")):
        g, _, _ = graphs(("si-refused", key), lambda: _bare(hx, grp))
        synd = torch.zeros((2, n), dtype=torch.uint8, device=g.device)
        with guarded(g) as h:
            for max_groups in (2, 0, 2):   # the second and third call meet the remembered refusal
                with pytest.raises(ValueError, match=re.escape(message)):
                    g.si_decode(synd, 2, 2, max_groups, llr_const=-2.0)
            torch.cuda.synchronize()
            for rec in h.records:
                h.assert_untouched(h.payload(rec), "an output of a refused call")
        g.relay_decode(synd, torch.zeros((1, n), dtype=torch.float32, device=g.device), 2, 2, 1, 0.8, llr_const=-2.0)  # the graph itself is fine
    ok = many.copy()
    ok[1, 22:32] = 0                 # 22 bits in 66 checks: two checks too many
    g, _, _ = graphs(("si-refused", "ok66"), lambda: _bare(hx, ok))
    with pytest.raises(ValueError, match="has 66 adjacent checks"):
        g.si_decode(torch.zeros((2, n), dtype=torch.uint8, device=g.device), 2, 2, 1, llr_const=-2.0)
    ok[1, 21] = 0
    ok[1, 33] = 1                    # bit 33 shares its three checks with bit 0: 22 bits, 63 checks
    g, _, _ = graphs(("si-refused", "ok63"), lambda: _bare(hx, ok))
    e, synd = span_noise(hx, 24, 0.1, 3)
    both(g, hx, ok, synd, 4, 3, 3, llr_const=_llr_const(0.05))
