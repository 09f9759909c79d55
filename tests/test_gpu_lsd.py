"""`fgnn_lsd` on the GPU against the NumPy restatement of tests/lsd_reference.py: e_hat and all four stats columns bit for bit at the
smallest shapes where the kernel can go wrong (m below one word, word edges, dependent rows and columns, a dead cluster, more than one
word per lane), the two reliability inputs, an unordered index list, both caps, the refusal of a pivot cap that does not fit, guard
bands around both outputs, and the decoder / model built on it."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd.decoding import _binary_graph
from guarded import guarded
from helpers import code, gpu_graph, random_sparse_basis, to_gpu
from lsd_reference import Matrix, lsd_batch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5  # e_hat byte of a sample the call must not touch


def side_matrix(name, side):
    c = code(name)
    return np.asarray(c.hx if side == 0 else c.hz).astype(np.uint8)


def informed(rng, err, sigma=1.5):
    """Reliabilities that know something about the error (clusters stay small), with ties and a -0.0."""
    r = (rng.normal(3.0, sigma, size=err.shape) - 4.0 * err).astype(np.float32)
    r[:, ::7] = np.float32(0.75)
    r[:, 1] = np.float32(-0.0)
    r[:, 2] = np.float32(0.0)
    return r


def blind(rng, shape):
    """Reliabilities that know nothing (the clusters percolate), with ties."""
    r = rng.normal(1.0, 2.5, size=shape).astype(np.float32)
    r[:, ::5] = np.float32(0.75)
    return r


def errors(rng, B, n, p):
    return (rng.random((B, n)) < p).astype(np.uint8)


def run_gpu(g, side, synd, llr_bin=None, marg=None, idx=None, max_pivots=0, max_rounds=0):
    B, n = synd.shape[0], g.n
    e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
    stats = torch.full((B, 4), -7, dtype=torch.int32, device="cuda")
    out = g.lsd(side, to_gpu(synd), e, marg=None if marg is None else to_gpu(marg), llr_bin=None if llr_bin is None else to_gpu(llr_bin),
                index=None if idx is None else to_gpu(np.asarray(idx, np.int32)), nact=0 if idx is None else len(idx),
                max_pivots=max_pivots, max_rounds=max_rounds, stats=stats)
    assert out[0] is e and out[1] is stats
    torch.cuda.synchronize()
    return e.cpu().numpy(), stats.cpu().numpy()


def check(g, H, side, synd, r, idx=None, max_pivots=0, max_rounds=0, marg=None):
    """The kernel's e_hat and stats of the listed samples equal the restatement's; the other rows keep their sentinels.  `r` is what
    the restatement ranks by; the kernel gets it as llr_bin unless `marg` is given."""
    B = synd.shape[0]
    ids = np.arange(B) if idx is None else np.asarray(idx)
    rest = np.setdiff1d(np.arange(B), ids)
    e, stats = run_gpu(g, side, synd, llr_bin=None if marg is not None else r, marg=marg, idx=idx, max_pivots=max_pivots,
                       max_rounds=max_rounds)
    assert (e[rest] == SENTINEL).all() and (stats[rest] == -7).all(), "unprocessed samples must be left untouched"
    cap = max_pivots or g.lsd_max_pivots(side)
    re, rs = lsd_batch(Matrix(H) if not isinstance(H, Matrix) else H, synd, r, cap, max_rounds, ids)
    bad = ids[(stats[ids] != rs[ids]).any(1)]
    assert not len(bad), f"stats differ on samples {bad[:6]}: {stats[bad[:3]]} != {rs[bad[:3]]}"
    bad = ids[(e[ids] != re[ids]).any(1)]
    assert not len(bad), f"e_hat differs on samples {bad[:6]}"
    return e, stats


@pytest.mark.parametrize("name", ["steane", "toric4", "gb126"])
@pytest.mark.parametrize("side", [0, 1])
def test_small_codes_bit_for_bit(name, side):
    H = side_matrix(name, side)
    m, n = H.shape
    g = gpu_graph(name)
    assert g.lsd_max_pivots(side) == min(m, n)
    rng = np.random.default_rng(11 + side)
    B = 24
    err = errors(rng, B, n, np.linspace(0.0, 0.3, B)[:, None])
    synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    synd[1] = 0
    synd[1, m // 2] = 1  # a single defect: outside the image where the rows are dependent (toric4: a dead cluster)
    synd[2] = 1          # every check a defect
    r = informed(rng, err)
    r[3] = np.float32(1.0)  # uniform: every selection is a tie
    e, stats = check(g, H, side, synd, r)
    ok = np.array_equal(e[0].astype(np.int64) @ H.T % 2, synd[0]) and (stats[3:, 0] == 1).all()
    assert ok and np.array_equal(e[3:].astype(np.int64) @ H.T % 2, synd[3:]), "syndromes of errors are solved"
    assert (stats[0] == [1, 0, 0, 0]).all() and not e[0].any()
    if name == "toric4":
        assert stats[1, 0] == 0 and stats[1, 2] == n, "the single defect's component grows until it is whole and dies"
    check(g, H, side, synd, blind(rng, (B, n)))


@pytest.mark.parametrize("m", [31, 32, 33, 64, 65])
def test_word_edges_and_dependent_columns(m):
    H, _ = random_sparse_basis(2 * m, m, seed=m)
    g = _binary_graph(H, None, None)
    rng = np.random.default_rng(m)
    B = 16
    err = errors(rng, B, 2 * m, np.linspace(0.02, 0.5, B)[:, None])
    synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    synd[0] = 1
    _, stats = check(g, H, 0, synd, blind(rng, (B, 2 * m)))
    assert (stats[:, 2] > stats[:, 3]).any(), "dependent columns must occur"
    check(g, H, 0, synd, informed(rng, err), max_pivots=m // 4)
    check(g, H, 0, synd, informed(rng, err), max_rounds=1)


@pytest.fixture(scope="module")
def ghp():
    """ghp882, both sides: 16 samples at p = 0.03 under blind reliabilities (percolating clusters) and 16 at p = 0.01 under informed
    ones, with the restatement's matrices built once."""
    out = {}
    for side in (0, 1):
        H = side_matrix("ghp882", side)
        rng = np.random.default_rng(882 + side)
        err = np.r_[errors(rng, 16, H.shape[1], 0.03), errors(rng, 16, H.shape[1], 0.01)]
        synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
        r = np.r_[blind(rng, (16, H.shape[1])), informed(rng, err[16:])]
        out[side] = (H, Matrix(H), err, synd, r)
    return out


@pytest.mark.parametrize("side", [0, 1])
def test_ghp882_bit_for_bit(ghp, side):
    H, M, err, synd, r = ghp[side]
    g = gpu_graph("ghp882")
    assert g.lsd_max_pivots(side) == H.shape[0]
    e, stats = check(g, M, side, synd, r)
    assert (stats[:, 0] == 1).all() and np.array_equal(e.astype(np.int64) @ H.T % 2, synd)
    assert stats[:16, 3].min() > 64 and (stats[16:, 1] == 1).any(), "percolating clusters and one-round solutions both occur"


def test_ghp882_index_list_out_of_order(ghp):
    H, M, err, synd, r = ghp[0]
    check(gpu_graph("ghp882"), M, 0, synd, r, idx=[30, 17, 2, 25, 16, 0, 9])


def test_ghp882_marginal_input(ghp):
    """Reliabilities from BP4 marginals.  The triples (X, 7, Z) come from a grid on which llr_z = softplus(-X) - lse2(-Z, -Y) (and llr_x
    with X and Z swapped) takes values at least 1e-3 apart unless the triples are equal, so the order of the keys, which is all LSD
    reads of them, is that of the float64 value, and equal triples tie exactly."""
    H0, M0, err, synd0, _ = ghp[0]
    n = H0.shape[1]
    rng = np.random.default_rng(5)
    X = rng.integers(0, 8, size=(8, n)) * 0.75 - 2.0
    Z = rng.integers(0, 8, size=(8, n)) * 0.59 - 1.9
    marg = np.stack([X, np.full_like(X, 7.0), Z], 1).astype(np.float32)
    X, Z = marg[:, 0].astype(np.float64), marg[:, 2].astype(np.float64)

    def llr(a, y, b):  # log P(no component) / P(component) of the component whose marginal is b
        return np.logaddexp(0, -a) - np.logaddexp(-b, -y)

    g = gpu_graph("ghp882")
    for side, (a, b) in enumerate(((X, Z), (Z, X))):
        r64 = llr(a, 7.0, b)
        vals = np.unique(r64.round(9))
        assert np.diff(vals).min() > 1e-3, "the grid must separate the reliabilities"
        H, M, _, synd, _ = ghp[side]
        check(g, M, side, synd[16:24], r64.astype(np.float32), marg=marg)


def test_ghp882_caps(ghp):
    H, M, err, synd, r = ghp[0]
    g = gpu_graph("ghp882")
    rng = np.random.default_rng(50)
    err5 = errors(rng, 16, H.shape[1], 0.05)
    synd5 = (err5.astype(np.int64) @ H.T % 2).astype(np.uint8)
    _, stats = check(g, M, 0, synd5, informed(rng, err5, sigma=1.0), max_pivots=64)
    assert 0 < stats[:, 0].sum() < 16, "both outcomes must occur under the pivot cap"
    assert (stats[stats[:, 0] == 0, 3] == 64).all()
    _, stats = check(g, M, 0, synd, r, max_rounds=2)
    assert (stats[:, 1] <= 2).all() and 0 < stats[:, 0].sum() < 32, "both outcomes must occur under the round cap"


def test_more_than_one_word_per_lane():
    H = side_matrix("hp_big", 0)
    m, n = H.shape
    assert m > 64 * 32
    g = gpu_graph("hp_big")
    cap = g.lsd_max_pivots(0)
    assert 64 <= cap < m, "the LDS bounds the pivots of this code"
    rng = np.random.default_rng(6480)
    err = errors(rng, 4, n, 0.004)
    err[0, -1] = 1
    synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    synd[3, m - 1] ^= 1  # a defect in the last word
    e, stats = check(g, H, 0, synd, informed(rng, err, sigma=1.0))
    assert (stats[:3, 0] == 1).all() and np.array_equal(e[:3].astype(np.int64) @ H.T % 2, synd[:3])
    assert stats[3, 0] == 0 and stats[3, 3] == cap, "the lone extra defect grows its cluster until the LDS's pivot cap ends the sample"


def test_a_pivot_cap_beyond_the_lds_is_refused_and_nothing_is_written():
    g = gpu_graph("hp_big")
    cap = g.lsd_max_pivots(0)
    m, n = side_matrix("hp_big", 0).shape
    e = torch.full((2, n), SENTINEL, dtype=torch.uint8, device="cuda")
    stats = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    s = torch.ones((2, m), dtype=torch.uint8, device="cuda")
    llr = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match=f"largest count that fits is {cap}"):
        g.lsd(0, s, e, llr_bin=llr, max_pivots=cap + 1, stats=stats)
    marg = torch.zeros((2, 3, n), dtype=torch.float32, device="cuda")
    for kw in (dict(llr_bin=llr, max_pivots=-1), dict(llr_bin=llr, max_rounds=-1), dict(), dict(llr_bin=llr, marg=marg)):
        with pytest.raises(ValueError):
            g.lsd(0, s, e, stats=stats, **kw)
    torch.cuda.synchronize()
    assert bool((e == SENTINEL).all()) and bool((stats == -7).all())


def test_no_write_beside_the_outputs_and_unlisted_rows_stay_untouched(ghp):
    H, M, err, synd, r = ghp[0]
    g = gpu_graph("ghp882")
    B, n = synd.shape[0], H.shape[1]
    idx = [31, 4, 20, 0]
    rest = np.setdiff1d(np.arange(B), idx)
    with guarded(g) as h:
        e = h.alloc((B, n), torch.uint8, name="e_hat")
        stats = h.alloc((B, 4), torch.int32, name="stats")
        g.lsd(0, to_gpu(synd), e, llr_bin=to_gpu(r), index=to_gpu(np.asarray(idx, np.int32)), nact=len(idx), stats=stats)
        h.check()
        h.assert_written(e[idx], "e_hat of the listed samples")
        h.assert_written(stats[idx], "stats of the listed samples")
        h.assert_untouched(e[rest], "e_hat of the other samples")
        h.assert_untouched(stats[rest], "stats of the other samples")
        _, own = g.lsd(0, to_gpu(synd), e, llr_bin=to_gpu(r))  # stats allocated by the wrapper, every sample
        h.check()
        h.assert_written(own, "stats")
        h.assert_written(e, "e_hat")
    re, rs = lsd_batch(M, synd, r, g.lsd_max_pivots(0), 0)
    assert np.array_equal(e.cpu().numpy(), re) and np.array_equal(own.cpu().numpy(), rs)


@pytest.mark.parametrize("fallback", ["osd0", None])
def test_lsd_decoder_standalone(ghp, fallback):
    H, M, err, synd, r = ghp[0]
    d = F.LSD_Decoder(H.shape[1], max_pivots=64, fallback=fallback)
    e = d(to_gpu(r), to_gpu(H), to_gpu(synd.T.copy())).cpu().numpy()
    stats = d.last_stats.cpu().numpy()
    re, rs = lsd_batch(M, synd, r, 64, 0)
    assert np.array_equal(stats, rs) and 0 < stats[:, 0].sum() < len(stats), "the pivot cap must bite on some samples"
    found = stats[:, 0] == 1
    assert np.array_equal(e[found], re[found].astype(bool))
    solved = (e.astype(np.int64) @ H.T % 2 == synd).all(1)
    assert solved[found].all()
    if fallback:
        assert solved.all(), "OSD-0 re-solves what LSD gave up"
    else:
        assert np.array_equal(e, re.astype(bool))


@pytest.mark.parametrize("fallback", ["osd0", None])
def test_bp4_lsd_model(fallback):
    c = code("ghp882")
    hx, hz = np.asarray(c.hx).astype(np.int64), np.asarray(c.hz).astype(np.int64)
    bp4 = F.QLDPCBPDecoder(code=c, num_iter=32, normalization_factor=0.8, cn_type="minsum", stage_one=True)
    m = F.BP4_LSD_Model(c, bp4, F.LSD_Decoder(c.N, max_pivots=0 if fallback else 200, fallback=fallback), seed=11)
    B = 256
    o = m.decode(B, 0.09)
    ex, ez, xh, zh = (o[k].cpu().numpy().astype(np.int64) for k in ("noise_x", "noise_z", "x_hat", "z_hat"))
    ok = ((hx @ (ez ^ zh).T % 2 == 0).all(0)) & ((hz @ (ex ^ xh).T % 2 == 0).all(0))
    stats = m.last_stats.cpu().numpy()
    assert 0 < m.last_num_lsd < B and m.last_num_fallback <= m.last_num_lsd
    assert ((stats[:, :, 3] > 0).any(0)).sum() == m.last_num_lsd, "LSD ran on the BP failures and on nothing else"
    found = (stats[:, :, 0] == 1).all(0)
    if fallback:
        assert ok.all(), "every final estimate reproduces both syndromes"
        assert m.last_num_fallback == (~found).sum()
    else:
        assert m.last_num_fallback == 0 and ok[found].all() and not ok[~found].any()
    zero, ls_hat = m(B, 0.09)
    assert tuple(ls_hat.shape) == (B, c.lz.shape[0] + c.lx.shape[0]) and not bool(zero.any())


def test_bp2_lsd_model():
    """Binary min-sum BP + LSD on hx of [[882,24]] over a BSC: LSD runs on the BP failures, nothing is left for the fallback without
    caps, and the logical-error count is small (BP2 + OSD-0 makes 117 in 200 000 at this p, examples/OSD.ipynb cell 3: about 12 in
    20 000; LSD-0 and OSD-0 need not pick the same solution, so the band is 4 sigma of a Poisson count of 12 on either side of it)."""
    c = code("ghp882")
    bp2 = F.LDPCBPDecoder(c.hx, is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    m = F.BP2_LSD_Model(c.hx, c.lx, bp2, F.LSD_Decoder(c.N))
    zeros, ls_hat = m(20000, 0.05)
    assert tuple(ls_hat.shape) == (20000, 24) and not bool(zeros.any())
    stats = m.last_stats[0].cpu().numpy()
    assert 0 < m.last_num_lsd < 20000 and m.last_num_fallback == 0 and (stats[:, 0] == 1).all()
    assert (stats[:, 3] > 0).sum() == m.last_num_lsd
    errs = int(ls_hat.any(1).sum())
    assert errs < 12 + 4 * np.sqrt(12), errs
