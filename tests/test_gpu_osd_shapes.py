"""OSD-0 and OSD-E / OSD-CS on the GPU across the shapes the kernels are specialised for: every osd_search_kernel<NPL> instantiation,
the bit-packing edges of W = ceil((n+1)/32), n up to the documented maximum 2047, both sides of the LDS refusal, rank-deficient bases,
m_x != m_z on the marginal path, order extremes and reliability edge values.  osd0 is held to the CPU oracle (og_osd0) bit for bit,
osd to the NumPy restatement of tests/test_osd_search_cpu.py."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd import codes_q as cq
from feedback_gnn_amd.decoding import _binary_graph
from feedback_gnn_amd.gf2 import rank as gf2_rank, row_echelon
from helpers import binary_oracle, code, random_sparse_basis, to_gpu
from test_osd_search_cpu import osd_search_batch

pytestmark = pytest.mark.gpu

METHOD = {"osd0": 0, "osd_e": 1, "osd_cs": 2}
SENTINEL = 0xA5  # e_hat byte of a sample the call must not touch
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h


def _np(n):
    """NP of osd_prepare: the least power of two >= n."""
    NP = 1
    while NP < n:
        NP <<= 1
    return NP


def npl(n):
    """The osd_search_kernel<NPL> instantiation fgnn_osd dispatches for n."""
    return max(_np(n), 64) // 64


def osd_lds_bytes(n, rows, search):
    """The LDS bytes osd_prepare asks for (fgnn_osd.hip: osd_lds_bytes, plus OSD_SEARCH_SCRATCH = 40 bytes 8-aligned for fgnn_osd)."""
    W = (n + 1 + 31) // 32
    WS = W | 1
    lds = 8 * _np(n) + 4 * rows * WS + 4 * (2 * n + rows)
    return ((lds + 7) & ~7) + 40 if search else lds


def max_rows(n, search):
    r = 0
    while osd_lds_bytes(n, r + 1, search) <= LDS_BUDGET:
        r += 1
    return r


SHAPES = [7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 511, 512, 513, 1023, 1025, 2046, 2047]
assert {npl(n) for n in SHAPES} == {1, 2, 4, 8, 16, 32}, "the sweep must reach every osd_search_kernel instantiation"


def _rows_for(n):
    return 400 if n >= 2046 else max(3, n // 2)  # n = 2047 fits at most max_rows(2047, True) rows


def _graph(basis):
    g = _binary_graph(basis, None, None)
    g.set_basis(0, np.arange(basis.shape[0], dtype=np.int32))
    return g


def _llr(rng, B, n):
    llr = rng.normal(1.0, 2.5, size=(B, n)).astype(np.float32)
    llr[:, ::5] = np.float32(0.75)  # ties in the sort
    return llr


def _check(g, og, basis, llr, synd, idx, configs, consistent=True, side=0, pivot_rows=None, search=True):
    """osd0 (against og_osd0) and every (method, order) of `configs` (against the restatement), each with e_hat / chosen sentinels, on
    the samples `idx` (None: all B).  Order 0 of every method must give osd0's bytes (unless not `search`: a basis only fgnn_osd0 fits).
    H e = s is asserted where `consistent`."""
    B, n = llr.shape
    m = basis.shape[0]
    rows = np.arange(m, dtype=np.int32) if pivot_rows is None else np.asarray(pivot_rows, np.int32)
    ids = np.arange(B) if idx is None else np.asarray(idx)
    rest = np.setdiff1d(np.arange(B), ids)
    gidx = None if idx is None else to_gpu(np.asarray(idx, np.int32))
    nact = 0 if idx is None else len(idx)
    llr_g, synd_g = to_gpu(llr), to_gpu(synd)

    def run(method, order):
        e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
        chosen = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        if method is None:
            g.osd0(side, synd_g, e, llr_bin=llr_g, index=gidx, nact=nact)
        else:
            g.osd(side, synd_g, e, method, order, llr_bin=llr_g, index=gidx, nact=nact, chosen=chosen)
        torch.cuda.synchronize()
        e, chosen = e.cpu().numpy(), chosen.cpu().numpy()
        assert (e[rest] == SENTINEL).all() and (chosen[rest] == -7).all(), "unprocessed samples must be left untouched"
        assert (e[ids] <= 1).all()
        return e, chosen

    e0, _ = run(None, 0)
    ref = og.osd0(side, rows, synd, llr_bin=llr, index=None if idx is None else np.asarray(idx, np.int32))
    bad = ids[(e0[ids] != ref[ids]).any(1)]
    assert not len(bad), f"osd0 differs from og_osd0 on samples {bad[:6]}"
    sh = synd[:, rows]
    if consistent:
        assert np.array_equal(e0[ids].astype(np.int64) @ basis.T % 2, sh[ids]), "osd0: H e != s"
    for method in METHOD if search else ():
        e, chosen = run(method, 0)
        assert np.array_equal(e[ids], e0[ids]) and (chosen[ids] == 0).all(), f"{method} order 0 != osd0"
    elims = {}
    for method, order in configs:
        e, chosen = run(method, order)
        re, rc = osd_search_batch(llr, basis, sh, METHOD[method], order, ids, elims=elims)
        bad = ids[(e[ids] != re[ids]).any(1)]
        assert not len(bad), f"{method} {order}: e_hat differs on samples {bad[:6]}"
        assert np.array_equal(chosen[ids], rc[ids]), f"{method} {order}: chosen {chosen[ids][:8]} vs {rc[ids][:8]}"
        if consistent:
            assert np.array_equal(e[ids].astype(np.int64) @ basis.T % 2, sh[ids]), f"{method} {order}: H e != s"
    return e0


@pytest.mark.parametrize("n", SHAPES)
def test_shape_sweep_bit_exact(n):
    basis, rk = random_sparse_basis(n, _rows_for(n), seed=n)
    k = n - rk
    g, og = _graph(basis), binary_oracle(basis)
    big = n >= 1023
    B = 5 if big else 12
    rng = np.random.RandomState(n + 1)
    llr = _llr(rng, B, n)
    err = (rng.uniform(size=(B, n)) < 0.05).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    idx = np.array([3, 1], np.int32) if big else np.array([9, 2, 6, 11, 4], np.int32)  # unsorted, gaps, nact < B
    configs = [("osd_e", 1), ("osd_e", min(k, 8)), ("osd_cs", 1), ("osd_cs", 7)]
    _check(g, og, basis, llr, synd, idx, configs)
    _check(g, og, basis, llr, synd, None, [("osd_cs", 7)] if big else configs)


def _full_hx_cases():
    gb, ghp = code("gb48"), code("ghp882")
    h, _ = random_sparse_basis(150, 70, seed=77)
    dep = np.concatenate([h, h[5:6], (h[0] ^ h[1] ^ h[2])[None]]).astype(np.uint8)
    dep = dep[np.random.RandomState(5).permutation(len(dep))]
    return [("gb48", np.asarray(gb.hx).astype(np.uint8)), ("ghp882", np.asarray(ghp.hx).astype(np.uint8)), ("random150", dep)]


@pytest.mark.parametrize("name", ["gb48", "ghp882", "random150"])
def test_rank_deficient_basis(name):
    """The full hx (dependent rows) installed as the basis: zero rows are ignored.  osd0 = og_osd0, H e = s for error syndromes, order 0
    of every method = osd0, higher orders = the restatement; random (inconsistent) syndromes give the oracle's / restatement's answer."""
    basis = dict(_full_hx_cases())[name]
    m, n = basis.shape
    rk = gf2_rank(basis)
    assert rk < m
    g, og = _graph(basis), binary_oracle(basis)
    rng = np.random.RandomState(m + n)
    B = 24 if n < 500 else 8
    llr = rng.uniform(-2.0, 6.0, size=(B, n)).astype(np.float32)
    llr[:, ::4] = np.float32(1.25)
    err = (rng.uniform(size=(B, n)) < 0.08).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    configs = [("osd_e", 8), ("osd_cs", 7)]
    _check(g, og, basis, llr, synd, None, configs)
    idx = np.arange(B - 1, -1, -2, dtype=np.int32)
    _check(g, og, basis, llr, synd, idx, configs)
    rs = (rng.uniform(size=(B, m)) < 0.5).astype(np.uint8)
    _check(g, og, basis, llr, rs, None, configs, consistent=False)


@pytest.mark.parametrize("make", [lambda n: F.OSD0_Decoder(n), lambda n: F.OSD_Decoder(n, "osd_cs", 7),
                                  lambda n: F.OSD_Decoder(n, "osd_e", 6)])
def test_standalone_call_with_full_hx(make):
    for name, basis in _full_hx_cases()[:2]:
        m, n = basis.shape
        B = 16
        rng = np.random.RandomState(n)
        llr = rng.uniform(-2.0, 6.0, size=(B, n)).astype(np.float32)
        err = (rng.uniform(size=(B, n)) < 0.06).astype(np.int64)
        s = err @ basis.T.astype(np.int64) % 2
        e = make(n)(torch.from_numpy(llr).cuda(), torch.from_numpy(basis.astype(np.int32)).cuda(), torch.from_numpy(s.T.copy()).cuda(), B)
        assert np.array_equal(e.cpu().numpy().astype(np.int64) @ basis.T % 2, s), name


def test_osd_e_order_16():
    n = 200
    basis, rk = random_sparse_basis(n, 100, seed=16)
    assert n - rk >= 16 and _np(n) <= 256
    g, og = _graph(basis), binary_oracle(basis)
    rng = np.random.RandomState(16)
    llr = _llr(rng, 3, n)
    err = (rng.uniform(size=(3, n)) < 0.06).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    _check(g, og, basis, llr, synd, None, [("osd_e", 16)])


def test_osd_cs_order_64():
    n = 300
    basis, rk = random_sparse_basis(n, 150, seed=64)
    assert n - rk >= 64
    g, og = _graph(basis), binary_oracle(basis)
    rng = np.random.RandomState(64)
    llr = _llr(rng, 6, n)
    err = (rng.uniform(size=(6, n)) < 0.06).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    _check(g, og, basis, llr, synd, np.array([5, 0, 3], np.int32), [("osd_cs", 64), ("osd_cs", 63)])


def test_square_invertible_basis_k0():
    """k = 0: no free columns, a single candidate — every method at order 5 is OSD-0 with chosen = 0."""
    n = 48
    rng = np.random.RandomState(48)
    while True:
        basis = (rng.uniform(size=(n, n)) < 0.3).astype(np.uint8)
        if gf2_rank(basis) == n and basis.any(0).all():
            break
    g, og = _graph(basis), binary_oracle(basis)
    llr = _llr(rng, 10, n)
    synd = (rng.uniform(size=(10, n)) < 0.5).astype(np.uint8)  # every syndrome is consistent
    e0 = _check(g, og, basis, llr, synd, None, [("osd_e", 5), ("osd_cs", 5)])
    for method in ("osd_e", "osd_cs"):
        e = torch.zeros((10, n), dtype=torch.uint8, device="cuda")
        chosen = torch.full((10,), -7, dtype=torch.int32, device="cuda")
        g.osd(0, to_gpu(synd), e, method, 5, llr_bin=to_gpu(llr), chosen=chosen)
        assert np.array_equal(e.cpu().numpy(), e0) and not chosen.cpu().numpy().any()


FLT_MAX = np.finfo(np.float32).max


def _edge_llr(kind, rng, B, n):
    if kind == "all_equal":
        return np.full((B, n), 1.5, np.float32)
    if kind == "many_ties":
        return rng.choice(np.float32([-1.0, 0.5, 2.0]), size=(B, n)).astype(np.float32)
    if kind == "signed_zeros":
        x = rng.choice(np.float32([0.0, -0.0]), size=(B, n)).astype(np.float32)
        x[B // 2:, ::7] = rng.normal(size=(B - B // 2, len(range(0, n, 7)))).astype(np.float32)
        return x
    if kind == "flt_max":  # +FLT_MAX and -FLT_MAX in separate samples: a cost may overflow to +-inf, never to inf - inf
        x = np.abs(rng.normal(1.0, 2.0, size=(B, n))).astype(np.float32)
        x[rng.uniform(size=(B, n)) < 0.3] = FLT_MAX
        x[1::2] = -x[1::2]
        return x
    if kind == "subnormal":
        return (rng.uniform(-1.0, 1.0, size=(B, n)) * 1e-39).astype(np.float32)
    if kind == "huge":
        return (rng.choice([-1.0, 1.0], size=(B, n)) * rng.uniform(0.5, 2.0, size=(B, n)) * 1e30).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["all_equal", "many_ties", "signed_zeros", "flt_max", "subnormal", "huge"])
def test_reliability_edge_values(kind):
    n = 129
    basis, _ = random_sparse_basis(n, 60, seed=129)
    g, og = _graph(basis), binary_oracle(basis)
    rng = np.random.RandomState(len(kind))
    B = 8
    llr = _edge_llr(kind, rng, B, n)
    if kind == "subnormal":
        assert ((np.abs(llr) < np.finfo(np.float32).tiny) & (llr != 0)).mean() > 0.9
    err = (rng.uniform(size=(B, n)) < 0.06).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    _check(g, og, basis, llr, synd, None, [("osd_e", 6), ("osd_cs", 7)])


def test_marginal_path_both_sides_with_unequal_check_counts():
    """A hypergraph product of two rectangular matrices: m_x != m_z, so side 1 reads its checks at the offset m_x of the combined check
    list.  Random finite marginals [B,3,n]: osd0 = og_osd0 on both sides, and order 0 of every method = osd0."""
    rng = np.random.RandomState(2)
    h1 = (rng.uniform(size=(6, 10)) < 0.35).astype(int)
    h2 = (rng.uniform(size=(7, 9)) < 0.35).astype(int)
    h1[0, h1.sum(0) == 0] = 1
    h2[0, h2.sum(0) == 0] = 1
    h1[h1.sum(1) == 0, 0] = 1
    h2[h2.sum(1) == 0, 0] = 1
    c = cq.hypergraph_product(h1, h2)
    hx, hz = np.asarray(c.hx).astype(np.uint8), np.asarray(c.hz).astype(np.uint8)
    assert hx.shape[0] != hz.shape[0]
    from feedback_gnn_amd.graph import TannerGraph
    from oracle.oracle import OracleGraph
    gg = TannerGraph(c)
    og = OracleGraph(c, forms="library-default")
    n = hx.shape[1]
    B = 32
    marg = rng.normal(0.0, 3.0, size=(B, 3, n)).astype(np.float32)
    marg[:, :, ::6] = np.float32(0.25)
    idx = np.array([30, 3, 17, 8, 21], np.int32)
    for side, h in ((0, hx), (1, hz)):
        rows = np.asarray(row_echelon(h.T)[3], np.int32)  # independent rows of h
        assert len(rows) == gf2_rank(h)
        gg.set_basis(side, rows)
        err = (rng.uniform(size=(B, n)) < 0.1).astype(np.uint8)
        synd = (err.astype(np.int64) @ h.T.astype(np.int64) % 2).astype(np.uint8)
        for index in (None, idx):
            ids = np.arange(B) if index is None else index
            gi = None if index is None else to_gpu(index)
            e0 = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
            gg.osd0(side, to_gpu(synd), e0, marg=to_gpu(marg), index=gi, nact=len(ids))
            E0 = e0.cpu().numpy()
            ref = og.osd0(side, rows, synd, marg=marg, index=index)
            assert np.array_equal(E0[ids], ref[ids]), f"side {side}: osd0 != og_osd0"
            assert (E0[np.setdiff1d(np.arange(B), ids)] == SENTINEL).all()
            assert np.array_equal(E0[ids].astype(np.int64) @ h[rows].T % 2, synd[ids][:, rows])
            for method in METHOD:
                e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
                gg.osd(side, to_gpu(synd), e, method, 0, marg=to_gpu(marg), index=gi, nact=len(ids))
                assert np.array_equal(e.cpu().numpy(), E0), f"side {side}: {method} order 0 != osd0"


@pytest.mark.parametrize("n", [600, 2047])
def test_lds_boundary(n):
    """The largest row count osd_prepare accepts, restated from osd_lds_bytes: at it both calls run and are exact; one row more is
    refused with FGNN_ERR_ARG (ValueError) before anything launches.  Rows may repeat (a rank-deficient basis), so the boundary is
    reachable at any n."""
    r0, r1 = max_rows(n, False), max_rows(n, True)
    assert r1 <= r0 and osd_lds_bytes(n, r0, False) <= LDS_BUDGET < osd_lds_bytes(n, r0 + 1, False)
    m = min(r0 + 1, 500)
    basis, _ = random_sparse_basis(n, m, seed=n + 3)
    g = _binary_graph(basis, None, None)
    og = binary_oracle(basis)
    rng = np.random.RandomState(n)
    B = 2
    llr = _llr(rng, B, n)
    err = (rng.uniform(size=(B, n)) < 0.04).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)

    def rows_of(count):
        return np.arange(count, dtype=np.int32) % m

    for count, search_ok in [(r1, True)] + ([(r0, False)] if r0 > r1 else []):
        rows = rows_of(count)
        g.set_basis(0, rows)
        sub = basis[rows]
        _check(g, og, sub, llr, synd, None, [("osd_cs", 3)] if search_ok else [], pivot_rows=rows, search=search_ok)
        if not search_ok:
            e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
            with pytest.raises(ValueError, match="too large for the LDS"):
                g.osd(0, to_gpu(synd), e, "osd_cs", 3, llr_bin=to_gpu(llr))
            assert (e.cpu().numpy() == SENTINEL).all()
    g.set_basis(0, rows_of(r0 + 1))
    for call in (lambda e: g.osd0(0, to_gpu(synd), e, llr_bin=to_gpu(llr)),
                 lambda e: g.osd(0, to_gpu(synd), e, "osd_e", 2, llr_bin=to_gpu(llr))):
        e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="too large for the LDS"):
            call(e)
        torch.cuda.synchronize()
        assert (e.cpu().numpy() == SENTINEL).all()


def test_n_2048_is_refused():
    basis, _ = random_sparse_basis(2048, 8, seed=2048, col_weight=1)
    g = _graph(basis)
    synd = to_gpu(np.zeros((2, 8), np.uint8))
    llr = to_gpu(np.ones((2, 2048), np.float32))
    e = torch.full((2, 2048), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="n <= 2047"):
        g.osd0(0, synd, e, llr_bin=llr)
    with pytest.raises(ValueError, match="n <= 2047"):
        g.osd(0, synd, e, "osd_cs", 2, llr_bin=llr)
    assert (e.cpu().numpy() == SENTINEL).all()
