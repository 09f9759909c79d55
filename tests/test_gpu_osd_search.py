"""OSD-E / OSD-CS on the GPU (fgnn_osd, Graph.osd, OSD_Decoder): bit-exact against the NumPy restatement of
tests/test_osd_search_cpu.py on the llr_bin path, order 0 = fgnn_osd0 byte for byte on the marginal path, and the model level.
Shape coverage (every osd_search_kernel instantiation, n up to 2047, the LDS limit, rank-deficient bases, m_x != m_z, order extremes,
edge-value reliabilities) is in tests/test_gpu_osd_shapes.py."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd.decoding import _binary_graph
from helpers import code, gpu_graph, llr_const, to_gpu
from test_osd_search_cpu import osd_search_batch

pytestmark = pytest.mark.gpu

METHOD = {"osd0": 0, "osd_e": 1, "osd_cs": 2}


def _bp2_failures(name, p, B, iters, seed=0x5EED):
    """Binary min-sum BP on hx (BP2_OSD_Model's first step): the graph with the hx basis installed, the syndromes, -soft as the
    binary reliabilities, and the sample ids whose estimate misses the syndrome (ascending)."""
    c = code(name)
    g = _binary_graph(c.hx, c.lx, None)
    g.set_basis(0, c.pivot_hx)
    noise = g.bsc_noise(seed, p, 0, B)
    zeros = torch.zeros_like(noise)
    synd, _ = g.syndrome(zeros, noise)
    pf = np.float32(p)
    soft, hard = g.bp2_decode(synd, iters, "minsum", 0.8, llr_const=float(-np.log((np.float32(1.0) - pf) / pf, dtype=np.float32)), B=B)
    _, _, flags = g.residual(noise, zeros, hard, zeros, want_arrays=False)
    idx = np.nonzero(flags.cpu().numpy() & 1)[0].astype(np.int32)
    return c, g, synd, (-soft).contiguous(), hard, idx


def _check_llr_bin(g, basis_rows, h, synd, llr, idx, method, order):
    B, n = llr.shape
    basis = np.asarray(h)[np.asarray(basis_rows)].astype(np.uint8)
    e_hat = torch.zeros((B, n), dtype=torch.uint8, device=llr.device)
    chosen = torch.full((B,), -7, dtype=torch.int32, device=llr.device)
    g.osd(0, synd, e_hat, method, order, llr_bin=llr, index=to_gpu(idx), nact=len(idx), chosen=chosen)
    sh = synd.cpu().numpy()[:, np.asarray(basis_rows)]
    ref_e, ref_c = osd_search_batch(llr.cpu().numpy(), basis, sh, METHOD[method], order, idx)
    ge, gc = e_hat.cpu().numpy(), chosen.cpu().numpy()
    assert np.array_equal(ge[idx], ref_e[idx]), f"{method} {order}: e_hat differs on samples {idx[(ge[idx] != ref_e[idx]).any(1)][:5]}"
    assert np.array_equal(gc[idx], ref_c[idx]), f"{method} {order}: chosen {gc[idx][:8]} vs {ref_c[idx][:8]}"
    rest = np.setdiff1d(np.arange(B), idx)
    assert (gc[rest] == -7).all() and not ge[rest].any(), "unprocessed samples must be left untouched"
    assert np.array_equal(ge[idx].astype(np.int64) @ basis.T % 2, sh[idx])
    return gc[idx]


@pytest.mark.parametrize("method,order", [("osd_e", 1), ("osd_e", 4), ("osd_e", 8), ("osd_e", 12), ("osd_cs", 1), ("osd_cs", 7),
                                          ("osd_cs", 20), ("osd0", 5)])
def test_llr_bin_bit_exact_on_bp2_failures_882(method, order):
    c, g, synd, llr, _, idx = _bp2_failures("ghp882", 0.06, 4000, 20)
    assert len(idx) >= 8, "test point must produce BP failures"
    idx = idx[:24]
    ch = _check_llr_bin(g, c.pivot_hx, c.hx, synd, llr, idx, method, order)
    if (method, order) in (("osd_e", 12), ("osd_cs", 20)):
        assert (ch != 0).any(), "the search should improve on OSD-0 for some BP failure"


@pytest.mark.parametrize("method,order", [("osd_e", 8), ("osd_cs", 10)])
def test_llr_bin_bit_exact_on_bp2_failures_1270(method, order):
    """[[1270,28]]: the largest LDS footprint (NP = 2048, 32 positions per lane)."""
    c, g, synd, llr, _, idx = _bp2_failures("ghp1270", 0.06, 4000, 20)
    assert len(idx) >= 4, "test point must produce BP failures"
    _check_llr_bin(g, c.pivot_hx, c.hx, synd, llr, idx[:12], method, order)


@pytest.mark.parametrize("name,method,order", [("gb48", "osd_cs", 64), ("steane", "osd_e", 16), ("steane", "osd_cs", 9)])
def test_order_above_k_clamps(name, method, order):
    """Random reliabilities (with ties) on small codes whose k = n - rank is below the order: lambda = k, and the result is still the
    restatement's."""
    c = code(name)
    basis = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    assert basis.shape[1] - basis.shape[0] < order
    g = _binary_graph(c.hx, c.lx, None)
    g.set_basis(0, c.pivot_hx)
    rng = np.random.RandomState(11)
    B, n = 40, basis.shape[1]
    llr = rng.uniform(-2.0, 5.0, size=(B, n)).astype(np.float32)
    llr[:, ::3] = 1.25
    err = (rng.uniform(size=(B, n)) < 0.1).astype(np.uint8)
    synd = (err.astype(np.int64) @ np.asarray(c.hx).T % 2).astype(np.uint8)
    _check_llr_bin(g, c.pivot_hx, c.hx, to_gpu(synd), to_gpu(llr), np.arange(0, B, 2, dtype=np.int32), method, order)


def _rel(marg, side):
    X, Y, Z = (marg[:, i, :].astype(np.float64) for i in range(3))
    if side == 0:
        return np.logaddexp(0.0, -X) - np.logaddexp(-Z, -Y)
    return np.logaddexp(0.0, -Z) - np.logaddexp(-X, -Y)


@pytest.mark.parametrize("name,p", [("ghp882", 0.10), ("ghp1270", 0.10)])
def test_marginal_path_both_sides(name, p):
    c = code(name)
    gg = gpu_graph(name)
    B = 256
    gx, gz = gg.pauli_noise(0x5EED, p, 5, B)
    tx, tz = gg.syndrome(gx, gz)
    g = gg.bp4_decode(tx, tz, 30, "minsum", 0.8, llr_const=llr_const(p), want_logits=False)
    fl = gg.residual(gx, gz, g["x_hat"], g["z_hat"], want_arrays=False)[2]
    gi, nact = gg.compact(fl, 1)
    assert nact >= 3, "test point must produce BP failures"
    gg.set_basis(0, c.pivot_hx)
    gg.set_basis(1, c.pivot_hz)
    ids = np.sort(gi[:nact].cpu().numpy())
    marg = g["llr"].cpu().numpy()
    for side, synd, key, h, rows in ((0, tx, "z_hat", c.hx, c.pivot_hx), (1, tz, "x_hat", c.hz, c.pivot_hz)):
        base = g[key].clone()
        e0 = base.clone()
        gg.osd0(side, synd, e0, marg=g["llr"], index=gi, nact=nact)
        for method in ("osd_e", "osd_cs"):
            e = base.clone()
            gg.osd(side, synd, e, method, 0, marg=g["llr"], index=gi, nact=nact)
            assert torch.equal(e, e0), f"{method} order 0 != fgnn_osd0 (side {side})"
        basis = np.asarray(h)[np.asarray(rows)].astype(np.int64)
        sh = synd.cpu().numpy()[:, np.asarray(rows)]
        E0 = e0.cpu().numpy()
        r = _rel(marg, side)
        for method, order in (("osd_e", 8), ("osd_cs", 7)):
            e = base.clone()
            chosen = torch.zeros(B, dtype=torch.int32, device=e.device)
            gg.osd(side, synd, e, method, order, marg=g["llr"], index=gi, nact=nact, chosen=chosen)
            E, ch = e.cpu().numpy(), chosen.cpu().numpy()
            assert np.array_equal(E[ids].astype(np.int64) @ basis.T % 2, sh[ids]), f"{method} side {side}: H e != s"
            same = ch[ids] == 0
            assert np.array_equal(E[ids][same], E0[ids][same]), "winner 0 must be the OSD-0 solution"
            w = (E[ids] * r[ids]).sum(1)
            w0 = (E0[ids] * r[ids]).sum(1)
            assert (w <= w0 + 1e-3 * (1.0 + np.abs(w0))).all(), f"{method} side {side}: costs more than OSD-0"
            outside = np.setdiff1d(np.arange(B), ids)
            assert np.array_equal(E[outside], base.cpu().numpy()[outside])


def test_bp4_osd_model_osd_cs_no_worse_than_osd0():
    """examples/OSD.ipynb cell 6 shape: [[882,24]], BP4 min-sum x 120, factor 0.8, 50 000 samples, p = 0.09, the same samples."""
    c = code("ghp882")
    out = {}
    for tag, osd in (("osd0", F.OSD0_Decoder(c.N)), ("osd_cs7", F.OSD_Decoder(c.N, "osd_cs", 7))):
        dec = F.QLDPCBPDecoder(code=c, num_iter=120, normalization_factor=0.8, cn_type="minsum", stage_one=True)
        m = F.BP4_OSD_Model(c, dec, osd, seed=0x5EED)
        _, ls = m(50000, 0.09)
        out[tag] = (int(ls.any(1).sum()), m.last_num_osd, m.last_osd_improved)
    print("logical errors / OSD samples / improved:", out)
    assert out["osd0"][1] == out["osd_cs7"][1] > 0
    assert out["osd0"][2] == 0 and out["osd_cs7"][2] > 0
    assert out["osd_cs7"][0] <= out["osd0"][0], out


def test_bp2_osd_model_takes_the_search():
    c = code("ghp882")
    out = {}
    for tag, osd in (("osd0", F.OSD0_Decoder(c.N)), ("osd_e6", F.OSD_Decoder(c.N, "osd_e", 6))):
        bp2 = F.LDPCBPDecoder(c.hx, is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=30, normalization_factor=0.8)
        m = F.BP2_OSD_Model(c.hx, c.hx_basis, c.pivot_hx, c.lx, bp2, osd)
        _, ls = m(20000, 0.06)
        out[tag] = (int(ls.any(1).sum()), m.last_num_osd, m.last_osd_improved)
    assert out["osd0"][1] == out["osd_e6"][1] > 0 and out["osd0"][2] == 0 and out["osd_e6"][2] > 0, out


def test_standalone_call_agrees_with_graph_osd():
    c = code("ghp882")
    basis = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    rank, n = basis.shape
    B = 33
    rng = np.random.RandomState(4)
    llr = rng.uniform(-3.0, 6.0, size=(B, n)).astype(np.float32)
    llr[:, ::7] = 1.5
    err = (rng.uniform(size=(B, n)) < 0.06).astype(np.uint8)
    s = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).T  # [rank, bs]
    for method, order in (("osd_cs", 7), ("osd_e", 5), ("osd0", 0)):
        osd = F.OSD_Decoder(n, method, order)
        pcm = torch.from_numpy(np.tile(basis[None], (B, 1, 1)).astype(np.int32)).cuda()
        e_hat = osd(torch.from_numpy(llr).cuda(), pcm, torch.from_numpy(s).cuda(), B)
        assert e_hat.dtype == torch.bool and tuple(e_hat.shape) == (B, n)
        g = _binary_graph(basis, None, None)
        g.set_basis(0, np.arange(rank, dtype=np.int32))
        ref = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
        g.osd(0, to_gpu(s.T.astype(np.uint8)), ref, method, order, llr_bin=to_gpu(llr))
        assert torch.equal(e_hat, ref.bool()), method
        assert np.array_equal(e_hat.cpu().numpy().astype(np.int64) @ basis.T % 2, s.T)


@pytest.mark.parametrize("make", [lambda n: F.OSD0_Decoder(n), lambda n: F.OSD_Decoder(n, "osd_cs", 3)])
def test_standalone_cache_with_fresh_alternating_tiles(make):
    """Freshly allocated tiles of the hx and hz bases (equal shapes) in turn: a freed tile's storage may come back for the other basis
    with an identical (pointer, shape, strides, version) key — every call must still solve its own basis."""
    c = code("ghp882")
    bx = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    bz = np.asarray(c.hz)[np.asarray(c.pivot_hz)].astype(np.uint8)
    assert bx.shape == bz.shape
    n, B = bx.shape[1], 6
    rng = np.random.RandomState(9)
    llr = torch.from_numpy(rng.uniform(-1.0, 5.0, size=(B, n)).astype(np.float32)).cuda()
    err = (rng.uniform(size=(B, n)) < 0.05).astype(np.int64)
    osd = make(n)
    for it in range(8):
        basis = bx if it % 2 == 0 else bz
        pcm = torch.from_numpy(basis).cuda().to(torch.int32)[None].repeat(B, 1, 1)
        s = err @ basis.T.astype(np.int64) % 2
        e = osd(llr, pcm, torch.from_numpy(s.T.copy()).cuda(), B).cpu().numpy().astype(np.int64)
        assert np.array_equal(e @ basis.T.astype(np.int64) % 2, s), it
        del pcm
