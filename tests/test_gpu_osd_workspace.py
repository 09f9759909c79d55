"""OSD beyond LDS (fgnn_osd_ws): one persistent workgroup per workspace slot, the augmented matrix word-major in global memory.  Held bit
for bit to the LDS-resident kernels everywhere they run, to og_osd0 and the NumPy restatement where they refuse (n up to 16 384, row
counts past the LDS budget, the [[6480,1296]] hypergraph product), and through the models and standalone decoders that now take it."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd.decoding import _binary_graph
from helpers import binary_oracle, code, gpu_graph, llr_const, oracle_library_forms, random_sparse_basis, to_gpu
from test_gpu_osd_shapes import SENTINEL, SHAPES, max_rows
from test_osd_search_cpu import osd_search_batch
from test_osd_workspace_cpu import eliminate_packed

pytestmark = pytest.mark.gpu

METHOD = {"osd0": 0, "osd_e": 1, "osd_cs": 2}
SEED = 0x5EED


def _graph(basis, rows=None):
    g = _binary_graph(basis, None, None)
    g.set_basis(0, np.arange(basis.shape[0], dtype=np.int32) if rows is None else rows)
    return g


def _inputs(rng, B, basis, p=0.05):
    n = basis.shape[1]
    llr = rng.normal(1.0, 2.5, size=(B, n)).astype(np.float32)
    llr[:, ::5] = np.float32(0.75)  # ties in the sort
    err = (rng.uniform(size=(B, n)) < p).astype(np.int64)
    synd = (err @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    return llr, synd


def _run(g, fn, B, n, idx, **kw):
    """e_hat / chosen after one call with sentinels everywhere; the unlisted samples must keep them."""
    e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
    chosen = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    gidx = None if idx is None else to_gpu(np.asarray(idx, np.int32))
    fn(e, chosen, gidx, 0 if idx is None else len(idx))
    torch.cuda.synchronize()
    e, chosen = e.cpu().numpy(), chosen.cpu().numpy()
    rest = np.setdiff1d(np.arange(B), np.arange(B) if idx is None else idx)
    assert (e[rest] == SENTINEL).all() and (chosen[rest] == -7).all(), "unlisted samples must be left untouched"
    return e, chosen


def _ws_call(g, synd, llr, method, order, side=0, workspace=None, marg=None):
    def fn(e, chosen, gidx, nact):
        kw = dict(marg=to_gpu(marg)) if marg is not None else dict(llr_bin=to_gpu(llr))
        g.osd_ws(side, to_gpu(synd), e, method, order, index=gidx, nact=nact, chosen=chosen, workspace=workspace, **kw)
    return fn


def _deficient(basis, rng):
    """The same row space with two duplicate rows and a sum of two rows added (each reduces to an all-zero row), rows shuffled."""
    s = basis[0] ^ basis[1]
    extra = [basis[-1], basis[0]] + ([s] if s.any() else [])
    d = np.concatenate([basis, np.stack(extra)]).astype(np.uint8)
    return d[rng.permutation(len(d))]


@pytest.mark.parametrize("n", SHAPES)
def test_equal_to_the_lds_kernels(n):
    """osd_ws == osd0 / osd bit for bit in e_hat and chosen at every n of the LDS kernels' shape sweep, full-rank and rank-deficient
    bases, with and without an index list.  A zero row of the rank-deficient basis reaches the workspace kernel's zero-row branch."""
    rng = np.random.RandomState(n)
    full, _ = random_sparse_basis(n, 400 if n >= 2046 else max(3, n // 2), seed=n)
    B = 5 if n >= 1023 else 10
    for basis in (full, _deficient(full, rng)):
        assert basis.shape[0] <= max_rows(n, True)
        g = _graph(basis)
        llr, synd = _inputs(rng, B, basis)
        ws = g.osd_workspace(0, "osd_cs", 7, slots=3)
        for idx in (None, np.array([B - 1, 0, 2], np.int32)):
            for method, order in (("osd0", 0), ("osd_e", 4), ("osd_cs", 7)):
                if method == "osd0":
                    e_ref, _ = _run(g, lambda e, c, i, k: g.osd0(0, to_gpu(synd), e, llr_bin=to_gpu(llr), index=i, nact=k), B, n, idx)
                    _, c_ref = _run(g, lambda e, c, i, k: g.osd(0, to_gpu(synd), e, "osd0", 0, llr_bin=to_gpu(llr), index=i, nact=k,
                                                                chosen=c), B, n, idx)
                else:
                    e_ref, c_ref = _run(g, lambda e, c, i, k: g.osd(0, to_gpu(synd), e, method, order, llr_bin=to_gpu(llr), index=i,
                                                                    nact=k, chosen=c), B, n, idx)
                e, c = _run(g, _ws_call(g, synd, llr, method, order, workspace=ws), B, n, idx)
                assert np.array_equal(e, e_ref), f"{method} {order}: e_hat differs"
                assert np.array_equal(c, c_ref), f"{method} {order}: chosen differs"


def _check_against_restatement(g, basis, llr, synd, configs, idx, og=None, rows=None, consistent=True):
    B, n = llr.shape
    ids = np.arange(B) if idx is None else np.asarray(idx)
    e0, c0 = _run(g, _ws_call(g, synd, llr, "osd0", 0), B, n, idx)
    assert (c0[ids] == 0).all()
    sh = synd if rows is None else synd[:, rows]
    sub = basis if rows is None else basis[rows]
    if og is not None:
        ref = og.osd0(0, np.arange(basis.shape[0], dtype=np.int32) if rows is None else rows, synd, llr_bin=llr,
                      index=None if idx is None else np.asarray(idx, np.int32))
        assert np.array_equal(e0[ids], ref[ids]), "osd0 differs from og_osd0"
    if consistent:
        assert np.array_equal(e0[ids].astype(np.int64) @ sub.T % 2, sh[ids]), "osd0: H e != s"
    elims = {b: eliminate_packed(llr[b], sub, sh[b]) for b in ids}
    for method, order in configs:
        e, c = _run(g, _ws_call(g, synd, llr, method, order), B, n, idx)
        re, rc = osd_search_batch(llr, sub, sh, METHOD[method], order, ids, elims=elims)
        assert np.array_equal(e[ids], re[ids]), f"{method} {order}: e_hat differs"
        assert np.array_equal(c[ids], rc[ids]), f"{method} {order}: chosen differs"
        if consistent:
            assert np.array_equal(e[ids].astype(np.int64) @ sub.T % 2, sh[ids]), f"{method} {order}: H e != s"


@pytest.mark.parametrize("n", [600, 2047])
def test_rows_past_the_lds_budget(n):
    """One row more than fgnn_osd0 takes (rows repeat: a rank-deficient basis); the LDS kernels refuse, osd_ws answers."""
    r0 = max_rows(n, False)
    m = min(r0 + 1, 500)
    basis, _ = random_sparse_basis(n, m, seed=n + 3)
    rows = np.arange(r0 + 1, dtype=np.int32) % m
    g = _graph(basis, rows)
    assert not g.osd_resident(0, "osd0") and not g.osd_resident(0, "osd_cs")
    rng = np.random.RandomState(n)
    llr, synd = _inputs(rng, 3, basis, 0.04)
    _check_against_restatement(g, basis, llr, synd, [("osd_e", 4), ("osd_cs", 3)], np.array([2, 0], np.int32), og=binary_oracle(basis),
                               rows=rows)


@pytest.mark.parametrize("n", [2048, 2049, 4095, 4096, 4097, 8191, 8193, 16384])
def test_n_past_2047(n):
    basis, _ = random_sparse_basis(n, 96, seed=n)
    g = _graph(basis)
    assert not g.osd_resident(0, "osd0")
    rng = np.random.RandomState(n)
    llr, synd = _inputs(rng, 3, basis, 0.002)
    configs = [("osd_e", 4)] + ([("osd_cs", 3)] if n <= 4097 else [])
    _check_against_restatement(g, basis, llr, synd, configs, np.array([1, 2], np.int32), og=binary_oracle(basis))


def test_n_16385_is_refused():
    n = 16385
    basis, _ = random_sparse_basis(n, 8, seed=n, col_weight=1)
    g = _graph(basis)
    e = torch.full((2, n), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    for method in ("osd0", "osd_cs"):
        with pytest.raises(ValueError, match="n <= 16384"):
            g.osd_ws(0, to_gpu(np.zeros((2, 8), np.uint8)), e, method, 2, llr_bin=to_gpu(np.ones((2, n), np.float32)), workspace=ws)
        with pytest.raises(ValueError, match="n <= 16384"):
            g.osd_workspace(0, method, 2, slots=1)
    torch.cuda.synchronize()
    assert (e.cpu().numpy() == SENTINEL).all()


def _hp_big_failures(B=32, p=0.03):
    """BP4 (the GMEM kernel: hp_big's state does not fit in LDS) on B samples at p: the oracle's and the GPU's outputs and the failures."""
    c = code("hp_big")
    og, gg = oracle_library_forms("hp_big"), gpu_graph("hp_big")
    ex, ez = og.pauli_noise(SEED, p, 0, B)
    sx, sz = og.syndrome(ex, ez)
    o = gg.bp4_decode(to_gpu(sx), to_gpu(sz), 10, "minsum", 0.8, llr_const=llr_const(p), want_logits=False)
    _, _, flags = og.residual(ex, ez, o["x_hat"].cpu().numpy(), o["z_hat"].cpu().numpy())
    fail = np.nonzero(flags & 1)[0].astype(np.int32)
    assert len(fail) >= 4, len(fail)
    return c, og, gg, sx, sz, o, fail


def test_hp_big_osd0_both_sides_equals_the_oracle():
    c, og, gg, sx, sz, o, fail = _hp_big_failures()
    gg.set_basis(0, c.pivot_hx)
    gg.set_basis(1, c.pivot_hz)
    assert not gg.osd_resident(0, "osd0") and not gg.osd_resident(1, "osd0")
    marg = o["llr"].cpu().numpy()
    idx = fail[:6]
    for side, synd, pivot in ((0, sx, c.pivot_hx), (1, sz, c.pivot_hz)):
        B = synd.shape[0]
        e, ch = _run(gg, _ws_call(gg, synd, None, "osd0", 0, side=side, marg=marg), B, c.N, idx)
        ref = og.osd0(side, pivot, synd, marg=marg, index=idx)
        assert np.array_equal(e[idx], ref[idx]), f"side {side}"
        h = np.asarray(c.hx if side == 0 else c.hz)
        assert np.array_equal(e[idx].astype(np.int64) @ h.T % 2, synd[idx]), f"side {side}: H e != s"


def test_hp_big_osd_cs_8_equals_the_restatement():
    c, og, gg, sx, sz, o, fail = _hp_big_failures()
    gg.set_basis(0, c.pivot_hx)
    basis = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    marg = o["llr"].cpu().numpy()
    llr = (marg[:, 2] - marg[:, 1]).astype(np.float32)  # any finite binary reliabilities
    idx = fail[:3]
    sh = sx[:, c.pivot_hx]
    e, ch = _run(gg, _ws_call(gg, sx, llr, "osd_cs", 8), sx.shape[0], c.N, idx)
    elims = {b: eliminate_packed(llr[b], basis, sh[b]) for b in idx}
    re, rc = osd_search_batch(llr, basis, sh, METHOD["osd_cs"], 8, idx, elims=elims)
    assert np.array_equal(e[idx], re[idx]) and np.array_equal(ch[idx], rc[idx])
    assert np.array_equal(e[idx].astype(np.int64) @ np.asarray(c.hx).T % 2, sx[idx])


def test_workspace_contract():
    """1, 3 and the default number of slots give identical outputs; a canary after the reported bytes is untouched; one byte short of
    one slot is refused (ValueError) with e_hat untouched."""
    n = 2049
    basis, _ = random_sparse_basis(n, 300, seed=9)
    g = _graph(basis)
    rng = np.random.RandomState(9)
    B = 7
    llr, synd = _inputs(rng, B, basis)
    idx = np.array([6, 1, 3, 0, 5], np.int32)
    for method, order in (("osd0", 0), ("osd_cs", 5)):
        slot = g.osd_slot_bytes(0, method, order)
        outs = []
        for slots in (1, 3, None):
            ws = g.osd_workspace(0, method, order, slots=slots)
            nbytes = ws.numel()
            assert nbytes == slot * (slots or g.osd_default_slots(0, method, order))
            buf = torch.full((nbytes + 4096,), 0x3C, dtype=torch.uint8, device="cuda")
            outs.append(_run(g, _ws_call(g, synd, llr, method, order, workspace=buf[:nbytes]), B, n, idx))
            assert bool((buf[nbytes:] == 0x3C).all()), "bytes past the workspace were written"
        for e, c in outs[1:]:
            assert np.array_equal(e, outs[0][0]) and np.array_equal(c, outs[0][1])
        short = torch.zeros(slot - 1, dtype=torch.uint8, device="cuda")
        e = torch.full((B, n), SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="workspace too small"):
            g.osd_ws(0, to_gpu(synd), e, method, order, llr_bin=to_gpu(llr), workspace=short)
        torch.cuda.synchronize()
        assert (e.cpu().numpy() == SENTINEL).all()
    assert 1 <= g.osd_default_slots(0, "osd_cs", 5) <= 2 * torch.cuda.get_device_properties(0).multi_processor_count


def test_bp4_osd_model_on_hp_big_equals_the_oracle_pipeline():
    c = code("hp_big")
    B, p, IT = 32, 0.03, 10
    dec = F.QLDPCBPDecoder(code=c, num_iter=IT, normalization_factor=0.8, cn_type="minsum", stage_one=True)
    m = F.BP4_OSD_Model(c, dec, F.OSD0_Decoder(c.N), seed=SEED)
    o = m.decode(B, p)
    assert m.last_num_osd > 0
    og = oracle_library_forms("hp_big")
    ex, ez = og.pauli_noise(SEED, p, 0, B)
    assert np.array_equal(ex, o["noise_x"].cpu().numpy()) and np.array_equal(ez, o["noise_z"].cpu().numpy())
    sx, sz = og.syndrome(ex, ez)
    r = og.bp4_decode(sx, sz, IT, "minsum", 0.8, llr_const=llr_const(p))
    _, _, flags = og.residual(ex, ez, r["x_hat"], r["z_hat"])
    fail = np.nonzero(flags & 1)[0].astype(np.int32)
    assert len(fail) == m.last_num_osd
    z, x = r["z_hat"].copy(), r["x_hat"].copy()
    og.osd0(0, c.pivot_hx, sx, marg=r["llr"], index=fail, e_hat=z)
    og.osd0(1, c.pivot_hz, sz, marg=r["llr"], index=fail, e_hat=x)
    xg, zg = o["x_hat"].cpu().numpy(), o["z_hat"].cpu().numpy()
    assert np.array_equal(zg, z) and np.array_equal(xg, x)
    assert np.array_equal(zg[fail].astype(np.int64) @ np.asarray(c.hx).T % 2, sx[fail])
    assert np.array_equal(xg[fail].astype(np.int64) @ np.asarray(c.hz).T % 2, sz[fail])


def test_bp4_osd_model_on_hp_big_with_osd_cs():
    c = code("hp_big")
    dec = F.QLDPCBPDecoder(code=c, num_iter=10, normalization_factor=0.8, cn_type="minsum", stage_one=True)
    m = F.BP4_OSD_Model(c, dec, F.OSD_Decoder(c.N, "osd_cs", 4), seed=SEED)
    o = m.decode(16, 0.03)
    assert m.last_num_osd > 0
    sx, sz = m.graph.syndrome(o["noise_x"], o["noise_z"])
    s2x, s2z = m.graph.syndrome(o["x_hat"], o["z_hat"])
    assert torch.equal(sx, s2x) and torch.equal(sz, s2z), "every OSD-processed sample satisfies its syndrome"


def test_bp2_osd_model_on_hp_big_hx():
    c = code("hp_big")
    bp2 = F.LDPCBPDecoder(c.hx, is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=10, normalization_factor=0.8)
    m = F.BP2_OSD_Model(c.hx, c.hx_basis, c.pivot_hx, c.lx, bp2, F.OSD0_Decoder(c.N))
    zeros, ls = m(16, 0.03)
    assert ls.shape == (16, np.asarray(c.lx).shape[0]) and not bool(zeros.any())
    assert m.last_num_osd > 0


def test_standalone_decoders_on_hp_big_agree_with_osd_ws():
    c = code("hp_big")
    basis = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    rank, n = basis.shape
    g = _graph(basis)
    rng = np.random.RandomState(6480)
    B = 3
    llr, synd = _inputs(rng, B, basis, 0.02)
    for dec, method, order in ((F.OSD0_Decoder(n), "osd0", 0), (F.OSD_Decoder(n, "osd_cs", 7), "osd_cs", 7)):
        e = dec(torch.from_numpy(llr).cuda(), torch.from_numpy(basis.astype(np.int32)).cuda(), torch.from_numpy(synd.T.copy()).cuda(), B)
        ref = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
        g.osd_ws(0, to_gpu(synd), ref, method, order, llr_bin=to_gpu(llr))
        assert np.array_equal(e.cpu().numpy(), ref.cpu().numpy().astype(bool)), method
        assert np.array_equal(e.cpu().numpy().astype(np.int64) @ basis.T % 2, synd)
