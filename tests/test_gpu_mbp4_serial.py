"""MBP4 / AMBP4 in the serial schedule on the GPU (fgnn_mbp4_decode_serial), held to the restatement tests/mbp4_serial_reference.py bit
for bit: x_hat and z_hat as bytes, all four stats columns as int32, no tolerance anywhere and no sample left out.  The restatement is
NumPy float32 on the rules of tests/mbp4_reference.py; tests/test_mbp4_serial_reference_cpu.py checks its schedule and ties the
single-output check rule of the kernel to cn_update.

Where a test relies on samples leaving the kernel at different attempts it asserts so on the restatement's stats."""
import zlib

import numpy as np
import pytest
import torch

import mbp4_reference as MB
import mbp4_serial_reference as MS
import test_gpu_bp4gd as TGD
from helpers import _bare_code, code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_bp4fb_reference_cpu import depolarizing
from test_mbp4_serial_reference_cpu import (GHP882_SERIAL_FIGURES, ghp882_samples, ghp882_serial_figures, ghp882_serial_reference,
                                            irregular_code, one_layer_code, one_layer_llrs, random_syndromes)

pytestmark = pytest.mark.gpu

F32 = np.float32
LDS_BUDGET = TGD.LDS_BUDGET
CN_TYPES = TGD.CN_TYPES
noisy, informed_edge_channel = TGD.noisy, TGD.informed_edge_channel


def serial_lds_bytes(E, n, cpb):
    """fgnn_mbp4_decode_serial: E messages each way and n decision bytes per codeword, each area rounded up to 4 floats; the two
    64-float tables, a stamp per codeword and ndone."""
    area = ((n + 3) // 4 + 3) & ~3
    per_cw = 2 * ((E + 3) & ~3) + area
    return per_cw * 4 * cpb + 2 * 64 * 4 + ((cpb + 1 + 3) & ~3) * 4


def tables(alphas, base=0.8):
    return MB.mbp4_tables(alphas, base)


def bare_graph(c):
    from feedback_gnn_amd.graph import TannerGraph
    return TannerGraph(_bare_code(c.hx, c.hz), stage_one=False)


def gpu(g, sx, sz, factors, owns, pre, att, cn_type="minsum", restart=True, **llr):
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    xh, zh, stats = g.mbp4_decode_serial(to_gpu(sx), to_gpu(sz), factors, owns, pre, att, cn_type, restart=restart, **gl)
    assert stats.dtype == torch.int32 and xh.dtype == torch.uint8 and zh.dtype == torch.uint8
    return xh.cpu().numpy(), zh.cpu().numpy(), stats.cpu().numpy()


def both(c, g, sx, sz, factors, owns, pre, att, cn_type="minsum", restart=True, ref=None, layer_of=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, stats).  `ref`:
    a restatement result to compare with instead of computing it; `layer_of`: the layering the graph carries, for the restatement."""
    x1, z1, s1 = gpu(g, sx, sz, factors, owns, pre, att, cn_type, restart, **llr)
    x0, z0, s0 = ref or MS.mbp4_decode_serial(c, sx, sz, factors, owns, pre, att, cn_type, restart=restart, layer_of=layer_of, **llr)
    print(cn_type, "restart", restart, "found", s0[:, 0].tolist(), "a", s0[:, 1].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    assert x0.tobytes() == x1.tobytes() and z0.tobytes() == z1.tobytes()
    return x0, z0, s0


def split(stats):
    solved = stats[:, 0] > 0
    return int((solved & (stats[:, 1] == 0)).sum()), int((solved & (stats[:, 1] > 0)).sum()), int((~solved).sum())


def ibm72_batch():
    return depolarizing(oracle_library_forms("ibm72", stage_one=False), 0.10, 40)


# ---- 1: ibm72, all three rules, restart on and off --------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_ibm72(cn_type, restart):
    c, g = code("ibm72"), gpu_graph("ibm72")
    _, _, sx, sz = ibm72_batch()
    _, _, s0 = both(c, g, sx, sz, *tables((1.0, 0.8, 0.6)), 3, 2, cn_type, restart, llr_const=llr_const(0.10))
    first, later, never = split(s0)
    assert first > 0 and later > 0 and never > 0, "samples solved in attempt 0, solved later and never solved"
    if cn_type == "minsum":
        assert (first, later, never) == ((22, 2, 16) if restart else (22, 16, 2))
    num, lay = g.qubit_layers()  # a graph without a layering got the greedy one; the tests that install another put it back
    num0, lay0 = MS.greedy_qubit_layers(c.hx, c.hz)
    assert num == num0 and np.array_equal(lay, lay0)


# ---- 2: fuzz ------------------------------------------------------------------------------------------------------------------------------
def test_ibm72_fuzzed():
    """B in 1..70, pre_iter and attempt_iter <= 6; one attempt with own = 1, three descending alphas with restart, five seeded weights
    and factors (own above 1 and own = 0 among them) without; a constant prior and per-qubit LLRs with edge values."""
    c, g, og = code("ibm72"), gpu_graph("ibm72"), oracle_library_forms("ibm72")
    rng = np.random.RandomState(zlib.crc32(b"mbs-ibm72"))
    p = 0.10
    for (factors, owns), restart in ((tables((1.0,), 1.0), False), (tables((1.0, 0.8, 0.6)), True),
                                    ((rng.uniform(0.4, 1.3, 5).astype(F32), np.array([1.0, 0.0, 1.25, 0.7, 0.45], F32)), False)):
        B, pre, att = int(rng.randint(1, 71)), int(rng.randint(1, 7)), int(rng.randint(1, 7))
        ex, ez, sx, sz = noisy(og, p, B, first=int(rng.randint(1 << 20)))
        both(c, g, sx, sz, factors, owns, pre, att, "minsum", restart, llr_const=llr_const(p))
        _, _, s0 = both(c, g, sx, sz, factors, owns, pre, att, "minsum", restart,
                        llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))))
    ex, ez, sx, sz = noisy(og, p, 40)
    _, _, s0 = both(c, g, sx, sz, *tables((1.0, 0.9, 0.8, 0.7, 0.6, 0.5)), 3, 3, "minsum", True, llr_ch=informed_edge_channel(ex, ez, 77))
    assert (s0[:, 0] > 0).any() and (s0[:, 1] > 0).any(), "solutions and later attempts must occur under per-qubit LLRs too"


# ---- 3: runtime degrees -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_irregular_graph(cn_type):
    """Checks of degree 1, 2, 3, 4, 5 and 6, qubits of degree 0 to 4 (qubit 11 has no check), and rsurf5 with its boundary checks of
    degree 2 and several codewords per workgroup."""
    c = irregular_code()
    assert sorted(set(c.hx.sum(1).tolist() + c.hz.sum(1).tolist())) == [1, 2, 3, 4, 5, 6]
    g = bare_graph(c)
    B = 37
    sx, sz = random_syndromes(c, B, 9)
    llr = np.random.RandomState(4).uniform(-1.0, 5.0, size=(B, 3, 12)).astype(F32)
    for restart in (True, False):
        _, _, s0 = both(c, g, sx, sz, *tables((1.0, 0.7, 0.5)), 3, 2, cn_type, restart, llr_ch=llr)
        assert len(set(s0[:, 2].tolist())) >= 3, "samples must stop after different numbers of iterations"
    c, g, og = code("rsurf5"), gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    assert g.info()["codewords_per_block"] > 1
    _, _, sx, sz = noisy(og, 0.15, g.info()["codewords_per_block"] + 3)
    _, _, s0 = both(c, g, sx, sz, *tables((1.0, 0.8, 0.6, 0.4)), 3, 2, cn_type, True, llr_const=llr_const(0.15))
    assert (s0[:, 1] > 0).any() and (s0[:, 0] > 0).any()


# ---- 4: layerings of the caller -------------------------------------------------------------------------------------------------------------
def test_custom_layerings():
    c, g = code("ibm72"), gpu_graph("ibm72")
    _, _, sx, sz = ibm72_batch()
    args = (sx, sz, *tables((1.0, 0.8, 0.6)), 3, 2, "minsum", True)
    g.set_qubit_layers(None)
    greedy = both(c, g, *args, llr_const=llr_const(0.10))
    num, lay = g.qubit_layers()
    try:
        _custom_layerings(c, g, args, greedy, num, lay)
    finally:
        g.set_qubit_layers(None)  # the graph may be shared with other tests
    assert np.array_equal(g.qubit_layers()[1], lay)
    both(c, g, *args, ref=greedy, llr_const=llr_const(0.10))


def _custom_layerings(c, g, args, greedy, num, lay):
    for layer_of in (np.arange(72, dtype=np.int32), (num - 1 - lay).astype(np.int32)):
        g.set_qubit_layers(layer_of)
        assert g.qubit_layers()[0] == int(layer_of.max()) + 1 and np.array_equal(g.qubit_layers()[1], layer_of)
        other = both(c, g, *args, layer_of=layer_of, llr_const=llr_const(0.10))
        assert not (other[0].tobytes() == greedy[0].tobytes() and other[1].tobytes() == greedy[1].tobytes()
                    and np.array_equal(other[2], greedy[2])), "another order of the qubits gives another result"
    # a refused layering leaves the installed one in place
    kept = g.qubit_layers()[1].copy()
    with pytest.raises(ValueError, match=r"qubit \d+ and qubit \d+ of layer \d+ share h[xz] check \d+"):
        g.set_qubit_layers(np.zeros(72, np.int32))
    with pytest.raises(ValueError, match="layer_of must have shape"):
        g.set_qubit_layers(np.zeros(71, np.int32))
    assert np.array_equal(g.qubit_layers()[1], kept)


# ---- 5: launch geometries -------------------------------------------------------------------------------------------------------------------
def test_launch_geometries_give_identical_bytes():
    c, g = code("ibm72"), gpu_graph("ibm72")
    _, _, sx, sz = ibm72_batch()
    sx, sz = sx[:37], sz[:37]
    args = (sx, sz, *tables((1.0, 0.8, 0.6)), 3, 2, "boxplus-phi", False)
    ref = both(c, g, *args, llr_const=llr_const(0.10))
    assert (ref[2][:, 1] > 0).any()
    try:
        for tpc, cpb in ((64, 1), (32, 4), (4, 16), (128, 2), (1024, 1)):
            assert 37 % cpb != 0 or cpb == 1
            g.set_launch(tpc, cpb)
            both(c, g, *args, ref=ref, llr_const=llr_const(0.10))
    finally:
        g.set_launch(0, 0)


# ---- 6: one layer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_one_layer_code_is_the_flooding_kernel(cn_type):
    c = one_layer_code()
    g = bare_graph(c)
    B = 48
    sx, sz = random_syndromes(c, B, 5, p=0.3)
    llr = to_gpu(one_layer_llrs(B))
    f3, o3 = tables((1.0, 0.8, 0.6))
    later = False
    for f, o, restart in ((f3[:1], o3[:1], False), (f3, o3, True), (f3, np.full(3, 0.7, F32), False)):
        for kw in (dict(llr_const=0.4), dict(llr_ch=llr)):
            want = g.mbp4_decode(to_gpu(sx), to_gpu(sz), f, o, 3, 2, cn_type, restart=restart, **kw)
            got = g.mbp4_decode_serial(to_gpu(sx), to_gpu(sz), f, o, 3, 2, cn_type, restart=restart, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (cn_type, restart, sorted(kw))
            later |= bool((want[2][:, 1] > 0).any())
    assert g.qubit_layers()[0] == 1 and later


# ---- 7: [[882,24]] --------------------------------------------------------------------------------------------------------------------------
def test_ghp882_batch():
    """The batch of tests/test_mbp4_serial_reference_cpu.py at alpha 1.0 alone: identical to the restatement, and its figures."""
    c, g = code("ghp882"), gpu_graph("ghp882")
    _, _, sx, sz = ghp882_samples()
    x0, z0, st = both(c, g, sx, sz, *tables((1.0,)), 64, 64, ref=ghp882_serial_reference(), llr_const=llr_const(0.10))
    assert g.qubit_layers()[0] == 14
    assert ghp882_serial_figures(x0, z0, st) == GHP882_SERIAL_FIGURES and GHP882_SERIAL_FIGURES[0] < 7


# ---- 8: refusals and the empty batch ----------------------------------------------------------------------------------------------------------
def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    need = serial_lds_bytes(g.E_x + g.E_z, g.n, 1)
    assert 2 * (g.E_x + g.E_z) * 4 > LDS_BUDGET and need > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS.*{need} bytes.*limit is {LDS_BUDGET}"):
        g.mbp4_decode_serial(sx, sz, [0.8, 1.0], [1.0, 0.8], 3, 3, llr_const=2.0)


def test_ghp882_lds_is_what_the_kernel_states():
    g = gpu_graph("ghp882")
    assert serial_lds_bytes(g.E_x + g.E_z, g.n, 1) == 43232 + 512 + 16
    assert 3 * serial_lds_bytes(g.E_x + g.E_z, g.n, 1) <= 160 * 1024 < 4 * serial_lds_bytes(g.E_x + g.E_z, g.n, 1)


def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.mbp4_decode_serial(sx, sz, [0.8], [1.0], 2, 2, cn_type="sum-product")
    for count in (0, 65):
        with pytest.raises(ValueError, match="num_attempts"):
            g.mbp4_decode_serial(sx, sz, [0.8] * count, [1.0] * count, 2, 2)
    with pytest.raises(ValueError, match="same length"):
        g.mbp4_decode_serial(sx, sz, [0.8, 0.9], [1.0], 2, 2)
    for pre, att in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            g.mbp4_decode_serial(sx, sz, [0.8], [1.0], pre, att)
    with pytest.raises(ValueError, match="restart"):
        g.mbp4_decode_serial(sx, sz, [0.8], [1.0], 2, 2, restart=2)
    for f in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="factor"):
            g.mbp4_decode_serial(sx, sz, [0.8, f], [1.0, 1.0], 2, 2)
    for o in (-0.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="own"):
            g.mbp4_decode_serial(sx, sz, [0.8, 0.8], [1.0, o], 2, 2)
    with pytest.raises(ValueError, match="synd_x"):
        g.mbp4_decode_serial(sx[:, :-1].contiguous(), sz, [0.8], [1.0], 2, 2)
    with pytest.raises(ValueError, match="llr_ch"):
        g.mbp4_decode_serial(sx, sz, [0.8], [1.0], 2, 2, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="B is needed"):
        g.mbp4_decode_serial(None, None, [0.8], [1.0], 2, 2)
    xh, zh, st = (torch.zeros((2, n), dtype=torch.uint8, device=g.device), torch.zeros((2, n), dtype=torch.uint8, device=g.device),
                  torch.zeros((2, 4), dtype=torch.int32, device=g.device))
    tab = np.array([0.8], F32)
    call = lambda factor, own, stats: _lib.lib().fgnn_mbp4_decode_serial(  # noqa: E731
        g.handle, 2, 1, factor, own, 2, 2, 1, None, 2.0, sx.data_ptr(), sz.data_ptr(), 2, xh.data_ptr(), zh.data_ptr(), stats, None)
    t = tab.ctypes.data
    for factor, own, stats, word in ((None, t, st.data_ptr(), "factor and own"), (t, None, st.data_ptr(), "factor and own"),
                                     (t, t, None, "no output buffer")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(factor, own, stats))


def test_zero_and_null_syndrome_and_an_empty_batch():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n, B = g.n, 9
    factors, owns = tables((1.0, 0.7))
    zx, zz = np.zeros((B, g.m_x), np.uint8), np.zeros((B, g.m_z), np.uint8)
    x0, z0, s0 = both(code("ibm72"), g, zx, zz, factors, owns, 6, 5, llr_const=2.0)
    assert not x0.any() and not z0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1)))
    xn, zn, sn = g.mbp4_decode_serial(None, None, factors, owns, 6, 5, llr_const=2.0, B=B)
    assert not xn.any() and not zn.any() and np.array_equal(sn.cpu().numpy(), s0)
    sx = torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((0, g.m_z), dtype=torch.uint8, device=g.device)
    xh, zh, st = g.mbp4_decode_serial(sx, sz, [0.8], [1.0], 2, 2)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)
    tab = np.array([0.8], F32)
    assert _lib.lib().fgnn_mbp4_decode_serial(g.handle, 2, 1, tab.ctypes.data, tab.ctypes.data, 2, 2, 1, None, 2.0, None, None, 0, None,
                                              None, None, None) == 0


# ---- 9: classes -------------------------------------------------------------------------------------------------------------------------------
def test_ambp4_decoder_and_model_in_the_serial_schedule():
    import feedback_gnn_amd as F
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    n, B, p = og.n, 40, 0.10
    g = gpu_graph("ibm72")
    flooding = F.AMBP4Decoder(c, num_iter=3, graph=g)
    assert flooding.schedule == "flooding"
    dec = F.AMBP4Decoder(c, num_iter=3, graph=g, schedule="serial")
    assert dec.schedule == "serial" and g.qubit_layers()[0] == 8
    ex, ez, sx, sz = noisy(og, p, B)
    llr = np.full((B, 3, n), llr_const(p), F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    x0, z0, s0 = MS.mbp4_decode_serial(c, sx, sz, dec.factors, dec.owns, 3, 3, "minsum", restart=True, llr_ch=llr)
    assert np.array_equal(x_hat.cpu().numpy(), x0) and np.array_equal(z_hat.cpu().numpy(), z0)
    assert np.array_equal(dec.last_stats.cpu().numpy(), s0) and (s0[:, 1] > 0).any()
    xf, zf = flooding((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    xm, zm, sm = MB.mbp4_decode(c, sx, sz, dec.factors, dec.owns, 3, 3, "minsum", restart=True, llr_ch=llr)
    assert np.array_equal(xf.cpu().numpy(), xm) and np.array_equal(flooding.last_stats.cpu().numpy(), sm), "flooding is as it was"
    order = np.arange(n, dtype=np.int32)
    try:
        lit = F.AMBP4Decoder(c, num_iter=3, graph=g, schedule="serial", layers=order)
        assert lit.graph is g and np.array_equal(g.qubit_layers()[1], order)
    finally:
        g.set_qubit_layers(None)
    model = F.BP4_AMBP_Model(c, dec, seed=0x5EED)
    model(B, p)
    ox, oz = og.pauli_noise(0x5EED, p, 0, B)
    sx, sz = og.syndrome(ox, oz)
    x0, z0, s0 = MS.mbp4_decode_serial(c, sx, sz, dec.factors, dec.owns, 3, 3, llr_const=llr_const(p))
    assert np.array_equal(model.last_x_hat.cpu().numpy(), x0) and np.array_equal(model.last_stats.cpu().numpy(), s0)
    assert model.last_num_unsolved == int((s0[:, 0] == 0).sum())
