"""BP4 with message-strength control on the GPU (fgnn_mbp4_decode) at every mbp4_kernel instantiation, held to the restatement
tests/mbp4_reference.py bit for bit: x_hat and z_hat as bytes, all four stats columns as int32, no tolerance anywhere and no sample
left out.  The restatement is NumPy float32 on the oracle's transcendentals; tests/test_mbp4_reference_cpu.py ties it to the oracle's
BP4 and to the host build of vn_edge_own.

The noise is the library's seeded depolarizing stream at the rate per code of tests/test_gpu_bp4gd.py (P_OF).  Where a test relies on
samples leaving the kernel at different attempts it asserts so on the restatement's stats."""
import zlib

import numpy as np
import pytest
import torch

import mbp4_reference as MB
import test_gpu_bp4gd as TGD
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_mbp4_reference_cpu import ALPHAS, GHP882_FIGURES, ghp882_figures, ghp882_reference, ghp882_samples

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = TGD.LDS_BUDGET
P_OF = TGD.P_OF
CN_TYPES = TGD.CN_TYPES
noisy, informed_edge_channel, instantiation = TGD.noisy, TGD.informed_edge_channel, TGD.instantiation  # the dispatch rule is BP4-GD's


def mbp4_lds_bytes(E, n, cpb):
    """fgnn_mbp4_decode: E messages and n decision bytes per codeword, each rounded up to 4 floats; the two 64-float tables, a stamp per
    codeword and ndone."""
    area = ((n + 3) // 4 + 3) & ~3
    per_cw = ((E + 3) & ~3) + area
    return per_cw * 4 * cpb + 2 * 64 * 4 + ((cpb + 1 + 3) & ~3) * 4


def tables(alphas, base=0.8):
    return MB.mbp4_tables(alphas, base)


def both(name, g, sx, sz, factors, owns, pre, att, cn_type="minsum", restart=True, ref=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, stats).  `ref`:
    a restatement result to compare with instead of computing it."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    xh, zh, stats = g.mbp4_decode(to_gpu(sx), to_gpu(sz), factors, owns, pre, att, cn_type, restart=restart, **gl)
    x0, z0, s0 = ref or MB.mbp4_decode(code(name), sx, sz, factors, owns, pre, att, cn_type, restart=restart, **llr)
    assert stats.dtype == torch.int32 and xh.dtype == torch.uint8 and zh.dtype == torch.uint8
    s1, x1, z1 = stats.cpu().numpy(), xh.cpu().numpy(), zh.cpu().numpy()
    print(name, cn_type, "restart", restart, "found", s0[:, 0].tolist(), "a", s0[:, 1].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    assert x0.tobytes() == x1.tobytes() and z0.tobytes() == z1.tobytes()
    return x0, z0, s0


def split(stats):
    solved = stats[:, 0] > 0
    return int((solved & (stats[:, 1] == 0)).sum()), int((solved & (stats[:, 1] > 0)).sum()), int((~solved).sum())


def fuzz(name, g, og, rng, cn_types=("minsum",)):
    """B in 1..70, pre_iter and attempt_iter <= 12; one attempt with own = 1, three descending alphas with restart, five seeded weights
    and factors (own above 1 and own = 0 among them) without; a constant prior and per-qubit LLRs with edge values.  Then the fixed
    batch of 40 samples under the default alphas with short attempts, restart off and on."""
    p = P_OF[name]
    for cn in cn_types:
        for (factors, owns), restart in ((tables((1.0,), 1.0), False), (tables((1.0, 0.8, 0.6)), True),
                                        ((rng.uniform(0.4, 1.3, 5).astype(F32), np.array([1.0, 0.0, 1.25, 0.7, 0.45], F32)), False)):
            B, pre, att = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            ex, ez, sx, sz = noisy(og, p, B, first=int(rng.randint(1 << 20)))
            both(name, g, sx, sz, factors, owns, pre, att, cn, restart, llr_const=llr_const(p))
            both(name, g, sx, sz, factors, owns, pre, att, cn, restart, llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))))
        ex, ez, sx, sz = noisy(og, p, 40)
        for restart in (False, True):
            _, _, s0 = both(name, g, sx, sz, *tables(ALPHAS), 6, 4, cn, restart, llr_const=llr_const(p))
            first, later, never = split(s0)
            assert first > 0 and later + never > 0, "the batch must hold samples solved by the first alpha and samples that go on"
        _, _, s0 = both(name, g, sx, sz, *tables(ALPHAS), 6, 6, cn, True, llr_ch=informed_edge_channel(ex, ez, 77))
        assert (s0[:, 0] > 0).any() and (s0[:, 1] > 0).any(), "solutions and later attempts must occur under per-qubit LLRs too"


# ---- 1-3: both kinds of instantiation, all three check rules ------------------------------------------------------------------------------
def test_regular_instantiation():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    info = g.info()
    assert (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6) and instantiation(g) == (3, 6)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"mb-ibm72")))


def test_force_generic_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    g.force_generic(True)
    try:
        fuzz("ibm72", g, og, np.random.RandomState(17))
    finally:
        g.force_generic(False)


@pytest.mark.parametrize("cn_type", ["boxplus", "boxplus-phi"])
def test_the_two_other_rules_on_a_regular_graph(cn_type):
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"mb-ibm72" + cn_type.encode())), cn_types=(cn_type,))


@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb126"])
def test_loop_instantiation(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g) == (0, 0)
    fuzz(name, g, og, np.random.RandomState(zlib.crc32(b"mb-" + name.encode())))


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_loop_instantiation_toric4(cn_type):
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("toric4", g, og, np.random.RandomState(zlib.crc32(b"mb-toric4" + cn_type.encode())), cn_types=(cn_type,))


# ---- 4: several codewords per workgroup -------------------------------------------------------------------------------------------------
WG_ALPHAS = tuple(np.linspace(1.0, 0.3, 12).tolist())


@pytest.mark.parametrize("restart", [False, True])
def test_codewords_of_one_workgroup_stop_at_different_attempts(restart):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    L = llr_const(P_OF["rsurf5"])
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], B)  # the same first rows for every B
        _, _, stats = both("rsurf5", g, sx, sz, *tables(WG_ALPHAS), 4, 3, "minsum", restart, llr_const=L)
        first = stats[:cpb - 1]  # samples of the first workgroup
        assert len(set(first[:, 1].tolist())) >= 3, "the workgroup's samples must stop at different attempts"
        assert (first[:, 0] == 1).any()


# ---- 5: priors ------------------------------------------------------------------------------------------------------------------------------
def test_a_constant_prior_is_the_same_llr_on_every_qubit():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    p = P_OF["ibm72"]
    _, _, sx, sz = noisy(og, p, 24)
    L = llr_const(p)
    ref = both("ibm72", g, sx, sz, *tables(ALPHAS), 6, 4, llr_const=L)
    both("ibm72", g, sx, sz, *tables(ALPHAS), 6, 4, ref=ref, llr_ch=np.full((24, 3, og.n), L, F32))
    assert (ref[2][:, 1] > 0).any()


# ---- 6: syndromes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    B = 9
    zx, zz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    factors, owns = tables((1.0, 0.7))
    x0, z0, s0 = both(name, g, zx, zz, factors, owns, 6, 5, llr_const=2.0)
    assert not x0.any() and not z0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1)))
    xn, zn, sn = g.mbp4_decode(None, None, factors, owns, 6, 5, llr_const=2.0, B=B)
    assert not xn.any() and not zn.any() and np.array_equal(sn.cpu().numpy(), s0)


# ---- 7: the largest number of attempts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [False, True])
def test_sixty_four_attempts(restart):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    _, _, sx, sz = noisy(og, 0.25, 20)
    own = np.linspace(1.0, 0.05, 64).astype(F32)
    factor = np.linspace(0.5, 1.5, 64).astype(F32)
    _, _, s0 = both("rsurf5", g, sx, sz, factor, own, 2, 1, "minsum", restart, llr_const=llr_const(0.25))
    assert s0[:, 1].max() == 63 and (s0[:, 0] == 0).any(), "a sample must walk all 64 attempts"
    assert np.array_equal(s0[s0[:, 0] == 0], np.tile(np.array([0, 63, 2 + 63, 1], np.int32), (int((s0[:, 0] == 0).sum()), 1)))


# ---- 8: the stated equivalence, on the GPU --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_one_attempt_with_own_one_is_bp4fb_without_attempts_on_the_gpu(cn_type):
    g = gpu_graph("ghp882")
    B, T, p = 8, 12, 0.03
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    llr = to_gpu(informed_edge_channel(ex.cpu().numpy(), ez.cpu().numpy(), 5))
    for launch in ((0, 0), (256, 1)):
        g.set_launch(*launch)
        try:
            for kw in (dict(llr_const=llr_const(p)), dict(llr_ch=llr)):
                x0, z0, s0 = g.bp4fb_decode(sx, sz, "perturb", T, 5, 0, 2.0, cn_type, 0.8, **kw)
                for restart in (False, True):
                    xh, zh, st = g.mbp4_decode(sx, sz, [0.8], [1.0], T, 5, cn_type, restart=restart, **kw)
                    assert torch.equal(xh, x0) and torch.equal(zh, z0) and torch.equal(st, s0) and not st[:, 1].any()
            assert (s0[:, 0] == 1).any()
        finally:
            g.set_launch(0, 0)


# ---- 9: launch geometries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tpc,cpb", [(1, 64), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], cpb + 3, first=100)
        for restart in (False, True):
            _, _, s0 = both("rsurf5", g, sx, sz, *tables(WG_ALPHAS), 4, 3, "minsum", restart, llr_const=llr_const(P_OF["rsurf5"]))
            assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


# ---- 10-12: LDS and the packed rows -----------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    """ghp1270 with two codewords per workgroup (128 threads each): 2 x 31 760 bytes of codeword state, on the (3,3,6) instantiation."""
    g, og = gpu_graph("ghp1270"), oracle_library_forms("ghp1270")
    assert instantiation(g) == (3, 6)
    assert mbp4_lds_bytes(og.E_x + og.E_z, og.n, 1) <= 48 * 1024 < mbp4_lds_bytes(og.E_x + og.E_z, og.n, 2) <= LDS_BUDGET
    g.set_launch(128, 2)
    try:
        _, _, sx, sz = noisy(og, 0.08, 3)
        _, _, s0 = both("ghp1270", g, sx, sz, *tables((1.0, 0.8, 0.6)), 4, 3, llr_const=llr_const(0.08))
        assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


def test_packed_rows_above_32k():
    """bb1800: (3,3,6)-regular with packed slot offsets up to 43 196; dec[((off >> 2) - base) / DV] through the upper half of the 16-bit
    range.  Then the loop on the same inputs, against the same reference outputs."""
    g, og = gpu_graph("bb1800"), oracle_library_forms("bb1800")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    assert mbp4_lds_bytes(og.E_x + og.E_z, og.n, 1) <= LDS_BUDGET
    _, _, sx, sz = noisy(og, 0.05, 4)
    ref = both("bb1800", g, sx, sz, *tables((1.0, 0.8, 0.6)), 6, 3, llr_const=llr_const(0.05))
    assert (ref[2][:, 1] > 0).any(), "a sample must reach a later attempt"
    g.force_generic(True)
    try:
        both("bb1800", g, sx, sz, *tables((1.0, 0.8, 0.6)), 6, 3, ref=ref, llr_const=llr_const(0.05))
    finally:
        g.force_generic(False)


def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    need = mbp4_lds_bytes(g.E_x + g.E_z, g.n, 1)
    assert need > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS.*{need} bytes.*limit is {LDS_BUDGET}"):
        g.mbp4_decode(sx, sz, [0.8, 1.0], [1.0, 0.8], 3, 3, llr_const=2.0)


# ---- 13-14: arguments -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.mbp4_decode(sx, sz, [0.8], [1.0], 2, 2, cn_type="sum-product")
    for count in (0, 65):
        with pytest.raises(ValueError, match="num_attempts"):
            g.mbp4_decode(sx, sz, [0.8] * count, [1.0] * count, 2, 2)
    with pytest.raises(ValueError, match="same length"):
        g.mbp4_decode(sx, sz, [0.8, 0.9], [1.0], 2, 2)
    for pre, att in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            g.mbp4_decode(sx, sz, [0.8], [1.0], pre, att)
    with pytest.raises(ValueError, match="restart"):
        g.mbp4_decode(sx, sz, [0.8], [1.0], 2, 2, restart=2)
    for f in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="factor"):
            g.mbp4_decode(sx, sz, [0.8, f], [1.0, 1.0], 2, 2)
    for o in (-0.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="own"):
            g.mbp4_decode(sx, sz, [0.8, 0.8], [1.0, o], 2, 2)
    with pytest.raises(ValueError, match="synd_x"):
        g.mbp4_decode(sx[:, :-1].contiguous(), sz, [0.8], [1.0], 2, 2)
    with pytest.raises(ValueError, match="synd_z"):
        g.mbp4_decode(sx, sz.to(torch.int32), [0.8], [1.0], 2, 2)
    with pytest.raises(ValueError, match="llr_ch"):
        g.mbp4_decode(sx, sz, [0.8], [1.0], 2, 2, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="B is needed"):
        g.mbp4_decode(None, None, [0.8], [1.0], 2, 2)
    # the C entry point itself: a table or an output buffer missing
    xh, zh, st = (torch.zeros((2, n), dtype=torch.uint8, device=g.device), torch.zeros((2, n), dtype=torch.uint8, device=g.device),
                  torch.zeros((2, 4), dtype=torch.int32, device=g.device))
    tab = np.array([0.8], F32)
    call = lambda factor, own, stats: _lib.lib().fgnn_mbp4_decode(  # noqa: E731
        g.handle, 2, 1, factor, own, 2, 2, 1, None, 2.0, sx.data_ptr(), sz.data_ptr(), 2, xh.data_ptr(), zh.data_ptr(), stats, None)
    t = tab.ctypes.data
    for factor, own, stats, word in ((None, t, st.data_ptr(), "factor and own"), (t, None, st.data_ptr(), "factor and own"),
                                     (t, t, None, "no output buffer")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(factor, own, stats))
    g.mbp4_decode(sx, sz, [0.8, 0.8], [1.0, 0.0], 2, 2)  # own = 0 is allowed


def test_an_empty_batch_needs_no_buffers():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((0, g.m_z), dtype=torch.uint8, device=g.device)
    xh, zh, st = g.mbp4_decode(sx, sz, [0.8], [1.0], 2, 2)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)
    tab = np.array([0.8], F32)
    assert _lib.lib().fgnn_mbp4_decode(g.handle, 2, 1, tab.ctypes.data, tab.ctypes.data, 2, 2, 1, None, 2.0, None, None, 0, None, None, None,
                                       None) == 0


# ---- 15: [[882,24]] -------------------------------------------------------------------------------------------------------------------------
def test_ghp882_batch():
    """The batch of tests/test_mbp4_reference_cpu.py under the default alpha sweep: identical to the restatement, and its figures."""
    g = gpu_graph("ghp882")
    assert instantiation(g) == (3, 6)
    _, _, sx, sz = ghp882_samples()
    x0, z0, st = both("ghp882", g, sx, sz, *tables(ALPHAS), 64, 64, ref=ghp882_reference(), llr_const=llr_const(0.10))
    assert ghp882_figures(x0, z0, st) == GHP882_FIGURES and GHP882_FIGURES[0] < 7 and GHP882_FIGURES[4] == 0


# ---- 16-17: classes ---------------------------------------------------------------------------------------------------------------------------
def test_ambp4_decoder_class():
    import feedback_gnn_amd as F
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    n = og.n
    dec = F.AMBP4Decoder(c, num_iter=6, graph=gpu_graph("ibm72"))
    assert (dec.alphas, dec.num_iter, dec.cn_type, dec.factor, dec.restart) == (ALPHAS, 6, "minsum", 0.8, True)
    default = F.AMBP4Decoder(c, graph=dec.graph)
    assert default.num_iter == 64 and default.alphas == ALPHAS
    f0, o0 = tables(ALPHAS)
    assert dec.factors.tobytes() == f0.tobytes() and dec.owns.tobytes() == o0.tobytes()
    B = 40
    ex, ez, sx, sz = noisy(og, P_OF["ibm72"], B)
    llr = np.full((B, 3, n), llr_const(P_OF["ibm72"]), F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, n) and tuple(z_hat.shape) == (B, n)
    x0, z0, s0 = MB.mbp4_decode(c, sx, sz, f0, o0, 6, 6, "minsum", restart=True, llr_ch=llr)
    assert np.array_equal(x_hat.cpu().numpy(), x0) and np.array_equal(z_hat.cpu().numpy(), z0)
    assert dec.last_stats.dtype == torch.int32 and np.array_equal(dec.last_stats.cpu().numpy(), s0)
    # the alpha that solved each sample
    alpha = dec.last_alpha.cpu().numpy()
    solved = s0[:, 0] == 1
    assert alpha.dtype == F32 and alpha.shape == (B,)
    assert np.array_equal(alpha[solved], o0[s0[solved, 1]]) and np.isnan(alpha[~solved]).all()
    assert len(set(alpha[solved].tolist())) >= 2 and (~solved).any(), "more than one alpha must solve samples, and one sample stay unsolved"
    for kw in (dict(num_iter=0), dict(num_iter=2.5), dict(alphas=()), dict(alphas=(1.0,) * 65), dict(alphas=(1.0, 0.0)), dict(alphas=(1.0, -0.5)),
               dict(alphas=(float("nan"),)), dict(factor=0.0), dict(factor=float("inf")), dict(cn_type="sum-product")):
        with pytest.raises(ValueError):
            F.AMBP4Decoder(c, graph=dec.graph, **kw)
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((to_gpu(llr.astype(np.float64)), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="length n"):
        dec((to_gpu(llr[:, :, :-1].copy()), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((to_gpu(llr), to_gpu(sx.copy()), to_gpu(sz.T.copy())))


def _model(rank=0, world_size=1, p0=None):
    import feedback_gnn_amd as F
    c = code("ibm72")
    dec = F.AMBP4Decoder(c, num_iter=6, graph=gpu_graph("ibm72"))
    return F.BP4_AMBP_Model(c, dec, p0=p0, seed=SEED, rank=rank, world_size=world_size), dec


def test_bp4_ambp_model():
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    B, p = 40, P_OF["ibm72"]
    for p0 in (None, 0.05):
        model, dec = _model(p0=p0)
        for call in range(2):  # the second batch decodes global samples B .. 2B - 1
            s_hat, ls_hat = model(B, p)
            ex, ez = model.last_noise_x.cpu().numpy(), model.last_noise_z.cpu().numpy()
            xh, zh, stats = model.last_x_hat.cpu().numpy(), model.last_z_hat.cpu().numpy(), model.last_stats.cpu().numpy()
            assert tuple(s_hat.shape) == (B, hz.shape[0] + hx.shape[0]) and tuple(ls_hat.shape) == (B, hxp.shape[0] + hzp.shape[0])
            ox, oz = og.pauli_noise(SEED, p, call * B, B)
            assert np.array_equal(ex, ox) and np.array_equal(ez, oz), "depolarizing noise of the seeded stream"
            sx, sz = og.syndrome(ex, ez)
            x0, z0, s0 = MB.mbp4_decode(c, sx, sz, *tables(ALPHAS), 6, 6, llr_const=llr_const(p if p0 is None else p0))
            assert np.array_equal(xh, x0) and np.array_equal(zh, z0) and np.array_equal(stats, s0)
            assert torch.equal(dec.last_stats, model.last_stats) and dec.last_alpha is model.last_alpha
            xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
            solved = stats[:, 0] > 0
            assert solved.any() and (stats[:, 1] > 0).any()
            assert np.array_equal(s_hat.cpu().numpy(), np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1))
            assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
            assert np.array_equal(ls_hat.cpu().numpy(), np.concatenate([xd @ hxp.T % 2, zd @ hzp.T % 2], axis=1))
            assert model.last_num_unsolved == int((~solved).sum())


def test_two_ranks_decode_as_one_process():
    B = 16
    one, m0, m1 = _model()[0], _model(0, 2)[0], _model(1, 2)[0]
    one(2 * B, P_OF["ibm72"])
    assert m0.next_sample_range(B) == (0, B) and m1.next_sample_range(B) == (B, 2 * B)
    m0(B, P_OF["ibm72"]), m1(B, P_OF["ibm72"])
    for attr in ("last_noise_x", "last_noise_z", "last_x_hat", "last_z_hat", "last_stats"):
        assert torch.equal(getattr(one, attr), torch.cat([getattr(m0, attr), getattr(m1, attr)])), attr
    assert (m1.last_stats[:, 1] > 0).any(), "the second shard must reach a later alpha"


def test_sim_ber_drives_the_model():
    import feedback_gnn_amd as F
    model, _ = _model()
    flagged, bler = F.sim_ber(model, [0.12, 0.06], batch_size=64, max_mc_iter=3, verbose=False, early_stop=False, qldpc=True)
    st = F.sim_ber.last
    assert (np.asarray(st["num_blocks"]) == 64 * 3).all()
    assert len(flagged) == 2 and len(bler) == 2
    assert flagged[0] > flagged[1] >= 0 and bler[0] >= flagged[0], "every unsolved sample is flagged; more of them at the higher rate"
