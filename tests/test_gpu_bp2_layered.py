"""Binary BP in the layered (serial) schedule on the GPU (fgnn_bp2_decode_layered), held to the restatement
tests/bp2_layered_reference.py bit for bit: soft outputs, decisions and stats as bytes, no tolerance anywhere and no sample left out.
Every bp2_layered_kernel<CN_TYPE, DV, DC> is reached: the (3,6) rows (ibm72, ghp882, hp_c7), the (4,8) rows (gb48), the predicated
min-sum for degrees up to 8 (steane, rsurf5, the degenerate matrix) and up to 16 (gb126, gb46_oc), and the loop (phi and boxplus on the
irregular matrices, everything under force_generic with FGNN_BP2_NO_PRED)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import bp2_layered_reference as BR
from helpers import code, gpu_graph, oracle_library_forms, to_gpu
from test_bp2_reference_cpu import _llr_const, degenerate_hx

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
CODES = ["steane", "rsurf5", "gb48", "hp_c7", "ibm72", "ghp882", "gb126"]


def layered_lds_bytes(E_x, n, cpb, tests=False):
    """fgnn_bp2_decode_layered: E_x messages and n posteriors per codeword, each rounded up to 4 floats; with stop or stats one word
    per codeword of the workgroup, rounded up to 4 words."""
    return (((E_x + 3) & ~3) + ((n + 3) & ~3)) * 4 * cpb + (((cpb + 3) & ~3) * 4 if tests else 0)


def hx_of(name):
    return np.asarray(code(name).hx)


@functools.lru_cache(maxsize=None)
def noisy(name, p, B, first=0, seed=SEED):
    """BSC noise of the oracle's seeded stream and its syndrome under hx, computed once per case (read only)."""
    e = oracle_library_forms(name).bsc_noise(seed, p, first, B)
    return e, (e.astype(np.int64) @ hx_of(name).T.astype(np.int64) % 2).astype(np.uint8)


def channel(B, n, seed):
    """Per-bit logits: mostly 'no error' at different strengths, some on the error side, a few zeros, values beyond the +-20 clip and
    a denormal."""
    rng = np.random.RandomState(seed)
    llr = -rng.uniform(-1.5, 6.0, size=(B, n)).astype(F32)
    special = rng.rand(B, n) < 0.05
    llr[special] = rng.choice(np.array([0.0, -0.0, -20.0, -25.0, 31.0, 3.0, 1e-40], F32), size=int(special.sum()))
    return llr


def assert_same(out, ref, what=""):
    for k, got, want in zip(("soft", "hard", "stats"), out, ref):
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, k, got.dtype, got.shape)
        assert got.tobytes() == want.tobytes(), (what, k, int((got != want).sum()))


def both(g, hx, synd, T, cn_type, factor, layer_of=None, stop=False, **llr):
    """Kernel and restatement on the same inputs; asserts identical soft, hard and stats, returns the restatement's three."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    out = g.bp2_decode_layered(None if synd is None else to_gpu(synd), T, cn_type, factor, stop=stop, want_stats=True, **gl)
    ref = BR.bp2_layered_decode(hx, synd, T, cn_type, factor, layer_of=layer_of, stop=stop, **llr)
    assert_same(out, ref, (cn_type, T, factor, stop, sorted(llr)))
    return ref


@functools.lru_cache(maxsize=None)
def binary_graph(key):
    """A TannerGraph of one matrix on both sides, as decoding._binary_graph builds it."""
    from feedback_gnn_amd.decoding import _binary_graph
    return _binary_graph({"degenerate": degenerate_hx}[key](), None, None)


# ---- every code, every check rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", CODES)
def test_constant_prior(name, cn_type):
    g, hx = gpu_graph(name), hx_of(name)
    g.set_bit_layers()
    num, lay = g.bit_layers()
    num_py, lay_py = BR.greedy_bit_layers(hx)
    assert num == num_py and np.array_equal(lay, lay_py) and lay.dtype == np.int32
    _, synd = noisy(name, 0.08, 37)
    for factor, T in ((0.8, 2), (1.0, 3)):
        both(g, hx, synd, T, cn_type, factor, llr_const=_llr_const(0.08))


@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", CODES)
def test_per_bit_prior(name, cn_type):
    g, hx = gpu_graph(name), hx_of(name)
    _, synd = noisy(name, 0.08, 37)
    llr = channel(37, g.n, 7)
    for factor, T in ((0.8, 4), (1.0, 1)):
        both(g, hx, synd, T, cn_type, factor, llr_ch=llr)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_degree_one_check_and_edge_free_bit(cn_type):
    g, hx = binary_graph("degenerate"), degenerate_hx()
    rng = np.random.RandomState(9)
    B = 32
    synd = rng.randint(0, 2, size=(B, hx.shape[0])).astype(np.uint8)
    for factor in (0.8, 1.0):
        both(g, hx, synd, 3, cn_type, factor, llr_const=_llr_const(0.1))  # the first call installs the greedy layering
        s, _, _ = both(g, hx, synd, 3, cn_type, factor, llr_ch=channel(B, 12, 6), stop=True)
    assert g.bit_layers()[1].tolist() == [0, 0, 1, 2, 2, 0, 3]
    s, _, _ = both(g, hx, synd, 2, cn_type, 0.8, llr_const=-1.5)
    assert (s[:, 11] == F32(-1.5)).all()  # the edge-free bit keeps its channel logit


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_many_layers_and_heavy_bits(cn_type):
    """hx of gb46_oc (over-complete checks): 190 layers of 1 to 3 checks, up to 94 checks at a bit, one codeword per workgroup."""
    g, hx = gpu_graph("gb46_oc"), hx_of("gb46_oc")
    assert g.info()["codewords_per_block"] == 1
    g.set_bit_layers()
    assert g.bit_layers()[0] == 190 and int(hx.sum(0).max()) == 94
    _, synd = noisy("gb46_oc", 0.08, 5)
    both(g, hx, synd, 2, cn_type, 0.8, llr_const=_llr_const(0.08))
    both(g, hx, synd, 2, cn_type, 1.0, llr_ch=channel(5, g.n, 2), stop=True)


# ---- stop --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch(name, count):
    """`count` samples of a pool of 96 at p = 0.06 chosen from the restatement's stats under stop (min-sum, factor 0.8, 6 iterations):
    first one sample of every (outcome, iteration count) met, those that never stop leading, then the pool in order."""
    hx = hx_of(name)
    _, synd = noisy(name, 0.06, 96, first=7)
    _, _, st = BR.bp2_layered_decode(hx, synd, 6, "minsum", 0.8, llr_const=_llr_const(0.06), stop=True)
    seen, first, rest = set(), [], []
    for b in range(96):
        (rest if tuple(st[b]) in seen else first).append(b)
        seen.add(tuple(st[b]))
    first.sort(key=lambda b: (st[b, 0], st[b, 1]))
    pick = (first + rest)[:count]
    return synd[pick]


@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_stop_with_several_codewords_per_workgroup(name):
    g, hx = gpu_graph(name), hx_of(name)
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    synd = mixed_batch(name, cpb + 1)
    L = _llr_const(0.06)
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, st = both(g, hx, synd[:B], 6, "minsum", 0.8, llr_const=L, stop=True)
        # samples of one workgroup stop at different iterations and some never do
        assert len(set(st[st[:, 0] == 1, 1].tolist())) >= 2 and ((st[:, 0] == 0) & (st[:, 1] == 6)).any(), st.tolist()
        both(g, hx, synd[:B], 6, "boxplus-phi", 1.0, llr_ch=channel(B, g.n, 3), stop=True)
        _, _, st = both(g, hx, synd[:B], 3, "minsum", 0.8, llr_const=L)
        assert (st[:, 1] == 3).all()  # stop off: it_run = num_iter, one test after the last iteration
        _, hard, st = both(g, hx, synd[:B], 0, "minsum", 0.8, llr_const=L, stop=True)
        assert (st[:, 1] == 0).all() and not hard.any() and np.array_equal(st[:, 0] == 1, ~synd[:B].any(1))  # the prior's decision


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_stop_with_one_codeword_per_workgroup(cn_type):
    """[[882,24]]: a workgroup leaves the loop with its codeword."""
    g, hx = gpu_graph("ghp882"), hx_of("ghp882")
    _, synd = noisy("ghp882", 0.04, 24, seed=1234)
    _, _, st = both(g, hx, synd, 6, cn_type, 0.8, llr_const=_llr_const(0.04), stop=True)
    assert len(set(st[:, 1].tolist())) >= 2


# ---- launch geometry, forced kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tpc,cpb", [(64, 1), (256, 1), (64, 3), (32, 2), (4, 16), (8, 8)])
def test_set_launch_geometries(tpc, cpb):
    """hx of ibm72 has 4 layers of 9 checks: thread counts below (4, 8) and above a layer's size, and (32, 2)."""
    g, hx = gpu_graph("ibm72"), hx_of("ibm72")
    g.set_launch(tpc, cpb)
    try:
        _, synd = noisy("ibm72", 0.08, 37)
        B = 2 * cpb + 1
        both(g, hx, synd[:B], 2, "minsum", 0.8, llr_const=_llr_const(0.08))
        both(g, hx, synd[:B], 3, "boxplus-phi", 0.8, llr_ch=channel(B, g.n, 4), stop=True)
        both(g, hx, synd[:B], 2, "boxplus", 1.0, llr_ch=channel(B, g.n, 4))
    finally:
        g.set_launch(0, 0)


@pytest.mark.parametrize("no_pred", [False, True])
@pytest.mark.parametrize("name", ["ibm72", "gb48", "gb126"])
def test_force_generic(name, no_pred):
    """The regular matrices on the runtime-degree kernels: min-sum predicated (degrees up to 8 / 16), and on the loop under
    FGNN_BP2_NO_PRED; phi on the loop."""
    g, hx = gpu_graph(name), hx_of(name)
    _, synd = noisy(name, 0.08, 37)
    g.force_generic(True)
    if no_pred:
        os.environ["FGNN_BP2_NO_PRED"] = "1"
    try:
        both(g, hx, synd[:9], 3, "minsum", 0.8, llr_ch=channel(9, g.n, 5), stop=True)
        both(g, hx, synd[:9], 2, "boxplus-phi", 1.0, llr_const=_llr_const(0.08))
    finally:
        os.environ.pop("FGNN_BP2_NO_PRED", None)
        g.force_generic(False)


# ---- layerings ---------------------------------------------------------------------------------------------------------------------------
def test_a_callers_layering():
    g, hx = gpu_graph("gb48"), hx_of("gb48")
    m = hx.shape[0]
    reverse = np.arange(m - 1, -1, -1).astype(np.int32)  # one check per layer, the last check first
    _, synd = noisy("gb48", 0.08, 37)
    L = _llr_const(0.08)
    try:
        g.set_bit_layers(reverse)
        num, lay = g.bit_layers()
        assert num == m and np.array_equal(lay, reverse) and lay.dtype == np.int32
        mine = both(g, hx, synd, 2, "minsum", 0.8, layer_of=reverse, llr_const=L)
        g.set_bit_layers()
        assert g.bit_layers()[0] == BR.greedy_bit_layers(hx)[0] < m
        greedy = both(g, hx, synd, 2, "minsum", 0.8, llr_const=L)
        assert mine[0].tobytes() != greedy[0].tobytes()
    finally:
        g.set_bit_layers()


def test_set_bit_layers_refuses_and_keeps_the_installed_layering():
    g, hx = gpu_graph("steane"), hx_of("steane")
    g.set_bit_layers()
    before = g.bit_layers()
    assert before[0] == 3
    v = int(np.nonzero(hx[0] & hx[1])[0][0])
    with pytest.raises(ValueError, match=rf"check 0 and check 1 of layer 0 share bit {v}"):
        g.set_bit_layers([0, 0, 1])
    with pytest.raises(ValueError, match="layer 2 is empty"):
        g.set_bit_layers([0, 1, 3])
    with pytest.raises(ValueError, match=r"check 1 has layer -1, outside \[0, 3\)"):
        g.set_bit_layers([0, -1, 2])
    with pytest.raises(ValueError, match="shape"):
        g.set_bit_layers([0, 1, 2, 3, 4, 5])
    after = g.bit_layers()
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    try:
        g.set_bit_layers([2, 1, 0])
        assert g.bit_layers()[1].tolist() == [2, 1, 0]
    finally:
        g.set_bit_layers()
    assert g.bit_layers()[1].tolist() == [0, 1, 2]


# ---- the other decoders next to it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_other_decoders_are_untouched_by_a_bit_layering(name):
    from helpers import llr_const as llr4
    g, hx = gpu_graph(name), hx_of(name)
    _, synd = noisy(name, 0.08, 37)
    sz = torch.zeros((37, g.m_z), dtype=torch.uint8, device=g.device)
    s = to_gpu(synd)
    L = _llr_const(0.08)
    gamma = to_gpu(np.random.RandomState(1).uniform(-0.2, 0.6, size=(3, g.n)).astype(F32))
    g.set_layers()
    bp4_layers = g.layers()

    def others():
        flo = g.bp2_decode(s, 3, "minsum", 0.8, llr_const=L)
        rel = g.relay_decode(s, gamma, 4, 3, 1, 0.8, llr_const=L)
        lay4 = g.bp4_decode_layered(s, sz, 2, "minsum", 0.8, llr_const=llr4(0.08), return_msgs=True)
        return list(flo) + list(rel) + [lay4[k] for k in ("llr", "x_hat", "z_hat", "msg_x", "msg_z")]

    before = others()
    m = hx.shape[0]
    try:
        g.set_bit_layers(np.arange(m - 1, -1, -1).astype(np.int32))
        assert g.layers()[0] == bp4_layers[0] and np.array_equal(g.layers()[1], bp4_layers[1])  # the BP4 layering stays
        layered = g.bp2_decode_layered(s, 3, "minsum", 0.8, llr_const=L)
        for a, b in zip(before, others()):
            assert torch.equal(a, b)
        g.set_layers(np.arange(g.m_x + g.m_z, dtype=np.int32))  # and a BP4 layering leaves the bit layering alone
        assert g.bit_layers()[0] == m
    finally:
        g.set_bit_layers()
        g.set_layers()
    for a, b in zip(before, others()):
        assert torch.equal(a, b)
    assert not torch.equal(layered[0], before[0]), "the two schedules are different decoders"
    og = oracle_library_forms(name)
    so, ho = og.bp2_decode(synd, 3, "minsum", 0.8, llr_const=L)
    assert before[0].cpu().numpy().tobytes() == so.tobytes() and np.array_equal(before[1].cpu().numpy(), ho)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_zero_iterations_are_bp2_decode_at_zero(cn_type):
    g, hx = gpu_graph("hp_c7"), hx_of("hp_c7")
    _, synd = noisy("hp_c7", 0.08, 37)
    s = to_gpu(synd)
    llr = channel(37, g.n, 11)
    for kw in (dict(llr_const=_llr_const(0.08)), dict(llr_const=0.0), dict(llr_ch=to_gpu(llr))):
        a = g.bp2_decode_layered(s, 0, cn_type, 0.8, **kw)
        b = g.bp2_decode(s, 0, cn_type, 0.8, **kw)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    both(g, hx, synd, 0, cn_type, 0.8, llr_ch=llr)


def test_null_syndrome_and_null_llr_through_ctypes():
    from feedback_gnn_amd import _lib
    g, hx = gpu_graph("ibm72"), hx_of("ibm72")
    B, n = 5, g.n
    llr = channel(B, n, 2)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    for llr_ch, llr_const, synd in ((llr, 0.0, None), (None, -1.25, noisy("ibm72", 0.08, 37)[1][:B]), (None, 2.5, None)):
        soft = torch.empty((B, n), dtype=torch.float32, device=g.device)
        hard = torch.empty((B, n), dtype=torch.uint8, device=g.device)
        stats = torch.empty((B, 2), dtype=torch.int32, device=g.device)
        dl = None if llr_ch is None else to_gpu(llr_ch)
        ds = None if synd is None else to_gpu(synd)
        _lib.check(_lib.lib().fgnn_bp2_decode_layered(g.handle, 2, 2, 0.8, None if dl is None else p(dl), llr_const, None if ds is None else p(ds), B, 1, p(soft), p(hard),
                                                      p(stats), st))
        kw = dict(llr_const=llr_const) if llr_ch is None else dict(llr_ch=llr_ch)
        ref = BR.bp2_layered_decode(hx, np.zeros((B, g.m_x), np.uint8) if synd is None else synd, 2, "minsum", 0.8, stop=True, **kw)
        assert_same((soft, hard, stats), ref)


def test_outputs_wanted_and_the_empty_batch():
    g = gpu_graph("ibm72")
    _, synd = noisy("ibm72", 0.08, 37)
    s = to_gpu(synd)
    soft, hard, stats = g.bp2_decode_layered(s, 2, "minsum", 0.8, llr_const=-2.0, want_stats=True)
    only_soft = g.bp2_decode_layered(s, 2, "minsum", 0.8, llr_const=-2.0, want_hard=False)
    only_hard = g.bp2_decode_layered(s, 2, "minsum", 0.8, llr_const=-2.0, want_soft=False, want_stats=True)
    assert only_soft[1] is None and torch.equal(only_soft[0], soft)
    assert only_hard[0] is None and torch.equal(only_hard[1], hard) and torch.equal(only_hard[2], stats)
    with pytest.raises(ValueError, match="no output buffer"):
        g.bp2_decode_layered(s, 2, "minsum", 0.8, want_soft=False, want_hard=False)
    empty = torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device)
    soft, hard, stats = g.bp2_decode_layered(empty, 3, "minsum", 0.8, llr_const=2.0, stop=True, want_stats=True)
    assert tuple(soft.shape) == (0, g.n) and tuple(hard.shape) == (0, g.n) and tuple(stats.shape) == (0, 2)
    assert g.bp2_decode_layered(empty, 3, "minsum", 0.8, want_soft=False, want_hard=False) == (None, None)  # an empty batch needs no buffers


def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    s = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.bp2_decode_layered(s, 2, "sum-product")
    with pytest.raises(ValueError, match=">= 0"):
        g.bp2_decode_layered(s, -1, "minsum")
    with pytest.raises(ValueError, match="syndrome"):
        g.bp2_decode_layered(s[:, :-1].contiguous(), 2, "minsum")
    with pytest.raises(ValueError, match="llr_ch"):
        g.bp2_decode_layered(s, 2, "minsum", llr_ch=torch.zeros((2, 3, g.n), dtype=torch.float32, device=g.device))
    soft = torch.empty((2, g.n), dtype=torch.float32, device=g.device)
    rc = _lib.lib().fgnn_bp2_decode_layered(g.handle, 2, 2, 0.8, None, 0.0, None, 2, 2, ctypes.c_void_p(soft.data_ptr()), None, None, None)
    assert rc == -1 and b"stop must be 0 or 1" in _lib.lib().fgnn_last_error()


# ---- LDS ---------------------------------------------------------------------------------------------------------------------------------
LDS_N = 4000
LDS_E = LDS_BUDGET // 4 - LDS_N  # E_x + n floats exactly at FGNN_LDS_BUDGET: both are multiples of 4


@functools.lru_cache(maxsize=None)
def lds_graph(extra):
    """hx with LDS_E + extra edges on LDS_N bits (and a thin hz), built as test_gpu_bp4_shapes.graphs builds its cases."""
    from feedback_gnn_amd.graph import TannerGraph
    from test_gpu_bp4_shapes import sparse_bare
    c = sparse_bare(LDS_N, LDS_E + extra, LDS_N, 9)()
    return TannerGraph(c), np.asarray(c.hx)


def test_the_lds_budget():
    """A graph whose E_x + n floats fill the LDS budget to the byte decodes (the parity words of stop / stats take 16 bytes more, and
    are then refused); one edge more, which rounds up to four floats, is refused: there is no global-memory variant."""
    g, hx = lds_graph(0)
    assert g.info()["codewords_per_block"] == 1 and layered_lds_bytes(g.E_x, g.n, 1) == LDS_BUDGET
    rng = np.random.RandomState(1)
    synd = rng.randint(0, 2, size=(2, g.m_x)).astype(np.uint8)
    llr = channel(2, g.n, 5)
    soft, hard = g.bp2_decode_layered(to_gpu(synd), 1, "minsum", 0.8, llr_ch=to_gpu(llr))
    ref = BR.bp2_layered_decode(hx, synd, 1, "minsum", 0.8, llr_ch=llr)
    assert_same((soft, hard), ref[:2])
    with pytest.raises(ValueError, match=rf"LDS.*{LDS_BUDGET + 16} bytes.*limit is {LDS_BUDGET}"):
        g.bp2_decode_layered(to_gpu(synd), 1, "minsum", 0.8, llr_ch=to_gpu(llr), want_stats=True)
    big = lds_graph(1)[0]
    need = layered_lds_bytes(big.E_x, big.n, 1)
    assert need == LDS_BUDGET + 16
    s = torch.zeros((2, big.m_x), dtype=torch.uint8, device=big.device)
    with pytest.raises(ValueError, match=rf"LDS.*{need} bytes.*limit is {LDS_BUDGET}"):
        big.bp2_decode_layered(s, 2, "minsum", 0.8, llr_const=2.0)


# ---- classes -----------------------------------------------------------------------------------------------------------------------------
def test_decoder_class_routes_the_layered_schedule():
    import feedback_gnn_amd as F
    hx = hx_of("ibm72")
    B, n = 23, hx.shape[1]
    synd = noisy("ibm72", 0.08, 37)[1][:B]
    llr = channel(B, n, 8)
    dec = F.LDPCBPDecoder(hx, cn_type="minsum", num_iter=3, normalization_factor=0.8, is_syndrome=True, hard_out=False, schedule="layered")
    assert dec.schedule == "layered" and dec.stop_early is False and dec.graph.bit_layers()[0] == 4
    assert F.LDPCBPDecoder(hx, is_syndrome=True, graph=dec.graph).schedule == "flooding"
    got = dec((to_gpu(llr), to_gpu(synd.T.copy())))
    ref = BR.bp2_layered_decode(hx, synd, 3, "minsum", 0.8, llr_ch=llr)
    assert got.dtype == torch.float32 and got.cpu().numpy().tobytes() == ref[0].tobytes()
    flooding = F.LDPCBPDecoder(hx, cn_type="minsum", num_iter=3, normalization_factor=0.8, is_syndrome=True, hard_out=False, graph=dec.graph)
    assert not torch.equal(flooding((to_gpu(llr), to_gpu(synd.T.copy()))), got)
    # hard output with stop_early, without a syndrome (ordinary decoding), and a layering given to the constructor
    own = np.arange(hx.shape[0], dtype=np.int32)[::-1].copy()
    hard = F.LDPCBPDecoder(hx, cn_type="boxplus-phi", num_iter=4, schedule="layered", layers=own, stop_early=True)
    assert np.array_equal(hard.graph.bit_layers()[1], own) and hard.stop_early is True
    out = hard(to_gpu(llr))
    ref = BR.bp2_layered_decode(hx, None, 4, "boxplus-phi", 1.0, llr_ch=llr, layer_of=own, stop=True)
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), ref[1].astype(F32))


def test_schedule_errors():
    import feedback_gnn_amd as F
    hx = hx_of("ibm72")
    g = gpu_graph("ibm72")
    for bad in ("serial", "Layered", None, 1):
        with pytest.raises(ValueError, match="schedule"):
            F.LDPCBPDecoder(hx, graph=g, schedule=bad)
    with pytest.raises(ValueError, match="layers="):
        F.LDPCBPDecoder(hx, graph=g, layers=np.zeros(g.m_x, np.int32))
    with pytest.raises(ValueError, match="stop_early"):
        F.LDPCBPDecoder(hx, graph=g, stop_early=True)
    with pytest.raises(ValueError, match="share bit"):
        F.LDPCBPDecoder(hx, schedule="layered", layers=np.zeros(g.m_x, np.int32))


@pytest.mark.parametrize("model", ["osd", "lsd", "bsc"])
def test_models_dispatch_on_the_schedule(model):
    """The pinned batch of tests/test_bp2_layered_reference_cpu.py (hx of [[882,24]], p = 0.04, seed 1234, min-sum 0.8, 8 iterations):
    a layered decoder hands 1 sample to the post-processor, a flooding one 18; where BP reproduced the syndrome the model's logical
    residual is that of the restatement's decision, and the post-processed samples reproduce theirs by construction."""
    import feedback_gnn_amd as F
    c = code("ghp882")
    hx, lx = hx_of("ghp882"), np.asarray(c.lx).astype(np.int64)
    e, synd = noisy("ghp882", 0.04, 64, seed=1234)
    L = _llr_const(0.04)
    refs = dict(layered=BR.bp2_layered_decode(hx, synd, 8, "minsum", 0.8, llr_const=L)[1],
                flooding=oracle_library_forms("ghp882").bp2_decode(synd, 8, "minsum", 0.8, llr_const=L)[1])
    handed = {}
    for tag in ("layered", "flooding"):
        kw = dict(schedule="layered") if tag == "layered" else {}
        bp2 = F.LDPCBPDecoder(c.hx, is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=8, normalization_factor=0.8, **kw)
        if model == "osd":
            m = F.BP2_OSD_Model(c.hx, c.hx_basis, c.pivot_hx, c.lx, bp2, F.OSD0_Decoder(c.N), seed=1234)
        elif model == "lsd":
            m = F.BP2_LSD_Model(c.hx, c.lx, bp2, F.LSD_Decoder(c.N), seed=1234)
        else:
            m = F.BP_BSC_Model(c.hx, bp2, c.lx, seed=1234)
        out = m(64, 0.04)
        ls_hat = out[1].cpu().numpy()
        solved = BR.parity_ok(hx, refs[tag], synd)
        want = ((e ^ refs[tag]).astype(np.int64) @ lx.T % 2).astype(np.uint8)
        if model == "bsc":
            assert np.array_equal(ls_hat, want)  # no post-processor: every row is BP's
            assert np.array_equal(out[0].cpu().numpy().any(1), ~solved)
            handed[tag] = int((~solved).sum())
        else:
            assert np.array_equal(ls_hat[solved], want[solved])
            handed[tag] = m.last_num_osd if model == "osd" else m.last_num_lsd
            assert handed[tag] == int((~solved).sum())
    assert handed == {"layered": 1, "flooding": 18}
