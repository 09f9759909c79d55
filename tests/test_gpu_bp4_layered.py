"""BP4 in the layered (serial) schedule on the GPU (fgnn_bp4_decode_layered), held to the restatement tests/layered_reference.py bit for
bit: marginals, decisions, both soft syndromes and the final messages as bytes, no tolerance anywhere and no sample left out.  The
restatement's steps are the CPU oracle's flooding iterations (the float operations the BP4 kernels are held to) with NumPy selecting
which messages a layer keeps, so nothing depends on a reduction order.  Iteration counts are 1 to 4: a restated iteration costs one
oracle call per layer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import layered_reference as LR
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
CODES = ["steane", "rsurf5", "gb48", "hp_c7", "ibm72", "ghp882"]
KEYS = ("llr", "x_hat", "z_hat", "x_logit", "z_logit", "msg_x", "msg_z")


def layered_lds_bytes(E, n, cpb):
    """fgnn_bp4_decode_layered: E messages and 3n channel / binary LLRs per codeword, each rounded up to 4 floats."""
    return (((E + 3) & ~3) + ((3 * n + 3) & ~3)) * 4 * cpb


@functools.lru_cache(maxsize=None)
def noisy(name, p, B, first=0):
    """Depolarizing noise of the oracle's seeded stream and its syndromes: (synd_x, synd_z), computed once per case (read only)."""
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, p, first, B)
    sx, sz = og.syndrome(ex, ez)
    return sx, sz


def channel(B, n, seed):
    """Per-qubit channel LLRs: mostly 'no error' at different strengths, some negative, a few zeros and values beyond the min-sum clip."""
    rng = np.random.RandomState(seed)
    llr = rng.uniform(-1.5, 6.0, size=(B, 3, n)).astype(F32)
    special = rng.rand(B, 3, n) < 0.05
    llr[special] = rng.choice(np.array([0.0, 20.0, 25.0, -3.0, 1e-40], F32), size=int(special.sum()))
    return llr


def assert_same(out, ref, what=""):
    for k in KEYS:
        got = out[k].cpu().numpy()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (what, k)
        assert got.tobytes() == ref[k].tobytes(), (what, k, int((got != ref[k]).sum()))


def both(g, og, sx, sz, T, cn_type, factor, layer_of=None, msg_init=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns (kernel's dict, restatement's dict)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    mi = None if msg_init is None else (to_gpu(msg_init[0]), to_gpu(msg_init[1]))
    out = g.bp4_decode_layered(to_gpu(sx), to_gpu(sz), T, cn_type, factor, msg_init=mi, return_msgs=True, **gl)
    ref = LR.layered_decode(og, sx, sz, T, cn_type, factor, layer_of=layer_of, msg_init=msg_init, **llr)
    assert_same(out, ref, (cn_type, T, factor, sorted(llr)))
    return out, ref


# ---- every code, every check rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", CODES)
def test_constant_prior(name, cn_type):
    g, og = gpu_graph(name), oracle_library_forms(name)
    g.set_layers()
    num, lay = g.layers()
    num_py, lay_py = LR.greedy_layers(og.code.hx, og.code.hz)
    assert num == num_py and np.array_equal(lay, lay_py)
    sx, sz = noisy(name, 0.08, 37)
    for factor, T in ((0.8, 2), (1.0, 3)):
        both(g, og, sx, sz, T, cn_type, factor, llr_const=llr_const(0.08))


@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", CODES)
def test_per_qubit_prior(name, cn_type):
    g, og = gpu_graph(name), oracle_library_forms(name)
    sx, sz = noisy(name, 0.08, 37)
    llr = channel(37, og.n, 7)
    for factor, T in ((0.8, 4), (1.0, 1)):
        both(g, og, sx, sz, T, cn_type, factor, llr_ch=llr)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_bare_code_with_degree_one_checks_and_edge_free_qubits(cn_type):
    """hx with a degree-1 and a degree-2 check; qubits 0-3 have no hz edge and qubit 11 has no hx edge (tests/test_bp4_reference_cpu.py)."""
    from feedback_gnn_amd.graph import TannerGraph
    from oracle.oracle import OracleGraph
    from test_bp4_reference_cpu import bare_code
    c = bare_code()
    g, og = TannerGraph(c), OracleGraph(c, forms="literal")
    assert g.layers() == (0, None)
    rng = np.random.RandomState(9)
    B = 32
    sx = rng.randint(0, 2, size=(B, 7)).astype(np.uint8)
    sz = rng.randint(0, 2, size=(B, 5)).astype(np.uint8)
    for factor in (0.8, 1.0):
        both(g, og, sx, sz, 3, cn_type, factor, llr_const=llr_const(0.1))  # the first call installs the greedy layering
        both(g, og, sx, sz, 3, cn_type, factor, llr_ch=channel(B, 12, 6))
    num, lay = g.layers()
    assert num == LR.greedy_layers(c.hx, c.hz)[0] and LR.is_valid_layering(c.hx, c.hz, num, lay)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_many_layers_and_heavy_qubits(cn_type):
    """gb46_oc (over-complete checks): 329 layers, up to 176 checks at a qubit, one codeword per workgroup."""
    g, og = gpu_graph("gb46_oc"), oracle_library_forms("gb46_oc")
    assert g.info()["codewords_per_block"] == 1
    g.set_layers()
    assert g.layers()[0] == 329 and int((np.asarray(og.code.hx).sum(0) + np.asarray(og.code.hz).sum(0)).max()) == 176
    sx, sz = noisy("gb46_oc", 0.08, 5)
    both(g, og, sx, sz, 2, cn_type, 0.8, llr_const=llr_const(0.08))


# ---- launch geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rsurf5", "steane"])
def test_several_codewords_per_workgroup(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    for B in (1, cpb - 1, cpb, cpb + 1):
        sx, sz = noisy(name, 0.08, cpb + 1)
        both(g, og, sx[:B], sz[:B], 2, "minsum", 0.8, llr_const=llr_const(0.08))
        both(g, og, sx[:B], sz[:B], 2, "boxplus-phi", 1.0, llr_ch=channel(B, og.n, 3))


@pytest.mark.parametrize("tpc,cpb", [(64, 1), (256, 1), (64, 3), (32, 2)])
def test_set_launch_geometries(tpc, cpb):
    """ibm72's layers hold 9 checks and 54 edges: fewer than any of these thread counts, and (32, 2) deals a thread two edges."""
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    g.set_launch(tpc, cpb)
    try:
        sx, sz = noisy("ibm72", 0.08, 37)
        B = 2 * cpb + 1
        both(g, og, sx[:B], sz[:B], 2, "minsum", 0.8, llr_const=llr_const(0.08))
        both(g, og, sx[:B], sz[:B], 2, "boxplus", 0.8, llr_ch=channel(B, og.n, 4))
    finally:
        g.set_launch(0, 0)


# ---- layerings ---------------------------------------------------------------------------------------------------------------------------
def test_a_callers_layering():
    g, og = gpu_graph("gb48"), oracle_library_forms("gb48")
    m = og.m_x + og.m_z
    reverse = np.arange(m - 1, -1, -1).astype(np.int32)  # one check per layer, the last check first
    sx, sz = noisy("gb48", 0.08, 37)
    L = llr_const(0.08)
    try:
        g.set_layers(reverse)
        num, lay = g.layers()
        assert num == m and np.array_equal(lay, reverse) and lay.dtype == np.int32
        _, mine = both(g, og, sx, sz, 2, "minsum", 0.8, layer_of=reverse, llr_const=L)
        g.set_layers()
        assert g.layers()[0] == LR.greedy_layers(og.code.hx, og.code.hz)[0] < m
        _, greedy = both(g, og, sx, sz, 2, "minsum", 0.8, llr_const=L)
        assert mine["msg_x"].tobytes() != greedy["msg_x"].tobytes() and mine["llr"].tobytes() != greedy["llr"].tobytes()
    finally:
        g.set_layers()


def test_set_layers_refuses_and_keeps_the_installed_layering():
    g = gpu_graph("steane")
    hx, hz = np.asarray(code("steane").hx), np.asarray(code("steane").hz)
    g.set_layers()
    before = g.layers()
    assert before[0] == 6
    v = int(np.nonzero(hx[0] & hz[0])[0][0])
    with pytest.raises(ValueError, match=rf"hx check 0 and hz check 0 \(number 3\) of layer 0 share qubit {v}"):
        g.set_layers([0, 1, 2, 0, 3, 4])
    with pytest.raises(ValueError, match="layer 5 is empty"):
        g.set_layers([0, 1, 2, 3, 4, 6])
    with pytest.raises(ValueError, match=r"hx check 1 has layer -1, outside \[0, 6\)"):
        g.set_layers([0, -1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="shape"):
        g.set_layers([0, 1, 2, 3, 4])
    after = g.layers()
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    g.set_layers([5, 4, 3, 2, 1, 0])
    assert g.layers()[1].tolist() == [5, 4, 3, 2, 1, 0]
    g.set_layers()
    assert g.layers()[1].tolist() == [0, 1, 2, 3, 4, 5]


# ---- chaining, zero iterations, the flooding decoder next to it --------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_chaining_and_zero_iterations(cn_type):
    g, og = gpu_graph("hp_c7"), oracle_library_forms("hp_c7")
    sx, sz = noisy("hp_c7", 0.08, 37)
    gx, gz = to_gpu(sx), to_gpu(sz)
    llr = channel(37, og.n, 11)
    for kw in (dict(llr_const=llr_const(0.08)), dict(llr_ch=to_gpu(llr))):
        one = g.bp4_decode_layered(gx, gz, 1, cn_type, 0.8, return_msgs=True, **kw)
        two = g.bp4_decode_layered(gx, gz, 1, cn_type, 0.8, msg_init=(one["msg_x"], one["msg_z"]), return_msgs=True, **kw)
        whole = g.bp4_decode_layered(gx, gz, 2, cn_type, 0.8, return_msgs=True, **kw)
        for k in KEYS:
            assert torch.equal(two[k], whole[k]), k
        assert not torch.equal(one["msg_x"], whole["msg_x"])
        # zero iterations: the flooding entry point's epilogue, on zero messages and on given ones
        for mi in (None, (one["msg_x"], one["msg_z"])):
            a = g.bp4_decode_layered(gx, gz, 0, cn_type, 0.8, msg_init=mi, return_msgs=True, **kw)
            b = g.bp4_decode(gx, gz, 0, cn_type, 0.8, msg_init=mi, return_msgs=True, **kw)
            for k in KEYS:
                assert torch.equal(a[k], b[k]), k
    ref0 = og.bp4_decode(sx, sz, 0, cn_type, 0.8, llr_ch=llr, return_msgs=True)
    assert_same(g.bp4_decode_layered(gx, gz, 0, cn_type, 0.8, llr_ch=to_gpu(llr), return_msgs=True), ref0)
    # only the soft syndromes or only the messages, or neither
    bare = g.bp4_decode_layered(gx, gz, 2, cn_type, 0.8, llr_const=llr_const(0.08), want_logits=False)
    assert bare["x_logit"] is None and torch.equal(bare["llr"], g.bp4_decode_layered(gx, gz, 2, cn_type, 0.8, llr_const=llr_const(0.08))["llr"])


@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_flooding_decode_is_untouched_by_a_layering(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    sx, sz = noisy(name, 0.08, 37)
    g.set_layers()
    layered = g.bp4_decode_layered(to_gpu(sx), to_gpu(sz), 3, "boxplus-phi", 1.0, llr_const=llr_const(0.08), return_msgs=True)
    for cn_type, factor in (("boxplus-phi", 1.0), ("minsum", 0.8)):
        out = g.bp4_decode(to_gpu(sx), to_gpu(sz), 3, cn_type, factor, llr_const=llr_const(0.08), return_msgs=True)
        assert_same(out, og.bp4_decode(sx, sz, 3, cn_type, factor, llr_const=llr_const(0.08), return_msgs=True))
    flooding = g.bp4_decode(to_gpu(sx), to_gpu(sz), 3, "boxplus-phi", 1.0, llr_const=llr_const(0.08), return_msgs=True)
    assert not torch.equal(layered["msg_x"], flooding["msg_x"]), "the two schedules are different decoders"


def test_null_syndromes_are_zero_syndromes():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    B, n = 5, g.n
    zx = torch.zeros((B, g.m_x), dtype=torch.uint8, device=g.device)
    zz = torch.zeros((B, g.m_z), dtype=torch.uint8, device=g.device)
    llr = to_gpu(channel(B, n, 2))
    want = g.bp4_decode_layered(zx, zz, 2, "minsum", 0.8, llr_ch=llr, want_logits=False)
    out = torch.empty((B, 3, n), dtype=torch.float32, device=g.device)
    xh = torch.empty((B, n), dtype=torch.uint8, device=g.device)
    zh = torch.empty((B, n), dtype=torch.uint8, device=g.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    _lib.check(_lib.lib().fgnn_bp4_decode_layered(g.handle, 2, 2, 0.8, p(llr), 0.0, None, None, B, None, None, p(out), p(xh), p(zh),
                                                  None, None, None, None, st))
    assert torch.equal(out, want["llr"]) and torch.equal(xh, want["x_hat"]) and torch.equal(zh, want["z_hat"])


def test_empty_batch():
    g = gpu_graph("ibm72")
    sx = torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((0, g.m_z), dtype=torch.uint8, device=g.device)
    out = g.bp4_decode_layered(sx, sz, 3, "minsum", 0.8, llr_const=2.0, return_msgs=True)
    assert tuple(out["llr"].shape) == (0, 3, g.n) and tuple(out["x_hat"].shape) == (0, g.n) and tuple(out["msg_z"].shape) == (0, g.E_z)


# ---- LDS ---------------------------------------------------------------------------------------------------------------------------------
def test_the_lds_budget():
    """A graph whose E + 3n floats fill the LDS budget to the byte decodes; one edge more is refused, and so is the [[6480,1296]]
    hypergraph product: there is no global-memory variant."""
    from test_gpu_bp4_shapes import graphs
    g, og, _ = graphs("lds_at")
    assert layered_lds_bytes(g.E_x + g.E_z, g.n, 1) == LDS_BUDGET
    rng = np.random.RandomState(1)
    sx = rng.randint(0, 2, size=(2, g.m_x)).astype(np.uint8)
    sz = rng.randint(0, 2, size=(2, g.m_z)).astype(np.uint8)
    both(g, og, sx, sz, 1, "minsum", 0.8, llr_ch=channel(2, g.n, 5))
    for big in (graphs("lds_over")[0], gpu_graph("hp_big")):
        need = layered_lds_bytes(big.E_x + big.E_z, big.n, 1)
        assert need > LDS_BUDGET
        sx = torch.zeros((2, big.m_x), dtype=torch.uint8, device=big.device)
        sz = torch.zeros((2, big.m_z), dtype=torch.uint8, device=big.device)
        with pytest.raises(ValueError, match=rf"LDS.*{need} bytes.*limit is {LDS_BUDGET}"):
            big.bp4_decode_layered(sx, sz, 2, "minsum", 0.8, llr_const=2.0)


def test_argument_errors():
    g = gpu_graph("ibm72")
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.bp4_decode_layered(sx, sz, 2, "sum-product")
    with pytest.raises(ValueError, match=">= 0"):
        g.bp4_decode_layered(sx, sz, -1, "minsum")
    with pytest.raises(ValueError, match="synd_x"):
        g.bp4_decode_layered(sx[:, :-1].contiguous(), sz, 2, "minsum")
    with pytest.raises(ValueError, match="llr_ch"):
        g.bp4_decode_layered(sx, sz, 2, "minsum", llr_ch=torch.zeros((2, g.n), dtype=torch.float32, device=g.device))


# ---- classes -----------------------------------------------------------------------------------------------------------------------------
def test_decoder_class_routes_the_layered_schedule():
    import feedback_gnn_amd as F
    c = code("ibm72")
    g = gpu_graph("ibm72")
    og = oracle_library_forms("ibm72")
    B, n = 23, og.n
    sx, sz = noisy("ibm72", 0.08, 37)
    sx, sz = sx[:B], sz[:B]
    llr = channel(B, n, 8)
    dec = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=3, normalization_factor=0.8, stage_one=True, schedule="layered", graph=g)
    assert dec.schedule == "layered" and g.layers()[0] == 8
    assert F.QLDPCBPDecoder(c, stage_one=True, graph=g).schedule == "flooding"
    got = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    want = g.bp4_decode_layered(to_gpu(sx), to_gpu(sz), 3, "minsum", 0.8, llr_ch=to_gpu(llr))
    assert len(got) == 7
    for i in range(3):
        assert torch.equal(got[i], want["llr"][:, i, :])
    assert got[3].dtype == torch.int64 and got[4].dtype == torch.float64
    assert torch.equal(got[3], want["x_hat"].to(torch.int64)) and torch.equal(got[4], want["z_hat"].to(torch.float64))
    assert torch.equal(got[5], want["x_logit"].t()) and torch.equal(got[6], want["z_logit"].t())
    ref = LR.layered_decode(og, sx, sz, 3, "minsum", 0.8, llr_ch=llr)
    assert np.array_equal(got[3].cpu().numpy(), ref["x_hat"]) and got[0].cpu().numpy().tobytes() == ref["llr"][:, 0, :].tobytes()
    flooding = g.bp4_decode(to_gpu(sx), to_gpu(sz), 3, "minsum", 0.8, llr_ch=to_gpu(llr))
    assert not torch.equal(flooding["llr"], want["llr"])
    # the plain call: (x_hat, z_hat); a layering given to the constructor is installed on the graph
    g2 = gpu_graph("ibm72", stage_one=False)
    m = og.m_x + og.m_z
    own = np.arange(m, dtype=np.int32)
    try:
        plain = F.QLDPCBPDecoder(c, cn_type="boxplus-phi", num_iter=2, normalization_factor=1.0, schedule="layered", layers=own, graph=g2)
        assert np.array_equal(g2.layers()[1], own)
        xh, zh = plain((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
        ref = LR.layered_decode(og, sx, sz, 2, "boxplus-phi", 1.0, layer_of=own, llr_ch=llr)
        assert np.array_equal(xh.cpu().numpy(), ref["x_hat"]) and np.array_equal(zh.cpu().numpy(), ref["z_hat"])
    finally:
        g2.set_layers()


def test_schedule_errors():
    import feedback_gnn_amd as F
    c = code("ibm72")
    g = gpu_graph("ibm72")
    for bad in ("serial", "Layered", None, 1):
        with pytest.raises(ValueError, match="schedule"):
            F.QLDPCBPDecoder(c, stage_one=True, graph=g, schedule=bad)
    with pytest.raises(ValueError, match="layers="):
        F.QLDPCBPDecoder(c, stage_one=True, graph=g, layers=np.zeros(g.m_x + g.m_z, np.int32))
    for kw in (dict(trainable=True, stage_one=True), dict(stage_two=True)):
        with pytest.raises(NotImplementedError, match="layered"):
            F.QLDPCBPDecoder(c, graph=g, schedule="layered", **kw)
    lay = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=4, normalization_factor=0.8, stage_one=True, graph=g, schedule="layered")
    flo = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=4, normalization_factor=0.8, stage_one=True, graph=g)
    fb = F.Feedback_GNN(code=c, num_msg_dims=20, num_hidden_units=40, num_mlp_layers=2, reduce_op="mean", activation="tanh",
                        use_bias=True, graph=g)
    for decoders in ([lay, flo], [flo, lay]):
        with pytest.raises(NotImplementedError, match="layered"):
            F.Sandwich_BP_GNN_Evaluation_Model(c, decoders, [fb], num_layers=2)
    F.Sandwich_BP_GNN_Evaluation_Model(c, [flo, lay], [fb], num_layers=1)  # the layered decoder is not a layer of this sandwich
    with pytest.raises(NotImplementedError, match="layered"):
        F.Second_Stage_GNN_BP_Model(c, fb, lay)


def test_models_dispatch_on_the_schedule():
    """The ghp882 batch of the CPU sanity check: eight layered min-sum iterations solve all 64 samples, eight flooding ones leave 44."""
    import feedback_gnn_amd as F
    c = code("ghp882")
    g, og = gpu_graph("ghp882"), oracle_library_forms("ghp882")
    kw = dict(cn_type="minsum", num_iter=8, normalization_factor=0.8, stage_one=True, graph=g)
    lay, flo = F.QLDPCBPDecoder(c, schedule="layered", **kw), F.QLDPCBPDecoder(c, **kw)
    assert g.layers()[0] == 13
    ex, ez = og.pauli_noise(1234, 0.09, 0, 64)
    sx, sz = og.syndrome(ex, ez)
    counts = {}
    for tag, dec in (("layered", lay), ("flooding", flo)):
        model = F.BP4_OSD_Model(c, dec, F.OSD0_Decoder(c.N), seed=1234)
        o = model.decode(64, 0.09)
        assert np.array_equal(o["noise_x"].cpu().numpy(), ex) and np.array_equal(o["noise_z"].cpu().numpy(), ez)
        counts[tag] = model.last_num_osd
    assert counts == {"layered": 0, "flooding": 44}
    direct = g.bp4_decode_layered(to_gpu(sx), to_gpu(sz), 8, "minsum", 0.8, llr_const=llr_const(0.05))
    h_vn, lx, lz = F.First_Stage_BP_Model(c, lay, p0=0.05)(ex, ez)
    assert torch.equal(h_vn, direct["llr"].permute(0, 2, 1)) and torch.equal(lx, direct["x_logit"].t()) and torch.equal(lz, direct["z_logit"].t())
    h_flo, _, _ = F.First_Stage_BP_Model(c, flo, p0=0.05)(ex, ez)
    assert not torch.equal(h_flo, h_vn)
