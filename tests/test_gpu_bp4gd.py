"""BP4 with guided decimation on the GPU (fgnn_bp4gd_decode) at every bp4gd_kernel instantiation, held to the restatement
tests/bp4gd_reference.py bit for bit: x_hat and z_hat as bytes, stats as int32, no tolerance anywhere and no sample left out.  The
restatement's BP4 steps are the CPU oracle's (the float operations the BP4 kernels are held to); the margin is one IEEE float32
subtraction and the selection a maximum under a total order, so nothing depends on a reduction or arrival order.

The noise is the library's seeded depolarizing stream at a rate per code (P_OF) at which, on the restatement alone, a batch holds
samples solved before anything is fixed, samples solved after at least one fix and samples never solved: `mix` asserts it where a test
relies on it."""
import zlib

import numpy as np
import pytest
import torch

import bp4gd_reference as GD
from feedback_gnn_amd import gf2
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h
P_OF = {"steane": 0.15, "rsurf5": 0.15, "ibm72": 0.10, "gb126": 0.05, "toric4": 0.2}
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
# max_rounds of the fixed batch (pre_iter 6, round_iter 3): 8, except where 8 rounds solve every sample of the batch (steane, gb126: 3)
# and on rsurf5, where all n rounds leave two samples with every qubit fixed and no solution
ROUNDS_OF = {"steane": 3, "rsurf5": 25, "ibm72": 8, "gb126": 3, "toric4": 8}


def bp4gd_lds_bytes(E, n, cpb):
    """fgnn_bp4gd_decode: E messages, n decision bytes and n fix bytes per codeword, each rounded up to 4 floats; two 64-bit keys and a
    stamp per codeword, and ndone."""
    area = ((n + 3) // 4 + 3) & ~3
    per_cw = ((E + 3) & ~3) + 2 * area
    return per_cw * 4 * cpb + ((5 * cpb + 1 + 3) & ~3) * 4


def instantiation(g, cn_type="minsum", force_generic=False):
    """The bp4gd_kernel<CN_TYPE, DV, DC> fgnn_bp4gd_decode launches: (3, 6) for min-sum on a (3,3,6)-regular graph with packed slot
    rows, else the loop."""
    info = g.info()
    packed = info["dv_x"] > 0 and info["dv_z"] > 0 and 0 < info["dc"] <= 8 and 4 * (info["E_x"] + info["E_z"]) < 65536
    if cn_type == "minsum" and packed and not force_generic and (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6):
        return (3, 6)
    return (0, 0)


def noisy(og, p, B, first=0):
    """Depolarizing noise of the seeded stream and its syndromes: (ex, ez, synd_x, synd_z)."""
    ex, ez = og.pauli_noise(SEED, p, first, B)
    return (ex, ez) + og.syndrome(ex, ez)


EDGE = np.array([20.0, np.nextafter(F32(20.0), F32(30.0)), np.nextafter(F32(20.0), F32(0.0)), 0.0, 1e-40, 1.4e-45, 25.0], F32)


def informed_edge_channel(ex, ez, seed):
    """llr_ch [B,3,n]: moderate magnitudes with, on one entry in six, an edge value (the +-20 clip of min-sum and its neighbours, the
    default decimation LLR, zeros, subnormals).  The ordering knows half of the noise: at a noisy qubit, with probability 1/2, the LLR of
    the Pauli that hit it is the negative one (that Pauli is then the likeliest of the four); every other LLR says "no error".  Unrelated
    priors would leave every sample unsolved; these let solutions occur, and qubits be fixed to a Pauli, under per-qubit LLRs too."""
    rng = np.random.RandomState(seed)
    B, n = ex.shape
    mag = rng.uniform(0.5, 6.0, size=(B, 3, n)).astype(F32)
    edge = rng.rand(B, 3, n) < 1.0 / 6.0
    mag[edge] = EDGE[rng.randint(len(EDGE), size=int(edge.sum()))]
    row = np.where(ex & ez, 1, np.where(ez != 0, 2, 0))  # rows X, Y, Z of llr_ch
    told = ((ex | ez) != 0) & (rng.rand(B, n) < 0.5)
    neg = np.zeros((B, 3, n), bool)
    b, v = np.nonzero(told)
    neg[b, row[b, v], v] = True
    return np.where(neg, -mag, mag).astype(F32)


def both(g, og, sx, sz, pre, rnd, rounds, factor, cn_type="minsum", decim=25.0, tie_log=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, stats, fixed)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    xh, zh, stats = g.bp4gd_decode(to_gpu(sx), to_gpu(sz), pre, rnd, rounds, decim, cn_type, factor, **gl)
    x0, z0, s0, fixed = GD.bp4gd_decode(og, sx, sz, pre, rnd, rounds, decim, cn_type, factor, tie_log=tie_log, **llr)
    assert stats.dtype == torch.int32 and xh.dtype == torch.uint8 and zh.dtype == torch.uint8
    s1, x1, z1 = stats.cpu().numpy(), xh.cpu().numpy(), zh.cpu().numpy()
    print(cn_type, "found", s0[:, 0].tolist(), "fixed", s0[:, 1].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    assert x0.tobytes() == x1.tobytes() and z0.tobytes() == z1.tobytes()
    return x0, z0, s0, fixed


def mix(stats):
    """Some samples solved with nothing fixed, some after at least one fix, some never: the three ways a codeword leaves the kernel."""
    solved = stats[:, 0] > 0
    return (solved & (stats[:, 1] == 0)).any() and (solved & (stats[:, 1] > 0)).any() and (~solved).any()


def fuzz(name, g, og, rng, cn_types=("minsum",)):
    """B in 1..70, pre_iter and round_iter <= 12, max_rounds 0 / 3 / n, three factors, a constant prior and per-qubit LLRs with edge
    values.  Then one fixed batch per code and rule that holds all three fates."""
    n, p = og.n, P_OF[name]
    for cn in cn_types:
        for rounds, factor in ((0, 1.0), (3, 0.8), (n, 0.625)):
            B, pre, rnd = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            ex, ez, sx, sz = noisy(og, p, B, first=int(rng.randint(1 << 20)))
            both(g, og, sx, sz, pre, rnd, rounds, factor, cn, llr_const=llr_const(p))
            both(g, og, sx, sz, pre, rnd, rounds, factor, cn, llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))))
        ex, ez, sx, sz = noisy(og, p, 40)
        _, _, s0, _ = both(g, og, sx, sz, 6, 3, ROUNDS_OF[name], 0.8, cn, llr_const=llr_const(p))
        assert mix(s0), "the batch must hold samples solved with nothing fixed, solved after a fix and never solved"
        if name == "rsurf5" and cn == "minsum":
            assert ROUNDS_OF[name] == n
            assert ((s0[:, 0] == 0) & (s0[:, 1] == n)).sum() == 2, "two samples end with every qubit fixed and no solution"
        _, _, s0, fixed = both(g, og, sx, sz, 6, 3, 8, 0.8, cn, llr_ch=informed_edge_channel(ex, ez, 77))
        assert (s0[:, 0] > 0).any(), "solutions must occur under per-qubit LLRs too"
        assert (fixed > 0).any(), "qubits must be fixed to a Pauli, not to the identity alone"


# ---- both kinds of instantiation ----------------------------------------------------------------------------------------------------------
def test_regular_instantiation():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    info = g.info()
    assert (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6) and instantiation(g) == (3, 6)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"ibm72")))


def test_force_generic_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    g.force_generic(True)
    try:
        fuzz("ibm72", g, og, np.random.RandomState(17))
    finally:
        g.force_generic(False)


def test_the_two_other_rules_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g, "boxplus") == (0, 0) and instantiation(g, "boxplus-phi") == (0, 0)
    fuzz("ibm72", g, og, np.random.RandomState(23), cn_types=("boxplus", "boxplus-phi"))


@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb126"])
def test_loop_instantiation(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g) == (0, 0)
    if name == "gb126":
        assert int(np.asarray(code(name).hx).sum(1).max()) == 10
    fuzz(name, g, og, np.random.RandomState(zlib.crc32(name.encode())))


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_loop_instantiation_toric4(cn_type):
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("toric4", g, og, np.random.RandomState(zlib.crc32(b"toric4" + cn_type.encode())), cn_types=(cn_type,))


# ---- several codewords per workgroup ---------------------------------------------------------------------------------------------------
def test_codewords_of_one_workgroup_stop_at_different_rounds():
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    L = llr_const(P_OF["rsurf5"])
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], B)  # the same first rows for every B
        _, _, stats, _ = both(g, og, sx, sz, 5, 3, og.n, 0.8, llr_const=L)
        first = stats[:cpb]  # the first workgroup
        assert ((first[:, 0] > 0) & (first[:, 1] == 0)).any(), "no sample of the workgroup stops before anything is fixed"
        assert ((first[:, 0] > 0) & (first[:, 1] > 0)).any(), "no sample of the workgroup stops in a later round"
        assert len(set(first[:, 1].tolist())) >= 3, "the workgroup's samples must stop at different rounds"


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], cpb + 3, first=100)
        _, _, s0, _ = both(g, og, sx, sz, 4, 3, og.n, 0.8, llr_const=llr_const(P_OF["rsurf5"]))
        assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


# ---- anchor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_no_rounds_is_bp4_on_the_gpu(cn_type):
    g = gpu_graph("ghp882")
    B, T, p = 8, 12, 0.03
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    # the geometry of a small batch (a thread per node) and the 256 threads per codeword of a large one
    for launch in ((0, 0), (256, 1)):
        g.set_launch(*launch)
        try:
            for factor in (1.0, 0.8):
                xh, zh, stats = g.bp4gd_decode(sx, sz, T, 5, 0, 25.0, cn_type, factor, llr_const=llr_const(p))
                st = stats.cpu().numpy()
                assert (st[:, 1] == 0).all() and (st[:, 2] == st[:, 3]).all() and (st[st[:, 0] == 0, 3] == T).all() and (st[:, 0] <= 1).all()
                ks = st[:, 3]
                print(cn_type, "found", st[:, 0].tolist(), "k", ks.tolist())
                assert (st[:, 0] == 1).any() and len(set(ks.tolist())) >= 2
                for k in sorted(set(ks.tolist())):
                    out = g.bp4_decode(sx, sz, int(k), cn_type, factor, llr_const=llr_const(p), want_logits=False)
                    sel = torch.from_numpy(ks == k).to(g.device)
                    assert torch.equal(out["x_hat"][sel], xh[sel]) and torch.equal(out["z_hat"][sel], zh[sel]), (launch, factor, k)
        finally:
            g.set_launch(0, 0)


# ---- syndromes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    B = 9
    zx, zz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    x0, z0, s0, _ = both(g, og, zx, zz, 6, 5, 4, 0.8, llr_const=2.0)
    assert not x0.any() and not z0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1)))
    xn, zn, sn = g.bp4gd_decode(None, None, 6, 5, 4, factor=0.8, llr_const=2.0, B=B)
    assert not xn.any() and not zn.any() and np.array_equal(sn.cpu().numpy(), s0)


def test_syndrome_outside_the_column_space():
    """toric4's hx has dependent rows (rank < m_x): a syndrome s for which [hx | s] has a larger rank than hx is the syndrome of no error,
    so no test can pass: found = 0, every round is used, every qubit ends fixed, the output is the pair of the last test.  On this small,
    symmetric code margins tie, and the lowest index wins."""
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    hx = np.asarray(code("toric4").hx, np.int64) % 2
    rk = gf2.rank(hx)
    assert rk < hx.shape[0]
    B, n, rnd = 7, og.n, 2
    _, _, sx, sz = noisy(og, 0.06, B)
    u = np.asarray(gf2.kernel(hx.T)[0], np.int64)[0] % 2  # u hx = 0: u . s = 1 puts s outside the column space
    assert u.any() and not ((u @ hx) % 2).any()
    sx = sx.copy()
    sx[(sx.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1
    for b in range(B):
        assert gf2.rank(np.concatenate([hx, sx[b][:, None].astype(np.int64)], axis=1)) == rk + 1
    ties = []
    _, _, s0, fixed = both(g, og, sx, sz, 4, rnd, n, 0.8, tie_log=ties, llr_const=llr_const(0.06))
    assert (s0[:, 0] == 0).all() and (s0[:, 1] == n).all() and (s0[:, 3] == rnd).all() and (s0[:, 2] == 4 + n * rnd).all()
    assert (fixed >= 0).all() and len(ties) == n and sum(ties) > 0, "ties among the margins must occur"
    # more rounds than qubits are n rounds
    xh, zh, st = g.bp4gd_decode(to_gpu(sx), to_gpu(sz), 4, rnd, n + 5, factor=0.8, llr_const=llr_const(0.06))
    assert np.array_equal(st.cpu().numpy(), s0)


# ---- LDS -------------------------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    """ghp1270 with two codewords per workgroup (128 threads each): 2 x 33 040 bytes of codeword state, on the (3,3,6) instantiation."""
    g, og = gpu_graph("ghp1270"), oracle_library_forms("ghp1270")
    assert instantiation(g) == (3, 6)
    assert bp4gd_lds_bytes(og.E_x + og.E_z, og.n, 1) <= 48 * 1024 < bp4gd_lds_bytes(og.E_x + og.E_z, og.n, 2) <= LDS_BUDGET
    g.set_launch(128, 2)
    try:
        _, _, sx, sz = noisy(og, 0.08, 3)
        _, _, s0, _ = both(g, og, sx, sz, 4, 3, 3, 0.8, llr_const=llr_const(0.08))
        assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    assert bp4gd_lds_bytes(g.E_x + g.E_z, g.n, 1) > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS.*{bp4gd_lds_bytes(g.E_x + g.E_z, g.n, 1)} bytes.*limit is {LDS_BUDGET}"):
        g.bp4gd_decode(sx, sz, 3, 3, 2, factor=0.8, llr_const=2.0)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.bp4gd_decode(sx, sz, 2, 2, 1, cn_type="sum-product")
    for pre, rnd in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            g.bp4gd_decode(sx, sz, pre, rnd, 1)
    with pytest.raises(ValueError, match="max_rounds must be >= 0"):
        g.bp4gd_decode(sx, sz, 2, 2, -1)
    for D in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="decim_llr must be > 0"):
            g.bp4gd_decode(sx, sz, 2, 2, 1, decim_llr=D)
    with pytest.raises(ValueError, match="synd_x"):
        g.bp4gd_decode(sx[:, :-1].contiguous(), sz, 2, 2, 1)
    with pytest.raises(ValueError, match="synd_z"):
        g.bp4gd_decode(sx, sz.to(torch.int32), 2, 2, 1)
    with pytest.raises(ValueError, match="llr_ch"):
        g.bp4gd_decode(sx, sz, 2, 2, 1, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="B is needed"):
        g.bp4gd_decode(None, None, 2, 2, 1)
    # an empty batch is fine and needs no buffers
    xh, zh, st = g.bp4gd_decode(sx[:0], sz[:0], 2, 2, 1)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def test_bp4gd_decoder_class():
    import feedback_gnn_amd as F
    c = code("ibm72")
    og = oracle_library_forms("ibm72")
    n = og.n
    dec = F.BP4GDDecoder(c, pre_iter=6, round_iter=3, max_rounds=8, decim_llr=20.0, normalization_factor=0.8, graph=gpu_graph("ibm72"))
    default = F.BP4GDDecoder(c, graph=dec.graph)
    assert (default.pre_iter, default.round_iter, default.max_rounds, default.decim_llr, default.cn_type,
            default.normalization_factor) == (32, 4, n, 25.0, "minsum", 0.8)
    B = 23
    ex, ez, sx, sz = noisy(og, P_OF["ibm72"], B)
    llr = np.full((B, 3, n), llr_const(P_OF["ibm72"]), F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, n) and tuple(z_hat.shape) == (B, n)
    x0, z0, s0, _ = GD.bp4gd_decode(og, sx, sz, 6, 3, 8, 20.0, "minsum", 0.8, llr_ch=llr)
    assert np.array_equal(x_hat.cpu().numpy(), x0) and np.array_equal(z_hat.cpu().numpy(), z0)
    assert dec.last_stats.dtype == torch.int32 and np.array_equal(dec.last_stats.cpu().numpy(), s0)
    assert (s0[:, 1] > 0).any()
    for kw in (dict(pre_iter=0), dict(round_iter=0), dict(pre_iter=2.5), dict(max_rounds=-1), dict(max_rounds=1.5), dict(decim_llr=0.0),
               dict(cn_type="sum-product")):
        with pytest.raises(ValueError):
            F.BP4GDDecoder(c, graph=dec.graph, **kw)
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((to_gpu(llr.astype(np.float64)), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="length n"):
        dec((to_gpu(llr[:, :, :-1].copy()), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((to_gpu(llr), to_gpu(sx.copy()), to_gpu(sz.T.copy())))


def _gd_model(rank=0, world_size=1, p0=None):
    import feedback_gnn_amd as F
    c = code("ibm72")
    dec = F.BP4GDDecoder(c, pre_iter=6, round_iter=3, max_rounds=8, normalization_factor=0.8, graph=gpu_graph("ibm72"))
    return F.BP4_GD_Model(c, dec, p0=p0, seed=SEED, rank=rank, world_size=world_size), dec


def test_bp4_gd_model():
    c = code("ibm72")
    og = oracle_library_forms("ibm72")
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    B, p = 64, P_OF["ibm72"]
    for p0 in (None, 0.05):
        model, dec = _gd_model(p0=p0)
        s_hat, ls_hat = model(B, p)
        ex, ez = model.last_noise_x.cpu().numpy(), model.last_noise_z.cpu().numpy()
        xh, zh, stats = model.last_x_hat.cpu().numpy(), model.last_z_hat.cpu().numpy(), model.last_stats.cpu().numpy()
        assert tuple(s_hat.shape) == (B, hz.shape[0] + hx.shape[0]) and tuple(ls_hat.shape) == (B, hxp.shape[0] + hzp.shape[0])
        ox, oz = og.pauli_noise(SEED, p, 0, B)
        assert np.array_equal(ex, ox) and np.array_equal(ez, oz), "depolarizing noise of the seeded stream"
        sx, sz = og.syndrome(ex, ez)
        x0, z0, s0, _ = GD.bp4gd_decode(og, sx, sz, 6, 3, 8, 25.0, "minsum", 0.8, llr_const=llr_const(p if p0 is None else p0))
        assert np.array_equal(xh, x0) and np.array_equal(zh, z0) and np.array_equal(stats, s0)
        assert torch.equal(dec.last_stats, model.last_stats)
        xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
        solved = stats[:, 0] > 0
        assert solved.any() and not solved.all(), "the batch must hold solved and unsolved samples"
        assert np.array_equal(s_hat.cpu().numpy(), np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1))
        assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
        assert np.array_equal(ls_hat.cpu().numpy(), np.concatenate([xd @ hxp.T % 2, zd @ hzp.T % 2], axis=1))
        assert model.last_num_unsolved == int((~solved).sum())
        model(B, p)
        assert not np.array_equal(ex, model.last_noise_x.cpu().numpy()), "a second call draws the next samples"


def test_two_ranks_draw_disjoint_sample_ranges():
    og = oracle_library_forms("ibm72")
    B, p = 16, P_OF["ibm72"]
    m0, m1 = _gd_model(0, 2)[0], _gd_model(1, 2)[0]
    for call in range(2):
        r0, r1 = m0.next_sample_range(B), m1.next_sample_range(B)
        assert r0 == (2 * call * B, 2 * call * B + B) and r1 == (2 * call * B + B, 2 * call * B + 2 * B)
        m0(B, p), m1(B, p)
        for m, (first, last) in ((m0, r0), (m1, r1)):
            ox, oz = og.pauli_noise(SEED, p, first, last - first)
            assert np.array_equal(m.last_noise_x.cpu().numpy(), ox) and np.array_equal(m.last_noise_z.cpu().numpy(), oz)


def test_sim_ber_drives_the_model():
    import feedback_gnn_amd as F
    model, _ = _gd_model()
    flagged, bler = F.sim_ber(model, [0.12, 0.06], batch_size=64, max_mc_iter=3, verbose=False, early_stop=False)
    st = F.sim_ber.last
    assert (np.asarray(st["num_blocks"]) == 64 * 3).all()
    assert len(flagged) == 2 and len(bler) == 2
    assert flagged[0] > flagged[1] >= 0 and bler[0] >= flagged[0], "every unsolved sample is flagged; more of them at the higher rate"
