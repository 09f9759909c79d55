"""Relay-BP4 on the GPU (fgnn_relay4_decode) at both relay4_kernel instantiations, held to the restatement tests/relay4_reference.py
bit for bit: x_hat and z_hat as bytes, stats as int32, no tolerance anywhere and no sample left out.  The restatement's BP4 steps are
the CPU oracle's (the float operations the BP4 kernels are held to), everything else is IEEE float32 add and multiply in a fixed order
and integers, so nothing depends on a reduction order.

The noise is the library's seeded depolarizing stream at a rate per code (P_OF) at which, on the restatement alone, a batch holds
samples solved in leg 0, samples solved in a later leg and samples never solved: `mix` asserts it where a test relies on it."""
import zlib

import numpy as np
import pytest
import torch

import relay4_reference as R4
from feedback_gnn_amd import gf2
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h
P_OF = {"steane": 0.15, "rsurf5": 0.15, "ibm72": 0.10, "gb126": 0.05, "toric4": 0.2}


def relay4_lds_bytes(E, n, cpb):
    """fgnn_relay4_decode: E messages, 3n marginals and n decision bytes per codeword, each rounded up to 4 floats; stamp and wacc per
    codeword and ndone."""
    per_cw = ((E + 3) & ~3) + ((3 * n + 3) & ~3) + (((n + 3) // 4 + 3) & ~3)
    return per_cw * 4 * cpb + ((2 * cpb + 1 + 3) & ~3) * 4


def instantiation(g, force_generic=False):
    """The relay4_kernel<DV, DC> fgnn_relay4_decode launches: (3, 6) on a (3,3,6)-regular graph with packed slot rows, else the loop."""
    info = g.info()
    packed = info["dv_x"] > 0 and info["dv_z"] > 0 and 0 < info["dc"] <= 8 and 4 * (info["E_x"] + info["E_z"]) < 65536
    if packed and not force_generic and (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6):
        return (3, 6)
    return (0, 0)


def noisy(og, p, B, first=0):
    """Depolarizing noise of the seeded stream and its syndromes: (ex, ez, synd_x, synd_z)."""
    ex, ez = og.pauli_noise(SEED, p, first, B)
    return (ex, ez) + og.syndrome(ex, ez)


EDGE = np.array([20.0, np.nextafter(F32(20.0), F32(30.0)), np.nextafter(F32(20.0), F32(0.0)), 0.0, 1e-40, 1.4e-45, 25.0], F32)


def informed_edge_channel(ex, ez, seed):
    """llr_ch [B,3,n]: moderate magnitudes with, on one entry in six, an edge value (the +-20 clip of the weight and its neighbours, a
    value beyond it, zeros, subnormals).  The ordering knows half of the noise: at a noisy qubit, with probability 1/2, the LLR of the
    Pauli that hit it is the negative one (that Pauli is then the likeliest of the four); every other LLR says "no error".  Unrelated
    priors would leave every sample unsolved; these let solutions, and their weights, occur under per-qubit LLRs too."""
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


def both(g, og, sx, sz, gamma, pre, leg, stop, factor, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, stats, solutions)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    xh, zh, stats = g.relay4_decode(to_gpu(sx), to_gpu(sz), to_gpu(gamma), pre, leg, stop, factor, **gl)
    x0, z0, s0, sols = R4.relay4_decode(og, sx, sz, gamma, pre, leg, stop, factor, **llr)
    assert stats.dtype == torch.int32 and xh.dtype == torch.uint8 and zh.dtype == torch.uint8
    s1, x1, z1 = stats.cpu().numpy(), xh.cpu().numpy(), zh.cpu().numpy()
    print("found", s0[:, 0].tolist(), "leg", s0[:, 2].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    assert x0.tobytes() == x1.tobytes() and z0.tobytes() == z1.tobytes()
    return x0, z0, s0, sols


def mix(stats, legs):
    """Some samples solved in leg 0, some in a later leg, some never: the three ways a codeword leaves the kernel."""
    solved = stats[:, 0] > 0
    return (solved & (stats[:, 2] == 0)).any() and (legs == 1 or (solved & (stats[:, 2] > 0)).any()) and (~solved).any()


def fuzz(name, g, og, rng):
    """B in 1..70, pre_iter and leg_iter <= 12, 1 / 2 / 5 legs, stop_nconv 1 and 3, three factors, a constant prior and per-qubit LLRs with
    edge values; gamma rows with 0, negative values and values above 0.5.  Then one fixed batch per code that holds all three fates."""
    n = og.n
    for legs, factor in ((1, 1.0), (2, 0.8), (5, 0.625)):
        for stop in (1, 3):
            B, pre, leg = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            ex, ez, sx, sz = noisy(og, P_OF[name], B, first=int(rng.randint(1 << 20)))
            gamma = mixed_gamma(legs, n, int(rng.randint(1 << 30)))
            both(g, og, sx, sz, gamma, pre, leg, stop, factor, llr_const=llr_const(P_OF[name]))
            both(g, og, sx, sz, gamma, pre, leg, stop, factor, llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))))
    ex, ez, sx, sz = noisy(og, P_OF[name], 40)
    _, _, s0, _ = both(g, og, sx, sz, mixed_gamma(5, n, 1), 8, 6, 1, 0.8, llr_const=llr_const(P_OF[name]))
    assert mix(s0, 5), "the batch must hold samples solved in leg 0, solved later and never solved"
    both(g, og, sx, sz, mixed_gamma(5, n, 1), 8, 6, 3, 0.8, llr_const=llr_const(P_OF[name]))
    _, _, s0, _ = both(g, og, sx, sz, mixed_gamma(5, n, 1), 8, 6, 1, 0.8, llr_ch=informed_edge_channel(ex, ez, 77))
    assert (s0[:, 0] > 0).any(), "solutions must occur under per-qubit LLRs too"


# ---- both instantiations ------------------------------------------------------------------------------------------------------------------
def test_regular_instantiation():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    info = g.info()
    assert (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6) and instantiation(g) == (3, 6)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"ibm72")))


@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb126", "toric4"])
def test_loop_instantiation(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g) == (0, 0)
    if name == "gb126":
        assert int(np.asarray(code(name).hx).sum(1).max()) == 10
    fuzz(name, g, og, np.random.RandomState(zlib.crc32(name.encode())))


def test_force_generic_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    g.force_generic(True)
    try:
        fuzz("ibm72", g, og, np.random.RandomState(17))
    finally:
        g.force_generic(False)


# ---- several codewords per workgroup ---------------------------------------------------------------------------------------------------
def test_codewords_of_one_workgroup_stop_at_different_legs():
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    legs = 4
    gamma = mixed_gamma(legs, og.n, 3)
    L = llr_const(P_OF["rsurf5"])
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], B)  # the same first rows for every B
        _, _, stats, _ = both(g, og, sx, sz, gamma, 5, 4, 1, 0.8, llr_const=L)
        first = stats[:cpb]  # the first workgroup
        assert ((first[:, 0] > 0) & (first[:, 2] == 0)).any(), "no sample of the workgroup stops in the first leg"
        assert ((first[:, 0] > 0) & (first[:, 2] > 0)).any(), "no sample of the workgroup stops in a later leg"
        assert len(set(map(tuple, first[:, 2:]))) >= 3, "the workgroup's samples must stop at different steps"
    # stop_nconv = 3: solved samples go on into further legs while others of the workgroup are finished
    _, _, sx, sz = noisy(og, P_OF["rsurf5"], cpb + 1)
    both(g, og, sx, sz, gamma, 5, 4, 3, 0.8, llr_const=L)


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], cpb + 3, first=100)
        both(g, og, sx, sz, mixed_gamma(3, og.n, 4), 4, 3, 2, 0.8, llr_const=llr_const(P_OF["rsurf5"]))
    finally:
        g.set_launch(0, 0)


# ---- anchor ----------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_one_leg_is_bp4_minsum_on_the_gpu():
    g = gpu_graph("ghp882")
    B, T, n, p = 8, 12, g.n, 0.03
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    gamma = torch.zeros((1, n), dtype=torch.float32, device=g.device)
    # the geometry of a small batch (a thread per node) and the 256 threads per codeword of a large one
    for launch in ((0, 0), (256, 1)):
        g.set_launch(*launch)
        try:
            for factor in (1.0, 0.8):
                xh, zh, stats = g.relay4_decode(sx, sz, gamma, T, T, 1, factor, llr_const=llr_const(p))
                st = stats.cpu().numpy()
                assert (st[:, 2] == 0).all() and (st[st[:, 0] == 0, 3] == T).all() and (st[:, 0] <= 1).all()
                ks = st[:, 3]
                print("found", st[:, 0].tolist(), "k", ks.tolist())
                assert (st[:, 0] == 1).any() and len(set(ks.tolist())) >= 2
                for k in sorted(set(ks.tolist())):
                    out = g.bp4_decode(sx, sz, int(k), "minsum", factor, llr_const=llr_const(p), want_logits=False)
                    sel = torch.from_numpy(ks == k).to(g.device)
                    assert torch.equal(out["x_hat"][sel], xh[sel]) and torch.equal(out["z_hat"][sel], zh[sel]), (launch, factor, k)
        finally:
            g.set_launch(0, 0)


# ---- syndromes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    B, n = 9, og.n
    gamma = mixed_gamma(3, n, 5)
    zx, zz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    x0, z0, s0, _ = both(g, og, zx, zz, gamma, 6, 5, 1, 0.8, llr_const=2.0)
    assert not x0.any() and not z0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 0, 1], np.int32), (B, 1)))
    xn, zn, sn = g.relay4_decode(None, None, to_gpu(gamma), 6, 5, 1, 0.8, llr_const=2.0, B=B)
    assert not xn.any() and not zn.any() and np.array_equal(sn.cpu().numpy(), s0)


def test_syndrome_outside_the_column_space():
    """toric4's hx has dependent rows (rank < m_x): a syndrome s for which [hx | s] has a larger rank than hx is the syndrome of no error,
    so no test can pass: found = 0, every leg is used, the output is the pair of the last test of the last leg."""
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    hx = np.asarray(code("toric4").hx, np.int64) % 2
    rk = gf2.rank(hx)
    assert rk < hx.shape[0]
    B, legs, leg_iter = 7, 3, 5
    _, _, sx, sz = noisy(og, 0.06, B)
    u = np.asarray(gf2.kernel(hx.T)[0], np.int64)[0] % 2  # u hx = 0: u . s = 1 puts s outside the column space
    assert u.any() and not ((u @ hx) % 2).any()
    sx = sx.copy()
    sx[(sx.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1
    for b in range(B):
        assert gf2.rank(np.concatenate([hx, sx[b][:, None].astype(np.int64)], axis=1)) == rk + 1
    for stop in (1, 3):
        _, _, s0, sols = both(g, og, sx, sz, mixed_gamma(legs, og.n, 6), 6, leg_iter, stop, 0.8, llr_const=llr_const(0.06))
        assert (s0[:, 0] == 0).all() and (s0[:, 2] == legs - 1).all() and (s0[:, 3] == leg_iter).all() and not any(sols)


# ---- LDS -------------------------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    """ghp1270 with two codewords per workgroup (128 threads each): 2 x 47 008 bytes of codeword state, on the (3,3,6) instantiation."""
    g, og = gpu_graph("ghp1270"), oracle_library_forms("ghp1270")
    assert instantiation(g) == (3, 6)
    assert relay4_lds_bytes(og.E_x + og.E_z, og.n, 1) <= 48 * 1024 < relay4_lds_bytes(og.E_x + og.E_z, og.n, 2) <= LDS_BUDGET
    g.set_launch(128, 2)
    try:
        _, _, sx, sz = noisy(og, 0.04, 3)
        both(g, og, sx, sz, mixed_gamma(2, og.n, 7), 4, 3, 1, 0.8, llr_const=llr_const(0.04))
    finally:
        g.set_launch(0, 0)


def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    assert relay4_lds_bytes(g.E_x + g.E_z, g.n, 1) > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    gamma = torch.zeros((1, g.n), dtype=torch.float32, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS.*{relay4_lds_bytes(g.E_x + g.E_z, g.n, 1)} bytes.*limit is {LDS_BUDGET}"):
        g.relay4_decode(sx, sz, gamma, 3, 3, 1, 0.8, llr_const=2.0)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    gamma = torch.zeros((2, n), dtype=torch.float32, device=g.device)
    for cn in ("boxplus", "boxplus-phi"):
        with pytest.raises(ValueError, match="min-sum"):
            g.relay4_decode(sx, sz, gamma, 2, 2, 1, cn_type=cn)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.relay4_decode(sx, sz, gamma, 2, 2, 1, cn_type="sum-product")
    for pre, leg, stop in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError, match=">= 1"):
            g.relay4_decode(sx, sz, gamma, pre, leg, stop)
    with pytest.raises(ValueError, match="gamma is NULL"):
        g.relay4_decode(sx, sz, None, 2, 2, 1)
    with pytest.raises(ValueError, match="gamma"):
        g.relay4_decode(sx, sz, gamma[:, :n - 1].contiguous(), 2, 2, 1)
    with pytest.raises(ValueError, match="gamma"):
        g.relay4_decode(sx, sz, gamma.double(), 2, 2, 1)
    with pytest.raises(ValueError, match="synd_x"):
        g.relay4_decode(sx[:, :-1].contiguous(), sz, gamma, 2, 2, 1)
    with pytest.raises(ValueError, match="llr_ch"):
        g.relay4_decode(sx, sz, gamma, 2, 2, 1, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    # an empty batch is fine and needs no buffers: not even gamma
    xh, zh, st = g.relay4_decode(sx[:0], sz[:0], None, 2, 2, 1)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def test_relay_bp4_decoder_class():
    import feedback_gnn_amd as F
    c = code("ibm72")
    og = oracle_library_forms("ibm72")
    n = og.n
    dec = F.RelayBP4Decoder(c, gamma0=0.125, pre_iter=8, num_sets=3, set_max_iter=6, stop_nconv=2, normalization_factor=0.8, seed=5)
    same = F.RelayBP4Decoder(c, pre_iter=8, num_sets=3, set_max_iter=6, seed=5, graph=dec.graph)
    other = F.RelayBP4Decoder(c, pre_iter=8, num_sets=3, set_max_iter=6, seed=6, graph=dec.graph)
    gam = dec.gamma.cpu().numpy()
    assert dec.num_legs == 4 and gam.shape == (4, n) and gam.dtype == F32 and (gam[0] == F32(0.125)).all()
    assert gam[1:].min() >= -0.24 and gam[1:].max() <= 0.66 and gam[1:].min() < 0 and gam[1:].max() > 0.5
    assert torch.equal(dec.gamma, same.gamma) and not torch.equal(dec.gamma, other.gamma)
    assert np.array_equal(gam[1:], np.random.default_rng(5).uniform(-0.24, 0.66, size=(3, n)).astype(F32))
    B = 23
    ex, ez, sx, sz = noisy(og, P_OF["ibm72"], B)
    llr = np.full((B, 3, n), llr_const(P_OF["ibm72"]), F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, n) and tuple(z_hat.shape) == (B, n)
    x0, z0, s0, _ = R4.relay4_decode(og, sx, sz, gam, 8, 6, 2, 0.8, llr_ch=llr)
    assert np.array_equal(x_hat.cpu().numpy(), x0) and np.array_equal(z_hat.cpu().numpy(), z0)
    assert dec.last_stats.dtype == torch.int32 and np.array_equal(dec.last_stats.cpu().numpy(), s0)
    dec.gamma = np.zeros((4, n))
    assert dec.gamma.dtype == torch.float32 and not dec.gamma.any() and dec.gamma.device == dec.graph.device
    with pytest.raises(ValueError, match="gamma must have shape"):
        dec.gamma = np.zeros((3, n))
    for kw in (dict(pre_iter=0), dict(set_max_iter=0), dict(stop_nconv=0), dict(pre_iter=2.5), dict(num_sets=-1),
               dict(gamma_dist_interval=(0.5, 0.1))):
        with pytest.raises(ValueError):
            F.RelayBP4Decoder(c, graph=dec.graph, **kw)
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((to_gpu(llr.astype(np.float64)), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="length n"):
        dec((to_gpu(llr[:, :, :-1].copy()), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((to_gpu(llr), to_gpu(sx.copy()), to_gpu(sz.T.copy())))


def _relay4_model(rank=0, world_size=1, p0=None):
    import feedback_gnn_amd as F
    c = code("ibm72")
    dec = F.RelayBP4Decoder(c, pre_iter=10, num_sets=3, set_max_iter=8, normalization_factor=0.8, seed=1, graph=gpu_graph("ibm72"))
    return F.BP4_Relay_Model(c, dec, p0=p0, seed=SEED, rank=rank, world_size=world_size), dec


def test_bp4_relay_model():
    c = code("ibm72")
    og = oracle_library_forms("ibm72")
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    B, p = 64, P_OF["ibm72"]
    for p0 in (None, 0.05):
        model, dec = _relay4_model(p0=p0)
        s_hat, ls_hat = model(B, p)
        ex, ez = model.last_noise_x.cpu().numpy(), model.last_noise_z.cpu().numpy()
        xh, zh, stats = model.last_x_hat.cpu().numpy(), model.last_z_hat.cpu().numpy(), model.last_stats.cpu().numpy()
        assert tuple(s_hat.shape) == (B, hz.shape[0] + hx.shape[0]) and tuple(ls_hat.shape) == (B, hxp.shape[0] + hzp.shape[0])
        ox, oz = og.pauli_noise(SEED, p, 0, B)
        assert np.array_equal(ex, ox) and np.array_equal(ez, oz), "depolarizing noise of the seeded stream"
        sx, sz = og.syndrome(ex, ez)
        x0, z0, s0, _ = R4.relay4_decode(og, sx, sz, dec.gamma.cpu().numpy(), 10, 8, 1, 0.8, llr_const=llr_const(p if p0 is None else p0))
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
    m0, m1 = _relay4_model(0, 2)[0], _relay4_model(1, 2)[0]
    for call in range(2):
        r0, r1 = m0.next_sample_range(B), m1.next_sample_range(B)
        assert r0 == (2 * call * B, 2 * call * B + B) and r1 == (2 * call * B + B, 2 * call * B + 2 * B)
        m0(B, p), m1(B, p)
        for m, (first, last) in ((m0, r0), (m1, r1)):
            ox, oz = og.pauli_noise(SEED, p, first, last - first)
            assert np.array_equal(m.last_noise_x.cpu().numpy(), ox) and np.array_equal(m.last_noise_z.cpu().numpy(), oz)


def test_sim_ber_drives_the_model():
    import feedback_gnn_amd as F
    model, _ = _relay4_model()
    flagged, bler = F.sim_ber(model, [0.12, 0.06], batch_size=64, max_mc_iter=3, verbose=False, early_stop=False)
    st = F.sim_ber.last
    assert (np.asarray(st["num_blocks"]) == 64 * 3).all()
    assert len(flagged) == 2 and len(bler) == 2
    assert flagged[0] > flagged[1] >= 0 and bler[0] >= flagged[0], "every unsolved sample is flagged; more of them at the higher rate"
