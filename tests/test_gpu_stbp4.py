"""Space-time BP4 on the GPU (fgnn_stbp4_decode) at every stbp4_kernel instantiation (the runtime-degree loop for each check rule and
min-sum on the packed rows of a (3,3,6)-regular graph), held to the restatement tests/stbp4_reference.py bit for bit: x_hat, z_hat, u_x_hat and u_z_hat as bytes, all four stats columns as
int32, no tolerance anywhere and no window left out.  The restatement is NumPy float32 on the oracle's transcendentals;
tests/test_stbp4_reference_cpu.py ties it to the soft-syndrome restatement, to the oracle's check rules and to the host build of
fgnn_cn.h.

The data noise is the library's seeded depolarizing stream, a fresh error before every round; the syndromes are those of the
accumulated error with flips of the seeded syndrome-noise streams.  Where a test relies on an outcome occurring it asserts so on the
restatement's outputs."""
import functools
import zlib

import numpy as np
import pytest
import torch

import mbp4_reference as MB
import stbp4_reference as ST
import test_gpu_bp4gd as TGD
from guarded import guarded
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_dsbp4_reference_cpu import gamma_of_q
from test_gpu_dsbp4 import GAMMA_EDGE
from test_stbp4_reference_cpu import window_noise

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
SEED = 0x5EED
LDS_BUDGET = TGD.LDS_BUDGET
P_OF = TGD.P_OF
informed_edge_channel, instantiation = TGD.informed_edge_channel, TGD.instantiation  # the dispatch rule is BP4-GD's
OUT = ("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats")
ALPHAS3 = (1.0, 0.8, 0.6)


def tables(alphas, base=0.8):
    return MB.mbp4_tables(alphas, base)


def gamma_arrays(og, B, R, seed):
    """Per-check syndrome LLRs [B,R,m_x], [B,R,m_z]: moderate values with, on one entry in eight, an edge value of dsbp4's table."""
    rng = np.random.RandomState(seed)
    out = []
    for m in (og.m_x, og.m_z):
        g = rng.uniform(1.0, 5.0, size=(B, R, m)).astype(F32)
        edge = rng.rand(B, R, m) < 0.125
        g[edge] = GAMMA_EDGE[rng.randint(len(GAMMA_EDGE), size=int(edge.sum()))]
        out.append(g)
    return dict(synd_llr_x=out[0], synd_llr_z=out[1])


def both(name, g, sx, sz, factors, owns, pre, att, cn_type="minsum", restart=True, ref=None, **kw):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's five."""
    dev = {k: (to_gpu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    got = g.stbp4_decode(to_gpu(sx), to_gpu(sz), factors, owns, pre, att, cn_type, restart=restart, **dev)
    want = ref or ST.stbp4_decode(code(name), sx, sz, factors, owns, pre, att, cn_type, restart=restart, **kw)
    assert [t.dtype for t in got] == [torch.uint8] * 4 + [torch.int32]
    s0, s1 = want[4], got[4].cpu().numpy()
    print(name, cn_type, "R", sx.shape[1], "restart", restart, "found", s0[:, 0].tolist(), "a", s0[:, 1].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    for label, w, t in zip(OUT[:4], want, got):
        a = t.cpu().numpy()
        assert a.shape == w.shape and w.tobytes() == a.tobytes(), (label, np.nonzero((w != a).any((1, 2)))[0])
    return want


# ---- 1: fuzz, every instantiation ----------------------------------------------------------------------------------------------------------------
FUZZ = [(name, "minsum") for name in ("steane", "rsurf5", "toric4", "ibm72", "gb126")] + \
       [(name, cn) for name in ("toric4", "ibm72") for cn in ("boxplus", "boxplus-phi")]


def forced_loop(g, on):
    """Context of a test that runs the runtime-degree loop on a regular graph."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        g.force_generic(on)
        try:
            yield
        finally:
            g.force_generic(False)
    return cm()


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("name,cn", FUZZ)
def test_fuzz(name, cn, R):
    fuzz(name, cn, R)


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_fuzz_of_the_loop_on_a_regular_graph(R):
    g = gpu_graph("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    with forced_loop(g, True):
        fuzz("ibm72", "minsum", R, salt="loop")


def fuzz(name, cn, R, salt=""):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g, cn) == ((3, 6) if (name, cn) == ("ibm72", "minsum") else (0, 0))
    rng = np.random.RandomState(zlib.crc32(f"st-{name}-{cn}-{R}{salt}".encode()))
    p, q = P_OF[name] / R, 0.05
    gq = gamma_of_q(q)
    found = set()
    for i, ((factors, owns), restart) in enumerate(((tables((1.0,), 1.0), False), (tables(ALPHAS3), True),
                                                    ((rng.uniform(0.4, 1.3, 5).astype(F32), np.array([1.0, 0.0, 1.25, 0.7, 0.45], F32)), False))):
        B, pre, att = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
        ex, ez, sx, sz, _, _ = window_noise(name, p, q, B, R, first=int(rng.randint(1 << 16)), perfect_last=(i == 0))
        prev = dict(prev_x=rng.randint(0, 2, size=(B, og.m_x)).astype(np.uint8), prev_z=rng.randint(0, 2, size=(B, og.m_z)).astype(np.uint8))
        if i == 0:
            kw = dict(gamma_x=gq, gamma_z=gq, llr_const=llr_const(p))
        elif i == 1:
            kw = dict(gamma_arrays(og, B, R, int(rng.randint(1 << 30))), **prev,
                      llr_ch=informed_edge_channel(ex[:, 0] | ex[:, R - 1], ez[:, 0] | ez[:, R - 1], int(rng.randint(1 << 30))))
        else:
            kw = dict(gamma_x=gq, gamma_z=2.0, gamma_last_x=1.5, gamma_last_z=gq, llr_const=llr_const(p), **prev)
        ref = both(name, g, sx, sz, factors, owns, pre, att, cn, restart, **kw)
        found |= set(ref[4][:, 0].tolist())
    print(name, cn, R, "outcomes", found)


# ---- 2: the fixed batch -----------------------------------------------------------------------------------------------------------------------------
# (p per round, q) at which 40 seeded windows of R = 3 under the alphas (1.0, 0.8, 0.6), 6 then 4 iterations, hold solved and unsolved
# windows and a non-zero u_hat at the interior round, for all three check rules (asserted below on the restatement)
FIXED = {"steane": (0.05, 0.15), "rsurf5": (0.05, 0.1), "toric4": (0.06, 0.1), "ibm72": (0.04, 0.05), "gb126": (0.03, 0.05)}


@functools.lru_cache(maxsize=None)
def fixed_batch_reference(name, cn):
    p, q = FIXED[name]
    _, _, sx, sz, _, _ = window_noise(name, p, q, 40, 3)
    gq = gamma_of_q(q)
    ref = ST.stbp4_decode(code(name), sx, sz, *tables(ALPHAS3), 6, 4, cn, llr_const=llr_const(p), gamma_x=gq, gamma_z=gq)
    solved = ref[4][:, 0] > 0
    interior = int((ref[2][:, 1].any(1) | ref[3][:, 1].any(1)).sum())
    print(name, cn, "solved", int(solved.sum()), "unsolved", int((~solved).sum()), "windows with u_hat != 0 at the interior round", interior)
    assert solved.any() and (~solved).any() and interior > 0
    return sx, sz, gq, ref


@pytest.mark.parametrize("cn", TGD.CN_TYPES)
@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_batch(name, cn):
    sx, sz, gq, ref = fixed_batch_reference(name, cn)
    g = gpu_graph(name)
    both(name, g, sx, sz, *tables(ALPHAS3), 6, 4, cn, ref=ref, llr_const=llr_const(FIXED[name][0]), gamma_x=gq, gamma_z=gq)
    if instantiation(g, cn) == (3, 6):  # then the loop on the same inputs, against the same reference
        with forced_loop(g, True):
            both(name, g, sx, sz, *tables(ALPHAS3), 6, 4, cn, ref=ref, llr_const=llr_const(FIXED[name][0]), gamma_x=gq, gamma_z=gq)


# ---- 3: one round is soft-syndrome BP4, on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", TGD.CN_TYPES)
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_one_round_equals_dsbp4_decode_on_the_device(name, cn):
    g, og = gpu_graph(name), oracle_library_forms(name)
    B, p = 45, P_OF[name]
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    ux, uz = g.syndrome_noise(SEED, 0.05, 0, B)
    sx, sz = sx ^ ux, sz ^ uz
    arr = {k: to_gpu(v) for k, v in gamma_arrays(og, B, 1, 3).items()}
    for alphas, restart in ((ALPHAS3, True), (ALPHAS3, False)):
        for ds_kw, st_kw in ((dict(gamma_x=2.5, gamma_z=3.5), dict(gamma_x=2.5, gamma_z=3.5, gamma_last_x=2.5, gamma_last_z=3.5)),
                             (dict(synd_llr_x=arr["synd_llr_x"][:, 0].contiguous(), synd_llr_z=arr["synd_llr_z"][:, 0].contiguous()), arr)):
            want = g.dsbp4_decode(sx, sz, *tables(alphas), 6, 4, cn, restart=restart, llr_const=llr_const(p), **ds_kw)
            got = g.stbp4_decode(sx[:, None].contiguous(), sz[:, None].contiguous(), *tables(alphas), 6, 4, cn, restart=restart,
                                 llr_const=llr_const(p), **st_kw)
            for label, w, t in zip(OUT, want, got):
                assert torch.equal(w.reshape(t.shape), t), (label, alphas, restart)
            assert 0 < int(want[4][:, 0].sum()) < B and bool(want[2].any())


# ---- 4: launch geometries --------------------------------------------------------------------------------------------------------------------------
def test_the_outputs_do_not_depend_on_the_launch_geometry():
    """The default plan for the window, one thread per window (every node and every time variable in one lane; the difference bits are
    then read again in every step), and 64 threads with two windows per workgroup."""
    name, R = "rsurf5", 3
    g, og = gpu_graph(name), oracle_library_forms(name)
    B, p = 11, 0.06
    _, _, sx, sz, _, _ = window_noise(name, p, 0.1, B, R, first=100)
    kw = dict(gamma_arrays(og, B, R, 5), llr_const=llr_const(p))
    ref = both(name, g, sx, sz, *tables(ALPHAS3), 4, 3, "minsum", True, **kw)
    assert 0 < int(ref[4][:, 0].sum()) < B and (ref[4][:, 1] > 0).any() and ref[2].any()
    for tpc, cpb in ((1, 64), (64, 2)):
        g.set_launch(tpc, cpb)
        try:
            both(name, g, sx, sz, *tables(ALPHAS3), 4, 3, "minsum", True, ref=ref, **kw)
        finally:
            g.set_launch(0, 0)


# ---- 5: the LDS limit ---------------------------------------------------------------------------------------------------------------------------------
def test_the_largest_window_of_ghp882_runs_and_the_next_is_refused():
    name = "ghp882"
    g, og = gpu_graph(name), oracle_library_forms(name)
    E, m = og.E_x + og.E_z, og.m_x + og.m_z
    fit = max(R for R in range(1, 12) if ST.stbp4_lds_bytes(E, og.n, m, R, 1) <= LDS_BUDGET)
    assert fit == 5 and ST.stbp4_lds_bytes(E, og.n, m, fit, 1) > 48 * 1024
    B, p = 2, 0.02
    _, _, sx, sz, _, _ = window_noise(name, p, 0.01, B, fit)
    gq = gamma_of_q(0.01)
    assert instantiation(g) == (3, 6)
    ref = both(name, g, sx, sz, *tables((1.0,)), 2, 2, "minsum", llr_const=llr_const(p), gamma_x=gq, gamma_z=gq)
    assert ref[0].any() or ref[1].any()
    with forced_loop(g, True):
        both(name, g, sx, sz, *tables((1.0,)), 2, 2, "minsum", ref=ref, llr_const=llr_const(p), gamma_x=gq, gamma_z=gq)
    need = ST.stbp4_lds_bytes(E, og.n, m, fit + 1, 1)
    assert need > LDS_BUDGET
    sx6 = torch.zeros((B, fit + 1, og.m_x), dtype=torch.uint8, device=g.device)
    sz6 = torch.zeros((B, fit + 1, og.m_z), dtype=torch.uint8, device=g.device)
    with guarded(g) as guard:
        with pytest.raises(ValueError, match=rf"{fit + 1} rounds need {need} bytes of LDS.*limit is {LDS_BUDGET}.*largest number of rounds that fits is {fit}"):
            g.stbp4_decode(sx6, sz6, *tables((1.0,)), 2, 2, llr_const=2.0)
        for r in guard.records:  # nothing was launched: every output still holds its poison
            guard.assert_untouched(guard.payload(r), "output")


# ---- 6: guard bands ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_generic", [False, True], ids=["regular", "loop"])
def test_outputs_between_guards(force_generic):
    """Every output of the entry point is a poisoned payload between two guards: no byte is written outside, none is left stale.  Six
    windows, one per workgroup; some are solved and leave early."""
    name, R = "ibm72", 3
    g, og = gpu_graph(name), oracle_library_forms(name)
    B, (p, q) = 6, FIXED[name]
    # rounds 1 .. 3 of a four-round experiment, from the exact syndrome of round 0; the syndrome LLRs as full arrays
    _, _, sx, sz, ux, uz = window_noise(name, p, q, B, R + 1)
    prev = dict(prev_x=np.ascontiguousarray(sx[:, 0] ^ ux[:, 0]), prev_z=np.ascontiguousarray(sz[:, 0] ^ uz[:, 0]))
    sx, sz = np.ascontiguousarray(sx[:, 1:]), np.ascontiguousarray(sz[:, 1:])
    gam = dict(synd_llr_x=np.full((B, R, og.m_x), gamma_of_q(q), F32), synd_llr_z=np.full((B, R, og.m_z), gamma_of_q(q), F32))
    gam["synd_llr_x"][:, R - 1], gam["synd_llr_z"][:, R - 1] = INF, INF
    assert prev["prev_x"].any() and prev["prev_z"].any()
    ref = ST.stbp4_decode(code(name), sx, sz, *tables(ALPHAS3), 6, 4, "minsum", llr_const=llr_const(p), **gam, **prev)
    assert 0 < int(ref[4][:, 0].sum()) < B, "windows must leave the kernel solved and unsolved"
    dev = {k: to_gpu(v) for k, v in dict(gam, **prev).items()}
    dsx, dsz = to_gpu(sx), to_gpu(sz)
    keep = [t.clone() for t in (dsx, dsz, *dev.values())]
    assert instantiation(g, force_generic=force_generic) == ((0, 0) if force_generic else (3, 6))
    with forced_loop(g, force_generic), guarded(g) as guard:
        got = g.stbp4_decode(dsx, dsz, *tables(ALPHAS3), 6, 4, "minsum", llr_const=llr_const(p), **dev)
        guard.label(dict(zip(OUT, got)))
        assert len(guard.records) == 5, "all five outputs come from the allocator"
        guard.check()
        for label, t in zip(OUT, got):
            guard.assert_written(t, label)
    for label, w, t in zip(OUT, ref, got):
        assert np.array_equal(w, t.cpu().numpy()), label
    for before, after in zip(keep, (dsx, dsz, *dev.values())):
        assert before.view(torch.uint8).equal(after.view(torch.uint8)), "the inputs are read only"


# ---- 7: arguments -------------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_batch_needs_no_buffers():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    R = 3
    sx = torch.zeros((0, R, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((0, R, g.m_z), dtype=torch.uint8, device=g.device)
    xh, zh, ux, uz, st = g.stbp4_decode(sx, sz, [0.8], [1.0], 2, 2)
    assert tuple(xh.shape) == (0, R, g.n) and tuple(zh.shape) == (0, R, g.n) and tuple(st.shape) == (0, 4)
    assert tuple(ux.shape) == (0, R, g.m_x) and tuple(uz.shape) == (0, R, g.m_z)
    tab = np.array([0.8], F32)
    t = tab.ctypes.data
    assert _lib.lib().fgnn_stbp4_decode(g.handle, 2, 1, t, t, 2, 2, 1, R, None, 2.0, None, None, None, None, None, 3.0, 3.0, None, 3.0, 3.0, 0,
                                        None, None, None, None, None, None) == 0


def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    R = 2
    sx = torch.zeros((2, R, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, R, g.m_z), dtype=torch.uint8, device=g.device)
    for count in (0, 65):
        with pytest.raises(ValueError, match="num_attempts"):
            g.stbp4_decode(sx, sz, [0.8] * count, [1.0] * count, 2, 2)
    for pre, att in ((0, 1), (1, 0)):
        with pytest.raises(ValueError, match=">= 1"):
            g.stbp4_decode(sx, sz, [0.8], [1.0], pre, att)
    with pytest.raises(ValueError, match="restart"):
        g.stbp4_decode(sx, sz, [0.8], [1.0], 2, 2, restart=2)
    with pytest.raises(ValueError, match="factor"):
        g.stbp4_decode(sx, sz, [0.8, 0.0], [1.0, 1.0], 2, 2)
    with pytest.raises(ValueError, match="own"):
        g.stbp4_decode(sx, sz, [0.8, 0.8], [1.0, -0.5], 2, 2)
    for key in ("gamma_x", "gamma_z", "gamma_last_x", "gamma_last_z"):
        with pytest.raises(ValueError, match="NaN"):
            g.stbp4_decode(sx, sz, [0.8], [1.0], 2, 2, **{key: float("nan")})
    tab = np.array([0.8], F32)
    t = tab.ctypes.data
    xh, zh = (torch.zeros((2, R, g.n), dtype=torch.uint8, device=g.device) for _ in range(2))
    ux, uz = torch.zeros_like(sx), torch.zeros_like(sz)
    st = torch.zeros((2, 4), dtype=torch.int32, device=g.device)

    def call(rounds, ux_ptr):
        return _lib.lib().fgnn_stbp4_decode(g.handle, 2, 1, t, t, 2, 2, 1, rounds, None, 2.0, sx.data_ptr(), sz.data_ptr(), None, None, None, 3.0,
                                            3.0, None, 3.0, 3.0, 2, xh.data_ptr(), zh.data_ptr(), ux_ptr, uz.data_ptr(), st.data_ptr(), None)

    for args, word in (((0, ux.data_ptr()), "rounds must be >= 1"), ((R, None), "no output buffer")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(*args))
    _lib.check(call(R, ux.data_ptr()))
    g.stbp4_decode(sx, sz, [0.8, 0.8], [1.0, 0.0], 2, 2, gamma_x=-1.0, gamma_z=float("-inf"), gamma_last_x=0.0)  # legal values


# ---- 8: the decoder and the model ---------------------------------------------------------------------------------------------------------------
MODEL = {"steane": (0.04, 0.05), "toric4": (0.05, 0.05)}


@pytest.mark.parametrize("window,commit", [(3, 1), (3, 2)])
@pytest.mark.parametrize("name", sorted(MODEL))
def test_phenomenological_model_is_the_numpy_loop(name, window, commit):
    import feedback_gnn_amd as F
    c, og = code(name), oracle_library_forms(name)
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    rounds, B, (p, q) = 5, 24, MODEL[name]
    dec = F.SpaceTimeBP4Decoder(c, window, alphas=ALPHAS3, num_iter=6, graph=gpu_graph(name))
    model = F.BP4_Phenomenological_Model(c, dec, q, rounds, window, commit, seed=SEED)
    f, o = tables(ALPHAS3)
    g, L = gamma_of_q(q), llr_const(p)

    def decode(wx, wz, px, pz, gl):
        return ST.stbp4_decode(c, wx, wz, f, o, 6, 6, "minsum", prev_x=px, prev_z=pz, llr_const=L, gamma_x=g, gamma_z=g, gamma_last_x=gl,
                               gamma_last_z=gl)

    seen = 0
    for call in range(2):  # the second batch decodes global samples B .. 2B - 1
        s_hat, ls_hat = model(B, p)
        ex, ez, sx, sz, ux, uz = window_noise(name, p, q, B, rounds, first=call * B)
        for attr, w in (("last_noise_x", ex), ("last_noise_z", ez), ("last_u_x", ux), ("last_u_z", uz)):
            assert np.array_equal(getattr(model, attr).cpu().numpy(), w), attr
        xh, zh, uxh, uzh, unsolved, calls = ST.sliding_decode(decode, sx, sz, rounds, window, commit, g)
        for attr, w in (("last_x_hat", xh), ("last_z_hat", zh), ("last_u_x_hat", uxh), ("last_u_z_hat", uzh)):
            assert np.array_equal(getattr(model, attr).cpu().numpy(), w), attr
        assert model.last_num_unsolved == unsolved and len(model.last_window_stats) == len(calls)
        xd = (np.bitwise_xor.reduce(ex, axis=1) ^ np.bitwise_xor.reduce(xh, axis=1)).astype(np.int64)
        zd = (np.bitwise_xor.reduce(ez, axis=1) ^ np.bitwise_xor.reduce(zh, axis=1)).astype(np.int64)
        assert np.array_equal(s_hat.cpu().numpy(), np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1))
        assert np.array_equal(ls_hat.cpu().numpy(), np.concatenate([xd @ hxp.T % 2, zd @ hzp.T % 2], axis=1))
        seen += int(uxh.any()) + int(uzh.any())
    assert seen > 0, "the batches must estimate measurement flips"


def test_decoder_call_keeps_the_dtypes_of_its_siblings():
    import feedback_gnn_amd as F
    name, R = "toric4", 3
    c, og = code(name), oracle_library_forms(name)
    p, q = MODEL[name]
    dec = F.SpaceTimeBP4Decoder(c, R, alphas=ALPHAS3, num_iter=6, graph=gpu_graph(name))
    B = 16
    _, _, sx, sz, _, _ = window_noise(name, p, q, B, R)
    llr = np.full((B, 3, og.n), llr_const(p), F32)
    dec.gamma = gamma_of_q(q)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(np.ascontiguousarray(sx.transpose(1, 2, 0))), to_gpu(np.ascontiguousarray(sz.transpose(1, 2, 0)))))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, og.n) and tuple(z_hat.shape) == (B, og.n)
    want = ST.stbp4_decode(c, sx, sz, *tables(ALPHAS3), 6, 6, "minsum", llr_ch=llr, gamma_x=dec.gamma, gamma_z=dec.gamma)
    assert np.array_equal(x_hat.cpu().numpy(), np.bitwise_xor.reduce(want[0], axis=1))
    assert np.array_equal(z_hat.cpu().numpy(), np.bitwise_xor.reduce(want[1], axis=1))
    assert np.array_equal(dec.last_stats.cpu().numpy(), want[4]) and np.array_equal(dec.last_u_x_hat.cpu().numpy(), want[2])
    assert dec.last_correction_x.dtype == torch.uint8 and np.array_equal(dec.last_correction_z.cpu().numpy(), np.bitwise_xor.reduce(want[1], axis=1))
