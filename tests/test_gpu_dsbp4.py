"""Soft-syndrome BP4 on the GPU (fgnn_dsbp4_decode) at every dsbp4_kernel instantiation, held to the restatement
tests/dsbp4_reference.py bit for bit: x_hat, z_hat, u_x_hat and u_z_hat as bytes, all four stats columns as int32, no tolerance
anywhere and no sample left out.  The restatement is NumPy float32 on the oracle's transcendentals; tests/test_dsbp4_reference_cpu.py
ties it to the oracle's check rules, to the host build of fgnn_cn.h and to the AMBP4 restatement.

The data noise is the library's seeded depolarizing stream at the rate per code of tests/test_gpu_bp4gd.py (P_OF); the syndromes carry
flips of the seeded syndrome-noise streams at q = 0.05.  Where a test relies on an outcome occurring it asserts so on the
restatement's outputs."""
import zlib

import numpy as np
import pytest
import torch

import dsbp4_reference as DS
import mbp4_reference as MB
import test_gpu_bp4gd as TGD
from guarded import guarded
from helpers import code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_dsbp4_reference_cpu import gamma_of_q, syndrome_noise, syndrome_noise_seeds
from test_mbp4_reference_cpu import ALPHAS

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
SEED = 0x5EED
Q = 0.05
# steane at q = 0.05: its six checks of four qubits under gamma = log(19) never estimate a flip in the fixed batch (counted on the
# restatement: 39 solved, 1 unsolved, no u_hat); at 0.15 the batch holds 37 / 3 / 24
Q_OF = {"steane": 0.15}
LDS_BUDGET = TGD.LDS_BUDGET
P_OF = TGD.P_OF
CN_TYPES = TGD.CN_TYPES
informed_edge_channel, instantiation = TGD.informed_edge_channel, TGD.instantiation  # the dispatch rule is BP4-GD's
GAMMA_EDGE = np.array([0.0, 1e-3, 20.0, 25.0, INF, -0.7, -2.0], F32)
OUT = ("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats")


def tables(alphas, base=0.8):
    return MB.mbp4_tables(alphas, base)


def noisy(og, p, B, first=0, q=Q):
    """Depolarizing noise of the seeded stream, its syndromes with flips of rate q: (ex, ez, sx ^ ux, sz ^ uz, ux, uz)."""
    ex, ez, sx, sz = TGD.noisy(og, p, B, first)
    ux, uz = syndrome_noise(og, SEED, q, first, B)
    return ex, ez, sx ^ ux, sz ^ uz, ux, uz


def gamma_arrays(og, B, seed):
    """Per-check syndrome LLRs [B,m_x], [B,m_z]: moderate values around log((1-q)/q) with, on one entry in eight, an edge value: 0,
    small, the min-sum clip and beyond it, +inf and a few negatives."""
    rng = np.random.RandomState(seed)
    out = []
    for m in (og.m_x, og.m_z):
        g = rng.uniform(1.0, 5.0, size=(B, m)).astype(F32)
        edge = rng.rand(B, m) < 0.125
        g[edge] = GAMMA_EDGE[rng.randint(len(GAMMA_EDGE), size=int(edge.sum()))]
        out.append(g)
    return dict(synd_llr_x=out[0], synd_llr_z=out[1])


def scalar_gamma(q=Q):
    return dict(gamma_x=gamma_of_q(q), gamma_z=gamma_of_q(q))


def both(name, g, sx, sz, factors, owns, pre, att, cn_type="minsum", restart=True, ref=None, gam=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, u_x_hat, u_z_hat,
    stats).  `gam`: the syndrome LLRs, arrays or scalars (default: the scalar of q); `ref`: a restatement result to compare with."""
    gam = scalar_gamma() if gam is None else gam
    dev = {k: (to_gpu(v) if isinstance(v, np.ndarray) else v) for k, v in {**llr, **gam}.items()}
    got = g.dsbp4_decode(to_gpu(sx), to_gpu(sz), factors, owns, pre, att, cn_type, restart=restart, **dev)
    want = ref or DS.dsbp4_decode(code(name), sx, sz, factors, owns, pre, att, cn_type, restart=restart, **llr, **gam)
    assert [t.dtype for t in got] == [torch.uint8] * 4 + [torch.int32]
    s0, s1 = want[4], got[4].cpu().numpy()
    print(name, cn_type, "restart", restart, "found", s0[:, 0].tolist(), "a", s0[:, 1].tolist(), "k", s0[:, 3].tolist(), "u_hat",
          (want[2].sum(1) + want[3].sum(1)).tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    for label, w, t in zip(OUT[:4], want, got):
        a = t.cpu().numpy()
        assert a.shape == w.shape and w.tobytes() == a.tobytes(), (label, np.nonzero((w != a).any(1))[0])
    return want


def outcomes(ref):
    """(solved, unsolved, samples with a non-zero u_hat) of a restatement result."""
    solved = ref[4][:, 0] > 0
    return int(solved.sum()), int((~solved).sum()), int((ref[2].any(1) | ref[3].any(1)).sum())


def fuzz(name, g, og, rng, cn_types=("minsum",)):
    """B in 1..70, pre_iter and attempt_iter <= 12; one attempt with own = 1, three descending alphas with restart, five seeded weights
    and factors (own above 1 and own = 0 among them) without; a constant prior and per-qubit LLRs with edge values; gamma as a scalar
    and as per-check arrays with edge values.  Then the fixed batch of 40 samples under the default alphas with short attempts."""
    p, q = P_OF[name], Q_OF.get(name, Q)
    for cn in cn_types:
        for (factors, owns), restart in ((tables((1.0,), 1.0), False), (tables((1.0, 0.8, 0.6)), True),
                                        ((rng.uniform(0.4, 1.3, 5).astype(F32), np.array([1.0, 0.0, 1.25, 0.7, 0.45], F32)), False)):
            B, pre, att = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            ex, ez, sx, sz, _, _ = noisy(og, p, B, first=int(rng.randint(1 << 20)), q=q)
            both(name, g, sx, sz, factors, owns, pre, att, cn, restart, gam=scalar_gamma(q), llr_const=llr_const(p))
            both(name, g, sx, sz, factors, owns, pre, att, cn, restart, gam=gamma_arrays(og, B, int(rng.randint(1 << 30))),
                 llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))))
        fixed_batch(name, g, cn)


def fixed_batch_reference(name, cn):
    """The restatement on 40 seeded samples under the default alphas, 6 then 4 iterations: scalar gamma with restart off and on, then
    per-check gammas.  Asserts that the batch holds non-zero u_hat and both solved and unsolved samples."""
    og, c, p, q = oracle_library_forms(name), code(name), P_OF[name], Q_OF.get(name, Q)
    _, _, sx, sz, _, _ = noisy(og, p, 40, q=q)
    cases = [dict(restart=False, gam=scalar_gamma(q)), dict(restart=True, gam=scalar_gamma(q)), dict(restart=True, gam=gamma_arrays(og, 40, 77))]
    refs = []
    for kw in cases:
        ref = DS.dsbp4_decode(c, sx, sz, *tables(ALPHAS), 6, 4, cn, restart=kw["restart"], llr_const=llr_const(p), **kw["gam"])
        solved, unsolved, flagged = outcomes(ref)
        print(name, cn, "solved", solved, "unsolved", unsolved, "samples with u_hat != 0", flagged)
        assert solved > 0 and unsolved > 0 and flagged > 0, "the batch must hold solved and unsolved samples and non-zero u_hat"
        refs.append(ref)
    return sx, sz, cases, refs


def fixed_batch(name, g, cn):
    sx, sz, cases, refs = fixed_batch_reference(name, cn)
    for kw, ref in zip(cases, refs):
        both(name, g, sx, sz, *tables(ALPHAS), 6, 4, cn, kw["restart"], ref=ref, gam=kw["gam"], llr_const=llr_const(P_OF[name]))


# ---- 1-3: both kinds of instantiation, all three check rules ------------------------------------------------------------------------------
def test_regular_instantiation():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    info = g.info()
    assert (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6) and instantiation(g) == (3, 6)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"ds-ibm72")))


def test_force_generic_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    g.force_generic(True)
    try:
        fuzz("ibm72", g, og, np.random.RandomState(19))
    finally:
        g.force_generic(False)


@pytest.mark.parametrize("cn_type", ["boxplus", "boxplus-phi"])
def test_the_two_other_rules_on_a_regular_graph(cn_type):
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"ds-ibm72" + cn_type.encode())), cn_types=(cn_type,))


@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb126"])
def test_loop_instantiation(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g) == (0, 0)
    fuzz(name, g, og, np.random.RandomState(zlib.crc32(b"ds-" + name.encode())))


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_loop_instantiation_toric4(cn_type):
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("toric4", g, og, np.random.RandomState(zlib.crc32(b"ds-toric4" + cn_type.encode())), cn_types=(cn_type,))


# ---- 4: several codewords per workgroup -------------------------------------------------------------------------------------------------
WG_ALPHAS = tuple(np.linspace(1.0, 0.3, 12).tolist())


@pytest.mark.parametrize("restart", [False, True])
def test_codewords_of_one_workgroup_stop_at_different_attempts(restart):
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    L = llr_const(P_OF["rsurf5"])
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, sx, sz, _, _ = noisy(og, P_OF["rsurf5"], B)  # the same first rows for every B
        ref = both("rsurf5", g, sx, sz, *tables(WG_ALPHAS), 4, 3, "minsum", restart, llr_const=L)
        first = ref[4][:cpb - 1]  # samples of the first workgroup
        assert len(set(first[:, 1].tolist())) >= 3, "the workgroup's samples must stop at different attempts"
        assert (first[:, 0] == 1).any() and (ref[2][:cpb - 1].any() or ref[3][:cpb - 1].any())


# ---- 5: launch geometries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tpc,cpb", [(1, 64), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    """One thread per codeword owns every check (the syndrome LLRs are then read again in every step), and 64 threads own at most one."""
    g, og = gpu_graph("rsurf5"), oracle_library_forms("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        _, _, sx, sz, _, _ = noisy(og, P_OF["rsurf5"], cpb + 3, first=100)
        for restart, gam in ((False, None), (True, gamma_arrays(og, cpb + 3, 5))):
            ref = both("rsurf5", g, sx, sz, *tables(WG_ALPHAS), 4, 3, "minsum", restart, gam=gam, llr_const=llr_const(P_OF["rsurf5"]))
            assert (ref[4][:, 1] > 0).any() and outcomes(ref)[2] > 0
    finally:
        g.set_launch(0, 0)


# ---- 6-8: LDS and the packed rows -------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    """ghp1270 with two codewords per workgroup (128 threads each, ten checks per lane), on the (3,3,6) instantiation."""
    g, og = gpu_graph("ghp1270"), oracle_library_forms("ghp1270")
    assert instantiation(g) == (3, 6)
    E, m = og.E_x + og.E_z, og.m_x + og.m_z
    assert DS.dsbp4_lds_bytes(E, og.n, m, 1) <= 48 * 1024 < DS.dsbp4_lds_bytes(E, og.n, m, 2) <= LDS_BUDGET
    g.set_launch(128, 2)
    try:
        _, _, sx, sz, _, _ = noisy(og, 0.08, 3, q=0.01)
        ref = both("ghp1270", g, sx, sz, *tables((1.0, 0.8, 0.6)), 4, 3, gam=scalar_gamma(0.01), llr_const=llr_const(0.08))
        assert (ref[4][:, 1] > 0).any() and outcomes(ref)[2] > 0
    finally:
        g.set_launch(0, 0)


def test_packed_rows_above_32k():
    """bb1800: (3,3,6)-regular with packed slot offsets up to 43 196.  Then the loop on the same inputs, against the same reference."""
    g, og = gpu_graph("bb1800"), oracle_library_forms("bb1800")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    assert DS.dsbp4_lds_bytes(og.E_x + og.E_z, og.n, og.m_x + og.m_z, 1) <= LDS_BUDGET
    _, _, sx, sz, _, _ = noisy(og, 0.05, 4, q=0.01)
    gam = gamma_arrays(og, 4, 3)
    ref = both("bb1800", g, sx, sz, *tables((1.0, 0.8, 0.6)), 6, 3, gam=gam, llr_const=llr_const(0.05))
    assert (ref[4][:, 1] > 0).any() and outcomes(ref)[2] > 0
    g.force_generic(True)
    try:
        both("bb1800", g, sx, sz, *tables((1.0, 0.8, 0.6)), 6, 3, ref=ref, gam=gam, llr_const=llr_const(0.05))
    finally:
        g.force_generic(False)


def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    need = DS.dsbp4_lds_bytes(g.E_x + g.E_z, g.n, g.m_x + g.m_z, 1)
    assert need > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS.*{need} bytes.*limit is {LDS_BUDGET}"):
        g.dsbp4_decode(sx, sz, [0.8, 1.0], [1.0, 0.8], 3, 3, llr_const=2.0, gamma_x=3.0, gamma_z=3.0)


# ---- 9: syndromes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    B = 9
    zx, zz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    factors, owns = tables((1.0, 0.7))
    gam = dict(gamma_x=3.0, gamma_z=2.0)
    ref = both(name, g, zx, zz, factors, owns, 6, 5, gam=gam, llr_const=2.0)
    assert not any(a.any() for a in ref[:4]) and np.array_equal(ref[4], np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1)))
    got = g.dsbp4_decode(None, None, factors, owns, 6, 5, llr_const=2.0, B=B, **gam)
    assert not any(bool(t.any()) for t in got[:4]) and np.array_equal(got[4].cpu().numpy(), ref[4])


# ---- 10: perfect measurements ------------------------------------------------------------------------------------------------------------------
def test_minsum_with_perfect_measurements_is_mbp4_on_the_gpu():
    g = gpu_graph("ghp882")
    assert instantiation(g) == (3, 6)
    B, p = 8, 0.10
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    llr = to_gpu(informed_edge_channel(ex.cpu().numpy(), ez.cpu().numpy(), 5))
    for launch in ((0, 0), (256, 1)):
        g.set_launch(*launch)
        try:
            for kw in (dict(llr_const=llr_const(p)), dict(llr_ch=llr)):
                for alphas, restart in (((1.0,), True), (ALPHAS, True), (ALPHAS, False)):
                    x0, z0, s0 = g.mbp4_decode(sx, sz, *tables(alphas), 12, 5, "minsum", restart=restart, **kw)
                    xh, zh, ux, uz, st = g.dsbp4_decode(sx, sz, *tables(alphas), 12, 5, "minsum", restart=restart, **kw)
                    assert torch.equal(xh, x0) and torch.equal(zh, z0) and torch.equal(st, s0) and not ux.any() and not uz.any()
            assert (s0[:, 0] == 1).any()
        finally:
            g.set_launch(0, 0)


# ---- 11: guard bands ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_generic", [False, True], ids=["regular", "loop"])
def test_outputs_between_guards(force_generic):
    """Every output of the entry point, the two u_hat arrays included, is a poisoned payload between two guards: no byte is written
    outside, none is left stale.  Six codewords, one per workgroup; two of them are solved and leave early."""
    name = "ibm72"
    g, og = gpu_graph(name), oracle_library_forms(name)
    B = 6
    _, _, sx, sz, _, _ = noisy(og, P_OF[name], B)
    gam = gamma_arrays(og, B, 21)
    ref = DS.dsbp4_decode(code(name), sx, sz, *tables(ALPHAS[:3]), 6, 4, "minsum", llr_const=llr_const(P_OF[name]), **gam)
    assert 0 < int(ref[4][:, 0].sum()) < B, "codewords must leave the kernel solved and unsolved"
    dsx, dsz, dgam = to_gpu(sx), to_gpu(sz), {k: to_gpu(v) for k, v in gam.items()}
    keep = [t.clone() for t in (dsx, dsz, dgam["synd_llr_x"], dgam["synd_llr_z"])]
    g.force_generic(force_generic)
    try:
        assert instantiation(g, force_generic=force_generic) == ((0, 0) if force_generic else (3, 6))
        with guarded(g) as guard:
            got = g.dsbp4_decode(dsx, dsz, *tables(ALPHAS[:3]), 6, 4, "minsum", llr_const=llr_const(P_OF[name]), **dgam)
            guard.label(dict(zip(OUT, got)))
            assert len(guard.records) == 5, "all five outputs come from the allocator"
            guard.check()
            for label, t in zip(OUT, got):
                guard.assert_written(t, label)
    finally:
        g.force_generic(False)
    for label, w, t in zip(OUT, ref, got):
        assert np.array_equal(w, t.cpu().numpy()), label
    for before, after in zip(keep, (dsx, dsz, dgam["synd_llr_x"], dgam["synd_llr_z"])):
        assert before.view(torch.uint8).equal(after.view(torch.uint8)), "the inputs are read only"


# ---- 12-13: arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, cn_type="sum-product")
    for count in (0, 65):
        with pytest.raises(ValueError, match="num_attempts"):
            g.dsbp4_decode(sx, sz, [0.8] * count, [1.0] * count, 2, 2)
    with pytest.raises(ValueError, match="same length"):
        g.dsbp4_decode(sx, sz, [0.8, 0.9], [1.0], 2, 2)
    for pre, att in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            g.dsbp4_decode(sx, sz, [0.8], [1.0], pre, att)
    with pytest.raises(ValueError, match="restart"):
        g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, restart=2)
    for f in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="factor"):
            g.dsbp4_decode(sx, sz, [0.8, f], [1.0, 1.0], 2, 2)
    for o in (-0.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="own"):
            g.dsbp4_decode(sx, sz, [0.8, 0.8], [1.0, o], 2, 2)
    for kw in (dict(gamma_x=float("nan")), dict(gamma_z=float("nan"))):
        with pytest.raises(ValueError, match="NaN"):
            g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, **kw)
    with pytest.raises(ValueError, match="synd_x"):
        g.dsbp4_decode(sx[:, :-1].contiguous(), sz, [0.8], [1.0], 2, 2)
    with pytest.raises(ValueError, match="synd_z"):
        g.dsbp4_decode(sx, sz.to(torch.int32), [0.8], [1.0], 2, 2)
    with pytest.raises(ValueError, match="llr_ch"):
        g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="synd_llr_x"):
        g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, synd_llr_x=torch.zeros((2, g.m_x + 1), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="synd_llr_z"):
        g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2, synd_llr_z=torch.zeros((2, g.m_z), dtype=torch.float64, device=g.device))
    with pytest.raises(ValueError, match="B is needed"):
        g.dsbp4_decode(None, None, [0.8], [1.0], 2, 2)
    # the C entry point itself: a table or an output buffer missing, a NaN scalar
    xh, zh = (torch.zeros((2, n), dtype=torch.uint8, device=g.device) for _ in range(2))
    ux, uz = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device), torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    st = torch.zeros((2, 4), dtype=torch.int32, device=g.device)
    tab = np.array([0.8], F32)

    def call(factor, own, ux_ptr, stats, gamma_x=3.0):
        return _lib.lib().fgnn_dsbp4_decode(g.handle, 2, 1, factor, own, 2, 2, 1, None, 2.0, sx.data_ptr(), sz.data_ptr(), None, gamma_x, None,
                                            3.0, 2, xh.data_ptr(), zh.data_ptr(), ux_ptr, uz.data_ptr(), stats, None)

    t = tab.ctypes.data
    for args, word in (((None, t, ux.data_ptr(), st.data_ptr()), "factor and own"), ((t, None, ux.data_ptr(), st.data_ptr()), "factor and own"),
                       ((t, t, None, st.data_ptr()), "no output buffer"), ((t, t, ux.data_ptr(), None), "no output buffer"),
                       ((t, t, ux.data_ptr(), st.data_ptr(), float("nan")), "NaN")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(*args))
    _lib.check(call(t, t, ux.data_ptr(), st.data_ptr()))
    g.dsbp4_decode(sx, sz, [0.8, 0.8], [1.0, 0.0], 2, 2, gamma_x=-1.0, gamma_z=float("-inf"))  # own = 0 and negative gammas are allowed


def test_an_empty_batch_needs_no_buffers():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((0, g.m_z), dtype=torch.uint8, device=g.device)
    xh, zh, ux, uz, st = g.dsbp4_decode(sx, sz, [0.8], [1.0], 2, 2)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)
    assert tuple(ux.shape) == (0, g.m_x) and tuple(uz.shape) == (0, g.m_z)
    tab = np.array([0.8], F32)
    assert _lib.lib().fgnn_dsbp4_decode(g.handle, 2, 1, tab.ctypes.data, tab.ctypes.data, 2, 2, 1, None, 2.0, None, None, None, 3.0, None, 3.0,
                                        0, None, None, None, None, None, None) == 0


# ---- 14: the decoder class ----------------------------------------------------------------------------------------------------------------------
def test_soft_syndrome_decoder_class():
    import feedback_gnn_amd as F
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    n = og.n
    dec = F.SoftSyndromeBP4Decoder(c, alphas=(1.0, 0.8, 0.6), num_iter=6, graph=gpu_graph("ibm72"))
    assert (dec.alphas, dec.num_iter, dec.cn_type, dec.factor, dec.restart) == ((1.0, 0.8, 0.6), 6, "minsum", 0.8, True)
    default = F.SoftSyndromeBP4Decoder(c, graph=dec.graph)
    assert default.num_iter == 64 and default.alphas == (1.0,)
    f0, o0 = tables((1.0, 0.8, 0.6))
    assert dec.factors.tobytes() == f0.tobytes() and dec.owns.tobytes() == o0.tobytes()
    B = 40
    _, _, sx, sz, _, _ = noisy(og, P_OF["ibm72"], B)
    gam = gamma_arrays(og, B, 8)
    gam = {k: np.abs(v) for k, v in gam.items()}  # from_soft returns magnitudes
    # analog syndromes: the sign is the bit, the magnitude the LLR (a zero magnitude under a set bit would read as bit 0)
    soft_x = np.where(sx != 0, -np.maximum(gam["synd_llr_x"], F32(1e-3)), gam["synd_llr_x"]).astype(F32)
    soft_z = np.where(sz != 0, -np.maximum(gam["synd_llr_z"], F32(1e-3)), gam["synd_llr_z"]).astype(F32)
    bx, lx = dec.from_soft(to_gpu(soft_x))
    bz, lz = dec.from_soft(to_gpu(soft_z))
    assert bx.dtype == torch.uint8 and lx.dtype == torch.float32 and np.array_equal(bx.cpu().numpy(), sx) and np.array_equal(bz.cpu().numpy(), sz)
    assert np.array_equal(lx.cpu().numpy(), np.abs(soft_x)) and np.array_equal(lz.cpu().numpy(), np.abs(soft_z))
    L = llr_const(P_OF["ibm72"])
    want = DS.dsbp4_decode(c, sx, sz, f0, o0, 6, 6, "minsum", restart=True, llr_const=L, synd_llr_x=np.abs(soft_x), synd_llr_z=np.abs(soft_z))
    got = dec.decode(bx, bz, lx, lz, llr_const=L)
    for label, w, t in zip(OUT, want, got):
        assert np.array_equal(w, t.cpu().numpy()), label
    assert got[0].dtype == torch.uint8 and tuple(got[2].shape) == (B, og.m_x) and tuple(got[3].shape) == (B, og.m_z)
    assert dec.last_stats is got[4] and dec.last_u_x_hat is got[2] and dec.last_u_z_hat is got[3]
    solved, unsolved, flagged = outcomes(want)
    assert solved > 0 and unsolved > 0 and flagged > 0
    # a scalar gamma for both sides
    want_s = DS.dsbp4_decode(c, sx, sz, f0, o0, 6, 6, "minsum", restart=True, llr_const=L, gamma_x=2.5, gamma_z=2.5)
    got_s = dec.decode(bx, bz, gamma=2.5, llr_const=L)
    for label, w, t in zip(OUT, want_s, got_s):
        assert np.array_equal(w, t.cpu().numpy()), label
    # the reference's layout: syndromes and their LLRs as [m, bs]
    llr = np.full((B, 3, n), L, F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy()), lx.t().contiguous(), lz.t().contiguous()))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, n) and tuple(z_hat.shape) == (B, n)
    assert np.array_equal(x_hat.cpu().numpy(), want[0]) and np.array_equal(z_hat.cpu().numpy(), want[1])
    assert np.array_equal(dec.last_stats.cpu().numpy(), want[4]) and np.array_equal(dec.last_u_x_hat.cpu().numpy(), want[2])
    x_inf, _ = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy()), None, None))  # no LLRs: perfect measurements
    x0, z0, s0 = MB.mbp4_decode(c, sx, sz, f0, o0, 6, 6, "minsum", restart=True, llr_ch=llr)
    assert np.array_equal(x_inf.cpu().numpy(), x0) and np.array_equal(dec.last_stats.cpu().numpy(), s0) and not dec.last_u_x_hat.any()
    for kw in (dict(num_iter=0), dict(num_iter=2.5), dict(alphas=()), dict(alphas=(1.0,) * 65), dict(alphas=(1.0, 0.0)), dict(alphas=(1.0, -0.5)),
               dict(alphas=(float("nan"),)), dict(factor=0.0), dict(factor=float("inf")), dict(cn_type="sum-product")):
        with pytest.raises(ValueError):
            F.SoftSyndromeBP4Decoder(c, graph=dec.graph, **kw)
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((to_gpu(llr.astype(np.float64)), to_gpu(sx.T.copy()), to_gpu(sz.T.copy()), None, None))
    with pytest.raises(ValueError, match="length n"):
        dec((to_gpu(llr[:, :, :-1].copy()), to_gpu(sx.T.copy()), to_gpu(sz.T.copy()), None, None))
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((to_gpu(llr), to_gpu(sx.copy()), to_gpu(sz.T.copy()), None, None))
    with pytest.raises(ValueError, match="syndrome LLRs must have shape"):
        dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy()), lx, None))


# ---- 15-17: the model ---------------------------------------------------------------------------------------------------------------------------
MODEL_Q = 0.02


def _model(rank=0, world_size=1, p0=None, q=MODEL_Q, q0=None):
    import feedback_gnn_amd as F
    c = code("ibm72")
    dec = F.SoftSyndromeBP4Decoder(c, alphas=(1.0, 0.8, 0.6), num_iter=6, graph=gpu_graph("ibm72"))
    return F.BP4_SoftSyndrome_Model(c, dec, q, p0=p0, q0=q0, seed=SEED, rank=rank, world_size=world_size), dec


def test_syndrome_noise_streams():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    ux, uz = g.syndrome_noise(SEED, 0.05, 7, 33)
    wx, wz = syndrome_noise(og, SEED, 0.05, 7, 33)
    assert ux.dtype == torch.uint8 and tuple(ux.shape) == (33, og.m_x) and tuple(uz.shape) == (33, og.m_z)
    assert np.array_equal(ux.cpu().numpy(), wx) and np.array_equal(uz.cpu().numpy(), wz) and wx.any() and wz.any()
    assert g.syndrome_noise_seeds(SEED) == syndrome_noise_seeds(SEED)
    ax, az = g.syndrome_noise(SEED, 0.05, 0, 40)  # indexed by global sample: rows 7 .. 39 of a longer draw
    assert torch.equal(ax[7:], ux) and torch.equal(az[7:], uz)


def test_bp4_soft_syndrome_model():
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    B, p = 40, P_OF["ibm72"]
    for p0, q0 in ((None, None), (0.05, 0.04)):
        model, dec = _model(p0=p0, q0=q0)
        assert model.gamma == gamma_of_q(MODEL_Q if q0 is None else q0)
        for call in range(2):  # the second batch decodes global samples B .. 2B - 1
            s_hat, ls_hat = model(B, p)
            ex, ez = model.last_noise_x.cpu().numpy(), model.last_noise_z.cpu().numpy()
            ux, uz = model.last_u_x.cpu().numpy(), model.last_u_z.cpu().numpy()
            got = [t.cpu().numpy() for t in (model.last_x_hat, model.last_z_hat, model.last_u_x_hat, model.last_u_z_hat, model.last_stats)]
            assert tuple(s_hat.shape) == (B, hz.shape[0] + hx.shape[0]) and tuple(ls_hat.shape) == (B, hxp.shape[0] + hzp.shape[0])
            ox, oz = og.pauli_noise(SEED, p, call * B, B)
            assert np.array_equal(ex, ox) and np.array_equal(ez, oz), "depolarizing noise of the seeded stream"
            wx, wz = syndrome_noise(og, SEED, MODEL_Q, call * B, B)
            assert np.array_equal(ux, wx) and np.array_equal(uz, wz), "syndrome flips of the two derived streams"
            sx, sz = og.syndrome(ex, ez)
            gq = gamma_of_q(MODEL_Q if q0 is None else q0)
            want = DS.dsbp4_decode(c, sx ^ ux, sz ^ uz, *tables((1.0, 0.8, 0.6)), 6, 6, llr_const=llr_const(p if p0 is None else p0),
                                   gamma_x=gq, gamma_z=gq)
            for label, w, t in zip(OUT, want, got):
                assert np.array_equal(w, t), (label, "s ^ u is what is decoded")
            assert dec.last_stats is model.last_stats and dec.last_u_x_hat is model.last_u_x_hat
            xd, zd = (ex ^ got[0]).astype(np.int64), (ez ^ got[1]).astype(np.int64)
            solved = got[4][:, 0] > 0
            res = np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1)
            assert np.array_equal(s_hat.cpu().numpy(), res)
            assert np.array_equal(ls_hat.cpu().numpy(), np.concatenate([xd @ hxp.T % 2, zd @ hzp.T % 2], axis=1))
            miss = np.concatenate([uz ^ got[3], ux ^ got[2]], axis=1)
            assert np.array_equal(res[solved], miss[solved]), "on a solved sample the residual syndrome is u ^ u_hat"
            assert solved.any() and (~solved).any() and (~miss[solved].any(1)).any()
            if q0 is None:  # under the matched gamma both batches hold a solved sample whose u_hat misses u
                assert miss[solved].any()
            assert model.last_num_unsolved == int((~solved).sum())
    quiet, _ = _model(q=0.0)  # no flips, perfect measurements: AMBP4 on the true syndromes
    quiet(B, p)
    assert quiet.gamma == INF and not quiet.last_u_x.any() and not quiet.last_u_z.any() and not quiet.last_u_x_hat.any()
    ex, ez = og.pauli_noise(SEED, p, 0, B)
    x0, z0, s0 = MB.mbp4_decode(c, *og.syndrome(ex, ez), *tables((1.0, 0.8, 0.6)), 6, 6, llr_const=llr_const(p))
    assert np.array_equal(quiet.last_x_hat.cpu().numpy(), x0) and np.array_equal(quiet.last_stats.cpu().numpy(), s0)
    import feedback_gnn_amd as F
    for kw in (dict(q=-0.1), dict(q=1.0), dict(q=0.1, q0=1.5)):
        with pytest.raises(ValueError):
            F.BP4_SoftSyndrome_Model(c, _model()[1], **kw)


def test_two_ranks_decode_as_one_process():
    B = 16
    one, m0, m1 = _model()[0], _model(0, 2)[0], _model(1, 2)[0]
    one(2 * B, P_OF["ibm72"])
    assert m0.next_sample_range(B) == (0, B) and m1.next_sample_range(B) == (B, 2 * B)
    m0(B, P_OF["ibm72"]), m1(B, P_OF["ibm72"])
    for attr in ("last_noise_x", "last_noise_z", "last_u_x", "last_u_z", "last_x_hat", "last_z_hat", "last_u_x_hat", "last_u_z_hat", "last_stats"):
        assert torch.equal(getattr(one, attr), torch.cat([getattr(m0, attr), getattr(m1, attr)])), attr
    assert m1.last_u_x.any() and m1.last_u_x_hat.any(), "the second shard must draw and estimate flips"


def test_sim_ber_drives_the_model():
    import feedback_gnn_amd as F
    model, _ = _model()
    flagged, bler = F.sim_ber(model, [0.12, 0.04], batch_size=64, max_mc_iter=3, verbose=False, early_stop=False, qldpc=True)
    st = F.sim_ber.last
    assert (np.asarray(st["num_blocks"]) == 64 * 3).all()
    assert len(flagged) == 2 and len(bler) == 2
    assert flagged[0] > flagged[1] >= 0 and bler[0] >= flagged[0], "more residual syndromes at the higher rate"
