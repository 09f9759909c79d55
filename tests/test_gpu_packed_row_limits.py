"""The kernels that read a check's edges as packed 16-bit rows, on rows that use the upper half of the 16-bit range and on both sides
of the limits that switch the rows off.

fgnn_graph_create hands the kernels `cslot16` / `cslot32` (byte offsets 4 * slot; uploaded when every degree is uniform, dc <= 8 and
4 E < 65 536) and `cvn16` (a check's qubits; dc uniform, dc <= 8, n < 65 536).  Every consumer unpacks them itself: fgnn_bp4.hip (the
(3,3,6) and (4,4,8) instantiations, the register-LLR NQ kernels through cslot32, the fused flag epilogue through cvn16), fgnn_bp2.hip,
fgnn_relay.hip, fgnn_relay4.hip, fgnn_bp4gd.hip (which also derives a qubit from an offset) and syndrome_kernel of fgnn_channel.hip.  The
zoo's largest regular code, ghp1270, ends at offset 30 476 and qubit 1269; a sign extension, a 15-bit assumption or a `short`
temporary would decode silently wrong above 32 767.  The synthetic codes of tests/helpers.py (tests/test_check_rows_limits_cpu.py holds
their tables) go up to offset 65 516 (bb2730) and qubit 65 534 (wide65535), and past each limit (bb2738, gb2048, side0_36_over,
wide65536), where the kernels must fall back to the CSR loop.

Everything is held to the CPU oracle, or to the restatements built on it, by exact equality: floats as bytes, decisions as bytes, stats
as int32; no tolerance, no sample left out.  A with-rows case decodes on the default path, with fgnn_graph_force_generic and on the
oracle, and all three agree; before decoding it asserts, from fgnn_graph_info and from fgnn_check_rows on the graph's own edges, that
the instantiation it is meant for is the one the host dispatches and that the largest packed offset it reads is >= 32 768.

Not reachable, and therefore not here:
  - the compile-time-trip NT kernels (first decoder, one constant LLR) need 256 threads per codeword and at most 5 trips, n <= 1280:
    their cslot32 offsets never pass 30 720;
  - fgnn_bp4_layered.hip reads no packed rows;
  - cvn16 entries above 32 767 in the BP4 fused flag epilogue: it runs in the NQ / NT kernels only (n <= 5 * 1024); the full range of
    cvn16 is read by syndrome_kernel (wide65535).

LDS: with two codewords per workgroup and per-qubit channel LLRs in LDS, BP4 refuses bb2730 and bb2738 (2 x 98 KB; the global-memory
variant takes one codeword per workgroup only): the refusal is asserted with its message, and bb1800 (2 x 65 KB) is the largest code of
the set that runs that geometry with per-qubit LLRs.  Every other decoder takes every code here."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_bp2_shapes as TB2
import test_gpu_bp4gd as TGD
import test_gpu_relay as TR
import test_gpu_relay4 as TR4
from feedback_gnn_amd import _lib
from helpers import WEIGHTS_882, code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_bp2_reference_cpu import _llr_const
from test_gpu_bp4_hot_loops import _channel_llrs, _eq
from test_gpu_bp4_shapes import CN_ID, LDS_BUDGET, bits_equal, bp4_variant
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

SEED = 0x5EED
RULES = ("boxplus-phi", "minsum", "boxplus")
FACTORS = (1.0, 0.8)
ITERS = (1, 16)
TOP = {"bb1800": 43196, "bb2730": 65516, "gb2000": 63996}  # the largest packed offset of the codes with slot rows
SIDE0_TOP = {"side0_36": 42332, "side0_48": 51196}        # ... of their side-0 rows, all that the binary decoders read


# ---- what the graph carries, from the library itself -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(name):
    """(have, cslot32 rows, cvn16 rows) of fgnn_check_rows on the edges fgnn_graph_edges reports for the GPU graph."""
    g = gpu_graph(name)
    (cx, vx), (cz, vz) = g.edges(0), g.edges(1)
    m = g.m_x + g.m_z
    have = (C.c_int32 * 2)()
    slot, qub = np.zeros((m, 8), np.uint32), np.zeros((m, 8), np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().fgnn_check_rows(g.n, g.m_x, g.m_z, len(cx), p(cx), p(vx), len(cz), p(cz), p(vz), have, p(slot), p(qub)))
    return list(have), slot, qub


@functools.lru_cache(maxsize=None)
def info(name):
    """fgnn_graph_info at the library's launch, with the max_vdeg bp4_variant asks for."""
    c = code(name)
    return dict(gpu_graph(name).info(), max_vdeg=int((c.hx.sum(0, dtype=np.int64) + c.hz.sum(0, dtype=np.int64)).max()))


def slot_rows_expected(name, with_rows, side0=False):
    """The precondition every decoder test shares: the slot rows are there (or not), the restated rule of the dispatch mirrors agrees
    with the library's own tables, and a with-rows code reads an offset in the upper half of the range."""
    have, slot, _ = rows(name)
    i = info(name)
    rule = i["dv_x"] > 0 and i["dv_z"] > 0 and 0 < i["dc"] <= 8 and 4 * (i["E_x"] + i["E_z"]) < 65536
    assert have[0] == int(with_rows) == int(rule), (name, have, rule)
    if with_rows:
        top = int(slot[:i["m_x"]].max()) if side0 else int(slot.max())
        assert top == (SIDE0_TOP if side0 else TOP)[name] and top >= 32768, (name, top)


# ---- BP4 ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bp4_inputs(name, B=3):
    """Syndromes of the seeded depolarizing stream at p = 0.08 (nothing saturates) and per-qubit LLRs; shared, nobody writes to them."""
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 700, B)
    return og.syndrome(ex, ez) + (_channel_llrs(B, og.n, 21),)


@functools.lru_cache(maxsize=None)
def bp4_oracle(name, cn, factor, iters, per_qubit):
    sx, sz, llr = bp4_inputs(name)
    chan = dict(llr_ch=llr) if per_qubit else dict(llr_const=llr_const(0.08))
    return oracle_library_forms(name).bp4_decode(sx, sz, iters, cn, factor, return_msgs=True, **chan)


def bp4_case(name, cn, launch, shape, lreg_of):
    """Every factor, iteration count, LLR kind and shortcut setting of one (code, rule, launch): default path, forced fallback, oracle.
    `shape` = the (DVX, DVZ, DC) the default path must dispatch, `lreg_of(per_qubit)` the NQ it must take under the phi rule."""
    gg = gpu_graph(name)
    i = info(name)
    with_rows = shape != (0, 0, 0)
    slot_rows_expected(name, with_rows)
    sx, sz, llr = bp4_inputs(name)
    B = sx.shape[0]
    tx, tz, tl = to_gpu(sx), to_gpu(sz), to_gpu(llr)
    refused = 0
    try:
        if launch:
            gg.set_launch(*launch)
        for per_qubit in (False, True):
            chan = dict(llr_ch=tl) if per_qubit else dict(llr_const=llr_const(0.08))
            for factor in FACTORS:
                for iters in ITERS:
                    o = bp4_oracle(name, cn, factor, iters, per_qubit)
                    for shortcut in (False, True):
                        for generic in ((False, True) if with_rows else (False,)):
                            v = bp4_variant(i, cn, B, iters, llr_ch=per_qubit, launch=launch, shortcut=shortcut, force_generic=generic)
                            what = f"{name} {cn} launch={launch} per_qubit={per_qubit} factor={factor} it={iters} shortcut={shortcut} generic={generic}"
                            gg.set_saturation_shortcut(shortcut)
                            gg.force_generic(generic)
                            if v["gmem"]:  # 2 x (E + 3n) floats: beyond the LDS, and the global-memory variant takes cpb = 1 only
                                assert v["cpb"] == 2 and per_qubit and name != "bb1800", what
                                with pytest.raises(_lib.FgnnError, match="global-memory BP4 variant needs one codeword per workgroup"):
                                    gg.bp4_decode(tx, tz, iters, cn, factor, return_msgs=True, **chan)
                                refused += 1
                                continue
                            assert v["kernel"][:4] == (CN_ID[cn],) + ((0, 0, 0) if generic else shape), (what, v)
                            if cn == "boxplus-phi" and not generic:
                                assert v["lreg"] == lreg_of(per_qubit), (what, v)
                            _eq(o, gg.bp4_decode(tx, tz, iters, cn, factor, return_msgs=True, **chan), what)
    finally:
        gg.force_generic(False)
        gg.set_saturation_shortcut(True)
        gg.set_launch(0, 0)
    return refused


# B = 3 at the library's launch (1024 threads: 2 or 3 qubits per thread, per-qubit LLRs in the registers of the NQ = 4 kernel, slots
# through cslot32), at (640, 1) (3 trips on bb1800: NQ = 4; 5 on bb2730: NQ = 5) and at (256, 2): cslot16 on a non-zero codeword base
BB_LAUNCHES = {"library": None, "640x1": (640, 1), "256x2": (256, 2)}
BB_LREG = {("bb1800", "library"): 4, ("bb2730", "library"): 4, ("bb1800", "640x1"): 4, ("bb2730", "640x1"): 5,
           ("bb1800", "256x2"): 0, ("bb2730", "256x2"): 0}


@pytest.mark.parametrize("launch", list(BB_LAUNCHES))
@pytest.mark.parametrize("cn", RULES)
@pytest.mark.parametrize("name", ["bb1800", "bb2730", "bb2738"])
def test_bp4_336(name, cn, launch):
    with_rows = name != "bb2738"  # bb2738: 4 E = 65 712, the default path is the fallback already
    if with_rows and launch != "256x2":
        n, tpc = info(name)["n"], 1024 if launch == "library" else 640
        assert (n + tpc - 1) // tpc == {"bb1800": (2, 3), "bb2730": (3, 5)}[name][launch == "640x1"]
    refused = bp4_case(name, cn, BB_LAUNCHES[launch], (3, 3, 6) if with_rows else (0, 0, 0),
                       lambda per_qubit: BB_LREG[name, launch] if (with_rows and per_qubit) else 0)
    # two codewords with per-qubit LLRs in LDS: bb1800 is the largest code that fits, the two others are refused (module docstring)
    i = info(name)
    two = 2 * 4 * ((i["E_x"] + i["E_z"] + 3 * i["n"] + 3) & ~3)
    assert (two > LDS_BUDGET) == (name != "bb1800")
    per_cell = 2 if with_rows else 1  # default and forced fallback
    assert refused == (len(FACTORS) * len(ITERS) * 2 * per_cell if (launch == "256x2" and name != "bb1800") else 0)


@pytest.mark.parametrize("cn", RULES)
@pytest.mark.parametrize("name", ["gb2000", "gb2048"])
def test_bp4_448(name, cn):
    with_rows = name == "gb2000"  # gb2048: 4 E = 65 536 exactly, the first size without slot rows
    assert bp4_case(name, cn, None, (4, 4, 8) if with_rows else (0, 0, 0), lambda per_qubit: 0) == 0


def test_bp4_logit_trace_on_bb2730():
    """The (3,3,6) trace variant (fixed dataflow, channel LLRs in LDS) on offsets up to 65 516: slot k of the soft syndromes and of the
    tape equals the oracle after k iterations, bit for bit, as tests/test_gpu_bp4_shapes.py and test_gpu_api.py hold the trace."""
    name, B, T, factor = "bb2730", 2, 3, 0.9
    gg, og = gpu_graph(name), oracle_library_forms(name)
    slot_rows_expected(name, True)
    sx, sz, llr = (a[:B] for a in bp4_inputs(name))
    v = bp4_variant(info(name), "boxplus-phi", B, T, llr_ch=True, trace=True)
    assert v["kernel"] == (CN_ID["boxplus-phi"], 3, 3, 6, False, 0, True, False, 2) and not v["gmem"]
    refs = [og.bp4_decode(sx, sz, k, "boxplus-phi", factor, llr_ch=llr, return_msgs=True) for k in range(T + 1)]
    for generic in (False, True):
        try:
            gg.force_generic(generic)
            tr = gg.bp4_logit_trace(to_gpu(llr), to_gpu(sx), to_gpu(sz), T, factor)
        finally:
            gg.force_generic(False)
        tr = {k: t.cpu().numpy() for k, t in tr.items()}
        for k, o in enumerate(refs):
            for got, want in (("x_logit", "x_logit"), ("z_logit", "z_logit"), ("tape_x", "msg_x"), ("tape_z", "msg_z")):
                assert bits_equal(tr[got][k], o[want]), (generic, k, got)
        assert bits_equal(tr["llr"], refs[-1]["llr"]) and np.array_equal(tr["x_hat"], refs[-1]["x_hat"])
        assert np.array_equal(tr["z_hat"], refs[-1]["z_hat"])


# ---- Relay-BP4 and BP4-GD ---------------------------------------------------------------------------------------------------------------
# Chosen on the restatements alone (CPU): depolarizing noise of the seeded stream, samples 0..5, at p = 0.05.  Relay-BP4 with 3 legs,
# pre_iter 6, leg_iter 4, stop_nconv 1: on each of the three codes at least one sample is not solved in leg 0 and enters leg 1.
# BP4-GD with pre_iter 6, round_iter 3, max_rounds 3: on each of them at least one sample is not solved before a qubit is fixed.
POST_P, POST_B = 0.05, 6
RELAY4 = dict(pre=6, leg=4, stop=1, legs=3, gamma_seed=1)
GD = dict(pre=6, rnd=3, rounds=3)
POST_CODES = {"bb1800": True, "bb2730": True, "bb2738": False}


@pytest.mark.parametrize("name", list(POST_CODES))
def test_relay4(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    with_rows = POST_CODES[name]
    slot_rows_expected(name, with_rows)
    assert TR4.instantiation(g) == ((3, 6) if with_rows else (0, 0)) and TR4.instantiation(g, force_generic=True) == (0, 0)
    assert TR4.relay4_lds_bytes(og.E_x + og.E_z, og.n, 1) <= LDS_BUDGET
    ex, ez, sx, sz = TR4.noisy(og, POST_P, POST_B)
    gamma = mixed_gamma(RELAY4["legs"], og.n, RELAY4["gamma_seed"])
    sched = (RELAY4["pre"], RELAY4["leg"], RELAY4["stop"], 0.8)
    for k, llr in enumerate((dict(llr_const=llr_const(POST_P)), dict(llr_ch=TR4.informed_edge_channel(ex[:3], ez[:3], 77)))):
        s = slice(None) if k == 0 else slice(0, 3)
        x0, z0, s0, _ = TR4.both(g, og, sx[s], sz[s], gamma, *sched, **llr)
        assert (s0[:, 2] > 0).any(), "a sample must enter a leg beyond the first"
        if with_rows:  # the fallback on the same inputs, against the same reference outputs
            gl = {kk: (to_gpu(v) if kk == "llr_ch" else v) for kk, v in llr.items()}
            try:
                g.force_generic(True)
                xh, zh, st = g.relay4_decode(to_gpu(sx[s]), to_gpu(sz[s]), to_gpu(gamma), *sched, **gl)
            finally:
                g.force_generic(False)
            assert np.array_equal(st.cpu().numpy(), s0)
            assert xh.cpu().numpy().tobytes() == x0.tobytes() and zh.cpu().numpy().tobytes() == z0.tobytes()


@pytest.mark.parametrize("name", list(POST_CODES))
def test_bp4gd(name):
    """A fixed qubit sends dec[((off >> 2) - base) / DV] through offsets up to 43 196 / 65 516."""
    g, og = gpu_graph(name), oracle_library_forms(name)
    with_rows = POST_CODES[name]
    slot_rows_expected(name, with_rows)
    assert TGD.instantiation(g) == ((3, 6) if with_rows else (0, 0)) and TGD.instantiation(g, force_generic=True) == (0, 0)
    assert TGD.bp4gd_lds_bytes(og.E_x + og.E_z, og.n, 1) <= LDS_BUDGET
    ex, ez, sx, sz = TGD.noisy(og, POST_P, POST_B)
    sched = (GD["pre"], GD["rnd"], GD["rounds"], 0.8)
    for k, llr in enumerate((dict(llr_const=llr_const(POST_P)), dict(llr_ch=TGD.informed_edge_channel(ex[:3], ez[:3], 77)))):
        s = slice(None) if k == 0 else slice(0, 3)
        x0, z0, s0, _ = TGD.both(g, og, sx[s], sz[s], *sched, **llr)
        assert (s0[:, 1] > 0).any(), "a sample must have a qubit fixed"
        if with_rows:
            gl = {kk: (to_gpu(v) if kk == "llr_ch" else v) for kk, v in llr.items()}
            try:
                g.force_generic(True)
                xh, zh, st = g.bp4gd_decode(to_gpu(sx[s]), to_gpu(sz[s]), GD["pre"], GD["rnd"], GD["rounds"], 25.0, "minsum", 0.8, **gl)
            finally:
                g.force_generic(False)
            assert np.array_equal(st.cpu().numpy(), s0)
            assert xh.cpu().numpy().tobytes() == x0.tobytes() and zh.cpu().numpy().tobytes() == z0.tobytes()


# ---- the binary decoders: side 0 only ---------------------------------------------------------------------------------------------------
# side0_36 / side0_48: hx offsets up to 42 332 / 51 196 with the rows present (4 E = 56 448 / 64 000); side0_36_over: 4 E = 73 728
SIDE0 = {"side0_36": (3, 6), "side0_48": (4, 8), "side0_36_over": None}


def side0_graphs(name):
    return gpu_graph(name), oracle_library_forms(name), code(name).hx


@pytest.mark.parametrize("cn", ["boxplus-phi", "minsum"])
@pytest.mark.parametrize("name", list(SIDE0))
def test_bp2(name, cn):
    g, og, hx = side0_graphs(name)
    shape = SIDE0[name]
    slot_rows_expected(name, shape is not None, side0=True)
    assert TB2.bp2_lds_bytes(og.E_x, 1) <= LDS_BUDGET
    assert TB2.instantiation(g, hx, cn) == ((cn,) + shape if shape else ("minsum", 0, 8) if cn == "minsum" else (cn, 0, 0))
    for factor in FACTORS:
        TB2.check(g, og, hx, 3, 9, cn, factor, 12, p=0.02)
        if shape:
            assert TB2.instantiation(g, hx, cn, force_generic=True)[1:] == ((0, 8) if cn == "minsum" else (0, 0))
            try:
                g.force_generic(True)
                TB2.check(g, og, hx, 3, 9, cn, factor, 12, p=0.02)
            finally:
                g.force_generic(False)


@pytest.mark.parametrize("name", list(SIDE0))
def test_relay(name):
    """BSC noise at p = 0.02, seed 11, B = 5, three legs of 6 / 4 / 4 iterations, stop_nconv 1: on the restatement alone, samples
    solved in leg 0 and samples that use every leg."""
    g, _, hx = side0_graphs(name)
    shape = SIDE0[name]
    slot_rows_expected(name, shape is not None, side0=True)
    assert TR.instantiation(g, hx) == (shape or (0, 8)) and TR.instantiation(g, hx, force_generic=True) == (0, 8)
    assert TR.relay_lds_bytes(int(hx.sum()), hx.shape[1], 1) <= LDS_BUDGET
    e, synd = TR.noisy(hx, 5, 0.02, 11)
    gamma = mixed_gamma(3, hx.shape[1], 4)
    for k, llr in enumerate((dict(llr_const=_llr_const(0.02)), dict(llr_ch=TR.informed_edge_channel(hx, e[:2], 5)))):
        s = slice(None) if k == 0 else slice(0, 2)
        h0, s0, _ = TR.both(g, hx, synd[s], gamma, 6, 4, 1, 0.8, **llr)
        assert (s0[:, 2] > 0).any(), "a sample must enter a leg beyond the first"
        if shape:
            gl = {kk: (to_gpu(v) if kk == "llr_ch" else v) for kk, v in llr.items()}
            try:
                g.force_generic(True)
                hard, st = g.relay_decode(to_gpu(synd[s]), to_gpu(gamma), 6, 4, 1, 0.8, **gl)
            finally:
                g.force_generic(False)
            assert np.array_equal(st.cpu().numpy(), s0) and np.array_equal(hard.cpu().numpy(), h0)


# ---- the byte kernels: qubit rows near 2^16 ---------------------------------------------------------------------------------------------
def wide_noise(n, seed):
    """B = 3 rows: qubit n - 1 alone, all of [32 768, n), and seeded random bytes with qubit n - 1 set."""
    rng = np.random.RandomState(seed)
    e = np.zeros((3, n), np.uint8)
    e[0, n - 1] = 1
    e[1, 32768:] = 1
    e[2] = rng.rand(n) < 0.3
    e[2, n - 1] = 1
    return e


@pytest.mark.parametrize("name", ["wide65535", "wide65536"])
def test_syndrome_flag_and_residual_on_qubits_up_to_n_minus_1(name):
    """fgnn_syndrome reads cvn16 at n = 65 535 (entries up to 65 534, half of them >= 32 768) and the CSR tables at n = 65 536;
    fgnn_flag_update and fgnn_residual run beside it on the same graphs.  All against int64 NumPy products."""
    c, g = code(name), gpu_graph(name)
    n = g.n
    hx, hz = c.hx.astype(np.int64), c.hz.astype(np.int64)
    have, _, qub = rows(name)
    i = info(name)
    assert have == [0, int(n < 65536)] == [0, int(0 < i["dc"] <= 8 and n < 65536)]
    if have[1]:
        assert int(qub.max()) == 65534 and int((qub >= 32768).sum()) == 128  # half of the 256 entries
    ex, ez = wide_noise(n, 3), wide_noise(n, 4)[::-1].copy()
    want_sx, want_sz = (ez @ hx.T % 2).astype(np.uint8), (ex @ hz.T % 2).astype(np.uint8)
    assert want_sx.any() and want_sz.any() and not want_sx.all()
    for generic in ((False, True) if have[1] else (False,)):
        try:
            g.force_generic(generic)
            sx, sz = g.syndrome(to_gpu(ex), to_gpu(ez))
        finally:
            g.force_generic(False)
        assert np.array_equal(sx.cpu().numpy(), want_sx) and np.array_equal(sz.cpu().numpy(), want_sz), (name, generic)
    # flag_update: errors &= (the estimate's syndrome differs from the measured one); sample 0 reproduces it, 1 and 2 do not, and
    # sample 2 enters unflagged
    xh, zh = wide_noise(n, 5), wide_noise(n, 6)[::-1].copy()
    msx, msz = (zh @ hx.T % 2).astype(np.uint8), (xh @ hz.T % 2).astype(np.uint8)
    msx[1, 15] ^= 1  # hx row 15 holds qubit n - 1
    msz[2, 0] ^= 1
    errors = to_gpu(np.array([1, 1, 0], np.uint8))
    g.flag_update(to_gpu(xh), to_gpu(zh), to_gpu(msx), to_gpu(msz), errors)
    assert errors.cpu().numpy().tolist() == [0, 1, 0]
    # residual: s_hat = [hz xd ; hx zd], ls_hat = the all-zero hx_perp / hz_perp rows, flags = bit 0 any(s_hat)
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    want_s = np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1).astype(np.uint8)
    s_hat, ls_hat, flags = g.residual(to_gpu(ex), to_gpu(ez), to_gpu(xh), to_gpu(zh))
    assert np.array_equal(s_hat.cpu().numpy(), want_s) and not ls_hat.cpu().numpy().any()
    assert np.array_equal(flags.cpu().numpy(), want_s.any(1).astype(np.uint8)) and want_s.any()


def test_syndrome_on_bb2730():
    c, g = code("bb2730"), gpu_graph("bb2730")
    have, _, qub = rows("bb2730")
    assert have[1] == 1 and int(qub.max()) == g.n - 1
    rng = np.random.RandomState(11)
    ex, ez = ((rng.rand(3, g.n) < 0.3).astype(np.uint8) for _ in range(2))
    want_sx = (ez.astype(np.int64) @ c.hx.T.astype(np.int64) % 2).astype(np.uint8)
    want_sz = (ex.astype(np.int64) @ c.hz.T.astype(np.int64) % 2).astype(np.uint8)
    for generic in (False, True):
        try:
            g.force_generic(generic)
            sx, sz = g.syndrome(to_gpu(ex), to_gpu(ez))
        finally:
            g.force_generic(False)
        assert np.array_equal(sx.cpu().numpy(), want_sx) and np.array_equal(sz.cpu().numpy(), want_sz), generic


# ---- the sandwich driver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch,iters", [((256, 1), [3, 8]), ((640, 1), [3, 4, 4])], ids=["256x1-two-stages", "640x1-three-stages"])
def test_sandwich_on_bb2730(launch, iters):
    """The driver with the shipped [[882,24]] weights on bb2730, every second sample noiseless (it leaves after the first decoder), one
    codeword per workgroup, so the decoders' epilogues write the flags.  At (256, 1) a thread owns 11 qubits: both decoders run the
    runtime-trip (3,3,6) kernels on cslot16 and the flag test walks the CSR tables.  The fused flag test reads cvn16 rows in the NQ
    kernels only, and its flag is used only when another round follows: three stages at (640, 1) make the second decoder the NQ = 5
    kernel (offsets through cslot32) and have the third round depend on the flag it formed from cvn16."""
    from feedback_gnn_amd.graph import GnnWeights
    from feedback_gnn_amd.weights_io import read_weight_list
    name, B, p = "bb2730", 6, 0.05
    gg, og = gpu_graph(name), oracle_library_forms(name)
    slot_rows_expected(name, True)
    assert rows(name)[0] == [1, 1]
    i = info(name)
    first = bp4_variant(i, "boxplus-phi", B, iters[0], launch=launch, flagged=True)
    later = bp4_variant(i, "boxplus-phi", B, iters[1], llr_ch=True, launch=launch, flagged=len(iters) > 2)
    assert first["kernel"][1:4] == later["kernel"][1:4] == (3, 3, 6) and first["cpb"] == 1 and first["lreg"] == 0
    assert later["lreg"] == (5 if launch == (640, 1) else 0)
    w = read_weight_list(WEIGHTS_882)
    ex, ez = og.pauli_noise(SEED, p, 900, B)
    ex, ez = ex.copy(), ez.copy()
    ex[::2], ez[::2] = 0, 0
    sx, sz = og.syndrome(ex, ez)
    L0 = llr_const(p)
    ws = [w] * (len(iters) - 1)
    o = og.sandwich_decode(sx, sz, iters, ws, L0, return_llr=True)
    assert not o["rounds"][::2].any() and o["rounds"][1::2].all(), o["rounds"].tolist()
    gw = GnnWeights(w, gg.device)
    for generic in (False, True):
        try:
            gg.set_launch(*launch)
            gg.force_generic(generic)
            got = gg.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw] * len(ws), L0, return_llr=True, return_rounds=True)
        finally:
            gg.force_generic(False)
            gg.set_launch(0, 0)
        assert np.array_equal(o["rounds"], got["rounds"].cpu().numpy()), generic
        assert o["x_hat"].tobytes() == got["x_hat"].cpu().numpy().tobytes() and o["z_hat"].tobytes() == got["z_hat"].cpu().numpy().tobytes()
        assert o["llr"].tobytes() == got["llr"].cpu().numpy().tobytes(), generic
