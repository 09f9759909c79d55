"""The layered (serial) schedule of binary BP on the CPU: the host half of the feature (fgnn_greedy_bit_layers,
fgnn_validate_bit_layers), the restatement tests/bp2_layered_reference.py held to a float64 restatement of the same schedule and to the
oracle's flooding decoder at zero iterations, a pinned sanity check of what the schedule buys, and the build surface (header, library
export, public classes).  No GPU.  That a refused layering keeps the installed one needs a graph handle, and a handle needs a device:
tests/test_gpu_bp2_layered.py checks it."""
import ctypes
import os
import re

import numpy as np
import pytest

import bp2_layered_reference as BR
from helpers import binary_oracle, code, oracle_library_forms
from oracle import numpy_ref as R
from test_bp2_reference_cpu import _channel, _llr_const, _tol, degenerate_hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RULES = ("boxplus-phi", "minsum", "boxplus")
CODES = ("steane", "rsurf5", "gb48", "hp_c7", "ibm72", "ghp882", "gb126")
NEW_SYMBOLS = ("fgnn_greedy_bit_layers", "fgnn_validate_bit_layers", "fgnn_graph_set_bit_layers", "fgnn_graph_bit_layers",
               "fgnn_bp2_decode_layered")


def hx_of(name):
    return degenerate_hx() if name == "degenerate" else np.asarray(code(name).hx)


def _edges(hx):
    hx = np.asarray(hx)
    r, c = np.nonzero(hx)
    r, c = np.ascontiguousarray(r, np.int32), np.ascontiguousarray(c, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return (hx.shape[1], hx.shape[0], len(r), ptr(r), ptr(c)), (r, c)


def lib_greedy(hx):
    from feedback_gnn_amd import _lib
    args, _keep = _edges(hx)
    lay = np.full(args[1], -7, np.int32)
    num = ctypes.c_int32(-1)
    _lib.check(_lib.lib().fgnn_greedy_bit_layers(*args, lay.ctypes.data_as(ctypes.c_void_p), ctypes.byref(num)))
    return int(num.value), lay


def lib_validate(hx, num_layers, layer_of):
    """(return code, message) of fgnn_validate_bit_layers."""
    from feedback_gnn_amd import _lib
    args, _keep = _edges(hx)
    lay = np.ascontiguousarray(layer_of, np.int32)
    rc = _lib.lib().fgnn_validate_bit_layers(*args, int(num_layers), lay.ctypes.data_as(ctypes.c_void_p))
    return rc, _lib.lib().fgnn_last_error().decode()


# ---- layers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES + ("degenerate",))
def test_greedy_bit_layers_of_the_library_are_the_python_greedy_and_valid(name):
    hx = hx_of(name)
    num, lay = lib_greedy(hx)
    num_py, lay_py = BR.greedy_bit_layers(hx)
    assert num == num_py and np.array_equal(lay, lay_py)
    assert BR.is_valid_bit_layering(hx, num, lay)
    assert lib_validate(hx, num, lay)[0] == 0


def test_greedy_bit_layer_counts_of_known_codes():
    """From the restatement: hx of [[882,24]] alone takes 9 layers of 3 to 91 checks (13 with hz), hx of ibm72 4 layers of 9."""
    counts = {name: BR.greedy_bit_layers(hx_of(name))[0] for name in CODES + ("degenerate",)}
    assert counts == dict(steane=3, rsurf5=2, gb48=8, hp_c7=8, ibm72=4, ghp882=9, gb126=14, degenerate=4)
    num, lay = lib_greedy(hx_of("ghp882"))
    sizes = np.bincount(lay, minlength=num)
    assert num == 9 and sizes.min() == 3 and sizes.max() == 91 and sizes.sum() == 441
    num, lay = lib_greedy(hx_of("ibm72"))
    assert num == 4 and np.bincount(lay).tolist() == [9] * 4
    num, lay = lib_greedy(hx_of("steane"))  # every two checks of the Hamming matrix share a bit
    assert num == 3 and lay.tolist() == [0, 1, 2]
    assert lib_greedy(degenerate_hx())[1].tolist() == [0, 0, 1, 2, 2, 0, 3]


def test_validation_names_the_cause():
    hx = hx_of("steane")
    one_each = np.arange(3, dtype=np.int32)
    assert lib_validate(hx, 3, one_each)[0] == 0
    # two checks of one layer and the bit they share
    v = int(np.nonzero(hx[0] & hx[1])[0][0])
    rc, msg = lib_validate(hx, 2, np.array([0, 0, 1], np.int32))
    assert rc == -1 and "check 0 and check 1 of layer 0" in msg and f"share bit {v}" in msg and "hx" not in msg and "qubit" not in msg
    # an empty layer
    rc, msg = lib_validate(hx, 4, np.array([0, 1, 3], np.int32))
    assert rc == -1 and "layer 2 is empty" in msg
    # out of range, above and below
    rc, msg = lib_validate(hx, 3, np.array([0, 1, 3], np.int32))
    assert rc == -1 and "check 2 has layer 3" in msg and "[0, 3)" in msg
    rc, msg = lib_validate(hx, 3, np.array([0, -1, 2], np.int32))
    assert rc == -1 and "check 1 has layer -1" in msg
    rc, msg = lib_validate(hx, 0, one_each)
    assert rc == -1 and "num_layers" in msg
    # a disjoint pair may share a layer: rsurf5's greedy layering is valid, with its two layers merged it is not
    hx = hx_of("rsurf5")
    num, lay = lib_greedy(hx)
    assert num == 2 and lib_validate(hx, 1, np.zeros(hx.shape[0], np.int32))[0] == -1
    assert not BR.is_valid_bit_layering(hx, 1, np.zeros(hx.shape[0], np.int32))
    # checks that hx and hz would make collide are no concern of this layering: hx of steane twice over is refused by the BP4 rules
    # (fgnn_validate_layers) and never seen here
    assert lib_validate(hx_of("steane"), 3, np.array([2, 1, 0], np.int32))[0] == 0


# ---- the restatement against float64 -----------------------------------------------------------------------------------------------------
def layered64(hx, synd, num_iter, cn_type, factor, layer_of, llr_ch=None, llr_const=None):
    """The schedule of fgnn_bp2_decode_layered in float64 on the check rules of oracle/numpy_ref.py (_bp2_cn, written from the
    reference's Python): returns the soft outputs [B,n]."""
    hx = np.asarray(hx)
    B, n = synd.shape[0], hx.shape[1]
    chk, var = np.nonzero(hx)  # check-major edges
    llr = np.full((n, B), np.float64(F32(llr_const))) if llr_ch is None else np.asarray(llr_ch, F32).T.astype(np.float64)
    P = -1.0 * np.clip(llr, -20.0, 20.0)
    mu = np.zeros((len(chk), B))
    fac = np.float64(F32(factor))
    layers = []
    for l in range(int(np.max(layer_of)) + 1):
        e = np.nonzero(np.asarray(layer_of)[chk] == l)[0]
        first = np.r_[True, chk[e][1:] != chk[e][:-1]]
        starts = np.flatnonzero(first)
        layers.append((e, np.cumsum(first) - 1, starts, ((-1.0) ** synd.T.astype(np.float64))[chk[e][starts]]))
    for _ in range(num_iter):
        for e, seg, starts, sign in layers:
            nu = P[var[e]] - mu[e]
            mu[e] = R._bp2_cn(cn_type, nu, seg, starts, sign) * fac
            P[var[e]] = nu + mu[e]
    return np.ascontiguousarray((-1.0 * P).T)


@pytest.mark.parametrize("name", CODES + ("degenerate",))
@pytest.mark.parametrize("cn_type", RULES)
def test_one_and_two_iterations_against_float64(name, cn_type):
    """The bound and its scale are those of test_bp2_reference_cpu._compare: relative to the sample's largest |logit|, floored at one.
    Inputs in the channel range of the library's models.  Under phi the bit of the degenerate matrix's degree-1 check is left out, for
    the reason test_degree_one_check_and_edge_free_bit gives (phi(0) is 16.635532 in float32 and 16.974 in float64), and that matrix is
    compared at one iteration.

    Which prior at which count.  Per-bit priors (|llr| in [0.2, 4]) run one and two iterations under all three rules.  The constant
    prior runs one iteration under all three and two under min-sum only.  A serial iteration passes a posterior on at once: with one
    prior L on every bit a check's smallest input is L, a bit of degree dv ends its first iteration near (1 + dv) |L| (11 on gb48 at
    L = 2.2) and the second iteration's messages lie where float32 evaluates phi(x) = log(e^x + 1) - log(e^x - 1) ~ 2 e^-x as the
    difference of two logarithms near x (one ulp of x = 10 is 1e-6, phi(10) is 9e-5: a percent of it) and where tanh saturates.  That
    rounding is the reference's own and the module docstring of test_bp2_reference_cpu.py sets such inputs aside for the same reason
    (its over-complete matrix at one iteration).  Measured there, float32 against float64, two iterations on the constant prior:
    up to 0.13 (phi) and 0.07 (tanh) of the scale on gb126 and gb48, with every such sample sending a message beyond 9.6 into a
    check; min-sum, which has no transcendental, stays within its bound."""
    hx = hx_of(name)
    rng = np.random.RandomState(3)
    B = 24
    e = (rng.rand(B, hx.shape[1]) < 0.05).astype(np.int64)
    synd = (e @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    num, lay = BR.greedy_bit_layers(hx)
    phi_gap = name == "degenerate" and cn_type == "boxplus-phi"
    cols = np.arange(hx.shape[1]) != 3 if phi_gap else slice(None)
    tol = _tol(cn_type)
    worst = 0.0
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=_llr_const(0.1)), dict(llr_ch=_channel(B, hx.shape[1], 3))):
            for it in ((1,) if phi_gap or ("llr_const" in llr and cn_type != "minsum") else (1, 2)):
                s0, h0, _ = BR.bp2_layered_decode(hx, synd, it, cn_type, factor, **llr)
                s1 = layered64(hx, synd, it, cn_type, factor, lay, **llr)
                assert s0.dtype == F32
                scale = np.maximum(1.0, np.abs(s1).max(1, keepdims=True))
                dev = (np.abs(s0.astype(np.float64) - s1) / scale)[:, cols]
                worst = max(worst, float(dev.max()))
                assert dev.max() <= tol, (name, cn_type, factor, it, sorted(llr), float(dev.max()))
                firm = (np.abs(s1) > tol * scale)[:, cols]
                assert np.array_equal(h0[:, cols][firm], (0.0 < s1)[:, cols][firm])
    print(name, cn_type, "largest relative deviation", worst)


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("gb48", "rsurf5", "degenerate"))
def test_zero_iterations_are_the_flooding_decoder_at_zero(name, cn_type):
    hx = hx_of(name)
    og = binary_oracle(hx)
    B = 16
    synd = np.random.RandomState(5).randint(0, 2, size=(B, hx.shape[0])).astype(np.uint8)
    llr = _channel(B, hx.shape[1], 4)
    llr[:, 0] = [0.0, -0.0, 25.0, -30.0, 1e-40, -1e-40, 20.0, -20.0] * 2
    for kw in (dict(llr_const=-1.5), dict(llr_const=0.0), dict(llr_ch=llr)):
        s0, h0 = og.bp2_decode(synd, 0, cn_type, 0.8, **kw)
        s1, h1, st = BR.bp2_layered_decode(hx, synd, 0, cn_type, 0.8, **kw)
        assert s1.tobytes() == s0.tobytes() and h1.tobytes() == h0.tobytes()
        assert (st[:, 1] == 0).all() and np.array_equal(st[:, 0].astype(bool), BR.parity_ok(hx, h0, synd))


def test_the_tanh_rule_is_the_shared_one_wherever_no_nan_arises():
    """bp2_layered_reference._tanh_rule against mbp4_reference.cn_update on every check of gb126 and of the degenerate matrix; and a
    denormal input whose check's product underflows: the shared restatement hands a NaN on, the device's fmaxf / fminf clip it."""
    import types
    import mbp4_reference as MB
    from relay_reference import _Graph
    for hx in (hx_of("gb126"), degenerate_hx()):
        G = _Graph(hx)
        side = types.SimpleNamespace(m=G.m, cn_tab=np.maximum(G.chk_slots, 0), cn_mask=G.chk_slots >= 0)
        rng = np.random.RandomState(8)
        nu = rng.uniform(-6.0, 6.0, size=(16, G.E)).astype(F32)
        nu[rng.rand(16, G.E) < 0.05] = 0.0
        synd = rng.randint(0, 2, size=(16, G.m)).astype(np.uint8)
        for factor in (1.0, 0.8):
            assert BR._tanh_rule(side, nu, synd, factor).tobytes() == MB.cn_update(side, nu, synd, "boxplus", factor).tobytes()
    nu[:] = F32(1e-3)  # ten of them and a denormal: the product is 0, 1 / t of the denormal is inf
    nu[:, G.chk_slots[6, 0]] = F32(1e-40)
    with np.errstate(invalid="ignore"):
        assert np.isnan(MB.cn_update(side, nu, synd, "boxplus", 1.0)[:, G.chk_slots[6, 0]]).all()
    mine = BR._tanh_rule(side, nu, synd, 1.0)
    assert np.isfinite(mine).all() and (mine[:, G.chk_slots[6, 0]] < -15.0).all()  # 2 atanh(-clipv) = -16.6


def test_one_layer_per_check_in_order_differs_from_the_greedy_layering():
    hx = hx_of("gb48")
    rng = np.random.RandomState(2)
    synd = rng.randint(0, 2, size=(8, hx.shape[0])).astype(np.uint8)
    a, _, _ = BR.bp2_layered_decode(hx, synd, 2, "minsum", 0.8, llr_const=-2.0)
    b, _, _ = BR.bp2_layered_decode(hx, synd, 2, "minsum", 0.8, llr_const=-2.0, layer_of=np.arange(hx.shape[0])[::-1])
    assert a.tobytes() != b.tobytes()


def test_stop_freezes_a_sample_at_its_first_solution():
    hx = hx_of("ibm72")
    og = oracle_library_forms("ibm72")
    e = og.bsc_noise(1234, 0.04, 0, 64)
    synd = (e.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    L = _llr_const(0.04)
    s, h, st = BR.bp2_layered_decode(hx, synd, 8, "minsum", 0.8, llr_const=L, stop=True)
    assert len(set(st[st[:, 0] == 1, 1].tolist())) > 1 and (st[st[:, 0] == 0, 1] == 8).all() and (st[:, 0] == 0).any()
    for b in range(64):
        sb, hb, stb = BR.bp2_layered_decode(hx, synd[b:b + 1], int(st[b, 1]), "minsum", 0.8, llr_const=L)
        assert sb.tobytes() == s[b:b + 1].tobytes() and stb[0, 0] == st[b, 0]
        if st[b, 0] and st[b, 1] > 1:  # one iteration earlier it was no solution yet
            assert BR.bp2_layered_decode(hx, synd[b:b + 1], int(st[b, 1]) - 1, "minsum", 0.8, llr_const=L)[2][0, 0] == 0


def test_pinned_layered_8_against_flooding_on_ghp882():
    """hx of [[882,24]], BSC p = 0.04, the 64 first samples of the oracle's noise stream at seed 1234, min-sum at factor 0.8 with the
    prior of p: samples whose decision does not reproduce the syndrome.  Eight layered iterations leave 1, eight flooding iterations
    18 and sixty-four flooding iterations 4."""
    og = oracle_library_forms("ghp882")
    hx = hx_of("ghp882")
    e = og.bsc_noise(1234, 0.04, 0, 64)
    synd = (e.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    L = _llr_const(0.04)
    layered = BR.unsolved(hx, synd, BR.bp2_layered_decode(hx, synd, 8, "minsum", 0.8, llr_const=L)[1])
    flooding8 = BR.unsolved(hx, synd, og.bp2_decode(synd, 8, "minsum", 0.8, llr_const=L)[1])
    flooding64 = BR.unsolved(hx, synd, og.bp2_decode(synd, 64, "minsum", 0.8, llr_const=L)[1])
    print("layered-8", layered, "flooding-8", flooding8, "flooding-64", flooding64)
    assert layered < flooding8 and layered <= flooding64
    assert (layered, flooding8, flooding64) == (1, 18, 4)


# ---- build surface -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_bp2_layered\.hip\b", mk, flags=re.M)


def test_null_graph_is_an_argument_error():
    from feedback_gnn_amd import _lib
    L = _lib.lib()
    assert L.fgnn_bp2_decode_layered(None, 2, 1, 1.0, None, 0.0, None, 1, 0, None, None, None, None) == -1
    assert b"graph is NULL" in L.fgnn_last_error()
    assert L.fgnn_graph_set_bit_layers(None, 0, None) == -1
    num = ctypes.c_int32(5)
    assert L.fgnn_graph_bit_layers(None, ctypes.byref(num), None) == -1
    lay = np.zeros(3, np.int32)
    assert L.fgnn_greedy_bit_layers(7, 3, 0, None, None, lay.ctypes.data_as(ctypes.c_void_p), None) == -1
    args, _keep = _edges(hx_of("steane"))
    assert L.fgnn_validate_bit_layers(*args, 3, None) == -1 and b"layer_of is NULL" in L.fgnn_last_error()


def test_public_classes():
    import inspect
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(TannerGraph.set_bit_layers) and callable(TannerGraph.bit_layers) and callable(TannerGraph.bp2_decode_layered)
    a, b = inspect.signature(TannerGraph.bp2_decode), inspect.signature(TannerGraph.bp2_decode_layered)
    assert list(b.parameters) == list(a.parameters) + ["stop", "want_stats"]
    assert [p.default for p in b.parameters.values()] == [p.default for p in a.parameters.values()] + [False, False]
    sig = inspect.signature(F.LDPCBPDecoder.__init__)
    assert sig.parameters["schedule"].default == "flooding" and sig.parameters["layers"].default is None
    assert sig.parameters["stop_early"].default is False
    assert isinstance(F.LDPCBPDecoder.schedule, property)
