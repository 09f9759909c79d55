"""The layered (serial) BP4 schedule on the CPU: the host half of the feature (fgnn_greedy_layers, fgnn_validate_layers), the restatement
tests/layered_reference.py tied to the C oracle's flooding BP4, a pinned sanity check of what the schedule buys, and the build surface
(header, library export, public classes).  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import layered_reference as LR
from helpers import CODE_MAKERS, code, llr_const, oracle_library_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ("fgnn_greedy_layers", "fgnn_validate_layers", "fgnn_graph_set_layers", "fgnn_graph_layers", "fgnn_bp4_decode_layered")


def _coo(mat):
    r, c = np.nonzero(np.asarray(mat))
    return np.ascontiguousarray(r, np.int32), np.ascontiguousarray(c, np.int32)


def _edges(hx, hz):
    hx, hz = np.asarray(hx), np.asarray(hz)
    rx, cx = _coo(hx)
    rz, cz = _coo(hz)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    keep = (rx, cx, rz, cz)
    return (hx.shape[1], hx.shape[0], hz.shape[0], len(rx), ptr(rx), ptr(cx), len(rz), ptr(rz), ptr(cz)), keep


def lib_greedy(hx, hz):
    from feedback_gnn_amd import _lib
    args, _keep = _edges(hx, hz)
    lay = np.full(args[1] + args[2], -7, np.int32)
    num = ctypes.c_int32(-1)
    _lib.check(_lib.lib().fgnn_greedy_layers(*args, lay.ctypes.data_as(ctypes.c_void_p), ctypes.byref(num)))
    return int(num.value), lay


def lib_validate(hx, hz, num_layers, layer_of):
    """(return code, message) of fgnn_validate_layers."""
    from feedback_gnn_amd import _lib
    args, _keep = _edges(hx, hz)
    lay = np.ascontiguousarray(layer_of, np.int32)
    rc = _lib.lib().fgnn_validate_layers(*args, int(num_layers), lay.ctypes.data_as(ctypes.c_void_p))
    return rc, _lib.lib().fgnn_last_error().decode()


# ---- layers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODE_MAKERS))
def test_greedy_layers_of_the_library_are_the_python_greedy_and_valid(name):
    c = code(name)
    num, lay = lib_greedy(c.hx, c.hz)
    num_py, lay_py = LR.greedy_layers(c.hx, c.hz)
    assert num == num_py and np.array_equal(lay, lay_py)
    assert LR.is_valid_layering(c.hx, c.hz, num, lay)
    assert lib_validate(c.hx, c.hz, num, lay)[0] == 0


def test_greedy_layer_counts_of_known_codes():
    c = code("ghp882")
    num, lay = lib_greedy(c.hx, c.hz)
    sizes = np.bincount(lay, minlength=num)
    assert num == 13 and sizes.min() == 6 and sizes.max() == 96 and sizes.sum() == 882
    c = code("ibm72")
    num, lay = lib_greedy(c.hx, c.hz)
    assert num == 8 and np.bincount(lay).tolist() == [9] * 8
    c = code("steane")  # every two checks of the Steane code share a qubit
    num, lay = lib_greedy(c.hx, c.hz)
    assert num == 6 and lay.tolist() == list(range(6))


def test_validation_names_the_cause():
    c = code("steane")
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    m_x = hx.shape[0]
    one_each = np.arange(6, dtype=np.int32)
    assert lib_validate(hx, hz, 6, one_each)[0] == 0
    # hx check 0 and hz check 0 have the same support: one layer for both collides across the two sides
    lay = np.array([0, 1, 2, 0, 3, 4], np.int32)
    v = int(np.nonzero(hx[0] & hz[0])[0][0])
    rc, msg = lib_validate(hx, hz, 5, lay)
    assert rc == -1 and "hx check 0" in msg and "hz check 0" in msg and f"number {m_x}" in msg and f"share qubit {v}" in msg and "layer 0" in msg
    # two hx checks of one layer
    rc, msg = lib_validate(hx, hz, 5, np.array([0, 0, 1, 2, 3, 4], np.int32))
    assert rc == -1 and "hx check 0" in msg and "hx check 1" in msg and "share qubit" in msg
    # an empty layer
    rc, msg = lib_validate(hx, hz, 7, np.array([0, 1, 2, 3, 4, 6], np.int32))
    assert rc == -1 and "layer 5 is empty" in msg
    # out of range, above and below
    rc, msg = lib_validate(hx, hz, 6, np.array([0, 1, 2, 3, 4, 6], np.int32))
    assert rc == -1 and "hz check 2" in msg and "has layer 6" in msg and "[0, 6)" in msg
    rc, msg = lib_validate(hx, hz, 6, np.array([0, -1, 2, 3, 4, 5], np.int32))
    assert rc == -1 and "hx check 1" in msg and "has layer -1" in msg
    rc, msg = lib_validate(hx, hz, 0, one_each)
    assert rc == -1 and "num_layers" in msg
    # a disjoint pair may share a layer: rsurf5's greedy layering with two layers merged is refused, the greedy one is not
    c = code("rsurf5")
    num, lay = lib_greedy(c.hx, c.hz)
    assert num < np.asarray(c.hx).shape[0] + np.asarray(c.hz).shape[0], "some layer holds more than one check"
    merged = np.where(lay == num - 1, 0, lay)
    assert not LR.is_valid_layering(c.hx, c.hz, num - 1, merged) and lib_validate(c.hx, c.hz, num - 1, merged)[0] == -1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def disjoint_code():
    """Checks that are pairwise disjoint, across hx and hz: ONE layer is a valid layering, and the layered schedule is flooding."""
    hx = np.zeros((3, 14), np.int64)
    hz = np.zeros((2, 14), np.int64)
    hx[0, [0, 1, 2]] = 1
    hx[1, [3, 4]] = 1
    hx[2, [5]] = 1
    hz[0, [6, 7, 8, 9]] = 1
    hz[1, [10, 11, 12]] = 1  # qubit 13 has no check
    zero = np.zeros((1, 14), np.int64)
    return types.SimpleNamespace(hx=hx, hz=hz, hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("llr", "x_hat", "z_hat", "x_logit", "z_logit", "msg_x", "msg_z"))


@pytest.mark.parametrize("cn_type", ["boxplus", "boxplus-phi", "minsum"])
def test_anchor_one_layer_is_flooding(cn_type):
    from oracle.oracle import OracleGraph
    c = disjoint_code()
    og = OracleGraph(c, forms="literal")
    assert LR.greedy_layers(c.hx, c.hz)[0] == 1 and lib_greedy(c.hx, c.hz)[0] == 1
    rng = np.random.RandomState(4)
    B = 16
    sx = rng.randint(0, 2, size=(B, 3)).astype(np.uint8)
    sz = rng.randint(0, 2, size=(B, 2)).astype(np.uint8)
    llr = rng.uniform(-1.0, 4.0, size=(B, 3, 14)).astype(F32)
    for T in (0, 1, 3):
        for kw in (dict(llr_const=llr_const(0.1)), dict(llr_ch=llr)):
            want = og.bp4_decode(sx, sz, T, cn_type, 0.8, return_msgs=True, **kw)
            assert same(LR.layered_decode(og, sx, sz, T, cn_type, 0.8, **kw), want)
            assert same(LR.layered_decode(og, sx, sz, T, cn_type, 0.8, layer_of=np.zeros(5, np.int32), keep_all=True, **kw), want)
    # on a code whose checks overlap, ONE kept-whole step per iteration is flooding too; the layered schedule is not
    og = oracle_library_forms("steane")
    ex, ez = og.pauli_noise(11, 0.1, 0, B)
    sx, sz = og.syndrome(ex, ez)
    want = og.bp4_decode(sx, sz, 3, cn_type, 0.8, llr_const=llr_const(0.1), return_msgs=True)
    assert same(LR.layered_decode(og, sx, sz, 3, cn_type, 0.8, layer_of=np.zeros(6, np.int32), keep_all=True, llr_const=llr_const(0.1)), want)
    assert not same(LR.layered_decode(og, sx, sz, 3, cn_type, 0.8, llr_const=llr_const(0.1)), want)


def test_chained_steps_equal_one_run():
    og = oracle_library_forms("rsurf5")
    ex, ez = og.pauli_noise(5, 0.1, 0, 12)
    sx, sz = og.syndrome(ex, ez)
    kw = dict(cn_type="minsum", factor=0.8, llr_const=llr_const(0.1))
    one = LR.layered_decode(og, sx, sz, 1, **kw)
    two = LR.layered_decode(og, sx, sz, 1, msg_init=(one["msg_x"], one["msg_z"]), **kw)
    assert same(two, LR.layered_decode(og, sx, sz, 2, **kw))


def test_pinned_layered_8_against_flooding_16_on_ghp882():
    """[[882,24]], depolarizing p = 0.09, 64 samples of the seeded stream, min-sum at factor 0.8 with the prior of p: samples whose
    decision does not reproduce its syndromes.  Eight layered iterations leave none, sixteen flooding iterations leave 22."""
    og = oracle_library_forms("ghp882")
    c = code("ghp882")
    ex, ez = og.pauli_noise(1234, 0.09, 0, 64)
    sx, sz = og.syndrome(ex, ez)
    L = llr_const(0.09)
    layered = LR.unsolved(c, sx, sz, LR.layered_decode(og, sx, sz, 8, "minsum", 0.8, llr_const=L))
    flooding = LR.unsolved(c, sx, sz, og.bp4_decode(sx, sz, 16, "minsum", 0.8, llr_const=L))
    print("layered-8", layered, "flooding-16", flooding)
    assert layered == 0 and flooding == 22 and layered <= flooding


# ---- build surface -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_layered_entry_points():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_bp4_layered\.hip\b", mk, flags=re.M)


def test_null_graph_is_an_argument_error():
    from feedback_gnn_amd import _lib
    L = _lib.lib()
    assert L.fgnn_bp4_decode_layered(None, 2, 1, 1.0, None, 0.0, None, None, 1, *([None] * 10)) == -1
    assert b"graph is NULL" in L.fgnn_last_error()
    assert L.fgnn_graph_set_layers(None, 0, None) == -1
    num = ctypes.c_int32(5)
    assert L.fgnn_graph_layers(None, ctypes.byref(num), None) == -1


def test_public_classes():
    import inspect
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(TannerGraph.set_layers) and callable(TannerGraph.layers) and callable(TannerGraph.bp4_decode_layered)
    a, b = inspect.signature(TannerGraph.bp4_decode), inspect.signature(TannerGraph.bp4_decode_layered)
    assert list(a.parameters) == list(b.parameters) and [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()]
    sig = inspect.signature(F.QLDPCBPDecoder.__init__)
    assert sig.parameters["schedule"].default == "flooding" and sig.parameters["layers"].default is None
    assert isinstance(F.QLDPCBPDecoder.schedule, property)
