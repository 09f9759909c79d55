"""MBP4 / AMBP4 in the serial schedule: the restatement tests/mbp4_serial_reference.py checked for what the algorithm at
fgnn_mbp4_decode_serial (include/fgnn.h) states, its layer functions against the library's, the single-output check rule of
fgnn_cn1.h against cn_update on the host, the figures of the schedule, and the build surface of the feature.  CPU only."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import mbp4_reference as MB
import mbp4_serial_reference as MS
from helpers import code, llr_const, oracle_library_forms
from test_bp4fb_reference_cpu import depolarizing, ghp882_samples, solves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
P = 0.10
ALPHAS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)
NEW_SYMBOLS = ("fgnn_mbp4_decode_serial", "fgnn_greedy_qubit_layers", "fgnn_validate_qubit_layers", "fgnn_graph_set_qubit_layers",
               "fgnn_graph_qubit_layers")


def one_layer_code():
    """hx = rows e_0 .. e_4 and hz = rows e_5 .. e_8 of I_12: no two qubits share a check, qubits 9 .. 11 have none."""
    eye = np.eye(12, dtype=np.uint8)
    return types.SimpleNamespace(hx=eye[0:5].copy(), hz=eye[5:9].copy())


def irregular_code():
    """12 qubits under hx checks of degree 1, 2, 3, 5 and hz checks of degree 1, 2, 2, 4, 6; qubit degrees 0 .. 4.  The two matrices
    do not commute: nothing here needs a code space."""
    hx, hz = np.zeros((4, 12), np.uint8), np.zeros((5, 12), np.uint8)
    for r, cols in enumerate([(0,), (1, 2), (2, 3, 4), (0, 4, 5, 6, 7)]):
        hx[r, list(cols)] = 1
    for r, cols in enumerate([(8,), (0, 9), (3, 8), (1, 4, 6, 9), (0, 2, 5, 7, 8, 10)]):
        hz[r, list(cols)] = 1
    return types.SimpleNamespace(hx=hx, hz=hz)


def one_layer_llrs(B):
    """Channel LLRs [B,3,12] for the one-layer code.  A degree-one check sends its qubit about 17 (the two phi rules) or 10 000 + |nu|
    (min-sum), which a prior of the usual size never outweighs: every sample would be solved by the first iteration.  Some qubits of
    every second sample get priors of up to 100, some of every fourth of up to 40 000, so that samples stay unsolved under every
    rule and walk all attempts."""
    llr = np.random.RandomState(6).uniform(-3.0, 4.0, size=(B, 3, 12)).astype(F32)
    llr[::2, :, 1::4] *= F32(25.0)
    llr[::4, :, 2::5] *= F32(1e4)
    return llr


def random_syndromes(c, B, seed, p=0.15):
    rng = np.random.RandomState(seed)
    n = c.hx.shape[1]
    ex, ez = (rng.rand(B, n) < p).astype(np.int64), (rng.rand(B, n) < p).astype(np.int64)
    return (ez @ c.hx.T.astype(np.int64) % 2).astype(np.uint8), (ex @ c.hz.T.astype(np.int64) % 2).astype(np.uint8)


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


# ---- one layer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_on_a_one_layer_code_the_serial_schedule_is_the_flooding_one(cn_type):
    """One layer holds every qubit: an iteration is one check update on the nu of the iteration before, then every qubit.  That is
    MB.mbp4_decode bit for bit with one attempt, with restart, and with equal own weights; with the messages kept and different
    weights the first check update of a later attempt reads the nu formed with the weight before (the header says so): the next
    test shows that on the messages."""
    c = one_layer_code()
    assert MS.greedy_qubit_layers(c.hx, c.hz)[0] == 1
    B = 48
    sx, sz = random_syndromes(c, B, 5, p=0.3)
    per_qubit = one_layer_llrs(B)
    f3, o3 = MB.mbp4_tables((1.0, 0.8, 0.6), 0.8)
    cases = [(f3[:1], o3[:1], True), (f3[:1], o3[:1], False), (f3, o3, True), (f3, np.full(3, 0.7, F32), False)]
    later = False
    for llr in (dict(llr_const=0.4), dict(llr_ch=per_qubit)):
        for f, o, restart in cases:
            want = MB.mbp4_decode(c, sx, sz, f, o, 3, 2, cn_type, restart=restart, **llr)
            got = MS.mbp4_decode_serial(c, sx, sz, f, o, 3, 2, cn_type, restart=restart, **llr)
            assert same(got, want), (cn_type, restart, sorted(llr))
            later |= bool((want[2][:, 1] > 0).any())
    assert later, "a sample must reach a later attempt"


def test_with_the_messages_kept_a_new_own_weight_reaches_the_first_check_update_one_iteration_later():
    """The one place where the two schedules part on a one-layer graph (the header says so): flooding opens attempt a > 0 by forming nu
    with own[a], the serial schedule opens it with a check update on the nu the last visit of attempt a - 1 formed with own[a - 1].
    Shown on the messages: after two flooding iterations at own = 1.0, the c->v messages of the next iteration at own = 0.6 differ
    between the two under min-sum, whose degree-one output 10 000 + |nu| carries the input; with own = 1.0 again they are the same bits.
    (On the samples of the test above the decisions of the two do not differ.)"""
    c = one_layer_code()
    G = MB.graph_of(c)
    B = 16
    sx, sz = random_syndromes(c, B, 5, p=0.3)
    lam = one_layer_llrs(B)
    f = F32(0.8)
    mux, muz = np.zeros((B, G.x.E), F32), np.zeros((B, G.z.E), F32)
    for _ in range(2):
        mux, muz, _ = G.step(mux, muz, lam, sx, sz, "minsum", f, 1.0)
    layers = MS.layer_tables(G, np.zeros(12, np.int32))
    for own, differ in ((0.6, True), (1.0, False)):
        fx, fz, _ = G.step(mux, muz, lam, sx, sz, "minsum", f, own)
        nux, nuz = G.qubit_update(mux, muz, lam, 1.0)  # what the last visit of the attempt before left
        qx, qz, hard = mux.copy(), muz.copy(), np.zeros((B, 12), np.uint8)
        MS.serial_iteration(G, layers, qx, qz, nux, nuz, hard, lam, sx, sz, "minsum", f, own)
        assert (qx.tobytes() != fx.tobytes() or qz.tobytes() != fz.tobytes()) == differ, own
        if differ:
            assert (qx != fx).mean() > 0.5 and (qz != fz).mean() > 0.5


# ---- control ------------------------------------------------------------------------------------------------------------------------------------
def ibm72_batch(B=40):
    og = oracle_library_forms("ibm72", stage_one=False)
    return depolarizing(og, P, B)


def test_a_sample_solved_in_attempt_zero_ends_as_with_one_attempt():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    factors, owns = MB.mbp4_tables((1.0, 0.8, 0.6), 0.8)
    x1, z1, s1 = MS.mbp4_decode_serial(c, sx, sz, factors[:1], owns[:1], 3, 2, llr_const=L)
    for restart in (False, True):
        x3, z3, s3 = MS.mbp4_decode_serial(c, sx, sz, factors, owns, 3, 2, restart=restart, llr_const=L)
        first = s1[:, 0] == 1
        assert first.any() and not first.all()
        assert np.array_equal(s3[first], s1[first]) and np.array_equal(x3[first], x1[first]) and np.array_equal(z3[first], z1[first])
        assert (s3[~first, 1] > 0).all()
        assert ((s3[:, 0] == 1) & (s3[:, 1] > 0)).any(), "a later alpha must solve a sample"


def test_restart_with_identical_parameters_repeats_attempt_zero():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    pre, att, A = 3, 3, 4
    f, o = np.full(A, 0.8, F32), np.full(A, 0.9, F32)
    x0, z0, s0 = MS.mbp4_decode_serial(c, sx, sz, f[:1], o[:1], pre, att, restart=True, llr_const=L)
    xh, zh, st = MS.mbp4_decode_serial(c, sx, sz, f, o, pre, att, restart=True, llr_const=L)
    solved = s0[:, 0] == 1
    assert solved.any() and not solved.all()
    assert np.array_equal(st[solved], s0[solved])
    assert np.array_equal(st[~solved], np.tile(np.array([0, A - 1, pre + (A - 1) * att, att], np.int32), ((~solved).sum(), 1)))
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0), "every attempt ends where attempt 0 ended"


def test_without_restart_attempts_of_identical_parameters_are_one_long_attempt():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    T, A = 2, 4
    f, o = np.full(A, 0.8, F32), np.full(A, 0.7, F32)
    x0, z0, s0 = MS.mbp4_decode_serial(c, sx, sz, f[:1], o[:1], A * T, 1, restart=False, llr_const=L)
    xh, zh, st = MS.mbp4_decode_serial(c, sx, sz, f, o, T, T, restart=False, llr_const=L)
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0)
    assert np.array_equal(st[:, 0], s0[:, 0]) and np.array_equal(st[:, 2], s0[:, 2])
    assert np.array_equal(st[:, 1] * T + st[:, 3], s0[:, 3]), "(a, k) counts the same iterations"
    assert (st[:, 1] > 0).any() and (st[:, 0] == 1).any() and (st[:, 0] == 0).any()


def test_the_order_of_the_layers_matters_and_the_order_inside_a_layer_cannot():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch(16)
    L = llr_const(P)
    f, o = MB.mbp4_tables((1.0, 0.8), 0.8)
    num, lay = MS.greedy_qubit_layers(c.hx, c.hz)
    a = MS.mbp4_decode_serial(c, sx, sz, f, o, 3, 2, llr_const=L)
    assert same(a, MS.mbp4_decode_serial(c, sx, sz, f, o, 3, 2, llr_const=L, layer_of=lay))
    assert not same(a, MS.mbp4_decode_serial(c, sx, sz, f, o, 3, 2, llr_const=L, layer_of=num - 1 - lay))
    assert not same(a, MS.mbp4_decode_serial(c, sx, sz, f, o, 3, 2, llr_const=L, layer_of=np.arange(72)))


# ---- layers -------------------------------------------------------------------------------------------------------------------------------------
def _edges(c):
    """The argument head (n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z) of the two host entry points, and what keeps it alive."""
    keep, args = [], [c.hx.shape[1], c.hx.shape[0], c.hz.shape[0]]
    for h in (c.hx, c.hz):
        chk, var = (np.ascontiguousarray(a, dtype=np.int32) for a in np.nonzero(np.asarray(h) % 2))
        keep += [chk, var]
        args += [len(chk), chk.ctypes.data_as(ctypes.c_void_p), var.ctypes.data_as(ctypes.c_void_p)]
    return args, keep


def lib_greedy(c):
    from feedback_gnn_amd import _lib
    args, _keep = _edges(c)
    lay, num = np.full(c.hx.shape[1], -1, np.int32), ctypes.c_int32(0)
    assert _lib.lib().fgnn_greedy_qubit_layers(*args, lay.ctypes.data_as(ctypes.c_void_p), ctypes.byref(num)) == 0
    return int(num.value), lay


def lib_validate(c, num_layers, layer_of):
    """None, or the library's refusal."""
    from feedback_gnn_amd import _lib
    args, _keep = _edges(c)
    lay = np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = _lib.lib().fgnn_validate_qubit_layers(*args, int(num_layers), lay.ctypes.data_as(ctypes.c_void_p))
    assert rc in (0, -1)
    return None if rc == 0 else _lib.lib().fgnn_last_error().decode()


@pytest.mark.parametrize("name", ["ibm72", "rsurf5", "steane", "ghp882", "one_layer", "irregular"])
def test_greedy_qubit_layers_of_the_library(name):
    c = {"one_layer": one_layer_code, "irregular": irregular_code}[name]() if name in ("one_layer", "irregular") else code(name)
    num, lay = MS.greedy_qubit_layers(c.hx, c.hz)
    num1, lay1 = lib_greedy(c)
    assert num1 == num and np.array_equal(lay1, lay)
    assert lib_validate(c, num, lay) is None and MS.validate_qubit_layers(c.hx, c.hz, num, lay) is None
    n = c.hx.shape[1]
    assert lib_validate(c, n, np.arange(n)) is None, "one qubit per layer is always valid"
    if name == "ghp882":
        assert num == 14
    if name == "one_layer":
        assert num == 1


def test_validate_qubit_layers_names_the_offender():
    c = irregular_code()
    num, lay = MS.greedy_qubit_layers(c.hx, c.hz)
    cases = []
    bad = lay.copy(); bad[3] = num + 5
    cases.append((num, bad, f"qubit 3 has layer {num + 5}, outside [0, {num})"))
    bad = lay.copy(); bad[0] = -1
    cases.append((num, bad, f"qubit 0 has layer -1, outside [0, {num})"))
    cases.append((num + 1, lay, f"layer {num} is empty"))
    cases.append((0, lay, "num_layers = 0 must be >= 1"))
    bad = np.arange(12, dtype=np.int32); bad[2] = bad[1]  # qubits 1 and 2 share hx check 1
    cases.append((12, bad, "layer 2 is empty"))
    bad = np.array([0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], np.int32)
    cases.append((11, bad, "qubit 1 and qubit 2 of layer 1 share hx check 1"))
    bad = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 9, 10], np.int32)  # qubits 0 and 9 share hz check 1, combined number 5
    cases.append((11, bad, "qubit 0 and qubit 9 of layer 0 share hz check 1 (number 5)"))
    for num_layers, layer_of, message in cases:
        assert MS.validate_qubit_layers(c.hx, c.hz, num_layers, layer_of) == message
        assert lib_validate(c, num_layers, layer_of) == message
    from feedback_gnn_amd import _lib
    args, _keep = _edges(c)
    assert _lib.lib().fgnn_validate_qubit_layers(*args, 3, None) == -1 and b"layer_of is NULL" in _lib.lib().fgnn_last_error()
    assert _lib.lib().fgnn_greedy_qubit_layers(*args, None, None) == -1
    assert _lib.lib().fgnn_graph_set_qubit_layers(None, 0, None) == -1 and b"graph is NULL" in _lib.lib().fgnn_last_error()
    assert _lib.lib().fgnn_graph_qubit_layers(None, None, None) == -1


# ---- the single-output check rule -------------------------------------------------------------------------------------------------------------
def rule_rows():
    """(deg, syndrome bit, factor, 8 inputs): degrees 1 .. 8 (and 0), both syndrome bits, seeded inputs in the decoder's range and rows
    with zeros, signed zeros, equal magnitudes, inputs at and beyond the min-sum clip of +-20, tiny and large values."""
    rng = np.random.RandomState(0xC41)
    rows = []
    special = np.array([0.0, -0.0, 20.0, -20.0, 25.0, -31.5, 1e-30, -1e-30, 16.635532, 3.0, -3.0, 0.5], F32)
    for deg in range(0, 9):
        for synd in (0, 1):
            for factor in (1.0, 0.8, 1.25):
                for kind in range(6):
                    v = (rng.standard_normal(8) * (6.0 if kind < 3 else 14.0)).astype(F32)
                    if kind in (1, 4):
                        pick = rng.rand(8) < 0.5
                        v[pick] = special[rng.randint(len(special), size=int(pick.sum()))]
                    if kind == 2:
                        v[:] = np.abs(v[0]) * rng.choice([-1.0, 1.0], size=8)  # every magnitude equal: the second minimum is the minimum
                    if kind == 5:
                        v[:] = special[rng.randint(len(special), size=8)]
                    rows.append(np.concatenate([[deg, synd, factor], v]))
    return np.array(rows, F32)


def build_and_run(flags, table):
    src = os.path.join(ROOT, "tests", "cn_output_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "cn_output_check")
        cc = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function"] + flags +
                            ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], input=np.ascontiguousarray(table, dtype=F32).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:])
    lines = run.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(table), run.stdout[-2000:]
    return np.array([[int(h, 16) for h in ln.split()] for ln in lines], np.uint32).reshape(len(table), 3, 2, 8)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_cn_output_of_the_header_equals_cn_update_bitwise(flags):
    rows = rule_rows()
    got = build_and_run(flags, rows)
    deg = rows[:, 0].astype(int)
    assert set(deg.tolist()) == set(range(9)) and set(rows[:, 1].tolist()) == {0.0, 1.0}
    assert (np.abs(rows[:, 3:]) == 20.0).any() and (np.abs(rows[:, 3:]) > 20.0).any() and (rows[:, 3:] == 0.0).any()
    for r, name in enumerate(CN_TYPES):
        update, single = got[:, r, 0], got[:, r, 1]
        bad = (update != single).any(1)
        assert not bad.any(), (name, np.nonzero(bad)[0][:10], rows[bad][:3], update[bad][:3], single[bad][:3])
        assert len(np.unique(update[deg >= 2][:, 0])) > 50, "the outputs are not all one value"
    # and cn_update of the header is the restatement's rule: the program's first columns against MB.cn_update, degree by degree
    for d in range(1, 9):
        sel = np.nonzero(deg == d)[0]
        side = types.SimpleNamespace(m=len(sel), cn_tab=np.arange(len(sel) * d).reshape(len(sel), d), cn_mask=np.ones((len(sel), d), bool))
        nu = rows[sel, 3:3 + d].reshape(1, -1).copy()
        for r, name in enumerate(CN_TYPES):
            for factor in np.unique(rows[sel, 2]):
                fs = rows[sel, 2] == factor
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    want = MB.cn_update(side, nu, rows[sel, 1][None, :].astype(np.uint8), name, factor).reshape(len(sel), d)
                ok = np.isfinite(want[fs]).all(1)  # the NumPy boxplus hands a NaN on where the device's fmaxf / fminf clip it
                assert ok.mean() > 0.5
                assert np.array_equal(got[sel, r, 0, :d][fs][ok], want[fs][ok].view(np.uint32)), (name, d, float(factor))


# ---- figures ----------------------------------------------------------------------------------------------------------------------------------
GHP882_SERIAL_FIGURES = (0, 22, 0)  # alpha 1.0 alone, 64 iterations: (unsolved, largest its, logical errors)


@functools.lru_cache(maxsize=None)
def ghp882_serial_reference():
    """Serial MBP4 at alpha 1.0 alone (64 iterations, min-sum, base factor 0.8, greedy layers) on [[882,24]], p = 0.10, samples 0..63."""
    c = code("ghp882")
    _, _, sx, sz = ghp882_samples()
    factors, owns = MB.mbp4_tables((1.0,), 0.8)
    return MS.mbp4_decode_serial(c, sx, sz, factors, owns, 64, 64, "minsum", restart=True, llr_const=llr_const(0.10))


def logical_errors(c, ex, ez, xh, zh, solved):
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64) % 2, np.asarray(c.hz_perp, np.int64) % 2
    return int(((((xd @ hxp.T) % 2).any(1) | ((zd @ hzp.T) % 2).any(1)) & solved).sum())


def ghp882_serial_figures(xh, zh, st):
    c = code("ghp882")
    ex, ez, sx, sz = ghp882_samples()
    solved = st[:, 0] == 1
    assert np.array_equal(solves(c, xh, zh, sx, sz), solved)
    return int((~solved).sum()), int(st[:, 2].max()), logical_errors(c, ex, ez, xh, zh, solved)


def test_ghp882_figures():
    """Flooding min-sum BP4-64 leaves 7 of these 64 samples unsolved and the flooding alpha sweep 1 (tests/test_mbp4_reference_cpu.py);
    the serial schedule at alpha 1.0 alone must leave strictly fewer than 7 and make no logical error."""
    xh, zh, st = ghp882_serial_reference()
    print("its", st[:, 2].tolist())
    figures = ghp882_serial_figures(xh, zh, st)
    print("figures", figures, "mean its", float(st[:, 2].mean()))
    assert figures[0] < 7 and figures[2] == 0
    assert figures == GHP882_SERIAL_FIGURES


P12_FIGURES = (5, 4, 1, 0)  # (left by alpha 1.0, solved at a > 0, unsolved after the sweep, logical errors), messages kept


def test_depolarizing_012_figures():
    """[[882,24]] at p = 0.12, 64 samples, alphas 1.0 .. 0.5 with 32 iterations each and the messages kept: a later alpha must solve
    samples, and no solved sample may carry a logical error."""
    og, c = oracle_library_forms("ghp882", stage_one=False), code("ghp882")
    ex, ez, sx, sz = depolarizing(og, 0.12, 64)
    factors, owns = MB.mbp4_tables(ALPHAS, 0.8)
    xh, zh, st = MS.mbp4_decode_serial(c, sx, sz, factors, owns, 32, 32, "minsum", restart=False, llr_const=llr_const(0.12))
    solved = st[:, 0] == 1
    assert np.array_equal(solves(c, xh, zh, sx, sz), solved)
    later = int((solved & (st[:, 1] > 0)).sum())
    figures = (int(((st[:, 1] > 0) | ~solved).sum()), later, int((~solved).sum()), logical_errors(c, ex, ez, xh, zh, solved))
    print("a", st[:, 1].tolist(), "figures", figures)
    assert later > 0 and figures[3] == 0
    assert figures == P12_FIGURES


# ---- build surface ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    assert _lib._SIGNATURES["fgnn_mbp4_decode_serial"] == _lib._SIGNATURES["fgnn_mbp4_decode"]
    assert _lib._SIGNATURES["fgnn_greedy_qubit_layers"] == _lib._SIGNATURES["fgnn_greedy_layers"]
    assert _lib._SIGNATURES["fgnn_validate_qubit_layers"] == _lib._SIGNATURES["fgnn_validate_layers"]
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_mbp4_serial\.hip\b", mk, flags=re.M) and re.search(r"^HDRS :=.*\bfgnn_cn1\.h\b", mk, flags=re.M)
    cn1 = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "fgnn_cn1.h")).read()
    assert re.search(r"FG_FN\s+float\s+cn_output\s*\(", cn1)
    assert os.path.exists(os.path.join(ROOT, "tests", "cn_output_check.cpp"))


def test_public_classes_take_the_schedule():
    import inspect
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(TannerGraph.mbp4_decode_serial) and callable(TannerGraph.set_qubit_layers) and callable(TannerGraph.qubit_layers)
    assert inspect.signature(TannerGraph.mbp4_decode_serial) == inspect.signature(TannerGraph.mbp4_decode)
    sig = inspect.signature(F.AMBP4Decoder.__init__).parameters
    assert sig["schedule"].default == "flooding" and sig["layers"].default is None
