"""BP4 with message-strength control (MBP4 / AMBP4): the restatement tests/mbp4_reference.py, tied to the C oracle's BP4 and to the host
build of vn_edge_own, and checked for what the algorithm at fgnn_mbp4_decode (include/fgnn.h) states; and the build surface of the
feature (header, library export, public classes).  CPU only.

Anchor.  With one attempt and own = 1 the product own * mu is mu bit for bit and the restatement is BP4 stopped at its first solution:
tests/bp4gd_reference.py with max_rounds = 0, whose every step is one call of the oracle.  The restatement writes the check rules out
in NumPy, so this equality, for all three rules, is what ties them to the oracle."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bp4gd_reference as GD
import mbp4_reference as MB
from helpers import code, llr_const, oracle_library_forms
from test_bp4fb_reference_cpu import depolarizing, ghp882_samples, solves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
P = 0.10
ALPHAS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)


def one(x):
    return np.array([x], F32)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_one_attempt_with_own_one_is_bp4_stopped_at_its_first_solution(cn_type):
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    B, T = 32, 12
    _, _, sx, sz = depolarizing(og, P, B)
    per_qubit = np.random.RandomState(3).uniform(1.0, 6.0, size=(B, 3, og.n)).astype(F32)
    for llr in (dict(llr_const=llr_const(P)), dict(llr_ch=per_qubit)):
        x0, z0, s0, _ = GD.bp4gd_decode(og, sx, sz, T, 5, 0, 25.0, cn_type, 0.8, **llr)
        for restart in (False, True):
            xh, zh, st = MB.mbp4_decode(c, sx, sz, one(0.8), one(1.0), T, 5, cn_type, restart=restart, **llr)
            assert xh.tobytes() == x0.tobytes() and zh.tobytes() == z0.tobytes() and np.array_equal(st, s0) and not st[:, 1].any()
        assert (st[:, 0] == 1).any() and (st[:, 0] == 0).any()


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def edge_rows():
    """(num, A, Y, mu, w) rows: seeded values in the ranges the decoder forms, w among the default alphas, 0, 1 and other weights, and
    rows with zeros, the min-sum clip and large totals, where the log-sum-exp saturates."""
    rng = np.random.RandomState(0x4D4250)
    N = 4000
    num = np.abs(rng.standard_normal(N) * 3.0)
    A, Y = rng.standard_normal(N) * 12.0, rng.standard_normal(N) * 12.0
    mu = rng.standard_normal(N) * 6.0
    w = rng.choice(np.array(ALPHAS + (0.0, 1.0, 0.33, 1.25, 2.0)), size=N)
    rows = np.stack([num, A, Y, mu, w], axis=1).astype(F32)
    edge = np.array([[0.0, 0.0, 0.0, 0.0, 0.5], [1.0, 20.0, -20.0, 20.0, 0.9], [0.5, -45.0, 60.0, -16.0, 0.7], [2.0, 3.0, 3.0, -0.0, 0.6],
                     [0.25, 1e-40, -1e-40, 1.4e-45, 0.5], [3.0, 100.0, 99.0, 25.0, 0.8]], F32)
    return np.concatenate([edge, rows])


def build_and_run(flags, table):
    src = os.path.join(ROOT, "tests", "vn_edge_own_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vn_edge_own_check")
        cc = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function"] + flags +
                            ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], input=np.ascontiguousarray(table, dtype=F32).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(table), run.stdout[-2000:]
    return np.array([[int(h, 16) for h in ln.split()] for ln in lines], np.uint32)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_vn_edge_own_of_the_header_equals_the_restatement_bitwise(flags):
    rows = edge_rows()
    got = build_and_run(flags, rows)
    num, A, Y, mu, w = (rows[:, i].copy() for i in range(5))
    want = np.empty(len(rows), F32)
    for wv in np.unique(w):  # the helper takes one weight per call, as the decoder does
        sel = w == wv
        want[sel] = MB.vn_edge_own(num[sel], A[sel], Y[sel], mu[sel], wv)
    assert np.array_equal(got[:, 0], want.view(np.uint32)), np.nonzero(got[:, 0] != want.view(np.uint32))[0][:10]
    plain = w == F32(1.0)
    assert plain.sum() > 100 and np.array_equal(got[plain, 0], got[plain, 1]), "w = 1: vn_edge_own is vn_edge bit for bit"
    other = (w != F32(1.0)) & (mu != 0)
    assert (got[other, 0] != got[other, 1]).mean() > 0.9, "another weight gives another message"
    # the product is rounded before it is subtracted: a contracted one would differ on some of these rows
    Ae_fused = (A.astype(np.float64) - w.astype(np.float64) * mu.astype(np.float64)).astype(F32)
    Ae = (A - (w * mu).astype(F32)).astype(F32)
    assert (Ae_fused != Ae).sum() >= 5, "the table tells the rounded product from a contracted one"


# ---- the own weight -------------------------------------------------------------------------------------------------------------------------
def nonzero_state(c, B, seed):
    G = MB.graph_of(c)
    rng = np.random.RandomState(seed)
    mux = (rng.standard_normal((B, G.x.E)) * 3.0).astype(F32)
    muz = (rng.standard_normal((B, G.z.E)) * 3.0).astype(F32)
    lam = rng.uniform(1.0, 5.0, size=(B, 3, G.n)).astype(F32)
    return G, mux, muz, lam


def test_own_zero_takes_nothing_out():
    """own = 0, one qubit update from non-zero messages: the edge value is num - lse2(-A, -Y), the same for every edge of a qubit and
    side."""
    G, mux, muz, lam = nonzero_state(code("ibm72"), 5, 11)
    nux, nuz = G.qubit_update(mux, muz, lam, 0.0)
    X, Y, Z = G.totals(mux, muz, lam)
    wantx = (MB.softplus(-X) - MB.lse2(-Z, -Y)).astype(F32)
    wantz = (MB.softplus(-Z) - MB.lse2(-X, -Y)).astype(F32)
    assert nux.tobytes() == wantx[:, G.x.v_of].tobytes() and nuz.tobytes() == wantz[:, G.z.v_of].tobytes()
    n1x, _ = G.qubit_update(mux, muz, lam, 1.0)
    assert (n1x != nux).mean() > 0.9


def test_own_enters_through_the_product_alone():
    """Two weights whose float32 products with the message agree give the same bits.  1.7 and the float after it, on seeded messages:
    where 1.7 mu crosses into the next binade the change is under one ulp of the product and rounds away on part of the rows."""
    rng = np.random.RandomState(2)
    N = 2000
    mu = (rng.standard_normal(N) * 4.0).astype(F32)
    w1 = F32(1.7)
    w2 = np.nextafter(w1, F32(2.0))
    same = (w1 * mu).astype(F32) == (w2 * mu).astype(F32)
    assert same.sum() >= 50 and (~same).sum() >= 50
    num, A, Y = (rng.uniform(0.1, 9.0, N).astype(F32) for _ in range(3))
    e1, e2 = MB.vn_edge_own(num, A, Y, mu, w1), MB.vn_edge_own(num, A, Y, mu, w2)
    assert np.array_equal(e1[same].view(np.uint32), e2[same].view(np.uint32))
    assert (e1[~same] != e2[~same]).any()


# ---- control ----------------------------------------------------------------------------------------------------------------------------------
def ibm72_batch(B=40):
    og = oracle_library_forms("ibm72", stage_one=False)
    return depolarizing(og, P, B)


def test_a_sample_solved_in_attempt_zero_ends_as_with_one_attempt():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    factors, owns = MB.mbp4_tables((1.0, 0.8, 0.6), 0.8)
    x1, z1, s1 = MB.mbp4_decode(c, sx, sz, factors[:1], owns[:1], 6, 4, llr_const=L)
    for restart in (False, True):
        x3, z3, s3 = MB.mbp4_decode(c, sx, sz, factors, owns, 6, 4, restart=restart, llr_const=L)
        first = s1[:, 0] == 1
        assert first.any() and not first.all()
        assert np.array_equal(s3[first], s1[first]) and np.array_equal(x3[first], x1[first]) and np.array_equal(z3[first], z1[first])
        assert (s3[~first, 1] > 0).all()
        assert ((s3[:, 0] == 1) & (s3[:, 1] > 0)).any(), "a later alpha must solve a sample"


def test_restart_with_identical_parameters_repeats_attempt_zero():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    pre, att, A = 5, 5, 4
    f, o = np.full(A, 0.8, F32), np.full(A, 0.9, F32)
    x0, z0, s0 = MB.mbp4_decode(c, sx, sz, f[:1], o[:1], pre, att, restart=True, llr_const=L)
    xh, zh, st = MB.mbp4_decode(c, sx, sz, f, o, pre, att, restart=True, llr_const=L)
    solved = s0[:, 0] == 1
    assert solved.any() and not solved.all()
    assert np.array_equal(st[solved], s0[solved])
    assert np.array_equal(st[~solved], np.tile(np.array([0, A - 1, pre + (A - 1) * att, att], np.int32), ((~solved).sum(), 1)))
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0), "every attempt ends where attempt 0 ended"


def test_without_restart_attempts_of_identical_parameters_are_one_long_attempt():
    c = code("ibm72")
    _, _, sx, sz = ibm72_batch()
    L = llr_const(P)
    T, A = 3, 4
    f, o = np.full(A, 0.8, F32), np.full(A, 0.7, F32)
    x0, z0, s0 = MB.mbp4_decode(c, sx, sz, f[:1], o[:1], A * T, 1, restart=False, llr_const=L)
    xh, zh, st = MB.mbp4_decode(c, sx, sz, f, o, T, T, restart=False, llr_const=L)
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0)
    assert np.array_equal(st[:, 0], s0[:, 0]) and np.array_equal(st[:, 2], s0[:, 2])
    assert np.array_equal(st[:, 1] * T + st[:, 3], s0[:, 3]), "(a, k) counts the same iterations"
    assert (st[:, 1] > 0).any() and (st[:, 0] == 1).any() and (st[:, 0] == 0).any()


# ---- figures ----------------------------------------------------------------------------------------------------------------------------------
GHP882_FIGURES = (1, 6, 5, 384, 0)  # (unsolved, solved only after attempt 0, largest a, largest its, logical errors)


@functools.lru_cache(maxsize=None)
def ghp882_reference(restart=True):
    """The default AMBP4 (alphas 1.0 .. 0.5, 64 iterations each, min-sum, base factor 0.8) on [[882,24]], p = 0.10, samples 0..63."""
    c = code("ghp882")
    _, _, sx, sz = ghp882_samples()
    factors, owns = MB.mbp4_tables(ALPHAS, 0.8)
    return MB.mbp4_decode(c, sx, sz, factors, owns, 64, 64, "minsum", restart=restart, llr_const=llr_const(0.10))


def ghp882_figures(xh, zh, st):
    c = code("ghp882")
    ex, ez, sx, sz = ghp882_samples()
    solved = st[:, 0] == 1
    assert np.array_equal(solves(c, xh, zh, sx, sz), solved)
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64) % 2, np.asarray(c.hz_perp, np.int64) % 2
    logical = (((xd @ hxp.T) % 2).any(1) | ((zd @ hzp.T) % 2).any(1)) & solved
    return int((~solved).sum()), int((solved & (st[:, 1] > 0)).sum()), int(st[:, 1].max()), int(st[:, 2].max()), int(logical.sum())


def test_ghp882_figures():
    """Flooding min-sum BP4-64 leaves 7 of these 64 samples unsolved (pinned by tests/test_bp4fb_reference_cpu.py); the alpha sweep
    must leave strictly fewer and make no logical error among the samples it solves."""
    xh, zh, st = ghp882_reference()
    print("a", st[:, 1].tolist(), "its", st[:, 2].tolist())
    figures = ghp882_figures(xh, zh, st)
    print("figures", figures)
    assert figures[0] < 7 and figures[4] == 0
    assert figures == GHP882_FIGURES
    # attempt 0 of the sweep is flooding BP4-64: the samples it leaves are the 7
    assert int(((st[:, 1] > 0) | (st[:, 0] == 0)).sum()) == 7


# ---- build surface ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_mbp4_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_mbp4_decode\s*\(", text)
    assert "fgnn_mbp4_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_mbp4_decode")
    vn = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "fgnn_vn.h")).read()
    assert re.search(r"FG_FN\s+float\s+vn_edge_own\s*\(", vn)


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    assert callable(F.AMBP4Decoder) and callable(F.BP4_AMBP_Model)
    assert callable(TannerGraph.mbp4_decode)
    assert ALPHA_DEFAULTS == ALPHAS
    f, o = mbp4_tables(ALPHA_DEFAULTS, 0.8)
    f0, o0 = MB.mbp4_tables(ALPHAS, 0.8)
    assert f.dtype == F32 and o.dtype == F32 and f.tobytes() == f0.tobytes() and o.tobytes() == o0.tobytes()
    assert f.tobytes() == np.array([F32(0.8) / F32(x) for x in ALPHAS], F32).tobytes(), "one float32 division each"
