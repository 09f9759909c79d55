"""Soft-syndrome BP4: the restatement tests/dsbp4_reference.py, tied to `mbp4_reference.cn_update` (itself tied to the C oracle) on
the data-syndrome matrix [h | I], to the host build of the rules of fgnn_cn.h with one extra input, and to
`mbp4_reference.mbp4_decode`; checked for what the algorithm at fgnn_dsbp4_decode (include/fgnn.h) states; and the build surface of
the feature.  CPU only."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import dsbp4_reference as DS
import mbp4_reference as MB
from helpers import code, llr_const, oracle_library_forms
from oracle.oracle import _p, lib as oracle_lib
from test_bp4fb_reference_cpu import depolarizing
from test_mbp4_reference_cpu import ALPHAS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
SEED = 0x5EED
# syndrome LLRs the rules must take: zero, small, moderate, the min-sum clip and beyond it, a perfect measurement, negatives
GAMMA_TABLE = np.array([0.0, 1e-3, 0.4, 1.0, 2.5, 4.6, 7.0, 13.0, 20.0, 25.0, INF, -0.7, -3.0, -25.0], F32)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def syndrome_noise_seeds(seed):
    """TannerGraph.syndrome_noise_seeds, restated."""
    step, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1
    return (seed + step) & mask, (seed + 2 * step) & mask


def syndrome_noise(og, seed, q, first, B):
    """The flips TannerGraph.syndrome_noise draws, from the oracle's og_bsc_noise at widths m_x and m_z."""
    out = []
    for s, width in zip(syndrome_noise_seeds(seed), (og.m_x, og.m_z)):
        u = np.empty((B, width), np.uint8)
        oracle_lib().og_bsc_noise(int(s), float(np.float32(q)), int(first), B, width, _p(u))
        out.append(u)
    return out[0], out[1]


def gamma_of_q(q):
    q = F32(q)
    return float(np.log((F32(1.0) - q) / q, dtype=F32))


def noisy_syndromes(name, p, q, B, first=0):
    """(ex, ez, sx ^ ux, sz ^ uz, ux, uz) of the seeded streams."""
    og = oracle_library_forms(name, stage_one=False)
    ex, ez, sx, sz = depolarizing(og, p, B, first)
    ux, uz = syndrome_noise(og, SEED, q, first, B)
    return ex, ez, sx ^ ux, sz ^ uz, ux, uz


# ---- 1: the rule against cn_update on [h | I] ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", ["ibm72", "toric4", "gb126"])
def test_the_soft_rule_is_the_rule_on_the_data_syndrome_matrix(name, cn_type):
    c = code(name)
    rng = np.random.RandomState(0xD5 + len(name))
    B = 12
    for h in (np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2):
        side, wide = MB.Side(h), MB.Side(np.hstack([h, np.eye(h.shape[0], dtype=np.int64)]))
        assert wide.E == side.E + side.m and np.array_equal(wide.v_of[:side.E], side.v_of) and np.array_equal(wide.c_of[:side.E], side.c_of)
        assert np.array_equal(wide.c_of[side.E:], np.arange(side.m)), "the extra edge of check c is edge E + c"
        assert (wide.cn_tab[np.arange(side.m), wide.cn_mask.sum(1) - 1] == side.E + np.arange(side.m)).all(), "and the check's last input"
        nu = (rng.standard_normal((B, side.E)) * 6.0).astype(F32)
        edge = rng.rand(B, side.E) < 0.1  # no subnormal here: boxplus divides by tanh(nu / 2), with or without a soft syndrome
        nu[edge] = rng.choice(np.array([0.0, 20.0, -20.0, 25.0, -1e-3], F32), size=int(edge.sum()))
        synd = rng.randint(0, 2, size=(B, side.m)).astype(np.uint8)
        gamma = GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=(B, side.m))]
        assert np.isinf(gamma).any() and (gamma == 0).any() and (gamma < 0).any()
        for factor in (F32(1.0), F32(0.8)):
            mu, w = DS.soft_cn_update(side, nu, synd, gamma, cn_type, factor)
            ref = MB.cn_update(wide, np.concatenate([nu, gamma], axis=1), synd, cn_type, factor)
            assert not np.isnan(ref).any() and not np.isnan(w).any()
            assert np.array_equal(bits(mu), bits(ref[:, :side.E])), "real edges"
            assert np.array_equal(bits(w), bits(ref[:, side.E:])), "the extra edge's output is w_c"
            assert not DS.u_hat_of(gamma, w)[np.isposinf(gamma)].any(), "a perfect measurement is never estimated wrong"


# ---- 2: the header ------------------------------------------------------------------------------------------------------------------------------
DMAX = 12


def rule_rows():
    """(deg, syndrome bit, gamma, factor, 12 inputs) rows: degrees 2 .. 12, seeded inputs in the ranges the decoder forms with gamma from
    the table, and edge rows: zeros, the +-20 clip, subnormals, gamma = +inf, duplicate minima that include gamma."""
    rng = np.random.RandomState(0x50F7)
    N = 3000
    rows = np.zeros((N, 4 + DMAX), F32)
    rows[:, 0] = rng.randint(2, DMAX + 1, size=N)
    rows[:N // 3, 0] = 6  # the compile-time degree of the register form
    rows[:, 1] = rng.randint(0, 2, size=N)
    rows[:, 2] = GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=N)]
    rows[:, 3] = rng.choice(np.array([1.0, 0.8, 0.8 / 0.7, 1.6], F32), size=N)
    rows[:, 4:] = (rng.standard_normal((N, DMAX)) * 5.0).astype(F32)
    clip = rng.rand(N, DMAX) < 0.08
    rows[:, 4:][clip] = rng.choice(np.array([20.0, -20.0, 25.0, -31.0, 0.0, -0.0, 1e-40, -1.4e-45, 1e-3], F32), size=int(clip.sum()))

    def row(deg, s, g, f, vals):
        r = np.zeros(4 + DMAX, F32)
        r[:4] = (deg, s, g, f)
        r[4:4 + len(vals)] = vals
        return r

    edge = [row(6, 0, 0.0, 1.0, [0.0] * 6), row(6, 1, INF, 0.8, [20.0, -20.0, 25.0, -25.0, 20.0, 19.999998]),
            row(6, 0, 20.0, 0.8, [20.0] * 6), row(6, 1, 25.0, 1.0, [21.0, 22.0, -23.0, 24.0, 25.0, 26.0]),
            row(6, 0, 1.5, 0.8, [1.5, 3.0, -1.5, 4.0, 5.0, 6.0]), row(6, 1, 1.5, 0.8, [2.0, 3.0, -1.5, 4.0, 5.0, 6.0]),
            row(6, 0, -1.5, 0.8, [2.0, 3.0, 1.5, 4.0, 5.0, 6.0]), row(6, 0, 1e-40, 1.0, [1e-40, -1.4e-45, 1e-39, 0.0, 2.0, 3.0]),
            row(2, 1, INF, 0.8, [3.0, -4.0]), row(2, 0, 0.0, 0.8, [3.0, -4.0]), row(12, 1, 2.0, 0.8, [2.0] * 12),
            row(12, 0, INF, 1.0, [1e-3] * 12), row(3, 0, 1e-3, 1.0, [0.0, 0.0, 7.0]), row(7, 1, -25.0, 0.8, [9.0, -8.0, 7.0, -6.0, 5.0, -4.0, 3.0])]
    return np.concatenate([np.stack(edge), rows])


_BUILD = tempfile.TemporaryDirectory()  # the builds of cn_rule_check.cpp, one per set of flags, shared by the tests that run it


@functools.lru_cache(maxsize=None)
def cn_rule_exe(flags):
    src = os.path.join(ROOT, "tests", "cn_rule_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    exe = os.path.join(_BUILD.name, "cn_rule_check" + "".join(re.sub(r"\W", "_", f) for f in flags))
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function"] + list(flags) +
                        ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    return exe


def run_cn_rule_check(flags, table):
    """[N, 5 * 14] words of tests/cn_rule_check.cpp, built with `flags`, on (deg, syndrome bit, number of extras, factor, extra 0,
    extra 1, 12 inputs) rows."""
    run = subprocess.run([cn_rule_exe(tuple(flags))], input=np.ascontiguousarray(table, dtype=F32).tobytes(), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(table), run.stdout[-2000:]
    return np.array([[int(h, 16) for h in ln.split()] for ln in lines], np.uint32)


def build_and_run(flags, table):
    """The (deg, syndrome bit, gamma, factor, 12 inputs) rows as rows with one extra input, gamma; [N, 5 * 13] words: the 12 slots and
    w of each group.  The word of the second extra input, which these rows do not have, is 0."""
    one = np.zeros((len(table), 6 + DMAX), F32)
    one[:, 0], one[:, 1], one[:, 2], one[:, 3], one[:, 4], one[:, 6:] = table[:, 0], table[:, 1], 1, table[:, 3], table[:, 2], table[:, 4:]
    got = run_cn_rule_check(flags, one).reshape(len(table), 5, 14)
    assert not got[:, :, 13].any()
    return np.ascontiguousarray(got[:, :, :13]).reshape(len(table), 5 * 13)


@functools.lru_cache(maxsize=None)
def rule_rows_reference():
    """{cn_type: [R, 13] bits} of the restatement on rule_rows(): the 12 slots, then w."""
    rows = rule_rows()
    deg = rows[:, 0].astype(int)
    mask = np.arange(DMAX)[None, :] < deg[:, None]
    want = {}
    for cn in CN_TYPES:
        out, w = DS.soft_rule(rows[:, 4:].copy(), mask, rows[:, 1] != 0, rows[:, 2].copy(), cn, rows[:, 3].copy())
        assert not np.isnan(out).any() and not np.isnan(w).any()
        want[cn] = np.concatenate([bits(out), bits(w)[:, None]], axis=1)
    return want


def same_bits(got, want):
    return (got == want).all(1)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_rules_of_the_header_equal_the_restatement_bitwise(flags):
    rows = rule_rows()
    got = build_and_run(flags, rows)
    assert got.shape == (len(rows), 5 * 13)
    want = rule_rows_reference()
    for g, cn in enumerate(CN_TYPES):  # the loop form
        bad = np.nonzero(~same_bits(got[:, 13 * g:13 * g + 13], want[cn]))[0]
        assert len(bad) == 0, (cn, bad[:10], rows[bad[:3]])
    bad = np.nonzero(~same_bits(got[:, 39:52], want["minsum"]))[0]
    assert len(bad) == 0, ("register form, guarded", bad[:10])
    six = rows[:, 0] == 6
    assert six.sum() > 500 and same_bits(got[six, 52:65], want["minsum"][six]).all(), "register form at its compile-time degree"
    assert not got[~six, 52:65].any()
    # the table reaches what it says: duplicate minima that include gamma, and gamma as the only minimum
    a = np.minimum(np.abs(rows[:, 4:]), 20)
    a[np.arange(DMAX)[None, :] >= rows[:, 0:1]] = np.inf
    ag = np.minimum(np.abs(rows[:, 2]), 20)
    assert ((a.min(1) == ag).sum() >= 5) and ((a.min(1) > ag).sum() >= 100) and ((a.min(1) < ag).sum() >= 100)


# ---- 3: the decoder anchor --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("ibm72", 0.10), ("rsurf5", 0.15)])
def test_minsum_with_perfect_measurements_is_mbp4(name, p):
    c = code(name)
    hx, hz = np.asarray(c.hx) % 2, np.asarray(c.hz) % 2
    assert hx.sum(1).min() >= 2 and hz.sum(1).min() >= 2, "the equality needs checks of degree >= 2"
    og = oracle_library_forms(name, stage_one=False)
    _, _, sx, sz = depolarizing(og, p, 32)
    L = llr_const(p)
    for alphas in ((1.0,), ALPHAS):
        factors, owns = MB.mbp4_tables(alphas, 0.8)
        for restart in (True, False):
            x0, z0, s0 = MB.mbp4_decode(c, sx, sz, factors, owns, 6, 4, "minsum", restart=restart, llr_const=L)
            xh, zh, ux, uz, st = DS.dsbp4_decode(c, sx, sz, factors, owns, 6, 4, "minsum", restart=restart, llr_const=L)
            assert xh.tobytes() == x0.tobytes() and zh.tobytes() == z0.tobytes() and np.array_equal(st, s0)
            assert not ux.any() and not uz.any()
        assert (s0[:, 0] == 1).any() and (s0[:, 0] == 0).any()
    assert (s0[:, 1] > 0).any()


# ---- 4: the meaning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_one_iteration_is_bp4_on_the_data_syndrome_code(cn_type):
    """With pre_iter = 1 and one attempt, soft-syndrome BP4 is BP4 on hx' = [hx | I | 0], hz' = [hz | 0 | I] with the priors (X, Y, Z) =
    (big, big, gamma) on an hx check's qubit and (gamma, big, big) on an hz check's: at the first update the extra qubit's message is
    0 - (log(1 + e^-20) - gamma), and log(1 + e^-20) = 2.06e-9 is far below half an ulp of any gamma in [0.5, 8] (2.98e-8 at least), so
    it is gamma bit for bit.  Beyond the first iteration the data-syndrome route forms (gamma + mu) - mu and the two differ in bits."""
    c = code("ibm72")
    hx, hz = np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2
    (mx, n), mz = hx.shape, hz.shape[0]
    wide = types.SimpleNamespace(hx=np.hstack([hx, np.eye(mx, dtype=np.int64), np.zeros((mx, mz), np.int64)]),
                                 hz=np.hstack([hz, np.zeros((mz, mx), np.int64), np.eye(mz, dtype=np.int64)]))
    B, p, big = 48, 0.10, F32(1e4)
    _, _, sx, sz, ux, uz = noisy_syndromes("ibm72", p, 0.05, B)
    rng = np.random.RandomState(41)
    gx, gz = rng.uniform(0.5, 8.0, (B, mx)).astype(F32), rng.uniform(0.5, 8.0, (B, mz)).astype(F32)
    L = llr_const(p)
    lam = np.full((B, 3, n + mx + mz), F32(L), F32)
    lam[:, 0, n:n + mx], lam[:, 1, n:n + mx], lam[:, 2, n:n + mx] = big, big, gx
    lam[:, 0, n + mx:], lam[:, 1, n + mx:], lam[:, 2, n + mx:] = gz, big, big
    f, o = np.array([0.8], F32), np.array([1.0], F32)
    xh, zh, uxh, uzh, st = DS.dsbp4_decode(c, sx, sz, f, o, 1, 1, cn_type, llr_const=L, synd_llr_x=gx, synd_llr_z=gz)
    x1, z1, s1 = MB.mbp4_decode(wide, sx, sz, f, o, 1, 1, cn_type, llr_ch=lam)
    assert np.array_equal(x1[:, :n], xh) and np.array_equal(z1[:, :n], zh), "the decisions on the real qubits"
    assert np.array_equal(z1[:, n:n + mx], uxh), "an hx check's qubit carries a Z component iff u_hat"
    assert np.array_equal(x1[:, n + mx:], uzh), "an hz check's qubit carries an X component iff u_hat"
    assert np.array_equal(s1, st)
    assert uxh.any() and uzh.any() and (uxh != ux).any() and (st[:, 0] == 0).any()


# ---- 5: control and stats -----------------------------------------------------------------------------------------------------------------------
Q_BATCH = 0.02


@functools.lru_cache(maxsize=None)
def ibm72_noisy_batch(B=96):
    """ibm72 at p = 0.10 with syndrome flips at q = 0.02, decoded by one attempt of 12 iterations and by three alphas of 6.  q is 0.02
    and not 0.05: at 0.05 a sample draws 3.6 flips on its 72 checks, 1 sample in 40 draws none, and the seeded batch of 96 then holds
    one sample solved with u_hat = 0 under one attempt and none under the sweep (counted: (1, 18, 16, 77) and (0, 16, 12, 80) for the
    four outcomes below); at 0.02 it holds (24, 21, 21, 51) and (20, 16, 13, 60)."""
    c = code("ibm72")
    ex, ez, sx, sz, ux, uz = noisy_syndromes("ibm72", 0.10, Q_BATCH, B)
    g = gamma_of_q(Q_BATCH)
    one = DS.dsbp4_decode(c, sx, sz, *MB.mbp4_tables((1.0,), 0.8), 12, 12, llr_const=llr_const(0.10), gamma_x=g, gamma_z=g)
    sweep = DS.dsbp4_decode(c, sx, sz, *MB.mbp4_tables((1.0, 0.8, 0.6), 0.8), 6, 6, llr_const=llr_const(0.10), gamma_x=g, gamma_z=g)
    return (sx, sz, ux, uz), one, sweep


def test_a_noisy_batch_holds_every_outcome_and_solved_means_the_joint_test():
    c = code("ibm72")
    (sx, sz, ux, uz), one, sweep = ibm72_noisy_batch()
    for xh, zh, uxh, uzh, st in (one, sweep):
        solved = st[:, 0] == 1
        u, uh = np.concatenate([ux, uz], 1), np.concatenate([uxh, uzh], 1)
        kinds = (int((solved & ~uh.any(1)).sum()), int((solved & uh.any(1)).sum()),
                 int((solved & (uh == u).all(1) & u.any(1)).sum()), int((~solved).sum()))
        print("solved with u_hat = 0, solved with u_hat != 0, solved with u_hat = u != 0, unsolved:", kinds)
        assert all(kinds), kinds
        ok = DS.joint_test(c, xh, zh, uxh, uzh, sx, sz)
        assert np.array_equal(ok, solved), "solved is the joint test of the last decisions; an unsolved sample's last test failed"
    assert (sweep[4][:, 1] > 0).any() and ((sweep[4][:, 0] == 1) & (sweep[4][:, 1] > 0)).any(), "a later alpha must solve a sample"
    first = one[4][:, 3] <= 6
    assert first.any() and np.array_equal(sweep[4][first & (one[4][:, 0] == 1)], one[4][first & (one[4][:, 0] == 1)])


def test_gamma_zero_silences_a_check_under_minsum():
    c = code("ibm72")
    G = MB.graph_of(c)
    rng = np.random.RandomState(9)
    B, chk = 6, 5
    nu = (rng.standard_normal((B, G.x.E)) * 4.0).astype(F32)
    synd = rng.randint(0, 2, size=(B, G.x.m)).astype(np.uint8)
    gamma = np.full((B, G.x.m), F32(3.0), F32)
    gamma[:, chk] = 0.0
    mu, w = DS.soft_cn_update(G.x, nu, synd, gamma, "minsum", F32(0.8))
    on = G.x.c_of == chk
    assert on.sum() == 6 and (mu[:, on] == 0).all() and (mu[:, ~on] != 0).all()
    assert (w[:, chk] != 0).all(), "the unreliable bit itself hears the other inputs"


# ---- 6: the build surface -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_dsbp4_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_dsbp4_decode\s*\(", text)
    assert "fgnn_dsbp4_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_dsbp4_decode")
    # the rule the kernel calls is declared FG_FN, so it is host-callable: tests/cn_rule_check.cpp runs it
    rule = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "fgnn_cn.h")).read()
    assert re.search(r"FG_FN\s+void\s+cn_update\s*\(", rule) and re.search(r"FG_FN\s+void\s+cn_minsum_regular\s*\(", rule)


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.SoftSyndromeBP4Decoder) and callable(F.BP4_SoftSyndrome_Model)
    assert callable(TannerGraph.dsbp4_decode) and callable(TannerGraph.syndrome_noise)
    assert TannerGraph.syndrome_noise_seeds(SEED) == syndrome_noise_seeds(SEED)
    assert len({SEED} | set(syndrome_noise_seeds(SEED))) == 3
