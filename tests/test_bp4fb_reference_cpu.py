"""BP4 with prior feedback: the restatement tests/bp4fb_reference.py, tied to the C oracle's BP4 and to the BP4-GD restatement, and
checked for what the two rules state; and the build surface of the feature (header, library export, public classes).  CPU only.

Anchor.  With max_attempts = 0 no feedback step is made, lamhat stays the channel LLRs: the result is that of BP4-GD with max_rounds = 0,
which tests/test_bp4gd_reference_cpu.py ties to plain BP4 stopped at its first solution."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import bp4fb_reference as FB
import bp4gd_reference as GD
from helpers import code, llr_const, oracle_library_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 0x5EED
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
STRENGTH = {"perturb": 2.0, "enhanced": 10.0}
PRE, ATT, A, P, B40 = 6, 3, 8, 0.10, 40  # the fixed batch on ibm72


def depolarizing(og, p, B, first=0):
    """Seeded depolarizing noise (the oracle's Philox stream) and its two syndromes."""
    ex, ez = og.pauli_noise(SEED, p, first, B)
    sx, sz = og.syndrome(ex, ez)
    return ex, ez, sx, sz


def solves(c, xh, zh, sx, sz):
    hx, hz = np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2
    return ((xh.astype(np.int64) @ hz.T) % 2 == sz).all(1) & ((zh.astype(np.int64) @ hx.T) % 2 == sx).all(1)


def unsatisfied(c, d, sx, sz):
    """The checks (hx first, then hz) whose parity on the decisions d [n] differs from the syndrome bit."""
    hx, hz = np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2
    par = np.concatenate([((d >> 1).astype(np.int64) @ hx.T) % 2, ((d & 1).astype(np.int64) @ hz.T) % 2])
    return np.nonzero(par != np.concatenate([sx, sz]))[0]


class RecordingOracle:
    """An OracleGraph that keeps the llr_ch of every bp4_decode call of a one-sample batch."""

    def __init__(self, og):
        self._og, self.llr = og, []

    def __getattr__(self, name):
        return getattr(self._og, name)

    def bp4_decode(self, synd_x, *args, **kw):
        assert len(synd_x) == 1
        self.llr.append(np.array(kw["llr_ch"][0], F32))
        return self._og.bp4_decode(synd_x, *args, **kw)


@functools.lru_cache(maxsize=None)
def recorded(rule, restart=False, att=ATT):
    """The fixed batch on ibm72 decoded sample by sample (sample b as global sample b) through a recording oracle, with per-qubit LLRs:
    (lam, sx, sz, per sample (stats row, x_hat, z_hat, recorded llr_ch list, feedback log))."""
    og = oracle_library_forms("ibm72", stage_one=False)
    _, _, sx, sz = depolarizing(og, P, B40)
    lam = np.random.RandomState(5).uniform(2.0, 4.5, size=(B40, 3, og.n)).astype(F32)
    rows = []
    for b in range(B40):
        rec, log = RecordingOracle(og), []
        xh, zh, st = FB.bp4fb_decode(rec, sx[b:b + 1], sz[b:b + 1], rule, PRE, att, A, STRENGTH[rule], "minsum", 0.8, restart=restart,
                                     seed=SEED, first_sample=b, llr_ch=lam[b:b + 1], log=log)
        found, a, its, k = st[0]
        assert len(rec.llr) == its == (k if a == 0 else PRE + (a - 1) * att + k) and len(log) == a
        rows.append((st[0], xh[0], zh[0], rec.llr, log))
    return lam, sx, sz, rows


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_no_attempts_is_bp4gd_without_rounds(cn_type):
    og = oracle_library_forms("ibm72", stage_one=False)
    B, T = 32, 12
    _, _, sx, sz = depolarizing(og, P, B)
    per_qubit = np.random.RandomState(3).uniform(1.0, 6.0, size=(B, 3, og.n)).astype(F32)
    for rule in FB.RULES:
        for llr in (dict(llr_const=llr_const(P)), dict(llr_ch=per_qubit)):
            x0, z0, s0, _ = GD.bp4gd_decode(og, sx, sz, T, 5, 0, 25.0, cn_type, 0.8, **llr)
            xh, zh, st = FB.bp4fb_decode(og, sx, sz, rule, T, 5, 0, STRENGTH[rule], cn_type, 0.8, **llr)
            assert np.array_equal(xh, x0) and np.array_equal(zh, z0) and np.array_equal(st, s0) and not st[:, 1].any()
            assert (st[:, 0] == 1).any() and (st[:, 0] == 0).any()


def test_perturb_changes_exactly_the_qubits_of_the_unsatisfied_checks():
    """At every attempt a >= 1 the BP4 steps see lam - F * u, bitwise, on the qubits of the checks the previous attempt's last test
    left unsatisfied, and lam everywhere else: so nothing accumulates across attempts."""
    c = code("ibm72")
    H = np.concatenate([np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2])
    lam, sx, sz, rows = recorded("perturb")
    F = F32(STRENGTH["perturb"])
    steps = returned = 0
    for b, (st, _, _, llr, log) in enumerate(rows):
        assert all(np.array_equal(l, lam[b]) for l in llr[:PRE]), "no feedback before the first attempt ends"
        before = np.zeros(H.shape[1], bool)
        for e in log:
            a = e["att"]
            seen = llr[PRE + (a - 1) * ATT:PRE + a * ATT]
            assert len(seen) >= 1 and all(np.array_equal(l, seen[0]) for l in seen), "lamhat is fixed within an attempt"
            support = H[unsatisfied(c, e["d"], sx[b], sz[b])].sum(0) > 0
            assert support.any()
            want = lam[b].copy()
            for v in np.nonzero(support)[0]:
                w = FB.draw(SEED, b, int(v), a, 3)
                for row in range(3):
                    want[row, v] = lam[b, row, v] - F * FB.unit(w[row])
            assert seen[0].tobytes() == want.tobytes(), (b, a)
            assert np.array_equal((seen[0] != lam[b]).any(0), support), (b, a)
            assert (seen[0] <= lam[b]).all() and (seen[0] >= lam[b] - F).all()
            returned += int((before & ~support).sum())
            before = support
            steps += 1
    assert steps > B40 and returned > 0, "qubits must leave the support again, and then carry lam"


def test_enhanced_changes_one_qubit_of_one_unsatisfied_check():
    """At every attempt a >= 1 exactly one qubit differs from lam: it lies on a check the previous test left unsatisfied, and two of its
    LLRs (Z and Y for an hx check, X and Y for an hz check) are lam - F when the check's syndrome bit is 1 and lam + F when it is 0."""
    c = code("ibm72")
    H = np.concatenate([np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2])
    m_x = np.asarray(c.hx).shape[0]
    lam, sx, sz, rows = recorded("enhanced")
    F = F32(STRENGTH["enhanced"])
    cases = set()
    for b, (st, _, _, llr, log) in enumerate(rows):
        assert all(np.array_equal(l, lam[b]) for l in llr[:PRE])
        synd = np.concatenate([sx[b], sz[b]])
        for e in log:
            a = e["att"]
            seen = llr[PRE + (a - 1) * ATT:PRE + a * ATT]
            assert len(seen) >= 1 and all(np.array_equal(l, seen[0]) for l in seen)
            diff = seen[0] != lam[b]
            vs = np.nonzero(diff.any(0))[0]
            assert len(vs) == 1, (b, a, vs)
            v = int(vs[0])
            changed = tuple(np.nonzero(diff[:, v])[0])
            assert changed in ((1, 2), (0, 1)), changed  # rows X, Y, Z of llr_ch
            side = 0 if changed == (1, 2) else 1
            U = unsatisfied(c, e["d"], sx[b], sz[b])
            cands = [int(u) for u in U if H[u, v] and (u >= m_x) == bool(side)]
            assert cands, "the qubit lies on no unsatisfied check of the side its change names"
            assert e["check"] in cands and e["qubit"] == v
            s = int(synd[e["check"]])
            t = -F if s else F
            for row in changed:
                assert seen[0][row, v] == lam[b, row, v] + t, (b, a, row)
            # the draws: largest key among U, then the j-th qubit of the check
            keys = {int(u): (int(FB.draw(SEED, b, int(u), a, 4)[0]) << 32) | (0xFFFFFFFF - int(u)) for u in U}
            assert max(keys, key=keys.get) == e["check"]
            q = np.nonzero(H[e["check"]])[0]
            assert q[FB.fy_pick(FB.unit(FB.draw(SEED, b, e["check"], a, 4)[1]), len(q))] == v
            cases.add((side, s))
    assert cases == {(0, 0), (0, 1), (1, 0), (1, 1)}, f"every (side, syndrome bit) case must occur, got {cases}"


@pytest.mark.parametrize("rule", FB.RULES)
def test_zero_strength_with_restart_repeats_attempt_zero(rule):
    og = oracle_library_forms("ibm72", stage_one=False)
    T, attempts = 5, 3
    _, _, sx, sz = depolarizing(og, P, B40)
    L = llr_const(P)
    x0, z0, s0 = FB.bp4fb_decode(og, sx, sz, rule, T, T, 0, 0.0, "minsum", 0.8, restart=True, llr_const=L)
    xh, zh, st = FB.bp4fb_decode(og, sx, sz, rule, T, T, attempts, 0.0, "minsum", 0.8, restart=True, llr_const=L)
    solved = s0[:, 0] == 1
    assert solved.any() and not solved.all()
    assert np.array_equal(st[solved], s0[solved]), "a sample solved in attempt 0 ends as with no attempts"
    assert np.array_equal(st[~solved], np.tile(np.array([0, attempts, T + attempts * T, T], np.int32), ((~solved).sum(), 1)))
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0), "every attempt ends where attempt 0 ended"


@pytest.mark.parametrize("rule", FB.RULES)
def test_restart_runs_plain_bp4_on_the_attempts_lamhat(rule):
    """With restart a sample that stops at (a, k) carries the decisions of plain BP4 with num_iter = k from zero messages on the lamhat
    of attempt a."""
    og = oracle_library_forms("ibm72", stage_one=False)
    lam, sx, sz, rows = recorded(rule, True, 12)  # three iterations from zero messages solve nothing
    later = 0
    for b, (st, xh, zh, llr, log) in enumerate(rows):
        found, a, its, k = st
        out = og.bp4_decode(sx[b:b + 1], sz[b:b + 1], int(k), "minsum", 0.8, llr_ch=llr[-1][None])
        assert np.array_equal(out["x_hat"][0], xh) and np.array_equal(out["z_hat"][0], zh), (b, a, k)
        later += int(a > 0 and found == 1)
    assert later > 0, "samples must be solved in a later attempt"


@pytest.mark.parametrize("rule", FB.RULES)
def test_a_shard_decodes_its_samples_as_the_whole_batch_does(rule):
    og = oracle_library_forms("ibm72", stage_one=False)
    _, _, sx, sz = depolarizing(og, P, 32)
    _, _, sx1, sz1 = depolarizing(og, P, 16, first=16)
    assert np.array_equal(sx[16:], sx1) and np.array_equal(sz[16:], sz1)
    args = (rule, PRE, ATT, A, STRENGTH[rule], "minsum", 0.8)
    xh, zh, st = FB.bp4fb_decode(og, sx, sz, *args, llr_const=llr_const(P))
    x1, z1, s1 = FB.bp4fb_decode(og, sx1, sz1, *args, first_sample=16, llr_const=llr_const(P))
    assert np.array_equal(xh[16:], x1) and np.array_equal(zh[16:], z1) and np.array_equal(st[16:], s1)
    assert (s1[:, 1] > 0).any()
    x2, z2, s2 = FB.bp4fb_decode(og, sx1, sz1, *args, first_sample=0, llr_const=llr_const(P))
    assert not (np.array_equal(x2, x1) and np.array_equal(z2, z1) and np.array_equal(s2, s1)), "the draws depend on the sample index"


def ibm72_split(rule):
    """(solved before feedback, solved after feedback, never solved) of the fixed batch, constant prior, messages kept."""
    og = oracle_library_forms("ibm72", stage_one=False)
    _, _, sx, sz = depolarizing(og, P, B40)
    _, _, st = FB.bp4fb_decode(og, sx, sz, rule, PRE, ATT, A, STRENGTH[rule], "minsum", 0.8, llr_const=llr_const(P))
    solved = st[:, 0] == 1
    return int((solved & (st[:, 1] == 0)).sum()), int((solved & (st[:, 1] > 0)).sum()), int((~solved).sum())


def test_ibm72_splits():
    assert ibm72_split("perturb") == (22, 15, 3)
    assert ibm72_split("enhanced") == (22, 14, 4)


@functools.lru_cache(maxsize=None)
def ghp882_samples():
    og = oracle_library_forms("ghp882", stage_one=False)
    return depolarizing(og, 0.10, 64)


def ghp882_figures(rule, pre, att, attempts, strength):
    """(unsolved, solved only after feedback, largest a, largest its, logical errors) on [[882,24]], p = 0.10, samples 0..63, min-sum
    at factor 0.8, the prior of p, messages kept."""
    og, c = oracle_library_forms("ghp882", stage_one=False), code("ghp882")
    ex, ez, sx, sz = ghp882_samples()
    xh, zh, st = FB.bp4fb_decode(og, sx, sz, rule, pre, att, attempts, strength, "minsum", 0.8, llr_const=llr_const(0.10))
    print(rule, "a", st[:, 1].tolist(), "its", st[:, 2].tolist())
    solved = st[:, 0] == 1
    assert np.array_equal(solves(c, xh, zh, sx, sz), solved)
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64) % 2, np.asarray(c.hz_perp, np.int64) % 2
    logical = ((xd @ hxp.T) % 2).any(1) | ((zd @ hzp.T) % 2).any(1) | ~solved
    return int((~solved).sum()), int((solved & (st[:, 1] > 0)).sum()), int(st[:, 1].max()), int(st[:, 2].max()), int(logical.sum())


def test_ghp882_flooding_leaves_seven():
    assert ghp882_figures("perturb", 64, 1, 0, 0.0)[0] == 7


def test_ghp882_perturb_figures():
    assert ghp882_figures("perturb", 32, 8, 40, 2.0) == (0, 23, 10, 106, 0)


def test_ghp882_enhanced_figures():
    assert ghp882_figures("enhanced", 32, 16, 20, 10.0) == (0, 23, 5, 97, 0)


def test_header_declares_and_library_exports_bp4fb_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_bp4fb_decode\s*\(", text)
    assert re.search(r"FGNN_FB_PERTURB\s*=\s*0\s*,\s*FGNN_FB_ENHANCED\s*=\s*1", text)
    assert "fgnn_bp4fb_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_bp4fb_decode")


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    from feedback_gnn_amd.prior_feedback import RULE_DEFAULTS
    assert callable(F.BP4FeedbackDecoder) and callable(F.BP4_Feedback_Model)
    assert callable(TannerGraph.bp4fb_decode)
    assert RULE_DEFAULTS == {"perturb": (8, 40, 2.0), "enhanced": (16, 20, 10.0)}
