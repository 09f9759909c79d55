"""Augmented BP4: the restatement tests/bp4aug_reference.py, tied to BP4 on the literally augmented code (run by the MBP4 restatement
and by the C oracle) and to the BP4-GD restatement, and checked for what fgnn_bp4aug_decode (include/fgnn.h) states; the host build of
vn_sums_dup; and the build surface of the feature (header, library export, public classes).  CPU only.

Anchor.  Insert the copy of a check row directly after its original: in flooding BP from zero messages the copy sees the inputs of its
original in the same order, so its messages equal the original's bit for bit, and a qubit's ascending sum meets the two equal messages
one after the other.  So attempt a >= 1 of a restarting decoder IS plain BP4 on the code with the marked rows inserted, and the
restatement's duplicated sum is held to that, for all three check rules."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bp4aug_reference as AU
import bp4gd_reference as GD
import mbp4_reference as MB
from helpers import _bare_code, code, llr_const, oracle_library_forms
from test_bp4fb_reference_cpu import depolarizing, ghp882_samples, solves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 0x5EED
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
P = 0.10
P_TIE = {"ibm72": 0.10, "steane": 0.15, "toric4": 0.2}


def one(x):
    return np.array([x], F32)


def split(stats):
    """(solved in attempt 0, solved later, unsolved)."""
    solved = stats[:, 0] > 0
    return int((solved & (stats[:, 1] == 0)).sum()), int((solved & (stats[:, 1] > 0)).sum()), int((~solved).sum())


# ---- the anchor: BP4 on the code with the rows inserted ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", ["ibm72", "steane", "toric4"])
def test_a_restarting_attempt_is_bp4_on_the_code_with_the_rows_inserted(name, cn_type):
    """A fixed set of about 30 % of the rows, one attempt of 7 iterations after 3: every sample that reaches attempt 1 ends with the
    decisions, found and k of BP4 stopped at its first solution on the doubled code (the MBP4 restatement with own = 1), and with the
    decisions of the oracle's BP4 with num_iter = k on it."""
    from oracle.oracle import OracleGraph
    c, og = code(name), oracle_library_forms(name, stage_one=False)
    p, T = P_TIE[name], 7
    _, _, sx, sz = depolarizing(og, p, 24)
    dup = np.zeros(og.m_x + og.m_z, bool)
    dup[(np.random.RandomState(3).rand(len(dup)) < 0.25) | (np.arange(len(dup)) % og.m_x == 1)] = True  # seeded, and a row of each side
    assert 0.2 < dup.mean() <= 0.5 and dup[:og.m_x].any() and dup[og.m_x:].any()
    hx2, hz2, rx, rz = AU.doubled_code(c, dup)
    assert hx2.shape[0] == og.m_x + dup[:og.m_x].sum() and hz2.shape[0] == og.m_z + dup[og.m_x:].sum()
    c2 = _bare_code(hx2, hz2)
    og2 = OracleGraph(c2, stage_one=False, forms="library-default")
    L = llr_const(p)
    xa, za, sa = AU.bp4aug_decode(c, sx, sz, 3, T, 1, 0.5, cn_type, 0.8, restart=True, llr_const=L, fixed=dup)
    xm, zm, sm = MB.mbp4_decode(c2, sx[:, rx], sz[:, rz], one(0.8), one(1.0), T, 1, cn_type, llr_const=L)
    late = sa[:, 1] == 1
    assert late.sum() >= 5, "samples must reach the attempt"
    assert name != "ibm72" or (sa[late, 0] == 1).any(), "on ibm72 the attempt solves samples, under every rule"
    assert xa[late].tobytes() == xm[late].tobytes() and za[late].tobytes() == zm[late].tobytes()
    assert np.array_equal(sa[late][:, [0, 3]], sm[late][:, [0, 3]]) and np.array_equal(sa[late, 2], 3 + sm[late, 2])
    for b in np.nonzero(late)[0]:
        o = og2.bp4_decode(sx[b:b + 1][:, rx], sz[b:b + 1][:, rz], int(sa[b, 3]), cn_type, 0.8, llr_const=L)
        assert np.array_equal(o["x_hat"][0], xa[b]) and np.array_equal(o["z_hat"][0], za[b]), (b, sa[b])
    # the marks matter: without them the attempt ends elsewhere
    x0, z0, s0 = AU.bp4aug_decode(c, sx, sz, 3, T, 1, 0.5, cn_type, 0.8, restart=True, llr_const=L, fixed=np.zeros_like(dup))
    assert not (np.array_equal(x0, xa) and np.array_equal(z0, za) and np.array_equal(s0, sa))


# ---- the draws -------------------------------------------------------------------------------------------------------------------------------
def test_density_one_duplicates_every_row_and_density_zero_none():
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    m = og.m_x + og.m_z
    for sample, a in ((0, 1), (7, 3), ((1 << 32) + 5, 65535)):
        assert AU.marks(SEED, sample, m, a, 1.0).all() and not AU.marks(SEED, sample, m, a, 0.0).any()
    _, _, sx, sz = depolarizing(og, P, 16)
    L = llr_const(P)
    for restart in (False, True):
        log = []
        got = AU.bp4aug_decode(c, sx, sz, 4, 5, 2, 1.0, "minsum", 0.8, restart=restart, llr_const=L, log=log)
        want = AU.bp4aug_decode(c, sx, sz, 4, 5, 2, 0.5, "minsum", 0.8, restart=restart, llr_const=L, fixed=np.ones(m, bool))
        assert len(log) > 0 and all(d.all() for _, _, d in log)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_the_marked_fraction_is_the_density():
    """Over many draws the fraction of marked rows lies within 4 sigma of the density."""
    m = 72
    for density in (0.05, 0.1, 0.3):
        d = np.concatenate([AU.marks(SEED, sample, m, a, density) for sample in range(12) for a in range(1, 9)])
        sigma = np.sqrt(density * (1 - density) / d.size)
        assert abs(d.mean() - density) < 4 * sigma, (density, d.mean(), sigma)
    # a draw is a function of (seed, sample, attempt, check) alone
    base = AU.marks(SEED, 3, m, 2, 0.3)
    assert np.array_equal(base, AU.marks(SEED, 3, m, 2, 0.3))
    for other in (AU.marks(SEED + 1, 3, m, 2, 0.3), AU.marks(SEED, 4, m, 2, 0.3), AU.marks(SEED, 3, m, 3, 0.3),
                  AU.marks(SEED, 3 + (1 << 32), m, 2, 0.3)):
        assert not np.array_equal(base, other)
    # a larger density marks a superset: the compare is against one uniform per row
    assert not (base & ~AU.marks(SEED, 3, m, 2, 0.5)).any()


def test_density_zero_with_restart_repeats_attempt_zero():
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    T, attempts = 5, 3
    _, _, sx, sz = depolarizing(og, P, 40)
    L = llr_const(P)
    x0, z0, s0 = AU.bp4aug_decode(c, sx, sz, T, T, 0, 0.0, "minsum", 0.8, restart=True, llr_const=L)
    xh, zh, st = AU.bp4aug_decode(c, sx, sz, T, T, attempts, 0.0, "minsum", 0.8, restart=True, llr_const=L)
    solved = s0[:, 0] == 1
    assert solved.any() and not solved.all()
    assert np.array_equal(st[solved], s0[solved]), "a sample solved in attempt 0 ends as with no attempts"
    assert np.array_equal(st[~solved], np.tile(np.array([0, attempts, T + attempts * T, T], np.int32), ((~solved).sum(), 1)))
    assert np.array_equal(xh, x0) and np.array_equal(zh, z0), "every attempt ends where attempt 0 ended"


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_no_attempts_is_bp4gd_without_rounds(cn_type):
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    B, T = 32, 12
    _, _, sx, sz = depolarizing(og, P, B)
    per_qubit = np.random.RandomState(3).uniform(1.0, 6.0, size=(B, 3, og.n)).astype(F32)
    for llr in (dict(llr_const=llr_const(P)), dict(llr_ch=per_qubit)):
        x0, z0, s0, _ = GD.bp4gd_decode(og, sx, sz, T, 5, 0, 25.0, cn_type, 0.8, **llr)
        for restart in (False, True):
            xh, zh, st = AU.bp4aug_decode(c, sx, sz, T, 5, 0, 0.3, cn_type, 0.8, restart=restart, **llr)
            assert xh.tobytes() == x0.tobytes() and zh.tobytes() == z0.tobytes() and np.array_equal(st, s0) and not st[:, 1].any()
        assert (st[:, 0] == 1).any() and (st[:, 0] == 0).any()


def test_a_shard_decodes_its_samples_as_the_whole_batch_does():
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    _, _, sx, sz = depolarizing(og, P, 32)
    _, _, sx1, sz1 = depolarizing(og, P, 16, first=16)
    assert np.array_equal(sx[16:], sx1) and np.array_equal(sz[16:], sz1)
    args = (6, 3, 8, 0.1, "minsum", 0.8)
    L = llr_const(P)
    xh, zh, st = AU.bp4aug_decode(c, sx, sz, *args, restart=False, llr_const=L)
    x1, z1, s1 = AU.bp4aug_decode(c, sx1, sz1, *args, restart=False, first_sample=16, llr_const=L)
    assert np.array_equal(xh[16:], x1) and np.array_equal(zh[16:], z1) and np.array_equal(st[16:], s1)
    assert (s1[:, 1] > 0).any()
    x2, z2, s2 = AU.bp4aug_decode(c, sx1, sz1, *args, restart=False, first_sample=0, llr_const=L)
    assert not (np.array_equal(x2, x1) and np.array_equal(z2, z1) and np.array_equal(s2, s1)), "the draws depend on the sample index"
    x3, z3, s3 = AU.bp4aug_decode(c, sx1, sz1, *args, restart=False, seed=SEED + 1, first_sample=16, llr_const=L)
    assert not (np.array_equal(x3, x1) and np.array_equal(z3, z1) and np.array_equal(s3, s1)), "the draws depend on the seed"


# ---- figures -----------------------------------------------------------------------------------------------------------------------------------
def test_ibm72_splits():
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    _, _, sx, sz = depolarizing(og, P, 40)
    L = llr_const(P)
    _, _, st = AU.bp4aug_decode(c, sx, sz, 6, 12, 8, 0.2, "minsum", 0.8, restart=True, llr_const=L)
    assert split(st) == (22, 16, 2)
    _, _, st = AU.bp4aug_decode(c, sx, sz, 6, 3, 8, 0.1, "minsum", 0.8, restart=False, llr_const=L)
    assert split(st) == (22, 14, 4)


# (solved in attempt 0, solved later, unsolved), largest a, largest its, logical errors among the solved
GHP882_FIGURES = {True: ((41, 23, 0), 34, 1118, 0), False: ((41, 23, 0), 4, 141, 0)}


@functools.lru_cache(maxsize=None)
def ghp882_reference(restart):
    """The default decoder (pre 32, attempt 32, 40 attempts, density 0.1, min-sum at factor 0.8) on [[882,24]], p = 0.10, samples 0..63."""
    _, _, sx, sz = ghp882_samples()
    return AU.bp4aug_decode(code("ghp882"), sx, sz, 32, 32, 40, 0.1, "minsum", 0.8, restart=restart, llr_const=llr_const(0.10))


def ghp882_figures(xh, zh, st):
    c = code("ghp882")
    ex, ez, sx, sz = ghp882_samples()
    solved = st[:, 0] == 1
    assert np.array_equal(solves(c, xh, zh, sx, sz), solved)
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64) % 2, np.asarray(c.hz_perp, np.int64) % 2
    logical = (((xd @ hxp.T) % 2).any(1) | ((zd @ hzp.T) % 2).any(1)) & solved
    return split(st), int(st[:, 1].max()), int(st[:, 2].max()), int(logical.sum())


@pytest.mark.parametrize("restart", [True, False])
def test_ghp882_figures(restart):
    """Flooding min-sum BP4-64 leaves 7 of these 64 samples unsolved (pinned by tests/test_bp4fb_reference_cpu.py); the default decoder
    leaves none, restarting or not, and makes no logical error."""
    xh, zh, st = ghp882_reference(restart)
    figures = ghp882_figures(xh, zh, st)
    print("restart", restart, "figures", figures, "a", st[:, 1].tolist())
    assert figures == GHP882_FIGURES[restart]


# ---- the host build of the duplicated sum ------------------------------------------------------------------------------------------------------
def sum_rows():
    """(dx, dz, msg [dx + dz], dup [dx + dz]) records: seeded degrees 0 .. 16, messages of mixed magnitude so that the order of the
    adds shows, marks at density 0.4; and rows without marks, with every mark, with one slot, with the min-sum clip and subnormals."""
    rng = np.random.RandomState(0x415547)
    rows = []
    for _ in range(3000):
        dx, dz = int(rng.randint(0, 17)), int(rng.randint(0, 17))
        msg = (rng.standard_normal(dx + dz) * np.exp(rng.uniform(-4, 4, dx + dz))).astype(F32)
        rows.append((dx, dz, msg, (rng.rand(dx + dz) < 0.4).astype(np.uint8)))
    e = np.array([20.0, -20.0, 1e-40, 1.4e-45, -0.0, 0.1, 0.7, 1e7], F32)
    rows += [(0, 0, e[:0], np.zeros(0, np.uint8)), (8, 0, e, np.ones(8, np.uint8)), (0, 8, e, np.ones(8, np.uint8)),
             (4, 4, e, np.zeros(8, np.uint8)), (1, 0, e[5:6], np.ones(1, np.uint8)), (3, 5, e, np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8))]
    return rows


def run_sums(a, dup, assoc="twice"):
    """The ascending float32 sum from 0.0f: a marked message is added twice in a row ("twice"), or once as 2 m ("doubled")."""
    S = F32(0.0)
    for mj, dj in zip(a, dup):
        if assoc == "doubled" and dj:
            S = F32(S + F32(F32(2.0) * mj))
            continue
        S = F32(S + mj)
        if dj:
            S = F32(S + mj)
    return S


def build_and_run(flags, rows):
    src = os.path.join(ROOT, "tests", "vn_sums_dup_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    blob = b"".join(np.array([dx, dz], np.int32).tobytes() + np.ascontiguousarray(msg, F32).tobytes() + np.ascontiguousarray(dup, np.uint8).tobytes()
                    for dx, dz, msg, dup in rows)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vn_sums_dup_check")
        cc = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function"] + flags +
                            ["-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        run = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(rows), run.stdout[-2000:]
    return np.array([[int(h, 16) for h in ln.split()] for ln in lines], np.uint32)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_vn_sums_dup_of_the_header_equals_numpy_bitwise(flags):
    rows = sum_rows()
    got = build_and_run(flags, rows)
    want = np.zeros((len(rows), 4), F32)
    other = np.zeros((len(rows), 2), F32)
    for i, (dx, dz, msg, dup) in enumerate(rows):
        none = np.zeros_like(dup)
        want[i] = (run_sums(msg[dx:], dup[dx:]), run_sums(msg[:dx], dup[:dx]), run_sums(msg[dx:], none[dx:]), run_sums(msg[:dx], none[:dx]))
        other[i] = (run_sums(msg[dx:], dup[dx:], "doubled"), run_sums(msg[:dx], dup[:dx], "doubled"))
    bad = np.nonzero((got != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (bad[:10], got[bad[:3]], want.view(np.uint32)[bad[:3]])
    unmarked = np.array([not dup.any() for _, _, _, dup in rows])
    assert unmarked.sum() >= 3 and np.array_equal(got[unmarked, :2], got[unmarked, 2:]), "no mark: vn_sums bit for bit"
    assert (got[~unmarked, :2] != got[~unmarked, 2:]).any(1).mean() > 0.9, "a mark changes the sum"
    # the second add is a separate rounding: S + 2 m would differ on part of these rows
    assert (other.view(np.uint32) != want[:, :2].view(np.uint32)).any(1).sum() >= 100, "the rows tell (S + m) + m from S + 2 m"


# ---- build surface ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_bp4aug_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_bp4aug_decode\s*\(", text)
    assert "fgnn_bp4aug_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_bp4aug_decode")
    vn = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "fgnn_vn.h")).read()
    assert re.search(r"FG_FN\s+void\s+vn_sums_dup\s*\(", vn)


def test_public_classes_import():
    import inspect

    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.BP4AugmentedDecoder) and callable(F.BP4_Augmented_Model)
    assert callable(TannerGraph.bp4aug_decode)
    sig = inspect.signature(F.BP4AugmentedDecoder.__init__).parameters
    got = {k: sig[k].default for k in ("pre_iter", "attempt_iter", "max_attempts", "density", "restart", "cn_type", "normalization_factor", "seed")}
    assert got == dict(pre_iter=32, attempt_iter=32, max_attempts=40, density=0.1, restart=True, cn_type="minsum",
                       normalization_factor=0.8, seed=0x5EED)
