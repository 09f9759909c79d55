"""Space-time BP4: the restatement tests/stbp4_reference.py, tied to `dsbp4_reference.dsbp4_decode` at R = 1, to
`mbp4_reference.cn_update` on [h | I | I], to `dsbp4_reference.soft_rule` with one extra input and to the host build of the rules of
fgnn_cn.h with one and two extra inputs; checked for what the algorithm at fgnn_stbp4_decode (include/fgnn.h) states (decoupling under
perfect measurements, a known answer worked by hand); the window loop of the sliding model; and the Python layer in front of the library.  CPU only."""
import functools
import os

import numpy as np
import pytest
import torch

import dsbp4_reference as DS
import mbp4_reference as MB
import stbp4_reference as ST
import test_python_frontend_cpu as FE
from helpers import code, llr_const, oracle_library_forms
from test_bp4fb_reference_cpu import depolarizing
from test_dsbp4_reference_cpu import GAMMA_TABLE, bits, gamma_of_q, run_cn_rule_check, syndrome_noise
from test_python_frontend_cpu import lib_graph  # noqa: F401  (the recording library, a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]
SEED = 0x5EED
OUT = ("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats")


def window_noise(name, p, q, B, R, first=0, perfect_last=True):
    """The draws of `BP4_Phenomenological_Model`: rows first * R .. of the seeded streams viewed as [B,R,.]; (ex, ez per round, the
    measured syndromes sx, sz of the accumulated error with flips of rate q, the flips ux, uz)."""
    og = oracle_library_forms(name, stage_one=False)
    ex, ez = og.pauli_noise(SEED, p, first * R, B * R)
    cx, cz = np.bitwise_xor.accumulate(ex.reshape(B, R, -1), axis=1), np.bitwise_xor.accumulate(ez.reshape(B, R, -1), axis=1)
    sx, sz = og.syndrome(np.ascontiguousarray(cx.reshape(B * R, -1)), np.ascontiguousarray(cz.reshape(B * R, -1)))
    if q > 0:
        ux, uz = syndrome_noise(og, SEED, q, first * R, B * R)
    else:
        ux, uz = np.zeros_like(sx), np.zeros_like(sz)
    ux, uz = ux.reshape(B, R, -1).copy(), uz.reshape(B, R, -1).copy()
    if perfect_last:
        ux[:, R - 1], uz[:, R - 1] = 0, 0
    return ex.reshape(B, R, -1), ez.reshape(B, R, -1), sx.reshape(B, R, -1) ^ ux, sz.reshape(B, R, -1) ^ uz, ux, uz


# ---- 1: R = 1 is soft-syndrome BP4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name,p", [("steane", 0.15), ("rsurf5", 0.15), ("gb126", 0.05)])
def test_one_round_is_dsbp4(name, p, cn_type):
    c = code(name)
    og = oracle_library_forms(name, stage_one=False)
    B = 10
    _, _, sx, sz = depolarizing(og, p, B)
    ux, uz = syndrome_noise(og, SEED, 0.1, 0, B)
    sx, sz = sx ^ ux, sz ^ uz
    rng = np.random.RandomState(len(name))
    arrays = {k: GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=(B, m))] for k, m in (("synd_llr_x", og.m_x), ("synd_llr_z", og.m_z))}
    assert all(np.isinf(v).any() and (v < 0).any() and (v == 0).any() for v in arrays.values())
    L = llr_const(p)
    stopped = set()
    for gam in (dict(gamma_x=2.0, gamma_z=3.0), dict(gamma_x=INF, gamma_z=-0.7), arrays):
        for alphas, restart in (((1.0,), True), ((1.0, 0.7, 0.5), True), ((1.0, 0.7, 0.5), False)):
            factors, owns = MB.mbp4_tables(alphas, 0.8)
            want = DS.dsbp4_decode(c, sx, sz, factors, owns, 4, 3, cn_type, restart=restart, llr_const=L, **gam)
            win = {k: (v[:, None] if isinstance(v, np.ndarray) else v) for k, v in gam.items()}
            if "gamma_x" in gam:  # R = 1: the last round is the only one
                win = dict(gamma_x=-5.0, gamma_z=-5.0, gamma_last_x=gam["gamma_x"], gamma_last_z=gam["gamma_z"])
            got = ST.stbp4_decode(c, sx[:, None], sz[:, None], factors, owns, 4, 3, cn_type, restart=restart, llr_const=L, **win)
            for label, w, g in zip(OUT, want, got):
                assert (w.reshape(g.shape) == g).all() and w.dtype == g.dtype, (label, gam.keys(), alphas, restart)
            stopped |= set(want[4][:, 0].tolist())
    assert stopped == {0, 1}, "the batches must hold solved and unsolved samples"


# ---- 2: the rule against cn_update on [h | I | I] and against the soft rule ----------------------------------------------------------------
@pytest.mark.parametrize("cn_type", CN_TYPES)
@pytest.mark.parametrize("name", ["ibm72", "toric4", "gb126"])
def test_the_rule_is_the_rule_on_the_widened_matrix(name, cn_type):
    c = code(name)
    rng = np.random.RandomState(0x57 + len(name))
    B = 12
    for h in (np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2):
        eye = np.eye(h.shape[0], dtype=np.int64)
        side, wide = MB.Side(h), MB.Side(np.hstack([h, eye, eye]))
        assert wide.E == side.E + 2 * side.m and np.array_equal(wide.v_of[:side.E], side.v_of)
        deg = wide.cn_mask.sum(1)
        assert (wide.cn_tab[np.arange(side.m), deg - 2] == side.E + np.arange(side.m)).all(), "a is the check's last input but one"
        assert (wide.cn_tab[np.arange(side.m), deg - 1] == side.E + side.m + np.arange(side.m)).all(), "b is its last"
        nu = (rng.standard_normal((B, side.E)) * 6.0).astype(F32)
        edge = rng.rand(B, side.E) < 0.1  # no subnormal here: boxplus divides by tanh(nu / 2)
        nu[edge] = rng.choice(np.array([0.0, 20.0, -20.0, 25.0, -1e-3], F32), size=int(edge.sum()))
        synd = rng.randint(0, 2, size=(B, side.m)).astype(np.uint8)
        a = GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=(B, side.m))]
        b = GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=(B, side.m))]
        assert np.isinf(a).any() and (b == 0).any() and (a < 0).any() and (a == b).any()
        for factor in (F32(1.0), F32(0.8)):
            mu, (wa, wb) = ST.st_cn_update(side, nu, synd, [a, b], cn_type, factor)
            ref = MB.cn_update(wide, np.concatenate([nu, a, b], axis=1), synd, cn_type, factor)
            assert not np.isnan(ref).any()
            assert np.array_equal(bits(mu), bits(ref[:, :side.E])), "real edges"
            assert np.array_equal(bits(wa), bits(ref[:, side.E:side.E + side.m])), "the output for a is w_up"
            assert np.array_equal(bits(wb), bits(ref[:, side.E + side.m:])), "the output for b is w_dn"
            mu1, (w1,) = ST.st_cn_update(side, nu, synd, [b], cn_type, factor)
            mus, ws = DS.soft_cn_update(side, nu, synd, b, cn_type, factor)
            assert np.array_equal(bits(mu1), bits(mus)) and np.array_equal(bits(w1), bits(ws)), "one extra input: dsbp4's soft rule"


# ---- 3: the header ----------------------------------------------------------------------------------------------------------------------------
DMAX, HEAD = 12, 6


def rule_rows():
    """(deg, syndrome bit, number of extras, factor, extra 0, extra 1, 12 inputs) rows: degrees 2 .. 12, one and two extras from the
    gamma table and from the range the time variables form, and edge rows: zeros, the +-20 clip, subnormals, +inf, duplicate minima
    that include an extra input or both."""
    rng = np.random.RandomState(0x57F7)
    N = 3000
    rows = np.zeros((N, HEAD + DMAX), F32)
    rows[:, 0] = rng.randint(2, DMAX + 1, size=N)
    rows[:N // 3, 0] = 6  # the compile-time degree of the register form
    rows[:, 1] = rng.randint(0, 2, size=N)
    rows[:, 2] = rng.randint(1, 3, size=N)
    rows[:, 3] = rng.choice(np.array([1.0, 0.8, 0.8 / 0.7, 1.6], F32), size=N)
    rows[:, 4:6] = GAMMA_TABLE[rng.randint(len(GAMMA_TABLE), size=(N, 2))]
    formed = rng.rand(N, 2) < 0.4
    rows[:, 4:6][formed] = (rng.standard_normal(int(formed.sum())) * 5.0).astype(F32)
    rows[:, HEAD:] = (rng.standard_normal((N, DMAX)) * 5.0).astype(F32)
    clip = rng.rand(N, DMAX) < 0.08
    rows[:, HEAD:][clip] = rng.choice(np.array([20.0, -20.0, 25.0, -31.0, 0.0, -0.0, 1e-40, -1.4e-45, 1e-3], F32), size=int(clip.sum()))

    def row(deg, s, nx, f, x0, x1, vals):
        r = np.zeros(HEAD + DMAX, F32)
        r[:HEAD] = (deg, s, nx, f, x0, x1)
        r[HEAD:HEAD + len(vals)] = vals
        return r

    edge = [row(6, 0, 2, 1.0, 0.0, 0.0, [0.0] * 6), row(6, 1, 2, 0.8, INF, INF, [20.0, -20.0, 25.0, -25.0, 20.0, 19.999998]),
            row(6, 0, 2, 0.8, 20.0, 25.0, [20.0] * 6), row(6, 1, 2, 1.0, 1.5, 1.5, [2.0, 3.0, -1.5, 4.0, 5.0, 6.0]),
            row(6, 0, 2, 0.8, 1.5, -1.5, [2.0, 3.0, 4.0, 4.0, 5.0, 6.0]), row(6, 0, 2, 0.8, 1.5, 9.0, [1.5, 3.0, 4.0, 4.0, 5.0, 6.0]),
            row(6, 0, 2, 1.0, 1e-40, -1.4e-45, [1e-40, -1.4e-45, 1e-39, 0.0, 2.0, 3.0]), row(2, 1, 2, 0.8, INF, 3.0, [3.0, -4.0]),
            row(2, 0, 1, 0.8, 0.0, 0.0, [3.0, -4.0]), row(12, 1, 2, 0.8, 2.0, 2.0, [2.0] * 12), row(12, 0, 1, 1.0, INF, 0.0, [1e-3] * 12),
            row(3, 0, 2, 1.0, 1e-3, INF, [0.0, 0.0, 7.0]), row(7, 1, 2, 0.8, -25.0, 25.0, [9.0, -8.0, 7.0, -6.0, 5.0, -4.0, 3.0])]
    return np.concatenate([np.stack(edge), rows])


@functools.lru_cache(maxsize=None)
def rule_rows_reference():
    """{cn_type: [N, 14] bits} of the restatement on rule_rows(): the 12 slots, then the outputs for the extras (0 for a missing one)."""
    rows = rule_rows()
    deg = rows[:, 0].astype(int)
    mask = np.arange(DMAX)[None, :] < deg[:, None]
    two = rows[:, 2] == 2
    want = {}
    for cn in CN_TYPES:
        res = np.zeros((len(rows), DMAX + 2), np.uint32)
        for sel, nx in ((~two, 1), (two, 2)):
            out, ws = ST.st_rule(rows[sel, HEAD:].copy(), mask[sel], rows[sel, 1] != 0, [rows[sel, 4 + e].copy() for e in range(nx)], cn,
                                 rows[sel, 3].copy())
            assert not np.isnan(out).any() and not any(np.isnan(w).any() for w in ws)
            res[sel, :DMAX] = bits(out)
            for e, w in enumerate(ws):
                res[sel, DMAX + e] = bits(w)
        want[cn] = res
    return want


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_rules_of_the_header_equal_the_restatement_bitwise(flags):
    rows = rule_rows()
    got = run_cn_rule_check(flags, rows)
    assert got.shape == (len(rows), 5 * 14)
    want = rule_rows_reference()
    for g, cn in enumerate(CN_TYPES):  # the loop form
        bad = np.nonzero(~(got[:, 14 * g:14 * g + 14] == want[cn]).all(1))[0]
        assert len(bad) == 0, (cn, bad[:10], rows[bad[:3]])
    bad = np.nonzero(~(got[:, 42:56] == want["minsum"]).all(1))[0]
    assert len(bad) == 0, ("register form, guarded", bad[:10])
    six = rows[:, 0] == 6
    assert six.sum() > 500 and (got[six, 56:70] == want["minsum"][six]).all(), "register form at its compile-time degree"
    assert not got[~six, 56:70].any() and set(rows[six, 2].astype(int)) == {1, 2}
    # the table reaches what it says: every degree with one and with two extras, an extra as the only minimum and among duplicates
    for nx in (1, 2):
        assert set(rows[rows[:, 2] == nx, 0].astype(int)) >= set(range(2, DMAX + 1))
    a = np.minimum(np.abs(rows[:, HEAD:]), 20)
    a[np.arange(DMAX)[None, :] >= rows[:, 0:1]] = np.inf
    two = rows[:, 2] == 2
    ax = np.minimum(np.abs(rows[:, 4:6]), 20)
    assert ((a.min(1) == ax[:, 0]) & two).sum() >= 3 and ((ax[:, 0] == ax[:, 1]) & two).sum() >= 5
    assert ((a.min(1) > ax.min(1)) & two).sum() >= 100 and ((a.min(1) < ax.min(1)) & two).sum() >= 100


# ---- 4: perfect measurements decouple the rounds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("ibm72", 0.12), ("rsurf5", 0.2)])
def test_perfect_measurements_decouple_the_rounds(name, p):
    """Min-sum with every gamma = +inf: an extra input clips to 20, which no clipped edge exceeds, so a and b change no edge output and
    every round runs dsbp4's iterations on its own difference syndrome.  The window stops only when every round is solved at the
    same test; on windows in which dsbp4 solves none of the rounds within K both make their last test at k = K."""
    c = code(name)
    B, R, K = 40, 3, 3
    _, _, sx, sz, _, _ = window_noise(name, p, 0.0, B, R)
    dx, dz = ST.differences(sx, None), ST.differences(sz, None)
    f, o = MB.mbp4_tables((1.0,), 0.8)
    L = llr_const(p)
    per_round = [DS.dsbp4_decode(c, dx[:, t], dz[:, t], f, o, K, K, "minsum", llr_const=L) for t in range(R)]
    none_solved = np.all([r[4][:, 0] == 0 for r in per_round], axis=0)
    print(name, "windows in which no round is solved within", K, ":", int(none_solved.sum()))
    assert none_solved.sum() >= 10
    got = ST.stbp4_decode(c, sx, sz, f, o, K, K, "minsum", llr_const=L)
    assert not got[2].any() and not got[3].any(), "a perfect measurement is never estimated wrong"
    for t in range(R):
        for j, label in enumerate(OUT[:4]):
            assert np.array_equal(got[j][none_solved, t], per_round[t][j][none_solved]), (label, t)
    assert np.array_equal(got[4][none_solved], np.tile(np.array([0, 0, K, K], np.int32), (int(none_solved.sum()), 1)))


# ---- 5: a known answer ---------------------------------------------------------------------------------------------------------------------------
KNOWN_P0, KNOWN_Q0 = 0.01, 0.05


@pytest.mark.parametrize("name", ["steane", "toric4"])
def test_one_measurement_flip_is_found_at_the_first_test(name):
    """No data error and one flipped bit u_{c,1} = 1 at the interior round of an R = 3 window: s_0 = 0, s_1 = e_c, s_2 = 0, so d_1 and d_2
    both carry check c.  First min-sum iteration by hand, with L = log(3 * 0.99 / 0.01) = 5.69, g = log(0.95 / 0.05) = 2.94: every
    qubit sends lse-reduced priors of about L - log 2 = 5.0 > g, so at the checks (c,1) and (c,2) the smallest input is a time
    message (a = b = g; b of the last round is +inf).  Check (c,1), syndrome 1: its edges and w_up get sign -, magnitude g, except
    that the outputs towards a and b see the other one, g as well: w_dn(c,1) = -0.8 g.  Check (c,2), syndrome 1, inputs (edges, a = g,
    b = inf): w_up(c,2) = -0.8 * min(edges) = -0.8 * 5.0.  Gamma(c,1) = (g - 0.8 g) - 4.0 < 0: u_hat(c,1) = 1.  Gamma(c,0) = (g + 0.8 g)
    - 0.8 g > 0.  A qubit of c hears -0.8 g from rounds 1 and 2 against a prior of 5.69: no data error.  Every other check is quiet."""
    c = code(name)
    hx, hz = np.asarray(c.hx) % 2, np.asarray(c.hz) % 2
    mx, mz, R = hx.shape[0], hz.shape[0], 3
    B = mx + mz
    sx, sz = np.zeros((B, R, mx), np.uint8), np.zeros((B, R, mz), np.uint8)
    sx[np.arange(mx), 1, np.arange(mx)] = 1
    sz[mx + np.arange(mz), 1, np.arange(mz)] = 1
    f, o = MB.mbp4_tables((1.0,), 0.8)
    g = gamma_of_q(KNOWN_Q0)
    xh, zh, uxh, uzh, st = ST.stbp4_decode(c, sx, sz, f, o, 8, 8, "minsum", llr_const=llr_const(KNOWN_P0), gamma_x=g, gamma_z=g)
    assert np.array_equal(st, np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1))), "solved at the first test"
    assert not xh.any() and not zh.any()
    assert np.array_equal(uxh, sx) and np.array_equal(uzh, sz), "u_hat is the single flip"


# ---- 6: the sliding windows ---------------------------------------------------------------------------------------------------------------------
PLANS = [(5, 3, 1), (5, 3, 2), (4, 4, 4), (7, 3, 3)]


@pytest.mark.parametrize("rounds,window,commit", PLANS)
def test_committed_rounds_tile_the_experiment(rounds, window, commit):
    import feedback_gnn_amd as F
    plan = ST.window_plan(rounds, window, commit)
    covered = [t for a, W, Fc, last in plan for t in range(a, a + Fc)]
    assert covered == list(range(rounds)), "every round is committed exactly once, in order"
    assert all(W <= window and a + W <= rounds for a, W, _, _ in plan) and [last for *_, last in plan] == [False] * (len(plan) - 1) + [True]
    assert plan[-1][0] + plan[-1][1] == rounds and all(a + W < rounds for a, W, _, last in plan if not last)
    if rounds <= window:
        assert plan == [(0, rounds, rounds, True)]
    stub = StStub()
    dec = F.SpaceTimeBP4Decoder(FE.CODE, window, graph=stub)
    assert F.BP4_Phenomenological_Model(FE.CODE, dec, 0.1, rounds, window, commit, seed=7).windows() == plan
    assert F.BP4_Phenomenological_Model(FE.CODE, F.SpaceTimeBP4Decoder(FE.CODE, rounds, graph=stub), 0.1, rounds).windows() == [(0, rounds, rounds, True)]


@pytest.mark.parametrize("rounds,window,commit", PLANS)
def test_the_sliding_loop_over_the_restatement(rounds, window, commit):
    """`prev` is what the previous window's last committed round leaves; a window that is not the last decodes with gamma_last = gamma."""
    name, p, q, B = "steane", 0.04, 0.05, 12
    c = code(name)
    ex, ez, sx, sz, ux, uz = window_noise(name, p, q, B, rounds)
    f, o = MB.mbp4_tables((1.0,), 0.8)
    g, L = gamma_of_q(q), llr_const(p)
    seen = []

    def decode(wx, wz, px, pz, gl):
        seen.append((wx.copy(), None if px is None else px.copy()))
        return ST.stbp4_decode(c, wx, wz, f, o, 6, 6, "minsum", prev_x=px, prev_z=pz, llr_const=L, gamma_x=g, gamma_z=g, gamma_last_x=gl,
                               gamma_last_z=gl)

    xh, zh, uxh, uzh, unsolved, calls = ST.sliding_decode(decode, sx, sz, rounds, window, commit, g)
    plan = ST.window_plan(rounds, window, commit)
    assert [(a, W) for a, W, _, _ in plan] == [(a, W) for a, W, _, _ in calls]
    assert [gl for _, _, gl, _ in calls] == [g] * (len(plan) - 1) + [INF] and [pv for *_, pv in calls] == [False] + [True] * (len(plan) - 1)
    for i, (a, W, Fc, last) in enumerate(plan):
        assert np.array_equal(seen[i][0], sx[:, a:a + W])
        if i > 0:
            assert np.array_equal(seen[i][1], sx[:, a - 1] ^ uxh[:, a - 1]), "prev = s ^ u_hat of the last committed round"
    if len(plan) == 1:
        one = decode(sx, sz, None, None, INF)
        assert all(np.array_equal(a, b) for a, b in zip((xh, zh, uxh, uzh), one[:4])) and unsolved == int((one[4][:, 0] == 0).sum())
    assert 0 <= unsolved <= B * len(plan) and xh.shape == ex.shape and uxh.shape == ux.shape


# ---- 7: the wrapper, the decoder and the model ---------------------------------------------------------------------------------------------
n, m_x, m_z, B = FE.n, FE.m_x, FE.m_z, FE.B
U8, I32, T32 = torch.uint8, torch.int32, torch.float32
R = 3


@pytest.mark.parametrize("given", ["synd", "x", "llr+rounds", "soft_z", "B+rounds"])
def test_stbp4_decode_wrapper(lib_graph, given):  # noqa: F811
    g, rec = lib_graph
    z, p = FE.z, FE.p
    sx = z((B, R, m_x)) if given in ("synd", "x") else None
    sz = z((B, R, m_z)) if given == "synd" else None
    llr_ch = z((B, 3, n), T32) if given in ("synd", "llr+rounds") else None
    slz = z((B, R, m_z), T32) if given in ("synd", "soft_z") else None
    slx = z((B, R, m_x), T32) if given == "synd" else None
    px, pz = (z((B, m_x)), z((B, m_z))) if given == "synd" else (None, None)
    kw = dict(rounds=R) if given.endswith("rounds") else {}
    if given == "B+rounds":
        kw["B"] = B
    factors, owns = FE._tables()
    out, name, a, allocs = FE.run(g, rec, g.stbp4_decode, sx, sz, factors, owns, 7, 8, "boxplus", restart=False, prev_x=px, prev_z=pz,
                                  llr_ch=llr_ch, llr_const=1.5, synd_llr_x=slx, synd_llr_z=slz, gamma_x=2.5, gamma_z=3.5, gamma_last_x=4.5,
                                  gamma_last_z=5.5, **kw)
    xh, zh, uxh, uzh, stats = out
    assert name == "fgnn_stbp4_decode"
    assert a == [None, FE.CN_TYPES["boxplus"], 3, factors.ctypes.data, owns.ctypes.data, 7, 8, 0, R, p(llr_ch), 1.5, p(sx), p(sz), p(px), p(pz),
                 p(slx), 2.5, 4.5, p(slz), 3.5, 5.5, B, p(xh), p(zh), p(uxh), p(uzh), p(stats), None]
    assert allocs == [((B, R, n), U8), ((B, R, n), U8), ((B, R, m_x), U8), ((B, R, m_z), U8), ((B, 4), I32)]
    assert all(FE.shaped(t, s, d) for t, (s, d) in zip(out, allocs))


def test_stbp4_decode_defaults_and_refusals(lib_graph):  # noqa: F811
    g, rec = lib_graph
    z, refused = FE.z, FE.refused
    sx, sz = z((B, R, m_x)), z((B, R, m_z))
    factors, owns = FE._tables()
    _, _, a, _ = FE.run(g, rec, g.stbp4_decode, sx, sz, factors, owns, 7, 8)
    assert a[1] == FE.CN_TYPES["minsum"] and a[7] == 1 and a[8] == R and a[13:21] == [None, None, None, INF, INF, None, INF, INF]
    rec.calls.clear()
    one = ([1.0], [1.0], 7, 8)
    refused(ValueError, "Unknown node type.", g.stbp4_decode, sx, sz, *one, cn_type="boxminus")
    refused(ValueError, "factors and owns must have the same length", g.stbp4_decode, None, None, [1.0, 2.0], [1.0], 7, 8)
    refused(ValueError, "rounds is needed when neither syndromes nor syndrome LLRs are given", g.stbp4_decode, None, None, *one, B=4)
    refused(ValueError, "rounds must be >= 1", g.stbp4_decode, None, None, *one, rounds=0, B=4)
    refused(ValueError, "B is needed when neither syndromes nor llr_ch nor syndrome LLRs are given", g.stbp4_decode, None, None, *one, rounds=2)
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.stbp4_decode, z((B, R, m_x), T32), sz, *one)
    refused(ValueError, "synd_x must have shape (4, 3, 3), got (4, 3)", g.stbp4_decode, z((B, m_x)), sz, *one)
    refused(ValueError, "synd_z must have shape (4, 3, 2), got (4, 3, 3)", g.stbp4_decode, sx, sx, *one)
    refused(ValueError, "synd_x must have shape (4, 2, 3), got (4, 3, 3)", g.stbp4_decode, sx, sz, *one, rounds=2)
    refused(ValueError, "prev_x must have shape (4, 3), got (4, 2)", g.stbp4_decode, sx, sz, *one, prev_x=z((B, m_z)))
    refused(ValueError, "prev_z must be torch.uint8, got torch.float32", g.stbp4_decode, sx, sz, *one, prev_z=z((B, m_z), T32))
    refused(ValueError, "llr_ch must have shape (4, 3, 6), got (4, 6)", g.stbp4_decode, sx, sz, *one, llr_ch=z((B, n), T32))
    refused(ValueError, "synd_llr_x must be torch.float32, got torch.uint8", g.stbp4_decode, sx, sz, *one, synd_llr_x=sx)
    refused(ValueError, "synd_llr_z must have shape (4, 3, 2), got (4, 2)", g.stbp4_decode, sx, sz, *one, synd_llr_z=z((B, m_z), T32))
    refused(ValueError, "synd_x must have shape (5, 3, 3), got (4, 3, 3)", g.stbp4_decode, sx, sz, *one, synd_llr_z=z((5, R, m_z), T32))
    assert rec.calls == []
    # a non-contiguous input arrives contiguous
    wide = z((B, R, 2 * m_x))[:, :, ::2]
    _, _, a, _ = FE.run(g, rec, g.stbp4_decode, wide, sz, *one)
    assert a[11] is not None and a[11] != FE.p(wide)


N, MX, MZ = FE.N, FE.MX, FE.MZ


class StStub(FE.StubGraph):
    """`StubGraph` with the calls of the phenomenological model shaped by their arguments: noise and syndromes of the batch asked for,
    `stbp4_decode` zero tensors of the window given."""

    def _rec(self, name, args, kw):
        self.calls.append((name, args, kw))

    def pauli_noise(self, seed, p, first, B):
        self._rec("pauli_noise", (seed, p, first, B), {})
        return FE.z((B, N)), FE.z((B, N))

    def syndrome(self, ex, ez):
        self._rec("syndrome", (ex, ez), {})
        return FE.z((ex.shape[0], MX)), FE.z((ex.shape[0], MZ))

    def syndrome_noise(self, seed, q, first, B):
        self._rec("syndrome_noise", (seed, q, first, B), {})
        return torch.ones((B, MX), dtype=U8), torch.ones((B, MZ), dtype=U8)

    def stbp4_decode(self, synd_x, synd_z, *args, **kw):
        self._rec("stbp4_decode", (synd_x, synd_z) + args, kw)
        B, R = synd_x.shape[:2]
        return FE.z((B, R, N)), FE.z((B, R, N)), FE.z((B, R, MX)), FE.z((B, R, MZ)), FE.z((B, 4), I32)

    def residual(self, *args, **kw):
        self._rec("residual", args, kw)
        B = args[0].shape[0]
        return FE.z((B, MZ + MX)), FE.z((B, 12)), FE.z((B,))


def test_decoder_forwards_to_the_graph_and_keeps_the_sibling_dtypes():
    import feedback_gnn_amd as F
    g = StStub()
    d = F.SpaceTimeBP4Decoder(FE.CODE, 4, alphas=(1.0, 0.5), num_iter=5, cn_type="boxplus", factor=0.75, restart=False, graph=g)
    assert d.graph is g and d.code is FE.CODE and d.num_vns == N and d.last_stats is None and d.rounds == 4 and d.alphas == (1.0, 0.5)
    assert type(d).call is type(d).__call__ and F.SpaceTimeBP4Decoder(FE.CODE, 2, graph=g).alphas == (1.0,)
    sx, sz, px = FE.z((2, 3, MX)), FE.z((2, 3, MZ)), FE.z((2, MX))
    out = d.decode(sx, sz, prev_x=px, gamma=2.5, gamma_last=3.5, llr_const=1.5)
    FE.assert_call(g.calls[0], "stbp4_decode", (sx, sz, d.factors, d.owns, 5, 5, "boxplus"),
                   dict(restart=False, rounds=3, prev_x=px, prev_z=None, llr_ch=None, llr_const=1.5, synd_llr_x=None, synd_llr_z=None, gamma_x=2.5,
                        gamma_z=2.5, gamma_last_x=3.5, gamma_last_z=3.5))
    assert len(out) == 5 and d.last_stats is out[4] and d.last_u_x_hat is out[2] and d.last_u_z_hat is out[3]
    assert FE.shaped(d.last_correction_x, (2, N), U8) and FE.shaped(d.last_correction_z, (2, N), U8)
    FE.refused(ValueError, "a window holds at most 4 rounds, got 5", d.decode, FE.z((2, 5, MX)), FE.z((2, 5, MZ)))
    # the call of the reference's decoders, the rounds stacked in front: int64 and float64 [bs, n]
    g.calls.clear()
    llr_ch = torch.zeros((2, 3, N), dtype=T32)
    rng = np.random.default_rng(5)
    cx, cz = rng.integers(-4, 5, size=(3, MX, 2)), torch.from_numpy(rng.integers(-4, 5, size=(3, MZ, 2)).astype(np.float64))
    x_hat, z_hat = d((llr_ch, cx, cz))
    assert FE.shaped(x_hat, (2, N), torch.int64) and FE.shaped(z_hat, (2, N), torch.float64)
    call = g.calls[0]
    assert torch.equal(call[1][0], torch.from_numpy((cx & 1).astype(np.uint8)).permute(2, 0, 1)) and call[1][0].is_contiguous()
    assert torch.equal(call[1][1], (cz.to(torch.int64) & 1).to(U8).permute(2, 0, 1)) and call[2]["rounds"] == 3
    assert call[2]["gamma_x"] == INF and call[2]["gamma_last_z"] == INF and call[2]["llr_ch"] is llr_ch
    FE.refused(TypeError, "Invalid input dtype.", d, (llr_ch.double(), cx, cz))
    FE.refused(ValueError, f"syndrome must have shape [rounds, {MX}, batch_size], got ({MX}, 2)", d, (llr_ch, cx[0], cz))
    FE.refused(ValueError, "batch sizes of llr_ch and the syndromes differ.", d, (llr_ch, cx[:, :, :1], cz))
    FE.refused(ValueError, "the two syndromes must hold the same number of rounds", d, (llr_ch, cx[:2], cz))


def test_constructor_refusals():
    import feedback_gnn_amd as F
    g = StStub()
    refused = FE.refused
    for rounds in (0, -1, 2.0):
        refused(ValueError, "rounds must be a positive integer", F.SpaceTimeBP4Decoder, FE.CODE, rounds, graph=g)
    refused(ValueError, "alphas must hold 1 .. 64 values", F.SpaceTimeBP4Decoder, FE.CODE, 2, alphas=(), graph=g)
    refused(ValueError, "Unknown node type.", F.SpaceTimeBP4Decoder, FE.CODE, 2, cn_type="x", graph=g)
    refused(ValueError, "factor / alpha must be finite in float32", F.SpaceTimeBP4Decoder, FE.CODE, 2, alphas=(1e-30,), factor=1e30, graph=g)
    d = F.SpaceTimeBP4Decoder(FE.CODE, 3, graph=g)
    M = F.BP4_Phenomenological_Model
    refused(ValueError, "rounds must be a positive integer", M, FE.CODE, d, 0.1, 0)
    refused(ValueError, "commit must be in 1 .. window", M, FE.CODE, d, 0.1, 5, 3, 4)
    refused(ValueError, "commit must be in 1 .. window", M, FE.CODE, d, 0.1, 5, 3, 0)
    refused(ValueError, "window must be a positive integer", M, FE.CODE, d, 0.1, 5, 0)
    refused(ValueError, "commit needs a window", M, FE.CODE, d, 0.1, 3, None, 1)
    for q in (1.0, -0.1):
        refused(ValueError, "q must be in [0, 1)", M, FE.CODE, d, q, 3)
    refused(ValueError, "q0 must be in [0, 1)", M, FE.CODE, d, 0.1, 3, q0=1.5)
    refused(ValueError, "the decoder's windows hold at most 3 rounds", M, FE.CODE, d, 0.1, 5)
    refused(ValueError, "the decoder's windows hold at most 3 rounds", M, FE.CODE, d, 0.1, 7, 4, 2)
    m = M(FE.CODE, d, 0.125, 5, 3, seed=7)
    assert (m.rounds, m.window, m.commit, m.q, m.q0, m.p0) == (5, 3, 1, 0.125, None, None) and m.last_num_unsolved == 0 and m.last_stats is None
    assert m.gamma == gamma_of_q(0.125) and M(FE.CODE, d, 0.0, 3).gamma == INF


def test_model_draws_the_rows_one_process_draws_and_walks_the_windows():
    import feedback_gnn_amd as F
    rounds, window, commit = 6, 3, 2

    def build(**kw):
        g = StStub()
        return F.BP4_Phenomenological_Model(FE.CODE, F.SpaceTimeBP4Decoder(FE.CODE, window, num_iter=5, graph=g), 0.125, rounds, window, commit,
                                            seed=7, **kw), g

    one, g1 = build()
    one(16, 0.05)
    assert g1.named("pauli_noise")[0][1] == (7, 0.05, 0, 16 * rounds) and g1.named("syndrome_noise")[0][1] == (7, 0.125, 0, 16 * rounds)
    assert one._next == 16
    rows = []
    for rank in (0, 1):
        m, g = build(rank=rank, world_size=2)
        assert m.next_sample_range(8) == (8 * rank, 8 * rank + 8)
        s_hat, ls_hat = m(8, p=0.05)
        noise, flips = g.named("pauli_noise")[0][1], g.named("syndrome_noise")[0][1]
        assert noise == (7, 0.05, 8 * rank * rounds, 8 * rounds) and flips == (7, 0.125, 8 * rank * rounds, 8 * rounds) and m._next == 16
        rows += list(range(noise[2], noise[2] + noise[3]))
        assert FE.shaped(s_hat, (8, MZ + MX), U8) and FE.shaped(ls_hat, (8, 12), U8)
        # the windows: (0,3) and (2,3) with gamma_last = gamma and two rounds committed, then (4,2) with the perfect read-out
        calls = g.named("stbp4_decode")
        gam = gamma_of_q(0.125)
        assert [tuple(c[1][0].shape) for c in calls] == [(8, 3, MX), (8, 3, MX), (8, 2, MX)]
        assert [c[2]["gamma_last_x"] for c in calls] == [gam, gam, INF] and all(c[2]["gamma_x"] == gam for c in calls)
        assert [c[2]["prev_x"] is None for c in calls] == [True, False, False]
        assert all(c[2]["llr_const"] == FE.depolarizing_expr(0.05) for c in calls)
        # the stub's flips are all ones except in the perfect last round, its exact syndromes zero, its u_hat zero: prev = s ^ 0
        assert bool(calls[0][1][0].all()) and bool(calls[1][2]["prev_x"].all()) and bool(calls[2][1][0][:, 0].all()) and not bool(calls[2][1][0][:, 1].any())
        assert bool(m.last_u_x[:, :rounds - 1].all()) and not bool(m.last_u_x[:, rounds - 1].any())
        assert FE.shaped(m.last_x_hat, (8, rounds, N), U8) and FE.shaped(m.last_u_z_hat, (8, rounds, MZ), U8)
        assert len(m.last_window_stats) == 3 and m.last_stats is m.last_window_stats[-1] and m.last_num_unsolved == 3 * 8
        assert len(g.named("residual")) == 1 and g.named("residual")[0][2] == dict(want_arrays=True)
    assert rows == list(range(16 * rounds)), "two shards of 8 samples draw the rows one process of 16 draws"


def test_the_build_surface():
    import ctypes
    import re
    import feedback_gnn_amd as F
    from feedback_gnn_amd import _lib
    from feedback_gnn_amd.graph import TannerGraph
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgnn.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fgnn_stbp4_decode\s*\(", text) and "fgnn_stbp4_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_stbp4_decode")
    assert callable(F.SpaceTimeBP4Decoder) and callable(F.BP4_Phenomenological_Model) and callable(TannerGraph.stbp4_decode)
    make = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert "fgnn_stbp4.hip" in make and "fgnn_cn.h" in make.split("HDRS :=")[1].split("\n")[0].split(), "the header the kernel includes"
    assert '#include "fgnn_cn.h"' in open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "fgnn_stbp4.hip")).read()
    # the byte formula: a five-round window of [[882,24]] fits the LDS budget, a six-round one does not
    budget = 160 * 1024 - 256
    E, nq, m = 2 * 2646, 882, 882
    assert ST.stbp4_lds_bytes(E, nq, m, 5, 1) <= budget < ST.stbp4_lds_bytes(E, nq, m, 6, 1)
    assert ST.stbp4_lds_bytes(E, nq, m, 1, 1) == DS.dsbp4_lds_bytes(E, nq, m, 1) + 4 * 884, "R = 1: dsbp4's LDS and the b slots"
