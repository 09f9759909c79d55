"""The restatement of window post-processing (tests/stpost_reference.py) on the CPU: its soft decoder against
`stbp4_reference.stbp4_decode`, the window matrix against the checks it stands for, its OSD-0 against the existing OSD restatement, the
whole pipeline against the joint test of the window, the fixture conditions of tests/test_gpu_stpost.py, and the plumbing of the three
new `TannerGraph` wrappers against a recording library.  tests/test_gpu_stpost.py holds the kernels to this restatement bit for bit."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mbp4_reference as MB
import stbp4_reference as ST
import stpost_reference as SP
from feedback_gnn_amd import _lib, gf2, graph as G
from feedback_gnn_amd import space_time
from guarded import guarded
from helpers import llr_const
from stpost_cases import CASES, LOW_CAP, case_code, case_inputs, case_settings, case_variant
from test_osd_search_cpu import OSD_0, osd_search

INF = float("inf")
U8, I32, F32 = torch.uint8, torch.int32, torch.float32


# ---- the soft decoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_hard_outputs_equal_the_plain_restatement_and_fixture_conditions_hold(case):
    """x_hat, z_hat, u_hat and stats of the soft restatement equal stbp4_reference.stbp4_decode exactly; the committed seed leaves at
    least a quarter of the windows unsolved and solves at least two; soft rows are zero exactly on the solved windows."""
    code, (sx, sz), kw = case_code(case), case_inputs(case), case_settings(case)
    soft = SP.stbp4_decode_soft(code, sx, sz, **kw)
    plain = ST.stbp4_decode(code, sx, sz, **kw)
    for a, b in zip(soft[:5], plain):
        assert np.array_equal(a, b)
    stats, marg, gx, gz = soft[4:]
    B = len(stats)
    unsolved = stats[:, 0] == 0
    assert 4 * int(unsolved.sum()) >= B and int((~unsolved).sum()) >= 2, (int(unsolved.sum()), B)
    assert not marg[~unsolved].any() and not gx[~unsolved].any() and not gz[~unsolved].any()
    assert (np.abs(marg[unsolved]).reshape(int(unsolved.sum()), -1).max(1) > 0).all(), "an unsolved window has marginals"
    # the decisions and u_hat of an unsolved window are those of its soft values
    dn = MB.decisions(marg[unsolved][:, :, 0], marg[unsolved][:, :, 1], marg[unsolved][:, :, 2])
    assert np.array_equal(dn & 1, soft[0][unsolved]) and np.array_equal(dn >> 1, soft[1][unsolved])
    assert np.array_equal((gx[unsolved] < 0).astype(np.uint8), soft[2][unsolved])
    assert np.array_equal((gz[unsolved] < 0).astype(np.uint8), soft[3][unsolved])


@pytest.mark.parametrize("case", ["tiny_r2", "tiny_r3", "ghp_r2"])
@pytest.mark.parametrize("cn_type,restart", [("minsum", True), ("boxplus-phi", False), ("boxplus", True)])
def test_soft_decoder_with_prev_arrays_and_sweep_equals_the_plain_restatement(case, cn_type, restart):
    code, (sx, sz) = case_code(case), case_inputs(case)
    kw = case_variant(case, cn_type=cn_type, restart=restart)
    soft, plain = SP.stbp4_decode_soft(code, sx, sz, **kw), ST.stbp4_decode(code, sx, sz, **kw)
    for a, b in zip(soft[:5], plain):
        assert np.array_equal(a, b)
    assert 0 < soft[4][:, 0].sum() < len(sx), "solved and unsolved windows both occur"


# ---- the window matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 5])
def test_window_matrix_is_the_window_checks_and_has_full_row_rank(R):
    code = case_code("tiny_r1")
    rng = np.random.default_rng(R)
    for h in (np.asarray(code.hx), np.asarray(code.hz)):
        m, n = h.shape
        H = space_time.window_matrix(h, R)
        assert H.dtype == np.uint8 and np.array_equal(H, SP.window_matrix(h, R))
        e, u = rng.integers(0, 2, (R, n)), rng.integers(0, 2, (R, m))
        before = np.zeros_like(u)
        before[1:] = u[:-1]
        d = ((e @ h.T.astype(np.int64)) + u + before) % 2  # H e_t ^ u_t ^ u_{t-1}
        assert np.array_equal(H.astype(np.int64) @ np.r_[e.reshape(-1), u.reshape(-1)] % 2, d.reshape(-1))
        assert gf2.rank(H) == R * m
    assert np.array_equal(space_time.window_matrix(code.hx, 1), np.hstack([np.asarray(code.hx) % 2, np.eye(code.hx.shape[0])]).astype(np.uint8))
    with pytest.raises(ValueError):
        space_time.window_matrix(code.hx, 0)


# ---- OSD-0 on packed rows against the existing OSD restatement ----------------------------------------------------------------------------
def test_packed_osd0_equals_the_existing_osd_restatement():
    code = case_code("tiny_r2")
    rng = np.random.default_rng(7)
    for h, R in ((code.hx, 2), (code.hz, 3)):
        H = SP.window_matrix(h, R)
        for trial in range(6):
            r = rng.normal(1.0, 2.0, H.shape[1]).astype(np.float32)
            r[::5] = np.float32(0.5)   # ties
            r[-3:] = np.float32(np.inf)  # a perfect read-out
            r[1] = np.float32(-0.0)
            synd = rng.integers(0, 2, H.shape[0]).astype(np.uint8)
            e = SP.osd0(H, synd, r)
            ref, _ = osd_search(r, H, synd, OSD_0, 0)
            assert np.array_equal(e, ref)
            assert np.array_equal(H.astype(np.int64) @ e % 2, synd)
    Hd = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.uint8)  # a dependent row, one inconsistent syndrome
    for synd in ([1, 1, 0], [1, 0, 1]):
        r = np.array([0.3, 0.2, 0.1], np.float32)
        assert np.array_equal(SP.osd0(Hd, np.array(synd, np.uint8), r), osd_search(r, Hd, np.array(synd, np.uint8), OSD_0, 0)[0])


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------
def _pipeline(case, **kw):
    code, (sx, sz), st = case_code(case), case_inputs(case), case_settings(case)
    out = SP.post_decode(code, sx, sz, st["factors"], st["owns"], st["pre_iter"], st["cn_type"], st["restart"], gamma=st["gamma_x"],
                         gamma_last=st["gamma_last_x"], llr_const=st["llr_const"], **kw)
    ok = ST.window_test(code, out[0], out[1], out[2], out[3], ST.differences(sx, None), ST.differences(sz, None))
    return out, ok


@pytest.mark.parametrize("case", ["tiny_r1", "tiny_r2", "tiny_r3", "ghp_r2"])
@pytest.mark.parametrize("method", ["lsd", "osd0"])
def test_every_window_post_processed_without_caps_passes_the_joint_test(case, method):
    out, ok = _pipeline(case, method=method, fallback=None)
    stats, post, nact, nfall = out[4:]
    assert nact >= len(stats) // 4 and nfall == 0
    assert (stats[:, 0] == 1).all() and ok.all()
    plain = ST.stbp4_decode(case_code(case), *case_inputs(case), **case_settings(case))
    solved = plain[4][:, 0] == 1
    for a, b in zip(out[:4], plain[:4]):
        assert np.array_equal(a[solved], b[solved]), "solved windows are returned as the decoder returns them"
    assert np.array_equal(out[4][:, 1:], plain[4][:, 1:])
    assert (post[:, solved] == [1, 0, 0, 0]).all()
    if method == "lsd":
        assert (post[:, ~solved, 3] > 0).any()
    else:
        assert (post == [1, 0, 0, 0]).all()


@pytest.mark.parametrize("case", ["tiny_r1", "tiny_r2", "tiny_r3", "ghp_r2"])
def test_low_pivot_cap_takes_the_fallback_and_still_solves(case):
    cap = LOW_CAP[case]
    out, ok = _pipeline(case, method="lsd", max_pivots=cap, fallback=None)
    stats, post, nact, _ = out[4:]
    unsolved = (post[:, :, 0] == 0).any(0)
    assert 0 < int(unsolved.sum()) < nact, "the cap must leave found = 0 and found = 1 windows"
    assert np.array_equal(stats[:, 0] == 0, unsolved) and ok[~unsolved].all()
    out2, ok2 = _pipeline(case, method="lsd", max_pivots=cap, fallback="osd0")
    assert out2[7] == int(unsolved.sum()) and out2[6] == nact
    assert (out2[4][:, 0] == 1).all() and ok2.all()
    assert np.array_equal(out2[5], post), "the LSD stats stay visible behind the fallback"
    keep = ~unsolved
    for a, b in zip(out2[:4], out[:4]):
        assert np.array_equal(a[keep], b[keep])


# ---- the new wrappers against a recording library ---------------------------------------------------------------------------------------
n, m_x, m_z, B, R = 6, 3, 2, 4, 2


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


@pytest.fixture
def lib_graph(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(G, "_stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    g = G.TannerGraph.__new__(G.TannerGraph)
    g.handle, g.device = None, torch.device("cpu")
    g.n, g.m_x, g.m_z = n, m_x, m_z
    yield g, rec
    g.handle = None


def p(t):
    return None if t is None else ("ptr", t.data_ptr())


def _norm(a):
    return ("ptr", a.value) if isinstance(a, C.c_void_p) else a


def run(g, rec, fn, *args, **kw):
    rec.calls.clear()
    with guarded(g) as h:
        out = fn(*args, **kw)
    assert len(rec.calls) == 1, [c[0] for c in rec.calls]
    name, cargs = rec.calls[0]
    return out, name, [_norm(a) for a in cargs], [(r.shape, r.dtype) for r in h.records]


def z(shape, dtype=U8):
    return torch.zeros(shape, dtype=dtype)


def test_stbp4_decode_soft_wrapper(lib_graph):
    g, rec = lib_graph
    sx, sz, px = z((B, R, m_x)), z((B, R, m_z)), z((B, m_x))
    lz = z((B, R, m_z), F32)
    f, o = np.array([0.5, 0.25], np.float32), np.array([1.0, 0.5], np.float32)
    out, name, a, allocs = run(g, rec, g.stbp4_decode_soft, sx, sz, f, o, 7, 5, "minsum", restart=False, prev_x=px, llr_const=1.5, synd_llr_z=lz,
                               gamma_x=2.0, gamma_last_x=INF)
    assert name == "fgnn_stbp4_decode_soft"
    xh, zh, uxh, uzh, stats, marg, gx, gz = out
    assert a[:9] == [None, 2, 2, a[3], a[4], 7, 5, 0, R] and isinstance(a[3], int) and isinstance(a[4], int)
    assert a[9:] == [None, 1.5, p(sx), p(sz), p(px), None, None, 2.0, INF, p(lz), INF, INF, B, p(xh), p(zh), p(uxh), p(uzh), p(stats),
                     p(marg), p(gx), p(gz), None]
    assert len(a) == len(_lib._SIGNATURES["fgnn_stbp4_decode_soft"][1]) == len(_lib._SIGNATURES["fgnn_stbp4_decode"][1]) + 3
    assert allocs == [((B, R, n), U8), ((B, R, n), U8), ((B, R, m_x), U8), ((B, R, m_z), U8), ((B, 4), I32), ((B, R, 3, n), F32),
                      ((B, R, m_x), F32), ((B, R, m_z), F32)]
    # the plain wrapper is unchanged: the same first 27 arguments, no soft allocation
    out5, name5, a5, allocs5 = run(g, rec, g.stbp4_decode, sx, sz, f, o, 7, 5, "minsum", restart=False, prev_x=px, llr_const=1.5, synd_llr_z=lz,
                                   gamma_x=2.0, gamma_last_x=INF)
    assert name5 == "fgnn_stbp4_decode" and len(out5) == 5 and allocs5 == allocs[:5] and len(a5) == len(a) - 3
    assert a5[5:22] == a[5:22] and a5[-1] is None
    with pytest.raises(ValueError, match="rounds is needed"):
        g.stbp4_decode_soft(None, None, f, o, 7, 5)
    with pytest.raises(ValueError, match="synd_z must have shape"):
        g.stbp4_decode_soft(sx, z((B, R + 1, m_z)), f, o, 7, 5)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.stbp4_decode_soft(sx, sz, f, o, 7, 5, "max")


@pytest.mark.parametrize("side", [0, 1])
def test_st_window_problem_wrapper(lib_graph, side):
    g, rec = lib_graph
    m = m_x if side == 0 else m_z
    marg, gam, synd, prev = z((B, R, 3, n), F32), z((B, R, m), F32), z((B, R, m)), z((B, m))
    index = torch.tensor([3, 1, 0, 0], dtype=I32)
    (d, llr), name, a, allocs = run(g, rec, g.st_window_problem, side, marg, gam, synd=synd, prev=prev, index=index, nact=2)
    assert name == "fgnn_st_window_problem"
    assert a == [None, side, R, p(synd), p(prev), p(marg), p(gam), p(index), 2, p(d), p(llr), None]
    assert allocs == [((2, R * m), U8), ((2, R * (n + m)), F32)]
    (d, llr), _, a, allocs = run(g, rec, g.st_window_problem, side, marg, gam)
    assert a == [None, side, R, None, None, p(marg), p(gam), None, B, p(d), p(llr), None]
    assert allocs == [((B, R * m), U8), ((B, R * (n + m)), F32)]
    (d, llr), _, a, allocs = run(g, rec, g.st_window_problem, side, marg, gam, index=index, nact=0)
    assert a[8] == 0 and allocs == [((0, R * m), U8), ((0, R * (n + m)), F32)]
    for bad, msg in ((dict(side=2), "side must be 0 or 1"), (dict(nact=-1), "nact must be >= 0"), (dict(nact=B + 1), "the batch holds"),
                     (dict(index=index, nact=5), "index holds 4 entries"), (dict(gam=z((B, R, m + 1), F32)), "gam must have shape"),
                     (dict(synd=z((B, R, m), I32)), "synd must be torch.uint8"), (dict(marg=z((B, 3, n), F32)), "marg must have shape"),
                     (dict(index=index.to(torch.int64), nact=1), "index must be torch.int32")):
        kw = dict(side=side, marg=marg, gam=gam)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            g.st_window_problem(kw.pop("side"), kw.pop("marg"), kw.pop("gam"), **kw)


@pytest.mark.parametrize("side", [0, 1])
def test_st_window_apply_wrapper(lib_graph, side):
    g, rec = lib_graph
    m = m_x if side == 0 else m_z
    hat, u_hat, e = z((B, R, n)), z((B, R, m)), z((3, R * (n + m)))
    index = torch.tensor([2, 0, 1], dtype=I32)
    out, name, a, allocs = run(g, rec, g.st_window_apply, side, e, hat, u_hat, index=index)
    assert name == "fgnn_st_window_apply" and out[0] is hat and out[1] is u_hat and allocs == []
    assert a == [None, side, R, p(e), p(index), 3, p(hat), p(u_hat), None]
    _, _, a, _ = run(g, rec, g.st_window_apply, side, e, hat, u_hat, index=index, nact=2)
    assert a[5] == 2
    for args, kw, msg in (((2, e, hat, u_hat), {}, "side must be 0 or 1"), ((side, e, hat, u_hat), dict(nact=4), "e holds 3 rows"),
                          ((side, e, hat[:, :, :n - 1], u_hat), {}, "hat must have shape"),
                          ((side, e, hat, z((B, R, m + 1))), {}, "u_hat must have shape"),
                          ((side, z((3, R * (n + m) + 1)), hat, u_hat), {}, "e must have shape"),
                          ((side, e, hat.permute(0, 2, 1).contiguous().permute(0, 2, 1), u_hat), {}, "must be contiguous"),
                          ((side, z((B + 1, R * (n + m))), hat, u_hat), {}, "the batch holds")):
        with pytest.raises(ValueError, match=msg):
            g.st_window_apply(*args, **kw)


def test_header_states_the_three_contracts_and_the_binding_lists_them():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "fgnn.h")) as f:
        text = f.read()
    for name, nargs in (("fgnn_stbp4_decode_soft", 31), ("fgnn_st_window_problem", 12), ("fgnn_st_window_apply", 9)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS and len(_lib._SIGNATURES[name][1]) == nargs
    with open(os.path.join(here, "..", "feedback_gnn_amd", "csrc", "Makefile")) as f:
        assert "fgnn_stpost.hip" in f.read()


def test_post_decoder_refuses_bad_settings_and_windows_beyond_the_solvers():
    class _Dec:
        rounds, graph = 40, None
        code = case_code("ghp_r2")
    with pytest.raises(ValueError, match="method must be one of"):
        space_time.SpaceTimePostDecoder(_Dec(), method="osd_cs")
    with pytest.raises(ValueError, match="fallback must be"):
        space_time.SpaceTimePostDecoder(_Dec(), fallback="lsd")
    with pytest.raises(ValueError, match="must be >= 0"):
        space_time.SpaceTimePostDecoder(_Dec(), max_pivots=-1)
    m, nq = _Dec.code.hx.shape
    with pytest.raises(ValueError, match=r"fgnn_lsd takes at most 8192.*method='osd0'"):
        space_time.SpaceTimePostDecoder(_Dec(), fallback=None).window_graph(0, 8192 // m + 1)
    with pytest.raises(ValueError, match="OSD-0 takes at most 16384"):
        space_time.SpaceTimePostDecoder(_Dec(), method="osd0").window_graph(1, 16384 // (nq + m) + 1)
