"""The Python layer in front of the library, on the CPU and without the library: what every `TannerGraph` wrapper hands to its C
entry point (symbol, argument order, scalars, input and output pointers), what it allocates through `_new` and in which order, and
every message it refuses a call with; what the five code-based decoders forward to the graph and refuse; how the nine sharded models
walk their sample stream.  The library is replaced by a recorder whose every function returns 0, the graph of the decoders and
models by a stub that records its calls and returns zero tensors: nothing here computes, the tests pin the plumbing."""
import contextlib
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd import _lib, decoding, graph as G, relay
from feedback_gnn_amd._lib import CN_TYPES, FB_RULES
from guarded import guarded
from helpers import code

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
n, m_x, m_z, E_x, E_z, B = 6, 3, 2, 9, 6, 4
ROWS = dict(rows_xp=2, rows_zp=3, rows_hxp=4, rows_hzp=5, rows_lx=1, rows_lz=7)
INF = float("inf")


# ---- TannerGraph against a recording library ----------------------------------------------------------------------------------------
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
    g.n, g.m_x, g.m_z, g.E_x, g.E_z = n, m_x, m_z, E_x, E_z
    for k, v in ROWS.items():
        setattr(g, k, v)
    yield g, rec
    g.handle = None  # nothing for __del__ to destroy


def p(t):
    """What a pointer argument must look like after `_norm`."""
    return None if t is None else ("ptr", t.data_ptr())


def _norm(a):
    return ("ptr", a.value) if isinstance(a, C.c_void_p) else a


def run(g, rec, fn, *args, **kw):
    """One wrapper call under the guarded allocator: (result, symbol, normalised C arguments, [(shape, dtype)] of the `_new` calls)."""
    rec.calls.clear()
    with guarded(g) as h:
        out = fn(*args, **kw)
    assert len(rec.calls) == 1, [c[0] for c in rec.calls]
    name, cargs = rec.calls[0]
    return out, name, [_norm(a) for a in cargs], [(r.shape, r.dtype) for r in h.records]


def z(shape, dtype=U8):
    return torch.zeros(shape, dtype=dtype)


def synd():
    return z((B, m_x)), z((B, m_z))


def shaped(t, shape, dtype):
    return tuple(t.shape) == tuple(shape) and t.dtype == dtype


XZS = [((B, n), U8), ((B, n), U8), ((B, 4), I32)]


@pytest.mark.parametrize("method,symbol", [("bp4_decode", "fgnn_bp4_decode"), ("bp4_decode_layered", "fgnn_bp4_decode_layered")])
@pytest.mark.parametrize("want_logits", [False, True])
@pytest.mark.parametrize("return_msgs", [False, True])
def test_bp4_decode_and_layered(lib_graph, method, symbol, want_logits, return_msgs):
    g, rec = lib_graph
    sx, sz = synd()
    llr_ch = z((B, 3, n), F32) if want_logits else None
    mi = (z((B, E_x), F32), z((B, E_z), F32)) if return_msgs else None
    out, name, a, allocs = run(g, rec, getattr(g, method), sx, sz, 5, "minsum", 0.5, llr_ch=llr_ch, llr_const=1.5, msg_init=mi,
                               return_msgs=return_msgs, want_logits=want_logits)
    assert name == symbol
    assert a == [None, CN_TYPES["minsum"], 5, 0.5, p(llr_ch), 1.5, p(sx), p(sz), B, p(mi and mi[0]), p(mi and mi[1]), p(out["llr"]),
                 p(out["x_hat"]), p(out["z_hat"]), p(out["x_logit"]), p(out["z_logit"]), p(out.get("msg_x")), p(out.get("msg_z")), None]
    assert allocs == ([((B, 3, n), F32), ((B, n), U8), ((B, n), U8)]
                      + [((B, ROWS["rows_xp"]), F32), ((B, ROWS["rows_zp"]), F32)] * want_logits + [((B, E_x), F32), ((B, E_z), F32)] * return_msgs)
    assert set(out) == {"llr", "x_hat", "z_hat", "x_logit", "z_logit"} | ({"msg_x", "msg_z"} if return_msgs else set())
    assert shaped(out["llr"], (B, 3, n), F32) and shaped(out["x_hat"], (B, n), U8) and shaped(out["z_hat"], (B, n), U8)
    assert (out["x_logit"] is None and out["z_logit"] is None) != want_logits
    if want_logits:
        assert shaped(out["x_logit"], (B, 2), F32) and shaped(out["z_logit"], (B, 3), F32)
    if return_msgs:
        assert shaped(out["msg_x"], (B, E_x), F32) and shaped(out["msg_z"], (B, E_z), F32)


@pytest.mark.parametrize("want_tape", [False, True])
def test_bp4_decode_trace(lib_graph, want_tape):
    g, rec = lib_graph
    sx, sz = synd()
    llr_ch = None if want_tape else z((B, 3, n), F32)
    mi = (z((B, E_x), F32), z((B, E_z), F32)) if want_tape else None
    T = 3
    out, name, a, allocs = run(g, rec, g.bp4_decode_trace, sx, sz, T, "boxplus", 0.5, llr_ch=llr_ch, llr_const=1.5, msg_init=mi,
                               want_tape=want_tape)
    assert name == "fgnn_bp4_decode_trace"
    assert a == [None, CN_TYPES["boxplus"], T, 0.5, p(llr_ch), 1.5, p(sx), p(sz), B, p(mi and mi[0]), p(mi and mi[1]), p(out["llr"]),
                 p(out["x_hat"]), p(out["z_hat"]), p(out["x_logit"]), p(out["z_logit"]), p(out.get("tape_x")), p(out.get("tape_z")), None]
    assert allocs == ([((B, 3, n), F32), ((B, n), U8), ((B, n), U8), ((T + 1, B, 2), F32), ((T + 1, B, 3), F32)]
                      + [((T + 1, B, E_x), F32), ((T + 1, B, E_z), F32)] * want_tape)
    assert set(out) == {"llr", "x_hat", "z_hat", "x_logit", "z_logit"} | ({"tape_x", "tape_z"} if want_tape else set())
    assert shaped(out["x_logit"], (T + 1, B, 2), F32) and shaped(out["z_logit"], (T + 1, B, 3), F32)
    if want_tape:
        assert shaped(out["tape_x"], (T + 1, B, E_x), F32) and shaped(out["tape_z"], (T + 1, B, E_z), F32)


@pytest.mark.parametrize("given", ["synd", "llr", "both", "llr+B", "B"])
@pytest.mark.parametrize("want_soft", [False, True])
@pytest.mark.parametrize("want_hard", [False, True])
def test_bp2_decode(lib_graph, given, want_soft, want_hard):
    g, rec = lib_graph
    s = z((B, m_x)) if given in ("synd", "both") else None
    llr_ch = z((B, n), F32) if given in ("llr", "both", "llr+B") else None
    Bk = B if given in ("llr+B", "B") else None
    (soft, hard), name, a, allocs = run(g, rec, g.bp2_decode, s, 5, "boxplus", 0.5, llr_ch=llr_ch, llr_const=1.5, B=Bk, want_soft=want_soft,
                                        want_hard=want_hard)
    assert name == "fgnn_bp2_decode"
    assert a == [None, CN_TYPES["boxplus"], 5, 0.5, p(llr_ch), 1.5, p(s), B, p(soft), p(hard), None]
    assert allocs == [((B, n), F32)] * want_soft + [((B, n), U8)] * want_hard
    assert (soft is None) != want_soft and (hard is None) != want_hard
    assert soft is None or shaped(soft, (B, n), F32)
    assert hard is None or shaped(hard, (B, n), U8)


def test_bp2_decode_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    s = z((B, m_x))
    (soft, hard), _, a, allocs = run(g, rec, g.bp2_decode, s, 5)
    assert a[1:4] == [CN_TYPES["boxplus-phi"], 5, 1.0] and a[4:6] == [None, 0.0] and allocs == [((B, n), F32), ((B, n), U8)]
    rec.calls.clear()
    f = z((B, m_x), F32)
    refused(ValueError, "Unknown node type.", g.bp2_decode, f, 5, "boxminus")  # before the syndrome
    refused(ValueError, "syndrome must be torch.uint8, got torch.float32", g.bp2_decode, f, 5, llr_ch=z((B, n)))  # before llr_ch
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.bp2_decode, z((B, m_z)), 5)
    refused(ValueError, "llr_ch must be torch.float32, got torch.uint8", g.bp2_decode, s, 5, llr_ch=z((B, n)))
    refused(ValueError, "llr_ch must have shape (4, 6), got (4, 3, 6)", g.bp2_decode, s, 5, llr_ch=z((B, 3, n), F32))
    refused(ValueError, "llr_ch must have shape (4, 6), got (5, 6)", g.bp2_decode, s, 5, llr_ch=z((5, n), F32))  # the syndrome's batch size wins
    refused(ValueError, "llr_ch must have shape (5, 6), got (4, 6)", g.bp2_decode, None, 5, llr_ch=z((B, n), F32), B=5)  # then B
    refused(ValueError, "llr_ch must have shape (4, 6), got (5, 6)", g.relay_decode, s, z((5, n), F32), 7, 8, 3, llr_ch=z((5, n), F32))
    refused(ValueError, "llr_ch must have shape (5, 6), got (4, 6)", g.relay_decode, None, z((5, n), F32), 7, 8, 3, llr_ch=z((B, n), F32), B=5)
    assert rec.calls == []


@pytest.mark.parametrize("given", ["synd", "llr", "both"])
def test_relay_decode(lib_graph, given):
    g, rec = lib_graph
    s = z((B, m_x)) if given != "llr" else None
    llr_ch = z((B, n), F32) if given != "synd" else None
    gamma = z((5, n), F32)
    (hard, stats), name, a, allocs = run(g, rec, g.relay_decode, s, gamma, 7, 8, 3, 0.5, llr_ch=llr_ch, llr_const=1.5)
    assert name == "fgnn_relay_decode"
    assert a == [None, 0.5, 7, 5, 8, 3, p(gamma), p(llr_ch), 1.5, p(s), B, p(hard), p(stats), None]
    assert allocs == [((B, n), U8), ((B, 4), I32)] and shaped(hard, (B, n), U8) and shaped(stats, (B, 4), I32)


def _quaternary_inputs(given):
    """(synd_x, synd_z, llr_ch, B keyword) for one of the ways a step-loop decoder learns its batch size."""
    sx, sz = synd()
    return {"both": (sx, sz, None, None), "x": (sx, None, None, None), "z": (None, sz, z((B, 3, n), F32), None),
            "llr": (None, None, z((B, 3, n), F32), None), "B": (None, None, None, B)}[given]


GIVEN = ["both", "x", "z", "llr", "B"]


@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("with_gamma", [True, False])
def test_relay4_decode(lib_graph, given, with_gamma):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given)
    gamma = z((5, n), F32) if with_gamma else None
    (xh, zh, stats), name, a, allocs = run(g, rec, g.relay4_decode, sx, sz, gamma, 7, 8, 3, 0.5, llr_ch=llr_ch, llr_const=1.5,
                                           cn_type="boxplus-phi", B=Bk)
    assert name == "fgnn_relay4_decode"
    assert a == [None, CN_TYPES["boxplus-phi"], 0.5, 7, 5 if with_gamma else 1, 8, 3, p(gamma), p(llr_ch), 1.5, p(sx), p(sz), B, p(xh),
                 p(zh), p(stats), None]
    assert allocs == XZS and shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(stats, (B, 4), I32)


@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("max_rounds", [None, 9])
def test_bp4gd_decode(lib_graph, given, max_rounds):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given)
    (xh, zh, stats), name, a, allocs = run(g, rec, g.bp4gd_decode, sx, sz, 7, 8, max_rounds, 12.5, "boxplus", 0.5, llr_ch=llr_ch,
                                           llr_const=1.5, B=Bk)
    assert name == "fgnn_bp4gd_decode"
    assert a == [None, CN_TYPES["boxplus"], 0.5, 7, 8, n if max_rounds is None else 9, 12.5, p(llr_ch), 1.5, p(sx), p(sz), B, p(xh),
                 p(zh), p(stats), None]
    assert allocs == XZS and shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(stats, (B, 4), I32)


@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("rule,restart", [("perturb", False), ("enhanced", True)])
def test_bp4fb_decode(lib_graph, given, rule, restart):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given)
    seed, first = (1 << 64) - 1, (1 << 63) + 5
    (xh, zh, stats), name, a, allocs = run(g, rec, g.bp4fb_decode, sx, sz, rule, 7, 8, 9, 2.5, "boxplus", 0.5, restart=restart, seed=seed,
                                           first_sample=first, llr_ch=llr_ch, llr_const=1.5, B=Bk)
    assert name == "fgnn_bp4fb_decode"
    assert a == [None, FB_RULES[rule], CN_TYPES["boxplus"], 0.5, 7, 8, 9, 2.5, int(restart), seed, first, p(llr_ch), 1.5, p(sx), p(sz), B,
                 p(xh), p(zh), p(stats), None]
    assert allocs == XZS and shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(stats, (B, 4), I32)


def _tables():
    return np.array([0.75, 0.5, 0.25], np.float32), np.array([1.0, 2.0, 4.0], np.float32)


@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("restart", [False, True])
def test_mbp4_decode(lib_graph, given, restart):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given)
    factors, owns = _tables()
    (xh, zh, stats), name, a, allocs = run(g, rec, g.mbp4_decode, sx, sz, factors, owns, 7, 8, "boxplus", restart=restart, llr_ch=llr_ch,
                                           llr_const=1.5, B=Bk)
    assert name == "fgnn_mbp4_decode"
    assert a == [None, CN_TYPES["boxplus"], 3, factors.ctypes.data, owns.ctypes.data, 7, 8, int(restart), p(llr_ch), 1.5, p(sx), p(sz), B,
                 p(xh), p(zh), p(stats), None]
    assert allocs == XZS and shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(stats, (B, 4), I32)


@pytest.mark.parametrize("given", GIVEN + ["soft_x", "soft_z"])
def test_dsbp4_decode(lib_graph, given):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given if given in GIVEN else "B")
    slx = z((B, m_x), F32) if given in ("soft_x", "both") else None
    slz = z((B, m_z), F32) if given in ("soft_z", "both") else None
    if given not in GIVEN:
        Bk = None  # the batch size comes from the syndrome LLRs alone
    factors, owns = _tables()
    out, name, a, allocs = run(g, rec, g.dsbp4_decode, sx, sz, factors, owns, 7, 8, "boxplus", restart=False, llr_ch=llr_ch,
                               llr_const=1.5, synd_llr_x=slx, synd_llr_z=slz, gamma_x=2.5, gamma_z=3.5, B=Bk)
    xh, zh, uxh, uzh, stats = out
    assert name == "fgnn_dsbp4_decode"
    assert a == [None, CN_TYPES["boxplus"], 3, factors.ctypes.data, owns.ctypes.data, 7, 8, 0, p(llr_ch), 1.5, p(sx), p(sz), p(slx), 2.5,
                 p(slz), 3.5, B, p(xh), p(zh), p(uxh), p(uzh), p(stats), None]
    assert allocs == [((B, n), U8), ((B, n), U8), ((B, m_x), U8), ((B, m_z), U8), ((B, 4), I32)]
    assert shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(uxh, (B, m_x), U8) and shaped(uzh, (B, m_z), U8)
    assert shaped(stats, (B, 4), I32)


def test_dsbp4_decode_defaults_to_perfect_measurements(lib_graph):
    g, rec = lib_graph
    sx, sz = synd()
    factors, owns = _tables()
    _, _, a, _ = run(g, rec, g.dsbp4_decode, sx, sz, factors, owns, 7, 8)
    assert a[1] == CN_TYPES["minsum"] and a[7] == 1 and a[12:16] == [None, INF, None, INF]


def _osd_inputs(side, full):
    s = z((B, m_x if side == 0 else m_z))
    e_hat = z((B, n))
    if not full:
        return s, e_hat, None, None, None, None
    return s, e_hat, z((B, 3, n), F32), z((B, n), F32), z((B,), I32), z((B,), I32)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("full", [False, True])
def test_osd_wrappers(lib_graph, side, full):
    g, rec = lib_graph
    s, e_hat, marg, llr_bin, index, chosen = _osd_inputs(side, full)
    out, name, a, allocs = run(g, rec, g.osd0, side, s, e_hat, marg=marg, llr_bin=llr_bin, index=index, nact=3)
    assert name == "fgnn_osd0" and out is e_hat and allocs == []
    assert a == [None, side, p(marg), p(llr_bin), p(s), B, p(index), 3, p(e_hat), None]
    out, name, a, allocs = run(g, rec, g.osd, side, s, e_hat, "osd_cs", 7, marg=marg, llr_bin=llr_bin, index=index, nact=3, chosen=chosen)
    assert name == "fgnn_osd" and out is e_hat and allocs == []
    assert a == [None, side, 2, 7, p(marg), p(llr_bin), p(s), B, p(index), 3, p(e_hat), p(chosen), None]
    ws = z((40,))
    out, name, a, allocs = run(g, rec, g.osd_ws, side, s, e_hat, "osd_e", 5, marg=marg, llr_bin=llr_bin, index=index, nact=3,
                               chosen=chosen, workspace=ws)
    assert name == "fgnn_osd_ws" and out is e_hat and allocs == []
    assert a == [None, side, 1, 5, p(marg), p(llr_bin), p(s), B, p(index), 3, p(e_hat), p(chosen), p(ws), 40, None]


def _gnn_inputs():
    return z((B, 3, n), F32), z((B, m_x), F32), z((B, m_z), F32), z((B, m_x)), z((B, m_z))


def test_feedback_gnn(lib_graph):
    g, rec = lib_graph
    w = types.SimpleNamespace(handle=C.c_void_p(0x1234))
    llr, lhx, lhz, sx, sz = _gnn_inputs()
    out, name, a, allocs = run(g, rec, g.feedback_gnn, w, llr, lhx, lhz, sx, sz)
    assert name == "fgnn_feedback_gnn"
    assert a == [None, ("ptr", 0x1234), p(llr), p(lhx), p(lhz), p(sx), p(sz), B, p(out), None]
    assert allocs == [((B, 3, n), F32)] and shaped(out, (B, 3, n), F32)


def _four():
    return z((B, n)), z((B, n)), z((B, n)), z((B, n))


def test_syndrome_flag_update_merge(lib_graph):
    g, rec = lib_graph
    ex, ez, xh, zh = _four()
    (sx, sz), name, a, allocs = run(g, rec, g.syndrome, ex, ez)
    assert name == "fgnn_syndrome" and a == [None, p(ex), p(ez), B, p(sx), p(sz), None]
    assert allocs == [((B, m_x), U8), ((B, m_z), U8)] and shaped(sx, (B, m_x), U8) and shaped(sz, (B, m_z), U8)
    errors = z((B,))
    out, name, a, allocs = run(g, rec, g.flag_update, xh, zh, sx, sz, errors)
    assert name == "fgnn_flag_update" and out is errors and allocs == []
    assert a == [None, p(xh), p(zh), p(sx), p(sz), B, p(errors), None]
    out, name, a, allocs = run(g, rec, g.merge, errors, ex, ez, xh, zh)
    assert name == "fgnn_merge" and out is None and allocs == []
    assert a == [p(errors), p(ex), p(ez), B, n, p(xh), p(zh), None]


@pytest.mark.parametrize("want_arrays", [False, True])
def test_residual(lib_graph, want_arrays):
    g, rec = lib_graph
    ex, ez, xh, zh = _four()
    (s_hat, ls_hat, flags), name, a, allocs = run(g, rec, g.residual, ex, ez, xh, zh, want_arrays=want_arrays)
    assert name == "fgnn_residual" and a == [None, p(ex), p(ez), p(xh), p(zh), B, p(s_hat), p(ls_hat), p(flags), None]
    assert allocs == [((B, m_z + m_x), U8), ((B, 4 + 5), U8)] * want_arrays + [((B,), U8)] and shaped(flags, (B,), U8)
    if want_arrays:
        assert shaped(s_hat, (B, m_z + m_x), U8) and shaped(ls_hat, (B, 9), U8)
    else:
        assert s_hat is None and ls_hat is None


def test_residual_rows(lib_graph):
    g, rec = lib_graph
    ex, ez, xh, zh = _four()
    (ls_hat, flags), name, a, allocs = run(g, rec, g.residual_rows, _lib.ROWS_LZ, _lib.ROWS_LX, ex, ez, xh, zh)
    assert name == "fgnn_residual_rows"
    assert a == [None, _lib.ROWS_LZ, _lib.ROWS_LX, p(ex), p(ez), p(xh), p(zh), B, None, p(ls_hat), p(flags), None]
    assert allocs == [((B, 7 + 1), U8), ((B,), U8)] and shaped(ls_hat, (B, 8), U8) and shaped(flags, (B,), U8)
    (ls_hat, _), _, a, allocs = run(g, rec, g.residual_rows, 0, 3, ex, ez, xh, zh)
    assert a[1:3] == [0, 3] and allocs[0] == ((B, 2 + 5), U8)


@pytest.mark.parametrize("with_out", [False, True])
def test_pauli_noise_calls(lib_graph, with_out):
    g, rec = lib_graph
    out = (z((B, n)), z((B, n))) if with_out else None
    allocs_want = [] if with_out else [((B, n), U8), ((B, n), U8)]
    seed, first = (1 << 64) - 3, 1 << 40

    def same(res):
        ex, ez = res
        assert shaped(ex, (B, n), U8) and shaped(ez, (B, n), U8)
        assert not with_out or (ex is out[0] and ez is out[1])
        return ex, ez

    res, name, a, allocs = run(g, rec, g.pauli_noise, seed, 0.25, first, B, out=out)
    ex, ez = same(res)
    assert name == "fgnn_pauli_noise" and a == [seed, 0.25, first, B, n, p(ex), p(ez), None] and allocs == allocs_want
    first_dev = z((1,), I64)
    res, name, a, allocs = run(g, rec, g.pauli_noise, seed, 0.25, first, B, out=out, first_dev=first_dev)
    ex, ez = same(res)
    assert name == "fgnn_pauli_noise_dev" and a == [seed, 0.25, p(first_dev), first, B, n, p(ex), p(ez), None] and allocs == allocs_want
    res, name, a, allocs = run(g, rec, g.pauli_noise_xyz, seed, 0.125, 0.25, 0.5, first, B, out=out)
    ex, ez = same(res)
    assert name == "fgnn_pauli_noise_xyz" and a == [seed, 0.125, 0.25, 0.5, first, B, n, p(ex), p(ez), None] and allocs == allocs_want
    res, name, a, allocs = run(g, rec, g.pauli_noise_wt, seed, 3, first, B, out=out)
    ex, ez = same(res)
    assert name == "fgnn_pauli_noise_wt" and a == [seed, 3, first, B, n, p(ex), p(ez), None] and allocs == allocs_want


def test_pauli_noise_rounds_p_to_float32(lib_graph):
    g, rec = lib_graph
    _, _, a, _ = run(g, rec, g.pauli_noise, 1, 0.1, 0, B)
    assert a[1] == float(np.float32(0.1)) != 0.1


def test_count_flags(lib_graph):
    g, rec = lib_graph
    flags, counts, ring = z((B,)), z((3,), I64), z((4, 3), I64)
    out, name, a, allocs = run(g, rec, g.count_flags, flags, counts)
    assert name == "fgnn_count_flags" and out is counts and a == [p(flags), B, p(counts), None] and allocs == []
    rec.calls.clear()
    with guarded(g) as h:
        out = g.count_flags_batches(flags, 1, counts, ring)  # k = 4 batches of 1: the two counts differ
        scratch = h.payload(h.records[0])
    name, cargs = rec.calls[0]
    assert name == "fgnn_count_flags_batches" and out is counts and len(rec.calls) == 1
    assert [_norm(x) for x in cargs] == [p(flags), 4, 1, p(counts), p(ring), p(scratch), None]
    assert [(r.shape, r.dtype) for r in h.records] == [((8,), I32)]


# ---- refusals of TannerGraph: the full message, and which one when two inputs are wrong ---------------------------------------------
def refused(exc, message, fn, *args, **kw):
    with pytest.raises(exc, match="^" + re.escape(message) + "$"):
        fn(*args, **kw)


CN_METHODS = {
    "bp4_decode": lambda g, cn: g.bp4_decode(*synd(), 5, cn),
    "bp4_decode_layered": lambda g, cn: g.bp4_decode_layered(*synd(), 5, cn),
    "bp4_decode_trace": lambda g, cn: g.bp4_decode_trace(*synd(), 5, cn),
    "relay4_decode": lambda g, cn: g.relay4_decode(*synd(), None, 7, 8, 3, cn_type=cn),
    "bp4gd_decode": lambda g, cn: g.bp4gd_decode(*synd(), 7, 8, cn_type=cn),
    "bp4fb_decode": lambda g, cn: g.bp4fb_decode(*synd(), "no-rule", 7, 8, 9, 2.5, cn_type=cn),
    "mbp4_decode": lambda g, cn: g.mbp4_decode(*synd(), [1.0, 2.0], [1.0], 7, 8, cn_type=cn),
    "dsbp4_decode": lambda g, cn: g.dsbp4_decode(*synd(), [1.0, 2.0], [1.0], 7, 8, cn_type=cn),
}


@pytest.mark.parametrize("method", sorted(CN_METHODS))
def test_unknown_cn_type_is_refused_first(lib_graph, method):
    g, rec = lib_graph
    refused(ValueError, "Unknown node type.", CN_METHODS[method], g, "boxminus")
    assert rec.calls == []


def test_refused_rule_tables_gamma_seed(lib_graph):
    g, rec = lib_graph
    sx, sz = synd()
    bad = z((B, m_x), F32)
    refused(ValueError, 'rule must be "perturb" or "enhanced"', g.bp4fb_decode, None, None, "random", 7, 8, 9, 2.5)  # before "B is needed"
    for fn in (g.mbp4_decode, g.dsbp4_decode):
        refused(ValueError, "factors and owns must have the same length", fn, None, None, [1.0, 2.0], [1.0], 7, 8)  # before "B is needed"
    for gamma in (z((n,), F32), z((0, n), F32), z((2, 1, n), F32)):
        refused(ValueError, "gamma must have shape [num_legs, n]", g.relay_decode, sx, gamma, 7, 8, 3)
        refused(ValueError, "gamma must have shape [num_legs, n]", g.relay4_decode, sx, sz, gamma, 7, 8, 3)
    refused(ValueError, "gamma must have shape (5, 6), got (5, 7)", g.relay_decode, sx, z((5, 7), F32), 7, 8, 3)
    refused(ValueError, "gamma must be torch.float32, got torch.float64", g.relay4_decode, sx, sz, z((5, n), torch.float64), 7, 8, 3)
    # relay_decode looks at the syndrome and llr_ch before gamma, relay4_decode too
    refused(ValueError, "syndrome must be torch.uint8, got torch.float32", g.relay_decode, bad, z((n,), F32), 7, 8, 3)
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.relay4_decode, bad, sz, z((n,), F32), 7, 8, 3)
    for kw in (dict(seed=1 << 64), dict(seed=-1), dict(first_sample=1 << 64), dict(first_sample=-1)):
        refused(ValueError, "seed and first_sample must fit 64 unsigned bits", g.bp4fb_decode, sx, sz, "perturb", 7, 8, 9, 2.5, **kw)
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.bp4fb_decode, bad, sz, "perturb", 7, 8, 9, 2.5, seed=-1)
    assert rec.calls == []


def test_refused_without_a_batch_size(lib_graph):
    g, rec = lib_graph
    first = "B is needed when neither syndromes nor llr_ch are given"
    refused(ValueError, first, g.relay4_decode, None, None, None, 7, 8, 3)
    refused(ValueError, first, g.bp4gd_decode, None, None, 7, 8)
    refused(ValueError, first, g.bp4fb_decode, None, None, "perturb", 7, 8, 9, 2.5)
    refused(ValueError, first, g.mbp4_decode, None, None, [1.0], [1.0], 7, 8)
    refused(ValueError, "B is needed when neither syndromes nor llr_ch nor syndrome LLRs are given", g.dsbp4_decode, None, None, [1.0], [1.0],
            7, 8)
    assert rec.calls == []


def test_the_last_given_input_sets_the_batch_size(lib_graph):
    """B comes from the last of (synd_x, synd_z, llr_ch[, synd_llr_x, synd_llr_z]) that is given; an earlier one of another batch size is
    the one refused."""
    g, _ = lib_graph
    sx, sz = synd()
    refused(ValueError, "synd_x must have shape (5, 3), got (4, 3)", g.bp4gd_decode, sx, z((5, m_z)), 7, 8)
    refused(ValueError, "synd_x must have shape (5, 3), got (4, 3)", g.mbp4_decode, sx, sz, [1.0], [1.0], 7, 8, llr_ch=z((5, 3, n), F32))
    refused(ValueError, "synd_x must have shape (5, 3), got (4, 3)", g.dsbp4_decode, sx, sz, [1.0], [1.0], 7, 8, synd_llr_z=z((5, m_z), F32))
    refused(ValueError, "synd_llr_x must have shape (4, 3), got (4, 2)", g.dsbp4_decode, sx, sz, [1.0], [1.0], 7, 8, synd_llr_x=z((B, m_z), F32),
            B=9)


def test_refused_dtype_shape_contiguity(lib_graph):
    g, rec = lib_graph
    sx, sz = synd()
    ex, ez, xh, zh = _four()
    f = z((B, m_x), F32)
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.bp4_decode, f, sz, 5)
    refused(ValueError, "synd_z must have shape (4, 2), got (4, 3)", g.bp4_decode_layered, sx, sx, 5)
    refused(ValueError, "llr_ch must have shape (4, 3, 6), got (4, 6)", g.bp4_decode_trace, sx, sz, 5, llr_ch=z((B, n), F32))
    refused(ValueError, "msg_init_x must have shape (4, 9), got (4, 6)", g.bp4_decode, sx, sz, 5, msg_init=(z((B, E_z), F32), z((B, E_z), F32)))
    refused(ValueError, "msg_init_z must be torch.float32, got torch.uint8", g.bp4_decode_layered, sx, sz, 5, msg_init=(z((B, E_x), F32), z((B, E_z))))
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.bp4_decode, f, z((B, 5)), 5, llr_ch=z((B, n)))  # the first of three
    for fn, args in ((g.relay4_decode, (None, 7, 8, 3)), (g.bp4gd_decode, (7, 8)), (g.bp4fb_decode, ("perturb", 7, 8, 9, 2.5)),
                     (g.mbp4_decode, ([1.0], [1.0], 7, 8)), (g.dsbp4_decode, ([1.0], [1.0], 7, 8))):
        refused(ValueError, "synd_x must be torch.uint8, got torch.float32", fn, f, sz, *args)
        refused(ValueError, "synd_z must have shape (4, 2), got (4, 3)", fn, sx, sx, *args)
        refused(ValueError, "llr_ch must be torch.float32, got torch.uint8", fn, sx, sz, *args, llr_ch=z((B, 3, n)))
        refused(ValueError, "synd_x must be torch.uint8, got torch.float32", fn, f, sx, *args, llr_ch=z((B, 3, n)))  # the first of three
    refused(ValueError, "synd_llr_x must be torch.float32, got torch.uint8", g.dsbp4_decode, sx, sz, [1.0], [1.0], 7, 8, synd_llr_x=sx)
    refused(ValueError, "synd_llr_z must have shape (4, 2), got (4, 3)", g.dsbp4_decode, sx, sz, [1.0], [1.0], 7, 8, synd_llr_z=f)
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.relay_decode, sz, z((5, n), F32), 7, 8, 3)
    refused(ValueError, "llr_ch must have shape (4, 6), got (4, 3, 6)", g.relay_decode, sx, z((5, n), F32), 7, 8, 3, llr_ch=z((B, 3, n), F32))
    # the GNN's five inputs, in order
    llr, lhx, lhz, _, _ = _gnn_inputs()
    w = types.SimpleNamespace(handle=None)
    refused(ValueError, "llr must have shape (4, 3, 6), got (4, 6)", g.feedback_gnn, w, z((B, n), F32), sx, sx, f, f)
    refused(ValueError, "logit_hx must be torch.float32, got torch.uint8", g.feedback_gnn, w, llr, sx, sx, f, f)
    refused(ValueError, "logit_hz must have shape (4, 2), got (4, 3)", g.feedback_gnn, w, llr, lhx, lhx, f, f)
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.feedback_gnn, w, llr, lhx, lhz, f, f)
    refused(ValueError, "synd_z must be torch.uint8, got torch.float32", g.feedback_gnn, w, llr, lhx, lhz, sx, lhz)
    # the four [B, n] arrays, in order
    for fn, pre in ((g.residual, ()), (g.residual_rows, (4, 5))):
        refused(ValueError, "noise_x must have shape (4, 6), got (4, 3)", fn, *pre, sx, sx, sx, sx)
        refused(ValueError, "noise_z must be torch.uint8, got torch.float32", fn, *pre, ex, z((B, n), F32), sx, sx)
        refused(ValueError, "x_hat must have shape (4, 6), got (4, 3)", fn, *pre, ex, ez, sx, sx)
        refused(ValueError, "z_hat must have shape (4, 6), got (4, 2)", fn, *pre, ex, ez, xh, sz)
    refused(ValueError, "noise_z must have shape (4, 6), got (4, 2)", g.syndrome, ex, sz)
    errors = z((B,))
    refused(ValueError, "x_hat must have shape (4, 6), got (4, 3)", g.flag_update, sx, sx, sz, sz, errors)
    refused(ValueError, "z_hat must have shape (4, 6), got (4, 3)", g.flag_update, xh, sx, sz, sz, errors)
    refused(ValueError, "synd_x must have shape (4, 3), got (4, 2)", g.flag_update, xh, zh, sz, sz, errors)
    refused(ValueError, "synd_z must have shape (4, 2), got (4, 3)", g.flag_update, xh, zh, sx, sx, errors)
    refused(ValueError, "errors must have shape (4,), got (4, 3)", g.flag_update, xh, zh, sx, sz, sx)
    refused(ValueError, "errors is written in place and must be contiguous", g.flag_update, xh, zh, sx, sz, z((2 * B,))[::2])
    refused(ValueError, "errors must have shape (4,), got (4, 6)", g.merge, ex, ex, ez, xh, zh)
    refused(ValueError, "x_upd must have shape (4, 6), got (4, 3)", g.merge, errors, sx, sx, xh, zh)
    refused(ValueError, "z_upd must have shape (4, 6), got (4, 3)", g.merge, errors, ex, sx, xh, zh)
    refused(ValueError, "x_hat is written in place and must be contiguous", g.merge, errors, ex, ez, z((B, 2 * n))[:, ::2], zh)
    refused(ValueError, "z_hat is written in place and must be contiguous", g.merge, errors, ex, ez, xh, z((n, B)).t())
    assert rec.calls == []


def test_refused_noise_outputs_and_counters(lib_graph):
    g, rec = lib_graph
    ok, strided = z((B, n)), z((B, 2 * n))[:, ::2]
    for fn, args in ((g.pauli_noise, (1, 0.25, 0, B)), (g.pauli_noise_xyz, (1, 0.1, 0.1, 0.1, 0, B)), (g.pauli_noise_wt, (1, 3, 0, B))):
        refused(ValueError, "noise_x is written in place and must be contiguous", fn, *args, out=(strided, ok))
        refused(ValueError, "noise_z is written in place and must be contiguous", fn, *args, out=(ok, strided))
        refused(ValueError, "noise_x must have shape (4, 6), got (4, 3)", fn, *args, out=(z((B, m_x)), strided))
        refused(ValueError, "noise_z must be torch.uint8, got torch.int32", fn, *args, out=(ok, z((B, n), I32)))
    for first_dev in (z((1,), I32), z((2,), I64)):
        refused(ValueError, "first_dev must be one int64 on cpu", g.pauli_noise, 1, 0.25, 0, B, first_dev=first_dev)
    flags = z((B,))
    for counts in (z((3,), I32), z((4,), I64), z((6,), I64)[::2]):
        refused(ValueError, "counts must be a contiguous int64[3] on cpu", g.count_flags, flags, counts)
        refused(ValueError, "counts must be a contiguous int64[3] on cpu", g.count_flags_batches, flags, 2, counts, z((2, 3), I64))
    for ring in (z((2, 3), I32), z((3, 3), I64), z((2, 6), I64)[:, ::2]):
        refused(ValueError, "ring must be a contiguous int64[2, 3] on cpu", g.count_flags_batches, flags, 2, z((3,), I64), ring)
    for batch in (3, 0, -2):
        refused(ValueError, "flags must hold a whole number of batches", g.count_flags_batches, flags, batch, z((3,), I64), z((2, 3), I64))
    refused(ValueError, "flags must be torch.uint8, got torch.int32", g.count_flags, z((B,), I32), z((3,), I64))
    refused(ValueError, "flags must be torch.uint8, got torch.int32", g.count_flags_batches, z((B,), I32), 2, z((3,), I32), z((2, 3), I64))
    assert rec.calls == []


def test_refused_osd_inputs(lib_graph):
    g, rec = lib_graph
    s, e_hat, marg, llr_bin, index, chosen = _osd_inputs(0, True)
    d64 = z((B, n), torch.float64)
    calls = ((g.osd0, ()), (g.osd, ("osd_cs", 7)), (g.osd_ws, ("osd_cs", 7)))
    for fn, args in calls:
        ws = dict(workspace=z((40,))) if fn == g.osd_ws else {}
        refused(ValueError, "synd must have shape (4, 2), got (4, 3)", fn, 1, s, e_hat, *args, **ws)
        refused(ValueError, "e_hat is written in place and must be contiguous", fn, 0, s, z((B, 2 * n))[:, ::2], *args, marg=d64, **ws)
        refused(ValueError, "marg must be torch.float32, got torch.float64", fn, 0, s, e_hat, *args, marg=d64, llr_bin=d64, **ws)
        refused(ValueError, "llr_bin must be torch.float32, got torch.float64", fn, 0, s, e_hat, *args, marg=marg, llr_bin=d64, index=marg, **ws)
        refused(ValueError, "index must be torch.int32, got torch.int64", fn, 0, s, e_hat, *args, llr_bin=llr_bin, index=z((B,), I64), **ws)
    for fn, args in calls[1:]:
        ws = dict(workspace=z((40,), I32)) if fn == g.osd_ws else {}
        refused(ValueError, "chosen must have shape (4,), got (5,)", fn, 0, s, e_hat, *args, chosen=z((5,), I32), **ws)
        refused(ValueError, "chosen is written in place and must be contiguous", fn, 0, s, e_hat, *args, chosen=z((2 * B,), I32)[::2], **ws)
        refused(ValueError, "unknown OSD method 'osd_x' (one of " + str(sorted(G.OSD_METHODS)) + ")", fn, 0, s, e_hat, "osd_x", 7)
    refused(ValueError, "workspace must be torch.uint8, got torch.int32", g.osd_ws, 0, s, e_hat, "osd_cs", 7, workspace=z((40,), I32))
    refused(ValueError, "workspace is written in place and must be contiguous", g.osd_ws, 0, s, e_hat, "osd_cs", 7, workspace=z((80,))[::2])
    assert rec.calls == []


# ---- the decoders and models against a recording stub graph -------------------------------------------------------------------------
CODE = code("ibm72")
N, MX, MZ = CODE.hx.shape[1], CODE.hx.shape[0], CODE.hz.shape[0]
BS = 3


class StubGraph:
    """`device`, the sizes the front end reads, and every other attribute a method that records `(name, args, kwargs)` and returns zero
    tensors shaped like the real one's for a batch of `self.B`."""
    device = torch.device("cpu")

    def __init__(self, B=BS):
        self.n, self.m_x, self.m_z, self.E_x = N, MX, MZ, int(CODE.hx.sum())
        self.rows_hxp, self.rows_hzp = 5, 7
        self.B, self.calls = B, []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def f(*args, **kw):
            self.calls.append((name, args, kw))
            B = self.B
            xz = (z((B, N)), z((B, N)))
            if name in ("relay4_decode", "bp4gd_decode", "bp4fb_decode", "mbp4_decode"):
                return xz + (z((B, 4), I32),)
            if name == "dsbp4_decode":
                return xz + (z((B, MX)), z((B, MZ)), z((B, 4), I32))
            return {"pauli_noise": xz, "syndrome": (z((B, MX)), z((B, MZ))), "bsc_noise": xz[0], "set_basis": None,
                    "syndrome_noise": (torch.ones((B, MX), dtype=U8), torch.ones((B, MZ), dtype=U8)),
                    "residual": (z((B, MZ + MX)), z((B, 12)), z((B,))), "residual_rows": (z((B, 12)), z((B,))),
                    "relay_decode": (xz[0], z((B, 4), I32)), "bp2_decode": (z((B, N), F32), xz[0]),
                    "bp4_decode": dict(llr=z((B, 3, N), F32), x_hat=xz[0], z_hat=xz[1]), "compact": (z((B,), I32), 0)}[name]
        return f

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


def same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def assert_call(call, name, args, kw):
    assert call[0] == name and len(call[1]) == len(args) and sorted(call[2]) == sorted(kw), (call[0], len(call[1]), sorted(call[2]))
    for i, (a, b) in enumerate(zip(call[1], args)):
        assert same(a, b), (name, i, a, b)
    for k in kw:
        assert same(call[2][k], kw[k]), (name, k, call[2][k], kw[k])


# (class, constructor keywords, graph method, positional arguments after the syndromes, keywords beside llr_ch)
DECODERS = {
    "gd": (lambda: F.BP4GDDecoder, dict(pre_iter=5, round_iter=3, max_rounds=9, decim_llr=12.5, cn_type="boxplus", normalization_factor=0.75),
           "bp4gd_decode", lambda d: (5, 3, 9, 12.5, "boxplus", 0.75), lambda d: dict(llr_const=0.0)),
    "fb": (lambda: F.BP4FeedbackDecoder, dict(rule="enhanced", pre_iter=5, attempt_iter=3, max_attempts=9, strength=2.5, restart=True,
                                               cn_type="boxplus", normalization_factor=0.75, seed=77),
           "bp4fb_decode", lambda d: ("enhanced", 5, 3, 9, 2.5, "boxplus", 0.75),
           lambda d: dict(restart=True, seed=77, first_sample=0, llr_const=0.0)),
    "ambp": (lambda: F.AMBP4Decoder, dict(alphas=(1.0, 0.5), num_iter=5, cn_type="boxplus", factor=0.75, restart=False),
             "mbp4_decode", lambda d: (d.factors, d.owns, 5, 5, "boxplus"), lambda d: dict(restart=False, llr_const=0.0)),
    "relay": (lambda: F.RelayBP4Decoder, dict(gamma0=0.25, pre_iter=5, num_sets=2, set_max_iter=3, stop_nconv=4, normalization_factor=0.75, seed=3),
              "relay4_decode", lambda d: (d.gamma, 5, 3, 4, 0.75), lambda d: dict(llr_const=0.0)),
    "soft": (lambda: F.SoftSyndromeBP4Decoder, dict(alphas=(1.0, 0.5), num_iter=5, cn_type="boxplus", factor=0.75, restart=False),
             "dsbp4_decode", lambda d: (d.factors, d.owns, 5, 5, "boxplus"),
             lambda d: dict(restart=False, llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=INF, gamma_z=INF)),
}


def make(kind, g):
    cls, ckw, method, pos, kw = DECODERS[kind]
    return cls()(CODE, graph=g, **ckw), method, pos, kw


def call_inputs(kind, llr_ch, sx, sz, lx=None, lz=None):
    return (llr_ch, sx, sz, lx, lz) if kind == "soft" else (llr_ch, sx, sz)


def _syndromes():
    """Integer (with negatives) for x, float (with negatives) for z; `& 1` of the integer value is the bit."""
    rng = np.random.default_rng(5)
    sx = rng.integers(-4, 5, size=(MX, BS))
    sz = torch.from_numpy(rng.integers(-4, 5, size=(MZ, BS)).astype(np.float64))
    want_x = torch.from_numpy((sx & 1).astype(np.uint8)).t()
    want_z = (sz.to(I64) & 1).to(U8).t()
    assert want_x.any() and want_z.any() and (sx < 0).any() and bool((sz < 0).any())
    return sx, sz, want_x, want_z


@pytest.mark.parametrize("kind", sorted(DECODERS))
def test_decoder_call_forwards_to_the_graph(kind):
    g = StubGraph()
    d, method, pos, kw = make(kind, g)
    assert d.graph is g and d.code is CODE and d.num_vns == N and d.last_stats is None
    assert type(d).call is type(d).__call__
    sx, sz, want_x, want_z = _syndromes()
    llr_ch = torch.arange(BS * 3 * N, dtype=F32).reshape(BS, 3, N)
    x_hat, z_hat = d(call_inputs(kind, llr_ch, sx, sz))
    assert len(g.calls) == 1
    assert_call(g.calls[0], method, (want_x, want_z) + pos(d), dict(kw(d), llr_ch=llr_ch))
    assert all(t.is_contiguous() for t in g.calls[0][1][:2]) and g.calls[0][2]["llr_ch"].is_contiguous()
    assert shaped(x_hat, (BS, N), I64) and shaped(z_hat, (BS, N), torch.float64)
    assert shaped(d.last_stats, (BS, 4), I32)
    # a non-contiguous llr_ch arrives contiguous; .call is the same entry
    g.calls.clear()
    wide = torch.arange(BS * 3 * 2 * N, dtype=F32).reshape(BS, 3, 2 * N)[:, :, ::2]
    d.call(call_inputs(kind, wide, sx, sz))
    assert_call(g.calls[0], method, (want_x, want_z) + pos(d), dict(kw(d), llr_ch=wide.contiguous()))
    assert g.calls[0][2]["llr_ch"].is_contiguous()


def test_soft_syndrome_decoder_forwards_the_syndrome_llrs():
    g = StubGraph()
    d, method, pos, kw = make("soft", g)
    sx, sz, want_x, want_z = _syndromes()
    llr_ch = z((BS, 3, N), F32)
    lx = np.arange(MX * BS, dtype=np.float64).reshape(MX, BS)
    lz = torch.arange(MZ * BS, dtype=I64).reshape(MZ, BS)
    for give_x, give_z in ((True, True), (True, False), (False, True)):
        g.calls.clear()
        d((llr_ch, sx, sz, lx if give_x else None, lz if give_z else None))
        want = dict(kw(d), llr_ch=llr_ch, synd_llr_x=torch.from_numpy(lx).to(F32).t() if give_x else None,
                    synd_llr_z=lz.to(F32).t() if give_z else None)
        assert_call(g.calls[0], method, (want_x, want_z) + pos(d), want)
        assert all(v.is_contiguous() for k, v in g.calls[0][2].items() if k.startswith("synd_llr") and v is not None)
    assert shaped(d.last_u_x_hat, (BS, MX), U8) and shaped(d.last_u_z_hat, (BS, MZ), U8)


@pytest.mark.parametrize("kind", sorted(DECODERS))
def test_decoder_call_refusals(kind):
    g = StubGraph()
    d = make(kind, g)[0]
    ok, sx, sz = z((BS, 3, N), F32), z((MX, BS)), z((MZ, BS))

    def no(exc, message, llr_ch, a, b, *soft):
        refused(exc, message, d, call_inputs(kind, llr_ch, a, b, *soft))

    no(TypeError, "Invalid input dtype.", z((BS, 3, N), torch.float64), sx, sz)
    no(TypeError, "Invalid input dtype.", z((BS, 3, N + 1), torch.float64), sx, sz)  # dtype before the last dimension
    no(ValueError, "Last dimension must be of length n.", z((BS, 3, N + 1), F32), sx, sz)
    no(ValueError, "Last dimension must be of length n.", z((BS, N + 1), F32), sx, sz)  # last dimension before the rank
    no(ValueError, "llr_ch must have shape [batch_size, 3, n].", z((BS, 2, N), F32), sx, sz)
    no(ValueError, "llr_ch must have shape [batch_size, 3, n].", z((BS, N), F32), sx, sz)
    no(ValueError, "llr_ch must have shape [batch_size, 3, n].", z((2, BS, 3, N), F32), sx, sz)
    no(ValueError, "llr_ch must have shape [batch_size, 3, n].", z((BS, 2, N), F32), z((MX + 1, BS)), sz)  # llr_ch before the syndromes
    no(ValueError, f"syndrome must have shape [{MX}, batch_size], got ({MX + 1}, {BS})", ok, z((MX + 1, BS)), sz)
    no(ValueError, f"syndrome must have shape [{MX}, batch_size], got ({MX},)", ok, z((MX,)), sz)
    no(ValueError, f"syndrome must have shape [{MZ}, batch_size], got ({BS}, {MZ + 2})", ok, sx, z((BS, MZ + 2)))
    no(ValueError, "batch sizes of llr_ch and the syndromes differ.", ok, z((MX, BS + 1)), sz)
    no(ValueError, "batch sizes of llr_ch and the syndromes differ.", ok, sx, z((MZ, BS + 1)))
    no(ValueError, "batch sizes of llr_ch and the syndromes differ.", ok, z((MX, BS + 1)), z((MZ + 1, BS)))  # x's batch before z's shape
    no(ValueError, f"syndrome must have shape [{MX}, batch_size], got ({MX + 1}, {BS + 1})", ok, z((MX + 1, BS + 1)), sz)  # shape before batch
    if kind == "soft":
        no(ValueError, f"syndrome LLRs must have shape ({MX}, {BS}), got ({BS}, {MX})", ok, sx, sz, z((BS, MX), F32), None)
        no(ValueError, f"syndrome LLRs must have shape ({MZ}, {BS}), got ({MZ},)", ok, sx, sz, None, z((MZ,), F32))
        no(ValueError, f"syndrome LLRs must have shape ({MX}, {BS}), got ({MX}, 1)", ok, sx, z((MZ + 1, BS)), z((MX, 1), F32), None)  # x's LLRs before z
        no(ValueError, "batch sizes of llr_ch and the syndromes differ.", ok, z((MX, BS + 1)), sz, z((MX, 1), F32), None)  # the bits before their LLRs
    assert g.calls == [] and d.last_stats is None


def test_decoder_constructor_refusals():
    g = StubGraph()
    for cls in (F.AMBP4Decoder, F.SoftSyndromeBP4Decoder):
        refused(ValueError, "alphas must hold 1 .. 64 values", cls, CODE, alphas=(), graph=g)
        refused(ValueError, "alphas must hold 1 .. 64 values", cls, CODE, alphas=(1.0,) * 65, num_iter=0, graph=g)
        refused(ValueError, "every alpha must be finite and positive", cls, CODE, alphas=(1.0, 0.0), num_iter=0, graph=g)
        refused(ValueError, "every alpha must be finite and positive", cls, CODE, alphas=(INF,), graph=g)
        refused(ValueError, "num_iter must be a positive integer", cls, CODE, alphas=(1.0,), num_iter=0, factor=0.0, graph=g)
        refused(ValueError, "num_iter must be a positive integer", cls, CODE, alphas=(1.0,), num_iter=2.0, graph=g)
        refused(ValueError, "factor must be finite and positive", cls, CODE, alphas=(1.0,), factor=0.0, cn_type="x", graph=g)
        refused(ValueError, "factor must be finite and positive", cls, CODE, alphas=(1.0,), factor=INF, graph=g)
        refused(ValueError, "Unknown node type.", cls, CODE, alphas=(1e-30,), factor=1e30, cn_type="x", graph=g)
        refused(ValueError, "factor / alpha must be finite in float32", cls, CODE, alphas=(1e-30,), factor=1e30, graph=g)
    assert F.AMBP4Decoder(CODE, graph=g).alphas == (1.0, 0.9, 0.8, 0.7, 0.6, 0.5) and F.SoftSyndromeBP4Decoder(CODE, graph=g).alphas == (1.0,)
    d = F.AMBP4Decoder(CODE, alphas=[1, 0.5], factor=0.75, graph=g)
    assert d.alphas == (1.0, 0.5) and d.owns.dtype == d.factors.dtype == np.float32
    assert d.owns.tolist() == [1.0, 0.5] and d.factors.tolist() == [0.75, 1.5]
    refused(ValueError, "Unknown node type.", F.BP4GDDecoder, CODE, cn_type="x", graph=g)
    refused(ValueError, "Unknown node type.", F.BP4FeedbackDecoder, CODE, cn_type="x", graph=g)
    assert F.BP4GDDecoder(CODE, graph=g).max_rounds == N
    r = F.RelayBP4Decoder(CODE, num_sets=2, graph=g)
    assert r.num_legs == 3 and shaped(r.gamma, (3, N), F32)
    refused(ValueError, f"gamma must have shape {(3, N)}, got {(2, N)}", setattr, r, "gamma", np.zeros((2, N)))


# ---- the nine sharded models ------------------------------------------------------------------------------------------------------------
P_VALUES = (1e-4, 0.01, 0.05, 0.1, 0.3)


def depolarizing_expr(p0):
    p0 = np.float32(p0)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p0) / p0, dtype=np.float32))


def bsc_expr(p0):
    p0 = np.float32(p0)
    return float(-np.log((np.float32(1.0) - p0) / p0, dtype=np.float32))


def _bp4_model(kind, model, **extra):
    def build(g, **kw):
        return getattr(F, model)(CODE, make(kind, g)[0], **extra, **kw)
    return build


def _bp4_osd_model(g, **kw):
    bp4 = types.SimpleNamespace(graph=g, num_iter=5, cn_type="boxplus", normalization_factor=0.75)
    return F.BP4_OSD_Model(CODE, bp4, None, **kw)


def _binary_decoder(g):
    return F.LDPCBPDecoder(CODE.hx, cn_type="minsum", num_iter=5, normalization_factor=0.75, is_syndrome=True, graph=g)


# name -> (builder(graph, seed=, rank=, world_size=), noise method, the graph's decode method, "depolarizing" / "bsc", has next_sample_range)
MODELS = {
    "BP4_GD_Model": (_bp4_model("gd", "BP4_GD_Model"), "pauli_noise", "bp4gd_decode", "depolarizing", True),
    "BP4_Feedback_Model": (_bp4_model("fb", "BP4_Feedback_Model"), "pauli_noise", "bp4fb_decode", "depolarizing", True),
    "BP4_AMBP_Model": (_bp4_model("ambp", "BP4_AMBP_Model"), "pauli_noise", "mbp4_decode", "depolarizing", True),
    "BP4_Relay_Model": (_bp4_model("relay", "BP4_Relay_Model"), "pauli_noise", "relay4_decode", "depolarizing", True),
    "BP4_SoftSyndrome_Model": (_bp4_model("soft", "BP4_SoftSyndrome_Model", q=0.125), "pauli_noise", "dsbp4_decode", "depolarizing", True),
    "BP2_Relay_Model": (lambda g, **kw: F.BP2_Relay_Model(CODE.hx, CODE.lx, F.RelayBPDecoder(CODE.hx, num_sets=2, graph=g), **kw),
                        "bsc_noise", "relay_decode", "bsc", False),
    "BP4_OSD_Model": (_bp4_osd_model, "pauli_noise", "bp4_decode", "depolarizing", False),
    "BP2_OSD_Model": (lambda g, **kw: F.BP2_OSD_Model(CODE.hx, CODE.hx, np.arange(3), CODE.lx, _binary_decoder(g), None, **kw),
                      "bsc_noise", "bp2_decode", "bsc", False),
    "BP_BSC_Model": (lambda g, **kw: F.BP_BSC_Model(CODE.hx, _binary_decoder(g), CODE.lx, **kw), "bsc_noise", "bp2_decode", "bsc", False),
}


@pytest.fixture
def stub(monkeypatch):
    g = StubGraph(B=4)
    monkeypatch.setattr(decoding, "_binary_graph", lambda pcm, logical_pcm, device: g)
    monkeypatch.setattr(relay, "_binary_graph", lambda pcm, logical_pcm, device: g)
    return g


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_cursor(stub, name):
    build, noise, decode, _, has_range = MODELS[name]
    m = build(stub, seed=7, rank=1, world_size=3)
    assert (m.rank, m.world_size, m._next) == (1, 3, 0) and type(m).call is type(m).__call__

    def firsts():
        return [c[1][2] for c in stub.named(noise)]

    if has_range:
        assert m.next_sample_range(4) == (4, 8) and m.next_sample_range(10) == (10, 20)
    m(4, 0.05)
    assert firsts() == [4] and m._next == 12
    assert not has_range or m.next_sample_range(4) == (16, 20)
    m(4, p=0.05)
    assert firsts() == [4, 16] and m._next == 24
    m._next = 0
    assert not has_range or m.next_sample_range(4) == (4, 8)
    m.call(4, 0.05)
    assert firsts() == [4, 16, 4] and m._next == 12
    for c in stub.named(noise):
        assert c[1][0] == 7 and c[1][1] == 0.05 and c[1][3] == 4  # seed, p, batch
    assert len(stub.named(decode)) == 3
    if name == "BP4_Feedback_Model":
        assert [(c[2]["first_sample"], c[2]["seed"]) for c in stub.named(decode)] == [(4, 7), (16, 7), (4, 7)]
    if name == "BP4_SoftSyndrome_Model":
        assert [c[1] for c in stub.named("syndrome_noise")] == [(7, 0.125, 4, 4), (7, 0.125, 16, 4), (7, 0.125, 4, 4)]
    single = build(StubGraph(B=4) if name.startswith("BP4") else stub, seed=7)
    assert (single.rank, single.world_size) == (0, 1)
    single(4, 0.05)
    assert single._next == 4 and (not has_range or single.next_sample_range(4) == (4, 8))


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("prob", P_VALUES)
def test_model_prior_is_the_float32_expression(stub, name, prob):
    build, _, decode, channel, _ = MODELS[name]
    m = build(stub, seed=7)
    m(4, prob)
    want = depolarizing_expr(prob) if channel == "depolarizing" else bsc_expr(prob)
    assert stub.named(decode)[-1][2]["llr_const"] == want
    if hasattr(m, "p0"):
        m.p0 = 0.2
        m(4, prob)
        assert stub.named(decode)[-1][2]["llr_const"] == (depolarizing_expr(0.2) if channel == "depolarizing" else bsc_expr(0.2))


@pytest.mark.parametrize("prob", P_VALUES)
def test_prior_functions_are_bit_equal_to_the_expressions_they_replace(prob):
    from feedback_gnn_amd._frontend import bsc_logit, depolarizing_llr
    for fn, expr in ((depolarizing_llr, depolarizing_expr), (bsc_logit, bsc_expr)):
        got = fn(prob)
        assert type(got) is float and np.float32(got).tobytes() == np.float32(expr(prob)).tobytes() and got == expr(prob)


@pytest.mark.parametrize("kind,model,attr", [("gd", "BP4_GD_Model", "gd_decoder"), ("fb", "BP4_Feedback_Model", "decoder"),
                                             ("ambp", "BP4_AMBP_Model", "decoder"), ("relay", "BP4_Relay_Model", "relay_decoder")])
def test_bp4_model_call(kind, model, attr):
    g = StubGraph(B=4)
    d, method, pos, kw = make(kind, g)
    m = getattr(F, model)(CODE, d, seed=7)
    assert getattr(m, attr) is d and m.graph is g and m.code is CODE and m.p0 is None and m.seed == 7
    assert m.last_noise_x is None and m.last_stats is None and m.last_num_unsolved == 0
    s_hat, ls_hat = m(4, 0.05)
    assert [c[0] for c in g.calls] == ["pauli_noise", "syndrome", method, "residual"]
    noise, syn, dec, res = g.calls
    assert noise[1:] == ((7, 0.05, 0, 4), {})
    assert syn[1][0] is m.last_noise_x and syn[1][1] is m.last_noise_z and syn[2] == {}
    want_kw = dict(kw(d), llr_ch=None, llr_const=depolarizing_expr(0.05))
    if kind == "fb":
        want_kw.update(first_sample=0, seed=7)
    assert_call(dec, method, (z((4, MX)), z((4, MZ))) + pos(d), want_kw)
    assert len(res[1]) == 4 and res[2] == dict(want_arrays=True)
    assert all(a is b for a, b in zip(res[1], (m.last_noise_x, m.last_noise_z, m.last_x_hat, m.last_z_hat)))
    assert shaped(s_hat, (4, MZ + MX), U8) and shaped(ls_hat, (4, 12), U8)
    assert m.last_stats is d.last_stats and m.last_num_unsolved == 4
    if kind == "ambp":
        assert m.last_alpha is d.last_alpha and shaped(m.last_alpha, (4,), F32) and bool(torch.isnan(m.last_alpha).all())


@pytest.mark.parametrize("q", [0.125, 0.0])
def test_soft_syndrome_model_call(q):
    g = StubGraph(B=4)
    d, method, pos, kw = make("soft", g)
    m = F.BP4_SoftSyndrome_Model(CODE, d, q, seed=7, rank=1, world_size=2)
    assert m.decoder is d and m.q == q and m.q0 is None and m.last_u_x is None and m.last_u_z_hat is None
    m(4, 0.05)
    flips = [("syndrome_noise",)] if q else []
    assert [c[0] for c in g.calls] == ["pauli_noise", "syndrome"] + [f[0] for f in flips] + [method, "residual"]
    gamma = float(np.log((np.float32(1.0) - np.float32(q)) / np.float32(q), dtype=np.float32)) if q else INF
    assert m.gamma == gamma
    bit = 1 if q else 0  # the stub's flips are all ones, its syndromes all zero
    want_kw = dict(kw(d), llr_ch=None, llr_const=depolarizing_expr(0.05), gamma_x=gamma, gamma_z=gamma)
    assert_call(g.named(method)[0], method, (torch.full((4, MX), bit, dtype=U8), torch.full((4, MZ), bit, dtype=U8)) + pos(d), want_kw)
    assert same(m.last_u_x, torch.full((4, MX), bit, dtype=U8)) and same(m.last_u_z, torch.full((4, MZ), bit, dtype=U8))
    assert m.last_u_x_hat is d.last_u_x_hat and m.last_u_z_hat is d.last_u_z_hat and m.last_stats is d.last_stats
    refused(ValueError, "q must be in [0, 1)", F.BP4_SoftSyndrome_Model, CODE, d, 1.0)
    refused(ValueError, "q0 must be in [0, 1)", F.BP4_SoftSyndrome_Model, CODE, d, 0.1, q0=-0.5)
