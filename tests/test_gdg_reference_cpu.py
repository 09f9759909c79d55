"""BP-GDG: the NumPy float32 restatement tests/gdg_reference.py, checked for the identities include/fgnn.h states at fgnn_gdg_decode and
for the benefit the path tree is built for; the Python plumbing in front of the library; the build surface of the feature.  CPU only.

The restatement walks one path of a whole batch with masks.  `one_sample` below walks one path of one sample with plain control flow
and forced guesses, on the same min-sum step: the two agree, which is the third identity (path p at depth d is a depth-0 run whose
first d picks are forced to p's bits) and a check of the masks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gdg_reference as G
import relay_reference as R
from helpers import code
from test_bp2_reference_cpu import _channel, _llr_const
from test_python_frontend_cpu import (B, BS, F32 as TF32, I32, MX, N, U8, StubGraph, _norm, lib_graph, m_x, n, p, refused, shaped,  # noqa: F401
                                      z)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def noisy(hx, B, prob, seed):
    e = (np.random.RandomState(seed).rand(B, hx.shape[1]) < prob).astype(np.int64)
    return e, (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


def one_sample(Gr, L, q, s, pre_iter, round_iter, R_, tail, D, factor, guesses):
    """One path of one sample, by the text of the contract: (d, found, w, bits fixed, its)."""
    D, factor = F32(D), F32(factor)
    s = s[None, :]
    mu = np.zeros((1, Gr.E), F32)
    Lhat = L[None, :].copy()
    free = np.ones(Gr.n, bool)
    its = 0
    for r in range(R_ + 1):
        for k in range(1, (pre_iter if r == 0 else round_iter) + 1):
            x = R._bit_sums(Gr, mu) + Lhat
            mu = R._minsum(Gr, x[:, Gr.slot_bit] - mu, s, factor)
            its += 1
            P = (Lhat + R._bit_sums(Gr, mu))[0]
            d = P < 0
            if np.array_equal(Gr.hx.astype(np.int64) @ d % 2, s[0]):
                return d.astype(np.uint8), 1, int((d * q.astype(np.int64)).sum()), r, its
        if r == R_:
            return d.astype(np.uint8), 0, 0, r, its
        least = r < len(guesses) or tail == G.LEAST
        a = np.abs(P)
        cand = [v for v in range(Gr.n) if free[v]]
        v = min(cand, key=lambda v: (a[v], v)) if least else min(cand, key=lambda v: (-a[v], v))
        val = bool(P[v] < 0) ^ bool(r < len(guesses) and guesses[r])
        free[v] = False
        Lhat[0, v] = -D if val else D


# ---- identity 1: depth 0 and no rounds is one Relay-BP leg with gamma 0 ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_depth_0_no_rounds_is_relay_with_gamma_zero(name):
    hx = np.asarray(code(name).hx)
    Bn, T = 32, 12
    e, synd = noisy(hx, Bn, {"gb48": 0.06, "rsurf5": 0.15}[name], 11)  # rates at which 12 iterations solve some samples and not others
    gamma = np.zeros((1, hx.shape[1]), F32)
    mixed = 0
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=_llr_const(0.06)), dict(llr_ch=-np.abs(_channel(Bn, hx.shape[1], 3)))):
            h0, s0, _ = R.relay_decode(hx, synd, gamma, T, T, 1, factor, **llr)
            for tail in ("least", "most"):
                h1, s1, ps = G.gdg_decode(hx, synd, T, 3, 0, 0, tail=tail, factor=factor, **llr)
                assert np.array_equal(h0, h1)
                assert np.array_equal(s0[:, 0], s1[:, 0]) and np.array_equal(s0[:, 0], ps[:, 0, 0])
                solved = s0[:, 0] > 0
                mixed += bool(solved.any() and not solved.all())
                assert np.array_equal(s0[solved, 1], s1[solved, 1]) and not s1[~solved, 1].any()
                assert np.array_equal(s0[:, 3], ps[:, 0, 3]), "its of the one path = k of the one leg"
                assert not s1[:, 2:].any() and not ps[:, 0, 2].any()
    assert mixed >= 4, "solved and unsolved samples must meet in one batch, under a constant logit at least"


# ---- identities 2 and 3: binary BPGD, and a path as a forced depth-0 run ------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_paths_equal_forced_single_sample_runs(name):
    hx = np.asarray(code(name).hx)
    Gr = R._Graph(hx)
    Bn, pre, rnd, Rm = 10, 6, 3, 4
    e, synd = noisy(hx, Bn, 0.15, 5)
    llr = -np.abs(_channel(Bn, hx.shape[1], 4))
    L, q = G.priors(Gr.n, Bn, llr, 0.0)
    picked_other_value, found_paths, lost_paths = 0, 0, 0
    for depth, tail in ((0, "most"), (0, "least"), (2, "most"), (2, "least")):
        hard, stats, ps = G.gdg_decode(Gr, synd, pre, rnd, Rm, depth, tail=tail, decim_llr=25.0, factor=0.8, llr_ch=llr)
        for b in range(Bn):
            rows = []
            for path in range(1 << depth):
                d, found, w, r, its = one_sample(Gr, L[b], q[b], synd[b], pre, rnd, Rm, G.TAILS[tail], 25.0, 0.8,
                                                 [(path >> i) & 1 for i in range(depth)])
                assert ps[b, path].tolist() == [found, w, r, its], (depth, tail, b, path)
                rows.append((d, found, w, r))
            solved = [(w, i) for i, (_, f, w, _) in enumerate(rows) if f]
            best = min(solved)[1] if solved else 0
            assert stats[b].tolist() == [len(solved), rows[best][2] if solved else 0, best, rows[best][3]]
            assert np.array_equal(hard[b], rows[best][0])
            if solved:
                assert np.array_equal(hx.astype(np.int64) @ hard[b] % 2, synd[b])
                assert stats[b, 1] == (hard[b].astype(np.int64) * q[b]).sum()
            picked_other_value += best != 0
        assert (ps[:, :, 2] > 0).any(), "some path must fix a bit"
        found_paths += int((ps[:, :, 0] == 1).sum())
        lost_paths += int((ps[:, :, 0] == 0).sum())
    assert found_paths and lost_paths, "paths that find a solution and paths that do not"
    assert picked_other_value, "some output must come from a path other than 0"


def test_binary_bpgd_fixes_the_most_reliable_bit_to_its_decision():
    """depth 0 with the most reliable pick: after the first round the fixed bit is the one of largest |P| of the last test, held at its
    own decision; the messages are kept, so a run with max_rounds = 1 continues the run with max_rounds = 0."""
    hx = np.asarray(code("gb48").hx)
    Gr = R._Graph(hx)
    e, synd = noisy(hx, 12, 0.1, 2)
    llr = _llr_const(0.1)
    _, s0, p0 = G.gdg_decode(Gr, synd, 5, 4, 0, 0, tail="most", llr_const=llr)
    _, s1, p1 = G.gdg_decode(Gr, synd, 5, 4, 1, 0, tail="most", llr_const=llr)
    un = s0[:, 0] == 0
    assert un.any() and (~un).any()
    assert np.array_equal(s0[~un], s1[~un]) and np.array_equal(p0[~un], p1[~un])
    assert ((p1[un, 0, 2] == 1) | (p1[un, 0, 0] == 1)).all() and (p1[un, 0, 3] > 5).all() and (p1[un, 0, 3] <= 9).all()


def test_a_shallower_tree_is_the_front_of_a_deeper_one():
    """With the least reliable pick in the tail, path p < 2^d of a tree of depth d + 1 guesses nothing at its pick d: it is path p of
    the tree of depth d."""
    hx = np.asarray(code("rsurf5").hx)
    e, synd = noisy(hx, 9, 0.12, 8)
    llr = _llr_const(0.12)
    _, _, p1 = G.gdg_decode(hx, synd, 4, 3, 6, 1, tail="least", llr_const=llr)
    _, _, p3 = G.gdg_decode(hx, synd, 4, 3, 6, 3, tail="least", llr_const=llr)
    assert np.array_equal(p3[:, :2], p1) and not np.array_equal(p3[:, 2:4], p1)


def test_selection_rule():
    res = np.zeros((5, 4, 4), np.int64)
    res[0, :, :] = [[0, 0, 3, 9], [1, 7, 2, 5], [1, 7, 1, 4], [1, 8, 0, 1]]      # a tie in w: the lower path
    res[1, :, :] = [[1, 5, 0, 1], [1, -5, 2, 5], [0, 0, 3, 9], [1, -2, 1, 4]]    # signed comparison
    res[2, :, :] = [[0, 0, 3, 9], [0, 0, 3, 8], [0, 0, 3, 7], [0, 0, 2, 6]]      # none found: path 0
    res[3, :, :] = [[1, 4, 0, 1]] * 4                                            # all equal: path 0
    res[4, :, :] = [[0, 0, 3, 9], [0, 0, 3, 9], [0, 0, 3, 9], [1, 0, 1, 2]]      # a solution of weight 0 on the last path
    path, stats = G.select(res)
    assert path.tolist() == [1, 1, 0, 0, 3]
    assert stats.tolist() == [[3, 7, 1, 2], [3, -5, 1, 2], [0, 0, 0, 3], [4, 4, 0, 0], [1, 0, 3, 1]]


# ---- what the tree is for ----------------------------------------------------------------------------------------------------------
def test_depth_3_solves_what_100_flooding_iterations_leave():
    """hx of the bivariate-bicycle [[144,12,12]] code, BSC p = 0.04, 200 samples of RandomState(1), min-sum factor 0.8.  The
    restatement's counts: 100 flooding iterations leave 7 samples unsolved; pre_iter 32, round_iter 4, max_rounds 40 at depth 3
    leaves 0, and 8 outputs come from a path other than 0."""
    from feedback_gnn_amd import codes_q as cq
    hx = np.asarray(cq.create_bivariate_QC_codes(12, 6, [3], [1, 2], [1, 2], [3]).hx).astype(np.int64)
    assert hx.shape == (72, 144)
    Gr = R._Graph(hx)
    prob = 0.04
    e, synd = noisy(hx, 200, prob, 1)
    llr = _llr_const(prob)
    _, s100, _ = G.gdg_decode(Gr, synd, 100, 1, 0, 0, factor=0.8, llr_const=llr)
    flooding = int((s100[:, 0] == 0).sum())
    _, s32, _ = G.gdg_decode(Gr, synd, 32, 1, 0, 0, factor=0.8, llr_const=llr)
    rest = np.nonzero(s32[:, 0] == 0)[0]  # a sample plain BP solves within pre_iter is solved on every path, at round 0
    hard, stats, ps = G.gdg_decode(Gr, synd, 32, 4, 40, 3, tail="least", factor=0.8, llr_const=llr, index=rest, out=(e * 0, s32))
    tree = int((stats[:, 0] == 0).sum())
    other = int((stats[:, 2] != 0).sum())
    print("flooding-100 unsolved", flooding, "depth-3 unsolved", tree, "outputs from a path != 0", other)
    assert (flooding, tree, other) == (7, 0, 8)
    assert flooding > tree and other >= 1
    solved = stats[rest, 0] > 0
    assert np.array_equal(hard[rest][solved].astype(np.int64) @ hx.T % 2, synd[rest][solved])
    assert (ps[:, :, 0].sum(1) == stats[rest, 0]).all()


# ---- the Python layer against the recording library and the stub graph ----------------------------------------------------------------
def _calls(g, rec, fn, *args, **kw):
    from guarded import guarded
    rec.calls.clear()
    with guarded(g) as h:
        out = fn(*args, **kw)
    return out, [(name, [_norm(a) for a in cargs]) for name, cargs in rec.calls], [(r.shape, r.dtype) for r in h.records]


@pytest.mark.parametrize("given", ["synd", "llr", "both"])
@pytest.mark.parametrize("want", [False, True])
def test_graph_gdg_decode_hands_the_library_its_arguments(lib_graph, given, want):
    g, rec = lib_graph
    s = z((B, m_x)) if given != "llr" else None
    llr_ch = z((B, n), TF32) if given != "synd" else None
    out, calls, allocs = _calls(g, rec, g.gdg_decode, s, 7, 8, 9, 3, "most", 12.5, 0.5, llr_ch=llr_ch, llr_const=1.5, want_path_stats=want)
    assert [c[0] for c in calls] == ["fgnn_gdg_workspace_bytes", "fgnn_gdg_decode"]
    size = calls[0][1]
    assert size[:3] == [None, 3, B] and isinstance(size[3], type(ctypes.byref(ctypes.c_size_t())))
    hard, stats = out[:2]
    a = calls[1][1]
    ws_ptr = a[17]
    assert a[:17] == [None, 0.5, 7, 8, 9, 3, 0, 12.5, p(llr_ch), 1.5, p(s), B, None, B, p(hard), p(stats), p(out[2]) if want else None]
    assert ws_ptr is not None and a[18] == 0 and a[19] is None  # the recorder reports 0 bytes: a one-byte buffer stands in
    assert allocs == [((B, n), U8), ((B, 4), I32), ((1,), U8)] + ([((B, 8, 4), I32)] if want else [])
    assert shaped(hard, (B, n), U8) and shaped(stats, (B, 4), I32) and (not want or shaped(out[2], (B, 8, 4), I32))


def test_graph_gdg_decode_index_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    s = z((B, m_x))
    index = torch.tensor([2, 0, 3, 1], dtype=I32)
    hard0, stats0 = z((B, n)), z((B, 4), I32)
    out, calls, allocs = _calls(g, rec, g.gdg_decode, s, 7, 8, None, 2, index=index, nact=3, out=(hard0, stats0), want_path_stats=True)
    a = calls[1][1]
    assert calls[0][1][:3] == [None, 2, 3]
    assert a[1:8] == [0.8, 7, 8, n, 2, 1, 25.0] and a[9] == 0.0  # factor, max_rounds None = n, tail "least", decim_llr, llr_const
    assert a[12:16] == [p(index), 3, p(hard0), p(stats0)] and out[0] is hard0 and out[1] is stats0
    assert allocs == [((1,), U8), ((3, 4, 4), I32)]
    out, calls, allocs = _calls(g, rec, g.gdg_decode, s, 7, 8, 5, 1, index=index)
    assert calls[1][1][13] == B and allocs[:2] == [((B, n), U8), ((B, 4), I32)] and not out[0].any() and not out[1].any()
    rec.calls.clear()
    refused(ValueError, 'tail must be "least" or "most"', g.gdg_decode, s, 7, 8, 5, 1, tail="middle")
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.gdg_decode, z((B, m_x - 1)), 7, 8, 5, 1)
    refused(ValueError, "without a syndrome and llr_ch, B must be given", g.gdg_decode, None, 7, 8, 5, 1)
    refused(ValueError, "index must be torch.int32, got torch.int64", g.gdg_decode, s, 7, 8, 5, 1, index=index.long())
    refused(ValueError, "nact must be in 0 .. min(len(index), B)", g.gdg_decode, s, 7, 8, 5, 1, index=index, nact=5)
    refused(ValueError, "hard must have shape (4, 6), got (3, 6)", g.gdg_decode, s, 7, 8, 5, 1, out=(z((3, n)), stats0))
    refused(ValueError, "stats must be torch.int32, got torch.int64", g.gdg_decode, s, 7, 8, 5, 1, out=(hard0, stats0.long()))
    assert rec.calls == []


class _GdgStub(StubGraph):
    """The stub graph with a `gdg_decode` that reports `unsolved` as unsolved and a `compact` that lists them."""

    def __init__(self, unsolved):
        super().__init__()
        self.unsolved = list(unsolved)

    def gdg_decode(self, *args, **kw):
        self.calls.append(("gdg_decode", args, kw))
        if "out" in kw:
            return kw["out"]
        stats = torch.ones((BS, 4), dtype=I32)
        stats[self.unsolved, 0] = 0
        return z((BS, N)), stats

    def compact(self, mask, bit=1):
        self.calls.append(("compact", (mask,), dict(bit=bit)))
        return torch.tensor(self.unsolved + [0] * (BS - len(self.unsolved)), dtype=I32), len(self.unsolved)


CTOR = dict(pre_iter=5, round_iter=3, max_rounds=9, depth=2, tail="most", decim_llr=12.5, normalization_factor=0.75)


def _decoder(g, **kw):
    import feedback_gnn_amd as F
    return F.GDGDecoder(np.asarray(code("gb48").hx), graph=g, **dict(CTOR, **kw))


def test_decoder_prefilter_makes_two_launches():
    g = _GdgStub([2])
    dec = _decoder(g)
    synd = z((BS, MX))
    hard, stats = dec.decode(synd, llr_const=-2.0)
    first, comp, second = g.calls
    common = dict(tail="most", decim_llr=12.5, factor=0.75, llr_ch=None, llr_const=-2.0, B=None)
    assert first[0] == "gdg_decode" and first[1][0] is synd and first[1][1:] == (5, 3, 0, 0) and first[2] == common
    assert comp[0] == "compact" and comp[1][0].dtype == U8 and comp[1][0].tolist() == [0, 0, 1]
    assert second[0] == "gdg_decode" and second[1][0] is synd and second[1][1:] == (5, 3, 9, 2)
    assert second[2]["nact"] == 1 and second[2]["index"].tolist()[:1] == [2] and second[2]["out"][0] is hard and second[2]["out"][1] is stats
    assert {k: v for k, v in second[2].items() if k in common} == common
    assert dec.last_stats is stats


def test_decoder_prefilter_skips_the_tree_when_all_are_solved_and_without_a_tree():
    g = _GdgStub([])
    _decoder(g).decode(z((BS, MX)))
    assert [c[0] for c in g.calls] == ["gdg_decode", "compact"]
    g = _GdgStub([1])
    _decoder(g, depth=0, max_rounds=0).decode(z((BS, MX)))
    assert [c[0] for c in g.calls] == ["gdg_decode"] and g.calls[0][1][1:] == (5, 3, 0, 0)


def test_decoder_without_prefilter_and_call_surface():
    g = _GdgStub([1])
    dec = _decoder(g, prefilter=False)
    llr = z((BS, N), TF32)
    e_hat = dec((llr, z((MX, BS), torch.int64)))
    assert [c[0] for c in g.calls] == ["gdg_decode"] and g.calls[0][1][1:] == (5, 3, 9, 2)
    assert g.calls[0][1][0].dtype == U8 and tuple(g.calls[0][1][0].shape) == (BS, MX) and g.calls[0][2]["llr_ch"].data_ptr() == llr.data_ptr()
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (BS, N) and dec.last_stats is not None
    assert dec.max_rounds == 9 and _decoder(g, max_rounds=None).max_rounds == N and dec.num_vns == N and dec.num_cns == MX
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((llr, z((MX + 1, BS))))
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((llr.double(), z((MX, BS))))


def test_decoder_constructor_refusals():
    g = _GdgStub([])
    for kw, message in ((dict(pre_iter=0), "pre_iter must be a positive integer"), (dict(round_iter=0), "round_iter must be a positive integer"),
                        (dict(max_rounds=-1), "max_rounds cannot be negative"), (dict(depth=7), "depth must be an integer in 0 .. 6"),
                        (dict(depth=-1), "depth must be an integer in 0 .. 6"), (dict(tail="both"), 'tail must be "least" or "most"'),
                        (dict(decim_llr=0.0), "decim_llr must be positive")):
        with pytest.raises(ValueError, match=re.escape(message)):
            _decoder(g, **kw)
    import feedback_gnn_amd as F
    with pytest.raises(AssertionError, match="binary"):
        F.GDGDecoder(np.full((2, 3), 2), graph=g)


# ---- build surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_gdg():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    assert "FGNN_GDG_MOST = 0" in text and "FGNN_GDG_LEAST = 1" in text and "FGNN_GDG_MAX_DEPTH = 6" in text
    assert _lib.GDG_TAILS == {"most": 0, "least": 1} and _lib.GDG_MAX_DEPTH == 6
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("fgnn_gdg_decode", 20), ("fgnn_gdg_workspace_bytes", 4)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in _lib.ABI_SYMBOLS and len(_lib._SIGNATURES[name][1]) == nargs and hasattr(L, name)
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_gdg\.hip\b", mk, flags=re.M)


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd._frontend import ShardedModel
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.GDGDecoder) and callable(F.BP2_GDG_Model) and issubclass(F.BP2_GDG_Model, ShardedModel)
    assert callable(TannerGraph.gdg_decode) and callable(TannerGraph.gdg_workspace_bytes)
