"""BP-SI: the NumPy float32 restatement tests/si_reference.py, checked for the identities include/fgnn.h states at fgnn_si_decode, its
solve against brute force, and the benefit inactivation is built for; the Python plumbing in front of the library; the build surface of
the feature.  CPU only."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

import relay_reference as R
import si_reference as S
from feedback_gnn_amd import gf2
from helpers import code
from test_bp2_reference_cpu import _channel, _llr_const
from test_python_frontend_cpu import (B, BS, CODE, F32 as TF32, I32, MX, MZ, N, U8, StubGraph, _norm, lib_graph, m_x, n, p, refused, run,  # noqa: F401
                                      shaped, z)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def noisy(hx, B, prob, seed):
    e = (np.random.RandomState(seed).rand(B, hx.shape[1]) < prob).astype(np.int64)
    return e, (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


def syndrome_of(hx, e):
    return (np.asarray(e, np.int64) @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


# ---- identity: without a group the decoder is one Relay-BP leg with gamma 0 -------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5", "hp_c7"])
def test_no_groups_is_relay_with_gamma_zero(name):
    c = code(name)
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    Bn, T = 24, 9
    e, synd = noisy(hx, Bn, 0.06, 3)
    gamma = np.zeros((1, hx.shape[1]), F32)
    seen = []
    for llr in (dict(llr_const=_llr_const(0.06)), dict(llr_ch=_channel(Bn, hx.shape[1], 4))):
        for factor in (1.0, 0.8):
            h0, s0, _ = R.relay_decode(hx, synd, gamma, T, T, 1, factor, **llr)
            h1, s1 = S.si_decode(hx, hz, synd, T, 5, 0, factor, **llr)
            found = s0[:, 0] > 0
            assert np.array_equal(h0, h1) and np.array_equal(s0[:, 0], s1[:, 0]) and np.array_equal(s0[found, 3], s1[found, 2])
            assert not s1[:, 1].any() and (s1[:, 3] == -1).all() and not s1[~found, 2].any()
            seen += found.tolist()
    assert any(seen) and not all(seen)


# ---- what found means, and what a sample without a solution keeps --------------------------------------------------------------------
@pytest.mark.parametrize("name,prob", [("toric4", 0.12), ("hp_c7", 0.08), ("gb126", 0.08)])
def test_found_outputs_satisfy_the_syndrome_and_the_others_are_plain_bp(name, prob):
    c = code(name)
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    e, synd = noisy(hx, 32, prob, 11)
    plain, _ = S.si_decode(hx, hz, synd, 6, 4, 0, llr_const=_llr_const(prob))
    hard, stats, trace = S.si_decode(hx, hz, synd, 6, 4, 7, llr_const=_llr_const(prob), want_trace=True)
    found = stats[:, 0] == 1
    assert np.array_equal(syndrome_of(hx, hard[found]), synd[found])
    assert np.array_equal(hard[~found], plain[~found]) and (syndrome_of(hx, hard[~found]) != synd[~found]).any(1).all()
    assert (stats[~found] == (0, 7, 0, -1)).all(), "attempts made, and nothing else"
    rescued = found & (stats[:, 1] > 0)
    assert rescued.any() and (~found).any(), "the batch must hold rescues and samples no group rescues"
    for b in np.nonzero(rescued)[0]:
        a = stats[b, 1]
        assert len(trace[b]) == a and trace[b][-1] == (stats[b, 3], stats[b, 2], "solved") and all(t[2] != "solved" for t in trace[b][:-1])
        assert len({t[0] for t in trace[b]}) == a, "no group is tried twice"


def test_groups_come_in_ascending_key_order_and_empty_groups_are_left_out():
    P = np.array([0.5, -0.25, 0.0, -0.0, 3.0, -0.5], F32)
    groups = [np.array([4]), np.array([], np.int64), np.array([0, 1]), np.array([2, 3]), np.array([1, 5]), np.array([0, 1])]
    keys = S.group_keys(P, groups)
    assert [j for _, j in keys] == [3, 2, 4, 5, 0], "score 0 first; a tie in the score goes to the lower index; the empty group is absent"
    assert keys[1][0] >> 32 == int(np.array(0.75, F32).view(np.uint32)) and keys[1][0] >> 32 == keys[2][0] >> 32 == keys[3][0] >> 32


# ---- the solve against brute force ---------------------------------------------------------------------------------------------------
def brute_force(M, r):
    """All 2^|I| assignments: the solutions of M x = r, and among them the one that is 0 on every column that is a sum of earlier
    columns (found by trying every subset of the earlier columns)."""
    rows, cols = M.shape
    dependent = [any(np.array_equal(M[:, list(sub)].sum(1) % 2, M[:, c]) for k in range(c + 1) for sub in itertools.combinations(range(c), k))
                 for c in range(cols)]
    sols = [np.array(x, np.uint8) for x in itertools.product((0, 1), repeat=cols) if np.array_equal(M @ np.array(x) % 2, r)]
    pick = [x for x in sols if not x[dependent].any()]
    assert len(pick) == (1 if sols else 0), "the contract's solution is unique"
    return pick[0] if pick else None


@pytest.mark.parametrize("name", ["steane", "toric4", "hp_c7"])
def test_solve_agrees_with_brute_force(name):
    c = code(name)
    hx, hz = np.asarray(c.hx).astype(np.int64), np.asarray(c.hz).astype(np.int64)
    rng = np.random.RandomState(5)
    solvable = unsolvable = dependent = 0
    for j in range(hz.shape[0]):
        I = np.nonzero(hz[j])[0]
        adjacent = hx[:, I].any(1)
        M = hx[np.ix_(adjacent, I)]
        rhs = [M @ np.array(x) % 2 for x in itertools.product((0, 1), repeat=len(I))]
        rhs += [rng.randint(0, 2, size=M.shape[0]) for _ in range(24)]
        for r in rhs:
            want, got = brute_force(M, r), S.solve(M, r)
            assert (want is None) == (got is None) and (want is None or np.array_equal(want, got)), (name, j, r)
            solvable += want is not None
            unsolvable += want is None
        dependent += gf2.rank(M) < len(I)
    assert solvable and dependent, "solvable right-hand sides, and groups with dependent columns"
    assert unsolvable or name == "steane", "the Hamming matrix has full row rank: every right-hand side is solvable there"


def test_solve_on_a_matrix_with_a_dependent_column_in_the_middle():
    M = np.array([[1, 1, 0, 1], [0, 0, 1, 1], [1, 1, 1, 0]])   # column 1 = column 0; column 3 = columns 0 + 2; row 2 = rows 0 + 1
    assert S.solve(M, [1, 1, 0]).tolist() == [1, 0, 1, 0] and S.solve(M, [1, 0, 1]).tolist() == [1, 0, 0, 0] and S.solve(M, [1, 0, 0]) is None
    assert S.solve(np.zeros((2, 3), int), [0, 0]).tolist() == [0, 0, 0] and S.solve(np.zeros((2, 3), int), [0, 1]) is None


# ---- the benefit: the counts of the setting the feature was specified in ---------------------------------------------------------------
def test_ghp882_at_p_0_0467_every_failure_of_300_is_rescued():
    """hx of [[882,24]], hz as the groups, BSC at p = 0.0467, factor 0.8, 64 + 32 iterations, at most 20 groups, the errors drawn as
    np.random.default_rng(7).random((300, 882)) < p: plain min-sum leaves 27 of 300 unsolved, inactivation none, and no residual
    anticommutes with a logical operator.  Pinned from the restatement: 20 rescues take one group, 5 two, 1 four and 1 five."""
    c = code("ghp882")
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    prob, Bn = 0.0467, 300
    e = (np.random.default_rng(7).random((Bn, 882)) < prob).astype(np.uint8)
    hard, stats = S.si_decode(hx, hz, syndrome_of(hx, e), 64, 32, 20, 0.8, llr_const=_llr_const(prob))
    assert int((stats[:, 1] > 0).sum() + (stats[:, 0] == 0).sum()) == 27, "unsolved by attempt 0"
    assert int((stats[:, 0] == 0).sum()) == 0, "unsolved after SI"
    assert np.bincount(stats[:, 1]).tolist() == [273, 20, 5, 0, 1, 1]
    res = hard ^ e
    assert not syndrome_of(hx, res).any() and not syndrome_of(np.asarray(c.lx), res).any()


# ---- the Python layer against the recording library and the stub graph ----------------------------------------------------------------
@pytest.mark.parametrize("given", ["synd", "llr", "both"])
def test_graph_si_decode_hands_the_library_its_arguments(lib_graph, given):
    g, rec = lib_graph
    s = z((B, m_x)) if given != "llr" else None
    llr_ch = z((B, n), TF32) if given != "synd" else None
    (hard, stats), name, a, allocs = run(g, rec, g.si_decode, s, 7, 8, 9, 0.5, llr_ch=llr_ch, llr_const=1.5)
    assert name == "fgnn_si_decode"
    assert a == [None, 0.5, 7, 8, 9, p(llr_ch), 1.5, p(s), B, None, B, p(hard), p(stats), None]
    assert allocs == [((B, n), U8), ((B, 4), I32)] and shaped(hard, (B, n), U8) and shaped(stats, (B, 4), I32)


def test_graph_si_decode_index_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    s = z((B, m_x))
    index = torch.tensor([2, 0, 3, 1], dtype=I32)
    hard0, stats0 = z((B, n)), z((B, 4), I32)
    out, name, a, allocs = run(g, rec, g.si_decode, s, 7, 8, 9, index=index, nact=3, out=(hard0, stats0))
    assert a[1] == 0.8 and a[6] == 0.0 and a[9:13] == [p(index), 3, p(hard0), p(stats0)] and out[0] is hard0 and out[1] is stats0 and allocs == []
    out, name, a, allocs = run(g, rec, g.si_decode, s, 7, 8, 9, index=index)
    assert a[10] == B and allocs == [((B, n), U8), ((B, 4), I32)] and not out[0].any() and not out[1].any(), "unlisted rows read zero"
    out, name, a, allocs = run(g, rec, g.si_decode, s, 7, 8, 9, index=index[:0])
    assert a[9] is not None and a[10] == 0, "an empty list still is a list"
    rec.calls.clear()
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.si_decode, z((B, m_x - 1)), 7, 8, 9)
    refused(ValueError, "without a syndrome and llr_ch, B must be given", g.si_decode, None, 7, 8, 9)
    refused(ValueError, "index must be torch.int32, got torch.int64", g.si_decode, s, 7, 8, 9, index=index.long())
    refused(ValueError, "nact must be in 0 .. min(len(index), B)", g.si_decode, s, 7, 8, 9, index=index, nact=5)
    refused(ValueError, "hard must have shape (4, 6), got (3, 6)", g.si_decode, s, 7, 8, 9, out=(z((3, n)), stats0))
    refused(ValueError, "stats must be torch.int32, got torch.int64", g.si_decode, s, 7, 8, 9, out=(hard0, stats0.long()))
    assert rec.calls == []


class SiStub(StubGraph):
    """The stub graph with what the SI classes need on top: BP4 flags `failed`, an `si_decode` that reports found = 0 for the samples
    `missed`, and a `compact` that really compacts."""

    def __init__(self, failed=(), missed=(), B=BS):
        super().__init__(B)
        self.failed, self.missed = list(failed), list(missed)

    def residual(self, *args, **kw):
        self.calls.append(("residual", args, kw))
        flags = z((self.B,))
        flags[self.failed] = 1
        return z((self.B, MZ + MX)), z((self.B, 12)), flags

    def compact(self, mask, bit=1):
        self.calls.append(("compact", (mask.clone(), bit), {}))
        idx = torch.nonzero(mask & bit).flatten().to(I32)
        return torch.cat([idx, z((self.B - len(idx),), I32)]), len(idx)

    def si_decode(self, *args, **kw):
        self.calls.append(("si_decode", args, dict(kw)))
        hard, stats = kw["out"] if kw.get("out") is not None else (z((self.B, self.n)), z((self.B, 4), I32))
        for b in kw["index"][:kw["nact"]].tolist() if kw.get("index") is not None else range(self.B):
            stats[b] = torch.tensor([0, 6, 0, -1] if b in self.missed else [1, 2, 5, 4], dtype=I32)
        return hard, stats


def _decoder(g, pcm=None, group=None, **kw):
    import feedback_gnn_amd as F
    pcm = np.asarray(CODE.hx) if pcm is None else pcm
    group = np.asarray(CODE.hz) if group is None else group
    return F.SIDecoder(pcm, group, graph=g, **dict(dict(num_iter=5, si_iter=3, max_groups=6, normalization_factor=0.75), **kw))


def test_decoder_forwards_its_settings_and_is_called_like_relay():
    g = SiStub()
    dec = _decoder(g)
    synd = z((BS, MX))
    hard, stats = dec.decode(synd, llr_const=-2.0)
    (name, args, kw), = g.calls
    assert name == "si_decode" and args[0] is synd and args[1:] == (5, 3, 6, 0.75)
    assert kw == dict(llr_ch=None, llr_const=-2.0, B=None, index=None, nact=None, out=None) and dec.last_stats is stats
    g.calls.clear()
    llr = z((BS, N), TF32)
    e_hat = dec((llr, z((MX, BS), torch.int64)))
    (name, args, kw), = g.calls
    assert args[0].dtype == U8 and tuple(args[0].shape) == (BS, MX) and kw["llr_ch"].data_ptr() == llr.data_ptr()
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (BS, N)
    assert (dec.num_vns, dec.num_cns, dec.num_iter, dec.si_iter, dec.max_groups) == (N, MX, 5, 3, 6) and dec.group_pcm.shape == (MZ, N)
    d = _decoder(g, num_iter=64, si_iter=32, max_groups=10, normalization_factor=0.8)
    import feedback_gnn_amd as F
    dflt = F.SIDecoder(np.asarray(CODE.hx), np.asarray(CODE.hz), graph=g)
    assert (d.num_iter, d.si_iter, d.max_groups, d.normalization_factor) == (dflt.num_iter, dflt.si_iter, dflt.max_groups, dflt.normalization_factor)
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((llr, z((MX + 1, BS))))
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((llr.double(), z((MX, BS))))


def test_decoder_constructor_refusals():
    import feedback_gnn_amd as F
    g = SiStub()
    for kw, message in ((dict(num_iter=0), "num_iter must be a positive integer"), (dict(si_iter=0), "si_iter must be a positive integer"),
                        (dict(si_iter=2.0), "si_iter must be a positive integer"), (dict(max_groups=-1), "max_groups cannot be negative")):
        with pytest.raises(ValueError, match=re.escape(message)):
            _decoder(g, **kw)
    with pytest.raises(AssertionError, match="PC matrix must be a binary matrix"):
        F.SIDecoder(np.full((2, 3), 2), np.ones((1, 3), int), graph=g)
    with pytest.raises(AssertionError, match="group matrix must be a binary matrix"):
        F.SIDecoder(np.ones((2, 3), int), np.full((1, 3), 2), graph=g)
    with pytest.raises(ValueError, match="same number of columns"):
        F.SIDecoder(np.ones((2, 3), int), np.ones((1, 4), int), graph=g)
    with pytest.raises(ValueError, match="graph does not have pcm on side 0 and group_pcm on side 1"):
        _decoder(g, group=np.asarray(CODE.hz)[:-1])


def test_bp2_si_model_takes_noise_and_residual_through_side_0(monkeypatch):
    import feedback_gnn_amd as F
    from feedback_gnn_amd import inactivation
    dec_graph, model_graph = SiStub(missed=[1]), SiStub()
    made = []
    monkeypatch.setattr(inactivation, "_si_graph", lambda *a: made.append(a) or model_graph)
    dec = _decoder(dec_graph)
    m = F.BP2_SI_Model(CODE.hx, CODE.hz, CODE.lx, dec, seed=7, rank=1, world_size=2)
    assert made == [(CODE.hx, CODE.hz, CODE.lx, dec_graph.device)]
    s_hat, ls_hat = m(BS, 0.05)
    assert [c[0] for c in model_graph.calls] == ["bsc_noise", "syndrome", "residual"] and [c[0] for c in dec_graph.calls] == ["si_decode"]
    noise = m.last_noise
    sy, rs = model_graph.named("syndrome")[0], model_graph.named("residual")[0]
    assert sy[1][1] is noise and not sy[1][0].any(), "the noise is the array side 0 measures"
    assert rs[1][1] is noise and rs[1][3] is m.last_estimate and rs[1][0] is rs[1][2] and not rs[1][0].any()
    sd = dec_graph.calls[0]
    assert sd[1][1:] == (5, 3, 6, 0.75) and sd[2]["llr_const"] == F32(-np.log((F32(1) - F32(0.05)) / F32(0.05))) and sd[2]["B"] == BS
    assert shaped(s_hat, (BS, MX), U8) and shaped(ls_hat, (BS, 12 - model_graph.rows_hxp), U8), "the columns behind side 1's"
    assert m.last_num_unsolved == 1 and m.last_stats is dec.last_stats
    assert model_graph.named("bsc_noise")[0][1][2] == BS and m._next == 2 * BS


def _bp4(g):
    return types.SimpleNamespace(graph=g, num_iter=5, cn_type="boxplus", normalization_factor=0.75)


def test_bp4_si_model_hands_the_failures_to_both_sides():
    import feedback_gnn_amd as F
    g = SiStub(failed=[0, 2, 3], B=4)
    gz, gx = SiStub(missed=[2], B=4), SiStub(missed=[2, 3], B=4)
    dz = _decoder(gz)
    gx.m_x, gx.m_z = MZ, MX
    dx = _decoder(gx, pcm=np.asarray(CODE.hz), group=np.asarray(CODE.hx))
    m = F.BP4_SI_Model(CODE, _bp4(g), dz, dx, seed=7)
    s_hat, ls_hat = m(4, 0.06)
    assert [c[0] for c in g.calls] == ["pauli_noise", "syndrome", "bp4_decode", "residual", "compact", "residual", "residual_rows"]
    bp = g.named("bp4_decode")[0]
    sx, sz = bp[1][0], bp[1][1]
    (cz,), (cx,) = gz.named("si_decode"), gx.named("si_decode")
    assert cz[1][0] is sx and cx[1][0] is sz, "hx's syndrome gives z_hat, hz's gives x_hat"
    prior = F32(-np.log((F32(1) - F32(2.0 * 0.06 / 3.0)) / F32(2.0 * 0.06 / 3.0)))
    for side, c in enumerate((cz, cx)):
        kw = c[2]
        assert kw["llr_const"] == prior and kw["nact"] == 3 and kw["index"][:3].tolist() == [0, 2, 3] and kw["llr_ch"] is None
        assert kw["out"][1].data_ptr() == m.last_stats[side].data_ptr() and shaped(kw["out"][0], (4, N), U8)
    z_hat, x_hat = cz[2]["out"][0], cx[2]["out"][0]
    rr = g.named("residual_rows")[0]
    assert z_hat is not x_hat and rr[1][4] is x_hat and rr[1][5] is z_hat and rr[1][:2] == (5, 4)
    assert m.last_stats[:, 1].tolist() == [[1, 0, 0, -1], [1, 0, 0, -1]], "a sample BP4 solved reads found by attempt 0"
    assert (m.last_num_si, m.last_num_unsolved) == (3, 2) and shaped(s_hat, (4, MZ + MX), U8) and shaped(ls_hat, (4, 12), U8)
    g2 = SiStub(failed=[], B=4)
    m = F.BP4_SI_Model(CODE, _bp4(g2), dz, dx, seed=7, rank=1, world_size=3)
    gz.calls.clear()
    m(4, 0.06)
    assert not gz.named("si_decode") and (m.last_num_si, m.last_num_unsolved) == (0, 0) and m._next == 12
    with pytest.raises(ValueError, match="si_decoder_x decodes on code.hz"):
        F.BP4_SI_Model(CODE, _bp4(g), dz, types.SimpleNamespace(num_vns=N, num_cns=MZ + 1))
    with pytest.raises(ValueError, match="si_decoder_z decodes on code.hx"):
        F.BP4_SI_Model(CODE, _bp4(g), types.SimpleNamespace(num_vns=N + 1, num_cns=MX), dx)


# ---- build surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_si():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    assert "FGNN_SI_MAX_GROUP_BITS = 32" in text and "FGNN_SI_MAX_ADJACENT = 64" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+fgnn_si_decode\s*\(", text)
    assert "fgnn_si_decode" in _lib.ABI_SYMBOLS and len(_lib._SIGNATURES["fgnn_si_decode"][1]) == 14 and hasattr(L, "fgnn_si_decode")
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_si\.hip\b", mk, flags=re.M)


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd import inactivation
    from feedback_gnn_amd._frontend import ShardedModel
    from feedback_gnn_amd.graph import TannerGraph
    assert F.SIDecoder is inactivation.SIDecoder and F.BP2_SI_Model is inactivation.BP2_SI_Model and F.BP4_SI_Model is inactivation.BP4_SI_Model
    assert issubclass(F.BP2_SI_Model, ShardedModel) and issubclass(F.BP4_SI_Model, ShardedModel) and callable(TannerGraph.si_decode)
