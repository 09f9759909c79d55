"""The Python layer in front of `fgnn_lsd`, on the CPU and without the library, with the recorder and the stub graph of
tests/test_python_frontend_cpu.py: what `TannerGraph.lsd` / `lsd_max_pivots` hand to their C entry points, allocate and refuse, and
how `LSD_Decoder`'s settings, `BP4_LSD_Model` and `BP2_LSD_Model` walk compaction, the two LSD calls, the second compaction and the
OSD-0 fallback."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd import decoding, graph as G, lsd as lsd_mod
from guarded import guarded
from test_python_frontend_cpu import (B, CODE, F32, I32, I64, MX, MZ, N, U8, StubGraph, _norm, _osd_inputs, lib_graph, n, p, refused,  # noqa: F401
                                      run, shaped, z)


# ---- TannerGraph.lsd against the recording library ----------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("full", [False, True])
def test_lsd_wrapper(lib_graph, side, full):
    g, rec = lib_graph
    s, e_hat, marg, llr_bin, index, _ = _osd_inputs(side, full)
    stats_in = z((B, 4), I32) if full else None
    (out, stats), name, a, allocs = run(g, rec, g.lsd, side, s, e_hat, marg=marg, llr_bin=llr_bin, index=index, nact=3, max_pivots=17,
                                        max_rounds=5, stats=stats_in)
    assert name == "fgnn_lsd" and out is e_hat
    assert a == [None, side, p(marg), p(llr_bin), p(s), B, p(index), 3, 17, 5, p(e_hat), p(stats), None]
    assert allocs == ([] if full else [((B, 4), I32)]) and shaped(stats, (B, 4), I32) and (not full or stats is stats_in)
    (_, stats), _, a, _ = run(g, rec, g.lsd, side, s, e_hat, llr_bin=z((B, n), F32))
    assert a[6:10] == [None, 0, 0, 0], "index, nact, max_pivots, max_rounds default to none, 0, 0, 0"


def test_lsd_max_pivots(lib_graph):
    g, rec = lib_graph
    rec.calls.clear()
    with guarded(g) as h:
        cap = g.lsd_max_pivots(1)
    assert cap == 0 and h.records == [] and len(rec.calls) == 1  # the recorder leaves the c_int at 0
    name, cargs = rec.calls[0]
    assert name == "fgnn_lsd_max_pivots" and cargs[:2] == (None, 1)


def test_lsd_refusals(lib_graph):
    g, rec = lib_graph
    s, e_hat, marg, llr_bin, index, _ = _osd_inputs(0, True)
    d64 = z((B, n), torch.float64)
    refused(ValueError, "synd must have shape (4, 2), got (4, 3)", g.lsd, 1, s, e_hat)
    refused(ValueError, "e_hat is written in place and must be contiguous", g.lsd, 0, s, z((B, 2 * n))[:, ::2], marg=d64)
    refused(ValueError, "marg must be torch.float32, got torch.float64", g.lsd, 0, s, e_hat, marg=d64, llr_bin=d64)
    refused(ValueError, "llr_bin must be torch.float32, got torch.float64", g.lsd, 0, s, e_hat, marg=marg, llr_bin=d64, index=marg)
    refused(ValueError, "index must be torch.int32, got torch.int64", g.lsd, 0, s, e_hat, llr_bin=llr_bin, index=z((B,), I64))
    refused(ValueError, "stats must have shape (4, 4), got (4,)", g.lsd, 0, s, e_hat, llr_bin=llr_bin, stats=z((B,), I32))
    refused(ValueError, "stats must be torch.int32, got torch.int64", g.lsd, 0, s, e_hat, llr_bin=llr_bin, stats=z((B, 4), I64))
    refused(ValueError, "stats is written in place and must be contiguous", g.lsd, 0, s, e_hat, llr_bin=llr_bin, stats=z((B, 8), I32)[:, ::2])
    assert rec.calls == []


# ---- the decoder's settings and the two models against a stub graph -----------------------------------------------------------------
def test_lsd_decoder_settings_and_exports():
    assert F.LSD_Decoder is lsd_mod.LSD_Decoder and F.BP4_LSD_Model is lsd_mod.BP4_LSD_Model and F.BP2_LSD_Model is lsd_mod.BP2_LSD_Model
    d = F.LSD_Decoder(N)
    assert (d.n, d.max_pivots, d.max_rounds, d.fallback, d.last_stats) == (N, 0, 0, "osd0", None)
    d = F.LSD_Decoder(N, max_pivots=9, max_rounds=3, fallback=None)
    assert (d.max_pivots, d.max_rounds, d.fallback) == (9, 3, None)
    assert issubclass(F.LSD_Decoder, F.OSD0_Decoder.__mro__[1]) and F.LSD_Decoder.call is F.LSD_Decoder.__call__
    with pytest.raises(ValueError, match="fallback must be one of"):
        F.LSD_Decoder(N, fallback="osd_cs")
    with pytest.raises(ValueError, match="must be >= 0"):
        F.LSD_Decoder(N, max_pivots=-1)
    assert set(G.OSD_METHODS.values()) == {0, 1, 2} and not any("lsd" in k for k in G.OSD_METHODS), "LSD is no OSD method"


class LsdStub(StubGraph):
    """The stub graph with what the LSD models need on top: BP flags `failed`, an `lsd` that reports found = 0 for the samples
    `missed[side]`, a `compact` that really compacts, and recorded `osd0` calls."""

    def __init__(self, failed, missed, B=4):
        super().__init__(B)
        self.failed, self.missed = failed, missed

    def residual(self, *args, **kw):
        self.calls.append(("residual", args, kw))
        flags = z((self.B,))
        flags[self.failed] = 1
        return z((self.B, MZ + MX)), z((self.B, 12)), flags

    def compact(self, mask, bit=1):
        self.calls.append(("compact", (mask.clone(), bit), {}))
        idx = torch.nonzero(mask & bit).flatten().to(I32)
        return torch.cat([idx, z((self.B - len(idx),), I32)]), len(idx)

    def lsd(self, side, synd, e_hat, **kw):
        self.calls.append(("lsd", (side, synd, e_hat), dict(kw)))
        stats = kw["stats"]
        for b in kw["index"][:kw["nact"]].tolist() if kw.get("index") is not None else range(self.B):
            stats[b] = torch.tensor([0 if b in self.missed[side] else 1, 2, 5, 4], dtype=I32)
        return e_hat, stats

    def osd_resident(self, side, method="osd0"):
        return True

    def osd0(self, side, synd, e_hat, **kw):
        self.calls.append(("osd0", (side, synd, e_hat), dict(kw)))
        return e_hat


def _bp4(g):
    return types.SimpleNamespace(graph=g, num_iter=5, cn_type="boxplus", normalization_factor=0.75)


@pytest.mark.parametrize("fallback", ["osd0", None])
def test_bp4_lsd_model_walks_lsd_then_the_fallback(fallback):
    g = LsdStub(failed=[0, 2, 3], missed={0: [2], 1: [2, 3]})
    l = F.LSD_Decoder(N, max_pivots=9, max_rounds=3, fallback=fallback)
    m = F.BP4_LSD_Model(CODE, _bp4(g), l, seed=7)
    assert [c[1][0] for c in g.named("set_basis")] == ([0, 1] if fallback else []), "the bases serve only the fallback"
    if fallback:
        assert all(np.array_equal(c[1][1], piv) for c, piv in zip(g.named("set_basis"), (CODE.pivot_hx, CODE.pivot_hz)))
    g.calls.clear()
    zero, ls_hat = m(4, 0.05)
    names = [c[0] for c in g.calls]
    want = ["pauli_noise", "syndrome", "bp4_decode", "residual", "compact", "lsd", "lsd"]
    assert names == want + (["compact", "osd0", "osd0"] if fallback else []) + ["residual_rows"]
    bp = g.named("bp4_decode")[0]
    sx, sz = bp[1][0], bp[1][1]
    l0, l1 = g.named("lsd")
    assert l0[1][0] == 0 and l0[1][1] is sx and l1[1][0] == 1 and l1[1][1] is sz, "side 0 solves from hx's syndrome, side 1 from hz's"
    z_hat, x_hat = l0[1][2], l1[1][2]
    assert z_hat is not x_hat and shaped(z_hat, (4, N), U8)
    for side, c in enumerate((l0, l1)):
        kw = c[2]
        assert sorted(kw) == ["index", "marg", "max_pivots", "max_rounds", "nact", "stats"]
        assert (kw["nact"], kw["max_pivots"], kw["max_rounds"]) == (3, 9, 3) and kw["index"][:3].tolist() == [0, 2, 3]
        assert shaped(kw["marg"], (4, 3, N), F32) and kw["marg"] is l0[2]["marg"]
        assert kw["stats"].data_ptr() == m.last_stats[side].data_ptr() and shaped(m.last_stats, (2, 4, 4), I32)
    assert m.last_stats[:, 1].tolist() == [[1, 0, 0, 0], [1, 0, 0, 0]], "a sample BP solved reads found, nothing done"
    assert m.last_num_lsd == 3
    if fallback:
        second = g.named("compact")[1]
        assert second[1][0].tolist() == [0, 0, 1, 1] and m.last_num_fallback == 2, "found = 0 on either side"
        o0, o1 = g.named("osd0")
        assert (o0[1][0], o1[1][0]) == (0, 1) and o0[1][1] is sx and o1[1][1] is sz and o0[1][2] is z_hat and o1[1][2] is x_hat
        for c in (o0, o1):
            assert c[2]["nact"] == 2 and c[2]["index"][:2].tolist() == [2, 3] and c[2]["marg"] is l0[2]["marg"]
    else:
        assert m.last_num_fallback == 0
    rr = g.named("residual_rows")[0]
    assert rr[1][4] is x_hat and rr[1][5] is z_hat and shaped(ls_hat, (4, 12), U8) and not zero.any()


def test_bp4_lsd_model_without_failures_or_misses_stops_early():
    g = LsdStub(failed=[], missed={0: [], 1: []})
    m = F.BP4_LSD_Model(CODE, _bp4(g), F.LSD_Decoder(N), seed=7, rank=1, world_size=3)
    m(4, 0.05)
    assert not g.named("lsd") and not g.named("osd0") and len(g.named("compact")) == 1 and (m.last_num_lsd, m.last_num_fallback) == (0, 0)
    assert g.named("pauli_noise")[0][1][2] == 4 and m._next == 12
    g = LsdStub(failed=[1], missed={0: [], 1: []})
    m = F.BP4_LSD_Model(CODE, _bp4(g), F.LSD_Decoder(N), seed=7)
    m(4, 0.05)
    assert len(g.named("lsd")) == 2 and len(g.named("compact")) == 2 and not g.named("osd0") and (m.last_num_lsd, m.last_num_fallback) == (1, 0)


@pytest.mark.parametrize("fallback", ["osd0", None])
def test_bp2_lsd_model_walks_lsd_then_the_fallback(monkeypatch, fallback):
    g = LsdStub(failed=[1, 3], missed={0: [3]})
    monkeypatch.setattr(decoding, "_binary_graph", lambda pcm, logical_pcm, device: g)
    bp2 = F.LDPCBPDecoder(CODE.hx, cn_type="minsum", num_iter=5, normalization_factor=0.75, is_syndrome=True, graph=g)
    m = F.BP2_LSD_Model(CODE.hx, CODE.lx, bp2, F.LSD_Decoder(N, max_rounds=6, fallback=fallback), seed=7)
    basis = g.named("set_basis")
    assert len(basis) == (1 if fallback else 0) and (not fallback or (basis[0][1][0] == 0 and basis[0][1][1].tolist() == list(range(MX))))
    g.calls.clear()
    zero, ls_hat = m(4, 0.05)
    names = [c[0] for c in g.calls]
    assert names == ["bsc_noise", "syndrome", "bp2_decode", "residual", "compact", "lsd"] + (["compact", "osd0"] if fallback else []) + ["residual"]
    c = g.named("lsd")[0]
    assert c[1][0] == 0 and sorted(c[2]) == ["index", "llr_bin", "max_pivots", "max_rounds", "nact", "stats"]
    assert (c[2]["nact"], c[2]["max_pivots"], c[2]["max_rounds"]) == (2, 0, 6) and c[2]["index"][:2].tolist() == [1, 3]
    assert shaped(c[2]["llr_bin"], (4, N), F32) and c[2]["llr_bin"].is_contiguous()
    assert m.last_num_lsd == 2 and m.last_num_fallback == (1 if fallback else 0)
    if fallback:
        o = g.named("osd0")[0]
        assert o[1][0] == 0 and o[1][2] is c[1][2] and o[2]["nact"] == 1 and o[2]["index"][:1].tolist() == [3] and o[2]["llr_bin"] is c[2]["llr_bin"]
    assert shaped(ls_hat, (4, 5), U8) and not zero.any()
