"""The Python layer in front of the layered binary decoder, on the CPU and without the library (the recorder and the stub graph of
tests/test_python_frontend_cpu.py): what `TannerGraph.bp2_decode_layered`, `set_bit_layers` and `bit_layers` hand to their C entry
points and allocate, what they refuse, what `LDPCBPDecoder` and the three binary models forward under either schedule — and that a
flooding decoder makes exactly the calls it made before the schedule existed."""
import types

import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd._lib import CN_TYPES
from test_python_frontend_cpu import (B, CODE, F32, I32, MX, N, U8, StubGraph, assert_call, bsc_expr, lib_graph, m_x, m_z, n, p,  # noqa: F401
                                      refused, run, shaped, z)


# ---- TannerGraph against the recording library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", ["synd", "llr", "both", "llr+B", "B"])
@pytest.mark.parametrize("want_soft,want_hard,stop,want_stats", [(True, True, False, False), (False, True, True, True),
                                                                 (True, False, True, False), (False, False, False, True)])
def test_bp2_decode_layered(lib_graph, given, want_soft, want_hard, stop, want_stats):
    g, rec = lib_graph
    s = z((B, m_x)) if given in ("synd", "both") else None
    llr_ch = z((B, n), F32) if given in ("llr", "both", "llr+B") else None
    Bk = B if given in ("llr+B", "B") else None
    out, name, a, allocs = run(g, rec, g.bp2_decode_layered, s, 5, "boxplus", 0.5, llr_ch=llr_ch, llr_const=1.5, B=Bk, want_soft=want_soft,
                               want_hard=want_hard, stop=stop, want_stats=want_stats)
    assert len(out) == (3 if want_stats else 2)
    soft, hard, stats = out if want_stats else out + (None,)
    assert name == "fgnn_bp2_decode_layered"
    assert a == [None, CN_TYPES["boxplus"], 5, 0.5, p(llr_ch), 1.5, p(s), B, int(stop), p(soft), p(hard), p(stats), None]
    assert allocs == [((B, n), F32)] * want_soft + [((B, n), U8)] * want_hard + [((B, 2), I32)] * want_stats
    assert (soft is None) != want_soft and (hard is None) != want_hard and (stats is None) != want_stats
    assert soft is None or shaped(soft, (B, n), F32)
    assert hard is None or shaped(hard, (B, n), U8)
    assert stats is None or shaped(stats, (B, 2), I32)


def test_bp2_decode_layered_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    s = z((B, m_x))
    (soft, hard), _, a, allocs = run(g, rec, g.bp2_decode_layered, s, 5)
    assert a[1:4] == [CN_TYPES["boxplus-phi"], 5, 1.0] and a[4:6] == [None, 0.0] and a[8] == 0 and a[11] is None
    assert allocs == [((B, n), F32), ((B, n), U8)]
    rec.calls.clear()
    f = z((B, m_x), F32)
    refused(ValueError, "Unknown node type.", g.bp2_decode_layered, f, 5, "boxminus")  # before the syndrome
    refused(ValueError, "syndrome must be torch.uint8, got torch.float32", g.bp2_decode_layered, f, 5, llr_ch=z((B, n)))
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.bp2_decode_layered, z((B, m_z)), 5)
    refused(ValueError, "llr_ch must be torch.float32, got torch.uint8", g.bp2_decode_layered, s, 5, llr_ch=z((B, n)))
    refused(ValueError, "llr_ch must have shape (4, 6), got (5, 6)", g.bp2_decode_layered, s, 5, llr_ch=z((5, n), F32))
    refused(ValueError, "llr_ch must have shape (5, 6), got (4, 6)", g.bp2_decode_layered, None, 5, llr_ch=z((B, n), F32), B=5)
    assert rec.calls == []


def test_bit_layer_wrappers(lib_graph):
    g, rec = lib_graph
    g.set_bit_layers()
    assert rec.calls == [("fgnn_graph_set_bit_layers", (None, 0, None))]
    rec.calls.clear()
    g.set_bit_layers([2, 0, 1])
    (name, args), = rec.calls
    assert name == "fgnn_graph_set_bit_layers" and args[:2] == (None, 3)
    rec.calls.clear()
    refused(ValueError, "layer_of must have shape (3,), got (5,)", g.set_bit_layers, np.zeros(m_x + m_z, np.int32))
    assert rec.calls == []
    assert g.bit_layers() == (0, None)  # the recorder leaves the count at zero
    assert [c[0] for c in rec.calls] == ["fgnn_graph_bit_layers"]


# ---- LDPCBPDecoder and the models against the stub graph -----------------------------------------------------------------------------
class LayeredStub(StubGraph):
    """The stub graph with what a layered decoder asks of it: a layering to read and install, and the layered decode."""

    def __init__(self, B=4, layering=(0, None)):
        super().__init__(B)
        self.layering = layering

    def bit_layers(self):
        self.calls.append(("bit_layers", (), {}))
        return self.layering

    def set_bit_layers(self, layer_of=None):
        self.calls.append(("set_bit_layers", (layer_of,), {}))

    def bp2_decode_layered(self, *args, **kw):
        self.calls.append(("bp2_decode_layered", args, kw))
        out = (z((self.B, N), F32), z((self.B, N)))
        return out + (z((self.B, 2), I32),) if kw.get("want_stats") else out


def _decoder(g, **kw):
    return F.LDPCBPDecoder(CODE.hx, cn_type="minsum", num_iter=5, normalization_factor=0.75, is_syndrome=True, graph=g, **kw)


def test_decoder_schedule_and_refusals():
    g = LayeredStub()
    d = _decoder(g)
    assert d.schedule == "flooding" and d.stop_early is False and g.calls == []  # a flooding decoder asks nothing of the graph
    for bad in ("serial", "Layered", None, 1):
        refused(ValueError, f"schedule must be 'flooding' or 'layered', got {bad!r}", _decoder, g, schedule=bad)
    refused(ValueError, "layers= belongs to schedule='layered'", _decoder, g, layers=np.zeros(MX, np.int32))
    refused(ValueError, "stop_early=True belongs to schedule='layered'", _decoder, g, stop_early=True)
    assert g.calls == []
    d = _decoder(g, schedule="layered", stop_early=True)
    assert d.schedule == "layered" and d.stop_early is True
    assert [c[0] for c in g.calls] == ["bit_layers", "set_bit_layers"] and g.calls[1][1] == (None,)  # no layering yet: the greedy one
    own = np.arange(MX, dtype=np.int32)
    g = LayeredStub(layering=(4, np.zeros(MX, np.int32)))
    _decoder(g, schedule="layered")
    assert [c[0] for c in g.calls] == ["bit_layers"]  # a shared graph keeps the layering it has
    g.calls.clear()
    _decoder(g, schedule="layered", layers=own)
    assert [c[0] for c in g.calls] == ["set_bit_layers"] and g.calls[0][1][0] is own


@pytest.mark.parametrize("schedule", ["flooding", "layered"])
@pytest.mark.parametrize("hard_out", [True, False])
def test_decoder_call_forwards_to_the_graph(schedule, hard_out):
    g = LayeredStub(B=3, layering=(4, np.zeros(MX, np.int32)))
    layered = schedule == "layered"
    d = F.LDPCBPDecoder(CODE.hx, cn_type="minsum", num_iter=5, normalization_factor=0.75, is_syndrome=True, graph=g, hard_out=hard_out,
                        **(dict(schedule="layered", stop_early=True) if layered else {}))
    g.calls.clear()
    llr = torch.arange(3 * N, dtype=F32).reshape(3, N)
    s = torch.ones((MX, 3), dtype=torch.int64)
    out = d((llr, s))
    assert shaped(out, (3, N), F32) and len(g.calls) == 1
    want = dict(llr_ch=llr, want_soft=not hard_out, want_hard=hard_out)
    if layered:
        want["stop"] = True
    assert_call(g.calls[0], "bp2_decode_layered" if layered else "bp2_decode", (torch.ones((3, MX), dtype=U8), 5, "minsum", 0.75), want)


MODELS = {
    "BP_BSC_Model": (lambda d, **kw: F.BP_BSC_Model(CODE.hx, d, CODE.lx, **kw), dict(want_soft=False)),
    "BP2_OSD_Model": (lambda d, **kw: F.BP2_OSD_Model(CODE.hx, CODE.hx, np.arange(3), CODE.lx, d, None, **kw), {}),
    "BP2_LSD_Model": (lambda d, **kw: F.BP2_LSD_Model(CODE.hx, CODE.lx, d, types.SimpleNamespace(fallback=None, max_pivots=0, max_rounds=0),
                                                      **kw), {}),
}


@pytest.fixture
def layered_stub(monkeypatch):
    from feedback_gnn_amd import decoding
    g = LayeredStub(B=4, layering=(4, np.arange(MX, dtype=np.int32) % 4))
    monkeypatch.setattr(decoding, "_binary_graph", lambda pcm, logical_pcm, device: g)
    return g


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_dispatch_on_the_schedule(layered_stub, name):
    g = layered_stub
    build, extra = MODELS[name]
    # flooding: the calls of today, and nothing asked about layers
    m = build(_decoder(g), seed=7)
    g.calls.clear()
    m(4, 0.05)
    assert not g.named("bp2_decode_layered") and not g.named("bit_layers") and not g.named("set_bit_layers")
    (call,) = g.named("bp2_decode")
    assert_call(call, "bp2_decode", (z((4, MX)), 5, "minsum", 0.75), dict(extra, llr_const=bsc_expr(0.05), B=4))
    # layered: the model's graph takes the layering of the decoder's graph, and the decode is the layered one with the decoder's stop
    for stop in (False, True):
        g.calls.clear()
        d = _decoder(g, schedule="layered", stop_early=stop)
        m = build(d, seed=7)
        installs = g.named("set_bit_layers")
        assert len(installs) == 1 and installs[0][1][0] is g.layering[1]
        g.calls.clear()
        m(4, 0.05)
        assert not g.named("bp2_decode")
        (call,) = g.named("bp2_decode_layered")
        assert_call(call, "bp2_decode_layered", (z((4, MX)), 5, "minsum", 0.75), dict(extra, llr_const=bsc_expr(0.05), B=4, stop=stop))
