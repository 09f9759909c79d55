"""The Python layer in front of Relay-BP with layered legs, on the CPU and without the library (the recorder and the stub graph of
tests/test_python_frontend_cpu.py): what `TannerGraph.relay_decode_layered` hands to its C entry point and allocates, what it refuses,
what `RelayBPDecoder` and `BP2_Relay_Model` forward under either schedule — and that a flooding decoder makes exactly the calls it
made before the schedule existed."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd import decoding, relay
from test_python_frontend_bp2_layered_cpu import LayeredStub
from test_python_frontend_cpu import (B, CODE, F32, I32, MX, N, U8, assert_call, bsc_expr, lib_graph, m_x, m_z, n, p,  # noqa: F401
                                      refused, run, shaped, z)


class RelayStub(LayeredStub):
    """The layered stub graph with the layered relay decode."""

    def relay_decode_layered(self, *args, **kw):
        self.calls.append(("relay_decode_layered", args, kw))
        return z((self.B, N)), z((self.B, 4), I32)


# ---- TannerGraph against the recording library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", ["synd", "llr", "both", "llr+B", "B"])
def test_relay_decode_layered(lib_graph, given):
    g, rec = lib_graph
    s = z((B, m_x)) if given in ("synd", "both") else None
    llr_ch = z((B, n), F32) if given in ("llr", "both", "llr+B") else None
    Bk = B if given in ("llr+B", "B") else None
    gamma = z((5, n), F32)
    (hard, stats), name, a, allocs = run(g, rec, g.relay_decode_layered, s, gamma, 7, 8, 3, 0.5, llr_ch=llr_ch, llr_const=1.5, B=Bk)
    assert name == "fgnn_relay_decode_layered"
    assert a == [None, 0.5, 7, 5, 8, 3, p(gamma), p(llr_ch), 1.5, p(s), B, p(hard), p(stats), None]
    assert allocs == [((B, n), U8), ((B, 4), I32)] and shaped(hard, (B, n), U8) and shaped(stats, (B, 4), I32)


def test_relay_decode_layered_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    s, gamma = z((B, m_x)), z((5, n), F32)
    _, _, a, _ = run(g, rec, g.relay_decode_layered, s, gamma, 7, 8, 3)
    assert a[1] == 1.0 and a[7:9] == [None, 0.0]
    rec.calls.clear()
    refused(ValueError, "syndrome must be torch.uint8, got torch.float32", g.relay_decode_layered, z((B, m_x), F32), z((n,), F32), 7, 8, 3)
    refused(ValueError, "syndrome must have shape (4, 3), got (4, 2)", g.relay_decode_layered, z((B, m_z)), gamma, 7, 8, 3)
    refused(ValueError, "llr_ch must have shape (4, 6), got (5, 6)", g.relay_decode_layered, s, gamma, 7, 8, 3, llr_ch=z((5, n), F32))
    refused(ValueError, "llr_ch must have shape (5, 6), got (4, 6)", g.relay_decode_layered, None, gamma, 7, 8, 3, llr_ch=z((B, n), F32), B=5)
    refused(ValueError, "gamma must have shape [num_legs, n]", g.relay_decode_layered, s, z((n,), F32), 7, 8, 3)
    refused(ValueError, "gamma must have shape (5, 6), got (5, 7)", g.relay_decode_layered, s, z((5, 7), F32), 7, 8, 3)
    refused(ValueError, "gamma must be torch.float32, got torch.float64", g.relay_decode_layered, s, z((5, n), torch.float64), 7, 8, 3)
    assert rec.calls == []


def test_the_two_bindings_have_one_signature():
    from feedback_gnn_amd import _lib
    assert _lib._SIGNATURES["fgnn_relay_decode_layered"] == _lib._SIGNATURES["fgnn_relay_decode"]


# ---- RelayBPDecoder and BP2_Relay_Model against the stub graph -----------------------------------------------------------------------
def _decoder(g, **kw):
    return F.RelayBPDecoder(CODE.hx, gamma0=0.25, pre_iter=5, num_sets=2, set_max_iter=3, stop_nconv=4, normalization_factor=0.75, seed=3,
                            graph=g, **kw)


def test_decoder_schedule_and_refusals():
    g = RelayStub()
    d = _decoder(g)
    assert d.schedule == "flooding" and g.calls == []  # a flooding decoder asks nothing of the graph
    for bad in ("serial", "Layered", None, 1):
        refused(ValueError, f"schedule must be 'flooding' or 'layered', got {bad!r}", _decoder, g, schedule=bad)
    refused(ValueError, "layers= belongs to schedule='layered'", _decoder, g, layers=np.zeros(MX, np.int32))
    assert g.calls == []
    d = _decoder(g, schedule="layered")
    assert d.schedule == "layered"
    assert [c[0] for c in g.calls] == ["bit_layers", "set_bit_layers"] and g.calls[1][1] == (None,)  # no layering yet: the greedy one
    own = np.arange(MX, dtype=np.int32)
    g = RelayStub(layering=(4, np.zeros(MX, np.int32)))
    _decoder(g, schedule="layered")
    assert [c[0] for c in g.calls] == ["bit_layers"]  # a shared graph keeps the layering it has
    g.calls.clear()
    _decoder(g, schedule="layered", layers=own)
    assert [c[0] for c in g.calls] == ["set_bit_layers"] and g.calls[0][1][0] is own


@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_decoder_forwards_to_the_graph(schedule):
    g = RelayStub(B=3, layering=(4, np.zeros(MX, np.int32)))
    d = _decoder(g, **({} if schedule == "flooding" else dict(schedule="layered")))
    method = "relay_decode" if schedule == "flooding" else "relay_decode_layered"
    g.calls.clear()
    llr = torch.arange(3 * N, dtype=F32).reshape(3, N)
    out = d((llr, torch.ones((MX, 3), dtype=torch.int64)))
    assert shaped(out, (3, N), F32) and len(g.calls) == 1
    assert_call(g.calls[0], method, (torch.ones((3, MX), dtype=U8), d.gamma, 5, 3, 4, 0.75), dict(llr_ch=llr, llr_const=0.0, B=None))
    assert shaped(d.last_stats, (3, 4), I32)
    g.calls.clear()
    s = z((3, MX))
    hard, stats = d.decode(s, llr_const=-1.5, B=3)
    assert len(g.calls) == 1 and shaped(hard, (3, N), U8) and stats is d.last_stats
    assert_call(g.calls[0], method, (s, d.gamma, 5, 3, 4, 0.75), dict(llr_ch=None, llr_const=-1.5, B=3))


@pytest.fixture
def relay_stub(monkeypatch):
    g = RelayStub(B=4, layering=(4, np.arange(MX, dtype=np.int32) % 4))
    monkeypatch.setattr(decoding, "_binary_graph", lambda pcm, logical_pcm, device: g)
    monkeypatch.setattr(relay, "_binary_graph", lambda pcm, logical_pcm, device: g)
    return g


def test_model_follows_its_decoders_schedule(relay_stub):
    g = relay_stub
    # flooding: the calls of today, and nothing asked about layers
    m = F.BP2_Relay_Model(CODE.hx, CODE.lx, _decoder(g), seed=7)
    assert g.calls == []
    m(4, 0.05)
    assert not g.named("relay_decode_layered") and not g.named("bit_layers") and not g.named("set_bit_layers")
    (call,) = g.named("relay_decode")
    assert_call(call, "relay_decode", (z((4, MX)), m.relay_decoder.gamma, 5, 3, 4, 0.75), dict(llr_const=bsc_expr(0.05), B=4))
    # layered: the model's graph takes the layering of the decoder's graph, and the decode is the layered one
    g.calls.clear()
    d = _decoder(g, schedule="layered")
    m = F.BP2_Relay_Model(CODE.hx, CODE.lx, d, seed=7)
    installs = g.named("set_bit_layers")
    assert len(installs) == 1 and installs[0][1][0] is g.layering[1]
    g.calls.clear()
    m(4, 0.05)
    assert not g.named("relay_decode")
    (call,) = g.named("relay_decode_layered")
    assert_call(call, "relay_decode_layered", (z((4, MX)), d.gamma, 5, 3, 4, 0.75), dict(llr_const=bsc_expr(0.05), B=4))
    assert m.last_stats is d.last_stats and shaped(m.last_stats, (4, 4), I32)
