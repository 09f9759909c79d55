"""The Python layer in front of MBP4 in the serial schedule, on the CPU and without the library (the recorder and the stub graph of
tests/test_python_frontend_cpu.py): what `TannerGraph.mbp4_decode_serial`, `set_qubit_layers` and `qubit_layers` hand to their C
entry points and allocate, what they refuse, what `AMBP4Decoder` and `BP4_AMBP_Model` forward under either schedule — and that a
flooding decoder makes exactly the calls it made before the schedule existed."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from feedback_gnn_amd._lib import CN_TYPES
from test_python_frontend_cpu import (B, CODE, F32, GIVEN, I32, MX, MZ, N, U8, XZS, StubGraph, _quaternary_inputs, _tables, assert_call,  # noqa: F401
                                      depolarizing_expr, lib_graph, m_x, m_z, n, p, refused, run, shaped, synd, z)


# ---- TannerGraph against the recording library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("method,symbol", [("mbp4_decode", "fgnn_mbp4_decode"), ("mbp4_decode_serial", "fgnn_mbp4_decode_serial")])
def test_mbp4_decode_and_serial(lib_graph, given, restart, method, symbol):
    g, rec = lib_graph
    sx, sz, llr_ch, Bk = _quaternary_inputs(given)
    factors, owns = _tables()
    (xh, zh, stats), name, a, allocs = run(g, rec, getattr(g, method), sx, sz, factors, owns, 7, 8, "boxplus", restart=restart,
                                           llr_ch=llr_ch, llr_const=1.5, B=Bk)
    assert name == symbol
    assert a == [None, CN_TYPES["boxplus"], 3, factors.ctypes.data, owns.ctypes.data, 7, 8, int(restart), p(llr_ch), 1.5, p(sx), p(sz), B,
                 p(xh), p(zh), p(stats), None]
    assert allocs == XZS and shaped(xh, (B, n), U8) and shaped(zh, (B, n), U8) and shaped(stats, (B, 4), I32)


def test_mbp4_decode_serial_defaults_and_refusals(lib_graph):
    g, rec = lib_graph
    sx, sz = synd()
    _, _, a, _ = run(g, rec, g.mbp4_decode_serial, sx, sz, [1.0], [1.0], 7, 8)
    assert a[1] == CN_TYPES["minsum"] and a[7] == 1 and a[8:10] == [None, 0.0]
    rec.calls.clear()
    refused(ValueError, "Unknown node type.", g.mbp4_decode_serial, sx, sz, [1.0, 2.0], [1.0], 7, 8, cn_type="sum-product")  # first
    refused(ValueError, "factors and owns must have the same length", g.mbp4_decode_serial, sx, sz, [1.0, 2.0], [1.0], 7, 8)
    refused(ValueError, "synd_x must have shape (5, 3), got (4, 3)", g.mbp4_decode_serial, sx, sz, [1.0], [1.0], 7, 8,
            llr_ch=z((5, 3, n), F32))
    refused(ValueError, "synd_x must be torch.uint8, got torch.float32", g.mbp4_decode_serial, z((B, m_x), F32), sz, [1.0], [1.0], 7, 8)
    with pytest.raises(ValueError, match="B is needed"):
        g.mbp4_decode_serial(None, None, [1.0], [1.0], 7, 8)
    assert rec.calls == []


def test_qubit_layer_wrappers(lib_graph):
    g, rec = lib_graph
    g.set_qubit_layers()
    assert rec.calls == [("fgnn_graph_set_qubit_layers", (None, 0, None))]
    rec.calls.clear()
    g.set_qubit_layers([2, 0, 1, 1, 0, 2])
    (name, args), = rec.calls
    assert name == "fgnn_graph_set_qubit_layers" and args[:2] == (None, 3)
    rec.calls.clear()
    refused(ValueError, "layer_of must have shape (6,), got (5,)", g.set_qubit_layers, np.zeros(m_x + m_z, np.int32))
    assert rec.calls == []
    assert g.qubit_layers() == (0, None)  # the recorder leaves the count at zero
    assert [c[0] for c in rec.calls] == ["fgnn_graph_qubit_layers"]


# ---- AMBP4Decoder and BP4_AMBP_Model against the stub graph ------------------------------------------------------------------------------
class SerialStub(StubGraph):
    """The stub graph with what a serial decoder asks of it: a qubit layering to read and install, and the serial decode."""

    def __init__(self, B=3, layering=(0, None)):
        super().__init__(B)
        self.layering = layering

    def qubit_layers(self):
        self.calls.append(("qubit_layers", (), {}))
        return self.layering

    def set_qubit_layers(self, layer_of=None):
        self.calls.append(("set_qubit_layers", (layer_of,), {}))

    def mbp4_decode_serial(self, *args, **kw):
        self.calls.append(("mbp4_decode_serial", args, kw))
        return z((self.B, N)), z((self.B, N)), z((self.B, 4), I32)


def _decoder(g, **kw):
    return F.AMBP4Decoder(CODE, alphas=(1.0, 0.5), num_iter=5, cn_type="boxplus", factor=0.75, restart=False, graph=g, **kw)


def test_decoder_schedule_and_refusals():
    g = SerialStub()
    d = _decoder(g)
    assert d.schedule == "flooding" and g.calls == []  # a flooding decoder asks nothing of the graph
    for bad in ("layered", "Serial", None, 1):
        refused(ValueError, f"schedule must be 'flooding' or 'serial', got {bad!r}", _decoder, g, schedule=bad)
    refused(ValueError, "layers= belongs to schedule='serial'", _decoder, g, layers=np.zeros(N, np.int32))
    assert g.calls == []
    d = _decoder(g, schedule="serial")
    assert d.schedule == "serial"
    assert [c[0] for c in g.calls] == ["qubit_layers", "set_qubit_layers"] and g.calls[1][1] == (None,)  # no layering yet: the greedy one
    own = np.arange(N, dtype=np.int32)
    g = SerialStub(layering=(4, np.zeros(N, np.int32)))
    _decoder(g, schedule="serial")
    assert [c[0] for c in g.calls] == ["qubit_layers"]  # a shared graph keeps the layering it has
    g.calls.clear()
    _decoder(g, schedule="serial", layers=own)
    assert [c[0] for c in g.calls] == ["set_qubit_layers"] and g.calls[0][1][0] is own


@pytest.mark.parametrize("schedule", ["flooding", "serial"])
def test_decoder_forwards_to_the_graph(schedule):
    g = SerialStub(B=3, layering=(4, np.zeros(N, np.int32)))
    d = _decoder(g, **({} if schedule == "flooding" else dict(schedule="serial")))
    method = "mbp4_decode" if schedule == "flooding" else "mbp4_decode_serial"
    g.calls.clear()
    llr = torch.arange(3 * 3 * N, dtype=F32).reshape(3, 3, N)
    x_hat, z_hat = d((llr, torch.ones((MX, 3), dtype=torch.int64), torch.zeros((MZ, 3), dtype=torch.int64)))
    assert shaped(x_hat, (3, N), torch.int64) and shaped(z_hat, (3, N), torch.float64) and len(g.calls) == 1
    assert_call(g.calls[0], method, (torch.ones((3, MX), dtype=U8), z((3, MZ)), d.factors, d.owns, 5, 5, "boxplus"),
                dict(restart=False, llr_ch=llr, llr_const=0.0))
    assert shaped(d.last_stats, (3, 4), I32) and shaped(d.last_alpha, (3,), F32)
    g.calls.clear()
    sx, sz = z((3, MX)), z((3, MZ))
    xh, zh, stats = d.decode(sx, sz, llr_const=-1.5, first_sample=9, seed=4)
    assert len(g.calls) == 1 and stats is d.last_stats
    assert_call(g.calls[0], method, (sx, sz, d.factors, d.owns, 5, 5, "boxplus"), dict(restart=False, llr_ch=None, llr_const=-1.5))


@pytest.mark.parametrize("schedule", ["flooding", "serial"])
def test_model_follows_its_decoders_schedule(schedule):
    g = SerialStub(B=4, layering=(4, np.zeros(N, np.int32)))
    d = _decoder(g, **({} if schedule == "flooding" else dict(schedule="serial")))
    m = F.BP4_AMBP_Model(CODE, d, seed=7)
    g.calls.clear()
    m(4, 0.05)
    used, other = ("mbp4_decode", "mbp4_decode_serial") if schedule == "flooding" else ("mbp4_decode_serial", "mbp4_decode")
    assert not g.named(other) and not g.named("set_qubit_layers")
    if schedule == "flooding":
        assert not g.named("qubit_layers")
    (call,) = g.named(used)
    assert_call(call, used, (z((4, MX)), z((4, MZ)), d.factors, d.owns, 5, 5, "boxplus"),
                dict(restart=False, llr_ch=None, llr_const=depolarizing_expr(0.05)))
    assert m.last_stats is d.last_stats and m.last_alpha is d.last_alpha
