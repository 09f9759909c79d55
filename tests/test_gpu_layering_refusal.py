"""A refused layering leaves the installed one decoding: the three kinds of layering (checks, bits, qubits) share one record, one
installer and one free in fgnn_graph.hip, so a refusal must leave the device tables of its own kind, and both other kinds, as they were.
The decoders' own files compare them with the CPU restatements; here the same graph decodes twice, around a refusal, to the same bytes."""
import numpy as np
import pytest

import mbp4_reference as MB
from helpers import gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_bp4fb_reference_cpu import depolarizing

pytestmark = pytest.mark.gpu

ITER = 3
KINDS = {
    "checks": ("layers", "set_layers", r"h[xz] check \d+.* and h[xz] check \d+.* of layer 0 share qubit \d+"),
    "bits": ("bit_layers", "set_bit_layers", r"check \d+ and check \d+ of layer 0 share bit \d+"),
    "qubits": ("qubit_layers", "set_qubit_layers", r"qubit \d+ and qubit \d+ of layer 0 share h[xz] check \d+"),
}


def decode(g, kind, sx, sz):
    """Every output array of the kind's decoder as bytes."""
    L = llr_const(0.10)
    if kind == "checks":
        out = g.bp4_decode_layered(to_gpu(sx), to_gpu(sz), ITER, "minsum", 0.8, llr_const=L, return_msgs=True)
        out = [out[k] for k in sorted(out)]
    elif kind == "bits":
        out = g.bp2_decode_layered(to_gpu(sx), ITER, "minsum", 0.8, llr_const=-L, stop=True, want_stats=True)
    else:
        out = g.mbp4_decode_serial(to_gpu(sx), to_gpu(sz), *MB.mbp4_tables((1.0, 0.8), 0.8), ITER, ITER, "minsum", True, llr_const=L)
    return [t.cpu().numpy().tobytes() for t in out]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_refused_layering_leaves_the_device_tables(kind):
    g = gpu_graph("ibm72")
    _, _, sx, sz = depolarizing(oracle_library_forms("ibm72", stage_one=False), 0.10, g.info()["codewords_per_block"] + 3)
    getter, setter, message = KINDS[kind]
    for _, other_setter, _ in KINDS.values():
        getattr(g, other_setter)(None)
    others = {k: getattr(g, v[0])() for k, v in KINDS.items() if k != kind}

    def others_unchanged():
        for k, (num, lay) in others.items():
            num1, lay1 = getattr(g, KINDS[k][0])()
            assert num1 == num > 0 and np.array_equal(lay1, lay), k

    num, greedy = getattr(g, getter)()
    custom = (num - 1 - greedy).astype(np.int32)  # the greedy layers in reverse order
    try:
        getattr(g, setter)(custom)
        others_unchanged()
        first = decode(g, kind, sx, sz)
        with pytest.raises(ValueError, match=message):
            getattr(g, setter)(np.zeros(len(custom), np.int32))
        assert getattr(g, getter)()[0] == num and np.array_equal(getattr(g, getter)()[1], custom)
        others_unchanged()
        assert decode(g, kind, sx, sz) == first
        others_unchanged()
    finally:
        getattr(g, setter)(None)
    assert np.array_equal(getattr(g, getter)()[1], greedy)
