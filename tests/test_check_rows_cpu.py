"""The per-check row tables of a check-regular graph against the parity-check matrices, without a GPU.

fgnn_graph_create hands three kernels a check's edges ready-made: `cslot32` (the byte offsets 4 * slot of its message slots as 32-bit
values, the address operand of the BP4 check phase) and `cvn16` (its qubits, read by the syndrome kernel and the fused flag test).
fgnn_check_rows forms both on the host with the code the upload runs; here NumPy forms them from hx and hz alone: messages are laid
out hx edges first, then hz edges, each block sorted by (qubit, check); the combined checks are hx's rows, then hz's; a row lists its
edges in ascending qubit order and is padded with zeros to eight entries."""
import ctypes as C

import numpy as np
import pytest

from feedback_gnn_amd import _lib
from helpers import code


def _tables(hx, hz):
    hx, hz = np.asarray(hx) != 0, np.asarray(hz) != 0
    n, mx, mz = hx.shape[1], hx.shape[0], hz.shape[0]
    slot = np.zeros((mx + mz, 8), np.uint32)
    qub = np.zeros((mx + mz, 8), np.uint16)
    base = 0
    for h, row0 in ((hx, 0), (hz, mx)):
        v, c = np.nonzero(h.T)  # sorted by (qubit, check): edge e of this side is message slot base + e
        for r in range(h.shape[0]):
            e = np.nonzero(c == r)[0]  # ascending e = ascending qubit
            slot[row0 + r, :len(e)] = 4 * (base + e)
            qub[row0 + r, :len(e)] = v[e]
        base += len(v)
    return slot, qub


def _library(hx, hz):
    hx, hz = np.asarray(hx), np.asarray(hz)
    edges = []
    for h in (hx, hz):
        r, c = np.nonzero(h)
        edges.append((np.ascontiguousarray(r, np.int32), np.ascontiguousarray(c, np.int32)))
    m = hx.shape[0] + hz.shape[0]
    have = (C.c_int32 * 2)()
    slot = np.full((m, 8), 0xDEADBEEF, np.uint32)
    qub = np.full((m, 8), 0xBEEF, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    (rx, cx), (rz, cz) = edges
    _lib.check(_lib.lib().fgnn_check_rows(hx.shape[1], hx.shape[0], hz.shape[0], len(rx), p(rx), p(cx), len(rz), p(rz), p(cz), have,
                                          p(slot), p(qub)))
    return list(have), slot, qub


@pytest.mark.parametrize("name,dc", [("ghp882", 6), ("ghp1270", 6), ("hp_c7", 6), ("gb48", 8)])
def test_rows_equal_a_numpy_construction(name, dc):
    c = code(name)
    deg = np.concatenate([np.asarray(c.hx).sum(1), np.asarray(c.hz).sum(1)])
    assert (deg == dc).all(), "the zoo's code is no longer check-regular: pick another"
    have, slot, qub = _library(c.hx, c.hz)
    want_slot, want_qub = _tables(c.hx, c.hz)
    assert have[1] == 1 and qub.tobytes() == want_qub.tobytes()
    # qubits of one degree per side (all four codes): the offsets exist as well
    regular = all(len(set(np.asarray(h).sum(0).tolist())) == 1 for h in (c.hx, c.hz))
    assert have[0] == int(regular)
    if regular:
        assert slot.tobytes() == want_slot.tobytes()
        assert slot.max() < 4 * (int(np.asarray(c.hx).sum()) + int(np.asarray(c.hz).sum())) and (slot % 4 == 0).all()


def test_an_irregular_graph_carries_no_rows():
    c = code("rsurf3")  # checks of degree 2 and 4
    have, slot, qub = _library(c.hx, c.hz)
    assert have == [0, 0]
    assert (slot == 0xDEADBEEF).all() and (qub == 0xBEEF).all()  # nothing is written for a table the graph does not carry
