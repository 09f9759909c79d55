"""The C ABI of the OSD path beyond LDS (fgnn_osd_resident, fgnn_osd_workspace_bytes, fgnn_osd_ws) without a GPU: declared, bound, and
its argument checks answered with error codes before any device work.  Also a bit-packed restatement of the elimination (the GPU tests
use it on bases too large for the uint8 one of tests/test_osd_search_cpu.py), held here to that restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feedback_gnn_amd import _lib
from test_osd_search_cpu import eliminate, sortable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fgnn_osd_resident", "fgnn_osd_workspace_bytes", "fgnn_osd_ws")


def eliminate_packed(r, basis, synd):
    """`eliminate` (steps 1-4 of fgnn_osd0) on rows packed into uint64 words, the same return values: (order, r_sorted, reduced
    augmented matrix [rank, n+1] uint8, pivot of every row, real pivot rows)."""
    r = np.asarray(r, dtype=np.float32) + np.float32(0.0)  # -0 -> +0
    order = np.argsort(sortable(r), kind="stable")
    m, n = basis.shape
    W = (n + 1 + 63) // 64
    a = np.zeros((m, W * 64), np.uint8)
    a[:, :n] = basis[:, order]
    a[:, n] = np.asarray(synd, np.uint8) & 1
    P = np.packbits(a, axis=1, bitorder="little").view("<u8").copy()  # column j = bit j & 63 of word j >> 6
    piv = np.zeros(m, np.int64)
    for i in range(m):
        nz = np.flatnonzero(P[i])
        if not len(nz):
            continue  # all-zero row: pivot 0, and XORing it changes nothing
        w = int(nz[0])
        x = int(P[i, w])
        p = w * 64 + (x & -x).bit_length() - 1
        piv[i] = p
        hit = ((P[:, w] >> np.uint64(p & 63)) & np.uint64(1)).astype(bool)
        hit[i] = False
        rows = np.flatnonzero(hit)
        if len(rows):
            P[np.ix_(rows, np.arange(w, W))] ^= P[i, w:]
    out = np.unpackbits(P.view(np.uint8), axis=1, bitorder="little")[:, :n + 1].copy()
    real = np.array([piv[i] < n and out[i, piv[i]] == 1 for i in range(m)], dtype=bool)
    return order, r[order], out, piv, real


@pytest.mark.parametrize("seed", range(6))
def test_packed_elimination_equals_the_restatement(seed):
    rng = np.random.RandomState(seed)
    m, n = [(12, 26), (40, 63), (30, 64), (50, 65), (70, 130), (45, 200)][seed]
    h = (rng.uniform(size=(m, n)) < 0.15).astype(np.uint8)
    if seed % 2:  # rank-deficient: a duplicate row, a sum of two rows, a zero row
        h = np.concatenate([h, h[:1], h[1:2] ^ h[2:3], np.zeros((1, n), np.uint8)])[rng.permutation(m + 3)]
    r = rng.normal(1.0, 2.0, size=n).astype(np.float32)
    r[::4] = np.float32(0.5)
    r[1::9] = np.float32(-0.0)
    synd = (rng.uniform(size=h.shape[0]) < 0.5).astype(np.uint8)
    ref, got = eliminate(r, h, synd), eliminate_packed(r, h, synd)
    for k, (x, y) in enumerate(zip(ref, got)):
        assert np.array_equal(x, y), k


def test_header_declares_and_lib_binds_the_workspace_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and name in _lib._SIGNATURES
    assert "size_t workspace_bytes" in hdr
    assert _lib.lib().fgnn_version() == 2


def _err():
    return _lib.lib().fgnn_last_error().decode()


def _osd_ws(method=2, order=7, workspace=C.c_void_p(64), nbytes=1 << 20):
    e_hat = (C.c_uint8 * 4)()
    synd = (C.c_uint8 * 4)()
    llr = (C.c_float * 4)()
    return _lib.lib().fgnn_osd_ws(None, 0, method, order, None, llr, synd, 1, None, 0, e_hat, None, workspace, nbytes, None)


def test_argument_errors_come_back_as_codes():
    L = _lib.lib()
    fits = C.c_int(-5)
    assert L.fgnn_osd_resident(None, 0, 0, C.byref(fits)) == -1 and "bad OSD arguments" in _err() and fits.value == -5
    assert L.fgnn_osd_resident(None, 0, 9, C.byref(fits)) == -1 and "unknown OSD method" in _err()
    nbytes = C.c_size_t(123)
    assert L.fgnn_osd_workspace_bytes(None, 0, 2, 7, 4, C.byref(nbytes)) == -1 and "bad OSD arguments" in _err()
    assert L.fgnn_osd_workspace_bytes(None, 0, 7, 0, 4, C.byref(nbytes)) == -1 and "unknown OSD method" in _err()
    assert L.fgnn_osd_workspace_bytes(None, 0, 1, 17, 4, C.byref(nbytes)) == -1 and "osd_e supports order <= 16" in _err()
    assert L.fgnn_osd_workspace_bytes(None, 0, 2, 7, 0, C.byref(nbytes)) == -1
    assert nbytes.value == 123
    assert _osd_ws() == -1 and "bad OSD arguments" in _err()  # NULL graph
    assert _osd_ws(method=3) == -1 and "unknown OSD method" in _err()
    assert _osd_ws(method=2, order=65) == -1 and "osd_cs supports order <= 64" in _err()
    assert _osd_ws(method=1, order=17) == -1 and "osd_e supports order <= 16" in _err()
    assert _osd_ws(method=0, order=-1) == -1 and "order must be >= 0" in _err()
    assert _osd_ws(workspace=None) == -1 and "workspace is NULL" in _err()
    assert _osd_ws(workspace=C.c_void_p(68)) == -1 and "8-byte aligned" in _err()
