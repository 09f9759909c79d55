"""Relay-BP: the NumPy float32 restatement tests/relay_reference.py, tied to the C oracle and checked for the properties the
algorithm promises; and the build surface of the feature (header, library export, public classes).  CPU only.

Anchor.  With gamma = 0 and one leg the memory term is Lam = 1 * L + 0 * P = L, so a sample that stops after k check updates carries
the hard decisions of plain min-sum BP with num_iter = k: og_bp2_decode, the C oracle the binary BP kernels are held to."""
import ctypes
import os
import re

import numpy as np
import pytest

import relay_reference as R
from helpers import code, oracle_library_forms
from oracle.oracle import OracleGraph
from test_bp2_reference_cpu import _channel, _llr_const, _syndromes
from test_gpu_bp2_shapes import irregular

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _case(name):
    """(oracle graph, hx) of a named code, or of the irregular graph with degree-1 checks and edge-free bits of the bp2 shape tests."""
    if name == "irr_8":
        c = irregular(9, 60, 30, 8)()
        return OracleGraph(c, forms="library-default"), np.asarray(c.hx)
    return oracle_library_forms(name), np.asarray(code(name).hx)


def mixed_gamma(legs, n, seed):
    """Memory strengths in the published interval with 0, negative values and values above 0.5 in every row."""
    g = np.random.RandomState(seed).uniform(-0.24, 0.66, size=(legs, n)).astype(F32)
    g[:, 0], g[:, 1], g[:, 2] = 0.0, -0.2, 0.6
    return g


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "irr_8"])
def test_anchor_gamma_zero_is_plain_minsum(name):
    og, hx = _case(name)
    B, T = 32, 12
    _, synd = _syndromes(og, hx, 0.06, B)
    gamma = np.zeros((1, hx.shape[1]), F32)
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=_llr_const(0.06)), dict(llr_ch=-np.abs(_channel(B, hx.shape[1], 3)))):  # per-bit reliabilities, every prior on "no error"
            hard, stats, _ = R.relay_decode(hx, synd, gamma, T, T, 1, factor, **llr)
            assert (stats[:, 2] == 0).all() and (stats[stats[:, 0] == 0, 3] == T).all()
            ks = sorted(set(stats[:, 3].tolist()))
            assert len(ks) >= 2, "the batch must stop at more than one iteration count"
            for k in ks:
                sel = stats[:, 3] == k
                sub = {key: (v[sel] if key == "llr_ch" else v) for key, v in llr.items()}
                _, h0 = og.bp2_decode(synd[sel], k, "minsum", factor, **sub)
                assert np.array_equal(h0, hard[sel]), (factor, k)


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "irr_8"])
@pytest.mark.parametrize("stop", [1, 3])
def test_structure(name, stop):
    og, hx = _case(name)
    n = hx.shape[1]
    B, legs = 40, 5
    _, synd = _syndromes(og, hx, 0.08, B, first=9)
    llr = _channel(B, n, 5)
    hard, stats, sols = R.relay_decode(hx, synd, mixed_gamma(legs, n, 1), 8, 6, stop, 0.8, llr_ch=llr)
    q = np.rint(F32(1024.0) * (F32(-1.0) * np.clip(llr, -20, 20).astype(F32))).astype(np.int64)
    solved = stats[:, 0] > 0
    assert solved.any()
    assert np.array_equal((hard[solved].astype(np.int64) @ hx.T.astype(np.int64)) % 2, synd[solved])
    assert np.array_equal(stats[:, 1], (hard.astype(np.int64) * q).sum(1))
    assert (stats[:, 0] <= stop).all()
    for b in range(B):
        assert len(sols[b]) == stats[b, 0]
        if sols[b]:
            w, r, k = min(sols[b], key=lambda t: t[0])  # the first of the lightest: a later solution replaces only if lighter
            assert (stats[b, 1], stats[b, 2], stats[b, 3]) == (w, r, k)
            assert [s[1] for s in sols[b]] == sorted(set(s[1] for s in sols[b])), "at most one solution per leg"
        else:
            assert (stats[b, 2], stats[b, 3]) == (legs - 1, 6)
    if stop == 3:
        assert max(len(s) for s in sols) >= 2, "some sample must meet more than one solution"


def test_header_declares_and_library_exports_relay_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_relay_decode\s*\(", text)
    assert "fgnn_relay_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_relay_decode")


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.RelayBPDecoder) and callable(F.BP2_Relay_Model)
    assert callable(TannerGraph.relay_decode)
