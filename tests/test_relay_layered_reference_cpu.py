"""Relay-BP with layered legs: the NumPy float32 restatement tests/relay_layered_reference.py, tied to the layered binary BP restatement
and checked for the properties the algorithm promises; and the build surface of the feature (header, library export, wrapper).  CPU only.

Anchor.  With gamma = 0, one leg and pre_iter = 1 the memory term is Lam = 1 * L + 0 * L = L and the posterior starts as P = L + 0.0f,
which is what bp2_layered_reference starts from: one layered min-sum iteration gives the same decisions bit for bit.  From the second
iteration on the two associate the same sum differently (include/fgnn.h says so), so the anchor is held at one iteration only."""
import ctypes
import os
import re

import numpy as np
import pytest

import bp2_layered_reference as BR
import relay_layered_reference as RL
import relay_reference as R
from helpers import code
from test_bp2_reference_cpu import _channel, _llr_const
from test_gpu_bp2_shapes import irregular
from test_relay_reference_cpu import mixed_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _hx(name):
    if name == "irr_8":
        return np.asarray(irregular(9, 60, 30, 8)().hx)
    return np.asarray(code(name).hx)


def _noise(hx, B, p, seed):
    e = (np.random.RandomState(seed).rand(B, hx.shape[1]) < p).astype(np.int64)
    return e, (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "irr_8", "ghp882"])
def test_anchor_gamma_zero_one_iteration_is_layered_minsum(name):
    hx = _hx(name)
    B, n = 32, hx.shape[1]
    _, synd = _noise(hx, B, 0.03, 11)
    gamma = np.zeros((1, n), F32)
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=_llr_const(0.03)), dict(llr_ch=-np.abs(_channel(B, n, 3)))):
            hard, stats, _ = RL.relay_layered_decode(hx, synd, gamma, 1, 1, 1, factor, **llr)
            _, h0, s0 = BR.bp2_layered_decode(hx, synd, 1, "minsum", factor, stop=True, **llr)
            assert hard.tobytes() == h0.tobytes(), factor
            assert np.array_equal(stats[:, 0], s0[:, 0]) and (stats[:, 2] == 0).all() and (stats[:, 3] == 1).all()


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "irr_8"])
@pytest.mark.parametrize("stop", [1, 3])
def test_structure(name, stop):
    """stop_nconv = 3 lists the solutions in the order met, at most one per leg, and keeps the first of the lightest."""
    hx = _hx(name)
    n = hx.shape[1]
    B, legs = 40, 5
    _, synd = _noise(hx, B, 0.08, 9)
    llr = _channel(B, n, 5)
    hard, stats, sols = RL.relay_layered_decode(hx, synd, mixed_gamma(legs, n, 1), 8, 6, stop, 0.8, llr_ch=llr)
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
            assert [s[1] for s in sols[b]] == sorted(set(s[1] for s in sols[b])), "at most one solution per leg, in the order met"
            assert all(1 <= s[2] <= (8 if s[1] == 0 else 6) for s in sols[b])
        else:
            assert (stats[b, 2], stats[b, 3]) == (legs - 1, 6)
    if stop == 3:
        assert max(len(s) for s in sols) >= 2, "some sample must meet more than one solution"


def test_a_callers_layering_differs_from_the_greedy_one():
    hx = _hx("gb48")
    m, n = hx.shape
    reverse = np.arange(m - 1, -1, -1).astype(np.int32)  # one check per layer, the last check first
    assert BR.is_valid_bit_layering(hx, m, reverse) and BR.greedy_bit_layers(hx)[0] < m
    _, synd = _noise(hx, 37, 0.08, 4)
    args = (hx, synd, mixed_gamma(3, n, 2), 3, 2, 1, 0.8)
    mine = RL.relay_layered_decode(*args, llr_const=_llr_const(0.08), layer_of=reverse)
    greedy = RL.relay_layered_decode(*args, llr_const=_llr_const(0.08))
    assert (mine[0] != greedy[0]).any(1).any() or (mine[1] != greedy[1]).any(1).any(), "the layering must matter on some sample"
    for out, lay in ((mine, reverse), (greedy, BR.greedy_bit_layers(hx)[1])):
        again = RL.relay_layered_decode(*args, llr_const=_llr_const(0.08), layer_of=lay)
        assert again[0].tobytes() == out[0].tobytes() and again[1].tobytes() == out[1].tobytes() and again[2] == out[2]


def test_layered_legs_solve_what_flooding_legs_leave_on_ghp882():
    """hx of [[882,24]], BSC p = 0.0467, factor 1.0, gamma0 = 0.125 and rows of default_rng(0).uniform(-0.24, 0.66), B = 100, the schedule
    (16, 4 x 12): the flooding restatement leaves 23 samples unsolved, the layered one none, and no solved sample is a logical error."""
    c = code("ghp882")
    hx = np.asarray(c.hx)
    n, p, B = hx.shape[1], 0.0467, 100
    gamma = np.empty((5, n), F32)
    gamma[0] = F32(0.125)
    gamma[1:] = np.random.default_rng(0).uniform(-0.24, 0.66, size=(4, n)).astype(F32)
    e = (np.random.RandomState(7).rand(B, n) < p).astype(np.int64)
    synd = (e @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    llr = float(np.log(p / (1 - p)))
    _, sf, _ = R.relay_decode(hx, synd, gamma, 16, 12, 1, 1.0, llr_const=llr)
    hl, sl, _ = RL.relay_layered_decode(hx, synd, gamma, 16, 12, 1, 1.0, llr_const=llr)
    flooding, layered = int((sf[:, 0] == 0).sum()), int((sl[:, 0] == 0).sum())
    print("unsolved: flooding", flooding, "layered", layered, "mean iterations layered", float(_iterations(sl, 16, 12).mean()))
    assert (flooding, layered) == (23, 0) and layered < flooding
    solved = sl[:, 0] > 0
    res = (e ^ hl)[solved]
    assert not (res @ hx.T.astype(np.int64) % 2).any()
    assert not (res @ np.asarray(c.hz_perp, np.int64).T % 2).any(), "a solved sample is a logical error"


def _iterations(stats, pre, leg):
    """Iterations a sample ran up to its output: the legs before it in full, then k."""
    return np.where(stats[:, 2] == 0, stats[:, 3], pre + (stats[:, 2] - 1) * leg + stats[:, 3])


def test_header_declares_and_library_exports_relay_decode_layered():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_relay_decode_layered\s*\(", text)
    assert "fgnn_relay_decode_layered" in _lib.ABI_SYMBOLS
    assert _lib._SIGNATURES["fgnn_relay_decode_layered"] == _lib._SIGNATURES["fgnn_relay_decode"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_relay_decode_layered")


def test_public_surface():
    import inspect
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert inspect.signature(TannerGraph.relay_decode_layered) == inspect.signature(TannerGraph.relay_decode)
    params = inspect.signature(F.RelayBPDecoder.__init__).parameters
    assert params["schedule"].default == "flooding" and params["layers"].default is None
