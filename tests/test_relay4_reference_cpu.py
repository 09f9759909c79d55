"""Relay-BP4: the restatement tests/relay4_reference.py, tied to the C oracle's BP4 and checked for the properties the algorithm
promises; and the build surface of the feature (header, library export, public classes).  CPU only.

Anchor.  With gamma = 0 and one leg the memory term is Lam = 1 * lam + 0 * M = lam, so a sample that stops after k check updates
carries the decisions of plain min-sum BP4 with num_iter = k: og_bp4_decode, the C oracle the BP4 kernels are held to."""
import ctypes
import os
import re

import numpy as np
import pytest

import relay4_reference as R4
from helpers import code, llr_const, oracle_library_forms
from test_relay_reference_cpu import mixed_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 0x5EED
CODES = ["steane", "rsurf5", "ibm72"]
# depolarizing rates at which a batch of each code holds samples solved at once, solved late and never solved
P_OF = {"steane": 0.15, "rsurf5": 0.15, "ibm72": 0.10}


def depolarizing(og, p, B, first=0):
    """Seeded depolarizing noise (the oracle's Philox stream) and its two syndromes."""
    ex, ez = og.pauli_noise(SEED, p, first, B)
    sx, sz = og.syndrome(ex, ez)
    return ex, ez, sx, sz


class CountingOracle:
    """An OracleGraph that records the batch size of every bp4_decode call."""

    def __init__(self, og):
        self._og, self.calls = og, []

    def __getattr__(self, name):
        return getattr(self._og, name)

    def bp4_decode(self, synd_x, *args, **kw):
        self.calls.append(len(synd_x))
        return self._og.bp4_decode(synd_x, *args, **kw)


@pytest.mark.parametrize("name", CODES)
def test_anchor_gamma_zero_is_plain_minsum_bp4(name):
    og = oracle_library_forms(name, stage_one=False)
    B, T = 32, 12
    _, _, sx, sz = depolarizing(og, P_OF[name], B)
    gamma = np.zeros((1, og.n), F32)
    rng = np.random.RandomState(3)
    per_qubit = rng.uniform(1.0, 6.0, size=(B, 3, og.n)).astype(F32)  # per-qubit reliabilities, every prior on "no error"
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=llr_const(P_OF[name])), dict(llr_ch=per_qubit)):
            xh, zh, stats, _ = R4.relay4_decode(og, sx, sz, gamma, T, T, 1, factor, **llr)
            assert (stats[:, 2] == 0).all() and (stats[stats[:, 0] == 0, 3] == T).all()
            ks = sorted(set(stats[:, 3].tolist()))
            assert len(ks) >= 2, "the batch must stop at more than one iteration count"
            for k in ks:
                sel = stats[:, 3] == k
                sub = {key: (v[sel] if key == "llr_ch" else v) for key, v in llr.items()}
                out = og.bp4_decode(sx[sel], sz[sel], k, "minsum", factor, **sub)
                assert np.array_equal(out["x_hat"], xh[sel]) and np.array_equal(out["z_hat"], zh[sel]), (factor, k)


@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("stop", [1, 3])
def test_structure(name, stop):
    og = oracle_library_forms(name, stage_one=False)
    c = code(name)
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    n, B, legs = og.n, 40, 5
    _, _, sx, sz = depolarizing(og, P_OF[name], B, first=9)
    llr = np.random.RandomState(5).uniform(0.5, 5.0, size=(B, 3, n)).astype(F32)
    xh, zh, stats, sols = R4.relay4_decode(og, sx, sz, mixed_gamma(legs, n, 1), 8, 6, stop, 0.8, llr_ch=llr)
    solved = stats[:, 0] > 0
    assert solved.any()
    assert np.array_equal((xh[solved].astype(np.int64) @ hz.T) % 2, sz[solved])
    assert np.array_equal((zh[solved].astype(np.int64) @ hx.T) % 2, sx[solved])
    # the weight again, one qubit at a time: X -> row 0, Y -> row 1, Z -> row 2 of llr_ch
    for b in range(B):
        w = 0
        for v in range(n):
            row = {(0, 0): None, (1, 0): 0, (1, 1): 1, (0, 1): 2}[(int(xh[b, v]), int(zh[b, v]))]
            if row is not None:
                w += int(np.rint(F32(1024.0) * F32(np.clip(llr[b, row, v], -20, 20))))
        assert stats[b, 1] == w
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


@pytest.mark.parametrize("name", CODES)
def test_legs_after_the_stop_are_not_run(name):
    """One oracle call per BP4 step: a sample that meets its stop_nconv-th solution at (r, k) has cost pre_iter-or-k calls per leg up to
    there and none afterwards, whatever num_legs is."""
    og = CountingOracle(oracle_library_forms(name, stage_one=False))
    n, pre, leg, legs, NB = og.n, 8, 6, 5, 40
    _, _, sx, sz = depolarizing(og, P_OF[name], NB)
    gamma = mixed_gamma(legs, n, 1)
    L = llr_const(P_OF[name])
    seen = set()
    for b in range(NB):
        og.calls.clear()
        _, _, stats, sols = R4.relay4_decode(og, sx[b:b + 1], sz[b:b + 1], gamma, pre, leg, 1, 0.8, llr_const=L)
        found, _, r, k = stats[0]
        if found:
            assert len(og.calls) == (pre + (r - 1) * leg if r > 0 else 0) + k and len(sols[0]) == 1
            seen.add("first leg" if r == 0 else "later leg")
        else:
            assert len(og.calls) == pre + (legs - 1) * leg and (r, k) == (legs - 1, leg)
            seen.add("never")
    assert {"first leg", "later leg"} <= seen, seen
    # a batch costs what its slowest sample costs, and a finished sample leaves the calls
    og.calls.clear()
    _, _, stats, _ = R4.relay4_decode(og, sx, sz, gamma, pre, leg, 1, 0.8, llr_const=L)
    assert og.calls[0] == NB and og.calls[-1] < NB and og.calls == sorted(og.calls, reverse=True)
    assert len(og.calls) == pre + (legs - 1) * leg or (stats[:, 0] > 0).all()


@pytest.mark.parametrize("name", CODES)
def test_zero_syndrome_is_solved_at_once_with_weight_zero(name):
    og = oracle_library_forms(name, stage_one=False)
    B = 5
    sx, sz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    for stop in (1, 3):
        xh, zh, stats, sols = R4.relay4_decode(og, sx, sz, mixed_gamma(3, og.n, 5), 6, 5, stop, 0.8, llr_const=llr_const(0.05))
        assert not xh.any() and not zh.any()
        assert (stats[:, 1:] == np.array([0, 0, 1])).all() and (stats[:, 0] == stop).all()
        assert all(s[0] == (0, 0, 1) for s in sols)


def test_header_declares_and_library_exports_relay4_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_relay4_decode\s*\(", text)
    assert "fgnn_relay4_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_relay4_decode")


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.RelayBP4Decoder) and callable(F.BP4_Relay_Model)
    assert callable(TannerGraph.relay4_decode)
