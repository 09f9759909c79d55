"""BP4 with guided decimation: the restatement tests/bp4gd_reference.py, tied to the C oracle's BP4 and checked for what the algorithm
states; and the build surface of the feature (header, library export, public classes).  CPU only.

Anchor.  With max_rounds = 0 nothing is ever fixed, lamhat stays the channel LLRs, so a sample that stops after k check updates carries
the decisions of plain BP4 with num_iter = k, and no smaller num_iter solves it: og_bp4_decode, the C oracle the BP4 kernels are held to."""
import ctypes
import os
import re

import numpy as np
import pytest

import bp4gd_reference as GD
from helpers import code, llr_const, oracle_library_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 0x5EED
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]


def depolarizing(og, p, B, first=0):
    """Seeded depolarizing noise (the oracle's Philox stream) and its two syndromes."""
    ex, ez = og.pauli_noise(SEED, p, first, B)
    sx, sz = og.syndrome(ex, ez)
    return ex, ez, sx, sz


def solves(c, xh, zh, sx, sz):
    hx, hz = np.asarray(c.hx, np.int64) % 2, np.asarray(c.hz, np.int64) % 2
    return ((xh.astype(np.int64) @ hz.T) % 2 == sz).all(1) & ((zh.astype(np.int64) @ hx.T) % 2 == sx).all(1)


class RecordingOracle:
    """An OracleGraph that keeps the llr_ch of every bp4_decode call of a one-sample batch."""

    def __init__(self, og):
        self._og, self.llr = og, []

    def __getattr__(self, name):
        return getattr(self._og, name)

    def bp4_decode(self, synd_x, *args, **kw):
        assert len(synd_x) == 1
        self.llr.append(np.array(kw["llr_ch"][0], F32))
        return self._og.bp4_decode(synd_x, *args, **kw)


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_no_rounds_is_bp4_stopped_at_its_first_solution(cn_type):
    og, c = oracle_library_forms("ibm72", stage_one=False), code("ibm72")
    B, T, p = 32, 12, 0.10
    _, _, sx, sz = depolarizing(og, p, B)
    per_qubit = np.random.RandomState(3).uniform(1.0, 6.0, size=(B, 3, og.n)).astype(F32)
    for factor in (1.0, 0.8):
        for llr in (dict(llr_const=llr_const(p)), dict(llr_ch=per_qubit)):
            xh, zh, stats, fixed = GD.bp4gd_decode(og, sx, sz, T, 5, 0, 25.0, cn_type, factor, **llr)
            assert (fixed < 0).all() and (stats[:, 1] == 0).all() and (stats[:, 2] == stats[:, 3]).all()
            assert (stats[stats[:, 0] == 0, 3] == T).all()
            assert len(set(stats[:, 3].tolist())) >= 2, "the batch must stop at more than one iteration count"
            first = np.full(B, T)  # the first num_iter at which plain BP4 reproduces both syndromes, T if none does
            hit = np.zeros(B, bool)
            for k in range(1, T + 1):
                out = og.bp4_decode(sx, sz, k, cn_type, factor, **llr)
                ok = solves(c, out["x_hat"], out["z_hat"], sx, sz) & ~hit
                first[ok], hit = k, hit | ok
                sel = stats[:, 3] == k
                assert np.array_equal(out["x_hat"][sel], xh[sel]) and np.array_equal(out["z_hat"][sel], zh[sel]), (factor, k)
            assert np.array_equal(first, stats[:, 3]) and np.array_equal(hit, stats[:, 0] == 1)


def test_a_fixed_qubit_carries_its_lamhat_row():
    """Every BP4 step after a fix sees, at the fixed qubit, exactly (+D,+D,+D) / (-D,+0,+0) / (+0,+0,-D) / (+0,-D,+0) for I / X / Z / Y
    (order X, Y, Z; the sign of the zeros included), and the channel LLRs at every free qubit."""
    og = oracle_library_forms("ibm72", stage_one=False)
    n, pre, rnd, R, D = og.n, 6, 3, 8, 7.5
    ex, ez, sx, sz = depolarizing(og, 0.10, 40)
    # moderate priors on "no error", except that in three samples of four half of the noisy qubits know their Pauli well: those are the clearest decisions of
    # their sample, so qubits get fixed to X, Z and Y too, not to the identity alone
    rng = np.random.RandomState(11)
    lam = rng.uniform(0.5, 5.0, size=(40, 3, n)).astype(F32)
    row = np.where(ex & ez, 1, np.where(ez != 0, 2, 0))  # rows X, Y, Z of llr_ch
    b_, v_ = np.nonzero(((ex | ez) != 0) & (rng.rand(40, n) < 0.5) & (np.arange(40) % 4 != 0)[:, None])  # not in every fourth sample
    lam[b_, row[b_, v_], v_] = -rng.uniform(8.0, 12.0, size=len(b_)).astype(F32)
    table = {0: (D, D, D), 1: (-D, 0.0, 0.0), 2: (0.0, 0.0, -D), 3: (0.0, -D, 0.0)}
    seen = set()
    for b in range(40):
        rec = RecordingOracle(og)
        _, _, stats, fixed = GD.bp4gd_decode(rec, sx[b:b + 1], sz[b:b + 1], pre, rnd, R, D, "minsum", 0.8, llr_ch=lam[b:b + 1])
        found, nfix, its, k = stats[0]
        assert len(rec.llr) == its == (k if nfix == 0 else pre + (nfix - 1) * rnd + k)
        assert (fixed[0] >= 0).sum() == nfix <= R
        assert all(np.array_equal(l, lam[b]) for l in rec.llr[:pre]), "nothing is fixed before the first round ends"
        last = rec.llr[-1]
        for v in range(n):
            if fixed[0, v] < 0:
                assert np.array_equal(last[:, v], lam[b, :, v])
            else:
                want = np.array(table[int(fixed[0, v])], F32)
                assert np.array_equal(last[:, v], want) and np.array_equal(np.signbit(last[:, v]), np.signbit(want))
                seen.add(int(fixed[0, v]))
        # one more qubit differs from the channel in each round, and a fixed qubit stays as it was fixed
        for r in range(1, nfix + 1):
            cur = rec.llr[pre + (r - 1) * rnd]
            assert ((cur != lam[b]).any(0) | (np.signbit(cur) != np.signbit(lam[b])).any(0)).sum() == r
            fx = (cur != lam[b]).any(0)
            assert np.array_equal(cur[:, fx], last[:, fx])
    assert seen == {0, 1, 2, 3}, f"qubits must be fixed to every Pauli and to the identity, got {seen}"


def test_ghp882_figures():
    """[[882,24]], seeded depolarizing samples 0..63 at p = 0.10, min-sum at factor 0.8: flooding BP4-64 leaves 7 unsolved; BP4-GD with
    pre_iter 32, round_iter 4, max_rounds n and D = 25 leaves none, fixes at most 33 qubits, takes at most 164 iterations on any sample
    and makes no logical error."""
    og, c = oracle_library_forms("ghp882", stage_one=False), code("ghp882")
    B, p = 64, 0.10
    ex, ez, sx, sz = depolarizing(og, p, B)
    L = llr_const(p)
    xh, zh, stats, _ = GD.bp4gd_decode(og, sx, sz, 64, 4, 0, 25.0, "minsum", 0.8, llr_const=L)
    assert int((stats[:, 0] == 0).sum()) == 7
    xh, zh, stats, fixed = GD.bp4gd_decode(og, sx, sz, 32, 4, None, 25.0, "minsum", 0.8, llr_const=L)
    print("fixed", stats[:, 1].tolist(), "its", stats[:, 2].tolist())
    assert int((stats[:, 0] == 0).sum()) == 0
    assert solves(c, xh, zh, sx, sz).all()
    assert stats[:, 1].max() <= 33 and stats[:, 2].max() <= 164
    assert np.array_equal((fixed >= 0).sum(1), stats[:, 1])
    xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64) % 2, np.asarray(c.hz_perp, np.int64) % 2
    assert not ((xd @ hxp.T) % 2).any() and not ((zd @ hzp.T) % 2).any(), "no logical error"


def test_header_declares_and_library_exports_bp4gd_decode():
    from feedback_gnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fgnn_bp4gd_decode\s*\(", text)
    assert "fgnn_bp4gd_decode" in _lib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fgnn_bp4gd_decode")


def test_public_classes_import():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import TannerGraph
    assert callable(F.BP4GDDecoder) and callable(F.BP4_GD_Model)
    assert callable(TannerGraph.bp4gd_decode)
