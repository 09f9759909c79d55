"""bp4_kernel's bounded-argument variant (BND) against the C oracle by exact equality, on both sides of the host's proof.

The NT = 4 / 5 kernels (first decoder, one constant channel LLR, 256 threads per codeword) and the NQ = 4 / 5 kernels (later decoders of
a sandwich, per-qubit LLRs in registers) exist twice: with the range guards of the qubit update's softplus and log-sum-exp, and without
them (fgnn_math_ranged.h: fg_softplus_bounded, fg_lse2_bounded).  plan_bp4 picks the second only if the launch arguments prove every
argument within 80: zero start messages, 3 phi0 |factor| + L_b <= 80 and 3 phi0 |factor| + 2 L_b + 1 <= 80, L_b = |llr_const| or the
bound the feedback GNN's weights give for its output.  The oracle compiles fgnn_math.h with every guard in place, so:
  * bounded side: the outputs must not move by a bit — converged codewords (p = 0.01: saturated messages, log-sum-exp distances of
    20 to 56, where the dropped minimum used to act) and unconverged ones (p = 0.12: distances near 0);
  * fallback side: the guarded kernels must be the ones that run — on these inputs the bounded routines leave fg_exp's domain (a
    softplus argument below -87 returns the exponential's wrapped bits instead of 0), so a wrong pick shows as a mismatch;
  * threshold edges: llr_const one float either side of both inequalities (the first is implied by the second for every L_b >= 0, so
    both of its sides take the guarded kernels).
Marginals, decisions, both soft syndromes and the final messages; B = 3 and 5, 6 and 12 iterations, shortcuts on and off, literal and
shared log-sum-exp."""
import functools

import numpy as np
import pytest

from feedback_gnn_amd.graph import GnnWeights
from feedback_gnn_amd.weights_io import read_weight_list
from helpers import WEIGHTS_882, WEIGHTS_1270, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_gpu_bp4_hot_loops import _eq
from test_gpu_bp4_shapes import graphs

pytestmark = pytest.mark.gpu
F32 = np.float32
PHI0 = 16.6355324
BOUNDED_MAX = 80.0
NT_CODES = ["ghp882", "ghp1270"]          # 4 / 5 qubits and checks per thread at 256 threads per codeword
NQ_CASES = [("gb3_128", 4), ("gb3_150", 5)]  # (3,3,6) codes of tests/test_gpu_bp4_shapes.py: lreg 4 / 5 at launch (64, 1)


def proven(factor, L_b):
    """plan_bp4's test restated (in double, as the host evaluates it) for a zero-start launch."""
    M = 3.0 * PHI0 * abs(float(F32(factor)))
    L_b = abs(float(L_b))
    return bool(np.isfinite(M) and np.isfinite(L_b) and M + L_b <= BOUNDED_MAX and M + 2.0 * L_b + 1.0 <= BOUNDED_MAX)


def pair(name):
    """(GPU graph, oracle graph) of a named code or of a (3,3,6) case of tests/test_gpu_bp4_shapes.py"""
    if name in NT_CODES:
        return gpu_graph(name), oracle_library_forms(name)
    g, og, _ = graphs(name)
    return g, og


@functools.lru_cache(maxsize=None)
def syndromes(name, B, p):
    _, og = pair(name)
    ex, ez = og.pauli_noise(0xB0D + B, p, 300, B)
    return og.syndrome(ex, ez)  # shared by the cases of one code: nobody writes to them


class configured:
    def __init__(self, g, og, launch, shared):
        self.g, self.og, self.launch, self.shared = g, og, launch, shared

    def __enter__(self):
        self.g.set_launch(*self.launch)
        self.g.set_bp4_shared_lse(self.shared)
        self.og.set_vn_shared_lse(self.shared)

    def __exit__(self, *exc):
        self.g.set_launch(0, 0)
        self.g.set_bp4_shared_lse(False)
        self.og.set_vn_shared_lse(False)
        self.g.set_saturation_shortcut(True)


def decode_both_ways(name, B, p, iters, factor, launch, shared, what, **chan):
    """One oracle decode, the GPU's with the shortcuts off and on, everything compared."""
    g, og = pair(name)
    sx, sz = syndromes(name, B, p)
    gchan = {k: (to_gpu(v) if k == "llr_ch" else tuple(to_gpu(m) for m in v) if k == "msg_init" else v) for k, v in chan.items()}
    with configured(g, og, launch, shared):
        o = og.bp4_decode(sx, sz, iters, "boxplus-phi", factor, return_msgs=True, **chan)
        for shortcut in (False, True):
            g.set_saturation_shortcut(shortcut)
            got = g.bp4_decode(to_gpu(sx), to_gpu(sz), iters, "boxplus-phi", factor, return_msgs=True, **gchan)
            _eq(o, got, f"{name} B={B} p={p} it={iters} factor={factor} shared={shared} shortcut={shortcut} {what}")


# ---- bounded side -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("name", NT_CODES)
def test_first_decoder_bounded(name, B):
    for p0 in (0.05, 0.3):
        L = llr_const(p0)
        for factor in (1.0, 0.8):
            assert proven(factor, L)
            for p in (0.01, 0.12):
                for iters in (6, 12):
                    for shared in (False, True):
                        decode_both_ways(name, B, p, iters, factor, (256, 1), shared, f"llr_const({p0})", llr_const=L)


@functools.lru_cache(maxsize=None)
def weights(name, wname, scale):
    """(host list, device handle on the code's GPU) of a shipped weight file with W_out scaled: uploaded once"""
    w = [a.copy() for a in read_weight_list(wname)]
    w[0] = (w[0] * F32(scale)).astype(F32)
    return w, GnnWeights(w, pair(name)[0].device)


def sandwich_both_ways(name, wname, B, p, iters, factors, launch, shared, scale=1.0):
    """The sandwich in full and compacted, shortcuts off and on, against the oracle's: decisions, rounds and the marginals byte for byte
    (compacted: of the last decoder for the samples it ran on, of the first for those that left the flagged set before it)."""
    g, og = pair(name)
    sx, sz = syndromes(name, B, p)
    w, gw = weights(name, wname, scale)
    L0 = llr_const(0.05)
    with configured(g, og, launch, shared):
        o = og.sandwich_decode(sx, sz, iters, [w], L0, factors=factors, return_llr=True)
        first = og.bp4_decode(sx, sz, iters[0], "boxplus-phi", factors[0], llr_const=L0)
        for shortcut in (False, True):
            g.set_saturation_shortcut(shortcut)
            for compact in (False, True):
                got = g.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw], L0, factors=factors, compact=compact, return_llr=True,
                                        return_rounds=True)
                what = f"{name} B={B} p={p} it={iters} factors={factors} shared={shared} shortcut={shortcut} compact={compact} scale={scale}"
                rounds, llr = got["rounds"].cpu().numpy(), got["llr"].cpu().numpy()
                assert np.array_equal(o["rounds"], rounds), what
                assert o["x_hat"].tobytes() == got["x_hat"].cpu().numpy().tobytes(), what
                assert o["z_hat"].tobytes() == got["z_hat"].cpu().numpy().tobytes(), what
                ran = (rounds == 1) if compact else np.ones(B, bool)
                assert llr[ran].tobytes() == o["llr"][ran].tobytes(), what + ": marginals of the second decoder"
                assert llr[~ran].tobytes() == first["llr"][~ran].tobytes(), what + ": marginals of the first decoder"
    return o["rounds"]


def gnn_bound(wname, scale=1.0):
    w = read_weight_list(wname)
    return float((np.abs(w[0].astype(np.float64) * scale).sum(axis=0) + np.abs(w[1].astype(np.float64))).max()) * (1.0 + 1e-5)


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("name,lreg", NQ_CASES)
def test_later_decoder_bounded_in_the_sandwich(name, lreg, B):
    """The second decoder reads the GNN's output as per-qubit LLRs (NQ = lreg) with the bound of the shipped weights."""
    g, _ = pair(name)
    assert (g.n + 63) // 64 == lreg
    ran = 0
    for factor in (1.0, 0.8):
        assert proven(factor, gnn_bound(WEIGHTS_882))
        for p in (0.01, 0.12):
            for it2 in (6, 12):
                for shared in (False, True):
                    ran += int(sandwich_both_ways(name, WEIGHTS_882, B, p, [6, it2], [factor, factor], (64, 1), shared).sum())
    assert ran > 0  # the second decoder did run on flagged samples


@pytest.mark.parametrize("name,wname", [("ghp882", WEIGHTS_882), ("ghp1270", WEIGHTS_1270)])
def test_both_decoders_bounded_at_256_threads(name, wname):
    """The benchmark's own shape: NT = 4 / 5 first, then NQ = 4 / 5 on the feedback GNN's output."""
    assert proven(1.0, gnn_bound(wname)) and proven(1.0, llr_const(0.05))
    ran = 0
    for p in (0.01, 0.12):
        for shared in (False, True):
            ran += int(sandwich_both_ways(name, wname, 5, p, [6, 12], [1.0, 1.0], (256, 1), shared).sum())
    assert ran > 0


# ---- fallback side ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NT_CODES)
def test_first_decoder_falls_back(name):
    g, og = pair(name)
    L = llr_const(0.05)
    assert not proven(1.6, L) and not proven(1.0, 60.0)
    rng = np.random.RandomState(5)
    for B in (3, 5):
        init = (rng.uniform(-200.0, 200.0, size=(B, og.E_x)).astype(F32), rng.uniform(-200.0, 200.0, size=(B, og.E_z)).astype(F32))
        for p in (0.01, 0.12):
            for shared in (False, True):
                decode_both_ways(name, B, p, 6, 1.6, (256, 1), shared, "factor 1.6", llr_const=L)
                decode_both_ways(name, B, p, 12, 1.0, (256, 1), shared, "llr_const 60", llr_const=60.0)
                decode_both_ways(name, B, p, 6, 1.0, (256, 1), shared, "msg_init +-200", llr_const=L, msg_init=init)


@pytest.mark.parametrize("name,lreg", NQ_CASES + [("ghp882", 4), ("ghp1270", 5)])
def test_callers_own_llrs_fall_back(name, lreg):
    """fgnn_bp4_decode with llr_ch comes without a bound, whatever the values: +-100 here, beyond both domains' edges once summed."""
    g, og = pair(name)
    launch = (256, 1) if name in NT_CODES else (64, 1)
    assert (g.n + launch[0] - 1) // launch[0] == lreg
    rng = np.random.RandomState(6)
    for B in (3, 5):
        llr = (np.where(rng.rand(B, 3, g.n) < 0.5, -100.0, 100.0) * rng.uniform(0.9, 1.0, size=(B, 3, g.n))).astype(F32)
        for shared in (False, True):
            for factor in (1.0, 0.8):
                decode_both_ways(name, B, 0.12, 6, factor, launch, shared, "llr_ch +-100", llr_ch=llr)


@pytest.mark.parametrize("name,lreg", NQ_CASES)
def test_sandwich_with_scaled_output_weights_falls_back(name, lreg):
    """W_out x 30: the GNN's outputs reach magnitudes of 30 to 40 (with three saturated messages: totals past 87) and its bound, 42.8,
    says so, which takes the second decoder to the guarded kernel.  Again x 100 (outputs past 87 by themselves), where a bounded
    softplus is certain to leave its domain: a library built to pick the bounded kernel regardless fails here at x 100, not at x 30."""
    ran = 0
    for scale in (30.0, 100.0):
        assert not proven(1.0, gnn_bound(WEIGHTS_882, scale))
        for B in (3, 5):
            for shared in (False, True):
                ran += int(sandwich_both_ways(name, WEIGHTS_882, B, 0.12, [6, 12], [1.0, 1.0], (64, 1), shared, scale=scale).sum())
    assert ran > 0


# ---- threshold edges --------------------------------------------------------------------------------------------------------------------
def _edge(limit):
    """(largest float32 <= limit, the float32 after it)"""
    f = F32(limit)
    if float(f) > limit:
        f = np.nextafter(f, F32(0))
    return f, np.nextafter(f, F32(np.inf))


def test_llr_const_either_side_of_both_inequalities():
    M = 3.0 * PHI0
    in2, out2 = _edge((BOUNDED_MAX - 1.0 - M) / 2.0)  # M + 2 L + 1 <= 80: L = 14.5467...
    in1, out1 = _edge(BOUNDED_MAX - M)                # M + L <= 80:       L = 30.0934...
    assert proven(1.0, in2) and not proven(1.0, out2) and not proven(1.0, in1) and not proven(1.0, out1)
    assert M + float(in1) <= BOUNDED_MAX < M + float(out1)
    for L in (in2, out2, in1, out1, -in2, -out2):
        for p in (0.01, 0.12):
            decode_both_ways("ghp882", 3, p, 6, 1.0, (256, 1), False, f"llr_const {float(L)!r}", llr_const=float(L))
