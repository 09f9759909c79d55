"""The BP4 hot loops with compile-time trips, against the C oracle by exact equality.

With 256 threads per codeword a thread of the (3,3,6)-regular phi kernels owns ceil(n / 256) qubits and as many checks: 4 on [[882,24]],
whose fourth trip has 114 of 256 lanes active, and 5 on [[1270,28]], whose fifth has 246.  The first decoder (one constant channel LLR)
runs those trips unrolled from one per-thread LDS base, the later decoders (per-qubit channel LLRs in registers, NQ = 4 / 5) run their
check phase the same way, every kernel reads a check's packed row at a scalar base plus a per-thread offset, and the log of every
log-sum-exp is the range-specialised one of fgnn_math_ranged.h.  None of it may change a bit: marginals, decisions, soft syndromes and
final messages must equal the oracle's for 1, 2, 3 and 16 iterations, at batch sizes 1 and 3 (a thread per node: one guarded trip),
3 at 256 threads per codeword and 257 (the default launch of a large batch), with the literal and the shared log-sum-exp, and with
normalisation factors 1.0 and 0.8 (the two copies of the check update), in the fixed dataflow and with the exact shortcuts on.
Noise at p = 0.08, so messages are not saturated.  The sample index of a compacted round reaches BP4 through the sandwich driver only
(the C ABI's fgnn_bp4_decode takes none, so a permuted index cannot be given): the last test runs it there on both codes, with a proper
subset of the samples flagged, and compares the marginals byte for byte.
"""
import numpy as np
import pytest

from helpers import WEIGHTS_882, WEIGHTS_1270, gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu
SEED = 0x5EED
KEYS = ("llr", "x_hat", "z_hat", "x_logit", "z_logit", "msg_x", "msg_z")
ITERS = (1, 2, 3, 16)
FACTORS = (1.0, 0.8)
# (batch, launch): launch = (threads per codeword, codewords per workgroup) or None for the library's choice
BATCHES = [(1, None), (3, None), (3, (256, 1)), (257, None)]


def _eq(o, g, what):
    for k in KEYS:
        a = o[k] if isinstance(o[k], np.ndarray) else o[k].cpu().numpy()
        b = g[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"{what} {k}: {int((a != b).sum())} of {a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


def _channel_llrs(B, n, seed):
    """Per-qubit LLRs of both signs, with zeros and a few magnitudes beyond the softplus / phi / log-sum-exp thresholds."""
    rng = np.random.RandomState(seed)
    llr = rng.uniform(-4.0, 6.0, size=(B, 3, n)).astype(np.float32)
    specials = np.array([0.0, -0.0, 13.95, -13.95, 16.7, 20.0, -25.0, 37.5], np.float32)
    pick = rng.rand(B, 3, n) < 0.05
    llr[pick] = specials[rng.randint(0, len(specials), size=int(pick.sum()))]
    return llr


@pytest.mark.parametrize("shared", [False, True], ids=["literal", "shared"])
@pytest.mark.parametrize("per_qubit", [False, True], ids=["constant-llr", "per-qubit-llr"])
@pytest.mark.parametrize("B,launch", BATCHES)
@pytest.mark.parametrize("name", ["ghp882", "ghp1270"])
def test_outputs_equal_the_oracle(name, B, launch, per_qubit, shared):
    og, gg = oracle_library_forms(name), gpu_graph(name)
    prev = gg.bp4_shared_lse
    try:
        og.set_vn_shared_lse(shared)
        gg.set_bp4_shared_lse(shared)
        if launch:
            gg.set_launch(*launch)
        ex, ez = og.pauli_noise(SEED, 0.08, 700, B)
        sx, sz = og.syndrome(ex, ez)
        tx, tz = to_gpu(sx), to_gpu(sz)
        if per_qubit:
            llr = _channel_llrs(B, gg.n, 21)
            chan_o, chan_g = dict(llr_ch=llr), dict(llr_ch=to_gpu(llr))
        else:
            chan_o = chan_g = dict(llr_const=llr_const(0.08))
        for factor in FACTORS:
            for iters in ITERS:
                o = og.bp4_decode(sx, sz, iters, "boxplus-phi", factor, return_msgs=True, **chan_o)
                for shortcut in (False, True):
                    gg.set_saturation_shortcut(shortcut)
                    g = gg.bp4_decode(tx, tz, iters, "boxplus-phi", factor, return_msgs=True, **chan_g)
                    _eq(o, g, f"{name} B={B} launch={launch} per_qubit={per_qubit} shared={shared} factor={factor} it={iters} shortcut={shortcut}")
    finally:
        og.set_vn_shared_lse(prev)
        gg.set_bp4_shared_lse(prev)
        gg.set_saturation_shortcut(True)
        gg.set_launch(0, 0)


@pytest.mark.parametrize("name,wname", [("ghp882", WEIGHTS_882), ("ghp1270", WEIGHTS_1270)])
def test_compacted_round_in_the_sandwich(name, wname):
    """BP4-3 -> GNN -> BP4-16 with the flagged subset compacted, at 256 threads per codeword: the second decoder runs the register-LLR
    kernel with all its 4 ([[882,24]]) / 5 ([[1270,28]]) trips through the sample index.  Every second sample is noiseless, so the
    index is a proper subset (1, 3, 5, 7 of 9).  It is the ascending list fgnn_compact emits: the public ABI offers no way to hand
    BP4 a permuted one (fgnn_bp4_decode takes no index), and the sandwich returns no messages or soft syndromes, so what can be reached
    is compared as strictly as it can be: rounds, decisions and the marginals byte for byte — of the last decoder for the samples
    it ran on, of the first decoder (a BP4-3 oracle decode) for the samples that left the flagged set before it."""
    from feedback_gnn_amd.graph import GnnWeights
    from feedback_gnn_amd.weights_io import read_weight_list
    B, iters = 9, [3, 16]
    w = read_weight_list(wname)
    og, gg = oracle_library_forms(name), gpu_graph(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 800, B)
    ex, ez = ex.copy(), ez.copy()
    ex[::2], ez[::2] = 0, 0
    sx, sz = og.syndrome(ex, ez)
    L0 = llr_const(0.08)
    gw = GnnWeights(w, gg.device)
    o = og.sandwich_decode(sx, sz, iters, [w], L0, return_llr=True)
    first = og.bp4_decode(sx, sz, iters[0], "boxplus-phi", 1.0, llr_const=L0)
    for shortcut in (False, True):
        try:
            gg.set_saturation_shortcut(shortcut)
            gg.set_launch(256, 1)
            g = gg.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw], L0, compact=True, return_llr=True, return_rounds=True)
        finally:
            gg.set_saturation_shortcut(True)
            gg.set_launch(0, 0)
        rounds = g["rounds"].cpu().numpy()
        assert np.array_equal(o["rounds"], rounds)
        assert not rounds[::2].any() and rounds[1::2].all(), rounds.tolist()  # the noiseless samples leave, the others stay flagged
        assert o["x_hat"].tobytes() == g["x_hat"].cpu().numpy().tobytes() and o["z_hat"].tobytes() == g["z_hat"].cpu().numpy().tobytes()
        llr = g["llr"].cpu().numpy()
        ran = rounds == 1
        bad = np.argwhere((llr != o["llr"]).any((1, 2)) & ran).ravel().tolist()
        assert llr[ran].tobytes() == o["llr"][ran].tobytes(), f"{name} shortcut={shortcut}: marginals of the second decoder differ for samples {bad}"
        assert llr[~ran].tobytes() == first["llr"][~ran].tobytes(), f"{name} shortcut={shortcut}: marginals of the first decoder differ"
