"""The BP4 kernels that take a check's edges ready-made from the graph upload, against the C oracle by exact equality.

The (3,3,6)-regular phi kernels with compile-time trips — the first decoder (NT = 4 on [[882,24]], last trip 114 of 256 lanes; NT = 5 on
[[1270,28]], last trip 246) and the register-LLR decoders (NQ = 4 / 5) — read a check's slots as 32-bit LDS offsets (g.cslot32) and hand
them to the LDS instructions as they are; their epilogue evaluates phi(|llr|) once per qubit and sums the stored values per soft-syndrome
row, keeps the decisions in registers for the fused flag test and takes each check's qubits from its g.cvn16 row.  These are the only
shapes the changed code runs at.  None of it may change a bit: marginals, decisions, soft syndromes and final messages equal the oracle's
for 1, 2 and 16 iterations, at batch 1 and 3 (a thread per node: one guarded trip), 3 at 256 threads per codeword and 257, with factors
1.0 and 0.8 (the two copies of the check update), one constant and per-qubit channel LLRs, the literal and the shared log-sum-exp, and
the exact shortcuts off and on.  Noise at p = 0.08, so nothing saturates.  The fused flag reaches a caller through the sandwich driver
only: three decoders at (256, 1) with every second sample noiseless, so the flag of the first decoder (NT kernel) and of the second (NQ
kernel) takes both values within one launch, checked by `rounds`.  One case runs with the runtime-degree fallback forced.
"""
import functools

import numpy as np
import pytest

from helpers import WEIGHTS_882, WEIGHTS_1270, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_gpu_bp4_hot_loops import _channel_llrs, _eq

pytestmark = pytest.mark.gpu
SEED = 0x5EED
ITERS = (1, 2, 16)
FACTORS = (1.0, 0.8)
# (batch, launch): launch = (threads per codeword, codewords per workgroup) or None for the library's choice
BATCHES = [(1, None), (3, None), (3, (256, 1)), (257, None)]


@functools.lru_cache(maxsize=None)
def _syndromes(name, B):
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 700, B)
    return og.syndrome(ex, ez)  # shared by the cases of one code and batch: nobody writes to them


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
        sx, sz = _syndromes(name, B)
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


@pytest.mark.parametrize("per_qubit", [False, True], ids=["constant-llr", "per-qubit-llr"])
@pytest.mark.parametrize("name", ["ghp882", "ghp1270"])
def test_generic_fallback_is_still_reached_and_equal(name, per_qubit):
    """fgnn_graph_force_generic: the runtime-degree kernel (CSR tables, no ready-made row) on the same inputs gives the same bytes as
    the oracle and as the ready-row kernels."""
    og, gg = oracle_library_forms(name), gpu_graph(name)
    B = 3
    sx, sz = _syndromes(name, B)
    if per_qubit:
        llr = _channel_llrs(B, gg.n, 21)
        chan_o, chan_g = dict(llr_ch=llr), dict(llr_ch=to_gpu(llr))
    else:
        chan_o = chan_g = dict(llr_const=llr_const(0.08))
    o = og.bp4_decode(sx, sz, 16, "boxplus-phi", 0.8, return_msgs=True, **chan_o)
    try:
        gg.set_launch(256, 1)
        ready = gg.bp4_decode(to_gpu(sx), to_gpu(sz), 16, "boxplus-phi", 0.8, return_msgs=True, **chan_g)
        gg.force_generic(True)
        generic = gg.bp4_decode(to_gpu(sx), to_gpu(sz), 16, "boxplus-phi", 0.8, return_msgs=True, **chan_g)
    finally:
        gg.force_generic(False)
        gg.set_launch(0, 0)
    _eq(o, ready, f"{name} ready rows")
    _eq(o, generic, f"{name} forced generic")


@pytest.mark.parametrize("name,wname", [("ghp882", WEIGHTS_882), ("ghp1270", WEIGHTS_1270)])
def test_fused_flag_takes_both_values_in_one_launch(name, wname):
    """BP4-3 -> GNN -> BP4-8 -> GNN -> BP4-16 at 256 threads per codeword.  The first decoder (NT kernel) and the second (NQ kernel)
    write the flag of the next round from their epilogues.  Every second sample is noiseless and leaves after the first decoder
    (rounds 0); of the others some leave after the second (rounds 1) and some stay (rounds 2): both launches write both flag values.
    `rounds`, the decisions and the final marginals of the samples that ran all rounds equal the oracle's."""
    from feedback_gnn_amd.graph import GnnWeights
    from feedback_gnn_amd.weights_io import read_weight_list
    B, iters = 12, [3, 8, 16]
    w = read_weight_list(wname)
    og, gg = oracle_library_forms(name), gpu_graph(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 900, B)
    ex, ez = ex.copy(), ez.copy()
    ex[::2], ez[::2] = 0, 0
    sx, sz = og.syndrome(ex, ez)
    L0 = llr_const(0.08)
    gw = GnnWeights(w, gg.device)
    o = og.sandwich_decode(sx, sz, iters, [w, w], L0, return_llr=True)
    assert set(o["rounds"].tolist()) == {0, 1, 2}, o["rounds"].tolist()  # the inputs do what the docstring says
    for compact in (False, True):
        for shortcut in (False, True):
            try:
                gg.set_saturation_shortcut(shortcut)
                gg.set_launch(256, 1)
                g = gg.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw, gw], L0, compact=compact, return_llr=True, return_rounds=True)
            finally:
                gg.set_saturation_shortcut(True)
                gg.set_launch(0, 0)
            what = f"{name} compact={compact} shortcut={shortcut}"
            rounds = g["rounds"].cpu().numpy()
            assert np.array_equal(o["rounds"], rounds), (what, rounds.tolist(), o["rounds"].tolist())
            assert o["x_hat"].tobytes() == g["x_hat"].cpu().numpy().tobytes(), what
            assert o["z_hat"].tobytes() == g["z_hat"].cpu().numpy().tobytes(), what
            last = rounds == 2
            assert g["llr"].cpu().numpy()[last].tobytes() == o["llr"][last].tobytes(), what
