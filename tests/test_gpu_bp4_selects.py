"""bp4_kernel with the selects of phi and softplus as one v_med3_f32 / v_max_f32, against the C oracle by exact equality.

Every bp4_kernel takes its phi and its softplus from fgnn_math_ranged.h (fg_phi_med, fg_softplus_max: the last select of the routine
as a median / a maximum); the oracle compiles fgnn_math.h and keeps the compare-and-select forms.  The inputs here sit where the two
forms take different routes to the same float: a softplus argument beyond +-13.9423847 (identity above, exp below, flushed under -87),
and a phi argument in (13.9423857, 14.7666502], where the computed log1p exceeds its argument and only the median with
S = log1p(exp(threshold)) — not a maximum — returns the argument.
  * first decoder (one constant channel LLR: the NT = 4 kernel on [[882,24]], NT = 5 on [[1270,28]]): LLR 14.2, and 13.9423847 exactly;
  * later decoders (per-qubit LLRs in registers: NQ = 4 / 5): LLRs from +-[13.9, 14.8], from +-[86, 88], and mixed with ordinary ones;
  * each with factor 1.0 and 0.8 (the two copies of the check update), in the fixed dataflow and with the exact shortcuts on, through
    the trace entry point, with the runtime-degree kernel forced, and on gb126 ((5,10)-regular: no compile-time instantiation).
Marginals, decisions, soft syndromes and final messages after 3 iterations, B = 320: one codeword per workgroup needs B > 256, below it
the thread-per-node launch runs.  Noise at p = 0.08.
"""
import functools

import numpy as np
import pytest

from helpers import gpu_graph, oracle_library_forms, to_gpu
from test_gpu_bp4_hot_loops import _eq

pytestmark = pytest.mark.gpu
SEED, B, ITERS = 0x5EED, 320, 3
THR = np.float32(13.9423847)                 # FG_SOFTPLUS_THRESH
S_AT_THR = np.float32(13.9423857)            # FG_SOFTPLUS_AT_THRESH, the float after it
CHANNELS = ["const-14.2", "const-thr", "band", "deep", "mixed"]


@functools.lru_cache(maxsize=None)
def _syndromes(name):
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 1100, B)
    return og.syndrome(ex, ez)  # shared by the cases of one code: nobody writes to them


@functools.lru_cache(maxsize=None)
def _llrs(kind, n):
    rng = np.random.RandomState({"band": 31, "deep": 32, "mixed": 33}[kind])
    sign = np.where(rng.rand(B, 3, n) < 0.5, -1.0, 1.0)
    band = rng.uniform(13.9, 14.8, size=(B, 3, n)) * sign
    deep = rng.uniform(86.0, 88.0, size=(B, 3, n)) * sign
    if kind == "band":
        return band.astype(np.float32)
    if kind == "deep":
        return deep.astype(np.float32)
    llr = rng.uniform(-4.0, 6.0, size=(B, 3, n))
    u = rng.rand(B, 3, n)
    llr = np.where(u < 0.30, band, np.where(u < 0.40, deep, llr)).astype(np.float32)
    specials = np.array([THR, -THR, S_AT_THR, -S_AT_THR, 87.0, -87.0, 0.0, -0.0, 14.7666502, 16.635532], np.float32)
    pick = rng.rand(B, 3, n) < 0.05
    llr[pick] = specials[rng.randint(0, len(specials), size=int(pick.sum()))]
    return llr


def _channel(kind, n):
    """(oracle keywords, GPU keywords) of one channel setting"""
    if kind.startswith("const"):
        L0 = float(np.float32(14.2) if kind == "const-14.2" else THR)
        return dict(llr_const=L0), dict(llr_const=L0)
    llr = _llrs(kind, n)
    return dict(llr_ch=llr), dict(llr_ch=to_gpu(llr))


def _check(name, kind, factors, generic=False):
    og, gg = oracle_library_forms(name), gpu_graph(name)
    sx, sz = _syndromes(name)
    tx, tz = to_gpu(sx), to_gpu(sz)
    chan_o, chan_g = _channel(kind, gg.n)
    try:
        gg.force_generic(generic)
        for factor in factors:
            o = og.bp4_decode(sx, sz, ITERS, "boxplus-phi", factor, return_msgs=True, **chan_o)
            for shortcut in (False, True):
                gg.set_saturation_shortcut(shortcut)
                g = gg.bp4_decode(tx, tz, ITERS, "boxplus-phi", factor, return_msgs=True, **chan_g)
                _eq(o, g, f"{name} {kind} generic={generic} factor={factor} shortcut={shortcut}")
    finally:
        gg.force_generic(False)
        gg.set_saturation_shortcut(True)


@pytest.mark.parametrize("kind", CHANNELS)
@pytest.mark.parametrize("name", ["ghp882", "ghp1270"])
def test_outputs_equal_the_oracle(name, kind):
    _check(name, kind, (1.0, 0.8))


@pytest.mark.parametrize("kind", CHANNELS)
def test_runtime_degree_kernel_forced(kind):
    _check("ghp882", kind, (0.8,), generic=True)


@pytest.mark.parametrize("kind", CHANNELS)
def test_runtime_degree_code(kind):
    _check("gb126", kind, (1.0, 0.8))


@pytest.mark.parametrize("kind", ["const-14.2", "const-thr", "mixed"])
@pytest.mark.parametrize("name", ["ghp882", "ghp1270"])
def test_trace_entry_point(name, kind):
    """One launch that records the soft syndromes and the messages after 0 .. 3 iterations: every slot equals the oracle's decode of
    that many iterations, the marginals and decisions those of the last."""
    og, gg = oracle_library_forms(name), gpu_graph(name)
    sx, sz = _syndromes(name)
    chan_o, chan_g = _channel(kind, gg.n)
    for factor in (1.0, 0.8):
        tr = gg.bp4_decode_trace(to_gpu(sx), to_gpu(sz), ITERS, "boxplus-phi", factor, want_tape=True, **chan_g)
        for k in range(ITERS + 1):
            o = og.bp4_decode(sx, sz, k, "boxplus-phi", factor, return_msgs=True, **chan_o)
            for key, got in (("x_logit", tr["x_logit"][k]), ("z_logit", tr["z_logit"][k]), ("msg_x", tr["tape_x"][k]),
                             ("msg_z", tr["tape_z"][k])):
                assert o[key].tobytes() == got.cpu().numpy().tobytes(), f"{name} {kind} factor={factor} trace slot {k} {key}"
        for key in ("llr", "x_hat", "z_hat"):
            assert o[key].tobytes() == tr[key].cpu().numpy().tobytes(), f"{name} {kind} factor={factor} trace {key}"
