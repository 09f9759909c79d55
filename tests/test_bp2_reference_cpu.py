"""Binary syndrome BP (LDPCBPDecoder.call with is_syndrome=True, sionna/fec/ldpc/decoding.py:874-1048): the C oracle og_bp2_decode
against the independent float64 restatement numpy_ref.bp2_decode, written from the reference's Python.  CPU only.

Bounds.  After one or two iterations nothing has been amplified yet, so every soft output must agree with float64 to a bound relative
to the sample's largest |logit| (floored at one logit, so that an all-zero sample compares absolutely):
  - min-sum, MINSUM_TOL = 2e-6: no transcendentals, only float32 adds and the products with the factor.  Each output is a sum of
    at most dv + 1 rounded terms, a few float32 ulps (2^-24 = 6e-8) per term; 94-edge bits of the over-complete matrix reach 1.3e-6.
  - phi and tanh, SOFT_TOL = 2e-5, ten times looser: the reference evaluates log(exp(x)+1) - log(exp(x)-1) and tanh / atanh near
    +-1 in float32, where a few ulps of the argument become ~1e-5 of the result (largest seen: 8.3e-6, phi on gb48 at two
    iterations).
That holds for inputs in the channel range of the library's models, |llr| <= 4 (p >= 0.018).  Stronger messages put the float32
phi in its cancellation regime (phi(x) for x above ~12 is 0 or 1 ulp of x) and tanh in saturation; the reference itself carries
that rounding there, so those inputs are compared only where they cannot dominate a check (the edge-LLR test) or by decoding
outcome (the many-iteration test).  For the same reason the over-complete matrix, whose bits have 76-94 edges, is compared at one
iteration only: its second-iteration messages are sums of ~90 terms and already saturate phi.

Open questions, not tested: a NaN input (the reference's clip_by_value and the library's FG_MIN / FG_MAX order NaN differently, and
the spec has no rule for it), and an input logit in (1e-45, 5.9e-39): the tanh rule's msg**-1 (:600) of half of it overflows to inf
in float32, in the reference as in the oracle, and the clip then sends +-16.6 where float64 sends the product of the other inputs.
"""
import numpy as np
import pytest

from helpers import binary_oracle, code, oracle_library_forms
from oracle import numpy_ref as R

SEED = 0x5EED
RULES = ("boxplus-phi", "minsum", "boxplus")
FACTORS = (1.0, 0.8, 0.625)
CODES = ("ghp882", "gb48", "rsurf5", "hp_c7", "gb126", "gb46_oc")
OVERCOMPLETE = ("gb46_oc",)
SOFT_TOL = 2e-5
MINSUM_TOL = 2e-6
F32 = np.float32


def _tol(cn_type):
    return MINSUM_TOL if cn_type == "minsum" else SOFT_TOL


def _llr_const(p0):
    """The BSC logit of BP_BSC_Model (decoding.py :210-211): log(p0 / (1 - p0)) in float32."""
    p0 = F32(p0)
    return float(-np.log((F32(1) - p0) / p0, dtype=F32))


def _syndromes(og, hx, p, B, first=0):
    e = og.bsc_noise(SEED, p, first, B)
    return e, (e.astype(np.int64) @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


def _channel(B, n, seed):
    """Per-bit logits with |llr| in [0.2, 4], 15 % of them on the 'error' side."""
    rng = np.random.RandomState(seed)
    mag = rng.uniform(0.2, 4.0, size=(B, n))
    return (mag * np.where(rng.rand(B, n) < 0.15, 1.0, -1.0)).astype(F32)


def _compare(og, hx, synd, iters, cn_type, factor, tol, cols=slice(None), **llr):
    """The oracle and the restatement at each iteration count: soft outputs (of the bits `cols`) within tol * max(1, max |logit|) per
    sample, hard decisions identical wherever |logit| exceeds that bound.  Returns the largest relative deviation seen."""
    worst = 0.0
    for it in iters:
        s0, h0 = og.bp2_decode(synd, it, cn_type, factor, **llr)
        s1, h1 = R.bp2_decode(hx, synd, it, cn_type, factor, **llr)
        s0, h0, s1, h1 = s0[:, cols], h0[:, cols], s1[:, cols], h1[:, cols]
        scale = np.maximum(1.0, np.abs(s1).max(1, keepdims=True))
        dev = np.abs(s0.astype(np.float64) - s1) / scale
        worst = max(worst, float(dev.max()))
        assert dev.max() <= tol, (cn_type, factor, it, float(dev.max()))
        firm = np.abs(s1) > tol * scale
        assert np.array_equal(h0[firm], h1[firm]), (cn_type, factor, it)
    return worst


@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("cn_type", RULES)
def test_one_and_two_iterations_against_float64(name, cn_type):
    og, hx = oracle_library_forms(name), np.asarray(code(name).hx)
    B = 24
    _, synd = _syndromes(og, hx, 0.05, B)
    iters = (1,) if name in OVERCOMPLETE else (1, 2)
    llr = _channel(B, og.n, 3)
    for factor in FACTORS:
        _compare(og, hx, synd, iters, cn_type, factor, _tol(cn_type), llr_const=_llr_const(0.1))
        _compare(og, hx, synd, iters, cn_type, factor, _tol(cn_type), llr_ch=llr)


# (code, p, iterations): noise at which plain min-sum (factor 1) still converges on most samples
MANY = [("ghp882", 0.02, 64), ("gb48", 0.03, 32), ("rsurf5", 0.03, 24), ("hp_c7", 0.03, 32), ("gb126", 0.02, 24), ("gb46_oc", 0.03, 24)]


@pytest.mark.parametrize("name,p,iters", MANY)
@pytest.mark.parametrize("cn_type", RULES)
def test_many_iterations_same_logical_class(name, p, iters, cn_type):
    """The bar of test_c_oracle_vs_numpy_restatement (tests/test_oracle_kat.py): over many iterations float32 rounding of phi and tanh
    (see the module docstring) is amplified through the transient, so two faithful implementations can end a trapping-set sample on
    different sides of convergence.  On samples BOTH converge to the syndrome the corrections must lie in the same logical class, the
    test BP_BSC_Model applies (hz_perp . (e_hat_1 ^ e_hat_2) = 0, logical_pcm = hz_perp for pcm = hx); convergence flips are counted,
    not compared, and the convergence rates agree within a margin.  Normalized min-sum (factor < 1) has no transcendentals and rounds
    only in adds and products: its bar is three times tighter (flips 5 % rather than 15 %, rates 2 % rather than 6 %) and every
    commonly converged sample must have the same class (seen: at most 1 flip in 96).  Plain min-sum (factor 1) keeps the looser bar:
    its messages are sums of multiples of the one channel logit, which cancel to exactly 0 in float64 but to +-1 ulp in float32, and
    the sign of a zero message (+1, :697-703) flips every other output of its check (seen: up to 6 flips in 96 here, 40 on gb126 at
    p = 0.03)."""
    c = code(name)
    og, hx = oracle_library_forms(name), np.asarray(c.hx, np.int64)
    B = 96
    _, synd = _syndromes(og, hx, p, B, first=77)
    L = _llr_const(p)
    for factor in FACTORS:
        _, h0 = og.bp2_decode(synd, iters, cn_type, factor, llr_const=L)
        _, h1 = R.bp2_decode(hx, synd, iters, cn_type, factor, llr_const=L)
        conv0 = ((h0.astype(np.int64) @ hx.T % 2) == synd).all(1)
        conv1 = ((h1.astype(np.int64) @ hx.T % 2) == synd).all(1)
        both, flipped = conv0 & conv1, conv0 ^ conv1
        assert both.sum() >= B // 4, "too few converged samples for the comparison to mean anything"
        exact = cn_type == "minsum" and factor != 1.0
        assert flipped.mean() <= (0.05 if exact else 0.15), (factor, flipped.mean())
        assert abs(conv0.mean() - conv1.mean()) <= (0.02 if exact else 0.06), (factor, conv0.mean(), conv1.mean())
        same_class = ~((((h0 ^ h1).astype(np.int64) @ np.asarray(c.hz_perp, np.int64).T) % 2).any(1))
        assert same_class[both].mean() >= (1.0 if exact else 0.98), (factor, same_class[both].mean())


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("gb48", "rsurf5", "gb126"))
def test_zero_channel_logits(name, cn_type):
    """llr_const = 0: every message starts at 0 — phi's lower clip (phi(8.5e-8) = 16.6355 in float32, whose own phi is 0 there, against
    1.19e-7 in float64: inside the floored bound), exact min-sum ties, and the tanh rule's t == 0 guard."""
    og, hx = oracle_library_forms(name), np.asarray(code(name).hx)
    synd = np.random.RandomState(5).randint(0, 2, size=(16, hx.shape[0])).astype(np.uint8)
    for factor in FACTORS:
        _compare(og, hx, synd, (1, 2), cn_type, factor, _tol(cn_type), llr_const=0.0)
    if cn_type != "boxplus-phi":  # exact ties and the tanh guard: exactly zero messages, exactly zero logits
        s0, _ = og.bp2_decode(synd, 2, cn_type, 0.8, llr_const=0.0)
        assert not s0.any()


EDGE_LLRS = np.array([20.0, -20.0, np.nextafter(F32(20), F32(0)), np.nextafter(F32(20), F32(np.inf)),
                      -np.nextafter(F32(20), F32(0)), -np.nextafter(F32(20), F32(np.inf)), 0.0, -0.0, 1e-45, -1e-45,
                      np.nextafter(np.finfo(F32).tiny, F32(0)), -np.nextafter(np.finfo(F32).tiny, F32(0)), np.inf, -np.inf, 25.0,
                      -1e30], dtype=F32)


def edge_channel(hx, B, seed):
    """Moderate per-bit logits with the values of EDGE_LLRS on bits no two of which share a check (rotated through the batch, so that
    every value occurs): the +-20 clip exactly, one ulp inside and outside it, +-0, the smallest and the largest subnormal, +-inf and
    far beyond the clip.  One extreme per check keeps the float32 phi out of its cancellation regime (a check whose other inputs are
    all strong) and is enough to reach every input path."""
    hx = np.asarray(hx)
    rng = np.random.RandomState(seed)
    llr = _channel(B, hx.shape[1], seed)
    for b in range(B):
        used = np.zeros(hx.shape[0], bool)
        k = b
        for v in rng.permutation(hx.shape[1]):
            if not (used & (hx[:, v] != 0)).any():
                used |= hx[:, v] != 0
                llr[b, v] = EDGE_LLRS[k % len(EDGE_LLRS)]
                k += 1
    return llr


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("ghp882", "gb48", "rsurf5", "gb126"))
def test_edge_channel_logits(name, cn_type):
    og, hx = oracle_library_forms(name), np.asarray(code(name).hx)
    B = 16
    _, synd = _syndromes(og, hx, 0.05, B)
    llr = edge_channel(hx, B, 11)
    # a second iteration sends the strong bits' messages (20 + their checks' outputs) into the float32 phi's cancellation regime and
    # the tanh's saturation; min-sum has neither
    iters = (1, 2) if cn_type == "minsum" else (1,)
    for factor in FACTORS:
        _compare(og, hx, synd, iters, cn_type, factor, _tol(cn_type), llr_ch=llr)
    # the input clip itself: after zero iterations the output is clip(llr, -20, 20) exactly (decoding.py :918-920, :1031)
    s0, h0 = og.bp2_decode(synd, 0, cn_type, 0.8, llr_ch=llr)
    s1, h1 = R.bp2_decode(hx, synd, 0, cn_type, 0.8, llr_ch=llr)
    assert np.array_equal(s0, s1.astype(F32)) and np.array_equal(h0, h1)
    assert np.array_equal(s0, np.clip(llr, -20, 20)) and np.isfinite(s0).all()


@pytest.mark.parametrize("cn_type", RULES)
def test_all_ones_syndrome_and_zero_iterations(cn_type):
    name = "gb48"
    og, hx = oracle_library_forms(name), np.asarray(code(name).hx)
    B = 8
    ones = np.ones((B, hx.shape[0]), np.uint8)
    for factor in FACTORS:
        _compare(og, hx, ones, (1, 2), cn_type, factor, _tol(cn_type), llr_const=_llr_const(0.1))
        _compare(og, hx, ones, (1, 2), cn_type, factor, _tol(cn_type), llr_ch=_channel(B, og.n, 4))
    s0, h0 = og.bp2_decode(ones, 0, cn_type, 0.8, llr_const=-1.5)
    assert (s0 == F32(-1.5)).all() and not h0.any()


def degenerate_hx():
    """A 7 x 12 check matrix with a degree-1 check (row 0: min-sum's min2 = LARGE + min path, the phi rule's T - a = 0), a degree-2
    check, a bit with no edge (column 11) and irregular degrees elsewhere."""
    h = np.zeros((7, 12), np.uint8)
    h[0, 3] = 1
    h[1, [0, 5]] = 1
    for r, cols in ((2, [0, 1, 2, 4]), (3, [1, 3, 6, 7, 8]), (4, [2, 5, 9]), (5, [4, 6, 8, 9, 10]), (6, [0, 7, 10, 3, 1, 2])):
        h[r, cols] = 1
    return h


@pytest.mark.parametrize("cn_type", RULES)
def test_degree_one_check_and_edge_free_bit(cn_type):
    """A degree-1 check sends phi(T - a) = phi(0) under the phi rule: phi at its lower clip, which float32 evaluates to ln(2^24) =
    16.635532 (exp(8.5e-8) rounds to 1 + 2^-23) and float64 to 16.974.  That gap is the reference's own float32 value, so under
    phi the bit of the degree-1 check is held to it exactly, the others to the usual bound, at one iteration (a second would spread
    the gap)."""
    h = degenerate_hx()
    og = binary_oracle(h)
    rng = np.random.RandomState(9)
    B = 32
    synd = rng.randint(0, 2, size=(B, h.shape[0])).astype(np.uint8)
    phi = cn_type == "boxplus-phi"
    iters, cols = ((1,), np.arange(h.shape[1]) != 3) if phi else ((1, 2), slice(None))
    llrs = (dict(llr_const=_llr_const(0.1)), dict(llr_ch=_channel(B, h.shape[1], 6)))
    for factor in FACTORS:
        for llr in llrs:
            _compare(og, h, synd, iters, cn_type, factor, _tol(cn_type), cols=cols, **llr)
            if phi:
                s0, _ = og.bp2_decode(synd, 1, cn_type, factor, **llr)
                s1, _ = R.bp2_decode(h, synd, 1, cn_type, factor, **llr)
                gap = (R._bp2_phi(0.0) - np.float64(F32(16.635532))) * np.float64(F32(factor))
                assert np.abs(np.abs(s0[:, 3] - s1[:, 3]) - gap).max() <= SOFT_TOL * max(1.0, np.abs(s1).max())
    s0, _ = og.bp2_decode(synd, 2, cn_type, 0.8, llr_const=-1.5)
    assert (s0[:, 11] == F32(-1.5)).all()  # the edge-free bit keeps its channel logit
