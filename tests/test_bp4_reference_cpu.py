"""Quaternary BP (QLDPCBPDecoder.call, sionna/fec/ldpc/decoding_q.py:661-797): the C oracle og_bp4_decode against the independent
float64 restatement numpy_ref.bp4_decode64, written from the reference's Python, for all three check rules.  CPU only.

Bounds.  After one or two iterations nothing has been amplified yet, so the marginals [B,3,n] and the final c->v messages must agree
with float64 to a bound relative to the sample's largest magnitude of that output (floored at 1, so that an all-zero sample compares
absolutely):
  - min-sum, MINSUM_TOL = 6e-6: the check rule has no transcendentals, only float32 compares, adds and the product with the factor.
    What rounds is the qubit update (softplus and a two-term log-sum-exp, each a few ulps of its result) and the totals, sums of at
    most dv + 1 terms: one float32 rounding (2^-24 of the sample's largest magnitude) per term, 95 terms on gb46_oc: 5.7e-6.
    Largest seen: 1.6e-6.
  - phi and tanh, SOFT_TOL = 1e-4: every message goes through two float32 phi evaluations (or tanh and atanh).  For x above ~2,
    phi(x) = softplus(x) - log(exp(x) - 1) is the difference of two numbers near x, so its relative error is about 2 ulp(x) / phi(x):
    2.6e-5 at x = 4, 1e-4 at x = 5.3, the largest v->c message these inputs give at one or two iterations.  At a degree-2 check the
    outgoing message is phi(phi(|nu|)), which carries that relative error back to the scale of |nu|.  Largest seen: 3.1e-5 (phi),
    1.2e-5 (tanh).
  - Soft syndromes (cal_logit over the hz / hx rows or hx_perp / hz_perp) are compared as an interval, not a point.  Their inputs, the
    binary LLRs, reach 10-30 after one iteration.  There phi(|v|) is ~2 exp(-|v|), but float32 evaluates it from two logs of
    magnitude |v|: the absolute error is up to 4 ulp(|v|), which moves phi's input by 4 ulp(|v|) sinh(|v|).  At |v| >= 16.635532 the
    float32 phi is exactly 0.  The reference runs in float32 and carries both effects.  So each input of a row is widened by that
    amount, plus twice the marginals' bound (a binary LLR is 1-Lipschitz in each marginal).  The row's magnitude must then lie in
    [phi(T_hi), phi(T_lo)], by the monotonicity of phi, with the base bound on either side; T_hi and T_lo are the float64 sums at the
    ends of the widened inputs.  Where no input can change sign, the signs must agree as well.  A row whose inputs are all saturated
    has float32 T = 0 and logit +-phi32(clip min) = +-16.635532 exactly; float64 gives up to phi(8.5e-8) = 16.974 there, and that
    gap is asserted exactly (test_saturating_channel_llrs).
Decisions (argmin over [0, X, Z, Y], :783-790) must be identical wherever the float64 margin between the two smallest entries
exceeds twice the marginals' bound.

The soft syndromes' largest excess beyond their interval: 1.1e-6 of the scale, for every rule.

The inputs are in the channel range of the library's models: llr_const = log(3 (1 - p) / p) at p = 0.1 (3.3), or per-qubit LLRs
with |llr| in [0.2, 4] and both signs.  The over-complete gb46_oc, whose qubits have 76-94 edges, is compared at one iteration only:
its second-iteration totals are sums of ~90 messages and saturate phi.
"""
import types

import numpy as np
import pytest

from helpers import code, llr_const as _llr_const, oracle_library_forms, oracle_literal_forms, oracle_reassociated_forms
from oracle import numpy_ref as R
from oracle.oracle import OracleGraph

SEED = 0x5EED
RULES = ("boxplus-phi", "minsum", "boxplus")
FACTORS = (1.0, 0.8, 0.625)
CODES = ("ghp882", "ibm72", "gb48", "gb126", "rsurf5", "hp_c7", "gb46_oc")
OVERCOMPLETE = ("gb46_oc",)
SOFT_TOL = 1e-4
MINSUM_TOL = 6e-6
F32 = np.float32
PHI_HI = np.float64(F32(16.635532))
PHI0_F32 = F32(16.635532)  # phi(clip min) in float32: exp(8.5e-8) rounds to 1 + 2^-23, so log(exp(x) - 1) = -ln(2^23)


def tol_of(cn_type):
    return MINSUM_TOL if cn_type == "minsum" else SOFT_TOL


def channel(B, n, seed):
    """Per-qubit LLRs [B,3,n] with |llr| in [0.2, 4], 15 % of them negative."""
    rng = np.random.RandomState(seed)
    mag = rng.uniform(0.2, 4.0, size=(B, 3, n))
    return (mag * np.where(rng.rand(B, 3, n) < 0.15, -1.0, 1.0)).astype(F32)


def syndromes(og, p, B, first=0):
    ex, ez = og.pauli_noise(SEED, p, first, B)
    return og.syndrome(ex, ez)


def _scale(ref):
    return np.maximum(1.0, np.abs(ref).reshape(ref.shape[0], -1).max(1)).reshape((-1,) + (1,) * (ref.ndim - 1))


def _rows(c, stage_one):
    return (np.asarray(c.hz), np.asarray(c.hx)) if stage_one else (np.asarray(c.hx_perp), np.asarray(c.hz_perp))


def soft_syndrome_excess(rows, v64, dv, got, tol):
    """The interval test of the module docstring for the soft syndromes `got` [B,R] of the rows [R,n] on the float64 binary LLRs v64
    [B,n], known to within dv [B,1].  Returns the largest excess beyond the interval relative to the floored scale (<= tol passes)."""
    r, c = np.nonzero(rows)
    nr = rows.shape[0]
    x = np.abs(v64[:, c])
    d = dv + 4.0 * np.spacing(x.astype(F32)).astype(np.float64) * np.sinh(np.minimum(x, 40.0))
    lo_terms = np.where(x + d >= PHI_HI, 0.0, R._bp4_phi(x + d))
    hi_terms = R._bp4_phi(np.maximum(x - d, 0.0))

    def rowsum(t):
        return np.stack([np.bincount(r, weights=row, minlength=nr) for row in t])

    mag_lo, mag_hi = R._bp4_phi(rowsum(hi_terms)), R._bp4_phi(rowsum(lo_terms))
    unsure = rowsum((x - d <= 0).astype(np.float64)) > 0
    sign64 = 1.0 - 2.0 * (rowsum((v64[:, c] < 0).astype(np.float64)) % 2)
    g = got.astype(np.float64)
    scale = np.maximum(1.0, np.maximum(np.abs(g), mag_hi).max(1, keepdims=True))
    m = np.abs(g)
    excess = np.maximum(mag_lo - m, m - mag_hi)
    wrong_sign = ~unsure & (np.where(g < 0, -1.0, 1.0) != sign64) & (m > tol * scale)
    excess = np.where(wrong_sign, np.inf, excess)
    return float((excess / scale).max()) if excess.size else 0.0


def against_float64(out, ref, c, cn_type, tol, stage_one=True, cols=None):
    """A float32 BP4 result `out` (oracle or GPU, NumPy arrays) against bp4_decode64's `ref` with the bounds of the module docstring.
    `cols` (a boolean mask over the qubits) restricts the marginals and decisions; messages and soft syndromes are compared when `out`
    holds them.  Asserts every bound and returns the largest relative deviation of the marginals and messages."""
    cols = np.ones(ref["llr"].shape[2], bool) if cols is None else cols
    llr64 = ref["llr"][:, :, cols]
    sc = _scale(llr64)
    worst = float((np.abs(out["llr"][:, :, cols].astype(np.float64) - llr64) / sc).max())
    assert worst <= tol, ("llr", cn_type, worst)
    for k in ("msg_x", "msg_z"):
        if out.get(k) is not None and out[k].size:
            worst = max(worst, float((np.abs(out[k].astype(np.float64) - ref[k]) / _scale(ref[k])).max()))
            assert worst <= tol, (k, cn_type, worst)
    X, Y, Z = llr64[:, 0], llr64[:, 1], llr64[:, 2]
    s = np.sort(np.stack([np.zeros_like(X), X, Z, Y], 0), axis=0)
    firm = (s[1] - s[0]) > 2 * tol * sc[:, :, 0]
    for k in ("x_hat", "z_hat"):
        assert np.array_equal(out[k][:, cols][firm], ref[k][:, cols][firm]), (k, cn_type)
    dv = 2 * tol * _scale(ref["llr"])[:, :, 0]
    for k, rows, v in (("x_logit", _rows(c, stage_one)[0], ref["llr_x"]), ("z_logit", _rows(c, stage_one)[1], ref["llr_z"])):
        if out.get(k) is not None:
            ex = soft_syndrome_excess(rows, v, dv, out[k], tol)
            assert ex <= tol, (k, cn_type, ex)
    return worst


def compare(og, c, sx, sz, iters, cn_type, factor, tol, stage_one=True, cols=None, **kw):
    """The oracle and the restatement at each iteration count; returns the largest relative deviation."""
    worst = 0.0
    for it in iters:
        out = og.bp4_decode(sx, sz, it, cn_type, factor, return_msgs=True, **kw)
        ref = R.bp4_decode64(c, sx, sz, it, cn_type, factor, stage_one=stage_one, **kw)
        worst = max(worst, against_float64(out, ref, c, cn_type, tol, stage_one=stage_one, cols=cols))
    return worst


@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("cn_type", RULES)
def test_one_and_two_iterations_against_float64(name, cn_type):
    og, c = oracle_library_forms(name), code(name)
    B = 24
    sx, sz = syndromes(og, 0.05, B)
    iters = (1,) if name in OVERCOMPLETE else (1, 2)
    llr = channel(B, og.n, 3)
    for factor in FACTORS:
        compare(og, c, sx, sz, iters, cn_type, factor, tol_of(cn_type), llr_const=_llr_const(0.1))
        compare(og, c, sx, sz, iters, cn_type, factor, tol_of(cn_type), llr_ch=llr)


def random_messages(c, B, seed):
    """c->v messages (VN-major [B,E_x], [B,E_z]) of both signs in [-1.5, 1.5] with exact zeros (+0 and -0) among them, and +-20 on one edge
    of qubits no two of which share a check of that side, all of whose checks of that side have degree >= 3.  A +-20 makes its
    qubit's other v->c messages of that side saturate; one such input per check of degree >= 3 keeps float32 phi and tanh out of
    their saturation (a degree-2 check would pass the saturated value straight on: phi(phi(x)), or atanh of a product within ulps
    of 1).  Magnitudes up to 1.5 keep the totals, and with them the v->c messages, below ~10, where phi is well conditioned."""
    rng = np.random.RandomState(seed)
    out = []
    for pcm in (np.asarray(c.hx), np.asarray(c.hz)):
        var = R._bp4_side(pcm)["var"]
        wide = pcm.sum(1) >= 3
        first = np.searchsorted(var, np.arange(pcm.shape[1]))
        m = rng.uniform(-1.5, 1.5, size=(B, var.size)).astype(F32)
        k = rng.rand(B, var.size)
        m[k < 0.08] = 0.0
        m[(k >= 0.08) & (k < 0.16)] = -0.0
        for b in range(B):
            used = np.zeros(pcm.shape[0], bool)
            for v in rng.permutation(pcm.shape[1]):
                if pcm[:, v].any() and not (used & (pcm[:, v] != 0)).any() and wide[pcm[:, v] != 0].all():
                    used |= pcm[:, v] != 0
                    m[b, first[v] + rng.randint(pcm[:, v].sum())] = F32(20.0) * rng.choice([-1, 1])
        out.append(m)
    return out


@pytest.mark.parametrize("name", ("ghp882", "gb48", "rsurf5", "gb126"))
@pytest.mark.parametrize("cn_type", RULES)
def test_restart_from_messages(name, cn_type):
    """msg_init: the decoder restarted from given c->v messages (one iteration: nothing is amplified)."""
    og, c = oracle_library_forms(name), code(name)
    B = 16
    sx, sz = syndromes(og, 0.05, B)
    mi = random_messages(c, B, 8)
    assert (np.abs(mi[0]) == 20).any() and (mi[0] == 0).any() and (np.signbit(mi[0]) & (mi[0] == 0)).any()
    for factor in FACTORS:
        compare(og, c, sx, sz, (1,), cn_type, factor, tol_of(cn_type), llr_const=_llr_const(0.1), msg_init=mi)
        compare(og, c, sx, sz, (1,), cn_type, factor, tol_of(cn_type), llr_ch=channel(B, og.n, 4), msg_init=mi)
    # zero iterations hand the initial messages back unchanged
    out = og.bp4_decode(sx, sz, 0, cn_type, 0.8, llr_const=1.0, msg_init=mi, return_msgs=True)
    assert np.array_equal(out["msg_x"].view(np.int32), mi[0].view(np.int32))
    assert np.array_equal(out["msg_z"].view(np.int32), mi[1].view(np.int32))


@pytest.mark.parametrize("name", ("ghp882", "rsurf5", "gb126"))
@pytest.mark.parametrize("cn_type", RULES)
def test_both_qubit_update_forms(name, cn_type):
    """The literal (one log-sum-exp per edge) and the re-associated (its a - b part once per qubit and side) qubit updates are the same
    real function: both are held to the same float64 value within the same bound."""
    c = code(name)
    B = 16
    for og in (oracle_literal_forms(name), oracle_reassociated_forms(name)):
        sx, sz = syndromes(og, 0.05, B)
        for factor in (1.0, 0.625):
            compare(og, c, sx, sz, (1, 2), cn_type, factor, tol_of(cn_type), llr_const=_llr_const(0.1))
            compare(og, c, sx, sz, (1, 2), cn_type, factor, tol_of(cn_type), llr_ch=channel(B, og.n, 5))


@pytest.mark.parametrize("cn_type", RULES)
def test_non_stage_one_soft_syndromes(cn_type):
    """stage_one=False: the soft syndromes run over the dense hx_perp / hz_perp rows (decoding_q.py:33-34)."""
    name = "gb48"
    og, c = oracle_library_forms(name, stage_one=False), code(name)
    assert og.rows_xp == np.asarray(c.hx_perp).shape[0] and og.rows_zp == np.asarray(c.hz_perp).shape[0]
    B = 16
    sx, sz = syndromes(og, 0.05, B)
    for factor in FACTORS:
        compare(og, c, sx, sz, (0, 1, 2), cn_type, factor, tol_of(cn_type), stage_one=False, llr_const=_llr_const(0.1))
        compare(og, c, sx, sz, (1, 2), cn_type, factor, tol_of(cn_type), stage_one=False, llr_ch=channel(B, og.n, 6))


def converged(c, sx, sz, xh, zh):
    """The decision reproduces both syndromes: hx rows check z_hat, hz rows x_hat."""
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    return ((zh.astype(np.int64) @ hx.T % 2) == sx).all(1) & ((xh.astype(np.int64) @ hz.T % 2) == sz).all(1)


# (code, p, iterations): depolarizing noise at which most samples converge
MANY = [("ghp882", 0.03, 32), ("gb48", 0.03, 24), ("rsurf5", 0.03, 24), ("gb126", 0.02, 24)]


@pytest.mark.parametrize("name,p,iters", MANY)
@pytest.mark.parametrize("cn_type", ("minsum", "boxplus"))
def test_many_iterations_same_correction_class(name, p, iters, cn_type):
    """The bar of test_c_oracle_vs_numpy_restatement (tests/test_oracle_kat.py): over many iterations float32 rounding is amplified
    through the transient, so two faithful implementations can end a trapping-set sample on different sides of convergence.  On the
    samples BOTH converge the corrections must lie in the same class (hx_perp . (x_1 ^ x_2) = 0 and hz_perp . (z_1 ^ z_2) = 0, the
    residual test of feedback_gnn.py:352-353); convergence flips are counted, not compared, and the rates agree within a margin.
    Normalized min-sum (factor < 1) has no transcendentals in its check rule: its bar is three times tighter (flips 5 % rather than
    15 %, rates 2 % rather than 6 %) and every commonly converged sample must be in the same class."""
    c = code(name)
    og = oracle_library_forms(name)
    B = 96
    sx, sz = syndromes(og, p, B, first=77)
    L = _llr_const(p)
    for factor in FACTORS:
        o = og.bp4_decode(sx, sz, iters, cn_type, factor, llr_const=L)
        r = R.bp4_decode64(c, sx, sz, iters, cn_type, factor, llr_const=L)
        conv0, conv1 = converged(c, sx, sz, o["x_hat"], o["z_hat"]), converged(c, sx, sz, r["x_hat"], r["z_hat"])
        both, flipped = conv0 & conv1, conv0 ^ conv1
        assert both.sum() >= B // 2, "too few converged samples for the comparison to mean anything"
        exact = cn_type == "minsum" and factor != 1.0
        assert flipped.mean() <= (0.05 if exact else 0.15), (factor, flipped.mean())
        assert abs(conv0.mean() - conv1.mean()) <= (0.02 if exact else 0.06), (factor, conv0.mean(), conv1.mean())
        _, _, flags = og.residual(o["x_hat"], o["z_hat"], r["x_hat"], r["z_hat"])
        same_class = (flags & 2) == 0
        assert same_class[both].mean() >= (1.0 if exact else 0.98), (factor, same_class[both].mean())


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("gb48", "rsurf5", "gb126"))
def test_zero_channel_llrs(name, cn_type):
    """llr_const = 0: every qubit sends softplus(0) - logsumexp(0, 0) = 0, so min-sum meets exact ties at every check and the tanh rule
    its t == 0 guard (tanh(0) -> 1e-12, the product of a check's 1e-12 underflows, the 1e-7 zeroing sends exact zeros).  The phi rule
    meets phi at its lower clip: phi32(8.5e-8) = 16.635532 against 16.974 in float64, after which phi of the sum is 0 against 1.2e-7:
    within the floored bound."""
    og, c = oracle_library_forms(name), code(name)
    rng = np.random.RandomState(5)
    B = 16
    sx = rng.randint(0, 2, size=(B, og.m_x)).astype(np.uint8)
    sz = rng.randint(0, 2, size=(B, og.m_z)).astype(np.uint8)
    for factor in FACTORS:
        compare(og, c, sx, sz, (1, 2), cn_type, factor, tol_of(cn_type), llr_const=0.0)
    if cn_type != "boxplus-phi":  # exactly zero messages, exactly zero marginals
        out = og.bp4_decode(sx, sz, 2, cn_type, 0.8, llr_const=0.0, return_msgs=True)
        assert not out["llr"].any() and not out["msg_x"].any() and not out["msg_z"].any()


EDGE_LLRS = np.array([20.0, -20.0, 30.0, -30.0, 17.0, -17.0, np.nextafter(F32(16.635532), F32(0)), 16.635532, 0.0, -0.0, 1e-45,
                      -1e-45, np.finfo(F32).tiny, -np.finfo(F32).tiny], dtype=F32)


def edge_channel(c, B, seed):
    """Moderate per-qubit LLRs with the values of EDGE_LLRS on qubits no two of which share a check on either side (rotated through the
    batch and the three planes so that every value occurs in every plane): beyond phi's clip, one ulp below and at it, +-0, the
    smallest subnormal and the smallest normal magnitude.  One extreme per check, and only in checks of degree >= 3, keeps the float32
    phi and tanh out of their saturation in the check update (a degree-2 check passes a saturated input straight on: phi(phi(x)) at
    phi's clip, or atanh of a product within a few ulps of 1, where one ulp of the product moves the message by ~0.3)."""
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    n = hx.shape[1]
    rng = np.random.RandomState(seed)
    llr = channel(B, n, seed)
    wide_x, wide_z = hx.sum(1) >= 3, hz.sum(1) >= 3
    k = 0
    for b in range(B):
        used_x, used_z = np.zeros(hx.shape[0], bool), np.zeros(hz.shape[0], bool)
        for v in rng.permutation(n):
            if (not (used_x & (hx[:, v] != 0)).any() and not (used_z & (hz[:, v] != 0)).any() and wide_x[hx[:, v] != 0].all()
                    and wide_z[hz[:, v] != 0].all()):
                used_x |= hx[:, v] != 0
                used_z |= hz[:, v] != 0
                llr[b, k % 3, v] = EDGE_LLRS[(k // 3) % len(EDGE_LLRS)]
                k += 1
    return llr


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("ghp882", "gb48", "rsurf5"))
def test_saturating_channel_llrs(name, cn_type):
    og, c = oracle_library_forms(name), code(name)
    B = 16
    sx, sz = syndromes(og, 0.05, B)
    llr = edge_channel(c, B, 11)
    for factor in FACTORS:
        compare(og, c, sx, sz, (1,), cn_type, factor, tol_of(cn_type), llr_ch=llr)
    # zero iterations: the marginals are the channel LLRs (no input clip in QLDPCBPDecoder, :705-708 are commented out), Y = (0 + 0) + ly
    out = og.bp4_decode(sx, sz, 0, cn_type, 0.8, llr_ch=llr)
    assert np.array_equal(out["llr"], llr + F32(0))
    # every qubit saturated: every binary LLR is beyond phi's clip, phi32 of each is exactly 0, and every soft syndrome is
    # +-phi32(clip min) = +-16.635532 exactly; float64 sends +-phi(sum of the 2 exp(-|v|)), between 13 and 16.974: the documented gap
    sat = np.full((B, 3, og.n), 40.0, F32)
    sat[:, 1] = 45.0
    out = og.bp4_decode(sx, sz, 0, cn_type, 0.8, llr_ch=sat)
    ref = R.bp4_decode64(c, sx, sz, 0, cn_type, 0.8, llr_ch=sat)
    for k in ("x_logit", "z_logit"):
        assert (np.abs(out[k]) == PHI0_F32).all()
        assert np.array_equal(np.sign(out[k]), np.sign(ref[k]))
        assert (np.abs(ref[k]) > 13.0).all() and (np.abs(ref[k]) <= R._bp4_phi(0.0)).all()


def edge_check_degrees(pcm):
    """The degree of each VN-major edge's check."""
    pcm = np.asarray(pcm)
    chk, var = np.nonzero(pcm)
    return pcm.sum(1)[chk[np.lexsort((chk, var))]]


@pytest.mark.parametrize("cn_type", RULES)
@pytest.mark.parametrize("name", ("gb48", "rsurf5"))
def test_all_inputs_saturated(name, cn_type):
    """Every channel LLR at 40 (45 on Y): at one iteration every v->c message is ~40, beyond every rule's saturation.
    - Min-sum clips it to _llr_max = 20 and meets a tie at every check: the double-minimum detector must keep 20.
    - tanh: the clip 1 - 1e-7 is 0.99999988 in float32 (:49).  float64 tanh(20) is 1, so every message is 2 atanh(clip) = 16.6355.
      The library's float32 tanh stops one ulp short of 1 (1 - 2^-24, within its documented ulp bound), so the product of the other
      d - 1 inputs is (1 - 2^-24)^(d-1): at a degree-2 check above the clip (the same 16.6355, asserted exactly), at d >= 3 below
      it, 2 atanh of it up to the few ulps the quotient P / t rounds by (15.5 at d = 8): asserted as that interval.
    - phi(40) is exactly 0 in float32 and phi(16.635532) = 1.19e-7 in float64, so the phi rule sends phi32(0) = phi(clip min) =
      16.635532 against phi64((d - 1) 1.19e-7): the documented gap, asserted exactly."""
    og, c = oracle_library_forms(name), code(name)
    B = 8
    sx, sz = syndromes(og, 0.05, B)
    sat = np.full((B, 3, og.n), 40.0, F32)
    sat[:, 1] = 45.0
    for factor in FACTORS:
        out = og.bp4_decode(sx, sz, 1, cn_type, factor, llr_ch=sat, return_msgs=True)
        ref = R.bp4_decode64(c, sx, sz, 1, cn_type, factor, llr_ch=sat)
        fac = np.float64(F32(factor))
        for k, pcm in (("msg_x", c.hx), ("msg_z", c.hz)):
            d = edge_check_degrees(pcm)[None, :]
            assert np.array_equal(np.sign(out[k]), np.sign(ref[k]))
            m32, m64 = np.abs(out[k]).astype(np.float64), np.abs(ref[k])
            if cn_type == "minsum":
                assert (m32 == np.float64(F32(20) * F32(factor))).all() and np.allclose(m64, 20 * fac, rtol=1e-15)
            elif cn_type == "boxplus":
                assert np.allclose(m64, 2 * np.arctanh(R._ATANH_CLIP) * fac, rtol=1e-12)
                lo = 2 * np.arctanh(1.0 - 2 * d * 2.0 ** -24) * fac  # the quotient P / t within a few ulps of 1 - (d - 1) 2^-24
                assert (m32 >= lo - 1e-6).all() and (m32 <= m64 + 1e-6).all()
                assert (m32[np.broadcast_to(d == 2, m32.shape)] == np.float64(F32(2 * np.arctanh(R._ATANH_CLIP)) * F32(factor))).all()
            else:
                assert (m32 == np.float64(PHI0_F32 * F32(factor))).all()
                assert np.allclose(m64, R._bp4_phi((d - 1) * R._bp4_phi(PHI_HI)) * fac, rtol=1e-12)
        if cn_type == "minsum" and name == "gb48":
            against_float64(out, ref, c, cn_type, tol_of(cn_type))


@pytest.mark.parametrize("cn_type", RULES)
def test_all_ones_syndrome_and_zero_iterations(cn_type):
    name = "gb48"
    og, c = oracle_library_forms(name), code(name)
    B = 8
    sx, sz = np.ones((B, og.m_x), np.uint8), np.ones((B, og.m_z), np.uint8)
    for factor in FACTORS:
        compare(og, c, sx, sz, (0, 1, 2), cn_type, factor, tol_of(cn_type), llr_const=_llr_const(0.1))
        compare(og, c, sx, sz, (1, 2), cn_type, factor, tol_of(cn_type), llr_ch=channel(B, og.n, 4))
    out = og.bp4_decode(sx, sz, 0, cn_type, 0.8, llr_const=-1.5, return_msgs=True)
    assert (out["llr"] == F32(-1.5)).all() and not out["msg_x"].any() and not out["msg_z"].any()
    assert (out["x_hat"] == 1).all() and (out["z_hat"] == 0).all()  # argmin([0, X, Z, Y]) with X = Y = Z < 0: the first, X


def bare_code():
    """hx [7,12] with a degree-1 check (row 0: min-sum's min2 = LARGE + min path, the phi rule's T - a = 0), a degree-2 check and
    irregular degrees; hz [5,12] leaves qubits 0-3 without an hz edge and qubit 11 has no hx edge."""
    hx = np.zeros((7, 12), np.int64)
    hx[0, 3] = 1
    hx[1, [0, 5]] = 1
    for r, cols in ((2, [0, 1, 2, 4]), (3, [1, 3, 6, 7, 8]), (4, [2, 5, 9]), (5, [4, 6, 8, 9, 10]), (6, [0, 7, 10, 3, 1, 2])):
        hx[r, cols] = 1
    hz = np.zeros((5, 12), np.int64)
    for r, cols in ((0, [4, 5]), (1, [5, 6, 7, 11]), (2, [8, 9]), (3, [9, 10, 11, 4]), (4, [6, 8, 10])):
        hz[r, cols] = 1
    zero = np.zeros((1, 12), np.int64)
    return types.SimpleNamespace(hx=hx, hz=hz, hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)


@pytest.mark.parametrize("cn_type", RULES)
def test_degree_one_check_and_one_sided_qubits(cn_type):
    """A degree-1 check sends phi(T - a) = phi(0) under the phi rule: phi at its lower clip, 16.635532 in float32 against 16.974 in
    float64.  That gap is the reference's own float32 value, so under phi the message of the degree-1 check is held to it exactly (times
    the factor), and the qubit it enters (qubit 3) and the soft syndromes are left out of the point comparison, at one iteration."""
    c = bare_code()
    og = OracleGraph(c, forms="literal")
    assert og.E_x == 26 and int(np.asarray(c.hz).sum(0)[:4].max()) == 0 and int(np.asarray(c.hx).sum(0)[11]) == 0
    rng = np.random.RandomState(9)
    B = 32
    sx = rng.randint(0, 2, size=(B, 7)).astype(np.uint8)
    sz = rng.randint(0, 2, size=(B, 5)).astype(np.uint8)
    phi = cn_type == "boxplus-phi"
    cols = np.arange(12) != 3 if phi else None
    e3 = int(np.flatnonzero(R._bp4_side(c.hx)["var"] == 3)[0])  # VN-major slot of the edge (check 0, qubit 3): qubit 3's first check
    keep = np.arange(og.E_x) != e3
    for factor in FACTORS:
        for llr in (dict(llr_const=_llr_const(0.1)), dict(llr_ch=channel(B, 12, 6))):
            for it in ((1,) if phi else (1, 2)):
                out = og.bp4_decode(sx, sz, it, cn_type, factor, return_msgs=True, **llr)
                ref = R.bp4_decode64(c, sx, sz, it, cn_type, factor, **llr)
                if phi:
                    gap = (R._bp4_phi(0.0) - np.float64(PHI0_F32)) * np.float64(F32(factor))
                    assert np.abs(np.abs(out["msg_x"][:, e3] - ref["msg_x"][:, e3]) - gap).max() <= SOFT_TOL * 17
                    assert (np.abs(out["msg_x"][:, e3]) == PHI0_F32 * F32(factor)).all()
                    out = dict(out, msg_x=out["msg_x"][:, keep], x_logit=None, z_logit=None)
                    ref = dict(ref, msg_x=ref["msg_x"][:, keep])
                against_float64(out, ref, c, cn_type, tol_of(cn_type), cols=cols)
    out = og.bp4_decode(sx, sz, 2, cn_type, 0.8, llr_const=-1.5)
    assert (out["llr"][:, 0, :4] == F32(-1.5)).all()  # no hz edge: X = 0 + llr_x exactly
    assert (out["llr"][:, 2, 11] == F32(-1.5)).all()  # no hx edge: Z = 0 + llr_z exactly
