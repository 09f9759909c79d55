"""Binary BP in the layered (serial) schedule (fgnn_bp2_decode_layered, include/fgnn.h) restated in NumPy float32, vectorised over the
batch — what the kernel is held to bit for bit.

Every intermediate is np.float32 (NumPy rounds every elementwise float32 operation once, to nearest even, and never fuses two of them).
The slot order is the library's (`relay_reference._Graph`: slots sorted by bit, then check; a check's loops ascend over its bits).  The
min-sum rule is `mbp4_reference.cn_update` unchanged; the phi rule has that function's structure with the phi of the binary kernels,
`math_apply("phi_gnn", .)` (PhiGnn of fgnn_cn.h: log(exp(x) + 1) - log(exp(x) - 1)) where it calls "phi"; the tanh rule has its
structure with the device's clip of a NaN quotient, which only a denormal prior can produce (`_tanh_rule`).  Every transcendental is
the oracle's: `math_apply` evaluates the shared routines of fgnn_math.h, compiled by gcc.

The schedule is the accumulator form: per codeword the messages mu_e and the running posteriors P_v; a check of the layer forms
nu_e = P_v - mu_e on its edges, the rule gives the new mu_e, and P_v = nu_e + mu_e.  The checks of a layer share no bit, so a layer is
one vectorised step.  Samples are independent: with `stop` a sample that has reproduced its syndrome leaves the batch."""
import types

import numpy as np

import mbp4_reference as MB
from oracle.oracle import math_apply
from relay_reference import _Graph

F32 = np.float32


# ---- layers of one matrix -----------------------------------------------------------------------------------------------------------
def greedy_bit_layers(hx):
    """(num_layers, layer_of [m] int32): checks in ascending number, each into the lowest layer that holds no check sharing a bit."""
    hx = np.asarray(hx) != 0
    m, n = hx.shape
    at = [set() for _ in range(n)]  # the layers that hold a check of bit v
    layer_of = np.zeros(m, np.int32)
    num = 0
    for c in range(m):
        bits = np.nonzero(hx[c])[0]
        taken = set().union(*[at[v] for v in bits]) if len(bits) else set()
        l = 0
        while l in taken:
            l += 1
        num = max(num, l + 1)
        layer_of[c] = l
        for v in bits:
            at[v].add(l)
    return num, layer_of


def is_valid_bit_layering(hx, num_layers, layer_of):
    """Values in [0, num_layers), no layer empty, no two checks of a layer share a bit."""
    hx = (np.asarray(hx) != 0).astype(np.int64)
    lay = np.asarray(layer_of)
    if lay.shape != (hx.shape[0],) or num_layers < 1 or lay.min() < 0 or lay.max() >= num_layers:
        return False
    if len(np.unique(lay)) != num_layers:
        return False
    return all(hx[lay == l].sum(0).max() <= 1 for l in range(num_layers))


# ---- the check rules ----------------------------------------------------------------------------------------------------------------
def _phi_rule(side, nu, synd, factor):
    """cn_update<FGNN_CN_BOXPLUS_PHI, PhiGnn> (fgnn_cn.h): the structure of mbp4_reference.cn_update's phi branch, on phi_gnn; the
    parked word with_sign(phi(|v|), v < 0) is read back as the kernel reads it (its magnitude, its sign bit)."""
    B = nu.shape[0]
    tab, mask = side.cn_tab, side.cn_mask
    D = tab.shape[1]
    v = nu[:, tab]
    factor = F32(factor)
    neg = synd.astype(bool).copy()
    T = np.zeros((B, side.m), F32)
    a = np.zeros_like(v)
    ng = np.zeros(v.shape, bool)
    for j in range(D):
        mj = mask[:, j]
        ng[:, :, j] = (v[:, :, j] < 0) & mj
        neg ^= ng[:, :, j]
        a[:, :, j] = math_apply("phi_gnn", np.abs(v[:, :, j]))
        T = np.where(mj, MB._f(T + a[:, :, j]), T)
    out = np.zeros_like(v)
    for j in range(D):
        o = math_apply("phi_gnn", MB._f(T - np.abs(a[:, :, j])))
        out[:, :, j] = MB._f(MB.with_sign(o, neg ^ ng[:, :, j] ^ np.signbit(a[:, :, j])) * factor)
    mu = np.zeros_like(nu)
    mu[np.arange(B)[:, None], tab[mask][None, :]] = out[:, mask]
    return mu


def _tanh_rule(side, nu, synd, factor):
    """cn_update<FGNN_CN_BOXPLUS> (fgnn_cn.h): mbp4_reference.cn_update's tanh branch with one difference, the clip of the quotient.
    The binary decoder hands a prior straight to the rule, and a denormal prior makes t = tanh(nu / 2) denormal: 1 / t is inf, the
    product of the check's t may underflow to 0, and inf * 0 is NaN.  The kernel clips with FG_MAX / FG_MIN, on the device fmaxf /
    fminf, which return the operand that is a number (here -clipv); np.maximum / np.minimum would hand the NaN on.  np.fmax / np.fmin
    are that pair.  Without a NaN the two branches agree bit for bit."""
    B = nu.shape[0]
    tab, mask = side.cn_tab, side.cn_mask
    D = tab.shape[1]
    v = nu[:, tab]
    factor = F32(factor)
    t = np.zeros_like(v)
    P = np.ones((B, side.m), F32)
    for j in range(D):
        tj = math_apply("tanh", MB._f(v[:, :, j] / F32(2.0)))
        tj = np.where(tj == 0, F32(1e-12), tj).astype(F32)
        t[:, :, j] = tj
        P = np.where(mask[:, j], tj if j == 0 else MB._f(P * tj), P)
    P = MB._f(P * np.where(synd.astype(bool), F32(-1.0), F32(1.0)).astype(F32))
    clipv = F32(0.99999988)
    with np.errstate(invalid="ignore"):
        q = MB._f(math_apply("rcp_unit", np.where(mask, t, F32(1.0))) * P[:, :, None])
        q = np.where(np.abs(q) < F32(1e-7), F32(0.0), q).astype(F32)
    q = np.fmin(np.fmax(q, -clipv), clipv)
    out = MB._f(MB._f(F32(2.0) * math_apply("atanh", q)) * factor)
    mu = np.zeros_like(nu)
    mu[np.arange(B)[:, None], tab[mask][None, :]] = out[:, mask]
    return mu


def cn_rule(side, nu, synd, cn_type, factor):
    """The c->v messages [B,E] of the checks of `side` (zeros elsewhere) from nu [B,E] and their syndrome bits [B, side.m]."""
    if cn_type == "boxplus-phi":
        return _phi_rule(side, nu, synd, factor)
    if cn_type == "boxplus":
        return _tanh_rule(side, nu, synd, factor)
    return MB.cn_update(side, nu, synd, cn_type, factor)


class _Layers:
    """The checks of every layer as the padded tables cn_update reads, with the layer's slots and their bits."""

    def __init__(self, G, num_layers, layer_of):
        self.sides = []
        for l in range(num_layers):
            chk = np.nonzero(np.asarray(layer_of) == l)[0]
            tab = G.chk_slots[chk]
            mask = tab >= 0
            slots = tab[mask]
            self.sides.append(types.SimpleNamespace(m=len(chk), chk=chk, cn_tab=np.maximum(tab, 0), cn_mask=mask, slots=slots,
                                                    bits=G.slot_bit[slots]))


def parity_ok(hx, d, synd):
    """[B] bool: H d == s."""
    return ((np.asarray(d).astype(np.int64) @ (np.asarray(hx) != 0).astype(np.int64).T) % 2 == (np.asarray(synd) & 1)).all(1)


def bp2_layered_decode(hx, synd, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0, B=None, layer_of=None,
                       stop=False):
    """Returns (soft [B,n] float32, hard [B,n] uint8, stats [B,2] int32 = (H hard == s, iterations run)).  layer_of None: greedy."""
    assert cn_type in MB.CN_TYPES
    G = _Graph(hx)
    if synd is None:
        B = llr_ch.shape[0] if B is None else B
        synd = np.zeros((B, G.m), np.uint8)
    synd = np.asarray(synd, np.uint8) & 1
    B = synd.shape[0]
    if layer_of is None:
        num_layers, layer_of = greedy_bit_layers(hx)
    else:
        layer_of = np.asarray(layer_of, np.int32)
        num_layers = int(layer_of.max()) + 1
        assert is_valid_bit_layering(hx, num_layers, layer_of)
    lay = _Layers(G, num_layers, layer_of)
    llr = np.asarray(llr_ch, F32) if llr_ch is not None else np.full((B, G.n), F32(llr_const), F32)
    L = F32(-1.0) * np.minimum(np.maximum(llr, F32(-20.0)), F32(20.0))
    P = MB._f(L + F32(0.0))
    mu = np.zeros((B, G.E), F32)
    run = np.ones(B, bool)
    it_run = np.zeros(B, np.int32)
    for it in range(1, int(num_iter) + 1):
        idx = np.nonzero(run)[0]
        if len(idx) == 0:
            break
        Pi, mi, si = P[idx], mu[idx], synd[idx]
        for side in lay.sides:
            nu = MB._f(Pi[:, side.bits] - mi[:, side.slots])
            nu_all = np.zeros_like(mi)
            nu_all[:, side.slots] = nu
            new = cn_rule(side, nu_all, si[:, side.chk], cn_type, factor)[:, side.slots]
            mi[:, side.slots] = new
            Pi[:, side.bits] = MB._f(nu + new)
        P[idx], mu[idx] = Pi, mi
        it_run[idx] = it
        if stop:
            run[idx[parity_ok(hx, Pi < 0, si)]] = False
    soft = MB._f(F32(-1.0) * P)
    hard = (F32(0.0) < soft).astype(np.uint8)
    stats = np.stack([parity_ok(hx, hard, synd).astype(np.int32), it_run], axis=1).astype(np.int32)
    return soft, hard, stats


def unsolved(hx, synd, hard):
    """Samples whose decision does not reproduce the syndrome."""
    return int((~parity_ok(hx, hard, synd)).sum())
