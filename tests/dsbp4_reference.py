"""Soft-syndrome BP4 (fgnn_dsbp4_decode, include/fgnn.h) restated in NumPy float32.

The qubit update, totals, decisions and attempt control are those of tests/mbp4_reference.py (`Graph`, `decisions`, `mbp4_tables`).
The soft check rule is written out here per rule, every float operation in the order of feedback_gnn_amd/csrc/fgnn_cn.h, on
float32 arrays (NumPy rounds every elementwise float32 operation once and never fuses two of them) and on the oracle's
transcendentals (`math_apply`): a check with d edges is the rule of that cn_type on the d + 1 inputs (nu_1, .., nu_d, gamma) in that
order; outputs 1 .. d times the factor are the c->v messages, output d + 1 times the factor is w_c, Gamma_c = gamma_c + w_c is one add
and u_hat_c = Gamma_c < 0.  tests/test_dsbp4_reference_cpu.py ties the rule to `mbp4_reference.cn_update` on [h | I], to the host build
of the header, and the decoder to `mbp4_reference.mbp4_decode`."""
import numpy as np

import mbp4_reference as MB
from mbp4_reference import F32, _f, with_sign
from oracle.oracle import math_apply

CN_TYPES = MB.CN_TYPES
INF = float("inf")


def soft_rule(v, mask, synd, gamma, cn_type, factor):
    """One soft check per row.  v [R,D] float32 inputs (entry j takes part where mask [R,D]), synd [R] bits, gamma [R] float32, factor a
    float32 scalar or [R].  Returns (out [R,D] float32, zero where masked off, and w [R] float32)."""
    v, gamma = _f(np.ascontiguousarray(v)), _f(np.ascontiguousarray(gamma))
    R, D = v.shape
    mask = np.broadcast_to(mask, v.shape)
    synd = np.asarray(synd).astype(bool)
    factor = np.asarray(factor, F32)
    fcol = factor[:, None] if factor.ndim else factor
    deg0 = ~mask.any(1)
    if cn_type == "boxplus-phi":
        ng = (v < 0) & mask
        neg = synd ^ (ng.sum(1) % 2).astype(bool)
        a = math_apply("phi", np.abs(v))
        T = np.zeros(R, F32)
        for j in range(D):
            T = np.where(mask[:, j], _f(T + a[:, j]), T)
        ngg = gamma < 0
        neg = neg ^ ngg
        ag = math_apply("phi", np.abs(gamma))
        T = _f(T + ag)
        o = math_apply("phi", _f(T[:, None] - a))
        out = _f(with_sign(o, neg[:, None] ^ ng) * fcol)
        w = _f(with_sign(math_apply("phi", _f(T - ag)), neg ^ ngg) * factor)
    elif cn_type == "minsum":
        LARGE = F32(10000.0)
        vc = np.minimum(np.maximum(v, F32(-20.0)), F32(20.0))
        ng = (vc < 0) & mask
        neg = synd ^ (ng.sum(1) % 2).astype(bool)
        a = np.abs(vc)
        vg = np.minimum(np.maximum(gamma, F32(-20.0)), F32(20.0))
        ngg = vg < 0
        neg = neg ^ ngg
        ag = np.abs(vg)
        minv = np.minimum(np.where(mask, a, F32(np.inf)).min(1), ag).astype(F32)
        d = _f(a - minv[:, None])
        d = np.where(d == 0, LARGE, d)
        dg = _f(ag - minv)
        dg = np.where(dg == 0, LARGE, dg)
        min2 = np.minimum(np.where(mask, d, F32(np.inf)).min(1), dg).astype(F32)
        nsum = np.zeros(R, F32)
        for j in range(D):
            nsum = np.where(mask[:, j], _f(nsum + d[:, j]), nsum)
        nsum = _f(nsum + dg)
        min2 = _f(min2 + minv)
        nsum = _f(nsum - F32(F32(2.0) * LARGE - F32(1.0)))
        sg = np.where(nsum > 0, F32(1.0), np.where(nsum < 0, F32(-1.0), F32(0.0))).astype(F32)
        dm = _f(F32(0.5) * _f(F32(1.0) - sg))
        min_e = _f(_f(_f(F32(1.0) - dm) * minv) + _f(dm * min2))
        o = np.where(_f(a - minv[:, None]) == 0, min_e[:, None], minv[:, None]).astype(F32)
        out = _f(with_sign(o, neg[:, None] ^ ng) * fcol)
        og = np.where(_f(ag - minv) == 0, min_e, minv).astype(F32)
        w = _f(with_sign(og, neg ^ ngg) * factor)
    else:  # boxplus
        t = np.zeros_like(v)
        P = np.ones(R, F32)
        for j in range(D):
            tj = math_apply("tanh", _f(v[:, j] / F32(2.0)))
            tj = np.where(tj == 0, F32(1e-12), tj).astype(F32)
            t[:, j] = tj
            P = np.where(mask[:, j], tj if j == 0 else _f(P * tj), P)
        tg = math_apply("tanh", _f(gamma / F32(2.0)))
        tg = np.where(tg == 0, F32(1e-12), tg).astype(F32)
        P = np.where(deg0, tg, _f(P * tg))
        P = _f(P * np.where(synd, F32(-1.0), F32(1.0)).astype(F32))
        clipv = F32(0.99999988)

        def back(tt, PP):
            with np.errstate(invalid="ignore"):
                q = _f(math_apply("rcp_unit", tt) * PP)
            q = np.where(np.abs(q) < F32(1e-7), F32(0.0), q).astype(F32)
            # fmax / fmin: where a subnormal input made 1 / t infinite and the product had underflowed, q is 0 * inf, and both
            # v_max_f32 and the host's (q > lo ? q : lo) return the other operand
            with np.errstate(invalid="ignore"):
                return np.fmin(np.fmax(q, -clipv), clipv)

        out = _f(_f(F32(2.0) * math_apply("atanh", back(np.where(mask, t, F32(1.0)), P[:, None]))) * fcol)
        w = _f(_f(F32(2.0) * math_apply("atanh", back(tg, P))) * factor)
    return np.where(mask, out, F32(0.0)).astype(F32), w


def soft_cn_update(side, nu, synd, gamma, cn_type, factor):
    """The soft rule on every check of one side: nu [B,E] v->c messages, synd [B,m] bits, gamma [B,m] float32.  Returns the c->v
    messages [B,E] and w [B,m]."""
    B = nu.shape[0]
    tab, mask = side.cn_tab, side.cn_mask
    D = tab.shape[1]
    v = nu[:, tab].reshape(B * side.m, D)
    out, w = soft_rule(v, np.tile(mask, (B, 1)), np.asarray(synd).reshape(-1), _f(gamma).reshape(-1), cn_type, F32(factor))
    out = out.reshape(B, side.m, D)
    mu = np.zeros_like(nu)
    mu[np.arange(B)[:, None], tab[mask][None, :]] = out[:, mask]
    return mu, w.reshape(B, side.m)


def u_hat_of(gamma, w):
    """Gamma = gamma + w (one float32 add); u_hat = Gamma < 0."""
    return (_f(_f(gamma) + w) < 0).astype(np.uint8)


def gammas(B, m, arr, scalar):
    """The [B,m] float32 syndrome LLRs of one side: the array, or the scalar for every check."""
    if arr is not None:
        arr = np.asarray(arr, F32)
        assert arr.shape == (B, m), arr.shape
        return arr.copy()
    assert not np.isnan(scalar)
    return np.full((B, m), F32(scalar), F32)


def dsbp4_decode(code, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None, llr_const=0.0,
                 synd_llr_x=None, synd_llr_z=None, gamma_x=INF, gamma_z=INF):
    """`code`: an object with hx and hz.  Returns (x_hat [B,n], z_hat [B,n], u_x_hat [B,m_x], u_z_hat [B,m_z] uint8, stats [B,4] int32 =
    found, the a of the last test, iterations, the k of the last test)."""
    assert cn_type in CN_TYPES and len(factors) == len(owns) >= 1
    G = MB.graph_of(code)
    n = G.n
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B = synd_x.shape[0]
    gx, gz = gammas(B, G.x.m, synd_llr_x, gamma_x), gammas(B, G.z.m, synd_llr_z, gamma_z)
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    mux, muz = np.zeros((B, G.x.E), F32), np.zeros((B, G.z.E), F32)
    hard = np.zeros((B, n), np.uint8)
    ux, uz = np.zeros((B, G.x.m), np.uint8), np.zeros((B, G.z.m), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for a in range(len(factors)):
        T = pre_iter if a == 0 else attempt_iter
        if restart and a > 0:
            mux[:], muz[:] = 0, 0
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            nux, nuz = G.qubit_update(mux[idx], muz[idx], lam[idx], F32(owns[a]))
            mux[idx], wx = soft_cn_update(G.x, nux, synd_x[idx], gx[idx], cn_type, F32(factors[a]))
            muz[idx], wz = soft_cn_update(G.z, nuz, synd_z[idx], gz[idx], cn_type, F32(factors[a]))
            dn = MB.decisions(*G.totals(mux[idx], muz[idx], lam[idx]))
            uxk, uzk = u_hat_of(gx[idx], wx), u_hat_of(gz[idx], wz)
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ G.hz.T) % 2 == (synd_z[idx] ^ uzk)).all(1) & ((z @ G.hx.T) % 2 == (synd_x[idx] ^ uxk)).all(1)
            hard[idx], ux[idx], uz[idx] = dn, uxk, uzk
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), ux, uz, stats


def joint_test(code, x_hat, z_hat, u_x_hat, u_z_hat, synd_x, synd_z):
    """[B] bool: H e_hat == s ^ u_hat on both graphs, with integer matrices."""
    hx, hz = np.asarray(code.hx, np.int64) % 2, np.asarray(code.hz, np.int64) % 2
    return ((x_hat.astype(np.int64) @ hz.T) % 2 == (synd_z ^ u_z_hat)).all(1) & ((z_hat.astype(np.int64) @ hx.T) % 2 == (synd_x ^ u_x_hat)).all(1)


def dsbp4_lds_bytes(E, n, m, cpb):
    """fgnn_dsbp4_decode: E messages, n decision bytes and m u_hat bytes per codeword, each rounded up to 4 floats; the two 64-float
    tables, a stamp per codeword and ndone."""
    area = lambda x: ((x + 3) // 4 + 3) & ~3  # noqa: E731
    per_cw = ((E + 3) & ~3) + area(n) + area(m)
    return per_cw * 4 * cpb + 2 * 64 * 4 + ((cpb + 1 + 3) & ~3) * 4
