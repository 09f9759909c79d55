"""Space-time BP4 (fgnn_stbp4_decode, include/fgnn.h) restated in NumPy float32.

The qubit update, totals, decisions and attempt control are those of tests/mbp4_reference.py (`Graph`, `decisions`), walked as
tests/dsbp4_reference.py walks them.  The check rule with one or two time-like inputs and the time variable rule are written out here
per rule, every float operation in the order of feedback_gnn_amd/csrc/fgnn_cn.h, on float32 arrays and on the oracle's
transcendentals (`math_apply`): check (c,t) with d edges is the rule of that cn_type on the inputs (nu_1, .., nu_d, b) for t = 0 and
(nu_1, .., nu_d, a, b) for t >= 1, in that order.  tests/test_stbp4_reference_cpu.py ties the rule to `mbp4_reference.cn_update` on
[h | I | I], to `dsbp4_reference.soft_rule` with one extra input, to the host build of the header, and the decoder with R = 1 to
`dsbp4_reference.dsbp4_decode`.  `sliding_decode` restates the window loop of `BP4_Phenomenological_Model`."""
import numpy as np

import mbp4_reference as MB
from mbp4_reference import F32, _f, with_sign
from oracle.oracle import math_apply

CN_TYPES = MB.CN_TYPES
INF = float("inf")


def st_rule(v, mask, synd, xs, cn_type, factor):
    """One check per row.  v [N,D] float32 edge inputs (entry j takes part where mask [N,D]), synd [N] bits, xs = the one or two extra
    inputs in order, each [N] float32, factor a float32 scalar or [N].  Returns (out [N,D] float32, zero where masked off, and the
    outputs for the extra inputs, a list of [N] float32)."""
    v = _f(np.ascontiguousarray(v))
    xs = [_f(np.ascontiguousarray(x)) for x in xs]
    assert len(xs) in (1, 2)
    N, D = v.shape
    mask = np.broadcast_to(mask, v.shape)
    synd = np.asarray(synd).astype(bool)
    factor = np.asarray(factor, F32)
    fcol = factor[:, None] if factor.ndim else factor
    deg0 = ~mask.any(1)
    if cn_type == "boxplus-phi":
        ng = (v < 0) & mask
        neg = synd ^ (ng.sum(1) % 2).astype(bool)
        a = math_apply("phi", np.abs(v))
        T = np.zeros(N, F32)
        for j in range(D):
            T = np.where(mask[:, j], _f(T + a[:, j]), T)
        ngx, ax = [], []
        for x in xs:
            ngx.append(x < 0)
            neg = neg ^ ngx[-1]
            ax.append(math_apply("phi", np.abs(x)))
            T = _f(T + ax[-1])
        o = math_apply("phi", _f(T[:, None] - a))
        out = _f(with_sign(o, neg[:, None] ^ ng) * fcol)
        ws = [_f(with_sign(math_apply("phi", _f(T - ae)), neg ^ ne) * factor) for ae, ne in zip(ax, ngx)]
    elif cn_type == "minsum":
        LARGE = F32(10000.0)
        vc = np.minimum(np.maximum(v, F32(-20.0)), F32(20.0))
        ng = (vc < 0) & mask
        neg = synd ^ (ng.sum(1) % 2).astype(bool)
        a = np.abs(vc)
        minv = np.where(mask, a, F32(np.inf)).min(1).astype(F32)
        ngx, ax = [], []
        for x in xs:
            vg = np.minimum(np.maximum(x, F32(-20.0)), F32(20.0))
            ngx.append(vg < 0)
            neg = neg ^ ngx[-1]
            ax.append(np.abs(vg))
            minv = np.minimum(minv, ax[-1]).astype(F32)
        d = _f(a - minv[:, None])
        d = np.where(d == 0, LARGE, d)
        min2 = np.where(mask, d, F32(np.inf)).min(1).astype(F32)
        nsum = np.zeros(N, F32)
        for j in range(D):
            nsum = np.where(mask[:, j], _f(nsum + d[:, j]), nsum)
        for ae in ax:
            dg = _f(ae - minv)
            dg = np.where(dg == 0, LARGE, dg)
            min2 = np.minimum(min2, dg).astype(F32)
            nsum = _f(nsum + dg)
        min2 = _f(min2 + minv)
        nsum = _f(nsum - F32(F32(2.0) * LARGE - F32(1.0)))
        sg = np.where(nsum > 0, F32(1.0), np.where(nsum < 0, F32(-1.0), F32(0.0))).astype(F32)
        dm = _f(F32(0.5) * _f(F32(1.0) - sg))
        min_e = _f(_f(_f(F32(1.0) - dm) * minv) + _f(dm * min2))
        o = np.where(_f(a - minv[:, None]) == 0, min_e[:, None], minv[:, None]).astype(F32)
        out = _f(with_sign(o, neg[:, None] ^ ng) * fcol)
        ws = [_f(with_sign(np.where(_f(ae - minv) == 0, min_e, minv).astype(F32), neg ^ ne) * factor) for ae, ne in zip(ax, ngx)]
    else:  # boxplus
        t = np.zeros_like(v)
        P = np.ones(N, F32)
        for j in range(D):
            tj = math_apply("tanh", _f(v[:, j] / F32(2.0)))
            tj = np.where(tj == 0, F32(1e-12), tj).astype(F32)
            t[:, j] = tj
            P = np.where(mask[:, j], tj if j == 0 else _f(P * tj), P)
        tx = []
        for e, x in enumerate(xs):
            tg = math_apply("tanh", _f(x / F32(2.0)))
            tg = np.where(tg == 0, F32(1e-12), tg).astype(F32)
            P = np.where(deg0, tg, _f(P * tg)) if e == 0 else _f(P * tg)
            tx.append(tg)
        P = _f(P * np.where(synd, F32(-1.0), F32(1.0)).astype(F32))
        clipv = F32(0.99999988)

        def back(tt, PP):
            with np.errstate(invalid="ignore"):
                q = _f(math_apply("rcp_unit", tt) * PP)
            q = np.where(np.abs(q) < F32(1e-7), F32(0.0), q).astype(F32)
            with np.errstate(invalid="ignore"):  # fmax / fmin: 0 * inf, as dsbp4_reference.soft_rule
                return np.fmin(np.fmax(q, -clipv), clipv)

        out = _f(_f(F32(2.0) * math_apply("atanh", back(np.where(mask, t, F32(1.0)), P[:, None]))) * fcol)
        ws = [_f(_f(F32(2.0) * math_apply("atanh", back(tg, P))) * factor) for tg in tx]
    return np.where(mask, out, F32(0.0)).astype(F32), ws


def st_cn_update(side, nu, synd, xs, cn_type, factor):
    """The rule on every check of one side: nu [N,E] v->c messages, synd [N,m] bits, xs = one or two [N,m] float32 extra inputs.
    Returns the c->v messages [N,E] and the outputs for the extra inputs, each [N,m]."""
    N = nu.shape[0]
    tab, mask = side.cn_tab, side.cn_mask
    D = tab.shape[1]
    v = nu[:, tab].reshape(N * side.m, D)
    out, ws = st_rule(v, np.tile(mask, (N, 1)), np.asarray(synd).reshape(-1), [_f(x).reshape(-1) for x in xs], cn_type, F32(factor))
    out = out.reshape(N, side.m, D)
    mu = np.zeros_like(nu)
    mu[np.arange(N)[:, None], tab[mask][None, :]] = out[:, mask]
    return mu, [w.reshape(N, side.m) for w in ws]


def window_gammas(B, R, m, arr, scalar, scalar_last):
    """The [B,R,m] float32 syndrome LLRs of one side: the array, or the scalar for rounds 0 .. R-2 and the last round's own."""
    if arr is not None:
        arr = np.asarray(arr, F32)
        assert arr.shape == (B, R, m), arr.shape
        return arr.copy()
    assert not np.isnan(scalar) and not np.isnan(scalar_last)
    g = np.full((B, R, m), F32(scalar), F32)
    g[:, R - 1] = F32(scalar_last)
    return g


def differences(s, prev):
    """d_0 = s_0 ^ prev, d_t = s_t ^ s_{t-1}; s [B,R,m] bits, prev [B,m] bits or None."""
    s = np.asarray(s, np.uint8) & 1
    before = np.zeros_like(s)
    before[:, 1:] = s[:, :-1]
    if prev is not None:
        before[:, 0] = np.asarray(prev, np.uint8) & 1
    return s ^ before


class _SideState:
    """One side of a window: messages mu [B,R,E], check outputs w_dn [B,R,m] and w_up [B,R,m] (w_up[:,t] is the output of check (c,t)
    towards time variable (c,t-1); row 0 stays zero and is never read), syndrome LLRs g and differences d."""

    def __init__(self, side, g, d):
        B, R, _ = g.shape
        self.side, self.g, self.d, self.R = side, g, d, R
        self.mu = np.zeros((B, R, side.E), F32)
        self.wdn, self.wup = np.zeros((B, R, side.m), F32), np.zeros((B, R, side.m), F32)

    def zero(self):
        self.mu[:], self.wdn[:], self.wup[:] = 0, 0, 0

    def time_messages(self, idx):
        """(a [N,R,m] with a[:,t] the message into check (c,t) from time variable (c,t-1), row 0 unused; b [N,R,m])."""
        g, wdn, wup, R = self.g[idx], self.wdn[idx], self.wup[idx], self.R
        s1 = _f(g + wdn)
        a = np.zeros_like(g)
        a[:, 1:] = s1[:, :-1]
        b = g.copy()  # the last round: gamma itself, no add
        b[:, :R - 1] = _f(g[:, :R - 1] + wup[:, 1:])
        return a, b

    def check_update(self, idx, nu, cn_type, factor):
        """nu [N,R,E]: the v->c messages of every round.  Writes mu, w_dn, w_up of the samples idx."""
        N, R, side = len(idx), self.R, self.side
        a, b = self.time_messages(idx)
        d = self.d[idx]
        mu, wdn, wup = np.zeros_like(nu), np.zeros_like(b), np.zeros_like(b)
        mu[:, 0], (wdn[:, 0],) = st_cn_update(side, nu[:, 0], d[:, 0], [b[:, 0]], cn_type, factor)
        if R > 1:
            flat = lambda x: np.ascontiguousarray(x[:, 1:]).reshape(N * (R - 1), -1)  # noqa: E731
            m1, (u1, d1) = st_cn_update(side, flat(nu), flat(d), [flat(a), flat(b)], cn_type, factor)
            mu[:, 1:], wup[:, 1:], wdn[:, 1:] = m1.reshape(N, R - 1, -1), u1.reshape(N, R - 1, -1), d1.reshape(N, R - 1, -1)
        self.mu[idx], self.wdn[idx], self.wup[idx] = mu, wdn, wup

    def u_hat(self, idx):
        g, wdn, wup, R = self.g[idx], self.wdn[idx], self.wup[idx], self.R
        G = _f(g + wdn)
        G[:, :R - 1] = _f(G[:, :R - 1] + wup[:, 1:])
        return (G < 0).astype(np.uint8)


def window_test(code, x_hat, z_hat, u_x_hat, u_z_hat, dx, dz):
    """[B] bool: for every round, H e_hat_t == d_t ^ u_hat_t ^ u_hat_{t-1} on both graphs, with integer matrices."""
    hx, hz = np.asarray(code.hx, np.int64) % 2, np.asarray(code.hz, np.int64) % 2

    def side(h, e, d, u):
        before = np.zeros_like(u)
        before[:, 1:] = u[:, :-1]
        return ((e.astype(np.int64) @ h.T) % 2 == (d ^ u ^ before)).all((1, 2))

    return side(hz, x_hat, dz, u_z_hat) & side(hx, z_hat, dx, u_x_hat)


def stbp4_decode(code, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, prev_x=None, prev_z=None,
                 llr_ch=None, llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=INF, gamma_z=INF, gamma_last_x=INF, gamma_last_z=INF):
    """`code`: an object with hx and hz; synd_x [B,R,m_x], synd_z [B,R,m_z] raw syndromes.  Returns (x_hat [B,R,n], z_hat [B,R,n],
    u_x_hat [B,R,m_x], u_z_hat [B,R,m_z] uint8, stats [B,4] int32 = found, the a of the last test, iterations, the k of the last
    test)."""
    assert cn_type in CN_TYPES and len(factors) == len(owns) >= 1
    G = MB.graph_of(code)
    n = G.n
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B, R = synd_x.shape[:2]
    assert synd_x.shape == (B, R, G.x.m) and synd_z.shape == (B, R, G.z.m)
    X = _SideState(G.x, window_gammas(B, R, G.x.m, synd_llr_x, gamma_x, gamma_last_x), differences(synd_x, prev_x))
    Z = _SideState(G.z, window_gammas(B, R, G.z.m, synd_llr_z, gamma_z, gamma_last_z), differences(synd_z, prev_z))
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    hard = np.zeros((B, R, n), np.uint8)
    ux, uz = np.zeros((B, R, G.x.m), np.uint8), np.zeros((B, R, G.z.m), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for a in range(len(factors)):
        T = pre_iter if a == 0 else attempt_iter
        if restart and a > 0:
            X.zero()
            Z.zero()
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            N = len(idx)
            if N == 0:
                break
            lamr = np.repeat(lam[idx], R, axis=0)  # [N*R,3,n]: the same prior in every round
            nux, nuz = G.qubit_update(X.mu[idx].reshape(N * R, -1), Z.mu[idx].reshape(N * R, -1), lamr, F32(owns[a]))
            X.check_update(idx, nux.reshape(N, R, -1), cn_type, F32(factors[a]))
            Z.check_update(idx, nuz.reshape(N, R, -1), cn_type, F32(factors[a]))
            dn = MB.decisions(*G.totals(X.mu[idx].reshape(N * R, -1), Z.mu[idx].reshape(N * R, -1), lamr)).reshape(N, R, n)
            uxk, uzk = X.u_hat(idx), Z.u_hat(idx)
            ok = window_test(code, dn & 1, dn >> 1, uxk, uzk, X.d[idx], Z.d[idx])
            hard[idx], ux[idx], uz[idx] = dn, uxk, uzk
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), ux, uz, stats


def stbp4_lds_bytes(E, n, m, R, cpb):
    """fgnn_stbp4_decode: per window R message areas of E floats, R m floats of b slots, (R-1) m floats of a slots, R n decision bytes
    and R m u_hat bytes, each area rounded up to 4 floats; per workgroup the two 64-float tables, a stamp per window and ndone."""
    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    area = lambda x: r4((x + 3) // 4)  # noqa: E731
    per_win = R * r4(E) + r4(R * m) + r4((R - 1) * m) + area(R * n) + area(R * m)
    return per_win * 4 * cpb + 2 * 64 * 4 + r4(cpb + 1) * 4


def window_plan(rounds, window, commit):
    """[(first round, rounds in the window, rounds committed, is the last)] of `BP4_Phenomenological_Model`."""
    if window is None or rounds <= window:
        return [(0, rounds, rounds, True)]
    assert 1 <= commit <= window
    plan, a = [], 0
    while a + window < rounds:
        plan.append((a, window, commit, False))
        a += commit
    plan.append((a, rounds - a, rounds - a, True))
    return plan


def sliding_decode(decode, sx, sz, rounds, window, commit, gamma):
    """The window loop of `BP4_Phenomenological_Model` over `decode(synd_x, synd_z, prev_x, prev_z, gamma_last)` -> the five outputs:
    sx [B,rounds,m_x], sz [B,rounds,m_z] measured syndromes.  Returns the committed (x_hat, z_hat [B,rounds,n], u_x_hat, u_z_hat
    [B,rounds,m]), the number of unsolved windows and the list of calls made as (first round, rounds, gamma_last, prev given)."""
    B = sx.shape[0]
    out, calls, unsolved = None, [], 0
    px = pz = None
    for a, W, F, last in window_plan(rounds, window, commit):
        gl = INF if last else gamma
        xh, zh, uxh, uzh, st = decode(np.ascontiguousarray(sx[:, a:a + W]), np.ascontiguousarray(sz[:, a:a + W]), px, pz, gl)
        calls.append((a, W, gl, px is not None))
        unsolved += int((st[:, 0] == 0).sum())
        if out is None:
            out = [np.zeros((B, rounds) + t.shape[2:], np.uint8) for t in (xh, zh, uxh, uzh)]
        for o, t in zip(out, (xh, zh, uxh, uzh)):
            assert not o[:, a:a + F].any(), "a round is committed once"
            o[:, a:a + F] = t[:, :F]
        if not last:
            px, pz = sx[:, a + F - 1] ^ uxh[:, F - 1], sz[:, a + F - 1] ^ uzh[:, F - 1]
    return out[0], out[1], out[2], out[3], unsolved, calls
