"""BP4 with message-strength control (fgnn_mbp4_decode, include/fgnn.h) restated in NumPy float32.

The oracle's BP4 step has no own-weight, so this restatement cannot take its steps from `OracleGraph.bp4_decode` the way its siblings
do.  Every float operation is written out here in the order of feedback_gnn_amd/csrc/fgnn_vn.h and fgnn_cn.h, on float32 arrays
(NumPy rounds every elementwise float32 operation once, to nearest even, and never fuses two of them), and every transcendental is
the oracle's: `math_apply` evaluates the shared routines of fgnn_math.h, compiled by gcc.

    softplus(t)  = math_apply("softplus", t)
    lse2(a, b)   = math_apply("lse2_corr", a - b) + max(a, b)          fg_lse2: lse2_corr depends on |a - b| alone
    phi(x)       = math_apply("phi", x)
    tanh, atanh, 1 / t of the boxplus rule: "tanh", "atanh", "rcp_unit"

tests/test_mbp4_reference_cpu.py ties the result to the oracle: with one attempt and own = 1 it equals BP4 stopped at its first
solution for all three check rules, and the per-edge value equals the host build of vn_edge_own bit for bit.

Messages live on the edges of the two graphs in qubit-major order (a qubit's hx edges by ascending check, then the next qubit), the
slot order of the library: a qubit's sums ascend over its slots, a check's loops ascend over its qubits.  Degrees may differ from node
to node; a padded edge carries a mask.  Samples are independent: the batch runs in lock-step and a finished sample leaves."""
import numpy as np

from oracle.oracle import math_apply

F32 = np.float32
CN_TYPES = ("boxplus", "boxplus-phi", "minsum")


def _f(x):
    assert x.dtype == F32, x.dtype
    return x


def softplus(t):
    return math_apply("softplus", _f(t))


def lse2(a, b):
    """fg_lse2: lse2_corr(a, b) + max(a, b), where lse2_corr(a, b) = log(1 + exp(-min(|a - b|, 20))) reads a - b alone."""
    return _f(math_apply("lse2_corr", _f(a - b)) + np.maximum(a, b))


def with_sign(mag, neg):
    """The magnitude's bits with the sign bit flipped where `neg` (fgnn_cn.h)."""
    return (mag.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(F32)


def vn_edge_own(num, A, Y, mu, w):
    """fgnn_vn.h: own = w * mu (one product); Ae = A - own; Ye = Y - own; num - lse2(-Ae, -Ye).  Broadcasts; all float32."""
    own = _f(F32(w) * mu)
    Ae, Ye = _f(A - own), _f(Y - own)
    return _f(num - lse2(-Ae, -Ye))


class Side:
    """One Tanner graph (hx or hz) as padded index tables: for every qubit its edges in ascending check order, for every check its
    edges in ascending qubit order.  Edge e = position in the qubit-major list."""

    def __init__(self, h):
        h = np.asarray(h, np.int64) % 2
        self.m, self.n = h.shape
        v, c = np.nonzero(h.T)  # qubit-major, checks ascending within a qubit
        self.E = len(v)
        self.v_of, self.c_of = v, c
        self.vn_tab, self.vn_mask = self._table(v, self.n)
        order = np.lexsort((v, c))  # check-major, qubits ascending within a check
        self.cn_tab, self.cn_mask = self._table(c[order], self.m, order)

    @staticmethod
    def _table(owner, count, edge=None):
        edge = np.arange(len(owner)) if edge is None else edge
        deg = np.bincount(owner, minlength=count)
        tab = np.zeros((count, max(int(deg.max()), 1)), np.int64)
        mask = np.zeros(tab.shape, bool)
        start = np.concatenate([[0], np.cumsum(deg)])
        for i in range(count):  # owner is sorted
            tab[i, :deg[i]] = edge[start[i]:start[i + 1]]
            mask[i, :deg[i]] = True
        return tab, mask

    def vn_sum(self, mu):
        """[B,n]: the sum of a qubit's messages, ascending over its slots from 0.0f."""
        S = np.zeros((mu.shape[0], self.n), F32)
        for j in range(self.vn_tab.shape[1]):
            S = np.where(self.vn_mask[:, j], _f(S + mu[:, self.vn_tab[:, j]]), S)
        return S


def cn_update(side, nu, synd, cn_type, factor):
    """fgnn_cn.h cn_update on every check of one side: nu [B,E] v->c messages, synd [B,m] bits; returns the c->v messages [B,E]."""
    B = nu.shape[0]
    tab, mask = side.cn_tab, side.cn_mask
    D = tab.shape[1]
    v = nu[:, tab]  # [B,m,D]
    factor = F32(factor)
    synd = synd.astype(bool)
    out = np.zeros_like(v)
    if cn_type == "boxplus-phi":
        neg = synd.copy()
        T = np.zeros((B, side.m), F32)
        a = np.zeros_like(v)
        ng = np.zeros(v.shape, bool)
        for j in range(D):
            mj = mask[:, j]
            ng[:, :, j] = (v[:, :, j] < 0) & mj
            neg ^= ng[:, :, j]
            a[:, :, j] = math_apply("phi", np.abs(v[:, :, j]))
            T = np.where(mj, _f(T + a[:, :, j]), T)
        for j in range(D):
            o = math_apply("phi", _f(T - a[:, :, j]))
            out[:, :, j] = _f(with_sign(o, neg ^ ng[:, :, j]) * factor)
    elif cn_type == "minsum":
        LARGE = F32(10000.0)
        vc = np.minimum(np.maximum(v, F32(-20.0)), F32(20.0))
        ng = (vc < 0) & mask
        neg = synd ^ (ng.sum(-1) % 2).astype(bool)
        a = np.abs(vc)
        minv = np.where(mask, a, F32(np.inf)).min(-1).astype(F32)
        d = _f(a - minv[:, :, None])
        d = np.where(d == 0, LARGE, d)
        min2 = np.where(mask, d, F32(np.inf)).min(-1).astype(F32)
        nsum = np.zeros((B, side.m), F32)
        for j in range(D):
            nsum = np.where(mask[:, j], _f(nsum + d[:, :, j]), nsum)
        min2 = _f(min2 + minv)
        nsum = _f(nsum - F32(F32(2.0) * LARGE - F32(1.0)))
        sg = np.where(nsum > 0, F32(1.0), np.where(nsum < 0, F32(-1.0), F32(0.0))).astype(F32)
        dm = _f(F32(0.5) * _f(F32(1.0) - sg))
        min_e = _f(_f(_f(F32(1.0) - dm) * minv) + _f(dm * min2))
        o = np.where(_f(a - minv[:, :, None]) == 0, min_e[:, :, None], minv[:, :, None]).astype(F32)
        out = _f(with_sign(o, neg[:, :, None] ^ ng) * factor)
    else:  # boxplus
        t = np.zeros_like(v)
        P = np.ones((B, side.m), F32)
        for j in range(D):
            tj = math_apply("tanh", _f(v[:, :, j] / F32(2.0)))
            tj = np.where(tj == 0, F32(1e-12), tj).astype(F32)
            t[:, :, j] = tj
            P = np.where(mask[:, j], tj if j == 0 else _f(P * tj), P)
        P = _f(P * np.where(synd, F32(-1.0), F32(1.0)).astype(F32))
        clipv = F32(0.99999988)
        tsafe = np.where(mask, t, F32(1.0))
        q = _f(math_apply("rcp_unit", tsafe) * P[:, :, None])
        q = np.where(np.abs(q) < F32(1e-7), F32(0.0), q).astype(F32)
        q = np.minimum(np.maximum(q, -clipv), clipv)
        out = _f(_f(F32(2.0) * math_apply("atanh", q)) * factor)
    mu = np.zeros_like(nu)
    bsel = np.arange(B)[:, None]
    mu[bsel, tab[mask][None, :]] = out[:, mask]
    return mu


def decisions(X, Y, Z):
    """vn_decide: the smallest of X, Z, Y below 0 in that order with strict comparisons, else the identity."""
    cand = np.stack([np.zeros_like(X), X, Z, Y], axis=0)
    return np.argmin(cand, axis=0).astype(np.uint8)


class Graph:
    """The two sides of a code and one MBP4 iteration on them."""

    def __init__(self, code):
        self.hx, self.hz = np.asarray(code.hx, np.int64) % 2, np.asarray(code.hz, np.int64) % 2
        self.x, self.z = Side(self.hx), Side(self.hz)
        self.n = self.hx.shape[1]

    def totals(self, mux, muz, lam):
        Sz, Sx = self.z.vn_sum(muz), self.x.vn_sum(mux)
        Y = _f(_f(Sz + Sx) + lam[:, 1])
        X = _f(Sz + lam[:, 0])
        Z = _f(Sx + lam[:, 2])
        return X, Y, Z

    def qubit_update(self, mux, muz, lam, own):
        """The v->c messages (nu_x [B,E_x], nu_z [B,E_z]) of vn_edge_own from the c->v messages and the channel LLRs lam [B,3,n]."""
        X, Y, Z = self.totals(mux, muz, lam)
        numx, numz = softplus(-X), softplus(-Z)
        vx, vz = self.x.v_of, self.z.v_of
        nux = vn_edge_own(numx[:, vx], Z[:, vx], Y[:, vx], mux, own)
        nuz = vn_edge_own(numz[:, vz], X[:, vz], Y[:, vz], muz, own)
        return nux, nuz

    def step(self, mux, muz, lam, synd_x, synd_z, cn_type, factor, own):
        """One iteration: qubit update with `own`, check update * `factor`; returns the new messages and the decisions of their
        marginals."""
        nux, nuz = self.qubit_update(mux, muz, lam, own)
        mux, muz = cn_update(self.x, nux, synd_x, cn_type, factor), cn_update(self.z, nuz, synd_z, cn_type, factor)
        return mux, muz, decisions(*self.totals(mux, muz, lam))


_GRAPHS = {}


def graph_of(code):
    g = _GRAPHS.get(id(code))
    if g is None or g[0] is not code:
        g = _GRAPHS[id(code)] = (code, Graph(code))
    return g[1]


def mbp4_tables(alphas, base):
    """own[a] = float32(alpha_a), factor[a] = float32(base) / float32(alpha_a): one IEEE float32 division."""
    own = np.asarray(alphas, F32).reshape(-1)
    return (F32(base) / own).astype(F32), own


def mbp4_decode(code, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None, llr_const=0.0):
    """`code`: an object with hx and hz.  Returns (x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, the a of the last
    test, iterations, the k of the last test)."""
    assert cn_type in CN_TYPES and len(factors) == len(owns) >= 1
    G = graph_of(code)
    n = G.n
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B = synd_x.shape[0]
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    mux, muz = np.zeros((B, G.x.E), F32), np.zeros((B, G.z.E), F32)
    hard = np.zeros((B, n), np.uint8)
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
            mux[idx], muz[idx], dn = G.step(mux[idx], muz[idx], lam[idx], synd_x[idx], synd_z[idx], cn_type, F32(factors[a]), F32(owns[a]))
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ G.hz.T) % 2 == synd_z[idx]).all(1) & ((z @ G.hx.T) % 2 == synd_x[idx]).all(1)
            hard[idx] = dn
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats
