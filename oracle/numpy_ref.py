"""Independent NumPy restatement of the reference's BP4 + feedback-GNN arithmetic, and of binary syndrome BP in float64.

TEST INFRASTRUCTURE ONLY.  Purpose: a second, independently written statement of
/root/reference sionna/fec/ldpc/decoding_q.py and feedback_gnn.py that uses NumPy's OWN float32
exp/log/log1p/tanh (not the polynomial routines of fgnn_math.h) and the reference's own data layout
(edge-major tensors [E, batch], batch as the minor axis, np.add.reduceat for the ragged sums).  The C
oracle must agree with it to <= 1e-4 on converged samples and reproduce the reference's
known-answer values; that bounds what the custom elementary functions can have changed.
"""
import numpy as np

F = np.float32
_THR = F(np.log(np.finfo(np.float32).eps, dtype=np.float32) + F(2.0))  # tf2xla Softplus threshold (negative)


def softplus(t):
    """tf.math.softplus as lowered by tf2xla."""
    t = t.astype(F, copy=False)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(np.minimum(t, F(30.0)))
        mid = np.log1p(e)
    return np.where(t > -_THR, t, np.where(t < _THR, e, mid)).astype(F)


def lse2(a, b):
    """tf.reduce_logsumexp(stack([a, b], -1), -1): max-shifted."""
    m = np.maximum(a, b)
    with np.errstate(under="ignore"):
        s = np.exp(a - m) + np.exp(b - m)
    return (np.log(s) + m).astype(F)


def phi(x):
    """decoding_q.py:365-373."""
    x = np.clip(x, F(8.5e-8), F(16.635532)).astype(F)
    with np.errstate(under="ignore"):
        return (softplus(x) - np.log(np.exp(x) - F(1.0))).astype(F)


class Graph:
    def __init__(self, code, stage_one=True):
        self.n = code.hx.shape[1]
        self.sides = []
        for pcm in (code.hx, code.hz):
            chk, var = np.nonzero(np.asarray(pcm))
            o = np.lexsort((chk, var))  # by qubit, then check (canonical VN-major order)
            chk, var = chk[o], var[o]
            to_cn = np.lexsort((var, chk))  # CN-major: by check, then qubit
            inv = np.argsort(to_cn)
            vstart = np.searchsorted(var, np.arange(self.n))
            cstart = np.searchsorted(chk[to_cn], np.arange(pcm.shape[0]))
            self.sides.append(dict(chk=chk, var=var, to_cn=to_cn, inv=inv, vstart=vstart, cstart=cstart,
                                   m=pcm.shape[0], cn_of=chk[to_cn]))
        xp, zp = (code.hz, code.hx) if stage_one else (code.hx_perp, code.hz_perp)
        self.logit_rows = [self._rows(xp), self._rows(zp)]

    @staticmethod
    def _rows(mat):
        r, c = np.nonzero(np.asarray(mat))
        return dict(col=c, start=np.searchsorted(r, np.arange(mat.shape[0])), row_of=r, rows=mat.shape[0])


def _seg_sum(vals, start):
    return np.add.reduceat(vals, start, axis=0).astype(F)


def _cn_phi(msg, side, sigma, factor):
    """_cn_update_phi (:376-431) on CN-major messages [E,B]; sigma [m,B] = 1-2*syndrome."""
    sgn = np.where(msg < 0, F(-1), F(1))
    prod = np.multiply.reduceat(sgn, side["cstart"], axis=0) * sigma
    a = phi(np.abs(msg))
    T = _seg_sum(a, side["cstart"])
    out = sgn * prod[side["cn_of"]] * phi(T[side["cn_of"]] - a)
    return (out * F(factor)).astype(F)


def _logits(g, which, llr):
    rows = g.logit_rows[which]
    v = llr[rows["col"]]
    sgn = np.where(v < 0, F(-1), F(1))
    prod = np.multiply.reduceat(sgn, rows["start"], axis=0)
    T = _seg_sum(phi(np.abs(v)), rows["start"])
    return (prod * phi(T)).astype(F)


def bp4_decode(g, synd_x, synd_z, num_iter, llr_const=None, llr_ch=None, factor=1.0):
    """boxplus-phi BP4; inputs codeword-major ([B,m] syndromes, [B,3,n] LLRs), math batch-minor.
    Returns dict(llr [B,3,n], x_hat, z_hat, x_logit [B,rows], z_logit)."""
    B = synd_x.shape[0]
    n = g.n
    if llr_ch is None:
        L = np.full((3, n, B), F(llr_const), F)
    else:
        L = np.ascontiguousarray(np.transpose(llr_ch, (1, 2, 0)), dtype=F)
    sig = [(F(1) - F(2) * synd_x.T.astype(F)), (F(1) - F(2) * synd_z.T.astype(F))]
    msg = [np.zeros((s["chk"].size, B), F) for s in g.sides]  # VN-major c->v messages

    def totals():
        Sx = _seg_sum(msg[0], g.sides[0]["vstart"])
        Sz = _seg_sum(msg[1], g.sides[1]["vstart"])
        return Sz + L[0], (Sz + Sx) + L[1], Sx + L[2]

    for _ in range(num_iter):
        X, Y, Z = totals()
        vx, vz = g.sides[0]["var"], g.sides[1]["var"]
        nux = softplus(-X)[vx] - lse2(-(Z[vx] - msg[0]), -(Y[vx] - msg[0]))
        nuz = softplus(-Z)[vz] - lse2(-(X[vz] - msg[1]), -(Y[vz] - msg[1]))
        for s, nu in ((0, nux), (1, nuz)):
            side = g.sides[s]
            msg[s] = _cn_phi(nu[side["to_cn"]], side, sig[s], factor)[side["inv"]]
    X, Y, Z = totals()
    dec = np.argmin(np.stack([np.zeros_like(X), X, Z, Y], 0), axis=0)
    llr_z = softplus(-X) - lse2(-Z, -Y)
    llr_x = softplus(-Z) - lse2(-X, -Y)
    return dict(llr=np.ascontiguousarray(np.stack([X, Y, Z], 0).transpose(2, 0, 1)),
                x_hat=(dec & 1).T.astype(np.uint8), z_hat=(dec >> 1).T.astype(np.uint8),
                x_logit=_logits(g, 0, llr_x).T.copy(), z_logit=_logits(g, 1, llr_z).T.copy())


def feedback_gnn(g, w, llr, logit_hx, logit_hz, synd_x, synd_z):
    """Feedback_GNN.call (feedback_gnn.py:161-188) with float32 matmuls; llr [B,3,n] -> [B,3,n]."""
    h_vn = np.transpose(llr, (0, 2, 1)).astype(F)  # [B,n,3]
    out_m = []
    for s, (logit, synd, k) in enumerate(((logit_hx, synd_x, 2), (logit_hz, synd_z, 6))):
        side = g.sides[s]
        h_cn = (logit * (F(1) - F(2) * synd.astype(F)))[:, :, None]  # [B,m,1]
        feat = np.concatenate([h_cn[:, side["chk"], :], h_vn[:, side["var"], :]], axis=-1)  # VN-major edges
        hid = np.tanh(feat @ w[k] + w[k + 1]).astype(F)
        m = (hid @ w[k + 2] + w[k + 3]).astype(F)  # [B,E,20]
        ssum = np.add.reduceat(m, side["vstart"], axis=1)
        deg = np.diff(np.append(side["vstart"], side["chk"].size)).astype(F)
        out_m.append((ssum / deg[None, :, None]).astype(F))
    z = np.concatenate([out_m[0], out_m[1], h_vn], axis=-1)
    o = (np.tanh(z @ w[10] + w[11]).astype(F) @ w[0] + w[1]).astype(F)  # [B,n,3]
    return np.ascontiguousarray(np.transpose(o, (0, 2, 1)))


def gnn_bp4(code, w, synd_x, synd_z, num_iter, D=20):
    """GNN_BP4.call (sionna/fec/ldpc/gnn.py:383-423) in the reference's own batch-first tensor form, with the two
    repairs/restatements of oracle/fgnn_oracle.c (4-value cal_logit; message width = num_embed_dims).
    w = the 30 arrays of the oracle's order.  Returns dict(x_hat [B,n], z_hat, llr [B,3,n], x_logit_all, z_logit_all)."""
    hx, hz = np.asarray(code.hx), np.asarray(code.hz)
    B = synd_x.shape[0]
    n = hx.shape[1]
    sgx = (F(1) - F(2) * synd_x.astype(F))  # [B,m_x]
    sgz = (F(1) - F(2) * synd_z.astype(F))

    def mlp(x, ws):
        return (np.tanh(x @ ws[0] + ws[1]).astype(F) @ ws[2] + ws[3]).astype(F)

    def edges(pcm):
        c, v = np.nonzero(pcm)  # row-major: check-major, ascending qubit
        return c, v

    ex, ez = edges(hx), edges(hz)

    def mean_by(msgs, idx, count):  # msgs [B,E,D], aggregate rows with equal idx (ascending edge id inside a group)
        out = np.zeros((B, count, msgs.shape[-1]), F)
        order = np.argsort(idx, kind="stable")
        starts = np.searchsorted(idx[order], np.arange(count))
        out = np.add.reduceat(msgs[:, order, :], starts, axis=1).astype(F)
        deg = np.bincount(idx, minlength=count).astype(F)
        return (out / deg[None, :, None]).astype(F)

    def update_cn(h_vn, hcx, hcz, lgx, lgz):
        new = []
        for (c, v), hc, lg, wm, we in ((ex, hcx, lgx, w[0:4], w[8:12]), (ez, hcz, lgz, w[4:8], w[12:16])):
            m = mean_by(mlp(np.concatenate([h_vn[:, v, :], hc[:, c, :]], -1), wm), c, hc.shape[1])
            new.append(mlp(np.concatenate([m, hc, lg[:, :, None]], -1), we))
        return new

    def update_vn(hcx, hcz, h_vn):
        ms = []
        for (c, v), hc, sg, wm in ((ex, hcx, sgx, w[16:20]), (ez, hcz, sgz, w[20:24])):
            msg = mlp(np.concatenate([hc[:, c, :], h_vn[:, v, :]], -1), wm) * sg[:, c, None]
            ms.append(mean_by(msg.astype(F), v, n))
        return mlp(np.concatenate([ms[0], ms[1], h_vn], -1), w[24:28])

    def phi_g(x):
        x = np.clip(x, F(8.5e-8), F(16.635532)).astype(F)
        return (np.log(np.exp(x) + F(1)) - np.log(np.exp(x) - F(1))).astype(F)

    def rows_logit(mat, llr):  # llr [B,n] -> [B,rows]
        r, c = np.nonzero(np.asarray(mat))
        v = llr[:, c]
        sgn = np.where(v < 0, F(-1), F(1))
        starts = np.searchsorted(r, np.arange(mat.shape[0]))
        prod = np.multiply.reduceat(sgn, starts, axis=1)
        T = np.add.reduceat(phi_g(np.abs(v)), starts, axis=1).astype(F)
        return (prod * phi_g(T)).astype(F)

    h_vn = np.ones((B, n, D), F)
    hcx = np.zeros((B, hx.shape[0], D), F)
    hcz = np.zeros((B, hz.shape[0], D), F)
    hcx, hcz = update_cn(h_vn, hcx, hcz, np.zeros_like(sgx), np.zeros_like(sgz))
    xl_all, zl_all = [], []
    for it in range(num_iter):
        h_vn = update_vn(hcx, hcz, h_vn)
        L = (h_vn @ w[28] + w[29]).astype(F)  # [B,n,3]
        llrx, llry, llrz = L[..., 0], L[..., 1], L[..., 2]
        llr_z = softplus(-llrx) - lse2(-llrz, -llry)
        llr_x = softplus(-llrz) - lse2(-llrx, -llry)
        hz_l, lz_l = rows_logit(hz, llr_x), rows_logit(code.lz, llr_x)
        hx_l, lx_l = rows_logit(hx, llr_z), rows_logit(code.lx, llr_z)
        xl_all.append(np.concatenate([hz_l, lz_l], 1))
        zl_all.append(np.concatenate([hx_l, lx_l], 1))
        if it == num_iter - 1:
            break
        hcx, hcz = update_cn(h_vn, hcx, hcz, hx_l * sgx, hz_l * sgz)
    dec = np.argmin(np.stack([np.zeros_like(llrx), llrx, llrz, llry], 0), axis=0)
    return dict(x_hat=(dec & 1).astype(np.uint8), z_hat=(dec >> 1).astype(np.uint8),
                llr=np.ascontiguousarray(np.stack([llrx, llry, llrz], 1)), x_logit_all=np.stack(xl_all), z_logit_all=np.stack(zl_all))


def gnn_bp4_general(code, cfg, w, synd_x, synd_z, num_iter):
    """GNN_BP4.call for any constructor setting (gnn.py:131-207, :494-751), batch-first tensors and NumPy matmuls like the reference.
    cfg = (D, H, L, reduce_op 0 sum / 1 mean / 2 max / 3 min, activation 0 linear / 1 tanh / 2 relu / 3 sigmoid, use_bias,
    use_attributes, An, Am); w in the order of og_gnn_bp4_general.  Same two repairs as gnn_bp4 above."""
    D, H, L, rop, act, bias, attr, An, Am = [int(x) for x in cfg]
    if not attr:
        An = Am = 0
    hx, hz = np.asarray(code.hx), np.asarray(code.hz)
    B, n = synd_x.shape[0], hx.shape[1]
    sgx = (F(1) - F(2) * synd_x.astype(F))
    sgz = (F(1) - F(2) * synd_z.astype(F))
    st = 1 + bias
    fa = {0: lambda x: x, 1: np.tanh, 2: lambda x: np.maximum(x, F(0)), 3: lambda x: (F(1) / (F(1) + np.exp(-x))).astype(F)}[act]
    mlps, pos = [], 0
    for _ in range(7):
        layers = []
        for k in range(L):
            layers.append((w[pos], w[pos + 1] if bias else None, k < L - 1))
            pos += st
        mlps.append(layers)
    Winv, binv = w[pos], (w[pos + 1] if bias else None)
    pos += st
    cn_node, cn_msga, vn_node, vn_msga = ([None, None], [None, None], None, [None, None])
    if attr:
        cn_node, cn_msga, vn_node, vn_msga = [w[pos], w[pos + 1]], [w[pos + 2], w[pos + 3]], w[pos + 4], [w[pos + 5], w[pos + 6]]

    def mlp(x, layers):
        for W, b, hidden in layers:
            x = (x @ W).astype(F)
            if b is not None:
                x = (x + b).astype(F)
            if hidden:
                x = fa(x).astype(F)
        return x

    def tile(a):
        return np.broadcast_to(a[None], (B,) + a.shape).astype(F)

    def reduce_by(msgs, idx, count):
        order = np.argsort(idx, kind="stable")
        starts = np.searchsorted(idx[order], np.arange(count))
        m = msgs[:, order, :]
        if rop == 2:
            return np.maximum.reduceat(m, starts, axis=1).astype(F)
        if rop == 3:
            return np.minimum.reduceat(m, starts, axis=1).astype(F)
        out = np.add.reduceat(m, starts, axis=1).astype(F)
        if rop == 1:
            out = (out / np.bincount(idx, minlength=count).astype(F)[None, :, None]).astype(F)
        return out

    ex, ez = np.nonzero(hx), np.nonzero(hz)  # row-major edges (check, qubit): the reference's edge order

    def update_cn(h_vn, hcx, hcz, lgx, lgz):
        new = []
        for s, ((c, v), hc, lg) in enumerate(((ex, hcx, lgx), (ez, hcz, lgz))):
            f = [h_vn[:, v, :], hc[:, c, :]] + ([tile(cn_msga[s])] if Am else [])
            m = reduce_by(mlp(np.concatenate(f, -1), mlps[s]), c, hc.shape[1])
            f = [m] + ([tile(cn_node[s])] if An else []) + [hc, lg[:, :, None]]
            new.append(mlp(np.concatenate(f, -1), mlps[2 + s]))
        return new

    def update_vn(hcx, hcz, h_vn):
        ms = []
        for s, ((c, v), hc, sg) in enumerate(((ex, hcx, sgx), (ez, hcz, sgz))):
            f = [hc[:, c, :], h_vn[:, v, :]] + ([tile(vn_msga[s])] if Am else [])
            msg = (mlp(np.concatenate(f, -1), mlps[4 + s]) * sg[:, c, None]).astype(F)
            ms.append(reduce_by(msg, v, n))
        f = [ms[0], ms[1]] + ([tile(vn_node)] if An else []) + [h_vn]
        return mlp(np.concatenate(f, -1), mlps[6])

    def phi_g(x):
        x = np.clip(x, F(8.5e-8), F(16.635532)).astype(F)
        return (np.log(np.exp(x) + F(1)) - np.log(np.exp(x) - F(1))).astype(F)

    def rows_logit(mat, llr):
        r, c = np.nonzero(np.asarray(mat))
        v = llr[:, c]
        sgn = np.where(v < 0, F(-1), F(1))
        starts = np.searchsorted(r, np.arange(mat.shape[0]))
        return (np.multiply.reduceat(sgn, starts, axis=1) * phi_g(np.add.reduceat(phi_g(np.abs(v)), starts, axis=1).astype(F))).astype(F)

    h_vn = np.ones((B, n, D), F)
    hcx, hcz = np.zeros((B, hx.shape[0], D), F), np.zeros((B, hz.shape[0], D), F)
    hcx, hcz = update_cn(h_vn, hcx, hcz, np.zeros_like(sgx), np.zeros_like(sgz))
    xl_all, zl_all = [], []
    for it in range(num_iter):
        h_vn = update_vn(hcx, hcz, h_vn)
        Lv = (h_vn @ Winv).astype(F)
        if binv is not None:
            Lv = (Lv + binv).astype(F)
        llrx, llry, llrz = Lv[..., 0], Lv[..., 1], Lv[..., 2]
        llr_z = softplus(-llrx) - lse2(-llrz, -llry)
        llr_x = softplus(-llrz) - lse2(-llrx, -llry)
        hz_l, lz_l = rows_logit(hz, llr_x), rows_logit(code.lz, llr_x)
        hx_l, lx_l = rows_logit(hx, llr_z), rows_logit(code.lx, llr_z)
        xl_all.append(np.concatenate([hz_l, lz_l], 1))
        zl_all.append(np.concatenate([hx_l, lx_l], 1))
        if it == num_iter - 1:
            break
        hcx, hcz = update_cn(h_vn, hcx, hcz, hx_l * sgx, hz_l * sgz)
    dec = np.argmin(np.stack([np.zeros_like(llrx), llrx, llrz, llry], 0), axis=0)
    return dict(x_hat=(dec & 1).astype(np.uint8), z_hat=(dec >> 1).astype(np.uint8),
                llr=np.ascontiguousarray(np.stack([llrx, llry, llrz], 1)), x_logit_all=np.stack(xl_all), z_logit_all=np.stack(zl_all))


def gnn_bp4_general_shapes(code, cfg):
    """Shapes of the weight list of og_gnn_bp4_general / gnn_bp4_general for a configuration."""
    D, H, L, rop, act, bias, attr, An, Am = [int(x) for x in cfg]
    if not attr:
        An = Am = 0
    nin = [2 * D + Am] * 2 + [2 * D + An + 1] * 2 + [2 * D + Am] * 2 + [3 * D + An]
    shapes = []
    for q in range(7):
        for k in range(L):
            K, J = (nin[q] if k == 0 else H), (D if k == L - 1 else H)
            shapes.append((K, J))
            if bias:
                shapes.append((J,))
    shapes.append((D, 3))
    if bias:
        shapes.append((3,))
    if attr:
        hx, hz = np.asarray(code.hx), np.asarray(code.hz)
        shapes += [(hx.shape[0], An), (hz.shape[0], An), (int(hx.sum()), Am), (int(hz.sum()), Am), (hx.shape[1], An),
                   (int(hx.sum()), Am), (int(hz.sum()), Am)]
    return shapes


# ---- binary syndrome BP: LDPCBPDecoder.call with is_syndrome=True (sionna/fec/ldpc/decoding.py:874-1048), float64 ----
# The reference holds these constants in float32 tensors; the restatement uses the float32 values in float64 arithmetic.
_D = np.float64
_LLR_MAX = _D(F(20.0))                 # self._llr_max (:320)
_ATANH_CLIP = _D(F(1 - 1e-7))          # self._atanh_clip_value (:318), 0.99999988 as a float32
_PHI_LO, _PHI_HI = _D(F(8.5e-8)), _D(F(16.635532))  # _phi's clip (:632)
_TANH_ZERO, _TANH_SMALL = _D(F(1e-12)), _D(F(1e-7))  # _where_ragged / _where_ragged_inv (:563, :568)
_LARGE = _D(10000.0)                   # LARGE_VAL (:756)


def _bp2_phi(x):
    """_phi (:625-633): log(exp(x)+1) - log(exp(x)-1) after the clip."""
    x = np.clip(x, _PHI_LO, _PHI_HI)
    return np.log(np.exp(x) + 1.0) - np.log(np.exp(x) - 1.0)


def _bp2_sign(x):
    """tf.sign with 0 replaced by 1 (:697-703): -0 counts as +1 too."""
    s = np.sign(x)
    return np.where(s == 0, 1.0, s)


def _bp2_cn(rule, msg, seg, starts, syndrome):
    """One check-node update on check-major messages [E,B]; seg [E] = the check of each edge (0.. over non-empty checks), starts its
    first edges, syndrome [checks,B] = (-1)^s."""
    def reduce(ufunc, v):
        return ufunc.reduceat(v, starts, axis=0)

    if rule == "boxplus-phi":  # _cn_update_phi (:637-693)
        sign_val = _bp2_sign(msg)
        sign_node = reduce(np.multiply, sign_val) * syndrome
        sign_val = sign_val * sign_node[seg]
        a = _bp2_phi(np.abs(msg))
        msg_sum = reduce(np.add, a)
        return sign_val * _bp2_phi(-1.0 * a + msg_sum[seg])
    if rule == "minsum":  # _cn_update_minsum (:744-850)
        msg = np.clip(msg, -_LLR_MAX, _LLR_MAX)
        sign_val = _bp2_sign(msg)
        sign_node = reduce(np.multiply, sign_val) * syndrome
        sign_val = sign_val * sign_node[seg]
        msg = np.abs(msg)
        min_val = reduce(np.minimum, msg)
        msg = msg - min_val[seg]
        msg = np.where(msg == 0, _LARGE, msg)
        min_val2 = reduce(np.minimum, msg) + min_val
        node_sum = reduce(np.add, msg) - (2 * _LARGE - 1.0)
        double_min = 0.5 * (1 - np.sign(node_sum))
        min_val_e = (1 - double_min) * min_val + double_min * min_val2
        return sign_val * np.where(msg == _LARGE, min_val_e[seg], min_val[seg])
    # _cn_update_tanh (:575-623)
    t = np.tanh(msg / 2)
    t = np.where(t == 0, _TANH_ZERO, t)
    prod = reduce(np.multiply, t) * syndrome
    q = t ** -1 * prod[seg]
    q = np.where(np.abs(q) < _TANH_SMALL, 0.0, q)
    q = np.clip(q, -_ATANH_CLIP, _ATANH_CLIP)
    return 2 * np.arctanh(q)


def bp2_decode(hx, synd, num_iter, cn_type, factor, llr_ch=None, llr_const=None):
    """LDPCBPDecoder.call with is_syndrome=True (decoding.py:874-1048) on the parity-check matrix hx [m,n], in float64 with the reference's
    batch-minor edge tensors.  synd [B,m]; llr_ch [B,n] logits (log p(1)/p(0)) or llr_const for every bit.  Returns (soft [B,n], hard [B,n]):
    the output logits -(-clip(llr) + sum of incoming messages) (:1025-1031) and their hard decisions 0 < logit (:1033-1034)."""
    hx = np.asarray(hx)
    synd = np.asarray(synd)
    B, (m, n) = synd.shape[0], hx.shape
    chk, var = np.nonzero(hx)  # check-major edges, ascending bits inside a check
    E = chk.size
    first = np.r_[True, chk[1:] != chk[:-1]] if E else np.zeros(0, bool)
    starts = np.flatnonzero(first)
    seg = np.cumsum(first) - 1
    syndrome = ((-1.0) ** synd.T.astype(_D))[chk[starts]]  # (:904-908), for the non-empty checks
    if llr_ch is None:
        llr = np.full((n, B), _D(F(llr_const)))
    else:
        llr = np.asarray(llr_ch, F).T.astype(_D)
    llr = -1.0 * np.clip(llr, -_LLR_MAX, _LLR_MAX)  # (:918-920, :940)
    fac = _D(F(factor))

    def vn_sum(msg):  # reduce_sum over each bit's edges (a bit without edges sums to 0)
        idx = (var[:, None] * B + np.arange(B)[None, :]).ravel()
        return np.bincount(idx, weights=msg.ravel(), minlength=n * B).reshape(n, B)

    msg = np.zeros((E, B))  # check-to-bit messages
    for _ in range(num_iter):
        x = vn_sum(msg) + llr  # _vn_update (:511-537)
        msg_vn = -1.0 * msg + x[var]
        msg = _bp2_cn(cn_type, msg_vn, seg, starts, syndrome) * fac  # (:988-991)
    x_hat = -1.0 * (llr + vn_sum(msg))
    return np.ascontiguousarray(x_hat.T), np.ascontiguousarray((0.0 < x_hat).T.astype(np.uint8))


# ---- BP4: QLDPCBPDecoder.call (sionna/fec/ldpc/decoding_q.py:661-797), float64 ----
# Line-by-line reading of decoding.py against decoding_q.py: _cn_update_tanh (decoding.py:573-623 / decoding_q.py:313-363) and
# _cn_update_minsum (:744-850 / :539-644) state the same operations with the same constants (_atanh_clip_value = 1 - 1e-7, _llr_max = 20,
# LARGE_VAL = 10000, the 1e-12 / 1e-7 substitutions); they differ only in decoding.py's `syndrome=None` default, and QLDPCBPDecoder always
# passes the syndrome.  So those two rules reuse _bp2_cn.  _phi differs: decoding_q.py:373 returns softplus(x) - log(exp(x) - 1),
# decoding.py:633 log(exp(x) + 1) - log(exp(x) - 1) — the same real function, restated below in its own form.
def _bp4_phi(x):
    """_phi (decoding_q.py:365-373): softplus(x) - log(exp(x) - 1) after the clip."""
    x = np.clip(x, _PHI_LO, _PHI_HI)
    return np.logaddexp(0.0, x) - np.log(np.expm1(x))


def _bp4_cn(rule, msg, seg, starts, syndrome):
    """One check-node update of QLDPCBPDecoder on check-major messages [E,B] (the arguments of _bp2_cn)."""
    if rule != "boxplus-phi":
        return _bp2_cn(rule, msg, seg, starts, syndrome)
    # _cn_update_phi (:376-431)
    sign_val = _bp2_sign(msg)
    sign_node = np.multiply.reduceat(sign_val, starts, axis=0) * syndrome
    sign_val = sign_val * sign_node[seg]
    a = _bp4_phi(np.abs(msg))
    msg_sum = np.add.reduceat(a, starts, axis=0)
    return sign_val * _bp4_phi(-1.0 * a + msg_sum[seg])


def _bp4_side(pcm):
    """Edges of one Tanner graph: VN-major (by qubit, then check: the slot order of the library and the oracle) and the check-major
    permutation with its segments over the non-empty checks."""
    chk, var = np.nonzero(np.asarray(pcm))
    o = np.lexsort((chk, var))
    chk, var = chk[o], var[o]
    to_cn = np.lexsort((var, chk))
    c = chk[to_cn]
    first = np.r_[True, c[1:] != c[:-1]] if c.size else np.zeros(0, bool)
    starts = np.flatnonzero(first)
    return dict(var=var, to_cn=to_cn, inv=np.argsort(to_cn), starts=starts, seg=np.cumsum(first) - 1, cn_chk=c[starts])


def _bp4_soft_syndrome(rows, llr):
    """_cn_update_phi_loss (:433-453) over the rows of `rows` [r,n] on binary LLRs [n,B]: the sign product (0 -> +1) times
    phi(sum of phi(|llr|)); an empty row gives phi(0)."""
    rows = np.asarray(rows)
    r, c = np.nonzero(rows)
    v = llr[c]
    neg = np.zeros((rows.shape[0], llr.shape[1]))
    np.add.at(neg, r, (v < 0).astype(np.float64))
    T = np.zeros_like(neg)
    np.add.at(T, r, _bp4_phi(np.abs(v)))
    return (1.0 - 2.0 * (neg % 2)) * _bp4_phi(T)


def bp4_decode64(code, synd_x, synd_z, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=None, msg_init=None,
                 stage_one=True):
    """QLDPCBPDecoder.call (decoding_q.py:661-797) in float64 with the reference's batch-minor edge tensors.  synd_x [B,m_x] / synd_z
    [B,m_z]; llr_ch [B,3,n] (x, y, z planes) or llr_const for every qubit and plane; msg_init = (msg_x [B,E_x], msg_z [B,E_z]): the c->v
    messages to start from, VN-major (the reference starts from zeros, :726-727).  The soft syndromes are over hz / hx (stage_one,
    :35-37) or hx_perp / hz_perp.  Returns dict(llr [B,3,n], x_hat, z_hat [B,n], x_logit, z_logit [B,rows], msg_x [B,E_x], msg_z
    [B,E_z], llr_x, llr_z [B,n]: the binary LLRs the soft syndromes are formed from), the soft outputs in float64."""
    hx, hz = np.asarray(code.hx), np.asarray(code.hz)
    sx, sz = np.asarray(synd_x), np.asarray(synd_z)
    B, n = sx.shape[0], hx.shape[1]
    sides = [_bp4_side(hx), _bp4_side(hz)]
    syndrome = [((-1.0) ** s.T.astype(_D))[d["cn_chk"]] for s, d in zip((sx, sz), sides)]  # 0 -> +1, 1 -> -1 (:720-721)
    if llr_ch is None:
        L = np.full((3, n, B), _D(F(llr_const)))
    else:  # [3,n,B] (:716); the input clip of :705-708 is commented out in the reference
        L = np.transpose(np.asarray(llr_ch, F), (1, 2, 0)).astype(_D)
    fac = _D(F(factor))
    if msg_init is None:
        msg = [np.zeros((d["var"].size, B)) for d in sides]
    else:
        msg = [np.asarray(m, F).T.astype(_D) for m in msg_init]

    def vn_sum(m, var):
        idx = (var[:, None] * B + np.arange(B)[None, :]).ravel()
        return np.bincount(idx, weights=m.ravel(), minlength=n * B).reshape(n, B)

    def totals():  # (:244-248): X = sum of hz messages + llr_x, Z = sum of hx messages + llr_z, Y = both + llr_y
        Sz, Sx = vn_sum(msg[1], sides[1]["var"]), vn_sum(msg[0], sides[0]["var"])
        return Sz + L[0], (Sz + Sx) + L[1], Sx + L[2]

    def softplus(t):
        return np.logaddexp(0.0, t)

    for _ in range(num_iter):
        X, Y, Z = totals()
        vx, vz = sides[0]["var"], sides[1]["var"]
        # _vn_update (:250-273): an hx edge sends softplus(-X) - logsumexp(-(Z - mu), -(Y - mu)), an hz edge softplus(-Z) -
        # logsumexp(-(X - mu), -(Y - mu)), mu = the edge's own incoming c->v message
        nu = [softplus(-X)[vx] - np.logaddexp(-(Z[vx] - msg[0]), -(Y[vx] - msg[0])),
              softplus(-Z)[vz] - np.logaddexp(-(X[vz] - msg[1]), -(Y[vz] - msg[1]))]
        for s, d in enumerate(sides):  # CN-order gather, check rule, normalization, gather back (:752-767)
            msg[s] = (_bp4_cn(cn_type, nu[s][d["to_cn"]], d["seg"], d["starts"], syndrome[s]) * fac)[d["inv"]]
    X, Y, Z = totals()  # the sum_only pass (:777)
    dec = np.argmin(np.stack([np.zeros_like(X), X, Z, Y], 0), axis=0)  # (:783-790), the first minimum wins
    llr_z = softplus(-X) - np.logaddexp(-Z, -Y)  # cal_logit (:455-464)
    llr_x = softplus(-Z) - np.logaddexp(-X, -Y)
    xp, zp = (hz, hx) if stage_one else (code.hx_perp, code.hz_perp)
    return dict(llr=np.ascontiguousarray(np.stack([X, Y, Z], 0).transpose(2, 0, 1)),
                x_hat=(dec & 1).T.astype(np.uint8), z_hat=(dec >> 1).T.astype(np.uint8),
                x_logit=np.ascontiguousarray(_bp4_soft_syndrome(xp, llr_x).T),
                z_logit=np.ascontiguousarray(_bp4_soft_syndrome(zp, llr_z).T),
                msg_x=np.ascontiguousarray(msg[0].T), msg_z=np.ascontiguousarray(msg[1].T),
                llr_x=np.ascontiguousarray(llr_x.T), llr_z=np.ascontiguousarray(llr_z.T))
