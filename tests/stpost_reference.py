"""Post-processing of unsolved space-time BP4 windows restated in NumPy float32 (a plain module: tests import it, pytest does not).

`stbp4_decode_soft` is the loop of `stbp4_reference.stbp4_decode` that also keeps the totals (X, Y, Z) of every qubit and the Gamma of
every time variable of a window's last test, the soft outputs of fgnn_stbp4_decode_soft (zeros for solved windows).  `window_matrix`,
`window_problem` and `window_apply` restate the layout of fgnn_st_window_problem / fgnn_st_window_apply (include/fgnn.h): check (c,t)
is row t m + c, data bit (v,t) column t n + v, time bit (c,t) column R n + t m + c.  The binary LLRs are vn_llr_z / vn_llr_x of
fgnn_vn.h on the float32 softplus and lse2 of tests/mbp4_reference.py (the oracle's transcendentals).  `post_decode` is
`SpaceTimePostDecoder.decode`: LSD by `lsd_reference.lsd_decode`, OSD-0 by `osd0`, the elimination of the existing OSD restatement
(tests/test_osd_search_cpu.py, `eliminate`) on rows kept as Python ints, which tests/test_stpost_reference_cpu.py ties to it."""
import numpy as np

import mbp4_reference as MB
import stbp4_reference as ST
from lsd_reference import Matrix, lsd_decode, sortable
from mbp4_reference import F32, _f

INF = float("inf")


def stbp4_decode_soft(code, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, prev_x=None, prev_z=None,
                      llr_ch=None, llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=INF, gamma_z=INF, gamma_last_x=INF,
                      gamma_last_z=INF):
    """`stbp4_reference.stbp4_decode` with three more results: marg [B,R,3,n], gam_x [B,R,m_x], gam_z [B,R,m_z] float32."""
    assert cn_type in ST.CN_TYPES and len(factors) == len(owns) >= 1
    G = MB.graph_of(code)
    n = G.n
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B, R = synd_x.shape[:2]
    assert synd_x.shape == (B, R, G.x.m) and synd_z.shape == (B, R, G.z.m)
    X = ST._SideState(G.x, ST.window_gammas(B, R, G.x.m, synd_llr_x, gamma_x, gamma_last_x), ST.differences(synd_x, prev_x))
    Z = ST._SideState(G.z, ST.window_gammas(B, R, G.z.m, synd_llr_z, gamma_z, gamma_last_z), ST.differences(synd_z, prev_z))
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    hard = np.zeros((B, R, n), np.uint8)
    ux, uz = np.zeros((B, R, G.x.m), np.uint8), np.zeros((B, R, G.z.m), np.uint8)
    marg = np.zeros((B, R, 3, n), F32)
    gam_x, gam_z = np.zeros((B, R, G.x.m), F32), np.zeros((B, R, G.z.m), F32)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)

    def gammas(S, idx):  # Gamma_{c,t} = (gamma + w_dn) + w_up_{c,t+1} for t < R-1, gamma + w_dn for t = R-1
        Gm = _f(S.g[idx] + S.wdn[idx])
        Gm[:, :R - 1] = _f(Gm[:, :R - 1] + S.wup[idx][:, 1:])
        return Gm

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
            lamr = np.repeat(lam[idx], R, axis=0)
            nux, nuz = G.qubit_update(X.mu[idx].reshape(N * R, -1), Z.mu[idx].reshape(N * R, -1), lamr, F32(owns[a]))
            X.check_update(idx, nux.reshape(N, R, -1), cn_type, F32(factors[a]))
            Z.check_update(idx, nuz.reshape(N, R, -1), cn_type, F32(factors[a]))
            tot = G.totals(X.mu[idx].reshape(N * R, -1), Z.mu[idx].reshape(N * R, -1), lamr)
            dn = MB.decisions(*tot).reshape(N, R, n)
            gx, gz = gammas(X, idx), gammas(Z, idx)
            uxk, uzk = (gx < 0).astype(np.uint8), (gz < 0).astype(np.uint8)
            assert np.array_equal(uxk, X.u_hat(idx)) and np.array_equal(uzk, Z.u_hat(idx))
            ok = ST.window_test(code, dn & 1, dn >> 1, uxk, uzk, X.d[idx], Z.d[idx])
            hard[idx], ux[idx], uz[idx] = dn, uxk, uzk
            marg[idx] = np.stack([t.reshape(N, R, n) for t in tot], axis=2)
            gam_x[idx], gam_z[idx] = gx, gz
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    solved = stats[:, 0] == 1
    marg[solved], gam_x[solved], gam_z[solved] = 0, 0, 0
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), ux, uz, stats, marg, gam_x, gam_z


def window_matrix(h, rounds):
    """H_st [R m, R (n + m)] uint8 of one side: h on the block diagonal, time bits (c,t) and (c,t-1) in row (c,t)."""
    h = (np.asarray(h) != 0).astype(np.uint8)
    m, n = h.shape
    R = int(rounds)
    H = np.zeros((R * m, R * (n + m)), np.uint8)
    for t in range(R):
        for c in range(m):
            H[t * m + c, t * n:(t + 1) * n] = h[c]
            H[t * m + c, R * n + t * m + c] = 1
            if t > 0:
                H[t * m + c, R * n + (t - 1) * m + c] = 1
    return H


def vn_llr_z(X, Y, Z):
    return _f(MB.softplus(-X) - MB.lse2(-Z, -Y))


def vn_llr_x(X, Y, Z):
    return _f(MB.softplus(-Z) - MB.lse2(-X, -Y))


def window_problem(side, synd, prev, marg, gam, index):
    """(d [nact, R m] uint8, llr [nact, R (n + m)] float32) of the windows `index`: synd [B,R,m] (None: zero), prev [B,m] or None,
    marg [B,R,3,n], gam [B,R,m]."""
    marg, gam = np.asarray(marg, F32), np.asarray(gam, F32)
    B, R, m = gam.shape
    n = marg.shape[3]
    index = np.asarray(index, np.int64)
    if len(index) == 0:
        return np.zeros((0, R * m), np.uint8), np.zeros((0, R * (n + m)), F32)
    s = np.zeros((B, R, m), np.uint8) if synd is None else np.asarray(synd, np.uint8)
    d = ST.differences(s, prev)[index].reshape(len(index), R * m)
    mg = np.ascontiguousarray(marg[index])
    X, Y, Z = (np.ascontiguousarray(mg[:, :, i]).reshape(len(index), R * n) for i in range(3))
    data = vn_llr_z(X, Y, Z) if side == 0 else vn_llr_x(X, Y, Z)
    return d.astype(np.uint8), np.concatenate([data, gam[index].reshape(len(index), R * m)], axis=1).astype(F32)


def window_apply(e, index, hat, u_hat):
    """hat [B,R,n] and u_hat [B,R,m] with the rows `index` replaced by the solutions e [nact, R (n + m)]; the others as they were."""
    hat, u_hat = hat.copy(), u_hat.copy()
    B, R, n = hat.shape
    m = u_hat.shape[2]
    for i, b in enumerate(np.asarray(index, np.int64)):
        hat[b] = e[i, :R * n].reshape(R, n)
        u_hat[b] = e[i, R * n:].reshape(R, m)
    return hat, u_hat


class PackedRows:
    """H [m, n] with every row as a Python int (bit v = column v), for `osd0`."""

    def __init__(self, H):
        H = np.asarray(H) != 0
        self.m, self.n = H.shape
        self.cols = [np.nonzero(H[c])[0] for c in range(self.m)]


def osd0(H, synd, r):
    """OSD-0 of one sample on all rows of H (fgnn_osd0 with the basis of all rows): `eliminate` of tests/test_osd_search_cpu.py with
    the rows of the column-sorted augmented matrix as Python ints (bit p = sorted position p, bit n = the syndrome), then candidate 0:
    e[pivot of row i] = the reduced syndrome bit, every other bit 0."""
    P = H if isinstance(H, PackedRows) else PackedRows(H)
    m, n = P.m, P.n
    r = np.asarray(r, F32) + F32(0.0)
    order = np.argsort(sortable(r), kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    rows = []
    for c in range(m):
        x = (int(synd[c]) & 1) << n
        for p in pos[P.cols[c]].tolist():
            x |= 1 << p
        rows.append(x)
    piv = [0] * m
    for i in range(m):
        x = rows[i]
        p = (x & -x).bit_length() - 1 if x else 0
        piv[i] = p
        bit = 1 << p
        if x & bit:
            for j in range(m):
                if j != i and rows[j] & bit:
                    rows[j] ^= x
    e = np.zeros(n, np.uint8)
    for i in range(m):
        if piv[i] < n and (rows[i] >> piv[i]) & 1:
            e[order[piv[i]]] = (rows[i] >> n) & 1
    return e


def post_decode(code, synd_x, synd_z, factors, owns, num_iter, cn_type="minsum", restart=True, prev_x=None, prev_z=None, gamma=INF,
                gamma_last=INF, llr_ch=None, llr_const=0.0, method="lsd", max_pivots=0, max_rounds=0, fallback="osd0", lds_caps=(0, 0),
                cache=None):
    """`SpaceTimePostDecoder.decode`: (x_hat, z_hat, u_x_hat, u_z_hat, stats, post_stats [2,B,4], windows post-processed, windows handed
    to the fallback).  `lds_caps` = `lsd_max_pivots` of the two window graphs, what max_pivots = 0 means on the device (0: min(m, n));
    `cache` (a dict) keeps the window matrices between calls."""
    assert method in ("lsd", "osd0") and fallback in ("osd0", None)
    xh, zh, uxh, uzh, stats, marg, gx, gz = stbp4_decode_soft(
        code, synd_x, synd_z, factors, owns, num_iter, num_iter, cn_type, restart, prev_x, prev_z, llr_ch, llr_const, None, None, gamma,
        gamma, gamma_last, gamma_last)
    B, R = synd_x.shape[:2]
    post = np.zeros((2, B, 4), np.int32)
    post[:, :, 0] = 1
    index = np.nonzero(stats[:, 0] == 0)[0]
    nact, nfall = len(index), 0
    if nact:
        cache = {} if cache is None else cache
        sides = ((code.hx, synd_x, prev_x, gx, zh, uxh), (code.hz, synd_z, prev_z, gz, xh, uzh))
        work = []
        lsd_stats = np.zeros((2, nact, 4), np.int32)
        lsd_stats[:, :, 0] = 1
        for side, (h, synd, prev, gam, _, _) in enumerate(sides):
            if (side, R) not in cache:
                H = window_matrix(h, R)
                cache[(side, R)] = (H, Matrix(H), PackedRows(H))
            H, M, P = cache[(side, R)]
            d, llr = window_problem(side, synd, prev, marg, gam, index)
            e = np.zeros((nact, H.shape[1]), np.uint8)
            for i in range(nact):
                if method == "lsd":
                    e[i], lsd_stats[side, i] = lsd_decode(M, d[i], llr[i], max_pivots or lds_caps[side], max_rounds)
                else:
                    e[i] = osd0(P, d[i], llr[i])
            work.append((P, d, llr, e))
        found = (lsd_stats[:, :, 0] != 0).all(0)
        if method == "lsd" and fallback == "osd0":
            missed = np.nonzero(~found)[0]
            nfall = len(missed)
            for P, d, llr, e in work:
                for i in missed:
                    e[i] = osd0(P, d[i], llr[i])
            found[:] = True
        out = []
        for side, (_, _, _, _, hat, u_hat) in enumerate(sides):
            out.append(window_apply(work[side][3], index, hat, u_hat))
        (zh, uxh), (xh, uzh) = out
        post[:, index] = lsd_stats
        stats = stats.copy()
        stats[index, 0] = found.astype(np.int32)
    return xh, zh, uxh, uzh, stats, post, nact, nfall


def draw_windows(code, R, B, p, q, seed, perfect_last=True):
    """A seeded batch of memory experiments of R rounds: before each measurement a fresh depolarizing error of rate p joins the
    accumulated one, and every measurement (but the last, if `perfect_last`) flips each bit with probability q.  Returns the raw
    syndromes (synd_x [B,R,m_x], synd_z [B,R,m_z]) uint8."""
    rng = np.random.default_rng(seed)
    hx, hz = np.asarray(code.hx, np.int64) % 2, np.asarray(code.hz, np.int64) % 2
    n = hx.shape[1]
    pauli = rng.choice(4, size=(B, R, n), p=[1 - p, p / 3, p / 3, p / 3])  # 0 I, 1 X, 2 Z, 3 Y
    ex, ez = np.cumsum((pauli == 1) | (pauli == 3), axis=1) % 2, np.cumsum((pauli == 2) | (pauli == 3), axis=1) % 2
    sx, sz = (ez @ hx.T) % 2, (ex @ hz.T) % 2  # hx rows see the Z components, hz rows the X components
    ux, uz = rng.random(sx.shape) < q, rng.random(sz.shape) < q
    if perfect_last:
        ux[:, R - 1], uz[:, R - 1] = False, False
    return (sx ^ ux).astype(np.uint8), (sz ^ uz).astype(np.uint8)
