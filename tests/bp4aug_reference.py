"""Augmented BP4 (fgnn_bp4aug_decode, include/fgnn.h) restated in NumPy float32 on the parts of tests/mbp4_reference.py: `Side`,
`cn_update`, `vn_edge_own` with own = 1 (the product 1.0f * mu is mu bit for bit, so this is vn_edge) and `decisions`, whose every
transcendental is the oracle's.  Its own are the duplicated sum, where the message of a marked check is added a second time directly
after the first, as a separate float32 add, and the marks: dup_c = unit(w(c, a, 5)[0]) < density with `draw` and `unit` of
tests/bp4fb_reference.py.

tests/test_bp4aug_reference_cpu.py ties the result to the oracle: for a fixed set of marked rows the restatement equals BP4 on the
code with those rows inserted once more after their originals, run by `mbp4_reference.mbp4_decode` and by `OracleGraph.bp4_decode`.

Samples are independent: the batch runs in lock-step and a finished sample leaves."""
import numpy as np

import mbp4_reference as MB
from bp4fb_reference import draw, unit

F32 = np.float32
STREAM = 5


def marks(seed, sample, m, a, density):
    """dup_c of attempt a >= 1 for the checks c = 0 .. m - 1 (hx rows first) of global sample `sample`: a float32 compare."""
    d = F32(density)
    return np.array([unit(draw(seed, sample, c, a, STREAM)[0]) < d for c in range(m)], bool)


def vn_sum_dup(side, mu, dup):
    """[B,n]: the sum of a qubit's messages, ascending over its slots from 0.0f; a slot whose check is marked in dup [B,m] is added
    twice in a row."""
    S = np.zeros((mu.shape[0], side.n), F32)
    for j in range(side.vn_tab.shape[1]):
        e = side.vn_tab[:, j]
        mj = mu[:, e]
        S = np.where(side.vn_mask[:, j], MB._f(S + mj), S)
        S = np.where(side.vn_mask[:, j] & dup[:, side.c_of[e]], MB._f(S + mj), S)
    return S


def totals(G, mux, muz, lam, dupx, dupz):
    Sz, Sx = vn_sum_dup(G.z, muz, dupz), vn_sum_dup(G.x, mux, dupx)
    Y = MB._f(MB._f(Sz + Sx) + lam[:, 1])
    X = MB._f(Sz + lam[:, 0])
    Z = MB._f(Sx + lam[:, 2])
    return X, Y, Z


def step(G, mux, muz, lam, synd_x, synd_z, cn_type, factor, dupx, dupz):
    """One iteration on the duplicated sums: qubit update (the edge's own message taken out once), check update * factor; returns the
    new messages and the decisions of their marginals."""
    X, Y, Z = totals(G, mux, muz, lam, dupx, dupz)
    numx, numz = MB.softplus(-X), MB.softplus(-Z)
    vx, vz = G.x.v_of, G.z.v_of
    nux = MB.vn_edge_own(numx[:, vx], Z[:, vx], Y[:, vx], mux, 1.0)
    nuz = MB.vn_edge_own(numz[:, vz], X[:, vz], Y[:, vz], muz, 1.0)
    mux, muz = MB.cn_update(G.x, nux, synd_x, cn_type, factor), MB.cn_update(G.z, nuz, synd_z, cn_type, factor)
    return mux, muz, MB.decisions(*totals(G, mux, muz, lam, dupx, dupz))


def bp4aug_decode(code, synd_x, synd_z, pre_iter, attempt_iter, max_attempts, density, cn_type="minsum", factor=1.0, restart=True,
                  seed=0x5EED, first_sample=0, llr_ch=None, llr_const=0.0, fixed=None, log=None):
    """`code`: an object with hx and hz.  Returns (x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, the a of the last
    test, iterations, the k of the last test).  `fixed`: a bool array [m_x + m_z] that stands in for the draw of every attempt a >= 1
    (the tests that compare with an explicitly augmented code).  `log`: a list that receives (b, a, marks [m]) per draw."""
    assert cn_type in MB.CN_TYPES
    G = MB.graph_of(code)
    n, m_x, m = G.n, G.x.m, G.x.m + G.z.m
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B, A = synd_x.shape[0], int(max_attempts)
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    mux, muz = np.zeros((B, G.x.E), F32), np.zeros((B, G.z.E), F32)
    dup = np.zeros((B, m), bool)
    hard = np.zeros((B, n), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for a in range(A + 1):
        T = pre_iter if a == 0 else attempt_iter
        if a > 0:
            for b in np.nonzero(run)[0]:
                dup[b] = fixed if fixed is not None else marks(seed, int(first_sample) + int(b), m, a, density)
                if log is not None:
                    log.append((int(b), a, dup[b].copy()))
            if restart:
                mux[:], muz[:] = 0, 0
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            mux[idx], muz[idx], dn = step(G, mux[idx], muz[idx], lam[idx], synd_x[idx], synd_z[idx], cn_type, F32(factor),
                                          dup[idx, :m_x], dup[idx, m_x:])
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ G.hz.T) % 2 == synd_z[idx]).all(1) & ((z @ G.hx.T) % 2 == synd_x[idx]).all(1)
            hard[idx] = dn
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats


def doubled_code(code, dup):
    """(hx', hz', rx, rz): hx and hz with every row marked in dup [m_x + m_z] inserted once more directly after itself, and the row
    indices rx, rz into the original sides (a syndrome [B,m] of the doubled code is synd[:, r])."""
    hx, hz = np.asarray(code.hx, np.uint8) % 2, np.asarray(code.hz, np.uint8) % 2
    dup = np.asarray(dup, bool)
    rx = np.repeat(np.arange(hx.shape[0]), 1 + dup[:hx.shape[0]].astype(np.int64))
    rz = np.repeat(np.arange(hz.shape[0]), 1 + dup[hx.shape[0]:].astype(np.int64))
    return hx[rx], hz[rz], rx, rz
