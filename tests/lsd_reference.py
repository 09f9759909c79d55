"""A NumPy / Python-int restatement of LSD-0 with synchronous growth, the contract of `fgnn_lsd` in include/fgnn.h, operation by
operation (a plain module: tests import it, pytest does not).  Vectors over the m checks are Python ints (bit c = check c)."""
import numpy as np


def sortable(r):
    """The order-preserving float32 -> uint32 map of fgnn_osd.hip, after r + 0.0f (-0 -> +0)."""
    r = np.asarray(r, np.float32) + np.float32(0.0)
    u = np.ascontiguousarray(r).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keys(r):
    """key(v) = (sortable(r[v]) << 32) | v as Python ints."""
    return [(int(s) << 32) | v for v, s in enumerate(sortable(r))]


class Matrix:
    """H [m, n] as the adjacency lists and column bit vectors the walk reads (built once per matrix)."""

    def __init__(self, H):
        H = np.asarray(H) != 0
        self.m, self.n = H.shape
        self.rows = [np.nonzero(H[c])[0].tolist() for c in range(self.m)]
        self.cols = [np.nonzero(H[:, v])[0].tolist() for v in range(self.n)]
        self.colbits = [sum(1 << c for c in cs) for cs in self.cols]


def lsd_decode(H, s, r, max_pivots=0, max_rounds=0, trace=None):
    """One sample: (e [n] uint8, [found, rounds, columns, pivots]).  `max_pivots` = 0: min(m, n); `max_rounds` = 0: no limit.
    `trace` (a dict) receives the final state: piv, col, the appended bits in order, the labels, the dead labels."""
    M = H if isinstance(H, Matrix) else Matrix(H)
    m, n = M.m, M.n
    cap = max_pivots or min(m, n)
    key = keys(r)
    s = np.asarray(s).astype(np.int64) & 1
    t = sum(1 << c for c in range(m) if s[c])
    lab = [c if s[c] else -1 for c in range(m)]
    inB = [False] * n
    is_pivot = 0
    piv, col, L, appended = [], [], [], []
    dead = set()
    rounds = columns = 0
    capped = False

    def invalid():
        bad = t & ~is_pivot
        return {lab[c] for c in range(m) if lab[c] >= 0 and (bad >> c) & 1}

    while True:
        grow = invalid() - dead
        if not grow or capped or (max_rounds and rounds >= max_rounds):
            break
        rounds += 1
        S = set()
        checks_of = {l: [] for l in grow}
        for c in range(m):
            if lab[c] in checks_of:
                checks_of[lab[c]].append(c)
        for l in grow:  # select, on the state at the start of the round
            best = None
            for c in checks_of[l]:
                for v in M.rows[c]:
                    if not inB[v] and (best is None or key[v] < best):
                        best = key[v]
            if best is None:
                dead.add(l)
            else:
                S.add(best)
        for k in sorted(S):  # append in ascending key order
            v = k & 0xFFFFFFFF
            inB[v] = True
            appended.append(v)
            old = {lab[c] for c in M.cols[v] if lab[c] >= 0}
            members = [c for c in range(m) if lab[c] in old] + M.cols[v]
            new = min(members)
            for c in members:
                lab[c] = new
            columns += 1
            x = M.colbits[v]
            for j in range(len(piv)):
                if (x >> piv[j]) & 1:
                    x ^= L[j] & ~(1 << piv[j])
            free = x & ~is_pivot
            if free == 0:
                continue
            if len(piv) == cap:
                capped = True
                break
            p = (free & -free).bit_length() - 1
            piv.append(p)
            col.append(v)
            L.append(x)
            is_pivot |= 1 << p
            if (t >> p) & 1:
                t ^= x & ~(1 << p)
    e = np.zeros(n, np.uint8)
    for p, v in zip(piv, col):
        e[v] = (t >> p) & 1
    if trace is not None:
        trace.update(piv=piv, col=col, appended=appended, lab=lab, dead=dead)
    return e, [int(not invalid()), rounds, columns, len(piv)]


def lsd_batch(H, synd, r, max_pivots=0, max_rounds=0, ids=None):
    """(e_hat [B, n] uint8, stats [B, 4] int32) of the samples `ids` (None: all); the rows of the others are zero."""
    M = H if isinstance(H, Matrix) else Matrix(H)
    synd, r = np.asarray(synd), np.asarray(r)
    B = synd.shape[0]
    e = np.zeros((B, M.n), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    for b in (range(B) if ids is None else ids):
        e[b], stats[b] = lsd_decode(M, synd[b], r[b], max_pivots, max_rounds)
    return e, stats

