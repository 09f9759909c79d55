"""BP-SI (fgnn_si_decode, include/fgnn.h) restated in NumPy float32, vectorised over the samples.

The check rule, the slot order and the bit sums are those of tests/relay_reference.py (`_Graph`, `_bit_sums`, `_minsum`), so the
min-sum step has one definition.  Every intermediate is np.float32; only IEEE add, multiply, min, max, abs and compare occur, the
pick is an integer minimum of key_j = bits(score_j) << 32 | j, and the solve is written out plainly (`solve`: the columns in ascending
order, a column that depends on the earlier ones gets 0), so the kernel is held to this restatement bit for bit.  Samples are
independent: attempt 0 walks the batch in lock-step (a sample that has ended waits, masked out, for the others), the attempts with a
group inactivated run one sample at a time, as each has its own group."""
import numpy as np

from relay_reference import F32, _Graph, _bit_sums, _minsum


def priors(n, B, llr_ch, llr_const):
    """L [B,n] float32 = -1 * clamp(llr, -20, 20)."""
    llr = np.asarray(llr_ch, F32) if llr_ch is not None else np.full((B, n), F32(llr_const), F32)
    return F32(-1.0) * np.minimum(np.maximum(llr, F32(-20.0)), F32(20.0))


def solve(M, r):
    """The contract's solution of M x = r over GF(2), M [rows, cols] and r [rows] of 0/1: the columns are taken in ascending order, a
    column that is a combination of the earlier independent ones gets x = 0, the others are then determined.  Returns x [cols] uint8,
    or None when r is not in the column space."""
    M = (np.asarray(M) != 0).astype(np.uint8)
    rows, cols = M.shape
    A = np.concatenate([M, (np.asarray(r).reshape(rows, 1) != 0).astype(np.uint8)], axis=1)
    used = np.zeros(rows, bool)
    pivot = -np.ones(cols, np.int64)
    for c in range(cols):
        cand = np.nonzero(~used & (A[:, c] == 1))[0]
        if len(cand) == 0:
            continue                       # depends on the earlier columns: x_c = 0
        p = cand[0]
        used[p] = True
        pivot[c] = p
        for i in np.nonzero(A[:, c])[0]:
            if i != p:
                A[i] ^= A[p]
    if A[~used, cols].any():
        return None
    x = np.zeros(cols, np.uint8)
    for c in range(cols):
        if pivot[c] >= 0:
            x[c] = A[pivot[c], cols]
    return x


def group_keys(P, groups):
    """key_j = (bits(score_j) << 32) | j per non-empty group, score_j = ((0 + |P_v0|) + |P_v1|) + ... over its bits ascending, for one
    sample: the (key, j) pairs in ascending key order."""
    keys = []
    for j, I in enumerate(groups):
        if len(I) == 0:
            continue
        s = F32(0.0)
        for v in I:
            s = F32(s + np.abs(P[v]))
        keys.append(((int(np.asarray(s, F32).view(np.uint32)) << 32) | j, j))
    return sorted(keys)


def _plain(G, L, synd, num_iter, factor):
    """Attempt 0 of every sample: (found [B] bool, k [B], d [B,n] uint8 of the test that ended it, P [B,n] of that test)."""
    B = L.shape[0]
    hxi = G.hx.astype(np.int64)
    mu = np.zeros((B, G.E), F32)
    P = L.copy()
    d_out = np.zeros((B, G.n), np.uint8)
    found = np.zeros(B, bool)
    k_out = np.zeros(B, np.int64)
    run = np.ones(B, bool)
    for k in range(num_iter + 1):
        idx = np.nonzero(run)[0]
        if len(idx) == 0:
            break
        S = _bit_sums(G, mu[idx])
        if k > 0:
            Pn = L[idx] + S
            assert Pn.dtype == F32
            P[idx] = Pn
            d = Pn < 0
            d_out[idx] = d
            ok = ((d.astype(np.int64) @ hxi.T) % 2 == synd[idx]).all(1)
            found[idx[ok]] = True
            k_out[idx[ok]] = k
            ended = ok | (k == num_iter)
            run[idx[ended]] = False
            idx, S = idx[~ended], S[~ended]
            if len(idx) == 0:
                break
        x = S + L[idx]
        nu = x[:, G.slot_bit] - mu[idx]
        assert nu.dtype == F32
        mu[idx] = _minsum(G, nu, synd[idx], factor)
    return found, k_out, d_out, P


def _attempt(G, L, synd, I, si_iter, factor):
    """One attempt of one sample with the bits I erased: (k of its last test, e [n] uint8 or None, "solved" | "unsolvable" | "ran out")."""
    hxi = G.hx.astype(np.int64)
    inact = np.zeros(G.n, bool)
    inact[I] = True
    adjacent = G.hx[:, I].any(1)
    erased = inact[G.slot_bit]
    mu = np.zeros((1, G.E), F32)
    L, synd = L[None, :], synd[None, :]
    for k in range(si_iter + 1):
        S = _bit_sums(G, mu)
        if k > 0:
            Pn = L + S
            d = (Pn[0] < 0) & ~inact
            par = (d.astype(np.int64) @ hxi.T) % 2 ^ synd[0]
            if not par[~adjacent].any():
                x = solve(G.hx[np.ix_(adjacent, I)], par[adjacent])
                if x is None:
                    return k, None, "unsolvable"
                e = d.astype(np.uint8)
                e[I] = x
                return k, e, "solved"
            if k == si_iter:
                return k, None, "ran out"
        x = S + L
        nu = x[:, G.slot_bit] - mu
        nu[:, erased] = F32(0.0)
        assert nu.dtype == F32
        mu = _minsum(G, nu, synd, factor)
    raise AssertionError("unreachable")


def si_decode(hx, group_pcm, synd, num_iter, si_iter, max_groups, factor=0.8, llr_ch=None, llr_const=0.0, B=None, index=None, out=None,
              want_trace=False):
    """Returns (hard [B,n] uint8, stats [B,4] int32 = found, attempt, k, group or -1).  The groups are the rows of `group_pcm`.
    `index`: the listed samples only; the rows of the others are those of `out` = (hard, stats), which is copied (zeros without it).
    `want_trace`: also a list per listed sample of what each attempt from 1 on did: (group, k, "solved" | "unsolvable" | "ran out")."""
    G = hx if isinstance(hx, _Graph) else _Graph(hx)
    groups = [np.nonzero(row)[0] for row in (np.asarray(group_pcm) != 0)]
    if synd is None:
        B = llr_ch.shape[0] if B is None else B
        synd = np.zeros((B, G.m), np.uint8)
    synd = np.asarray(synd, np.uint8) & 1
    B = synd.shape[0]
    factor = F32(factor)
    L = priors(G.n, B, llr_ch, llr_const)
    sel = np.arange(B) if index is None else np.asarray(index, np.int64)
    hard = np.zeros((B, G.n), np.uint8) if out is None else np.array(out[0], np.uint8)
    stats = np.zeros((B, 4), np.int32) if out is None else np.array(out[1], np.int32)
    trace = [[] for _ in sel]
    attempts = min(max_groups, sum(len(I) > 0 for I in groups))
    if len(sel):
        found, k0, d0, P0 = _plain(G, L[sel], synd[sel], num_iter, factor)
        for i, b in enumerate(sel):
            hard[b] = d0[i]
            stats[b] = (1, 0, k0[i], -1) if found[i] else (0, attempts, 0, -1)
            if found[i]:
                continue
            for a, (_, j) in enumerate(group_keys(P0[i], groups)[:attempts], start=1):
                k, e, why = _attempt(G, L[b], synd[b], groups[j], si_iter, factor)
                trace[i].append((j, k, why))
                if e is not None:
                    hard[b] = e
                    stats[b] = (1, a, k, j)
                    break
    return (hard, stats, trace) if want_trace else (hard, stats)
