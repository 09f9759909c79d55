"""BP-GDG (fgnn_gdg_decode, include/fgnn.h) restated in NumPy float32: one path at a time, vectorised over the samples.

The check rule, the slot order and the bit sums are those of tests/relay_reference.py (`_Graph`, `_bit_sums`, `_minsum`), so the
min-sum step has one definition.  Every intermediate is np.float32; only IEEE add, multiply, min, max, abs and compare occur, the
pick is the first extremum of |P| over the free bits in index order and the weight is an integer, so the kernel is held to this
restatement bit for bit.  Paths never interact: `run_path` walks one path of every sample (a sample whose path has stopped waits,
masked out, for the others) and `gdg_decode` calls it once per path and then applies the selection rule."""
import numpy as np

from relay_reference import F32, _Graph, _bit_sums, _minsum

MOST, LEAST = 0, 1
TAILS = {"most": MOST, "least": LEAST}


def priors(n, B, llr_ch, llr_const):
    """L [B,n] float32 = -clamp(llr, -20, 20) and q = (int32) rint(1024 L)."""
    llr = np.asarray(llr_ch, F32) if llr_ch is not None else np.full((B, n), F32(llr_const), F32)
    L = F32(-1.0) * np.minimum(np.maximum(llr, F32(-20.0)), F32(20.0))
    return L, np.rint(F32(1024.0) * L).astype(np.int32)


def run_path(G, L, q, synd, pre_iter, round_iter, R, tail, D, factor, guesses):
    """One path of every sample.  `guesses` = the bits the first len(guesses) picks are flipped by (path p at depth d: bit r of p for
    r < d); those picks take the least reliable bit, the later ones follow `tail`.
    Returns (d [B,n] uint8, res [B,4] int64 = found, w or 0, bits fixed, its)."""
    B, n = L.shape
    D, factor = F32(D), F32(factor)
    hxi = G.hx.astype(np.int64)
    mu = np.zeros((B, G.E), F32)
    Lhat = L.copy()
    P = L.copy()
    free = np.ones((B, n), bool)
    d_out = np.zeros((B, n), np.uint8)
    res = np.zeros((B, 4), np.int64)
    run = np.ones(B, bool)
    for r in range(R + 1):
        T = pre_iter if r == 0 else round_iter
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            S = _bit_sums(G, mu[idx])
            x = S + Lhat[idx]
            nu = x[:, G.slot_bit] - mu[idx]
            mu[idx] = _minsum(G, nu, synd[idx], factor)
            res[idx, 3] += 1
            Pn = Lhat[idx] + _bit_sums(G, mu[idx])
            assert Pn.dtype == F32 and nu.dtype == F32
            P[idx] = Pn
            d = Pn < 0
            d_out[idx] = d
            res[idx, 2] = r
            ok = ((d.astype(np.int64) @ hxi.T) % 2 == synd[idx]).all(1)
            res[idx[ok], 0] = 1
            res[idx[ok], 1] = (d[ok] * q[idx[ok]].astype(np.int64)).sum(1)
            run[idx[ok]] = False
        idx = np.nonzero(run)[0]
        if r == R or len(idx) == 0:
            break
        guessing = r < len(guesses)
        a = np.abs(P[idx])
        if guessing or tail == LEAST:
            v = np.argmin(np.where(free[idx], a, F32(np.inf)), axis=1)    # the first minimum: lowest index on ties
        else:
            v = np.argmax(np.where(free[idx], a, F32(-1.0)), axis=1)
        val = P[idx, v] < 0
        if guessing:
            val = val ^ bool(guesses[r])
        free[idx, v] = False
        Lhat[idx, v] = np.where(val, -D, D).astype(F32)
    return d_out, res


def select(res):
    """The selection rule on res [B,P,4]: (path [B], stats [B,4]): lowest w among the paths that found a solution, ties to the lowest
    path; path 0 where none did."""
    B, P, _ = res.shape
    path = np.zeros(B, np.int64)
    stats = np.zeros((B, 4), np.int64)
    for b in range(B):
        cand = [(int(res[b, p, 1]), p) for p in range(P) if res[b, p, 0]]
        p = min(cand)[1] if cand else 0
        path[b] = p
        stats[b] = (len(cand), res[b, p, 1] if cand else 0, p, res[b, p, 2])
    return path, stats


def gdg_decode(hx, synd, pre_iter, round_iter, max_rounds, depth, tail="least", decim_llr=25.0, factor=0.8, llr_ch=None, llr_const=0.0,
               B=None, index=None, out=None, want_paths=False):
    """Returns (hard [B,n] uint8, stats [B,4] int32, path_stats [nact,P,4] int32).  `index`: the listed samples only; the rows of the
    others are those of `out` = (hard, stats), which is copied (zeros without it).  `want_paths`: also the decisions of every path,
    [nact,P,n] uint8."""
    G = hx if isinstance(hx, _Graph) else _Graph(hx)
    tail = TAILS.get(tail, tail)
    if synd is None:
        B = llr_ch.shape[0] if B is None else B
        synd = np.zeros((B, G.m), np.uint8)
    synd = np.asarray(synd, np.uint8) & 1
    B = synd.shape[0]
    L, q = priors(G.n, B, llr_ch, llr_const)
    sel = np.arange(B) if index is None else np.asarray(index, np.int64)
    P, R = 1 << depth, min(max_rounds, G.n)
    hard = np.zeros((B, G.n), np.uint8) if out is None else np.array(out[0], np.uint8)
    stats = np.zeros((B, 4), np.int32) if out is None else np.array(out[1], np.int32)
    d = np.zeros((len(sel), P, G.n), np.uint8)
    res = np.zeros((len(sel), P, 4), np.int64)
    if len(sel):
        for p in range(P):
            d[:, p], res[:, p] = run_path(G, L[sel], q[sel], synd[sel], pre_iter, round_iter, R, tail, decim_llr, factor,
                                          [(p >> r) & 1 for r in range(depth)])
        path, st = select(res)
        hard[sel] = d[np.arange(len(sel)), path]
        stats[sel] = st
    return (hard, stats, res.astype(np.int32)) + ((d,) if want_paths else ())
