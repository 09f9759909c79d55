"""Relay-BP with layered legs (fgnn_relay_decode_layered, include/fgnn.h) restated in NumPy float32, vectorised over the batch — what
the kernel is held to bit for bit.

Built from the flooding restatement and the layered one: `relay_reference` gives the slot order (`_Graph`: slots sorted by bit, then
check), a bit's ascending sum from 0.0f (`_bit_sums`) and the min-sum rule (`_minsum`, cn_update<FGNN_CN_MINSUM> operation by
operation); `bp2_layered_reference` gives the layerings (`greedy_bit_layers`, `is_valid_bit_layering`) and the tables of a layer
(`_Layers`).  Every intermediate is np.float32; only IEEE add, multiply, min, max and compare occur.

An iteration k = 1 .. T of a leg: the memory term Lam = (1 - gam) L + gam P on the posteriors the previous iteration (or leg) ended
with, P = Lam + S with S re-summed over the bit's messages (zeros at k = 1), then layer by layer nu = P - mu, mu = min-sum of nu,
P = nu + mu on the edges of the layer's checks (they share no bit, so a layer is one vectorised step), then the test of d = (P < 0).
Samples are independent, so the batch walks the legs in lock-step: a sample that ends a leg early waits, masked out, for the others."""
import types

import numpy as np

from bp2_layered_reference import _Layers, greedy_bit_layers, is_valid_bit_layering
from relay_reference import F32, _Graph, _bit_sums, _minsum


def relay_layered_decode(hx, synd, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0, B=None, layer_of=None):
    """Returns (hard [B,n] uint8, stats [B,4] int32, solutions): solutions[b] = [(weight, leg, k), ...] in the order met.  layer_of
    None: the greedy layering."""
    G = _Graph(hx)
    gamma = np.asarray(gamma, F32)
    num_legs = gamma.shape[0]
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
    # the checks of a layer as a graph of their own for _minsum (it reads m and chk_slots; slot numbers stay those of the codeword)
    layers = [(side, types.SimpleNamespace(m=side.m, chk_slots=G.chk_slots[side.chk])) for side in _Layers(G, num_layers, layer_of).sides]
    factor = F32(factor)
    llr = np.asarray(llr_ch, F32) if llr_ch is not None else np.full((B, G.n), F32(llr_const), F32)
    L = F32(-1.0) * np.minimum(np.maximum(llr, F32(-20.0)), F32(20.0))
    q = np.rint(F32(1024.0) * L).astype(np.int32)
    hxi = G.hx.astype(np.int64)

    P = L.copy()
    found = np.zeros(B, np.int64)
    best = np.zeros((B, 3), np.int64)          # weight, leg, k of the best solution
    hard = np.zeros((B, G.n), np.uint8)
    last_d = np.zeros((B, G.n), np.uint8)      # the last test made
    last = np.zeros((B, 3), np.int64)
    solutions = [[] for _ in range(B)]
    alive = np.ones(B, bool)
    for r in range(num_legs):
        if not alive.any():
            break
        T = pre_iter if r == 0 else leg_iter
        g = gamma[r][None, :]
        om = F32(1.0) - g
        mu = np.zeros((B, G.E), F32)
        run = alive.copy()
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            Lam = om * L[idx] + g * P[idx]
            Pi = Lam + _bit_sums(G, mu[idx])
            mi, si = mu[idx], synd[idx]
            for side, sub in layers:
                nu = Pi[:, side.bits] - mi[:, side.slots]
                nu_all = np.zeros_like(mi)
                nu_all[:, side.slots] = nu
                new = _minsum(sub, nu_all, si[:, side.chk], factor)[:, side.slots]
                mi[:, side.slots] = new
                Pi[:, side.bits] = nu + new
            assert Pi.dtype == F32 and mi.dtype == F32 and Lam.dtype == F32
            P[idx], mu[idx] = Pi, mi
            d = Pi < 0
            ok = ((d.astype(np.int64) @ hxi.T) % 2 == si).all(1)
            w = (d * q[idx].astype(np.int64)).sum(1)
            last_d[idx] = d
            last[idx, 0], last[idx, 1], last[idx, 2] = w, r, k
            for i in np.nonzero(ok)[0]:
                b = idx[i]
                found[b] += 1
                solutions[b].append((int(w[i]), r, k))
                if found[b] == 1 or w[i] < best[b, 0]:
                    best[b] = (w[i], r, k)
                    hard[b] = d[i]
            run[idx[ok]] = False
        alive &= found < stop_nconv
    none = found == 0
    hard[none] = last_d[none]
    best[none] = last[none]
    stats = np.concatenate([found[:, None], best], axis=1).astype(np.int32)
    return hard, stats, solutions
