"""Relay-BP (fgnn_relay_decode, include/fgnn.h) restated in NumPy float32, vectorised over the batch.

Every intermediate is np.float32; a bit's sum runs over its slots in ascending order from 0.0f, a check's over its bits in ascending
order; the min-sum rule follows cn_update<FGNN_CN_MINSUM> (feedback_gnn_amd/csrc/fgnn_cn.h) operation by operation.  Only IEEE add,
multiply, min, max and compare occur, so the kernel is held to this restatement bit for bit.  Samples are independent, so the batch
walks the legs in lock-step: a sample that ends a leg early waits, masked out, for the others."""
import numpy as np

F32 = np.float32
LARGE = F32(10000.0)


class _Graph:
    """Slots of hx in VN-major order (sorted by bit, then check), as the library numbers them."""

    def __init__(self, hx):
        self.hx = (np.asarray(hx) != 0)
        self.m, self.n = self.hx.shape
        self.slot_bit, self.slot_chk = np.nonzero(self.hx.T)   # ascending bit, then ascending check
        self.E = len(self.slot_bit)
        self.bit_slots = self._pad(self.slot_bit, self.n, np.arange(self.E))
        order = np.lexsort((self.slot_bit, self.slot_chk))      # by check, then ascending bit
        self.chk_slots = self._pad(self.slot_chk[order], self.m, order)

    @staticmethod
    def _pad(owner, count, slots):
        """[count, max degree] slot numbers of each owner in the given order, -1 where the owner has fewer."""
        deg = np.bincount(owner, minlength=count)
        out = -np.ones((count, max(1, int(deg.max()) if len(deg) else 1)), np.int64)
        pos = np.zeros(count, np.int64)
        for o, s in zip(owner, slots):
            out[o, pos[o]] = s
            pos[o] += 1
        return out


def _bit_sums(G, mu):
    """S_v = ((0 + mu_0) + mu_1) + ... over the bit's slots in ascending order."""
    S = np.zeros((mu.shape[0], G.n), F32)
    for j in range(G.bit_slots.shape[1]):
        has = G.bit_slots[:, j] >= 0
        S[:, has] = S[:, has] + mu[:, G.bit_slots[has, j]]
    return S


def _minsum(G, nu, synd, factor):
    """cn_update<FGNN_CN_MINSUM>: messages nu [B,E] -> mu [B,E]."""
    B = nu.shape[0]
    D = G.chk_slots.shape[1]
    has = G.chk_slots >= 0
    mu = np.zeros_like(nu)
    neg = synd.astype(bool).copy()
    a = np.zeros((B, G.m, D), F32)
    ng = np.zeros((B, G.m, D), bool)
    minv = np.zeros((B, G.m), F32)
    for j in range(D):
        h = has[:, j]
        v = np.minimum(np.maximum(nu[:, G.chk_slots[h, j]], F32(-20.0)), F32(20.0))
        ng[:, h, j] = v < 0
        neg[:, h] ^= ng[:, h, j]
        a[:, h, j] = np.abs(v)
        minv[:, h] = a[:, h, j] if j == 0 else np.minimum(minv[:, h], a[:, h, j])
    min2 = np.zeros((B, G.m), F32)
    nsum = np.zeros((B, G.m), F32)
    for j in range(D):
        h = has[:, j]
        d = a[:, h, j] - minv[:, h]
        d = np.where(d == 0, LARGE, d).astype(F32)
        min2[:, h] = d if j == 0 else np.minimum(min2[:, h], d)
        nsum[:, h] = nsum[:, h] + d
    min2 = min2 + minv
    nsum = nsum - (F32(2.0) * LARGE - F32(1.0))
    sg = np.where(nsum > 0, F32(1.0), np.where(nsum < 0, F32(-1.0), F32(0.0))).astype(F32)
    dm = F32(0.5) * (F32(1.0) - sg)
    min_e = (F32(1.0) - dm) * minv + dm * min2
    for j in range(D):
        h = has[:, j]
        d = a[:, h, j] - minv[:, h]
        out = np.where(d == 0, min_e[:, h], minv[:, h]).astype(F32)
        out = np.where(neg[:, h] ^ ng[:, h, j], -out, out).astype(F32)
        mu[:, G.chk_slots[h, j]] = out * factor
    assert mu.dtype == F32
    return mu


def relay_decode(hx, synd, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0, B=None):
    """Returns (hard [B,n] uint8, stats [B,4] int32, solutions): solutions[b] = [(weight, leg, k), ...] in the order met."""
    G = _Graph(hx)
    gamma = np.asarray(gamma, F32)
    num_legs = gamma.shape[0]
    if synd is None:
        B = llr_ch.shape[0] if B is None else B
        synd = np.zeros((B, G.m), np.uint8)
    synd = np.asarray(synd, np.uint8) & 1
    B = synd.shape[0]
    factor = F32(factor)
    llr = np.asarray(llr_ch, F32) if llr_ch is not None else np.full((B, G.n), F32(llr_const), F32)
    L = F32(-1.0) * np.minimum(np.maximum(llr, F32(-20.0)), F32(20.0))
    q = np.rint(F32(1024.0) * L).astype(np.int32)
    hxi = G.hx.astype(np.int64)

    P = L.copy()
    Lam = np.zeros_like(L)
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
        for k in range(T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            S = _bit_sums(G, mu[idx])
            if k > 0:
                Pn = Lam[idx] + S
                P[idx] = Pn
                d = Pn < 0
                ok = ((d.astype(np.int64) @ hxi.T) % 2 == synd[idx]).all(1)
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
                ended = ok | (k == T)
                run[idx[ended]] = False
                idx, S = idx[~ended], S[~ended]
                if len(idx) == 0:
                    break
            Lam[idx] = om * L[idx] + g * P[idx]
            x = S + Lam[idx]
            nu = x[:, G.slot_bit] - mu[idx]
            assert nu.dtype == F32 and Lam.dtype == F32 and P.dtype == F32
            mu[idx] = _minsum(G, nu, synd[idx], factor)
        alive &= found < stop_nconv
    none = found == 0
    hard[none] = last_d[none]
    best[none] = last[none]
    stats = np.concatenate([found[:, None], best], axis=1).astype(np.int32)
    return hard, stats, solutions
