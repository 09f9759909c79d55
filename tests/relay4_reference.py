"""Relay-BP4 (fgnn_relay4_decode, include/fgnn.h) restated: NumPy float32 for the memory term, the decision, the parity tests, the integer
weight and the leg control; every BP4 step is ONE call of the CPU oracle with num_iter = 1,

    OracleGraph.bp4_decode(..., num_iter=1, cn_type="minsum", llr_ch=Lam, msg_init=(mu_x, mu_z), return_msgs=True)

which runs the qubit update on Lam, the min-sum check update, and returns the next messages and llr = the next marginals M (the sums
of the new messages plus Lam): the chaining property include/fgnn.h states at fgnn_bp4_decode_trace.  So no softplus or log-sum-exp is
restated here, and the kernel is held to this restatement bit for bit.  Samples are independent, so the batch walks the legs in
lock-step: a sample that ends a leg early waits, masked out, for the others."""
import numpy as np

F32 = np.float32
LLR_OF_DECISION = np.array([0, 0, 2, 1])  # decision d (1 = X, 2 = Z, 3 = Y) -> row of llr_ch [., 3, n] (X, Y, Z)


def weights_q(lam):
    """q [B,3,n] int64 = rint(1024 * clamp(lam, -20, 20)), rows X, Y, Z."""
    return np.rint(F32(1024.0) * np.minimum(np.maximum(lam, F32(-20.0)), F32(20.0))).astype(np.int32).astype(np.int64)


def decisions(M):
    """d [B,n] = argmin(0, M^X, M^Z, M^Y), the first minimum wins (BP4's rule: strict comparisons in that order)."""
    cand = np.stack([np.zeros_like(M[:, 0]), M[:, 0], M[:, 2], M[:, 1]], axis=0)
    return np.argmin(cand, axis=0).astype(np.uint8)


def weight_of(d, q):
    """sum_v q^{d_v}_v with q^I = 0."""
    pick = np.take_along_axis(q, LLR_OF_DECISION[d][:, None, :], axis=1)[:, 0, :]
    return np.where(d != 0, pick, 0).sum(1)


def relay4_decode(og, synd_x, synd_z, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0):
    """`og`: the OracleGraph of the code.  Returns (x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32, solutions):
    solutions[b] = [(weight, leg, k), ...] in the order met."""
    hx, hz = np.asarray(og.code.hx, np.int64) % 2, np.asarray(og.code.hz, np.int64) % 2
    n = hx.shape[1]
    gamma = np.asarray(gamma, F32)
    num_legs = gamma.shape[0]
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B = synd_x.shape[0]
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    q = weights_q(lam)

    M = lam.copy()
    found = np.zeros(B, np.int64)
    best = np.zeros((B, 3), np.int64)          # weight, leg, k of the best solution
    hard = np.zeros((B, n), np.uint8)          # its decisions d
    last_d = np.zeros((B, n), np.uint8)        # the last test made
    last = np.zeros((B, 3), np.int64)
    solutions = [[] for _ in range(B)]
    alive = np.ones(B, bool)
    for r in range(num_legs):
        if not alive.any():
            break
        T = pre_iter if r == 0 else leg_iter
        g = gamma[r][None, None, :]
        om = F32(1.0) - g
        mux, muz = np.zeros((B, og.E_x), F32), np.zeros((B, og.E_z), F32)
        Mnext = np.zeros_like(M)
        run = alive.copy()
        for k in range(T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            if k > 0:
                M[idx] = Mnext[idx]
                d = decisions(M[idx])
                x, z = (d & 1).astype(np.int64), (d >> 1).astype(np.int64)
                ok = ((x @ hz.T) % 2 == synd_z[idx]).all(1) & ((z @ hx.T) % 2 == synd_x[idx]).all(1)
                w = weight_of(d, q[idx])
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
                idx = idx[~ended]
                if len(idx) == 0:
                    break
            Lam = om * lam[idx] + g * M[idx]
            assert Lam.dtype == F32 and M.dtype == F32
            out = og.bp4_decode(synd_x[idx], synd_z[idx], 1, "minsum", float(factor), llr_ch=Lam, msg_init=(mux[idx], muz[idx]),
                                return_msgs=True)
            mux[idx], muz[idx], Mnext[idx] = out["msg_x"], out["msg_z"], out["llr"]
            dn = decisions(out["llr"])
            assert np.array_equal(dn & 1, out["x_hat"]) and np.array_equal(dn >> 1, out["z_hat"]), "the oracle decides by the same rule"
        alive &= found < stop_nconv
    none = found == 0
    hard[none] = last_d[none]
    best[none] = last[none]
    stats = np.concatenate([found[:, None], best], axis=1).astype(np.int32)
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats, solutions
