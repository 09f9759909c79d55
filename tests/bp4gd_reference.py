"""BP4 with guided decimation (fgnn_bp4gd_decode, include/fgnn.h) restated: NumPy float32 for the decimated LLRs, the decision, the
parity tests, the margin, the selection and the round control; every BP4 step is ONE call of the CPU oracle with num_iter = 1,

    OracleGraph.bp4_decode(..., num_iter=1, cn_type, factor, llr_ch=lamhat, msg_init=(mu_x, mu_z), return_msgs=True)

which runs the qubit update on lamhat, the check update, and returns the next messages and llr = the marginals M (the sums of the new
messages plus lamhat).  So no softplus or log-sum-exp is restated here, and the kernel is held to this restatement bit for bit.
Samples are independent and walk the same schedule, so the batch runs in lock-step; a finished sample leaves the calls."""
import numpy as np

F32 = np.float32


def decisions(M):
    """d [B,n] = argmin(0, M^X, M^Z, M^Y), the first minimum wins (BP4's rule: strict comparisons in that order)."""
    cand = np.stack([np.zeros_like(M[:, 0]), M[:, 0], M[:, 2], M[:, 1]], axis=0)
    return np.argmin(cand, axis=0).astype(np.uint8)


def margins(M, d):
    """margin [B,n] = min(c_j, j != d) - c_d with c = (0, M^X, M^Z, M^Y): one float32 subtraction."""
    cand = np.stack([np.zeros_like(M[:, 0]), M[:, 0], M[:, 2], M[:, 1]], axis=-1)  # [B,n,4]
    cd = np.take_along_axis(cand, d[..., None].astype(np.int64), axis=-1)[..., 0]
    others = np.where(np.arange(4)[None, None, :] == d[..., None], F32(np.inf), cand)
    out = others.min(-1) - cd
    assert out.dtype == F32
    return out


def fixed_llrs(d, D):
    """lamhat (X, Y, Z) of a qubit fixed to d: I (+D,+D,+D), X (-D,+0,+0), Z (+0,+0,-D), Y (+0,-D,+0)."""
    D = F32(D)
    z = F32(0.0)
    return {0: (D, D, D), 1: (-D, z, z), 2: (z, z, -D), 3: (z, -D, z)}[int(d)]


def bp4gd_decode(og, synd_x, synd_z, pre_iter, round_iter, max_rounds=None, decim_llr=25.0, cn_type="minsum", factor=1.0,
                 llr_ch=None, llr_const=0.0, tie_log=None):
    """`og`: the OracleGraph of the code.  Returns (x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, qubits fixed,
    iterations, k of the last test; fixed [B,n] int8 = -1 while free, else the Pauli d the qubit was fixed to).  `tie_log`: a list that
    receives, per selection, how many samples had their largest margin at more than one free qubit."""
    hx, hz = np.asarray(og.code.hx, np.int64) % 2, np.asarray(og.code.hz, np.int64) % 2
    n = hx.shape[1]
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B = synd_x.shape[0]
    R = n if max_rounds is None else min(int(max_rounds), n)
    lamhat = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    mux, muz = np.zeros((B, og.E_x), F32), np.zeros((B, og.E_z), F32)
    fixed = np.full((B, n), -1, np.int8)
    hard = np.zeros((B, n), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for r in range(R + 1):
        T = pre_iter if r == 0 else round_iter
        M = d = None
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            out = og.bp4_decode(synd_x[idx], synd_z[idx], 1, cn_type, float(factor), llr_ch=lamhat[idx], msg_init=(mux[idx], muz[idx]),
                                return_msgs=True)
            mux[idx], muz[idx] = out["msg_x"], out["msg_z"]
            M = np.zeros((B, 3, n), F32)
            M[idx] = out["llr"]
            dn = decisions(out["llr"])
            assert np.array_equal(dn & 1, out["x_hat"]) and np.array_equal(dn >> 1, out["z_hat"]), "the oracle decides by the same rule"
            d = np.zeros((B, n), np.uint8)
            d[idx] = dn
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ hz.T) % 2 == synd_z[idx]).all(1) & ((z @ hx.T) % 2 == synd_x[idx]).all(1)
            hard[idx] = dn
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = r, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        idx = np.nonzero(run)[0]
        if len(idx) == 0 or r == R:
            break
        mg = margins(M[idx], d[idx])
        assert (mg >= 0).all() and not np.signbit(mg).any()
        mg = np.where(fixed[idx] < 0, mg, F32(-1.0))  # the free qubits only
        vs = np.argmax(mg, axis=1)  # the first of the largest: lowest index on ties
        if tie_log is not None:
            tie_log.append(int(((mg == mg.max(1, keepdims=True)).sum(1) > 1).sum()))
        for b, v in zip(idx, vs):
            assert fixed[b, v] < 0
            fixed[b, v] = d[b, v]
            lamhat[b, :, v] = fixed_llrs(d[b, v], decim_llr)
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats, fixed
