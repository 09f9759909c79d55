"""BP4 with prior feedback (fgnn_bp4fb_decode, include/fgnn.h) restated: NumPy float32 for the two feedback rules, the decision, the
parity tests and the attempt control; the draws are `oracle.philox` blocks; every BP4 step is ONE call of the CPU oracle with
num_iter = 1,

    OracleGraph.bp4_decode(..., num_iter=1, cn_type, factor, llr_ch=lamhat, msg_init=(mu_x, mu_z), return_msgs=True)

which runs the qubit update on lamhat, the check update, and returns the next messages and llr = the marginals M (the sums of the new
messages plus lamhat).  So no softplus or log-sum-exp is restated here, and the kernel is held to this restatement bit for bit.
Samples are independent and walk the same schedule, so the batch runs in lock-step; a finished sample leaves the calls."""
import numpy as np

from bp4gd_reference import decisions
from oracle.oracle import philox

F32 = np.float32
M32 = 0xFFFFFFFF
STREAM_PERTURB, STREAM_ENHANCED = 3, 4
RULES = ("perturb", "enhanced")


def draw(seed, sample, idx, att, stream):
    """w(idx, att, s): the Philox4x32-10 block at counter (lo32(i), hi32(i), idx, att << 8 | s) under the key (lo32(seed), hi32(seed))."""
    return philox([sample & M32, (sample >> 32) & M32, idx, (att << 8) | stream], [seed & M32, (seed >> 32) & M32])


def unit(x):
    """fg_u32_to_unit: 23 mantissa bits into [1, 2), minus 1.0f."""
    return F32(np.array((int(x) >> 9) | 0x3F800000, np.uint32).view(F32) - F32(1.0))


def fy_pick(u, remaining):
    """fg_fy_pick: min((int)(u * (float) remaining), remaining - 1), the product in float32."""
    return min(int(F32(u) * F32(remaining)), remaining - 1)


def bp4fb_decode(og, synd_x, synd_z, rule, pre_iter, attempt_iter, max_attempts, strength, cn_type="minsum", factor=1.0, restart=False,
                 seed=0x5EED, first_sample=0, llr_ch=None, llr_const=0.0, log=None):
    """`og`: the OracleGraph of the code.  Returns (x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, feedback steps
    made, iterations, k of the last test).  `log`: a list that receives one dict per feedback step of a sample: b, the attempt number
    a + 1 it prepares, d = the decisions of the test it follows, and for "enhanced" the chosen check and qubit."""
    assert rule in RULES
    hx, hz = np.asarray(og.code.hx, np.int64) % 2, np.asarray(og.code.hz, np.int64) % 2
    H = np.concatenate([hx, hz], axis=0)  # checks 0..m_x-1 are hx, m_x..m_x+m_z-1 are hz
    m_x, n = hx.shape
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    synd = np.concatenate([synd_x, synd_z], axis=1)
    B, A, F = synd_x.shape[0], int(max_attempts), F32(strength)
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    lamhat = lam.copy()
    mux, muz = np.zeros((B, og.E_x), F32), np.zeros((B, og.E_z), F32)
    hard = np.zeros((B, n), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for a in range(A + 1):
        T = pre_iter if a == 0 else attempt_iter
        if restart and a > 0:
            mux[:], muz[:] = 0, 0
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            out = og.bp4_decode(synd_x[idx], synd_z[idx], 1, cn_type, float(factor), llr_ch=lamhat[idx], msg_init=(mux[idx], muz[idx]),
                                return_msgs=True)
            mux[idx], muz[idx] = out["msg_x"], out["msg_z"]
            dn = decisions(out["llr"])
            assert np.array_equal(dn & 1, out["x_hat"]) and np.array_equal(dn >> 1, out["z_hat"]), "the oracle decides by the same rule"
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ hz.T) % 2 == synd_z[idx]).all(1) & ((z @ hx.T) % 2 == synd_x[idx]).all(1)
            hard[idx] = dn
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        idx = np.nonzero(run)[0]
        if len(idx) == 0 or a == A:
            break
        for b in idx:
            d = hard[b]
            par = np.concatenate([((d >> 1).astype(np.int64) @ hx.T) % 2, ((d & 1).astype(np.int64) @ hz.T) % 2])
            U = np.nonzero(par != synd[b])[0]
            assert len(U) > 0
            sample = int(first_sample) + int(b)
            lamhat[b] = lam[b]  # feedback never accumulates
            entry = dict(b=int(b), att=a + 1, d=d.copy())
            if rule == "perturb":
                for v in np.nonzero(H[U].sum(0))[0]:
                    w = draw(seed, sample, int(v), a + 1, STREAM_PERTURB)
                    for row in range(3):  # X, Y, Z: one product, then one subtraction
                        lamhat[b, row, v] = lam[b, row, v] - F * unit(w[row])
            else:
                keys = [(int(draw(seed, sample, int(c), a + 1, STREAM_ENHANCED)[0]) << 32) | (M32 - int(c)) for c in U]
                cs = M32 - (max(keys) & M32)
                qubits = np.nonzero(H[cs])[0]  # ascending
                entry.update(check=int(cs), qubit=None)
                if len(qubits):
                    w = draw(seed, sample, cs, a + 1, STREAM_ENHANCED)
                    v = int(qubits[fy_pick(unit(w[1]), len(qubits))])
                    t = -F if synd[b, cs] else F
                    for row in ((2, 1) if cs < m_x else (0, 1)):  # hx: Z and Y; hz: X and Y
                        lamhat[b, row, v] = lam[b, row, v] + t
                    entry["qubit"] = v
            if log is not None:
                log.append(entry)
    assert lamhat.dtype == F32
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats
