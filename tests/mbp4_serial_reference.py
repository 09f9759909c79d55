"""MBP4 / AMBP4 in Kuo and Lai's serial schedule (fgnn_mbp4_decode_serial, include/fgnn.h) restated in NumPy float32.

Only the schedule is new: the check rules (`cn_update`), the edge rule (`vn_edge_own`), the totals, the decision and the index
tables (`Side`) are those of tests/mbp4_reference.py, which tests/test_mbp4_reference_cpu.py ties to the oracle.  A codeword keeps
nu (v->c) and mu (c->v) on the edges of both graphs; the qubits are visited layer by layer, and a visit takes the outputs of the
qubit's checks on the nu of this moment, forms the qubit's totals and decision, and sends its new nu.

The check rule is evaluated on every check and the outputs at the layer's edges are kept: output e of a check reads the check's nu
alone, so this is the message the library evaluates for that edge by itself.  Qubits of one layer share no check, so the order inside
a layer cannot matter and the layer is done at once.  Samples are independent: the batch runs in lock-step and a finished sample
leaves."""
import numpy as np

import mbp4_reference as MB

F32 = np.float32


# ---- layers -----------------------------------------------------------------------------------------------------------------------------------
def _check_rows(hx, hz):
    """The qubits of every check, hx rows first, ascending."""
    h = np.concatenate([np.asarray(hx, np.int64) % 2, np.asarray(hz, np.int64) % 2], axis=0)
    return [np.nonzero(r)[0] for r in h], h.shape[1]


def greedy_qubit_layers(hx, hz):
    """fgnn_greedy_qubit_layers: qubits ascending, each into the lowest-numbered layer that holds no qubit sharing a check with it.
    Returns (num_layers, layer_of [n] int32)."""
    rows, n = _check_rows(hx, hz)
    at = [[] for _ in range(n)]
    for c, r in enumerate(rows):
        for v in r:
            at[v].append(c)
    held = [set() for _ in rows]  # the layers that hold a qubit of check c
    lay = np.zeros(n, np.int32)
    for v in range(n):
        taken = set().union(*(held[c] for c in at[v])) if at[v] else set()
        l = 0
        while l in taken:
            l += 1
        lay[v] = l
        for c in at[v]:
            held[c].add(l)
    return int(lay.max()) + 1, lay


def validate_qubit_layers(hx, hz, num_layers, layer_of):
    """fgnn_validate_qubit_layers: None, or the library's message."""
    rows, n = _check_rows(hx, hz)
    m_x = np.asarray(hx).shape[0]
    if num_layers < 1:
        return f"num_layers = {num_layers} must be >= 1"
    for v in range(n):
        if not 0 <= layer_of[v] < num_layers:
            return f"qubit {v} has layer {layer_of[v]}, outside [0, {num_layers})"
    for l in range(num_layers):
        if not (np.asarray(layer_of) == l).any():
            return f"layer {l} is empty"
    for c, r in enumerate(rows):
        last = {}
        for v in r:
            l = int(layer_of[v])
            if l in last:
                name = f"hx check {c}" if c < m_x else f"hz check {c - m_x} (number {c})"
                return f"qubit {last[l]} and qubit {v} of layer {l} share {name}"
            last[l] = v
    return None


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------
def _first_nu(G, lam):
    """mu = 0 on every edge and the nu that follows: the qubit rule on zero messages (own * 0 = 0 for every own weight)."""
    B = lam.shape[0]
    mux, muz = np.zeros((B, G.x.E), F32), np.zeros((B, G.z.E), F32)
    nux, nuz = G.qubit_update(mux, muz, lam, 1.0)
    return mux, muz, nux, nuz


def serial_iteration(G, layers, mux, muz, nux, nuz, hard, lam, synd_x, synd_z, cn_type, factor, own):
    """One iteration, in place on the arrays of the running samples: every layer in turn."""
    vx, vz = G.x.v_of, G.z.v_of
    for ex, ez, q in layers:
        if len(ex):
            mux[:, ex] = MB.cn_update(G.x, nux, synd_x, cn_type, factor)[:, ex]
        if len(ez):
            muz[:, ez] = MB.cn_update(G.z, nuz, synd_z, cn_type, factor)[:, ez]
        X, Y, Z = G.totals(mux, muz, lam)
        hard[:, q] = MB.decisions(X, Y, Z)[:, q]
        numx, numz = MB.softplus(np.ascontiguousarray(-X[:, q])), MB.softplus(np.ascontiguousarray(-Z[:, q]))
        pos = np.zeros(G.n, np.int64)
        pos[q] = np.arange(len(q))
        if len(ex):
            v = vx[ex]
            nux[:, ex] = MB.vn_edge_own(numx[:, pos[v]], Z[:, v], Y[:, v], mux[:, ex], own)
        if len(ez):
            v = vz[ez]
            nuz[:, ez] = MB.vn_edge_own(numz[:, pos[v]], X[:, v], Y[:, v], muz[:, ez], own)


def layer_tables(G, layer_of):
    """Per layer: its hx edges, its hz edges, its qubits."""
    layer_of = np.asarray(layer_of)
    out = []
    for l in range(int(layer_of.max()) + 1):
        out.append((np.nonzero(layer_of[G.x.v_of] == l)[0], np.nonzero(layer_of[G.z.v_of] == l)[0], np.nonzero(layer_of == l)[0]))
    return out


def mbp4_decode_serial(code, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None,
                       llr_const=0.0, layer_of=None):
    """`code`: an object with hx and hz; `layer_of` [n]: the qubit layering (None: the greedy one).  Returns (x_hat [B,n] uint8, z_hat
    [B,n] uint8, stats [B,4] int32 = found, the a of the last test, iterations, the k of the last test), as MB.mbp4_decode."""
    assert cn_type in MB.CN_TYPES and len(factors) == len(owns) >= 1
    G = MB.graph_of(code)
    n = G.n
    if layer_of is None:
        layer_of = greedy_qubit_layers(G.hx, G.hz)[1]
    assert validate_qubit_layers(G.hx, G.hz, int(np.max(layer_of)) + 1, layer_of) is None
    layers = layer_tables(G, layer_of)
    synd_x, synd_z = np.asarray(synd_x, np.uint8) & 1, np.asarray(synd_z, np.uint8) & 1
    B = synd_x.shape[0]
    lam = np.asarray(llr_ch, F32).copy() if llr_ch is not None else np.full((B, 3, n), F32(llr_const), F32)
    mux, muz, nux, nuz = _first_nu(G, lam)
    hard = np.zeros((B, n), np.uint8)
    stats = np.zeros((B, 4), np.int32)
    run = np.ones(B, bool)
    for a in range(len(factors)):
        T = pre_iter if a == 0 else attempt_iter
        if restart and a > 0:
            mux, muz, nux, nuz = _first_nu(G, lam)
        for k in range(1, T + 1):
            idx = np.nonzero(run)[0]
            if len(idx) == 0:
                break
            part = [mux[idx], muz[idx], nux[idx], nuz[idx], hard[idx]]
            serial_iteration(G, layers, *part, lam[idx], synd_x[idx], synd_z[idx], cn_type, F32(factors[a]), F32(owns[a]))
            mux[idx], muz[idx], nux[idx], nuz[idx], hard[idx] = part
            dn = part[4]
            x, z = (dn & 1).astype(np.int64), (dn >> 1).astype(np.int64)
            ok = ((x @ G.hz.T) % 2 == synd_z[idx]).all(1) & ((z @ G.hx.T) % 2 == synd_x[idx]).all(1)
            stats[idx, 1], stats[idx, 2], stats[idx, 3] = a, stats[idx, 2] + 1, k
            stats[idx[ok], 0] = 1
            run[idx[ok]] = False
        if not run.any():
            break
    return (hard & 1).astype(np.uint8), (hard >> 1).astype(np.uint8), stats
