"""Restatement of BP4 in the layered (serial) schedule — what fgnn_bp4_decode_layered is held to bit for bit — on the unchanged CPU oracle.

One layer step is one flooding iteration of the oracle (`OracleGraph.bp4_decode(..., num_iter=1, msg_init=mu, return_msgs=True)`) whose
new c->v messages are kept on the edges of that layer's checks only: the flooding iteration forms every v->c message from the current
mu and every check's new messages from the v->c messages on its own edges, so the messages it returns on the layer's checks are what
the serial schedule writes there, and the messages of every other check stay as they were.  After the last step a call with
num_iter = 0 and msg_init = mu gives the marginals, decisions and soft syndromes of the final messages.

The slot -> check map is NumPy's: slots are sorted by (qubit, check), which is the order of np.nonzero(h.T)."""
import numpy as np


def slot_checks(code):
    """The check number (hx checks 0..m_x-1, hz checks m_x..m_x+m_z-1) of every hx slot and of every hz slot."""
    hx, hz = np.asarray(code.hx), np.asarray(code.hz)
    return np.nonzero(hx.T)[1], np.nonzero(hz.T)[1] + hx.shape[0]


def greedy_layers(hx, hz):
    """Checks in ascending number, each into the lowest-numbered layer that holds no check sharing a qubit with it: (num_layers, layer_of)."""
    H = np.vstack([np.asarray(hx), np.asarray(hz)]) != 0
    used = [set() for _ in range(H.shape[1])]  # the layers that hold a check of qubit v
    layer_of = np.zeros(H.shape[0], np.int32)
    for c in range(H.shape[0]):
        qubits = np.nonzero(H[c])[0]
        taken = set().union(*[used[v] for v in qubits]) if len(qubits) else set()
        l = 0
        while l in taken:
            l += 1
        layer_of[c] = l
        for v in qubits:
            used[v].add(l)
    return int(layer_of.max()) + 1, layer_of


def is_valid_layering(hx, hz, num_layers, layer_of):
    """Every check has a layer in range, no layer is empty, no two checks of a layer share a qubit (across hx and hz)."""
    H = (np.vstack([np.asarray(hx), np.asarray(hz)]) != 0).astype(np.int64)
    layer_of = np.asarray(layer_of)
    if layer_of.shape != (H.shape[0],) or layer_of.min() < 0 or layer_of.max() >= num_layers:
        return False
    if len(set(layer_of.tolist())) != num_layers:
        return False
    return all(int(H[layer_of == l].sum(0).max()) <= 1 for l in range(num_layers))


def layered_decode(og, synd_x, synd_z, num_iter, cn_type="boxplus-phi", factor=1.0, layer_of=None, llr_ch=None, llr_const=0.0,
                   msg_init=None, keep_all=False):
    """The result dict of `og.bp4_decode(..., return_msgs=True)` for the layered schedule.  `layer_of` None: the greedy layering.
    `keep_all`: every step keeps the whole flooding iteration (with ONE layer that is the flooding schedule itself: the anchor)."""
    code = og.code
    if layer_of is None:
        _, layer_of = greedy_layers(code.hx, code.hz)
    layer_of = np.asarray(layer_of)
    num_layers = int(layer_of.max()) + 1
    cx, cz = slot_checks(code)
    B = len(synd_x)
    llr = dict(llr_ch=llr_ch) if llr_ch is not None else dict(llr_const=llr_const)
    if msg_init is None:
        mu_x, mu_z = np.zeros((B, og.E_x), np.float32), np.zeros((B, og.E_z), np.float32)
    else:
        mu_x, mu_z = np.array(msg_init[0], np.float32), np.array(msg_init[1], np.float32)
    for _ in range(int(num_iter)):
        for l in range(num_layers):
            out = og.bp4_decode(synd_x, synd_z, 1, cn_type, factor, msg_init=(mu_x, mu_z), return_msgs=True, **llr)
            if keep_all:
                mu_x, mu_z = out["msg_x"], out["msg_z"]
            else:
                sel_x, sel_z = layer_of[cx] == l, layer_of[cz] == l
                mu_x[:, sel_x] = out["msg_x"][:, sel_x]
                mu_z[:, sel_z] = out["msg_z"][:, sel_z]
    return og.bp4_decode(synd_x, synd_z, 0, cn_type, factor, msg_init=(mu_x, mu_z), return_msgs=True, **llr)


def unsolved(code, synd_x, synd_z, out):
    """Samples whose decision does not reproduce its syndromes: hx z_hat != synd_x or hz x_hat != synd_z."""
    hx, hz = np.asarray(code.hx, np.int64), np.asarray(code.hz, np.int64)
    bad_x = ((out["z_hat"].astype(np.int64) @ hx.T) % 2 != synd_x).any(1)
    bad_z = ((out["x_hat"].astype(np.int64) @ hz.T) % 2 != synd_z).any(1)
    return int((bad_x | bad_z).sum())
