"""Inputs and restatement runs shared by tests/test_backward_reference_cpu.py and tests/test_gpu_backward_elementwise.py: the feedback
GNN's reverse pass through oracle/torch_ref.py in float64 or float32, every per-row array as NumPy in the library's row order, and
the crafted inputs on which max / min ties and dead relu units are the same in both precisions."""
import numpy as np
import torch

from helpers import code, gen_cfg_codes
from oracle import torch_ref as R

F32 = np.float32
TIE_CONSTANTS = (2.0, -3.0)  # logit * (1 - 2 s) on the tied checks of hx / hz


def reference_pairs(name, cfg, w, llr, lhx, lhz, sx, sz, gout, dtype, edges=None):
    """Reverse pass of sum(gout * Feedback_GNN(...)) through the restatement in ``dtype``.  cfg None: the shipped architecture
    (R.feedback_gnn), else a constructor setting with names (R.feedback_gnn_general).  ``edges`` = [(chk, var) of side 0, of side 1] in
    the library's order (TannerGraph.edges), None = the restatement's own order.  Returns dict(out [B,3,n], acts / pre / deltas: one
    [rows, width] float64 array per Dense layer in the kernel's layer order, z_grad [B,n,2D+3], wgrads in get_weights() order)."""
    tg = R.Graph(code(name))
    tw = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in w]
    args = [torch.from_numpy(np.asarray(a)).to(dtype) for a in (llr, lhx, lhz)]
    args += [torch.as_tensor(np.asarray(a, np.uint8)) for a in (sx, sz)]
    if cfg is None:
        L = 2
        out, pairs = R.feedback_gnn(tg, tw, *args, return_pairs=True)
    else:
        L = cfg[2]
        out, pairs = R.feedback_gnn_general(tg, gen_cfg_codes(cfg), tw, *args, return_pairs=True)
    assert len(pairs) == 3 * L and out.dtype == dtype
    z = pairs[2 * L][0]  # input of the embed MLP (of _llr_inv_embed when L = 1): [reduced_x | reduced_z | X Y Z]
    z.retain_grad()
    (out * torch.from_numpy(np.asarray(gout)).to(dtype)).sum().backward()
    res = dict(out=out.detach().double().numpy(), acts=[], pre=[], deltas=[], z_grad=z.grad.double().numpy(),
               wgrads=[t.grad.double().numpy() for t in tw])
    for li, (x, y) in enumerate(pairs):
        for key, t in (("acts", x.detach()), ("pre", y.detach()), ("deltas", y.grad)):
            if li < 2 * L and edges is not None:
                t = t[:, R.library_edge_rows(tg, li // L, *edges[li // L])]
            res[key].append(t.double().numpy().reshape(-1, t.shape[-1]))
    return res


def tie_case(name, cfg, B, seed):
    """Inputs of a relu / max or relu / min setting with exact ties and dead units whose pattern float32 and float64 share:
    - about half of the checks of each side carry logit * (1 - 2 s) = one constant (TIE_CONSTANTS) under both syndrome values, so the
      edges of a qubit into such checks have identical inputs and identical messages, bit for bit, in any precision;
    - every input (LLRs, the other logits) is an integer and the first Dense layer of both message MLPs has entries in {-1, 0, 1} with
      a bias that is an odd multiple of 0.5: its pre-activations are exact half-integers, at least 0.5 away from 0.
    Returns dict(w, llr, lhx, lhz, sx, sz, gout, tied=[mask over the hx checks, over the hz checks])."""
    from feedback_gnn_amd.graph import gnn_weight_shapes
    D, H, L, _, _, bias = cfg
    assert bias and L >= 2
    c = code(name)
    n, m = c.hx.shape[1], (c.hx.shape[0], c.hz.shape[0])
    rng = np.random.RandomState(seed)
    w = [rng.uniform(-0.5, 0.5, size=s).astype(F32) for s in gnn_weight_shapes(D, H, L, bias)]
    for s in range(2):
        k = 2 * (1 + s * L)  # first layer of the message MLP of side s in get_weights() order (kernel, bias per Dense)
        w[k] = rng.randint(-1, 2, size=w[k].shape).astype(F32)
        w[k + 1] = (rng.randint(-3, 3, size=w[k + 1].shape) + 0.5).astype(F32)
    llr = rng.randint(-2, 7, size=(B, 3, n)).astype(F32)
    synd = [rng.randint(0, 2, size=(B, ms)).astype(np.uint8) for ms in m]
    logits, tied = [], []
    for s in range(2):
        lg = rng.randint(-8, 9, size=(B, m[s])).astype(F32)
        t = rng.rand(m[s]) < 0.5
        lg[:, t] = (TIE_CONSTANTS[s] * (1.0 - 2.0 * synd[s][:, t])).astype(F32)
        logits.append(lg)
        tied.append(t)
    gout = rng.normal(size=(B, 3, n)).astype(F32)
    return dict(w=w, llr=llr, lhx=logits[0], lhz=logits[1], sx=synd[0], sz=synd[1], gout=gout, tied=tied)


def tie_expectation(ref, var, D, L, is_max):
    """The few lines of NumPy that state the convention: per side, the delta of the last message layer is gr / count on the edges that
    attain the qubit's extremum and 0 on the others, gr = the gradient at the reduced message.  ``ref`` from `reference_pairs`,
    ``var`` = [qubit of every edge row of side 0, of side 1] for ONE codeword (rows are codeword-major).  Returns
    ([expected deltas per side], [tie counts per side as arrays [B, n, D], 0 where a qubit has no edge])."""
    B, n = ref["z_grad"].shape[:2]
    want, counts = [], []
    for s in range(2):
        m = ref["pre"][s * L + L - 1].reshape(B, -1, D)
        gr = ref["z_grad"][:, :, s * D:(s + 1) * D]
        exp, cnt = np.zeros_like(m), np.zeros((B, n, D), np.int64)
        for v in range(n):
            rows = np.nonzero(np.asarray(var[s]) == v)[0]
            if rows.size == 0:
                continue
            sel = m[:, rows]
            ext = sel.max(1, keepdims=True) if is_max else sel.min(1, keepdims=True)
            hit = sel == ext
            cnt[:, v] = hit.sum(1)
            exp[:, rows] = hit * (gr[:, v] / hit.sum(1))[:, None, :]
        want.append(exp.reshape(-1, D))
        counts.append(cnt)
    return want, counts
