"""Differentiable torch restatement of GNN_BP4.call (TEST INFRASTRUCTURE): a translation of oracle/numpy_ref.gnn_bp4_general for
reduce_op sum / mean without attributes, in any dtype.  Autograd of it in float64 is the checker of the hand-written reverse pass
(feedback_gnn_amd/csrc/fgnn_gnnbp4_backward.hip); in float32 on the GPU it is the baseline of tools/bench_gnnbp4_train.py.

Gradient conventions as oracle/torch_ref.py: the sign products are constants, the clip inside phi passes the gradient as
torch.clamp does, abs differentiates to the sign."""
import numpy as np
import torch

from oracle.torch_ref import phi

_ACT = {0: lambda x: x, 1: torch.tanh, 2: torch.relu, 3: torch.sigmoid}


class Graph:
    """Index tensors of one CSS code: check-major edges of hx / hz (the reference's np.nonzero order) and the logical rows."""

    def __init__(self, code, device="cpu"):
        self.n = int(np.asarray(code.hx).shape[1])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.sides = []
        for pcm in (code.hx, code.hz):
            pcm = np.asarray(pcm)
            c, v = np.nonzero(pcm)
            self.sides.append(dict(c=t(c), v=t(v), m=int(pcm.shape[0]), cdeg=t(pcm.sum(1).astype(np.float64)),
                                   vdeg=t(pcm.sum(0).astype(np.float64))))
        self.rows = {}
        for key, mat in (("hx", code.hx), ("hz", code.hz), ("lx", code.lx), ("lz", code.lz)):
            mat = np.asarray(mat)
            r, c = np.nonzero(mat)
            self.rows[key] = (t(r), t(c), int(mat.shape[0]))


def split_weights(cfg, w):
    """The weight list of gnnbp4_weight_shapes (no attributes) as 7 MLPs of (W, b or None) layers + (Winv, binv)."""
    D, H, L, rop, act, bias = cfg[:6]
    st, pos, mlps = 1 + int(bool(bias)), 0, []
    for _ in range(7):
        layers = []
        for _ in range(L):
            layers.append((w[pos], w[pos + 1] if bias else None))
            pos += st
        mlps.append(layers)
    return mlps, w[pos], (w[pos + 1] if bias else None)


def _scatter(vals, idx, size):
    out = torch.zeros((vals.shape[0], size) + tuple(vals.shape[2:]), dtype=vals.dtype, device=vals.device)
    return out.index_add(1, idx, vals)


def forward(g, cfg, w, synd_x, synd_z, num_iter, record=None):
    """cfg = (D, H, L, reduce_op 0 sum / 1 mean, activation 0..3, use_bias); w tensors of one dtype (requires_grad ok);
    syndromes [B, m] 0/1.  Returns (x_logit_all, z_logit_all, llr): lists of [B, m_z + k] / [B, m_x + k] and the last [B, 3, n].
    ``record``: a dict that receives, per iteration, what the library's tape keeps — "h_vn" [B, n, D] after the VN update, "h_cn"
    [B, m_x + m_z, D] the VN update read, "hlog" [B, m_x + m_z] the hx then hz logits — and "llr_x" / "llr_z" [B, n], the binary
    LLRs the soft syndromes are taken from."""
    D, H, L, rop, act, bias = [int(x) for x in cfg[:6]]
    if rop not in (0, 1):
        raise NotImplementedError("sum / mean only")
    dt, dev = w[0].dtype, w[0].device
    mlps, Winv, binv = split_weights(cfg, w)
    B, n = synd_x.shape[0], g.n
    sg = [1.0 - 2.0 * synd_x.to(dt), 1.0 - 2.0 * synd_z.to(dt)]
    fa = _ACT[act]

    def mlp(x, layers):
        for i, (W, b) in enumerate(layers):
            x = x @ W
            if b is not None:
                x = x + b
            if i < len(layers) - 1:
                x = fa(x)
        return x

    def reduce_by(msgs, idx, count, deg):
        out = _scatter(msgs, idx, count)
        if rop == 1:
            out = out / torch.clamp(deg.to(dt), min=1.0)[None, :, None]
        return out

    def update_cn(h_vn, hc, lg):
        new = []
        for s, side in enumerate(g.sides):
            f = torch.cat([h_vn[:, side["v"], :], hc[s][:, side["c"], :]], -1)
            m = reduce_by(mlp(f, mlps[s]), side["c"], side["m"], side["cdeg"])
            new.append(mlp(torch.cat([m, hc[s], lg[s][:, :, None]], -1), mlps[2 + s]))
        return new

    def update_vn(hc, h_vn):
        ms = []
        for s, side in enumerate(g.sides):
            f = torch.cat([hc[s][:, side["c"], :], h_vn[:, side["v"], :]], -1)
            msg = mlp(f, mlps[4 + s]) * sg[s][:, side["c"], None]
            ms.append(reduce_by(msg, side["v"], n, side["vdeg"]))
        return mlp(torch.cat([ms[0], ms[1], h_vn], -1), mlps[6])

    def rows_logit(key, llr):
        r, c, rows = g.rows[key]
        v = llr[:, c]
        neg = _scatter((v < 0).to(dt), r, rows)
        sgn = 1.0 - 2.0 * torch.remainder(neg, 2.0)
        return sgn.detach() * phi(_scatter(phi(v.abs()), r, rows))

    sp = torch.nn.functional.softplus
    lse = lambda a, b: torch.logsumexp(torch.stack([a, b], -1), -1)
    h_vn = torch.ones((B, n, D), dtype=dt, device=dev)
    hc = [torch.zeros((B, s["m"], D), dtype=dt, device=dev) for s in g.sides]
    hc = update_cn(h_vn, hc, [torch.zeros_like(sg[0]), torch.zeros_like(sg[1])])
    xs, zs = [], []
    if record is not None:
        record.update(h_vn=[], h_cn=[], hlog=[], llr_x=[], llr_z=[])
    for it in range(num_iter):
        if record is not None:
            record["h_cn"].append(torch.cat(hc, 1))
        h_vn = update_vn(hc, h_vn)
        Lv = h_vn @ Winv
        if binv is not None:
            Lv = Lv + binv
        X, Y, Z = Lv[..., 0], Lv[..., 1], Lv[..., 2]
        llr_z = sp(-X) - lse(-Z, -Y)
        llr_x = sp(-Z) - lse(-X, -Y)
        hz_l, lz_l = rows_logit("hz", llr_x), rows_logit("lz", llr_x)
        hx_l, lx_l = rows_logit("hx", llr_z), rows_logit("lx", llr_z)
        xs.append(torch.cat([hz_l, lz_l], 1))
        zs.append(torch.cat([hx_l, lx_l], 1))
        if record is not None:
            record["h_vn"].append(h_vn)
            record["hlog"].append(torch.cat([hx_l, hz_l], 1))
            record["llr_x"].append(llr_x)
            record["llr_z"].append(llr_z)
        if it == num_iter - 1:
            break
        hc = update_cn(h_vn, hc, [hx_l * sg[0], hz_l * sg[1]])
    return xs, zs, torch.stack([X, Y, Z], 1)


def labels(code, noise_x, noise_z):
    """1 - parity: for x_logit rows the parities of noise_x on hz then lz, for z_logit rows those of noise_z on hx then lx."""
    par = lambda mat, e: (np.asarray(e).astype(np.int64) @ np.asarray(mat).astype(np.int64).T) % 2
    gx = 1 - np.concatenate([par(code.hz, noise_x), par(code.lz, noise_x)], 1)
    gz = 1 - np.concatenate([par(code.hx, noise_z), par(code.lx, noise_z)], 1)
    return gx, gz


def loss(xs, zs, gt_x, gt_z, loss_from=0, sides=(True, True)):
    """Sum over iterations loss_from .. T-1 of the mean-reduced BCE-with-logits of both sides (or one, for the NULL-gradient test)."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    total = 0.0
    for i in range(loss_from, len(xs)):
        if sides[0]:
            total = total + bce(xs[i], gt_x)
        if sides[1]:
            total = total + bce(zs[i], gt_z)
    return total


def seeded_weights(shapes, seed, inv_scale=0.5, bias_lim=0.6, kernel_scale=1.0):
    """Glorot kernels, biases in (-bias_lim, bias_lim) as helpers.gnnbp4_weights draws them, and a NON-ZERO _llr_inv_embed kernel
    (with Keras' zero initialisation every upstream gradient is zero).  kernel_scale shrinks the Glorot kernels: a linear / sum
    configuration grows its embeddings from iteration to iteration, and float32 then decides the soft syndromes' signs differently."""
    rng = np.random.RandomState(seed)
    w = []
    for shp in shapes:
        lim = bias_lim if len(shp) == 1 else kernel_scale * np.sqrt(6.0 / (shp[0] + shp[1]))
        w.append(rng.uniform(-lim, lim, size=shp).astype(np.float32))
    k = [i for i, s in enumerate(shapes) if len(s) == 2 and s[1] == 3][-1]
    w[k] = rng.uniform(-inv_scale, inv_scale, size=shapes[k]).astype(np.float32)
    return w


def depolarizing_noise(code, B, seed, p=0.05):
    """Seeded depolarizing noise drawn on the host (X, Y, Z with probability p / 3 each) and its syndromes:
    (noise_x, noise_z, syndrome_x = hx noise_z, syndrome_z = hz noise_x), uint8.  The GPU tests and their CPU screening use the same draws."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(size=(B, np.asarray(code.hx).shape[1]))
    ex = (u < 2 * p / 3).astype(np.uint8)
    ez = ((u > p / 3) & (u < p)).astype(np.uint8)
    sx = ((ez.astype(np.int64) @ np.asarray(code.hx).T) % 2).astype(np.uint8)
    sz = ((ex.astype(np.int64) @ np.asarray(code.hz).T) % 2).astype(np.uint8)
    return ex, ez, sx, sz
