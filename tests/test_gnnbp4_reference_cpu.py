"""The float64 restatement tests/gnnbp4_reference.py — the checker of the GNN_BP4 reverse pass — against the CPU oracle (forward) and
against central finite differences (its autograd gradient).  No GPU."""
import numpy as np
import pytest
import torch

import gnnbp4_reference as R
from helpers import code, oracle_library_forms
from feedback_gnn_amd.graph import gnnbp4_weight_shapes

CONFIGS = [(20, 40, 2, 1, 1, 1), (6, 10, 3, 0, 2, 0)]  # (D, H, L, mean / sum, tanh / relu, bias)


def _shapes(name, cfg):
    D, H, L, rop, act, bias = cfg
    return gnnbp4_weight_shapes(code(name), (D, H, L, ("sum", "mean")[rop], None, bool(bias), False, 0, 0))


def _syndromes(name, B, seed):
    c = code(name)
    rng = np.random.RandomState(seed)
    ex = (rng.uniform(size=(B, c.hx.shape[1])) < 0.06).astype(np.uint8)
    ez = (rng.uniform(size=(B, c.hx.shape[1])) < 0.06).astype(np.uint8)
    sx = ((ez.astype(np.int64) @ np.asarray(c.hx).T) % 2).astype(np.uint8)
    sz = ((ex.astype(np.int64) @ np.asarray(c.hz).T) % 2).astype(np.uint8)
    return ex, ez, sx, sz


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_forward_matches_the_oracle(name, cfg):
    """x_logit_all, z_logit_all and llr of the float64 restatement against og_gnn_bp4_general to 1e-4 (the project's LLR tolerance)."""
    B, T = 3, 3
    w = R.seeded_weights(_shapes(name, cfg), 11)
    _, _, sx, sz = _syndromes(name, B, 3)
    ref = oracle_library_forms(name).gnn_bp4_general(tuple(cfg) + (0, 0, 0), w, sx, sz, T)
    xs, zs, llr = R.forward(R.Graph(code(name)), cfg, [torch.from_numpy(a).double() for a in w], torch.from_numpy(sx), torch.from_numpy(sz), T)
    assert np.abs(torch.stack(xs).numpy() - ref["x_logit_all"]).max() < 1e-4
    assert np.abs(torch.stack(zs).numpy() - ref["z_logit_all"]).max() < 1e-4
    assert np.abs(llr.numpy() - ref["llr"]).max() < 1e-4


def test_autograd_matches_finite_differences():
    """The checker's own gradient: autograd of the loss against a float64 central difference at a handful of entries of every array."""
    name, cfg, T = "gb48", CONFIGS[0], 2
    c = code(name)
    w = R.seeded_weights(_shapes(name, cfg), 5)
    ex, ez, sx, sz = _syndromes(name, 2, 9)
    gx, gz = (torch.from_numpy(a).double() for a in R.labels(c, ex, ez))
    tg = R.Graph(c)

    def loss_of(ws):
        xs, zs, _ = R.forward(tg, cfg, ws, torch.from_numpy(sx), torch.from_numpy(sz), T)
        return R.loss(xs, zs, gx, gz)

    tw = [torch.from_numpy(a).double().requires_grad_(True) for a in w]
    loss_of(tw).backward()
    rng = np.random.RandomState(1)
    h = 1e-6
    with torch.no_grad():
        for i, t in enumerate(tw):
            flat = t.view(-1)
            for j in rng.choice(flat.numel(), size=min(2, flat.numel()), replace=False):
                old = flat[j].item()
                flat[j] = old + h
                up = loss_of(tw).item()
                flat[j] = old - h
                dn = loss_of(tw).item()
                flat[j] = old
                fd, ag = (up - dn) / (2 * h), t.grad.view(-1)[j].item()
                assert abs(fd - ag) <= 1e-6 * max(1.0, abs(ag)) + 1e-8, (i, j, fd, ag)
