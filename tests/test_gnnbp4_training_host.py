"""Host-side pieces of GNN_BP4 training: the labels and the layout of the gradient list.  No GPU."""
import numpy as np
import torch

from helpers import code
from feedback_gnn_amd import gf2
from feedback_gnn_amd.gnn import gnnbp4_label_rows, gnnbp4_labels, split_flat_grads
from feedback_gnn_amd.graph import gnnbp4_weight_shapes


def test_labels_are_one_minus_the_parities_of_the_noise():
    """x_logit rows: noise_x on hz then lz; z_logit rows: noise_z on hx then lx — against GF(2) arithmetic on gb48."""
    c = code("gb48")
    rng = np.random.RandomState(4)
    ex = (rng.uniform(size=(7, c.hx.shape[1])) < 0.2).astype(np.uint8)
    ez = (rng.uniform(size=(7, c.hx.shape[1])) < 0.2).astype(np.uint8)
    gt_x, gt_z = gnnbp4_labels(gnnbp4_label_rows(c), (torch.from_numpy(ex), torch.from_numpy(ez)))
    par = lambda mat, e: np.asarray(gf2.int_mod_2(e.astype(np.int64) @ np.asarray(mat).astype(np.int64).T))
    want_x = 1 - np.concatenate([par(c.hz, ex), par(c.lz, ex)], 1)
    want_z = 1 - np.concatenate([par(c.hx, ez), par(c.lx, ez)], 1)
    assert gt_x.dtype == torch.float32 and tuple(gt_x.shape) == (7, c.hz.shape[0] + np.asarray(c.lz).shape[0])
    assert np.array_equal(gt_x.numpy(), want_x) and np.array_equal(gt_z.numpy(), want_z)
    # the hz part of the x labels is 1 - syndrome_z
    assert np.array_equal(gt_x.numpy()[:, :c.hz.shape[0]], 1 - (ex.astype(np.int64) @ np.asarray(c.hz).T) % 2)


def test_gradient_list_has_the_shapes_of_the_weight_list():
    for cfg in [(20, 40, 2, "mean", "tanh", True, False, 0, 0), (6, 10, 3, "sum", "relu", False, False, 0, 0)]:
        shapes = gnnbp4_weight_shapes(code("gb48"), cfg)
        total = sum(int(np.prod(s)) for s in shapes)
        grads = split_flat_grads(torch.arange(total, dtype=torch.float32), shapes)
        assert [tuple(g.shape) for g in grads] == [tuple(s) for s in shapes]
        assert torch.equal(torch.cat([g.reshape(-1) for g in grads]), torch.arange(total, dtype=torch.float32))
