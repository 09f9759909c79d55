"""The GNN_BP4 tape forward and reverse pass (fgnn_gnnbp4_forward_tape, fgnn_gnnbp4_backward, GNN_BP4.loss_and_grads,
training.train_gnn_bp4) against autograd of the float64 restatement tests/gnnbp4_reference.py.  Gradients are float32 on the GPU
and float64 in the checker; the bound is the one tests/test_gpu_backward.py uses for a float32 reverse pass through BP iterations:
max |got - ref| <= 2e-3 max |ref| per array, loss to 2e-4 relative."""
import functools

import numpy as np
import pytest
import torch

import gnnbp4_reference as R
from helpers import code, gpu_graph, to_gpu
from feedback_gnn_amd import _lib
from feedback_gnn_amd.gnn import GNN_BP4
from feedback_gnn_amd.graph import ACTIVATIONS, REDUCE_OPS, GnnBp4Weights, gnnbp4_weight_shapes

pytestmark = pytest.mark.gpu
SEED = 20240611
P = 0.05
GRAD_TOL, LOSS_TOL = 2e-3, 2e-4

CASES = {
    "gb48_small": ("gb48", (8, 16, 1, "sum", "linear", True)),
    "rsurf5_deep": ("rsurf5", (12, 24, 3, "mean", "relu", False)),
    "ghp882_survey": ("ghp882", (20, 40, 2, "mean", "tanh", True)),
    "gb48_limits": ("gb48", (32, 96, 4, "mean", "sigmoid", True)),
}


def _full(cfg):
    return tuple(cfg) + (False, 0, 0)


def _num(cfg):
    D, H, L, red, act, bias = cfg
    return (D, H, L, REDUCE_OPS[red], ACTIVATIONS[act], int(bias))


# Weight seed and kernel scale per configuration, kept where float32 autograd of the restatement stays within 1e-3 of float64 on the
# CPU for every (B, T, loss_from) used below (worst case 7.6e-4, gb48 at the width and depth limits; the sum / linear configuration
# needs Glorot kernels at half scale — at full scale its embeddings grow until float32 flips soft-syndrome signs: 0.1 .. 2.8).
WEIGHT_DRAW = {(8, 16, 1, "sum", "linear", True): (2, 0.5)}


@functools.lru_cache(maxsize=None)
def _weights(name, cfg):
    seed, kernel_scale = WEIGHT_DRAW.get(cfg, (7, 1.0))
    return R.seeded_weights(gnnbp4_weight_shapes(code(name), _full(cfg)), seed, kernel_scale=kernel_scale)


def _decoder(name, cfg, T):
    D, H, L, red, act, bias = cfg
    dec = GNN_BP4(code(name), D, D, H, L, T, reduce_op=red, activation=act, use_bias=bias, graph=gpu_graph(name))
    dec.set_weights(_weights(name, cfg))
    return dec


@functools.lru_cache(maxsize=None)
def _batch(name, B, seed=1):
    """Host-drawn noise and syndromes (the draws the CPU screening of the cases used), on the GPU."""
    return tuple(to_gpu(a) for a in R.depolarizing_noise(code(name), B, seed, P))


@functools.lru_cache(maxsize=None)
def _reference(name, cfg, B, T, loss_from, sides=(True, True)):
    """(loss, grads) of the float64 restatement; computed once per case and shared."""
    ex, ez, sx, sz = _batch(name, B)
    tg = R.Graph(code(name))
    tw = [torch.from_numpy(a).to(torch.float64).requires_grad_(True) for a in _weights(name, cfg)]
    xs, zs, _ = R.forward(tg, _num(cfg), tw, sx.cpu(), sz.cpu(), T)
    gx, gz = R.labels(code(name), ex.cpu().numpy(), ez.cpu().numpy())
    loss = R.loss(xs, zs, torch.from_numpy(gx).to(torch.float64), torch.from_numpy(gz).to(torch.float64), loss_from, sides)
    loss.backward()
    return loss.item(), [t.grad.numpy() for t in tw]


def _check(grads, ref, tol=GRAD_TOL):
    assert len(grads) == len(ref)
    for i, (got, want) in enumerate(zip(grads, ref)):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape, i
        assert np.isfinite(got).all(), i
        scale = np.abs(want).max()
        assert scale > 0, f"array {i}: the reference gradient is zero, the case checks nothing"
        err = np.abs(got - want).max() / scale
        print(f"array {i} {want.shape}: rel err {err:.2e}")
        assert err <= tol, (i, err)


@pytest.mark.parametrize("case", ["gb48_small", "rsurf5_deep", "ghp882_survey"])
def test_tape_forward_equals_decode(case):
    """On a runtime-shaped handle the tape forward returns the bits of fgnn_gnnbp4_decode."""
    name, cfg = CASES[case]
    g = gpu_graph(name)
    _, _, sx, sz = _batch(name, 3)
    W = GnnBp4Weights(_weights(name, cfg), g.device, config=_full(cfg), graph=g, force_general=True)
    dec = g.gnn_bp4_decode(W, sx, sz, 3)
    fwd = g.gnn_bp4_forward_tape(W, sx, sz, 3)
    assert torch.equal(fwd["x_logit_all"], dec["x_logit_all"])
    assert torch.equal(fwd["z_logit_all"], dec["z_logit_all"])
    assert fwd["tape"].numel() * 4 == g.gnn_bp4_tape_bytes(W, 3, 3) == 3 * 3 * ((g.n + g.m_x + g.m_z) * cfg[0] + g.m_x + g.m_z) * 4


@pytest.mark.parametrize("T,loss_from", [(1, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_float64_autograd(case, T, loss_from):
    """Every array of loss_and_grads within 2e-3 of the float64 autograd gradient's largest entry, the loss within 2e-4.  T = 1 has no
    CN update inside the loop: only the initial one contributes.  Screened on the CPU with the same draws: float32 autograd of
    the restatement is within 7.6e-4 of float64 in every case (WEIGHT_DRAW above)."""
    name, cfg = CASES[case]
    B = 3
    ex, ez, sx, sz = _batch(name, B)
    loss, grads = _decoder(name, cfg, T).loss_and_grads((sx, sz), (ex, ez), loss_from=loss_from)
    ref_loss, ref = _reference(name, cfg, B, T, loss_from)
    print(f"loss {loss:.6f} ref {ref_loss:.6f}")
    assert abs(loss - ref_loss) <= LOSS_TOL * abs(ref_loss)
    _check(grads, ref)


def test_both_instantiations_agree():
    """The SURVEY configuration on [[882,24]] through the compile-time kernels and, with force_generic, through the runtime-shaped
    ones: each within the bound of the checker, and within 1e-5 max |ref| of each other."""
    name, cfg = CASES["ghp882_survey"]
    B, T = 2, 3
    g = gpu_graph(name)
    ex, ez, sx, sz = _batch(name, B)
    dec = _decoder(name, cfg, T)
    _, fixed = dec.loss_and_grads((sx, sz), (ex, ez))
    g.force_generic(True)
    try:
        _, runtime = dec.loss_and_grads((sx, sz), (ex, ez))
    finally:
        g.force_generic(False)
    _, ref = _reference(name, cfg, B, T, 0)
    _check(fixed, ref)
    _check(runtime, ref)
    for i, (a, b, r) in enumerate(zip(fixed, runtime, ref)):
        d = (a - b).abs().max().item() / np.abs(r).max()
        assert d <= 1e-5, (i, d)


@pytest.mark.parametrize("side", [0, 1])
def test_null_gradient_side_contributes_nothing(side):
    """A NULL gradient on one side = the checker with that side's loss dropped."""
    name, cfg = CASES["gb48_small"]
    B, T = 3, 3
    g = gpu_graph(name)
    ex, ez, sx, sz = _batch(name, B)
    W = GnnBp4Weights(_weights(name, cfg), g.device, config=_full(cfg), graph=g, force_general=True)
    fwd = g.gnn_bp4_forward_tape(W, sx, sz, T)
    gx, gz = R.labels(code(name), ex.cpu().numpy(), ez.cpu().numpy())
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    key, gt = (("x_logit_all", gx), ("z_logit_all", gz))[side]
    lg = fwd[key].clone().requires_grad_(True)
    sum(bce(lg[i], torch.from_numpy(gt).float().cuda()) for i in range(T)).backward()
    flat = g.gnn_bp4_backward(W, sx, sz, T, fwd["tape"], lg.grad if side == 0 else None, lg.grad if side == 1 else None)
    from feedback_gnn_amd.gnn import split_flat_grads
    _, ref = _reference(name, cfg, B, T, 0, (side == 0, side == 1))
    _check(split_flat_grads(flat, [a.shape for a in _weights(name, cfg)]), ref)


@pytest.mark.parametrize("case,B", [("gb48_small", 1), ("rsurf5_deep", 5)])
def test_batch_sizes_and_small_checks(case, B):
    """B = 1, and an odd batch; rsurf5 has boundary checks of degree 2 under mean reduction."""
    name, cfg = CASES[case]
    ex, ez, sx, sz = _batch(name, B)
    loss, grads = _decoder(name, cfg, 2).loss_and_grads((sx, sz), (ex, ez))
    ref_loss, ref = _reference(name, cfg, B, 2, 0)
    assert abs(loss - ref_loss) <= LOSS_TOL * abs(ref_loss)
    _check(grads, ref)


def test_batch_beyond_the_workgroup_count():
    """The reverse pass runs at most 512 workgroups; codeword b goes to workgroup b mod 512.  515 codewords: three workgroups take two.
    The batch is 103 distinct codewords five times over, so the gradient is five times that of the 103 (to float32 summation)."""
    name, cfg = CASES["gb48_small"]
    T = 2
    ex, ez, sx, sz = _batch(name, 103)
    dec = _decoder(name, cfg, T)
    rep = lambda t: t.repeat(5, 1)
    _, small = dec.loss_and_grads((sx, sz), (ex, ez))
    _, big = dec.loss_and_grads((rep(sx), rep(sz)), (rep(ex), rep(ez)))
    for i, (a, b) in enumerate(zip(small, big)):  # the mean-reduced loss divides by the batch: the same gradient
        assert (a - b).abs().max().item() <= 1e-5 * a.abs().max().item(), i


def test_two_calls_give_the_same_bits():
    name, cfg = CASES["ghp882_survey"]
    ex, ez, sx, sz = _batch(name, 3)
    dec = _decoder(name, cfg, 2)
    _, a = dec.loss_and_grads((sx, sz), (ex, ez))
    _, b = dec.loss_and_grads((sx, sz), (ex, ez))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kw", [dict(reduce_op="max"), dict(reduce_op="min"), dict(use_attributes=True, node_attribute_dims=2, msg_attribute_dims=2)])
def test_undifferentiable_settings_are_refused(kw):
    dec = GNN_BP4(code("gb48"), 8, 8, 16, 2, 2, use_bias=True, graph=gpu_graph("gb48"), **kw)
    ex, ez, sx, sz = _batch("gb48", 2)
    with pytest.raises(NotImplementedError):
        dec.loss_and_grads((sx, sz), (ex, ez))
    with pytest.raises(NotImplementedError):
        gpu_graph("gb48").gnn_bp4_forward_tape(dec._weights, sx, sz, 2)


def test_undersized_buffers_are_refused_on_their_size():
    """The refusal is decided on the size argument: the buffers handed over are full-sized, the byte counts are not."""
    import ctypes as C
    name, cfg = CASES["gb48_small"]
    g = gpu_graph(name)
    _, _, sx, sz = _batch(name, 2)
    W = GnnBp4Weights(_weights(name, cfg), g.device, config=_full(cfg), graph=g, force_general=True)
    T, B = 2, 2
    fwd = g.gnn_bp4_forward_tape(W, sx, sz, T)
    tape, need_tape, need_ws = fwd["tape"], g.gnn_bp4_tape_bytes(W, T, B), g.gnn_bp4_backward_workspace_bytes(W, B)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.fgnn_gnnbp4_forward_tape(g.handle, W.handle, T, p(sx), p(sz), B, p(fwd["x_logit_all"]), p(fwd["z_logit_all"]), p(tape),
                                    need_tape - 4, None)
    assert rc == -1 and str(need_tape) in L.fgnn_last_error().decode() and str(need_tape - 4) in L.fgnn_last_error().decode()
    count = C.c_int()
    assert L.fgnn_gnnbp4_grad_count(g.handle, W.handle, C.byref(count)) == 0
    grad = torch.zeros(count.value, device=g.device)
    ws = torch.empty(need_ws, dtype=torch.uint8, device=g.device)
    gx = torch.zeros_like(fwd["x_logit_all"])
    args = lambda tb, wb: (g.handle, W.handle, T, p(sx), p(sz), B, p(tape), tb, p(gx), None, p(grad), count.value, p(ws), wb, None)
    assert L.fgnn_gnnbp4_backward(*args(need_tape - 4, need_ws)) == -1 and str(need_tape) in L.fgnn_last_error().decode()
    assert L.fgnn_gnnbp4_backward(*args(need_tape, need_ws - 1)) == -1
    msg = L.fgnn_last_error().decode()
    assert str(need_ws) in msg and str(need_ws - 1) in msg
    torch.cuda.synchronize()


def test_training_moves_the_loss():
    """train_gnn_bp4 on gb48, (8, 16, 2, mean, tanh, bias), T = 3, B = 64, p = 0.05, 40 steps, Adam 1e-2: the mean of the last five
    losses is below the mean of the first five.  The same loop on the CPU (float64 restatement, the same Adam and start weights,
    host-drawn depolarizing noise of the same strength) goes from 4.10 (first five) to 1.31 (last five) at this learning rate."""
    from feedback_gnn_amd.training import train_gnn_bp4
    name, cfg = "gb48", (8, 16, 2, "mean", "tanh", True)
    dec = _decoder(name, cfg, 3)
    hist = train_gnn_bp4(dec, P, 64, 40, 1e-2, SEED)
    assert len(hist) == 40 and np.isfinite(hist).all()
    print("first five", np.mean(hist[:5]), "last five", np.mean(hist[-5:]))
    assert np.mean(hist[-5:]) < np.mean(hist[:5])
    dec.set_weights(dec.get_weights())
