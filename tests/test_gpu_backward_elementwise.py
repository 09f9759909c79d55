"""The three reverse-pass kernels of feedback_gnn_amd/csrc/fgnn_backward.hip (bp4_backward_kernel, gnn_backward_kernel,
gnn_general_backward_kernel) element by element and row by row, at bounds taken from float32 rounding itself.

THE BOUND.  For every output array three values are computed from the same inputs: r64, the float64 restatement
(oracle/torch_ref.py); r32, the same statements in float32 on the CPU; got, the GPU result.  With e32 = max|r32 - r64| over the
array, the test asserts max|got - r64| <= K e32 and, elementwise, |got - r64| <= K e32 + 1e-5 |r64|.  Where e32 = 0 the array is a
copy of inputs (e_feat, the X Y Z columns of node_in, the deltas of _llr_inv_embed) and must be bit-equal.  The margin K exists
because the kernel's fg_exp / fg_log / fg_tanh / bw_expm1 are a few ulp from libm and its association differs from torch's; K is the
smallest power of two that leaves a factor 2 over the largest ratio max|got - r64| / e32 measured in this file on an MI355X (table
below).  On every array that tests/test_gpu_backward.py also checks (the BP4 gradient at 2e-3 / 1e-3 of its largest entry, the weight
gradients at 1e-3 shipped / 2e-3 runtime-shaped) K e32 must be at least 4 times tighter than that file's bound: `_check(loose=...)`
asserts it.  Every test prints its ratios (pytest -s).

MEASURED on an MI355X: the largest ratio max|got - r64| / e32 per group of arrays and, in brackets, the largest K e32 / max|r64| of
the group at K = 16.  The largest ratio of the file is 5.59, so K = 16 (8 would leave a factor 1.4 only).
  bp4 steane                                     grad 1.42 (1.5e-05)
  bp4 rsurf5                                     grad 1.32 (2.2e-05)
  bp4 gb48                                       grad 0.15 (2.1e-04)
  bp4 hp_c7                                      grad 0.72 (5.7e-05)
  bp4 ghp882                                     grad 0.58 (2.2e-05)
  bp4 ghp1270                                    grad 0.47 (2.5e-05)
  bp4 locality ghp882                            grad 1.11 (6.4e-05)
  bp4 locality rsurf5                            grad 1.55 (1.4e-05)
  bp4 clip, the unclipped neighbour row          grad 0.00 (1.7e-01)
  shipped gb48                                   deltas 1.54 (5.2e-06)  acts 1.18 (1.1e-05)  wgrad 1.71 (1.3e-05)
  shipped rsurf5                                 deltas 1.73 (4.4e-06)  acts 1.28 (9.5e-06)  wgrad 2.39 (9.0e-06)
  shipped ghp882                                 deltas 1.46 (6.7e-06)  acts 1.20 (1.4e-05)  wgrad 2.08 (4.2e-05)
  general gb48 (8, 16, 1, mean, tanh, bias)      deltas 1.00 (9.6e-07)  acts 0.76 (2.0e-06)  wgrad 1.25 (1.8e-05)
  general rsurf5 (12, 24, 3, sum, relu, no bias) deltas 1.45 (3.3e-06)  acts 1.60 (4.1e-06)  wgrad 1.06 (7.9e-06)
  general gb48 (20, 40, 2, max, sigmoid, bias)   deltas 1.19 (5.0e-06)  acts 1.21 (6.7e-06)  wgrad 1.57 (7.5e-06)
  general rsurf5 (6, 10, 4, min, tanh, bias)     deltas 2.05 (7.0e-06)  acts 1.52 (3.6e-06)  wgrad 3.06 (1.1e-05)
  general ghp882 (16, 32, 2, mean, tanh, no bias) deltas 1.80 (6.4e-06)  acts 1.25 (1.5e-05)  wgrad 5.59 (1.6e-05)
  general gb48 (20, 40, 2, mean, tanh, bias)     deltas 1.47 (4.8e-06)  acts 1.51 (1.3e-05)  wgrad 3.44 (1.2e-05)
  general gb48 (32, 96, 4, mean, tanh, bias)     deltas 1.21 (7.2e-05)  acts 1.31 (1.1e-04)  wgrad 1.17 (5.8e-05)
  general gb48 (1, 1, 1, sum, linear, no bias)   deltas 1.00 (9.9e-07)  acts 0.71 (1.8e-06)  wgrad 2.65 (8.1e-06)
  ties gb48 relu/max                             deltas 1.00 (2.0e-06)  acts 0.98 (4.4e-06)  wgrad 1.94 (9.1e-06)
  ties gb48 relu/min                             deltas 1.00 (1.3e-06)  acts 1.11 (2.1e-06)  wgrad 1.94 (9.9e-06)
  ties rsurf5 relu/max                           deltas 1.00 (2.0e-06)  acts 1.00 (2.3e-06)  wgrad 1.78 (5.1e-06)
  ties rsurf5 relu/min                           deltas 1.00 (2.2e-06)  acts 1.07 (3.0e-06)  wgrad 2.15 (4.9e-06)
The 4x condition: the bracketed figure stays below 2.5e-4 (arrays the other file holds to 1e-3: the BP4 gradient at zero
iterations, at most 1.5e-4 here; the shipped weight gradients) and below 5e-4 (2e-3 there) on every such array, so every bound here
is at least 6 times tighter than the other file's, and most are 50 to 400 times tighter.  Two places where the yardstick itself is wide: on gb48 the float32
restatement of the BP4 reverse pass is about ten times less accurate than the kernel (ratio 0.15; its phi is softplus - log expm1, a
difference of rounded terms, where the kernel has fg_phi and bw_expm1), and the unclipped row of the clip test takes phi' at a binary
LLR of 1e-3, whose float32 value carries a relative error of 1e-4 before the kernel does anything: there the exact zeros of the
clipped row are the check, and the bound on its neighbour only says that the row is alive and right to two digits.

The GNN kernels' rows are read through TannerGraph.feedback_gnn_backward_pairs, the one place their buffers are sized."""
import numpy as np
import pytest
import torch

from backward_cases import F32, reference_pairs, tie_case, tie_expectation
from helpers import WEIGHTS_882, code, gpu_graph, to_gpu
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
K = 16
PHI_MAX = 16.635532


def _np(t):
    return t.detach().cpu().double().numpy()


def _check(label, got, r64, r32, loose=None):
    """The bound of the module docstring on one array; ``loose`` = the relative bound tests/test_gpu_backward.py puts on the same array.
    Returns the measured ratio (0 where bit equality is required)."""
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    assert got.shape == r64.shape == r32.shape, (label, got.shape, r64.shape, r32.shape)
    assert np.isfinite(got).all(), label
    e32 = np.abs(r32 - r64).max()
    if e32 == 0.0:
        print(f"RATIO {label}: e32 = 0, bit equality")
        assert np.array_equal(got, r64), label
        return 0.0
    err, scale = np.abs(got - r64), np.abs(r64).max()
    ratio = err.max() / e32
    print(f"RATIO {label}: max|got-r64| = {err.max():.3e}  e32 = {e32:.3e}  ratio = {ratio:.3f}  K*e32/max|r64| = {K * e32 / scale:.2e}")
    assert err.max() <= K * e32, (label, ratio)
    assert (err <= K * e32 + 1e-5 * np.abs(r64)).all(), label
    if loose is not None:
        assert K * e32 <= loose / 4 * scale, (label, K * e32 / scale, loose)
    return ratio


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- bp4_backward ------------------------------------------------------------------------------------------------------------------------
def _bp4_inputs(name, B, seed=3):
    g = gpu_graph(name)
    ex, ez = g.pauli_noise(20240607, 0.03, 0, B)
    sx, sz = g.syndrome(ex, ez)
    llr = np.random.RandomState(seed).uniform(0.8, 2.5, size=(B, 3, g.n)).astype(F32)
    return g, sx, sz, llr


class _Bp4Ref:
    """The restatement's soft syndromes of one input in one precision, differentiated as often as a test has upstream gradients."""

    def __init__(self, name, llr, sx, sz, T, factor, dtype):
        self.dtype = dtype
        self.L = torch.from_numpy(llr).to(dtype).requires_grad_(True)
        xs, zs, _ = R.bp4_logit_trace(R.Graph(code(name)), self.L, sx.cpu(), sz.cpu(), T, factor)
        self.xs, self.zs = torch.stack(xs), torch.stack(zs)  # [T+1, B, rows]

    def grad(self, gx, gz):
        """d / d llr_ch of sum_k <xs[k], gx[k]> + <zs[k], gz[k]>; a side that is None does not enter."""
        loss = sum((a * torch.from_numpy(u).to(self.dtype)).sum() for a, u in ((self.xs, gx), (self.zs, gz)) if u is not None)
        return torch.autograd.grad(loss, self.L, retain_graph=True)[0].double().numpy()


def _bp4_gpu(g, llr, sx, sz, T, factor, gx, gz):
    d_llr = to_gpu(llr)
    tr = g.bp4_logit_trace(d_llr, sx, sz, T, factor)
    up = [None if u is None else to_gpu(u) for u in (gx, gz)]
    return _np(g.bp4_backward(d_llr, sx, sz, tr["tape_x"], tr["tape_z"], up[0], up[1], factor))


def _bp4_calibrated(name, B, T, factor):
    loose = 1e-3 if T == 0 else 2e-3  # tests/test_gpu_backward.py: 1e-3 at zero iterations, 2e-3 with iterations
    g, sx, sz, llr = _bp4_inputs(name, B)
    refs = [_Bp4Ref(name, llr, sx, sz, T, factor, dt) for dt in (torch.float64, torch.float32)]
    rng = np.random.RandomState(41)
    gx = rng.normal(size=(T + 1, B, g.rows_xp)).astype(F32)
    gz = rng.normal(size=(T + 1, B, g.rows_zp)).astype(F32)
    last = [np.where(np.arange(T + 1)[:, None, None] == T, u, 0).astype(F32) for u in (gx, gz)]
    modes = dict(every_slot=(gx, gz), x_side_null=(None, gz), z_side_null=(gx, None))
    if T > 0:
        modes["last_slot"] = tuple(last)
    for mode, (ux, uz) in modes.items():
        got = _bp4_gpu(g, llr, sx, sz, T, factor, ux, uz)
        r64, r32 = (r.grad(ux, uz) for r in refs)
        assert np.abs(r64).max() > 0
        _check(f"bp4 {name} T={T} f={factor} {mode}", got, r64, r32, loose=loose)


@pytest.mark.parametrize("factor", [1.0, 0.8])
@pytest.mark.parametrize("T", [0, 1, 2])
@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb48", "hp_c7"])
def test_bp4_backward_calibrated(name, T, factor):
    """Seeded normal upstream gradients fed to both sides directly (no BCE on GPU logits), B = 3, llr in [0.8, 2.5]: gradients in
    every slot, in the last slot only, and with either side NULL."""
    _bp4_calibrated(name, 3, T, factor)


@pytest.mark.parametrize("name,B,T,factor", [("ghp882", 3, 2, 1.0), ("ghp882", 3, 2, 0.8), ("ghp1270", 2, 1, 1.0)])
def test_bp4_backward_calibrated_strided(name, B, T, factor):
    """n > 256: a thread's `v += nt` loops take more than one qubit and more than one row; ghp1270 is the largest shipped code that
    fits the kernel's LDS."""
    assert gpu_graph(name).n > 256
    _bp4_calibrated(name, B, T, factor)


@pytest.mark.parametrize("side", ["x", "z"])
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("name", ["ghp882", "rsurf5"])
def test_bp4_backward_locality(name, k, side):
    """An upstream gradient in one row of one slot of one codeword: wherever the float64 gradient is exactly 0 (the qubits that k
    iterations cannot reach from the row, and every other codeword) the GPU gradient is exactly 0; the rest obeys the bound."""
    B, T, b = 3, 2, 1
    g, sx, sz, llr = _bp4_inputs(name, B)
    rows = g.rows_xp if side == "x" else g.rows_zp
    up = np.zeros((T + 1, B, rows), F32)
    up[k, b, rows - 1] = 1.75
    other = np.zeros((T + 1, B, g.rows_zp if side == "x" else g.rows_xp), F32)
    ux, uz = (up, other) if side == "x" else (other, up)
    got = _bp4_gpu(g, llr, sx, sz, T, 1.0, ux, uz)
    r64, r32 = (_Bp4Ref(name, llr, sx, sz, T, 1.0, dt).grad(ux, uz) for dt in (torch.float64, torch.float32))
    zero = r64 == 0
    assert zero.any() and (~zero[b]).any() and zero[[0, 2]].all()
    assert (got[zero] == 0).all(), np.abs(got[zero]).max()
    _check(f"bp4 locality {name} k={k} {side}", got, r64, r32)


@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_bp4_backward_batch_independence(name):
    """Codeword c alone, first of five and last of five: its tape and its gradient are byte-identical."""
    B, T, c = 5, 2, 2
    g, sx, sz, llr = _bp4_inputs(name, B)
    rng = np.random.RandomState(43)
    gx = rng.normal(size=(T + 1, B, g.rows_xp)).astype(F32)
    gz = rng.normal(size=(T + 1, B, g.rows_zp)).astype(F32)
    res = []
    for order, pos in (([c], 0), ([c, 0, 1, 3, 4], 0), ([0, 1, 3, 4, c], 4)):
        d_llr, s_x, s_z = to_gpu(llr[order]), sx[order].contiguous(), sz[order].contiguous()
        tr = g.bp4_logit_trace(d_llr, s_x, s_z, T, 0.9)
        out = g.bp4_backward(d_llr, s_x, s_z, tr["tape_x"], tr["tape_z"], to_gpu(gx[:, order]), to_gpu(gz[:, order]), 0.9)
        res.append((tr["tape_x"][:, pos], tr["tape_z"][:, pos], out[pos]))
    assert float(res[0][2].abs().max()) > 0
    for other in res[1:]:
        for a, b_ in zip(res[0], other):
            assert torch.equal(_bits(a), _bits(b_))


def test_bp4_backward_clipped_row_contributes_nothing():
    """T = 0 on gb48: three qubits of one hz row carry a binary llr_x of about 1e-3, so the row's T = sum phi(|v|) is far above PHI_MAX in
    both precisions and the clip blocks its gradient (dphi returns 0 outside [PHI_MIN, PHI_MAX]): an upstream gradient on that row
    alone gives all zeros; a neighbouring row that holds one of the three qubits is not clipped and obeys the bound."""
    name, B = "gb48", 3
    g, sx, sz, llr = _bp4_inputs(name, B)
    hz = np.asarray(code(name).hz)
    r0 = 5
    q = np.nonzero(hz[r0])[0][:3]
    a = 1e-3 + np.log(2.0) - np.log1p(np.exp(-3.0))  # X = Y = a, Z = 3: llr_x = softplus(-Z) - lse(-X, -Y) = 1e-3
    llr[:, 0, q] = llr[:, 1, q] = F32(a)
    llr[:, 2, q] = 3.0
    crafted = hz[:, q].sum(1)
    r1 = [r for r in np.argsort(crafted, kind="stable") if crafted[r] == 1 and r != r0][0]
    for dt in (np.float32, np.float64):  # the restatement's own formulas for the rows' T
        X, Y, Z = (llr[:, i].astype(dt) for i in range(3))
        llr_x = np.log1p(np.exp(-Z)) - np.logaddexp(-X, -Y)
        assert (np.abs(llr_x[:, q] - 1e-3) < 1e-5).all()
        Trow = (-np.log(np.tanh(np.abs(llr_x) / 2)))[:, None, :] * hz[None]
        Trow = Trow.sum(-1)
        assert (Trow[:, r0] > PHI_MAX + 4).all() and (Trow[:, r1] < PHI_MAX - 1).all(), (Trow[:, r0], Trow[:, r1])
    refs = [_Bp4Ref(name, llr, sx, sz, 0, 1.0, dt) for dt in (torch.float64, torch.float32)]
    rng = np.random.RandomState(47)
    for row, clipped in ((r0, True), (r1, False)):
        gx = np.zeros((1, B, g.rows_xp), F32)
        gx[0, :, row] = rng.normal(size=B)
        gz = np.zeros((1, B, g.rows_zp), F32)
        got = _bp4_gpu(g, llr, sx, sz, 0, 1.0, gx, gz)
        r64, r32 = (r.grad(gx, gz) for r in refs)
        if clipped:
            assert (r64 == 0).all() and (r32 == 0).all() and (got == 0).all()
        else:
            assert (r64 != 0).any()
            _check(f"bp4 clip neighbour row {row}", got, r64, r32)


def test_bp4_backward_refuses_a_code_too_large_for_lds_and_goes_on():
    big = gpu_graph("hp_big")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=big.device)  # noqa: E731
    u = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=big.device)  # noqa: E731
    with pytest.raises(ValueError, match="too large for the LDS-resident backward kernel"):
        big.bp4_backward(z(1, 3, big.n), u(1, big.m_x), u(1, big.m_z), z(1, 1, big.E_x), z(1, 1, big.E_z), z(1, 1, big.rows_xp),
                         z(1, 1, big.rows_zp))
    _bp4_calibrated("gb48", 3, 1, 0.8)


# ---- the feedback GNN's reverse kernels, row by row ----------------------------------------------------------------------------------------
def _gnn_inputs(name, B, lim, seed, cfg):
    """Inputs and weights as tests/test_gpu_backward.py draws them (shipped: cfg None)."""
    from feedback_gnn_amd.graph import gnn_weight_shapes
    from feedback_gnn_amd.weights_io import read_weight_list
    from test_gpu_backward import _case
    g, sx, sz, llr = _case(name, B, 0.04, -2.0, 6.0)
    rng = np.random.RandomState(seed)
    if cfg is None:
        w = read_weight_list(WEIGHTS_882)
        w[0] = rng.uniform(-0.4, 0.4, size=w[0].shape).astype(F32)
    else:
        w = [rng.uniform(-0.5, 0.5, size=shp).astype(F32) for shp in gnn_weight_shapes(cfg[0], cfg[1], cfg[2], cfg[5])]
    lhx = rng.uniform(-lim, lim, size=(B, g.m_x)).astype(F32)
    lhz = rng.uniform(-lim, lim, size=(B, g.m_z)).astype(F32)
    gout = rng.normal(size=(B, 3, g.n)).astype(F32)
    return g, dict(w=w, llr=llr, lhx=lhx, lhz=lhz, sx=sx.cpu().numpy(), sz=sz.cpu().numpy(), gout=gout)


def _weights(g, w, cfg):
    from feedback_gnn_amd.graph import GnnWeights
    W = GnnWeights(w, g.device) if cfg is None else GnnWeights(w, g.device, config=cfg, force_general=True)
    assert W.general == (cfg is not None)
    return W


def _gpu_args(t):
    return tuple(to_gpu(t[k]) for k in ("llr", "lhx", "lhz", "sx", "sz", "gout"))


def _refs(name, cfg, t, g):
    edges = [g.edges(0), g.edges(1)]
    args = (name, cfg, t["w"], t["llr"], t["lhx"], t["lhz"], t["sx"], t["sz"], t["gout"])
    return reference_pairs(*args, torch.float64, edges), reference_pairs(*args, torch.float32, edges)


def _check_rows(tag, g, pairs, r64, r32, cfg):
    """Every array the kernel wrote against the restatement's rows."""
    D, L = (20, 2) if cfg is None else (cfg[0], cfg[2])
    B = r64["out"].shape[0]
    rows = [B * g.E_x] * L + [B * g.E_z] * L + [B * g.n] * L
    assert len(pairs) == 3 * L
    for li, (a, d) in enumerate(pairs):
        a, d = _np(a), _np(d)
        assert a.shape[0] == d.shape[0] == rows[li], (tag, li)
        if li == 2 * L:  # [reduced_x | reduced_z | X Y Z], 44 wide with a zero column in the shipped kernel
            if cfg is None:
                assert a.shape[1] == 44 and (a[:, 43] == 0).all()
                a = a[:, :43]
            _check(f"{tag} acts[{li}] reduced", a[:, :2 * D], r64["acts"][li][:, :2 * D], r32["acts"][li][:, :2 * D])
            _check(f"{tag} acts[{li}] XYZ", a[:, 2 * D:], r64["acts"][li][:, 2 * D:], r32["acts"][li][:, 2 * D:])
        else:
            _check(f"{tag} acts[{li}]", a, r64["acts"][li], r32["acts"][li])
        _check(f"{tag} deltas[{li}]", d, r64["deltas"][li], r32["deltas"][li])


def _check_weight_grads(tag, grads, r64, r32, loose):
    assert len(grads) == len(r64["wgrads"])
    for i, got in enumerate(grads):
        _check(f"{tag} wgrad[{i}]", _np(got), r64["wgrads"][i], r32["wgrads"][i], loose=loose)


GENERAL_CASES = [("gb48", (8, 16, 1, "mean", "tanh", True)), ("rsurf5", (12, 24, 3, "sum", "relu", False)),
                 ("gb48", (20, 40, 2, "max", "sigmoid", True)), ("rsurf5", (6, 10, 4, "min", "tanh", True)),
                 ("ghp882", (16, 32, 2, "mean", "tanh", False)), ("gb48", (20, 40, 2, "mean", "tanh", True)),
                 ("gb48", (32, 96, 4, "mean", "tanh", True)),       # FGNN_GEN_MAX_D, FGNN_GEN_MAX_W and four layers: the per-thread arrays full
                 ("gb48", (1, 1, 1, "sum", "linear", False))]      # the smallest setting the constructor accepts


@pytest.mark.parametrize("name,B", [("gb48", 3), ("rsurf5", 3), ("ghp882", 2)])
def test_shipped_gnn_backward_rows(name, B):
    g, t = _gnn_inputs(name, B, 8, 5, None)
    W = _weights(g, t["w"], None)
    r64, r32 = _refs(name, None, t, g)
    _check_rows(f"gnn {name}", g, g.feedback_gnn_backward_pairs(W, *_gpu_args(t)), r64, r32, None)
    _check_weight_grads(f"gnn {name}", g.feedback_gnn_backward(W, *_gpu_args(t)), r64, r32, 1e-3)


@pytest.mark.parametrize("name,cfg", GENERAL_CASES)
def test_general_gnn_backward_rows(name, cfg):
    g, t = _gnn_inputs(name, 2 if name == "ghp882" else 3, 4, 17, cfg)
    W = _weights(g, t["w"], cfg)
    r64, r32 = _refs(name, cfg, t, g)
    tag = f"general {name} {cfg}"
    _check_rows(tag, g, g.feedback_gnn_backward_pairs(W, *_gpu_args(t)), r64, r32, cfg)
    _check_weight_grads(tag, g.feedback_gnn_backward(W, *_gpu_args(t)), r64, r32, 2e-3)


@pytest.mark.parametrize("name,cfg", [("gb48", None), ("rsurf5", (6, 10, 4, "min", "tanh", True)), ("gb48", (8, 16, 2, "max", "relu", True))])
def test_gnn_backward_batch_independence(name, cfg):
    """Codeword c alone, first of five and last of five: its rows of every activation / delta array are byte-identical."""
    B, c = 5, 2
    g, t = _gnn_inputs(name, B, 4, 29, cfg)
    W = _weights(g, t["w"], cfg)
    L = 2 if cfg is None else cfg[2]
    per = [g.E_x] * L + [g.E_z] * L + [g.n] * L
    res = []
    for order, pos in (([c], 0), ([c, 0, 1, 3, 4], 0), ([0, 1, 3, 4, c], 4)):
        args = tuple(to_gpu(t[k][order]) for k in ("llr", "lhx", "lhz", "sx", "sz", "gout"))
        pairs = g.feedback_gnn_backward_pairs(W, *args)
        res.append([x[pos * per[li]:(pos + 1) * per[li]] for li, pair in enumerate(pairs) for x in pair])
    assert len(res[0]) == 6 * L and all(x.shape[0] == per[i // 2] for i, x in enumerate(res[0]))
    for other in res[1:]:
        for i, (a, b_) in enumerate(zip(res[0], other)):
            assert torch.equal(_bits(a), _bits(b_)), i


@pytest.mark.parametrize("red", ["max", "min"])
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_general_gnn_backward_ties_and_dead_units(name, red):
    """relu with max / min on crafted inputs (backward_cases.tie_case).  Ties: edges of a qubit into the tied checks have identical
    inputs, so they attain the extremum together in any precision; the deltas of the last message layer are gr / count on them and
    exactly 0 on the other edges (the amax / amin restatement; tie counts 1, 2 and, where a qubit has more than two checks of a side,
    more than 2 all occur, and float32 agrees with float64 on every count).  Dead units: the first message layers' pre-activations
    are exact half-integers, so both precisions agree on h > 0; a dead unit's delta is exactly 0."""
    cfg = (8, 16, 2, red, "relu", True)
    D, L = cfg[0], cfg[2]
    B = 3
    g = gpu_graph(name)
    t = tie_case(name, cfg, B, 31)
    W = _weights(g, t["w"], cfg)
    r64, r32 = _refs(name, cfg, t, g)
    var = [g.edges(s)[1] for s in range(2)]
    want, counts = tie_expectation(r64, var, D, L, red == "max")
    _, counts32 = tie_expectation(r32, var, D, L, red == "max")
    seen = set()
    for s in range(2):
        assert np.array_equal(counts[s], counts32[s])
        assert np.abs(r64["deltas"][s * L + L - 1] - want[s]).max() <= 1e-15 * np.abs(want[s]).max()
        seen |= set(np.unique(counts[s]).tolist())
    max_deg = max(int(np.bincount(v).max()) for v in var)
    assert {1, 2} <= seen and (max(seen) > 2) == (max_deg > 2), (seen, max_deg)
    assert max_deg > 2 or name == "rsurf5"
    pairs = g.feedback_gnn_backward_pairs(W, *_gpu_args(t))
    tag = f"ties {name} {red}"
    _check_rows(tag, g, pairs, r64, r32, cfg)
    for s in range(2):
        last = _np(pairs[s * L + L - 1][1])
        assert (want[s] == 0).any() and (want[s] != 0).any()
        assert (last[want[s] == 0] == 0).all(), "an edge that does not attain the extremum received gradient"
        _check(f"{tag} tie deltas side {s}", last, want[s], r32["deltas"][s * L + L - 1])
        pre = r64["pre"][s * L]
        assert np.abs(pre).min() >= 0.5 and np.array_equal(pre, r32["pre"][s * L])
        dead, first = pre < 0, _np(pairs[s * L][1])
        assert dead.any() and (~dead).any()
        assert (first[dead] == 0).all(), "a dead relu unit received gradient"
        assert (first[~dead] != 0).any()
    _check_weight_grads(tag, g.feedback_gnn_backward(W, *_gpu_args(t)), r64, r32, 2e-3)
