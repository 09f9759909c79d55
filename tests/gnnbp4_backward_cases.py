"""Cases and restatement runs shared by tests/test_gnnbp4_backward_cases_cpu.py and tests/test_gpu_gnnbp4_backward_elementwise.py: the
GNN_BP4 reverse pass through tests/gnnbp4_reference.py in float64 (the checker) or float32 (the rounding yardstick), the seeded host
draws of both files, the launch plan of the reverse pass restated (a precondition on the cases, not an oracle), and the draw with
saturated binary LLRs of the clip test."""
import functools
from collections import namedtuple

import numpy as np
import torch

import gnnbp4_reference as R
from helpers import code
from feedback_gnn_amd.graph import ACTIVATIONS, REDUCE_OPS, gnnbp4_weight_shapes

P = 0.05
K = 32                                # the margin over e32 (tests/test_gpu_gnnbp4_backward_elementwise.py derives it)
PHI_MAX = 16.635532                   # FG_PHI_MAX of fgnn_math.h
LDS_BUDGET = 160 * 1024 - 256         # FGNN_LDS_BUDGET of fgnn_internal.h
SURVEY = (20, 40, 2, "mean", "tanh", True)   # the configuration the compile-time (FX) kernels are instantiated for
WIDE = (32, 96, 2, "mean", "tanh", True)     # the widest vectors of the runtime-shaped kernels: the 128- and 64-thread layouts
SMALL = (8, 16, 2, "mean", "tanh", True)     # a runtime-shaped small configuration

# weight seed and Glorot scale per configuration (tests/test_gpu_gnnbp4_backward.py WEIGHT_DRAW; everything else (7, 1.0))
WEIGHT_DRAW = {(8, 16, 1, "sum", "linear", True): (2, 0.5)}

# key -> (code, configuration, B, T, loss_from, FX): FX = the configuration is SURVEY and the case runs on the compile-time kernels and,
# under force_generic, on the runtime-shaped ones; otherwise on the runtime-shaped kernels only.  `four_x`: K e32 <= 5e-4 max|r64| is
# asserted (not for gb48_limits, whose float32 restatement is within 3.3e-4 only, nor for rsurf5_deep with its three relu layers,
# 7.5e-5: there the bound is min(K e32, 2e-3 max|r64|)).
Case = namedtuple("Case", "name cfg B T loss_from fx four_x inv_scale", defaults=(0.5,))
_EXISTING = {"gb48_small": ("gb48", (8, 16, 1, "sum", "linear", True)), "rsurf5_deep": ("rsurf5", (12, 24, 3, "mean", "relu", False)),
             "ghp882_survey": ("ghp882", SURVEY), "gb48_limits": ("gb48", (32, 96, 4, "mean", "sigmoid", True))}
CASES = {}
for _k, (_name, _cfg) in _EXISTING.items():   # the four cases of tests/test_gpu_gnnbp4_backward.py; ghp882: 256 threads, 4 chunks
    for _lf in (0, 1):
        CASES[f"{_k}_lf{_lf}"] = Case(_name, _cfg, 3, 3, _lf, _cfg == SURVEY, _k not in ("gb48_limits", "rsurf5_deep"))
CASES.update({
    # the FX instantiation on an irregular code with degree-2 checks (n = 25), on n = 48 < 64, on n = 98 = 64 + 34; T = 1; B = 1
    "fx_rsurf5": Case("rsurf5", SURVEY, 3, 3, 0, True, True),
    "fx_gb48": Case("gb48", SURVEY, 3, 3, 0, True, True),
    "fx_hp_c7": Case("hp_c7", SURVEY, 2, 2, 0, True, True),
    "fx_rsurf5_T1": Case("rsurf5", SURVEY, 3, 1, 0, True, True),
    "fx_gb48_B1": Case("gb48", SURVEY, 1, 2, 0, True, True),
    # 128 threads, 1270 = 9 * 128 + 118; 64 threads, 2730 = 42 * 64 + 42 and 1365 = 21 * 64 + 21 checks per side
    "wg128_ghp1270": Case("ghp1270", WIDE, 2, 2, 0, False, True),
    "wg64_bb2730": Case("bb2730", WIDE, 2, 2, 0, False, True),
    # past the workgroup cap of 512: workgroups 0, 1, 2 take a second codeword
    # (no four_x: float32 sums over 515 codewords' rows depend on how the host's BLAS blocks them, e32 / max|r64| was 6e-7 on one
    # machine and 4.5e-5 on another)
    "b515_gb48": Case("gb48", (8, 16, 1, "sum", "linear", True), 515, 2, 0, False, False),
    # the largest code the reverse pass takes at (4, 8, 1): [[6480, 1296]], 64 threads
    # (_llr_inv_embed drawn at 4: at 0.5 the high-degree rows saturate, phi(sum phi) = 1.2e-7, and almost no row has a gradient)
    # (no four_x, as for the 515 codewords: sums over 45 576 edge rows; K e32 / max|r64| was 6.8e-5 on one host, 3.1e-4 on another)
    "hp_big_fits": Case("hp_big", (4, 8, 1, "mean", "tanh", True), 1, 1, 0, False, False, 4.0),
})
PLAN_THREADS = {"ghp882_survey_lf0": 256, "wg128_ghp1270": 128, "wg64_bb2730": 64, "hp_big_fits": 64}
HP_BIG_REFUSED = (8, 16, 1, "mean", "tanh", True)
# code, configuration, B, T, inv_scale of the upstream-layout test (at 0.5 the logical rows of hp_c7 saturate and have no gradient)
ONE_HOT = ("hp_c7", SMALL, 3, 3, 2.0)
CLIP = dict(name="gb48", cfg=SURVEY, B=3, seed=9, inv_scale=8.0)


def full(cfg):
    return tuple(cfg) + (False, 0, 0)


def num(cfg):
    D, H, L, red, act, bias = cfg
    return (D, H, L, REDUCE_OPS[red], ACTIVATIONS[act], int(bias))


@functools.lru_cache(maxsize=None)
def weights(name, cfg, inv_scale=0.5, seed=None):
    s, kernel_scale = WEIGHT_DRAW.get(cfg, (7, 1.0))
    return R.seeded_weights(gnnbp4_weight_shapes(code(name), full(cfg)), s if seed is None else seed, inv_scale=inv_scale,
                            kernel_scale=kernel_scale)


@functools.lru_cache(maxsize=None)
def batch(name, B, seed=1):
    """(noise_x, noise_z, syndrome_x, syndrome_z) uint8 on the host: the draws of tests/test_gpu_gnnbp4_backward.py."""
    return R.depolarizing_noise(code(name), B, seed, P)


# ---- the launch plan of the reverse pass, restated (bwd_plan of fgnn_gnnbp4_backward.hip) -------------------------------------------------
def _up4(x):
    return (x + 3) & ~3


def plan_threads(name, cfg, fx=False):
    """(threads, LDS bytes) of the first workgroup size of 256, 128, 64 whose layout fits the budget; (0, bytes at 64 threads) = refused."""
    c = code(name)
    n, m = int(np.asarray(c.hx).shape[1]), int(np.asarray(c.hx).shape[0] + np.asarray(c.hz).shape[0])
    rows = int(np.asarray(c.lx).shape[0] + np.asarray(c.lz).shape[0])
    D, H, L = cfg[:3]
    if fx:
        assert tuple(cfg) == SURVEY
        KA, JD = 3 * D, H + D
    else:
        KA, JD = D, 4
        for nin in (2 * D, 2 * D, 2 * D + 1, 2 * D + 1, 2 * D, 2 * D, 3 * D):
            for l in range(L):
                KA = max(KA, nin if l == 0 else H)
                JD = max(JD, _up4(D if l == L - 1 else H))
    misc = _up4(4 * n + 2 * m + rows)
    for nt in (256, 128, 64):
        nbytes = (misc + _up4(KA * (nt + 1)) + nt * JD) * 4
        if nbytes <= LDS_BUDGET:
            return nt, nbytes
    return 0, nbytes


def tape_forward_lds_bytes(name):
    c = code(name)
    return (2 * int(np.asarray(c.hx).shape[1]) + int(np.asarray(c.hx).shape[0] + np.asarray(c.hz).shape[0])) * 4


# ---- restatement runs -------------------------------------------------------------------------------------------------------------------------
class Ref:
    """One forward of the restatement in one precision, with what the tape keeps, differentiated as often as a test has upstream
    gradients (loss-based: `loss_grads`; direct: `grad`)."""

    def __init__(self, name, cfg, B, T, dtype, w=None, seed=1):
        self.name, self.dtype, self.T, self.B = name, dtype, T, B
        self.ex, self.ez, sx, sz = batch(name, B, seed)
        self.w = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (weights(name, cfg) if w is None else w)]
        self.rec = {}
        xs, zs, _ = R.forward(R.Graph(code(name)), num(cfg), self.w, torch.from_numpy(sx), torch.from_numpy(sz), T, record=self.rec)
        self.xs, self.zs = torch.stack(xs), torch.stack(zs)  # [T, B, rows]
        assert self.xs.dtype == dtype

    def _grads(self, loss):
        out = torch.autograd.grad(loss, self.w, retain_graph=True, allow_unused=True)
        return [np.zeros(tuple(w.shape)) if g is None else g.double().numpy() for g, w in zip(out, self.w)]

    def loss_grads(self, loss_from=0, sides=(True, True)):
        gx, gz = R.labels(code(self.name), self.ex, self.ez)
        loss = R.loss(list(self.xs), list(self.zs), torch.from_numpy(gx).to(self.dtype), torch.from_numpy(gz).to(self.dtype), loss_from,
                      sides)
        return float(loss.detach()), self._grads(loss)

    def grad(self, gx, gz):
        """d / d weights of <xs, gx> + <zs, gz>; a side that is None does not enter."""
        loss = sum((a * torch.from_numpy(np.asarray(u)).to(self.dtype)).sum() for a, u in ((self.xs, gx), (self.zs, gz)) if u is not None)
        return self._grads(loss)

    def tape(self):
        """The tape's three parts as float64 arrays [B, T, ...]: h_vn, h_cn, hlog."""
        return {k: torch.stack(self.rec[k], 1).detach().double().numpy() for k in ("h_vn", "h_cn", "hlog")}

    def signs(self):
        return np.sign(np.concatenate([self.xs.detach().double().numpy().ravel(), self.zs.detach().double().numpy().ravel()]))


@functools.lru_cache(maxsize=None)
def case_refs(key):
    """(float64 Ref, float32 Ref, (loss64, grads64), (loss32, grads32)) of one loss-based case; computed once and shared."""
    c = CASES[key]
    w = weights(c.name, c.cfg, inv_scale=c.inv_scale)
    r64, r32 = (Ref(c.name, c.cfg, c.B, c.T, dt, w=w) for dt in (torch.float64, torch.float32))
    return r64, r32, r64.loss_grads(c.loss_from), r32.loss_grads(c.loss_from)


@functools.lru_cache(maxsize=None)
def refs(name, cfg, B, T, inv_scale=0.5):
    w = weights(name, cfg, inv_scale=inv_scale)
    return tuple(Ref(name, cfg, B, T, dt, w=w) for dt in (torch.float64, torch.float32))


def one_hot_points(name, T, B):
    """(side, k, b, row) of the upstream-layout test: both sides, k in {0, T-1}, b in {0, B-1}, the first and last check row and the
    first and last logical row."""
    c = code(name)
    pts = []
    for side, (chk, log) in enumerate(((c.hz, c.lz), (c.hx, c.lx))):   # x_logit rows: hz then lz; z_logit rows: hx then lx
        mc, ml = int(np.asarray(chk).shape[0]), int(np.asarray(log).shape[0])
        for k in sorted({0, T - 1}):
            for b in sorted({0, B - 1}):
                for row in (0, mc - 1, mc, mc + ml - 1):
                    pts.append((side, k, b, row))
    return pts


def one_hot(name, T, B, side, k, b, row, value=1.0):
    """(gx, gz) float32 [T, B, rows]: `value` at (k, b, row) of one side, zeros elsewhere."""
    c = code(name)
    rx = int(np.asarray(c.hz).shape[0] + np.asarray(c.lz).shape[0])
    rz = int(np.asarray(c.hx).shape[0] + np.asarray(c.lx).shape[0])
    g = [np.zeros((T, B, rx), np.float32), np.zeros((T, B, rz), np.float32)]
    g[side][k, b, row] = value
    return g[0], g[1]


# ---- the clip of phi ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_case():
    """gb48 at T = 1 with an _llr_inv_embed kernel drawn at CLIP["inv_scale"]: most binary LLRs lie above PHI_MAX, where the clipped phi
    has derivative 0.  On codeword 0, per side (0: hz rows on llr_x, 1: hx rows on llr_z): a `dead` check row, whose qubits are all
    clipped in float64 (its one-hot upstream gives a weight gradient that is exactly zero); and one `live` row for the draw: of the
    rows that hold a side's least saturated qubit (its phi dominates the row's sum, and float32 carries it best) the one on which
    float32 autograd comes closest to float64.  A row is eligible only if every qubit of it is at least 1e-3 (relative) from the
    clip edge in both precisions and on the same side of it.  Returns dict(w, refs, dead=[(side, row)], live=(side, row) or None,
    live_rel, frac=[clipped share of |llr| per side], margin=smallest relative distance of a chosen row's qubits from the edge)."""
    name, cfg, B = CLIP["name"], CLIP["cfg"], CLIP["B"]
    w = weights(name, cfg, inv_scale=CLIP["inv_scale"], seed=CLIP["seed"])
    r64, r32 = (Ref(name, cfg, B, 1, dt, w=w) for dt in (torch.float64, torch.float32))
    c = code(name)
    dead, cand, margin, frac = [], [], np.inf, []
    for side, (key, mat) in enumerate((("llr_x", c.hz), ("llr_z", c.hx))):
        a = np.abs(r64.rec[key][0].detach().numpy()[0])
        a32 = np.abs(r32.rec[key][0].detach().double().numpy()[0])
        mat = np.asarray(mat).astype(bool)
        frac.append(float((a > PHI_MAX).mean()))
        far = lambda r: min(np.abs(a[mat[r]] / PHI_MAX - 1).min(), np.abs(a32[mat[r]] / PHI_MAX - 1).min())
        ok = [r for r in range(mat.shape[0]) if far(r) > 1e-3 and ((a > PHI_MAX) == (a32 > PHI_MAX))[mat[r]].all()]
        dd = [r for r in ok if (a[mat[r]] > PHI_MAX).all()]
        lv = [r for r in ok if (a[mat[r]] <= PHI_MAX).any()]
        if dd:
            dead.append((side, dd[0]))
            margin = min(margin, far(dd[0]))
        if lv:
            r = min(lv, key=lambda r: a[mat[r]].min())
            gx, gz = one_hot(name, 1, B, side, 0, 0, r)
            g64, g32 = r64.grad(gx, gz), r32.grad(gx, gz)
            rel = max(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300) for x, y in zip(g32, g64))
            cand.append((rel, side, r, far(r)))
    live = min(cand) if cand else None
    if live:
        margin = min(margin, live[3])
    return dict(w=w, refs=(r64, r32), dead=dead, live=live and (live[1], live[2]), live_rel=live and float(live[0]), frac=frac,
                margin=float(margin))
