"""The checker of the reverse-pass kernels, checked on the CPU: oracle/torch_ref.py takes its dtype from its inputs (float32 runs of the
same statements are the rounding yardstick of tests/test_gpu_backward_elementwise.py), shares the gradient of max / min equally among
ties (TensorFlow's _MinOrMaxGrad, torch's amax / amin), and returns per Dense layer the (input activations, pre-activation) pairs whose
rows the kernels leave in HBM."""
import numpy as np
import pytest
import torch

from backward_cases import reference_pairs, tie_case, tie_expectation
from helpers import code
from oracle import torch_ref as R

# position-weighted sums of the float64 outputs and gradients of the two seeded cases below, computed by oracle/torch_ref.py as it
# stood before the dtype switch, amax / amin and the pairs option
BP4_BEFORE = [0.04662548748115365, -0.02272144640894035, 0.041311986167282023, -0.02285465370178141, 0.15947163842674072,
              0.3480410438794191]
GNN_BEFORE = [-4.9025993607570255, 41.509339139319785, -38.441508440361645, 29.117010996899545, -10.815364491737366,
              -19.17045482708757, -15.813499454692229, 0.4765279967671159, -1.9078248824670727, 23.370414240472474,
              -13.14373004874559, 7.40175706318559, -5.256126627451125, -2.90772699689242, 45.15482381325645, -16.615654061945712,
              62.47593796335375, -6.130977046723953, 9.65190197974794, -3.8834733339456577, -14.914429747217646, 17.587012008728024,
              23.4694380166794, -17.914554583936095, -26.63613139498274, 17.8677957802719]
SHIPPED_SHAPES = [(40, 3), (3,), (4, 40), (40,), (40, 20), (20,), (4, 40), (40,), (40, 20), (20,), (43, 40), (40,)]


def _mark(t):
    a = t.detach().double().numpy().ravel()
    return float((a * np.cos(np.arange(a.size) + 1.0)).sum())


def _bp4_case(dtype):
    """gb48, B = 2, three iterations at factor 0.9, loss = sum of sin(soft syndromes): outputs and d loss / d llr_ch."""
    c = code("gb48")
    g, rng, B = R.Graph(c), np.random.RandomState(101), 2
    llr = torch.from_numpy(rng.uniform(0.8, 2.5, size=(B, 3, g.n))).to(dtype).requires_grad_(True)
    sx = torch.from_numpy(rng.randint(0, 2, size=(B, c.hx.shape[0])).astype(np.uint8))
    sz = torch.from_numpy(rng.randint(0, 2, size=(B, c.hz.shape[0])).astype(np.uint8))
    xs, zs, tot = R.bp4_logit_trace(g, llr, sx, sz, 3, 0.9)
    sum(m.sin().sum() for m in xs + zs).backward()
    return [xs[0], zs[1], xs[3], zs[3], tot[1], llr.grad]


def _gnn_case(dtype):
    """rsurf5, B = 2: the runtime-shaped GNN at (6, 10, 2, max, tanh, bias) and the shipped architecture, loss = sum of sin(out):
    output and weight gradients of both."""
    from feedback_gnn_amd.graph import gnn_weight_shapes
    c = code("rsurf5")
    g, rng, B = R.Graph(c), np.random.RandomState(202), 2
    w = [torch.from_numpy(rng.uniform(-0.5, 0.5, size=s)).to(dtype).requires_grad_(True) for s in gnn_weight_shapes(6, 10, 2, True)]
    llr = torch.from_numpy(rng.uniform(-2, 6, size=(B, 3, g.n))).to(dtype)
    lhx = torch.from_numpy(rng.uniform(-4, 4, size=(B, c.hx.shape[0]))).to(dtype)
    lhz = torch.from_numpy(rng.uniform(-4, 4, size=(B, c.hz.shape[0]))).to(dtype)
    sx = torch.from_numpy(rng.randint(0, 2, size=(B, c.hx.shape[0])).astype(np.uint8))
    sz = torch.from_numpy(rng.randint(0, 2, size=(B, c.hz.shape[0])).astype(np.uint8))
    out = R.feedback_gnn_general(g, (6, 10, 2, 2, 1, True), w, llr, lhx, lhz, sx, sz)
    out.sin().sum().backward()
    res = [out] + [t.grad for t in w]
    ws = [torch.from_numpy(rng.uniform(-0.4, 0.4, size=s)).to(dtype).requires_grad_(True) for s in SHIPPED_SHAPES]
    out = R.feedback_gnn(g, ws, llr, lhx, lhz, sx, sz)
    out.sin().sum().backward()
    return res + [out] + [t.grad for t in ws]


@pytest.mark.parametrize("case,before", [(_bp4_case, BP4_BEFORE), (_gnn_case, GNN_BEFORE)], ids=["bp4", "gnn"])
def test_float64_outputs_are_what_they_were_and_float32_follows_them(case, before):
    """Float64 in, float64 out, the numbers of the module as it was (1e-12: the statements did not change); float32 in, float32 out,
    within 1e-4 of each array's largest entry of the float64 run (float32 rounding through three iterations or four Dense layers:
    measured 1e-7 .. 1e-5; a float64 constant left in a float32 run would promote the result and fail the dtype check)."""
    r64 = case(torch.float64)
    assert all(t.dtype == torch.float64 for t in r64)
    got = [_mark(t) for t in r64]
    assert len(got) == len(before)
    for i, (a, b) in enumerate(zip(got, before)):
        assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (i, a, b)
    r32 = case(torch.float32)
    assert all(t.dtype == torch.float32 for t in r32)
    for i, (a, b) in enumerate(zip(r32, r64)):
        a, b = a.detach().double().numpy(), b.detach().numpy()
        rel = np.abs(a - b).max() / np.abs(b).max()
        assert 0 < rel < 1e-4, (i, rel)  # 0 would mean the "float32" run was computed in float64


def test_second_stage_loss_takes_its_dtype_from_its_inputs():
    c = code("steane")
    g, rng, B = R.Graph(c), np.random.RandomState(7), 2
    sx = torch.from_numpy(rng.randint(0, 2, size=(B, c.hx.shape[0])).astype(np.uint8))
    sz = torch.from_numpy(rng.randint(0, 2, size=(B, c.hz.shape[0])).astype(np.uint8))
    draws = [rng.uniform(-0.4, 0.4, size=s) for s in SHIPPED_SHAPES] + [rng.uniform(0.8, 2.5, size=(B, 3, g.n)),
                                                                       rng.uniform(-4, 4, size=(B, c.hx.shape[0])),
                                                                       rng.uniform(-4, 4, size=(B, c.hz.shape[0]))]
    vals = {}
    for dt in (torch.float64, torch.float32):
        t = [torch.from_numpy(a).to(dt) for a in draws]
        loss, new_llr = R.second_stage_loss(g, t[:12], t[12], t[13], t[14], sx, sz, num_iter=3, loss_from=1)
        assert loss.dtype == new_llr.dtype == dt
        vals[dt] = float(loss)
    assert abs(vals[torch.float32] - vals[torch.float64]) < 1e-4 * abs(vals[torch.float64])


def test_library_edge_rows_maps_any_listing_of_the_edges():
    c = code("rsurf5")
    g = R.Graph(c)
    for s in range(2):
        chk, var = g.sides[s]["chk"].numpy(), g.sides[s]["var"].numpy()
        perm = np.random.RandomState(s).permutation(chk.size)
        idx = R.library_edge_rows(g, s, chk[perm], var[perm])
        assert np.array_equal(idx, perm)
        assert np.array_equal(R.library_edge_rows(g, s, chk, var), np.arange(chk.size))
    with pytest.raises(KeyError):
        R.library_edge_rows(g, 0, g.sides[1]["chk"].numpy(), g.sides[1]["var"].numpy())


@pytest.mark.parametrize("name,red", [("gb48", "max"), ("gb48", "min"), ("rsurf5", "max"), ("rsurf5", "min")])
def test_ties_share_the_gradient_equally_per_edge(name, red):
    """Crafted ties (backward_cases.tie_case): the per-edge deltas of the last message layer are gr / count on every edge that attains
    the extremum and 0 on the others — what amax / amin give and max(dim).values does not — against a few lines of NumPy, in float64
    exactly as far as a division goes (1e-15) and with the same tie pattern in float32."""
    cfg = (4, 6, 2, red, "relu", True)
    D, L = cfg[0], cfg[2]
    t = tie_case(name, cfg, 2, 11)
    args = (name, cfg, t["w"], t["llr"], t["lhx"], t["lhz"], t["sx"], t["sz"], t["gout"])
    r64, r32 = reference_pairs(*args, torch.float64), reference_pairs(*args, torch.float32)
    tg = R.Graph(code(name))
    var = [tg.sides[s]["var"].numpy() for s in range(2)]
    want, counts = tie_expectation(r64, var, D, L, red == "max")
    _, counts32 = tie_expectation(r32, var, D, L, red == "max")
    seen = set()
    for s in range(2):
        got = r64["deltas"][s * L + L - 1]
        assert np.abs(got - want[s]).max() <= 1e-15 * np.abs(want[s]).max()
        assert np.array_equal((got == 0), (want[s] == 0)) and (got == 0).any() and (got != 0).any()
        assert np.array_equal(counts[s], counts32[s]), "float32 and float64 disagree on who attains the extremum"
        seen |= set(np.unique(counts[s]).tolist())
        deg = np.bincount(var[s], minlength=tg.n)
        assert np.array_equal(counts[s] == 0, np.broadcast_to((deg == 0)[None, :, None], counts[s].shape))
    assert {1, 2} <= seen
    max_deg = max(int(np.bincount(v).max()) for v in var)
    assert (max(seen) > 2) == (max_deg > 2), (seen, max_deg)  # rsurf5: no qubit has more than two checks of one side
    # a selection that gives the whole gradient to one index would differ exactly on the shared entries
    shared = np.concatenate([(c > 1).ravel() for c in counts])
    assert shared.any()


@pytest.mark.parametrize("name,red", [("gb48", "max"), ("rsurf5", "min")])
def test_crafted_first_layers_keep_relu_units_half_a_unit_from_zero(name, red):
    cfg = (4, 6, 2, red, "relu", True)
    t = tie_case(name, cfg, 2, 11)
    args = (name, cfg, t["w"], t["llr"], t["lhx"], t["lhz"], t["sx"], t["sz"], t["gout"])
    r64, r32 = reference_pairs(*args, torch.float64), reference_pairs(*args, torch.float32)
    for li in (0, cfg[2]):
        pre = r64["pre"][li]
        assert np.abs(pre).min() >= 0.5 and (pre < 0).any() and (pre > 0).any()
        assert np.array_equal(pre, r32["pre"][li])  # half-integers: exact in both precisions
        assert (r64["deltas"][li][pre < 0] == 0).all()


@pytest.mark.parametrize("name,cfg", [("rsurf5", None), ("gb48", (8, 16, 1, "mean", "tanh", True)), ("rsurf5", (5, 7, 3, "sum", "relu", False)),
                                      ("gb48", (6, 10, 4, "min", "sigmoid", True)), ("steane", (1, 1, 1, "sum", "linear", False)),
                                      ("gb48", (4, 6, 2, "max", "relu", True))])
def test_pairs_reproduce_the_weight_gradients(name, cfg):
    """acts^T deltas and the column sums of the deltas are w.grad, in float64 to 1e-12 of each gradient's largest entry: the pairs are
    in the kernel's layer order, get_weights() lists _llr_inv_embed first."""
    from feedback_gnn_amd.graph import gnn_weight_shapes
    c, B = code(name), 2
    rng = np.random.RandomState(23)
    shapes = SHIPPED_SHAPES if cfg is None else gnn_weight_shapes(cfg[0], cfg[1], cfg[2], cfg[5])
    L, bias = (2, True) if cfg is None else (cfg[2], cfg[5])
    w = [rng.uniform(-0.5, 0.5, size=s) for s in shapes]
    llr = rng.uniform(-2, 6, size=(B, 3, c.hx.shape[1]))
    lhx, lhz = rng.uniform(-4, 4, size=(B, c.hx.shape[0])), rng.uniform(-4, 4, size=(B, c.hz.shape[0]))
    sx, sz = rng.randint(0, 2, size=(B, c.hx.shape[0])), rng.randint(0, 2, size=(B, c.hz.shape[0]))
    gout = rng.normal(size=(B, 3, c.hx.shape[1]))
    if cfg == (4, 6, 2, "max", "relu", True):  # with ties: any split among identical rows gives the same sums
        t = tie_case(name, cfg, B, 11)
        w, llr, lhx, lhz, sx, sz, gout = (t[k] for k in ("w", "llr", "lhx", "lhz", "sx", "sz", "gout"))
    ref = reference_pairs(name, cfg, w, llr, lhx, lhz, sx, sz, gout, torch.float64)
    st = 2 if bias else 1
    assert len(ref["wgrads"]) == 3 * L * st
    for f in range(3 * L):
        li = 3 * L - 1 if f == 0 else f - 1
        a, d, want = ref["acts"][li], ref["deltas"][li], ref["wgrads"][f * st]
        assert a.shape == (d.shape[0], want.shape[0]) and d.shape[1] == want.shape[1]
        assert np.abs(a.T @ d - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (f, li)
        if bias:
            assert np.abs(d.sum(0) - ref["wgrads"][f * st + 1]).max() <= 1e-12 * np.abs(ref["wgrads"][f * st + 1]).max(), (f, li)
    rows = [B * int(np.asarray(c.hx).sum())] * L + [B * int(np.asarray(c.hz).sum())] * L + [B * c.hx.shape[1]] * L
    assert [a.shape[0] for a in ref["acts"]] == rows
