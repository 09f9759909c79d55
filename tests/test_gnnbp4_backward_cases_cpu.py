"""The cases of tests/test_gpu_gnnbp4_backward_elementwise.py screened without a GPU (tests/gnnbp4_backward_cases.py): every case has a
yardstick (float32 autograd of the restatement differs from float64 on every array) and a gradient to check (no array is all zero),
float32 decides no soft syndrome's sign differently, the restated launch plan puts the cases on the workgroup sizes they are meant
for, and the draw of the clip test has the rows it needs, away from the clip edge."""
import numpy as np
import pytest
import torch

import gnnbp4_backward_cases as G
import gnnbp4_reference as R
from helpers import code


def _same_signs(r64, r32):
    """Sign bits, not np.sign: where the outer phi saturates, float64 gives +-1.19e-7 (phi at PHI_MAX) and float32's
    softplus - log expm1 gives +-0."""
    for a, b in ((r64.xs, r32.xs), (r64.zs, r32.zs)):
        a, b = a.detach().numpy(), b.detach().numpy()
        if not np.array_equal(np.signbit(a), np.signbit(b)):
            return False
    return True


@pytest.mark.parametrize("key", list(G.CASES))
def test_every_case_has_a_yardstick_and_a_gradient(key):
    c = G.CASES[key]
    r64, r32, (l64, g64), (l32, g32) = G.case_refs(key)
    assert len(g64) == len(g32) == (7 * c.cfg[2] + 1) * (2 if c.cfg[5] else 1)
    assert _same_signs(r64, r32)
    assert abs(l32 - l64) <= 2e-4 * abs(l64)
    worst = 0.0
    for i, (a, b) in enumerate(zip(g32, g64)):
        e32, scale = np.abs(a - b).max(), np.abs(b).max()
        assert e32 > 0 and scale > 0 and np.isfinite(a).all(), (key, i)
        worst = max(worst, e32 / scale)
    print(f"{key}: worst e32 / max|r64| = {worst:.2e}")
    assert worst <= 1e-3  # the screening of tests/test_gpu_gnnbp4_backward.py
    if c.four_x:
        assert G.K * worst <= 5e-4, (key, worst)  # K e32 leaves the bound four times tighter than 2e-3


def test_the_plan_puts_the_cases_on_every_workgroup_size():
    for key, threads in G.PLAN_THREADS.items():
        c = G.CASES[key]
        assert G.plan_threads(c.name, c.cfg, c.fx)[0] == threads, key
        n = np.asarray(code(c.name).hx).shape[1]
        assert n > threads and n % threads, "more than one chunk and a ragged tail"
    for key in ("wg128_ghp1270", "wg64_bb2730"):  # the checks of a side too
        mx = np.asarray(code(G.CASES[key].name).hx).shape[0]
        assert mx > G.PLAN_THREADS[key] and mx % G.PLAN_THREADS[key]
    assert G.plan_threads("gb48", G.CASES["gb48_limits_lf0"].cfg)[0] == 128  # one trip with idle threads: n = 48
    # bb2730 misses the 128-thread layout by 640 bytes
    c = code("bb2730")
    assert np.asarray(c.hx).shape == (1365, 2730) and not np.asarray(c.lx).any() and not np.asarray(c.lz).any()
    D, H = G.WIDE[:2]
    misc = (4 * 2730 + 2 * 2730 + 2 + 3) & ~3
    assert (misc + ((3 * D * 129 + 3) & ~3) + 128 * H) * 4 == G.LDS_BUDGET + 640
    # the FX cases run below a wave (gb48, rsurf5), on an irregular code (rsurf5) and on 98 = 64 + 34 qubits (hp_c7, which is
    # (3, 6)-regular like every product of circulants)
    for name, small, irregular in (("rsurf5", True, True), ("gb48", True, False), ("hp_c7", False, False)):
        hx, hz = np.asarray(code(name).hx), np.asarray(code(name).hz)
        assert (hx.shape[1] < 64) == small
        degs = set(hx.sum(1).tolist()) | set(hz.sum(1).tolist())
        assert (len(degs) > 1 or len(set(hx.sum(0).tolist())) > 1) == irregular, (name, degs)
    assert 2 in set(np.asarray(code("rsurf5").hx).sum(1).tolist())  # degree-2 checks under mean reduction


def test_hp_big_fits_at_one_width_and_is_refused_at_the_next():
    fits = G.CASES["hp_big_fits"]
    assert G.plan_threads("hp_big", fits.cfg) == (64, 159664)
    assert G.plan_threads("hp_big", G.HP_BIG_REFUSED) == (0, 163808) and 163808 > G.LDS_BUDGET == 163584
    c = code("hp_big")
    assert np.asarray(c.hx).shape[1] == 6480 and np.asarray(c.hx).shape[0] + np.asarray(c.hz).shape[0] == 5184
    assert np.asarray(c.lx).shape[0] == np.asarray(c.lz).shape[0] == 1296
    # the tape forward is refused on 2 n + m floats: wide65535, which the reverse pass would refuse as well
    assert G.tape_forward_lds_bytes("wide65535") > G.LDS_BUDGET >= G.tape_forward_lds_bytes("hp_big")


def test_one_hot_upstreams_have_a_gradient_and_a_yardstick():
    name, cfg, B, T, inv = G.ONE_HOT
    assert G.plan_threads(name, cfg)[0] > 0 and tuple(cfg) != G.SURVEY
    r64, r32 = G.refs(name, cfg, B, T, inv)
    assert _same_signs(r64, r32)
    pts = G.one_hot_points(name, T, B)
    assert len(pts) == 2 * 2 * 2 * 4 and len(set(pts)) == len(pts)
    worst = 0.0
    for pt in pts:
        gx, gz = G.one_hot(name, T, B, *pt)
        assert (gx != 0).sum() + (gz != 0).sum() == 1
        for i, (a, b) in enumerate(zip(r32.grad(gx, gz), r64.grad(gx, gz))):
            e32, scale = np.abs(a - b).max(), np.abs(b).max()
            assert e32 > 0 and scale > 0, (pt, i)
            worst = max(worst, e32 / scale)
    print(f"one-hot: worst e32 / max|r64| = {worst:.2e}")
    assert G.K * worst <= 2e-3  # K e32 is the binding half of min(K e32, 2e-3 max|r64|) on every array


def test_the_clip_draw_has_dead_and_live_rows_away_from_the_edge():
    cc = G.clip_case()
    r64, r32 = cc["refs"]
    print("clipped share per side", cc["frac"], "margin", cc["margin"], "live", cc["live"], cc["live_rel"], "dead", cc["dead"])
    assert all(0.5 < f < 1.0 for f in cc["frac"])
    assert sorted(s for s, _ in cc["dead"]) == [0, 1] and cc["live"] is not None
    assert cc["margin"] > 1e-3
    B = G.CLIP["B"]
    for side, row in cc["dead"]:
        gx, gz = G.one_hot(G.CLIP["name"], 1, B, side, 0, 0, row)
        for r in (r64, r32):
            assert all((a == 0).all() for a in r.grad(gx, gz))
    gx, gz = G.one_hot(G.CLIP["name"], 1, B, *cc["live"][:1], 0, 0, cc["live"][1])
    assert all(np.abs(a).max() > 0 for a in r64.grad(gx, gz))
    assert cc["live_rel"] <= 5e-4  # float32 arithmetic reaches 2e-3 on this row with a factor 4 to spare


def test_record_leaves_the_forward_as_it_was():
    name, cfg = "rsurf5", G.SURVEY
    _, _, sx, sz = G.batch(name, 2)
    w = [torch.from_numpy(a).double() for a in G.weights(name, cfg)]
    tg = R.Graph(code(name))
    plain = R.forward(tg, G.num(cfg), w, torch.from_numpy(sx), torch.from_numpy(sz), 2)
    rec = {}
    with_rec = R.forward(tg, G.num(cfg), w, torch.from_numpy(sx), torch.from_numpy(sz), 2, record=rec)
    for a, b in zip(plain[0] + plain[1] + [plain[2]], with_rec[0] + with_rec[1] + [with_rec[2]]):
        assert torch.equal(a, b)
    n, m = tg.n, tg.sides[0]["m"] + tg.sides[1]["m"]
    assert [tuple(t.shape) for t in rec["h_vn"]] == [(2, n, 20)] * 2 and [tuple(t.shape) for t in rec["h_cn"]] == [(2, m, 20)] * 2
    assert [tuple(t.shape) for t in rec["hlog"]] == [(2, m)] * 2
    mx = tg.sides[0]["m"]
    assert torch.equal(rec["hlog"][1][:, :mx], with_rec[1][1][:, :mx]) and torch.equal(rec["hlog"][1][:, mx:], with_rec[0][1][:, :m - mx])
