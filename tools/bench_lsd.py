"""BP+LSD against BP+OSD-0 on the same failures and marginals.  (a, b) [[882,24]] under min-sum-100 at factor 0.8, 50 000 samples at
p = 0.09, 0.05 and 0.02: fgnn_lsd (both sides) against fgnn_osd0 (both sides): ms per batch of failures, samples with found = 0,
logical errors of BP+LSD with and without the OSD-0 fallback against BP+OSD-0, the distribution of pivots and rounds.  (c) the
[[6480,1296]] hypergraph product (tests/helpers.py hp_big): the first 100 failures of a BP4 batch, both sides, against fgnn_osd_ws.
Timing: HIP events around 3 launches, the variants alternating inside each of 5 rounds, the median round.  Writes one JSON document.

    python tools/bench_lsd.py [--out profiles/lsd_bench.json] [--batch 50000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import code, llr_const  # noqa: E402

from feedback_gnn_amd._lib import ROWS_LX, ROWS_LZ  # noqa: E402
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402

ROUNDS, LAUNCHES = 5, 3


def timed(variants):
    """{name: median over ROUNDS of (ms per launch over LAUNCHES launches)}, the variants taking turns inside every round."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / LAUNCHES)
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def dist(x):
    x = np.asarray(x)
    if not len(x):
        return None
    return dict(min=int(x.min()), median=float(np.median(x)), mean=round(float(x.mean()), 2), p90=float(np.percentile(x, 90)),
                p99=float(np.percentile(x, 99)), max=int(x.max()))


def failures(g, B, p, num_iter):
    ex, ez = g.pauli_noise(0x5EED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    o = g.bp4_decode(sx, sz, num_iter, "minsum", 0.8, llr_const=llr_const(p), want_logits=False)
    _, _, flags = g.residual(ex, ez, o["x_hat"], o["z_hat"], want_arrays=False)
    index, nact = g.compact(flags, 1)
    return ex, ez, sx, sz, o, index, nact


def wrong(g, ex, ez, xh, zh):
    """Samples whose estimate misses a syndrome or flips a logical operator."""
    ls_hat, _ = g.residual_rows(ROWS_LZ, ROWS_LX, ex, ez, xh, zh)
    _, _, flags = g.residual(ex, ez, xh, zh, want_arrays=False)
    return int((((flags & 1) != 0) | (ls_hat != 0).any(1)).sum())


def fresh_stats(g, B):
    st = torch.zeros((2, B, 4), dtype=torch.int32, device=g.device)
    st[:, :, 0] = 1
    return st


def point_882(g, B, p):
    ex, ez, sx, sz, o, index, nact = failures(g, B, p, 100)
    marg = o["llr"]
    res = dict(p=p, batch=B, bp_failures=nact, bp_wrong=wrong(g, ex, ez, o["x_hat"], o["z_hat"]))
    if not nact:
        return res
    kw = dict(marg=marg, index=index, nact=nact)
    zl, xl, zo, xo = o["z_hat"].clone(), o["x_hat"].clone(), o["z_hat"].clone(), o["x_hat"].clone()
    st = fresh_stats(g, B)

    def lsd():
        g.lsd(0, sx, zl, stats=st[0], **kw)
        g.lsd(1, sz, xl, stats=st[1], **kw)

    def osd0():
        g.osd0(0, sx, zo, **kw)
        g.osd0(1, sz, xo, **kw)

    res["ms_per_batch_both_sides"] = timed(dict(lsd=lsd, osd0=osd0))
    res["lsd_over_osd0"] = round(res["ms_per_batch_both_sides"]["lsd"] / res["ms_per_batch_both_sides"]["osd0"], 3)
    s = st.cpu().numpy()
    fail = index[:nact].cpu().numpy()
    missed = (s[:, fail, 0] == 0).any(0)
    res["lsd_found0_samples"] = int(missed.sum())
    res["lsd_found0_per_side"] = [int((s[k, fail, 0] == 0).sum()) for k in (0, 1)]
    res["pivots"] = [dist(s[k, fail, 3]) for k in (0, 1)]
    res["rounds"] = [dist(s[k, fail, 1]) for k in (0, 1)]
    res["columns"] = [dist(s[k, fail, 2]) for k in (0, 1)]
    res["wrong_bp_lsd_no_fallback"] = wrong(g, ex, ez, xl, zl)
    res["wrong_bp_osd0"] = wrong(g, ex, ez, xo, zo)
    if missed.any():  # the fallback: OSD-0 on the samples LSD gave up
        idx2 = torch.from_numpy(fail[missed].astype(np.int32)).to(g.device)
        g.osd0(0, sx, zl, marg=marg, index=idx2, nact=len(idx2))
        g.osd0(1, sz, xl, marg=marg, index=idx2, nact=len(idx2))
    res["wrong_bp_lsd_with_fallback"] = wrong(g, ex, ez, xl, zl)
    return res


def point_big(g, B, p, take=100):
    ex, ez, sx, sz, o, index, nact = failures(g, B, p, 10)
    res = dict(p=p, batch=B, bp="minsum x10, factor 0.8 (GMEM kernel)", bp_failures=nact, timed_failures=min(take, nact))
    nact = min(take, nact)
    if not nact:
        return res
    kw = dict(marg=o["llr"], index=index, nact=nact)
    synd = (sx, sz)
    st = fresh_stats(g, B)
    for side in (0, 1):
        ws = g.osd_workspace(side, "osd0", 0)
        el, eo = (o["z_hat" if side == 0 else "x_hat"].clone() for _ in range(2))
        ms = timed(dict(lsd=lambda: g.lsd(side, synd[side], el, stats=st[side], **kw),
                        osd_ws=lambda: g.osd_ws(side, synd[side], eo, "osd0", 0, workspace=ws, **kw)))
        s = st[side].cpu().numpy()[index[:nact].cpu().numpy()]
        res[f"side{side}"] = dict(ms=ms, lsd_over_osd_ws=round(ms["lsd"] / ms["osd_ws"], 3), lsd_found0=int((s[:, 0] == 0).sum()),
                                  pivots=dist(s[:, 3]), rounds=dist(s[:, 1]), max_pivots=g.lsd_max_pivots(side))
        del ws
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsd_bench.json"))
    ap.add_argument("--batch", type=int, default=50000)
    args = ap.parse_args()
    res = dict(tool="tools/bench_lsd.py", method=f"HIP events, median of {ROUNDS} rounds of {LAUNCHES} launches, variants alternating",
               device=torch.cuda.get_device_name(0))
    c = code("ghp882")
    g = TannerGraph(c)
    g.set_basis(0, c.pivot_hx)
    g.set_basis(1, c.pivot_hz)
    res["ghp882"] = dict(code="[[882,24]]", bp="minsum x100, factor 0.8", max_pivots=[g.lsd_max_pivots(0), g.lsd_max_pivots(1)],
                         points=[point_882(g, args.batch, p) for p in (0.09, 0.05, 0.02)])
    del g
    torch.cuda.empty_cache()
    c = code("hp_big")
    g = TannerGraph(c)
    g.set_basis(0, c.pivot_hx)
    g.set_basis(1, c.pivot_hz)
    res["hp_big"] = dict(code="[[6480,1296]]", points=[point_big(g, 256, 0.03), point_big(g, 2048, 0.01)])
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
