"""OSD-0 vs OSD-CS vs OSD-E at the shape of examples/OSD.ipynb cell 6: [[882,24]], BP4 min-sum x 120, factor 0.8, 50 000 samples,
p = 0.09.  BP4 runs once; every method then re-solves both sides of the same BP failures.  Prints, per method and order, the OSD
time alone (median of --reps timed runs after one warm-up, both sides, device events) and the logical-error count of the batch.

    python tools/bench_osd_search.py [--samples 50000] [--p 0.09] [--reps 5]
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

import feedback_gnn_amd as F  # noqa: E402
from feedback_gnn_amd._lib import ROWS_LX, ROWS_LZ  # noqa: E402
from helpers import code  # noqa: E402

CONFIGS = [("osd0", 0), ("osd_cs", 7), ("osd_cs", 10), ("osd_cs", 20), ("osd_e", 4), ("osd_e", 8), ("osd_e", 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--p", type=float, default=0.09)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    c = code("ghp882")
    dec = F.QLDPCBPDecoder(code=c, num_iter=120, normalization_factor=0.8, cn_type="minsum", stage_one=True)
    model = F.BP4_OSD_Model(c, dec, F.OSD0_Decoder(c.N))  # installs the hx / hz bases, owns the seeded channel
    g, B = model.graph, args.samples
    ex, ez = model.channel(B, args.p, 0)
    sx, sz = g.syndrome(ex, ez)
    pf = np.float32(args.p)
    L = float(np.log(np.float32(3.0) * (np.float32(1.0) - pf) / pf, dtype=np.float32))
    out = g.bp4_decode(sx, sz, dec.num_iter, dec.cn_type, dec.normalization_factor, llr_const=L, want_logits=False)
    _, _, flags = g.residual(ex, ez, out["x_hat"], out["z_hat"], want_arrays=False)
    index, nact = g.compact(flags, 1)
    print(f"[[882,24]] BP4 min-sum x 120, factor 0.8, {B} samples, p = {args.p}: {nact} BP failures re-solved on both sides")
    rows = []
    for method, order in CONFIGS:
        x_hat, z_hat = out["x_hat"].clone(), out["z_hat"].clone()
        cz, cx = torch.zeros((2, B), dtype=torch.int32, device=g.device)

        def run():
            if method == "osd0":
                g.osd0(0, sx, z_hat, marg=out["llr"], index=index, nact=nact)
                g.osd0(1, sz, x_hat, marg=out["llr"], index=index, nact=nact)
            else:
                g.osd(0, sx, z_hat, method, order, marg=out["llr"], index=index, nact=nact, chosen=cz)
                g.osd(1, sz, x_hat, method, order, marg=out["llr"], index=index, nact=nact, chosen=cx)

        run()  # warm-up; the OSD output depends only on its inputs, so repeated runs rewrite the same bits
        times = []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        ls_hat, _ = g.residual_rows(ROWS_LZ, ROWS_LX, ex, ez, x_hat, z_hat)
        errs = int(ls_hat.any(1).sum())
        improved = int(((cz != 0) | (cx != 0)).sum())
        ms = float(np.median(times))
        label = "osd0" if method == "osd0" else f"{method} order {order}"
        print(f"  {label:16s} OSD {ms:8.2f} ms (both sides, {nact} samples)   logical errors {errs:4d}   improved on OSD-0 {improved:4d}")
        rows.append(dict(method=method, order=order, osd_ms=round(ms, 3), logical_errors=errs, improved=improved))
    print(json.dumps(dict(samples=B, p=args.p, failures=nact, results=rows)))


if __name__ == "__main__":
    main()
