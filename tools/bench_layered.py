"""Layered against flooding BP4 (fgnn_bp4_decode_layered / fgnn_bp4_decode) on [[882,24]] under depolarizing noise at p = 0.09, min-sum
and boxplus-phi at factor 0.8, the prior of p, the same seeded samples (the library's Philox stream) for every decoder.

    python tools/bench_layered.py [--out profiles/layered_bench.json]          (LAYERED_BENCH_B: batch size, default 16 384)

Per decoder — flooding-T and layered-T for T in 8, 16, 32, 64, the library's defaults (flooding with its exact shortcuts on, layered at
its default threads per codeword) — the time per batch by HIP events around REPS launches after a warm-up, the median of ROUNDS rounds
with the fastest and the slowest, and the samples whose decision does not reproduce its syndromes.  For the layered kernel also a sweep
of the threads per codeword (fgnn_graph_set_launch, one codeword per workgroup) at T = 16.  Writes one JSON object, prints it too."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402
from helpers import code  # noqa: E402

B = int(os.environ.get("LAYERED_BENCH_B", 16384))
P, FACTOR, SEED = 0.09, 0.8, 0x5EED
ITERS = (8, 16, 32, 64)
SWEEP_TPC, SWEEP_T = (64, 128, 192, 256, 384, 512), 16
REPS, ROUNDS = 3, 5


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def timed(fn):
    events(fn, 1)  # warm-up: code object load, clocks
    return spread([events(fn, REPS) for _ in range(ROUNDS)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layered needs a HIP device")
    g = TannerGraph(code("ghp882"), stage_one=False)
    g.set_layers()
    num_layers, lay = g.layers()
    ex, ez = g.pauli_noise(SEED, P, 0, B)
    sx, sz = g.syndrome(ex, ez)
    pf = np.float32(P)
    L = float(np.log(np.float32(3.0) * (np.float32(1.0) - pf) / pf, dtype=np.float32))

    def unsolved(out):
        _, _, flags = g.residual(ex, ez, out["x_hat"], out["z_hat"], want_arrays=False)
        return int((flags & 1).ne(0).sum().item())

    res = dict(code="ghp882 [[882,24]]", p=P, factor=FACTOR, B=B, device=torch.cuda.get_device_name(0), num_layers=num_layers,
               layer_sizes=np.bincount(lay).tolist(), launches_per_round=REPS, rounds=ROUNDS, decoders={}, sweep={})
    for cn in ("minsum", "boxplus-phi"):
        rows = {}
        for T in ITERS:
            for tag, fn in (("flooding", g.bp4_decode), ("layered", g.bp4_decode_layered)):
                run = lambda: fn(sx, sz, T, cn, FACTOR, llr_const=L, want_logits=False)  # noqa: E731
                rows[f"{tag}-{T}"] = dict(batch_ms=timed(run), unsolved=unsolved(run()))
        res["decoders"][cn] = rows
        sweep = {}
        for tpc in SWEEP_TPC:
            g.set_launch(tpc, 1)
            try:
                sweep[str(tpc)] = timed(lambda: g.bp4_decode_layered(sx, sz, SWEEP_T, cn, FACTOR, llr_const=L, want_logits=False))
            finally:
                g.set_launch(0, 0)
        res["sweep"][cn] = dict(iterations=SWEEP_T, threads_per_codeword=sweep)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
