"""Layered against flooding binary BP (fgnn_bp2_decode_layered / fgnn_bp2_decode) on the hx graph of [[882,24]] over a BSC, in the
setting of tools/bench_relay.py: p = 0.07 * 2 / 3, B = 10 000, min-sum at factor 0.8 with the prior of p, the same seeded samples for
every decoder.  For an MI355X.  Writes profiles/bp2_layered_bench.json and prints it.   python tools/bench_bp2_layered.py

The driver runs every step as a child process of its own under `timeout`, one after the other; a step that fails, faults or runs
out of time ends the run and nothing is written.  Steps:
  solve   time per batch and unsolved samples of flooding at 100 iterations and of layered at 8, 16, 32 and 100, stop off
  stop    the same layered runs with stop on, and the iterations they ran
  ratio   the cost of one layered iteration relative to one flooding iteration, both at fixed dataflow (no stop, no exit: neither
          kernel's work depends on the data): the slope between 32 and 100 iterations of either, which leaves the launch out
  sweep   threads per codeword 64 .. 512 through fgnn_graph_set_launch (one codeword per workgroup) at 16 iterations: the value the
          default cap FGNN_BP2L_TPC is taken from
Times are HIP events around REPS launches, ROUNDS rounds after a warm-up; the median round is reported with the fastest and slowest."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "bp2_layered_bench.json")
STEPS = (("solve", 240), ("stop", 240), ("ratio", 240), ("sweep", 240))  # name, seconds
B = int(os.environ.get("BP2L_BENCH_B", 10000))
P = 0.07 * 2 / 3
FACTOR = 0.8
LAYERED_ITERS = (8, 16, 32, 100)
SWEEP_TPC = (64, 128, 192, 256, 384, 512)
REPS, ROUNDS = 5, 9


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def step(name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from feedback_gnn_amd.graph import TannerGraph
    from helpers import code

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / REPS

    def timed(fn):
        events(fn)
        return spread([events(fn) for _ in range(ROUNDS)])

    c = code("ghp882")
    g = TannerGraph(c)
    synd = g.syndrome(torch.zeros((B, g.n), dtype=torch.uint8, device=g.device), g.bsc_noise(0x5EED, P, 0, B))[0]
    L = float(-np.log((np.float32(1.0) - np.float32(P)) / np.float32(P), dtype=np.float32))

    def unsolved(hard):
        return int((g.syndrome(torch.zeros_like(hard), hard)[0] != synd).any(1).sum())

    def flooding(T):
        return g.bp2_decode(synd, T, "minsum", FACTOR, llr_const=L, want_soft=False)[1]

    def layered(T, stop=False):
        return g.bp2_decode_layered(synd, T, "minsum", FACTOR, llr_const=L, want_soft=False, stop=stop, want_stats=stop)

    g.set_bit_layers()
    num, lay = g.bit_layers()
    out = dict(layers=num, layer_sizes=[int(x) for x in np.bincount(lay)])
    if name == "solve":
        out["flooding_100"] = dict(ms=timed(lambda: flooding(100)), unsolved=unsolved(flooding(100)))
        for T in LAYERED_ITERS:
            out[f"layered_{T}"] = dict(ms=timed(lambda: layered(T)), unsolved=unsolved(layered(T)[1]))
    elif name == "stop":
        for T in LAYERED_ITERS:
            _, hard, stats = layered(T, True)
            st = stats.cpu().numpy()
            assert unsolved(hard) == int((st[:, 0] == 0).sum())
            out[f"layered_{T}"] = dict(ms=timed(lambda: layered(T, True)), unsolved=int((st[:, 0] == 0).sum()),
                                       mean_iterations=round(float(st[:, 1].mean()), 3), max_iterations=int(st[:, 1].max()))
    elif name == "ratio":
        t = {k: {T: timed(lambda: fn(T)) for T in (32, 100)} for k, fn in (("flooding", flooding), ("layered", layered))}
        per = {k: (v[100]["median"] - v[32]["median"]) / 68 for k, v in t.items()}
        out.update(ms=t, ms_per_iteration={k: round(v, 5) for k, v in per.items()}, layered_over_flooding=round(per["layered"] / per["flooding"], 3))
    elif name == "sweep":
        res = {}
        for tpc in SWEEP_TPC:
            g.set_launch(tpc, 1)
            res[str(tpc)] = timed(lambda: layered(16))
        g.set_launch(0, 0)
        res["default"] = timed(lambda: layered(16))
        out.update(iterations=16, ms=res)
    else:
        raise SystemExit(f"unknown step {name}")
    print(json.dumps({name: out, "device": torch.cuda.get_device_name(0)}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    result = dict(code="ghp882 hx [[882,24]]", p=P, B=B, cn_type="minsum", factor=FACTOR, launches_per_round=REPS, rounds=ROUNDS)
    for name, seconds in STEPS:
        res = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name],
                             stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            raise SystemExit(f"step {name} ended with status {res.returncode}: the run stops here and nothing is written")
        result.update(json.loads(res.stdout.strip().splitlines()[-1]))
    text = json.dumps(result, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
