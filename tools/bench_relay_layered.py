"""Relay-BP with layered legs against flooding legs (fgnn_relay_decode_layered / fgnn_relay_decode) on the hx graph of [[882,24]] over a
BSC, in the setting of tools/bench_relay.py: p = 0.07 * 2 / 3, B = 10 000, factor 1.0 with the prior of p, the default gammas of
RelayBPDecoder (gamma0 = 0.125, seed 0), the same seeded samples for every decoder.  For an MI355X.  Writes
profiles/relay_layered_bench.json (RELAYL_BENCH_OUT names another file) and prints it.   python tools/bench_relay_layered.py

The driver runs every step as a child process of its own under `timeout`, one after the other; a step that fails, faults or runs
out of time ends the run and nothing is written.  Steps:
  default  time per batch, unsolved samples and iterations of flooding and layered Relay-BP at the default schedule (80, 60 x 60)
  short    the same for the schedules (16, 10 x 12) and (24, 8 x 16), layered and, for comparison, flooding
  one_leg  one leg of 64 iterations at gamma = 0 on syndromes no error produces (no sample stops, the work is fixed) against
           fgnn_bp2_decode_layered with 64 min-sum iterations, without and with its parity sweep (stop): what the memory term, the
           re-sum and the leg control cost
  sweep    threads per codeword 64 / 128 / 192 / 256 through fgnn_graph_set_launch (one codeword per workgroup), at the default
           schedule and on the fixed work of one_leg: the value the default cap FGNN_RELAYL_TPC is checked against
Times are HIP events around REPS launches, ROUNDS rounds after a warm-up; the median round is reported with the fastest and slowest."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("RELAYL_BENCH_OUT", os.path.join(ROOT, "profiles", "relay_layered_bench.json"))
STEPS = (("default", 240), ("short", 240), ("one_leg", 240), ("sweep", 240))  # name, seconds
B = int(os.environ.get("RELAYL_BENCH_B", 10000))
P = 0.07 * 2 / 3
FACTOR = 1.0
SHORT = ((16, 10, 12), (24, 8, 16))  # pre_iter, num_sets, set_max_iter
ONE_LEG_ITERS = 64
SWEEP_TPC = (64, 128, 192, 256)
REPS, ROUNDS = 5, 9


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def step(name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feedback_gnn_amd as F
    from feedback_gnn_amd import gf2
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
    g.set_bit_layers()
    hx = np.asarray(c.hx, np.int64)
    synd = g.syndrome(torch.zeros((B, g.n), dtype=torch.uint8, device=g.device), g.bsc_noise(0x5EED, P, 0, B))[0]
    L = float(-np.log((np.float32(1.0) - np.float32(P)) / np.float32(P), dtype=np.float32))

    def relay(schedule, pre, sets, it):
        """(time, unsolved, iterations up to the output: mean and max) of one RelayBPDecoder on the shared graph."""
        d = F.RelayBPDecoder(c.hx, pre_iter=pre, num_sets=sets, set_max_iter=it, normalization_factor=FACTOR, graph=g, schedule=schedule)
        hard, stats = d.decode(synd, llr_const=L)
        st = stats.cpu().numpy()
        solved = st[:, 0] > 0
        assert int((g.syndrome(torch.zeros_like(hard), hard)[0] != synd).any(1).sum()) == int((~solved).sum())
        its = np.where(st[:, 2] == 0, st[:, 3], pre + (st[:, 2] - 1) * it + st[:, 3])
        return dict(ms=timed(lambda: d.decode(synd, llr_const=L)), unsolved=int((~solved).sum()),
                    mean_iterations=round(float(its.mean()), 3), max_iterations=int(its.max()))

    def unsolvable():
        """The syndromes moved outside the column space of hx: no test passes, every sample runs every iteration."""
        left = np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2
        assert left.shape[0] >= 1, "hx has independent rows: every syndrome can be satisfied"
        u = left[0]
        s = synd.cpu().numpy()
        s[(s.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1
        return torch.from_numpy(s).to(g.device)

    def one_leg(bad, gamma):
        stats = g.relay_decode_layered(bad, gamma, ONE_LEG_ITERS, ONE_LEG_ITERS, 1, FACTOR, llr_const=L)[1]
        assert int((stats[:, 0] != 0).sum()) == 0 and int((stats[:, 3] != ONE_LEG_ITERS).sum()) == 0
        return timed(lambda: g.relay_decode_layered(bad, gamma, ONE_LEG_ITERS, ONE_LEG_ITERS, 1, FACTOR, llr_const=L))

    num, lay = g.bit_layers()
    out = dict(layers=num, layer_sizes=[int(x) for x in np.bincount(lay)])
    if name == "default":
        out["schedule"] = [80, 60, 60]
        out["flooding"] = relay("flooding", 80, 60, 60)
        out["layered"] = relay("layered", 80, 60, 60)
    elif name == "short":
        for pre, sets, it in SHORT:
            out[f"{pre}_{sets}x{it}"] = dict(layered=relay("layered", pre, sets, it), flooding=relay("flooding", pre, sets, it))
    elif name == "one_leg":
        bad = unsolvable()
        gamma = torch.zeros((1, g.n), dtype=torch.float32, device=g.device)
        t_relay = one_leg(bad, gamma)
        t_plain = timed(lambda: g.bp2_decode_layered(bad, ONE_LEG_ITERS, "minsum", FACTOR, llr_const=L, want_soft=False))
        t_stop = timed(lambda: g.bp2_decode_layered(bad, ONE_LEG_ITERS, "minsum", FACTOR, llr_const=L, want_soft=False, stop=True))
        out.update(iterations=ONE_LEG_ITERS, relay_layered_one_leg_ms=t_relay, bp2_layered_ms=t_plain, bp2_layered_stop_ms=t_stop,
                   over_bp2_layered=round(t_relay["median"] / t_plain["median"], 3),
                   over_bp2_layered_stop=round(t_relay["median"] / t_stop["median"], 3))
    elif name == "sweep":
        bad = unsolvable()
        gamma = torch.zeros((1, g.n), dtype=torch.float32, device=g.device)
        d = F.RelayBPDecoder(c.hx, normalization_factor=FACTOR, graph=g, schedule="layered")
        res = {}
        for tpc in SWEEP_TPC + (0,):
            g.set_launch(tpc, 1 if tpc else 0)
            res["default" if tpc == 0 else str(tpc)] = dict(default_schedule_ms=timed(lambda: d.decode(synd, llr_const=L)),
                                                            one_leg_ms=one_leg(bad, gamma))
        out.update(one_leg_iterations=ONE_LEG_ITERS, ms=res)
    else:
        raise SystemExit(f"unknown step {name}")
    print(json.dumps({name: out, "device": torch.cuda.get_device_name(0)}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    result = dict(code="ghp882 hx [[882,24]]", p=P, B=B, cn_type="minsum", factor=FACTOR, gamma0=0.125, gamma_seed=0,
                  launches_per_round=REPS, rounds=ROUNDS)
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
