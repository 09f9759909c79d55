"""BP4 with guided decimation (fgnn_bp4gd_decode) on [[882,24]] under depolarizing noise at p = 0.10, B = 16 384, the same seeded samples
(the library's Philox stream, samples 0..B-1) for every decoder.  Writes profiles/bp4gd_bench.json and prints it as one JSON line.
    python tools/bench_bp4gd.py

Timing: HIP events around 3 launches, 5 rounds after a warm-up; the median round is reported with the fastest and the slowest.

(a) What the decimation machinery costs when it is never used: max_rounds = 0 with pre_iter = 64 on syndromes no error produces (so no
    sample stops early), against one leg of fgnn_relay4_decode with gamma = 0 and 64 iterations on the same input; both min-sum at
    factor 0.8.  The Relay-BP4 kernel is the yardstick: same step structure, the memory term and the weight in place of the fix marks.
(b) Decoders on the same samples: the default BP4GDDecoder, round_iter 2 and 8, min-sum-64 flooding BP4 (factor 0.8), BP4_OSD_Model
    (min-sum-100 + OSD-0) and the default RelayBP4Decoder.  Per decoder: ms per batch from the seeded samples to the estimate (drawing
    the noise and its syndromes included, the same work for every decoder), the samples left without a solution (for BP4 + OSD: the
    samples BP4 hands to OSD; OSD-0 solves each of them), and the logical errors (a sample whose residual misses the syndrome or a
    logical operator) with their binomial standard error."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feedback_gnn_amd as F  # noqa: E402
from feedback_gnn_amd import gf2  # noqa: E402
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402
from helpers import code  # noqa: E402

B = int(os.environ.get("BP4GD_BENCH_B", 16384))
P = 0.10
ITERS, REPS, ROUNDS = 64, 3, 5
SEED = 0x5EED
OUT = os.path.join(ROOT, "profiles", "bp4gd_bench.json")


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


def llr_depolarizing(p):
    p = np.float32(p)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p) / p, dtype=np.float32))


def part_a(c):
    g = TannerGraph(c, stage_one=False)
    hx = np.asarray(c.hx, np.int64)
    left = np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has independent rows: every syndrome can be satisfied"
    u = left[0]
    sx, sz = g.syndrome(*g.pauli_noise(SEED, P, 0, B))
    sx = sx.cpu().numpy()
    sx[(sx.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    sx = torch.from_numpy(sx).to(g.device)
    L = llr_depolarizing(P)
    gamma = torch.zeros((1, g.n), dtype=torch.float32, device=g.device)
    out = {}

    def gd():
        out["gd"] = g.bp4gd_decode(sx, sz, ITERS, 4, 0, 25.0, "minsum", 0.8, llr_const=L)

    def relay4():
        out["relay4"] = g.relay4_decode(sx, sz, gamma, ITERS, ITERS, 1, 0.8, llr_const=L)

    for fn in (gd, relay4):
        events(fn, 2)
    for tag in ("gd", "relay4"):
        st = out[tag][2]
        assert int((st[:, 0] != 0).sum()) == 0 and int((st[:, 3] != ITERS).sum()) == 0, "no sample may stop early"
    same = bool(torch.equal(out["gd"][0], out["relay4"][0]) and torch.equal(out["gd"][1], out["relay4"][1]))
    t_gd, t_relay4 = [], []
    for _ in range(ROUNDS):
        t_gd.append(events(gd, REPS))
        t_relay4.append(events(relay4, REPS))
    a, b = spread(t_gd), spread(t_relay4)
    return dict(iterations=ITERS, bp4gd_no_rounds_ms=a, relay4_one_leg_gamma0_ms=b, ratio=round(a["median"] / b["median"], 3),
                estimates_identical=same, launches_per_round=REPS, rounds=ROUNDS)


def rate(k, n):
    r = k / n
    return dict(errors=int(k), samples=int(n), rate=r, stderr=float(np.sqrt(r * (1 - r) / n)))


def part_b(c):
    g = TannerGraph(c, stage_one=False)
    L = llr_depolarizing(P)

    def gd_run(**kw):
        dec = F.BP4GDDecoder(c, graph=g, **kw)
        model = F.BP4_GD_Model(c, dec, seed=SEED)

        def run():
            model._next = 0
            model(B, P)
            return model.last_x_hat, model.last_z_hat, model.last_num_unsolved
        cfg = dict(pre_iter=dec.pre_iter, round_iter=dec.round_iter, max_rounds=dec.max_rounds, decim_llr=dec.decim_llr,
                   cn_type=dec.cn_type, normalization_factor=dec.normalization_factor)
        return run, cfg, model

    relay_dec = F.RelayBP4Decoder(c, graph=g)
    relay = F.BP4_Relay_Model(c, relay_dec, seed=SEED)
    bp4 = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    osd = F.BP4_OSD_Model(c, bp4, F.OSD0_Decoder(c.N), seed=SEED)

    def run_relay():
        relay._next = 0
        relay(B, P)
        return relay.last_x_hat, relay.last_z_hat, relay.last_num_unsolved

    def run_flooding():
        ex, ez = g.pauli_noise(SEED, P, 0, B)
        sx, sz = g.syndrome(ex, ez)
        o = g.bp4_decode(sx, sz, ITERS, "minsum", 0.8, llr_const=L, want_logits=False)
        s_hat, _, _ = g.residual(ex, ez, o["x_hat"], o["z_hat"], want_arrays=True)
        return o["x_hat"], o["z_hat"], int(s_hat.any(1).sum().item())

    def run_osd():
        osd._next = 0
        o = osd.decode(B, P)
        return o["x_hat"], o["z_hat"], osd.last_num_osd

    gd_default, cfg_default, m_default = gd_run()
    gd_r2, cfg_r2, _ = gd_run(round_iter=2)
    gd_r8, cfg_r8, _ = gd_run(round_iter=8)
    runs = (("bp4gd_default", gd_default, cfg_default), ("bp4gd_round_iter_2", gd_r2, cfg_r2), ("bp4gd_round_iter_8", gd_r8, cfg_r8),
            ("bp4_minsum_64_flooding", run_flooding, dict(cn_type="minsum", num_iter=ITERS, normalization_factor=0.8)),
            ("bp4_osd0", run_osd, dict(cn_type="minsum", num_iter=100, normalization_factor=0.8, osd="osd0")),
            ("relay4_default", run_relay, dict(gamma0=relay_dec.gamma0, pre_iter=relay_dec.pre_iter, num_sets=relay_dec.num_sets,
                                               set_max_iter=relay_dec.set_max_iter, gamma_dist_interval=relay_dec.gamma_dist_interval,
                                               stop_nconv=relay_dec.stop_nconv, normalization_factor=relay_dec.normalization_factor)))
    ex, ez = g.pauli_noise(SEED, P, 0, B)  # the samples every decoder draws
    res = {}
    for tag, fn, cfg in runs:
        x_hat, z_hat, uns = fn()  # warm-up, and the figures
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)
        key = "bp_unsolved" if tag == "bp4_osd0" else "unsolved"
        res[tag] = {"config": cfg, key: int(uns), "logical": rate(int((flags != 0).sum().item()), B)}
        if tag == "bp4gd_default":
            st = m_default.last_stats
            res[tag]["max_fixed"], res[tag]["max_iterations"] = int(st[:, 1].max().item()), int(st[:, 2].max().item())
            res[tag]["mean_iterations"] = float(st[:, 2].float().mean().item())
        torch.cuda.synchronize()
    t = {tag: [] for tag, _, _ in runs}
    for _ in range(ROUNDS):
        for tag, fn, _ in runs:
            t[tag].append(events(fn, REPS))
    for tag, _, _ in runs:
        res[tag]["batch_ms"] = spread(t[tag])
    res["launches_per_round"], res["rounds"] = REPS, ROUNDS
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_bp4gd needs a HIP device")
    c = code("ghp882")
    parts = os.environ.get("BP4GD_BENCH_PARTS", "ab")
    out = dict(code="ghp882 [[882,24]]", p=P, B=B, seed=SEED, device=torch.cuda.get_device_name(0))
    if "a" in parts:
        out["a"] = part_a(c)
    if "b" in parts:
        out["b"] = part_b(c)
    line = json.dumps(out)
    if parts == "ab" and B == 16384:
        with open(OUT, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
