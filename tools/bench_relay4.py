"""Relay-BP4 (fgnn_relay4_decode) on [[882,24]] under depolarizing noise at p = 0.07 (per-side marginal 2p/3 = the BSC rate of
profiles/relay_bench.json), B = 10 000.  Prints one JSON line.   python tools/bench_relay4.py

(a) What the memory term, the decisions and the parity tests cost per iteration: one leg of 64 iterations on syndromes no error
    produces (so no sample stops early), against fgnn_bp4_decode min-sum with 64 iterations on the fixed dataflow (saturation shortcut
    off) on the same input.  HIP events around REPS launches, the two kernels alternating, ROUNDS rounds after a warm-up; the median
    round is reported with the fastest and the slowest.
(b) Three decoders on the same seeded samples (the library's Philox stream, BATCHES batches of B): the default RelayBP4Decoder; the
    default binary RelayBPDecoder on each side by itself (hx with the z part of the noise, hz with the x part, BSC prior 2p/3), a
    sample counting as solved when both sides are; BP4 min-sum-100 (factor 0.8) + OSD-0 through BP4_OSD_Model.  Per decoder: host
    time per batch around a device synchronise, the samples left without a solution (for BP4 + OSD: the samples BP4 hands to OSD;
    OSD-0 solves each of them), and the logical errors (a sample whose residual misses the syndrome or a logical operator) with their
    binomial standard error."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import feedback_gnn_amd as F  # noqa: E402
from feedback_gnn_amd import gf2  # noqa: E402
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402
from helpers import code  # noqa: E402

B = int(os.environ.get("RELAY4_BENCH_B", 10000))
P = 0.07
ITERS, REPS, ROUNDS = 64, 10, 15
BATCHES = int(os.environ.get("RELAY4_BENCH_BATCHES", 10))
SEED = 0x5EED


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
    g.set_saturation_shortcut(False)  # the fixed dataflow
    hx = np.asarray(c.hx, np.int64)
    left = np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has independent rows: every syndrome can be satisfied"
    u = left[0]
    sx, sz = g.syndrome(*g.pauli_noise(SEED, P, 0, B))
    sx = sx.cpu().numpy()
    sx[(sx.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    sx = torch.from_numpy(sx).to(g.device)
    L = llr_depolarizing(P)
    gamma = torch.full((1, g.n), 0.125, dtype=torch.float32, device=g.device)
    out = {}

    def bp4():
        g.bp4_decode(sx, sz, ITERS, "minsum", 1.0, llr_const=L, want_logits=False)

    def relay4():
        out["stats"] = g.relay4_decode(sx, sz, gamma, ITERS, ITERS, 1, 1.0, llr_const=L)[2]

    for fn in (bp4, relay4):
        events(fn, 3)
    assert int((out["stats"][:, 0] != 0).sum()) == 0 and int((out["stats"][:, 3] != ITERS).sum()) == 0
    t_bp4, t_relay4 = [], []
    for _ in range(ROUNDS):
        t_bp4.append(events(bp4, REPS))
        t_relay4.append(events(relay4, REPS))
    a, b = spread(t_bp4), spread(t_relay4)
    return dict(iterations=ITERS, bp4_minsum_fixed_dataflow_ms=a, relay4_one_leg_ms=b, ratio=round(b["median"] / a["median"], 3),
                launches_per_round=REPS, rounds=ROUNDS)


def rate(k, n):
    r = k / n
    return dict(errors=int(k), samples=int(n), rate=r, stderr=float(np.sqrt(r * (1 - r) / n)))


def relay_config(d):
    return dict(gamma0=d.gamma0, pre_iter=d.pre_iter, num_sets=d.num_sets, set_max_iter=d.set_max_iter,
                gamma_dist_interval=d.gamma_dist_interval, stop_nconv=d.stop_nconv, normalization_factor=d.normalization_factor)


def part_b(c):
    relay4 = F.BP4_Relay_Model(c, F.RelayBP4Decoder(c), seed=SEED)
    g = relay4.graph
    side_x, side_z = F.RelayBPDecoder(c.hx), F.RelayBPDecoder(c.hz)  # hx sees the z part of the noise, hz the x part
    bp4 = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    osd = F.BP4_OSD_Model(c, bp4, F.OSD0_Decoder(c.N), seed=SEED)
    side_p = np.float32(2.0 * P / 3.0)
    side_llr = float(-np.log((np.float32(1.0) - side_p) / side_p, dtype=np.float32))

    def run_relay4(first):
        relay4._next = first
        relay4(B, P)
        return relay4.last_x_hat, relay4.last_z_hat, relay4.last_num_unsolved

    def run_sides(first):
        sx, sz = g.syndrome(*g.pauli_noise(SEED, P, first, B))
        z_hat, stz = side_x.decode(sx, llr_const=side_llr, B=B)
        x_hat, stx = side_z.decode(sz, llr_const=side_llr, B=B)
        return x_hat, z_hat, int(((stz[:, 0] == 0) | (stx[:, 0] == 0)).sum().item())

    def run_osd(first):
        osd._next = first
        o = osd.decode(B, P)
        return o["x_hat"], o["z_hat"], osd.last_num_osd

    runs = (("relay4", run_relay4), ("relay_per_side", run_sides), ("bp4_osd0", run_osd))
    for _, fn in runs:
        fn(0)
    torch.cuda.synchronize()
    t = {tag: [] for tag, _ in runs}
    err = {tag: 0 for tag, _ in runs}
    unsolved = {tag: 0 for tag, _ in runs}
    for i in range(BATCHES):
        ex, ez = g.pauli_noise(SEED, P, i * B, B)  # the samples every decoder draws for this batch
        for tag, fn in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x_hat, z_hat, uns = fn(i * B)
            torch.cuda.synchronize()
            t[tag].append((time.perf_counter() - t0) * 1e3)
            _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)
            err[tag] += int((flags != 0).sum().item())
            unsolved[tag] += uns
    n = B * BATCHES
    return dict(batches=BATCHES,
                relay4=dict(config=relay_config(relay4.relay_decoder), batch_ms=spread(t["relay4"]), unsolved=unsolved["relay4"],
                            logical=rate(err["relay4"], n)),
                relay_per_side=dict(config=relay_config(side_x), bsc_p=float(side_p), batch_ms=spread(t["relay_per_side"]),
                                    unsolved=unsolved["relay_per_side"], logical=rate(err["relay_per_side"], n)),
                bp4_osd0=dict(config=dict(cn_type="minsum", num_iter=100, normalization_factor=0.8, osd="osd0"),
                              batch_ms=spread(t["bp4_osd0"]), bp_unsolved=unsolved["bp4_osd0"], logical=rate(err["bp4_osd0"], n)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_relay4 needs a HIP device")
    c = code("ghp882")
    print(json.dumps(dict(code="ghp882 [[882,24]]", p=P, B=B, device=torch.cuda.get_device_name(0), a=part_a(c), b=part_b(c))))


if __name__ == "__main__":
    main()
