"""Relay-BP (fgnn_relay_decode) on the hx graph of [[882,24]] over a BSC at the p of the reference's QLDPC.ipynb cell 7 row
(p = 0.07 * 2 / 3), B = 10 000.  Prints one JSON line.   python tools/bench_relay.py

(a) What the memory term and the parity test cost per iteration: one leg of 64 iterations on syndromes no error produces (so no
    sample stops early), against fgnn_bp2_decode min-sum with 64 iterations on the same input.  HIP events around REPS launches, the
    two kernels alternating, ROUNDS rounds after a warm-up; the median round is reported with the fastest and the slowest.
(b) The default RelayBPDecoder against min-sum BP (100 iterations, factor 0.8) + OSD-0, both through their evaluation models on
    their own Philox samples: host time per batch around a device synchronise, the share of samples left without a solution (for
    BP+OSD: the share BP hands to OSD; OSD-0 solves each of them), and the logical error rate (a flagged sample counts as an error)
    with its binomial standard error."""
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

B = int(os.environ.get("RELAY_BENCH_B", 10000))
P = 0.07 * 2 / 3
ITERS, REPS, ROUNDS = 64, 10, 15
BATCHES = int(os.environ.get("RELAY_BENCH_BATCHES", 10))


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


def part_a(c):
    g = TannerGraph(c)
    hx = np.asarray(c.hx, np.int64)
    left = np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has independent rows: every syndrome can be satisfied"
    u = left[0]
    synd = g.syndrome(torch.zeros((B, g.n), dtype=torch.uint8, device=g.device), g.bsc_noise(0x5EED, P, 0, B))[0].cpu().numpy()
    synd[(synd.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    synd = torch.from_numpy(synd).to(g.device)
    L = float(-np.log((np.float32(1.0) - np.float32(P)) / np.float32(P), dtype=np.float32))
    gamma = torch.full((1, g.n), 0.125, dtype=torch.float32, device=g.device)
    out = {}

    def bp2():
        g.bp2_decode(synd, ITERS, "minsum", 1.0, llr_const=L, want_soft=False)

    def relay():
        out["stats"] = g.relay_decode(synd, gamma, ITERS, ITERS, 1, 1.0, llr_const=L)[1]

    for fn in (bp2, relay):
        events(fn, 3)
    assert int((out["stats"][:, 0] != 0).sum()) == 0 and int((out["stats"][:, 3] != ITERS).sum()) == 0
    t_bp2, t_relay = [], []
    for _ in range(ROUNDS):
        t_bp2.append(events(bp2, REPS))
        t_relay.append(events(relay, REPS))
    a, b = spread(t_bp2), spread(t_relay)
    return dict(iterations=ITERS, bp2_minsum_ms=a, relay_one_leg_ms=b, ratio=round(b["median"] / a["median"], 3),
                launches_per_round=REPS, rounds=ROUNDS)


def rate(k, n):
    r = k / n
    return dict(errors=int(k), samples=int(n), rate=r, stderr=float(np.sqrt(r * (1 - r) / n)))


def part_b(c):
    relay = F.BP2_Relay_Model(c.hx, c.lx, F.RelayBPDecoder(c.hx))
    bp2 = F.LDPCBPDecoder(c.hx, is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    osd = F.BP2_OSD_Model(c.hx, c.hx_basis, c.pivot_hx, c.lx, bp2, F.OSD0_Decoder(c.N))
    for m in (relay, osd):
        m(B, P)
    torch.cuda.synchronize()
    t = {"relay": [], "osd": []}
    err = {"relay": 0, "osd": 0}
    unsolved = {"relay": 0, "osd": 0}
    for _ in range(BATCHES):
        for tag, m in (("relay", relay), ("osd", osd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s_hat, ls_hat = m(B, P)
            torch.cuda.synchronize()
            t[tag].append((time.perf_counter() - t0) * 1e3)
            err[tag] += int((s_hat.any(1) | ls_hat.any(1)).sum())
            unsolved[tag] += relay.last_num_unsolved if tag == "relay" else osd.last_num_osd
    n = B * BATCHES
    d = relay.relay_decoder
    return dict(batches=BATCHES,
                relay=dict(config=dict(gamma0=d.gamma0, pre_iter=d.pre_iter, num_sets=d.num_sets, set_max_iter=d.set_max_iter,
                                       gamma_dist_interval=d.gamma_dist_interval, stop_nconv=d.stop_nconv,
                                       normalization_factor=d.normalization_factor),
                           batch_ms=spread(t["relay"]), unsolved_share=unsolved["relay"] / n, logical=rate(err["relay"], n)),
                bp_osd0=dict(config=dict(cn_type="minsum", num_iter=100, normalization_factor=0.8, osd="osd0"),
                             batch_ms=spread(t["osd"]), bp_unsolved_share=unsolved["osd"] / n, logical=rate(err["osd"], n)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_relay needs a HIP device")
    c = code("ghp882")
    print(json.dumps(dict(code="ghp882 hx [[882,24]]", p=P, B=B, device=torch.cuda.get_device_name(0), a=part_a(c), b=part_b(c))))


if __name__ == "__main__":
    main()
