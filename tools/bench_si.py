"""BP-SI (fgnn_si_decode, SIDecoder, BP2_SI_Model) on the hx graph of [[882,24]], its hz as the groups, over a BSC at the p of
tools/bench_relay.py and tools/bench_gdg.py (p = 0.07 * 2 / 3), B = 10 000 syndromes per batch, 50 000 shared samples.  Writes
profiles/si_bench.json (or --out) and prints it as one JSON line.
    python tools/bench_si.py [--out FILE]

(a) The price of the frame: the kernel with max_groups = 0 against one Relay-BP leg with gamma 0 at the same iteration count, on
    syndromes no error produces (so no sample stops early).  HIP events around REPS launches, the two alternating, ROUNDS rounds after a
    warm-up; the median round with the fastest and the slowest, and the ratio of the medians.  BP-GDG at depth 0 measured 1.13 of a leg
    (profiles/gdg_bench.json) with the same kind of marks.
(b) Decoding.  Every decoder runs through its evaluation model on the same Philox samples (the models share the seed and walk the
    stream batch by batch): the default SIDecoder (64 + 32 iterations, factor 0.8) at max_groups 1 / 5 / 10 / 20 / all, min-sum BP with
    up to 100 iterations (factor 0.8, stopped at the first solution), the default Relay-BP, BP-GDG at depth 3 with max_rounds = 40, and
    min-sum-100 + OSD-0 and + LSD.  Per decoder: host time per batch around a device synchronise, the samples left without a solution
    (for + OSD-0 / + LSD: the samples BP hands on; the post-processor solves each of them) and the logical errors (an unsolved sample
    counts as one) with the binomial standard error; for SI also how many samples each number of attempts rescued.

No figure is gated: the comparisons are between decoders of the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feedback_gnn_amd as F  # noqa: E402
from feedback_gnn_amd import _lib, gf2  # noqa: E402
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402
from helpers import code  # noqa: E402

B = int(os.environ.get("SI_BENCH_B", 10000))
P = 0.07 * 2 / 3
ITERS, REPS, ROUNDS = 64, 10, 15
BATCHES = int(os.environ.get("SI_BENCH_BATCHES", 5))
OUT = os.path.join(ROOT, "profiles", "si_bench.json")


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


def logit(p):
    return float(-np.log((np.float32(1.0) - np.float32(p)) / np.float32(p), dtype=np.float32))


def rate(k, n):
    r = k / n
    return dict(errors=int(k), samples=int(n), rate=r, stderr=float(np.sqrt(r * (1 - r) / n)))


def part_a(c):
    g = TannerGraph(c)
    hx = np.asarray(c.hx, np.int64)
    left = np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has independent rows: every syndrome can be satisfied"
    u = left[0]
    synd = g.syndrome(torch.zeros((B, g.n), dtype=torch.uint8, device=g.device), g.bsc_noise(0x5EED, P, 0, B))[0].cpu().numpy()
    synd[(synd.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    synd = torch.from_numpy(synd).to(g.device)
    L = logit(P)
    gamma = torch.zeros((1, g.n), dtype=torch.float32, device=g.device)
    out = {}

    def relay():
        out["relay"] = g.relay_decode(synd, gamma, ITERS, ITERS, 1, 0.8, llr_const=L)

    def si():
        out["si"] = g.si_decode(synd, ITERS, 1, 0, 0.8, llr_const=L)

    for fn in (relay, si):
        events(fn, 3)
    assert torch.equal(out["relay"][0], out["si"][0]) and not out["si"][1][:, :3].any() and bool((out["si"][1][:, 3] == -1).all())
    t_relay, t_si = [], []
    for _ in range(ROUNDS):
        t_relay.append(events(relay, REPS))
        t_si.append(events(si, REPS))
    a, b = spread(t_relay), spread(t_si)
    return dict(iterations=ITERS, relay_one_leg_gamma0_ms=a, si_no_groups_ms=b, ratio=round(b["median"] / a["median"], 3),
                gdg_depth0_ratio_for_comparison=1.13, launches_per_round=REPS, rounds=ROUNDS)


def part_b(c):
    def si(**kw):
        return F.BP2_SI_Model(c.hx, c.hz, c.lx, F.SIDecoder(c.hx, c.hz, **kw))

    m_z = int(np.asarray(c.hz).shape[0])
    bp100 = dict(is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    models = {f"si_groups{k}": si(max_groups=k) for k in (1, 5, 10, 20)}
    models["si_groups_all"] = si(max_groups=m_z)
    models["minsum100"] = si(num_iter=100, max_groups=0)
    models["relay_default"] = F.BP2_Relay_Model(c.hx, c.lx, F.RelayBPDecoder(c.hx))
    models["gdg_depth3_rounds40"] = F.BP2_GDG_Model(c.hx, c.lx, F.GDGDecoder(c.hx, max_rounds=40))
    models["minsum100_osd0"] = F.BP2_OSD_Model(c.hx, c.hx_basis, c.pivot_hx, c.lx, F.LDPCBPDecoder(c.hx, **bp100), F.OSD0_Decoder(c.N))
    models["minsum100_lsd"] = F.BP2_LSD_Model(c.hx, c.lx, F.LDPCBPDecoder(c.hx, **bp100), F.LSD_Decoder(c.N))

    def unsolved_of(tag, m):
        return m.last_num_osd if tag.endswith("osd0") else m.last_num_lsd if tag.endswith("lsd") else m.last_num_unsolved

    for m in models.values():
        m(B, P)
    torch.cuda.synchronize()
    t = {tag: [] for tag in models}
    err = dict.fromkeys(models, 0)
    unsolved = dict.fromkeys(models, 0)
    attempts = {tag: np.zeros(0, np.int64) for tag in models if tag.startswith("si_")}
    for _ in range(BATCHES):
        for tag, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s_hat, ls_hat = m(B, P)
            torch.cuda.synchronize()
            t[tag].append((time.perf_counter() - t0) * 1e3)
            err[tag] += int((s_hat.any(1) | ls_hat.any(1)).sum())
            unsolved[tag] += unsolved_of(tag, m)
            if tag in attempts:
                st = m.last_stats
                cnt = np.bincount(st[st[:, 0] == 1, 1].cpu().numpy())
                both = np.zeros(max(len(cnt), len(attempts[tag])), np.int64)
                both[:len(cnt)] += cnt
                both[:len(attempts[tag])] += attempts[tag]
                attempts[tag] = both
    n = B * BATCHES
    res = dict(batches=BATCHES, samples=n)
    for tag, m in models.items():
        res[tag] = dict(batch_ms=spread(t[tag]), unsolved=int(unsolved[tag]), logical=rate(err[tag], n))
        if tag in attempts or tag == "minsum100":
            d = m.si_decoder
            res[tag]["config"] = dict(num_iter=d.num_iter, si_iter=d.si_iter, max_groups=d.max_groups, normalization_factor=d.normalization_factor)
        if tag in attempts:
            res[tag]["solved_by_attempt"] = attempts[tag].tolist()   # entry a: samples whose solution came from attempt a (0: plain BP)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_si needs a HIP device")
    c = code("ghp882")
    res = dict(code="ghp882 hx [[882,24]], groups = its hz", p=P, B=B, device=torch.cuda.get_device_name(0), library_sha256=_lib.library_sha256(),
               a=part_a(c), b=part_b(c))
    text = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
