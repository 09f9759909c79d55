"""BP-GDG (fgnn_gdg_decode, GDGDecoder, BP2_GDG_Model) on the hx graph of [[882,24]] over a BSC at the p of tools/bench_relay.py
(p = 0.07 * 2 / 3), B = 10 000 syndromes per batch.  Writes profiles/gdg_bench.json (or --out) and prints it as one JSON line.
    python tools/bench_gdg.py [--out FILE]

(a) The price of the frame: the kernel at depth 0 / max_rounds 0 against one Relay-BP leg with gamma 0 at the same iteration count,
    on syndromes no error produces (so no sample stops early).  HIP events around REPS launches, the two alternating, ROUNDS rounds
    after a warm-up; the median round with the fastest and the slowest, and the ratio of the medians.
(b) Decoding.  Every decoder runs through its evaluation model on the same Philox samples (the models share the seed and walk the
    stream batch by batch): the default GDGDecoder with and without the prefilter, depth 0 .. 4, the default with max_rounds = 40 (a
    path then gives up after 40 fixes instead of fixing every bit), min-sum BP with up to 100 iterations
    (factor 0.8, stopped at the first solution), the default Relay-BP, and min-sum-100 + OSD-0 and + LSD.  Per decoder: host time per
    batch around a device synchronise, the samples left without a solution (for + OSD-0 / + LSD: the samples BP hands on; the
    post-processor solves each of them) and the logical errors (an unsolved sample counts as one) with the binomial standard error.
(c) Per-bit priors: three rounds of noisy measurements of hx as one binary problem, H_st = window_matrix(hx, 3), data bits flipped
    with 2/3 of tools/bench_stbp4.py's P_ROUND per round and measurement bits with its Q (the last measurement perfect), the logits
    of those rates as llr_ch.  The default GDGDecoder, the one with max_rounds = 40, min-sum-100 and the default Relay-BP on the same
    host-drawn samples: time per batch, unsolved samples, and logical errors (unsolved, or a residual data error, summed over the
    rounds, that is not a stabiliser).

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

B = int(os.environ.get("GDG_BENCH_B", 10000))
P = 0.07 * 2 / 3
ITERS, REPS, ROUNDS = 64, 10, 15
BATCHES = int(os.environ.get("GDG_BENCH_BATCHES", 5))
P_ROUND, Q, WINDOW = 0.02, 0.01, 3   # tools/bench_stbp4.py
B_WINDOW = int(os.environ.get("GDG_BENCH_B_WINDOW", 2000))
OUT = os.path.join(ROOT, "profiles", "gdg_bench.json")


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

    def gdg():
        out["gdg"] = g.gdg_decode(synd, ITERS, 1, 0, 0, "least", 25.0, 0.8, llr_const=L, want_path_stats=True)

    for fn in (relay, gdg):
        events(fn, 3)
    assert torch.equal(out["relay"][0], out["gdg"][0]) and not out["gdg"][1][:, 0].any() and bool((out["gdg"][2][:, 0, 3] == ITERS).all())
    t_relay, t_gdg = [], []
    for _ in range(ROUNDS):
        t_relay.append(events(relay, REPS))
        t_gdg.append(events(gdg, REPS))
    a, b = spread(t_relay), spread(t_gdg)
    return dict(iterations=ITERS, relay_one_leg_gamma0_ms=a, gdg_depth0_no_rounds_ms=b, ratio=round(b["median"] / a["median"], 3),
                launches_per_round=REPS, rounds=ROUNDS)


def part_b(c):
    def gdg(**kw):
        return F.BP2_GDG_Model(c.hx, c.lx, F.GDGDecoder(c.hx, **kw))

    bp100 = dict(is_syndrome=True, hard_out=False, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    models = {"gdg_default": gdg(), "gdg_default_no_prefilter": gdg(prefilter=False)}
    for depth in range(5):
        models[f"gdg_depth{depth}"] = gdg(depth=depth)
    models["gdg_depth3_rounds40"] = gdg(max_rounds=40)
    models["minsum100"] = gdg(pre_iter=100, max_rounds=0, depth=0)
    models["relay_default"] = F.BP2_Relay_Model(c.hx, c.lx, F.RelayBPDecoder(c.hx))
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
    fixed = {tag: [] for tag in models if tag.startswith("gdg")}
    for _ in range(BATCHES):
        for tag, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s_hat, ls_hat = m(B, P)
            torch.cuda.synchronize()
            t[tag].append((time.perf_counter() - t0) * 1e3)
            err[tag] += int((s_hat.any(1) | ls_hat.any(1)).sum())
            unsolved[tag] += unsolved_of(tag, m)
            if tag in fixed:
                st = m.last_stats
                fixed[tag].append(dict(other_path=int((st[:, 2] != 0).sum()), max_bits_fixed=int(st[:, 3].max()),
                                       unsolved_bits_fixed=int(st[st[:, 0] == 0, 3].float().mean()) if bool((st[:, 0] == 0).any()) else None))
    n = B * BATCHES
    res = dict(batches=BATCHES, samples=n)
    for tag, m in models.items():
        res[tag] = dict(batch_ms=spread(t[tag]), unsolved=int(unsolved[tag]), logical=rate(err[tag], n))
        if tag in fixed:
            d = m.gdg_decoder
            res[tag]["config"] = dict(pre_iter=d.pre_iter, round_iter=d.round_iter, max_rounds=d.max_rounds, depth=d.depth, tail=d.tail,
                                      decim_llr=d.decim_llr, normalization_factor=d.normalization_factor, prefilter=d.prefilter)
            res[tag]["per_batch"] = fixed[tag]
    return res


def part_c(c):
    from feedback_gnn_amd.space_time import window_matrix
    hx, lx = np.asarray(c.hx, np.int64), np.asarray(c.lx, np.int64)
    m, n = hx.shape
    H = window_matrix(hx, WINDOW).astype(np.int64)
    # the last measurement is perfect: its time bits never flip and carry the clipped prior of "no flip"
    p_bit = np.concatenate([np.full(WINDOW * n, P_ROUND * 2 / 3), np.full((WINDOW - 1) * m, Q), np.zeros(m)])
    x = (np.random.RandomState(0x5EED).rand(B_WINDOW, H.shape[1]) < p_bit).astype(np.int64)
    synd_h = (x @ H.T % 2).astype(np.uint8)
    llr_h = np.broadcast_to(np.array([logit(p) if p > 0 else -20.0 for p in p_bit], np.float32), x.shape).copy()
    decs = {"gdg_default": F.GDGDecoder(H), "gdg_depth3_rounds40": F.GDGDecoder(H, max_rounds=40),
            "minsum100": F.GDGDecoder(H, pre_iter=100, max_rounds=0, depth=0), "relay_default": F.RelayBPDecoder(H)}
    g = decs["gdg_default"].graph
    synd, llr = torch.from_numpy(synd_h).to(g.device), torch.from_numpy(llr_h).to(g.device)
    res = dict(window_rounds=WINDOW, checks=int(H.shape[0]), bits=int(H.shape[1]), samples=B_WINDOW, p_data=P_ROUND * 2 / 3, q_measurement=Q,
               batches=BATCHES)
    for tag, d in decs.items():
        d.decode(synd, llr_ch=llr)
        torch.cuda.synchronize()
        ts = []
        for _ in range(BATCHES):
            t0 = time.perf_counter()
            hard, stats = d.decode(synd, llr_ch=llr)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        hard, solved = hard.cpu().numpy().astype(np.int64), (stats[:, 0] > 0).cpu().numpy()
        assert not ((hard[solved] @ H.T + synd_h[solved]) % 2).any()
        r = (x ^ hard)[:, :WINDOW * n].reshape(B_WINDOW, WINDOW, n).sum(1) % 2
        bad = (r @ hx.T % 2).any(1) | (r @ lx.T % 2).any(1) | ~solved
        res[tag] = dict(batch_ms=spread(ts), unsolved=int((~solved).sum()), logical=rate(int(bad.sum()), B_WINDOW))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gdg needs a HIP device")
    c = code("ghp882")
    res = dict(code="ghp882 hx [[882,24]]", p=P, B=B, device=torch.cuda.get_device_name(0), library_sha256=_lib.library_sha256(),
               a=part_a(c), b=part_b(c), c=part_c(c))
    text = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
