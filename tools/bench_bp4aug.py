"""Augmented BP4 (fgnn_bp4aug_decode) on [[882,24]] under depolarizing noise at p = 0.10, B = 16 384, the same seeded samples (the
library's Philox stream, samples 0..B-1) for every decoder.  Writes profiles/bp4aug_bench.json and prints it as one JSON line.
    python tools/bench_bp4aug.py

Timing: HIP events around 3 launches, 5 rounds after a warm-up; the median round is reported with the fastest and the slowest.

(a) What the duplicate marks cost when they are never used: max_attempts = 0 with pre_iter = 64 on syndromes no error produces (so no
    sample stops early), against fgnn_bp4fb_decode with max_attempts = 0 on the same input; min-sum at factor 0.8.  The feedback kernel
    is the yardstick: the same step structure with its mark bytes in place of the duplicate marks.  Recorded, not gated.
(b) Decoders on the same samples: the default BP4AugmentedDecoder (restart) and the same with the messages kept, min-sum-64 flooding
    BP4 (factor 0.8), BP4FeedbackDecoder with both rules at their defaults, the default BP4GDDecoder, the default AMBP4Decoder,
    BP4_OSD_Model (min-sum-100 + OSD-0) and the default RelayBP4Decoder.  Per decoder: ms per batch from the seeded samples to the
    estimate (drawing the noise and its syndromes included, the same work for every decoder), the samples left without a solution (for
    BP4 + OSD: the samples BP4 hands to OSD; OSD-0 solves each of them), and the logical errors (a sample whose residual misses the
    syndrome or a logical operator) with their binomial standard error."""
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

B = int(os.environ.get("BP4AUG_BENCH_B", 16384))
P = 0.10
ITERS, REPS, ROUNDS = 64, 3, 5
SEED = 0x5EED
OUT = os.path.join(ROOT, "profiles", "bp4aug_bench.json")


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
    out = {}

    def fb():
        out["fb"] = g.bp4fb_decode(sx, sz, "perturb", ITERS, 4, 0, 1.0, "minsum", 0.8, llr_const=L)

    def aug():
        out["aug"] = g.bp4aug_decode(sx, sz, ITERS, 4, 0, 0.1, "minsum", 0.8, llr_const=L)

    fns = dict(fb=fb, aug=aug)
    for fn in fns.values():
        events(fn, 2)
    for tag in fns:
        st = out[tag][2]
        assert int((st[:, 0] != 0).sum()) == 0 and int((st[:, 3] != ITERS).sum()) == 0, "no sample may stop early"
    same = all(bool(torch.equal(out["fb"][i], out["aug"][i])) for i in range(3))
    t = {tag: [] for tag in fns}
    for _ in range(ROUNDS):
        for tag, fn in fns.items():
            t[tag].append(events(fn, REPS))
    ms = {tag: spread(v) for tag, v in t.items()}
    return dict(iterations=ITERS, bp4fb_no_attempts_ms=ms["fb"], bp4aug_no_attempts_ms=ms["aug"],
                ratio=round(ms["aug"]["median"] / ms["fb"]["median"], 3), outputs_identical=same, launches_per_round=REPS, rounds=ROUNDS)


def rate(k, n):
    r = k / n
    return dict(errors=int(k), samples=int(n), rate=r, stderr=float(np.sqrt(r * (1 - r) / n)))


def part_b(c):
    g = TannerGraph(c, stage_one=False)
    L = llr_depolarizing(P)
    models = {}

    def model_run(model):
        def run():
            model._next = 0
            model(B, P)
            return model.last_x_hat, model.last_z_hat, model.last_num_unsolved
        return run

    def aug_run(tag, **kw):
        dec = F.BP4AugmentedDecoder(c, graph=g, seed=SEED, **kw)
        models[tag] = F.BP4_Augmented_Model(c, dec, seed=SEED)
        cfg = dict(pre_iter=dec.pre_iter, attempt_iter=dec.attempt_iter, max_attempts=dec.max_attempts, density=dec.density,
                   restart=dec.restart, cn_type=dec.cn_type, normalization_factor=dec.normalization_factor)
        return tag, model_run(models[tag]), cfg

    def fb_run(tag, rule):
        dec = F.BP4FeedbackDecoder(c, rule, graph=g, seed=SEED)
        models[tag] = F.BP4_Feedback_Model(c, dec, seed=SEED)
        cfg = dict(rule=rule, pre_iter=dec.pre_iter, attempt_iter=dec.attempt_iter, max_attempts=dec.max_attempts, strength=dec.strength,
                   restart=dec.restart, cn_type=dec.cn_type, normalization_factor=dec.normalization_factor)
        return tag, model_run(models[tag]), cfg

    gd_dec = F.BP4GDDecoder(c, graph=g)
    gd = F.BP4_GD_Model(c, gd_dec, seed=SEED)
    ambp_dec = F.AMBP4Decoder(c, graph=g)
    models["ambp4_default"] = F.BP4_AMBP_Model(c, ambp_dec, seed=SEED)
    relay_dec = F.RelayBP4Decoder(c, graph=g)
    relay = F.BP4_Relay_Model(c, relay_dec, seed=SEED)
    bp4 = F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=100, normalization_factor=0.8)
    osd = F.BP4_OSD_Model(c, bp4, F.OSD0_Decoder(c.N), seed=SEED)

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

    runs = (aug_run("bp4aug_default_restart"), aug_run("bp4aug_messages_kept", restart=False),
            ("bp4_minsum_64_flooding", run_flooding, dict(cn_type="minsum", num_iter=ITERS, normalization_factor=0.8)),
            fb_run("bp4fb_perturb_default", "perturb"), fb_run("bp4fb_enhanced_default", "enhanced"),
            ("bp4gd_default", model_run(gd), dict(pre_iter=gd_dec.pre_iter, round_iter=gd_dec.round_iter, max_rounds=gd_dec.max_rounds,
                                                  decim_llr=gd_dec.decim_llr, cn_type=gd_dec.cn_type,
                                                  normalization_factor=gd_dec.normalization_factor)),
            ("ambp4_default", model_run(models["ambp4_default"]), dict(alphas=[float(a) for a in ambp_dec.alphas], num_iter=ambp_dec.num_iter,
                                                                       cn_type=ambp_dec.cn_type, factor=ambp_dec.factor,
                                                                       restart=ambp_dec.restart)),
            ("bp4_osd0", run_osd, dict(cn_type="minsum", num_iter=100, normalization_factor=0.8, osd="osd0")),
            ("relay4_default", model_run(relay), dict(gamma0=relay_dec.gamma0, pre_iter=relay_dec.pre_iter, num_sets=relay_dec.num_sets,
                                                      set_max_iter=relay_dec.set_max_iter,
                                                      gamma_dist_interval=relay_dec.gamma_dist_interval, stop_nconv=relay_dec.stop_nconv,
                                                      normalization_factor=relay_dec.normalization_factor)))
    ex, ez = g.pauli_noise(SEED, P, 0, B)  # the samples every decoder draws
    res = {}
    for tag, fn, cfg in runs:
        x_hat, z_hat, uns = fn()  # warm-up, and the figures
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)
        key = "bp_unsolved" if tag == "bp4_osd0" else "unsolved"
        res[tag] = {"config": cfg, key: int(uns), "logical": rate(int((flags != 0).sum().item()), B)}
        if tag in models:
            st = models[tag].last_stats
            res[tag]["solved_after_attempt_0"] = int(((st[:, 0] == 1) & (st[:, 1] > 0)).sum().item())
            res[tag]["max_attempts_used"], res[tag]["max_iterations"] = int(st[:, 1].max().item()), int(st[:, 2].max().item())
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
        raise SystemExit("bench_bp4aug needs a HIP device")
    c = code("ghp882")
    parts = os.environ.get("BP4AUG_BENCH_PARTS", "ab")
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
