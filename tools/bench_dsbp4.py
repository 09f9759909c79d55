"""Soft-syndrome BP4 (fgnn_dsbp4_decode, SoftSyndromeBP4Decoder) on [[882,24]] under depolarizing noise at p = 0.05, B = 16 384 seeded
samples (the library's Philox streams, samples 0..B-1), min-sum at base factor 0.8.  Writes profiles/dsbp4_bench.json (or --out) and
prints it as one JSON line.
    python tools/bench_dsbp4.py [--out FILE]
Each part runs in a child process of its own under a time limit (--limit seconds, default 300); a part that fails or runs out of time
ends the tool, and nothing more is started on the GPU.

Timing: HIP events around 3 launches, 5 rounds after a warm-up; the median round is reported with the fastest and the slowest.

(a) What the extra check input and the u_hat bytes cost: fgnn_dsbp4_decode at gamma = +inf against fgnn_mbp4_decode on the same inputs
    and attempt list, with one attempt (alpha 1, 64 iterations) and with the default alpha sweep; on the seeded samples, and on
    syndromes no error produces (no sample stops early, so every launch runs every iteration).  gamma is given once as the scalar and
    once as per-check arrays filled with +inf, which the kernel has to fetch.  For min-sum the outputs must be identical to
    fgnn_mbp4_decode's with u_hat zero, and the tool asserts it.  Ratios are recorded, not gated.
(b) Decoding figures at q in {0, 0.01, 0.03}: soft-syndrome BP4 with one attempt, the soft-syndrome alpha sweep, and hard-syndrome
    fgnn_mbp4_decode under the same sweep fed the noisy bits (what a user has without this decoder).  Per decoder: samples left
    unsolved, samples with u_hat != u (the hard decoder estimates no flips: its u_hat is 0), samples whose residual syndrome is zero and
    the logical errors among them.  Recorded, not asserted."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = int(os.environ.get("DSBP4_BENCH_B", 16384))
P = 0.05
QS = (0.0, 0.01, 0.03)
ITERS, REPS, ROUNDS = 64, 3, 5
SEED = 0x5EED
BASE = 0.8
OUT = os.path.join(ROOT, "profiles", "dsbp4_bench.json")


def setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dsbp4 needs a HIP device")
    from feedback_gnn_amd.graph import TannerGraph
    from helpers import code
    c = code("ghp882")
    return torch, c, TannerGraph(c, stage_one=False)


def events(torch, fn, reps):
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
    import numpy as np
    p = np.float32(p)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p) / p, dtype=np.float32))


def part_a():
    import numpy as np
    torch, c, g = setup()
    from feedback_gnn_amd import _lib, gf2
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    L = llr_depolarizing(P)
    sx, sz = g.syndrome(*g.pauli_noise(SEED, P, 0, B))
    left = np.asarray(gf2.kernel(np.asarray(c.hx, np.int64).T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has dependent rows: some syndromes cannot be satisfied"
    u = left[0]
    bad = sx.cpu().numpy()
    bad[(bad.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    inputs = dict(seeded_samples=sx, no_sample_stops=torch.from_numpy(bad).to(g.device))
    inf_x = torch.full((B, g.m_x), float("inf"), dtype=torch.float32, device=g.device)
    inf_z = torch.full((B, g.m_z), float("inf"), dtype=torch.float32, device=g.device)
    res = dict(iterations=ITERS, launches_per_round=REPS, rounds=ROUNDS, library_sha256=_lib.library_sha256())
    for in_tag, synd_x in inputs.items():
        for at_tag, alphas in (("one_attempt", (1.0,)), ("default_sweep", ALPHA_DEFAULTS)):
            factors, owns = mbp4_tables(alphas, BASE)
            out = {}

            def mb():
                out["mbp4"] = g.mbp4_decode(synd_x, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L)

            def ds():
                out["dsbp4_scalar"] = g.dsbp4_decode(synd_x, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L)

            def da():
                out["dsbp4_arrays"] = g.dsbp4_decode(synd_x, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L, synd_llr_x=inf_x,
                                                     synd_llr_z=inf_z)

            fns = dict(mbp4=mb, dsbp4_scalar=ds, dsbp4_arrays=da)
            for fn in fns.values():
                events(torch, fn, 2)
            x0, z0, s0 = out["mbp4"]
            for tag in ("dsbp4_scalar", "dsbp4_arrays"):
                xh, zh, ux, uz, st = out[tag]
                assert torch.equal(xh, x0) and torch.equal(zh, z0) and torch.equal(st, s0), f"{tag} differs from fgnn_mbp4_decode"
                assert not bool(ux.any()) and not bool(uz.any()), f"{tag}: u_hat must be zero at gamma = +inf"
            if in_tag == "no_sample_stops":
                assert int((s0[:, 0] != 0).sum()) == 0, "no sample may stop early"
            t = {tag: [] for tag in fns}
            for _ in range(ROUNDS):
                for tag, fn in fns.items():
                    t[tag].append(events(torch, fn, REPS))
            ms = {tag: spread(v) for tag, v in t.items()}
            res[f"{in_tag}/{at_tag}"] = dict(
                alphas=list(alphas), solved=int((s0[:, 0] != 0).sum()), mean_iterations=float(s0[:, 2].float().mean()), ms=ms,
                ratio_scalar=round(ms["dsbp4_scalar"]["median"] / ms["mbp4"]["median"], 3),
                ratio_arrays=round(ms["dsbp4_arrays"]["median"] / ms["mbp4"]["median"], 3), outputs_identical=True)
    return res


def part_b():
    torch, c, g = setup()
    import feedback_gnn_amd as F
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    L = llr_depolarizing(P)
    ex, ez = g.pauli_noise(SEED, P, 0, B)
    sx, sz = g.syndrome(ex, ez)
    res = dict(alphas_sweep=list(ALPHA_DEFAULTS), num_iter=ITERS)

    def figures(x_hat, z_hat, stats, u_miss):
        s_hat, ls_hat, _ = g.residual(ex, ez, x_hat, z_hat, want_arrays=True)
        clean = ~(s_hat != 0).any(1)
        return dict(unsolved=int((stats[:, 0] == 0).sum()), u_hat_differs_from_u=int(u_miss.sum()), zero_residual=int(clean.sum()),
                    logical_errors_among_zero_residual=int((clean & (ls_hat != 0).any(1)).sum()),
                    mean_iterations=float(stats[:, 2].float().mean()))

    for q in QS:
        row = {}
        for tag, alphas in (("soft_one_attempt", (1.0,)), ("soft_alpha_sweep", ALPHA_DEFAULTS)):
            dec = F.SoftSyndromeBP4Decoder(c, alphas=alphas, num_iter=ITERS, cn_type="minsum", factor=BASE, graph=g)
            model = F.BP4_SoftSyndrome_Model(c, dec, q, seed=SEED)
            model(B, P)
            assert torch.equal(model.last_noise_x, ex) and torch.equal(model.last_noise_z, ez)
            miss = (model.last_u_x != model.last_u_x_hat).any(1) | (model.last_u_z != model.last_u_z_hat).any(1)
            row[tag] = figures(model.last_x_hat, model.last_z_hat, model.last_stats, miss)
            row["gamma"] = model.gamma if q > 0 else "inf"  # JSON has no infinity
            row["samples_with_flips"] = int(((model.last_u_x != 0).any(1) | (model.last_u_z != 0).any(1)).sum())
        if q > 0:
            ux, uz = g.syndrome_noise(SEED, q, 0, B)
        else:
            ux, uz = torch.zeros_like(sx), torch.zeros_like(sz)
        x_hat, z_hat, stats = g.mbp4_decode(sx ^ ux, sz ^ uz, *mbp4_tables(ALPHA_DEFAULTS, BASE), ITERS, ITERS, "minsum", llr_const=L)
        row["hard_alpha_sweep_on_noisy_bits"] = figures(x_hat, z_hat, stats, (ux != 0).any(1) | (uz != 0).any(1))
        res[f"q={q}"] = row
    return res


PARTS = dict(a=part_a, b=part_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--limit", type=int, default=300, help="seconds a part may take")
    ap.add_argument("--part", choices=sorted(PARTS), help="run one part in this process and print its JSON (what the tool starts)")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part]()))
        return
    out = dict(code="ghp882 [[882,24]]", p=P, B=B, seed=SEED, cn_type="minsum", base_factor=BASE)
    for part in sorted(PARTS):  # one fresh process per GPU step; the first that fails is the last that ran
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part], stdout=subprocess.PIPE, text=True,
                                 timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"part {part} ran past its limit of {args.limit} s")
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not lines:
            sys.stdout.write(run.stdout)
            raise SystemExit(f"part {part} failed with exit status {run.returncode}")
        out[part] = json.loads(lines[-1][len("RESULT "):])
    if B == 16384:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
