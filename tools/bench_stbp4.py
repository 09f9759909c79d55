"""Space-time BP4 (fgnn_stbp4_decode, SpaceTimeBP4Decoder, BP4_Phenomenological_Model) on [[882,24]], min-sum at base factor 0.8, 64
iterations, the library's seeded Philox streams.  Writes profiles/stbp4_bench.json (or --out) and prints it as one JSON line.
    python tools/bench_stbp4.py [--out FILE]
Each part runs in a child process of its own under a time limit (--limit seconds, default 300); a part that fails or runs out of time
ends the tool, and nothing more is started on the GPU.

Timing: HIP events around 3 launches, 5 rounds after a warm-up, the variants alternating inside every round; the median round is
reported with the fastest and the slowest.

(a) Cost.  R = 1 against fgnn_dsbp4_decode on the same inputs (seeded samples at p = 0.05 with flips at q = 0.01, one attempt), with
    identical outputs asserted.  R = 3 and R = 5 with every gamma = +inf on syndromes on which no window stops (the first round's
    syndrome lies outside the column space of hx, so every launch runs every iteration): the time per round of a window against
    fgnn_dsbp4_decode on B * R samples of the same kind, whose kernel this feature leaves as it was.  Ratios are recorded, not gated.
(b) Decoding a memory experiment of 5 rounds at P_ROUND per round with flips of rate Q (the last measurement perfect): one window of
    5 rounds, sliding windows of 3 rounds that commit 1, and single-shot fgnn_dsbp4_decode applied round by round to the measured
    syndrome with the committed corrections taken out.  Per decoder, for one attempt and for the default alpha sweep: samples with a
    window (a round) left unsolved, samples with a non-zero final residual syndrome, and the logical errors among the others.  Recorded,
    not asserted."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = int(os.environ.get("STBP4_BENCH_B", 16384))  # samples of part (b); part (a) times B // 4 windows
P = 0.05
P_ROUND, Q, EXPERIMENT = 0.02, 0.01, 5
ITERS, REPS, ROUNDS = 64, 3, 5
SEED = 0x5EED
BASE = 0.8
INF = float("inf")
OUT = os.path.join(ROOT, "profiles", "stbp4_bench.json")


def setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stbp4 needs a HIP device")
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


def gamma_of(q):
    import numpy as np
    q = np.float32(q)
    return float(np.log((np.float32(1.0) - q) / q, dtype=np.float32))


def alternate(torch, fns):
    """{tag: spread of ms per launch}: a warm-up of every variant, then ROUNDS rounds in which the variants take turns."""
    for fn in fns.values():
        events(torch, fn, 2)
    t = {tag: [] for tag in fns}
    for _ in range(ROUNDS):
        for tag, fn in fns.items():
            t[tag].append(events(torch, fn, REPS))
    return {tag: spread(v) for tag, v in t.items()}


def part_a():
    import numpy as np
    torch, c, g = setup()
    from feedback_gnn_amd import _lib, gf2
    from feedback_gnn_amd.mbp import mbp4_tables
    L = llr_depolarizing(P)
    Bw = max(B // 4, 1)
    factors, owns = mbp4_tables((1.0,), BASE)
    res = dict(windows=Bw, iterations=ITERS, launches_per_round=REPS, rounds=ROUNDS, library_sha256=_lib.library_sha256())
    # R = 1 against fgnn_dsbp4_decode
    sx, sz = g.syndrome(*g.pauli_noise(SEED, P, 0, Bw))
    ux, uz = g.syndrome_noise(SEED, Q, 0, Bw)
    sx, sz = sx ^ ux, sz ^ uz
    gq = gamma_of(Q)
    wx, wz = sx[:, None].contiguous(), sz[:, None].contiguous()
    out = {}

    def ds():
        out["dsbp4"] = g.dsbp4_decode(sx, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L, gamma_x=gq, gamma_z=gq)

    def st():
        out["stbp4"] = g.stbp4_decode(wx, wz, factors, owns, ITERS, ITERS, "minsum", llr_const=L, gamma_x=gq, gamma_z=gq, gamma_last_x=gq,
                                      gamma_last_z=gq)

    ms = alternate(torch, dict(dsbp4=ds, stbp4=st))
    for a, b in zip(out["dsbp4"], out["stbp4"]):
        assert torch.equal(a.reshape(b.shape), b), "R = 1 differs from fgnn_dsbp4_decode"
    res["R=1"] = dict(samples=Bw, solved=int((out["dsbp4"][4][:, 0] != 0).sum()), ms=ms, outputs_identical=True,
                      ratio=round(ms["stbp4"]["median"] / ms["dsbp4"]["median"], 3))
    # R = 3 and R = 5 on syndromes on which nothing stops
    left = np.asarray(gf2.kernel(np.asarray(c.hx, np.int64).T)[0], np.int64) % 2
    assert left.shape[0] >= 1, "hx has dependent rows: some syndromes cannot be satisfied"
    u = left[0]
    for R in (3, 5):
        ex, ez = g.pauli_noise(SEED, P, 0, Bw * R)
        fx, fz = g.syndrome(ex, ez)  # a round's difference syndrome is that of its fresh error
        bad = fx.cpu().numpy()
        flat = bad.copy()
        flat[(flat.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
        ds_x = torch.from_numpy(flat).to(g.device)
        # the window's raw syndromes: cumulative XOR of the differences, the first difference made unsatisfiable
        diff = bad.reshape(Bw, R, -1).copy()
        diff[:, 0] = flat.reshape(Bw, R, -1)[:, 0]
        raw_x = torch.from_numpy(np.bitwise_xor.accumulate(diff, axis=1)).to(g.device)
        raw_z = torch.from_numpy(np.bitwise_xor.accumulate(fz.cpu().numpy().reshape(Bw, R, -1), axis=1)).to(g.device)
        out = {}

        def ds_all():
            out["dsbp4"] = g.dsbp4_decode(ds_x, fz, factors, owns, ITERS, ITERS, "minsum", llr_const=L)

        def st_win():
            out["stbp4"] = g.stbp4_decode(raw_x, raw_z, factors, owns, ITERS, ITERS, "minsum", llr_const=L)

        ms = alternate(torch, dict(dsbp4_on_B_times_R_samples=ds_all, stbp4_windows=st_win))
        assert int((out["dsbp4"][4][:, 0] != 0).sum()) == 0 and int((out["stbp4"][4][:, 0] != 0).sum()) == 0, "nothing may stop early"
        assert int(out["stbp4"][4][:, 2].min()) == ITERS
        res[f"R={R}"] = dict(windows=Bw, dsbp4_samples=Bw * R, ms=ms,
                             ms_per_round_of_1000_windows=round(ms["stbp4_windows"]["median"] / (Bw * R) * 1000, 4),
                             ms_per_1000_dsbp4_samples=round(ms["dsbp4_on_B_times_R_samples"]["median"] / (Bw * R) * 1000, 4),
                             ratio_per_round=round(ms["stbp4_windows"]["median"] / ms["dsbp4_on_B_times_R_samples"]["median"], 3))
    return res


def part_b():
    torch, c, g = setup()
    import feedback_gnn_amd as F
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    L = llr_depolarizing(P_ROUND)
    gq = gamma_of(Q)
    R = EXPERIMENT
    res = dict(p_per_round=P_ROUND, q=Q, experiment_rounds=R, samples=B, alphas_sweep=list(ALPHA_DEFAULTS), num_iter=ITERS, gamma=gq)

    def figures(unsolved, s_hat, ls_hat):
        return dict(samples_with_an_unsolved_window=int(unsolved.sum()), nonzero_final_residual_syndrome=int((s_hat != 0).any(1).sum()),
                    logical_errors_among_zero_residual=int((~(s_hat != 0).any(1) & (ls_hat != 0).any(1)).sum()))

    for at_tag, alphas in (("one_attempt", (1.0,)), ("default_sweep", ALPHA_DEFAULTS)):
        row = {}
        for tag, window, commit in (("window_5", None, None), ("window_3_commit_1", 3, 1)):
            dec = F.SpaceTimeBP4Decoder(c, R if window is None else window, alphas=alphas, num_iter=ITERS, cn_type="minsum", factor=BASE, graph=g)
            model = F.BP4_Phenomenological_Model(c, dec, Q, R, window, commit, seed=SEED)
            s_hat, ls_hat = model(B, P_ROUND)
            unsolved = torch.zeros(B, dtype=torch.bool, device=g.device)
            for st in model.last_window_stats:
                unsolved |= st[:, 0] == 0
            row[tag] = dict(figures(unsolved, s_hat, ls_hat), launches=len(model.last_window_stats))
        # single-shot soft-syndrome BP4, round by round, the committed corrections taken out of the measured syndrome
        ex, ez, sx, sz = model.last_noise_x, model.last_noise_z, None, None
        cx, cz = ex.clone(), ez.clone()
        for t in range(1, R):
            cx[:, t] ^= cx[:, t - 1]
            cz[:, t] ^= cz[:, t - 1]
        factors, owns = mbp4_tables(alphas, BASE)
        hx_, hz_ = torch.zeros_like(ex[:, 0]), torch.zeros_like(ez[:, 0])  # the corrections committed so far
        unsolved = torch.zeros(B, dtype=torch.bool, device=g.device)
        for t in range(R):
            sx, sz = g.syndrome((cx[:, t] ^ hx_).contiguous(), (cz[:, t] ^ hz_).contiguous())  # = s_t ^ H (committed), before the flips
            sx, sz = sx ^ model.last_u_x[:, t], sz ^ model.last_u_z[:, t]
            gt = INF if t == R - 1 else gq
            xh, zh, _, _, st = g.dsbp4_decode(sx, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L, gamma_x=gt, gamma_z=gt)
            hx_, hz_ = hx_ ^ xh, hz_ ^ zh
            unsolved |= st[:, 0] == 0
        s_hat, ls_hat, _ = g.residual(cx[:, R - 1].contiguous(), cz[:, R - 1].contiguous(), hx_, hz_, want_arrays=True)
        row["dsbp4_round_by_round"] = dict(figures(unsolved, s_hat, ls_hat), launches=R)
        res[at_tag] = row
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
    out = dict(code="ghp882 [[882,24]]", B=B, seed=SEED, cn_type="minsum", base_factor=BASE)
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
