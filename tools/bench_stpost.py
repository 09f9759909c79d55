"""Post-processing of unsolved space-time BP4 windows (fgnn_stbp4_decode_soft, fgnn_st_window_problem / fgnn_st_window_apply,
SpaceTimePostDecoder) on the experiment of DESIGN.md section 4 "Repeated measurements": [[882,24]], min-sum at base factor 0.8, the
default alpha sweep, 64 iterations, five rounds, q = 0.01, 16 384 samples of the library's seeded Philox streams, p = 0.02 and 0.01 per
round.  Writes profiles/stpost_bench.json (or --out) and prints it as one JSON line.
    python tools/bench_stpost.py [--out FILE] [--parent-lib LIBRARY]
Each part runs in a child process of its own under a time limit (--limit seconds, default 420); a part that fails or runs out of time
ends the tool, and nothing more is started on the GPU.

(decode) Per p, on the same draws: the five-round window as it is, with LSD, with LSD and the OSD-0 fallback, and with OSD-0; sliding
    windows of three rounds that commit one, as they are and with LSD and the fallback; single-shot fgnn_dsbp4_decode round by round
    (the baseline of tools/bench_stbp4.py).  Per decoder: windows left unsolved, samples with one, samples with a non-zero final
    residual syndrome, logical errors among the others.  Per post-processing decoder: windows post-processed, windows LSD returned
    with found = 0, and the quantiles of LSD's pivots and rounds per side over the post-processed windows.  Recorded, not asserted.
(time) HIP events around 3 launches, 5 rounds after a warm-up, the variants alternating inside every round, the median round with
    the fastest and the slowest: fgnn_stbp4_decode_soft against fgnn_stbp4_decode on the inputs of the five-round window at p = 0.02,
    with identical hard outputs asserted; then every stage of the post-processing of that launch's unsolved windows on its own.
    With --parent-lib (a libfgnn_hip.so built from the parent commit) a further child process times fgnn_stbp4_decode of that library
    on the same inputs, and the ratio of the soft launch to it is written down."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = int(os.environ.get("STPOST_BENCH_B", 16384))
PS, Q, EXPERIMENT = (0.02, 0.01), 0.01, 5
ITERS, REPS, ROUNDS = 64, 3, 5
SEED = 0x5EED
BASE = 0.8
INF = float("inf")
OUT = os.path.join(ROOT, "profiles", "stpost_bench.json")


def setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stpost needs a HIP device")
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


def alternate(torch, fns):
    """{tag: spread of ms per launch}: a warm-up of every variant, then ROUNDS rounds in which the variants take turns."""
    for fn in fns.values():
        events(torch, fn, 2)
    t = {tag: [] for tag in fns}
    for _ in range(ROUNDS):
        for tag, fn in fns.items():
            t[tag].append(events(torch, fn, REPS))
    return {tag: spread(v) for tag, v in t.items()}


def llr_depolarizing(p):
    import numpy as np
    p = np.float32(p)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p) / p, dtype=np.float32))


def gamma_of(q):
    import numpy as np
    q = np.float32(q)
    return float(np.log((np.float32(1.0) - q) / q, dtype=np.float32))


def quantiles(x):
    import numpy as np
    x = np.asarray(x)
    if not len(x):
        return None
    return dict(min=int(x.min()), median=float(np.median(x)), p90=float(np.percentile(x, 90)), p99=float(np.percentile(x, 99)), max=int(x.max()))


def figures(unsolved_windows, unsolved, s_hat, ls_hat):
    return dict(unsolved_windows=int(unsolved_windows), samples_with_an_unsolved_window=int(unsolved.sum()),
                nonzero_final_residual_syndrome=int((s_hat != 0).any(1).sum()),
                logical_errors_among_zero_residual=int((~(s_hat != 0).any(1) & (ls_hat != 0).any(1)).sum()))


def part_decode(p):
    torch, c, g = setup()
    import numpy as np
    import feedback_gnn_amd as F
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    L, gq, R = llr_depolarizing(p), gamma_of(Q), EXPERIMENT
    res = dict(p_per_round=p, q=Q, experiment_rounds=R, samples=B, alphas_sweep=list(ALPHA_DEFAULTS), num_iter=ITERS, gamma=gq)
    decs = {W: F.SpaceTimeBP4Decoder(c, W, alphas=ALPHA_DEFAULTS, num_iter=ITERS, cn_type="minsum", factor=BASE, graph=g) for W in (5, 3)}
    posts = {}

    def run(tag, W, window, commit, method=None, fallback=None):
        dec = decs[W]
        calls = []
        if method is not None:
            post = posts.setdefault((W, method, fallback), F.SpaceTimePostDecoder(dec, method=method, fallback=fallback))
            inner = type(post).decode

            def recording(*a, **k):
                out = inner(post, *a, **k)
                calls.append((post.last_num_post, post.last_num_fallback, post.last_post_stats.cpu().numpy()))
                return out
            post.decode = recording
            dec = post
        model = F.BP4_Phenomenological_Model(c, dec, Q, R, window, commit, seed=SEED)
        s_hat, ls_hat = model(B, p)
        if method is not None:
            del post.decode
        unsolved = torch.zeros(B, dtype=torch.bool, device=g.device)
        for st in model.last_window_stats:
            unsolved |= st[:, 0] == 0
        row = dict(figures(model.last_num_unsolved, unsolved, s_hat, ls_hat), launches=len(model.last_window_stats))
        if method is not None:
            row["windows_post_processed"] = int(sum(cl[0] for cl in calls))
            if method == "lsd":
                st = np.concatenate([cl[2] for cl in calls], axis=1)  # [2, launches * B, 4]
                done = ((st[:, :, 0] == 0) | (st[:, :, 2] > 0)).any(0)
                row["lsd_found_0_windows"] = int((st[:, done, 0] == 0).any(0).sum())
                row["lsd_found_0_per_side"] = [int((st[s, done, 0] == 0).sum()) for s in (0, 1)]
                row["windows_to_fallback"] = int(sum(cl[1] for cl in calls))
                row["lsd_pivots"] = [quantiles(st[s, done, 3]) for s in (0, 1)]
                row["lsd_rounds"] = [quantiles(st[s, done, 1]) for s in (0, 1)]
                row["lsd_pivot_cap"] = [post.window_graph(s, W).lsd_max_pivots(0) for s in (0, 1)]
        res[tag] = row
        return model

    model = run("window_5", 5, None, None)
    run("window_5_lsd", 5, None, None, "lsd", None)
    run("window_5_lsd_osd0", 5, None, None, "lsd", "osd0")
    run("window_5_osd0", 5, None, None, "osd0", "osd0")
    run("window_3_commit_1", 3, 3, 1)
    run("window_3_commit_1_lsd_osd0", 3, 3, 1, "lsd", "osd0")
    run("window_3_commit_1_osd0", 3, 3, 1, "osd0", "osd0")
    # single-shot soft-syndrome BP4, round by round, the committed corrections taken out of the measured syndrome (bench_stbp4.py)
    ex, ez = model.last_noise_x, model.last_noise_z
    cx, cz = ex.clone(), ez.clone()
    for t in range(1, R):
        cx[:, t] ^= cx[:, t - 1]
        cz[:, t] ^= cz[:, t - 1]
    factors, owns = mbp4_tables(ALPHA_DEFAULTS, BASE)
    hx_, hz_ = torch.zeros_like(ex[:, 0]), torch.zeros_like(ez[:, 0])
    unsolved = torch.zeros(B, dtype=torch.bool, device=g.device)
    rounds_unsolved = 0
    for t in range(R):
        sx, sz = g.syndrome((cx[:, t] ^ hx_).contiguous(), (cz[:, t] ^ hz_).contiguous())
        sx, sz = sx ^ model.last_u_x[:, t], sz ^ model.last_u_z[:, t]
        gt = INF if t == R - 1 else gq
        xh, zh, _, _, st = g.dsbp4_decode(sx, sz, factors, owns, ITERS, ITERS, "minsum", llr_const=L, gamma_x=gt, gamma_z=gt)
        hx_, hz_ = hx_ ^ xh, hz_ ^ zh
        unsolved |= st[:, 0] == 0
        rounds_unsolved += int((st[:, 0] == 0).sum())
    s_hat, ls_hat, _ = g.residual(cx[:, R - 1].contiguous(), cz[:, R - 1].contiguous(), hx_, hz_, want_arrays=True)
    res["dsbp4_round_by_round"] = dict(figures(rounds_unsolved, unsolved, s_hat, ls_hat), launches=R)
    return res


def window_inputs(torch, g, p):
    """The raw syndromes [B,R,m] of the five-round experiment at p: the draws of BP4_Phenomenological_Model."""
    R = EXPERIMENT
    ex, ez = g.pauli_noise(SEED, p, 0, B * R)
    cx, cz = ex.view(B, R, g.n).clone(), ez.view(B, R, g.n).clone()
    for t in range(1, R):
        cx[:, t] ^= cx[:, t - 1]
        cz[:, t] ^= cz[:, t - 1]
    sx, sz = g.syndrome(cx.view(B * R, g.n), cz.view(B * R, g.n))
    ux, uz = g.syndrome_noise(SEED, Q, 0, B * R)
    ux, uz = ux.view(B, R, g.m_x), uz.view(B, R, g.m_z)
    ux[:, R - 1] = 0
    uz[:, R - 1] = 0
    return (sx.view(B, R, g.m_x) ^ ux).contiguous(), (sz.view(B, R, g.m_z) ^ uz).contiguous()


def part_time():
    torch, c, g = setup()
    import feedback_gnn_amd as F
    from feedback_gnn_amd import _lib
    from feedback_gnn_amd.bp_osd import _run_osd0
    from feedback_gnn_amd.mbp import ALPHA_DEFAULTS, mbp4_tables
    p, R = PS[0], EXPERIMENT
    L, gq = llr_depolarizing(p), gamma_of(Q)
    factors, owns = mbp4_tables(ALPHA_DEFAULTS, BASE)
    sx, sz = window_inputs(torch, g, p)
    kw = dict(llr_const=L, gamma_x=gq, gamma_z=gq)
    out = {}

    def plain():
        out["plain"] = g.stbp4_decode(sx, sz, factors, owns, ITERS, ITERS, "minsum", **kw)

    def soft():
        out["soft"] = g.stbp4_decode_soft(sx, sz, factors, owns, ITERS, ITERS, "minsum", **kw)

    if os.environ.get("FGNN_LIB_PATH"):  # a parent library: the plain launch alone
        return dict(library_sha256=_lib.library_sha256(), decode_ms=alternate(torch, dict(stbp4_decode=plain)))
    ms = alternate(torch, dict(stbp4_decode=plain, stbp4_decode_soft=soft))
    for a, b in zip(out["plain"], out["soft"]):
        assert torch.equal(a, b), "the hard outputs of the soft launch differ"
    res = dict(p_per_round=p, windows=B, rounds=R, launches_per_round=REPS, timing_rounds=ROUNDS, library_sha256=_lib.library_sha256(),
               decode_ms=ms, soft_over_plain=round(ms["stbp4_decode_soft"]["median"] / ms["stbp4_decode"]["median"], 4), hard_outputs_identical=True)
    xh, zh, uxh, uzh, stats, marg, gx, gz = out["soft"]
    index, nact = g.compact((stats[:, 0] == 0).to(torch.uint8), 1)
    res["unsolved_windows"] = nact
    post = F.SpaceTimePostDecoder(F.SpaceTimeBP4Decoder(c, R, alphas=ALPHA_DEFAULTS, num_iter=ITERS, factor=BASE, graph=g))
    sides = ((sx, gx, zh, uxh), (sz, gz, xh, uzh))
    wgs = [post.window_graph(s, R) for s in (0, 1)]
    prob = [g.st_window_problem(s, marg, sides[s][1], synd=sides[s][0], index=index, nact=nact) for s in (0, 1)]
    e = [torch.zeros((nact, wgs[s].n), dtype=torch.uint8, device=g.device) for s in (0, 1)]
    lst = torch.zeros((2, nact, 4), dtype=torch.int32, device=g.device)
    stages = dict(compact=lambda: g.compact((stats[:, 0] == 0).to(torch.uint8), 1))
    for s in (0, 1):
        stages[f"window_problem_side{s}"] = lambda s=s: g.st_window_problem(s, marg, sides[s][1], synd=sides[s][0], index=index, nact=nact)
        stages[f"lsd_side{s}"] = lambda s=s: wgs[s].lsd(0, prob[s][0], e[s], llr_bin=prob[s][1], stats=lst[s])
        stages[f"osd0_side{s}"] = lambda s=s: _run_osd0(wgs[s], post._ws, 0, prob[s][0], e[s], llr_bin=prob[s][1])
        stages[f"window_apply_side{s}"] = lambda s=s: g.st_window_apply(s, e[s], sides[s][2], sides[s][3], index=index, nact=nact)
    res["stage_ms"] = alternate(torch, stages)
    res["osd0_resident"] = [bool(wgs[s].osd_resident(0, "osd0")) for s in (0, 1)]
    res["window_graph"] = [dict(checks=wgs[s].m_x, bits=wgs[s].n, lsd_pivot_cap=wgs[s].lsd_max_pivots(0)) for s in (0, 1)]
    return res


PARTS = {"decode_p0.02": lambda: part_decode(PS[0]), "decode_p0.01": lambda: part_decode(PS[1]), "time": part_time}


def child(part, limit, env=None):
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part], stdout=subprocess.PIPE, text=True, timeout=limit,
                             env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"part {part} ran past its limit of {limit} s")
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
    if run.returncode != 0 or not lines:
        sys.stdout.write(run.stdout)
        raise SystemExit(f"part {part} failed with exit status {run.returncode}")
    return json.loads(lines[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--limit", type=int, default=420, help="seconds a part may take")
    ap.add_argument("--parent-lib", help="libfgnn_hip.so of the parent commit: its fgnn_stbp4_decode is timed on the same inputs")
    ap.add_argument("--part", choices=sorted(PARTS), help="run one part in this process and print its JSON (what the tool starts)")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part]()))
        return
    out = dict(code="ghp882 [[882,24]]", B=B, seed=SEED, cn_type="minsum", base_factor=BASE)
    for part in ("time", "decode_p0.02", "decode_p0.01"):  # one fresh process per GPU step; the first that fails is the last that ran
        out[part] = child(part, args.limit)
        sys.stderr.write(f"{part} done\n")
    if args.parent_lib:
        parent = child("time", args.limit, dict(os.environ, FGNN_LIB_PATH=os.path.abspath(args.parent_lib)))
        out["time"]["parent_library"] = dict(library_sha256=parent["library_sha256"], stbp4_decode_ms=parent["decode_ms"]["stbp4_decode"])
        out["time"]["soft_over_parent_plain"] = round(out["time"]["decode_ms"]["stbp4_decode_soft"]["median"]
                                                      / parent["decode_ms"]["stbp4_decode"]["median"], 4)
        out["time"]["plain_over_parent_plain"] = round(out["time"]["decode_ms"]["stbp4_decode"]["median"]
                                                       / parent["decode_ms"]["stbp4_decode"]["median"], 4)
    if B == 16384:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
