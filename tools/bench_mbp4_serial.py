"""MBP4 / AMBP4 in the serial schedule (fgnn_mbp4_decode_serial, AMBP4Decoder(schedule="serial")) on [[882,24]] under depolarizing
noise at p = 0.10, B = 16 384: the setting, the seeded samples and the comparison set of tools/bench_mbp4.py.  Writes
profiles/mbp4_serial_bench.json and prints it as one JSON line.
    python tools/bench_mbp4_serial.py
    make -C feedback_gnn_amd/csrc -j16 OUT=../lib/ab_per_qubit EXTRA=-DFGNN_MBP4_SERIAL_MAP=1      # the library of the other thread mapping
    MBP4_SERIAL_AB_LIB=feedback_gnn_amd/lib/ab_per_qubit/libfgnn_hip.so python tools/bench_mbp4_serial.py

Timing: HIP events around 3 launches, 5 rounds after a warm-up; the median round is reported with the fastest and the slowest.

(a) What an iteration costs: one attempt of 32 iterations (min-sum, factor 0.8, own 1) on syndromes no error produces, so that no
    sample stops early, in the serial schedule on the greedy layers and in the flooding schedule (fgnn_mbp4_decode); ms per batch, ms
    per iteration and their ratio.  Then the serial launch at several threads per codeword (fgnn_graph_set_launch); all must give the
    bytes of the default launch.  The thread mapping of the kernel is a compile-time choice (FGNN_MBP4_SERIAL_MAP): with
    MBP4_SERIAL_AB_LIB naming a library built with the other value, a child process repeats (a) on it and its figures are recorded
    next to these, with a comparison of the outputs.
(b) Decoders on the same samples: serial alpha 1.0 alone (64 iterations), the serial alpha sweep with restart and with the messages
    kept, the flooding sweep both ways, min-sum-64 BP4 in the check-layered schedule, and the decoders tools/bench_mbp4.py lists.  Per
    decoder: ms per batch from the seeded samples to the estimate, the samples left without a solution and the logical errors."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import feedback_gnn_amd as F  # noqa: E402
from bench_mbp4 import B, P, REPS, ROUNDS, SEED, events, llr_depolarizing, rate, spread  # noqa: E402
from feedback_gnn_amd import gf2  # noqa: E402
from feedback_gnn_amd.graph import TannerGraph  # noqa: E402
from helpers import code  # noqa: E402

ITERS_A, ITERS_B = 32, 64
TPCS = (64, 128, 192, 256, 384, 512, 1024)
OUT = os.path.join(ROOT, "profiles", "mbp4_serial_bench.json")


def digest(out):
    h = hashlib.sha256()
    for t in out:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def part_a(c):
    g = TannerGraph(c, stage_one=False)
    hx = np.asarray(c.hx, np.int64)
    u = (np.asarray(gf2.kernel(hx.T)[0], np.int64) % 2)[0]
    sx, sz = g.syndrome(*g.pauli_noise(SEED, P, 0, B))
    sx = sx.cpu().numpy()
    sx[(sx.astype(np.int64) @ u) % 2 == 0, int(np.nonzero(u)[0][0])] ^= 1  # u . s = 1: outside the column space of hx
    sx = torch.from_numpy(sx).to(g.device)
    L = llr_depolarizing(P)
    out = {}

    def flooding():
        out["flooding"] = g.mbp4_decode(sx, sz, [0.8], [1.0], ITERS_A, 4, "minsum", llr_const=L)

    def serial():
        out["serial"] = g.mbp4_decode_serial(sx, sz, [0.8], [1.0], ITERS_A, 4, "minsum", llr_const=L)

    fns = dict(flooding=flooding, serial=serial)
    for fn in fns.values():
        events(fn, 2)
    for tag in fns:
        st = out[tag][2]
        assert int((st[:, 0] != 0).sum()) == 0 and int((st[:, 3] != ITERS_A).sum()) == 0, "no sample may stop early"
    t = {tag: [] for tag in fns}
    for _ in range(ROUNDS):
        for tag, fn in fns.items():
            t[tag].append(events(fn, REPS))
    ms = {tag: spread(v) for tag, v in t.items()}
    ref = digest(out["serial"])
    res = dict(iterations=ITERS_A, layers=g.qubit_layers()[0], flooding_ms=ms["flooding"], serial_ms=ms["serial"],
               flooding_ms_per_iteration=round(ms["flooding"]["median"] / ITERS_A, 4),
               serial_ms_per_iteration=round(ms["serial"]["median"] / ITERS_A, 4),
               ratio=round(ms["serial"]["median"] / ms["flooding"]["median"], 2), serial_output_sha256=ref, threads_per_codeword={})
    for tpc in TPCS:
        g.set_launch(tpc, 1)
        events(serial, 2)
        same = digest(out["serial"]) == ref
        res["threads_per_codeword"][str(tpc)] = dict(ms=spread([events(serial, REPS) for _ in range(ROUNDS)]), outputs_identical=same)
    g.set_launch(0, 0)
    res["launches_per_round"], res["rounds"] = REPS, ROUNDS
    return res


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

    def ambp_run(tag, **kw):
        dec = F.AMBP4Decoder(c, graph=g, **kw)
        models[tag] = F.BP4_AMBP_Model(c, dec, seed=SEED)
        cfg = dict(alphas=list(dec.alphas), num_iter=dec.num_iter, cn_type=dec.cn_type, factor=dec.factor, restart=dec.restart,
                   schedule=dec.schedule)
        return tag, model_run(models[tag]), cfg

    def fb_run(tag, rule):
        dec = F.BP4FeedbackDecoder(c, rule, graph=g, seed=SEED)
        return tag, model_run(F.BP4_Feedback_Model(c, dec, seed=SEED)), dict(rule=rule, max_attempts=dec.max_attempts, strength=dec.strength)

    gd = F.BP4_GD_Model(c, F.BP4GDDecoder(c, graph=g), seed=SEED)
    relay = F.BP4_Relay_Model(c, F.RelayBP4Decoder(c, graph=g), seed=SEED)
    osd = F.BP4_OSD_Model(c, F.QLDPCBPDecoder(c, cn_type="minsum", num_iter=100, normalization_factor=0.8), F.OSD0_Decoder(c.N), seed=SEED)

    def bp4_run(decode):
        def run():
            ex, ez = g.pauli_noise(SEED, P, 0, B)
            sx, sz = g.syndrome(ex, ez)
            o = decode(sx, sz, ITERS_B, "minsum", 0.8, llr_const=L, want_logits=False)
            s_hat, _, _ = g.residual(ex, ez, o["x_hat"], o["z_hat"], want_arrays=True)
            return o["x_hat"], o["z_hat"], int(s_hat.any(1).sum().item())
        return run

    def run_osd():
        osd._next = 0
        o = osd.decode(B, P)
        return o["x_hat"], o["z_hat"], osd.last_num_osd

    bp4_cfg = dict(cn_type="minsum", num_iter=ITERS_B, normalization_factor=0.8)
    runs = (ambp_run("serial_alpha_1", schedule="serial", alphas=(1.0,)), ambp_run("serial_sweep_restart", schedule="serial", restart=True),
            ambp_run("serial_sweep_messages_kept", schedule="serial", restart=False),
            ambp_run("flooding_sweep_restart", restart=True), ambp_run("flooding_sweep_messages_kept", restart=False),
            ("bp4_minsum_64_check_layered", bp4_run(g.bp4_decode_layered), dict(bp4_cfg, layers=None)),
            ("bp4_minsum_64_flooding", bp4_run(g.bp4_decode), bp4_cfg),
            fb_run("bp4fb_perturb_default", "perturb"), fb_run("bp4fb_enhanced_default", "enhanced"),
            ("bp4gd_default", model_run(gd), {}), ("bp4_osd0", run_osd, dict(cn_type="minsum", num_iter=100, normalization_factor=0.8)),
            ("relay4_default", model_run(relay), {}))
    ex, ez = g.pauli_noise(SEED, P, 0, B)  # the samples every decoder draws
    res = {}
    for tag, fn, cfg in runs:
        x_hat, z_hat, uns = fn()  # warm-up, and the figures
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)
        key = "bp_unsolved" if tag == "bp4_osd0" else "unsolved"
        res[tag] = {"config": cfg, key: int(uns), "logical": rate(int((flags != 0).sum().item()), B)}
        if tag in models:
            st = models[tag].last_stats
            solved = st[:, 0] == 1
            res[tag]["solved_per_alpha"] = [int((solved & (st[:, 1] == a)).sum().item()) for a in range(len(cfg["alphas"]))]
            res[tag]["max_iterations"], res[tag]["mean_iterations"] = int(st[:, 2].max().item()), float(st[:, 2].float().mean().item())
        torch.cuda.synchronize()
    res["bp4_minsum_64_check_layered"]["config"]["layers"] = g.layers()[0]
    t = {tag: [] for tag, _, _ in runs}
    for _ in range(ROUNDS):
        for tag, fn, _ in runs:
            t[tag].append(events(fn, REPS))
    for tag, _, _ in runs:
        res[tag]["batch_ms"] = spread(t[tag])
    res["launches_per_round"], res["rounds"] = REPS, ROUNDS
    return res


def other_mapping(lib):
    """(a) on the library at `lib` (the other FGNN_MBP4_SERIAL_MAP), in a fresh process: one process binds one library."""
    env = dict(os.environ, FGNN_LIB_PATH=os.path.abspath(lib), MBP4_SERIAL_BENCH_PARTS="a")
    env.pop("MBP4_SERIAL_AB_LIB")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if res.returncode != 0:
        raise SystemExit("the run on " + lib + " failed")
    return json.loads(res.stdout.strip().split("\n")[-1])["a"]


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mbp4_serial needs a HIP device")
    c = code("ghp882")
    parts = os.environ.get("MBP4_SERIAL_BENCH_PARTS", "ab")
    ab_lib = os.environ.get("MBP4_SERIAL_AB_LIB")
    out = dict(code="ghp882 [[882,24]]", p=P, B=B, seed=SEED, device=torch.cuda.get_device_name(0))
    if "a" in parts:
        out["a"] = part_a(c)
        if ab_lib:
            torch.cuda.synchronize()
            out["a_other_mapping"] = dict(other_mapping(ab_lib), library=os.path.relpath(os.path.abspath(ab_lib), ROOT))
            out["a_other_mapping"]["outputs_identical"] = out["a_other_mapping"]["serial_output_sha256"] == out["a"]["serial_output_sha256"]
    if "b" in parts:
        out["b"] = part_b(c)
    line = json.dumps(out)
    if parts == "ab" and B == 16384:
        with open(OUT, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
