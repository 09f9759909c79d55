"""One GNN_BP4 training step on the GPU — tape forward, BCE, hand-written reverse pass — against what a user had before it: float32
torch autograd of the restatement tests/gnnbp4_reference.py on the same GPU.

[[882,24]], D = 20, H = 40, L = 2, tanh, mean, bias, T = 10, B = 256 (usage: python tools/bench_gnnbp4_train.py [B] [T]).  HIP
events, median of 10 after 3 warm-ups, the spread (min .. max) printed.  One JSON record into profiles/gnnbp4_train.json."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnnbp4_reference as R  # noqa: E402
from helpers import code as get_code  # noqa: E402
from feedback_gnn_amd import GNN_BP4  # noqa: E402
from feedback_gnn_amd.graph import GnnBp4Weights, gnnbp4_weight_shapes  # noqa: E402


def timed(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    name, cfg = "ghp882", (20, 40, 2, "mean", "tanh", True, False, 0, 0)
    c = get_code(name)
    w = R.seeded_weights(gnnbp4_weight_shapes(c, cfg), 7)
    dec = GNN_BP4(c, 20, 20, 40, 2, T, reduce_op="mean", activation="tanh", use_bias=True)
    dec.set_weights(w)
    g = dec.graph
    ex, ez, sx, sz = (torch.from_numpy(a).to(g.device) for a in R.depolarizing_noise(c, B, 1))
    hand = timed(lambda: dec.loss_and_grads((sx, sz), (ex, ez)))
    fwd_only = timed(lambda: g.gnn_bp4_decode(dec._weights, sx, sz, T))
    tg = R.Graph(c, device=g.device)
    gx, gz = (torch.from_numpy(a).float().to(g.device) for a in R.labels(c, ex.cpu().numpy(), ez.cpu().numpy()))
    tw = [torch.from_numpy(a).to(g.device).requires_grad_(True) for a in w]

    def autograd_step():
        for t in tw:
            t.grad = None
        xs, zs, _ = R.forward(tg, (20, 40, 2, 1, 1, 1), tw, sx, sz, T)
        R.loss(xs, zs, gx, gz).backward()

    base = timed(autograd_step)
    W = GnnBp4Weights(w, g.device, config=cfg, graph=g, force_general=True)
    rec = dict(code=name, config=list(cfg[:6]), B=B, T=T, hand_written_step=hand, torch_autograd_f32_step=base,
               ratio_autograd_over_hand=base["median_ms"] / hand["median_ms"], forward_only_decode=fwd_only,
               tape_bytes=g.gnn_bp4_tape_bytes(W, T, B), workspace_bytes=g.gnn_bp4_backward_workspace_bytes(W, B),
               device=torch.cuda.get_device_name(g.device))
    print(json.dumps(rec))
    out = os.path.join(ROOT, "profiles", "gnnbp4_train.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
