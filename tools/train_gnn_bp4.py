"""Train a GNN_BP4 decoder on depolarizing noise on the GPU (training.train_gnn_bp4: tape forward, BCE, hand-written reverse pass,
Adam) and save its weights with write_weight_list.

usage: python tools/train_gnn_bp4.py [--code gb48] [--dims 20] [--hidden 40] [--layers 2] [--reduce mean] [--activation tanh]
       [--no-bias] [--iters 3] [--p 0.05] [--batch 64] [--steps 100] [--lr 1e-2] [--seed 1] [--loss-from 0] [--out PATH.npz]
The start is glorot kernels, ones biases and a small random _llr_inv_embed kernel: with Keras' zero kernel every upstream gradient is
zero.  The saved list is in get_weights() order: GNN_BP4.set_weights(read_weight_list(PATH)) accepts it."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", default="gb48")
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=40)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reduce", default="mean", choices=["sum", "mean"])
    ap.add_argument("--activation", default="tanh")
    ap.add_argument("--no-bias", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--loss-from", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from helpers import code as get_code
    from feedback_gnn_amd import GNN_BP4
    from feedback_gnn_amd.training import train_gnn_bp4
    from feedback_gnn_amd.weights_io import read_weight_list, write_weight_list
    dec = GNN_BP4(get_code(a.code), a.dims, a.dims, a.hidden, a.layers, a.iters, reduce_op=a.reduce, activation=a.activation,
                  use_bias=not a.no_bias, seed=a.seed)
    w = dec.get_weights()
    k = [i for i, x in enumerate(w) if x.ndim == 2 and x.shape[1] == 3][-1]
    w[k] = np.random.RandomState(a.seed).uniform(-0.5, 0.5, size=w[k].shape).astype(np.float32)
    dec.set_weights(w)
    every = max(1, a.steps // 10)
    hist = train_gnn_bp4(dec, a.p, a.batch, a.steps, a.lr, a.seed, loss_from=a.loss_from,
                         on_step=lambda i, l: print(f"step {i + 1}/{a.steps} loss {l:.4f}") if (i + 1) % every == 0 else None)
    out = a.out or f"gnnbp4_{a.code}.npz"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    write_weight_list(dec.get_weights(), out)
    dec.set_weights(read_weight_list(out))  # the file is a weight list the decoder accepts
    print(f"loss {np.mean(hist[:5]):.4f} (first five steps) -> {np.mean(hist[-5:]):.4f} (last five); weights in {out}")


if __name__ == "__main__":
    main()
