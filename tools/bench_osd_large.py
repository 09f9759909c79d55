"""OSD beyond LDS on the [[6480,1296]] hypergraph product (tests/helpers.py hp_big): BP4 (the global-memory kernel) on a batch, then
OSD-0 and OSD-CS 7 through fgnn_osd_ws on both sides of the failures.  Prints one JSON line: failure count, ms per side per method, ms
per sample, the analytic bytes the elimination moves per sample and the achieved rate against the Infinity Cache (~8.6 TB/s) and HBM
(~6 TB/s) rates, a slot-count sweep, and og_osd0 (the CPU oracle) per sample on 16 threads.

    python tools/bench_osd_large.py [--batch 256] [--p 0.03]
"""
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

from helpers import code, llr_const  # noqa: E402

from feedback_gnn_amd.graph import TannerGraph  # noqa: E402

IC_RATE, HBM_RATE = 8.6e12, 6.0e12  # bytes/s: the guide's Infinity Cache rate, achievable HBM rate


def elimination_bytes(basis, order_cols, synd):
    """Bytes the workspace kernel's elimination moves for one sample (32-bit words, as the kernel packs them): per step the row copy
    (W words read), the pivot-column word of every row (rank words read) and, per row holding the pivot, words pw..W-1 read and written."""
    m, n = basis.shape
    W = (n + 1 + 31) // 32
    a = np.zeros((m, W * 32), np.uint8)
    a[:, :n] = basis[:, order_cols]
    a[:, n] = synd & 1
    P = np.packbits(a, axis=1, bitorder="little").view("<u4").copy()
    total = 0
    for i in range(m):
        total += 4 * (W + m)
        nz = np.flatnonzero(P[i])
        if not len(nz):
            continue
        w = int(nz[0])
        x = int(P[i, w])
        b = (x & -x).bit_length() - 1
        hit = ((P[:, w] >> np.uint32(b)) & np.uint32(1)).astype(bool)
        hit[i] = False
        rows = np.flatnonzero(hit)
        total += 8 * len(rows) * (W - w)
        if len(rows):
            P[np.ix_(rows, np.arange(w, W))] ^= P[i, w:]
    return total


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--p", type=float, default=0.03)
    args = ap.parse_args()
    c = code("hp_big")
    g = TannerGraph(c)
    g.set_basis(0, c.pivot_hx)
    g.set_basis(1, c.pivot_hz)
    B, p = args.batch, args.p
    ex, ez = g.pauli_noise(0x5EED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    o = g.bp4_decode(sx, sz, 10, "minsum", 0.8, llr_const=llr_const(p), want_logits=False)
    _, _, flags = g.residual(ex, ez, o["x_hat"], o["z_hat"], want_arrays=False)
    index, nact = g.compact(flags, 1)
    res = dict(code="hp_big [[6480,1296]]", batch=B, p=p, bp4="minsum x10, factor 0.8 (GMEM kernel)", failures=nact,
               resident=dict(side0=g.osd_resident(0, "osd0"), side1=g.osd_resident(1, "osd0")))
    synd = (sx, sz)
    ms = {}
    for method, order in (("osd0", 0), ("osd_cs", 7)):
        for side in (0, 1):
            ws = g.osd_workspace(side, method, order)
            e = o["z_hat" if side == 0 else "x_hat"].clone()
            t = timed(lambda: g.osd_ws(side, synd[side], e, method, order, marg=o["llr"], index=index, nact=nact, workspace=ws))
            ms[f"{method}{order if order else ''}_side{side}"] = dict(ms=round(t, 3), ms_per_sample=round(t / max(nact, 1), 4),
                                                                    slots=g.osd_default_slots(side, method, order),
                                                                    slot_bytes=g.osd_slot_bytes(side, method, order))
    res["osd_ws"] = ms
    # analytic elimination bytes of the first failure, side 0 (the order comes from the same reliabilities the kernel sorts)
    from oracle.oracle import OracleGraph, set_num_threads
    from test_osd_search_cpu import sortable
    fail = index[:nact].cpu().numpy()
    marg = o["llr"].cpu().numpy()
    b0 = int(fail[0])
    hx = np.asarray(c.hx).astype(np.uint8)
    basis = hx[np.asarray(c.pivot_hx)]
    X, Y, Z = (marg[b0, k].astype(np.float64) for k in range(3))
    r = (np.logaddexp(0, -X) - np.logaddexp(-Z, -Y)).astype(np.float32) + np.float32(0)  # float64 stand-in for the column order only
    order_cols = np.argsort(sortable(r), kind="stable")
    nbytes = elimination_bytes(basis, order_cols, sx[b0].cpu().numpy()[np.asarray(c.pivot_hx)])
    t0 = ms["osd0_side0"]["ms"] * 1e-3
    rate = nbytes * nact / t0
    res["elimination"] = dict(bytes_per_sample=int(nbytes), achieved_bytes_per_s=float(f"{rate:.4g}"),
                              fraction_of_infinity_cache=round(rate / IC_RATE, 4), fraction_of_hbm=round(rate / HBM_RATE, 4),
                              note="analytic bytes of one sample (side 0), applied to every failure; osd0 side-0 time")
    # slot-count sweep, OSD-0 side 0
    sweep = {}
    for slots in (32, 64, 128, 256, 512):
        ws = g.osd_workspace(0, "osd0", 0, slots=slots)
        e = o["z_hat"].clone()
        sweep[str(slots)] = round(timed(lambda: g.osd_ws(0, sx, e, "osd0", 0, marg=o["llr"], index=index, nact=nact, workspace=ws)), 3)
        del ws
        torch.cuda.empty_cache()
    res["slot_sweep_osd0_side0_ms"] = sweep
    # the CPU oracle on 16 threads
    og = OracleGraph(c, forms="library-default")
    set_num_threads(16)
    k = min(16, nact)
    t = time.perf_counter()
    og.osd0(0, c.pivot_hx, sx.cpu().numpy(), marg=marg, index=fail[:k].astype(np.int32))
    res["og_osd0_ms_per_sample_16_threads"] = round((time.perf_counter() - t) * 1e3 / k, 2)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
