"""The totals and the hard decision of fgnn_vn.h against NumPy float32, bit for bit, on the CPU (no GPU).

tests/vn_rules_check.cpp runs vn_totals and vn_decide, the functions the kernels inline, on a fixed table: the rows on which a
re-associated sum or a reordered decision ladder gives another answer, and a few hundred seeded random ones.  The expected values
are float32 NumPy scalars added in the oracle's order, (Sz + Sx) + ly, and the ladder "X, then Z, then Y, strict <" written out.
Compiled with the flags the oracle is compiled with.
"""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _decide(X, Y, Z):
    d, best = 0, F(0.0)
    for val, code in ((X, 1), (Z, 2), (Y, 3)):
        if val < best:
            best, d = val, code
    return d


def _decision_rows():
    rows = [(1.0, 2.0, 3.0), (0.5, 0.5, 0.5),                                       # all positive: the identity
            (-1.0, 2.0, 3.0), (1.0, -2.0, 3.0), (1.0, 2.0, -3.0),                   # each single negative
            (-2.0, -2.0, 5.0), (-2.0, 5.0, -2.0), (5.0, -2.0, -2.0),                # pairwise ties below zero: X = Y, X = Z, Z = Y
            (-2.0, -2.0, -1.0), (-2.0, -1.0, -2.0), (-1.0, -2.0, -2.0),             # ... with the third one negative but larger
            (-2.0, -2.0, -3.0), (-2.0, -3.0, -2.0), (-3.0, -2.0, -2.0),             # ... and with the third one the smallest
            (-2.0, -2.0, -2.0),                                                     # the three-way tie: X wins
            (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 0.0, 1.0), (0.0, -0.0, -0.0),  # +0 against -0: neither is below 0
            (-0.0, -1.0, 0.0), (-1e-45, -0.0, 0.0), (0.0, -0.0, -1e-45)]            # a zero never beats a negative, a denormal does
    rng = np.random.default_rng(20240607)
    rnd = rng.standard_normal((300, 3)).astype(F) * F(8.0)
    rnd[::7, 1] = rnd[::7, 0]   # random ties too
    rnd[3::11, 2] = rnd[3::11, 0]
    rnd[5::13, 1] = rnd[5::13, 2]
    return np.concatenate([np.array(rows, dtype=F), rnd])


def _total_rows():
    rows = [(0.0, 0.0, 1.0, 2.0, 3.0), (0.0, 0.0, -1.0, 2.0, 3.0), (0.0, 0.0, 1.0, -2.0, 3.0), (0.0, 0.0, 1.0, 2.0, -3.0),
            (-0.0, -0.0, -0.0, -0.0, -0.0), (0.0, -0.0, -0.0, 0.0, -0.0), (1.5, -1.5, -1.5, 0.0, 1.5),
            # (Sz + Sx) + ly against Sz + (Sx + ly): cancellation first, or absorption first
            (1e8, -1e8, 0.0, 1.0, 0.0), (1.0, 1e8, 0.0, -1e8, 0.0), (16.635532, 2.0 ** -20, 1.0, 2.0 ** -20, 1.0),
            (3.0, 2.0 ** -23, -7.0, 2.0 ** -23, 5.0), (-49.906596, 33.271064, 3.9512436, 3.9512436, 3.9512436)]
    rng = np.random.default_rng(882024)
    rnd = (rng.standard_normal((400, 5)) * np.array([30.0, 30.0, 4.0, 4.0, 4.0])).astype(F)
    return np.concatenate([np.array(rows, dtype=F), rnd])


def _run(exe, mode, table):
    run = subprocess.run([exe, mode], input=np.ascontiguousarray(table, dtype=F).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(table)
    return [ln.split() for ln in lines]


def test_totals_and_decision_equal_numpy_float32_bitwise():
    src = os.path.join(ROOT, "tests", "vn_rules_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    dec_rows, tot_rows = _decision_rows(), _total_rows()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vn_rules_check")
        cc = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Wno-unused-function", "-I" + inc, src,
                             "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        got_dec = _run(exe, "decide", dec_rows)
        got_tot = _run(exe, "totals", tot_rows)

    seen = set()
    for (X, Y, Z), got in zip(dec_rows, got_dec):
        want = _decide(X, Y, Z)
        assert int(got[0]) == want, (X, Y, Z, got, want)
        seen.add(want)
    assert seen == {0, 1, 2, 3}
    # the tie rows by hand: X before Z before Y
    assert [int(g[0]) for g in got_dec[5:15]] == [1, 1, 2, 1, 1, 2, 2, 3, 1, 1]
    assert [int(g[0]) for g in got_dec[15:22]] == [0, 0, 0, 0, 3, 1, 2]

    reassociated = 0
    for (Sz, Sx, lx, ly, lz), got in zip(tot_rows, got_tot):
        X, Y, Z = Sz + lx, (Sz + Sx) + ly, Sx + lz
        assert all(type(t) is F for t in (X, Y, Z))
        want = [int(np.array(t, dtype=F).view(np.uint32)) for t in (X, Y, Z)]
        assert [int(h, 16) for h in got[:3]] == want, (Sz, Sx, lx, ly, lz, got, want)
        assert int(got[3]) == _decide(X, Y, Z)
        reassociated += int(np.array(Sz + (Sx + ly), dtype=F).view(np.uint32)) != want[1]
    assert reassociated >= 5, reassociated  # the table does tell the two associations apart
