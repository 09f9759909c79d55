"""LSD-0 with synchronous growth on the CPU: the NumPy restatement of tests/lsd_reference.py against the properties the contract of
`fgnn_lsd` (include/fgnn.h) promises, and the kernel's sequential step (feedback_gnn_amd/csrc/fgnn_lsd.h) walked by the host program
tests/lsd_check.cpp against the restatement, plain and under the sanitizers.  No GPU."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from feedback_gnn_amd import _lib
from feedback_gnn_amd.gf2 import rank as gf2_rank
from helpers import code, random_sparse_basis
from lsd_reference import Matrix, keys, lsd_batch, lsd_decode, sortable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reliabilities(rng, B, n):
    """Seeded reliabilities with ties (every fifth bit), a -0.0 and a +0.0 that must tie, and negative values."""
    r = rng.normal(1.0, 2.5, size=(B, n)).astype(np.float32)
    r[:, ::5] = np.float32(0.75)
    r[:, 1] = np.float32(-0.0)
    r[:, 3 % n] = np.float32(0.0)
    return r


def seeded_errors(rng, B, n, p):
    e = (rng.random((B, n)) < p).astype(np.uint8)
    e[0] = 0
    e[0, n // 2] = 1  # a single error, whatever p
    return e


def test_sortable_orders_floats_and_ties_the_zeros():
    r = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.75, 2.0, np.inf], np.float32)
    s = sortable(r).astype(np.int64)
    assert (np.diff(s) >= 0).all() and s[3] == s[4] and len(set(s.tolist())) == len(r) - 1
    k = keys(np.array([0.5, -0.0, 0.0, 0.5], np.float32))
    assert sorted(range(4), key=lambda v: k[v]) == [1, 2, 0, 3], "ties go to the lower bit index"


@pytest.mark.parametrize("name,p,B", [("steane", 0.15, 12), ("toric4", 0.1, 12), ("gb126", 0.04, 8), ("ghp882", 0.01, 6)])
@pytest.mark.parametrize("side", [0, 1])
def test_every_syndrome_of_an_error_is_solved_without_caps(name, p, B, side):
    c = code(name)
    H = np.asarray(c.hx if side == 0 else c.hz).astype(np.uint8)
    m, n = H.shape
    rng = np.random.default_rng(100 + side)
    err = seeded_errors(rng, B, n, p)
    synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    r = reliabilities(rng, B, n)
    e, stats = lsd_batch(Matrix(H), synd, r)
    assert (stats[:, 0] == 1).all(), stats
    assert np.array_equal(e.astype(np.int64) @ H.T % 2, synd), "H e != s"
    assert (stats[:, 3] <= stats[:, 2]).all() and (stats[:, 3] <= min(m, n)).all()
    zero = synd.sum(1) == 0
    assert (stats[zero] == [1, 0, 0, 0]).all() and not e[zero].any()
    assert (stats[~zero, 1] >= 1).all()


def _toric():
    H = np.asarray(code("toric4").hx).astype(np.uint8)
    assert gf2_rank(H) == H.shape[0] - 1, "the rows of the checkerboard toric code's hx have one dependency"
    return H


def _far_defects(H):
    """Two checks of H that share no bit."""
    m = H.shape[0]
    for a in range(m):
        for b in range(a + 1, m):
            if not (H[a] & H[b]).any():
                return a, b
    raise AssertionError("no two disjoint checks")


def test_a_single_defect_outside_the_image_dies():
    H = _toric()
    m, n = H.shape
    s = np.zeros(m, np.uint8)
    s[2] = 1
    tr = {}
    e, (found, rounds, columns, pivots) = lsd_decode(H, s, np.ones(n, np.float32), trace=tr)
    assert found == 0 and len(tr["dead"]) == 1 and 1 <= rounds <= n + 1
    assert columns == n and pivots == gf2_rank(H), "the component grew until it was whole"
    assert len({l for l in tr["lab"] if l >= 0}) == 1 and min(tr["lab"]) == 0, "one cluster, labelled by its smallest check"


def test_two_defects_are_solved_and_the_caps_are_honoured():
    H = _toric()
    m, n = H.shape
    a, b = _far_defects(H)
    s = np.zeros(m, np.uint8)
    s[[a, b]] = 1
    r = np.ones(n, np.float32)
    e, (found, rounds, columns, pivots) = lsd_decode(H, s, r)
    assert found == 1 and pivots >= 2 and rounds >= 1
    assert np.array_equal(H.astype(np.int64) @ e % 2, s)
    e1, st1 = lsd_decode(H, s, r, max_pivots=1)
    assert st1[0] == 0 and st1[3] == 1 and st1[2] >= 2, st1  # the column that hits the cap is counted
    assert e1.sum() <= 1, "the read-out of the one pivot there is"
    for cap in range(1, rounds):
        ec, stc = lsd_decode(H, s, r, max_rounds=cap)
        assert stc[1] == cap and stc[0] == 0, (cap, stc)
    assert lsd_decode(H, s, r, max_rounds=rounds)[1] == [1, rounds, columns, pivots]


def _independent_in_order(H, order):
    """The columns a plain Gaussian elimination over H[:, order], taken in that order, finds independent of the ones before."""
    basis, picked = {}, []  # leading bit -> reduced vector
    for v in order:
        x = sum(1 << int(c) for c in np.nonzero(H[:, v])[0])
        while x:
            lead = x.bit_length() - 1
            if lead not in basis:
                basis[lead] = x
                picked.append(v)
                break
            x ^= basis[lead]
    return picked


@pytest.mark.parametrize("name", ["toric4", "steane"])
def test_the_pivot_columns_are_those_of_a_plain_elimination_in_append_order(name):
    H = np.asarray(code(name).hx).astype(np.uint8)
    m, n = H.shape
    rng = np.random.default_rng(7)
    s = np.zeros(m, np.uint8)
    s[0] = 1
    if gf2_rank(np.c_[H, s]) == gf2_rank(H):  # make the syndrome unreachable, so that the cluster grows until the component is whole
        H = np.r_[H, H[:1]]                   # a repeated row with a contradicting syndrome bit
        s = np.r_[s, np.zeros(1, np.uint8)]
        m += 1
    tr = {}
    _, (found, rounds, columns, pivots) = lsd_decode(H, s, rng.normal(size=n).astype(np.float32), trace=tr)
    assert found == 0 and len({l for l in tr["lab"] if l >= 0}) == 1 and columns == n == len(tr["appended"])
    assert tr["col"] == _independent_in_order(H, tr["appended"]) and pivots == gf2_rank(H)
    assert len(set(tr["piv"])) == pivots


# ---- the header's sequential step, walked on the host ------------------------------------------------------------------------------
def _case(H, synd, r, max_pivots, max_rounds):
    return dict(H=H, synd=synd, r=r, max_pivots=max_pivots, max_rounds=max_rounds)


def header_cases():
    """Word edges m = 31, 32, 33, 64, 65 (n = 2 m, dependent columns; a third of the samples under a pivot or a round cap) and one
    shape of more than 64 words."""
    cases = []
    for m in (31, 32, 33, 64, 65):
        H, _ = random_sparse_basis(2 * m, m, seed=m)
        rng = np.random.default_rng(m)
        B = 9
        err = (rng.random((B, 2 * m)) < np.linspace(0.02, 0.5, B)[:, None]).astype(np.uint8)
        synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
        r = reliabilities(rng, B, 2 * m)
        cases.append(_case(H, synd, r, 0, 0))
        cases.append(_case(H, synd[6:], r[6:], m // 4, 0))
        cases.append(_case(H, synd[6:], r[6:], 0, 2))
    m = 2100  # W = 66
    H, _ = random_sparse_basis(2 * m, m, seed=5)
    rng = np.random.default_rng(5)
    err = (rng.random((3, 2 * m)) < np.array([0.001, 0.004, 0.01])[:, None]).astype(np.uint8)
    err[:, -1] = 1  # a column whose checks may lie in the last words
    synd = (err.astype(np.int64) @ H.T % 2).astype(np.uint8)
    cases.append(_case(H, synd, reliabilities(rng, 3, 2 * m), 0, 0))
    return cases


def write_cases(path, cases):
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for c in cases:
            H, synd, r = c["H"], c["synd"], c["r"]
            m, n = H.shape
            f.write(f"{m} {n} {c['max_pivots']} {c['max_rounds']} {len(synd)}\n")
            for row in H:
                vs = np.nonzero(row)[0]
                f.write(" ".join(map(str, [len(vs), *vs])) + "\n")
            for b in range(len(synd)):
                f.write(" ".join(map(str, synd[b])) + "\n")
                f.write(" ".join(map(str, sortable(r[b]))) + "\n")


@pytest.fixture(scope="module")
def header_reference():
    cases = header_cases()
    want = []
    for c in cases:
        e, stats = lsd_batch(Matrix(c["H"]), c["synd"], c["r"], c["max_pivots"], c["max_rounds"])
        want += ["".join(map(str, e[b])) + " | " + " ".join(map(str, stats[b])) for b in range(len(e))]
    founds = [int(w.split("|")[1].split()[0]) for w in want]
    assert 0 in founds and 1 in founds, "both outcomes must occur"
    return cases, want


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_walk_of_the_header_equals_the_restatement(flags, header_reference):
    cases, want = header_reference
    src = os.path.join(ROOT, "tests", "lsd_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "lsd_check"), os.path.join(tmp, "cases.txt")
        cc = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-function"] + flags + ["-I" + inc, src, "-o", exe],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0, cc.stdout
        write_cases(data, cases)
        run = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"sample {i}: stats {g.split('|')[1]} != {w.split('|')[1]}" if g.split("|")[1] != w.split("|")[1] else f"sample {i}: e_hat"


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_shim_binds_both_entry_points():
    text = open(os.path.join(ROOT, "include", "fgnn.h")).read()
    for name in ("fgnn_lsd_max_pivots", "fgnn_lsd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS and name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["fgnn_lsd"][1]) == 13 and len(_lib._SIGNATURES["fgnn_lsd_max_pivots"][1]) == 3
    mk = open(os.path.join(ROOT, "feedback_gnn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfgnn_lsd\.hip\b", mk, flags=re.M) and re.search(r"^HDRS :=.*\bfgnn_lsd\.h\b", mk, flags=re.M)


def test_argument_errors_come_back_as_codes_without_a_gpu():
    L = _lib.lib()
    cap = ctypes.c_int(-5)
    assert L.fgnn_lsd_max_pivots(None, 0, ctypes.byref(cap)) == -1 and cap.value == -5
    assert b"LSD" in L.fgnn_last_error()
    assert L.fgnn_lsd(None, 0, None, None, None, 1, None, 0, 0, 0, None, None, None) == -1
    with pytest.raises(ValueError):
        _lib.check(-1)
    assert L.fgnn_version() == 2
