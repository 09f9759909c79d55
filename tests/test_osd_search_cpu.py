"""OSD-E / OSD-CS (include/fgnn.h, fgnn_osd) restated in NumPy, checked against brute force over the coset; the argument checks of
fgnn_osd across the C ABI.  No GPU needed: tests/test_gpu_osd_search.py holds the kernel to this restatement bit for bit."""

import numpy as np
import pytest

from feedback_gnn_amd import _lib
from feedback_gnn_amd.gf2 import kernel, rank

OSD_0, OSD_E, OSD_CS = 0, 1, 2


def sortable(x):
    """The order-preserving float32 -> uint32 map of the OSD sort key."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def eliminate(r, basis, synd):
    """Steps 1-4 of fgnn_osd0 for one sample: (order, r_sorted, reduced augmented matrix [rank, n+1], pivot of every row, and which
    rows are real pivot rows).  The pivot of a row is its first set column of the augmented row, syndrome column n included, or 0 for
    an all-zero row (tf.argmax).  A row of a rank-deficient basis that reduces to zero on H is not a real pivot row: its pivot bit is
    clear (all-zero row, pivot 0) or its pivot is column n (zero on H, syndrome bit 1: an inconsistent syndrome)."""
    r = np.asarray(r, dtype=np.float32) + np.float32(0.0)  # -0 -> +0
    order = np.argsort(sortable(r), kind="stable")
    m, n = basis.shape
    a = np.concatenate([basis[:, order], np.asarray(synd, np.uint8)[:, None]], axis=1).astype(np.uint8)
    piv = np.zeros(m, np.int64)
    for i in range(m):
        nz = np.nonzero(a[i])[0]
        p = int(nz[0]) if len(nz) else 0
        piv[i] = p
        rows = np.nonzero(a[:, p])[0]
        a[rows[rows != i]] ^= a[i]
    real = np.array([piv[i] < n and a[i, piv[i]] == 1 for i in range(m)], dtype=bool)
    return order, r[order], a, piv, real


def candidates(method, order, k):
    """[ncand, k] uint8: candidate c as a bit vector over T, in index order."""
    lam = min(order, k)
    if order == 0 or method == OSD_0:
        return np.zeros((1, k), np.uint8)
    if method == OSD_E:
        c = np.arange(1 << lam)
        C = np.zeros((len(c), k), np.uint8)
        for i in range(lam):
            C[:, i] = (c >> i) & 1
        return C
    rows = [np.zeros(k, np.uint8)]
    for j in range(k):
        v = np.zeros(k, np.uint8)
        v[j] = 1
        rows.append(v)
    for i in range(lam):
        for j in range(i + 1, lam):
            v = np.zeros(k, np.uint8)
            v[i] = v[j] = 1
            rows.append(v)
    return np.stack(rows)


def tree_cost(e_sorted, r_sorted):
    """Soft weight of each row of e_sorted [ncand, n]: the fixed-order pairwise float32 tree over NP (power of two >= n) positions."""
    ncand, n = e_sorted.shape
    NP = 1
    while NP < n:
        NP <<= 1
    x = np.zeros((ncand, NP), np.float32)
    x[:, :n] = np.where(e_sorted != 0, r_sorted[None, :], np.float32(0.0))
    h = NP // 2
    with np.errstate(over="ignore"):  # a sum may round to +-inf (FLT_MAX inputs), as on the device
        while h >= 1:
            x[:, :h] = x[:, :h] + x[:, h:2 * h]
            h //= 2
    return x[:, 0]


def osd_search(r, basis, synd, method, order, return_all=False, elim=None):
    """One sample of fgnn_osd: (e_hat in qubit order, winning candidate index).  `elim` = eliminate(r, basis, synd) if already known."""
    n = basis.shape[1]
    order_, rs, a, piv, real = eliminate(r, basis, synd) if elim is None else elim
    a, piv = a[real], piv[real]  # S and T from the real pivot rows only (osd_search_kernel step 5)
    T = np.setdiff1d(np.arange(n), piv)
    C = candidates(method, order, len(T))
    es = np.zeros((len(C), n), np.uint8)
    es[:, T] = C
    par = (C.astype(np.float64) @ a[:, T].T.astype(np.float64)).astype(np.int64) & 1  # exact: counts <= n
    es[:, piv] = (a[:, n][None, :] ^ par).astype(np.uint8)
    cost = tree_cost(es, rs)
    key = (sortable(cost).astype(np.uint64) << np.uint64(32)) | np.arange(len(C), dtype=np.uint64)
    w = int(np.argmin(key))
    e = np.zeros(n, np.uint8)
    e[order_] = es[w]
    if return_all:
        return e, w, es, cost, order_
    return e, w


def osd_search_batch(r, basis, synd, method, order, index, elims=None):
    """fgnn_osd over the samples `index`; `elims` (optional dict b -> eliminate(...)) caches the elimination across calls."""
    e = np.zeros((r.shape[0], basis.shape[1]), np.uint8)
    chosen = np.zeros(r.shape[0], np.int32)
    for b in index:
        el = None
        if elims is not None:
            el = elims.get(int(b))
            if el is None:
                el = elims[int(b)] = eliminate(r[b], basis, synd[b])
        e[b], chosen[b] = osd_search(r[b], basis, synd[b], method, order, elim=el)
    return e, chosen


def _random_full_rank(rng, m, n):
    while True:
        h = (rng.uniform(size=(m, n)) < 0.3).astype(np.uint8)
        if rank(h) == m:
            return h


def _deficient(rng, h):
    """h with dependent rows added and the rows shuffled: a duplicate row, a sum of two rows, an all-zero row.  Same row space."""
    extra = np.stack([h[-1], h[0] ^ h[1], np.zeros_like(h[0])])
    hb = np.concatenate([h, extra]).astype(np.uint8)
    return hb[rng.permutation(len(hb))]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_osd_e_at_full_order_is_the_minimum_soft_weight_of_the_coset(seed):
    _check_coset_minimum(seed, deficient=False)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_osd_e_at_full_order_is_the_minimum_soft_weight_of_the_coset_rank_deficient(seed):
    """The same row space with dependent rows added (a duplicate, a sum, an all-zero row): the zero rows are ignored, so still
    k = n - rank and 2^k candidates, exactly the coset."""
    _check_coset_minimum(seed, deficient=True)


def _check_coset_minimum(seed, deficient):
    rng = np.random.RandomState(seed)
    m, n = 12, 26
    h = _random_full_rank(rng, m, n)
    k = n - m
    r = rng.normal(1.0, 1.5, size=n).astype(np.float32)
    r[::5] = np.float32(0.75)  # ties in the sort
    if seed == 3:
        r = np.abs(r)
        r[:6] = np.float32(0.0)  # zero-weight columns: many solutions share the least cost, the tie rule decides
    err = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    hb = _deficient(rng, h) if deficient else h
    s = (hb.astype(np.int64) @ err % 2).astype(np.uint8)
    e, w, es, cost, order_ = osd_search(r, hb, s, OSD_E, k, return_all=True)
    assert len(es) == 1 << k
    assert np.array_equal(hb.astype(np.int64) @ e % 2, s)
    # brute force over the coset: e + span(kernel(H)), 2^k solutions, all different
    K = np.asarray(kernel(h)[0], dtype=np.int64) % 2
    assert K.shape == (k, n)
    coeff = (np.arange(1 << k)[:, None] >> np.arange(k)[None, :]) & 1
    coset = (e[None, :].astype(np.int64) + coeff @ K) % 2
    assert len({row.tobytes() for row in coset.astype(np.uint8)}) == 1 << k
    # the candidates are exactly the coset
    cand = np.zeros_like(es)
    cand[:, order_] = es
    assert {row.tobytes() for row in cand} == {row.tobytes() for row in coset.astype(np.uint8)}
    # the winner has the least soft weight of every solution (float64 sum: within rounding of the float32 tree) ...
    w64 = coset.astype(np.float64) @ r.astype(np.float64)
    assert abs(float(e.astype(np.float64) @ r.astype(np.float64)) - w64.min()) < 1e-4
    # ... is the least tree cost of all candidates, and the lowest index among equal costs
    assert cost[w] == cost.min() and w == int(np.nonzero(cost == cost.min())[0][0])
    assert cost[w] <= cost[0]


def test_osd_cs_candidate_count_and_order_zero_is_osd0():
    rng = np.random.RandomState(5)
    m, n = 12, 26
    h = _random_full_rank(rng, m, n)
    k = n - m
    for lam in (1, 2, 7, 14, 40):
        C = candidates(OSD_CS, lam, k)
        l = min(lam, k)
        assert len(C) == 1 + k + l * (l - 1) // 2
        assert len({row.tobytes() for row in C}) == len(C)
        assert C[1:1 + k].sum(1).tolist() == [1] * k and C[1:1 + k].argmax(1).tolist() == list(range(k))
        assert (C[1 + k:, l:] == 0).all() and (C[1 + k:].sum(1) == 2).all()
    assert len(candidates(OSD_E, 4, k)) == 16 and len(candidates(OSD_E, 40, k)) == 1 << k
    r = rng.normal(1.0, 1.5, size=n).astype(np.float32)
    s = (h.astype(np.int64) @ (rng.uniform(size=n) < 0.2) % 2).astype(np.uint8)
    # OSD-0 as bp_osd.py:14-77 states it
    order_ = np.argsort(r + np.float32(0.0), kind="stable")
    a = np.concatenate([h[:, order_], s[:, None]], axis=1)
    piv = []
    for i in range(m):
        c = int(np.argmax(a[i, :n]))
        piv.append(c)
        rows = np.nonzero(a[:, c])[0]
        a[rows[rows != i]] ^= a[i]
    e0 = np.zeros(n, np.uint8)
    e0[order_[piv]] = a[:, n]
    for method in (OSD_0, OSD_E, OSD_CS):
        e, w = osd_search(r, h, s, method, 0)
        assert w == 0 and np.array_equal(e, e0)
    e, w = osd_search(r, h, s, OSD_0, 9)
    assert w == 0 and np.array_equal(e, e0)
    # a higher order never costs more than OSD-0
    for method, order in ((OSD_E, 6), (OSD_CS, 5)):
        e, w, es, cost, _ = osd_search(r, h, s, method, order, return_all=True)
        assert cost[w] <= cost[0] and np.array_equal(h.astype(np.int64) @ e % 2, s)


@pytest.mark.parametrize("method,order,what", [
    (3, 1, b"unknown OSD method"), (-1, 1, b"unknown OSD method"), (OSD_CS, -1, b"order must be >= 0"),
    (OSD_E, 17, b"osd_e supports order <= 16"), (OSD_CS, 65, b"osd_cs supports order <= 64"), (OSD_CS, 7, b"bad OSD arguments"),
    (OSD_E, 16, b"bad OSD arguments"), (OSD_CS, 64, b"bad OSD arguments"), (OSD_0, 99, b"bad OSD arguments")])
def test_fgnn_osd_refuses_bad_arguments_with_error_codes(method, order, what):
    """No graph exists without a GPU: the last four rows (NULL graph, limits themselves accepted) reach the graph check."""
    L = _lib.lib()
    rc = L.fgnn_osd(None, 0, method, order, None, None, None, 1, None, 0, None, None, None)
    assert rc == -1 and what in L.fgnn_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_osd_decoder_method_names_and_limits():
    import feedback_gnn_amd as F
    from feedback_gnn_amd.graph import osd_method_id
    assert [osd_method_id(x) for x in ("osd0", "osd_e", "osd_cs", "OSD_CS", OSD_E)] == [0, 1, 2, 2, 1]
    d = F.OSD_Decoder(882)
    assert (d.osd_method, d.osd_order, d.method_id) == ("osd_cs", 7, OSD_CS)
    assert F.OSD_Decoder(882, "osd_e", 16).method_id == OSD_E
    for method, order in (("osd_e", 17), ("osd_cs", 65), ("osd_cs", -1), ("osd_x", 1)):
        with pytest.raises(ValueError):
            F.OSD_Decoder(882, method, order)


def _osd0_cases():
    """(name, basis) pairs: full-rank and rank-deficient random bases (dependent duplicate rows, row sums, an all-zero row)."""
    from helpers import random_sparse_basis
    rng = np.random.RandomState(21)
    out = []
    for n, m in ((7, 3), (33, 16), (65, 40), (96, 48)):
        h, _ = random_sparse_basis(n, m, seed=n)
        out.append((f"random{n}", h))
        out.append((f"deficient{n}", _deficient(rng, h)))
    h = _random_full_rank(rng, 12, 26)
    out.append(("duplicates", np.concatenate([h, h[:4], h[:2] ^ h[2:4]]).astype(np.uint8)))
    out.append(("rank1", np.tile(h[:1], (5, 1))))
    return out


@pytest.mark.parametrize("name,basis", _osd0_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_restatement_order0_equals_oracle_osd0_on_any_basis(name, basis):
    """The restatement at order 0 (real pivot rows only) is og_osd0 bit for bit on the llr_bin path, on full-rank and rank-deficient
    bases, for syndromes of errors (H e = s then holds) and for random — possibly inconsistent — syndromes."""
    from helpers import binary_oracle
    m, n = basis.shape
    og = binary_oracle(basis)
    rng = np.random.RandomState(m * 1000 + n)
    B = 48
    llr = rng.normal(1.0, 2.0, size=(B, n)).astype(np.float32)
    llr[::3, ::4] = np.float32(0.5)  # ties
    llr[1::3] = np.abs(llr[1::3]) * np.where(rng.uniform(size=(1, n)) < 0.5, np.float32(-0.0), np.float32(0.0))  # +-0
    err = (rng.uniform(size=(B, n)) < 0.15).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    synd[B // 2:] = (rng.uniform(size=(B - B // 2, m)) < 0.5).astype(np.uint8)  # random syndromes: inconsistent if rank < m
    piv = np.arange(m, dtype=np.int32)
    ref = og.osd0(0, piv, synd, llr_bin=llr)
    for method in (OSD_0, OSD_E, OSD_CS):
        e, w = osd_search_batch(llr, basis, synd, method, 0, np.arange(B))
        assert np.array_equal(e, ref), f"{name} method {method}: samples {np.nonzero((e != ref).any(1))[0][:6]} differ from og_osd0"
        assert not w.any()
    ok = (ref[:B // 2].astype(np.int64) @ basis.T % 2 == synd[:B // 2]).all(1)
    assert ok.all(), f"{name}: H e != s for an error syndrome"
    if rank(basis) < m:
        # an inconsistent syndrome: the zero rows with syndrome bit 1 write nothing, H e = s cannot hold there
        bad = ~(ref[B // 2:].astype(np.int64) @ basis.T % 2 == synd[B // 2:]).all(1)
        assert bad.any() or name == "rank1"


def test_restatement_pivot_rows_on_a_rank_deficient_basis():
    """The zero rows are exactly the dependent ones: real pivot rows = rank, pivots distinct, and the first set bit of every real row."""
    rng = np.random.RandomState(3)
    h = _random_full_rank(rng, 10, 24)
    hb = _deficient(rng, h)
    r = rng.normal(size=24).astype(np.float32)
    s = (rng.uniform(size=len(hb)) < 0.5).astype(np.uint8)
    order_, rs, a, piv, real = eliminate(r, hb, s)
    assert real.sum() == 10 and len(set(piv[real].tolist())) == 10
    for i in np.nonzero(~real)[0]:
        assert not a[i, :24].any()
        assert piv[i] == (24 if a[i, 24] else 0)
    for i in np.nonzero(real)[0]:
        assert int(np.nonzero(a[i])[0][0]) == piv[i]
        assert a[:, piv[i]].sum() == 1
