"""The integer kernels around the decoders (fgnn_channel.hip, `fgnn_compact`) each against dense NumPy: int64 `@` followed by `% 2`,
`np.where`, `np.cumsum` and `np.nonzero`, written as the Python reference writes them (feedback_gnn.py:305-361, misc.py:647-669).

These kernels decide which estimate a sample keeps and which samples are counted as errors; no float comparison shows a fault in them.
The inputs are seeded random bytes, not decoder outputs, so that both outcomes of every branch occur — each test asserts on its
reference that they do.  Codes: n mod 4 of 3, 1, 1, 0, 2, 2 and 32, 16, 8, 4, 1, 1 codewords per workgroup; batches of 1, one workgroup,
one workgroup plus a codeword, and 77.
"""
import numpy as np
import pytest
import torch

from feedback_gnn_amd._lib import ROWS_LX, ROWS_LZ
from helpers import code, gpu_graph, oracle_library_forms, to_gpu
from sandwich_reference import dense_flagged, dense_residual, dense_syndrome

pytestmark = pytest.mark.gpu

CPB = {"steane": 32, "surf3": 16, "rsurf5": 8, "gb48": 4, "hp_c7": 1, "ghp882": 1}
N_MOD_4 = {"steane": 3, "surf3": 1, "rsurf5": 1, "gb48": 0, "hp_c7": 2, "ghp882": 2}
CODES = list(CPB)


def _batches(name):
    return sorted({1, CPB[name], CPB[name] + 1, 77})


def _rng(name, B, salt):
    return np.random.RandomState((CODES.index(name) * 1000 + B) * 16 + salt)


def _bits(rng, shape):
    return rng.randint(0, 2, size=shape).astype(np.uint8)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", CODES)
def test_graph_geometry_is_the_one_the_cases_are_chosen_for(name):
    gg = gpu_graph(name)
    assert gg.info()["codewords_per_block"] == CPB[name] and gg.n % 4 == N_MOD_4[name]


@pytest.mark.parametrize("name", CODES)
def test_syndrome_equals_the_dense_product(name):
    og, gg = oracle_library_forms(name), gpu_graph(name)
    for B in _batches(name):
        rng = _rng(name, B, 0)
        ex, ez = _bits(rng, (B, gg.n)), _bits(rng, (B, gg.n))
        sx, sz = dense_syndrome(code(name), ex, ez)
        assert sx.shape == (B, gg.m_x) and sz.shape == (B, gg.m_z)
        if B == 77:
            assert sx.any() and not sx.all() and sz.any() and not sz.all()
        ox, oz = og.syndrome(ex, ez)
        assert np.array_equal(ox, sx) and np.array_equal(oz, sz), (name, B, "oracle")
        tx, tz = gg.syndrome(to_gpu(ex), to_gpu(ez))
        assert np.array_equal(_np(tx), sx) and np.array_equal(_np(tz), sz), (name, B, "kernel")


def _flag_inputs(name, B):
    """Estimates, the syndromes most of them reproduce, and incoming `errors` bytes from {0, 1, 2, 255}."""
    c = code(name)
    n = c.hx.shape[1]
    rng = _rng(name, B, 1)
    xh, zh = _bits(rng, (B, n)), _bits(rng, (B, n))
    sx, sz = dense_syndrome(c, xh, zh)  # (hx z_hat, hz x_hat): reproduced by construction
    flip = rng.randint(0, 3, size=B)  # 0: keep, 1: flip one bit of x_hat, 2: flip one bit of z_hat
    pos = rng.randint(0, n, size=B)
    for b in range(B):
        if flip[b] == 1:
            xh[b, pos[b]] ^= 1
        elif flip[b] == 2:
            zh[b, pos[b]] ^= 1
    errors = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=B)
    return xh, zh, sx, sz, errors


@pytest.mark.parametrize("name", CODES)
def test_flag_update_equals_the_dense_flag_test(name):
    gg = gpu_graph(name)
    for B in _batches(name):
        xh, zh, sx, sz, errors = _flag_inputs(name, B)
        bad = dense_flagged(code(name), xh, zh, sx, sz)
        want = ((errors != 0) & bad).astype(np.uint8)
        if B == 77:  # all four (incoming, bad) combinations, and every incoming byte value on both sides
            assert {(bool(e), bool(f)) for e, f in zip(errors != 0, bad)} == {(False, False), (False, True), (True, False), (True, True)}
            assert all(bad[errors == v].any() and not bad[errors == v].all() for v in (0, 1, 2, 255))
        got = _np(gg.flag_update(to_gpu(xh), to_gpu(zh), to_gpu(sx), to_gpu(sz), to_gpu(errors.copy())))
        assert np.array_equal(got, want), (name, B, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("name", CODES)
def test_merge_overwrites_exactly_the_flagged_rows(name):
    gg = gpu_graph(name)
    for B in _batches(name):
        rng = _rng(name, B, 2)
        xh, zh, xu, zu = (rng.randint(0, 256, size=(B, gg.n)).astype(np.uint8) for _ in range(4))
        errors = rng.choice(np.array([0, 1, 255], np.uint8), size=B)
        if B == 77:
            assert set(errors.tolist()) == {0, 1, 255}
        tx, tz = to_gpu(xh), to_gpu(zh)
        gg.merge(to_gpu(errors), to_gpu(xu), to_gpu(zu), tx, tz)
        wx, wz = np.where(errors[:, None] != 0, xu, xh), np.where(errors[:, None] != 0, zu, zh)
        assert np.array_equal(_np(tx), wx) and np.array_equal(_np(tz), wz), (name, B)
        keep = errors == 0
        assert np.array_equal(_np(tx)[keep], xh[keep]) and np.array_equal(_np(tz)[keep], zh[keep])


def _residual_inputs(name, B):
    """Errors and decisions of four kinds per side, drawn independently for the x and the z side: equal to the error, the error plus a
    stabilizer (a row of hx / hz), the error plus a logical operator (a row of code.lx / code.lz), random."""
    c = code(name)
    n = c.hx.shape[1]
    rng = _rng(name, B, 3)
    ex, ez = _bits(rng, (B, n)), _bits(rng, (B, n))
    xh, zh = ex.copy(), ez.copy()
    kinds = rng.randint(0, 4, size=(B, 2))
    for b in range(B):
        for side, (hat, stab, logical) in enumerate(((xh, c.hx, c.lx), (zh, c.hz, c.lz))):
            k = kinds[b, side]
            if k == 1:
                hat[b] ^= np.asarray(stab)[rng.randint(stab.shape[0])].astype(np.uint8)
            elif k == 2:
                hat[b] ^= np.asarray(logical)[rng.randint(logical.shape[0])].astype(np.uint8)
            elif k == 3:
                hat[b] = _bits(rng, n)
    return ex, ez, xh, zh, kinds


@pytest.mark.parametrize("name", CODES)
def test_residual_equals_the_dense_restatement(name):
    c, og, gg = code(name), oracle_library_forms(name), gpu_graph(name)
    for B in _batches(name):
        ex, ez, xh, zh, kinds = _residual_inputs(name, B)
        s0, l0, f0 = dense_residual(c, ex, ez, xh, zh)
        assert s0.shape == (B, gg.m_z + gg.m_x) and l0.shape == (B, gg.rows_hxp + gg.rows_hzp)
        if B == 77:
            assert {0, 2, 3} <= set(f0.tolist())
            equal = (kinds == 0).all(1)
            assert equal.any() and not f0[equal].any()  # rows that skip the row loops when no array is asked for ...
            stab = (kinds <= 1).all(1) & ~equal
            assert stab.any() and not f0[stab].any()  # ... and rows that run them and find all-zero parities
        o = og.residual(ex, ez, xh, zh)
        assert np.array_equal(o[0], s0) and np.array_equal(o[1], l0) and np.array_equal(o[2], f0), (name, B, "oracle")
        args = (to_gpu(ex), to_gpu(ez), to_gpu(xh), to_gpu(zh))
        s1, l1, f1 = gg.residual(*args)
        assert np.array_equal(_np(s1), s0) and np.array_equal(_np(l1), l0) and np.array_equal(_np(f1), f0), (name, B, "kernel")
        s2, l2, f2 = gg.residual(*args, want_arrays=False)
        assert s2 is None and l2 is None and np.array_equal(_np(f2), f0), (name, B, "flags only")


@pytest.mark.parametrize("name", CODES)
def test_residual_rows_on_the_logical_operators(name):
    """BP4_OSD_Model's check (bp_osd.py): ls_hat = [lz x_diff ; lx z_diff] on the decoder's own graph, no s_hat array."""
    c, gg = code(name), gpu_graph(name)
    for B in _batches(name):
        ex, ez, xh, zh, _ = _residual_inputs(name, B)
        _, l0, f0 = dense_residual(c, ex, ez, xh, zh, rows_x=c.lz, rows_z=c.lx)
        assert l0.shape == (B, gg.rows_lz + gg.rows_lx)
        if B == 77:
            assert {0, 3} <= set(f0.tolist()) and l0.any(0).all()
        l1, f1 = gg.residual_rows(ROWS_LZ, ROWS_LX, to_gpu(ex), to_gpu(ez), to_gpu(xh), to_gpu(zh))
        assert np.array_equal(_np(l1), l0) and np.array_equal(_np(f1), f0), (name, B)


def _count_ref(flags):
    f = flags.astype(np.int64)
    return np.array([(f & 1).sum(), ((f >> 1) & 1).sum(), f.shape[0]], np.int64)


@pytest.mark.parametrize("B", [1, 255, 257, 262144 + 513])
def test_count_flags_accumulates(B):
    """262 144 + 513 flags: more than 1024 blocks of 256, so the grid-stride loop of the block cap runs (and its last trip is partial)."""
    gg = gpu_graph("steane")
    rng = np.random.RandomState(B % 9973)
    start = np.array([5, 7, 11], np.int64)
    counts = to_gpu(start.copy())
    fa, fb = (rng.randint(0, 4, size=B).astype(np.uint8) for _ in range(2))
    gg.count_flags(to_gpu(fa), counts)
    assert np.array_equal(_np(counts), start + _count_ref(fa))
    gg.count_flags(to_gpu(fb), counts)
    assert np.array_equal(_np(counts), start + _count_ref(fa) + _count_ref(fb))
    if B > 1:
        assert 0 < _count_ref(fa)[0] < B and 0 < _count_ref(fa)[1] < B and _count_ref(fa)[0] != _count_ref(fa)[1]


@pytest.mark.parametrize("k,batch", [(1, 1), (3, 255), (5, 1000)])
def test_count_flags_batches_equals_the_cumulative_sums(k, batch):
    gg = gpu_graph("steane")
    rng = np.random.RandomState(100 * k + batch)
    flags = rng.randint(0, 4, size=k * batch).astype(np.uint8)
    start = np.array([3, 1, 4], np.int64)
    per = np.stack([_count_ref(flags[j * batch:(j + 1) * batch]) for j in range(k)])
    want = start + np.cumsum(per, axis=0)
    counts = to_gpu(start.copy())
    ring = torch.full((k, 3), -1, dtype=torch.int64, device=gg.device)
    gg.count_flags_batches(to_gpu(flags), batch, counts, ring)
    assert np.array_equal(_np(ring), want)
    assert np.array_equal(_np(counts), want[-1])
    seq = to_gpu(start.copy())
    for j in range(k):
        gg.count_flags(to_gpu(flags[j * batch:(j + 1) * batch]), seq)
        assert np.array_equal(_np(seq), want[j])


@pytest.mark.parametrize("bit", [1, 2])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_compact_lists_exactly_the_masked_samples(B, bit):
    gg = gpu_graph("steane")
    rng = np.random.RandomState(7 * B + bit)
    other = 3 - bit
    masks = {"none": rng.choice(np.array([0, other], np.uint8), size=B), "all": rng.choice(np.array([bit, 3], np.uint8), size=B),
             "some": np.where(rng.random_sample(B) < 0.3, rng.choice(np.array([bit, 3], np.uint8), size=B),
                              rng.choice(np.array([0, other], np.uint8), size=B)).astype(np.uint8)}
    for what, mask in masks.items():
        want = np.nonzero(mask & bit)[0]
        assert len(want) == {"none": 0, "all": B}.get(what, len(want))
        if what == "some" and B >= 255:
            assert 0 < len(want) < B and (mask & other).any()
        index, count = gg.compact(to_gpu(mask), bit=bit)
        assert count == len(want), (what, B, bit)
        got = _np(index)[:count]
        assert len(set(got.tolist())) == count, (what, "duplicates")
        assert np.array_equal(np.sort(got), want), (what, B, bit)


@pytest.mark.parametrize("first", [0, 2**32 - 2])
@pytest.mark.parametrize("name,wt,B", [("steane", 0, 5), ("steane", 7, 5), ("surf3", 5, 9), ("gb48", 1, 6), ("hp_c7", 37, 3), ("ghp882", 4, 1)])
def test_pauli_noise_wt_equals_the_oracle(name, wt, B, first):
    """Fixed-weight noise (pauli.py:80-97) at (n, wt, B) = (7,0,5), (7,7,5), (13,5,9), (48,1,6), (98,37,3), (882,4,1), from sample 0 and
    from a first sample two below 2^32 (the 64-bit sample counter carries into its high word inside the batch, or right after it)."""
    og, gg = oracle_library_forms(name), gpu_graph(name)
    seed = 0x5EED
    ox, oz = og.pauli_noise_wt(seed, wt, first, B)
    assert ((ox | oz).sum(1) == wt).all() and ox.max(initial=0) <= 1 and oz.max(initial=0) <= 1
    gx, gz = gg.pauli_noise_wt(seed, wt, first, B)
    assert np.array_equal(_np(gx), ox) and np.array_equal(_np(gz), oz)
    assert ((_np(gx) | _np(gz)).sum(1) == wt).all()
    if first and B >= 3 and 0 < wt < gg.n:  # samples 2^32, 2^32 + 1, ... are not samples 0, 1, ... again (a counter cut to 32 bits)
        lo = og.pauli_noise_wt(seed, wt, 0, B - 2)
        assert not (np.array_equal(lo[0], ox[2:]) and np.array_equal(lo[1], oz[2:]))
