"""Augmented BP4 on the GPU (fgnn_bp4aug_decode) at every bp4aug_kernel instantiation, held to the restatement
tests/bp4aug_reference.py bit for bit: x_hat and z_hat as bytes, stats as int32, no tolerance anywhere and no sample left out.  The
restatement is NumPy float32 on the oracle's transcendentals (tests/mbp4_reference.py); the marks are Philox blocks (integer
arithmetic) under one float32 compare, so nothing depends on a reduction or arrival order.  One anchor does not pass through the
restatement: with every row duplicated, a restarting attempt equals plain BP4 on the GPU graph of the doubled code.

The noise is the library's seeded depolarizing stream at the rate per code of tests/test_gpu_bp4gd.py (P_OF).  The fixed batch of 40
samples per code (pre_iter 6, attempt_iter 3, 8 attempts, density 0.3, messages kept) holds, on the restatement alone, samples solved
before any draw, samples solved after a draw and samples never solved: `mix` asserts it where a test relies on it."""
import zlib

import numpy as np
import pytest
import torch

import bp4aug_reference as AU
import test_gpu_bp4gd as TGD
from helpers import _bare_code, code, gpu_graph, llr_const, oracle_library_forms, to_gpu
from test_bp4aug_reference_cpu import GHP882_FIGURES, ghp882_figures, ghp882_reference, split
from test_bp4fb_reference_cpu import ghp882_samples

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
LDS_BUDGET = TGD.LDS_BUDGET
P_OF = TGD.P_OF
CN_TYPES = TGD.CN_TYPES
BIG_FIRST = (1 << 32) + 12345  # a sample index with a non-zero high counter word
noisy, informed_edge_channel, instantiation = TGD.noisy, TGD.informed_edge_channel, TGD.instantiation  # the dispatch rule is BP4-GD's


def bp4aug_lds_bytes(E, n, cpb, regular):
    """fgnn_bp4aug_decode: E messages, n decision bytes and the marks (n bytes on the (3,3,6) rows, E bytes in the loop) per codeword,
    each rounded up to 4 floats; a stamp per codeword and ndone."""
    area = lambda nbytes: ((nbytes + 3) // 4 + 3) & ~3  # noqa: E731
    per_cw = ((E + 3) & ~3) + area(n) + area(n if regular else E)
    return per_cw * 4 * cpb + ((cpb + 1 + 3) & ~3) * 4


def both(g, c, sx, sz, pre, att, attempts, density, factor, cn_type="minsum", restart=False, seed=SEED, first=0, ref=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (x_hat, z_hat, stats).  `ref`:
    a restatement result to compare with instead of computing it."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    xh, zh, stats = g.bp4aug_decode(to_gpu(sx), to_gpu(sz), pre, att, attempts, density, cn_type, factor, restart=restart, seed=seed,
                                    first_sample=first, **gl)
    x0, z0, s0 = ref or AU.bp4aug_decode(c, sx, sz, pre, att, attempts, density, cn_type, factor, restart=restart, seed=seed,
                                         first_sample=first, **llr)
    assert stats.dtype == torch.int32 and xh.dtype == torch.uint8 and zh.dtype == torch.uint8
    s1, x1, z1 = stats.cpu().numpy(), xh.cpu().numpy(), zh.cpu().numpy()
    print(cn_type, "density", density, "restart", restart, "found", s0[:, 0].tolist(), "a", s0[:, 1].tolist(), "k", s0[:, 3].tolist())
    bad = (s0 != s1).any(1)
    assert not bad.any(), (np.nonzero(bad)[0], s0[bad], s1[bad])
    assert x0.tobytes() == x1.tobytes() and z0.tobytes() == z1.tobytes()
    return x0, z0, s0


def mix(stats):
    """Some samples solved before any draw, some after a draw, some never: the three ways a codeword leaves the kernel."""
    return all(split(stats))


def fuzz(name, g, og, rng, cn_types=("minsum",)):
    """B in 1..70, pre_iter and attempt_iter <= 12, max_attempts 0 / 3 / 5, restart off and on, three factors, densities 0, 0.1, 0.5 and
    1, sample indices below and above 2^32, a constant prior and per-qubit LLRs with edge values.  Then the fixed batch per code."""
    p, c = P_OF[name], code(name)
    for cn in cn_types:
        for attempts, factor, restart, first, density in ((0, 1.0, False, 0, 0.5), (3, 0.8, True, BIG_FIRST, 0.1),
                                                          (5, 0.625, False, int(rng.randint(1 << 20)), 0.5), (3, 0.8, True, 7, 1.0),
                                                          (3, 0.8, False, BIG_FIRST + 1, 0.0)):
            B, pre, att = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            ex, ez, sx, sz = noisy(og, p, B, first=int(rng.randint(1 << 20)))
            kw = dict(restart=restart, first=first, seed=int(rng.randint(1 << 30)))
            both(g, c, sx, sz, pre, att, attempts, density, factor, cn, llr_const=llr_const(p), **kw)
            both(g, c, sx, sz, pre, att, attempts, density, factor, cn, llr_ch=informed_edge_channel(ex, ez, int(rng.randint(1 << 30))), **kw)
        ex, ez, sx, sz = noisy(og, p, 40)
        _, _, s0 = both(g, c, sx, sz, 6, 3, 8, 0.3, 0.8, cn, llr_const=llr_const(p))
        assert mix(s0), "the batch must hold samples solved before a draw, solved after a draw and never solved"
        if name == "ibm72" and cn == "minsum":
            assert split(s0) == (22, 9, 9)
            _, _, s1 = both(g, c, sx, sz, 6, 3, 8, 0.1, 0.8, cn, llr_const=llr_const(p))
            assert split(s1) == (22, 14, 4)
            _, _, s2 = both(g, c, sx, sz, 6, 12, 8, 0.2, 0.8, cn, restart=True, llr_const=llr_const(p))
            assert split(s2) == (22, 16, 2)
        _, _, s0 = both(g, c, sx, sz, 6, 6, 4, 0.3, 0.8, cn, restart=True, llr_ch=informed_edge_channel(ex, ez, 77))
        assert (s0[:, 0] > 0).any() and (s0[:, 1] > 0).any(), "solutions and draws must occur under per-qubit LLRs too"


# ---- both kinds of instantiation ----------------------------------------------------------------------------------------------------------
def test_regular_instantiation():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    info = g.info()
    assert (info["dv_x"], info["dv_z"], info["dc"]) == (3, 3, 6) and instantiation(g) == (3, 6)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"aug-ibm72")))


def test_force_generic_on_a_regular_graph():
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g) == (3, 6) and instantiation(g, force_generic=True) == (0, 0)
    g.force_generic(True)
    try:
        fuzz("ibm72", g, og, np.random.RandomState(17))
    finally:
        g.force_generic(False)


@pytest.mark.parametrize("cn_type", ["boxplus", "boxplus-phi"])
def test_the_two_other_rules_on_a_regular_graph(cn_type):
    g, og = gpu_graph("ibm72"), oracle_library_forms("ibm72")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("ibm72", g, og, np.random.RandomState(zlib.crc32(b"aug-ibm72" + cn_type.encode())), cn_types=(cn_type,))


@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb126"])
def test_loop_instantiation(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert instantiation(g) == (0, 0)
    fuzz(name, g, og, np.random.RandomState(zlib.crc32(b"aug-" + name.encode())))


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_loop_instantiation_toric4(cn_type):
    g, og = gpu_graph("toric4"), oracle_library_forms("toric4")
    assert instantiation(g, cn_type) == (0, 0)
    fuzz("toric4", g, og, np.random.RandomState(zlib.crc32(b"aug-toric4" + cn_type.encode())), cn_types=(cn_type,))


def test_qubit_degrees_above_eight_keep_a_mark_per_slot():
    """The over-complete GB matrices have 94 checks of each side on every qubit: far more marks than the bits of a byte."""
    g, og, c = gpu_graph("gb46_oc"), oracle_library_forms("gb46_oc"), code("gb46_oc")
    assert instantiation(g) == (0, 0) and np.asarray(c.hx).sum(0).min() > 8 and np.asarray(c.hz).sum(0).min() > 8
    _, _, sx, sz = noisy(og, 0.1, 3, first=18)
    for restart in (False, True):
        _, _, s0 = both(g, c, sx, sz, 3, 3, 4, 0.3, 0.8, restart=restart, llr_const=llr_const(0.1))
        assert restart or mix(s0)
    both(g, c, sx, sz, 3, 3, 2, 1.0, 0.8, restart=True, first=BIG_FIRST, llr_const=llr_const(0.1))


# ---- attempts, seeds, sample indices ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart,att", [(False, 3), (True, 6)])
def test_the_largest_max_attempts(restart, att):
    """max_attempts = 65 535 on steane, where the draws solve every sample of the batch within 54 attempts: the restatement with 300
    attempts solves them all, so its result is that of any larger limit."""
    g, og, c = gpu_graph("steane"), oracle_library_forms("steane"), code("steane")
    p = P_OF["steane"]
    _, _, sx, sz = noisy(og, p, 40)
    ref = AU.bp4aug_decode(c, sx, sz, 4, att, 300, 0.3, "minsum", 0.8, restart=restart, llr_const=llr_const(p))
    assert (ref[2][:, 0] == 1).all() and 5 <= ref[2][:, 1].max() < 300
    both(g, c, sx, sz, 4, att, 65535, 0.3, 0.8, restart=restart, ref=ref, llr_const=llr_const(p))


def test_seeds_and_sample_indices_choose_the_draws():
    g, og, c = gpu_graph("ibm72"), oracle_library_forms("ibm72"), code("ibm72")
    p = P_OF["ibm72"]
    _, _, sx, sz = noisy(og, p, 40)
    outs = [both(g, c, sx, sz, 6, 3, 8, 0.1, 0.8, seed=seed, first=first, llr_const=llr_const(p))
            for seed, first in ((SEED, 0), ((0xABCDEF << 32) | 7, 0), (SEED, BIG_FIRST), (SEED, BIG_FIRST - (1 << 32)))]
    for i in range(len(outs)):
        for j in range(i):
            assert not np.array_equal(outs[i][2], outs[j][2]), "another seed or another first sample (either counter word) gives other draws"
    # a shard: rows 16..39 as global samples 16.. equal the same rows of the whole batch
    both(g, c, sx[16:], sz[16:], 6, 3, 8, 0.1, 0.8, first=16, ref=tuple(o[16:] for o in outs[0]), llr_const=llr_const(p))


@pytest.mark.parametrize("cn_type", CN_TYPES)
def test_no_attempts_is_bp4gd_without_rounds_on_the_gpu(cn_type):
    g = gpu_graph("ghp882")
    B, T, p = 8, 12, 0.03
    ex, ez = g.pauli_noise(SEED, p, 0, B)
    sx, sz = g.syndrome(ex, ez)
    llr = to_gpu(informed_edge_channel(ex.cpu().numpy(), ez.cpu().numpy(), 5))
    for launch in ((0, 0), (256, 1)):
        g.set_launch(*launch)
        try:
            for kw in (dict(llr_const=llr_const(p)), dict(llr_ch=llr)):
                x0, z0, s0 = g.bp4gd_decode(sx, sz, T, 5, 0, 25.0, cn_type, 0.8, **kw)
                for restart in (False, True):
                    xh, zh, st = g.bp4aug_decode(sx, sz, T, 5, 0, 0.3, cn_type, 0.8, restart=restart, **kw)
                    assert torch.equal(xh, x0) and torch.equal(zh, z0) and torch.equal(st, s0) and not st[:, 1].any()
            assert (s0[:, 0] == 1).any()
        finally:
            g.set_launch(0, 0)


# ---- the doubled code on the GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cn_type", [("ibm72", "minsum"), ("ibm72", "boxplus-phi"), ("rsurf5", "minsum"), ("toric4", "boxplus")])
def test_every_row_duplicated_is_bp4_on_the_doubled_code(name, cn_type):
    """density 1, restart, one attempt: a sample unsolved after attempt 0 carries the x_hat, z_hat, found and k of BP4 stopped at its
    first solution (bp4gd_decode without rounds) on the GPU graph of the code with every row written twice, the syndrome bits repeated.
    Neither side of this comparison is the restatement."""
    from feedback_gnn_amd.graph import TannerGraph
    g, og, c = gpu_graph(name), oracle_library_forms(name), code(name)
    p, pre, T = P_OF[name], 4, 9
    _, _, sx, sz = noisy(og, p, 40)
    hx2, hz2, rx, rz = AU.doubled_code(c, np.ones(og.m_x + og.m_z, bool))
    assert hx2.shape[0] == 2 * og.m_x and hz2.shape[0] == 2 * og.m_z
    g2 = TannerGraph(_bare_code(hx2, hz2))
    for kw in (dict(llr_const=llr_const(p)), dict(llr_ch=to_gpu(informed_edge_channel(*noisy(og, p, 40)[:2], 9)))):
        xh, zh, st = g.bp4aug_decode(to_gpu(sx), to_gpu(sz), pre, T, 1, 1.0, cn_type, 0.8, restart=True, **kw)
        x2, z2, s2 = g2.bp4gd_decode(to_gpu(sx[:, rx].copy()), to_gpu(sz[:, rz].copy()), T, 1, 0, 25.0, cn_type, 0.8, **kw)
        x1, z1, s1 = g.bp4gd_decode(to_gpu(sx), to_gpu(sz), T, 1, 0, 25.0, cn_type, 0.8, **kw)
        late = st[:, 1] == 1
        assert int(late.sum()) >= 5
        assert torch.equal(xh[late], x2[late]) and torch.equal(zh[late], z2[late])
        assert torch.equal(st[late][:, [0, 3]], s2[late][:, [0, 3]]) and torch.equal(st[late, 2], pre + s2[late, 2])
        assert not (torch.equal(xh[late], x1[late]) and torch.equal(zh[late], z1[late])), "the code itself decodes otherwise"


# ---- several codewords per workgroup ---------------------------------------------------------------------------------------------------
def test_codewords_of_one_workgroup_stop_at_different_attempts():
    g, og, c = gpu_graph("rsurf5"), oracle_library_forms("rsurf5"), code("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    L = llr_const(P_OF["rsurf5"])
    for B in (cpb - 1, cpb, cpb + 1):
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], B)  # the same first rows for every B
        _, _, stats = both(g, c, sx, sz, 5, 3, 12, 0.3, 0.8, llr_const=L)
        first = stats[:cpb - 1]  # samples of the first workgroup
        assert mix(first) and len(set(first[:, 1].tolist())) >= 3, "the workgroup's samples must stop at different attempts"


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, og, c = gpu_graph("rsurf5"), oracle_library_forms("rsurf5"), code("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        _, _, sx, sz = noisy(og, P_OF["rsurf5"], cpb + 3, first=100)
        for restart in (False, True):
            _, _, s0 = both(g, c, sx, sz, 4, 3, 8, 0.3, 0.8, restart=restart, llr_const=llr_const(P_OF["rsurf5"]))
            assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


# ---- syndromes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ibm72", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, og, c = gpu_graph(name), oracle_library_forms(name), code(name)
    B = 9
    zx, zz = np.zeros((B, og.m_x), np.uint8), np.zeros((B, og.m_z), np.uint8)
    x0, z0, s0 = both(g, c, zx, zz, 6, 5, 4, 0.3, 0.8, llr_const=2.0)
    assert not x0.any() and not z0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 1, 1], np.int32), (B, 1)))
    xn, zn, sn = g.bp4aug_decode(None, None, 6, 5, 4, 0.3, factor=0.8, llr_const=2.0, B=B)
    assert not xn.any() and not zn.any() and np.array_equal(sn.cpu().numpy(), s0)


# ---- LDS and the packed rows ------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    """ghp1270 with two codewords per workgroup (128 threads each): 2 x 33 040 bytes of codeword state, on the (3,3,6) instantiation."""
    g, og, c = gpu_graph("ghp1270"), oracle_library_forms("ghp1270"), code("ghp1270")
    assert instantiation(g) == (3, 6)
    E = og.E_x + og.E_z
    assert bp4aug_lds_bytes(E, og.n, 1, True) <= 48 * 1024 < bp4aug_lds_bytes(E, og.n, 2, True) <= LDS_BUDGET
    assert bp4aug_lds_bytes(E, og.n, 2, True) == TGD.bp4gd_lds_bytes(E, og.n, 2) - 16 * 2, "BP4-GD's count without its keys"
    g.set_launch(128, 2)
    try:
        _, _, sx, sz = noisy(og, 0.08, 3)
        _, _, s0 = both(g, c, sx, sz, 4, 3, 3, 0.3, 0.8, llr_const=llr_const(0.08))
        assert (s0[:, 1] > 0).any()
    finally:
        g.set_launch(0, 0)


# bb1800 / bb2730: (3,3,6)-regular with packed slot offsets up to 43 196 / 65 516; bb2738: the first size without slot rows (the loop)
@pytest.mark.parametrize("name,with_rows", [("bb1800", True), ("bb2730", True), ("bb2738", False)])
def test_packed_rows_above_32k(name, with_rows):
    g, og, c = gpu_graph(name), oracle_library_forms(name), code(name)
    assert instantiation(g) == ((3, 6) if with_rows else (0, 0)) and instantiation(g, force_generic=True) == (0, 0)
    assert bp4aug_lds_bytes(og.E_x + og.E_z, og.n, 1, False) <= LDS_BUDGET
    ex, ez, sx, sz = noisy(og, 0.05, 4)
    ref = both(g, c, sx, sz, 6, 3, 3, 0.3, 0.8, llr_const=llr_const(0.05))
    assert (ref[2][:, 1] > 0).any(), "a sample must reach a draw"
    if with_rows:  # the loop on the same inputs, against the same reference outputs
        g.force_generic(True)
        try:
            both(g, c, sx, sz, 6, 3, 3, 0.3, 0.8, ref=ref, llr_const=llr_const(0.05))
        finally:
            g.force_generic(False)


def test_a_graph_beyond_the_lds_is_refused():
    g = gpu_graph("hp_big")
    need = bp4aug_lds_bytes(g.E_x + g.E_z, g.n, 1, False)
    assert need > LDS_BUDGET
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match=rf"LDS-resident augmented BP4.*{need} bytes.*limit is {LDS_BUDGET}"):
        g.bp4aug_decode(sx, sz, 3, 3, 2, 0.1, factor=0.8, llr_const=2.0)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from feedback_gnn_amd import _lib
    g = gpu_graph("ibm72")
    n = g.n
    sx = torch.zeros((2, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((2, g.m_z), dtype=torch.uint8, device=g.device)
    with pytest.raises(ValueError, match="Unknown node type"):
        g.bp4aug_decode(sx, sz, 2, 2, 1, 0.1, cn_type="sum-product")
    for pre, att in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            g.bp4aug_decode(sx, sz, pre, att, 1, 0.1)
    for attempts in (-1, 65536):
        with pytest.raises(ValueError, match="max_attempts"):
            g.bp4aug_decode(sx, sz, 2, 2, attempts, 0.1)
    for density in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            g.bp4aug_decode(sx, sz, 2, 2, 1, density)
    with pytest.raises(ValueError, match="synd_x"):
        g.bp4aug_decode(sx[:, :-1].contiguous(), sz, 2, 2, 1, 0.1)
    with pytest.raises(ValueError, match="synd_z"):
        g.bp4aug_decode(sx, sz.to(torch.int32), 2, 2, 1, 0.1)
    with pytest.raises(ValueError, match="llr_ch"):
        g.bp4aug_decode(sx, sz, 2, 2, 1, 0.1, llr_ch=torch.zeros((2, n), dtype=torch.float32, device=g.device))
    with pytest.raises(ValueError, match="B is needed"):
        g.bp4aug_decode(None, None, 2, 2, 1, 0.1)
    # the C entry point itself: density outside [0, 1], restart outside {0, 1}, an output buffer missing
    xh, zh, st = (torch.zeros((2, n), dtype=torch.uint8, device=g.device), torch.zeros((2, n), dtype=torch.uint8, device=g.device),
                  torch.zeros((2, 4), dtype=torch.int32, device=g.device))
    call = lambda density, restart, stats: _lib.lib().fgnn_bp4aug_decode(  # noqa: E731
        g.handle, 2, 0.8, 2, 2, 1, density, restart, SEED, 0, None, 2.0, sx.data_ptr(), sz.data_ptr(), 2, xh.data_ptr(), zh.data_ptr(),
        stats, None)
    for density, restart, stats, word in ((-0.1, 0, st.data_ptr(), "density"), (1.5, 0, st.data_ptr(), "density"),
                                          (float("nan"), 0, st.data_ptr(), "density"), (0.1, 2, st.data_ptr(), "restart"),
                                          (0.1, 0, None, "no output buffer")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(density, restart, stats))
    # densities 0 and 1 are allowed; an empty batch is fine and needs no buffers
    g.bp4aug_decode(sx, sz, 2, 2, 1, 0.0)
    g.bp4aug_decode(sx, sz, 2, 2, 1, 1.0)
    xh, zh, st = g.bp4aug_decode(sx[:0], sz[:0], 2, 2, 1, 0.1)
    assert tuple(xh.shape) == (0, n) and tuple(zh.shape) == (0, n) and tuple(st.shape) == (0, 4)


# ---- [[882,24]] ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [True, False])
def test_ghp882_batch(restart):
    """The batch of tests/test_bp4aug_reference_cpu.py at the default settings: identical to the restatement, and its figures."""
    g, c = gpu_graph("ghp882"), code("ghp882")
    assert instantiation(g) == (3, 6)
    _, _, sx, sz = ghp882_samples()
    xh, zh, st = both(g, c, sx, sz, 32, 32, 40, 0.1, 0.8, restart=restart, ref=ghp882_reference(restart), llr_const=llr_const(0.10))
    assert ghp882_figures(xh, zh, st) == GHP882_FIGURES[restart]


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def test_bp4_augmented_decoder_class():
    import feedback_gnn_amd as F
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    n = og.n
    dec = F.BP4AugmentedDecoder(c, pre_iter=6, attempt_iter=3, max_attempts=8, density=0.3, restart=False, seed=99, graph=gpu_graph("ibm72"))
    default = F.BP4AugmentedDecoder(c, graph=dec.graph)
    assert (default.pre_iter, default.attempt_iter, default.max_attempts, default.density, default.restart, default.cn_type,
            default.normalization_factor, default.seed) == (32, 32, 40, 0.1, True, "minsum", 0.8, SEED)
    B = 23
    ex, ez, sx, sz = noisy(og, P_OF["ibm72"], B)
    llr = np.full((B, 3, n), llr_const(P_OF["ibm72"]), F32)
    x_hat, z_hat = dec((to_gpu(llr), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64 and tuple(x_hat.shape) == (B, n) and tuple(z_hat.shape) == (B, n)
    x0, z0, s0 = AU.bp4aug_decode(c, sx, sz, 6, 3, 8, 0.3, "minsum", 0.8, restart=False, seed=99, llr_ch=llr)
    assert np.array_equal(x_hat.cpu().numpy(), x0) and np.array_equal(z_hat.cpu().numpy(), z0)
    assert dec.last_stats.dtype == torch.int32 and np.array_equal(dec.last_stats.cpu().numpy(), s0)
    assert (s0[:, 1] > 0).any()
    for kw in (dict(pre_iter=0), dict(attempt_iter=0), dict(pre_iter=2.5), dict(max_attempts=-1), dict(max_attempts=65536),
               dict(max_attempts=1.5), dict(density=-0.1), dict(density=1.5), dict(density=float("nan")), dict(cn_type="sum-product")):
        with pytest.raises(ValueError):
            F.BP4AugmentedDecoder(c, graph=dec.graph, **kw)
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((to_gpu(llr.astype(np.float64)), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="length n"):
        dec((to_gpu(llr[:, :, :-1].copy()), to_gpu(sx.T.copy()), to_gpu(sz.T.copy())))
    with pytest.raises(ValueError, match="syndrome must have shape"):
        dec((to_gpu(llr), to_gpu(sx.copy()), to_gpu(sz.T.copy())))


def _aug_model(rank=0, world_size=1, p0=None):
    import feedback_gnn_amd as F
    c = code("ibm72")
    dec = F.BP4AugmentedDecoder(c, pre_iter=6, attempt_iter=3, max_attempts=8, density=0.3, restart=False, graph=gpu_graph("ibm72"))
    return F.BP4_Augmented_Model(c, dec, p0=p0, seed=SEED, rank=rank, world_size=world_size), dec


def test_bp4_augmented_model():
    c, og = code("ibm72"), oracle_library_forms("ibm72")
    hx, hz = np.asarray(c.hx, np.int64), np.asarray(c.hz, np.int64)
    hxp, hzp = np.asarray(c.hx_perp, np.int64), np.asarray(c.hz_perp, np.int64)
    B, p = 40, P_OF["ibm72"]
    for p0 in (None, 0.05):
        model, dec = _aug_model(p0=p0)
        for call in range(2):  # the second batch decodes global samples B .. 2B - 1
            s_hat, ls_hat = model(B, p)
            ex, ez = model.last_noise_x.cpu().numpy(), model.last_noise_z.cpu().numpy()
            xh, zh, stats = model.last_x_hat.cpu().numpy(), model.last_z_hat.cpu().numpy(), model.last_stats.cpu().numpy()
            assert tuple(s_hat.shape) == (B, hz.shape[0] + hx.shape[0]) and tuple(ls_hat.shape) == (B, hxp.shape[0] + hzp.shape[0])
            ox, oz = og.pauli_noise(SEED, p, call * B, B)
            assert np.array_equal(ex, ox) and np.array_equal(ez, oz), "depolarizing noise of the seeded stream"
            sx, sz = og.syndrome(ex, ez)
            x0, z0, s0 = AU.bp4aug_decode(c, sx, sz, 6, 3, 8, 0.3, "minsum", 0.8, restart=False, seed=SEED, first_sample=call * B,
                                          llr_const=llr_const(p if p0 is None else p0))
            assert np.array_equal(xh, x0) and np.array_equal(zh, z0) and np.array_equal(stats, s0)
            assert torch.equal(dec.last_stats, model.last_stats)
            xd, zd = (ex ^ xh).astype(np.int64), (ez ^ zh).astype(np.int64)
            solved = stats[:, 0] > 0
            assert solved.any() and not solved.all() and (stats[:, 1] > 0).any()
            assert np.array_equal(s_hat.cpu().numpy(), np.concatenate([xd @ hz.T % 2, zd @ hx.T % 2], axis=1))
            assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
            assert np.array_equal(ls_hat.cpu().numpy(), np.concatenate([xd @ hxp.T % 2, zd @ hzp.T % 2], axis=1))
            assert model.last_num_unsolved == int((~solved).sum())


def test_two_ranks_decode_as_one_process():
    B = 16
    one, m0, m1 = _aug_model()[0], _aug_model(0, 2)[0], _aug_model(1, 2)[0]
    one(2 * B, P_OF["ibm72"])
    assert m0.next_sample_range(B) == (0, B) and m1.next_sample_range(B) == (B, 2 * B)
    m0(B, P_OF["ibm72"]), m1(B, P_OF["ibm72"])
    for attr in ("last_noise_x", "last_noise_z", "last_x_hat", "last_z_hat", "last_stats"):
        assert torch.equal(getattr(one, attr), torch.cat([getattr(m0, attr), getattr(m1, attr)])), attr
    assert (m1.last_stats[:, 1] > 0).any(), "the second shard must reach a draw"


def test_sim_ber_drives_the_model():
    import feedback_gnn_amd as F
    model, _ = _aug_model()
    flagged, bler = F.sim_ber(model, [0.12, 0.06], batch_size=64, max_mc_iter=3, verbose=False, early_stop=False)
    st = F.sim_ber.last
    assert (np.asarray(st["num_blocks"]) == 64 * 3).all()
    assert len(flagged) == 2 and len(bler) == 2
    assert flagged[0] > flagged[1] >= 0 and bler[0] >= flagged[0], "every unsolved sample is flagged; more of them at the higher rate"
