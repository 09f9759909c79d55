"""Binary syndrome BP (fgnn_bp2_decode) on the GPU at every bp2_kernel<CN_TYPE, DV, DC> instantiation and launch-time branch, held to the
CPU oracle og_bp2_decode bit for bit (soft outputs compared as int32 views, hard decisions as bytes): regular (3,6) / (4,8) graphs other
than ghp882 and gb48, runtime-degree graphs with check degree up to 8, 9-16 and above 16, irregular graphs with degree-1 checks and
edge-free bits, several codewords per workgroup, the B <= 256 widening, one to 40 checks per thread (syndrome in a register or re-read
from global memory), dynamic LDS above 48 KiB, both sides of the LDS refusal, the factor == 1 shortcut, soft-only / hard-only calls, a
null syndrome and the edge inputs of tests/test_bp2_reference_cpu.py; and bsc_noise against og_bsc_noise."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from feedback_gnn_amd import codes_q as cq
from feedback_gnn_amd.graph import TannerGraph
from helpers import code, gpu_graph, oracle_library_forms, to_gpu
from oracle.oracle import OracleGraph
from test_bp2_reference_cpu import edge_channel

pytestmark = pytest.mark.gpu

SEED = 0x5EED
RULES = ("boxplus-phi", "minsum", "boxplus")
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h


def _bare(hx, hz=None):
    """A code object carrying only what TannerGraph / OracleGraph read, with no GF(2) rank work: hz defaults to one single-edge row
    (the graph needs a non-empty side 1; binary BP never reads it)."""
    hx = np.asarray(hx, np.int64)
    n = hx.shape[1]
    if hz is None:
        hz = np.zeros((1, n), np.int64)
        hz[0, 0] = 1
    zero = np.zeros((1, n), np.int64)
    return types.SimpleNamespace(hx=hx, hz=np.asarray(hz, np.int64), hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)


_CACHE = {}


def graphs(key, make):
    """(TannerGraph, OracleGraph, hx) of one case, built once per session."""
    if key not in _CACHE:
        c = make()
        _CACHE[key] = (TannerGraph(c), OracleGraph(c, forms="library-default"), np.asarray(c.hx))
    return _CACHE[key]


def named(name):
    """(TannerGraph, OracleGraph, hx) of one of the suite's shared named codes."""
    return gpu_graph(name), oracle_library_forms(name), np.asarray(code(name).hx)


# ---- the host dispatch rule of fgnn_bp2_decode, restated ---------------------------------------------------------------------------
def instantiation(g, hx, cn_type, force_generic=False, no_pred=False):
    """The bp2_kernel<CN_TYPE, DV, DC> fgnn_bp2_decode launches for graph g: (rule, DV, DC), DV = DC = 0 for the runtime-degree loop.
    cslot16 (fgnn_graph.hip) exists for uniform degrees on both sides, dc <= 8 and 4 (E_x + E_z) < 65536."""
    info = g.info()
    cslot16 = info["dv_x"] > 0 and info["dv_z"] > 0 and 0 < info["dc"] <= 8 and 4 * (info["E_x"] + info["E_z"]) < 65536
    regular = cslot16 and not force_generic
    if regular and cn_type != "boxplus":
        if info["dv_x"] == 3 and info["dc"] == 6:
            return (cn_type, 3, 6)
        if info["dv_x"] == 4 and info["dc"] == 8:
            return (cn_type, 4, 8)
    md = 1 << 30 if (force_generic and no_pred) else int(np.asarray(hx).sum(1).max())
    if cn_type == "minsum" and md <= 8:
        return ("minsum", 0, 8)
    if cn_type == "minsum" and md <= 16:
        return ("minsum", 0, 16)
    return (cn_type, 0, 0)


ALL_INSTANTIATIONS = {("boxplus-phi", 3, 6), ("minsum", 3, 6), ("boxplus-phi", 4, 8), ("minsum", 4, 8), ("minsum", 0, 8),
                      ("minsum", 0, 16), ("boxplus-phi", 0, 0), ("minsum", 0, 0), ("boxplus", 0, 0)}


def gb(l, a, b):
    return functools.lru_cache(maxsize=None)(lambda: cq.create_generalized_bicycle_codes(l, [int(x) for x in a], [int(x) for x in b]))


def random_gb(seed, w, l):
    """A seeded generalized-bicycle code with |a| = |b| = w: a (w, 2w)-regular hx with its own slot offsets."""
    rng = np.random.RandomState(seed)
    a = sorted(rng.choice(l, size=w, replace=False))
    b = sorted(rng.choice(l, size=w, replace=False))
    return gb(l, a, b)


def irregular(seed, n, m, max_deg):
    """A seeded random sparse hx [m, n] with checks of degree 1 .. max_deg (two of degree 1) and two edge-free bits."""
    @functools.lru_cache(maxsize=None)
    def make():
        rng = np.random.RandomState(seed)
        h = np.zeros((m, n), np.int64)
        for c in range(m):
            d = 1 if c < 2 else rng.randint(2, max_deg + 1)
            h[c, rng.choice(n - 2, size=min(d, n - 2), replace=False)] = 1
        h[2, :] = 0
        h[2, [n - 3, n - 4]] = 1  # a degree-2 check; the last two bits keep no edge
        return _bare(h)
    return make


# (key, maker): every case runs every rule; the module assertion below checks that together they reach every instantiation
CASES = [
    ("gb_rand_3a", random_gb(1, 3, 31)), ("gb_rand_3b", random_gb(2, 3, 45)),     # (3,6)-regular
    ("gb_rand_4a", random_gb(3, 4, 29)), ("gb_rand_4b", random_gb(4, 4, 52)),     # (4,8)-regular
    ("gb_rand_6", random_gb(5, 6, 40)), ("gb_rand_8", random_gb(6, 8, 37)),       # check degree 12, 16
    ("gb_rand_9", random_gb(7, 9, 41)), ("gb_rand_11", random_gb(8, 11, 47)),     # check degree 18, 22
    ("irr_8", irregular(9, 60, 30, 8)), ("irr_16", irregular(10, 90, 40, 16)), ("irr_30", irregular(11, 120, 30, 30)),
]
_CASE_SHAPES = {"gb_rand_3a": (3, 6), "gb_rand_3b": (3, 6), "gb_rand_4a": (4, 8), "gb_rand_4b": (4, 8)}


def _case_instantiations():
    """The instantiations CASES reach, from the hx degrees alone (no GPU needed): regular GB codes of weight 3 / 4 have cslot16
    (uniform degrees on both sides, dc <= 8, 4 E < 65536 for these sizes); everything else takes the runtime-degree kernels."""
    out = set()
    for key, make in CASES:
        hx = np.asarray(make().hx)
        assert (key in _CASE_SHAPES) == (hx.sum(0).min() == hx.sum(0).max() and hx.sum(1).min() == hx.sum(1).max() <= 8)
        for cn in RULES:
            if key in _CASE_SHAPES and cn != "boxplus":
                out.add((cn,) + _CASE_SHAPES[key])
                continue
            md = int(hx.sum(1).max())
            out.add(("minsum", 0, 8) if cn == "minsum" and md <= 8 else ("minsum", 0, 16) if cn == "minsum" and md <= 16 else (cn, 0, 0))
    return out


assert _case_instantiations() == ALL_INSTANTIATIONS, "the cases must reach every bp2_kernel instantiation"


def _run(g, og, hx, synd, iters, cn_type, factor, B=None, **llr):
    gl = {k: to_gpu(v) for k, v in llr.items() if k == "llr_ch"}
    gl.update({k: v for k, v in llr.items() if k != "llr_ch"})
    s1, h1 = g.bp2_decode(to_gpu(synd) if synd is not None else None, iters, cn_type, factor, B=B, **gl)
    return s1.cpu().numpy(), h1.cpu().numpy()


def assert_bits(og, synd, iters, cn_type, factor, s1, h1, **llr):
    s0, h0 = og.bp2_decode(synd, iters, cn_type, factor, **llr)
    assert np.array_equal(s0.view(np.int32), s1.view(np.int32)), (cn_type, factor, iters)
    assert np.array_equal(h0, h1), (cn_type, factor, iters)


def check(g, og, hx, B, iters, cn_type, factor, seed, p=0.06):
    """Kernel against oracle with a constant logit and with per-bit logits carrying the edge values; a random syndrome of BSC(p)
    noise.  Returns the syndrome."""
    rng = np.random.RandomState(seed)
    e = (rng.rand(B, hx.shape[1]) < p).astype(np.int64)
    synd = (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)
    for llr in (dict(llr_const=-2.197), dict(llr_ch=edge_channel(hx, B, seed))):
        s1, h1 = _run(g, og, hx, synd, iters, cn_type, factor, **llr)
        assert_bits(og, synd, iters, cn_type, factor, s1, h1, **llr)
    return synd


@pytest.mark.parametrize("key", [k for k, _ in CASES])
def test_runtime_degree_fuzz(key):
    g, og, hx = graphs(key, dict(CASES)[key])
    rng = np.random.RandomState(zlib.crc32(key.encode()))
    for cn in RULES:
        assert instantiation(g, hx, cn) in ALL_INSTANTIATIONS
        for factor in (1.0, 0.8, 0.625):
            check(g, og, hx, int(rng.randint(1, 70)), int(rng.randint(1, 30)), cn, factor, int(rng.randint(1 << 30)))


def test_case_dispatch_matches_the_host_rule():
    """The restated rule on the built graphs (info() reports the degrees the library saw) gives what the module assertion assumed."""
    got = set()
    for key, make in CASES:
        g, _, hx = graphs(key, make)
        got |= {instantiation(g, hx, cn) for cn in RULES}
    assert got == ALL_INSTANTIATIONS


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "gb126", "ghp882"])
def test_named_codes_every_rule(name):
    g, og, hx = named(name)
    for cn in RULES:
        check(g, og, hx, 19, 9, cn, 0.8, 4)


def test_force_generic_reaches_the_loop_on_regular_graphs():
    g, og, hx = named("gb48")
    g.force_generic(True)
    try:
        for cn in RULES:
            assert instantiation(g, hx, cn, force_generic=True) in (("minsum", 0, 8), (cn, 0, 0))
            check(g, og, hx, 21, 11, cn, 0.8, 6)
    finally:
        g.force_generic(False)


# ---- launch geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Bs", [("rsurf5", (1, 7, 8, 9, 61)), ("gb48", (3, 5, 13))])
def test_several_codewords_per_workgroup(name, Bs):
    g, og, hx = named(name)
    assert g.info()["codewords_per_block"] > 1
    for B in Bs:
        for cn in RULES:
            check(g, og, hx, B, 6, cn, 0.8, B)


def test_b_256_and_257_on_an_irregular_single_codeword_graph():
    """gb48_oc: 1000 checks, one codeword per workgroup; B <= 256 widens the workgroup to 1024 threads, B = 257 keeps 256."""
    g, og, hx = named("gb48_oc")
    assert g.info()["codewords_per_block"] == 1
    for B in (256, 257):
        for cn in RULES:
            check(g, og, hx, B, 3, cn, 0.8, B)


def _checks_per_thread_hx(m):
    """m checks on 40 bits, each of degree 3, every bit used."""
    h = np.zeros((m, 40), np.int64)
    for c in range(m):
        h[c, [c % 40, (3 * c + 1) % 40, (7 * c + 5) % 40]] = 1
    h[0, np.nonzero(h.sum(0) == 0)[0]] = 1
    return h


@pytest.mark.parametrize("tpc,cpb,m", [(1, 64, 1), (1, 64, 31), (1, 64, 32), (1, 64, 33), (1, 64, 40), (2, 32, 64), (2, 32, 65),
                                       (4, 16, 80), (64, 1, 2048), (64, 1, 2049), (32, 2, 1024), (32, 2, 1025)])
def test_checks_per_thread(tpc, cpb, m):
    """set_launch geometries that give a thread 1 .. 40 checks: m = 32 tpc keeps the syndrome in a register with bit 31 in use,
    m = 32 tpc + 1 re-reads it from global memory every iteration."""
    hx = _checks_per_thread_hx(m)
    g, og, _ = graphs(("cpt", m), lambda: _bare(hx))
    g.set_launch(tpc, cpb)
    try:
        ones = np.ones((cpb + 3, m), np.uint8)  # every syndrome bit set, the thread's last one (bit 31 / the global path) included
        for cn in RULES:
            check(g, og, hx, cpb + 3, 5, cn, 0.8, m)
            s1, h1 = _run(g, og, hx, ones, 5, cn, 0.8, llr_const=-2.197)
            assert_bits(og, ones, 5, cn, 0.8, s1, h1, llr_const=-2.197)
    finally:
        g.set_launch(0, 0)


def test_set_launch_refusals():
    """Geometries set_launch cannot produce are refused: tpc * cpb not a multiple of 64, or above 1024."""
    g, _, _ = named("rsurf5")
    for tpc, cpb in ((1, 1), (3, 32), (64, 17), (2048, 1)):
        with pytest.raises(ValueError, match="multiple of 64"):
            g.set_launch(tpc, cpb)
    g.set_launch(0, 0)


# ---- LDS ----------------------------------------------------------------------------------------------------------------------------
def bp2_lds_bytes(E_x, cpb):
    """fgnn_bp2_decode: lds_per_cw = E_x rounded up to 4 floats, times codewords per workgroup."""
    return ((E_x + 3) & ~3) * 4 * cpb


def lds_hx(E):
    """n = E / 4 bits, checks of 8 consecutive bits (bit v in checks (v + k n) / 8, k < 4), then E mod 8 bits on one more check."""
    full, extra = divmod(E, 8)
    n = max(8, (8 * full) // 4)
    h = np.zeros((full + (1 if extra else 0), n), np.int64)
    for c in range(full):
        h[c, (8 * c + np.arange(8)) % n] = 1
    if extra:
        h[full, :extra] = 1
    return h


def hp_big_hx():
    """The hx of a hypergraph product of helpers' seeded 36 x 72 hp_big matrix with itself, by Kronecker products and without the
    rank work of the code class: 2592 checks of degree up to 9, about 23 000 edges, 91 KB of messages."""
    rng = np.random.RandomState(7)
    m, n, dv = 36, 72, 3
    per = dv * n // m // dv
    h = np.zeros((m, n), dtype=np.int64)
    for _ in range(dv):
        perm = rng.permutation(n)
        for r in range(m):
            h[r, perm[r * per:(r + 1) * per]] = 1
    return np.hstack([np.kron(h, np.eye(n, dtype=np.int64)), np.kron(np.eye(m, dtype=np.int64), h.T)])


def test_dynamic_lds_above_48k():
    hx = hp_big_hx()
    g, og, _ = graphs("hp_big_hx", lambda: _bare(hx))
    assert bp2_lds_bytes(int(hx.sum()), g.info()["codewords_per_block"]) > 48 * 1024
    assert {instantiation(g, hx, cn) for cn in RULES} == {("boxplus-phi", 0, 0), ("minsum", 0, 16), ("boxplus", 0, 0)}
    for cn in RULES:
        check(g, og, hx, 3, 4, cn, 0.8, 12, p=0.02)


@pytest.mark.parametrize("cpb", [1, 2])
def test_lds_budget_both_sides(cpb):
    E = LDS_BUDGET // 4 // cpb
    assert bp2_lds_bytes(E, cpb) <= LDS_BUDGET < bp2_lds_bytes(E + 1, cpb)
    hx = lds_hx(E)
    assert hx.sum() == E
    g, og, _ = graphs(("lds", E), lambda: _bare(hx))
    if cpb > 1:
        g.set_launch(g.info()["threads_per_codeword"], cpb)
    try:
        for cn in RULES:
            check(g, og, hx, 2 * cpb + 1, 3, cn, 0.8, 13)
    finally:
        g.set_launch(0, 0)
    over = lds_hx(E + 1)
    assert over.sum() == E + 1
    g2, _, _ = graphs(("lds", E + 1), lambda: _bare(over))
    if cpb > 1:
        g2.set_launch(g2.info()["threads_per_codeword"], cpb)
    try:
        synd = torch.zeros((2, over.shape[0]), dtype=torch.uint8, device=g2.device)
        with pytest.raises(ValueError, match="code too large for the LDS-resident kernel"):
            g2.bp2_decode(synd, 3, "minsum", 0.8, llr_const=-2.0)
    finally:
        g2.set_launch(0, 0)


# ---- arguments and outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb_rand_3a", "gb_rand_4a", "ghp882", "gb48"])
def test_factor_one_shortcut_and_its_neighbours(name):
    g, og, hx = named(name) if name in ("ghp882", "gb48") else graphs(name, dict(CASES)[name])
    assert instantiation(g, hx, "minsum")[1] > 0
    assert instantiation(g, hx, "boxplus-phi")[1] > 0
    for factor in (1.0, float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 0.0):
        for cn in RULES:
            check(g, og, hx, 9, 7, cn, factor, 21)


@pytest.mark.parametrize("name", ["gb48", "gb126", "rsurf5"])
def test_soft_only_hard_only_and_null_syndrome(name):
    g, og, hx = named(name)
    B = 11
    rng = np.random.RandomState(3)
    synd = to_gpu(rng.randint(0, 2, size=(B, hx.shape[0])).astype(np.uint8))
    for cn in RULES:
        s, h = g.bp2_decode(synd, 8, cn, 0.8, llr_const=-1.7)
        s_only, none_h = g.bp2_decode(synd, 8, cn, 0.8, llr_const=-1.7, want_hard=False)
        none_s, h_only = g.bp2_decode(synd, 8, cn, 0.8, llr_const=-1.7, want_soft=False)
        assert none_h is None and none_s is None
        assert torch.equal(s.view(torch.int32), s_only.view(torch.int32)) and torch.equal(h, h_only)
        z = torch.zeros_like(synd)
        s0, h0 = g.bp2_decode(z, 8, cn, 0.8, llr_const=-1.7)
        sn, hn = g.bp2_decode(None, 8, cn, 0.8, llr_const=-1.7, B=B)
        assert torch.equal(s0.view(torch.int32), sn.view(torch.int32)) and torch.equal(h0, hn)
        assert_bits(og, np.zeros((B, hx.shape[0]), np.uint8), 8, cn, 0.8, sn.cpu().numpy(), hn.cpu().numpy(), llr_const=-1.7)


def test_zero_and_all_ones_syndromes_and_zero_iterations():
    for key, make in CASES[:1] + CASES[4:5] + CASES[8:9]:
        g, og, hx = graphs(key, make)
        B = 6
        for synd in (np.zeros((B, hx.shape[0]), np.uint8), np.ones((B, hx.shape[0]), np.uint8)):
            for cn in RULES:
                for iters in (0, 1, 2):
                    for llr in (dict(llr_const=0.0), dict(llr_ch=edge_channel(hx, B, 2))):
                        s1, h1 = _run(g, og, hx, synd, iters, cn, 0.8, **llr)
                        assert_bits(og, synd, iters, cn, 0.8, s1, h1, **llr)


# ---- noise --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steane", "rsurf3", "rsurf5", "gb126"])  # n mod 4 = 3, 1, 1, 2
def test_bsc_noise_against_the_oracle(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    assert g.n % 4 != 0
    for p in (0.0, 1.0, 1e-7, 0.3):
        for first in (1, 12345, 2**40 + 3):
            assert np.array_equal(og.bsc_noise(SEED, p, first, 37), g.bsc_noise(SEED, p, first, 37).cpu().numpy()), (p, first)
    assert not g.bsc_noise(SEED, 0.0, 5, 9).cpu().numpy().any() and g.bsc_noise(SEED, 1.0, 5, 9).cpu().numpy().all()
