"""Relay-BP with layered legs on the GPU (fgnn_relay_decode_layered) at every relay_layered_kernel<DV, DC> instantiation, held to the
NumPy float32 restatement tests/relay_layered_reference.py bit for bit: hard decisions as bytes, stats as int32, no tolerance anywhere.
The update uses only IEEE float32 add, multiply, min, max and compare in a fixed order, and the weight of a decision is an integer, so
nothing depends on a reduction order.  Graphs, syndromes and edge inputs are those of tests/test_gpu_relay.py.

Layered legs solve more than flooding ones, so the noise rates and iteration counts are chosen on the restatement such that every
branch of the leg control is walked: each property is asserted on the restatement's own outputs, next to the case that must show it."""
import zlib

import numpy as np
import pytest
import torch

import bp2_layered_reference as BR
import relay_layered_reference as RL
from feedback_gnn_amd import gf2
from helpers import code, to_gpu
from test_bp2_reference_cpu import _llr_const, edge_channel
from test_gpu_bp2_shapes import CASES, LDS_BUDGET, _bare, bp2_lds_bytes, graphs, hp_big_hx, lds_hx, named
from test_gpu_relay import FUZZ, informed_edge_channel, instantiation, noise_syndromes, noisy, relay_lds_bytes
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED
FUZZ_P = 0.09  # BSC rate of the fuzz: at 0.06, test_gpu_relay's, layered legs leave too few samples for the later legs


def both(g, hx, synd, gamma, pre, leg, stop, factor, B=None, layer_of=None, **llr):
    """Kernel and restatement on the same inputs (layer_of: the layering installed on g, None = greedy); asserts identical outputs,
    returns the restatement's (hard, stats, solutions)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    hard, stats = g.relay_decode_layered(None if synd is None else to_gpu(synd), to_gpu(gamma), pre, leg, stop, factor, B=B, **gl)
    h0, s0, sols = RL.relay_layered_decode(hx, synd, gamma, pre, leg, stop, factor, B=B, layer_of=layer_of, **llr)
    assert stats.dtype == torch.int32 and hard.dtype == torch.uint8
    s1, h1 = stats.cpu().numpy(), hard.cpu().numpy()
    print("found", s0[:, 0].tolist(), "leg", s0[:, 2].tolist(), "k", s0[:, 3].tolist())
    assert s1.dtype == s0.dtype and s1.shape == s0.shape and h1.shape == h0.shape
    assert s0.tobytes() == s1.tobytes(), (np.nonzero((s0 != s1).any(1))[0], s0[(s0 != s1).any(1)], s1[(s0 != s1).any(1)])
    assert h0.tobytes() == h1.tobytes()
    return h0, s0, sols


def fuzz_cases(hx, rng):
    """B in 1..70, pre_iter and leg_iter <= 12, 1 / 2 / 5 legs, stop_nconv 1 and 3, three factors, a constant logit and per-bit logits with
    the edge values of edge_channel; gamma rows with 0, negative values and values above 0.5.  Yields (args, llr keywords)."""
    n = hx.shape[1]
    for legs, factor in ((1, 1.0), (2, 0.8), (5, 0.625)):
        for stop in (1, 3):
            B, pre, leg = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            e, synd = noisy(hx, B, FUZZ_P, int(rng.randint(1 << 30)))
            gamma = mixed_gamma(legs, n, int(rng.randint(1 << 30)))
            yield (synd, gamma, pre, leg, stop, factor), dict(llr_const=-2.197)
            yield (synd, gamma, pre, leg, stop, factor), dict(llr_ch=informed_edge_channel(hx, e, int(rng.randint(1 << 30))))


def fuzz(g, hx, rng):
    """Every case of fuzz_cases on kernel and restatement; returns the restatement's stats rows of all of them, [*, 4]."""
    g.set_bit_layers()
    return np.concatenate([both(g, hx, *args, **llr)[1] for args, llr in fuzz_cases(hx, rng)])


def walks_the_control(stats):
    """The branches of the leg control a batch of stats rows shows: unsolved samples, samples solved in leg 0, samples solved later."""
    return (stats[:, 0] == 0).any(), ((stats[:, 0] > 0) & (stats[:, 2] == 0)).any(), ((stats[:, 0] > 0) & (stats[:, 2] > 0)).any()


@pytest.mark.parametrize("key", list(FUZZ))
def test_every_instantiation(key):
    g, _, hx = graphs(key, dict(CASES)[key])
    assert instantiation(g, hx) == FUZZ[key]
    stats = fuzz(g, hx, np.random.RandomState(zlib.crc32(key.encode())))
    none, first, later = walks_the_control(stats)
    assert none, "no sample of the fuzz stays unsolved"
    assert first, "no sample of the fuzz is solved in leg 0"
    assert later, "no sample of the fuzz is solved in a later leg"


def test_force_generic_on_a_regular_graph():
    g, _, hx = named("gb48")
    assert instantiation(g, hx) == (4, 8) and instantiation(g, hx, force_generic=True) == (0, 8)
    g.force_generic(True)
    try:
        stats = fuzz(g, hx, np.random.RandomState(17))
        assert all(walks_the_control(stats))
    finally:
        g.force_generic(False)


# ---- several codewords per workgroup ---------------------------------------------------------------------------------------------------
RSURF_P = 0.2


def test_codewords_of_one_workgroup_stop_at_different_legs():
    g, _, hx = named("rsurf5")
    g.set_bit_layers()
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    n, legs = hx.shape[1], 4
    gamma = mixed_gamma(legs, n, 3)
    for B in (1, cpb - 1, cpb, cpb + 1):
        synd = noise_syndromes(hx, B, RSURF_P, 40)  # the same first rows for every B
        _, stats, _ = both(g, hx, synd, gamma, 2, 2, 1, 0.8, llr_const=_llr_const(RSURF_P))
        if B >= cpb - 1:
            first = stats[:cpb]  # the first workgroup
            assert (first[:, 2] == 0).any(), "no sample of the workgroup stops in the first leg"
            assert ((first[:, 0] > 0) & (first[:, 2] > 0)).any(), "no sample of the workgroup is solved in a later leg"
            assert len(set(map(tuple, first[:, 2:]))) >= 3, "the workgroup's samples must stop at three or more different (leg, k)"
    # stop_nconv = 3: solved samples go on into further legs while others of the workgroup are finished
    synd = noise_syndromes(hx, cpb + 1, RSURF_P, 40)
    _, _, sols = both(g, hx, synd, gamma, 2, 2, 3, 0.8, llr_const=_llr_const(RSURF_P))
    assert max(len(s) for s in sols) >= 2, "some sample must meet more than one solution"


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (2, 32), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, _, hx = named("rsurf5")
    g.set_bit_layers()
    g.set_launch(tpc, cpb)
    try:
        synd = noise_syndromes(hx, cpb + 3, RSURF_P, 41)
        _, stats, _ = both(g, hx, synd, mixed_gamma(3, hx.shape[1], 4), 2, 3, 2, 0.8, llr_const=_llr_const(RSURF_P))
        assert len(set(map(tuple, stats[:, 2:]))) >= 2, "the samples must stop at different (leg, k)"
    finally:
        g.set_launch(0, 0)


# ---- syndromes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, _, hx = named(name)
    g.set_bit_layers()
    B, n = 9, hx.shape[1]
    gamma = to_gpu(mixed_gamma(3, n, 5))
    zero = np.zeros((B, hx.shape[0]), np.uint8)
    h0, s0, _ = both(g, hx, zero, mixed_gamma(3, n, 5), 6, 5, 1, 0.8, llr_const=-2.0)
    assert not h0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 0, 1], np.int32), (B, 1)))
    hz, sz = g.relay_decode_layered(to_gpu(zero), gamma, 6, 5, 1, 0.8, llr_const=-2.0)
    hn, sn = g.relay_decode_layered(None, gamma, 6, 5, 1, 0.8, llr_const=-2.0, B=B)
    assert torch.equal(hz, hn) and torch.equal(sz, sn)
    assert np.array_equal(hn.cpu().numpy(), h0) and np.array_equal(sn.cpu().numpy(), s0)
    both(g, hx, None, mixed_gamma(3, n, 5), 6, 5, 1, 0.8, llr_ch=edge_channel(hx, B, 8))


def test_syndrome_outside_the_column_space():
    """gb48's hx has dependent rows: a syndrome s with u.s = 1 for a u in the left kernel (u H = 0) is the syndrome of no error, so
    no test can pass: found = 0, the output is the decision of the last test of the last leg."""
    g, _, hx = named("gb48")
    g.set_bit_layers()
    left = np.asarray(gf2.kernel(np.asarray(hx, np.int64).T)[0], np.int64) % 2
    assert left.shape[0] >= 1 and not ((left @ np.asarray(hx, np.int64)) % 2).any()
    u = left[0]
    B, legs, leg_iter = 7, 3, 5
    synd = noise_syndromes(hx, B, 0.06, 2)
    flip = int(np.nonzero(u)[0][0])
    for b in range(B):
        if (synd[b].astype(np.int64) @ u) % 2 == 0:
            synd[b, flip] ^= 1
    assert ((synd.astype(np.int64) @ u) % 2 == 1).all()
    for stop in (1, 3):
        _, s0, sols = both(g, hx, synd, mixed_gamma(legs, hx.shape[1], 6), 6, leg_iter, stop, 0.8, llr_const=_llr_const(0.06))
        assert (s0[:, 0] == 0).all() and (s0[:, 2] == legs - 1).all() and (s0[:, 3] == leg_iter).all() and not any(sols)


# ---- layerings -------------------------------------------------------------------------------------------------------------------------
def test_a_callers_layering():
    g, _, hx = named("gb48")
    m, n = hx.shape
    reverse = np.arange(m - 1, -1, -1).astype(np.int32)  # one check per layer, the last check first: m + 3 barriers per step
    synd = noise_syndromes(hx, 37, 0.08, 4)
    args = (synd, mixed_gamma(3, n, 2), 3, 2, 1, 0.8)
    try:
        g.set_bit_layers(reverse)
        mine = both(g, hx, *args, layer_of=reverse, llr_const=_llr_const(0.08))
        g.set_bit_layers()
        assert g.bit_layers()[0] == BR.greedy_bit_layers(hx)[0] < m
        greedy = both(g, hx, *args, llr_const=_llr_const(0.08))
        assert mine[0].tobytes() != greedy[0].tobytes() or mine[1].tobytes() != greedy[1].tobytes()
    finally:
        g.set_bit_layers()


def test_first_use_installs_the_greedy_layering():
    hx = np.asarray(dict(CASES)["irr_8"]().hx)
    from feedback_gnn_amd.graph import TannerGraph
    g = TannerGraph(dict(CASES)["irr_8"]())
    assert g.bit_layers() == (0, None)
    both(g, hx, noise_syndromes(hx, 5, 0.06, 3), mixed_gamma(2, hx.shape[1], 1), 3, 2, 1, 0.8, llr_const=-2.0)
    num, lay = g.bit_layers()
    assert num == BR.greedy_bit_layers(hx)[0] and np.array_equal(lay, BR.greedy_bit_layers(hx)[1])


# ---- anchor ----------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_one_leg_one_iteration_is_layered_minsum_on_the_gpu():
    """include/fgnn.h: with gamma = 0, one leg and pre_iter = 1 the decisions are those of fgnn_bp2_decode_layered (min-sum) bit for bit."""
    for name in ("ghp882", "gb48", "rsurf5"):
        g, _, hx = named(name)
        g.set_bit_layers()
        B, n = 19, hx.shape[1]
        synd = to_gpu(noise_syndromes(hx, B, 0.03, 5))
        gamma = torch.zeros((1, n), dtype=torch.float32, device=g.device)
        for factor in (1.0, 0.8):
            hard, stats = g.relay_decode_layered(synd, gamma, 1, 1, 1, factor, llr_const=_llr_const(0.03))
            _, h0, s0 = g.bp2_decode_layered(synd, 1, "minsum", factor, llr_const=_llr_const(0.03), want_soft=False, stop=True, want_stats=True)
            assert torch.equal(hard, h0), (name, factor)
            assert torch.equal(stats[:, 0], s0[:, 0]) and bool((stats[:, 2] == 0).all()) and bool((stats[:, 3] == 1).all())


# ---- LDS -------------------------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    hx = hp_big_hx()
    g, _, _ = graphs("hp_big_hx", lambda: _bare(hx))
    g.set_bit_layers()
    assert 48 * 1024 < relay_lds_bytes(int(hx.sum()), hx.shape[1], g.info()["codewords_per_block"]) <= LDS_BUDGET
    assert instantiation(g, hx) == (0, 16)
    synd = noise_syndromes(hx, 3, 0.01, 12)
    both(g, hx, synd, mixed_gamma(2, hx.shape[1], 7), 4, 3, 1, 0.8, llr_const=_llr_const(0.01))


def test_messages_beyond_the_budget_are_refused():
    E = LDS_BUDGET // 4 + 1
    assert bp2_lds_bytes(E, 1) > LDS_BUDGET
    over = lds_hx(E)
    g, _, _ = graphs(("lds", E), lambda: _bare(over))
    synd = torch.zeros((2, over.shape[0]), dtype=torch.uint8, device=g.device)
    gamma = torch.zeros((1, over.shape[1]), dtype=torch.float32, device=g.device)
    with pytest.raises(ValueError, match="code too large for the LDS-resident kernel"):
        g.relay_decode_layered(synd, gamma, 3, 3, 1, 0.8, llr_const=-2.0)


def test_posteriors_count_against_the_budget():
    """Messages that fit binary BP's budget with no room left for the n posteriors: bp2_decode runs, relay_decode_layered refuses."""
    E = LDS_BUDGET // 4
    hx = lds_hx(E)
    g, _, _ = graphs(("lds", E), lambda: _bare(hx))
    assert bp2_lds_bytes(E, 1) <= LDS_BUDGET < relay_lds_bytes(E, hx.shape[1], 1)
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    g.bp2_decode(synd, 1, "minsum", 0.8, llr_const=-2.0)
    with pytest.raises(ValueError, match="code too large for the LDS-resident kernel"):
        g.relay_decode_layered(synd, torch.zeros((1, hx.shape[1]), dtype=torch.float32, device=g.device), 3, 3, 1, 0.8, llr_const=-2.0)


def test_argument_errors():
    g, _, hx = named("gb48")
    n = hx.shape[1]
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    gamma = torch.zeros((2, n), dtype=torch.float32, device=g.device)
    for pre, leg, stop in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError, match=">= 1"):
            g.relay_decode_layered(synd, gamma, pre, leg, stop)
    with pytest.raises(ValueError, match="gamma"):
        g.relay_decode_layered(synd, gamma[:, :n - 1].contiguous(), 2, 2, 1)
    with pytest.raises(ValueError, match="gamma"):
        g.relay_decode_layered(synd, gamma.double(), 2, 2, 1)
    with pytest.raises(ValueError, match="syndrome"):
        g.relay_decode_layered(synd[:, :-1].contiguous(), gamma, 2, 2, 1)
    hard, stats = g.relay_decode_layered(synd[:0], gamma, 2, 2, 1)  # an empty batch: no launch, empty outputs
    assert tuple(hard.shape) == (0, n) and tuple(stats.shape) == (0, 4)


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def test_relay_bp_decoder_class():
    import feedback_gnn_amd as F
    hx = np.asarray(code("gb48").hx)
    m, n = hx.shape
    dec = F.RelayBPDecoder(hx, gamma0=0.125, pre_iter=3, num_sets=3, set_max_iter=2, stop_nconv=2, normalization_factor=0.8, seed=5,
                           schedule="layered")
    assert dec.schedule == "layered" and dec.graph.bit_layers()[0] == BR.greedy_bit_layers(hx)[0]
    gam = dec.gamma.cpu().numpy()
    B = 23
    synd = noise_syndromes(hx, B, 0.1, 9)
    llr = np.full((B, n), _llr_const(0.1), F32)
    e_hat = dec((to_gpu(llr), to_gpu(synd.T.copy())))
    h0, s0, _ = RL.relay_layered_decode(hx, synd, gam, 3, 2, 2, 0.8, llr_ch=llr)
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (B, n)
    assert np.array_equal(e_hat.cpu().numpy(), h0.astype(F32)) and np.array_equal(dec.last_stats.cpu().numpy(), s0)
    assert (s0[:, 2] > 0).any(), "some sample must use a later leg"
    hard, stats = dec.decode(to_gpu(synd), llr_const=_llr_const(0.1))
    assert np.array_equal(hard.cpu().numpy(), h0) and np.array_equal(stats.cpu().numpy(), s0)
    # a caller's layering, and the flooding decoder on the same matrix untouched by it
    reverse = np.arange(m - 1, -1, -1).astype(np.int32)
    own = F.RelayBPDecoder(hx, gamma0=0.125, pre_iter=3, num_sets=3, set_max_iter=2, stop_nconv=2, normalization_factor=0.8, seed=5,
                           schedule="layered", layers=reverse)
    assert np.array_equal(own.graph.bit_layers()[1], reverse)
    hard, stats = own.decode(to_gpu(synd), llr_const=_llr_const(0.1))
    h1, s1, _ = RL.relay_layered_decode(hx, synd, gam, 3, 2, 2, 0.8, llr_ch=llr, layer_of=reverse)
    assert np.array_equal(hard.cpu().numpy(), h1) and np.array_equal(stats.cpu().numpy(), s1)
    import relay_reference as R
    flood = F.RelayBPDecoder(hx, gamma0=0.125, pre_iter=3, num_sets=3, set_max_iter=2, stop_nconv=2, normalization_factor=0.8, seed=5,
                             graph=own.graph)
    hard, stats = flood.decode(to_gpu(synd), llr_const=_llr_const(0.1))
    h2, s2, _ = R.relay_decode(hx, synd, gam, 3, 2, 2, 0.8, llr_ch=llr)
    assert flood.schedule == "flooding" and np.array_equal(hard.cpu().numpy(), h2) and np.array_equal(stats.cpu().numpy(), s2)
    with pytest.raises(ValueError, match="schedule must be"):
        F.RelayBPDecoder(hx, schedule="serial")


def test_bp2_relay_model():
    import feedback_gnn_amd as F
    c = code("gb126")
    hx, logical = np.asarray(c.hx), np.asarray(c.hz_perp)
    m = hx.shape[0]
    num, greedy = BR.greedy_bit_layers(hx)
    own = (num - 1 - greedy).astype(np.int32)  # the greedy layers in reverse order
    dec = F.RelayBPDecoder(hx, pre_iter=3, num_sets=3, set_max_iter=2, normalization_factor=0.8, seed=1, schedule="layered", layers=own)
    model = F.BP2_Relay_Model(hx, logical, dec, seed=SEED)
    assert np.array_equal(model.graph.bit_layers()[1], own), "the model's graph takes its decoder's layering"
    B, p = 64, 0.09
    s_hat, ls_hat = model(B, p)
    noise, est, stats = model.last_noise.cpu().numpy(), model.last_estimate.cpu().numpy(), model.last_stats.cpu().numpy()
    assert tuple(s_hat.shape) == (B, m) and tuple(ls_hat.shape) == (B, logical.shape[0])
    synd = (noise.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    h0, s0, _ = RL.relay_layered_decode(hx, synd, dec.gamma.cpu().numpy(), 3, 2, 1, 0.8, llr_const=_llr_const(p), layer_of=own)
    assert np.array_equal(est, h0) and np.array_equal(stats, s0)
    res = noise ^ est
    solved = stats[:, 0] > 0
    assert solved.any() and not solved.all(), "the batch must hold solved and unsolved samples"
    assert np.array_equal(s_hat.cpu().numpy(), res.astype(np.int64) @ hx.T.astype(np.int64) % 2)
    assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
    assert np.array_equal(ls_hat.cpu().numpy(), res.astype(np.int64) @ logical.T.astype(np.int64) % 2)
    assert model.last_num_unsolved == int((~solved).sum())
