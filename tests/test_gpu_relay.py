"""Relay-BP on the GPU (fgnn_relay_decode) at every relay_kernel<DV, DC> instantiation, held to the NumPy float32 restatement
tests/relay_reference.py bit for bit: hard decisions as bytes, stats as int32, no tolerance anywhere.  The update uses only IEEE
float32 add, multiply, min, max and compare in a fixed order, and the weight of a decision is an integer, so nothing depends on a
reduction order.  Graph makers and edge inputs come from the binary BP shape tests."""
import zlib

import numpy as np
import pytest
import torch

import relay_reference as R
from feedback_gnn_amd import gf2
from helpers import code, to_gpu
from test_bp2_reference_cpu import _llr_const, edge_channel
from test_gpu_bp2_shapes import CASES, LDS_BUDGET, _bare, bp2_lds_bytes, graphs, hp_big_hx, lds_hx, named
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5EED


def relay_lds_bytes(E_x, n, cpb):
    """fgnn_relay_decode: messages and posteriors per codeword, each rounded up to 4 floats; stamp and wacc per codeword and ndone."""
    return (((E_x + 3) & ~3) + ((n + 3) & ~3)) * 4 * cpb + ((2 * cpb + 1 + 3) & ~3) * 4


def instantiation(g, hx, force_generic=False):
    """The relay_kernel<DV, DC> fgnn_relay_decode launches: the min-sum part of fgnn_bp2_decode's rule."""
    info = g.info()
    cslot16 = info["dv_x"] > 0 and info["dv_z"] > 0 and 0 < info["dc"] <= 8 and 4 * (info["E_x"] + info["E_z"]) < 65536
    if cslot16 and not force_generic and (info["dv_x"], info["dc"]) in ((3, 6), (4, 8)):
        return (info["dv_x"], info["dc"])
    md = int(np.asarray(hx).sum(1).max())
    return (0, 8) if md <= 8 else (0, 16) if md <= 16 else (0, 0)


def noisy(hx, B, p, seed):
    """BSC(p) noise and its syndrome."""
    e = (np.random.RandomState(seed).rand(B, hx.shape[1]) < p).astype(np.int64)
    return e, (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)


def noise_syndromes(hx, B, p, seed):
    return noisy(hx, B, p, seed)[1]


def informed_edge_channel(hx, e, seed):
    """The magnitudes of edge_channel (the +-20 clip and its neighbours, zeros, subnormals, infinities among moderate values) with signs
    that know half of the noise: a noisy bit's prior says "error" with probability 1/2, every other prior says "no error".  Unrelated
    priors would leave every sample unsolved; these let solutions, and their weights, occur under per-bit logits too."""
    mag = np.abs(edge_channel(hx, e.shape[0], seed))
    told = (e != 0) & (np.random.RandomState(seed ^ 0x55).rand(*e.shape) < 0.5)
    return np.where(told, mag, -mag).astype(F32)


def both(g, hx, synd, gamma, pre, leg, stop, factor, B=None, **llr):
    """Kernel and restatement on the same inputs; asserts identical outputs, returns the restatement's (hard, stats, solutions)."""
    gl = {k: (to_gpu(v) if k == "llr_ch" else v) for k, v in llr.items()}
    hard, stats = g.relay_decode(None if synd is None else to_gpu(synd), to_gpu(gamma), pre, leg, stop, factor, B=B, **gl)
    h0, s0, sols = R.relay_decode(hx, synd, gamma, pre, leg, stop, factor, B=B, **llr)
    assert stats.dtype == torch.int32 and hard.dtype == torch.uint8
    s1, h1 = stats.cpu().numpy(), hard.cpu().numpy()
    print("found", s0[:, 0].tolist(), "leg", s0[:, 2].tolist(), "k", s0[:, 3].tolist())
    assert np.array_equal(s0, s1), (np.nonzero((s0 != s1).any(1))[0], s0[(s0 != s1).any(1)], s1[(s0 != s1).any(1)])
    assert np.array_equal(h0, h1)
    return h0, s0, sols


def fuzz(g, hx, rng):
    """B in 1..70, pre_iter and leg_iter <= 12, 1 / 2 / 5 legs, stop_nconv 1 and 3, three factors, a constant logit and per-bit logits with
    the edge values of edge_channel; gamma rows with 0, negative values and values above 0.5."""
    n = hx.shape[1]
    for legs, factor in ((1, 1.0), (2, 0.8), (5, 0.625)):
        for stop in (1, 3):
            B, pre, leg = int(rng.randint(1, 71)), int(rng.randint(1, 13)), int(rng.randint(1, 13))
            e, synd = noisy(hx, B, 0.06, int(rng.randint(1 << 30)))
            gamma = mixed_gamma(legs, n, int(rng.randint(1 << 30)))
            both(g, hx, synd, gamma, pre, leg, stop, factor, llr_const=-2.197)
            both(g, hx, synd, gamma, pre, leg, stop, factor, llr_ch=informed_edge_channel(hx, e, int(rng.randint(1 << 30))))


# gb_rand_3a / 4a: (3,6) and (4,8) regular, l = 31 / 29; gb_rand_6 / 9: check degree 12 / 18; irregular graphs of max degree 8, 16, 30
FUZZ = {"gb_rand_3a": (3, 6), "gb_rand_4a": (4, 8), "gb_rand_6": (0, 16), "gb_rand_9": (0, 0), "irr_8": (0, 8), "irr_16": (0, 16),
        "irr_30": (0, 0)}
assert set(FUZZ.values()) == {(3, 6), (4, 8), (0, 8), (0, 16), (0, 0)}, "the cases must reach every relay_kernel instantiation"


@pytest.mark.parametrize("key", list(FUZZ))
def test_every_instantiation(key):
    g, _, hx = graphs(key, dict(CASES)[key])
    assert instantiation(g, hx) == FUZZ[key]
    fuzz(g, hx, np.random.RandomState(zlib.crc32(key.encode())))


def test_force_generic_on_a_regular_graph():
    g, _, hx = named("gb48")
    assert instantiation(g, hx) == (4, 8) and instantiation(g, hx, force_generic=True) == (0, 8)
    g.force_generic(True)
    try:
        fuzz(g, hx, np.random.RandomState(17))
    finally:
        g.force_generic(False)


# ---- several codewords per workgroup ---------------------------------------------------------------------------------------------------
def test_codewords_of_one_workgroup_stop_at_different_legs():
    g, _, hx = named("rsurf5")
    cpb = g.info()["codewords_per_block"]
    assert cpb > 1
    n, legs = hx.shape[1], 4
    gamma = mixed_gamma(legs, n, 3)
    for B in (1, cpb - 1, cpb, cpb + 1):
        synd = noise_syndromes(hx, B, 0.15, 40)  # the same first rows for every B
        _, stats, _ = both(g, hx, synd, gamma, 5, 4, 1, 0.8, llr_const=_llr_const(0.15))
        if B >= cpb - 1:
            first = stats[:cpb]  # the first workgroup
            assert (first[:, 2] == 0).any(), "no sample of the workgroup stops in the first leg"
            assert ((first[:, 0] == 0) | (first[:, 2] == legs - 1)).any(), "no sample of the workgroup uses every leg"
            assert len(set(map(tuple, first[:, 2:]))) >= 3, "the workgroup's samples must stop at different steps"
    # stop_nconv = 3: solved samples go on into further legs while others of the workgroup are finished
    synd = noise_syndromes(hx, cpb + 1, 0.15, 40)
    both(g, hx, synd, gamma, 5, 4, 3, 0.8, llr_const=_llr_const(0.15))


@pytest.mark.parametrize("tpc,cpb", [(1, 64), (2, 32), (64, 2)])
def test_set_launch_geometries(tpc, cpb):
    g, _, hx = named("rsurf5")
    g.set_launch(tpc, cpb)
    try:
        synd = noise_syndromes(hx, cpb + 3, 0.15, 41)
        both(g, hx, synd, mixed_gamma(3, hx.shape[1], 4), 4, 3, 2, 0.8, llr_const=_llr_const(0.15))
    finally:
        g.set_launch(0, 0)


# ---- syndromes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gb48", "rsurf5"])
def test_zero_and_null_syndrome(name):
    g, _, hx = named(name)
    B, n = 9, hx.shape[1]
    gamma = to_gpu(mixed_gamma(3, n, 5))
    zero = np.zeros((B, hx.shape[0]), np.uint8)
    h0, s0, _ = both(g, hx, zero, mixed_gamma(3, n, 5), 6, 5, 1, 0.8, llr_const=-2.0)
    assert not h0.any() and np.array_equal(s0, np.tile(np.array([1, 0, 0, 1], np.int32), (B, 1)))
    hz, sz = g.relay_decode(to_gpu(zero), gamma, 6, 5, 1, 0.8, llr_const=-2.0)
    hn, sn = g.relay_decode(None, gamma, 6, 5, 1, 0.8, llr_const=-2.0, B=B)
    assert torch.equal(hz, hn) and torch.equal(sz, sn)
    assert np.array_equal(hn.cpu().numpy(), h0) and np.array_equal(sn.cpu().numpy(), s0)
    both(g, hx, None, mixed_gamma(3, n, 5), 6, 5, 1, 0.8, llr_ch=edge_channel(hx, B, 8))


def test_syndrome_outside_the_column_space():
    """gb48's hx has dependent rows: a syndrome s with u.s = 1 for a u in the left kernel (u H = 0) is the syndrome of no error, so
    no test can pass: found = 0, the output is the decision of the last test of the last leg."""
    g, _, hx = named("gb48")
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


# ---- anchor ----------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_one_leg_is_bp2_minsum_on_the_gpu():
    g, _, hx = named("ghp882")
    B, T, n = 19, 12, hx.shape[1]
    synd = to_gpu(noise_syndromes(hx, B, 0.03, 5))
    gamma = torch.zeros((1, n), dtype=torch.float32, device=g.device)
    for factor in (1.0, 0.8):
        hard, stats = g.relay_decode(synd, gamma, T, T, 1, factor, llr_const=_llr_const(0.03))
        ks = stats[:, 3].cpu().numpy()
        assert len(set(ks.tolist())) >= 2
        for k in sorted(set(ks.tolist())):
            _, h0 = g.bp2_decode(synd, int(k), "minsum", factor, llr_const=_llr_const(0.03), want_soft=False)
            sel = torch.from_numpy(ks == k).to(g.device)
            assert torch.equal(h0[sel], hard[sel]), (factor, k)


# ---- LDS -------------------------------------------------------------------------------------------------------------------------------
def test_dynamic_lds_above_48k():
    hx = hp_big_hx()
    g, _, _ = graphs("hp_big_hx", lambda: _bare(hx))
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
        g.relay_decode(synd, gamma, 3, 3, 1, 0.8, llr_const=-2.0)


def test_posteriors_count_against_the_budget():
    """Messages that fit binary BP's budget with no room left for the n posteriors: bp2_decode runs, relay_decode refuses."""
    E = LDS_BUDGET // 4
    hx = lds_hx(E)
    g, _, _ = graphs(("lds", E), lambda: _bare(hx))
    assert bp2_lds_bytes(E, 1) <= LDS_BUDGET < relay_lds_bytes(E, hx.shape[1], 1)
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    g.bp2_decode(synd, 1, "minsum", 0.8, llr_const=-2.0)
    with pytest.raises(ValueError, match="code too large for the LDS-resident kernel"):
        g.relay_decode(synd, torch.zeros((1, hx.shape[1]), dtype=torch.float32, device=g.device), 3, 3, 1, 0.8, llr_const=-2.0)


def test_argument_errors():
    g, _, hx = named("gb48")
    n = hx.shape[1]
    synd = torch.zeros((2, hx.shape[0]), dtype=torch.uint8, device=g.device)
    gamma = torch.zeros((2, n), dtype=torch.float32, device=g.device)
    for pre, leg, stop in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError, match=">= 1"):
            g.relay_decode(synd, gamma, pre, leg, stop)
    with pytest.raises(ValueError, match="gamma"):
        g.relay_decode(synd, gamma[:, :n - 1].contiguous(), 2, 2, 1)
    with pytest.raises(ValueError, match="gamma"):
        g.relay_decode(synd, gamma.double(), 2, 2, 1)
    with pytest.raises(ValueError, match="syndrome"):
        g.relay_decode(synd[:, :-1].contiguous(), gamma, 2, 2, 1)


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def test_relay_bp_decoder_class():
    import feedback_gnn_amd as F
    hx = np.asarray(code("gb48").hx)
    n = hx.shape[1]
    dec = F.RelayBPDecoder(hx, gamma0=0.125, pre_iter=8, num_sets=3, set_max_iter=6, stop_nconv=2, normalization_factor=0.8, seed=5)
    same = F.RelayBPDecoder(hx, pre_iter=8, num_sets=3, set_max_iter=6, seed=5, graph=dec.graph)
    other = F.RelayBPDecoder(hx, pre_iter=8, num_sets=3, set_max_iter=6, seed=6, graph=dec.graph)
    gam = dec.gamma.cpu().numpy()
    assert gam.shape == (4, n) and gam.dtype == F32 and (gam[0] == F32(0.125)).all()
    assert gam[1:].min() >= -0.24 and gam[1:].max() <= 0.66 and gam[1:].min() < 0 and gam[1:].max() > 0.5
    assert torch.equal(dec.gamma, same.gamma) and not torch.equal(dec.gamma, other.gamma)
    expect = np.random.default_rng(5).uniform(-0.24, 0.66, size=(3, n)).astype(F32)
    assert np.array_equal(gam[1:], expect)
    B = 23
    synd = noise_syndromes(hx, B, 0.08, 9)
    llr = np.full((B, n), _llr_const(0.08), F32)
    e_hat = dec((to_gpu(llr), to_gpu(synd.T.copy())))
    hard, stats = dec.graph.relay_decode(to_gpu(synd), dec.gamma, 8, 6, 2, 0.8, llr_ch=to_gpu(llr))
    assert e_hat.dtype == torch.float32 and tuple(e_hat.shape) == (B, n)
    assert torch.equal(e_hat, hard.to(torch.float32)) and torch.equal(dec.last_stats, stats)
    h0, s0, _ = R.relay_decode(hx, synd, gam, 8, 6, 2, 0.8, llr_ch=llr)
    assert np.array_equal(hard.cpu().numpy(), h0) and np.array_equal(stats.cpu().numpy(), s0)
    dec.gamma = np.zeros((4, n))
    assert dec.gamma.dtype == torch.float32 and not dec.gamma.any() and dec.gamma.device == dec.graph.device
    with pytest.raises(ValueError, match="gamma must have shape"):
        dec.gamma = np.zeros((3, n))


def test_bp2_relay_model():
    import feedback_gnn_amd as F
    c = code("gb126")
    hx, logical = np.asarray(c.hx), np.asarray(c.hz_perp)
    dec = F.RelayBPDecoder(hx, pre_iter=10, num_sets=3, set_max_iter=8, normalization_factor=0.8, seed=1)
    model = F.BP2_Relay_Model(hx, logical, dec, seed=SEED)
    B, p = 64, 0.06
    s_hat, ls_hat = model(B, p)
    noise, est, stats = model.last_noise.cpu().numpy(), model.last_estimate.cpu().numpy(), model.last_stats.cpu().numpy()
    assert tuple(s_hat.shape) == (B, hx.shape[0]) and tuple(ls_hat.shape) == (B, logical.shape[0])
    synd = (noise.astype(np.int64) @ hx.T.astype(np.int64) % 2).astype(np.uint8)
    h0, s0, _ = R.relay_decode(hx, synd, dec.gamma.cpu().numpy(), 10, 8, 1, 0.8, llr_const=_llr_const(p))
    assert np.array_equal(est, h0) and np.array_equal(stats, s0)
    res = noise ^ est
    solved = stats[:, 0] > 0
    assert solved.any() and not solved.all(), "the batch must hold solved and unsolved samples"
    assert np.array_equal(s_hat.cpu().numpy(), res.astype(np.int64) @ hx.T.astype(np.int64) % 2)
    assert np.array_equal(s_hat.cpu().numpy().any(1), ~solved)
    assert np.array_equal(ls_hat.cpu().numpy(), res.astype(np.int64) @ logical.T.astype(np.int64) % 2)
    assert model.last_num_unsolved == int((~solved).sum())
    model(B, p)
    assert not np.array_equal(noise, model.last_noise.cpu().numpy()), "a second call draws the next samples"
