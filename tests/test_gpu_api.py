"""GPU tests of the reference-named Python classes (call contracts, shapes, dtypes, error behaviour) and the
published statistical known answers reproduced through them."""
import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
from helpers import WEIGHTS_882, code, llr_const, oracle_library_forms

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def _syndromes(name, p, B, first=0):
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, p, first, B)
    sx, sz = og.syndrome(ex, ez)
    return og, ex, ez, sx, sz


def test_qldpcbpdecoder_stage_one_contract():
    """decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs])) -> 7-tuple (decoding_q.py:792-793)."""
    c = code("ghp882")
    B = 20
    og, ex, ez, sx, sz = _syndromes("ghp882", 0.08, B)
    dec = F.QLDPCBPDecoder(code=c, num_iter=32, normalization_factor=1.0, cn_type="boxplus-phi", stage_one=True)
    llr = torch.full((B, 3, c.N), llr_const(0.05), dtype=torch.float32, device="cuda")
    out = dec((llr, torch.from_numpy(sx.T.astype(np.int64)).cuda(), torch.from_numpy(sz.T.astype(np.int64)).cuda()))
    llrx, llry, llrz, x_hat, z_hat, x_logit, z_logit = out
    assert llrx.shape == (B, c.N) and x_logit.shape == (c.hz.shape[0], B) and z_logit.shape == (c.hx.shape[0], B)
    assert x_hat.dtype == torch.int64 and z_hat.dtype == torch.float64  # decoding_q.py:788-790
    o = og.bp4_decode(sx, sz, 32, "boxplus-phi", 1.0, llr_const=llr_const(0.05))
    assert np.array_equal(o["llr"][:, 0], llrx.cpu().numpy()) and np.array_equal(o["llr"][:, 1], llry.cpu().numpy())
    assert np.array_equal(o["llr"][:, 2], llrz.cpu().numpy())
    assert np.array_equal(o["x_hat"], x_hat.cpu().numpy()) and np.array_equal(o["z_hat"], z_hat.cpu().numpy().astype(np.uint8))
    assert np.array_equal(o["x_logit"].T, x_logit.cpu().numpy()) and np.array_equal(o["z_logit"].T, z_logit.cpu().numpy())
    # default (non-stage) mode returns (x_hat, z_hat) only; default cn_type is 'boxplus', factor 0.625, 32 iterations
    dec0 = F.QLDPCBPDecoder(code=c)
    xh, zh = dec0((llr, torch.from_numpy(sx.T.copy()).cuda(), torch.from_numpy(sz.T.copy()).cuda()))
    o0 = oracle_library_forms("ghp882", False).bp4_decode(sx, sz, 32, "boxplus", 0.625, llr_const=llr_const(0.05))
    assert np.array_equal(o0["x_hat"], xh.cpu().numpy()) and np.array_equal(o0["z_hat"], zh.cpu().numpy().astype(np.uint8))


@pytest.mark.parametrize("cn_type", ["boxplus", "boxplus-phi"])
def test_baseline_configs0_literal_point(cn_type):
    """BASELINE.json configs[0], literally: [[882,24]] quaternary BP, 32 iterations, batch 256, p = 0.05 — the reference's
    CPU-runnable case, `Sandwich_BP_GNN_Evaluation_Model(code, [QLDPCBPDecoder(code, num_iter=32, stage_one=True)], [], num_layers=1)
    .call(256, 0.05)` with the class defaults cn_type='boxplus', normalization_factor=0.625 (decoding_q.py:18-22) and with the
    notebooks' 'boxplus-phi' (QLDPC.ipynb cell 11): noise, syndromes, decoder outputs, residual check and counters against the
    oracle, exactly (what tools/bench_c1.py times)."""
    c = code("ghp882")
    B, p = 256, 0.05
    og, ex, ez, sx, sz = _syndromes("ghp882", p, B)
    dec = F.QLDPCBPDecoder(code=c, num_iter=32, cn_type=cn_type, normalization_factor=0.625, stage_one=True)
    model = F.Sandwich_BP_GNN_Evaluation_Model(c, [dec], [], num_layers=1, seed=SEED)  # p0 = 0.05 (feedback_gnn.py:265)
    s_hat, ls_hat = model(B, p)
    o = og.bp4_decode(sx, sz, 32, cn_type, 0.625, llr_const=llr_const(0.05))
    s0, l0, f0 = og.residual(ex, ez, o["x_hat"], o["z_hat"])
    assert s_hat.shape == (B, 882) and ls_hat.shape == (B, 906)  # 441 + 441 checks, 453 + 453 rows of hx_perp / hz_perp
    assert np.array_equal(s0, s_hat.cpu().numpy()) and np.array_equal(l0, ls_hat.cpu().numpy())
    # the decoder call itself at that point: marginals, decisions, soft syndromes
    g = dec.graph
    out = g.bp4_decode(torch.from_numpy(sx).cuda(), torch.from_numpy(sz).cuda(), 32, cn_type, 0.625, llr_const=llr_const(0.05))
    for k in ("llr", "x_hat", "z_hat", "x_logit", "z_logit"):
        assert np.array_equal(o[k], out[k].cpu().numpy()), k
    counts = model.mc_step(B, p)  # the next 256 samples of the stream, counted on the device
    ex2, ez2 = og.pauli_noise(SEED, p, B, B)
    sx2, sz2 = og.syndrome(ex2, ez2)
    o2 = og.bp4_decode(sx2, sz2, 32, cn_type, 0.625, llr_const=llr_const(0.05))
    f2 = og.residual(ex2, ez2, o2["x_hat"], o2["z_hat"])[2]
    assert counts.tolist() == [int((f2 & 1).sum()), int(((f2 >> 1) & 1).sum()), B]
    assert int((f0 & 1).sum()) + int((f2 & 1).sum()) > 0  # p = 0.05 with factor 0.625 leaves a few flagged samples in 512


def test_qldpcbpdecoder_errors():
    c = code("steane")
    dec = F.QLDPCBPDecoder(code=c, num_iter=4, stage_one=True)
    sx = torch.zeros((3, 5), dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError, match="Invalid input dtype"):
        dec((torch.zeros((5, 3, 7), dtype=torch.float64, device="cuda"), sx, sx))
    with pytest.raises(ValueError, match="Last dimension must be of length n"):
        dec((torch.zeros((5, 3, 8), dtype=torch.float32, device="cuda"), sx, sx))
    with pytest.raises(ValueError):
        dec((torch.zeros((5, 3, 7), dtype=torch.float32, device="cuda"), sx[:2], sx))


def test_stage_two_logit_trace():
    """trainable/stage_two return mode: llr_hat[2*it], [2*it+1] = soft syndromes after `it` iterations."""
    name, B, IT = "gb48", 9, 5
    c = code(name)
    og, ex, ez, sx, sz = _syndromes(name, 0.06, B)
    dec = F.QLDPCBPDecoder(code=c, num_iter=IT, normalization_factor=0.8, cn_type="boxplus-phi", stage_two=True)
    rng = np.random.RandomState(0)
    llr = rng.uniform(0.5, 4.0, size=(B, 3, c.N)).astype(np.float32)
    hat, x_hat, z_hat = dec((torch.from_numpy(llr).cuda(), torch.from_numpy(sx.T.copy()).cuda(), torch.from_numpy(sz.T.copy()).cuda()))
    assert hat.shape == (2 * IT + 2, c.hz.shape[0], B)
    for it in range(IT + 1):
        o = og.bp4_decode(sx, sz, it, "boxplus-phi", 0.8, llr_ch=llr)
        assert np.array_equal(o["x_logit"].T, hat[2 * it].cpu().numpy()), it
        assert np.array_equal(o["z_logit"].T, hat[2 * it + 1].cpu().numpy()), it
    assert np.array_equal(o["x_hat"], x_hat.cpu().numpy())


@pytest.mark.parametrize("name,cn_type,factor,IT,generic", [("ghp882", "boxplus-phi", 1.0, 16, False), ("ghp882", "boxplus-phi", 0.8, 5, True),
                                                            ("ghp1270", "boxplus-phi", 1.0, 7, False), ("ghp882", "minsum", 0.8, 6, False),
                                                            ("ghp882", "boxplus", 0.625, 6, False), ("gb48", "boxplus-phi", 0.9, 9, False),
                                                            ("rsurf5", "minsum", 1.0, 4, False), ("gb254", "boxplus", 0.7, 3, False)])
def test_one_launch_trace_equals_the_chain_of_single_iteration_launches(name, cn_type, factor, IT, generic):
    """fgnn_bp4_decode_trace (one launch that records the soft syndromes and the message tape after every iteration) against the
    round-1/2 form of the same thing: IT + 1 chained fgnn_bp4_decode launches of 0, 1, 1, ... iterations through msg_init / msg_out
    — bit for bit, on the degree-regular kernel, the runtime-degree kernel, constant and per-qubit channel LLRs, restarts from given
    messages; and both against the oracle run with k iterations."""
    B = 13
    og, ex, ez, sx, sz = _syndromes(name, 0.07, B, first=321)
    c = code(name)
    from helpers import gpu_graph
    g = gpu_graph(name)
    tsx, tsz = torch.from_numpy(sx).cuda(), torch.from_numpy(sz).cuda()
    rng = np.random.RandomState(2)
    llr = rng.uniform(0.5, 4.0, size=(B, 3, c.N)).astype(np.float32)
    init = (rng.uniform(-3, 3, size=(B, g.E_x)).astype(np.float32), rng.uniform(-3, 3, size=(B, g.E_z)).astype(np.float32))
    g.force_generic(generic)
    try:
        for llr_ch, L0, msg_init in ((None, llr_const(0.05), None), (llr, 0.0, None), (llr, 0.0, init)):
            t_llr = None if llr_ch is None else torch.from_numpy(llr_ch).cuda()
            t_init = None if msg_init is None else tuple(torch.from_numpy(a).cuda() for a in msg_init)
            tr = g.bp4_decode_trace(tsx, tsz, IT, cn_type, factor, llr_ch=t_llr, llr_const=L0, msg_init=t_init, want_tape=True)
            msgs = t_init
            for k in range(IT + 1):
                o = g.bp4_decode(tsx, tsz, 0 if k == 0 else 1, cn_type, factor, llr_ch=t_llr, llr_const=L0, msg_init=msgs, return_msgs=True)
                msgs = (o["msg_x"], o["msg_z"])
                assert torch.equal(o["x_logit"], tr["x_logit"][k]) and torch.equal(o["z_logit"], tr["z_logit"][k]), (k, "logits")
                assert torch.equal(o["msg_x"], tr["tape_x"][k]) and torch.equal(o["msg_z"], tr["tape_z"][k]), (k, "tape")
            for key in ("llr", "x_hat", "z_hat"):
                assert torch.equal(o[key], tr[key]), key
            for k in (0, 1, IT):
                ref = og.bp4_decode(sx, sz, k, cn_type, factor, llr_ch=llr_ch, llr_const=L0, msg_init=msg_init, return_msgs=True)
                assert np.array_equal(ref["x_logit"], tr["x_logit"][k].cpu().numpy()) and np.array_equal(ref["msg_z"], tr["tape_z"][k].cpu().numpy())
            assert np.array_equal(ref["llr"], tr["llr"].cpu().numpy()) and np.array_equal(ref["x_hat"], tr["x_hat"].cpu().numpy())
    finally:
        g.force_generic(False)
    with pytest.raises(ValueError):
        g.bp4_decode_trace(tsx, tsz, 2, "no-such-rule")


def test_feedback_gnn_class_and_weights():
    c = code("ghp882")
    B = 6
    og, ex, ez, sx, sz = _syndromes("ghp882", 0.1, B)
    G = F.Feedback_GNN(code=c, num_msg_dims=20, num_hidden_units=40, num_mlp_layers=2, reduce_op="mean", activation="tanh",
                       use_bias=True)
    assert G.count_params() == 3923
    w0 = G.get_weights()
    assert np.all(w0[0] == 0) and np.all(w0[1] == 1)  # zeros kernel / ones bias of _llr_inv_embed (feedback_gnn.py:115-116)
    F.load_weights(G, "./sionna/fec/ldpc/weights/feedback_GNN_n882_k24_wt_4_60_iter_64_16_mixed.npy")
    w = G.get_weights()
    o = og.bp4_decode(sx, sz, 64, "boxplus-phi", 1.0, llr_const=llr_const(0.05))
    h_vn = torch.from_numpy(np.ascontiguousarray(o["llr"].transpose(0, 2, 1))).cuda()  # [bs,n,3]
    out = G((h_vn, torch.from_numpy(o["z_logit"].T.copy()).cuda(), torch.from_numpy(o["x_logit"].T.copy()).cuda(),
             torch.from_numpy(sx.T.astype(np.int64)).cuda(), torch.from_numpy(sz.T.astype(np.int64)).cuda()))
    assert out.shape == (B, c.N, 3)
    ref = og.feedback_gnn(w, o["llr"], o["z_logit"], o["x_logit"], sx, sz)
    assert np.array_equal(ref.transpose(0, 2, 1), out.cpu().numpy())
    G16 = F.Feedback_GNN(code=c, num_msg_dims=16, num_hidden_units=40, num_mlp_layers=2, use_bias=True, graph=G.graph)
    assert not G16.is_shipped_architecture and G16.count_params() == 40 * 3 + 3 + 2 * (4 * 40 + 40 + 40 * 16 + 16) + 35 * 40 + 40
    with pytest.raises(NotImplementedError):  # beyond the runtime-shaped kernel's limits
        F.Feedback_GNN(code=c, num_msg_dims=64, num_hidden_units=40, num_mlp_layers=2, use_bias=True, graph=G.graph)


def _model(c, iters, compact=False, **kw):
    d0 = F.QLDPCBPDecoder(code=c, num_iter=iters[0], normalization_factor=1.0, cn_type="boxplus-phi", stage_one=True)
    decs = [d0] + [F.QLDPCBPDecoder(code=c, num_iter=it, normalization_factor=1.0, cn_type="boxplus-phi", stage_one=True,
                                    graph=d0.graph) for it in iters[1:]]
    G = F.Feedback_GNN(code=c, num_msg_dims=20, num_hidden_units=40, num_mlp_layers=2, reduce_op="mean", activation="tanh",
                       use_bias=True, graph=d0.graph)
    F.load_weights(G, WEIGHTS_882)
    return F.Sandwich_BP_GNN_Evaluation_Model(c, decs, [G] * (len(iters) - 1), num_layers=len(iters), compact=compact, **kw)


def test_sandwich_model_call_contract_and_sharding():
    c = code("ghp882")
    m = _model(c, [64, 16])
    s_hat, ls_hat = m(48, 0.1)
    assert s_hat.shape == (48, 882) and ls_hat.shape == (48, 906) and s_hat.dtype == torch.uint8
    # successive calls draw fresh samples; two ranks of a world of 2 draw the disjoint halves of the same stream
    s2, _ = m(48, 0.1)
    assert not torch.equal(s_hat, s2)
    a = _model(c, [64, 16], rank=0, world_size=2).decode(24, 0.1)
    b = _model(c, [64, 16], rank=1, world_size=2).decode(24, 0.1)
    full = _model(c, [64, 16]).decode(48, 0.1)
    assert torch.equal(torch.cat([a["noise_x"], b["noise_x"]]), full["noise_x"])
    assert torch.equal(torch.cat([a["x_hat"], b["x_hat"]]), full["x_hat"])
    # flagged implies logical (a non-zero syndrome residual is never a stabilizer)
    assert bool(((s_hat.any(1)) <= (ls_hat.any(1))).all())


@pytest.mark.parametrize("p,expect,total", [(0.14, 2375 / 5000, 5000), (0.12, 396 / 5000, 5000), (0.10, 113 / 30000, 30000)])
def test_published_bler_rows_three_round_sandwich(p, expect, total):
    """examples/n882.ipynb cell 2: [[882,24]], (64, G,16, G,16, G,16), factor 1.0, p0=0.05.  Same sample counts as
    the reference's rows; acceptance = binomial 4-sigma band around the published rate (two independent draws)."""
    c = code("ghp882")
    m = _model(c, [64, 16, 16, 16], compact=True)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    m.mc_step(total, p, counts)
    fl, bl, n = counts.cpu().numpy()
    assert n == total and fl == bl  # the reference's table has Flagged == BLER on these rows
    sigma = np.sqrt(expect * (1 - expect) / total) * np.sqrt(2)
    assert abs(bl / total - expect) < 4 * sigma + 2 / total, (bl, total, expect)


def test_sim_ber_on_gpu_reaches_target():
    c = code("ghp882")
    m = _model(c, [64, 16])
    flagged, bler = F.sim_ber(m, [0.14, 0.12], batch_size=2000, max_mc_iter=20, num_target_block_errors=100, verbose=False)
    st = F.sim_ber.last
    assert (st["status"] == 4).all() and (st["block_errors"] >= 100).all()
    assert 0.3 < bler[0] < 0.85 and 0.03 < bler[1] < 0.3


def test_sim_ber_device_counters_equal_the_per_batch_path():
    """misc.py:636-738 on the product's fast path: counters stay on the device, the host reads a ring of per-batch snapshots only
    when the target could have been reached, and the stopping rule is applied to the snapshots in order — flag errors, block
    errors, block counts and status of every point equal the per-batch (array-returning) path's, compact or not."""
    c = code("ghp882")
    for compact in (False, True):
        ref_m, fast_m = _model(c, [64, 16], compact=compact), _model(c, [64, 16], compact=compact)
        F.sim_ber(ref_m, [0.13, 0.11, 0.09], batch_size=1500, max_mc_iter=12, num_target_block_errors=100, verbose=False,
                  early_stop=False, device_counters=False)
        ref = {k: np.array(v).copy() for k, v in F.sim_ber.last.items()}
        assert not F.sim_ber.last["device_counters"]
        F.sim_ber(fast_m, [0.13, 0.11, 0.09], batch_size=1500, max_mc_iter=12, num_target_block_errors=100, verbose=False,
                  early_stop=False)
        assert F.sim_ber.last["device_counters"]
        for k in ("flag_errors", "block_errors", "num_blocks", "status"):
            assert np.array_equal(ref[k], F.sim_ber.last[k]), (compact, k, ref[k], F.sim_ber.last[k])
        assert ref_m._next_sample == fast_m._next_sample
        assert ref["status"][0] == 4 and ref["status"][2] == 1  # a point that reaches the target and one that hits max iter


@pytest.mark.parametrize("rank,world,compact,wt", [(0, 1, False, False), (0, 1, True, False), (1, 3, True, False), (2, 3, False, True)])
def test_mc_steps_is_k_sequential_mc_steps_in_one_launch(rank, world, compact, wt):
    """`mc_steps` decodes k batches as one launch and takes the counters batch by batch: every ring row, the final counters and the
    stream position equal those of k `mc_step` calls — on one rank and on a rank of a sharded stream (whose batches are not
    contiguous in the global Philox stream), compacted or not, i.i.d. and fixed-weight noise."""
    c = code("ghp882")
    kw = dict(wt=True, p0=0.05) if wt else {}
    p = 45 if wt else 0.11
    a = _model(c, [64, 16], compact=compact, rank=rank, world_size=world, **kw)
    b = _model(c, [64, 16], compact=compact, rank=rank, world_size=world, **kw)
    k, bs = 5, 700
    ca = torch.zeros(3, dtype=torch.int64, device=a.graph.device)
    snaps = []
    for _ in range(k):
        a.mc_step(bs, p, ca)
        snaps.append(ca.clone())
    cb = torch.zeros(3, dtype=torch.int64, device=b.graph.device)
    ring = torch.zeros((k, 3), dtype=torch.int64, device=b.graph.device)
    b.mc_steps(bs, p, k, cb, ring)
    assert torch.equal(torch.stack(snaps), ring) and torch.equal(ca, cb)
    assert a._next_sample == b._next_sample == k * bs * world
    assert int(ca[0]) > 0 and int(ca[2]) == k * bs
    # and it continues from prior counters
    b.mc_steps(bs, p, 2, cb, ring[:2])
    a.mc_step(bs, p, ca); a.mc_step(bs, p, ca)
    assert torch.equal(ca, cb) and int(ring[1][2]) == (k + 2) * bs


def test_sim_ber_fused_launches_equal_the_per_batch_path():
    """The reference's scripts keep batch_size = 5 000 (n882.py:45); sim_ber then decodes fuse_samples // batch_size deferred batches per
    launch.  Counters, status and stream position equal the per-batch path's, and the fused path is the one that ran."""
    c = code("ghp882")
    ref_m, fused_m, plain_m = (_model(c, [64, 16], compact=True) for _ in range(3))
    pts, kw = [0.13, 0.10, 0.08], dict(batch_size=500, max_mc_iter=40, num_target_block_errors=60, verbose=False, early_stop=False)
    F.sim_ber(ref_m, pts, device_counters=False, **kw)
    ref = {k: np.array(v).copy() for k, v in F.sim_ber.last.items()}
    calls = []
    orig = fused_m.mc_steps
    fused_m.mc_steps = lambda *a, **k2: (calls.append(a[2]), orig(*a, **k2))[1]
    F.sim_ber(fused_m, pts, fuse_samples=4000, **kw)
    fused = {k: np.array(v).copy() for k, v in F.sim_ber.last.items()}
    F.sim_ber(plain_m, pts, fuse_samples=0, **kw)
    for k in ("flag_errors", "block_errors", "num_blocks", "status"):
        assert np.array_equal(ref[k], fused[k]) and np.array_equal(ref[k], F.sim_ber.last[k]), (k, ref[k], fused[k])
    assert ref_m._next_sample == fused_m._next_sample == plain_m._next_sample
    assert calls and max(calls) == 8  # 4000 // 500 batches per launch


def test_sim_ber_with_side_streams_equals_one_stream():
    """A `streams=2` / `streams=3` model under `sim_ber` (device-counter path, with and without fused launches): the snapshots of the
    shared counters are ordered behind the side streams, so every counter, status and the stream position equal the one-stream
    model's — round-4 advisor finding: the ring copies used to race with the side streams' atomic adds."""
    c = code("ghp882")
    pts, kw = [0.13, 0.10], dict(batch_size=700, max_mc_iter=30, num_target_block_errors=80, verbose=False, early_stop=False)
    res = {}
    for streams in (1, 2, 3):
        for fuse in (0, 2800):
            m = _model(c, [64, 16], compact=True, streams=streams, seed=5)
            F.sim_ber(m, pts, fuse_samples=fuse, **kw)
            assert F.sim_ber.last["device_counters"]
            res[(streams, fuse)] = ({k: np.array(F.sim_ber.last[k]).tolist() for k in ("flag_errors", "block_errors", "num_blocks", "status")},
                                    m._next_sample)
    assert res[(1, 0)][0]["status"][0] == 4
    for k, v in res.items():
        assert v == res[(1, 0)], (k, v, res[(1, 0)])


def test_fixed_weight_noise_and_failure_harvesting():
    """Pauli(wt=True) (pauli.py:80-97) and the dataset-harvesting flow of examples/Generate_dataset.ipynb."""
    c = code("ghp882")
    og = oracle_library_forms("ghp882")
    m = _model(c, [64], wt=True, p0=0.05)
    g = m.graph
    ex, ez = g.pauli_noise_wt(SEED, 37, 100, 500)
    oex, oez = og.pauli_noise_wt(SEED, 37, 100, 500)
    assert np.array_equal(oex, ex.cpu().numpy()) and np.array_equal(oez, ez.cpu().numpy())
    wt = (ex | ez).sum(1)
    assert bool((wt == 37).all())
    # X, Y, Z equiprobable
    nx, ny, nz = int((ex & ~ez & 1).sum()), int((ex & ez).sum()), int((~ex & ez & 1).sum())
    for cnt in (nx, ny, nz):
        assert abs(cnt / (500 * 37) - 1 / 3) < 0.02
    # positions uniform: every qubit is hit about 500*37/882 = 21 times
    hits = (ex | ez).sum(0).float()
    assert 5 < float(hits.min()) and float(hits.max()) < 45
    fx, fz = m.failures(4000, 60)  # weight-60 errors: plain BP-64 fails on a visible fraction
    assert fx.shape[1] == 882 and fx.shape == fz.shape and 0 < fx.shape[0] < 4000
    assert bool(((fx | fz).sum(1) == 60).all())


def test_first_and_second_stage_models():
    c = code("ghp882")
    og = oracle_library_forms("ghp882")
    dec1 = F.QLDPCBPDecoder(code=c, num_iter=16, normalization_factor=1.0, cn_type="boxplus-phi", stage_one=True)
    dec2 = F.QLDPCBPDecoder(code=c, num_iter=16, normalization_factor=1.0, cn_type="boxplus-phi", stage_two=True, graph=dec1.graph)
    G = F.Feedback_GNN(code=c, num_msg_dims=20, num_hidden_units=40, num_mlp_layers=2, reduce_op="mean", activation="tanh",
                       use_bias=True, graph=dec1.graph)
    F.load_weights(G, WEIGHTS_882)
    ex, ez = og.pauli_noise(SEED, 0.1, 0, 10)
    sx, sz = og.syndrome(ex, ez)
    stage1 = F.First_Stage_BP_Model(c, dec1, p0=0.05)
    h_vn, lhx, lhz = stage1(torch.from_numpy(ex).cuda(), torch.from_numpy(ez).cuda())
    o = og.bp4_decode(sx, sz, 16, "boxplus-phi", 1.0, llr_const=llr_const(0.05))
    assert np.array_equal(o["llr"].transpose(0, 2, 1), h_vn.cpu().numpy()) and np.array_equal(o["x_logit"].T, lhx.cpu().numpy())
    stage2 = F.Second_Stage_GNN_BP_Model(c, G, dec2, num_iter=16, loss_from=8)
    s_hat, ls_hat, loss = stage2(torch.from_numpy(ex).cuda(), torch.from_numpy(ez).cuda(), h_vn, lhx, lhz)
    assert s_hat.shape == (10, 882) and ls_hat.shape == (10, 906) and loss.dim() == 0 and float(loss) > 0
    # the same number from the oracle's pieces
    nl = og.feedback_gnn(read_w(), o["llr"], o["z_logit"], o["x_logit"], sx, sz)
    ref = 0.0
    for i in range(8, 16):
        oi = og.bp4_decode(sx, sz, i + 1, "boxplus-phi", 1.0, llr_ch=nl)
        for logit, lab in ((oi["x_logit"], 1 - sz), (oi["z_logit"], 1 - sx)):
            z = logit.astype(np.float64)
            ref += np.mean(np.maximum(z, 0) - z * lab + np.log1p(np.exp(-np.abs(z))))
    assert abs(float(loss) - ref) < 1e-4 * max(1.0, ref)


def read_w():
    from feedback_gnn_amd.weights_io import read_weight_list
    return read_weight_list(WEIGHTS_882)


def test_hw_transcendentals_are_opt_in_and_what_they_cost_in_fidelity():
    """FGNN_OPT_HW_TRANSCENDENTALS (v_exp_f32 / v_log_f32, not bit-exact) is off by default.  Switched on — with phi's two clip points
    pinned to the values the reference's known answer fixes (examples/n1270.ipynb cell 12: log 57 + deg * 16.635532) — it reproduces
    the notebook's saturated marginals, converged samples carry bit-identical marginals on all but the few per cent whose chaotic
    transient ended on another member of the same correction class, every differing decision is a stabilizer away, and a published
    error-rate row stays in its band (/root/reference examples/n882.ipynb cell 2: 3 feedback rounds, p = 0.12 -> 396 / 5000).
    The transient bits are no CPU's, which is why the path is opt-in only (bench.py reports the same measurements)."""
    c = code("ghp882")
    m = _model(c, [64, 16, 16, 16])
    g = m.graph
    ex, ez = g.pauli_noise(SEED, 0.06, 9000, 2048)
    sx, sz = g.syndrome(ex, ez)
    L0 = m._llr_const(0.06)
    g.set_saturation_shortcut(False)
    try:
        a = g.bp4_decode(sx, sz, 64, "boxplus-phi", 1.0, llr_const=L0)
        b = g.bp4_decode(sx, sz, 64, "boxplus-phi", 1.0, llr_const=L0)
        assert torch.equal(a["llr"], b["llr"])  # the default path is the exact one and is deterministic
        g.set_hw_transcendentals(True)
        h = g.bp4_decode(sx, sz, 64, "boxplus-phi", 1.0, llr_const=L0)
        hs_hat, hls_hat = m(5000, 0.12)
    finally:
        g.set_hw_transcendentals(False)
        g.set_saturation_shortcut(True)
    assert not torch.equal(a["llr"], h["llr"]), "the opt-in path must really run different arithmetic"
    assert bool(torch.isfinite(h["llr"]).all())
    ones = torch.ones(2048, dtype=torch.uint8, device=g.device)
    both = (g.flag_update(a["x_hat"], a["z_hat"], sx, sz, ones.clone()) == 0) & (g.flag_update(h["x_hat"], h["z_hat"], sx, sz, ones.clone()) == 0)
    assert int(both.sum()) > 1500
    hxp = torch.from_numpy(np.asarray(c.hx_perp)).to(g.device).float()
    hzp = torch.from_numpy(np.asarray(c.hz_perp)).to(g.device).float()
    dx, dz = (a["x_hat"] ^ h["x_hat"]).float(), (a["z_hat"] ^ h["z_hat"]).float()
    equiv = ~(((dx @ hxp.t()) % 2).bool().any(1) | ((dz @ hzp.t()) % 2).bool().any(1))
    same = (a["x_hat"] == h["x_hat"]).all(1) & (a["z_hat"] == h["z_hat"]).all(1)
    assert float(equiv[both].float().mean()) >= 0.999 and float(same[both].float().mean()) >= 0.95
    # same saturated fixed point: marginals of converged samples agree to the north-star tolerance wherever the decisions do
    dl = (a["llr"] - h["llr"]).abs().flatten(1).max(1).values
    assert float((dl[both & same] <= 1e-4).float().mean()) >= 0.99
    assert float(dl[both].median()) <= 1e-4
    # both paths reproduce the notebook's saturation values
    for o in (a, h):
        assert [f"{v:.9g}" for v in o["llr"].amax(dim=(0, 2)).cpu().numpy()] == ["53.9496498", "103.856247", "53.9496498"]
    bler = float(hls_hat.any(1).float().mean())
    assert abs(bler - 396 / 5000) < 4 * np.sqrt(0.0792 * 0.9208 / 5000) * np.sqrt(2), bler


def test_views_and_devices_are_handled_at_the_binding():
    """graph.py passes raw pointers to the C ABI, so layout mistakes must be caught in Python: a correctly shaped but non-contiguous
    READ-ONLY input is copied (same result as its contiguous twin), a non-contiguous IN-PLACE output is refused (a silent copy would
    receive the result), wrong dtypes / shapes / devices raise ValueError, and a bare "cuda" device means torch's current device."""
    from feedback_gnn_amd.graph import TannerGraph
    c = code("gb48")
    g = TannerGraph(c, device="cuda")
    assert g.device == torch.device("cuda", torch.cuda.current_device())
    ex, ez = g.pauli_noise(SEED, 0.08, 0, 64)
    sx, sz = g.syndrome(ex, ez)
    # non-contiguous read-only inputs: [n, B] tensors viewed as [B, n]
    sx2, sz2 = g.syndrome(ex.t().contiguous().t(), ez.t().contiguous().t())
    assert not ex.t().contiguous().t().is_contiguous() and torch.equal(sx, sx2) and torch.equal(sz, sz2)
    o = g.bp4_decode(sx, sz, 8, "boxplus-phi", 0.8, llr_const=llr_const(0.1))
    s1, l1, f1 = g.residual(ex, ez, o["x_hat"], o["z_hat"])
    s2, l2, f2 = g.residual(ex.t().contiguous().t(), ez, o["x_hat"].t().contiguous().t(), o["z_hat"])
    assert torch.equal(s1, s2) and torch.equal(l1, l2) and torch.equal(f1, f2)
    # in-place outputs must be contiguous
    errors = torch.ones(64, dtype=torch.uint8, device=g.device)
    xh_view = o["x_hat"].t().contiguous().t()
    with pytest.raises(ValueError, match="contiguous"):
        g.merge(errors, o["x_hat"], o["z_hat"], xh_view, o["z_hat"].clone())
    with pytest.raises(ValueError, match="contiguous"):
        g.flag_update(o["x_hat"], o["z_hat"], sx, sz, torch.ones(128, dtype=torch.uint8, device=g.device)[::2])
    g.merge(errors, o["x_hat"], o["z_hat"], o["x_hat"].clone(), o["z_hat"].clone())  # the contiguous call goes through
    with pytest.raises(ValueError):
        g.merge(errors.to(torch.int32), o["x_hat"], o["z_hat"], o["x_hat"].clone(), o["z_hat"].clone())  # dtype of `errors`
    with pytest.raises(ValueError):
        g.residual_rows(4, 5, ex[:, :-1], ez, o["x_hat"], o["z_hat"])  # shape
    with pytest.raises(ValueError):
        g.syndrome(ex.cpu(), ez.cpu())  # host tensors: wrong device, no CPU path
    with pytest.raises(ValueError):
        g.count_flags(f1, torch.zeros(3, dtype=torch.int32, device=g.device))


def test_options_round_trip_and_unknown_ids_are_refused():
    """fgnn_graph_set_option: every documented id is accepted with 0 and 1 on a live graph, anything else is an argument error whose text
    says so; the wrappers keep their mirror attributes in step."""
    from feedback_gnn_amd import _lib
    from helpers import LIBRARY_BP4_SHARED_LSE, LIBRARY_GNN_FACTORED, gpu_graph
    g = gpu_graph("gb48")
    L = _lib.lib()
    # the library's defaults (fgnn_internal.h): the raw calls bypass the wrappers' mirror attributes and the graph is shared by the whole
    # session, so each option must be LEFT at its default — options 4 and 5 at 0, the reference's formulas term by term
    defaults = {1: 1, 2: 1, 3: 0, 4: int(LIBRARY_GNN_FACTORED), 5: int(LIBRARY_BP4_SHARED_LSE), 6: 1}
    assert defaults[4] == 0 and defaults[5] == 0
    for opt, dflt in defaults.items():
        for v in (0, 1, dflt):
            assert L.fgnn_graph_set_option(g.handle, opt, v) == 0, opt
    for bad in (0, 7, -1, 1 << 20):
        assert L.fgnn_graph_set_option(g.handle, bad, 1) == -1 and b"unknown option" in L.fgnn_last_error()
    g.set_gnn_stream(False)
    assert g.gnn_stream is False
    g.set_gnn_stream("always")
    assert g.gnn_stream == "always"
    g.set_gnn_stream(True)
    assert g.gnn_stream is True and g.gnn_factored is False and g.bp4_shared_lse is False  # round 6: the re-associations are opt-in
    assert L.fgnn_graph_set_option(g.handle, 6, 3) == -1 and b"0, 1 or 2" in L.fgnn_last_error()


def test_empty_and_single_codeword_batches_through_every_entry_point():
    """Edge cases of the batch dimension: B = 0 (a compacted round with nothing left, an empty shard) must be accepted by every entry
    point and return empty outputs of the right shapes; B = 1 must equal row 0 of a larger launch."""
    from feedback_gnn_amd.graph import GnnBp4Weights, GnnWeights, TannerGraph
    from feedback_gnn_amd.weights_io import read_weight_list
    c = code("ghp882")
    g = TannerGraph(c)
    w = GnnWeights(read_weight_list(WEIGHTS_882), g.device)
    L0 = llr_const(0.05)
    ex0, ez0 = g.pauli_noise(SEED, 0.1, 0, 0)
    assert ex0.shape == (0, g.n)
    sx0, sz0 = g.syndrome(ex0, ez0)
    assert sx0.shape == (0, g.m_x)
    o0 = g.bp4_decode(sx0, sz0, 8, "boxplus-phi", 1.0, llr_const=L0, return_msgs=True)
    assert o0["llr"].shape == (0, 3, g.n) and o0["x_logit"].shape == (0, g.rows_xp) and o0["msg_x"].shape == (0, g.E_x)
    t0 = g.bp4_decode_trace(sx0, sz0, 3, "boxplus-phi", 1.0, llr_const=L0, want_tape=True)
    assert t0["x_logit"].shape == (4, 0, g.rows_xp) and t0["tape_z"].shape == (4, 0, g.E_z)
    assert g.feedback_gnn(w, o0["llr"], o0["z_logit"], o0["x_logit"], sx0, sz0).shape == (0, 3, g.n)
    s0 = g.sandwich_decode(sx0, sz0, [8, 4], [w], L0, compact=True, return_rounds=True)
    assert s0["x_hat"].shape == (0, g.n) and s0["rounds"].shape == (0,)
    r0 = g.residual(ex0, ez0, s0["x_hat"], s0["z_hat"])
    assert r0[0].shape[0] == 0 and r0[2].shape == (0,)
    counts = torch.zeros(3, dtype=torch.int64, device=g.device)
    g.count_flags(r0[2], counts)
    assert counts.tolist() == [0, 0, 0]
    rng = np.random.RandomState(0)
    from feedback_gnn_amd.graph import GNNBP4_SHAPES
    gw = GnnBp4Weights([rng.uniform(-0.3, 0.3, size=s).astype(np.float32) for s in GNNBP4_SHAPES], g.device)
    gb0 = g.gnn_bp4_decode(gw, sx0, sz0, 3)
    assert gb0["llr"].shape == (0, 3, g.n) and gb0["x_logit_all"].shape[:2] == (3, 0)
    s_b2, h_b2 = g.bp2_decode(torch.zeros((0, g.m_x), dtype=torch.uint8, device=g.device), 4, "boxplus-phi", 1.0, llr_const=-1.0)
    assert s_b2.shape == (0, g.n) and h_b2.shape == (0, g.n)
    # the reverse passes (shipped and runtime-shaped) and the forms comparison on an empty batch
    grads0 = g.feedback_gnn_backward(w, o0["llr"], o0["z_logit"], o0["x_logit"], sx0, sz0, o0["llr"])
    assert len(grads0) == 12 and all(float(t.abs().sum()) == 0.0 for t in grads0)
    from feedback_gnn_amd.graph import gnn_weight_shapes
    cfg = (8, 16, 3, "sum", "relu", True)
    wg = GnnWeights([rng.uniform(-0.3, 0.3, size=shp).astype(np.float32) for shp in gnn_weight_shapes(*cfg[:3], cfg[5])], g.device, config=cfg)
    gradsg = g.feedback_gnn_backward(wg, o0["llr"], o0["z_logit"], o0["x_logit"], sx0, sz0, o0["llr"])
    assert len(gradsg) == 18 and all(float(t.abs().sum()) == 0.0 for t in gradsg)
    fa0 = g.forms_agreement(sx0, sz0, [8, 4], [w], L0)
    assert fa0["samples"] == 0 and fa0["decisions_differ"] == 0 and fa0["max_abs_dllr"] == 0.0
    # B = 1 equals row 0 of B = 5
    ex, ez = g.pauli_noise(SEED, 0.1, 7, 5)
    sx, sz = g.syndrome(ex, ez)
    big = g.sandwich_decode(sx, sz, [16, 8], [w], L0, return_llr=True)
    one = g.sandwich_decode(sx[:1].contiguous(), sz[:1].contiguous(), [16, 8], [w], L0, return_llr=True)
    for k in ("x_hat", "z_hat", "llr"):
        assert torch.equal(one[k][0], big[k][0]), k
    tb = g.bp4_decode_trace(sx, sz, 4, "minsum", 0.8, llr_const=L0)
    t1 = g.bp4_decode_trace(sx[:1].contiguous(), sz[:1].contiguous(), 4, "minsum", 0.8, llr_const=L0)
    assert torch.equal(t1["x_logit"][:, 0], tb["x_logit"][:, 0]) and torch.equal(t1["llr"][0], tb["llr"][0])
    gb = g.gnn_bp4_decode(gw, sx, sz, 2)
    g1 = g.gnn_bp4_decode(gw, sx[:1].contiguous(), sz[:1].contiguous(), 2)
    assert torch.equal(g1["llr"][0], gb["llr"][0])


def test_mc_step_on_two_streams_counts_the_same_samples():
    """`Sandwich_BP_GNN_Evaluation_Model(streams=2)`: consecutive batches alternate between two side streams (own workspaces, shared
    atomic counters) so that independent batches overlap on the chip.  Scheduling only: after `join()` the counters equal those of the
    one-stream model over the same global samples, `mc_steps` after `mc_step` (shared workspaces) is ordered by the model itself, and a
    caller's zeroing of the counters on its own stream is ordered before the next batch."""
    from feedback_gnn_amd import QLDPCBPDecoder, Feedback_GNN, Sandwich_BP_GNN_Evaluation_Model, load_weights
    from helpers import gpu_graph
    c = code("ghp882")
    g = gpu_graph("ghp882")
    decs = [QLDPCBPDecoder(code=c, num_iter=it, normalization_factor=1.0, cn_type="boxplus-phi", stage_one=True, graph=g) for it in (24, 8)]
    G = Feedback_GNN(code=c, num_msg_dims=20, num_hidden_units=40, num_mlp_layers=2, reduce_op="mean", activation="tanh", use_bias=True, graph=g)
    load_weights(G, WEIGHTS_882)
    B, p, steps = 1500, 0.10, 7
    res = {}
    for streams in (1, 2, 3):
        m = Sandwich_BP_GNN_Evaluation_Model(c, decs, [G], num_layers=2, seed=77, streams=streams)
        counts = torch.zeros(3, dtype=torch.int64, device=g.device)
        for _ in range(steps):
            m.mc_step(B, p, counts)
        s_hat, ls_hat = m(B, p)             # a direct call while batches are in flight: runs behind them on the caller's stream
        m.join()
        first = counts.clone()
        direct = (int(s_hat.any(1).sum()), int(ls_hat.any(1).sum()))
        counts.zero_()                      # on the caller's stream, after the join
        m.mc_step(B, p, counts)             # must not start before the zeroing
        ring = torch.zeros((2, 3), dtype=torch.int64, device=g.device)
        m.mc_steps(B, p, 2, counts, ring)   # joins the side streams itself before it reuses a workspace
        m.join()
        torch.cuda.synchronize()
        res[streams] = (first.tolist(), counts.tolist(), ring.tolist(), direct)
    assert res[1][0][2] == steps * B and res[1][0][1] > 0
    assert res[2] == res[1] and res[3] == res[1], res


def _numpy_osd0(llr, basis, synd):
    """OSD-0 as bp_osd.py:14-77 states it, one sample: columns sorted by ascending llr (stable), Gauss-Jordan over GF(2) taking for
    every row the first remaining column with a 1, solution on the pivot columns."""
    order = np.argsort(llr, kind="stable")
    a = np.concatenate([basis[:, order], synd[:, None]], axis=1).astype(np.uint8)
    rank, n = basis.shape
    piv = []
    for r in range(rank):
        c = int(np.argmax(a[r, :n]))
        assert a[r, c] == 1, "basis must be full rank"
        piv.append(c)
        rows = np.nonzero(a[:, c])[0]
        rows = rows[rows != r]
        a[rows] ^= a[r]
    e = np.zeros(n, np.uint8)
    e[order[np.asarray(piv)]] = a[:, n]
    return e


@pytest.mark.parametrize("name", ["gb48", "ghp882"])
def test_osd0_decoder_standalone_call(name):
    """`OSD0_Decoder(n)(llr, pcm, s, bs)` as the reference's scripts call it (bp_osd.py:47-77, :147-157): the tiled full-rank basis as a
    batched tensor, syndromes `[rank, bs]` — against a NumPy statement of the algorithm, sample by sample, and `pcm e_hat = s`."""
    c = code(name)
    basis = np.asarray(c.hx)[np.asarray(c.pivot_hx)].astype(np.uint8)
    rank, n = basis.shape
    B = 37
    rng = np.random.RandomState(3)
    llr = rng.uniform(-3.0, 6.0, size=(B, n)).astype(np.float32)
    llr[:, ::7] = 1.5  # ties: the stable order decides
    err = (rng.uniform(size=(B, n)) < 0.06).astype(np.uint8)
    s = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.int64).T  # [rank, bs]
    osd = F.OSD0_Decoder(n)
    pcm = torch.from_numpy(np.tile(basis[None], (B, 1, 1)).astype(np.int32)).cuda()
    e_hat = osd(torch.from_numpy(llr).cuda(), pcm, torch.from_numpy(s).cuda(), B)
    assert e_hat.dtype == torch.bool and tuple(e_hat.shape) == (B, n)
    e = e_hat.cpu().numpy().astype(np.uint8)
    assert np.array_equal(e.astype(np.int64) @ basis.T.astype(np.int64) % 2, s.T)
    for b in range(B):
        assert np.array_equal(e[b], _numpy_osd0(llr[b], basis, s[:, b].astype(np.uint8))), b
    e2 = osd.call(llr, basis, s)  # a plain [rank, n] matrix, host inputs, the cached graph
    assert torch.equal(e2, e_hat)
    # advisor (round 5): the same pcm tensor again goes straight to the kernel (identity cache: no sync, no copy, no hash); an expanded
    # (stride-0) batch needs no tile check; a second basis does not evict the first (a script alternates hx and hz); an in-place write
    # to the tensor bumps its version and is seen
    g1 = osd._seen[next(iter(osd._seen))]
    assert torch.equal(osd(torch.from_numpy(llr).cuda(), pcm, torch.from_numpy(s).cuda(), B), e_hat) and len(osd._graphs) == 1
    exp = torch.from_numpy(basis.astype(np.int32)).cuda()[None].expand(B, rank, n)
    assert torch.equal(osd(torch.from_numpy(llr).cuda(), exp, torch.from_numpy(s).cuda(), B), e_hat) and len(osd._graphs) == 1
    other = np.asarray(c.hz)[np.asarray(c.pivot_hz)].astype(np.uint8)
    so = (err.astype(np.int64) @ other.T.astype(np.int64) % 2).astype(np.int64).T
    eo = osd(llr, torch.from_numpy(other.astype(np.int32)).cuda(), so).cpu().numpy().astype(np.int64)
    assert np.array_equal(eo @ other.T.astype(np.int64) % 2, so.T) and len(osd._graphs) == 2 and g1 in osd._graphs.values()
    pcm[:, 0, :] ^= pcm[:, 1, :]  # another basis of the same row space, written in place: resolved afresh, still a valid solution
    s2 = s.copy()
    s2[0] ^= s2[1]
    e3 = osd(torch.from_numpy(llr).cuda(), pcm, torch.from_numpy(s2).cuda(), B).cpu().numpy().astype(np.int64)
    assert len(osd._graphs) == 3 and np.array_equal(e3 @ basis.T.astype(np.int64) % 2, s.T)
    with pytest.raises(NotImplementedError):
        bad = pcm.clone()
        bad[1, 0, :] ^= 1
        osd(torch.from_numpy(llr).cuda(), bad, torch.from_numpy(s).cuda(), B)


def test_cal_logit_and_the_rest_of_the_decoder_surface():
    """`QLDPCBPDecoder.cal_logit(llrx, llry, llrz)` (decoding_q.py:455-471) on the marginals a stage-one call returned = the soft
    syndromes that call returned, bit for bit; `build` / `call` / `show_weights` and the read-only properties of `LDPCBPDecoder`
    (decoding.py:420-494) exist with the reference's meaning."""
    c = code("ghp882")
    B = 11
    og, ex, ez, sx, sz = _syndromes("ghp882", 0.09, B)
    dec = F.QLDPCBPDecoder(code=c, num_iter=9, normalization_factor=0.8, cn_type="boxplus-phi", stage_one=True)
    dec.build(None)
    llr = torch.full((B, 3, c.N), llr_const(0.05), dtype=torch.float32, device="cuda")
    llrx, llry, llrz, _, _, x_logit, z_logit = dec.call((llr, torch.from_numpy(sx.T.copy()).cuda(), torch.from_numpy(sz.T.copy()).cuda()))
    xl, zl = dec.cal_logit(llrx.t(), llry.t(), llrz.t())
    assert torch.equal(xl, x_logit) and torch.equal(zl, z_logit) and tuple(xl.shape) == (c.hz.shape[0], B)
    dec.graph.set_hw_transcendentals(True)  # advisor (round 5): the opt-in hardware path must not reach cal_logit
    try:
        xh, zh = dec.cal_logit(llrx.t(), llry.t(), llrz.t())
    finally:
        dec.graph.set_hw_transcendentals(False)
    assert torch.equal(xh, x_logit) and torch.equal(zh, z_logit)
    with pytest.raises(NotImplementedError):
        dec.show_weights()
    b2 = F.LDPCBPDecoder(np.asarray(c.hx), cn_type="minsum", num_iter=7, normalization_factor=0.9, is_syndrome=True, hard_out=True)
    assert (b2.num_cns, b2.num_vns, b2.num_edges) == (441, 882, 2646) and b2.has_weights is False and b2.llr_max == 20.0
    assert np.array_equal(b2.pcm, np.asarray(c.hx)) and b2.output_dtype == torch.float32 and b2.num_iter == 7
    b2.num_iter = 3
    assert b2.num_iter == 3
    with pytest.raises(AssertionError):
        b2.num_iter = -1
    for attr in ("edge_weights", "ie_c", "ie_v"):
        with pytest.raises(NotImplementedError):
            getattr(b2, attr)
    out = b2.call((torch.full((B, 882), -1.4, dtype=torch.float32, device="cuda"), torch.from_numpy(sx.T.copy()).cuda()))
    _, hard = og.bp2_decode(sx, 3, "minsum", 0.9, llr_const=-1.4)  # the oracle's binary BP on the hx graph (side 0 of the CSS graph)
    assert np.array_equal(out.cpu().numpy().astype(np.uint8), hard)


def test_pauli_channel_in_the_references_calling_convention():
    """`Pauli(wt=False)([cx, cz, px, py, pz])` (pauli.py:72-117, as feedback_gnn.py:298-300 and bp_osd.py:107-109 call it): the
    depolarizing split on a `[bs, n]` shape taken from `cx`, no graph needed — the same Philox samples as the native call and the
    oracle; `cz` given -> (y_x, y_z, noise_x, noise_z); `wt=True` -> exactly `wt` errors per row; any other (px, py, pz) is the general
    channel of pauli.py:98-108 (fgnn_pauli_noise_xyz) and equals the oracle's and NumPy's restatement of it."""
    c = code("ghp882")
    B, p = 50, 0.09
    og = oracle_library_forms("ghp882")
    ch = F.Pauli(wt=False, seed=SEED)
    nx, nz = ch([torch.zeros((B, c.N)), None, 2 * p / 3, p / 3, 2 * p / 3])
    ex, ez = og.pauli_noise(SEED, p, 0, B)
    assert nx.dtype == torch.bool and np.array_equal(nx.cpu().numpy(), ex.astype(bool)) and np.array_equal(nz.cpu().numpy(), ez.astype(bool))
    cx = torch.from_numpy((np.arange(B * c.N).reshape(B, c.N) % 3 == 0)).cuda()
    yx, yz, nx2, nz2 = ch.call([cx, torch.zeros_like(cx), 2 * p / 3, p / 3, 2 * p / 3])  # the NEXT B samples of the stream
    ex2, ez2 = og.pauli_noise(SEED, p, B, B)
    assert np.array_equal(nx2.cpu().numpy(), ex2.astype(bool)) and torch.equal(yx, cx ^ nx2) and torch.equal(yz, nz2)
    from helpers import gpu_graph
    native = F.Pauli(gpu_graph("ghp882"), seed=SEED)(B, p, 0)
    assert torch.equal(native[0].bool(), nx) and torch.equal(native[1].bool(), nz)
    wx, wz = F.Pauli(wt=True)([torch.zeros((B, c.N)), None, 7])
    assert ((wx | wz).sum(1) == 7).all()
    # any other triple is taken as pauli.py:98-108 takes it (round 6): a pure bit-flip channel, an asymmetric one — the oracle's
    # restatement on the next samples of the channel's stream, and NumPy's own float32 comparisons on the same Philox words
    from test_oracle_kat import numpy_pauli_xyz
    pos = 2 * B
    for triple in ((0.05, 0.0, 0.0), (0.11, 0.02, 0.05)):
        tx, tz = ch([torch.zeros((B, c.N)), None, *triple])
        ox, oz = og.pauli_noise_xyz(SEED, *triple, pos, B)
        assert np.array_equal(tx.cpu().numpy(), ox.astype(bool)) and np.array_equal(tz.cpu().numpy(), oz.astype(bool)), triple
        rx, rz = numpy_pauli_xyz(SEED, *triple, pos, 3, c.N)
        assert np.array_equal(ox[:3], rx) and np.array_equal(oz[:3], rz)
        pos += B
    assert not ch([torch.zeros((B, c.N)), None, 0.05, 0.0, 0.0])[1].any()  # px only: no Z component anywhere
    gg = gpu_graph("ghp882")
    big = gg.pauli_noise_xyz(SEED, 0.11, 0.02, 0.05, (1 << 32) - 100, 4096)  # a full launch across the 32-bit counter boundary
    obig = og.pauli_noise_xyz(SEED, 0.11, 0.02, 0.05, (1 << 32) - 100, 4096)
    assert np.array_equal(big[0].cpu().numpy(), obig[0]) and np.array_equal(big[1].cpu().numpy(), obig[1])
    with pytest.raises(ValueError):
        gg.pauli_noise_xyz(SEED, float("nan"), 0.0, 0.0, 0, 4)
    # seed-less channels do not replay each other (the reference's tf.random never repeats); an explicit seed reproduces
    a, b2 = F.Pauli(wt=False), F.Pauli(wt=False)
    assert a.seed != b2.seed
    s1 = F.Pauli(seed=123)([torch.zeros((4, c.N)), None, 0.3, 0.1, 0.3])
    s2 = F.Pauli(seed=123)([torch.zeros((4, c.N)), None, 0.3, 0.1, 0.3])
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 3)])
def test_mc_graph_replays_equal_the_same_number_of_mc_steps(rank, world):
    """`mc_graph`: K Monte-Carlo batches captured into one hipGraph whose noise launches read the stream position from a device counter
    the graph advances itself — R replays add exactly what R * K `mc_step` calls add (same Philox samples, also on a rank of a
    sharded stream), the host's stream position follows, and eager steps in between re-synchronise the device counter."""
    c = code("ghp882")
    B, p, K, R = 256, 0.11, 3, 4
    eager, graphed = (_model(c, [32, 8], seed=9, rank=rank, world_size=world) for _ in range(2))
    ce = torch.zeros(3, dtype=torch.int64, device="cuda")
    cg = torch.zeros(3, dtype=torch.int64, device="cuda")
    replay = graphed.mc_graph(B, p, K, cg)
    assert cg.tolist() == [0, 0, 0] and graphed._next_sample == 0  # capturing runs nothing
    for _ in range(R):
        replay()
    for _ in range(R * K):
        eager.mc_step(B, p, ce)
    torch.cuda.synchronize()
    assert cg.tolist() == ce.tolist() and ce[2].item() == R * K * B and ce[1].item() > 0
    assert graphed._next_sample == eager._next_sample == R * K * world * B
    graphed.mc_step(B, p, cg)  # an eager batch in between moves the host's position only ...
    eager.mc_step(B, p, ce)
    replay()                   # ... the next replay starts behind it
    for _ in range(K):
        eager.mc_step(B, p, ce)
    torch.cuda.synchronize()
    assert cg.tolist() == ce.tolist() and graphed._next_sample == eager._next_sample
    # advisor (round 5): a LARGER batch on the same model re-binds the model's workspace; the graph owns its own (replay.workspace) and
    # pins the weights it captured, so replays after the growth — and after the old tensor has gone back to the allocator and been
    # overwritten — still add exactly what eager steps add
    assert replay.workspace is not graphed._workspaces[0] and len(replay.weights) == 1 and replay.counts is cg
    before = replay.workspace.data_ptr()
    graphed.mc_steps(B, p, 4, torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros((4, 3), dtype=torch.int64, device="cuda"))
    for _ in range(4):
        eager.mc_step(B, p, torch.zeros(3, dtype=torch.int64, device="cuda"))
    junk = [torch.full((1 << 22,), 0x7f, dtype=torch.uint8, device="cuda") for _ in range(8)]  # recycle freed blocks
    replay()
    for _ in range(K):
        eager.mc_step(B, p, ce)
    torch.cuda.synchronize()
    del junk
    assert replay.workspace.data_ptr() == before and cg.tolist() == ce.tolist() and graphed._next_sample == eager._next_sample
    with pytest.raises(ValueError):
        _model(c, [32, 8], compact=True).mc_graph(B, p, K, cg)
    # the entry point the captured loop stands on: the stream position read on the device (fgnn_pauli_noise_dev) against the oracle
    from helpers import gpu_graph
    g = gpu_graph("ghp882")
    pos = torch.tensor([(1 << 33) + 100], dtype=torch.int64, device="cuda")
    dx, dz = g.pauli_noise(SEED, p, 7, 33, first_dev=pos)
    ox, oz = oracle_library_forms("ghp882").pauli_noise(SEED, p, (1 << 33) + 107, 33)
    assert np.array_equal(dx.cpu().numpy(), ox) and np.array_equal(dz.cpu().numpy(), oz)
