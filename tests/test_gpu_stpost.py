"""Window post-processing on the GPU, held to the restatement tests/stpost_reference.py bit for bit: the soft outputs of
fgnn_stbp4_decode_soft (hard outputs against fgnn_stbp4_decode as bytes, totals and Gamma as uint32 views), the window problem and its
way back (fgnn_st_window_problem, fgnn_st_window_apply), all three between guard bands, `SpaceTimePostDecoder` with LSD, LSD and the
OSD-0 fallback, and OSD-0, and `BP4_Phenomenological_Model` over sliding windows.  The fixtures are tests/stpost_cases.py: a tiny
irregular code with m_x != m_z (the runtime-degree loop, several windows per workgroup) and [[882,24]] (the packed-row instantiation),
whose conditions tests/test_stpost_reference_cpu.py checks on the CPU.  Every restatement result is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import feedback_gnn_amd as F
import stbp4_reference as ST
import stpost_reference as SP
from feedback_gnn_amd import _lib
from feedback_gnn_amd.graph import TannerGraph
from guarded import guarded
from helpers import llr_const
from stpost_cases import CASES, LOW_CAP, NUM_ITER, Q, case_code, case_inputs, case_settings, case_variant, gamma_of

pytestmark = pytest.mark.gpu

INF = float("inf")
ALL_CASES = sorted(CASES)
POISON = 0xA5


def to_gpu(a):
    """A device copy of a host array (the shared fixtures are read-only, which torch.from_numpy does not take)."""
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def graph_of(code_name):
    return TannerGraph(case_code(next(c for c in CASES if CASES[c][0] == code_name)), stage_one=False)


def case_graph(case):
    return graph_of(CASES[case][0])


@functools.lru_cache(maxsize=None)
def soft_ref(case, variant=False, cn_type="minsum", restart=True):
    kw = case_variant(case, cn_type=cn_type, restart=restart) if variant else case_settings(case, cn_type=cn_type, restart=restart)
    out = SP.stbp4_decode_soft(case_code(case), *case_inputs(case), **kw)
    for a in out:
        a.setflags(write=False)
    return kw, out


def dev_kw(kw):
    kw = dict(kw)
    args = [kw.pop(k) for k in ("factors", "owns", "pre_iter", "attempt_iter", "cn_type")]
    return args, {k: (to_gpu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_soft(case, got, want, plain):
    """got = the eight outputs of stbp4_decode_soft, want = the restatement's, plain = the five of stbp4_decode."""
    for name, t, p_ in zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats"), got, plain):
        assert t.dtype == p_.dtype and t.cpu().numpy().tobytes() == p_.cpu().numpy().tobytes(), (case, name, "differs from fgnn_stbp4_decode")
    for name, t, w in zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats"), got, want):
        assert np.array_equal(t.cpu().numpy(), w), (case, name)
    stats = want[4]
    unsolved = stats[:, 0] == 0
    print(case, "found", stats[:, 0].tolist())
    for name, t, w in zip(("marg", "gam_x", "gam_z"), got[5:], want[5:]):
        a = t.cpu().numpy()
        assert a.dtype == np.float32 and a.shape == w.shape, (case, name)
        assert not bits(a[~unsolved]).any(), (case, name, "a solved window's rows are +0.0f")
        bad = np.nonzero((bits(a[unsolved]) != bits(w[unsolved])).reshape(int(unsolved.sum()), -1).any(1))[0]
        assert not len(bad), (case, name, "unsolved windows", np.nonzero(unsolved)[0][bad])


def run_soft(case, variant=False, cn_type="minsum", restart=True):
    g = case_graph(case)
    kw, want = soft_ref(case, variant, cn_type, restart)
    sx, sz = (to_gpu(a) for a in case_inputs(case))
    args, dkw = dev_kw(kw)
    got = g.stbp4_decode_soft(sx, sz, *args, **dkw)
    plain = g.stbp4_decode(sx, sz, *args, **dkw)
    torch.cuda.synchronize()
    assert_soft(case, got, want, plain)
    return got, want


# ---- soft ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_soft_outputs_base_configuration(case):
    """prev = NULL, scalar gammas with gamma_last = +inf, one alpha: the loop on the tiny code, the packed rows on [[882,24]]."""
    _, want = run_soft(case)
    assert 0 < int(want[4][:, 0].sum()) < len(want[4])
    assert np.isinf(want[6][want[4][:, 0] == 0][:, -1]).all(), "Gamma of a perfect read-out is +inf"


@pytest.mark.parametrize("case", ["tiny_r2", "tiny_r3", "ghp_r2"])
@pytest.mark.parametrize("cn_type,restart", [("minsum", True), ("boxplus-phi", False), ("boxplus", True)])
def test_soft_outputs_with_prev_arrays_and_alpha_sweep(case, cn_type, restart):
    """prev given, per-qubit priors, per-check synd_llr on one side and scalars on the other, the alpha sweep with and without
    restart, every check rule."""
    _, want = run_soft(case, True, cn_type, restart)
    assert 0 < int(want[4][:, 0].sum()) < len(want[4])


@pytest.mark.parametrize("case,geoms", [("tiny_r2", ((32, 8), (64, 4), (256, 1), (1, 64))), ("tiny_r3", ((128, 2), (2, 32))),
                                        ("ghp_r2", ((1024, 1), (192, 1)))])
def test_soft_outputs_do_not_depend_on_the_launch_geometry(case, geoms):
    g = case_graph(case)
    for tpc, cpb in geoms:
        g.set_launch(tpc, cpb)
        try:
            run_soft(case, True)
        finally:
            g.set_launch(0, 0)


def test_one_round_equals_soft_syndrome_bp4():
    case = "tiny_r1"
    g = case_graph(case)
    kw = case_settings(case)
    sx, sz = (to_gpu(a) for a in case_inputs(case))
    got = g.stbp4_decode_soft(sx, sz, kw["factors"], kw["owns"], NUM_ITER, NUM_ITER, "minsum", llr_const=kw["llr_const"], gamma_x=INF,
                              gamma_z=INF, gamma_last_x=kw["gamma_x"], gamma_last_z=kw["gamma_z"])
    ds = g.dsbp4_decode(sx[:, 0].contiguous(), sz[:, 0].contiguous(), kw["factors"], kw["owns"], NUM_ITER, NUM_ITER, "minsum",
                        llr_const=kw["llr_const"], gamma_x=kw["gamma_x"], gamma_z=kw["gamma_z"])
    for a, b in zip(got[:4], ds[:4]):
        assert torch.equal(a[:, 0], b)
    assert torch.equal(got[4], ds[4]) and 0 < int(ds[4][:, 0].sum()) < len(ds[4])


# ---- problem and apply ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_r1", "tiny_r3", "ghp_r2", "ghp_r5"])
@pytest.mark.parametrize("side", [0, 1])
def test_window_problem_bit_for_bit(case, side):
    g = case_graph(case)
    kw, want = soft_ref(case, case in ("tiny_r3", "ghp_r2"))
    synd = case_inputs(case)[side]
    prev = kw.get("prev_x" if side == 0 else "prev_z")
    marg, gam = want[5], want[6 + side]
    B = len(marg)
    rng = np.random.default_rng(B + side)
    dm, dg, ds_, dp = to_gpu(marg), to_gpu(gam), to_gpu(synd), None if prev is None else to_gpu(prev)
    for index in (rng.permutation(B), rng.permutation(B)[:max(1, B // 3)], None, np.zeros(0, np.int64)):
        idx = None if index is None else to_gpu(np.r_[index, [B + 7] * 2].astype(np.int32))  # entries past nact are never read
        nact = B if index is None else len(index)
        d, llr = g.st_window_problem(side, dm, dg, synd=ds_, prev=dp, index=idx, nact=nact)
        wd, wl = SP.window_problem(side, synd, prev, marg, gam, np.arange(B) if index is None else index)
        assert d.dtype == torch.uint8 and llr.dtype == torch.float32 and tuple(d.shape) == wd.shape and tuple(llr.shape) == wl.shape
        assert np.array_equal(d.cpu().numpy(), wd)
        assert np.array_equal(bits(llr.cpu().numpy()), bits(wl))
    d, _ = g.st_window_problem(side, dm, dg, synd=None, prev=dp, nact=2)
    assert np.array_equal(d.cpu().numpy(), SP.window_problem(side, None, prev, marg, gam, [0, 1])[0]), "a NULL syndrome is all zero"


@pytest.mark.parametrize("case", ["tiny_r3", "ghp_r2"])
@pytest.mark.parametrize("side", [0, 1])
def test_window_apply_writes_the_listed_rows_only(case, side):
    g = case_graph(case)
    _, R, B, _, _ = CASES[case]
    m = g.m_x if side == 0 else g.m_z
    rng = np.random.default_rng(31 + side)
    index = rng.permutation(B)[:B // 2]
    e = rng.integers(0, 2, (len(index) + 1, R * (g.n + m))).astype(np.uint8)
    hat = torch.full((B, R, g.n), POISON, dtype=torch.uint8, device="cuda")
    u_hat = torch.full((B, R, m), POISON, dtype=torch.uint8, device="cuda")
    out = g.st_window_apply(side, to_gpu(e), hat, u_hat, index=to_gpu(index.astype(np.int32)), nact=len(index))
    assert out[0] is hat and out[1] is u_hat
    wh, wu = SP.window_apply(e, index, np.full((B, R, g.n), POISON, np.uint8), np.full((B, R, m), POISON, np.uint8))
    assert np.array_equal(hat.cpu().numpy(), wh) and np.array_equal(u_hat.cpu().numpy(), wu)
    rest = np.setdiff1d(np.arange(B), index)
    assert (hat.cpu().numpy()[rest] == POISON).all() and (u_hat.cpu().numpy()[rest] == POISON).all()
    g.st_window_apply(side, to_gpu(e), hat, u_hat, index=to_gpu(index.astype(np.int32)), nact=0)
    assert np.array_equal(hat.cpu().numpy(), wh), "an empty list writes nothing"


# ---- guards -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_r3", "ghp_r2", "ghp_r5"])
def test_guard_bands_around_every_output(case):
    g = case_graph(case)
    kw, want = soft_ref(case)
    sx, sz = (to_gpu(a) for a in case_inputs(case))
    args, dkw = dev_kw(kw)
    with guarded(g) as h:
        got = g.stbp4_decode_soft(sx, sz, *args, **dkw)
        h.label(dict(zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats", "marg", "gam_x", "gam_z"), got)))
        h.check()
        for name, t in zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats", "marg", "gam_x", "gam_z"), got):
            h.assert_written(t, name)  # the poison of a float32 is a NaN no total and no Gamma equals; +inf is not the poison
        assert_soft(case, got, want, got[:5])
        B = len(want[4])
        index = np.nonzero(want[4][:, 0] == 0)[0][::-1].copy()
        for side in (0, 1):
            d, llr = g.st_window_problem(side, got[5], got[6 + side], synd=(sx, sz)[side], index=to_gpu(index.astype(np.int32)), nact=len(index))
            h.label(dict(d=d, llr=llr))
            h.check()
            h.assert_written(d, "d")
            h.assert_written(llr, "llr")
            m = g.m_x if side == 0 else g.m_z
            hat, u_hat = h.alloc((B, got[0].shape[1], g.n), torch.uint8, "hat"), h.alloc((B, got[0].shape[1], m), torch.uint8, "u_hat")
            e = torch.zeros((len(index), llr.shape[1]), dtype=torch.uint8, device="cuda")
            g.st_window_apply(side, e, hat, u_hat, index=to_gpu(index.astype(np.int32)), nact=len(index))
            h.check()
            rest = np.setdiff1d(np.arange(B), index)
            h.assert_written(hat[to_gpu(index)], "hat")
            h.assert_written(u_hat[to_gpu(index)], "u_hat")
            h.assert_untouched(hat[to_gpu(rest)], "hat of unlisted windows")
            h.assert_untouched(u_hat[to_gpu(rest)], "u_hat of unlisted windows")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decoder_of(code_name, rounds):
    code = case_code(next(c for c in CASES if CASES[c][0] == code_name))
    return F.SpaceTimeBP4Decoder(code, rounds, alphas=(1.0,), num_iter=NUM_ITER, cn_type="minsum", factor=0.8, graph=graph_of(code_name))


@functools.lru_cache(maxsize=None)
def post_of(code_name, rounds, method, max_pivots, fallback):
    return F.SpaceTimePostDecoder(decoder_of(code_name, rounds), method=method, max_pivots=max_pivots, fallback=fallback)


_WINDOW_CACHE = {}


def reference_pipeline(code_name, post, sx, sz, prev_x, prev_z, gamma, gamma_last, p):
    R = sx.shape[1]
    caps = tuple(post.window_graph(side, R).lsd_max_pivots(0) for side in (0, 1)) if post.method == "lsd" else (0, 0)
    d = post.decoder
    code = d.code
    return SP.post_decode(code, sx, sz, d.factors, d.owns, d.num_iter, d.cn_type, d.restart, prev_x, prev_z, gamma, gamma_last,
                          llr_const=llr_const(p), method=post.method, max_pivots=post.max_pivots, max_rounds=post.max_rounds,
                          fallback=post.fallback, lds_caps=caps, cache=_WINDOW_CACHE.setdefault(code_name, {}))


E2E = [(case, "lsd", None, None) for case in ("tiny_r1", "tiny_r2", "tiny_r3", "ghp_r2", "ghp_r5")] + \
      [(case, "lsd", LOW_CAP[case], "osd0") for case in sorted(LOW_CAP)] + \
      [(case, "lsd", LOW_CAP[case], None) for case in ("tiny_r2",)] + \
      [(case, "osd0", None, "osd0") for case in ("tiny_r1", "tiny_r2", "tiny_r3", "ghp_r2")]


@pytest.mark.parametrize("case,method,max_pivots,fallback", E2E)
def test_post_decoder_equals_the_restated_pipeline(case, method, max_pivots, fallback):
    name, R, B, p, _ = CASES[case]
    post = post_of(name, 5 if name == "ghp882" else 3, method, max_pivots, fallback)
    sx, sz = case_inputs(case)
    g = gamma_of(Q)
    got = post.decode(to_gpu(sx), to_gpu(sz), gamma=g, gamma_last=INF, llr_const=llr_const(p))
    want = reference_pipeline(name, post, sx, sz, None, None, g, INF, p)
    for label, t, w in zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat", "stats"), got, want):
        assert np.array_equal(t.cpu().numpy(), w), (case, method, label)
    assert np.array_equal(post.last_post_stats.cpu().numpy(), want[5])
    assert (post.last_num_post, post.last_num_fallback) == (want[6], want[7])
    print(case, method, max_pivots, fallback, "post", want[6], "fallback", want[7], "found", want[4][:, 0].tolist())
    assert want[6] >= B // 4
    found = want[4][:, 0] == 1
    x, z, ux, uz = (t.cpu().numpy() for t in got[:4])
    ok = ST.window_test(post.code, x, z, ux, uz, ST.differences(sx, None), ST.differences(sz, None))
    assert ok[found].all(), "a window whose two sides are found satisfies its checks"
    if fallback == "osd0" or method == "osd0":
        assert found.all()
    if max_pivots and fallback == "osd0":
        assert 0 < want[7] < want[6], "the low cap takes the fallback for some windows"
    if max_pivots and fallback is None:
        assert 0 < int((~found).sum()) < want[6] and not ok[~found].any()
    assert post.last_stats is got[4] and torch.equal(post.last_correction_x, (got[0].sum(1) & 1).to(torch.uint8))


def test_post_decoder_call_interface():
    name, R, B, p, _ = CASES["tiny_r2"]
    post, dec = post_of(name, 3, "lsd", None, "osd0"), decoder_of(name, 3)
    sx, sz = case_inputs("tiny_r2")
    llr = torch.full((B, 3, post.graph.n), llr_const(p), device="cuda")
    post.gamma, post.gamma_last = gamma_of(Q), INF
    x, z = post((llr, to_gpu(sx).permute(1, 2, 0), to_gpu(sz).permute(1, 2, 0)))
    assert x.dtype == torch.int64 and z.dtype == torch.float64 and tuple(x.shape) == (B, post.graph.n)
    want = reference_pipeline(name, post, sx, sz, None, None, gamma_of(Q), INF, p)
    assert np.array_equal(x.cpu().numpy(), want[0].sum(1) % 2) and np.array_equal(z.cpu().numpy(), want[1].sum(1) % 2)
    assert post.rounds == dec.rounds and post.graph is dec.graph


@pytest.mark.parametrize("name,B", [("tiny", 24), ("ghp882", 6)])
def test_sliding_windows_equal_the_restated_loop(name, B):
    """BP4_Phenomenological_Model with window = 2, commit = 1 over 4 rounds on a post-processing decoder, against
    stbp4_reference.sliding_decode driven by the restated pipeline on the model's own draws."""
    p = 0.06 if name == "tiny" else 0.03
    post = post_of(name, 5 if name == "ghp882" else 3, "lsd", None, "osd0")
    model = F.BP4_Phenomenological_Model(post.code, post, Q, rounds=4, window=2, commit=1, seed=77)
    model(B, p)
    torch.cuda.synchronize()
    hx, hz = np.asarray(post.code.hx, np.int64) % 2, np.asarray(post.code.hz, np.int64) % 2
    cx, cz = (np.cumsum(t.cpu().numpy().astype(np.int64), axis=1) % 2 for t in (model.last_noise_x, model.last_noise_z))
    sx = ((cz @ hx.T) % 2).astype(np.uint8) ^ model.last_u_x.cpu().numpy()
    sz = ((cx @ hz.T) % 2).astype(np.uint8) ^ model.last_u_z.cpu().numpy()
    gamma = model.gamma

    def decode(wx, wz, px, pz, gamma_last):
        return reference_pipeline(name, post, wx, wz, px, pz, gamma, gamma_last, p)[:5]

    xh, zh, uxh, uzh, unsolved, calls = ST.sliding_decode(decode, sx, sz, 4, 2, 1, gamma)
    assert len(calls) == 3 and [c[3] for c in calls] == [False, True, True]
    for label, t, w in zip(("x_hat", "z_hat", "u_x_hat", "u_z_hat"), (model.last_x_hat, model.last_z_hat, model.last_u_x_hat, model.last_u_z_hat),
                           (xh, zh, uxh, uzh)):
        assert np.array_equal(t.cpu().numpy(), w), label
    assert model.last_num_unsolved == unsolved == 0, "with the fallback every window comes back solved"
    plain = F.BP4_Phenomenological_Model(post.code, post.decoder, Q, rounds=4, window=2, commit=1, seed=77)
    plain(B, p)
    assert plain.last_num_unsolved > 0, "the fixture leaves the plain decoder unsolved windows to post-process"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    case = "tiny_r2"
    g = case_graph(case)
    L = _lib.lib()
    kw = case_settings(case)
    sx, sz = (to_gpu(a) for a in case_inputs(case))
    B, R = sx.shape[:2]
    f, o = kw["factors"], kw["owns"]
    outs = [torch.zeros(s, dtype=torch.uint8, device="cuda") for s in ((B, R, g.n), (B, R, g.n), (B, R, g.m_x), (B, R, g.m_z))]
    stats = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    soft = [torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((B, R, 3, g.n), (B, R, g.m_x), (B, R, g.m_z))]

    def call(rounds=R, batch=B, soft_ptrs=None, out_ptrs=None, gamma=1.0, cn=2, h=g.handle):
        sp = [t.data_ptr() for t in soft] if soft_ptrs is None else soft_ptrs
        op = [t.data_ptr() for t in outs] + [stats.data_ptr()] if out_ptrs is None else out_ptrs
        return L.fgnn_stbp4_decode_soft(h, cn, len(f), f.ctypes.data, o.ctypes.data, 3, 3, 1, rounds, None, 1.0, sx.data_ptr(), sz.data_ptr(), None,
                                        None, None, gamma, INF, None, 1.0, INF, batch, *op, *sp, None)

    assert call() == 0
    for i in range(3):
        sp = [t.data_ptr() for t in soft]
        sp[i] = None
        assert call(soft_ptrs=sp) == -1 and b"soft output" in L.fgnn_last_error()
    assert call(batch=0, soft_ptrs=[None] * 3, out_ptrs=[None] * 5) == 0, "B = 0 needs no buffers"
    assert call(out_ptrs=[None] * 5) == -1 and b"no output buffer" in L.fgnn_last_error()
    assert call(rounds=0) == -1 and b"rounds must be >= 1" in L.fgnn_last_error()
    assert call(gamma=float("nan")) == -1 and call(cn=3) == -1 and call(h=None) == -1 and call(batch=-1) == -1
    big = case_graph("ghp_r2")
    with pytest.raises(ValueError, match="window too large") as soft_err:
        big.stbp4_decode_soft(None, None, f, o, 3, 3, rounds=40, B=1)
    with pytest.raises(ValueError, match="window too large") as plain_err:
        big.stbp4_decode(None, None, f, o, 3, 3, rounds=40, B=1)
    assert str(soft_err.value) == str(plain_err.value), "a window that does not fit is refused with the same message"

    marg, gam = soft[0], soft[1]
    d = torch.zeros((B, R * g.m_x), dtype=torch.uint8, device="cuda")
    llr = torch.zeros((B, R * (g.n + g.m_x)), dtype=torch.float32, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def problem(side=0, rounds=R, nact=B, marg_=marg, gam_=gam, d_=d, llr_=llr, h=g.handle):
        return L.fgnn_st_window_problem(h, side, rounds, sx.data_ptr(), None, P(marg_), P(gam_), None, nact, P(d_), P(llr_), None)

    assert problem() == 0
    for bad in (dict(side=2), dict(side=-1), dict(rounds=0), dict(nact=-1), dict(marg_=None), dict(gam_=None), dict(d_=None), dict(llr_=None),
                dict(h=None)):
        assert problem(**bad) == -1, bad
    assert problem(nact=0, marg_=None, gam_=None, d_=None, llr_=None) == 0, "an empty list needs no buffers"
    e = torch.zeros((B, R * (g.n + g.m_x)), dtype=torch.uint8, device="cuda")

    def apply(side=0, rounds=R, nact=B, e_=e, hat_=outs[1], u_=outs[2], h=g.handle):
        return L.fgnn_st_window_apply(h, side, rounds, P(e_), None, nact, P(hat_), P(u_), None)

    assert apply() == 0
    for bad in (dict(side=2), dict(rounds=0), dict(nact=-1), dict(e_=None), dict(hat_=None), dict(u_=None), dict(h=None)):
        assert apply(**bad) == -1, bad
    assert apply(nact=0, e_=None, hat_=None, u_=None) == 0
    torch.cuda.synchronize()


def test_symbols_are_exported():
    L = _lib.lib()
    for name in ("fgnn_stbp4_decode_soft", "fgnn_st_window_problem", "fgnn_st_window_apply"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
