"""Quaternary BP (fgnn_bp4_decode / fgnn_bp4_decode_trace) on the GPU at every bit-exact bp4_kernel instantiation launch_bp4 can pick and
at the run-time branches of plan_bp4, held two ways: bit for bit to the CPU oracle og_bp4_decode in the matching qubit-update form
(floats compared as int32 views), and at one and two iterations to the float64 restatement numpy_ref.bp4_decode64 with the bounds of
tests/test_bp4_reference_cpu.py, which does not share the oracle's code.

bp4_variant restates the host rule (plan_bp4, launch_bp4, launch_bp4_k of fgnn_bp4.hip; fgnn_geom of fgnn_graph.hip) in Python and the
module assertion below checks, from the case list alone, that the runs reach every instantiation: per rule (3,3,6) / (4,4,8) / (0,0,0)
with the shortcuts on and off, the trace kernels of (3,3,6) and (0,0,0) (the latter also for a (4,4,8) graph, which has no trace
kernel of its own), the global-memory variant, and the 12 boxplus-phi (3,3,6) kernels bp4_lse_kernels[lreg 0/4/5][shortcut][LSE].  The
opt-in hardware-transcendental kernels are not bit-exact and have their own test.  The run-time fields are covered the same way: the
channel LLRs in registers (lreg 4 and 5) or in LDS, the closed-form first iteration, the fixed-point early exit and why it is off, the
syndrome bits in one register or re-read, the fused flag bytes inside the message area or behind the tail, several codewords per
workgroup, the cslot16 limit and the LDS budget on both sides."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from feedback_gnn_amd import codes_q as cq
from feedback_gnn_amd.graph import TannerGraph
from helpers import WEIGHTS_882, code, to_gpu
from oracle import numpy_ref as R
from oracle.oracle import OracleGraph
from test_bp4_reference_cpu import against_float64, channel, edge_channel, random_messages, tol_of

pytestmark = pytest.mark.gpu

RULES = ("boxplus-phi", "minsum", "boxplus")
CN_ID = {"boxplus": 0, "boxplus-phi": 1, "minsum": 2}  # FGNN_CN_*
LDS_BUDGET = 160 * 1024 - 256  # FGNN_LDS_BUDGET, fgnn_internal.h
F32 = np.float32


# ---- codes ----------------------------------------------------------------------------------------------------------------------------
def _bare(hx, hz):
    """A code object carrying only what TannerGraph / OracleGraph / bp4_decode64 read, with no GF(2) rank work."""
    hx, hz = np.asarray(hx, np.int64), np.asarray(hz, np.int64)
    zero = np.zeros((1, hx.shape[1]), np.int64)
    return types.SimpleNamespace(hx=hx, hz=hz, hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)


def _circulant(l, pos):
    m = np.zeros((l, l), np.int64)
    for p in pos:
        m[np.arange(l), (np.arange(l) + p) % l] = 1
    return m


def bare_gb(seed, w, l):
    """A seeded generalized-bicycle code with |a| = |b| = w built bare: hx = [A | B], hz = [B^T | A^T], (w, w, 2w)-regular with its own
    slot offsets."""
    @functools.lru_cache(maxsize=None)
    def make():
        rng = np.random.RandomState(seed)
        A, B = (_circulant(l, sorted(rng.choice(l, size=w, replace=False))) for _ in range(2))
        return _bare(np.hstack([A, B]), np.hstack([B.T, A.T]))
    return make


def gb(seed, w, l):
    """The same construction through the code class (stabilizer rows, logicals): for the small codes."""
    @functools.lru_cache(maxsize=None)
    def make():
        rng = np.random.RandomState(seed)
        a, b = (sorted(int(x) for x in rng.choice(l, size=w, replace=False)) for _ in range(2))
        return cq.create_generalized_bicycle_codes(l, a, b)
    return make


def sparse_bare(n, E_x, E_z, seed):
    """An irregular bare code of n qubits with E_x / E_z edges: every qubit gets floor or ceil of E / n checks of each side, checks of
    degree ~6."""
    @functools.lru_cache(maxsize=None)
    def make():
        rng = np.random.RandomState(seed)
        out = []
        for E in (E_x, E_z):
            m = max(1, E // 6)
            h = np.zeros((m, n), np.int64)
            per = np.full(n, E // n)
            per[rng.choice(n, size=E - per.sum(), replace=False)] += 1
            for v in range(n):
                h[rng.choice(m, size=per[v], replace=False), v] = 1
            h = h[h.sum(1) > 0]
            out.append(h)
        assert out[0].sum() == E_x and out[1].sum() == E_z
        return _bare(*out)
    return make


def thin_bare(n):
    """One hx and one hz edge per qubit (checks of degree 3): E = 2n, below 2n + n/4 + 1, so the fused flag bytes go behind the tail."""
    @functools.lru_cache(maxsize=None)
    def make():
        hx = np.zeros((n // 3, n), np.int64)
        hz = np.zeros((n // 3, n), np.int64)
        hx[np.arange(n) // 3, np.arange(n)] = 1
        perm = np.random.RandomState(n).permutation(n)
        hz[np.arange(n) // 3, perm] = 1
        return _bare(hx, hz)
    return make


def named(name):
    return lambda: code(name)


# E + 3n floats of messages and channel LLRs exactly at FGNN_LDS_BUDGET (and one float over): n = 4000, 3n = 12 000
LDS_N = 4000
LDS_E = LDS_BUDGET // 4 - 3 * LDS_N
CASES = {
    "gb3_s": gb(1, 3, 21), "gb4_s": gb(2, 4, 23),                       # (3,3,6) / (4,4,8), several codewords per workgroup
    "gb3_128": bare_gb(3, 3, 128), "gb3_150": bare_gb(4, 3, 150),       # (3,3,6), one codeword per workgroup
    "gb3_180": bare_gb(5, 3, 180), "gb4_130": bare_gb(6, 4, 130),       # (3,3,6) / (4,4,8), one codeword per workgroup
    "cslot_in": bare_gb(7, 3, 1365), "cslot_out": bare_gb(7, 3, 1366),  # E = 16 380 / 16 392: 4 E below / above 65 536
    "synd32": bare_gb(8, 3, 1024), "synd33": bare_gb(8, 3, 1025),      # m = 2048 / 2050 checks on 64 threads
    "rsurf5": named("rsurf5"), "hp_c7": named("hp_c7"), "gb46_oc": named("gb46_oc"),  # irregular; gb46_oc: max_vdeg > 32
    "lds_at": sparse_bare(LDS_N, LDS_E // 2, LDS_E - LDS_E // 2, 9),
    "lds_over": sparse_bare(LDS_N, LDS_E // 2, LDS_E - LDS_E // 2 + 1, 9),
    "thin": thin_bare(300),
}

_GRAPHS = {}


def graphs(key):
    """(TannerGraph, OracleGraph in the literal forms, code) of one case, built once per session."""
    if key not in _GRAPHS:
        c = CASES[key]()
        _GRAPHS[key] = (TannerGraph(c), OracleGraph(c, forms="literal"), c)
    return _GRAPHS[key]


# ---- the host rule, restated ------------------------------------------------------------------------------------------------------------
def describe(c):
    """What fgnn_graph_create records and fgnn_graph_info reports, from the check matrices alone: sizes, uniform degrees (0 if
    irregular; fgnn_graph.hip uniform_degree), the default launch (default_launch) and max_vdeg."""
    hx, hz = np.asarray(c.hx), np.asarray(c.hz)
    n, m = hx.shape[1], hx.shape[0] + hz.shape[0]

    def uni(d):
        return int(d[0]) if (d == d[0]).all() else 0

    nodes = max(n, m)
    if nodes >= 256:
        tpc, cpb = 256, 1
    elif nodes >= 64:
        tpc, cpb = (nodes + 63) // 64 * 64, 1
    else:
        tpc = 1 << (nodes - 1).bit_length()
        cpb = 256 // tpc
    return dict(n=n, m_x=hx.shape[0], m_z=hz.shape[0], E_x=int(hx.sum()), E_z=int(hz.sum()), threads_per_codeword=tpc,
                codewords_per_block=cpb, dv_x=uni(hx.sum(0)), dv_z=uni(hz.sum(0)), dc=uni(np.r_[hx.sum(1), hz.sum(1)]),
                max_vdeg=int((hx.sum(0) + hz.sum(0)).max()))


def bp4_variant(info, cn_type, B, num_iter, llr_ch=False, msg_init=False, trace=False, flagged=False, launch=None, shortcut=True,
                early_exit=True, force_generic=False, shared_lse=False):
    """The kernel and the run-time fields of one fgnn_bp4_decode(_trace) call: fgnn_geom, plan_bp4, launch_bp4 and launch_bp4_k restated.
    `info` is describe()'s dict, `launch` the (tpc, cpb) of set_launch.  Returns dict(kernel = (CN_TYPE, DVX, DVZ, DC, OPT, NQ, TRACE,
    GMEM, LSE), lreg, first_closed, early_exit, synd_in_reg, flag ('inside' / 'behind' / None), tpc, cpb, lds_bytes)."""
    n, m, E = info["n"], info["m_x"] + info["m_z"], info["E_x"] + info["E_z"]
    tpc, cpb = launch if launch else (info["threads_per_codeword"], info["codewords_per_block"])
    if not launch and cpb == 1 and B <= 256:  # fgnn_geom: a thread per node for small launches
        tpc = min(1024, max(tpc, (max(n, m) + 63) // 64 * 64))
    phi = cn_type == "boxplus-phi"
    dvx, dvz, dc = info["dv_x"], info["dv_z"], info["dc"]
    cslot16 = dvx > 0 and dvz > 0 and 0 < dc <= 8 and 4 * E < 65536
    r336 = cslot16 and not force_generic and (dvx, dvz, dc) == (3, 3, 6)
    r448 = cslot16 and not force_generic and (dvx, dvz, dc) == (4, 4, 8)

    def round4(f):
        return (f + 3) & ~3

    def plan(gmem):
        sc = shortcut and not trace and not gmem
        lch_off = max(E, 2 * n)
        per_thread = (n + tpc - 1) // tpc
        lreg = (4 if per_thread <= 4 else 5) if (llr_ch and not trace and not gmem and phi and cpb == 1 and r336 and per_thread <= 5) else 0
        per = lch_off + (3 * n if llr_ch and not lreg else 0) + (2 * n if trace else 0)
        if not gmem:
            per = round4(per)
        tail = 0
        ee = sc and early_exit and info["max_vdeg"] <= 32 and phi and cpb == 1 and num_iter > 2
        if ee:
            if (per * cpb + n + 4) * 4 <= LDS_BUDGET:
                tail += n + 4
            else:
                ee = False
        flag = None
        if flagged:
            need = round4(n) // 4 + 1
            flag = "inside" if lch_off >= 2 * n + need else "behind"
            tail += 0 if flag == "inside" else need
        return dict(shortcut=sc, lreg=lreg, early_exit=ee, flag=flag, lds_bytes=0 if gmem else (per * cpb + tail) * 4)

    p = plan(False)
    gmem = p["lds_bytes"] > LDS_BUDGET
    if gmem:
        p = plan(True)
    cn, sc = CN_ID[cn_type], p["shortcut"]
    if gmem:
        kernel = (cn, 0, 0, 0, False, 0, False, True, 2)
    else:
        shape = (3, 3, 6) if r336 else (4, 4, 8) if (r448 and not trace) else (0, 0, 0)
        kernel = (cn,) + shape + (sc, 0, False, False, 2)
        if trace and shape != (4, 4, 8):
            kernel = (cn,) + shape + (False, 0, True, False, 2)
        if phi and shape == (3, 3, 6) and not trace:
            kernel = (cn, 3, 3, 6, sc, p["lreg"], False, False, int(shared_lse))
    regular = kernel[1] > 0
    first_closed = kernel[4] and regular and phi and sc and not llr_ch and not msg_init and num_iter > 0
    return dict(kernel=kernel, lreg=p["lreg"], first_closed=bool(first_closed), early_exit=p["early_exit"],
                synd_in_reg=(m + tpc - 1) // tpc <= 32, flag=p["flag"], tpc=tpc, cpb=cpb, lds_bytes=p["lds_bytes"], gmem=gmem)


def _all_kernels():
    """Every bit-exact bp4_kernel instantiation launch_bp4 can pick."""
    out = set()
    for cn in CN_ID.values():
        for shape in ((3, 3, 6), (4, 4, 8), (0, 0, 0)):
            for opt in (False, True):
                if not (cn == CN_ID["boxplus-phi"] and shape == (3, 3, 6)):
                    out.add((cn,) + shape + (opt, 0, False, False, 2))
        out.add((cn, 3, 3, 6, False, 0, True, False, 2))
        out.add((cn, 0, 0, 0, False, 0, True, False, 2))
        out.add((cn, 0, 0, 0, False, 0, False, True, 2))
    for nq in (0, 4, 5):
        for opt in (False, True):
            for lse in (0, 1):
                out.add((CN_ID["boxplus-phi"], 3, 3, 6, opt, nq, False, False, lse))
    return out


ALL_KERNELS = _all_kernels()
assert len(ALL_KERNELS) == 3 * 9 - 2 + 12


# ---- the runs -------------------------------------------------------------------------------------------------------------------------
def run(key, cn, B, it, **kw):
    return dict(key=key, cn=cn, B=B, it=it, **kw)


RUNS = []
for _cn in RULES:
    RUNS += [
        run("gb3_s", _cn, 7, 2), run("gb3_s", _cn, 9, 5, shortcut=False, llr="ch"),  # (3,3,6), several codewords per workgroup
        run("gb4_s", _cn, 5, 1), run("gb4_s", _cn, 6, 4, shortcut=False, llr="ch"),  # (4,4,8)
        run("gb4_130", _cn, 3, 2, llr="ch", msg_init=True), run("gb4_130", _cn, 2, 6),  # (4,4,8), one codeword: first_closed, exit
        run("rsurf5", _cn, 11, 2, llr="ch"), run("rsurf5", _cn, 13, 4, shortcut=False),  # (0,0,0)
        run("gb3_150", _cn, 4, 2, force_generic=True), run("gb3_150", _cn, 3, 5, force_generic=True, shortcut=False, llr="ch"),
        run("gb3_s", _cn, 6, 3, trace=True, llr="ch"), run("gb4_s", _cn, 5, 3, trace=True),  # trace: (3,3,6) and (4,4,8) -> (0,0,0)
        run("hp_c7", _cn, 4, 2, trace=True, msg_init=True),
        run("lds_at", _cn, 3, 2, llr="ch", msg_init=True), run("lds_over", _cn, 3, 2, llr="ch", msg_init=True),  # the LDS budget
        run("lds_at", _cn, 2, 3), run("cslot_in", _cn, 2, 2, llr="ch"), run("cslot_out", _cn, 2, 2, llr="ch"),  # cslot16 limit
        run("gb46_oc", _cn, 3, 3),                                                     # max_vdeg > 32
        run("synd32", _cn, 3, 3, launch=(64, 1)), run("synd33", _cn, 3, 3, launch=(64, 1), llr="ch"),
        run("gb3_128", _cn, 1, 2, llr="ch"), run("gb3_128", _cn, 256, 1), run("gb3_128", _cn, 257, 2, llr="ch"),
        run("gb3_s", _cn, 9, 0, synd="ones"), run("gb3_150", _cn, 5, 2, synd="ones", llr="zero", logits=False, msgs=False),
        run("gb4_s", _cn, 6, 2, llr="zero"), run("rsurf5", _cn, 7, 0, llr="ch", msg_init=True),
        run("gb4_s", _cn, 6, 1, llr="edge"), run("gb3_150", _cn, 3, 1, llr="edge", launch=(64, 1)), run("rsurf5", _cn, 5, 1, llr="edge"),
    ]
for _lse in (False, True):  # the 12 phi (3,3,6) kernels: lreg 0 / 4 / 5 x shortcut x LSE; set_launch gives 1, 4, 5, 6 qubits per thread
    for _sc in (True, False):
        RUNS += [
            run("gb3_150", "boxplus-phi", 3, 2, shared_lse=_lse, shortcut=_sc),                        # lreg 0 (constant LLR)
            run("gb3_150", "boxplus-phi", 3, 2, llr="ch", shared_lse=_lse, shortcut=_sc, launch=(320, 1)),  # 1 per thread: lreg 4
            run("gb3_128", "boxplus-phi", 2, 3, llr="ch", shared_lse=_lse, shortcut=_sc, launch=(64, 1)),   # 4 per thread: lreg 4
            run("gb3_150", "boxplus-phi", 2, 3, llr="ch", shared_lse=_lse, shortcut=_sc, launch=(64, 1)),   # 5 per thread: lreg 5
            run("gb3_180", "boxplus-phi", 2, 3, llr="ch", shared_lse=_lse, shortcut=_sc, launch=(64, 1)),   # 6 per thread: lreg 0
        ]
RUNS += [
    run("gb3_s", "boxplus-phi", 8, 2, llr="ch"),                                   # cpb > 1: lreg and the early exit forced off
    run("gb3_150", "boxplus-phi", 5, 1), run("gb3_150", "boxplus-phi", 5, 2),      # first_closed on (3,3,6), 1 and 2 iterations
    run("gb4_130", "boxplus-phi", 5, 1), run("gb4_130", "boxplus-phi", 5, 2),      # and on (4,4,8)
    run("gb3_150", "boxplus-phi", 5, 2, shortcut=False), run("gb3_150", "boxplus-phi", 5, 2, llr="ch"),  # each condition broken
    run("gb3_150", "boxplus-phi", 5, 2, msg_init=True), run("gb3_150", "boxplus-phi", 5, 0),
    run("gb3_150", "boxplus-phi", 5, 2, force_generic=True), run("gb4_130", "minsum", 5, 2),
    run("gb3_150", "boxplus-phi", 4, 12), run("gb3_150", "boxplus-phi", 4, 12, early_exit=False),  # the early exit on and off
    run("gb3_150", "boxplus-phi", 4, 2, p=0.01), run("gb3_150", "boxplus-phi", 4, 3, p=0.01),  # num_iter 2 against 3
    run("gb4_130", "boxplus-phi", 4, 16, p=0.01), run("rsurf5", "boxplus-phi", 4, 16, launch=(64, 1), p=0.01),
]
for _f in (1.0, float(np.nextafter(F32(1), F32(0))), float(np.nextafter(F32(1), F32(2))), 0.0):  # the F1 copy of cn_phi_regular
    RUNS += [run("gb3_150", "boxplus-phi", 3, 3, factor=_f), run("gb4_130", "boxplus-phi", 3, 3, factor=_f, llr="ch"),
             run("gb3_s", "boxplus-phi", 5, 3, factor=_f)]


def variant_of(r):
    return bp4_variant(describe(CASES[r["key"]]()), r["cn"], r["B"], r["it"], llr_ch=r.get("llr") in ("ch", "edge"),
                       msg_init=r.get("msg_init", False), trace=r.get("trace", False), launch=r.get("launch"),
                       shortcut=r.get("shortcut", True),
                       early_exit=r.get("early_exit", True), force_generic=r.get("force_generic", False),
                       shared_lse=r.get("shared_lse", False))


def _coverage():
    """What RUNS reach according to the restated rule: no GPU."""
    vs = [variant_of(r) for r in RUNS]
    return vs, {v["kernel"] for v in vs}


_VARIANTS, _REACHED = _coverage()
assert _REACHED == ALL_KERNELS, ("the runs must reach every bit-exact bp4_kernel instantiation", ALL_KERNELS - _REACHED)
assert {v["lreg"] for v in _VARIANTS} == {0, 4, 5}
assert {v["first_closed"] for v in _VARIANTS if v["kernel"][1] == 3} == {True, False}
assert {v["first_closed"] for v in _VARIANTS if v["kernel"][1] == 4} == {True, False}
assert {v["early_exit"] for v in _VARIANTS} == {True, False} and {v["synd_in_reg"] for v in _VARIANTS} == {True, False}
assert any(v["early_exit"] for v, r in zip(_VARIANTS, RUNS) if v["kernel"][1] == 4)
assert {v["cpb"] > 1 for v in _VARIANTS} == {True, False}


# ---- checking one call ------------------------------------------------------------------------------------------------------------
def inputs(r, g, og, c):
    """Syndromes and the LLR / msg_init arguments of a run, in NumPy."""
    seed = zlib.crc32(repr(sorted(r.items())).encode()) & 0x7FFFFFFF
    B = r["B"]
    if r.get("synd") == "ones":
        sx, sz = np.ones((B, og.m_x), np.uint8), np.ones((B, og.m_z), np.uint8)
    else:
        ex, ez = og.pauli_noise(seed, r.get("p", 0.05), 0, B)
        sx, sz = og.syndrome(ex, ez)
    kw = {}
    llr = r.get("llr", "const")
    if llr == "ch":
        kw["llr_ch"] = channel(B, og.n, seed)
    elif llr == "edge":  # saturating and signed-zero / subnormal LLRs, one per check (tests/test_bp4_reference_cpu.py)
        kw["llr_ch"] = edge_channel(c, B, seed)
    else:
        kw["llr_const"] = 0.0 if llr == "zero" else 3.2958  # log(3 (1 - p) / p) at p = 0.1
    if r.get("msg_init"):
        kw["msg_init"] = random_messages(c, B, seed)
    return sx, sz, kw


def gpu_call(g, r, sx, sz, kw):
    gkw = dict(llr_const=kw.get("llr_const", 0.0), llr_ch=to_gpu(kw["llr_ch"]) if "llr_ch" in kw else None,
               msg_init=tuple(to_gpu(m) for m in kw["msg_init"]) if "msg_init" in kw else None)
    if r.get("trace"):
        o = g.bp4_decode_trace(to_gpu(sx), to_gpu(sz), r["it"], r["cn"], r.get("factor", 0.8), **gkw)
    else:
        o = g.bp4_decode(to_gpu(sx), to_gpu(sz), r["it"], r["cn"], r.get("factor", 0.8), return_msgs=r.get("msgs", True),
                         want_logits=r.get("logits", True), **gkw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


class configured:
    """A GPU graph and its oracle set up for one run, restored on exit (the graphs are shared by the session)."""

    def __init__(self, g, og, r):
        self.g, self.og, self.r = g, og, r

    def __enter__(self):
        r, g = self.r, self.g
        g.set_saturation_shortcut(r.get("shortcut", True))
        g.set_fixed_point_exit(r.get("early_exit", True))
        g.force_generic(r.get("force_generic", False))
        g.set_bp4_shared_lse(r.get("shared_lse", False))
        self.og.set_vn_shared_lse(r.get("shared_lse", False))
        if r.get("launch"):
            g.set_launch(*r["launch"])

    def __exit__(self, *exc):
        self.g.set_saturation_shortcut(True)
        self.g.set_fixed_point_exit(True)
        self.g.force_generic(False)
        self.g.set_bp4_shared_lse(False)
        self.og.set_vn_shared_lse(False)
        self.g.set_launch(0, 0)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def check_run(r):
    g, og, c = graphs(r["key"])
    sx, sz, kw = inputs(r, g, og, c)
    factor = r.get("factor", 0.8)
    with configured(g, og, r):
        got = gpu_call(g, r, sx, sz, kw)
    if r.get("trace"):  # slot k of the trace = the soft syndromes after k iterations
        for k in range(r["it"] + 1):
            o = og.bp4_decode(sx, sz, k, r["cn"], factor, **kw)
            assert bits_equal(got["x_logit"][k], o["x_logit"]) and bits_equal(got["z_logit"][k], o["z_logit"]), (r, k)
        got["x_logit"], got["z_logit"] = got["x_logit"][-1], got["z_logit"][-1]
    with configured(g, og, r):
        ref = og.bp4_decode(sx, sz, r["it"], r["cn"], factor, return_msgs=True, **kw)
    assert bits_equal(got["llr"], ref["llr"]), (r, "llr")
    assert np.array_equal(got["x_hat"], ref["x_hat"]) and np.array_equal(got["z_hat"], ref["z_hat"]), (r, "decisions")
    for k in ("x_logit", "z_logit", "msg_x", "msg_z"):
        if got.get(k) is not None:
            assert bits_equal(got[k], ref[k]), (r, k)
    if r.get("logits", True) is False:
        assert got["x_logit"] is None and got["z_logit"] is None
    # the float64 yardstick, independent of the oracle: one and two iterations (a restart: one, as in the CPU file)
    if 1 <= r["it"] <= (1 if r.get("msg_init") else 2) and r.get("llr") != "zero" and r.get("synd") != "ones":
        f64 = R.bp4_decode64(c, sx, sz, r["it"], r["cn"], factor, **kw)
        against_float64(got, f64, c, r["cn"], tol_of(r["cn"]))
    return got


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[f"{r['key']}-{r['cn']}-B{r['B']}-it{r['it']}-{j}" for j, r in enumerate(RUNS)])
def test_run_against_oracle_and_float64(i):
    check_run(RUNS[i])


def test_built_graphs_report_the_assumed_degrees():
    """fgnn_graph_info of every built graph agrees with describe(), from which the module assertion computed the kernels."""
    for key in CASES:
        g, _, c = graphs(key)
        d, info = describe(c), g.info()
        assert all(info[k] == d[k] for k in info if k in d), (key, info, d)
        assert info["regular"] == int(d["dv_x"] > 0 and d["dv_z"] > 0 and d["dc"] > 0)


def test_variant_fields_of_the_named_edges():
    """The restated plan at the boundaries the cases are built for."""
    v = {key: describe(CASES[key]()) for key in ("cslot_in", "cslot_out", "lds_at", "lds_over", "synd32", "synd33", "thin")}
    assert v["cslot_in"]["E_x"] + v["cslot_in"]["E_z"] == 16380 and v["cslot_out"]["E_x"] + v["cslot_out"]["E_z"] == 16392
    assert bp4_variant(v["cslot_in"], "minsum", 2, 2)["kernel"][1:4] == (3, 3, 6)
    assert bp4_variant(v["cslot_out"], "minsum", 2, 2)["kernel"][1:4] == (0, 0, 0)
    at = bp4_variant(v["lds_at"], "boxplus-phi", 3, 3, llr_ch=True, msg_init=True)
    assert at["lds_bytes"] == LDS_BUDGET and not at["gmem"] and not at["early_exit"]  # at the budget; the exit's tail does not fit
    assert bp4_variant(v["lds_over"], "minsum", 3, 2, llr_ch=True)["gmem"]
    assert bp4_variant(v["synd32"], "minsum", 3, 3, launch=(64, 1))["synd_in_reg"]
    assert not bp4_variant(v["synd33"], "minsum", 3, 3, launch=(64, 1))["synd_in_reg"]
    assert bp4_variant(v["thin"], "boxplus-phi", 8, 4, flagged=True)["flag"] == "behind"
    assert bp4_variant(describe(CASES["gb3_150"]()), "boxplus-phi", 8, 4, flagged=True)["flag"] == "inside"
    # the qubits per thread of the lreg runs: 1 - 4 take lreg 4, 5 takes lreg 5, 6 takes the channel LLRs in LDS
    for key, tpc, per, lreg in (("gb3_150", 320, 1, 4), ("gb3_128", 64, 4, 4), ("gb3_150", 64, 5, 5), ("gb3_180", 64, 6, 0)):
        d = describe(CASES[key]())
        assert (d["n"] + tpc - 1) // tpc == per
        assert bp4_variant(d, "boxplus-phi", 2, 3, llr_ch=True, launch=(tpc, 1))["lreg"] == lreg


def test_trace_refused_on_a_global_memory_size_code():
    g, _, _ = graphs("lds_over")
    B = 2
    sx = torch.zeros((B, g.m_x), dtype=torch.uint8, device=g.device)
    sz = torch.zeros((B, g.m_z), dtype=torch.uint8, device=g.device)
    llr = torch.full((B, 3, g.n), 2.0, device=g.device)
    assert bp4_variant(describe(CASES["lds_over"]()), "minsum", B, 2, llr_ch=True, trace=True)["gmem"]
    with pytest.raises(ValueError, match="code too large for the LDS-resident trace kernel"):
        g.bp4_decode_trace(sx, sz, 2, "minsum", 0.8, llr_ch=llr)


@pytest.mark.parametrize("key", ["gb3_150", "thin"])
def test_fused_flag_bytes_inside_and_behind(key):
    """The sandwich's first decoders write the flag test of the next round from their epilogue (one codeword per workgroup): the n
    decision bytes inside the message area (gb3_150) or behind the tail (thin: E = 2n).  A wrong flag changes which samples the
    next round decodes, so the decisions and the rounds must equal the oracle's sandwich."""
    from feedback_gnn_amd.graph import GnnWeights
    from feedback_gnn_amd.weights_io import read_weight_list
    g, og, c = graphs(key)
    d = describe(c)
    assert d["codewords_per_block"] == 1
    assert bp4_variant(d, "boxplus-phi", 64, 6, flagged=True)["flag"] == ("behind" if key == "thin" else "inside")
    rng = np.random.RandomState(3)
    w = [rng.uniform(-0.5, 0.5, size=a.shape).astype(F32) for a in read_weight_list(WEIGHTS_882)]
    gw = GnnWeights(w, g.device)
    B = 64
    ex, ez = og.pauli_noise(17, 0.04, 0, B)
    sx, sz = og.syndrome(ex, ez)
    iters = [6, 4, 4]
    o = og.sandwich_decode(sx, sz, iters, [w, w], 3.2958, return_llr=True)
    got = g.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw, gw], 3.2958, return_llr=True, return_rounds=True)
    assert np.array_equal(o["x_hat"], got["x_hat"].cpu().numpy()) and np.array_equal(o["z_hat"], got["z_hat"].cpu().numpy())
    assert np.array_equal(o["rounds"], got["rounds"].cpu().numpy())
    assert bits_equal(o["llr"], got["llr"].cpu().numpy())
    assert 0 < o["rounds"].sum()
