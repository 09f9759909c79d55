"""Every device entry point of `TannerGraph` inside the guarded, poisoned allocator of tests/guarded.py.

A fresh `torch.empty` hides two errors from a bit-exact comparison: a store beside the buffer lands in the caching allocator's padding or
in a tensor nobody compares, and an element the kernel never stores can still hold the previous kernel variant's correct value, because
the freed block of the same size comes straight back.  Here every buffer of a call lies between two 64 KiB guards and starts out as
0xFF bytes, and each case asserts

  (a) both guards of every buffer of the call are intact,
  (b) no poison is left in an output include/fgnn.h says is written in full — and where the header says an element is left alone
      (OSD samples outside `index`, `chosen` of those samples) it still is poison,
  (c) the payload equals the reference of the entry point's own parity test: `==` for the forward kernels (the CPU oracle, the NumPy
      restatements tests/*_reference.py, the dense products of tests/sandwich_reference.py), the tolerances of tests/test_gpu_backward.py
      and tests/test_gpu_gnnbp4_backward.py for the three reverse passes,

and that the read-only inputs are what they were.  The guards see stores only: a read beside a buffer goes unnoticed, and so do the
buffers the model classes allocate themselves.

Shapes are the smallest with a tail in the index arithmetic: codes with n mod 4 of 3 (steane), 1 (rsurf3, rsurf5: irregular), 2 (gb126,
five checks per qubit and side) and 0 (gb48, four; ibm72, three), [[882,24]] (882 = 55 * 16 + 2: the padded 16-row tile) only for the
kernels that exist for (3,3,6)-regular graphs, at most 3 codewords of it; batches 0, 1, 3 and one more than a workgroup holds.  The
references are computed once at the largest batch and sliced: every sample is decoded on its own.

Kernels reached, and the switch that reaches them.  The dispatch rules are restated here from the launch code (fgnn_feedback_gnn_impl's
nsplit rule, launch_bp4, fgnn_gnnbp4_decode) and asserted where a size decides: they must be kept in step with it, and a change of a
rule there fails the assertion here.  Not reached: what the switches above do not select, i.e. the fixed-point exit switched off, the
opt-in hardware-transcendental BP4 and the global-memory BP4 variant of codes beyond LDS (tests/test_gpu_bp4_shapes.py runs those).
  pauli_noise / _xyz / _wt, bsc_noise   the one kernel each; host and device stream position; fresh and caller's buffers
  syndrome                              16-byte check rows (ibm72, gb48, [[882,24]]); CSR loop (irregular codes, force_generic)
  flag_update, merge                    plain, and on the index list inside sandwich_decode(compact=True)
  residual, residual_rows, count_flags, count_flags_batches, compact, pack / unpack     the one kernel each
  bp4_decode                            (3,3,6) and (4,4,8) register kernels (ibm72, [[882,24]]; gb48), runtime-degree kernel (steane,
                                        rsurf3, rsurf5, gb126; force_generic), shortcut off, set_bp4_shared_lse, set_launch(64, 4)
  bp4_decode_layered                    its own kernel, every code, three rules
  bp4_decode_trace, bp4_logit_trace     (3,3,6) trace kernel, runtime-degree trace kernel (the others, force_generic); one launch, chained
  feedback_gnn                          gnn_stream_kernel<3 / 4 / 5> (set_gnn_stream("always") on ibm72 and [[882,24]]; gb48; gb126),
                                        gnn_mfma_kernel at nsplit 16, 2 and 1 (set_gnn_stream(False)), gnn_kernel (irregular codes,
                                        force_generic), gnn_general_kernel (force_general: a max and a mean setting); each also with
                                        set_gnn_factored
  sandwich_decode                       full and compact, default launch and set_launch(64, 4), workspace of exactly the reported bytes
  bp2 / relay / relay4 / bp4gd / bp4fb / mbp4    regular instantiations (ibm72, gb48), loops (the others, force_generic), set_launch
  gnn_bp4_decode                        MFMA tiles with resident and with staged tables (FGNN_GNNBP4_NO_RESIDENT), streaming kernel
                                        (set_gnn_stream("always")), VALU kernel (irregular codes, gb48, force_generic), general kernel
  bp4_backward, feedback_gnn_backward (shipped, runtime-shaped), gnn_bp4_forward_tape / gnn_bp4_backward (compile-time, force_generic)
  osd0, osd, osd_ws                     LDS kernels on n = 13, 33, 65 and on the marginals of rsurf5 and gb48; workspace of one slot and
                                        of the default slot count; all samples, a list, a list of none
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import bp4fb_reference as FB
import bp4gd_reference as GD
import layered_reference as LR
import mbp4_reference as MB
import relay4_reference as R4
import relay_reference as R2
from feedback_gnn_amd import _lib
from feedback_gnn_amd._lib import ROWS_LX, ROWS_LZ
from feedback_gnn_amd.graph import GnnBp4Weights, GnnWeights
from guarded import guarded
from helpers import (GEN_CONFIGS, LIBRARY_BP4_SHARED_LSE, LIBRARY_GNN_FACTORED, WEIGHTS_882, binary_oracle, code, gen_cfg_codes, gen_weights,
                     gnnbp4_weights, gpu_graph, llr_const, oracle_library_forms, oracle_reassociated_forms, random_sparse_basis, to_gpu)
from sandwich_reference import dense_flagged, dense_residual, dense_syndrome, sandwich_reference
from test_mbp4_reference_cpu import ALPHAS
from test_osd_search_cpu import osd_search_batch
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

SEED = 0x5EED
F32 = np.float32
N_MOD_4 = {"steane": 3, "rsurf3": 1, "rsurf5": 1, "gb126": 2, "gb48": 0, "ibm72": 0, "ghp882": 2}
SMALL = ["steane", "rsurf3", "rsurf5", "gb126", "gb48", "ibm72"]
P_OF = {"steane": 0.15, "rsurf3": 0.15, "rsurf5": 0.15, "gb126": 0.05, "gb48": 0.08, "ibm72": 0.10, "ghp882": 0.08}


# ---- the frame of every case -----------------------------------------------------------------------------------------------------------------
# codewords per workgroup of the set_launch geometries the variants below install on these codes: (64, 4), (64, 4) and (2, 32)
LAUNCH_CPB = {"ibm72": 4, "gb48": 4, "rsurf5": 32}


def batches(name):
    """0, 1, 3 and one codeword more than a workgroup of the packing kernels holds, at the default launch and at the geometry a
    `launch-*` variant installs on the code (every variant runs the same list: the references are shared); [[882,24]] stays at 3
    codewords or fewer."""
    cpb = gpu_graph(name).info()["codewords_per_block"]
    extra = {LAUNCH_CPB[name] + 1} if name in LAUNCH_CPB else set()
    return sorted({0, 1, 3, cpb + 1} | extra) if name != "ghp882" else [0, 1, 3]


def bmax(name):
    return max(batches(name))


def test_the_codes_have_the_tails_the_cases_are_chosen_for():
    for name, r in N_MOD_4.items():
        assert gpu_graph(name).n % 4 == r, name
    deg = {name: (gpu_graph(name).info()["dv_x"], gpu_graph(name).info()["dv_z"], gpu_graph(name).info()["dc"]) for name in N_MOD_4}
    assert deg["ghp882"] == deg["ibm72"] == (3, 3, 6) and deg["gb48"] == (4, 4, 8) and deg["gb126"][:2] == (5, 5)
    assert deg["steane"][0] == 0 and deg["rsurf5"][0] == 0 and deg["rsurf3"][0] == 0  # irregular: the runtime-degree kernels
    assert gpu_graph("ghp882").n == 55 * 16 + 2
    assert all(gpu_graph(name).info()["codewords_per_block"] > 1 for name in ("steane", "rsurf3", "rsurf5", "gb48"))


def _gpu(ins):
    """Device copies of the read-only inputs and clones to compare them with afterwards."""
    t = {k: (to_gpu(v) if isinstance(v, np.ndarray) else v) for k, v in ins.items()}
    return t, {k: v.clone() for k, v in t.items() if isinstance(v, torch.Tensor)}


def _unchanged(t, keep, what):
    for k, v in keep.items():
        assert torch.equal(t[k].view(torch.uint8), v.view(torch.uint8)), f"{what}: the read-only input {k} was modified"


def _diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} differ, first at {bad[:3].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def _verify(h, out, want, what, partly=()):
    """(a) guards, (b) poison, (c) payload == reference for one call's outputs (`want` None: an empty batch, nothing to compare).
    `partly`: outputs of which only a part is written; the caller checks those."""
    h.label(out)
    h.check()
    for k, v in out.items():
        if v is not None and k not in partly:
            h.assert_written(v, f"{what} {k}")
    for k, w in (want or {}).items():
        if w is None:
            assert out[k] is None, (what, k)
            continue
        got = out[k].cpu().numpy()
        assert got.shape == w.shape, (what, k, got.shape, w.shape)
        assert np.array_equal(got, w), f"{what} {k}: {_diff(got, w)}"


def _rows(ref, B, axis1=()):
    """The first B samples of a reference computed at the largest batch; keys in `axis1` carry the batch on axis 1."""
    return {k: (None if v is None else v[:, :B] if k in axis1 else v[:B]) for k, v in ref.items()}


class switched:
    """Set the dispatcher switches of a shared graph and put the library's defaults back afterwards."""

    def __init__(self, g, generic=False, stream=True, factored=LIBRARY_GNN_FACTORED, shared_lse=LIBRARY_BP4_SHARED_LSE, launch=(0, 0),
                 shortcut=True, env=None):
        self.g, self.args, self.env = g, (generic, stream, factored, shared_lse, launch, shortcut), env

    def __enter__(self):
        generic, stream, factored, shared_lse, launch, shortcut = self.args
        self.g.force_generic(generic)
        self.g.set_gnn_stream(stream)
        self.g.set_gnn_factored(factored)
        self.g.set_bp4_shared_lse(shared_lse)
        self.g.set_launch(*launch)
        self.g.set_saturation_shortcut(shortcut)
        if self.env:
            os.environ[self.env] = "1"

    def __exit__(self, *exc):
        if self.env:
            del os.environ[self.env]
        self.g.force_generic(False)
        self.g.set_gnn_stream(True)
        self.g.set_gnn_factored(LIBRARY_GNN_FACTORED)
        self.g.set_bp4_shared_lse(LIBRARY_BP4_SHARED_LSE)
        self.g.set_launch(0, 0)
        self.g.set_saturation_shortcut(True)


@functools.lru_cache(maxsize=None)
def _noisy(name, first=40):
    """(ex, ez, sx, sz) of the oracle's seeded depolarizing stream at the largest batch of the code (read only)."""
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, P_OF[name], first, bmax(name))
    out = (ex, ez) + og.syndrome(ex, ez)
    for a in out:
        a.setflags(write=False)
    return out


def _bits(rng, shape):
    return rng.randint(0, 2, size=shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _channel(name, seed=3):
    """Per-qubit channel LLRs [bmax, 3, n]: mostly 'no error', some negative, zeros and values beyond the min-sum clip."""
    g = gpu_graph(name)
    rng = np.random.RandomState(seed)
    llr = rng.uniform(-1.0, 5.0, size=(bmax(name), 3, g.n)).astype(F32)
    special = rng.rand(*llr.shape) < 0.05
    llr[special] = rng.choice(np.array([0.0, 20.0, 25.0, -3.0], F32), size=int(special.sum()))
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _messages(name, seed=4):
    g = gpu_graph(name)
    rng = np.random.RandomState(seed)
    mx, mz = (rng.uniform(-3, 3, size=(bmax(name), E)).astype(F32) for E in (g.E_x, g.E_z))
    mx.setflags(write=False), mz.setflags(write=False)
    return mx, mz


# ---- noise -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["new", "out", "first_dev", "first_dev+out"])
@pytest.mark.parametrize("name", SMALL)
def test_pauli_noise(name, how):
    """pauli_kernel draws four qubits per Philox block: n mod 4 of 3, 1, 1, 2, 0, 0, into fresh buffers and into the caller's, with the
    stream position from the host and from a device word (whose sum with the offset crosses 2^32 inside the batch)."""
    g, og = gpu_graph(name), oracle_library_forms(name)
    for B in batches(name):
        dev = 2 ** 32 - 42 if "first_dev" in how else 0
        with guarded(g) as h:
            bufs = (h.alloc((B, g.n), torch.uint8), h.alloc((B, g.n), torch.uint8)) if "out" in how else None
            t, keep = _gpu(dict(first_dev=torch.tensor([dev], dtype=torch.int64, device=g.device)))
            ex, ez = g.pauli_noise(SEED, 0.1, 40, B, out=bufs, first_dev=t["first_dev"] if dev else None)
            assert bufs is None or (ex.data_ptr() == bufs[0].data_ptr() and ez.data_ptr() == bufs[1].data_ptr())
            want = og.pauli_noise(SEED, 0.1, 40 + dev, B) if B else None
            _verify(h, dict(noise_x=ex, noise_z=ez), want and dict(noise_x=want[0], noise_z=want[1]), f"{name} B={B} {how}")
            assert not B or len(h.records) == 2
        _unchanged(t, keep, how)


@pytest.mark.parametrize("out", [False, True], ids=["new", "out"])
@pytest.mark.parametrize("name", SMALL)
def test_pauli_noise_xyz(name, out):
    g, og = gpu_graph(name), oracle_library_forms(name)
    for B in batches(name):
        with guarded(g) as h:
            bufs = (h.alloc((B, g.n), torch.uint8), h.alloc((B, g.n), torch.uint8)) if out else None
            ex, ez = g.pauli_noise_xyz(SEED, 0.05, 0.1, 0.02, 7, B, out=bufs)
            want = og.pauli_noise_xyz(SEED, 0.05, 0.1, 0.02, 7, B) if B else None
            _verify(h, dict(noise_x=ex, noise_z=ez), want and dict(noise_x=want[0], noise_z=want[1]), f"{name} B={B}")


@pytest.mark.parametrize("out", [False, True], ids=["new", "out"])
@pytest.mark.parametrize("name", SMALL)
def test_pauli_noise_wt(name, out):
    g, og = gpu_graph(name), oracle_library_forms(name)
    for B in batches(name):
        for wt in (0, 3, g.n):
            with guarded(g) as h:
                bufs = (h.alloc((B, g.n), torch.uint8), h.alloc((B, g.n), torch.uint8)) if out else None
                ex, ez = g.pauli_noise_wt(SEED, wt, 2 ** 32 - 2, B, out=bufs)
                want = og.pauli_noise_wt(SEED, wt, 2 ** 32 - 2, B) if B else None
                _verify(h, dict(noise_x=ex, noise_z=ez), want and dict(noise_x=want[0], noise_z=want[1]), f"{name} B={B} wt={wt}")


@pytest.mark.parametrize("name", SMALL)
def test_bsc_noise(name):
    g, og = gpu_graph(name), oracle_library_forms(name)
    for B in batches(name):
        with guarded(g) as h:
            e = g.bsc_noise(SEED, 0.1, 11, B)
            _verify(h, dict(noise=e), dict(noise=og.bsc_noise(SEED, 0.1, 11, B)) if B else None, f"{name} B={B}")


# ---- byte kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["rows", "csr"])
@pytest.mark.parametrize("name", SMALL + ["ghp882"])
def test_syndrome(name, generic):
    """The 16-byte check rows of a check-regular graph (ibm72, gb48, [[882,24]]) and the CSR loop (the irregular codes; forced on all)."""
    g = gpu_graph(name)
    for B in batches(name):
        rng = np.random.RandomState(100 + B)
        ins = dict(noise_x=_bits(rng, (B, g.n)), noise_z=_bits(rng, (B, g.n)))
        sx, sz = dense_syndrome(code(name), ins["noise_x"], ins["noise_z"])
        t, keep = _gpu(ins)
        with switched(g, generic=generic), guarded(g) as h:
            tx, tz = g.syndrome(t["noise_x"], t["noise_z"])
            _verify(h, dict(synd_x=tx, synd_z=tz), dict(synd_x=sx, synd_z=sz) if B else None, f"{name} B={B}")
        _unchanged(t, keep, f"{name} B={B}")


def _estimates(name, B, salt):
    """Estimates of which about two in three reproduce their syndromes, and the syndromes."""
    c, n = code(name), gpu_graph(name).n
    rng = np.random.RandomState(1000 * salt + B)
    xh, zh = _bits(rng, (B, n)), _bits(rng, (B, n))
    sx, sz = dense_syndrome(c, xh, zh)
    flip, pos = rng.randint(0, 3, size=B), rng.randint(0, n, size=B)
    for b in range(B):
        if flip[b]:
            (xh if flip[b] == 1 else zh)[b, pos[b]] ^= 1
    return rng, xh, zh, sx, sz


@pytest.mark.parametrize("name", SMALL)
def test_flag_update(name):
    g = gpu_graph(name)
    for B in batches(name):
        rng, xh, zh, sx, sz = _estimates(name, B, 1)
        errors = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=B)
        want = ((errors != 0) & dense_flagged(code(name), xh, zh, sx, sz)).astype(np.uint8) if B else None
        t, keep = _gpu(dict(x_hat=xh, z_hat=zh, synd_x=sx, synd_z=sz))
        with guarded(g) as h:
            e = h.alloc((B,), torch.uint8, name="errors")
            e.copy_(to_gpu(errors))  # in / out: the incoming bytes replace the poison
            got = g.flag_update(t["x_hat"], t["z_hat"], t["synd_x"], t["synd_z"], e)
            h.check()
            assert got.data_ptr() == e.data_ptr()
            assert not B or np.array_equal(got.cpu().numpy(), want), (name, B)
        _unchanged(t, keep, f"{name} B={B}")


@pytest.mark.parametrize("name", SMALL)
def test_merge(name):
    g = gpu_graph(name)
    for B in batches(name):
        rng = np.random.RandomState(2000 + B)
        xh, zh, xu, zu = (rng.randint(0, 256, size=(B, g.n)).astype(np.uint8) for _ in range(4))
        errors = rng.choice(np.array([0, 1, 255], np.uint8), size=B)
        t, keep = _gpu(dict(errors=errors, x_upd=xu, z_upd=zu))
        with guarded(g) as h:
            tx, tz = h.alloc((B, g.n), torch.uint8, name="x_hat"), h.alloc((B, g.n), torch.uint8, name="z_hat")
            tx.copy_(to_gpu(xh)), tz.copy_(to_gpu(zh))
            g.merge(t["errors"], t["x_upd"], t["z_upd"], tx, tz)
            h.check()
            wx, wz = np.where(errors[:, None] != 0, xu, xh), np.where(errors[:, None] != 0, zu, zh)
            assert np.array_equal(tx.cpu().numpy(), wx) and np.array_equal(tz.cpu().numpy(), wz), (name, B)
        _unchanged(t, keep, f"{name} B={B}")


def _residual_inputs(name, B):
    """Decisions equal to the error, off by a stabilizer, off by a logical operator, random: independently per side."""
    c, n = code(name), gpu_graph(name).n
    rng = np.random.RandomState(3000 + B)
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
    return dict(noise_x=ex, noise_z=ez, x_hat=xh, z_hat=zh)


@pytest.mark.parametrize("want_arrays", [True, False], ids=["arrays", "flags-only"])
@pytest.mark.parametrize("name", SMALL)
def test_residual(name, want_arrays):
    g = gpu_graph(name)
    for B in batches(name):
        ins = _residual_inputs(name, B)
        s0, l0, f0 = dense_residual(code(name), ins["noise_x"], ins["noise_z"], ins["x_hat"], ins["z_hat"])
        t, keep = _gpu(ins)
        with guarded(g) as h:
            s1, l1, f1 = g.residual(t["noise_x"], t["noise_z"], t["x_hat"], t["z_hat"], want_arrays=want_arrays)
            want = dict(s_hat=s0 if want_arrays else None, ls_hat=l0 if want_arrays else None, flags=f0)
            assert want_arrays or (s1 is None and l1 is None and len(h.records) == 1)
            _verify(h, dict(s_hat=s1, ls_hat=l1, flags=f1), want if B else None, f"{name} B={B}")
        _unchanged(t, keep, f"{name} B={B}")


@pytest.mark.parametrize("name", SMALL)
def test_residual_rows(name):
    c, g = code(name), gpu_graph(name)
    for B in batches(name):
        ins = _residual_inputs(name, B)
        _, l0, f0 = dense_residual(c, ins["noise_x"], ins["noise_z"], ins["x_hat"], ins["z_hat"], rows_x=c.lz, rows_z=c.lx)
        t, keep = _gpu(ins)
        with guarded(g) as h:
            l1, f1 = g.residual_rows(ROWS_LZ, ROWS_LX, t["noise_x"], t["noise_z"], t["x_hat"], t["z_hat"])
            _verify(h, dict(ls_hat=l1, flags=f1), dict(ls_hat=l0, flags=f0) if B else None, f"{name} B={B}")
        _unchanged(t, keep, f"{name} B={B}")


def _count_ref(flags):
    f = flags.astype(np.int64)
    return np.array([(f & 1).sum(), ((f >> 1) & 1).sum(), f.shape[0]], np.int64)


@pytest.mark.parametrize("B", [0, 1, 3, 255, 257])
def test_count_flags(B):
    g = gpu_graph("steane")
    flags = np.random.RandomState(B).randint(0, 4, size=B).astype(np.uint8)
    start = np.array([5, 7, 11], np.int64)
    t, keep = _gpu(dict(flags=flags))
    with guarded(g) as h:
        counts = h.alloc((3,), torch.int64, name="counts")
        counts.copy_(to_gpu(start))
        g.count_flags(t["flags"], counts)
        h.check()
        assert np.array_equal(counts.cpu().numpy(), start + (_count_ref(flags) if B else 0))
    _unchanged(t, keep, B)


@pytest.mark.parametrize("k,batch", [(1, 1), (3, 5), (3, 255), (2, 257)])
def test_count_flags_batches(k, batch):
    g = gpu_graph("steane")
    flags = np.random.RandomState(100 * k + batch).randint(0, 4, size=k * batch).astype(np.uint8)
    start = np.array([3, 1, 4], np.int64)
    want = start + np.cumsum(np.stack([_count_ref(flags[j * batch:(j + 1) * batch]) for j in range(k)]), axis=0)
    t, keep = _gpu(dict(flags=flags))
    with guarded(g) as h:
        counts, ring = h.alloc((3,), torch.int64, name="counts"), h.alloc((k, 3), torch.int64, name="ring")
        counts.copy_(to_gpu(start))
        g.count_flags_batches(t["flags"], batch, counts, ring)
        assert len(h.records) == 3  # counts, ring and the wrapper's scratch words
        _verify(h, dict(ring=ring, counts=counts), dict(ring=want, counts=want[-1]), f"k={k} batch={batch}")
    _unchanged(t, keep, (k, batch))


@pytest.mark.parametrize("bit", [1, 2])
@pytest.mark.parametrize("B", [0, 1, 3, 255, 256, 257])
def test_compact(B, bit):
    """index[0 .. count) is written, one id each; the count word goes through the allocator as well."""
    g = gpu_graph("steane")
    rng = np.random.RandomState(7 * B + bit)
    for fill in (0.0, 0.4, 1.0):
        mask = np.where(rng.random_sample(B) < fill, rng.choice(np.array([bit, 3], np.uint8), size=B),
                        rng.choice(np.array([0, 3 - bit], np.uint8), size=B)).astype(np.uint8)
        want = np.nonzero(mask & bit)[0]
        t, keep = _gpu(dict(mask=mask))
        with guarded(g) as h:
            index, count = g.compact(t["mask"], bit=bit)
            h.check()
            assert len(h.records) == 2 and count == len(want), (B, bit, fill)
            h.assert_written(index[:count], "index[:count]")
            assert np.array_equal(np.sort(index[:count].cpu().numpy()), want), (B, bit, fill)
        _unchanged(t, keep, (B, bit))


@pytest.mark.parametrize("name", SMALL + ["ghp882"])
def test_pack_and_unpack_decisions(name):
    """fgnn_pack_decisions / fgnn_unpack_decisions on guarded buffers (utils.pack_decisions allocates its own): the last byte of a row
    holds 2n mod 8 bits (6, 2, 2, 4, 0, 0, 4) and the x|z seam falls inside a byte where n mod 8 != 0."""
    g, L = gpu_graph(name), _lib.lib()
    n, nb = g.n, (2 * g.n + 7) // 8
    stream = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    for B, flip in [(B, flip) for B in batches(name) for flip in (0, 1)]:
        # a packed byte of eight ones IS the poison value, so the poison count proves nothing here: the bits and their complement are
        # packed instead, and a byte that is never stored (0xFF both times) differs from one of the two references
        rng = np.random.RandomState(4000 + B)
        xh, zh = _bits(rng, (B, n)) ^ np.uint8(flip), _bits(rng, (B, n)) ^ np.uint8(flip)
        want = np.packbits(np.concatenate([xh, zh], axis=1), axis=1) if B else np.zeros((0, nb), np.uint8)
        t, keep = _gpu(dict(x_hat=xh, z_hat=zh))
        with guarded(g) as h, torch.cuda.device(g.device):
            packed = h.alloc((B, nb), torch.uint8, name="packed")
            _lib.check(L.fgnn_pack_decisions(ptr(t["x_hat"]), ptr(t["z_hat"]), B, n, ptr(packed), stream))
            _verify(h, dict(packed=packed), dict(packed=want), f"{name} B={B} pack", partly=("packed",))
            before = packed.clone()
            ux, uz = h.alloc((B, n), torch.uint8, name="x_hat"), h.alloc((B, n), torch.uint8, name="z_hat")
            _lib.check(L.fgnn_unpack_decisions(ptr(packed), B, n, ptr(ux), ptr(uz), stream))
            _verify(h, dict(x_hat=ux, z_hat=uz), dict(x_hat=xh, z_hat=zh), f"{name} B={B} unpack")
            assert torch.equal(packed, before)
        _unchanged(t, keep, f"{name} B={B}")


# ---- BP4 ---------------------------------------------------------------------------------------------------------------------------------------
BP4_KEYS = ("llr", "x_hat", "z_hat", "x_logit", "z_logit", "msg_x", "msg_z")
# the kernels launch_bp4 can pick: the (3,3,6) and (4,4,8) register-resident ones, the runtime-degree one (irregular codes, dv = 5, and
# forced), each with the saturation shortcut on and off, the shared log-sum-exp form, and a launch with several codewords per workgroup
BP4_VARIANTS = {"default": {}, "generic": dict(generic=True), "no-shortcut": dict(shortcut=False), "shared-lse": dict(shared_lse=True),
                "launch-64x4": dict(launch=(64, 4)), "launch-2x32": dict(launch=(2, 32))}


@functools.lru_cache(maxsize=None)
def _bp4_ref(name, cn_type, iters, chan, init, shared_lse=False):
    og = (oracle_reassociated_forms if shared_lse else oracle_library_forms)(name)
    _, _, sx, sz = _noisy(name)
    kw = dict(llr_ch=_channel(name)) if chan == "llr_ch" else dict(llr_const=llr_const(P_OF[name]))
    o = og.bp4_decode(sx, sz, iters, cn_type, 0.8, msg_init=_messages(name) if init else None, return_msgs=True, **kw)
    for a in o.values():
        a.setflags(write=False)
    return o


def _bp4_case(name, variant, cn_type, iters, chan, init, return_msgs, want_logits, layered=False):
    g = gpu_graph(name)
    sw = BP4_VARIANTS[variant]
    if layered:
        _, _, sx, sz = _noisy(name)
        kw = dict(llr_ch=_channel(name)) if chan == "llr_ch" else dict(llr_const=llr_const(P_OF[name]))
        ref = LR.layered_decode(oracle_library_forms(name), sx, sz, iters, cn_type, 0.8, msg_init=_messages(name) if init else None, **kw)
    else:
        ref = _bp4_ref(name, cn_type, iters, chan, init, bool(sw.get("shared_lse")))
    for B in batches(name):
        _, _, sx, sz = _noisy(name)
        ins = dict(synd_x=sx[:B], synd_z=sz[:B])
        if chan == "llr_ch":
            ins["llr_ch"] = _channel(name)[:B]
        if init:
            ins["msg_init_x"], ins["msg_init_z"] = (m[:B] for m in _messages(name))
        t, keep = _gpu(ins)
        what = f"{name} {variant} {cn_type} B={B}"
        with switched(g, **sw), guarded(g) as h:
            fn = g.bp4_decode_layered if layered else g.bp4_decode
            out = fn(t["synd_x"], t["synd_z"], iters, cn_type, 0.8, llr_ch=t.get("llr_ch"), llr_const=llr_const(P_OF[name]),
                     msg_init=(t["msg_init_x"], t["msg_init_z"]) if init else None, return_msgs=return_msgs, want_logits=want_logits)
            assert (out["x_logit"] is None) == (not want_logits) and ("msg_x" in out) == return_msgs
            assert len(h.records) == 3 + 2 * want_logits + 2 * return_msgs, "a buffer that is not part of the call"
            want = {k: ref[k] for k in BP4_KEYS if out.get(k) is not None}
            _verify(h, out, _rows(want, B) if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("cn_type", ["boxplus-phi", "minsum", "boxplus"])
@pytest.mark.parametrize("name,variant", [(n, "default") for n in SMALL + ["ghp882"]] + [(n, "generic") for n in ("ibm72", "gb48", "ghp882")]
                         + [(n, "no-shortcut") for n in ("ibm72", "gb48", "rsurf5")] + [(n, "shared-lse") for n in ("ibm72", "gb48", "rsurf5")]
                         + [("ibm72", "launch-64x4"), ("rsurf5", "launch-64x4")])
def test_bp4_decode(name, variant, cn_type):
    """Constant prior, zero start, every optional output asked for."""
    _bp4_case(name, variant, cn_type, 3, "llr_const", False, True, True)


@pytest.mark.parametrize("return_msgs,want_logits", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("name,variant", [("steane", "default"), ("rsurf5", "default"), ("gb48", "default"), ("ibm72", "default"),
                                          ("ibm72", "generic"), ("ghp882", "default")])
def test_bp4_decode_optional_outputs_llr_ch_and_msg_init(name, variant, return_msgs, want_logits):
    """Per-qubit channel LLRs, a start from given messages, and each optional output passed as NULL."""
    _bp4_case(name, variant, "boxplus-phi", 2, "llr_ch", True, return_msgs, want_logits)


@pytest.mark.parametrize("name,variant", [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("gb48", "launch-64x4")])
def test_bp4_decode_zero_and_one_iteration(name, variant):
    _bp4_case(name, variant, "boxplus-phi", 0, "llr_ch", True, True, True)
    _bp4_case(name, variant, "minsum", 1, "llr_const", False, True, True)


@pytest.mark.parametrize("cn_type", ["boxplus-phi", "minsum", "boxplus"])
@pytest.mark.parametrize("name", SMALL)
def test_bp4_decode_layered(name, cn_type):
    _bp4_case(name, "default", cn_type, 2, "llr_const", False, True, True, layered=True)
    _bp4_case(name, "default", cn_type, 1, "llr_ch", True, False, False, layered=True)


TRACE_AXIS1 = ("x_logit", "z_logit", "tape_x", "tape_z")


@functools.lru_cache(maxsize=None)
def _trace_ref(name, cn_type, T, chan, init):
    """The oracle run with 0, 1, ..., T iterations: soft syndromes and messages after each."""
    steps = [_bp4_ref(name, cn_type, k, chan, init) for k in range(T + 1)]
    ref = dict(x_logit=np.stack([s["x_logit"] for s in steps]), z_logit=np.stack([s["z_logit"] for s in steps]),
               tape_x=np.stack([s["msg_x"] for s in steps]), tape_z=np.stack([s["msg_z"] for s in steps]))
    ref.update({k: steps[-1][k] for k in ("llr", "x_hat", "z_hat")})
    return ref


@pytest.mark.parametrize("want_tape", [True, False], ids=["tape", "no-tape"])
@pytest.mark.parametrize("name,variant,cn_type", [("steane", "default", "boxplus-phi"), ("rsurf3", "default", "minsum"),
                                                  ("rsurf5", "default", "boxplus"), ("gb126", "default", "boxplus-phi"),
                                                  ("gb48", "default", "boxplus-phi"), ("ibm72", "default", "boxplus-phi"),
                                                  ("ibm72", "generic", "minsum"), ("ghp882", "default", "boxplus-phi")])
def test_bp4_decode_trace(name, variant, cn_type, want_tape):
    """x_logit / z_logit / tape are indexed [k, b, r], k = 0 .. T: the last slot and the last codeword of every slot."""
    g, T = gpu_graph(name), 3
    ref = _trace_ref(name, cn_type, T, "llr_ch", True)
    for B in batches(name):
        _, _, sx, sz = _noisy(name)
        t, keep = _gpu(dict(synd_x=sx[:B], synd_z=sz[:B], llr_ch=_channel(name)[:B], mx=_messages(name)[0][:B], mz=_messages(name)[1][:B]))
        what = f"{name} {variant} {cn_type} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            out = g.bp4_decode_trace(t["synd_x"], t["synd_z"], T, cn_type, 0.8, llr_ch=t["llr_ch"], msg_init=(t["mx"], t["mz"]),
                                     want_tape=want_tape)
            assert len(h.records) == 5 + 2 * want_tape
            want = {k: v for k, v in ref.items() if k in out}
            _verify(h, out, _rows(want, B, TRACE_AXIS1) if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("chained", [False, True], ids=["one-launch", "chained"])
@pytest.mark.parametrize("name", ["steane", "rsurf5", "gb48", "ibm72"])
def test_bp4_logit_trace(name, chained):
    g, T = gpu_graph(name), 3
    ref = _trace_ref(name, "boxplus-phi", T, "llr_ch", False)
    for B in batches(name):
        _, _, sx, sz = _noisy(name)
        t, keep = _gpu(dict(synd_x=sx[:B], synd_z=sz[:B], llr_ch=_channel(name)[:B]))
        what = f"{name} chained={chained} B={B}"
        with guarded(g) as h:
            out = g.bp4_logit_trace(t["llr_ch"], t["synd_x"], t["synd_z"], T, 0.8, chained=chained)
            _verify(h, out, _rows(ref, B, TRACE_AXIS1) if B else None, what)
        _unchanged(t, keep, what)


# ---- feedback GNN ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gnn_weights(kind):
    from feedback_gnn_amd.weights_io import read_weight_list
    w = read_weight_list(WEIGHTS_882)
    if kind == "random":  # no near-zero column hides a wrong element
        rng = np.random.RandomState(9)
        w = [rng.uniform(-0.7, 0.7, size=a.shape).astype(F32) for a in w]
    return w


def _gnn_inputs(name, B):
    """Marginals and soft syndromes of a 3-iteration decode of B seeded syndromes (the oracle's)."""
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, P_OF[name], 40, B)
    sx, sz = og.syndrome(ex, ez)
    o = og.bp4_decode(sx, sz, 3, "boxplus-phi", 1.0, llr_const=llr_const(P_OF[name]))
    return dict(llr=o["llr"], logit_hx=o["z_logit"], logit_hz=o["x_logit"], synd_x=sx, synd_z=sz)


@functools.lru_cache(maxsize=None)
def _gnn_ref(name, B, factored, cfg=None):
    og = (oracle_reassociated_forms if factored else oracle_library_forms)(name)
    ins = _gnn_inputs(name, B)
    if cfg is None:
        ref = og.feedback_gnn(_gnn_weights("random"), *ins.values())
    else:
        ref = og.feedback_gnn_general(gen_cfg_codes(cfg), gen_weights(cfg), *ins.values())
    for a in list(ins.values()) + [ref]:
        a.setflags(write=False)
    return ins, ref


def _gnn_case(name, Bs, sw, cfg=None, force_general=False):
    g = gpu_graph(name)
    factored = bool(sw.get("factored"))
    W = GnnWeights(_gnn_weights("random"), g.device) if cfg is None else GnnWeights(gen_weights(cfg), g.device, config=cfg,
                                                                                   force_general=force_general)
    ins_max, ref = _gnn_ref(name, max(Bs), factored, cfg)
    for B in Bs:
        t, keep = _gpu(_rows(ins_max, B))
        what = f"{name} {sw} cfg={cfg} B={B}"
        with switched(g, **sw), guarded(g) as h:
            out = g.feedback_gnn(W, *t.values())
            assert len(h.records) == 1
            _verify(h, dict(out=out), dict(out=ref[:B]) if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("factored", [False, True], ids=["literal", "factored"])
@pytest.mark.parametrize("name,dv,stream", [("ibm72", 3, "always"), ("ghp882", 3, "always"), ("gb48", 4, True), ("gb126", 5, True)])
def test_feedback_gnn_stream_kernels(name, dv, stream, factored):
    """gnn_stream_kernel<3 / 4 / 5>: one workgroup per codeword, one lane per qubit (n = 72, 882, 48, 126 over 128 lanes and more)."""
    info = gpu_graph(name).info()
    assert info["dv_x"] == info["dv_z"] == dv
    _gnn_case(name, batches(name), dict(stream=stream, factored=factored))


@pytest.mark.parametrize("factored", [False, True], ids=["literal", "factored"])
@pytest.mark.parametrize("name,Bs,nsplit", [("ghp882", (0, 1, 3), 16), ("ibm72", (1, 3, 5), 2), ("ibm72", (1024,), 2), ("ibm72", (1025,), 1)])
def test_feedback_gnn_mfma_tile_kernel(name, Bs, nsplit, factored):
    """gnn_mfma_kernel with its tiles dealt to `nsplit` wave-quads: 16 for 1 and 3 codewords of [[882,24]] (56 tiles, the last holds 2 of
    16 rows), 2 for the five tiles of ibm72 (the last holds 8 rows) up to 1 024 codewords, 1 from 1 025 on; four slots per workgroup,
    so B nsplit is no multiple of 4 at B = 1, 3, 5 and 1 025."""
    g = gpu_graph(name)
    ntiles = (g.n + 15) // 16
    for B in Bs:
        ns = 1
        while B and ns < 16 and B * ns * 2 <= 2048 and ns * 4 < ntiles:  # the rule of fgnn_feedback_gnn_impl
            ns *= 2
        assert not B or ns == nsplit, (name, B, ns)
    _gnn_case(name, Bs, dict(stream=False, factored=factored))


@pytest.mark.parametrize("factored", [False, True], ids=["literal", "factored"])
@pytest.mark.parametrize("name,generic", [("steane", False), ("rsurf3", False), ("rsurf5", False), ("ibm72", True), ("gb48", True)])
def test_feedback_gnn_valu_kernel(name, generic, factored):
    """gnn_kernel: any graph, `codewords_per_block` codewords per workgroup."""
    _gnn_case(name, batches(name), dict(generic=generic, factored=factored))


@pytest.mark.parametrize("cfg", [GEN_CONFIGS[1], GEN_CONFIGS[4], GEN_CONFIGS[0]], ids=["max", "mean", "shipped-as-general"])
@pytest.mark.parametrize("name", ["rsurf5", "gb48", "ibm72"])
def test_feedback_gnn_general_kernel(name, cfg):
    assert cfg[3] in ("max", "mean")
    _gnn_case(name, batches(name), {}, cfg=cfg, force_general=True)


# ---- sandwich ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sandwich_ref(name, iters):
    og = oracle_library_forms(name)
    _, _, sx, sz = _noisy(name, first=31)
    w = _gnn_weights("shipped")
    ref = sandwich_reference(og, sx, sz, list(iters), [w] * (len(iters) - 1), llr_const(0.05))
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("return_llr,return_rounds", [(True, True), (False, False)], ids=["llr+rounds", "decisions-only"])
@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
@pytest.mark.parametrize("name,launch", [("steane", (0, 0)), ("rsurf3", (0, 0)), ("rsurf5", (0, 0)), ("gb126", (0, 0)), ("gb48", (0, 0)),
                                         ("ibm72", (0, 0)), ("ibm72", (64, 4)), ("ghp882", (0, 0))])
def test_sandwich_decode(name, launch, compact, return_llr, return_rounds):
    """BP / GNN / BP / GNN / BP with 1, 2 and 8 iterations on a workspace of exactly `fgnn_sandwich_workspace_bytes`; `compact` runs
    flag_update, the feedback GNN, BP4 and merge on the index list of the samples still flagged."""
    g, iters = gpu_graph(name), (1, 2, 8)
    ref = _sandwich_ref(name, iters)
    W = GnnWeights(_gnn_weights("shipped"), g.device)
    for B in batches(name):
        _, _, sx, sz = _noisy(name, first=31)
        t, keep = _gpu(dict(synd_x=sx[:B], synd_z=sz[:B]))
        what = f"{name} launch={launch} compact={compact} B={B}"
        with switched(g, launch=launch), guarded(g) as h:
            out = g.sandwich_decode(t["synd_x"], t["synd_z"], list(iters), [W, W], llr_const(0.05), compact=compact, return_llr=return_llr,
                                    return_rounds=return_rounds)
            assert len(h.records) == 3 + return_llr + return_rounds and h.records[0].shape == (_lib.lib().fgnn_sandwich_workspace_bytes(g.handle, B),)
            want = dict(x_hat=ref["x_hat"], z_hat=ref["z_hat"])
            if return_rounds:
                want["rounds"] = ref["rounds"]
            if return_llr:
                want["llr"] = ref["llr_compact"] if compact else ref["llr"]
            _verify(h, out, _rows(want, B) if B else None, what)
        _unchanged(t, keep, what)
    assert ref["rounds"].max() >= 1, "no sample reaches a feedback round"


# ---- binary BP and the newer decoders ----------------------------------------------------------------------------------------------------------
def _hx_syndromes(name, B, seed=5):
    hx = np.asarray(code(name).hx, np.int64)
    e = (np.random.RandomState(seed).rand(B, hx.shape[1]) < P_OF[name]).astype(np.int64)
    return (e @ hx.T % 2).astype(np.uint8)


@pytest.mark.parametrize("want_soft,want_hard", [(True, True), (True, False), (False, True)], ids=["both", "soft", "hard"])
@pytest.mark.parametrize("cn_type", ["boxplus-phi", "minsum", "boxplus"])
@pytest.mark.parametrize("name,variant", [(n, "default") for n in SMALL + ["ghp882"]] + [("ibm72", "generic"), ("gb48", "generic"),
                                          ("rsurf5", "launch-2x32"), ("ibm72", "launch-64x4")])
def test_bp2_decode(name, variant, cn_type, want_soft, want_hard):
    g, og = gpu_graph(name), oracle_library_forms(name)
    synd = _hx_syndromes(name, bmax(name))
    L = float(-np.log((F32(1) - F32(0.2)) / F32(0.2), dtype=F32))
    s0, h0 = og.bp2_decode(synd, 3, cn_type, 0.8, llr_const=L)
    for B in batches(name):
        t, keep = _gpu(dict(synd=synd[:B]))
        what = f"{name} {variant} {cn_type} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            soft, hard = g.bp2_decode(t["synd"], 3, cn_type, 0.8, llr_const=L, want_soft=want_soft, want_hard=want_hard)
            assert len(h.records) == want_soft + want_hard
            want = dict(soft=s0[:B] if want_soft else None, hard=h0[:B] if want_hard else None)
            _verify(h, dict(soft=soft, hard=hard), want if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("name,variant", [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("gb48", "generic"), ("rsurf5", "launch-2x32"),
                                          ("ibm72", "launch-64x4")])
def test_relay_decode(name, variant):
    g = gpu_graph(name)
    hx = np.asarray(code(name).hx)
    synd, gamma = _hx_syndromes(name, bmax(name)), mixed_gamma(3, g.n, 3)
    L = float(-np.log((F32(1) - F32(P_OF[name])) / F32(P_OF[name]), dtype=F32))
    h0, s0, _ = R2.relay_decode(hx, synd, gamma, 3, 2, 1, 0.8, llr_const=L)
    for B in batches(name):
        t, keep = _gpu(dict(synd=synd[:B], gamma=gamma))
        what = f"{name} {variant} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            hard, stats = g.relay_decode(t["synd"], t["gamma"], 3, 2, 1, 0.8, llr_const=L)
            assert len(h.records) == 2
            _verify(h, dict(hard=hard, stats=stats), dict(hard=h0[:B], stats=s0[:B]) if B else None, what)
        _unchanged(t, keep, what)


QUATERNARY = [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("rsurf5", "launch-2x32"), ("ibm72", "launch-64x4")]


def _bp4_family_case(name, variant, run_gpu, run_ref, gamma=None):
    """x_hat, z_hat and stats of one of the quaternary decoders with a stopping rule against its restatement."""
    g = gpu_graph(name)
    _, _, sx, sz = _noisy(name)
    x0, z0, s0 = run_ref(sx, sz)[:3]
    for B in batches(name):
        t, keep = _gpu(dict(synd_x=sx[:B], synd_z=sz[:B], **({} if gamma is None else dict(gamma=gamma))))
        what = f"{name} {variant} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            xh, zh, stats = run_gpu(g, t["synd_x"], t["synd_z"], t.get("gamma"))
            _verify(h, dict(x_hat=xh, z_hat=zh, stats=stats), dict(x_hat=x0[:B], z_hat=z0[:B], stats=s0[:B]) if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("name,variant", QUATERNARY)
def test_relay4_decode(name, variant):
    og, L = oracle_library_forms(name), llr_const(P_OF[name])
    gamma = mixed_gamma(3, og.n, 1)
    _bp4_family_case(name, variant, lambda g, sx, sz, gam: g.relay4_decode(sx, sz, gam, 3, 2, 1, 0.8, llr_const=L),
                     lambda sx, sz: R4.relay4_decode(og, sx, sz, gamma, 3, 2, 1, 0.8, llr_const=L), gamma=gamma)


@pytest.mark.parametrize("name,variant", QUATERNARY)
def test_bp4gd_decode(name, variant):
    og, L = oracle_library_forms(name), llr_const(P_OF[name])
    _bp4_family_case(name, variant, lambda g, sx, sz, _: g.bp4gd_decode(sx, sz, 3, 2, 4, 25.0, "minsum", 0.8, llr_const=L),
                     lambda sx, sz: GD.bp4gd_decode(og, sx, sz, 3, 2, 4, 25.0, "minsum", 0.8, llr_const=L))


@pytest.mark.parametrize("rule,strength,restart", [("perturb", 2.0, False), ("enhanced", 10.0, True)])
@pytest.mark.parametrize("name,variant", QUATERNARY)
def test_bp4fb_decode(name, variant, rule, strength, restart):
    og, L = oracle_library_forms(name), llr_const(P_OF[name])
    _bp4_family_case(name, variant,
                     lambda g, sx, sz, _: g.bp4fb_decode(sx, sz, rule, 3, 2, 3, strength, "minsum", 0.8, restart=restart, seed=SEED,
                                                         first_sample=0, llr_const=L),
                     lambda sx, sz: FB.bp4fb_decode(og, sx, sz, rule, 3, 2, 3, strength, "minsum", 0.8, restart=restart, seed=SEED,
                                                    first_sample=0, llr_const=L))


@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("name,variant", QUATERNARY)
def test_mbp4_decode(name, variant, restart):
    L = llr_const(P_OF[name])
    factors, owns = MB.mbp4_tables(ALPHAS[:3], 1.0)
    _bp4_family_case(name, variant, lambda g, sx, sz, _: g.mbp4_decode(sx, sz, factors, owns, 3, 2, "minsum", restart=restart, llr_const=L),
                     lambda sx, sz: MB.mbp4_decode(code(name), sx, sz, factors, owns, 3, 2, "minsum", restart=restart, llr_const=L))


# ---- GNN_BP4 -----------------------------------------------------------------------------------------------------------------------------------
GNNBP4_KEYS = ("x_hat", "z_hat", "llr", "x_logit_all", "z_logit_all")
GNNBP4_AXIS1 = ("x_logit_all", "z_logit_all")
GNNBP4_GENERAL = (8, 16, 1, "max", "relu", False, False, 0, 0)


@functools.lru_cache(maxsize=None)
def _gnnbp4_ref(name, T, factored, general):
    og = (oracle_reassociated_forms if factored else oracle_library_forms)(name)
    _, _, sx, sz = _noisy(name)
    if general:
        from test_gpu_parity import _gnnbp4_cfg_codes, _gnnbp4_gen_weights
        return og.gnn_bp4_general(_gnnbp4_cfg_codes(GNNBP4_GENERAL), _gnnbp4_gen_weights(gpu_graph(name), GNNBP4_GENERAL), sx, sz, T)
    return og.gnn_bp4(gnnbp4_weights(11), sx, sz, T)


def _gnnbp4_case(name, sw, general=False, return_logits=True):
    """`gnn_bp4_decode` on a caller workspace of exactly `workspace_bytes` (and once on the wrapper's own, which now goes through the
    allocator): one workgroup per codeword."""
    g, T = gpu_graph(name), 2
    ref = _gnnbp4_ref(name, T, bool(sw.get("factored")), general)
    if general:
        from test_gpu_parity import _gnnbp4_gen_weights
        W = GnnBp4Weights(_gnnbp4_gen_weights(g, GNNBP4_GENERAL), g.device, config=GNNBP4_GENERAL, graph=g, force_general=True)
    else:
        W = GnnBp4Weights(gnnbp4_weights(11), g.device)
    for B in batches(name):
        _, _, sx, sz = _noisy(name)
        t, keep = _gpu(dict(synd_x=sx[:B], synd_z=sz[:B]))
        for own_workspace in (True, False):
            what = f"{name} {sw} general={general} B={B} caller's workspace={own_workspace}"
            with switched(g, **sw), guarded(g) as h:
                nbytes = _lib.lib().fgnn_gnnbp4_weights_workspace_bytes(g.handle, W.handle, B)
                ws = h.alloc((nbytes,), torch.uint8, name="workspace") if own_workspace else None
                out = g.gnn_bp4_decode(W, t["synd_x"], t["synd_z"], T, return_logits=return_logits, workspace=ws)
                assert len(h.records) == 4 + 2 * return_logits and h.records[0].shape == (nbytes,)
                want = {k: ref[k] for k in GNNBP4_KEYS if out[k] is not None}
                _verify(h, out, _rows(want, B, GNNBP4_AXIS1) if B else None, what)
            _unchanged(t, keep, what)


@pytest.mark.parametrize("factored", [False, True], ids=["literal", "factored"])
@pytest.mark.parametrize("name,tables", [("ibm72", "resident"), ("ghp882", "resident"), ("ibm72", "staged"), ("ghp882", "staged")])
def test_gnn_bp4_mfma_kernel(name, tables, factored):
    """The MFMA tiles of a (3,3,6)-regular graph, operand tables resident in LDS or staged per phase; n = 72 and 882 end in a tile of 8
    and of 2 rows."""
    _gnnbp4_case(name, dict(factored=factored, env="FGNN_GNNBP4_NO_RESIDENT" if tables == "staged" else None))


@pytest.mark.parametrize("name", ["ibm72", "ghp882"])
def test_gnn_bp4_stream_kernel(name):
    _gnnbp4_case(name, dict(stream="always"))
    _gnnbp4_case(name, dict(stream="always"), return_logits=False)


@pytest.mark.parametrize("factored", [False, True], ids=["literal", "factored"])
@pytest.mark.parametrize("name,generic", [("rsurf5", False), ("gb48", False), ("steane", False), ("ibm72", True)])
def test_gnn_bp4_valu_kernel(name, generic, factored):
    _gnnbp4_case(name, dict(generic=generic, factored=factored))


@pytest.mark.parametrize("name", ["rsurf5", "gb48", "ibm72"])
def test_gnn_bp4_general_kernel(name):
    _gnnbp4_case(name, {}, general=True)


# ---- reverse passes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,loss_from,factor", [("gb48", 4, 0, 0.9), ("rsurf5", 6, 2, 1.0)])
def test_bp4_backward(name, T, loss_from, factor):
    """The case, inputs and bound of tests/test_gpu_backward.py (2e-3 of the gradient's largest entry against float64 autograd), on a
    guarded tape and a guarded gradient."""
    from oracle import torch_ref as R
    from test_gpu_backward import _bce_grads, _case, _rel
    g, sx, sz, llr = _case(name, 4, 0.03, 0.8, 2.5)
    t, keep = _gpu(dict(llr_ch=llr, synd_x=sx, synd_z=sz))
    with guarded(g) as h:
        tr = g.bp4_logit_trace(t["llr_ch"], sx, sz, T, factor)
        h.label(tr)
        h.check()
        for k, v in tr.items():
            h.assert_written(v, f"trace {k}")
        _, gx, gz = _bce_grads(g, tr, sx, sz, loss_from, T)
        tape = {k: tr[k].clone() for k in ("tape_x", "tape_z")}
        grads_in = dict(grad_x_logit=gx, grad_z_logit=gz)
        grads_kept = {k: v.clone() for k, v in grads_in.items()}
        first = len(h.records)
        got = g.bp4_backward(t["llr_ch"], sx, sz, tr["tape_x"], tr["tape_z"], gx, gz, factor)
        assert len(h.records) == first + 1
        _verify(h, dict(grad_llr=got), None, f"{name} backward")
        assert all(torch.equal(tr[k], v) for k, v in tape.items()), "the tape is a read-only input of the reverse pass"
        _unchanged(grads_in, grads_kept, f"{name} backward")
    _unchanged(t, keep, name)
    tg = R.Graph(code(name))
    Lr = torch.from_numpy(llr).to(R.DT).requires_grad_(True)
    xs, zs, _ = R.bp4_logit_trace(tg, Lr, sx.cpu(), sz.cpu(), T, factor)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    gt_x, gt_z = (1 - sz.cpu()).to(R.DT), (1 - sx.cpu()).to(R.DT)
    sum(bce(xs[i + 1], gt_x) + bce(zs[i + 1], gt_z) for i in range(loss_from, T)).backward()
    err = _rel(got.cpu().numpy(), Lr.grad.numpy())
    print(f"{name}: rel err {err:.2e}")
    assert np.isfinite(got.cpu().numpy()).all() and err < 2e-3, err


@pytest.mark.parametrize("name,cfg", [("gb48", None), ("rsurf5", None), ("gb48", (8, 16, 1, "mean", "tanh", True)),
                                      ("rsurf5", (12, 24, 3, "sum", "relu", False))], ids=["gb48-shipped", "rsurf5-shipped", "gb48-runtime",
                                                                                         "rsurf5-runtime"])
def test_feedback_gnn_backward(name, cfg):
    """The shipped reverse kernel and the runtime-shaped one, which shrinks its workgroup to the widest layer: the cases, inputs and bounds
    of tests/test_gpu_backward.py (1e-3 / 2e-3 of each gradient's largest entry), every (activation, delta) buffer between guards.  A
    buffer must be written in full (include/fgnn.h), which the poison shows per buffer and element."""
    from oracle import torch_ref as R
    from feedback_gnn_amd.graph import ACTIVATIONS, REDUCE_OPS, gnn_weight_shapes
    from feedback_gnn_amd.weights_io import read_weight_list
    from test_gpu_backward import _case, _rel
    B = 3
    g, sx, sz, llr = _case(name, B, 0.04, -2.0, 6.0)
    if cfg is None:
        rng = np.random.RandomState(5)
        w = read_weight_list(WEIGHTS_882)
        w[0] = rng.uniform(-0.4, 0.4, size=w[0].shape).astype(F32)
        lim, tol = 8, 1e-3
        W = GnnWeights(w, g.device)
    else:
        rng = np.random.RandomState(17)
        w = [rng.uniform(-0.5, 0.5, size=shp).astype(F32) for shp in gnn_weight_shapes(cfg[0], cfg[1], cfg[2], cfg[5])]
        lim, tol = 4, 2e-3
        W = GnnWeights(w, g.device, config=cfg, force_general=True)
    lhx = rng.uniform(-lim, lim, size=(B, g.m_x)).astype(F32)
    lhz = rng.uniform(-lim, lim, size=(B, g.m_z)).astype(F32)
    gout = rng.normal(size=(B, 3, g.n)).astype(F32)
    t, keep = _gpu(dict(llr=llr, logit_hx=lhx, logit_hz=lhz, synd_x=sx, synd_z=sz, grad_out=gout))
    with guarded(g) as h:
        grads = g.feedback_gnn_backward(W, *t.values())
        h.check()
        if cfg is None:
            names = ["node_in", "node_h2", "node_d2"] + [f"{k}[{s}]" for k in ("edge_feat", "h1", "d1", "dm") for s in (0, 1)]
        else:
            names = [f"acts[{i}]" for i in range(3 * cfg[2])] + [f"deltas[{i}]" for i in range(3 * cfg[2])]
        assert len(h.records) == len(names) == (11 if cfg is None else 6 * cfg[2])
        for rec, nm in zip(h.records, names):  # include/fgnn.h: every (activation, delta) buffer is written in full, node_in's zero column too
            h.assert_written(h.payload(rec), f"{name} {nm} (buffer #{rec.order})")
    _unchanged(t, keep, name)
    tg = R.Graph(code(name))
    tw = [torch.from_numpy(a).to(R.DT).requires_grad_(True) for a in w]
    args = (torch.from_numpy(llr).to(R.DT), torch.from_numpy(lhx).to(R.DT), torch.from_numpy(lhz).to(R.DT), sx.cpu(), sz.cpu())
    if cfg is None:
        out = R.feedback_gnn(tg, tw, *args)
    else:
        out = R.feedback_gnn_general(tg, (cfg[0], cfg[1], cfg[2], REDUCE_OPS[cfg[3]], ACTIVATIONS[cfg[4]], cfg[5]), tw, *args)
    (out * torch.from_numpy(gout).to(R.DT)).sum().backward()
    assert len(grads) == len(tw)
    for i, (got, ref) in enumerate(zip(grads, tw)):
        assert tuple(got.shape) == tuple(ref.shape), i
        err = _rel(got.cpu().numpy(), ref.grad.numpy())
        print(f"{name} array {i}: rel err {err:.2e}")
        assert err < tol, (i, err)


@pytest.mark.parametrize("case,generic", [("gb48_small", False), ("rsurf5_deep", False), ("ghp882_survey", False), ("ghp882_survey", True)])
def test_gnn_bp4_forward_tape_and_backward(case, generic):
    """The cases, draws and bound of tests/test_gpu_gnnbp4_backward.py (2e-3 of each gradient's largest entry against float64 autograd,
    the loss to 2e-4) with the tape and the workspace at exactly the reported byte counts, and every element of the tape, the soft
    syndromes and the gradient written."""
    import gnnbp4_reference as R
    from feedback_gnn_amd.gnn import split_flat_grads
    from test_gpu_gnnbp4_backward import CASES, LOSS_TOL, _batch, _check, _full, _reference, _weights
    name, cfg = CASES[case]
    B, T = (2, 3) if name == "ghp882" else (3, 3)
    g = gpu_graph(name)
    ex, ez, sx, sz = _batch(name, B)
    w = _weights(name, cfg)
    W = GnnBp4Weights(w, g.device, config=_full(cfg), graph=g, force_general=True)
    keep = dict(sx=sx.clone(), sz=sz.clone())
    with switched(g, generic=generic), guarded(g) as h:
        tape = h.alloc((g.gnn_bp4_tape_bytes(W, T, B) // 4,), torch.float32, name="tape")
        fwd = g.gnn_bp4_forward_tape(W, sx, sz, T, tape=tape)
        assert len(h.records) == 3 and fwd["tape"].data_ptr() == tape.data_ptr()
        _verify(h, fwd, None, f"{case} forward")
        dec = g.gnn_bp4_decode(W, sx, sz, T)
        assert torch.equal(fwd["x_logit_all"], dec["x_logit_all"]) and torch.equal(fwd["z_logit_all"], dec["z_logit_all"])
        gx, gz = R.labels(code(name), ex.cpu().numpy(), ez.cpu().numpy())
        xl, zl = fwd["x_logit_all"].clone().requires_grad_(True), fwd["z_logit_all"].clone().requires_grad_(True)
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        loss = sum(bce(xl[i], to_gpu(gx).to(torch.float32)) + bce(zl[i], to_gpu(gz).to(torch.float32)) for i in range(T))
        loss.backward()
        tape_before, first = tape.clone(), len(h.records)
        grads_in = dict(grad_x_logit_all=xl.grad, grad_z_logit_all=zl.grad)
        grads_kept = {k: v.clone() for k, v in grads_in.items()}
        ws = h.alloc((g.gnn_bp4_backward_workspace_bytes(W, B),), torch.uint8, name="workspace")
        flat = g.gnn_bp4_backward(W, sx, sz, T, tape, xl.grad, zl.grad, workspace=ws)
        assert len(h.records) == first + 2
        _verify(h, dict(grad=flat), None, f"{case} backward")
        assert torch.equal(tape.view(torch.int32), tape_before.view(torch.int32)), "the tape is a read-only input of the reverse pass"
        _unchanged(grads_in, grads_kept, f"{case} backward")
    assert torch.equal(sx, keep["sx"]) and torch.equal(sz, keep["sz"])
    ref_loss, ref = _reference(name, cfg, B, T, 0)
    assert abs(float(loss.detach()) - ref_loss) <= LOSS_TOL * abs(ref_loss)
    _check(split_flat_grads(flat, [a.shape for a in w]), ref)


# ---- OSD ---------------------------------------------------------------------------------------------------------------------------------------
OSD_METHOD = {"osd0": 0, "osd_e": 1, "osd_cs": 2}


@functools.lru_cache(maxsize=None)
def _osd_setup(n):
    from test_gpu_osd_shapes import _graph
    basis, rk = random_sparse_basis(n, max(3, n // 2), seed=n)
    rng = np.random.RandomState(n + 1)
    B = 6
    llr = rng.normal(1.0, 2.5, size=(B, n)).astype(F32)
    llr[:, ::5] = F32(0.75)  # ties in the sort
    err = (rng.uniform(size=(B, n)) < 0.05).astype(np.uint8)
    synd = (err.astype(np.int64) @ basis.T.astype(np.int64) % 2).astype(np.uint8)
    return _graph(basis), binary_oracle(basis), basis, llr, synd


def _osd_case(n, method, order, idx, call, with_chosen=None):
    """`call(g, h, synd, e_hat, llr, index, nact, chosen)` runs one OSD entry point; e_hat and chosen are poisoned, so the samples that
    are not listed must still be poison afterwards and the listed ones fully written."""
    g, og, basis, llr, synd = _osd_setup(n)
    B = llr.shape[0]
    what = f"n={n} {method} order {order} index={idx}"
    idx, nact = ((4, 1), 0) if idx == "none" else (idx, 0 if idx is None else len(idx))  # "none": a list is given and nact = 0
    ids = np.arange(B) if idx is None else np.asarray(idx[:nact], np.int64)
    rest = np.setdiff1d(np.arange(B), ids)
    t, keep = _gpu(dict(llr=llr, synd=synd, **({} if idx is None else dict(index=np.asarray(idx, np.int32)))))
    with guarded(g) as h:
        e = h.alloc((B, n), torch.uint8, name="e_hat")
        with_chosen = method != "osd0" if with_chosen is None else with_chosen  # fgnn_osd0 has no such output, fgnn_osd_ws always
        chosen = h.alloc((B,), torch.int32, name="chosen") if with_chosen else None
        call(g, h, t["synd"], e, t["llr"], t.get("index"), nact, chosen)
        h.check()
        h.assert_written(e[to_gpu(ids)], f"{what}: e_hat of the listed samples")
        h.assert_untouched(e[to_gpu(rest)], f"{what}: e_hat of the samples that are not listed")
        if chosen is not None:
            h.assert_written(chosen[to_gpu(ids)], f"{what}: chosen of the listed samples")
            h.assert_untouched(chosen[to_gpu(rest)], f"{what}: chosen of the samples that are not listed")
        got = e.cpu().numpy()
        if not len(ids):
            return _unchanged(t, keep, what)
        if method == "osd0":
            ref = og.osd0(0, np.arange(basis.shape[0], dtype=np.int32), synd, llr_bin=llr, index=None if idx is None else np.asarray(idx, np.int32))
            assert chosen is None or not chosen.cpu().numpy()[ids].any(), f"{what}: chosen of an OSD-0 sample is 0"
        else:
            ref, rc = osd_search_batch(llr, basis, synd, OSD_METHOD[method], order, ids)
            assert np.array_equal(chosen.cpu().numpy()[ids], rc[ids]), what
        assert np.array_equal(got[ids], ref[ids]), f"{what}: {_diff(got[ids], ref[ids])}"
    _unchanged(t, keep, what)


OSD_N = [13, 33, 65]
OSD_INDEX = [None, (4, 1), "none"]  # the OSD entry points refuse B = 0 (a NULL buffer): an empty list is their empty batch


@pytest.mark.parametrize("idx", OSD_INDEX, ids=["all", "listed", "none-listed"])
@pytest.mark.parametrize("n", OSD_N)
def test_osd0(n, idx):
    _osd_case(n, "osd0", 0, idx, lambda g, h, synd, e, llr, index, nact, chosen: g.osd0(0, synd, e, llr_bin=llr, index=index, nact=nact))


@pytest.mark.parametrize("idx", OSD_INDEX, ids=["all", "listed", "none-listed"])
@pytest.mark.parametrize("method,order", [("osd_e", 3), ("osd_cs", 5)])
@pytest.mark.parametrize("n", OSD_N)
def test_osd(n, method, order, idx):
    _osd_case(n, method, order, idx,
              lambda g, h, synd, e, llr, index, nact, chosen: g.osd(0, synd, e, method, order, llr_bin=llr, index=index, nact=nact, chosen=chosen))


@pytest.mark.parametrize("idx", OSD_INDEX, ids=["all", "listed", "none-listed"])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", ["rsurf5", "gb48"])
def test_osd0_on_quaternary_marginals(name, side, idx):
    """The `marg` [B,3,n] input of the BP4 + OSD models on a code's own graph, both sides (the parity test's reference: og.osd0)."""
    c, g, og = code(name), gpu_graph(name), oracle_library_forms(name)
    pivots = (c.pivot_hx, c.pivot_hz)
    g.set_basis(0, c.pivot_hx)
    g.set_basis(1, c.pivot_hz)
    _, _, sx, sz = _noisy(name)
    B = bmax(name)
    marg = og.bp4_decode(sx, sz, 3, "minsum", 0.8, llr_const=llr_const(P_OF[name]))["llr"]
    synd = (sx, sz)[side]
    what = f"{name} side {side} index={idx}"
    idx, nact = ((4, 1), 0) if idx == "none" else (idx, 0 if idx is None else len(idx))
    ids = np.arange(B) if idx is None else np.asarray(idx[:nact], np.int64)
    rest = np.setdiff1d(np.arange(B), ids)
    t, keep = _gpu(dict(marg=marg, synd=synd, **({} if idx is None else dict(index=np.asarray(idx, np.int32)))))
    with guarded(g) as h:
        e = h.alloc((B, g.n), torch.uint8, name="e_hat")
        g.osd0(side, t["synd"], e, marg=t["marg"], index=t.get("index"), nact=nact)
        h.check()
        h.assert_written(e[to_gpu(ids)], f"{what}: e_hat of the listed samples")
        h.assert_untouched(e[to_gpu(rest)], f"{what}: e_hat of the samples that are not listed")
        ref = og.osd0(side, pivots[side], synd, marg=marg, index=None if idx is None else np.asarray(idx[:nact], np.int32))
        got = e.cpu().numpy()
        assert not len(ids) or np.array_equal(got[ids], ref[ids]), f"{what}: {_diff(got[ids], ref[ids])}"
    _unchanged(t, keep, what)


@pytest.mark.parametrize("slots", [1, None], ids=["one-slot", "default-slots"])
@pytest.mark.parametrize("idx", OSD_INDEX, ids=["all", "listed", "none-listed"])
@pytest.mark.parametrize("method,order", [("osd0", 0), ("osd_e", 3), ("osd_cs", 5)])
@pytest.mark.parametrize("n", OSD_N)
def test_osd_ws(n, method, order, idx, slots):
    """The workspace form on a caller workspace of exactly one slot (every sample walks through the same slot) and on the default
    slot count; the workspace is scratch, so only its guards are checked.  `chosen` is written for the processed samples under every
    method, 0 under "osd0"."""
    def call(g, h, synd, e, llr, index, nact, chosen):
        if slots == 1:
            ws = h.alloc((g.osd_slot_bytes(0, method, order),), torch.uint8, name="workspace")
        else:
            ws = g.osd_workspace(0, method, order)  # through the allocator
            assert ws.numel() == g.osd_default_slots(0, method, order) * g.osd_slot_bytes(0, method, order)
        g.osd_ws(0, synd, e, method, order, llr_bin=llr, index=index, nact=nact, chosen=chosen, workspace=ws)
        assert len(h.records) == 3
    _osd_case(n, method, order, idx, call, with_chosen=True)

