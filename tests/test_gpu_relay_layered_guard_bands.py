"""`TannerGraph.relay_decode_layered` (fgnn_relay_decode_layered: relay_layered_kernel<DV, DC>) inside the guarded, poisoned allocator of
tests/guarded.py, in the frame of tests/test_gpu_guard_bands.py: hard_out and stats each lie between two 64 KiB guards and start out as
0xFF bytes, and each case asserts

  (a) both guards of every buffer of the call are intact,
  (b) no poison is left in what include/fgnn.h says is written — all of hard_out and stats — and the call allocates those two only,
  (c) the payload equals the NumPy restatement tests/relay_layered_reference.py, `==`,

and that the read-only inputs (syndrome, gamma, llr_ch) are what they were.

Kernels reached: the (3,6) and (4,8) rows (ibm72, gb48), the predicated min-sum for degrees up to 8 (steane, the surface codes,
force_generic) and up to 16 (gb126), the loop (irr_30), set_launch(2, 32) and (64, 4); batches 0, 1, 3 and one more than a workgroup
holds; a constant logit and per-bit logits.  The schedule is (3, 2 x 2) with stop_nconv = 2: a codeword may write hard_out in more
than one leg."""
import numpy as np
import pytest

import relay_layered_reference as RL
from guarded import guarded
from helpers import code, gpu_graph
from test_gpu_bp2_shapes import CASES, graphs
from test_gpu_guard_bands import BP4_VARIANTS, SMALL, _gpu, _hx_syndromes, _unchanged, _verify, batches, bmax, switched
from test_relay_reference_cpu import mixed_gamma

pytestmark = pytest.mark.gpu

F32 = np.float32
PRE, LEG, LEGS, STOP = 3, 2, 3, 2
INSTANCES = [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("gb48", "generic"), ("rsurf5", "launch-2x32"), ("ibm72", "launch-64x4")]


def _llr(B, n):
    """Per-bit logits [B, n]: mostly 'no error', some positive, zeros and values beyond the clip."""
    rng = np.random.RandomState(3)
    llr = -rng.uniform(-1.0, 5.0, size=(B, n)).astype(F32)
    special = rng.rand(*llr.shape) < 0.05
    llr[special] = rng.choice(np.array([0.0, -20.0, -25.0, 3.0], F32), size=int(special.sum()))
    return llr


def _case(g, hx, synd, Bs, variant, what, per_bit):
    n = g.n
    gamma = mixed_gamma(LEGS, n, 3)
    kw = dict(llr_ch=_llr(len(synd), n)) if per_bit else dict(llr_const=-1.7)
    h0, s0, _ = RL.relay_layered_decode(hx, synd, gamma, PRE, LEG, STOP, 0.8, **kw)
    for B in Bs:
        ins = dict(synd=synd[:B], gamma=gamma)
        if per_bit:
            ins["llr_ch"] = kw["llr_ch"][:B]
        t, keep = _gpu(ins)
        llr = dict(llr_ch=t["llr_ch"]) if per_bit else kw
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            hard, stats = g.relay_decode_layered(t["synd"], t["gamma"], PRE, LEG, STOP, 0.8, **llr)
            assert [(r.shape, r.dtype) for r in h.records] == [((B, n), hard.dtype), ((B, 4), stats.dtype)]
            _verify(h, dict(hard=hard, stats=stats), dict(hard=h0[:B], stats=s0[:B]) if B else None, f"{what} B={B}")
        _unchanged(t, keep, f"{what} B={B}")


@pytest.mark.parametrize("per_bit", [False, True], ids=["const", "llr_ch"])
@pytest.mark.parametrize("name,variant", INSTANCES)
def test_relay_decode_layered(name, variant, per_bit):
    g = gpu_graph(name)
    g.set_bit_layers()
    _case(g, np.asarray(code(name).hx), _hx_syndromes(name, bmax(name)), batches(name), variant, f"{name} {variant}", per_bit)


@pytest.mark.parametrize("per_bit", [False, True], ids=["const", "llr_ch"])
def test_relay_decode_layered_on_the_loop(per_bit):
    """Check degrees up to 30: relay_layered_kernel<0, 0>."""
    g, _, hx = graphs("irr_30", dict(CASES)["irr_30"])
    assert int(hx.sum(1).max()) > 16
    g.set_bit_layers()
    cpb = g.info()["codewords_per_block"]
    Bs = sorted({0, 1, 3, cpb + 1})
    e = (np.random.RandomState(5).rand(max(Bs), hx.shape[1]) < 0.06).astype(np.int64)
    synd = (e @ np.asarray(hx, np.int64).T % 2).astype(np.uint8)
    _case(g, hx, synd, Bs, "default", "irr_30", per_bit)
