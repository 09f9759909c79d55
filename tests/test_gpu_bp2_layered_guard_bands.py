"""`TannerGraph.bp2_decode_layered` (fgnn_bp2_decode_layered: bp2_layered_kernel<CN_TYPE, DV, DC>) inside the guarded, poisoned
allocator of tests/guarded.py, in the frame of tests/test_gpu_guard_bands.py: soft_out, hard_out and stats each lie between two 64 KiB
guards and start out as 0xFF bytes, and each case asserts

  (a) both guards of every buffer of the call are intact,
  (b) no poison is left in what include/fgnn.h says is written — all of soft_out, hard_out and stats — and a call that does not ask
      for stats, soft or hard allocates and hands in no such buffer,
  (c) the payload equals the NumPy restatement tests/bp2_layered_reference.py, `==`,

and that the read-only inputs (syndrome, llr_ch) are what they were.

Kernels reached: the (3,6) and (4,8) rows (ibm72, gb48), the predicated min-sum for degrees up to 8 and 16 (the irregular codes,
gb126, force_generic) and the loop (phi, boxplus), set_launch(2, 32) and (64, 4); with and without stop; batches 0, 1, 3 and one more
than a workgroup holds."""
import numpy as np
import pytest

import bp2_layered_reference as BR
from guarded import guarded
from helpers import code, gpu_graph
from test_gpu_guard_bands import BP4_VARIANTS, SMALL, _gpu, _hx_syndromes, _unchanged, _verify, batches, bmax, switched

pytestmark = pytest.mark.gpu

F32 = np.float32
ITERS = 3
CASES = [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("gb48", "generic"), ("rsurf5", "launch-2x32"), ("ibm72", "launch-64x4")]


def _llr(name):
    """Per-bit logits [bmax, n]: mostly 'no error', some positive, zeros and values beyond the clip."""
    g = gpu_graph(name)
    rng = np.random.RandomState(3)
    llr = -rng.uniform(-1.0, 5.0, size=(bmax(name), g.n)).astype(F32)
    special = rng.rand(*llr.shape) < 0.05
    llr[special] = rng.choice(np.array([0.0, -20.0, -25.0, 3.0], F32), size=int(special.sum()))
    return llr


@pytest.mark.parametrize("cn_type,stop", [("minsum", True), ("minsum", False), ("boxplus-phi", True), ("boxplus", False)])
@pytest.mark.parametrize("name,variant", CASES)
def test_bp2_decode_layered(name, variant, cn_type, stop):
    g = gpu_graph(name)
    hx = np.asarray(code(name).hx)
    synd, llr = _hx_syndromes(name, bmax(name)), _llr(name)
    s0, h0, st0 = BR.bp2_layered_decode(hx, synd, ITERS, cn_type, 0.8, llr_ch=llr, stop=stop)
    for B in batches(name):
        t, keep = _gpu(dict(synd=synd[:B], llr_ch=llr[:B]))
        what = f"{name} {variant} {cn_type} stop={stop} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            soft, hard, stats = g.bp2_decode_layered(t["synd"], ITERS, cn_type, 0.8, llr_ch=t["llr_ch"], stop=stop, want_stats=True)
            assert [(r.shape, r.dtype) for r in h.records] == [((B, g.n), soft.dtype), ((B, g.n), hard.dtype), ((B, 2), stats.dtype)]
            _verify(h, dict(soft=soft, hard=hard, stats=stats), dict(soft=s0[:B], hard=h0[:B], stats=st0[:B]) if B else None, what)
            if B:
                assert soft.cpu().numpy().tobytes() == s0[:B].tobytes(), what  # `==` passes -0.0 for 0.0
        _unchanged(t, keep, what)


@pytest.mark.parametrize("name,variant", [("rsurf5", "default"), ("gb48", "default"), ("gb126", "default"), ("ibm72", "generic"),
                                          ("rsurf5", "launch-2x32")])
def test_only_what_is_asked_for(name, variant):
    """Without stats, soft or hard the call allocates no such buffer and the others are written in full, to the same bytes."""
    g = gpu_graph(name)
    hx = np.asarray(code(name).hx)
    B = bmax(name)
    synd, llr = _hx_syndromes(name, B), _llr(name)
    s0, h0, st0 = BR.bp2_layered_decode(hx, synd, ITERS, "minsum", 0.8, llr_ch=llr, stop=True)
    t, keep = _gpu(dict(synd=synd, llr_ch=llr))
    for kw, want in ((dict(), dict(soft=s0, hard=h0)), (dict(want_hard=False), dict(soft=s0, hard=None)),
                     (dict(want_soft=False, want_stats=True), dict(soft=None, hard=h0, stats=st0))):
        what = f"{name} {variant} {sorted(kw)}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            out = g.bp2_decode_layered(t["synd"], ITERS, "minsum", 0.8, llr_ch=t["llr_ch"], stop=True, **kw)
            assert len(h.records) == sum(v is not None for v in want.values()), what
            _verify(h, dict(zip(("soft", "hard", "stats"), out)), want, what)
        _unchanged(t, keep, what)
