"""`TannerGraph.gdg_decode` (fgnn_gdg_decode: gdg_kernel<DV, DC> and gdg_select_kernel) inside the guarded, poisoned allocator of
tests/guarded.py, in the frame of tests/test_gpu_guard_bands.py: every buffer of a call — hard_out, stats, path_stats and the
workspace — lies between two 64 KiB guards and starts out as 0xFF bytes, and each case asserts

  (a) both guards of every buffer of the call are intact,
  (b) no poison is left in the rows include/fgnn.h says are written — all of hard_out, stats and path_stats without an index list, the
      rows of the listed samples with one — and the rows of the samples that are not listed still are poison, every byte,
  (c) the payload equals the NumPy restatement tests/gdg_reference.py, `==`,

and that the read-only inputs (syndrome, llr_ch, index) are what they were.  The workspace is scratch: its guards are checked, and
that the kernels stored every byte of it that the selection reads (result words and decision rows of all nact * P paths).

Kernels reached: the (3,6) and (4,8) rows (ibm72, gb48), the predicated runtime-degree kernel (the irregular codes, gb126,
force_generic), set_launch(2, 32) and (64, 4); a tree of depth 2, so that the paths of a sample share a workgroup on the packing
codes and the last workgroup is partly filled; batches 0, 1, 3 and one more than a workgroup holds."""
import numpy as np
import pytest
import torch

import gdg_reference as G
from guarded import guarded
from helpers import code, gpu_graph
from test_gpu_guard_bands import BP4_VARIANTS, SMALL, _gpu, _hx_syndromes, _unchanged, _verify, batches, bmax, switched

pytestmark = pytest.mark.gpu

F32 = np.float32
DEPTH, ITERS = 2, (3, 2, 3)   # pre_iter, round_iter, max_rounds
CASES = [(n, "default") for n in SMALL] + [("ibm72", "generic"), ("gb48", "generic"), ("rsurf5", "launch-2x32"), ("ibm72", "launch-64x4")]


def _workspace(h, paths):
    """The two areas of the workspace of a call with `paths` = nact * P paths (the third buffer the call allocated): the result
    words as int32, whose poison is -1 in a word, and the decision rows as bytes."""
    ws = h.payload(h.records[2])
    if paths == 0:
        return {}
    return dict(workspace_results=ws[:16 * paths].view(torch.int32), workspace_decisions=ws[16 * paths:])


def _llr(name):
    """Per-bit logits [bmax, n]: mostly 'no error', some positive, zeros and values beyond the clip."""
    g = gpu_graph(name)
    rng = np.random.RandomState(3)
    llr = -rng.uniform(-1.0, 5.0, size=(bmax(name), g.n)).astype(F32)
    special = rng.rand(*llr.shape) < 0.05
    llr[special] = rng.choice(np.array([0.0, -20.0, -25.0, 3.0], F32), size=int(special.sum()))
    return llr


@pytest.mark.parametrize("tail", ["least", "most"])
@pytest.mark.parametrize("name,variant", CASES)
def test_gdg_decode(name, variant, tail):
    g = gpu_graph(name)
    hx = np.asarray(code(name).hx)
    synd, llr = _hx_syndromes(name, bmax(name)), _llr(name)
    h0, s0, p0 = G.gdg_decode(hx, synd, *ITERS, DEPTH, tail, 25.0, 0.8, llr_ch=llr)
    for B in batches(name):
        t, keep = _gpu(dict(synd=synd[:B], llr_ch=llr[:B]))
        what = f"{name} {variant} {tail} B={B}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            hard, stats, ps = g.gdg_decode(t["synd"], *ITERS, DEPTH, tail, 25.0, 0.8, llr_ch=t["llr_ch"], want_path_stats=True)
            assert [r.shape for r in h.records] == [(B, g.n), (B, 4), (max(B * 4 * (16 + g.n), 1),), (B, 4, 4)]
            _verify(h, dict(hard=hard, stats=stats, path_stats=ps, **(_workspace(h, B * 4) if B else {})),
                    dict(hard=h0[:B], stats=s0[:B], path_stats=p0[:B]) if B else None, what)
        _unchanged(t, keep, what)


@pytest.mark.parametrize("name,variant", [("rsurf5", "default"), ("gb48", "default"), ("gb126", "default"), ("ibm72", "generic"),
                                          ("rsurf5", "launch-2x32")])
def test_gdg_decode_on_an_index_list(name, variant):
    """A permuted subset, a list of one and a list of none: the rows of the listed samples are written in full, every other row of
    hard_out and stats stays poison, path_stats holds the listed samples in list order."""
    g = gpu_graph(name)
    hx = np.asarray(code(name).hx)
    B = bmax(name)
    synd, llr = _hx_syndromes(name, B), _llr(name)
    h0, s0, p0 = G.gdg_decode(hx, synd, *ITERS, DEPTH, "least", 25.0, 0.8, llr_ch=llr)
    perm = [int(i) for i in np.random.RandomState(B).permutation(B)[:max(1, B // 2)]]
    for listed, nact in ((perm, None), (perm, 1), (perm, 0)):
        take = listed if nact is None else listed[:nact]
        rest = sorted(set(range(B)) - set(take))
        t, keep = _gpu(dict(synd=synd, llr_ch=llr, index=np.asarray(listed, np.int32)))
        what = f"{name} {variant} index={take}"
        with switched(g, **BP4_VARIANTS[variant]), guarded(g) as h:
            hard, stats = h.alloc((B, g.n), torch.uint8, "hard"), h.alloc((B, 4), torch.int32, "stats")
            out = g.gdg_decode(t["synd"], *ITERS, DEPTH, "least", 25.0, 0.8, llr_ch=t["llr_ch"], index=t["index"], nact=nact,
                               out=(hard, stats), want_path_stats=True)
            assert out[0] is hard and out[1] is stats
            assert [r.shape for r in h.records[2:]] == [(max(len(take) * 4 * (16 + g.n), 1),), (len(take), 4, 4)]
            ws = _workspace(h, len(take) * 4)
            h.check()
            for k, v in (("hard", hard), ("stats", stats)):
                h.assert_written(v[take], f"{what} {k} of the listed samples")
                h.assert_untouched(v[rest], f"{what} {k} of the other samples")
            h.assert_written(out[2], f"{what} path_stats")
            for k, v in ws.items():
                h.assert_written(v, f"{what} {k}")
            if not take:
                h.assert_untouched(h.payload(h.records[2]), f"{what} workspace")
            assert np.array_equal(hard[take].cpu().numpy(), h0[take]) and np.array_equal(stats[take].cpu().numpy(), s0[take]), what
            assert np.array_equal(out[2].cpu().numpy(), p0[take]), what
        _unchanged(t, keep, what)
