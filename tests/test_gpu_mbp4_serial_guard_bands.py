"""fgnn_mbp4_decode_serial behind the guarded, poisoned allocator of tests/guarded.py: no store beside x_hat, z_hat or stats, and no
element of them left unwritten, for every check rule, with several codewords per workgroup and a batch that is no multiple of it,
on a graph with runtime degrees, with and without restart, and for samples that end solved, at a later attempt and unsolved."""
import numpy as np
import pytest

import mbp4_reference as MB
import test_gpu_bp4gd as TGD
from guarded import guarded
from helpers import gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu


def run(g, sx, sz, cn_type, restart, B=None, **kw):
    factors, owns = MB.mbp4_tables((1.0, 0.8, 0.6), 0.8)
    with guarded(g) as guard:
        xh, zh, st = g.mbp4_decode_serial(sx, sz, factors, owns, 3, 2, cn_type, restart=restart, B=B, **kw)
        guard.label(dict(x_hat=xh, z_hat=zh, stats=st))
        guard.check()
        for name, t in (("x_hat", xh), ("z_hat", zh), ("stats", st)):
            guard.assert_written(t, name)
    assert int(xh.max()) <= 1 and int(zh.max()) <= 1 and int(st.min()) >= 0
    return st.cpu().numpy()


@pytest.mark.parametrize("cn_type", TGD.CN_TYPES)
@pytest.mark.parametrize("name,launch,B", [("ibm72", (0, 0), 40), ("ibm72", (32, 4), 37), ("rsurf5", (0, 0), 19), ("ibm72", (1024, 1), 3)])
def test_outputs_are_written_in_full_and_nothing_beside_them(name, launch, B, cn_type):
    g, og = gpu_graph(name), oracle_library_forms(name)
    p = TGD.P_OF[name]
    _, _, sx, sz = TGD.noisy(og, p, B)
    g.set_launch(*launch)
    try:
        kinds = set()
        for restart in (True, False):
            st = run(g, to_gpu(sx), to_gpu(sz), cn_type, restart, llr_const=llr_const(p))
            kinds |= {(int(f), int(a) > 0) for f, a in st[:, :2]}
        if B >= 19:
            assert (1, False) in kinds and ((1, True) in kinds or (0, True) in kinds), "samples ending in attempt 0 and later"
        run(g, None, None, cn_type, True, B=B, llr_const=2.0)  # null syndromes: every sample solved at once
        llr = np.random.RandomState(1).uniform(0.5, 5.0, size=(B, 3, g.n)).astype(np.float32)
        run(g, to_gpu(sx), to_gpu(sz), cn_type, True, llr_ch=to_gpu(llr))
    finally:
        g.set_launch(0, 0)
