"""The literal feedback GNN's streaming kernel, whose first edge assigns the qubit's message sum and whose later edges add to it under a
scalar branch, against the C oracle by exact equality: on [[882,24]] (three checks per qubit and side) at 3 codewords with the
streaming kernel forced (by itself it takes launches of 4 096 codewords or more) and on the (4,4,8)-regular GB code (four edges per
side: streaming at every batch size), each with the shipped and with random weights.  Some input
LLRs are +0 and -0."""
import numpy as np
import pytest

from helpers import LIBRARY_GNN_FACTORED, WEIGHTS_882, gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def _inputs(name, B):
    """Syndromes at p = 0.08, the marginals and soft syndromes of an 8-iteration decode of them (the oracle's), zeros of both signs
    sprinkled over the marginals."""
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, 0.08, 40, B)
    sx, sz = og.syndrome(ex, ez)
    o = og.bp4_decode(sx, sz, 8, "boxplus-phi", 1.0, llr_const=llr_const(0.08))
    llr = o["llr"].copy()
    rng = np.random.RandomState(5)
    pick = rng.rand(*llr.shape)
    llr[pick < 0.03] = 0.0
    llr[pick > 0.97] = -0.0
    assert np.signbit(llr[llr == 0]).any() and not np.signbit(llr[llr == 0]).all()
    return llr, o["z_logit"], o["x_logit"], sx, sz


def _weights(kind):
    from feedback_gnn_amd.weights_io import read_weight_list
    w = read_weight_list(WEIGHTS_882)
    if kind == "random":  # no near-zero column hides a wrong element or edge
        rng = np.random.RandomState(9)
        w = [rng.uniform(-0.7, 0.7, size=a.shape).astype(np.float32) for a in w]
    return w


@pytest.mark.parametrize("name,B,stream,kind", [("ghp882", 3, "always", "shipped"), ("ghp882", 3, "always", "random"),
                                                ("gb48", 3, True, "shipped"), ("gb48", 130, True, "random")])
def test_literal_streaming_kernel_equals_the_oracle(name, B, stream, kind):
    from feedback_gnn_amd.graph import GnnWeights
    og, gg = oracle_library_forms(name), gpu_graph(name)
    assert gg.gnn_factored == LIBRARY_GNN_FACTORED is False and gg.info()["dv_x"] == (3 if name == "ghp882" else 4)
    w = _weights(kind)
    args = _inputs(name, B)
    ref = og.feedback_gnn(w, *args)
    try:
        gg.set_gnn_stream(stream)
        out = gg.feedback_gnn(GnnWeights(w, gg.device), *[to_gpu(a) for a in args]).cpu().numpy()
    finally:
        gg.set_gnn_stream(True)
    bad = np.argwhere(ref != out)
    assert ref.tobytes() == out.tobytes(), f"{len(bad)} of {ref.size} differ, first at {bad[:3].tolist()}"
    assert np.isfinite(ref).all()
