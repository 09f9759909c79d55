"""fgnn_syndrome against dense NumPy (H e mod 2) on seeded random bytes: a check-regular graph reads each check's qubits as one 16-byte
row of g.cvn16 — [[882,24]] and the hypergraph product of two (3,3) circulants with six per check, the GB code with eight — and the CSR
loop is the fallback (fgnn_graph_force_generic).  Batches: one codeword, one workgroup's worth of them, and one more."""
import numpy as np
import pytest

from helpers import code, gpu_graph, to_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("generic", [False, True], ids=["rows", "csr"])
@pytest.mark.parametrize("name", ["ghp882", "hp_c7", "gb48"])
def test_syndrome_equals_dense_numpy(name, generic):
    c, gg = code(name), gpu_graph(name)
    hx, hz = np.asarray(c.hx).astype(np.int64), np.asarray(c.hz).astype(np.int64)
    cpb = gg.info()["codewords_per_block"]
    rng = np.random.RandomState(11)
    try:
        gg.force_generic(generic)
        for B in (1, cpb, cpb + 1):
            ex = (rng.rand(B, gg.n) < 0.3).astype(np.uint8)
            ez = (rng.rand(B, gg.n) < 0.3).astype(np.uint8)
            sx, sz = gg.syndrome(to_gpu(ex), to_gpu(ez))
            # syndrome_x = hx noise_z, syndrome_z = hz noise_x
            assert np.array_equal(sx.cpu().numpy(), (ez.astype(np.int64) @ hx.T % 2).astype(np.uint8)), (name, B, generic)
            assert np.array_equal(sz.cpu().numpy(), (ex.astype(np.int64) @ hz.T % 2).astype(np.uint8)), (name, B, generic)
    finally:
        gg.force_generic(False)
