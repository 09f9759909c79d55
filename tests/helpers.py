"""Shared helpers for the test-suite: code zoo, golden fixtures, oracle/GPU graph caches."""
import functools
import os

import numpy as np

from feedback_gnn_amd import codes_q as cq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CODE_MAKERS = {
    "steane": lambda: cq.css_code(cq.hamming_code(3), cq.hamming_code(3), name="Steane_n7_k1_d3"),
    "rsurf3": lambda: cq.create_rotated_surface_codes(3),
    "rsurf5": lambda: cq.create_rotated_surface_codes(5),
    "surf3": lambda: cq.create_surface_codes(3),
    "toric4": lambda: cq.create_checkerboard_toric_codes(4),
    "gb48": lambda: cq.create_generalized_bicycle_codes(24, [0, 2, 8, 15], [0, 2, 12, 17], name="GB_n48_k6_d8"),
    "gb126": lambda: cq.create_generalized_bicycle_codes(63, [0, 1, 14, 16, 22], [0, 3, 13, 20, 42]),
    "gb254": lambda: cq.create_generalized_bicycle_codes(127, [0, 15, 20, 28, 66], [0, 58, 59, 100, 121]),
    "hp_c7": lambda: cq.hypergraph_product(cq.create_circulant_matrix(7, [0, 1, 3]), cq.create_circulant_matrix(7, [0, 1, 3])),
    "ibm72": lambda: cq.create_bivariate_QC_codes(6, 6, [3], [1, 2], [1, 2], [3]),
    "ghp882": lambda: cq.create_QC_GHP_codes(63, cq.create_cyclic_permuting_matrix(7, [27, 54, 0]), [0, 1, 6]),
    "ghp1270": lambda: cq.create_QC_GHP_codes(
        127, np.array([[0, -1, 51, 52, -1], [-1, 0, -1, 111, 20], [0, -1, 98, -1, 122], [0, 80, -1, 119, -1],
                       [-1, 0, 5, -1, 106]]), [0, 1, 7], name="GHP_n1270_k28"),
}



def _overcomplete(key):
    """The reference's over-complete GB check matrices (A-list data files, QLDPC.ipynb cell 5) from tests/golden/overcomplete.npz."""
    g = np.load(os.path.join(GOLDEN, "overcomplete.npz"))
    return cq.css_code(hx=unpack(g, key, "hx").astype(int), hz=unpack(g, key, "hz").astype(int), name=None, name_prefix="GB")


def _hp_big():
    """A hypergraph product too large for a CU's LDS: [[6480, 1296]] from a seeded (3,6)-like 36 x 72 matrix — 45 576 edges, so the BP4
    state of one codeword (E + 3n = 65 016 floats = 254 KB) takes the library's global-memory variant of the runtime-degree kernel."""
    rng = np.random.RandomState(7)
    m, n, dv = 36, 72, 3
    per = dv * n // m // dv
    h = np.zeros((m, n), dtype=int)
    for _ in range(dv):
        perm = rng.permutation(n)
        for r in range(m):
            h[r, perm[r * per:(r + 1) * per]] = 1
    return cq.hypergraph_product(h, h, "HP_n6480_lds_overflow")


def _bare_code(hx, hz):
    """A code object carrying only what TannerGraph / OracleGraph read (the wrapping of `binary_oracle`): dense uint8 hx and hz and one
    all-zero row each for hx_perp, hz_perp, lx and lz.  No GF(2) rank work: the logical rows are not what these codes test."""
    import types
    hx, hz = np.ascontiguousarray(hx, dtype=np.uint8), np.ascontiguousarray(hz, dtype=np.uint8)
    zero = np.zeros((1, hx.shape[1]), np.uint8)
    return types.SimpleNamespace(hx=hx, hz=hz, hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)


def _shift_sum(l, m, x_pows, y_pows):
    """The sum of the monomials x^e (e in x_pows) and y^e (e in y_pows) on Z_l x Z_m as a dense uint8 [l m, l m] matrix, in the
    convention of codes_q.create_bivariate_QC_codes (x = S_l (x) I_m, y = I_l (x) S_m, column i m + j <-> (i, j)): x^e has its ones at
    (((i - e) mod l) m + j, i m + j), y^e at (i m + (j - e) mod m, i m + j).  m = 1 gives an l x l circulant with the ones of
    codes_q.create_circulant_matrix(l, [-e, ...])."""
    i, j = np.divmod(np.arange(l * m), m)
    h = np.zeros((l * m, l * m), np.uint8)
    for e in x_pows:
        h[((i - e) % l) * m + j, i * m + j] ^= 1
    for e in y_pows:
        h[i * m + (j - e) % m, i * m + j] ^= 1
    return h


def bb_blocks(l, m):
    """(A, B) of the bivariate-bicycle construction with ibm72's polynomials, A = x^3 + y + y^2 and B = y^3 + x + x^2, on Z_l x Z_m:
    [A | B] is (3,6)-regular for l, m >= 4."""
    return _shift_sum(l, m, [3], [1, 2]), _shift_sum(l, m, [1, 2], [3])


def gb_blocks(l):
    """(A, B) of the generalized-bicycle construction with gb48's exponents [0,2,8,15] and [0,2,12,17] as circulants of size l
    (ones at (i + c mod l, i), codes_q.create_circulant_matrix): [A | B] is (4,8)-regular."""
    return _shift_sum(l, 1, [0, -2, -8, -15], []), _shift_sum(l, 1, [0, -2, -12, -17], [])


def _bicycle(A, B):
    """hx = [A | B], hz = [B^T | A^T]."""
    return _bare_code(np.hstack([A, B]), np.hstack([B.T, A.T]))


def _side0(A, B):
    """A graph for the binary decoders, which read side 0 only: hx = [A | B] and hz = n / dc rows of dc consecutive qubits (dv_z = 1,
    the same check degree), so every degree is uniform and the packed rows exist while hx's offsets alone pass 2^15.  hz does not
    commute with hx: this is no CSS code, and nothing here decodes side 1."""
    hx = np.hstack([A, B])
    n, dc = hx.shape[1], int(hx[0].sum())
    assert n % dc == 0
    hz = np.zeros((n // dc, n), np.uint8)
    hz[np.arange(n) // dc, np.arange(n)] = 1
    return _bare_code(hx, hz)


def _wide_rows(n):
    """16 hx and 16 hz checks of 8 distinct qubits each on n qubits (n = 65 535 / 65 536): entry j of a row lies near j n / 8, so
    entries 4..7 — half of them — lie in [32 768, n), and the last entry of hx row 15 and of hz row 0 is qubit n - 1.  Most qubits
    have no edge, so the qubit degrees are not uniform: no slot rows, and qubit rows exactly when n < 65 536."""
    r, j = np.arange(16)[:, None], np.arange(8)[None, :]
    qx = j * (n // 8) + 257 * r + 31 * j
    qz = j * (n // 8) + 263 * r + 37 * j + 2000
    qx[15, 7] = qz[0, 7] = n - 1
    assert qx.max() == qz.max() == n - 1 and all(len(set(row)) == 8 for q in (qx, qz) for row in q.tolist())
    hx, hz = np.zeros((16, n), np.uint8), np.zeros((16, n), np.uint8)
    hx[r, qx] = 1
    hz[r, qz] = 1
    return _bare_code(hx, hz)


# not one of the reference's constructions with a fixture under tests/golden (tests/test_codes.py walks CODE_MAKERS): its own table.
# The synthetic regular codes carry the packed 16-bit check rows (fgnn_graph.hip) through the upper half of their range and across
# both of their limits, 4 E < 65 536 for the slot offsets and n < 65 536 for the qubits; they are built from index arithmetic in
# milliseconds (tests/test_check_rows_limits_cpu.py states what each one reaches)
EXTRA_CODE_MAKERS = {
    "hp_big": _hp_big,
    # (3,3,6)-regular bivariate bicycle, n = 2 l m, 4 E = 24 n: offsets up to 43 196 / up to 65 516, the last code with slot rows /
    # 4 E = 65 712, the first without them (the qubit rows stay)
    "bb1800": lambda: _bicycle(*bb_blocks(30, 30)),
    "bb2730": lambda: _bicycle(*bb_blocks(35, 39)),
    "bb2738": lambda: _bicycle(*bb_blocks(37, 37)),
    # (4,4,8)-regular generalized bicycle, n = 2 l, 4 E = 64 l: offsets up to 63 996 / 4 E = 65 536, the first without slot rows
    "gb2000": lambda: _bicycle(*gb_blocks(1000)),
    "gb2048": lambda: _bicycle(*gb_blocks(1024)),
    # side 0 of the binary decoders: (3,6) with 4 E_x = 42 336 of 4 E = 56 448, (4,8) with 4 E_x = 51 200 of 4 E = 64 000, and (3,6)
    # past the limit (4 E = 73 728)
    "side0_36": lambda: _side0(*bb_blocks(42, 42)),
    "side0_48": lambda: _side0(*gb_blocks(1600)),
    "side0_36_over": lambda: _side0(*bb_blocks(48, 48)),
    # qubit rows near 2^16: present at n = 65 535 (qubit 65 534 is read), absent at n = 65 536
    "wide65535": lambda: _wide_rows(65535),
    "wide65536": lambda: _wide_rows(65536),
}
CODE_MAKERS["gb46_oc"] = lambda: _overcomplete("gb46_oc")
CODE_MAKERS["gb48_oc"] = lambda: _overcomplete("gb48_oc")

WEIGHTS_882 = "feedback_GNN_n882_k24_wt_4_60_iter_64_16_mixed.npz"
WEIGHTS_1270 = "feedback_GNN_n1270_k28_wt_10_80_iter_64_16_mixed.npz"


@functools.lru_cache(maxsize=None)
def code(name):
    return (CODE_MAKERS.get(name) or EXTRA_CODE_MAKERS[name])()


@functools.lru_cache(maxsize=None)
def _oracle_graph(name, stage_one, forms):
    from oracle.oracle import OracleGraph
    return OracleGraph(code(name), stage_one=stage_one, forms=forms)


def oracle_library_forms(name, stage_one=True):
    """The checker of the default parity tests: the oracle's restatement of the operation sequence libfgnn_hip runs BY DEFAULT — what
    `gpu_graph(name)` computes out of the box.  Since round 6 that is the reference's formulas term by term (FGNN_OPT_GNN_FACTORED =
    FGNN_OPT_BP4_SHARED_LSE = 0: one Dense per edge, one log-sum-exp per edge), i.e. the same restatement as `oracle_literal_forms`;
    the two opt-in re-associations are `oracle_reassociated_forms`, and tests/test_gpu_bp4_shared_lse.py, test_gpu_gnn_order.py and
    test_gpu_literal_forms.py hold the kernels to the oracle with the options on and off.  One cached graph per (code, stage_one);
    tests that flip a form with its setters restore it (LIBRARY_FORMS below)."""
    return _oracle_graph(name, stage_one, "library-default")


def oracle_literal_forms(name, stage_one=True):
    """The oracle's restatement of the reference's formulas term by term: one log-sum-exp per edge (decoding_q.py:254-273), one Dense per
    edge (feedback_gnn.py:175-184, gnn.py:573-610)."""
    return _oracle_graph(name, stage_one, "literal")


def oracle_reassociated_forms(name, stage_one=True):
    """The oracle's restatement of the library's two opt-in re-associations (Dense layers factored, the log-sum-exp term shared per qubit
    side): the checker of a GPU graph with `set_gnn_factored(True)` and `set_bp4_shared_lse(True)`."""
    return _oracle_graph(name, stage_one, "reassociated")


# what a fresh TannerGraph / OracleGraph(forms="library-default") runs: tests that switch a form restore these values
LIBRARY_GNN_FACTORED = False
LIBRARY_BP4_SHARED_LSE = False


@functools.lru_cache(maxsize=None)
def gpu_graph(name, stage_one=True):
    from feedback_gnn_amd.graph import TannerGraph
    return TannerGraph(code(name), stage_one=stage_one)


def llr_const(p0):
    """log(3(1-p0)/p0) in float32 arithmetic, feedback_gnn.py:312."""
    p0 = np.float32(p0)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p0) / p0, dtype=np.float32))


def gnnbp4_weights(seed):
    """Seeded GNN_BP4 weights in the shapes of GNNBP4_SHAPES: glorot-uniform kernels, biases uniform in (-0.6, 0.6)."""
    from feedback_gnn_amd.graph import GNNBP4_SHAPES
    rng = np.random.RandomState(seed)
    w = []
    for shp in GNNBP4_SHAPES:
        lim = 0.6 if len(shp) == 1 else np.sqrt(6.0 / (shp[0] + shp[1]))
        w.append(rng.uniform(-lim, lim, size=shp).astype(np.float32))
    return w


# Feedback_GNN constructor settings (num_msg_dims, num_hidden_units, num_mlp_layers, reduce_op, activation, use_bias): the shipped one
# first, then settings only the runtime-shaped kernel takes
GEN_CONFIGS = [(20, 40, 2, "mean", "tanh", True), (8, 16, 1, "max", "relu", False), (12, 24, 3, "sum", "sigmoid", True),
               (5, 7, 2, "min", None, True), (32, 96, 4, "mean", "relu", False)]


def gen_weights(cfg, seed=3):
    """Seeded uniform(-0.5, 0.5) Feedback_GNN weights in the shapes of one constructor setting."""
    from feedback_gnn_amd.graph import gnn_weight_shapes
    rng = np.random.RandomState(seed)
    return [rng.uniform(-0.5, 0.5, size=s).astype(np.float32) for s in gnn_weight_shapes(cfg[0], cfg[1], cfg[2], cfg[5])]


def gen_cfg_codes(cfg):
    """The integer-coded setting `OracleGraph.feedback_gnn_general` takes."""
    from feedback_gnn_amd.graph import ACTIVATIONS, REDUCE_OPS
    return (cfg[0], cfg[1], cfg[2], REDUCE_OPS[cfg[3]], ACTIVATIONS[cfg[4]], int(cfg[5]))


def golden_codes():
    out = dict(np.load(os.path.join(GOLDEN, "codes.npz")))
    out.update(np.load(os.path.join(GOLDEN, "overcomplete.npz")))
    return out


def unpack(g, key, attr):
    sh = g[f"{key}/{attr}_shape"]
    if sh[0] == 0:
        return np.zeros(sh, dtype=np.uint8)
    return np.unpackbits(g[f"{key}/{attr}"], axis=1)[:, :sh[1]]


def to_gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_sparse_basis(n, m, seed, col_weight=3):
    """A seeded random sparse binary matrix [m, n] (uint8) in which every row and every column holds at least one 1 (fgnn_graph_create
    takes no duplicate edges, and an edge-free row or column is no code), with its GF(2) rank: (basis, rank)."""
    from feedback_gnn_amd.gf2 import rank
    rng = np.random.RandomState(seed)
    h = np.zeros((m, n), np.uint8)
    for v in range(n):
        h[rng.choice(m, size=min(col_weight, m), replace=False), v] = 1
    for c in np.nonzero(h.sum(1) == 0)[0]:
        h[c, rng.randint(n)] = 1
    return h, rank(h)


def binary_oracle(basis):
    """The CPU oracle's graph of one binary parity-check matrix on both sides (what decoding._binary_graph builds on the GPU)."""
    import types
    from oracle.oracle import OracleGraph
    pcm = np.asarray(basis).astype(np.int64)
    zero = np.zeros((1, pcm.shape[1]), np.int64)
    c = types.SimpleNamespace(hx=pcm, hz=pcm, hx_perp=zero, hz_perp=zero, lx=zero, lz=zero)
    return OracleGraph(c, stage_one=True, forms="library-default")
