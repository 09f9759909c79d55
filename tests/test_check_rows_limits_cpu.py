"""The packed per-check rows at the top of their 16-bit range and on both sides of the limits that switch them off, without a GPU.

fgnn_graph_create uploads `cslot16` / `cslot32` (the byte offsets 4 * slot of a check's message slots) when every degree is uniform,
dc <= 8 and 4 E < 65 536, and `cvn16` (a check's qubits) when dc is uniform, dc <= 8 and n < 65 536.  The zoo's largest regular code
stops at offset 30 476 and qubit 1269; the synthetic codes of tests/helpers.py go on from there.  For each of them fgnn_check_rows (the
upload's own code, run on the host) is compared byte for byte with the NumPy construction of tests/test_check_rows_cpu.py, the `have`
flags and the largest entries are the ones the code was built to reach, and a table the graph does not carry is not written.
tests/test_gpu_packed_row_limits.py runs the kernels that read these rows on the same codes."""
import time

import numpy as np
import pytest

from helpers import EXTRA_CODE_MAKERS, bb_blocks, code, gb_blocks
from test_check_rows_cpu import _library, _tables

# name: (dv_x, dv_z, dc), n, 4 E, have = [slot rows, qubit rows], the largest slot offset (None: no slot rows)
EXPECT = {
    "bb1800": ((3, 3, 6), 1800, 43200, [1, 1], 43196),
    "bb2730": ((3, 3, 6), 2730, 65520, [1, 1], 65516),
    "bb2738": ((3, 3, 6), 2738, 65712, [0, 1], None),
    "gb2000": ((4, 4, 8), 2000, 64000, [1, 1], 63996),
    "gb2048": ((4, 4, 8), 2048, 65536, [0, 1], None),
    "side0_36": ((3, 1, 6), 3528, 56448, [1, 1], 56444),
    "side0_48": ((4, 1, 8), 3200, 64000, [1, 1], 63996),
    "side0_36_over": ((3, 1, 6), 4608, 73728, [0, 1], None),
    "wide65535": ((0, 0, 8), 65535, 1024, [0, 1], None),
    "wide65536": ((0, 0, 8), 65536, 1024, [0, 0], None),
}
# the largest offset of a side-0 slot (the first m_x rows: all that the binary decoders read)
SIDE0_MAX = {"side0_36": 42332, "side0_48": 51196}


def _uniform(d):
    return int(d[0]) if (d == d[0]).all() else 0


def test_every_synthetic_code_is_listed():
    assert set(EXPECT) == set(EXTRA_CODE_MAKERS) - {"hp_big"}


@pytest.mark.parametrize("name", list(EXPECT))
def test_rows_at_the_limits(name):
    degrees, n, four_e, want_have, max_slot = EXPECT[name]
    t0 = time.process_time()
    c = EXTRA_CODE_MAKERS[name]()
    built = time.process_time() - t0
    hx, hz = c.hx, c.hz
    assert hx.dtype == np.uint8 and hz.dtype == np.uint8 and hx.shape[1] == hz.shape[1] == n
    assert (_uniform(hx.sum(0)), _uniform(hz.sum(0)), _uniform(np.r_[hx.sum(1), hz.sum(1)])) == degrees
    assert 4 * (int(hx.sum()) + int(hz.sum())) == four_e
    for perp in (c.hx_perp, c.hz_perp, c.lx, c.lz):
        assert perp.shape == (1, n) and not perp.any()
    have, slot, qub = _library(hx, hz)
    assert have == want_have
    want_slot, want_qub = _tables(hx, hz)
    if have[0]:
        assert slot.tobytes() == want_slot.tobytes()
        assert int(slot.max()) == max_slot == four_e - 4 and (slot % 4 == 0).all()
        assert max_slot >= 32768, "the code must reach the upper half of the 16-bit range"
        if name in SIDE0_MAX:
            assert int(slot[:hx.shape[0]].max()) == SIDE0_MAX[name] >= 32768
    else:
        assert four_e >= 65536 or 0 in degrees[:2]
        assert (slot == 0xDEADBEEF).all()  # nothing is written for a table the graph does not carry
    if have[1]:
        assert qub.tobytes() == want_qub.tobytes()
        assert int(qub.max()) == n - 1
    else:
        assert n >= 65536 and (qub == 0xBEEF).all()
    print(f"{name}: built in {built * 1e3:.1f} ms")
    assert built < 1.0, "the synthetic codes are index arithmetic: well under a second of CPU time"


def test_the_wide_rows_lie_half_in_the_upper_half():
    for name in ("wide65535", "wide65536"):
        c = code(name)
        n = c.hx.shape[1]
        for h in (c.hx, c.hz):
            assert h.shape == (16, n) and (h.sum(1) == 8).all() and h[:, n - 1].any()
            assert h[:, 32768:].sum() == h.sum() // 2


def test_the_constructions_are_the_zoo_s_at_the_zoo_s_sizes():
    """The index arithmetic gives ibm72 at l, m = 6, 6 and gb48 at l = 24: the synthetic codes are larger members of those families."""
    A, B = bb_blocks(6, 6)
    ibm = code("ibm72")
    assert np.array_equal(np.hstack([A, B]), np.asarray(ibm.hx)) and np.array_equal(np.hstack([B.T, A.T]), np.asarray(ibm.hz))
    A, B = gb_blocks(24)
    gb = code("gb48")
    assert np.array_equal(np.hstack([A, B]), np.asarray(gb.hx)) and np.array_equal(np.hstack([B.T, A.T]), np.asarray(gb.hz))
