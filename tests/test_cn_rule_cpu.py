"""The check rules of fgnn_cn.h with no extra input, as the kernels of binary BP, BP4 and the step-loop decoders call them: the host
build (tests/cn_rule_check.cpp, plain and under the address and undefined-behaviour sanitizers) against `mbp4_reference.cn_update`,
bit for bit.  The rows with one and two extra inputs are in test_dsbp4_reference_cpu.py and test_stbp4_reference_cpu.py.  CPU only."""
import functools

import numpy as np
import pytest

import mbp4_reference as MB
from test_dsbp4_reference_cpu import bits, run_cn_rule_check
from test_stbp4_reference_cpu import DMAX, HEAD, rule_rows as st_rule_rows

F32 = np.float32
CN_TYPES = ["boxplus", "boxplus-phi", "minsum"]


def rule_rows(cn_type):
    """The row table of the space-time test with the number of extras set to 0 (the two extra values stay in the rows and must not
    be read).  The boxplus rows are drawn without subnormals, 1e-3 of the same sign in their place: where a subnormal input makes
    1 / tanh infinite and the product has underflowed, boxplus forms 0 * inf and clamps it, and NumPy's `maximum` in
    `mbp4_reference.cn_update` returns NaN where the header's FG_MAX returns the bound ("Soft syndromes"; the
    restatements with extra inputs use fmax / fmin and cover those rows).  Nothing is masked out afterwards."""
    rows = st_rule_rows().copy()
    rows[:, 2] = 0
    if cn_type == "boxplus":
        v = rows[:, HEAD:]
        sub = (v != 0) & (np.abs(v) < F32(1.17549435e-38))
        assert sub.sum() > 100
        v[sub] = np.copysign(F32(1e-3), v[sub])
    return rows


@functools.lru_cache(maxsize=None)
def rule_rows_reference():
    """{cn_type: [N, 12] bits} of `mbp4_reference.cn_update` on rule_rows(cn_type), a slot from deg on 0: per degree on the one-check
    graph of that degree, the rows of the degree (and of one factor: the restatement takes a scalar) as the batch."""
    want = {}
    for cn in CN_TYPES:
        rows = rule_rows(cn)
        deg = rows[:, 0].astype(int)
        want[cn] = np.zeros((len(rows), DMAX), np.uint32)
        for d in np.unique(deg):
            side = MB.Side(np.ones((1, d), np.int64))
            assert np.array_equal(side.cn_tab[0], np.arange(d)), "input j of the check is edge j"
            for f in np.unique(rows[deg == d, 3]):
                sel = (deg == d) & (rows[:, 3] == f)
                mu = MB.cn_update(side, rows[sel, HEAD:HEAD + d].copy(), (rows[sel, 1:2] != 0).astype(np.uint8), cn, F32(f))
                assert not np.isnan(mu).any(), (cn, d)
                want[cn][sel, :d] = bits(mu)
    return want


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_rules_without_extra_inputs_equal_the_restatement_bitwise(flags):
    want = rule_rows_reference()  # NaN-free, asserted there, before anything is compared
    for g, cn in enumerate(CN_TYPES):  # the loop form
        rows = rule_rows(cn)
        got = run_cn_rule_check(flags, rows).reshape(len(rows), 5, 14)
        assert not got[:, :, 12:].any(), "no extra input, no output for one"
        got = got[:, :, :12]
        bad = np.nonzero(~(got[:, g] == want[cn]).all(1))[0]
        assert len(bad) == 0, (cn, bad[:10], rows[bad[:3]])
    # rows and got are now those of min-sum, the full table
    bad = np.nonzero(~(got[:, 3] == want["minsum"]).all(1))[0]
    assert len(bad) == 0, ("register form, guarded", bad[:10])
    six = rows[:, 0] == 6
    assert six.sum() > 500 and (got[six, 4] == want["minsum"][six]).all(), "register form at its compile-time degree"
    assert not got[~six, 4].any()
    assert set(rows[:, 0].astype(int)) >= set(range(2, DMAX + 1)), "every degree"
