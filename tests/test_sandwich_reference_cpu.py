"""The stage-by-stage restatement of the sandwich driver (tests/sandwich_reference.py: the oracle's single stages joined by dense NumPy)
against the oracle's own driver `og.sandwich_decode`, on the CPU.  Exact equality: both run the same float32 stages, only the flag /
mask / merge logic between them is written twice.  The round histograms asserted here are the precondition of
tests/test_gpu_sandwich_shapes.py: a table row only reaches the compacted rounds it is listed for when samples leave the flagged set in
the rounds the table says."""
import numpy as np
import pytest

from helpers import WEIGHTS_882, llr_const, oracle_library_forms
from sandwich_reference import CASES, FIRST_SAMPLE, SEED, SHRINKING, case_oracle, case_reference, dense_syndrome, sandwich_reference


def _assert_same(r, o, what):
    for k in ("x_hat", "z_hat", "rounds", "llr"):
        assert np.array_equal(r[k], o[k]), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_oracle_driver_on_the_shape_table(name):
    cname, p, B, iters, hist = CASES[name]
    c, o = case_reference(name), case_oracle(name)
    r = c["ref"]
    og = oracle_library_forms(cname)
    osx, osz = og.syndrome(c["ex"], c["ez"])  # the table's syndromes are dense products: the oracle's CSR ones agree
    assert np.array_equal(osx, c["sx"]) and np.array_equal(osz, c["sz"])
    _assert_same(r, o, name)
    assert r["x_hat"].shape == (B, og.n) and r["llr"].shape == (B, 3, og.n) and r["llr"].dtype == np.float32
    assert np.bincount(r["rounds"], minlength=4).tolist() == hist
    if name in SHRINKING:
        assert min(hist) > 0
    # llr_compact: the marginals of the last decoder that runs on a sample in compacted mode; equal to llr exactly for the samples
    # that stay flagged to the last round, and a different decoder's output for a sample that left earlier
    last = r["rounds"] == len(iters) - 1
    assert np.array_equal(r["llr_compact"][last], r["llr"][last])
    assert (r["llr_compact"][~last] != r["llr"][~last]).any(axis=(1, 2)).all()
    d0 = og.bp4_decode(c["sx"], c["sz"], iters[0], llr_const=llr_const(0.05))
    never = r["rounds"] == 0
    assert np.array_equal(r["llr_compact"][never], d0["llr"][never])
    assert np.array_equal(r["x_hat"][never], d0["x_hat"][never]) and np.array_equal(r["z_hat"][never], d0["z_hat"][never])


MIXED = [
    # name, p, B, iters, cn_types, factors
    ("rsurf5", 0.07, 40, [1, 2, 4, 8], ["minsum", "boxplus", "boxplus-phi", "minsum"], [0.75, 1.0, 0.9, 0.625]),
    ("gb48", 0.07, 24, [2, 3, 5], ["boxplus-phi", "minsum", "boxplus"], [1.0, 0.8, 0.625]),
    ("ghp882", 0.09, 12, [16, 8, 8], ["boxplus-phi", "minsum", "boxplus"], [1.0, 0.8, 0.625]),
]


@pytest.mark.parametrize("name,p,B,iters,cn_types,factors", MIXED)
def test_restatement_stays_exact_with_mixed_check_rules_and_factors(name, p, B, iters, cn_types, factors):
    from feedback_gnn_amd.weights_io import read_weight_list
    og = oracle_library_forms(name)
    ex, ez = og.pauli_noise(SEED, p, FIRST_SAMPLE, B)
    sx, sz = dense_syndrome(og.code, ex, ez)
    w = read_weight_list(WEIGHTS_882)
    wl = [w] * (len(iters) - 1)
    r = sandwich_reference(og, sx, sz, iters, wl, llr_const(0.05), factors=factors, cn_types=cn_types)
    o = og.sandwich_decode(sx, sz, iters, wl, llr_const(0.05), factors=factors, cn_types=cn_types, return_llr=True)
    _assert_same(r, o, name)
    assert 0 < int((r["rounds"] > 0).sum()) < B, "both outcomes of the flag test must occur"
    plain = sandwich_reference(og, sx, sz, iters, wl, llr_const(0.05))
    assert not np.array_equal(plain["llr"], r["llr"]), "the per-layer settings must reach the decoders"
