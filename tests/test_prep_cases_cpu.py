"""The inputs of test_prep_shapes_gpu.py / test_pca_apply_gpu.py and the methods' own margins, without any
kernel: every prep case meets the two input conditions, numpy's float64 Gram route (what prep.hip does)
stays a thousand times inside the tolerances the GPU is held to, and float64 applyPCA stays within 1e-13
of its np.longdouble restatement."""
import numpy as np
import pytest

import prep_cases as pc
from oracle import wc_oracle as wo


@pytest.mark.parametrize("case", pc.ALL_CASES, ids=pc.case_id)
def test_case_is_well_conditioned_and_gram_route_agrees(case):
    n_s, n_b, n_comp = case
    want = pc.oracle(*case)
    assert want["masked"].shape == (n_b, n_s)
    assert int(want["mask"].sum()) == n_b and 0.05 < 1.0 - n_b / float(len(want["mask"])) < 0.15
    pc.check_conditions(want, n_comp)
    corrected, comps, mean = pc.gram_route(want["masked"], n_comp)
    assert np.array_equal(mean, want["mean"])
    comp_err, corr_err = pc.errors(corrected, comps, want)
    print("%s: components %.2e, correctedData %.2e (relative), ratios %s"
          % (pc.case_id(case), comp_err, corr_err, np.round(want["sing"][:n_comp] / want["sing"][1:n_comp + 1], 3)))
    # a thousandth of the GPU tests' tolerances: the method itself is not what they measure
    assert comp_err <= pc.COMP_ATOL / 1000
    assert corr_err <= pc.CORRECTED_RTOL / 1000


def test_cases_are_seeded():
    a, sa = pc.make_case(9, 65)
    pc.make_case.cache_clear()
    b, sb = pc.make_case(9, 65)
    assert a is not b and np.array_equal(a, b) and np.array_equal(sa, sb)
    assert a.dtype == np.int32 and len(sa) == 22 and a.shape == (9, int(sa.sum()))
    assert not np.array_equal(pc.make_case(9, 65, seed=1)[0], a)


@pytest.mark.parametrize("n_comp", pc.APPLY_COMPS)
@pytest.mark.parametrize("n_bins", pc.APPLY_BINS)
def test_apply_pca_float64_against_longdouble(n_comp, n_bins):
    x, mean, comps = pc.apply_case(n_comp, n_bins)
    want = pc.apply_want(n_comp, n_bins)
    assert comps.shape == (n_comp, n_bins) and x.shape == (33, n_bins)
    if n_comp:
        assert np.allclose(np.linalg.norm(comps, axis=1), 1.0, rtol=0, atol=1e-12)
    k = min(n_comp, n_bins)
    assert np.allclose(comps[:k] @ comps[:k].T, np.eye(k), rtol=0, atol=1e-12)
    got = np.stack([wo.apply_pca(row, mean, comps.reshape(n_comp, n_bins)) for row in x])
    assert np.all(np.isfinite(want)) and np.all(want > 0.5) and np.all(want < 2.0)
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    if n_comp == 0:
        assert np.array_equal(got, x / mean)          # (the longdouble form is rounded twice: not the same bits)
