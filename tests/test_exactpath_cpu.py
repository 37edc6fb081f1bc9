"""The partial oracle of tests/test_exactpath_gpu.py (wo.oracle_rows: chosen target rows only) against the
whole-matrix oracle it stands in for, where both are cheap.  No device needed."""
import numpy as np
import pytest

from oracle import wc_oracle as wo


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


@pytest.mark.parametrize("layout", [[120, 90, 1, 60, 29], [1, 0, 298, 1]])
@pytest.mark.parametrize("order", ["C", "F"])
def test_oracle_rows_equals_get_reference(layout, order):
    """300 bins x 40 samples, duplicate rows across chromosomes and a NaN entry, both summation orders (the
    second layout has the single-row pieces whose chromData is C ordered whatever the file's layout):
    oracle_rows on a fixed set of rows -- row 0, the last row, chromosome edges, the one-bin chromosome,
    the duplicates, the NaN row, rows in arbitrary order -- gives the corresponding rows of get_reference."""
    rng = np.random.RandomState(7)
    bins = np.array(layout, dtype=np.int64)
    sums = np.cumsum(bins)
    B, k = int(sums[-1]), 30
    assert B == 300
    data = 1.0 + 0.02 * rng.standard_normal((B, 40))
    data[[5, 130, 250]] = data[40]               # exact duplicates (ties)
    data[77, 3] = np.nan
    if order == "F":
        data = np.asfortranarray(data)
    with np.errstate(all="ignore"):
        want_i, want_d = wo.get_reference(data, bins, sums, k, 1, 1, fast=True)
        rows = [299, 0, 119, 120, 209, 210, 211, 5, 40, 130, 250, 77, 76] + list(rng.choice(B, 20, replace=False))
        got_i, got_d = wo.oracle_rows(data, bins, sums, k, rows)
    assert got_i.shape == (len(rows), k) and got_i.dtype == want_i.dtype
    assert np.array_equal(got_i, want_i[rows])
    assert same_bits(got_d, want_d[rows])
    assert (got_i[rows.index(77)] == -1).all() and (got_d[rows.index(77)] == 1e10).all()     # the NaN target: padding only
