"""wc_column_robust and wc_column_robust_dev (csrc/robust.hip) against the restatement of robust_restated.py, integers
equal and doubles by bits: the hand-written columns of robust_cases.py side by side in one wave, random matrices at every
row count around the kernel's unrolling and the wave's width, column counts around a workgroup's 64 lanes with a row stride
equal to and above them, repeated calls, and the refusals."""
import numpy as np
import pytest

import robust_cases as rc
import robust_restated as rr

pytestmark = pytest.mark.gpu
N_ROWS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 8192]
N_COLS = [1, 63, 64, 65, 129]


def host_entry(Z, n_cols=None, n_rows=None, col_i=None, col_f=None):
    """wc_column_robust on the first n_cols columns of Z: (return code, col_i, col_f)."""
    from wisecondor_amd import _lib
    lib = _lib.load()
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    n_cols = Z.shape[1] if n_cols is None else n_cols
    n_rows = Z.shape[0] if n_rows is None else n_rows
    col_i = np.full((max(n_cols, 1), 2), -7, dtype=np.int32) if col_i is None else col_i
    col_f = np.full((max(n_cols, 1), 2), -7.0) if col_f is None else col_f
    rc_ = lib.wc_column_robust(_lib.context(0), _lib.ptr(Z), Z.shape[1], n_rows, n_cols, _lib.ptr(col_i), _lib.ptr(col_f))
    return rc_, col_i, col_f


def assert_equal(got_i, got_f, Z, n_cols=None):
    want_i, want_f = rr.robust(Z, n_cols)
    assert np.array_equal(got_i, want_i), np.flatnonzero((got_i != want_i).any(axis=1))[:8]
    assert rr.same_bits(got_f, want_f), [(b, got_f[b].tolist(), want_f[b].tolist()) for b in range(len(want_f))
                                        if not rr.same_bits(got_f[b], want_f[b])][:4]


def test_hand_written_columns_in_one_wave():
    Z = rc.matrix()
    assert Z.shape[1] < 64
    code, col_i, col_f = host_entry(Z)
    assert code == 0
    for b, (name, values) in enumerate(rc.COLUMNS):
        want = rr.column(values)
        assert (int(col_i[b, 0]), int(col_i[b, 1])) == want[:2], name
        assert rr.same_bits(col_f[b], want[2:]), (name, col_f[b].tolist(), want[2:])
    assert_equal(col_i, col_f, Z)
    assert sorted(set(col_i[:, 0].tolist()))[:3] == [0, 1, 2]       # lanes of one wave with no value, one value, two
    median = col_f[[name for name, _ in rc.COLUMNS].index("pairs -x and +x"), 0]
    assert median == 0.0 and not np.signbit(median)
    # behind a wider stride, and with the columns in the reverse order
    wide = rc.matrix(stride=Z.shape[1] + 5)
    code, col_i, col_f = host_entry(wide, n_cols=Z.shape[1])
    assert code == 0
    assert_equal(col_i, col_f, Z)
    code, col_i, col_f = host_entry(Z[:, ::-1])
    assert code == 0
    assert_equal(col_i, col_f, Z[:, ::-1])


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_random_matrices_at_every_shape(n_rows):
    for n_cols in N_COLS:
        for stride in (None, n_cols + 3):
            Z = rc.random_matrix(1000 * n_rows + n_cols, n_rows, n_cols, stride=stride)
            code, col_i, col_f = host_entry(Z, n_cols=n_cols)
            assert code == 0, (n_cols, stride)
            assert_equal(col_i, col_f, Z, n_cols)


def test_every_row_holds_a_value_at_the_row_limit():
    """8 192 finite values in a column: the 16-bit digit counters at their largest count, all in one digit (equal values) and
    spread over all of them."""
    rng = np.random.RandomState(5)
    Z = np.stack([np.full(8192, 1.25), rng.standard_normal(8192), np.round(rng.standard_normal(8192)) + 0.5,
                  -np.abs(rng.standard_normal(8192)) * 1e300], axis=1)
    code, col_i, col_f = host_entry(Z)
    assert code == 0 and col_i[:, 0].tolist() == [8192] * 4
    assert_equal(col_i, col_f, Z)


def test_the_same_bits_twice_and_after_a_smaller_call():
    Z = rc.random_matrix(77, 257, 129)
    first = host_entry(Z)
    small = host_entry(Z[:5, :63].copy())
    assert small[0] == 0
    assert_equal(small[1], small[2], Z[:5, :63])
    second = host_entry(Z)
    assert first[0] == second[0] == 0 and np.array_equal(first[1], second[1]) and rr.same_bits(first[2], second[2])
    assert_equal(second[1], second[2], Z)


def test_device_entry_equals_host_entry():
    import torch
    from wisecondor_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    Z = rc.random_matrix(78, 65, 129, stride=140)
    _, want_i, want_f = host_entry(Z, n_cols=129)
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        z = torch.from_numpy(Z).to(dev)
        col_i = torch.full((129, 2), -7, dtype=torch.int32, device=dev)
        col_f = torch.full((129, 2), -7.0, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.wc_column_robust_dev(ctx, stream, z.data_ptr(), 140, 65, 129, col_i.data_ptr(), col_f.data_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(col_i.cpu().numpy(), want_i) and rr.same_bits(col_f.cpu().numpy(), want_f)
    assert_equal(want_i, want_f, Z, 129)
    from wisecondor_amd import blacklist
    got_i, got_f = blacklist.robustBins(Z[:, :129])
    assert np.array_equal(got_i, want_i) and rr.same_bits(got_f, want_f)


def test_refusals_leave_the_outputs_untouched():
    from wisecondor_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    Z = np.ones((8193, 2))
    code, col_i, col_f = host_entry(Z)
    assert code == _lib.E_LIMIT and (col_i == -7).all() and (col_f == -7.0).all()
    assert host_entry(Z[:8192])[0] == 0
    Z = np.ones((4, 3))
    for kwargs in (dict(n_rows=0), dict(n_cols=0), dict(n_cols=4), dict(n_rows=-1)):
        code, col_i, col_f = host_entry(Z, **kwargs)
        assert code == _lib.E_ARG and (col_i == -7).all() and (col_f == -7.0).all(), kwargs
    col_i, col_f = np.full((3, 2), -7, dtype=np.int32), np.full((3, 2), -7.0)
    for args in ((None, _lib.ptr(Z), 3, 4, 3, _lib.ptr(col_i), _lib.ptr(col_f)), (ctx, None, 3, 4, 3, _lib.ptr(col_i), _lib.ptr(col_f)),
                 (ctx, _lib.ptr(Z), 3, 4, 3, None, _lib.ptr(col_f)), (ctx, _lib.ptr(Z), 3, 4, 3, _lib.ptr(col_i), None)):
        assert lib.wc_column_robust(*args) == _lib.E_ARG
    assert (col_i == -7).all() and (col_f == -7.0).all()
    # the device entry refuses the same before it launches
    assert lib.wc_column_robust_dev(ctx, None, _lib.ptr(Z), 2, 4, 3, _lib.ptr(col_i), _lib.ptr(col_f)) == _lib.E_ARG
    assert lib.wc_column_robust_dev(ctx, None, _lib.ptr(Z), 3, 8193, 3, _lib.ptr(col_i), _lib.ptr(col_f)) == _lib.E_LIMIT
    assert lib.wc_column_robust_dev(ctx, None, None, 3, 4, 3, _lib.ptr(col_i), _lib.ptr(col_f)) == _lib.E_ARG
