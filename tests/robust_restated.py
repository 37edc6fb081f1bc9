"""The rule of wc_column_robust (include/wisecondor_hip.h) restated with numpy's sort: the definition the
kernel is held against, integers equal and doubles by bits.  Nothing here imports the package."""
import numpy as np

MAX_ROWS = 8192


class Refused(ValueError):
    """What the library answers with WC_E_ARG."""


class TooLarge(ValueError):
    """What the library answers with WC_E_LIMIT."""


def med(values):
    """The middle of `values` (float64, no NaN among them) sorted ascending: s[(n - 1) / 2] for odd n, else
    (s[n / 2 - 1] + s[n / 2]) / 2.0, the sum rounded first.  NaN for none."""
    s = np.sort(np.asarray(values, dtype=np.float64))
    n = len(s)
    if n == 0:
        return np.float64("nan")
    if n % 2:
        return s[(n - 1) // 2]
    with np.errstate(over="ignore"):
        return np.float64(s[n // 2 - 1] + s[n // 2]) / np.float64(2.0)


def column(z):
    """(finite, nonfinite, median, mad) of one column."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    tested = z[z != 0]                                  # both zeros are untested, NaN is tested
    v = tested[np.isfinite(tested)]
    median = med(v)
    mad = np.float64("nan")
    if len(v) and np.isfinite(median):
        with np.errstate(over="ignore"):
            mad = med(np.abs(v - median))
    return len(v), len(tested) - len(v), median, mad


def robust(Z, n_cols=None):
    """(col_i int32 [n_cols, 2], col_f float64 [n_cols, 2]) of the first n_cols columns of Z [n_rows, row_stride]."""
    Z = np.asarray(Z, dtype=np.float64)
    n_cols = Z.shape[1] if n_cols is None else int(n_cols)
    if Z.ndim != 2 or Z.shape[0] < 1 or n_cols < 1 or Z.shape[1] < n_cols:
        raise Refused("shape")
    if Z.shape[0] > MAX_ROWS:
        raise TooLarge("rows")
    col_i, col_f = np.zeros((n_cols, 2), dtype=np.int32), np.zeros((n_cols, 2), dtype=np.float64)
    for b in range(n_cols):
        col_i[b, 0], col_i[b, 1], col_f[b, 0], col_f[b, 1] = column(Z[:, b])
    return col_i, col_f


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)             # every NaN is one NaN: its payload is nobody's rule
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint64)[~nan_a], b.view(np.uint64)[~nan_b])
