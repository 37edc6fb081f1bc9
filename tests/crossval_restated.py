"""The rules of wc_crossval_stats (include/wisecondor_hip.h) restated as Python loops over np.float64: the
definition the kernels are held against, integers equal and doubles by bits.  Nothing here imports the package."""
import math

import numpy as np

SLOTS = 130


class Refused(ValueError):
    """What the library answers with WC_E_ARG."""


def check(Z, sizes, thr, asdef, calls, n_calls, sel, lengths):
    sizes = [int(v) for v in sizes]
    n_total = sum(sizes)
    if Z.shape[0] < 1 or not 1 <= len(sizes) <= 64 or min(sizes) < 0 or n_total < 1 or Z.shape[1] < n_total:
        raise Refused('layout')
    if calls.shape[1] < 1:
        raise Refused('max_calls')
    if not 1 <= len(sel) <= len(sizes) or len(set(sel)) != len(sel) or min(sel) < 1 or max(sel) > len(sizes):
        raise Refused('selection')
    if not 1 <= len(lengths) <= 16 or lengths[0] < 1 or any(b <= a for a, b in zip(lengths, lengths[1:])):
        raise Refused('lengths')
    for i in range(Z.shape[0]):
        for r in range(min(max(int(n_calls[i]), 0), calls.shape[1])):
            c, s, e = (np.float64(v) for v in calls[i, r, :3])
            if not (c == np.floor(c) and 1 <= c <= len(sizes)):
                raise Refused('call row %d of sample %d' % (r, i))
            size = sizes[int(c) - 1]
            if not (s == np.floor(s) and e == np.floor(e) and 0 <= s <= e <= size - 1):
                raise Refused('call row %d of sample %d' % (r, i))


def slot_of(w):
    if w < -16.0:
        return 0
    if not w < 16.0:
        return SLOTS - 1
    return min(SLOTS - 1, 1 + int(math.floor(float((np.float64(w) + np.float64(16.0)) * np.float64(4.0)))))


def stats(Z, sizes, thr, asdef, calls, n_calls, sel=None, lengths=(1, 2, 5, 10, 20, 50, 100)):
    """dict of bins_i, bins_f, rec_i, rec_f, win_n, win_i, win_hist; Refused where the library refuses."""
    Z = np.asarray(Z, dtype=np.float64)
    calls = np.asarray(calls, dtype=np.float64)
    sizes = [int(v) for v in sizes]
    sel = list(range(1, 23)) if sel is None else [int(c) for c in sel]
    lengths = [int(v) for v in lengths]
    check(Z, sizes, thr, asdef, calls, n_calls, sel, lengths)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, n_total, n_len = Z.shape[0], int(offs[-1]), len(lengths)
    bins_i = np.zeros((n_total, 6), dtype=np.int32)
    bins_f = np.zeros((n_total, 2), dtype=np.float64)
    rec_i = np.zeros((n, 8), dtype=np.int32)
    rec_f = np.zeros((n, 4), dtype=np.float64)
    win_n = np.zeros((n, n_len), dtype=np.int64)
    win_i = np.zeros((n_len, 4), dtype=np.int64)
    win_hist = np.zeros((n_len, SLOTS), dtype=np.int64)
    with np.errstate(all='ignore'):
        for i in range(n):
            t = np.float64(thr[i])
            finite = []
            for b in range(n_total):
                z = np.float64(Z[i, b])
                if not z != 0:
                    continue
                bins_i[b, 0] += 1
                rec_i[i, 2] += 1
                if not np.isfinite(z):
                    bins_i[b, 1] += 1
                    rec_i[i, 3] += 1
                    continue
                finite.append(z)
                if z >= t:
                    bins_i[b, 2] += 1
                    rec_i[i, 4] += 1
                if z <= -t:
                    bins_i[b, 3] += 1
                    rec_i[i, 5] += 1
                bins_f[b, 0] = bins_f[b, 0] + z
                bins_f[b, 1] = bins_f[b, 1] + z * z              # the product is rounded, then added
            count = min(max(int(n_calls[i]), 0), calls.shape[1])
            rec_i[i, 1] = count
            for r in range(count):
                c, s, e, z = int(calls[i, r, 0]), int(calls[i, r, 1]), int(calls[i, r, 2]), calls[i, r, 3]
                rec_i[i, 6] += e - s + 1
                if z > 0:
                    bins_i[offs[c - 1] + s:offs[c - 1] + e + 1, 4] += 1
                if z < 0:
                    bins_i[offs[c - 1] + s:offs[c - 1] + e + 1, 5] += 1
            rec_f[i] = [asdef[i], t, max(finite) if finite else np.nan, min(finite) if finite else np.nan]
            for c in sel:
                values = [np.float64(v) for v in Z[i, offs[c - 1]:offs[c]] if v != 0]
                if any(not np.isfinite(v) for v in values):
                    rec_i[i, 7] += 1
                    continue
                P = [np.float64(0.0)]
                for v in values:
                    P.append(P[-1] + v)
                for at, L in enumerate(lengths):
                    if len(values) < L:
                        continue
                    root = np.float64(math.sqrt(float(L)))
                    win_i[at, 0] += 1
                    for a in range(len(values) - L + 1):
                        w = (P[a + L] - P[a]) / root
                        win_n[i, at] += 1
                        win_i[at, 1] += 1
                        win_i[at, 2] += bool(w >= t)
                        win_i[at, 3] += bool(w <= -t)
                        win_hist[at, slot_of(w)] += 1
    return dict(bins_i=bins_i, bins_f=bins_f, rec_i=rec_i, rec_f=rec_f, win_n=win_n, win_i=win_i, win_hist=win_hist)


def same(got, want):
    """The first key at which two results differ (integers by value, doubles by bits, NaN equal to NaN), or None."""
    for key in ('bins_i', 'bins_f', 'rec_i', 'rec_f', 'win_n', 'win_i', 'win_hist'):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if a.shape != b.shape or a.dtype != b.dtype:
            return key + ': %s %s against %s %s' % (a.shape, a.dtype, b.shape, b.dtype)
        if a.dtype == np.float64:
            nan = np.isnan(a) & np.isnan(b)
            if not np.all(nan | (a.view(np.int64) == b.view(np.int64))):
                return key
        elif not np.array_equal(a, b):
            return key
    return None
