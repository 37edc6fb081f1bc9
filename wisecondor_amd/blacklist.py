"""Bin blacklists: which bins of a healthy cohort's held-out z-scores are spread too wide, as a BED file, and that file
back as the bins `newref` drops.

The robust figures, per bin the median and the median absolute deviation over the samples, come from the device
(wc_column_robust; include/wisecondor_hip.h has the rule).  Everything else here is host work on small arrays.
"""
import math

import numpy as np

from . import _lib

MAD_TO_SD = 1.4826                # the standard deviation of a normal distribution in units of its MAD


def robustBins(Z, device=0):
    """(col_i int32 [n_cols, 2] {finite, nonfinite}, col_f float64 [n_cols, 2] {median, mad}) of the columns of the host
    array Z [n_rows, n_cols] through wc_column_robust."""
    lib = _lib.load()
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    if Z.ndim != 2:
        raise ValueError('Z of %s' % (Z.shape,))
    col_i, col_f = np.zeros((Z.shape[1], 2), dtype=np.int32), np.zeros((Z.shape[1], 2), dtype=np.float64)
    _lib.check(lib.wc_column_robust(_lib.context(device), _lib.ptr(Z), Z.shape[1], Z.shape[0], Z.shape[1], _lib.ptr(col_i),
                                    _lib.ptr(col_f)))
    return col_i, col_f


def spreadOf(col_f):
    """1.4826 * mad: the robust stand-in for a standard deviation."""
    return MAD_TO_SD * np.asarray(col_f, dtype=np.float64).reshape(-1, 2)[:, 1]


def listedBins(col_i, col_f, n_samples, maxspread, maxshift=None, mincover=0.5):
    """bool [n_total]: a bin is listed when finite >= ceil(mincover * n_samples) and 1.4826 * mad > maxspread, or maxshift is
    given and fabs(median) > maxshift.  A bin no fold tested has no finite value and is never listed: the mask has dropped
    it already."""
    col_i = np.asarray(col_i).reshape(-1, 2)
    col_f = np.asarray(col_f, dtype=np.float64).reshape(-1, 2)
    if len(col_i) != len(col_f):
        raise ValueError('%d and %d bins' % (len(col_i), len(col_f)))
    finite = col_i[:, 0].astype(np.int64)
    covered = (finite >= int(math.ceil(float(mincover) * int(n_samples)))) & (finite > 0)
    with np.errstate(invalid='ignore'):
        listed = spreadOf(col_f) > float(maxspread)
        if maxshift is not None:
            listed |= np.fabs(col_f[:, 0]) > float(maxshift)
    return covered & listed


def _runs(listed, chrom_sizes):
    """(chromosome 1-based, first bin, last bin) of every run of adjacent listed bins inside a chromosome."""
    listed = np.asarray(listed).astype(bool).reshape(-1)
    sizes = [int(v) for v in chrom_sizes]
    if len(listed) != sum(sizes):
        raise ValueError('%d bins for a layout of %d' % (len(listed), sum(sizes)))
    out, at = [], 0
    for c, size in enumerate(sizes):
        row = listed[at:at + size]
        at += size
        first = None
        for g in range(size + 1):
            on = g < size and row[g]
            if on and first is None:
                first = g
            if not on and first is not None:
                out.append((c + 1, first, g - 1))
                first = None
    return out


def writeBlacklist(path, listed, chrom_sizes, binsize, prefix='chr', note=''):
    """One '#' line with the bin size and `note` (the criteria), then a BED3 line
    '<prefix><c>\\t<first * binsize>\\t<(last + 1) * binsize>' per run of adjacent listed bins inside a chromosome,
    chromosomes ascending.  Returns the number of runs."""
    runs = _runs(listed, chrom_sizes)
    binsize = int(binsize)
    with open(path, 'w') as handle:
        handle.write('# binsize=%d%s\n' % (binsize, ' ' + ' '.join(str(note).split()) if str(note).strip() else ''))
        for c, first, last in runs:
            handle.write('%s%d\t%d\t%d\n' % (prefix, c, first * binsize, (last + 1) * binsize))
    return len(runs)


def readBlacklist(path, chrom_sizes, binsize):
    """(drop uint8 [n_total], lines ignored) of a BED file in base pairs at the layout chrom_sizes of `binsize` bp bins: bin g
    of a chromosome is dropped when [g * binsize, (g + 1) * binsize) meets a line's [start, end).  Empty lines and lines
    that start with '#', 'track' or 'browser' are skipped; fields are split on white space; the chromosome is 1 .. 22 with
    or without a leading 'chr', any other name (X, Y, M, contigs) is ignored and counted; spans beyond the layout are
    clipped.  ValueError naming the line number: fewer than three fields, coordinates that are no whole numbers, start < 0,
    end <= start."""
    sizes = [int(v) for v in chrom_sizes]
    binsize = int(binsize)
    if binsize < 1:
        raise ValueError('a bin size of %d' % binsize)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    drop = np.zeros(int(offs[-1]), dtype=np.uint8)
    ignored = 0
    with open(path) as handle:
        for number, line in enumerate(handle, 1):
            text = line.strip()
            if not text or text.startswith(('#', 'track', 'browser')):
                continue
            fields = text.split()
            if len(fields) < 3:
                raise ValueError('%s line %d: %d fields, a BED line has three at least' % (path, number, len(fields)))
            try:
                start, end = int(fields[1]), int(fields[2])
            except ValueError:
                raise ValueError('%s line %d: coordinates %r %r are no whole numbers' % (path, number, fields[1], fields[2]))
            if start < 0 or end <= start:
                raise ValueError('%s line %d: a span of %d .. %d' % (path, number, start, end))
            name = fields[0][3:] if fields[0].startswith('chr') else fields[0]
            if not (name.isdigit() and name == str(int(name)) and 1 <= int(name) <= min(22, len(sizes))):
                ignored += 1
                continue
            c = int(name) - 1
            first, last = start // binsize, min((end - 1) // binsize, sizes[c] - 1)
            if first <= last:
                drop[offs[c] + first:offs[c] + last + 1] = 1
    return drop, ignored
