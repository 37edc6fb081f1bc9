"""convertBam (the reference's wisetools.py:116-217) with both of its extra parameters, `mapq` and `demandPair`,
restated in numpy without the per-read loop.  tests/test_convert_paired_cpu.py holds it against what the REAL
convertBam returned (tests/golden/convert_paired.npz, tools/make_convert_paired_golden.py) and, at mapq 1 in plain
mode, against tests/convert_restated.py; the GPU tests hold the kernels against it.

Paired mode: of a chromosome's reads behind the consumed first one, only those whose flag has 0x2 (proper pair) and
0x40 (first in pair) take part; the others add one to pair_fail each.  A duplicate has the position AND the mate
position of the previous read that took part -- the state is carried over ineligible reads and chromosomes alike and
starts as (-1, -1)."""
import numpy as np

from convert_restated import KEYS, chrom_key, n_bins

PROPER_PAIR, READ1 = 0x2, 0x40


def convert(names, lengths, pos_by_ref, mapq_by_ref, flag_by_ref, mate_by_ref, binsize, min_shift, threshold, min_mapq=1,
            paired=False):
    """(dict chromosome -> int32[bins] or None, dict of the five counters).  A chromosome without reads (the
    reference dies there) or with one read gives zeros and leaves the carried state alone."""
    out = {k: None for k in KEYS}
    rmdup = lowq = seen = kept = fail = 0
    larp = larp2 = -1
    for name, length, pos, mapq, flag, mate in zip(names, lengths, pos_by_ref, mapq_by_ref, flag_by_ref, mate_by_ref):
        key = chrom_key(name)
        if key is None:
            continue
        counts = np.zeros(n_bins(length, binsize), dtype=np.int32)
        p = np.asarray(pos, dtype=np.int64)[1:]          # the first read is consumed by sam_iter.next()
        q = np.asarray(mapq, dtype=np.int64)[1:]
        if paired:
            f = np.asarray(flag, dtype=np.int64)[1:]
            elig = ((f & PROPER_PAIR) != 0) & ((f & READ1) != 0)
            fail += int((~elig).sum())
            p, q, m = p[elig], q[elig], np.asarray(mate, dtype=np.int64)[1:][elig]
        if len(p):
            dup = p == np.concatenate(([larp], p[:-1]))
            if paired:
                dup &= m == np.concatenate(([larp2], m[:-1]))
                larp2 = int(m[-1])
            larp = int(p[-1])
            keep = ~dup & (q >= min_mapq)
            rmdup += int(dup.sum())
            lowq += int((~dup & (q < min_mapq)).sum())
            seen += len(p)
            k = p[keep]
            if len(k):
                head = np.concatenate(([True], np.diff(k) > min_shift))
                run = np.cumsum(head) - 1
                ok = (np.bincount(run)[run] <= threshold) | (threshold < 0)
                bins = (k[ok] / float(binsize)).astype(np.int64)
                if len(bins) and (bins.min() < 0 or bins.max() >= len(counts)):
                    raise IndexError("a read lies beyond the last bin of %s" % name)
                counts += np.bincount(bins, minlength=len(counts)).astype(np.int32)
        out[key] = counts
        kept += int(counts.sum())
    return out, dict(filter_rmdup=rmdup, filter_mapq=lowq, pre_retro=seen, post_retro=kept, pair_fail=fail)
