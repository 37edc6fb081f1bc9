"""convertBam (the reference's wisetools.py:116-217, as toolConvert calls it: mapq 1, demandPair False) restated in
numpy without the per-read loop.  tests/test_convert_cpu.py holds it against what the REAL convertBam returned
(tests/golden/convert.npz, tools/make_convert_golden.py); the GPU tests hold the kernels against it."""
import numpy as np

KEYS = [str(c) for c in range(1, 23)] + ["X", "Y"]


def chrom_key(name):
    key = name[3:] if name[:3].lower() == "chr" else name
    return key if key in KEYS else None


def n_bins(length, binsize):
    return int(int(length) / float(binsize) + 1)


def convert(names, lengths, pos_by_ref, mapq_by_ref, binsize, min_shift, threshold):
    """(dict chromosome -> int32[bins] or None, dict of the four filter counters + pair_fail).  A chromosome without
    reads (the reference dies there) or with one read gives zeros and leaves larp alone."""
    out = {k: None for k in KEYS}
    rmdup = lowq = seen = kept = 0
    larp = -1
    for name, length, pos, mapq in zip(names, lengths, pos_by_ref, mapq_by_ref):
        key = chrom_key(name)
        if key is None:
            continue
        counts = np.zeros(n_bins(length, binsize), dtype=np.int32)
        p = np.asarray(pos, dtype=np.int64)[1:]          # the first read is consumed by sam_iter.next()
        q = np.asarray(mapq)[1:]
        if len(p):
            prev = np.concatenate(([larp], p[:-1]))
            dup = p == prev
            keep = ~dup & (q >= 1)
            rmdup += int(dup.sum())
            lowq += int((~dup & (q < 1)).sum())
            seen += len(p)
            larp = int(p[-1])
            k = p[keep]
            if len(k):
                head = np.concatenate(([True], np.diff(k) > min_shift))
                run = np.cumsum(head) - 1
                length_of = np.bincount(run)
                ok = (length_of[run] <= threshold) | (threshold < 0)
                bins = (k[ok] / float(binsize)).astype(np.int64)
                if len(bins) and (bins.min() < 0 or bins.max() >= len(counts)):
                    raise IndexError("a read lies beyond the last bin of %s" % name)
                counts += np.bincount(bins, minlength=len(counts)).astype(np.int32)
        out[key] = counts
        kept += int(counts.sum())
    return out, dict(filter_rmdup=rmdup, filter_mapq=lowq, pre_retro=seen, post_retro=kept, pair_fail=0)

