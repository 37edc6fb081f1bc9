#!/usr/bin/env python3
"""Generate tests/golden/convert_paired.npz by RUNNING the upstream reference's convertBam with its `mapq` and
`demandPair` parameters (development container only, like make_convert_golden.py).

pysam is not installed, so an `AlignmentFile` stand-in that serves reads from arrays is put on the `pysam` shim
module of tools/ref_loader.py; its reads carry `is_proper_pair`, `is_read1` (flag bits 0x2 / 0x40) and
`next_reference_start` (the mate position) beside `pos` and `mapping_quality`.  Everything else is the reference's own
code.  Stored per case: the inputs (reference names and lengths, positions, mapping qualities, flag words, mate
positions, parameters) and what the REAL convertBam returned (counts per chromosome, the quality dict).  Arrays and
strings only; no reference source text is written.

Run:  python tools/make_convert_paired_golden.py      (needs the reference sources, see ref_loader.py)
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402
from make_convert_golden import KEYS, QUALITY, ReadIter  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PAIR = 0x43             # paired, proper pair, first in pair
OTHER = (0x0, 0x1, 0x41, 0x83, 0x2, 0x40, 0xA3)      # none of them both 0x2 and 0x40


class Read(object):
    __slots__ = ("pos", "mapping_quality", "is_proper_pair", "is_read1", "next_reference_start")

    def __init__(self, pos, mapq, flag, mate):
        self.pos, self.mapping_quality = pos, mapq
        self.is_proper_pair, self.is_read1, self.next_reference_start = bool(flag & 0x2), bool(flag & 0x40), mate


class FakeAlignmentFile(object):
    def __init__(self, names, lengths, reads):
        self.references, self.lengths, self._reads = names, lengths, reads
        self.mapped, self.unmapped, self.nocoordinate = 2100, 41, 5

    def fetch(self, chrom):
        return ReadIter([Read(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*self._reads[chrom])])


def base_reads():
    """(names, lengths, {name: (pos, mapq, flag, mate)}): the situations the paired branch has to get right"""
    rng = np.random.RandomState(31)
    names = ["chr1", "chrM", "2", "CHR3", "chr4", "GL000207.1", "6", "chrX", "Y", "chr22", "chr10", "chr11"]
    lengths = [61000, 16571, 58000, 52000, 47000, 4262, 44000, 40000, 30000, 21000, 35000, 33000]
    eligible = {"chr1": 1.0, "chrM": 0.5, "2": 0.5, "CHR3": 0.03, "chr4": 0.0, "GL000207.1": 0.5, "6": 0.6, "chrX": 0.9,
                "Y": 1.0, "chr22": 0.7, "chr10": 0.5, "chr11": 0.8}
    reads = {}
    for i, (nm, ln) in enumerate(zip(names, lengths)):
        n = 330 + 23 * i
        p = rng.randint(0, ln, n)
        extra = p[rng.rand(n) < 0.2]
        p = np.sort(np.concatenate([p, extra, extra[:len(extra) // 2], ln // 3 + np.arange(7), ln // 2 + 3 * np.arange(6)]))
        q = np.where(rng.rand(len(p)) < 0.15, 0, rng.choice([1, 5, 20, 29, 30, 60], len(p)))
        f = np.where(rng.rand(len(p)) < eligible[nm], PAIR, rng.choice(OTHER, len(p)))
        m = rng.randint(0, ln, len(p))
        same = rng.rand(len(p)) < 0.5                       # mate position equal to the previous read's
        m[1:][same[1:]] = m[:-1][same[1:]]
        m[rng.rand(len(p)) < 0.03] = -1
        reads[nm] = [p, q, f, m]

    def join(a, b):
        """the last read of `a` and the second read of `b` (the first one that is counted) become an equal eligible
        pair: `a` is cut short in front of b's first quartile, `b` loses what lies in front of that position"""
        pa, pb = reads[a][0], reads[b][0]
        short = pa < pb[len(pb) // 4]
        assert short.sum() >= 50
        reads[a] = [x[short] for x in reads[a]]
        pa, qa, fa, ma = reads[a]
        fa[-1], qa[-1] = PAIR, 60
        tail = np.flatnonzero(pb >= pa[-1])
        tail = tail[tail > 0]
        first = (min(pb[0], pa[-1]), 60, PAIR, 5)
        second = (pa[-1], 60, PAIR, ma[-1])
        reads[b] = [np.concatenate([[u, v], x[tail]]) for u, v, x in zip(first, second, reads[b])]

    join("chr1", "2")               # the skipped chrM lies between them
    join("chr10", "chr11")          # nothing between them
    # chr4 has no eligible read at all and the first 119 counted reads of "6" are made ineligible, so the pair (last
    # read of CHR3, read 120 of "6") is carried over a whole chromosome and a long run: make them equal
    p6, q6, f6, m6 = reads["6"]
    f6[1:120] = [OTHER[j % len(OTHER)] for j in range(119)]
    f6[120], q6[120] = PAIR, 60
    front = reads["CHR3"][0] <= p6[120]
    assert front.sum() >= 50
    reads["CHR3"] = [x[front] for x in reads["CHR3"]]
    p3, q3, f3, m3 = reads["CHR3"]
    p3[-1], q3[-1], f3[-1], m3[-1] = p6[120], 60, PAIR, m6[120]

    def put(nm, at, rows):
        """overwrite reads[nm][at:at + len(rows)] with (pos - pos[at - 1], mapq, flag, mate) rows; positions stay sorted"""
        p, q, f, m = reads[nm]
        lo, hi = p[at - 1], p[at + len(rows)]
        for j, (a, b, c, d) in enumerate(rows):
            assert lo + a <= hi, (nm, at, lo + a, hi)
            p[at + j], q[at + j], f[at + j], m[at + j] = lo + a, b, c, d

    # chr1 (all eligible): same position, different mate (paired: kept; plain: a duplicate); equal pairs, one of them
    # with low mapping quality, one with mate -1
    put("chr1", 40, [(0, 60, PAIR, 500), (0, 60, PAIR, 501), (0, 60, PAIR, 501), (0, 0, PAIR, 501), (0, 60, PAIR, -1),
                     (0, 60, PAIR, -1)])
    # an equal (pos, mate) pair separated by a run of ineligible reads on the same position (paired: one duplicate;
    # plain: every read of the run is a duplicate of its left neighbour)
    put("2", 60, [(0, 60, PAIR, 777)] + [(0, 60, OTHER[j % len(OTHER)], 100 + j) for j in range(9)] + [(0, 60, PAIR, 777)])
    # the same separated by an ineligible read that has the same mate, and a differing mate behind it
    put("2", 120, [(0, 30, PAIR, 42), (0, 30, 0x1, 42), (0, 30, PAIR, 42), (0, 30, PAIR, 43)])
    # towers (within min_shift 4) whose members are partly ineligible: 5 reads of which 3 remain, 6 of which 5 remain
    put("6", 200, [(0, 60, PAIR, 1), (1, 60, 0x41, 2), (1, 60, PAIR, 3), (1, 60, 0x83, 4), (2, 60, PAIR, 5)])
    put("chrX", 100, [(0, 60, PAIR, 1), (1, 60, PAIR, 2), (1, 60, 0x0, 3), (2, 60, PAIR, 4), (2, 60, PAIR, 5),
                      (3, 60, PAIR, 6)])
    reads["Y"] = [np.array([777]), np.array([60]), np.array([PAIR]), np.array([900])]          # a one-read chromosome
    for nm, ln in zip(names, lengths):
        p = reads[nm][0]
        assert np.all(np.diff(p) >= 0) and p.max() < ln and len({len(x) for x in reads[nm]}) == 1, nm
    return names, lengths, reads


def cases():
    """(name, binsize, min_shift, threshold, mapq, demandPair)"""
    out = [("paired_defaults", 1000.0, 4, 4, 1, True)]
    for q in (0, 1, 30, 61):
        out.append(("paired_mapq_%d" % q, 1000.0, 4, 4, q, True))
        out.append(("plain_mapq_%d" % q, 1000.0, 4, 4, q, False))
    out.append(("paired_threshold_-1", 1000.0, 4, -1, 1, True))
    out.append(("paired_min_shift_0", 1000.0, 0, 4, 1, True))
    out.append(("paired_min_shift_10", 777.25, 10, 2, 20, True))
    return out


def main():
    wt, _, _ = ref_loader.load()
    import pysam
    names, lengths, reads = base_reads()
    pysam.AlignmentFile = lambda f, mode: FakeAlignmentFile(names, lengths, reads)
    rec = {"names": np.array(names), "lengths": np.array(lengths, dtype=np.int64),
           "pos": np.concatenate([reads[n][0] for n in names]).astype(np.int32),
           "mapq": np.concatenate([reads[n][1] for n in names]).astype(np.uint8),
           "flag": np.concatenate([reads[n][2] for n in names]).astype(np.uint16),
           "mate_pos": np.concatenate([reads[n][3] for n in names]).astype(np.int32),
           "offsets": np.concatenate([[0], np.cumsum([len(reads[n][0]) for n in names])]).astype(np.int64)}
    listed = []
    for name, binsize, min_shift, threshold, mapq, paired in cases():
        with contextlib.redirect_stdout(io.StringIO()):
            counts, quality = wt.convertBam("x.bam", binsize=binsize, minShift=min_shift, threshold=threshold, mapq=mapq,
                                            demandPair=paired)
        listed.append(name)
        rec[name + "_params"] = np.array([binsize, min_shift, threshold, mapq, int(paired)], dtype=np.float64)
        rec[name + "_present"] = np.array([counts[k] is not None for k in KEYS])
        rec[name + "_bins"] = np.array([0 if counts[k] is None else len(counts[k]) for k in KEYS], dtype=np.int64)
        rec[name + "_counts"] = np.concatenate([counts[k] for k in KEYS if counts[k] is not None]).astype(np.int32)
        rec[name + "_quality"] = np.array([int(quality[k]) for k in QUALITY], dtype=np.int64)
    rec["cases"] = np.array(listed)
    rec["quality_keys"] = np.array(QUALITY)
    path = os.path.join(GOLD, "convert_paired.npz")
    np.savez_compressed(path, **rec)
    print("wrote tests/golden/convert_paired.npz: %d cases, %d bytes (convert.npz: %d)"
          % (len(listed), os.path.getsize(path), os.path.getsize(os.path.join(GOLD, "convert.npz"))))


if __name__ == "__main__":
    main()
