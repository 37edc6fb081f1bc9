#!/usr/bin/env python3
"""Generate tests/golden/convert.npz by RUNNING the upstream reference's convertBam / toolConvert / toolReport
(development container only, like make_goldens.py).

pysam is not installed, so an `AlignmentFile` stand-in that serves reads from arrays is put on the `pysam` shim
module of tools/ref_loader.py; everything else is the reference's own code.  Stored per case: the inputs (reference
names and lengths, positions, mapping qualities, parameters) and what the REAL convertBam returned (counts per
chromosome, the quality dict); and for `report`: the members of the two files it read and the text it printed.
Arrays and strings only; no reference source text is written.

Run:  python tools/make_convert_golden.py      (needs the reference sources, see ref_loader.py)
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = [str(c) for c in range(1, 23)] + ["X", "Y"]
QUALITY = ("mapped", "unmapped", "no_coordinate", "filter_rmdup", "filter_mapq", "pre_retro", "post_retro", "pair_fail")


class Read(object):
    __slots__ = ("pos", "mapping_quality")

    def __init__(self, pos, mapq):
        self.pos = pos
        self.mapping_quality = mapq


class ReadIter(object):
    def __init__(self, reads):
        self.it = iter(reads)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self.it)

    next = __next__            # the translated reference calls sam_iter.next()


class FakeAlignmentFile(object):
    def __init__(self, names, lengths, reads):
        self.references, self.lengths, self._reads = names, lengths, reads
        self.mapped, self.unmapped, self.nocoordinate = 1100, 22, 3

    def fetch(self, chrom):
        p, q = self._reads[chrom]
        return ReadIter([Read(int(a), int(b)) for a, b in zip(p, q)])


def tower(at, n, step=1):
    return at + step * np.arange(n)


def cases():
    """(name, reference names, lengths, {name: (pos, mapq)}, binsize, min_shift, threshold)"""
    rng = np.random.RandomState(20)

    def stream(length, n, dup=0.05, low=0.1, towers=()):
        p = rng.randint(0, length, n)
        p = np.concatenate([p, p[rng.rand(n) < dup]] + [tower(a, k, s) for a, k, s in towers])
        p = np.sort(p[p < length])
        q = np.where(rng.rand(len(p)) < low, 0, rng.choice([1, 20, 60], len(p)))
        return p.astype(np.int64), q.astype(np.int64)

    out = []
    # mixed names: chr-prefixed in both cases, unprefixed, skipped (chrM, GL...), X / Y; 5, 13, 21 absent
    names = ["chr1", "chrM", "2", "CHR3", "GL000207.1", "chr4", "6", "chrX", "Y", "chr7_random", "chr22"]
    lengths = [249250, 16571, 243199, 198022, 4262, 191154, 171115, 155270, 59373, 5000, 51304]
    reads = {}
    for i, (nm, ln) in enumerate(zip(names, lengths)):
        reads[nm] = stream(ln, 900 + 37 * i, towers=[(ln // 3, 3, 1), (ln // 2, 4, 2), (ln // 2 + 500, 5, 1),
                                                       (ln // 5, 6, 4)])
    # a chromosome whose second read repeats the consumed first read's position (NOT a duplicate: larp is the
    # previous chromosome's last position), and one whose second read equals the previous chromosome's last position
    p, q = reads["2"]
    p, q = p[p < 150000], q[p < 150000]
    reads["2"] = (np.concatenate([[p[0]], p]), np.concatenate([[60], q]))
    last = int(reads["2"][0][-1])
    p, q = reads["CHR3"]
    reads["CHR3"] = (np.concatenate([[3, last], p[p >= last]]), np.concatenate([[60, 60], q[p >= last]]))
    # a tower of 3 000 reads, with runs of mapq-0 reads inside it, and a one-read chromosome
    p, q = reads["chr4"]
    big = tower(100000, 3000, 1)
    bq = np.full(3000, 30)
    bq[500:520] = 0
    bq[1999] = 0
    order = np.argsort(np.concatenate([p, big]), kind="stable")
    reads["chr4"] = (np.concatenate([p, big])[order], np.concatenate([q, bq])[order])
    reads["Y"] = (np.array([777]), np.array([60]))
    base = (names, lengths, reads)
    out.append(("defaults",) + base + (1000.0, 4, 4))
    for th in (-1, 0, 1, 7):
        out.append(("threshold_%d" % th,) + base + (1000.0, 4, th))
    for ms in (-1, 0, 10):
        out.append(("min_shift_%d" % ms,) + base + (1000.0, ms, 4))
    out.append(("binsize_333",) + base + (333.0, 4, 4))
    out.append(("binsize_non_integer",) + base + (777.25, 2, 3))
    out.append(("binsize_1e6",) + base + (1e6, 4, 4))
    out.append(("wide_tower_filter",) + base + (1000.0, 10, 5000))
    return out


def main():
    wt, wc, _ = ref_loader.load()
    import pysam
    rec = {}
    listed = []
    for name, names, lengths, reads, binsize, min_shift, threshold in cases():
        pysam.AlignmentFile = lambda f, mode, N=names, L=lengths, R=reads: FakeAlignmentFile(N, L, R)
        with contextlib.redirect_stdout(io.StringIO()):
            counts, quality = wt.convertBam("x.bam", binsize=binsize, minShift=min_shift, threshold=threshold)
        assert counts["1"].dtype == np.int32
        listed.append(name)
        rec[name + "_names"] = np.array(names)
        rec[name + "_lengths"] = np.array(lengths, dtype=np.int64)
        rec[name + "_pos"] = np.concatenate([reads[n][0] for n in names]).astype(np.int32)
        rec[name + "_mapq"] = np.concatenate([reads[n][1] for n in names]).astype(np.uint8)
        rec[name + "_offsets"] = np.concatenate([[0], np.cumsum([len(reads[n][0]) for n in names])]).astype(np.int64)
        rec[name + "_params"] = np.array([binsize, min_shift, threshold], dtype=np.float64)
        rec[name + "_present"] = np.array([counts[k] is not None for k in KEYS])
        rec[name + "_bins"] = np.array([0 if counts[k] is None else len(counts[k]) for k in KEYS], dtype=np.int64)
        rec[name + "_counts"] = np.concatenate([counts[k] for k in KEYS if counts[k] is not None]).astype(np.int32)
        rec[name + "_quality"] = np.array([int(quality[k]) for k in QUALITY], dtype=np.int64)
    rec["cases"] = np.array(listed)
    rec["quality_keys"] = np.array(QUALITY)

    # toolConvert's file and toolReport's text
    name, names, lengths, reads, binsize, min_shift, threshold = cases()[0]
    pysam.AlignmentFile = lambda f, mode: FakeAlignmentFile(names, lengths, reads)
    tmp = tempfile.mkdtemp(prefix="wc_convert_")
    os.chdir(tmp)
    converted = "sample.npz"
    wt.getRuntime = lambda: {"version": "golden"}
    wc.getRuntime = wt.getRuntime
    with contextlib.redirect_stdout(io.StringIO()):
        wc.toolConvert(argparse.Namespace(infile="x.bam", outfile=converted, binsize=binsize, retdist=min_shift,
                                          retthres=threshold))
    back = np.load(converted, allow_pickle=True)
    rec["file_keys"] = np.array(sorted(back.files))
    rec["file_argument_keys"] = np.array(sorted(back["arguments"].item()))
    rec["file_sample_keys"] = np.array(sorted(back["sample"].item()))
    calls = np.array([[5.0, 10.0, 14.0, 6.25, 0.031], [9.0, 0.0, 3.0, -5.5, -0.012], [13.0, 40.0, 40.0, 7.0, 0.2]])
    result = "result.npz"
    np.savez_compressed(result, arguments={"infile": "sample.npz", "repeats": 5}, runtime={}, binsize=binsize,
                        results_calls=calls, threshold_z=np.float64(4.8204), asdef=np.float64(0.01234),
                        aasdef=np.float64(0.0594857))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        wc.toolReport(argparse.Namespace(testfile=converted, resultfile=result, mineffect=1.5))
    rec["report_text"] = np.array(buf.getvalue())
    rec["report_calls"] = calls
    rec["report_scalars"] = np.array([binsize, 4.8204, 0.01234, 0.0594857])
    np.savez_compressed(os.path.join(GOLD, "convert.npz"), **rec)
    print("wrote tests/golden/convert.npz: %d cases, %d bytes" % (len(listed), os.path.getsize(os.path.join(GOLD, "convert.npz"))))


if __name__ == "__main__":
    main()
