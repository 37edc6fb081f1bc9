"""`convert`'s paired-end mode and mapping-quality floor without a GPU: the numpy restatement
(tests/convert_paired_restated.py) against what the REAL convertBam(..., mapq, demandPair) returned
(tests/golden/convert_paired.npz, made by tools/make_convert_paired_golden.py) and, in plain mode at mapq 1, against
the restatement of the merged `convert`; the native reader's flag words and mate positions; the two new options of
the command line."""
import numpy as np
import pytest

import bam_writer as bw
import bam_writer_paired as bwp
import convert_paired_restated as cpr
import convert_restated as cr

KEYS = cr.KEYS
COUNTERS = ("filter_rmdup", "filter_mapq", "pre_retro", "post_retro", "pair_fail")
PAIR = 0x43
OTHER = (0x0, 0x1, 0x41, 0x83, 0x2, 0x40, 0xA3)


def paired_inputs(g):
    """(names, lengths, pos, mapq, flag, mate_pos per reference): the same reads for every case of the file"""
    offs = g["offsets"]
    split = lambda a: [a[lo:hi] for lo, hi in zip(offs[:-1], offs[1:])]
    return ([str(n) for n in g["names"]], [int(v) for v in g["lengths"]], split(g["pos"]), split(g["mapq"]),
            split(g["flag"]), split(g["mate_pos"]))


def paired_case(g, name):
    """(binsize, min_shift, threshold, mapq, demandPair, counts dict, quality dict) the reference returned"""
    binsize, min_shift, threshold, mapq, paired = g[name + "_params"]
    counts, at = {}, 0
    for key, present, bins in zip(KEYS, g[name + "_present"], g[name + "_bins"]):
        counts[key] = g[name + "_counts"][at:at + bins] if present else None
        at += int(bins) if present else 0
    quality = dict(zip([str(k) for k in g["quality_keys"]], [int(v) for v in g[name + "_quality"]]))
    return float(binsize), int(min_shift), int(threshold), int(mapq), bool(paired), counts, quality


def same_sample(got, want):
    for key in KEYS:
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key] is not None and got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key


def test_restatement_equals_the_reference(golden):
    g = golden("convert_paired.npz")
    names, lengths, pos, mapq, flag, mate = paired_inputs(g)
    assert len(g["cases"]) >= 12
    for name in g["cases"]:
        binsize, min_shift, threshold, min_mapq, paired, counts, quality = paired_case(g, str(name))
        got, stats = cpr.convert(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired)
        same_sample(got, counts)
        for key in COUNTERS:
            assert stats[key] == quality[key], (name, key)


def test_golden_covers_what_it_should(golden):
    g = golden("convert_paired.npz")
    names, lengths, pos, mapq, flag, mate = paired_inputs(g)
    params = [tuple(g[str(c) + "_params"]) for c in g["cases"]]
    assert {(q, p) for _, _, _, q, p in params} >= {(q, p) for q in (0, 1, 30, 61) for p in (0, 1)}
    assert {t for _, _, t, _, p in params if p} >= {-1, 4} and {m for _, m, _, _, p in params if p} >= {0, 4, 10}
    elig = [((f[1:] & 0x42) == 0x42) for f in flag]
    share = {n: (e.mean() if len(e) else None) for n, e in zip(names, elig)}
    assert share["chr1"] == 1.0 and 0.3 < share["2"] < 0.7 and 0 < share["CHR3"] < 0.1 and share["chr4"] == 0.0
    assert "chrM" in names and names.index("chr1") + 2 == names.index("2") and len(pos[names.index("Y")]) == 1
    assert (np.concatenate(mate) == -1).any()
    # the equal pairs across chromosome boundaries: over the skipped chrM, directly, and over a chromosome (chr4)
    # without eligible reads plus a run of ineligible ones
    for a, b, at in (("chr1", "2", 1), ("chr10", "chr11", 1), ("CHR3", "6", 120)):
        i, j = names.index(a), names.index(b)
        assert (pos[i][-1], mate[i][-1]) == (pos[j][at], mate[j][at]) and elig[i][-1] and elig[j][at - 1]
        assert not elig[j][:at - 1].any()
    # same position, different mate; equal pair behind a run of ineligible reads; a partly ineligible tower
    one = names.index("chr1")
    assert pos[one][40] == pos[one][41] and mate[one][40] != mate[one][41]
    two = names.index("2")
    assert (pos[two][60], mate[two][60]) == (pos[two][70], mate[two][70]) and not elig[two][60:69].any()
    six = names.index("6")
    assert pos[six][204] - pos[six][200] <= 4 and elig[six][199:204].sum() == 3
    # ... and every one of them shows in the reference's own counters
    by = {str(c): paired_case(g, str(c)) for c in g["cases"]}
    paired, plain = by["paired_mapq_1"][6], by["plain_mapq_1"][6]
    assert by["paired_defaults"][6] == paired
    assert paired["pair_fail"] == sum(int((~e).sum()) for n, e in zip(names, elig) if cr.chrom_key(n)) > 0
    assert plain["pair_fail"] == 0 and plain["pre_retro"] == paired["pre_retro"] + paired["pair_fail"]
    assert plain["filter_rmdup"] != paired["filter_rmdup"]
    assert by["paired_mapq_0"][6]["filter_mapq"] == 0 and by["plain_mapq_0"][6]["filter_mapq"] == 0
    assert by["paired_mapq_61"][6]["post_retro"] == 0 and by["plain_mapq_61"][6]["post_retro"] == 0
    assert by["paired_mapq_30"][6]["filter_mapq"] > paired["filter_mapq"] > 0


def random_paired_stream(rng, length, n, p_pair, towers=()):
    p = rng.randint(0, length, n)
    extra = p[rng.rand(n) < 0.15]
    p = np.concatenate([p, extra, extra[:len(extra) // 2]] + [a + s * np.arange(k) for a, k, s in towers])
    p = np.sort(p[(p >= 0) & (p < length)])
    q = np.where(rng.rand(len(p)) < 0.1, 0, rng.choice([1, 19, 20, 60], len(p)))
    f = np.where(rng.rand(len(p)) < p_pair, PAIR, rng.choice(OTHER, len(p)))
    m = rng.randint(0, length, len(p))
    same = rng.rand(len(p)) < 0.5
    m[1:][same[1:]] = m[:-1][same[1:]]
    m[rng.rand(len(p)) < 0.02] = -1
    return p, q, f, m


@pytest.mark.parametrize("seed", range(8))
def test_plain_mode_at_mapq_1_is_the_merged_restatement(seed):
    rng = np.random.RandomState(300 + seed)
    names = ["chr%s" % k for k in KEYS[:6]] + ["chrM", "chrX"]
    lengths = [int(rng.randint(20000, 90000)) for _ in names]
    cols = [random_paired_stream(rng, l, [0, 1, 700, 1500][rng.randint(0, 4)], rng.rand(), [(l // 2, 6, 1)]) for l in lengths]
    pos, mapq, flag, mate = ([c[i] for c in cols] for i in range(4))
    min_shift, threshold = int(rng.choice([-1, 0, 4, 10])), int(rng.choice([-1, 0, 1, 4]))
    want = cr.convert(names, lengths, pos, mapq, 777.25, min_shift, threshold)
    got = cpr.convert(names, lengths, pos, mapq, flag, mate, 777.25, min_shift, threshold, 1, False)
    same_sample(got[0], want[0])
    assert got[1] == want[1]
    # and the paired mode is the plain mode of the eligible reads alone, where only the position can differ
    # (every mate equal): each chromosome's consumed first read stays in front
    sub = [np.concatenate([[True], (f[1:] & 0x42) == 0x42]) if len(f) else np.zeros(0, bool) for f in flag]
    zeros = [np.zeros(len(p), dtype=np.int64) for p in pos]
    paired = cpr.convert(names, lengths, pos, mapq, flag, zeros, 777.25, min_shift, threshold, 1, True)
    plain = cr.convert(names, lengths, [p[s] for p, s in zip(pos, sub)], [q[s] for q, s in zip(mapq, sub)], 777.25,
                       min_shift, threshold)
    same_sample(paired[0], plain[0])
    assert {k: v for k, v in paired[1].items() if k != "pair_fail"} == {k: v for k, v in plain[1].items() if k != "pair_fail"}


REFS = [("chr1", 50000), ("chrM", 16571), ("2", 40000), ("GL000207.1", 4262), ("chrX", 30000), ("chrY", 9000)]


def _paired_reads(seed, n=2500):
    rng = np.random.RandomState(seed)
    ids, cols = [], []
    for r, (_, length) in enumerate(REFS):
        if r == 3:
            continue                                    # a reference without reads
        ids.append(r)
        p, q, f, m = random_paired_stream(rng, length, 1 if r == 5 else n + 17 * r, 0.6)
        f = np.where(rng.rand(len(p)) < 0.1, rng.randint(0, 1 << 12, len(p)) & ~0x4, f)       # any flag word is kept
        cols.append((p, q, f, m))
    return ids, cols


@pytest.mark.parametrize("seed", range(4))
def test_reader_returns_the_flags_and_mate_positions_that_were_written(tmp_path, seed):
    from wisecondor_amd import wisetools as wt
    ids, cols = _paired_reads(seed)
    recs = bwp.records_of(ids, *[[c[i] for c in cols] for i in range(4)], unplaced=6)
    path = str(tmp_path / "a.bam")
    bwp.write_bam(path, REFS, recs, seed=50 + seed)                 # BGZF cuts at arbitrary bytes
    with wt.BamReads(path, threads=1 + seed) as bam:
        assert bam.flag.dtype == np.uint16 and bam.mate_pos.dtype == np.int32
        assert len(bam.flag) == len(bam.mate_pos) == len(bam.pos) == sum(len(c[0]) for c in cols)
        for r in range(len(REFS)):
            a, b = int(bam.offsets[r]), int(bam.offsets[r + 1])
            if r in ids:
                p, q, f, m = cols[ids.index(r)]
                assert np.array_equal(bam.pos[a:b], p) and np.array_equal(bam.mapq[a:b], q)
                assert np.array_equal(bam.flag[a:b], f) and np.array_equal(bam.mate_pos[a:b], m)
            else:
                assert a == b
        assert bam.no_coordinate == 6 and bam.unmapped == 6
        assert bam.mapped == len(bam.pos)
    bam.close()
    assert bam.flag is None and bam.mate_pos is None


def test_reader_without_placed_records_has_empty_arrays(tmp_path):
    from wisecondor_amd import wisetools as wt
    path = str(tmp_path / "a.bam")
    bwp.write_bam(path, REFS, [(-1, -1, 0, 0x4, -1)])
    with wt.BamReads(path) as bam:
        assert len(bam.flag) == 0 and len(bam.mate_pos) == 0
        assert bam.flag.dtype == np.uint16 and bam.mate_pos.dtype == np.int32


def test_damaged_paired_file_is_a_format_error(tmp_path):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    ids, cols = _paired_reads(9, n=800)
    data = bwp.plain_bam(REFS, bwp.records_of(ids, *[[c[i] for c in cols] for i in range(4)], unplaced=2))
    good = bw.bgzf(data, list(range(5000, len(data), 5000)))
    path = str(tmp_path / "bad.bam")
    blob = bytearray(good)
    blob[len(good) // 2] ^= 0x55
    for bad in (bytes(blob), good[:len(good) // 2]):
        open(path, "wb").write(bad)
        with pytest.raises(_lib.WisecondorHipError) as e:
            wt.BamReads(path, threads=2)
        assert e.value.code == _lib.E_FORMAT and len(str(e.value)) > 30


def test_cli_options_are_absent_unless_given():
    from wisecondor_amd import wisecondor as cli
    p = cli.buildParser()
    for argv in (["convert", "in.bam", "out.npz"], ["convertbatch", "a.bam", "b.bam", "outdir"]):
        a = p.parse_args(argv)
        assert "mapq" not in vars(a) and "paired" not in vars(a)
        assert sorted(k for k in vars(a) if k not in ("infile", "outfile", "infiles", "outdir", "io", "func")) == \
            ["binsize", "retdist", "retthres"]
        a = p.parse_args(argv + ["-mapq", "20", "-paired"])
        assert a.mapq == 20 and a.paired is True
        a = p.parse_args(argv + ["-mapq", "0"])
        assert a.mapq == 0 and "paired" not in vars(a)
        a = p.parse_args(argv + ["-paired"])
        assert a.paired is True and "mapq" not in vars(a)
    with pytest.raises(SystemExit):
        p.parse_args(["convert", "in.bam", "out.npz", "-mapq", "high"])


def test_python_mirror_has_the_reference_names_and_defaults():
    import inspect
    from wisecondor_amd import wisetools as wt
    for fn in (wt.convertBam, wt.convertBamReads):
        sig = inspect.signature(fn).parameters
        assert sig["mapq"].default == 1 and sig["demandPair"].default is False
        assert list(sig)[-2:] == ["mapq", "demandPair"]
    sig = inspect.signature(wt.convertReads).parameters
    assert sig["minMapq"].default == 1 and sig["demandPair"].default is False and sig["flag"].default is None
    assert list(sig)[:10] == ["names", "lengths", "offsets", "pos", "mapq", "binsize", "minShift", "threshold", "device",
                              "verbose"]
