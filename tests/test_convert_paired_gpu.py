"""`convert`'s paired-end mode and mapping-quality floor on the GPU (csrc/convert.hip: k_cv_elig, k_cv_flags<true>,
k_cv_compact<true>) against the REAL convertBam(..., mapq, demandPair)'s recorded output
(tests/golden/convert_paired.npz) and against the numpy restatement (tests/convert_paired_restated.py): random streams,
the carry of the previous eligible read over segments, tiles and chromosomes, a few million reads, and BAM file ->
`convert -paired -mapq` -> .npz.  Counts and counters are integers: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import bam_writer_paired as bwp
import convert_paired_restated as cpr
import convert_restated as cr
from test_convert_cpu import golden_case
from test_convert_paired_cpu import COUNTERS, OTHER, PAIR, paired_case, paired_inputs, random_paired_stream, same_sample

pytestmark = pytest.mark.gpu
SWEEP = int(os.environ.get("WC_SWEEP", "1"))
KEYS = cr.KEYS
NAMES24 = ["chr%s" % k for k in KEYS]


def flat(cols, dtype):
    return np.ascontiguousarray(np.concatenate(cols) if len(cols) else np.zeros(0), dtype=dtype)


def processed(names, *per_ref):
    keep = [i for i, n in enumerate(names) if cr.chrom_key(n) is not None]
    return [[xs[i] for i in keep] for xs in (names,) + per_ref]


def tables(lengths, pos, binsize):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    bins = np.concatenate([[0], np.cumsum([cr.n_bins(l, binsize) for l in lengths])]).astype(np.int64)
    return offsets, bins


def run_ex(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired, with_pair_arrays=True):
    """wc_convert_reads_ex on host arrays (all names processed): (counts dict, stats[8])"""
    from wisecondor_amd import _lib
    lib = _lib.load()
    offsets, bins = tables(lengths, pos, binsize)
    p, q = flat(pos, np.int32), flat(mapq, np.uint8)
    f, m = flat(flag, np.uint16), flat(mate, np.int32)
    counts = np.full(int(bins[-1]) + 1, -5, dtype=np.int32)
    stats = np.full(8, -5, dtype=np.int64)
    _lib.check(lib.wc_convert_reads_ex(_lib.context(0), _lib.ptr(p), _lib.ptr(q), _lib.ptr(f) if with_pair_arrays else None,
                                       _lib.ptr(m) if with_pair_arrays else None, _lib.ptr(offsets), len(names),
                                       float(binsize), int(min_shift), int(threshold), int(min_mapq), int(paired),
                                       _lib.ptr(bins), _lib.ptr(counts), _lib.ptr(stats)))
    assert counts[-1] == -5                              # nothing written behind the last bin
    return {cr.chrom_key(n): counts[a:b] for n, a, b in zip(names, bins[:-1], bins[1:])}, stats


def run_ex_dev(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired):
    """wc_convert_reads_ex_dev on torch tensors (all names processed): (counts dict, stats[8])"""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    offsets, bins = tables(lengths, pos, binsize)
    dp, dq = torch.from_numpy(flat(pos, np.int32)).cuda(), torch.from_numpy(flat(mapq, np.uint8)).cuda()
    df = torch.from_numpy(flat(flag, np.uint16).view(np.int16)).cuda()
    dm = torch.from_numpy(flat(mate, np.int32)).cuda()
    counts = torch.full((int(bins[-1]) + 1,), -5, dtype=torch.int32, device="cuda")
    stats = torch.full((8,), -5, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.wc_convert_reads_ex_dev(_lib.context(0), ctypes.c_void_p(stream), ctypes.c_void_p(dp.data_ptr()),
                                           ctypes.c_void_p(dq.data_ptr()), ctypes.c_void_p(df.data_ptr()),
                                           ctypes.c_void_p(dm.data_ptr()), _lib.ptr(offsets), len(names), float(binsize),
                                           int(min_shift), int(threshold), int(min_mapq), int(paired), _lib.ptr(bins),
                                           ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(stats.data_ptr())))
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert c[-1] == -5
    return {cr.chrom_key(n): c[a:b] for n, a, b in zip(names, bins[:-1], bins[1:])}, stats.cpu().numpy()


def stats_of(quality):
    return [quality[k] for k in ("filter_rmdup", "filter_mapq", "pre_retro", "post_retro")]


def check(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired, want=None, dev=True):
    """the library's two entry points and the Python mirror against `want` (default: the restatement)"""
    from wisecondor_amd import wisetools as wt
    if want is None:
        want = cpr.convert(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired)
    counts, quality = want
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    got, got_stats = wt.convertReads(names, lengths, offsets, flat(pos, np.int32), flat(mapq, np.uint8), binsize, min_shift,
                                     threshold, flag=flat(flag, np.uint16), mate_pos=flat(mate, np.int32),
                                     minMapq=min_mapq, demandPair=paired)
    same_sample(got, counts)
    for key in COUNTERS:
        assert got_stats[key] == quality[key], key
    sub = processed(names, lengths, pos, mapq, flag, mate)
    kept = sum(int(v.sum()) for v in counts.values() if v is not None)
    for run in (run_ex, run_ex_dev) if dev else (run_ex,):
        dgot, dstats = run(*sub, binsize, min_shift, threshold, min_mapq, paired)
        for key, arr in dgot.items():
            assert np.array_equal(arr, counts[key]), (run.__name__, key)
        assert [int(v) for v in dstats[:5]] == stats_of(quality) + [0], run.__name__
        assert int(dstats[6]) == quality["pair_fail"] and int(dstats[7]) == 0 and int(dstats[3]) == kept, run.__name__
        assert int(dstats[5]) == quality["pre_retro"] - quality["filter_rmdup"] - quality["filter_mapq"], run.__name__


def test_every_golden_case(golden):
    g = golden("convert_paired.npz")
    names, lengths, pos, mapq, flag, mate = paired_inputs(g)
    for name in g["cases"]:
        binsize, min_shift, threshold, min_mapq, paired, counts, quality = paired_case(g, str(name))
        check(names, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired, want=(counts, quality))


def test_ex_with_mapq_1_unpaired_is_wc_convert_reads(golden):
    from wisecondor_amd import _lib
    lib = _lib.load()
    g = golden("convert.npz")
    for name in g["cases"]:
        names, lengths, pos, mapq, binsize, min_shift, threshold, counts, quality = golden_case(g, str(name))
        names, lengths, pos, mapq = processed(names, lengths, pos, mapq)
        nothing = [np.zeros(len(p), dtype=np.int64) for p in pos]
        for with_arrays in (False, True):                # flag / mate_pos may be NULL when demand_pair == 0
            got, stats = run_ex(names, lengths, pos, mapq, nothing, nothing, binsize, min_shift, threshold, 1, 0, with_arrays)
            offsets, bins = tables(lengths, pos, binsize)
            old = np.zeros(int(bins[-1]), dtype=np.int32)
            old_stats = np.zeros(8, dtype=np.int64)
            _lib.check(lib.wc_convert_reads(_lib.context(0), _lib.ptr(flat(pos, np.int32)), _lib.ptr(flat(mapq, np.uint8)),
                                            _lib.ptr(offsets), len(names), float(binsize), int(min_shift), int(threshold),
                                            _lib.ptr(bins), _lib.ptr(old), _lib.ptr(old_stats)))
            assert np.array_equal(np.concatenate([got[cr.chrom_key(n)] for n in names]), old)
            assert np.array_equal(stats, old_stats) and stats[6] == 0
            assert [int(v) for v in stats[:4]] == stats_of(quality)
            for n in names:
                assert np.array_equal(got[cr.chrom_key(n)], counts[cr.chrom_key(n)])


def test_paired_mode_without_the_arrays_is_an_argument_error():
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    pos, mapq = [np.array([5, 100, 2500])], [np.full(3, 60)]
    with pytest.raises(_lib.WisecondorHipError) as e:
        run_ex(["chr1"], [3000], pos, mapq, pos, pos, 1000.0, 4, 4, 1, 1, with_pair_arrays=False)
    assert e.value.code == _lib.E_ARG and "paired" in str(e.value)
    with pytest.raises(ValueError):
        wt.convertReads(["chr1"], [3000], [0, 3], pos[0], mapq[0], 1000.0, demandPair=True)


@pytest.mark.parametrize("min_mapq", [-3, 0, 1, 20, 255, 256, 1000])
def test_any_mapq_floor(min_mapq):
    rng = np.random.RandomState(5)
    p, q, f, m = random_paired_stream(rng, 90000, 6000, 0.7)
    q[::5] = 255
    for paired in (False, True):
        check(["chr1"], [90000], [p], [q], [f], [m], 1000.0, 4, 4, min_mapq, paired, dev=False)


@pytest.mark.parametrize("seed", range(6 * SWEEP))
def test_random_streams_24_chromosomes(seed):
    """24 chromosomes with the carry, empty and one-read chromosomes among them, eligible shares from 0 to 1."""
    rng = np.random.RandomState(500 + seed)
    lengths = [int(rng.randint(20000, 300000)) for _ in NAMES24]
    cols = []
    for c, length in enumerate(lengths):
        kind = rng.randint(0, 8)
        n = 0 if kind == 0 else 1 if kind == 1 else int(rng.randint(2, 6000))
        share = float(rng.choice([0.0, 0.02, 0.1, 0.5, 0.9, 1.0]))
        towers = [(int(rng.randint(0, length)), int(rng.randint(2, 9)), int(rng.randint(0, 6))) for _ in range(n // 50)]
        if n > 1:
            cols.append(random_paired_stream(rng, length, n, share, towers))
        else:
            cols.append((rng.randint(0, length, n), np.full(n, 60), np.full(n, PAIR), rng.randint(0, length, n)))
    pos, mapq, flag, mate = ([c[i] for c in cols] for i in range(4))
    binsize = float(rng.choice([100.0, 333.0, 1000.0, 777.25, 1e6]))
    min_shift, threshold = int(rng.choice([-1, 0, 1, 4, 10])), int(rng.choice([-1, 0, 1, 4, 7, 3000]))
    min_mapq = int(rng.choice([0, 1, 20, 61]))
    check(NAMES24, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, True)
    check(NAMES24, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, False, dev=False)


def test_the_carry_over_segments_tiles_and_chromosomes():
    """Two reads with equal (pos, mate) and nothing but ineligible reads between them: a duplicate, however long the
    run (longer than a segment, a tile, three tiles) and wherever the tile boundary falls between the two; the same
    pair with another mate is none.  Then the pair across a chromosome boundary that is a tile boundary."""
    from wisecondor_amd import _lib
    tile = _lib.load().wc_convert_tile_reads()
    assert tile >= 64 and tile % 64 == 0
    for offset in (-1, 0, 1):
        flag, mate, expect_dups = [0x0], [7], 0          # the consumed first read
        for j, gap in enumerate([0, 1, 63, 64, 65, 100, tile - 1, tile, tile + 1, 3 * tile + 5, 2 * tile, 70] * 2):
            # the second read of the pair lands on a multiple of the tile size plus `offset` (where there is room)
            at = len(flag) + 1 + gap
            pad = (-(at - offset)) % tile if j % 2 else 0
            flag += [OTHER[k % len(OTHER)] for k in range(pad)]
            mate += list(range(pad))
            equal = j % 3 != 2
            flag += [PAIR] + [OTHER[k % len(OTHER)] for k in range(gap)] + [PAIR]
            mate += [1000 + j] + [1000 + j] * gap + [1000 + j if equal else 999]
            expect_dups += int(equal)
            if j % 2:
                assert (len(flag) - 1 - offset) % tile == 0
        n = len(flag)
        assert n > 12 * tile
        pos = np.full(n, 4321, dtype=np.int64)           # one position: only the mates decide
        pos[0] = 0
        flag, mate = np.array(flag), np.array(mate)
        mapq = np.full(n, 60)
        want = cpr.convert(["chr1"], [10000], [pos], [mapq], [flag], [mate], 1000.0, 4, -1, 1, True)
        assert want[1]["filter_rmdup"] == expect_dups and want[1]["pair_fail"] == int((flag[1:] != PAIR).sum())
        check(["chr1"], [10000], [pos], [mapq], [flag], [mate], 1000.0, 4, -1, 1, True, want=want)
        check(["chr1"], [10000], [pos], [mapq], [flag], [mate], 1000.0, 4, 4, 1, True)
    # two chromosomes, the second one starting exactly at a tile boundary: the last read of the first and the second
    # read of the second are the equal pair; then the same with three tiles of ineligible reads and an empty and a
    # one-read chromosome between them
    for middle in (0, 3 * tile):
        n1 = 2 * tile
        pos1 = np.sort(np.random.RandomState(1).randint(0, 9000, n1))
        flag1 = np.where(np.arange(n1) % 3 == 0, PAIR, 0x1)
        flag1[-1] = PAIR
        mate1 = np.arange(n1) + 50
        pos2 = np.concatenate([[0], np.full(middle, 10), np.full(40, pos1[-1])])
        flag2 = np.concatenate([[PAIR], np.full(middle, 0x83), np.full(40, PAIR)])
        mate2 = np.concatenate([[mate1[-1]], np.arange(middle), [mate1[-1], mate1[-1], 5], np.arange(37) // 2])
        names = ["chr1", "chr2", "chr3", "chr4"]
        cols = [(pos1, flag1, mate1), (np.zeros(0, int),) * 3, (np.array([pos1[-1]]), np.array([PAIR]), np.array([mate1[-1]])),
                (pos2, flag2, mate2)]
        pos, flag, mate = ([c[i] for c in cols] for i in range(3))
        mapq = [np.full(len(p), 60) for p in pos]
        lengths = [10000] * 4
        want = cpr.convert(names, lengths, pos, mapq, flag, mate, 1000.0, 4, -1, 1, True)
        assert want[0]["4"].sum() == 1 + 19 and want[1]["filter_rmdup"] >= 2 + 18 and want[1]["pair_fail"] == int((flag1[1:] != PAIR).sum()) + middle
        check(names, lengths, pos, mapq, flag, mate, 1000.0, 4, -1, 1, True, want=want)


def test_millions_of_reads_and_repeatability():
    """>= 4 million reads in paired mode: the carry crosses many workgroups; the same call twice gives identical output."""
    rng = np.random.RandomState(11)
    lengths = [150_000_000, 90_000_000, 60_000_000]
    cols = []
    for length, n, share in zip(lengths, (2_000_000, 1_400_000, 700_000), (0.6, 0.97, 0.001)):
        p = rng.randint(0, length, n)
        towers = [int(a) + np.arange(int(k)) for a, k in zip(rng.randint(0, length - 20000, 300), rng.choice([3, 4, 5, 6, 9000], 300))]
        p = np.sort(np.concatenate([p, p[::9]] + towers))
        q = np.where(rng.rand(len(p)) < 0.1, 0, rng.choice([20, 60], len(p)))
        f = np.where(rng.rand(len(p)) < share, PAIR, 0x83)
        m = p + rng.randint(-2, 3, len(p)) * 100
        cols.append((p, q, f, m))
    pos, mapq, flag, mate = ([c[i] for c in cols] for i in range(4))
    assert sum(len(p) for p in pos) >= 4_000_000
    names = ["chr1", "chr2", "chrX"]
    want = cpr.convert(names, lengths, pos, mapq, flag, mate, 50000.0, 4, 4, 20, True)
    assert want[1]["filter_rmdup"] > 10000 and want[1]["pair_fail"] > 1_000_000
    check(names, lengths, pos, mapq, flag, mate, 50000.0, 4, 4, 20, True, want=want)
    first = run_ex(names, lengths, pos, mapq, flag, mate, 50000.0, 4, 4, 20, 1)
    second = run_ex(names, lengths, pos, mapq, flag, mate, 50000.0, 4, 4, 20, 1)
    assert np.array_equal(first[1], second[1])
    for key in first[0]:
        assert np.array_equal(first[0][key], second[0][key])
        assert np.array_equal(first[0][key], want[0][key])


def _paired_bam(path, seed):
    rng = np.random.RandomState(seed)
    refs = [("chr%s" % k, 2_000_000 + 100_000 * i) for i, k in enumerate(KEYS)] + [("chrM", 16571)]
    cols = [random_paired_stream(rng, length, 1200 + 10 * r, 0.7, [(length // 2, 6, 1)]) for r, (_, length) in enumerate(refs)]
    per = [[c[i] for c in cols] for i in range(4)]
    bwp.write_bam(path, refs, bwp.records_of(list(range(len(refs))), *per, unplaced=7), seed=seed)
    return (refs,) + tuple(per)


def test_paired_bam_to_file_through_the_cli(tmp_path):
    from wisecondor_amd import ingest
    from wisecondor_amd import wisecondor as cli
    from wisecondor_amd import wisetools as wt
    bams = []
    for i in range(3):
        path = str(tmp_path / ("p%d.bam" % i))
        bams.append((path,) + _paired_bam(path, 70 + i))
    outs = []
    for path, refs, pos, mapq, flag, mate in bams:
        out = path[:-4] + "_single.npz"
        cli.main(["convert", path, out, "-binsize", "50000", "-paired", "-mapq", "20"])
        outs.append(out)
        names, lengths = [n for n, _ in refs], [l for _, l in refs]
        want, stats = cpr.convert(names, lengths, pos, mapq, flag, mate, 50000.0, 4, 4, 20, True)
        assert stats["pair_fail"] > 0 and stats["filter_mapq"] > 0
        sample, own = ingest.read_sample(out)
        assert own == 50000.0
        same_sample(sample, want)
        back = np.load(out, allow_pickle=True)
        quality, arguments = back["quality"].item(), back["arguments"].item()
        assert quality["no_coordinate"] == 7 and quality["unmapped"] == 7
        for key in COUNTERS:
            assert quality[key] == stats[key], key
        assert arguments["mapq"] == 20 and arguments["paired"] is True and arguments["retdist"] == 4
        mirror, mirror_quality = wt.convertBam(path, binsize=50000.0, mapq=20, demandPair=True)
        same_sample(mirror, want)
        assert mirror_quality == quality
        sizes = [len(want[str(c)]) for c in range(1, 23)]
        rows = np.full((1, sum(sizes)), -1, dtype=np.int32)
        slow = []
        ingest.read_counts([out], sizes, 50000.0, rows, threads=2, fallbacks=slow)
        assert slow == [] and np.array_equal(rows[0], np.concatenate([want[str(c)] for c in range(1, 23)]))
    # convertbatch with the same options: the same arrays per file
    outdir = str(tmp_path / "batch")
    cli.main(["convertbatch"] + [b[0] for b in bams] + [outdir, "-binsize", "50000", "-io", "3", "-paired", "-mapq", "20"])
    for b, single in zip(bams, outs):
        one = np.load(single, allow_pickle=True)
        two = np.load(os.path.join(outdir, os.path.basename(b[0])[:-4] + ".npz"), allow_pickle=True)
        sa, sb = one["sample"].item(), two["sample"].item()
        for key in KEYS:
            assert sa[key].dtype == sb[key].dtype and sa[key].tobytes() == sb[key].tobytes()
        assert one["quality"].item() == two["quality"].item()
        args = two["arguments"].item()
        assert args["infile"] == b[0] and args["mapq"] == 20 and args["paired"] is True
    # without the options: neither key in the file, and the plain mode's numbers
    path, refs, pos, mapq, flag, mate = bams[0]
    plain_out = str(tmp_path / "plain.npz")
    cli.main(["convert", path, plain_out, "-binsize", "50000"])
    back = np.load(plain_out, allow_pickle=True)
    assert "mapq" not in back["arguments"].item() and "paired" not in back["arguments"].item()
    want, stats = cr.convert([n for n, _ in refs], [l for _, l in refs], pos, mapq, 50000.0, 4, 4)
    same_sample(back["sample"].item(), want)
    assert back["quality"].item()["pair_fail"] == 0 and back["quality"].item()["pre_retro"] == stats["pre_retro"]
