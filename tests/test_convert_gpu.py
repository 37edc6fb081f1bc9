"""`convert` on the GPU (csrc/convert.hip) against the REAL convertBam's recorded output (tests/golden/convert.npz)
and against the numpy restatement (tests/convert_restated.py) on random streams; then BAM file -> `convert` ->
.npz -> both sample readers, `convertbatch` against `convert`, and a converted cohort through `newrefprep`.
Counts and counters are integers: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import bam_writer as bw
import convert_restated as cr
from test_convert_cpu import golden_case, same_sample

pytestmark = pytest.mark.gpu
SWEEP = int(os.environ.get("WC_SWEEP", "1"))
KEYS = cr.KEYS
NAMES24 = ["chr%s" % k for k in KEYS]


def flat(pos, mapq):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    p = np.concatenate(pos).astype(np.int32) if len(pos) else np.zeros(0, np.int32)
    q = np.concatenate(mapq).astype(np.uint8) if len(mapq) else np.zeros(0, np.uint8)
    return offsets, p, q


def run_host(names, lengths, pos, mapq, binsize, min_shift, threshold):
    from wisecondor_amd import wisetools as wt
    offsets, p, q = flat(pos, mapq)
    return wt.convertReads(names, lengths, offsets, p, q, binsize, min_shift, threshold)


def run_dev(names, lengths, pos, mapq, binsize, min_shift, threshold):
    """wc_convert_reads_dev on torch tensors (all names processed); returns (counts dict, stats[8])."""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    offsets, p, q = flat(pos, mapq)
    bins = np.concatenate([[0], np.cumsum([cr.n_bins(l, binsize) for l in lengths])]).astype(np.int64)
    dp, dq = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    counts = torch.full((int(bins[-1]) + 1,), -5, dtype=torch.int32, device="cuda")
    stats = torch.full((8,), -5, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.wc_convert_reads_dev(_lib.context(0), ctypes.c_void_p(stream), ctypes.c_void_p(dp.data_ptr()),
                                        ctypes.c_void_p(dq.data_ptr()), _lib.ptr(offsets), len(names), float(binsize),
                                        int(min_shift), int(threshold), _lib.ptr(bins), ctypes.c_void_p(counts.data_ptr()),
                                        ctypes.c_void_p(stats.data_ptr())))
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert c[-1] == -5                                   # nothing written behind the last bin
    return {cr.chrom_key(n): c[a:b] for n, a, b in zip(names, bins[:-1], bins[1:])}, stats.cpu().numpy()


def check(names, lengths, pos, mapq, binsize, min_shift, threshold, want=None, dev=True):
    if want is None:
        want = cr.convert(names, lengths, pos, mapq, binsize, min_shift, threshold)
    counts, stats = want
    got, got_stats = run_host(names, lengths, pos, mapq, binsize, min_shift, threshold)
    same_sample(got, counts)
    for key in ("filter_rmdup", "filter_mapq", "pre_retro", "post_retro", "pair_fail"):
        assert got_stats[key] == stats[key], key
    if dev:
        keep = [i for i, n in enumerate(names) if cr.chrom_key(n) is not None]
        sub = lambda xs: [xs[i] for i in keep]
        dgot, dstats = run_dev(sub(names), sub(lengths), sub(pos), sub(mapq), binsize, min_shift, threshold)
        for key, arr in dgot.items():
            assert np.array_equal(arr, counts[key]), key
        assert [int(v) for v in dstats[:5]] == [stats["filter_rmdup"], stats["filter_mapq"], stats["pre_retro"],
                                                stats["post_retro"], 0]


def test_every_golden_case(golden):
    g = golden("convert.npz")
    for name in g["cases"]:
        names, lengths, pos, mapq, binsize, min_shift, threshold, counts, quality = golden_case(g, str(name))
        check(names, lengths, pos, mapq, binsize, min_shift, threshold, want=(counts, quality))


def random_stream(rng, length, n, towers=()):
    p = rng.randint(0, length, n)
    p = np.concatenate([p, p[rng.rand(n) < 0.05]] + [a + s * np.arange(k) for a, k, s in towers])
    p = np.sort(p[(p >= 0) & (p < length)])
    q = np.where(rng.rand(len(p)) < 0.1, 0, rng.choice([1, 20, 60], len(p)))
    return p, q


@pytest.mark.parametrize("seed", range(6 * SWEEP))
def test_random_streams_24_chromosomes(seed):
    """24 chromosomes with the larp carry, empty and one-read chromosomes among them, every parameter regime."""
    rng = np.random.RandomState(100 + seed)
    lengths = [int(rng.randint(20000, 300000)) for _ in NAMES24]
    pos, mapq = [], []
    for c, length in enumerate(lengths):
        kind = rng.randint(0, 8)
        n = 0 if kind == 0 else 1 if kind == 1 else int(rng.randint(2, 6000))
        towers = [(int(rng.randint(0, length)), int(rng.randint(2, 9)), int(rng.randint(0, 6))) for _ in range(n // 50)]
        p, q = random_stream(rng, length, n, towers) if n > 1 else (rng.randint(0, length, n), np.full(n, 60))
        pos.append(p)
        mapq.append(q)
    if len(pos[3]) > 1 and len(pos[2]) > 1 and pos[2][-1] < lengths[3]:
        pos[3] = np.sort(np.concatenate([[pos[2][-1], pos[2][-1]], pos[3][pos[3] >= pos[2][-1]]]))      # second read == larp
        mapq[3] = np.full(len(pos[3]), 60)
    binsize = float(rng.choice([100.0, 333.0, 1000.0, 777.25, 1e6]))
    check(NAMES24, lengths, pos, mapq, binsize, int(rng.choice([-1, 0, 1, 4, 10])), int(rng.choice([-1, 0, 1, 4, 7, 3000])))


def test_towers_across_tile_boundaries():
    """Runs that start, end and pass exactly at the kernels' tile and segment boundaries (in kept-read space), run
    lengths around the threshold on both sides, and one run longer than several tiles."""
    from wisecondor_amd import _lib
    tile = _lib.load().wc_convert_tile_reads()
    assert tile >= 64 and tile % 64 == 0
    for threshold, min_shift in ((4, 4), (tile, 1), (3 * tile + 5, 2), (0, 4), (-1, 4), (63, 0)):
        lengths_wanted = [max(1, threshold), threshold + 1, max(1, threshold - 1), 2, 5, 64, 65, tile, tile + 1]
        # in kept-read space: at every second tile boundary b (and the segment boundary 64 behind it) a run of a
        # wanted length that straddles it, ends at it or starts at it; single reads fill the gaps
        seq, at = [], 0
        for j, b in enumerate(sorted([2 * tile * t for t in range(1, 19)] + [2 * tile * t + 64 for t in range(1, 19)])):
            length = lengths_wanted[j % len(lengths_wanted)]
            start = (b - length // 2, b - length, b)[(j // len(lengths_wanted)) % 3]
            if start < at:
                continue
            seq += [1] * (start - at) + [length]
            at = start + length
        seq.append(3 * tile + 5)                         # a run longer than three tiles
        seq.append(3 * tile + 6)
        step = 1 if min_shift >= 1 else 0
        pos, x = [0], 10                                  # the consumed first read
        for length in seq:
            pos.extend(x + step * np.arange(length) if step else [x])
            x = pos[-1] + min_shift + 1 + 3
        pos = np.asarray(pos, dtype=np.int64)
        mapq = np.full(len(pos), 60)
        length = int(pos[-1]) + 10
        check(["chr1"], [length], [pos], [mapq], 1000.0, min_shift, threshold)
        # the same with mapq-0 reads and duplicates sprinkled in: kept space no longer equals read space
        rng = np.random.RandomState(threshold + 7)
        mapq2 = np.where(rng.rand(len(pos)) < 0.2, 0, 60)
        check(["chr1", "chr2"], [length, length], [pos, np.sort(np.concatenate([pos, pos[::7]]))],
              [mapq2, np.full(len(pos) + len(pos[::7]), 30)], 333.0, min_shift, threshold)


def test_five_million_reads_and_repeatability():
    """>= 5 million reads: runs cross many workgroups; the same call twice on one context gives identical output."""
    rng = np.random.RandomState(9)
    lengths = [150_000_000, 90_000_000, 60_000_000]
    pos, mapq = [], []
    for length, n in zip(lengths, (2_600_000, 1_700_000, 900_000)):
        p = rng.randint(0, length, n)
        towers = [int(a) + np.arange(int(k)) for a, k in zip(rng.randint(0, length - 20000, 300), rng.choice([3, 4, 5, 6, 9000], 300))]
        p = np.sort(np.concatenate([p] + towers))
        pos.append(p)
        mapq.append(np.where(rng.rand(len(p)) < 0.1, 0, 60))
    assert sum(len(p) for p in pos) >= 5_000_000
    names = ["chr1", "chr2", "chrX"]
    want = cr.convert(names, lengths, pos, mapq, 50000.0, 4, 4)
    check(names, lengths, pos, mapq, 50000.0, 4, 4, want=want)
    first = run_host(names, lengths, pos, mapq, 50000.0, 4, 4)
    second = run_host(names, lengths, pos, mapq, 50000.0, 4, 4)
    same_sample(second[0], first[0])
    assert first[1] == second[1]
    check(names, lengths, pos, mapq, 1e6, 2, 10000, dev=False)


def test_read_beyond_the_header_length_is_an_argument_error():
    from wisecondor_amd import _lib
    pos = [np.array([5, 100, 2500, 99999])]
    with pytest.raises(_lib.WisecondorHipError) as e:
        run_host(["chr1"], [3000], pos, [np.full(4, 60)], 1000.0, 4, 4)
    assert e.value.code == _lib.E_ARG and "beyond" in str(e.value)
    got, _ = run_host(["chr1"], [3000], [pos[0][:3]], [np.full(3, 60)], 1000.0, 4, 4)
    assert list(got["1"]) == [1, 0, 1, 0]


def _cohort_bam(path, seed, binsize_reads=40000):
    rng = np.random.RandomState(seed)
    refs = [("chr%s" % k, 2_000_000 + 100_000 * i) for i, k in enumerate(KEYS)] + [("chrM", 16571)]
    ids, pos, mapq = [], [], []
    for r, (_, length) in enumerate(refs):
        p, q = random_stream(rng, length, 1200 + 10 * r, [(length // 2, 6, 1)])
        ids.append(r)
        pos.append(p)
        mapq.append(q)
    bw.write_bam(path, refs, bw.records_of(ids, pos, mapq, unplaced=7), seed=seed)
    return refs, pos, mapq


def test_bam_to_file_through_the_cli(tmp_path):
    from wisecondor_amd import ingest
    from wisecondor_amd import wisecondor as cli
    bams = []
    for i in range(6):
        path = str(tmp_path / ("s%d.bam" % i))
        bams.append((path,) + _cohort_bam(path, 40 + i))
    outs = []
    for path, refs, pos, mapq in bams:
        out = path[:-4] + "_single.npz"
        cli.main(["convert", path, out, "-binsize", "50000"])
        outs.append(out)
        want, stats = cr.convert([n for n, _ in refs], [l for _, l in refs], pos, mapq, 50000.0, 4, 4)
        sample, own = ingest.read_sample(out)
        assert own == 50000.0
        same_sample(sample, want)
        back = np.load(out, allow_pickle=True)
        assert sorted(back.files) == ["arguments", "quality", "runtime", "sample"]
        quality = back["quality"].item()
        recs = bw.records_of(list(range(len(refs))), pos, mapq, 7)
        assert quality["no_coordinate"] == 7 and quality["unmapped"] == sum(1 for r in recs if r[3] & 4)
        assert quality["mapped"] == sum(1 for r in recs if r[0] >= 0 and not r[3] & 4)
        for key, value in stats.items():
            assert quality[key] == value, key
        assert back["arguments"].item()["retdist"] == 4 and back["arguments"].item()["binsize"] == 50000.0
        sizes = [len(want[str(c)]) for c in range(1, 23)]
        rows = np.full((1, sum(sizes)), -1, dtype=np.int32)
        slow = []
        ingest.read_counts([out], sizes, 50000.0, rows, threads=2, fallbacks=slow)
        assert slow == [] and np.array_equal(rows[0], np.concatenate([want[str(c)] for c in range(1, 23)]))
    # convertbatch: the same arrays per file
    outdir = str(tmp_path / "batch")
    cli.main(["convertbatch"] + [b[0] for b in bams] + [outdir, "-binsize", "50000", "-io", "3"])
    for (path, _, _, _), single in zip(bams, outs):
        a = np.load(single, allow_pickle=True)
        b = np.load(os.path.join(outdir, os.path.basename(path)[:-4] + ".npz"), allow_pickle=True)
        sa, sb = a["sample"].item(), b["sample"].item()
        for key in KEYS:
            assert sa[key].dtype == sb[key].dtype and sa[key].tobytes() == sb[key].tobytes()
        assert a["quality"].item() == b["quality"].item()
        assert b["arguments"].item()["infile"] == path
    # the converted cohort is what newrefprep eats
    prep = str(tmp_path / "cohort_prep.npz")
    cli.main(["newrefprep"] + outs + [prep])
    pz = np.load(prep, allow_pickle=True)
    assert pz["correctedData"].shape[1] == 6 and float(pz["binsize"]) == 50000.0
