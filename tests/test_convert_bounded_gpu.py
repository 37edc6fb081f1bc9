"""The bounded `convert` on the GPU: the resumable form (wc_convert_begin / feed / finish, the carry-in instances of the
kernels of csrc/convert.hip) against the unchanged whole call wc_convert_reads_ex and the numpy restatements, at every
cut of a small input, chosen straddles, tile and segment edges, the status word and the refusals; then the streamed
BAM route (wc_convert_bam_stream_dev, `convert -bounded`) against the whole-file device reader, its errors against
wc_bam_stream_dev's, and its memory against the file's length.  Integers throughout: every comparison is exact."""
import ctypes
import os
import struct

import numpy as np
import pytest

import bam_writer as bw
import bam_writer_paired as bwp
import convert_paired_restated as cpr
import convert_restated as cr
import test_bamstream_cpu as cpu
from test_convert_paired_cpu import COUNTERS, random_paired_stream, same_sample

pytestmark = pytest.mark.gpu
PAIR, OTHER = 0x43, 0x83
BINSIZE = 1000.0


# ------------------------------------------------------------------------------------------------ helpers
class Input(object):
    """Per-chromosome (pos, mapq, flag, mate) columns, the flat host arrays, and the same on the device."""

    def __init__(self, cols, lengths):
        import torch
        self.cols, self.lengths = cols, lengths
        self.sizes = [len(c[0]) for c in cols]
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n = int(self.starts[-1])
        cat = lambda i, dtype: np.ascontiguousarray(np.concatenate([np.asarray(c[i]) for c in cols]), dtype=dtype)
        self.host = (cat(0, np.int32), cat(1, np.uint8), cat(2, np.uint16), cat(3, np.int32))
        self.dev = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for a in self.host]
        self.bins = np.concatenate([[0], np.cumsum([cr.n_bins(l, BINSIZE) for l in lengths])]).astype(np.int64)

    def table(self, lo, hi):
        """the offsets table of the slice [lo, hi) of the concatenated reads"""
        return np.clip(self.starts - lo, 0, hi - lo).astype(np.int64)


def whole(inp, min_shift, threshold, min_mapq, paired):
    """wc_convert_reads_ex on the whole input: (rc, counts, stats)"""
    from wisecondor_amd import _lib
    lib = _lib.load()
    counts = np.full(int(inp.bins[-1]) + 1, -5, dtype=np.int32)
    stats = np.full(8, -5, dtype=np.int64)
    p, q, f, m = inp.host
    rc = lib.wc_convert_reads_ex(_lib.context(0), _lib.ptr(p), _lib.ptr(q), _lib.ptr(f), _lib.ptr(m), _lib.ptr(inp.starts),
                                 len(inp.cols), BINSIZE, int(min_shift), int(threshold), int(min_mapq), int(paired),
                                 _lib.ptr(inp.bins), _lib.ptr(counts), _lib.ptr(stats))
    assert counts[-1] == -5
    return rc, counts[:-1], stats


def begin(inp, min_shift, threshold, min_mapq, paired):
    from wisecondor_amd import _lib
    run = ctypes.c_void_p()
    _lib.check(_lib.load().wc_convert_begin(_lib.context(0), len(inp.cols), BINSIZE, int(min_shift), int(threshold),
                                            int(min_mapq), int(paired), _lib.ptr(inp.bins), ctypes.byref(run)))
    return run


def sliced_dev(inp, cuts, min_shift, threshold, min_mapq, paired):
    """The slices between `cuts` through wc_convert_feed_dev, nothing read back before the end: (counts, stats)"""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    run = begin(inp, min_shift, threshold, min_mapq, paired)
    try:
        edges = [0] + [int(c) for c in cuts] + [inp.n]
        for lo, hi in zip(edges[:-1], edges[1:]):
            ptrs = [ctypes.c_void_p(t.data_ptr() + lo * t.element_size()) for t in inp.dev]
            _lib.check(lib.wc_convert_feed_dev(run, None, ptrs[0], ptrs[1], ptrs[2], ptrs[3], _lib.ptr(inp.table(lo, hi))))
        counts = torch.full((int(inp.bins[-1]) + 1,), -5, dtype=torch.int32, device="cuda")
        stats = torch.full((8,), -5, dtype=torch.int64, device="cuda")
        _lib.check(lib.wc_convert_finish_dev(run, None, ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(stats.data_ptr())))
        torch.cuda.synchronize()
        c = counts.cpu().numpy()
        assert c[-1] == -5                              # nothing written behind the last bin
        return c[:-1], stats.cpu().numpy()
    finally:
        lib.wc_convert_end(run)


def sliced_host(inp, cuts, min_shift, threshold, min_mapq, paired):
    """The same through wc_convert_feed / wc_convert_finish: (rc of the first call that failed or 0, counts, stats)"""
    from wisecondor_amd import _lib
    lib = _lib.load()
    run = begin(inp, min_shift, threshold, min_mapq, paired)
    try:
        edges = [0] + [int(c) for c in cuts] + [inp.n]
        failed = 0
        for lo, hi in zip(edges[:-1], edges[1:]):
            arrays = [np.ascontiguousarray(a[lo:hi]) for a in inp.host]
            rc = lib.wc_convert_feed(run, *[_lib.ptr(a) for a in arrays], _lib.ptr(inp.table(lo, hi)))
            failed = failed or rc
        counts = np.full(int(inp.bins[-1]) + 1, -5, dtype=np.int32)
        stats = np.full(8, -5, dtype=np.int64)
        rc = lib.wc_convert_finish(run, _lib.ptr(counts), _lib.ptr(stats))
        assert counts[-1] == -5
        return failed or rc, counts[:-1], stats
    finally:
        lib.wc_convert_end(run)


def same(got, want):
    (counts, stats), (rc, want_counts, want_stats) = got, want
    assert rc == 0
    assert np.array_equal(counts, want_counts)
    assert [int(v) for v in stats[:7]] == [int(v) for v in want_stats[:7]]


def restated(inp, min_shift, threshold, min_mapq, paired):
    names = ["chr%s" % k for k in cr.KEYS[:len(inp.cols)]]
    pos, mapq, flag, mate = ([c[i] for c in inp.cols] for i in range(4))
    counts, stats = cpr.convert(names, inp.lengths, pos, mapq, flag, mate, BINSIZE, min_shift, threshold, min_mapq, paired)
    return np.concatenate([counts[cr.chrom_key(n)] for n in names]), stats


def against_restatement(want, inp, min_shift, threshold, min_mapq, paired):
    counts, stats = restated(inp, min_shift, threshold, min_mapq, paired)
    assert np.array_equal(want[1], counts)
    assert [int(v) for v in want[2][:4]] + [int(want[2][6])] == [stats[k] for k in COUNTERS]


def column(pos, mapq=None, flag=None, mate=None):
    pos = np.asarray(pos, dtype=np.int64)
    return (pos, np.full(len(pos), 60) if mapq is None else np.asarray(mapq),
            np.full(len(pos), PAIR) if flag is None else np.asarray(flag),
            np.arange(len(pos)) % 7 if mate is None else np.asarray(mate))


# ------------------------------------------------------------------------------------------------ 1. every cut
def small_input():
    """3 chromosomes of about 200 reads: duplicates, low mapping quality, ineligible reads, and towers of 1 .. 6 reads
    (threshold - 1, threshold and threshold + 1 for each threshold of the test) one base apart"""
    rng = np.random.RandomState(42)
    cols = []
    for c in range(3):
        pos = list(np.sort(rng.randint(0, 90000, 150)) + 100)
        for k in range(1, 7):
            pos += list(200000 + 1000 * (7 * c + k) + np.arange(k))
        pos = np.sort(np.array(pos + pos[10:40:3] + pos[11:12] * 2))
        n = len(pos)
        mapq = np.where(rng.rand(n) < 0.1, 0, 60)
        flag = np.where(rng.rand(n) < 0.8, PAIR, OTHER)
        mate = pos // 2                                 # equal positions have equal mates: duplicates in both modes
        cols.append((pos, mapq, flag, mate))
    return Input(cols, [300000] * 3)


@pytest.fixture(scope="module")
def small():
    return small_input()


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("min_shift", [0, 4])
@pytest.mark.parametrize("threshold", [-1, 0, 1, 4])
def test_every_cut_of_a_small_input(small, threshold, min_shift, paired):
    want = whole(small, min_shift, threshold, 1, paired)
    assert want[0] == 0 and want[2][0] > (3 if paired else 10) and want[2][1] > 10 and (want[2][6] > 50) == paired
    against_restatement(want, small, min_shift, threshold, 1, paired)
    for cut in range(small.n + 1):                      # both ends give an empty slice
        same(sliced_dev(small, [cut], min_shift, threshold, 1, paired), want)
    same(sliced_dev(small, list(range(1, small.n)), min_shift, threshold, 1, paired), want)      # slices of one read


# ------------------------------------------------------------------------------------------------ 2. chosen straddles
def check_cuts(inp, cut_sets, min_shift, threshold, min_mapq=1, modes=(False, True)):
    for paired in modes:
        want = whole(inp, min_shift, threshold, min_mapq, paired)
        assert want[0] == 0
        against_restatement(want, inp, min_shift, threshold, min_mapq, paired)
        for cuts in cut_sets:
            same(sliced_dev(inp, cuts, min_shift, threshold, min_mapq, paired), want)
    return want


def test_duplicates_first_reads_and_short_chromosomes_across_cuts():
    # chr1 ends with 500 500; chr2 has one read, chr3 none, chr4's second read repeats chr1's last (larp skips chr2, chr3)
    cols = [column([10, 20, 20, 300, 500, 500]), column([500]), column([]), column([7, 500, 500, 900, 900]),
            column([1]), column([5, 900, 901])]
    inp = Input(cols, [2000] * 6)
    starts = [int(s) for s in inp.starts]
    cuts = [[2], [3], [5], [6], [7], [8], [9], [6, 7], [7, 8], [5, 6, 7, 8, 9], [12], [12, 13], [13], [13, 14], [3, 3, 3]]
    want = check_cuts(inp, cuts, 0, -1, modes=(False,))
    assert int(want[2][0]) == 6         # 20, 500, chr4's 500 twice (larp, then its neighbour), 900, chr6's 900 (larp)
    assert starts[3] == 7 and starts[4] == 12
    check_cuts(inp, cuts, 4, 4)
    check_cuts(inp, cuts, 4, 1)


def test_a_tower_cut_at_each_inner_position_and_over_three_slices():
    tower = list(5000 + np.arange(6))
    cols = [column([1, 100, 2000] + tower + [9000, 9001]), column([3, 40, 41, 42, 43, 8000])]
    inp = Input(cols, [10000] * 2)
    first = 3
    cuts = [[first + k] for k in range(0, 8)] + [[first + 1, first + 3], [first + 2, first + 4], [first + 1, first + 5],
                                                 [first, first + 3, first + 6], [inp.sizes[0] + 2, inp.sizes[0] + 4]]
    for threshold in (4, 5, 6, 7):
        check_cuts(inp, cuts, 4, threshold)
    check_cuts(inp, cuts, 0, 4)                         # no two reads share a run


def test_a_tower_of_three_tiles_dead_and_pending():
    """The tower outgrows threshold 4 in its first slice and stays dead over the cuts; with the threshold at its length
    every one of its positions is carried until the read behind it closes the run -- and with one less none is counted."""
    from wisecondor_amd import _lib
    tile = _lib.load().wc_convert_tile_reads()
    n = 3 * tile
    tower = 1000 + np.arange(n)
    inp = Input([column(np.concatenate([[5, 40], tower, [n + 5000, n + 9000]]))], [n + 10000])
    cuts = [[2], [3], [tile], [tile + 2, 2 * tile + 2], [1, 2, 3, tile - 1, tile, tile + 1, 3 * tile + 1, 3 * tile + 2, 3 * tile + 3],
            [n + 2], [n + 3], list(range(64, n, 640))]
    want = check_cuts(inp, cuts, 4, 4, modes=(False,))
    assert int(want[2][3]) == 3 and int(want[2][5]) == n + 3
    want = check_cuts(inp, cuts, 4, n, modes=(False,))
    assert int(want[2][3]) == n + 3
    want = check_cuts(inp, cuts, 4, n - 1)
    assert int(want[2][3]) == 3


def test_paired_previous_read_lies_slices_back_and_across_a_chromosome():
    # eligible (7, 70); slices of ineligible reads only; then (7, 70) again: a duplicate.  Again across a chromosome change.
    k = 40
    pos1 = np.concatenate([[1, 7], np.full(k, 7), [7, 7]])
    flag1 = np.concatenate([[OTHER, PAIR], np.full(k, OTHER), [PAIR, PAIR]])
    mate1 = np.concatenate([[0, 70], np.arange(k), [70, 71]])
    pos2 = np.concatenate([[3], np.full(k, 7), [7, 7]])
    flag2 = np.concatenate([[PAIR], np.full(k, OTHER), [PAIR, PAIR]])
    mate2 = np.concatenate([[71], np.arange(k), [71, 70]])
    inp = Input([column(pos1, flag=flag1, mate=mate1), column([]), column([9], flag=[PAIR], mate=[71]),
                 column(pos2, flag=flag2, mate=mate2)], [1000] * 4)
    n1 = len(pos1)
    cuts = [[2, 2 + k // 2, 2 + k], [2, 12, 22, 32, 42], [n1 - 1], [n1], [n1 + 1], [n1 + 2, n1 + 2 + k // 2, n1 + 2 + k],
            [n1 - 1, n1 + 1, n1 + 2, n1 + 2 + k]]
    want = check_cuts(inp, cuts, 4, -1, modes=(True,))
    assert int(want[2][0]) == 2 and int(want[2][6]) == 2 * k          # both equal pairs are duplicates
    check_cuts(inp, cuts, 4, 4, modes=(True,))


# ------------------------------------------------------------------------------------------------ 3. tile and segment edges
def test_slices_at_segment_and_tile_edges():
    from wisecondor_amd import _lib
    tile = _lib.load().wc_convert_tile_reads()
    rng = np.random.RandomState(8)
    cols = []
    for n in (2 * tile + 300, 1, 0, 2 * tile + 77):
        towers = [(int(rng.randint(0, 500000)), int(rng.randint(2, 9)), 1) for _ in range(n // 40)]
        cols.append(random_paired_stream(rng, 500000, n, 0.8, towers) if n > 1 else column(rng.randint(0, 500000, n)))
    inp = Input(cols, [500000] * 4)
    assert inp.n > 4 * tile
    cut_sets = [list(np.cumsum([k] * 6)) for k in (63, 64, 65)]
    cut_sets += [list(np.cumsum([k] * 2)) for k in (tile - 1, tile, tile + 1)]
    cut_sets += [[3 * tile, 3 * tile + 1], [1, 3 * tile + 1]]
    check_cuts(inp, cut_sets, 4, 4, min_mapq=20)
    check_cuts(inp, cut_sets[3:], 1, 2, modes=(False,))


# ------------------------------------------------------------------------------------------------ 4. refusals, status word
def test_refusals_and_the_status_word():
    from wisecondor_amd import _lib
    lib = _lib.load()
    inp = Input([column([1, 10, 20]), column([2, 30, 40, 50])], [1000, 1000])
    run = begin(inp, 4, 4, 1, False)
    try:
        arrays = [_lib.ptr(a) for a in inp.host]
        late = [np.ascontiguousarray(a[3:]) for a in inp.host]
        assert lib.wc_convert_feed(run, *[_lib.ptr(a) for a in late], _lib.ptr(inp.table(3, 7))) == 0
        rc = lib.wc_convert_feed(run, *arrays, _lib.ptr(inp.table(0, 3)))      # back to the first chromosome
        assert rc == _lib.E_ARG and b"chromosome" in lib.wc_last_error()
        assert lib.wc_convert_feed(run, *arrays, _lib.ptr(np.array([1, 2, 3], dtype=np.int64))) == _lib.E_ARG
        assert lib.wc_convert_feed(run, *arrays, _lib.ptr(np.array([0, 2, 1], dtype=np.int64))) == _lib.E_ARG
    finally:
        lib.wc_convert_end(run)
    # a counted read beyond its chromosome's bins: the whole call's status word, WC_E_ARG from the host forms, counts untouched
    beyond = Input([column([1, 10, 20, 5000, 5001]), column([2, 30, 777777])], [1000, 1000])
    for paired in (False, True):
        rc, want_counts, want_stats = whole(beyond, 4, 4, 1, paired)
        assert rc == _lib.E_ARG and int(want_stats[4]) == 3
        for cuts in ([], [3], [4], [5, 6], [1, 2, 3, 4, 5, 6, 7]):
            counts, stats = sliced_dev(beyond, cuts, 4, 4, 1, paired)
            assert np.array_equal(counts, want_counts) and [int(v) for v in stats[:7]] == [int(v) for v in want_stats[:7]]
            rc, counts, stats = sliced_host(beyond, cuts, 4, 4, 1, paired)
            assert rc == _lib.E_ARG and b"beyond" in lib.wc_last_error()
            assert (counts == -5).all() and int(stats[4]) == 3


def test_host_and_device_feeds_give_the_same(small):
    for paired in (False, True):
        want = whole(small, 4, 4, 1, paired)
        for cuts in ([], [100], [64, 64, 300, 301]):
            rc, counts, stats = sliced_host(small, cuts, 4, 4, 1, paired)
            same((counts, stats), want)
            assert rc == 0 and int(stats[7]) == 0
            same(sliced_dev(small, cuts, 4, 4, 1, paired), want)


def test_convert_run_class(small):
    from wisecondor_amd import wisetools as wt
    names = ["chr1", "chrM", "chr2", "chr3"]
    cols = [small.cols[0], column([5, 6, 7]), small.cols[1], small.cols[2]]
    lengths = [300000, 16571, 300000, 300000]
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cols])])
    flat = [np.concatenate([np.asarray(c[i]) for c in cols]) for i in range(4)]
    for paired in (False, True):
        want, want_stats = wt.convertReads(names, lengths, offsets, flat[0], flat[1], BINSIZE, 4, 4, flag=flat[2],
                                           mate_pos=flat[3], demandPair=paired)
        with wt.ConvertRun(names, lengths, BINSIZE, 4, 4, demandPair=paired) as run:
            for lo, hi in ((0, 150), (150, 150), (150, 400), (400, int(offsets[-1]))):
                table = np.clip(offsets - lo, 0, hi - lo)
                run.feed(table, *[a[lo:hi] for a in flat])
            assert run.info()["slices"] == 3 and run.info()["carry_bound"] <= 4
            got, got_stats = run.finish()
        same_sample(got, want)
        assert got_stats == want_stats


# ------------------------------------------------------------------------------------------------ 5. from a BAM file
NAMES24 = ["chr%s" % k for k in cr.KEYS]


def _bam(path, seed, paired, n=160):
    """24 references and chrM between them, a few thousand reads, towers and duplicates everywhere: with one BGZF block
    per chunk the chunk cuts fall inside them"""
    rng = np.random.RandomState(seed)
    refs = [(name, 400000 + 1000 * i) for i, name in enumerate(NAMES24)]
    refs = refs[:5] + [("chrM", 16571)] + refs[5:]
    cols = []
    for r, (_, length) in enumerate(refs):
        k = 0 if r == 9 else 1 if r == 11 else n + 3 * r
        towers = [(int(rng.randint(0, length - 100)), int(rng.randint(2, 9)), 1) for _ in range(k // 12)]
        cols.append(random_paired_stream(rng, length, k, 0.8, towers) if k > 1 else
                    (rng.randint(0, length, k), np.full(k, 60), np.full(k, PAIR), rng.randint(0, length, k)))
    per = [[c[i] for c in cols] for i in range(4)]
    ids = list(range(len(refs)))
    if paired:
        bwp.write_bam(path, refs, bwp.records_of(ids, *per, unplaced=6), seed=seed)
    else:
        data = bw.plain_bam(refs, bw.records_of(ids, per[0], per[1], unplaced=6))
        open(path, "wb").write(bw.bgzf(data, list(range(1500, len(data), 1500))))
    return refs, per


@pytest.mark.parametrize("paired", [False, True])
def test_bam_file_at_every_chunk_size(tmp_path, monkeypatch, paired):
    from wisecondor_amd import wisetools as wt
    path = str(tmp_path / "b.bam")
    refs, per = _bam(path, 21 + paired, paired)
    kw = dict(binsize=50000.0, minShift=4, threshold=4, mapq=20, demandPair=paired)
    want, want_quality = wt.convertBam(path, **kw)      # the whole-file device reader
    names, lengths = [n for n, _ in refs], [l for _, l in refs]
    counts, stats = cpr.convert(names, lengths, per[0], per[1], per[2], per[3], 50000.0, 4, 4, 20, paired)
    same_sample(want, counts)
    for key in COUNTERS:
        assert want_quality[key] == stats[key], key
    assert want_quality["filter_rmdup"] > 100 and want_quality["no_coordinate"] == 6
    assert want_quality["pre_retro"] - want_quality["filter_rmdup"] - want_quality["filter_mapq"] > want_quality["post_retro"]
    for chunk in (1, 4096, 70000, 1 << 30):
        info = {}
        got, quality = wt.convertBamBounded(path, chunk=chunk, info=info, **kw)
        same_sample(got, want)
        assert quality == want_quality, chunk
        assert info["placed_records"] == sum(len(p) for p in per[0])
        assert info["largest_carry_positions"] <= 4
        if chunk == 1:
            assert info["chunks"] > 40 and info["largest_carry_positions"] >= 1
    monkeypatch.setattr(wt, "CONVERT_READER", "bounded")         # convertBam itself, by the reader choice
    monkeypatch.setattr(wt, "BAM_STREAM_CHUNK", 4096)
    got, quality = wt.convertBam(path, **kw)
    same_sample(got, want)
    assert quality == want_quality


def test_the_long_record_between_counted_reads(tmp_path):
    """The 225 042-byte record of tests/test_bamstream_gpu.py goes over several one-block chunks between counted reads."""
    from wisecondor_amd import wisetools as wt
    refs = [("chr1", 50000), ("chr2", 40000)]
    long_record = bw.record(0, 5, 30, l_seq=150000)
    assert len(long_record) == 225042
    tail = [bw.record(0, 10 + i // 2, 20, l_seq=i % 50) for i in range(3000)] + [bw.record(1, 7 * i, 60) for i in range(500)]
    data = bw.plain_bam(refs, []) + bw.record(0, 1, 1) + bw.record(0, 5, 30) + long_record + b"".join(tail)
    path = str(tmp_path / "long.bam")
    open(path, "wb").write(bw.bgzf(data, block=60000))
    want, want_quality = wt.convertBam(path, binsize=1000.0)
    assert want_quality["filter_rmdup"] == 1 + 1500 and want_quality["post_retro"] > 400
    for chunk in (1, 1 << 30):
        info = {}
        got, quality = wt.convertBamBounded(path, binsize=1000.0, chunk=chunk, info=info)
        same_sample(got, want)
        assert quality == want_quality
        if chunk == 1:
            assert info["chunks"] >= 5 and info["largest_carry_bytes"] >= 225042 - 60000


def _error(call):
    from wisecondor_amd import _lib
    with pytest.raises(_lib.WisecondorHipError) as e:
        call()
    return e.value.code, str(e.value)


def test_errors_are_the_streamed_readers(tmp_path):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    refs = [("chr1", 50000), ("chr2", 40000)]
    rng = np.random.RandomState(3)
    recs = [(0, 100 + 30 * i, 60, 0) for i in range(1500)]
    recs += [(1, int(p), 60, 0) for p in np.sort(rng.randint(0, 40000, 1500))]
    data = bw.plain_bam(refs, recs)
    head = len(bw.plain_bam(refs, []))
    where, at = [], head
    while at < len(data):
        where.append(at)
        at += 4 + struct.unpack("<i", data[at:at + 4])[0]
    cuts = list(range(5000, len(data), 5000))
    path = str(tmp_path / "bad.bam")
    for at in (where[0], where[len(where) // 2], where[-1]):           # the first, a middle and the last chunk
        bad = bytearray(data)
        bad[at + 4:at + 8] = struct.pack("<i", 99)
        open(path, "wb").write(bw.bgzf(bytes(bad), cuts))
        for chunk in (1, 4096):
            want = _error(lambda: wt.BamReadsStream(path, chunk=chunk))
            got = _error(lambda: wt.convertBamBounded(path, binsize=1000.0, chunk=chunk))
            assert got == want and got[0] == _lib.E_FORMAT and ("inflated offset %d " % at) in got[1]
    # an unsorted pair across a chunk cut
    unsorted = recs[:40] + [(0, recs[20][1], 60, 0)] + recs[40:]
    data = bw.plain_bam(refs, unsorted)
    offsets, at = [], head
    while at < len(data):
        offsets.append(at)
        at += 4 + struct.unpack("<i", data[at:at + 4])[0]
    for cut in ([offsets[40]], [offsets[40] - 3, offsets[40] + 2]):
        open(path, "wb").write(bw.bgzf(data, cut))
        want = _error(lambda: wt.BamReadsStream(path, chunk=1))
        got = _error(lambda: wt.convertBamBounded(path, binsize=1000.0, chunk=1))
        assert got == want and got[0] == _lib.E_ARG and "coordinate-sorted" in got[1]
    # a counted read beyond the header's length: WC_E_ARG as from the other routes
    open(path, "wb").write(bw.bgzf(bw.plain_bam(refs, recs[:1500] + [(0, 2000000, 60, 0)] + recs[1500:])))
    got = _error(lambda: wt.convertBamBounded(path, binsize=1000.0, chunk=1))
    assert got[0] == _lib.E_ARG and "beyond" in got[1]
    assert _error(lambda: wt.convertBam(path, binsize=1000.0))[0] == _lib.E_ARG


def test_memory_does_not_follow_the_length(tmp_path):
    """One file and one made the same way four times as long, at the same chunk size: both reserve by the same per-chunk
    rule, so the peak device bytes (everything) may differ by allocation granularity only: 1 MiB.  And the peak stays
    below the streamed handle's, which holds 11 bytes per read."""
    from wisecondor_amd import wisetools as wt
    chunk = 262144
    peaks = []
    for n in (12500, 50000):
        refs, recs = cpu.big_records(n)
        path = str(tmp_path / ("r%d.bam" % n))
        bw.write_bam(path, refs, recs)
        info = {}
        got, quality = wt.convertBamBounded(path, binsize=100000.0, chunk=chunk, info=info)
        assert info["placed_records"] == 4 * n and info["chunks"] >= 2
        with wt.BamReadsStream(path, chunk=chunk) as bam:
            want, want_quality = wt.convertBamReads(bam, binsize=100000.0)
            streamed_peak = bam.device_bytes
        same_sample(got, want)
        assert quality == want_quality
        print("records", 4 * n, "chunks", info["chunks"], "bounded peak", info["peak_device_bytes"], "streamed peak", streamed_peak)
        peaks.append((info["peak_device_bytes"], streamed_peak))
    assert peaks[1][0] <= peaks[0][0] + (1 << 20)
    assert peaks[1][0] < peaks[1][1]


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_bounded_through_the_cli(tmp_path):
    from wisecondor_amd import wisecondor as cli
    paths = [str(tmp_path / ("s%d.bam" % i)) for i in range(2)]
    for i, path in enumerate(paths):
        _bam(path, 50 + i, False)
    outs = {}
    for name, extra in (("plain", []), ("stream", ["-stream", "-chunk", "4096"]), ("bounded", ["-bounded", "-chunk", "4096"]),
                        ("bounded_default", ["-bounded"])):
        outs[name] = str(tmp_path / (name + ".npz"))
        cli.main(["convert", paths[0], outs[name], "-binsize", "50000"] + extra)
    loaded = {k: np.load(v, allow_pickle=True) for k, v in outs.items()}

    def same_file(a, b):
        sa, sb = a["sample"].item(), b["sample"].item()
        assert set(sa) == set(sb)
        for key in sa:
            assert sa[key].dtype == sb[key].dtype and sa[key].tobytes() == sb[key].tobytes()
        assert a["quality"].item() == b["quality"].item()

    for name in ("stream", "bounded", "bounded_default"):
        same_file(loaded["plain"], loaded[name])
    assert "bounded" not in loaded["plain"]["arguments"].item() and "bounded" not in loaded["stream"]["arguments"].item()
    args = loaded["bounded"]["arguments"].item()
    assert args["bounded"] is True and args["chunk"] == 4096 and "stream" not in args
    assert "chunk" not in loaded["bounded_default"]["arguments"].item()
    outdir = str(tmp_path / "batch")
    cli.main(["convertbatch"] + paths + [outdir, "-binsize", "50000", "-bounded", "-chunk", "4096"])
    batch = np.load(os.path.join(outdir, "s0.npz"), allow_pickle=True)
    same_file(loaded["bounded"], batch)
    assert batch["arguments"].item()["bounded"] is True and batch["arguments"].item()["infile"] == paths[0]
    single = str(tmp_path / "s1_single.npz")
    cli.main(["convert", paths[1], single, "-binsize", "50000", "-bounded", "-chunk", "4096"])
    same_file(np.load(single, allow_pickle=True), np.load(os.path.join(outdir, "s1.npz"), allow_pickle=True))
