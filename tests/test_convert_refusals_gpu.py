"""What the entries of `convert` refuse, and with which code and text: wc_convert_reads_ex, wc_convert_begin,
wc_convert_feed, wc_convert_feed_dev and wc_convert_finish, every row of the table through every entry that takes the
argument.  The codes and message fragments are literals: they are what the library answered before its argument
checks, its host staging and its result read-back became one function each, and they may not move.  Where two entries
answer the same input differently the row says so per entry.  Then one tiny input through the whole call and through a
run fed in one slice and in two, against the restatements.  Integers throughout: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import convert_restated as cr
import convert_sliced_restated as csr

pytestmark = pytest.mark.gpu
PAIR, OTHER = 0x43, 0x83
BINSIZE = 1000.0
MAX_CHROM = 256                                         # WC_CV_MAX_CHROM of include/wisecondor_hip.h
E_ARG, E_LIMIT = -1, -3
I64 = lambda v: np.asarray(v, dtype=np.int64)

# two chromosomes of 5000 bases (6 bins each), 3 and 2 reads; every row of the table changes one argument of it
BASE = dict(pos=np.array([10, 100, 200, 5, 50], dtype=np.int32), mapq=np.full(5, 60, dtype=np.uint8),
            flag=np.full(5, PAIR, dtype=np.uint16), mate=np.array([5, 50, 100, 2, 25], dtype=np.int32),
            offs=I64([0, 3, 5]), bins=I64([0, 6, 12]), n_chrom=2, binsize=BINSIZE, paired=0)
BEYOND = dict(pos=np.array([10, 20, 7000, 5, 50], dtype=np.int32))      # 7000 / 1000 = bin 7 of 6


def _message():
    from wisecondor_amd import _lib
    return _lib.load().wc_last_error().decode()


def reads_ex(**change):
    """wc_convert_reads_ex on BASE with `change`: (rc, message, counts, stats)"""
    from wisecondor_amd import _lib
    a = dict(BASE, **change)
    counts = np.full(64, -5, dtype=np.int32)
    stats = np.full(8, -5, dtype=np.int64)
    rc = _lib.load().wc_convert_reads_ex(_lib.context(0), _lib.ptr(a["pos"]), _lib.ptr(a["mapq"]), _lib.ptr(a["flag"]),
                                         _lib.ptr(a["mate"]), _lib.ptr(a["offs"]), int(a["n_chrom"]), float(a["binsize"]), 4, 2, 1,
                                         int(a["paired"]), _lib.ptr(a["bins"]), _lib.ptr(counts), _lib.ptr(stats))
    return rc, _message() if rc else "", counts, stats


def begin(**change):
    """wc_convert_begin with BASE's parameters and `change`: (rc, message, run handle)"""
    from wisecondor_amd import _lib
    a = dict(BASE, **change)
    run = ctypes.c_void_p()
    rc = _lib.load().wc_convert_begin(_lib.context(0), int(a["n_chrom"]), float(a["binsize"]), 4, 2, 1, int(a["paired"]),
                                      _lib.ptr(a["bins"]), ctypes.byref(run))
    return rc, _message() if rc else "", run


def feed(device, finish=False, **change):
    """A sound run, then one slice (BASE with `change`) through wc_convert_feed or, with `device`, wc_convert_feed_dev;
    with `finish` the answer is wc_convert_finish's behind a slice that was taken: (rc, message, counts, stats)"""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    a = dict(BASE, **change)
    rc, _, run = begin(paired=a["paired"])
    assert rc == 0
    counts = np.full(64, -5, dtype=np.int32)
    stats = np.full(8, -5, dtype=np.int64)
    try:
        arrays = [a["pos"], a["mapq"], a["flag"], a["mate"]]
        if device:
            keep = [None if x is None else torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in arrays]
            ptrs = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in keep]
            rc = lib.wc_convert_feed_dev(run, None, ptrs[0], ptrs[1], ptrs[2], ptrs[3], _lib.ptr(a["offs"]))
        else:
            rc = lib.wc_convert_feed(run, *[_lib.ptr(x) for x in arrays], _lib.ptr(a["offs"]))
        message = _message() if rc else ""
        if finish:
            assert rc == 0
            rc = lib.wc_convert_finish(run, _lib.ptr(counts), _lib.ptr(stats))
            message = _message() if rc else ""
        torch.cuda.synchronize()
        return rc, message, counts, stats
    finally:
        lib.wc_convert_end(run)


ENTRIES = {
    "reads_ex": lambda **c: reads_ex(**c)[:2],
    "begin": lambda **c: begin(**c)[:2],
    "feed": lambda **c: feed(False, **c)[:2],
    "feed_dev": lambda **c: feed(True, **c)[:2],
    "finish": lambda **c: feed(True, finish=True, **c)[:2],
}
MANY = dict(n_chrom=MAX_CHROM + 1, offs=I64(np.zeros(MAX_CHROM + 2)), bins=I64(np.zeros(MAX_CHROM + 2)))
NO_READS = dict(offs=I64([0, 0, 0]))
START, DECREASE = "the offset tables must start at 0", "offsets of chromosome 1 decrease"
BINSIZE_TEXT, PAIRED_TEXT = "is not a positive finite number", "the paired mode needs the flag and mate position arrays"
BEYOND_TEXT = "1 read(s) lie beyond their chromosome's last bin (a position past the header's length)"

# (row, entry, the changed arguments, code, fragment of the message); code 0: the entry takes the input
TABLE = [
    ("no chromosomes", "reads_ex", dict(n_chrom=0), E_LIMIT, "convert: 0 chromosomes (1..256 supported)"),
    ("no chromosomes", "begin", dict(n_chrom=0), E_LIMIT, "convert: 0 chromosomes (1..256 supported)"),
    ("too many chromosomes", "reads_ex", MANY, E_LIMIT, "convert: 257 chromosomes (1..256 supported)"),
    ("too many chromosomes", "begin", MANY, E_LIMIT, "convert: 257 chromosomes (1..256 supported)"),
    ("bin size 0", "reads_ex", dict(binsize=0.0), E_ARG, "bin size 0 " + BINSIZE_TEXT),
    ("bin size 0", "begin", dict(binsize=0.0), E_ARG, "bin size 0 " + BINSIZE_TEXT),
    ("bin size negative", "reads_ex", dict(binsize=-5.0), E_ARG, "bin size -5 " + BINSIZE_TEXT),
    ("bin size negative", "begin", dict(binsize=-5.0), E_ARG, "bin size -5 " + BINSIZE_TEXT),
    ("bin size inf", "reads_ex", dict(binsize=float("inf")), E_ARG, "bin size inf " + BINSIZE_TEXT),
    ("bin size inf", "begin", dict(binsize=float("inf")), E_ARG, "bin size inf " + BINSIZE_TEXT),
    ("bin size nan", "reads_ex", dict(binsize=float("nan")), E_ARG, "nan " + BINSIZE_TEXT),
    ("bin size nan", "begin", dict(binsize=float("nan")), E_ARG, "nan " + BINSIZE_TEXT),
    ("read table starts at 1", "reads_ex", dict(offs=I64([1, 3, 5])), E_ARG, START),
    ("read table starts at 1", "feed", dict(offs=I64([1, 3, 5])), E_ARG, START),
    ("read table starts at 1", "feed_dev", dict(offs=I64([1, 3, 5])), E_ARG, START),
    ("bin table starts at 1", "reads_ex", dict(bins=I64([1, 6, 12])), E_ARG, START),
    ("bin table starts at 1", "begin", dict(bins=I64([1, 6, 12])), E_ARG, START),
    ("read table descends", "reads_ex", dict(offs=I64([0, 5, 3])), E_ARG, DECREASE),
    ("read table descends", "feed", dict(offs=I64([0, 5, 3])), E_ARG, DECREASE),
    ("read table descends", "feed_dev", dict(offs=I64([0, 5, 3])), E_ARG, DECREASE),
    ("bin table descends", "reads_ex", dict(bins=I64([0, 12, 6])), E_ARG, DECREASE),
    ("bin table descends", "begin", dict(bins=I64([0, 12, 6])), E_ARG, DECREASE),
    # a table that descends below 0: the entries that take HOST arrays size their staging by the last entry before they
    # look at the table, and call it a limit; the others find the descent
    ("read table ends below 0", "reads_ex", dict(offs=I64([0, 3, -1])), E_LIMIT, "convert: -1 reads, 12 bins in one call"),
    ("read table ends below 0", "feed", dict(offs=I64([0, 3, -1])), E_LIMIT, "convert: -1 reads in one slice"),
    ("read table ends below 0", "feed_dev", dict(offs=I64([0, 3, -1])), E_ARG, DECREASE),
    ("bin table ends below 0", "reads_ex", dict(bins=I64([0, 6, -1])), E_LIMIT, "convert: 5 reads, -1 bins in one call"),
    ("bin table ends below 0", "begin", dict(bins=I64([0, 6, -1])), E_ARG, DECREASE),
    ("paired without flag", "reads_ex", dict(paired=1, flag=None), E_ARG, PAIRED_TEXT),
    ("paired without flag", "feed", dict(paired=1, flag=None), E_ARG, PAIRED_TEXT),
    ("paired without flag", "feed_dev", dict(paired=1, flag=None), E_ARG, PAIRED_TEXT),
    ("paired without mate_pos", "reads_ex", dict(paired=1, mate=None), E_ARG, PAIRED_TEXT),
    ("paired without mate_pos", "feed", dict(paired=1, mate=None), E_ARG, PAIRED_TEXT),
    ("paired without mate_pos", "feed_dev", dict(paired=1, mate=None), E_ARG, PAIRED_TEXT),
    # without reads the whole call still asks for the paired arrays; an empty slice of a run asks for nothing
    ("paired without flag, no reads", "reads_ex", dict(paired=1, flag=None, **NO_READS), E_ARG, PAIRED_TEXT),
    ("paired without flag, no reads", "feed", dict(paired=1, flag=None, **NO_READS), 0, ""),
    ("paired without flag, no reads", "feed_dev", dict(paired=1, flag=None, **NO_READS), 0, ""),
    ("no pos", "reads_ex", dict(pos=None), E_ARG, "convert: NULL read arrays"),
    ("no pos", "feed", dict(pos=None), E_ARG, "convert: NULL read arrays"),
    ("no pos", "feed_dev", dict(pos=None), E_ARG, "convert: NULL read arrays"),
    ("no mapq", "reads_ex", dict(mapq=None), E_ARG, "convert: NULL read arrays"),
    ("no mapq", "feed", dict(mapq=None), E_ARG, "convert: NULL read arrays"),
    ("no mapq", "feed_dev", dict(mapq=None), E_ARG, "convert: NULL read arrays"),
    # the device form of the feed does not wait for the slice: the run's finish finds the status word
    ("position past the length", "reads_ex", BEYOND, E_ARG, BEYOND_TEXT),
    ("position past the length", "feed", BEYOND, E_ARG, BEYOND_TEXT),
    ("position past the length", "feed_dev", BEYOND, 0, ""),
    ("position past the length", "finish", BEYOND, E_ARG, BEYOND_TEXT),
]


@pytest.mark.parametrize("row,entry,change,code,fragment", TABLE, ids=["%s-%s" % (r[1], r[0].replace(" ", "_")) for r in TABLE])
def test_refusal(row, entry, change, code, fragment):
    rc, message = ENTRIES[entry](**change)
    print(entry, row, rc, repr(message))
    assert rc == code
    assert fragment in message
    assert (rc == 0) == (message == "")


def test_the_sound_base_is_taken_by_every_entry():
    for entry in ENTRIES:
        for paired in (0, 1):
            assert ENTRIES[entry](paired=paired) == (0, "")


def test_what_is_written_behind_a_read_beyond_the_last_bin():
    """include/wisecondor_hip.h: the status word is stats [4]; wc_convert_finish writes stats_out and leaves counts_out
    alone.  The whole call writes its counts all the same (tests/test_convert_bounded_gpu.py compares them with a run's)."""
    rc, _, counts, stats = reads_ex(**BEYOND)
    assert rc == E_ARG and int(stats[4]) == 1 and [int(v) for v in stats[:4]] == [0, 0, 3, 2]
    assert [int(v) for v in counts[:12]] == [1] + [0] * 5 + [1] + [0] * 5 and np.all(counts[12:] == -5)
    rc, _, counts, stats = feed(True, finish=True, **BEYOND)
    assert rc == E_ARG and int(stats[4]) == 1 and [int(v) for v in stats[:4]] == [0, 0, 3, 2]
    assert np.all(counts == -5)


# ------------------------------------------------------------------------------------------------ one tiny input
# chr1: a duplicate (100 100), a read of mapping quality 0, a read that is no first-in-pair; chr2: a run of 3 reads (longer
# than the threshold of 2) and a run of 2 (4000, 4003) that the cut between reads 9 and 10 divides; chr3: one read
TINY = [(np.array([10, 100, 100, 300, 1000]), np.array([60, 60, 60, 0, 60]), np.array([PAIR] * 4 + [OTHER])),
        (np.array([5, 2000, 2001, 2002, 4000, 4003]), np.full(6, 60), np.full(6, PAIR)),
        (np.array([7]), np.full(1, 60), np.full(1, PAIR))]
TINY = [(p, q, f, p // 2) for p, q, f in TINY]          # equal positions have equal mates: duplicates in both modes
LENGTHS = [5000, 5000, 5000]
MIN_SHIFT, THRESHOLD, CUT = 4, 2, 10


def tiny_arrays():
    cat = lambda i, dtype: np.ascontiguousarray(np.concatenate([c[i] for c in TINY]), dtype=dtype)
    starts = I64(np.concatenate([[0], np.cumsum([len(c[0]) for c in TINY])]))
    bins = I64(np.concatenate([[0], np.cumsum([cr.n_bins(l, BINSIZE) for l in LENGTHS])]))
    return (cat(0, np.int32), cat(1, np.uint8), cat(2, np.uint16), cat(3, np.int32)), starts, bins


def tiny_run(cuts, paired):
    """The tiny input through wc_convert_begin / wc_convert_feed / wc_convert_finish, cut at `cuts`: (counts, stats)"""
    from wisecondor_amd import _lib
    lib = _lib.load()
    arrays, starts, bins = tiny_arrays()
    run = ctypes.c_void_p()
    _lib.check(lib.wc_convert_begin(_lib.context(0), 3, BINSIZE, MIN_SHIFT, THRESHOLD, 1, int(paired), _lib.ptr(bins),
                                    ctypes.byref(run)))
    try:
        edges = [0] + list(cuts) + [int(starts[-1])]
        for lo, hi in zip(edges[:-1], edges[1:]):
            piece = [np.ascontiguousarray(a[lo:hi]) for a in arrays]
            _lib.check(lib.wc_convert_feed(run, *[_lib.ptr(a) for a in piece], _lib.ptr(I64(np.clip(starts - lo, 0, hi - lo)))))
        counts = np.full(int(bins[-1]) + 1, -5, dtype=np.int32)
        stats = np.full(8, -5, dtype=np.int64)
        _lib.check(lib.wc_convert_finish(run, _lib.ptr(counts), _lib.ptr(stats)))
        assert counts[-1] == -5
        return counts[:-1], stats
    finally:
        lib.wc_convert_end(run)


@pytest.mark.parametrize("paired", [False, True])
def test_tiny_input_whole_and_in_slices(paired):
    from wisecondor_amd import _lib
    arrays, starts, bins = tiny_arrays()
    counts = np.full(int(bins[-1]) + 1, -5, dtype=np.int32)
    stats = np.full(8, -5, dtype=np.int64)
    _lib.check(_lib.load().wc_convert_reads_ex(_lib.context(0), *[_lib.ptr(a) for a in arrays], _lib.ptr(starts), 3, BINSIZE,
                                               MIN_SHIFT, THRESHOLD, 1, int(paired), _lib.ptr(bins), _lib.ptr(counts),
                                               _lib.ptr(stats)))
    assert counts[-1] == -5
    counts = counts[:-1]
    named = dict(zip(csr.COUNTERS, (int(v) for v in stats[:7])))
    # all of it occurs: a duplicate, a low mapping quality, a run over the threshold, the run across the cut counted
    assert named["filter_rmdup"] == 1 and named["filter_mapq"] == 1 and named["kept"] - named["post_retro"] == 3
    assert named["pair_fail"] == (1 if paired else 0) and named["outside"] == 0
    assert counts[int(bins[1]) + 4] == 2 and counts[int(bins[1]) + 2] == 0
    n_bins = [cr.n_bins(l, BINSIZE) for l in LENGTHS]
    for cuts in ([], [CUT]):
        got_counts, got_stats = tiny_run(cuts, paired)
        assert np.array_equal(got_counts, counts)
        assert [int(v) for v in got_stats[:7]] == [int(v) for v in stats[:7]]
        want_counts, want_stats, _ = csr.convert_sliced(n_bins, csr.cut(TINY, cuts), BINSIZE, MIN_SHIFT, THRESHOLD, 1, paired)
        assert np.array_equal(np.concatenate(want_counts), counts)
        assert want_stats == named
    if not paired:
        names = ["chr1", "chr2", "chr3"]
        sample, counters = cr.convert(names, LENGTHS, [c[0] for c in TINY], [c[1] for c in TINY], BINSIZE, MIN_SHIFT, THRESHOLD)
        assert np.array_equal(np.concatenate([sample[cr.chrom_key(n)] for n in names]), counts)
        assert counters == dict((k, named[k]) for k in counters)
