"""k_rescore at the shapes where a row's re-score takes another path: pair counts on both sides of the 64-lane waves and
of k, rows skipped for the exact path between rows that are not, rows of several trips (more pairs than the workgroup
has threads) with tied distances next to ordinary rows, more pairs than the fast path holds, sample counts below and
above the workgroup's thread count in both summation orders, row bands, and the same bits from repeated calls.

Everything here is the pattern of test_pick_batched_gpu.py: a few chromosomes, every threshold at FLT_MAX, so that a
row's list is exactly the other chromosomes; the output is held against the oracle bit for bit and the number of
exact-path rows against what the input implies.  k_rescore takes one row per workgroup; the cases were chosen
while a form that walked several rows per workgroup was tried (EXPERIMENTS.md: slower, not kept)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

K = 100
FMAX = np.finfo(np.float32).max


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


class Job(object):
    """prepare / thresholds / every threshold FLT_MAX / collect on one input; finish() as often as a test wants."""

    def __init__(self, data, bins, order="F"):
        import torch
        from wisecondor_amd import _lib, distributed
        self.torch = torch
        self.B = data.shape[0]
        self.X = torch.from_numpy(np.array(data, order="C")).cuda()          # (a copy: the cached input is read-only)
        self.st = distributed.HipStages(_lib.context(0), self.X, np.asarray(bins, dtype=np.int64), K,
                                        _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)
        self.st.prepare()
        self.st.thresholds(0, self.B)
        self.st.set_thr(0, self.B, torch.full((self.B,), float(FMAX), dtype=torch.float32, device="cuda"))
        self.st.collect(0, self.B, 0, 1)

    def finish(self, bands=None):
        """-> (idx, dst) of the whole job after finish(rb, re) for every band in turn; rows of no band keep -7 / NaN."""
        torch = self.torch
        idx = torch.full((self.B, K), -7, dtype=torch.int32, device="cuda")
        dst = torch.full((self.B, K), float("nan"), dtype=torch.float64, device="cuda")
        for rb, re in (bands or [(0, self.B)]):
            self.st.finish(rb, re, idx[rb:re], dst[rb:re])
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()

    def stats(self):
        from wisecondor_amd import wisetools
        return wisetools.newref_stats(0)


def noise(seed, rows, samples):
    return 1.0 + 0.03 * np.random.RandomState(seed).standard_normal((rows, samples))


@functools.lru_cache(maxsize=None)
def two_chromosomes(a, b, samples=100, bad=()):
    """-> (data, bins) of two chromosomes of a and b rows; the rows `bad` carry one value of 1e9 (no float16 image:
    listed nowhere, exact path)."""
    data = noise(1000 * a + b + 7 * samples, a + b, samples)
    for r in bad:
        data[r, 40 % samples] = 1e9
    data.setflags(write=False)
    return data, (a, b)


@functools.lru_cache(maxsize=None)
def tied_chromosomes(copies):
    """Three chromosomes of 70, 100 + copies and 70 rows; `copies` rows of the middle one are bit-identical and closer
    to every row than any other (all ones, the mean of the noise): a row of the outer chromosomes re-scores all of them
    with one tied distance.  A row of the middle one lists the 140 outer rows, of which k_pick passes on those with a
    key at or below its bound of the k-th distance: about 101 pairs, one trip (the tests check the mean)."""
    n = 70 + 100 + copies + 70
    data = noise(31 + copies, n, 100)
    data[70 + 50:70 + 50 + copies] = 1.0
    data.setflags(write=False)
    return data, (70, 100 + copies, 70)


@functools.lru_cache(maxsize=None)
def oracle(maker, args, order="F"):
    data, bins = maker(*args)
    laid = np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)
    with np.errstate(all="ignore"):
        return wo.get_reference(laid, np.asarray(bins), np.cumsum(bins), K, 1, 1, fast=True)


def check(got, want):
    assert np.array_equal(got[0], want[0])
    assert same_bits(got[1], want[1])


# second-chromosome sizes: an empty, a partly filled and a full second wave of the first chromosome's rows (R = b up
# to 100, with the sentinel padding for fewer candidates than k), and the sizes around k
@pytest.mark.parametrize("b", [1, 37, 63, 64, 65, 99, 100, 101, 129])
def test_pair_counts_around_the_waves(b):
    data, bins = two_chromosomes(130, b)
    job = Job(data, bins)
    got = job.finish()
    stats = job.stats()
    print("sizes (130, %d): %s" % (b, stats))
    check(got, oracle(two_chromosomes, (130, b)))
    if b < K:
        assert (got[0][:130, b:] == -1).all() and (got[0][:130, :b] >= 0).all()
    # one bin behind the first chromosome and none before it: its rows carry no layout in the reference and numpy
    # sums them pairwise (FinishArgs::lone_mask), which only the exact path does in the sequential order
    lone = 130 if b == 1 else 0
    assert stats["fast_rows"] == 130 + b - lone and stats["fallback_rows"] == lone, stats


def test_exact_path_rows_between_fast_rows():
    """Rows without a float16 image (exact path: their workgroup leaves at once) at the first, a middle and the last
    but one row of the band [128, 230) and two close together; finish() runs on that band first, then on [0, 128).
    The per-sample centre is taken from the first 128 rows of these 230: none of them.  All five are rows of the second chromosome (120 + 110 rows), which leaves a row
    of the first 105 candidates: with fewer than k it could not tell how far the unlisted rows are and would take
    the exact path as well."""
    a, b = 120, 110
    bad = (128, 180, 228, 141, 145)
    data, bins = two_chromosomes(a, b, 100, bad)
    job = Job(data, bins)
    got = job.finish([(128, a + b), (0, 128)])
    stats = job.stats()
    print("exact rows %s: %s" % (bad, stats))
    check(got, oracle(two_chromosomes, (a, b, 100, bad)))
    for r in bad:
        # 1e9 in the same sample: within the sentinel only of the rows of the other chromosome that carry it too
        near = sorted(q if q < a else q - a for q in bad if (q < a) != (r < a))
        assert sorted(got[0][r][got[0][r] >= 0].tolist()) == near
    assert stats["fast_rows"] + stats["fallback_rows"] == a + b, stats
    assert stats["fallback_rows"] == len(bad), stats


def test_several_trips_next_to_ordinary_rows():
    """200 tied nearest candidates: the rows of the outer chromosomes re-score more than the 128 pairs of a trip and
    run the tie sweep; the rows of the middle chromosome between them are ordinary."""
    data, bins = tied_chromosomes(200)
    job = Job(data, bins)
    got = job.finish()
    stats = job.stats()
    print("200 copies: %s" % (stats,))
    check(got, oracle(tied_chromosomes, (200,)))
    assert stats["fast_rows"] == 440 and stats["fallback_rows"] == 0, stats
    assert stats["rescored"] >= 140 * 200                # the outer rows took every copy: two trips each
    # (the 200 copies tie at an outer row's k-th distance, so it keeps them all) what is left for the 300 middle rows
    # is within one trip of 128 pairs each on average
    assert stats["rescored"] - 140 * 200 <= 300 * 128, stats


def test_more_pairs_than_the_fast_path_holds():
    """600 tied nearest candidates are more than the 512 pair slots of a row: the 140 outer rows go to the exact path,
    the middle rows between them stay on the fast one."""
    data, bins = tied_chromosomes(600)
    job = Job(data, bins)
    got = job.finish()
    stats = job.stats()
    print("600 copies: %s" % (stats,))
    check(got, oracle(tied_chromosomes, (600,)))
    assert stats["fast_rows"] == 700 and stats["fallback_rows"] == 140, stats
    assert stats["rescored"] <= 700 * 128, stats         # the middle rows: one trip each on average


# Sp = 16 n below and above the 128 threads of a workgroup: one, two and five own values per thread written to
# LDS, one to 38 chunks per candidate; "C" runs the LDS-DMA instantiation (the pairwise sum; below eight samples numpy's
# pairwise sum is the sequential one)
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("samples", [7, 16, 17, 100, 128, 129, 600])
def test_sample_counts(samples, order):
    data, bins = two_chromosomes(130, 101, samples)
    job = Job(data, bins, order)
    got = job.finish()
    stats = job.stats()
    print("%d samples, order %s: %s" % (samples, order, stats))
    check(got, oracle(two_chromosomes, (130, 101, samples), order))
    assert stats["fast_rows"] + stats["fallback_rows"] == 231, stats
    assert stats["fallback_rows"] == 0, stats


def test_row_bands():
    """finish(rb, re) with rb > 0, an odd number of rows, a single row; then the rest: the union is the whole job."""
    data, bins = two_chromosomes(130, 101)
    job = Job(data, bins)
    want = oracle(two_chromosomes, (130, 101))
    part = job.finish([(17, 120), (120, 121)])
    untouched = np.r_[0:17, 121:231]
    assert (part[0][untouched] == -7).all() and np.isnan(part[1][untouched]).all()
    assert np.array_equal(part[0][17:121], want[0][17:121]) and same_bits(part[1][17:121], want[1][17:121])
    check(job.finish([(17, 120), (120, 121), (0, 17), (121, 231)]), want)
    check(job.finish(), want)


def test_same_bits_every_time():
    """One prepared state: the same finish twice, and once more after a finish of another band."""
    data, bins = two_chromosomes(130, 101)
    job = Job(data, bins)
    first = job.finish()
    second = job.finish()
    job.finish([(40, 77)])
    third = job.finish()
    check(first, oracle(two_chromosomes, (130, 101)))
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and same_bits(first[1], other[1])
