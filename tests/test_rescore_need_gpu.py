"""k_rescore gathers only the candidate rows a wave has: its passes of eight rows (DMA groups of sixteen in the LDS-DMA
form) follow its number of pairs, and the slab rows of a pass left out keep whatever was there.  The cases sit on both
sides of every such boundary: pair counts of the first and of the second wave around every multiple of 8 and 16, a
second trip of one or nine pairs, and a job whose slabs hold the squares of a longer job when a skipped pass leaves
them unwritten.  Every S % 16 is here as well: the last chunk of sixteen samples is zero padded, a form that read and
summed it only as far as the real samples go was tried with these cases (EXPERIMENTS.md: no gain, not kept).

The pattern is the one of test_rescore_rows_gpu.py: a few chromosomes, every threshold at FLT_MAX, so that a row's list
is exactly the other chromosomes; the output is held against the oracle bit for bit (indexes equal, distances by
their int64 view) and the number of exact-path rows against what the input implies."""
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

    def finish(self):
        torch = self.torch
        idx = torch.full((self.B, K), -7, dtype=torch.int32, device="cuda")
        dst = torch.full((self.B, K), float("nan"), dtype=torch.float64, device="cuda")
        self.st.finish(0, self.B, idx, dst)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()

    def stats(self):
        from wisecondor_amd import wisetools
        return wisetools.newref_stats(0)


def noise(seed, rows, samples):
    return 1.0 + 0.03 * np.random.RandomState(seed).standard_normal((rows, samples))


@functools.lru_cache(maxsize=None)
def two_chromosomes(a, b, samples=100):
    data = noise(1000 * a + b + 7 * samples, a + b, samples)
    data.setflags(write=False)
    return data, (a, b)


@functools.lru_cache(maxsize=None)
def tied_chromosomes(copies):
    """Three chromosomes of 70, 100 + copies and 70 rows; `copies` rows of the middle one are bit-identical and closer
    to every row than any other (all ones, the mean of the noise): a row of the outer chromosomes re-scores all of them
    with one tied distance, in a first trip of 128 pairs and a second of copies - 128."""
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


def run_pair_count(b, order):
    """(130, b): the 130 rows of the first chromosome re-score exactly b pairs."""
    data, bins = two_chromosomes(130, b)
    job = Job(data, bins, order)
    got = job.finish()
    stats = job.stats()
    print("sizes (130, %d), order %s: %s" % (b, order, stats))
    check(got, oracle(two_chromosomes, (130, b), order))
    if b < K:
        assert (got[0][:130, b:] == -1).all() and (got[0][:130, :b] >= 0).all()
        assert (got[1][:130, b:] == 1e10).all()
    assert stats["fast_rows"] == 130 + b and stats["fallback_rows"] == 0, stats


# the second wave holds b - 64 = 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33 pairs: either side of every pass of
# eight rows and of every DMA group of sixteen
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("b", [65, 71, 72, 73, 79, 80, 81, 87, 88, 89, 95, 96, 97])
def test_pass_boundaries_of_the_second_wave(b, order):
    run_pair_count(b, order)


# the first wave alone (the second has no pair and no trip), with the sentinel padding behind the b candidates
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("b", [7, 8, 9, 16, 17, 33, 48, 49])
def test_pass_boundaries_of_the_first_wave(b, order):
    run_pair_count(b, order)


# copies - 128 = 1, 9 and 65 pairs in an outer row's second trip: one and two passes on wave 0, a full wave 0 and one
# pair on wave 1
@pytest.mark.parametrize("copies", [129, 137, 193])
def test_a_short_last_trip(copies):
    data, bins = tied_chromosomes(copies)
    job = Job(data, bins)
    got = job.finish()
    stats = job.stats()
    print("%d copies: %s" % (copies, stats))
    check(got, oracle(tied_chromosomes, (copies,)))
    assert stats["fast_rows"] == 240 + copies and stats["fallback_rows"] == 0, stats
    assert stats["rescored"] >= 140 * copies, stats      # the outer rows took every copy: two trips each


# S % 16 = 1 .. 15 and 0: the last chunk holds 1 .. 16 real samples; 1, 2 and 15: a single, partly filled chunk
@pytest.mark.parametrize("samples,order", [(s, o) for s in range(97, 113) for o in "FC"] + [(1, "F"), (2, "F"), (15, "F")])
def test_every_tail_width(samples, order):
    data, bins = two_chromosomes(130, 101, samples)
    job = Job(data, bins, order)
    got = job.finish()
    stats = job.stats()
    print("%d samples, order %s: %s" % (samples, order, stats))
    check(got, oracle(two_chromosomes, (130, 101, samples), order))
    assert stats["fast_rows"] == 231 and stats["fallback_rows"] == 0, stats


def test_stale_lds_never_reaches_an_output():
    """600 samples first (38 chunks through every slab row of both waves), then twice a job whose second wave has nine
    pairs: its passes 2 .. 7 write nothing, and those slab rows hold what the job before left there."""
    data, bins = two_chromosomes(130, 101, 600)
    check(Job(data, bins).finish(), oracle(two_chromosomes, (130, 101, 600)))
    want = oracle(two_chromosomes, (130, 73))
    data, bins = two_chromosomes(130, 73)
    first = Job(data, bins).finish()
    second = Job(data, bins).finish()
    check(first, want)
    check(second, want)
    assert np.array_equal(first[0], second[0]) and same_bits(first[1], second[1])
