"""The inputs of the draw tests (a helper module, not a conftest): the designed thinning input whose restated statistics
test_draw_cases_cpu.py holds as conditions, the thinning rows and the binomial spike's plans of test_draw_gpu.py.
Everything is made once and handed out read-only."""
import functools

import numpy as np

import draw_restated as dr

CUTOFF = 4096                    # wc_thin_wave_cutoff(): test_draw_gpu.py asserts that the library says the same
MAX_READS = 2 ** 24
HIGH_SEED = 0x9E3779B97F4A7C15   # a seed with its high word set
SMALL_COUNTS = [0, 1, 3, 4, 5, 255, 256, 257]
KEEPS = {1: [500000], 2: [1000000, 1], 8: [1000000, 900000, 500000, 250000, 100000, 1000, 1, 999999]}
SPIKE_PPM = [25000, -25000, 1500000, 2000000, -1000000, 100000000]
CLIP_COUNT = 21474837            # x 101 is beyond 2^31 - 1, x 3 is not


# ---------------------------------------------------------------------- the designed input of the statistics ----
DESIGNED = dict(bins=2000, mean=500, input_seed=0, seed=1, chrom=3, row=0, depths=[500000, 250000, 100000])


@functools.lru_cache(maxsize=None)
def designed_counts():
    counts = np.random.RandomState(DESIGNED["input_seed"]).poisson(DESIGNED["mean"], DESIGNED["bins"]).astype(np.int64)
    counts.setflags(write=False)
    return counts


@functools.lru_cache(maxsize=None)
def designed_thinned():
    """int64 [3, 2000]: the designed counts at the three depths, by the restatement."""
    out = dr.draw_segment(designed_counts(), 0, DESIGNED["chrom"], dr.TAG_THIN, DESIGNED["row"], DESIGNED["seed"], DESIGNED["depths"])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- the thinning ----
def thin_sizes(r):
    """Three chromosomes, 1021 + r bins, the middle one of ONE bin (its first bin is its last)."""
    return np.array([7, 1, 1013 + r], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def thin_base(n_base, r):
    """Poisson(30) rows.  Flat bins 20 .. 27: the small counts around a Philox block and around 256.  Flat bin 100: a bin
    at the cutoff among small ones.  Flat bins 200 .. 202: cutoff - 1, + 0, + 1 side by side (two wave-taken bins in one
    wave).  Flat bins 256 .. 319 (one wave of the first row): nothing but one bin at cutoff + 1, alone in its wave.
    Negative counts at flat bins 0 (a chromosome's first bin), 6 (its last), 7 (the one-bin chromosome, second row only)
    and 40; the row's last bin holds 257."""
    n_total = int(thin_sizes(r).sum())
    base = np.random.RandomState(70 + r).poisson(30, size=(n_base, n_total)).astype(np.int64)
    base[:, 20:28] = SMALL_COUNTS
    base[:, 100] = CUTOFF
    base[:, 200:203] = [CUTOFF - 1, CUTOFF, CUTOFF + 1]
    base[0, 256:320] = 0
    base[0, 300] = CUTOFF + 1
    base[:, 0], base[:, 6], base[:, 40] = -1, -5, -(2 ** 31)
    if n_base > 1:
        base[1, 7] = -3
    base[:, -1] = 257
    base = base.astype(np.int32)
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=None)
def thin_want(n_base, r, n_keep, seed):
    out = dr.thin(thin_base(n_base, r), thin_sizes(r), KEEPS[n_keep], seed)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tower_want():
    """(base [1, 3], sizes, keep, the restated thinning) of one bin of exactly 2^24 reads between two small ones."""
    base = np.array([[5, MAX_READS, 9]], dtype=np.int32)
    sizes = np.array([1, 2], dtype=np.int64)
    return base, sizes, [500000], dr.thin(base, sizes, [500000], 1)


# -------------------------------------------------------------------------------------- the binomial spike ----
def spike_sizes(r):
    return np.array([5, 3, 1, 1012 + r], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def spike_base(n_base, r):
    """Poisson(300) rows (2.5 % of a bin is 7.5 reads); 0 and -5 inside the spans that try every alignment, and CLIP_COUNT
    at bin 500 of the long chromosome, which only whole-multiple effects reach (they draw nothing)."""
    n_total = int(spike_sizes(r).sum())
    base = np.random.RandomState(80 + r).poisson(300, size=(n_base, n_total)).astype(np.int64)
    base[:, 9 + 3] = 0
    base[:, 9 + 6] = -5
    base[:, 9 + 500] = CLIP_COUNT
    base = base.astype(np.int32)
    base.setflags(write=False)
    return base


def spike_plan(n_base, r):
    """Spans on the long chromosome at every start 0 .. 7 x every length 1 .. 9 with the effects in rotation, every effect
    on the first bins of the array and on its last ones, the one-bin chromosome, the clip (100 000 000 ppm over
    CLIP_COUNT) and the same span at 2 000 000 ppm, which does not clip, and a control; base rows out of order."""
    long_size = 1012 + r
    spans = [(4, first, bins, SPIKE_PPM[(first + bins) % len(SPIKE_PPM)]) for first in range(8) for bins in range(1, 10)]
    spans += [(1, 0, 5, ppm) for ppm in SPIKE_PPM] + [(4, long_size - 4, 4, ppm) for ppm in SPIKE_PPM]
    spans += [(3, 0, 1, 25000), (4, 498, 5, 100000000), (4, 498, 5, 2000000), (2, 1, 1, 0), (4, 100, 300, 25000), (4, 100, 300, -25000)]
    return np.array([((n_base - 1 - i) % n_base,) + row for i, row in enumerate(spans)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def spike_want(n_base, r, seed, trial0):
    out, saturated = dr.spike_draw(spike_base(n_base, r), spike_sizes(r), spike_plan(n_base, r), seed, trial0)
    out.setflags(write=False)
    return out, saturated
