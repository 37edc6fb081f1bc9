"""Inputs of the refsize workgroup-shape tests of newref's fast path (a helper module, not a conftest; modelled on
zscore_batch_cases.py and call_cases.py; checked on the CPU by test_refsize_cases_cpu.py, used on the GPU by
test_newref_refsize_shapes_gpu.py).

newref_finish_part launches k_rescore with ps_of(k) threads, two to five waves for the refsizes the fast path serves
(k <= 256); wave w of a row takes the pairs [64 w + t ps, 64 w + t ps + 64) of trip t.  The layouts here fix how many
pairs a row re-scores by the code's own rules, with every threshold at FLT_MAX (admit-all):

* few(a, b): two noise chromosomes of a and b rows.  A row whose candidates number fewer than k re-scores all of them
  (pick_row's n < k branch): with a < k and b < k the rows of the first chromosome re-score exactly b pairs, those of
  the second exactly a, 2 a b in all.
* near(m, far, T): chromosome 1 is T noise rows (the target rows); chromosome 2 is a cluster of m rows of
  1 + 1e-6 N(0, 1) followed by `far` noise rows.  The cluster rows are nearer to every target row than any noise row,
  their float16 keys cannot be told apart (all inside the certified bound together), their float64 distances are all
  different: for m >= k a target row re-scores exactly m pairs.  A row of chromosome 2 has the T target rows as
  candidates: T pairs where T < k.
* copies(m, far, T): near with the m rows bit-identical (all ones): exact ties, the counting order's second sweep.

Noise is 1 + 0.03 N(0, 1).  Every array is read-only and cached.
"""
import functools

import numpy as np

from oracle import wc_oracle as wo

RMAX = 512               # csrc/newref.hip: pair slots of a row on the fast path; more pairs -> exact path
T_ROWS = 70              # target rows of near / copies, first chromosome of few
FAR = 40
FAR_RATIO = 1.25         # the nearest far row is at least this many times as far as the farthest cluster row
PERTURBATION = 1e-6      # of the cluster rows of near


def ps_of(k):
    """Threads of a k_rescore workgroup at refsize k (newref_finish_part): k + 28 rounded up to whole waves, at
    least two waves, at most 512 threads."""
    return max(128, min(512, -(-(k + 28) // 64) * 64))


def noise(seed, rows, samples):
    return 1.0 + 0.03 * np.random.RandomState(seed).standard_normal((rows, samples))


@functools.lru_cache(maxsize=None)
def few(a, b, samples=100):
    data = noise(1000 * a + b + 7 * samples, a + b, samples)
    data.setflags(write=False)
    return data, (a, b)


def far_ratio(data, T, m):
    """The smallest (nearest far row) / (farthest cluster row) over the target rows, in plain numpy."""
    worst = np.inf
    for t in range(T):
        d = ((data[T:] - data[t]) ** 2).sum(1)
        worst = min(worst, d[m:].min() / d[:m].max())
    return worst


@functools.lru_cache(maxsize=None)
def near(m, far=FAR, T=T_ROWS, samples=100):
    """The ratio of a far row's distance to a cluster row's is 2 on average over the T * far (target, far) pairs, with
    a spread of sqrt(6 / samples): 0.245 at 100 samples, where about one draw in four keeps all 2 800 pairs of the
    usual layout above FAR_RATIO.  The seed counts up from 5 until the draw does (with a margin for copies(), whose
    cluster sits 1e-6 elsewhere); test_refsize_cases_cpu.py holds the result to FAR_RATIO by the oracle."""
    for seed in range(5, 200):
        rng = np.random.RandomState(1000 * seed + 31 * m + 7 * far + 13 * samples)
        data = np.empty((T + m + far, samples))
        data[:T] = 1.0 + 0.03 * rng.standard_normal((T, samples))
        data[T:T + m] = 1.0 + PERTURBATION * rng.standard_normal((m, samples))
        data[T + m:] = 1.0 + 0.03 * rng.standard_normal((far, samples))
        if far_ratio(data, T, m) >= FAR_RATIO + 0.01:
            data.setflags(write=False)
            return data, (T, m + far)
    raise AssertionError("near(%d, %d, %d, %d): no draw keeps the far rows outside" % (m, far, T, samples))


@functools.lru_cache(maxsize=None)
def copies(m, far=FAR, T=T_ROWS, samples=100):
    data = np.array(near(m, far, T, samples)[0])
    data[T:T + m] = 1.0
    data.setflags(write=False)
    return data, (T, m + far)


MAKERS = {"few": few, "near": near, "copies": copies}


@functools.lru_cache(maxsize=None)
def oracle(family, args, k, order):
    """wo.get_reference(fast=True) of the layout in Fortran ("F": sequential sums) or C order (pairwise sums)."""
    data, bins = MAKERS[family](*args)
    laid = np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)
    with np.errstate(all="ignore"):
        idx, dst = wo.get_reference(laid, np.asarray(bins), np.cumsum(bins), k, 1, 1, fast=True)
    idx, dst = np.asarray(idx), np.asarray(dst)
    idx.setflags(write=False)
    dst.setflags(write=False)
    return idx, dst


@functools.lru_cache(maxsize=None)
def target_view(family, args, order):
    """Every candidate of every target row in the oracle's order: (positions [T, m + far], distances [T, m + far])."""
    data, bins = MAKERS[family](*args)
    laid = np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)
    T = bins[0]
    with np.errstate(all="ignore"):
        return wo.get_ref_for_bins_fast(bins[1], 0, T, laid, np.concatenate((laid[:0, :], laid[T:, :])))


def designed(family, args, k):
    """(rescored, fallback_rows) of a full finish at refsize k with every threshold at FLT_MAX."""
    if family == "few":
        a, b = args[:2]
        assert a < k and b < k
        return 2 * a * b, 0
    m = args[0]
    far = args[1] if len(args) > 1 else FAR
    T = args[2] if len(args) > 2 else T_ROWS
    assert m >= k and T < k
    if m > RMAX:
        return (m + far) * T, T          # the target rows have more pairs than slots: exact path
    return T * m + (m + far) * T, 0


# ------------------------------------------------------------------------------------------- the cases ----
# first trip, pair counts b of the first chromosome's rows: the last wave in use holds b - 128 (k = 164: third wave)
# or b - 192 (k = 228, 256: fourth wave) pairs, either side of every pass of eight and every DMA group of sixteen
FEW_B = {
    164: (127, 128, 129, 135, 136, 137, 143, 144, 145, 163),
    228: (191, 192, 193, 199, 200, 201, 207, 208, 209, 227),
    256: (193, 200, 201, 208, 209, 224, 225, 240, 241, 255),
}
# cluster sizes m: the waves up to the fifth, second and third trips, RMAX and one pair more (exact path)
NEAR_M = {
    101: (101, 193, 201, 257, 321, 385, 449, 512, 513),
    164: (164, 193, 385, 512),
    165: (165, 256, 257, 265, 321, 385, 449, 512, 513),
    228: (228, 257, 512),
    229: (229, 257, 264, 265, 272, 273, 319, 320, 321, 329, 385, 512, 513),
    256: (256, 257, 320, 321, 512, 513),
    100: (385,),
}
# k <= T: the rows of chromosome 2 have T >= k candidates and re-score what their bound admits, no designed number;
# the target rows' count is taken from a finish of their band alone
NEAR_M_SMALL = {1: (1, 2, 65, 129), 2: (2, 130)}
COPIES_KM = ((164, 193), (228, 257), (256, 321))
LEAN_K = (101, 256)
# 600 candidates per target row: pick_row's LEAN form.  400 samples: with 300 far rows a layout has 21 000 (target,
# far) pairs, and at 100 samples FAR_RATIO is three standard deviations below the mean ratio -- no draw keeps them all
# outside (the smallest of the first draw was 1.105); at 400 samples it is six.
LEAN_ARGS = (300, 300, T_ROWS, 400)
BIG_LDS_K = 256
BIG_LDS_ARGS = ((321, FAR, T_ROWS, 2048), (321, FAR, T_ROWS, 2047))
STALE_K = 229
STALE_ARGS = ((512,), (257,))
NATURAL_K = (101, 164, 165, 228, 229, 256)


def near_cases():
    """Every (k, args) of near that the GPU module runs."""
    out = [(k, (m,)) for k, ms in NEAR_M.items() for m in ms]
    out += [(k, (m,)) for k, ms in NEAR_M_SMALL.items() for m in ms]
    out += [(k, LEAN_ARGS) for k in LEAN_K]
    out += [(BIG_LDS_K, args) for args in BIG_LDS_ARGS]
    out += [(STALE_K, args) for args in STALE_ARGS]
    return list(dict.fromkeys(out))
