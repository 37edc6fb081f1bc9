"""The order of a row's pairs at the end of k_rescore: ranks by counting on a 32-bit image of the float64-ordered
distance key (csrc/common.h, order_key32: (key - anchor) >> 24, the anchor from the smallest high word of the row's
keys, one code from sixteen binades above it on, the top code for an entry without a distance), sixteen keys per trip
from a list padded with the top code; two elements with one image meet on one slot and the row is ordered again on
(key, position).  Nothing of that may show: every output here is held to the oracle's bits, which is numpy's stable
argsort on (distance, position).

The matrices have one to three samples (sixteen with thirteen zero columns where the pairwise order's kernel is
meant: fewer than eight samples are summed sequentially whatever the order), so that a distance is a sum of exactly
representable squares and the test chooses its bits.  Two chromosomes: two target rows, then n candidate rows; every
threshold at FLT_MAX, so a target's list is the other chromosome.  Near-tie candidates (sample values (+-2,
1 + j 2^-25, m 2^-25) against a target at 0) lie at

    d = 5 + j 2^-24 + (j^2 + m^2) 2^-50      (every term a multiple of the ulp 2^-50: exact)

all within 3e-5 of each other -- far inside the slack of the float16 bounds, so k_pick hands over ALL n of them
whatever the refsize -- and j moves bit 26 of the key (distinct images), m only bits below 24 (one image).  The +-2
column keeps the scale of the float16 image at the size of the values (no row is clamped) and adds exactly 4.
A refsize of 100 runs workgroups of two waves (a second trip from pair 128 on), 256 runs five waves.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
SH = 24                                  # the kernel's shift (test_order_key_cpu.py holds the exported rule to it)
U25 = 2.0 ** -25


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def finish(data, bins, k, order):
    """prepare / thresholds / every threshold FLT_MAX / collect / finish -> (idx, dst, stats)"""
    import torch
    from wisecondor_amd import _lib, distributed, wisetools
    B = data.shape[0]
    X = torch.from_numpy(np.array(data, order="C")).cuda()
    st = distributed.HipStages(_lib.context(0), X, np.asarray(bins, dtype=np.int64), k,
                               _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)
    st.prepare()
    st.thresholds(0, B)
    st.set_thr(0, B, torch.full((B,), float(FMAX), dtype=torch.float32, device="cuda"))
    st.collect(0, B, 0, 1)
    idx = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    dst = torch.full((B, k), float("nan"), dtype=torch.float64, device="cuda")
    st.finish(0, B, idx, dst)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dst.cpu().numpy(), wisetools.newref_stats(0)


def oracle(data, bins, k, order):
    laid = np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)
    with np.errstate(all="ignore"):
        return wo.get_reference(laid, np.asarray(bins), np.cumsum(bins), k, 1, 1, fast=True)


def widen(data, samples):
    """the same rows with zero columns up to `samples` (adds +0.0 to every distance)"""
    out = np.zeros((data.shape[0], samples))
    out[:, :data.shape[1]] = data
    return out


def near_ties(j, m, a_first=None):
    """Two targets (0, 0, 0), (0, 0.5, 0) and len(j) candidates (+-2, 1 + j 2^-25, m 2^-25); a_first: other second
    values for the leading candidates.  -> data, bins, the exact distances of target 0"""
    j = np.asarray(j, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    n = len(j)
    a = 1.0 + j * U25
    if a_first is not None:
        a[:len(a_first)] = a_first
    sign = np.where(np.random.RandomState(5).rand(n) < 0.5, -2.0, 2.0)
    data = np.zeros((2 + n, 3))
    data[1, 1] = 0.5
    data[2:, 0], data[2:, 1], data[2:, 2] = sign, a, m * U25
    d = (4.0 + a * a) + (m * U25) * (m * U25)
    assert np.all(d == 4.0 + (a * a + (m * U25) ** 2))          # exact: no rounding in either order
    return data, (2, n), d


def check(data, bins, k, order, d0=None, fast=True, samples=None):
    """output == oracle, bit for bit; target 0 also against numpy's stable argsort of its distances d0"""
    if samples:
        data = widen(data, samples)
    idx, dst, stats = finish(data, bins, k, order)
    print("bins %s k %d order %s samples %d: %s" % (bins, k, order, data.shape[1], stats))
    want_i, want_d = oracle(data, bins, k, order)
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    if d0 is not None:
        ok = np.flatnonzero(d0 < 1e10)                          # NaN and >= 1e10 are never admitted
        pos = ok[np.argsort(d0[ok], kind="stable")][:k]
        assert np.array_equal(idx[0, :len(pos)], pos) and same_bits(dst[0, :len(pos)], d0[pos])
        assert (idx[0, len(pos):] == -1).all() and (dst[0, len(pos):] == 1e10).all()
    if fast:
        # every row went through k_rescore, the targets with all n pairs, the candidates with the two targets
        B = data.shape[0]
        assert stats["fast_rows"] == B and stats["fallback_rows"] == 0, stats
        assert stats["rescored"] == 2 * (B - 2) + 2 * (B - 2), stats
    return idx, dst


ORDERS = [("F", None), ("C", None), ("C", 16)]       # ("C", 16): sixteen samples in the pairwise order, k_rescore<false, true>


def image(d, shift=-1):
    """the exported host form of the rule on float64 distances"""
    from wisecondor_amd import _lib
    key = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    key = np.where(key >> np.uint64(63), ~key, key | np.uint64(1 << 63))
    key[~(np.asarray(d) < 1e10)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    key = np.ascontiguousarray(key)
    out = np.zeros(key.shape, dtype=np.uint32)
    mn = np.zeros(1, dtype=np.uint32)
    _lib.check(_lib.load().wc_order_key_host(_lib.ptr(key), key.size, shift, _lib.ptr(out), _lib.ptr(mn)))
    return out


# ---------------------------------------------------------------- images that collide, keys that differ ----
@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("swap", [False, True])
def test_keys_that_differ_only_below_the_shift(swap, order, samples):
    """candidates 3 and 7 share j (one image) and differ in m (bits 0 and 2 of the key): the sweep on the full key
    decides, in both position orders; the other candidates have images of their own"""
    n = 12
    j = np.arange(n) * 2.0 + 1.0
    m = np.zeros(n)
    j[7] = j[3]
    m[3], m[7] = (2.0, 1.0) if swap else (1.0, 2.0)
    data, bins, d0 = near_ties(j, m)
    r = image(d0)
    assert r[3] == r[7] and d0[3] != d0[7] and len(set(r)) == n - 1
    idx, _ = check(data, bins, 100, order, d0, samples=samples)
    at3, at7 = list(idx[0]).index(3), list(idx[0]).index(7)
    assert (at3 < at7) == (not swap) and abs(at3 - at7) == 1


@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("n,tied", [(9, (2, 6)), (9, (7, 1, 4)), (9, tuple(range(9))), (130, tuple(range(130))),
                                    (70, (69, 0, 64))])
def test_exact_ties_are_ordered_by_position(n, tied, order, samples):
    """two, three and all pairs of a row at one distance (130: both waves and a second trip; (69, 0, 64): across the
    waves)"""
    j = np.random.RandomState(n).permutation(n) * 2.0 + 1.0
    j[list(tied)] = j[tied[0]]
    data, bins, d0 = near_ties(j, np.zeros(n))
    assert len(set(d0[list(tied)])) == 1
    idx, _ = check(data, bins, 100, order, d0, samples=samples)
    got = [p for p in idx[0] if p in tied]
    assert got == sorted(tied)[:len(got)]


# ------------------------------------------------------------------------------- the range of the image ----
def one_sample(values):
    """targets 0 and 3, candidates `values`, one sample: d = v^2, exact for values of at most 26 bits"""
    v = np.asarray(values, dtype=np.float64)
    data = np.concatenate([[0.0, 3.0], v])[:, None]
    with np.errstate(all="ignore"):
        d = v * v
    return data, (2, len(v)), d


BIG = [60000.0 + 1317.0 * i for i in range(30)] + [99498.0]            # up to d = 9.8999e9: keeps the scale large


@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("with_zero", [True, False])
def test_more_than_sixteen_binades(with_zero, order, samples):
    """0.0 from a row identical to the target beside 9.9e9: anchored at 0 every other key is beyond the image's range
    (one code: the full keys decide); anchored at 2^-40 the near ones have images, the far ones share one"""
    small = [2.0 ** -20, 1.0, 2.0 ** -10, 33.0, 2.0 ** -4, 1025.0, 2.0 ** -14, 5.0, 2.0 ** -20 * 1.5, 3.0 * 2.0 ** -18]
    values = BIG[:15] + ([0.0] if with_zero else []) + small + BIG[15:]
    values = list(np.random.RandomState(3).permutation(values))
    data, bins, d0 = one_sample(values)
    assert d0.max() > 9.89e9 and d0.max() < 1e10
    r = image(d0)
    if with_zero:
        assert sorted(set(r)) == [0, 0xFFFFFFFE]
    else:
        assert d0.min() == 2.0 ** -40 and 4 < len(set(r)) < len(values) and max(r) == 0xFFFFFFFE
    check(data, bins, 100, order, d0, samples=samples)


@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("far", [(4,), (0, 4, 5, 11), tuple(range(1, 40, 2))])
def test_entries_at_or_beyond_1e10(far, order, samples):
    """one, several and half of the pairs without a distance (1e10 itself is one): after every real one, -1 / 1e10"""
    values = list(np.random.RandomState(len(far)).permutation(BIG + [1.0, 2.0, 7.0, 99999.0, 12.0, 640.0, 99999.5,
                                                                     8191.0, 3.5]))
    for q, p in enumerate(far):
        values[p] = 100000.0 if q == 0 else 100000.0 + 4096.0 * q
    data, bins, d0 = one_sample(values)
    assert d0[far[0]] == 1e10 and (d0 >= 1e10).sum() == len(far)
    assert (image(d0) == 0xFFFFFFFF).sum() == len(far)
    idx, dst = check(data, bins, 100, order, d0, samples=samples)
    assert (idx[0, len(values) - len(far):] == -1).all() and not set(idx[0]) & set(far)


@pytest.mark.parametrize("order", ["F", "C"])
def test_nan_candidates(order):
    """rows with a NaN have no bounds and are never listed: the targets' lists are the finite rows (a single one in
    the second matrix: the only way to a row of one pair, a lone candidate row being a chromosome layout of its own);
    which path a row takes is the library's business here, the output is not"""
    for values in ([5.0, np.nan, 1.0, 3.0, np.nan, 2.0], [np.nan, 4.0, np.nan]):
        data, bins, d0 = one_sample(values)
        check(data, bins, 100, order, d0, fast=False)


# ------------------------------------------------------------------------- where the smallest key sits ----
@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("at", [0, 63, 70, 127, 150, 199])
def test_the_minimum_in_any_wave_and_trip(at, order, samples):
    """200 pairs on two waves are two trips; one candidate lies a quarter of a binade below the others (d = 4.25:
    a smaller HIGH word, the anchor), in the first or second wave, in the first or second trip"""
    n = 200
    j = np.random.RandomState(at).permutation(n) * 2.0 + 1.0
    data, bins, d0 = near_ties(j, np.zeros(n))
    data[2 + at, 1] = 0.5
    d0[at] = 4.25
    assert image(d0)[at] == 0 and len(set(image(d0))) == n
    idx, _ = check(data, bins, 100, order, d0, samples=samples)
    assert idx[0, 0] == at


# ----------------------------------------------------------------------------- every pad and trip edge ----
COUNTS = [2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 101, 102, 127, 128, 129, 512]


def count_case(n):
    """n candidates: distinct images, but for every seventh pair (an image shared with its neighbour, keys apart)"""
    rng = np.random.RandomState(n)
    j = rng.permutation(n) * 2.0 + 1.0
    m = np.zeros(n)
    if n >= 15:
        for p in range(3, n - 1, 7):
            j[p + 1] = j[p]
            m[p], m[p + 1] = rng.permutation([1.0, 3.0])
    return near_ties(j, m)


@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("n", COUNTS)
def test_pair_counts_two_waves(n, order, samples):
    """refsize 100: workgroups of 128 threads, trips of 128 pairs (512 = RMAX: four)"""
    data, bins, d0 = count_case(n)
    check(data, bins, 100, order, d0, samples=samples)


@pytest.mark.parametrize("order,samples", ORDERS)
@pytest.mark.parametrize("n", [c for c in COUNTS if c > 100])
def test_pair_counts_five_waves_every_rank_delivered(n, order, samples):
    """refsize 256: workgroups of 320 threads; up to 255 pairs every rank of the row is in the output"""
    data, bins, d0 = count_case(n)
    check(data, bins, 256, order, d0, samples=samples)


@pytest.mark.parametrize("n", [c for c in COUNTS if c < 15])
def test_pair_counts_distinct_images(n):
    """the short rows once more with an image of its own for every pair: the first sweep's ranks are the output"""
    data, bins, d0 = near_ties(np.random.RandomState(50 + n).permutation(n) * 2.0 + 1.0, np.zeros(n))
    assert len(set(image(d0))) == n
    check(data, bins, 100, "F", d0)


def test_a_short_row_behind_rmax_pairs():
    """512 pairs, then 5 in the same context: whatever the long row's rank keys left behind the short row's pad is
    never counted"""
    data, bins, d0 = count_case(512)
    check(data, bins, 100, "F", d0)
    short = near_ties([9.0, 1.0, 7.0, 3.0, 5.0], np.zeros(5))
    first = check(short[0], short[1], 100, "F", short[2])
    second = check(short[0], short[1], 100, "F", short[2])
    assert np.array_equal(first[0], second[0]) and same_bits(first[1], second[1])
    assert list(first[0][0, :5]) == [1, 3, 4, 2, 0]
