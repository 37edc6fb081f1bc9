"""zscore_batch_cases.py held to what test_zscore_batch_gpu.py relies on, from the oracle alone: the layouts and lists,
every kept count, the value classes and wave classes of the special variant, the composed expectation against
wo.test_sample, and the work the later-repeat cases leave for repeats 3 and 4."""
import numpy as np
import pytest

import zscore_batch_cases as zc
from oracle import wc_oracle as wo

KS = tuple(dict.fromkeys(zc.ALL_K + zc.K_LATE))


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


def test_checked_samples():
    """At least 16 samples per call: sample 0, the last real one, one of every leftover tile, one of a full tile."""
    for n_samples in zc.CALL_SIZES:
        got = zc.checked(n_samples)
        tiles = {s // 16 for s in got}
        n_tiles = (n_samples + 15) // 16
        assert set(range(n_tiles & ~7, n_tiles)) <= tiles and tiles & set(range(n_tiles & ~7)), (n_samples, tiles)
    assert [(-n) % 16 for n in zc.CALL_SIZES] == [15, 0, 0, 8]         # only the calls of 113 and 232 are padded
    assert [((n + 15) // 16) % 8 for n in zc.CALL_SIZES] == [0, 0, 1, 7]   # leftover tiles
    assert int(zc.call_weights(113)[0]) == 16 and int(zc.call_weights(113).sum()) == 128


def test_layouts_cover_both_residues():
    for family in (zc.K_SM, zc.K_ODD, zc.K_BM):
        assert {zc.case(k, "quiet").B % 4 for k in family} == {1, 3}
    assert all(k % 4 == 0 and k <= 100 for k in zc.K_SM) and all(k % 4 for k in zc.K_ODD)
    assert all(100 < k <= 128 for k in zc.K_BM) and 103 in zc.K_BM and 104 in zc.K_BM


@pytest.mark.parametrize("k,variant", [(k, v) for k in KS for v in ("quiet", "special")] + [(k, "quiet22") for k in zc.K_LATE])
def test_lists(k, variant):
    c = zc.case(k, variant)
    assert len(c.sizes) == 22 and int(c.sizes[2]) == 1 and c.B % 4 in (1, 3)
    assert c.B >= k + 1 and c.B - int(c.sizes.max()) >= k + 8
    assert sorted(c.cnt.tolist()) == sorted((np.arange(c.B) % (k + 1)).tolist())
    assert set(c.cnt.tolist()) == set(range(k + 1))                        # every kept count occurs
    assert c.comps.shape == (0, c.B) and not np.any((c.mean == 0) & np.signbit(c.mean))
    assert c.counts.shape == (zc.N_SAMPLES, c.B) and c.counts.dtype == np.int32
    for b in range(c.B):
        ch = int(np.searchsorted(c.sums, b, side="right"))
        n = int(c.cnt[b])
        row = c.idx[b]
        real = row[row >= 0]
        assert len(set(real.tolist())) == len(real) and np.all(real < c.B - int(c.sizes[ch]))
        assert np.all(c.dst[b, :n] < 0.5) and np.all(np.diff(c.dst[b, :n]) >= 0) and np.all(c.dst[b, n:] == 2.0)
        assert np.all(row[n:] >= 0)                                        # -1 only at kept positions
        own = zc.global_refs(c, b)
        assert not np.any((own >= c.sums[ch] - c.sizes[ch]) & (own < c.sums[ch]))
    minus = int(np.sum(c.idx < 0))
    if variant == "special":
        assert len(c.special) == 6 and minus >= 4
        for b in np.flatnonzero(c.planted >= 0):
            nb = 8 * (int(c.cnt[b]) // 8)
            at = int(c.planted[b])
            assert zc.global_refs(c, b)[at] in c.special
            assert (nb <= at < c.cnt[b]) if c.group[b] == 1 else (at < nb and c.group[b] == 2)
        clean = np.flatnonzero(c.group == 0)
        assert not any(np.isin(zc.global_refs(c, b), c.special).any() for b in clean)
    else:
        assert len(c.special) == 0 and minus == 0 and np.all(c.counts > 0) and np.all(c.mean > 0)
    if variant == "quiet22":
        lo, hi = int(c.sums[zc.TAIL_CHROM - 1] - c.sizes[zc.TAIL_CHROM - 1]), int(c.sums[zc.TAIL_CHROM - 1])
        assert hi - lo >= 8 and np.all(c.cnt[lo:hi] >= 8)


@pytest.mark.parametrize("k", KS)
def test_quiet_variant_keeps_every_reference(k):
    """n == cnt: positive finite data in all 232 samples, and the oracle's kept counts of three of them."""
    c = zc.case(k, "quiet")
    for s in (0, 112, 231):
        x = zc.data_row(k, "quiet", 0, s)
        assert np.all(np.isfinite(x)) and np.all(x > 0)
        assert np.array_equal(zc.expect(k, "quiet", 0, s, np.inf, 1)[0][2], c.cnt)
    assert same_bits(zc.data_row(k, "quiet", 0, 5), c.counts[5] / np.float64(c.counts[5].sum()) / c.mean)


@pytest.mark.parametrize("k", KS)
def test_special_variant_classes(k):
    """Negative, -0.0, +inf, NaN and +0.0 all occur among the kept-position references of tile 0, and its waves split
    into the three classes.  Clean and tail-only waves: at least a fifth each at every k.  Body waves need a bin with
    eight kept references or more -- (k - 7) / (k + 1) of the bins: none below k = 8, a handful at k = 8 and 10 (one
    is asked for), a fifth of the waves from k = 12 on."""
    seen = zc.value_classes(k, "special", 0, range(16))
    assert all(seen.values()), seen
    waves = zc.wave_classes(k, "special", 0)
    total = sum(waves.values())
    assert total == (zc.case(k, "special").B + 3) // 4
    assert 5 * waves["clean"] >= total and 5 * waves["tail_only"] >= total, waves
    if k >= 12:
        assert 5 * waves["body"] >= total, waves
    elif k >= 8:
        assert waves["body"] >= 1, waves
    else:
        assert waves["body"] == 0, waves
    quiet = zc.wave_classes(k, "quiet", 0)
    assert quiet["tail_only"] == 0 and quiet["body"] == 0


@pytest.mark.parametrize("k,variant,seed,thr,chrom", [(100, "special", 0, zc.LOW_THR, 3), (104, "special", 0, 3.0, 22),
                                                      (40, "quiet22", zc.TAIL_SEED[40], zc.TAIL_THR[40], zc.TAIL_CHROM)])
def test_expectation_is_the_references_test(monkeypatch, k, variant, seed, thr, chrom):
    """results_of(expect(...)) is what wo.test_sample stores, bit for bit, once its cutoff is the Reference's 0.8."""
    c = zc.case(k, variant, seed)
    monkeypatch.setattr(wo, "get_optimal_cutoff", lambda distances, repeats: (zc.CUTOFF, None))
    for s, minrefbins, repeats in ((0, 8, 2), (130, 0, 1)):
        with np.errstate(all="ignore"):
            want = wo.test_sample(zc.sample_dict(c, s), 1e6, zc.reference_of(c), minzscore=thr, chromosomes=[chrom],
                                  minrefbins=minrefbins, repeats=repeats)
        out, passes = zc.expect(k, variant, seed, s, thr, repeats)
        rz, rr, asdef = zc.results_of(out, minrefbins)
        assert same_bits(rz, np.concatenate(want["results_z"])) and same_bits(rr, np.concatenate(want["results_r"]))
        assert same_bits([asdef], [want["asdef"]]) and want["cutoff"] == zc.CUTOFF
        assert same_bits(zc.data_row(k, variant, seed, s), want["data"])
        assert all(same_bits(a, b) for a, b in zip(out, passes[-1]))


def test_a_shorter_run_is_a_prefix_of_a_longer_one():
    """repeat_test's result after two repeats is what the second repeat of a run of five returned."""
    k, s = 40, 21
    two = zc.expect(k, "special", 0, s, zc.LOW_THR, 2)[0]
    five = zc.expect(k, "special", 0, s, zc.LOW_THR, zc.LATE_REPEATS)[1]
    assert all(same_bits(a, b) for a, b in zip(two, five[1]))
    assert not same_bits(five[1][0], five[4][0])


@pytest.mark.parametrize("k", [100, 99, 104])
def test_zero_pattern_of_the_expectation(k):
    """Where results_z and results_r are both zero is exactly where the kept count is below minrefbins (no kept bin
    has z == 0 and ratio == 1), and each minrefbins cuts somewhere else."""
    cut = []
    for minrefbins in (1, 8, k):
        n_cut = 0
        for s in zc.checked(144):
            out = zc.expect(k, "special", 0, s, np.inf, 1)[0]
            rz, rr, _ = zc.results_of(out, minrefbins)
            assert np.array_equal((rz == 0) & (rr == 0), out[2] < minrefbins)
            n_cut += int(np.sum(out[2] < minrefbins))
        cut.append(n_cut)
    assert 0 < cut[0] < cut[1] < cut[2]
    n = np.stack([zc.expect(k, "special", 0, s, np.inf, 1)[0][2] for s in range(16)])
    assert np.any(n.min(axis=0) != n.max(axis=0))          # the kept count differs between the samples of a tile


@pytest.mark.parametrize("k", zc.K_LATE)
def test_low_threshold_leaves_work_for_the_late_repeats(k):
    """Pairs whose z changes in repeats 3 and 4, over the checked samples of the call of 144 alone (a lower bound of
    the call's), and the pairs queued for them: hundreds and more than the one-workgroup form would take."""
    changed = np.zeros(zc.LATE_REPEATS - 1, dtype=np.int64)
    queued = np.zeros(zc.LATE_REPEATS - 1, dtype=np.int64)
    for s in zc.checked(144):
        ch, q = zc.late_work(k, "special", 0, s, zc.LOW_THR, zc.LATE_REPEATS)
        changed += ch
        queued += q
    print("k %d, thr %.1f, %d samples: changed %s queued %s" % (k, zc.LOW_THR, len(zc.checked(144)), changed, queued))
    assert changed[1] > 0 and changed[2] > 0
    assert queued[0] > 1000 and np.all(changed <= queued)


@pytest.mark.parametrize("k", zc.K_LATE)
def test_tail_case_fits_the_one_workgroup_form(k):
    """`quiet22` at its threshold, every sample of the calls of 128 and 144 (sample 0 once more per padding sample:
    none here): repeats 3 and 4 change z-scores, no repeat from the third on has more than TAIL_PAIR_CAP pairs queued,
    and chromosome 22's z-scores are finite after every repeat count the GPU test uses."""
    seed, thr = zc.TAIL_SEED[k], zc.TAIL_THR[k]
    c = zc.case(k, "quiet22", seed)
    lo, hi = int(c.sums[zc.TAIL_CHROM - 1] - c.sizes[zc.TAIL_CHROM - 1]), int(c.sums[zc.TAIL_CHROM - 1])
    for n_samples in (128, 144):
        w = zc.call_weights(n_samples)
        changed = np.zeros(zc.LATE_REPEATS - 1, dtype=np.int64)
        queued = np.zeros(zc.LATE_REPEATS - 1, dtype=np.int64)
        for s in range(n_samples):
            ch, q = zc.late_work(k, "quiet22", seed, s, thr, zc.LATE_REPEATS)
            changed += w[s] * np.array(ch)
            queued += w[s] * np.array(q)
            _, passes = zc.expect(k, "quiet22", seed, s, thr, zc.LATE_REPEATS)
            assert all(np.all(np.isfinite(p[0][lo:hi])) for p in passes)
        print("k %d, thr %.1f, %d samples: changed %s queued %s" % (k, thr, n_samples, changed, queued))
        assert changed[1] > 0 and changed[2] > 0                      # repeats 3 and 4
        assert np.all(changed[1:] <= zc.TAIL_PAIR_CAP) and np.all(queued[1:] <= zc.TAIL_PAIR_CAP)
        assert queued[1] > 0 and queued[2] > 0


@pytest.mark.parametrize("k", [100, 99, 104])
def test_edge_threshold_tells_greater_equal_from_greater(k):
    """The threshold is abs(z) of a first-repeat z-score; the next larger double leaves that bin unflagged and the
    second repeat's results differ: a `>` in place of `>=` shows in the bits."""
    for n_samples, s in zc.EDGE_CALLS:
        assert s in zc.checked(n_samples)
        thr, b = zc.edge_case(k, "special", 0, s)
        first = zc.expect(k, "special", 0, s, np.inf, 1)[0]
        assert np.isfinite(thr) and abs(first[0][b]) == thr
        at = zc.expect(k, "special", 0, s, thr, 2)[0]
        above = zc.expect(k, "special", 0, s, float(np.nextafter(thr, np.inf)), 2)[0]
        assert not same_bits(at[0], above[0])
        assert 1 <= int(np.sum(np.abs(first[0]) >= thr)) < zc.case(k, "special").B // 10
