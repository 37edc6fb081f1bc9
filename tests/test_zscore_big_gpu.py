"""The z-score route of `-refsize` above 128 (`k_zscore_big` for every repeat: the kept references of a (bin, sample)
pair compacted into LDS, 64 list entries per trip, and summed by `wc::pw_node_group8<4>`; `k_flag` / `k_flag_pairs`
for the flags) against numpy's bits at EVERY number of kept references and every tree shape, not only at the counts
one data set happens to give.

Reference lists (`long_lists`): chromosomes of a, b, 1 and c bins; a bin's list is k distinct draws from the other
chromosomes' bins, its distances ascending in [0, 0.5), and the entries from position cnt[b] on at distance 2.0 --
beyond the cutoff 0.8 -- with cnt a shuffled arange(B) % (k + 1): bin b has exactly cnt[b] references below the
cutoff and every list length 0 .. k occurs.  The reference is the numpy oracle (`wo.repeat_test`, `wo.test_sample`);
z, ratio and the sd average are compared bit for bit (NaN equals NaN), the kept counts with np.array_equal."""
import functools
import os

import numpy as np
import pytest

from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
SWEEP = int(os.environ.get("WC_SWEEP", "1"))      # WC_SWEEP=8: eight times the seeds of the two sweeps
CUTOFF = 0.8
# every chromosome leaves at least k bins on the others, and B >= k + 1
LAYOUTS = {129: (150, 140, 1, 30), 136: (160, 150, 1, 30), 257: (290, 270, 1, 35), 300: (330, 310, 1, 40),
           520: (570, 550, 1, 45), 1024: (1100, 1100, 1, 60)}


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def long_lists(k, seed, layout=None):
    """(idx, dst, bins, sums, cnt) as the module's docstring says; shared between tests, never written to."""
    rng = np.random.RandomState(7000 + 13 * k + seed)
    bins = np.array(layout or LAYOUTS[k], dtype=np.int64)
    sums = np.cumsum(bins)
    B = int(sums[-1])
    assert B >= k + 1 and B - int(bins.max()) >= k
    idx = np.empty((B, k), dtype=np.int32)
    for c in range(len(bins)):
        lo, hi = int(sums[c] - bins[c]), int(sums[c])
        idx[lo:hi] = np.argsort(rng.rand(hi - lo, B - (hi - lo)), axis=1)[:, :k]     # k distinct places among the others
    dst = np.sort(0.5 * rng.rand(B, k), axis=1)
    cnt = rng.permutation(np.arange(B) % (k + 1))
    dst[np.arange(k)[None, :] >= cnt[:, None]] = 2.0
    return frozen(idx, dst, bins, sums, cnt)


def oracle_repeats(x, idx, dst, bins, sums, thr, repeats):
    """wo.repeat_test, and what each of its repeats returned on the way (its own calls of try_sample, recorded)."""
    passes = []
    inner = wo.try_sample

    def recording(*args):
        out = inner(*args)
        passes.append(out)
        return out
    wo.try_sample = recording
    try:
        with np.errstate(all="ignore"):
            out = wo.repeat_test(x, idx, dst, bins, sums, CUTOFF, thr, repeats)
    finally:
        wo.try_sample = inner
    assert len(passes) == repeats
    return out, passes


def assert_rows_match(got, want, what):
    z, r, n, sd = got
    for s, (wz, wr, wn, wsd) in enumerate(want):
        assert np.array_equal(n[s], wn), (what, s, np.flatnonzero(n[s] != wn)[:8])
        bad = np.flatnonzero(~(np.isnan(z[s]) & np.isnan(wz)) & (z[s].view(np.int64) != wz.view(np.int64)))
        assert same_bits(z[s], wz), (what, s, "kept counts of the first differing bins", wn[bad[:8]])
        assert same_bits(r[s], wr), (what, s)
        assert same_bits([sd[s]], [wsd]), (what, s)


def assert_same_outputs(got, want, what):
    for a, b, name in zip(got, want, ("z", "ratio", "kept", "sd average")):
        assert same_bits(a, b), (what, name)


# ------------------------------------------------------------------ 1. every kept count, first repeat ----
N_QUIET = 17


@functools.lru_cache(maxsize=None)
def quiet_case(k, seed, scaled):
    """17 quiet samples (nothing negative, no NaN; `scaled`: times 10**U(-3, 3) per bin, so that the order of the
    additions shows in the last bits) and the oracle's first repeat of each."""
    idx, dst, bins, sums, cnt = long_lists(k, seed)
    B = int(sums[-1])
    rng = np.random.RandomState(8000 + 17 * k + 2 * seed + int(scaled))
    data = 1.0 + 0.05 * rng.standard_normal((N_QUIET, B))
    if scaled:
        data = data * 10.0 ** rng.uniform(-3, 3, size=(N_QUIET, B))
    assert data.min() > 0
    want = [oracle_repeats(data[s], idx, dst, bins, sums, np.inf, 1)[0] for s in range(N_QUIET)]
    return frozen(data)[0], want


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("k,seed", [(k, s) for k in (129, 136, 257, 300, 520, 1024) for s in range(SWEEP)])
def test_every_kept_count_first_repeat(wt, k, seed, scaled):
    """Lists of every length 0 .. k in one call: no kept value (NaN mean), one (sd 0: z is +-inf or NaN), fewer than
    eight inside a long list, every n % 8 tail, every split of numpy's tree up to four levels, every fill of the
    64-entry compaction trips.  1, 3 and 17 samples: none a multiple of 16."""
    idx, dst, bins, sums, cnt = long_lists(k, seed)
    data, want = quiet_case(k, seed, scaled)
    seen = set()
    for _, _, wn, _ in want:
        assert np.array_equal(wn, cnt)                       # nothing but the cutoff drops a reference here
        seen.update(int(v) for v in wn)
    assert seen == set(range(k + 1)), "a kept count between 0 and %d does not occur" % k
    for ns in (1, 3, N_QUIET):
        got = wt.repeatTest(data[:ns], idx, dst, bins, sums, CUTOFF, np.inf, 1)
        assert_rows_match(got, want[:ns], (k, seed, scaled, ns))


# ------------------------------------------------------------------ 2. heavy flagging, later repeats ----
def heavy_samples(rng, n_samples, B):
    """The data of test_random_gpu.test_repeats_heavy_flagging: 8 % of the values x 1.5, 0.3 % negative, 0.2 % NaN."""
    data = 1.0 + 0.05 * rng.standard_normal((n_samples, B))
    data[rng.rand(n_samples, B) < 0.08] *= 1.5
    data[rng.rand(n_samples, B) < 0.003] = -0.5
    data[rng.rand(n_samples, B) < 0.002] = np.nan
    return data


HEAVY_THR, HEAVY_REPEATS = 1.5, 6


@functools.lru_cache(maxsize=None)
def heavy_case(k, n_samples, seed, layout=None):
    idx, dst, bins, sums, cnt = long_lists(k, seed, layout)
    rng = np.random.RandomState(9000 + 19 * k + seed)
    return frozen(heavy_samples(rng, n_samples, int(sums[-1])))[0]


@functools.lru_cache(maxsize=None)
def heavy_oracle(k, n_samples, seed):
    idx, dst, bins, sums, cnt = long_lists(k, seed)
    data = heavy_case(k, n_samples, seed)
    return [oracle_repeats(data[s], idx, dst, bins, sums, HEAVY_THR, HEAVY_REPEATS) for s in range(n_samples)]


@pytest.mark.parametrize("k,n_samples,seed", [(k, ns, 1 + s) for k, ns in ((129, 20), (300, 8), (1024, 4))
                                              for s in range(SWEEP)])
def test_heavy_flagging_later_repeats(wt, k, n_samples, seed):
    """A low threshold on noisy samples: every repeat adds flags, `k_flag` / `k_flag_pairs` queue the users of each
    new flag and `k_zscore_big` recomputes them from its pair list -- lists that lose references repeat after repeat,
    the tree's shape changing with them.  The sixth repeat still has work to do in every sample."""
    idx, dst, bins, sums, cnt = long_lists(k, seed)
    data = heavy_case(k, n_samples, seed)
    oracle = heavy_oracle(k, n_samples, seed)
    for s, (_, passes) in enumerate(oracle):
        changed = int(np.sum(passes[-2][2] != passes[-1][2]))
        assert changed >= 1, "sample %d: the last repeat changes no kept count" % s
    got = wt.repeatTest(data, idx, dst, bins, sums, CUTOFF, HEAVY_THR, HEAVY_REPEATS)
    assert_rows_match(got, [out for out, _ in oracle], (k, seed))


# ------------------------------------------------------------------ 3. special values in long lists ----
def test_special_values_in_long_lists(wt):
    """k = 300: lists whose kept values are all equal (variance exactly 0 at 1.25; at 1.1 whatever numpy's rounding
    of the mean leaves), +inf, -0.0 (kept: -0.0 >= 0) and a single NaN among the references of a full list, a sample
    that is negative everywhere (every list empty), and a list of two that the first repeat's flags empty."""
    k = 300
    idx, dst, bins, sums, cnt = long_lists(k, 0)
    B = int(sums[-1])
    rng = np.random.RandomState(31)
    starts = sums - bins

    def chrom_of(b):
        return int(np.searchsorted(sums, b, side="right"))

    def refs_of(b):
        """bin numbers of the references of bin b below the cutoff"""
        c = chrom_of(b)
        p = idx[b, :cnt[b]].astype(np.int64)
        return np.where(p < starts[c], p, p + bins[c])
    full = int(np.flatnonzero(cnt == k)[0])
    c_full = chrom_of(full)
    own = slice(int(starts[c_full]), int(sums[c_full]))               # never among the references of `full`
    base = 1.0 + 0.05 * rng.standard_normal((7, B))
    rows = []
    for const, other in ((1.25, 1.5), (1.1, 0.9)):
        x = np.full(B, const)
        x[own] = other                 # the lists of this chromosome hold `const` only; the others' are mixed
        x[full] = const
        rows.append(x)
    x = base[2].copy()
    x[refs_of(full)[150]] = np.inf
    x[rng.randint(0, B, size=3)] = np.inf
    rows.append(x)
    x = base[3].copy()
    x[rng.rand(B) < 0.05] = -0.0
    x[refs_of(full)[7]] = -0.0
    rows.append(x)
    x = base[4].copy()
    x[refs_of(full)[299]] = np.nan
    rows.append(x)
    rows.append(-base[5])
    two = None
    for b in np.flatnonzero(cnt == 2):
        if np.all(cnt[refs_of(b)] >= 60):
            two = int(b)
    assert two is not None
    x = base[6].copy()
    x[refs_of(two)] = 3.0              # against lists of sixty quiet values or more: flagged in the first repeat
    rows.append(x)
    data = np.stack(rows)
    thr, repeats = 3.0, 3
    oracle = [oracle_repeats(row, idx, dst, bins, sums, thr, repeats) for row in data]
    first = [passes[0] for _, passes in oracle]
    # the cases are what they claim to be
    z0, _, n0, _ = first[0]
    assert n0[full] == k and np.isnan(z0[full])                       # (1.25 - 1.25) / 0
    assert np.any(np.isposinf(z0[own]) & (n0[own] > 128))             # (1.5 - 1.25) / 0
    assert first[1][2][full] == k
    assert np.isnan(first[2][1][full]) or first[2][1][full] == 0.0    # mean +inf: ratio x / inf
    assert first[3][2][full] == k                                     # -0.0 is kept
    assert first[4][2][full] == k - 1                                 # the NaN is not
    assert not np.any(first[5][2]) and np.all(np.isnan(first[5][0]))
    assert first[6][2][two] == 2 and oracle[6][1][1][2][two] == 0 and np.isnan(oracle[6][0][0][two])
    got = wt.repeatTest(data, idx, dst, bins, sums, CUTOFF, thr, repeats)
    assert_rows_match(got, [out for out, _ in oracle], "special values")
    # and each row in a call of its own (one sample: another grid)
    for s in (0, 5, 6):
        alone = wt.repeatTest(data[s:s + 1], idx, dst, bins, sums, CUTOFF, thr, repeats)
        assert_rows_match(alone, [oracle[s][0]], ("special values, alone", s))


# ------------------------------------------------------------------ 4. the boundary: k = 128 against k > 128 ----
def widen(idx, dst, bins, extra):
    """`extra` more columns at distance 2.0 (never kept), their indices distinct from the row's own."""
    B, k = idx.shape
    sums = np.cumsum(bins)
    wide_i = np.empty((B, k + extra), dtype=np.int32)
    wide_d = np.full((B, k + extra), 2.0)
    wide_i[:, :k] = idx
    wide_d[:, :k] = dst
    for c in range(len(bins)):
        others = np.arange(B - int(bins[c]))
        for b in range(int(sums[c] - bins[c]), int(sums[c])):
            wide_i[b, k:] = np.setdiff1d(others, idx[b], assume_unique=True)[-extra:]
    return wide_i, wide_d


@pytest.mark.parametrize("layout,n_samples", [((330, 310, 1, 40), 3), ((330, 310, 1, 40), 128), ((330, 320, 1, 49), 100)])
def test_longer_lists_with_the_same_kept_references(wt, layout, n_samples):
    """One implementation against the other, no oracle: a refsize-128 reference (`k_zscore_pairs` at 3 samples,
    `k_zscore` at 100, `k_zscore_tiled` at 128, `k_zscore_pairs` for the later repeats -- each held to the oracle by
    test_random_gpu) and the same lists followed by 1, 8 and 172 entries beyond the cutoff, which send every repeat to
    `k_zscore_big` without changing a single kept reference.  87 168 and 70 000 (bin, sample) pairs: more than the
    65 536 of one trip of the kernel's grid stride."""
    k = 128
    idx, dst, bins, sums, cnt = long_lists(k, 2, layout)
    data = heavy_case(k, n_samples, 2, layout)
    want = wt.repeatTest(data, idx, dst, bins, sums, CUTOFF, HEAVY_THR, HEAVY_REPEATS)
    assert np.max(want[2]) > 64 and np.min(want[2]) == 0          # lists of more than one compaction trip, and empty ones
    for extra in (1, 8, 172):
        wide_i, wide_d = widen(idx, dst, bins, extra)
        # (other values into the context's result arrays first: a pair the kernel skipped must not find the
        #  run before's result of the same pair still standing there)
        wt.repeatTest(np.roll(data[::-1], 7, axis=1), wide_i, wide_d, bins, sums, CUTOFF, HEAVY_THR, 1)
        got =wt.repeatTest(data, wide_i, wide_d, bins, sums, CUTOFF, HEAVY_THR, HEAVY_REPEATS)
        assert_same_outputs(got, want, (n_samples, k + extra))


# ------------------------------------------------------------------ 5. the same bits every time ----
def test_same_bits_twice_and_after_a_shorter_job(wt):
    """The k = 1 024 call of the heavy-flagging test twice, and once more after a k = 129 call on the same context:
    the pair lists, the dirty bits and the counters of the context hold another job's contents by then."""
    idx, dst, bins, sums, cnt = long_lists(1024, 1)
    data = heavy_case(1024, 4, 1)

    def run():
        return wt.repeatTest(data, idx, dst, bins, sums, CUTOFF, HEAVY_THR, HEAVY_REPEATS)
    first = run()
    assert_same_outputs(run(), first, "second run")
    s_idx, s_dst, s_bins, s_sums, _ = long_lists(129, 1)
    short = heavy_case(129, 20, 1)
    wt.repeatTest(short, s_idx, s_dst, s_bins, s_sums, CUTOFF, HEAVY_THR, HEAVY_REPEATS)
    assert_same_outputs(run(), first, "after a k = 129 call")
    assert_rows_match(first, [out for out, _ in heavy_oracle(1024, 4, 1)], "k = 1 024")


# ------------------------------------------------------------------ 6. the whole `test` call ----
def close_or_both_nan(a, b):
    """within 1e-9 relative (the full path's contract: the PCA projection is not bit-reproducible), NaN equals NaN"""
    return bool(np.allclose(a, b, rtol=1e-9, atol=0.0, equal_nan=True))


@pytest.mark.parametrize("k,lo,hi,repeats", [(300, 40, 70, 4), (1024, 60, 80, 3)])
def test_whole_test_call_with_long_lists(wt, k, lo, hi, repeats):
    """A reference from the GPU newref at refsize 300 and 1 024 (built like test_random_gpu.test_degenerate_samples),
    20 Poisson samples -- a third with a planted gain or loss -- in one `test_batch` call (the batch route, the sample
    count padded to 32; the latency route refuses refsize > 128) against the oracle's toolTest body, and each sample
    alone against its row of the batch bit for bit."""
    rng = np.random.RandomState(600 + k)
    sizes = rng.randint(lo, hi, size=22).astype(np.int64)
    total = int(sizes.sum())
    mask = rng.rand(total) > 0.05
    offs = np.concatenate([[0], np.cumsum(sizes)])
    msizes = np.array([int(mask[offs[i]:offs[i + 1]].sum()) for i in range(22)], dtype=np.int64)
    B = int(msizes.sum())
    assert B - int(msizes.max()) >= k                        # every bin has k candidates on other chromosomes
    corrected = 1.0 + 0.02 * rng.standard_normal((B, 20))
    idx, dst = wt.getReference(np.asfortranarray(corrected), msizes, np.cumsum(msizes), k, 1, 1)
    comps = np.linalg.qr(rng.standard_normal((B, 3)))[0].T
    mean = np.full(B, 1.0 / B) * (1 + 0.01 * rng.standard_normal(B))
    ref = dict(binsize=np.float64(1e6), indexes=idx, distances=dst, chromosome_sizes=sizes, mask=mask,
               masked_sizes=msizes, pca_mean=mean, pca_components=comps)
    samples = []
    for s in range(20):
        lam = np.full(total, 3000.0) * (1 + 0.02 * rng.standard_normal(total)).clip(0.5)
        if s % 3 == 0:
            c = rng.randint(0, 22)
            a = offs[c] + rng.randint(0, sizes[c] - 14)
            lam[a:a + rng.randint(8, 14)] *= rng.choice([0.6, 1.4])
        counts = rng.poisson(lam).astype(np.int32)
        samples.append({str(c + 1): counts[offs[c]:offs[c + 1]] for c in range(22)})
    thr, minref = 4.2, 25
    reference = wt.Reference(idx, dst, sizes, msizes, mask, mean, comps, binsize=1e6)
    try:
        outs = wt.test_batch(reference, samples, thr, minrefbins=minref, repeats=repeats)
        alone = [wt.test_batch(reference, [s], thr, minrefbins=minref, repeats=repeats)[0] for s in samples]
    finally:
        reference.close()
    for i, (a, b) in enumerate(zip(alone, outs)):
        for key in ("results_z", "results_r"):
            assert same_bits(np.concatenate(a[key]), np.concatenate(b[key])), (i, key)
        assert same_bits(a["results_cwz"], b["results_cwz"]), i
        assert same_bits(np.asarray(a["results_calls"]).reshape(-1, 5), np.asarray(b["results_calls"]).reshape(-1, 5)), i
        assert same_bits([a["asdef"]], [b["asdef"]]), i
    n_calls, longest = 0, 0
    for i, (sample, out) in enumerate(zip(samples, outs)):
        with np.errstate(all="ignore"):
            want = wo.test_sample(sample, 1e6, ref, minzscore=thr, minrefbins=minref, repeats=repeats)
        wc_ = np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5)
        gc_ = np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)
        assert np.array_equal(gc_[:, :3], wc_[:, :3]), (i, gc_, wc_)
        assert close_or_both_nan(gc_[:, 3:], wc_[:, 3:]), (i, gc_, wc_)
        assert close_or_both_nan(np.concatenate(out["results_z"]), np.concatenate(want["results_z"])), i
        assert close_or_both_nan(np.concatenate(out["results_r"]), np.concatenate(want["results_r"])), i
        assert close_or_both_nan(out["results_cwz"], want["results_cwz"]), i
        n_calls += len(wc_)
        longest = max(longest, int(np.max(want["ref_sizes"])))
    assert n_calls >= 1
    assert longest > 128                                     # the final lists really are longer than one block


# ------------------------------------------------------------------ 7. limits ----
def test_refsize_limit(wt):
    """refsize 1 024 is taken, 1 025 refused with the library's message, and the context works afterwards."""
    from wisecondor_amd import _lib
    idx, dst, bins, sums, cnt = long_lists(1024, 0)
    B = int(sums[-1])
    accepted = wt.Reference(idx, dst, bins, bins, np.ones(B, np.uint8), np.zeros(B), np.zeros((0, B)), cutoff=CUTOFF)
    assert accepted.k == 1024
    accepted.close()
    wide_i = np.concatenate([idx, idx[:, :1]], axis=1)
    wide_d = np.concatenate([dst, np.full((B, 1), 2.0)], axis=1)
    with pytest.raises(_lib.WisecondorHipError, match=r"unsupported shape .*refsize 1025 \(max 1024\)"):
        wt.repeatTest(np.ones(B), wide_i, wide_d, bins, sums, CUTOFF, 3.0, 1)
    s_idx, s_dst, s_bins, s_sums, _ = long_lists(129, 0)
    data, want = quiet_case(129, 0, False)
    got = wt.repeatTest(data[:3], s_idx, s_dst, s_bins, s_sums, CUTOFF, np.inf, 1)
    assert_rows_match(got, want[:3], "after the refusal")
