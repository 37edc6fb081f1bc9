"""Inputs and the numpy expectation of the batch z-score tests (a helper module, not a conftest; modelled on
call_cases.py and prep_cases.py; checked on the CPU by test_zscore_batch_cases_cpu.py).

The production z-score route -- what wt.test_batch runs from 113 samples on: k_pca_apply_t writes the repeats' arrays,
k_zscore_tiled is the first repeat, k_flag_hits / k_zscore_pairs / k_flag_pairs / k_lat_repeats the later ones over
sample-major outputs -- is held to numpy's bits here at EVERY number of kept references of a list of k <= 128.

* Layout: 22 chromosomes, every bin unmasked, chromosome 3 a single bin, B bins with B % 4 == 3 or B % 4 == 1 (the
  tiled kernel's waves hold four consecutive bins: the last wave is short), every chromosome leaves at least k + 8
  bins to the others.
* Lists: idx[b] is k distinct positions among the other chromosomes' bins (the reference's "others" numbering),
  dst[b] ascending in [0, 0.5) and 2.0 -- beyond the cutoff CUTOFF, which the Reference is given -- from position
  cnt[b] on, cnt a shuffled arange(B) % (k + 1): every kept count 0 .. k occurs.
* No PCA components: data = x / pca_mean exactly (test_pca_apply_gpu.py), so everything behind it is numpy's bits.
* Samples: Poisson counts around 3 000.  The `special` variant has six special bins whose pca_mean makes their value
  negative or -0.0 (mean < 0), +inf or NaN (mean == 0) or +0.0 (ordinary mean), the second of each where the count
  is 0 -- 30 % of the special bins' counts are zeroed per sample, so a reference's class differs between the 16
  samples of a tile.  numpy keeps -0.0, +0.0 and +inf (`ref >= 0`) and drops negative values and NaN.  A few kept
  list entries are -1: numpy's negative indexing picks the last of the others.
* Wave classes: a wave of the tiled kernel is four consecutive bins x 16 samples; the 4-bin groups rotate through
  clean (ordinary references only), tail (one special bin among the kept positions from 8 (cnt // 8) on: dropped
  inside the kernel) and body (one special bin below 8 (cnt // 8): the whole wave goes to zscore_one).
* The `quiet` variant has no special bin and no -1: every wave stays inside the kernel at every kept count;
  `quiet22` is the same with the kept counts dealt so that every bin of chromosome 22 keeps at least eight references
  (its z-scores stay finite: a region the segmentation's walker takes).

The expectation is the oracle's alone: wo.to_numpy_ref_format, wo.apply_pca, wo.repeat_test.
"""
import collections
import functools

import numpy as np

from oracle import wc_oracle as wo

CUTOFF = 0.8
N_SAMPLES = 232
CALL_SIZES = (113, 128, 144, 232)        # padded to 128 with copies of sample 0; 8 tiles; 8 + 1 left over; 8 + 7 left over
K_SM = (100, 96, 64, 52, 12, 8, 4)       # k_zscore_tiled<12, 1, 25, true>: sample-major outputs
K_ODD = (99, 97, 10, 7, 1)               # k & 3: zscore_one with sample-major outputs
K_BM = (101, 103, 104, 128)              # k_zscore_tiled<12, 1, 26, false>: bin-major outputs and the transposes
K_LATE = (100, 40)                       # the later repeats
ALL_K = K_SM + K_ODD + K_BM
LAYOUT_OF = {k: i % 2 for i, k in enumerate(ALL_K + (40,))}     # both B % 4 layouts in every family
TAIL_CHROM = 22                          # `quiet22`: every bin of this chromosome keeps >= 8 references
TAIL_PAIR_CAP = 2048                     # csrc/testpath.hip: pairs a late repeat may hold for the one-workgroup form
# the samples the oracle computes: sample 0, the last real sample of every call size, one sample of every leftover
# tile of 144 (tile 8) and 232 (tiles 8 .. 14), and fillers from every full tile; at least 16 of them in every call
CHECK_POOL = (0, 5, 16, 21, 33, 38, 47, 54, 63, 70, 80, 87, 95, 99, 108, 112, 127, 130, 143, 150, 165, 180, 200, 215, 231)

Case = collections.namedtuple("Case", "k variant seed sizes sums B idx dst cnt mean comps counts special group planted")


def checked(n_samples):
    """The oracle's samples of a call of n_samples."""
    out = [s for s in CHECK_POOL if s < n_samples]
    assert len(out) >= 16 and out[0] == 0 and out[-1] == n_samples - 1
    return out


def chrom_sizes(k, which):
    """22 sizes: chromosome 3 one bin, the others 12 .. 25 bins; B % 4 == 3 (which 0) or 1 (which 1)."""
    B = (331 if k <= 100 else 471) + 2 * which
    q, r = divmod(B - 1, 21)
    rest = [q + (1 if i < r else 0) for i in range(21)]
    for a in range(0, 20, 2):                    # unequal neighbours
        rest[a] += 3
        rest[a + 1] -= 3
    sizes = np.array(rest[:2] + [1] + rest[2:], dtype=np.int64)
    assert int(sizes.sum()) == B and B % 4 == (1 if which else 3)
    assert B >= k + 1 and B - int(sizes.max()) >= k + 8
    return sizes


def _freeze(case):
    for v in case:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def case(k, variant, seed=0):
    """The reference and N_SAMPLES samples' counts of (k, variant, seed); read-only arrays."""
    assert variant in ("quiet", "special", "quiet22")
    special = variant == "special"
    rng = np.random.RandomState(9000 + 13 * k + 7 * seed + (1 if special else 0))
    sizes = chrom_sizes(k, LAYOUT_OF[k])
    sums = np.cumsum(sizes)
    B = int(sums[-1])
    starts = sums - sizes
    group = (np.arange(B) // 4) % 3              # of a wave's four bins: 0 clean, 1 tail, 2 body
    is_sp = np.zeros(B, dtype=bool)
    sp = np.zeros(0, dtype=np.int64)
    if special:
        # (never a bin that an index of -1 picks: B - 1, and for the last chromosome the bin in front of it)
        allowed = np.setdiff1d(np.arange(B), [B - 1, int(starts[-1]) - 1])
        while True:
            sp = np.sort(rng.choice(allowed, 6, replace=False))
            chroms = np.searchsorted(sums, sp, side="right")
            if len(set(chroms[0::3]) | set(chroms[1::3])) >= 2:      # every chromosome sees a dropped-value bin among its others
                break
        is_sp[sp] = True
    cnt = rng.permutation(np.arange(B) % (k + 1))
    if variant == "quiet22":
        lo, hi = int(starts[TAIL_CHROM - 1]), int(sums[TAIL_CHROM - 1])
        donors = [b for b in range(lo) if cnt[b] >= 8]
        for b in range(lo, hi):                  # swap: cnt stays a permutation of the same multiset
            if cnt[b] < 8:
                d = donors.pop(int(rng.randint(len(donors))))
                cnt[b], cnt[d] = cnt[d], cnt[b]
        assert np.all(cnt[lo:hi] >= 8)
    idx = np.empty((B, k), dtype=np.int32)
    planted = np.full(B, -1, dtype=np.int64)     # the list position of a bin's special reference
    for c in range(22):
        lo, hi = int(starts[c]), int(sums[c])
        others = np.concatenate([np.arange(0, lo), np.arange(hi, B)])
        ordinary = np.flatnonzero(~is_sp[others])            # positions in the "others" numbering
        specials = np.flatnonzero(is_sp[others])
        assert len(ordinary) >= k
        for b in range(lo, hi):
            idx[b] = rng.permutation(ordinary)[:k]
            n = int(cnt[b])
            body = 8 * (n // 8)
            if special and group[b] == 1 and n > body:
                planted[b] = rng.randint(body, n)
            elif special and group[b] == 2 and body > 0:
                planted[b] = rng.randint(0, body)
            if planted[b] >= 0:
                idx[b, planted[b]] = rng.choice(specials)
    if special:
        minus = [b for b in rng.permutation(B) if cnt[b] >= 2 or (cnt[b] == 1 and planted[b] < 0)][:8]
        for b in minus:
            at = int(rng.randint(cnt[b]))
            if at == planted[b]:
                at = (at + 1) % int(cnt[b])
            idx[b, at] = -1
    dst = np.sort(0.5 * rng.rand(B, k), axis=1)
    dst[np.arange(k)[None, :] >= cnt[:, None]] = 2.0
    mean = np.full(B, 1.0 / B) * (1 + 0.01 * rng.standard_normal(B))
    if special:
        mean[sp[0::3]] *= -1.0                   # negative (dropped); -0.0 (kept) where the count is 0
        mean[sp[1::3]] = 0.0                     # +inf (kept); NaN (dropped) where the count is 0
    lam = 3000.0 * (1 + 0.02 * rng.standard_normal((N_SAMPLES, B))).clip(0.5)
    counts = rng.poisson(lam).astype(np.int32)
    if special:
        sub = counts[:, sp]
        sub[rng.rand(N_SAMPLES, len(sp)) < 0.3] = 0
        counts[:, sp] = sub
    return _freeze(Case(k, variant, seed, sizes, sums, B, idx, dst, cnt, mean, np.zeros((0, B)), counts, sp, group,
                        planted))


def sample_dict(c, s):
    """Sample s as a converted sample: chromosome name -> int32 counts."""
    starts = c.sums - c.sizes
    return {str(ch + 1): c.counts[s, int(starts[ch]):int(c.sums[ch])] for ch in range(22)}


def reference_of(c):
    """The mapping wo.test_sample takes as a reference .npz."""
    return dict(binsize=np.float64(1e6), indexes=c.idx, distances=c.dst, chromosome_sizes=c.sizes,
                mask=np.ones(c.B, dtype=bool), masked_sizes=c.sizes, pca_mean=c.mean, pca_components=c.comps)


@functools.lru_cache(maxsize=None)
def data_row(k, variant, seed, s):
    """What the z-score stage sees of sample s: the oracle's toNumpyRefFormat and applyPCA."""
    c = case(k, variant, seed)
    x = wo.to_numpy_ref_format(sample_dict(c, s), [int(v) for v in c.sizes], np.ones(c.B, dtype=bool))
    with np.errstate(all="ignore"):
        x = wo.apply_pca(x, c.mean, c.comps)
    x.setflags(write=False)
    return x


def oracle_repeats(x, c, thr, repeats):
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
            out = wo.repeat_test(x, c.idx, c.dst, c.sizes, c.sums, CUTOFF, thr, repeats)
    finally:
        wo.try_sample = inner
    assert len(passes) == repeats
    return out, passes


@functools.lru_cache(maxsize=None)
def expect(k, variant, seed, s, thr, repeats):
    """THE EXPECTATION of sample s: ((z, r, n, sd) of wo.repeat_test, [the same of every repeat])."""
    c = case(k, variant, seed)
    (z, r, n, sd), passes = oracle_repeats(data_row(k, variant, seed, s), c, thr, repeats)
    for a in (z, r, n):
        a.setflags(write=False)
    return (z, r, n, sd), passes


def results_of(out, minrefbins):
    """(results_z, results_r, asdef) of toolTest from repeat_test's output: every bin is unmasked, so the inflated
    arrays are z and r - 1 where the bin keeps minrefbins references and 0.0 elsewhere (wisecondor.py:216-262)."""
    z, r, n, sd = out
    keep = n >= minrefbins
    with np.errstate(all="ignore"):
        return np.where(keep, z, 0.0), np.where(keep, r - 1.0, 0.0), sd


# ------------------------------------------------------------------------------------ what the cases hold ----
def global_refs(c, b):
    """The bin numbers of the references bin b keeps (an index of -1: the last of the others)."""
    ch = int(np.searchsorted(c.sums, b, side="right"))
    lo, size = int(c.sums[ch] - c.sizes[ch]), int(c.sizes[ch])
    p = c.idx[b, :int(c.cnt[b])].astype(np.int64)
    p = np.where(p < 0, p + (c.B - size), p)
    return np.where(p < lo, p, p + size)


def kept_values(c, rows, b):
    """[len(rows), cnt[b]]: the values of bin b's kept list positions in the data rows `rows` ([n, B])."""
    return rows[:, global_refs(c, b)]


def high_word(v):
    return (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def wave_classes(k, variant, seed, tile=0):
    """How many (4-bin group, tile) waves of one sample tile are clean / tail_only / body, judged the way
    k_zscore_tiled judges: a body value (list positions below 8 (cnt // 8)) whose high word is >= 0x7ff00000 sends
    the wave to zscore_one; a tail value with !(v >= 0) is dropped inside the kernel."""
    c = case(k, variant, seed)
    rows = np.stack([data_row(k, variant, seed, s) for s in range(16 * tile, 16 * tile + 16)])
    out = dict(clean=0, tail_only=0, body=0)
    for b0 in range(0, c.B, 4):
        body_bad = tail_bad = False
        for b in range(b0, min(b0 + 4, c.B)):
            v = kept_values(c, rows, b)
            nb = 8 * (int(c.cnt[b]) // 8)
            body_bad = body_bad or bool(np.any(high_word(v[:, :nb]) >= 0x7ff00000))
            tail_bad = tail_bad or bool(np.any(~(v[:, nb:] >= 0)))
        out["body" if body_bad else "tail_only" if tail_bad else "clean"] += 1
    return out


def value_classes(k, variant, seed, samples):
    """Which of negative / -0.0 / +inf / NaN / +0.0 occur among the kept-position references of `samples`."""
    c = case(k, variant, seed)
    rows = np.stack([data_row(k, variant, seed, s) for s in samples])
    used = np.zeros(c.B, dtype=bool)
    for b in range(c.B):
        used[global_refs(c, b)] = True
    v = rows[:, used]
    neg_zero = (v == 0) & np.signbit(v)
    return dict(negative=bool(np.any(v < 0)), neg_zero=bool(np.any(neg_zero)), pos_inf=bool(np.any(np.isposinf(v))),
                nan=bool(np.any(np.isnan(v))), pos_zero=bool(np.any((v == 0) & ~np.signbit(v))))


@functools.lru_cache(maxsize=None)
def users_matrix(k, variant, seed):
    """U[b, g]: bin b keeps bin g as a reference (k_count_users / k_fill_users: the reverse lists)."""
    c = case(k, variant, seed)
    U = np.zeros((c.B, c.B), dtype=np.int64)
    for b in range(c.B):
        U[b, global_refs(c, b)] = 1
    U.setflags(write=False)
    return U


def late_work(k, variant, seed, s, thr, repeats):
    """Per repeat 2 .. `repeats` of sample s, from the oracle's recorded repeats: (pairs whose z differs from the
    repeat before, pairs the repeat has queued -- the bins that keep a reference the repeat before flagged anew)."""
    _, passes = expect(k, variant, seed, s, thr, repeats)
    U = users_matrix(k, variant, seed)
    x = data_row(k, variant, seed, s)
    flagged = np.zeros(len(x), dtype=bool)
    changed, queued = [], []
    for it in range(1, repeats):
        z0, z1 = passes[it - 1][0], passes[it][0]
        with np.errstate(all="ignore"):
            new = (np.abs(z0) >= thr) & ~flagged & (x != -1.0)
        flagged |= new
        queued.append(int(np.count_nonzero(U @ new.astype(np.int64))))
        changed.append(int(np.count_nonzero(~((np.isnan(z0) & np.isnan(z1)) | (z0.view(np.int64) == z1.view(np.int64))))))
    return changed, queued


def call_weights(n_samples):
    """How often each real sample of a call of n_samples is computed: once, sample 0 also for every padding sample."""
    w = np.ones(n_samples, dtype=np.int64)
    w[0] += -n_samples % 16
    return w


# ------------------------------------------------------------------------------------ the later repeats ----
LATE_REPEATS = 5
LOW_THR = 2.5                # chromosomes=[]: thousands of pairs per late repeat, a launch pair each
# chromosomes=[22] on `quiet22`: repeats 3 and 4 have pairs queued, no repeat from the third on more than
# TAIL_PAIR_CAP (the oracle's counts over a call's samples: test_zscore_batch_cases_cpu.py).  The second repeat's
# flags are mostly the lists of two references that lost one to a list of one (sd 0, z infinite), whatever the
# threshold: how many pairs that queues varies between seeds by a factor of ten, hence the seed of k = 40.
TAIL_THR = {100: 4.0, 40: 5.0}
TAIL_SEED = {100: 0, 40: 2}
EDGE_CALLS = ((128, 0), (144, 130))      # (samples of the call, the sample whose z-score is the threshold)


def edge_case(k, variant, seed, s):
    """A threshold that IS abs(z) of a first-repeat z-score of sample s: the finite |z| nearest the 99th percentile
    among the bins that somebody keeps as a reference.  Returns (threshold, bin)."""
    (z, _, _, _), _ = expect(k, variant, seed, s, np.inf, 1)
    used = users_matrix(k, variant, seed).sum(axis=0) > 0
    cand = np.flatnonzero(np.isfinite(z) & used)
    a = np.abs(z[cand])
    b = int(cand[np.argsort(a)[int(0.99 * (len(a) - 1))]])
    return float(abs(z[b])), b
