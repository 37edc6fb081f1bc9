"""Inputs and the CPU reference of the call-row tests (a helper module, not a conftest; modelled on prep_cases.py).

A call's effect size is np.median(clean_r[x:y + 1]) - 1 (wisecondor.py:233-257).  The samples made here control
each call's length and each call's multiset of ratios through the real wt.test_batch:

* zero PCA components and a constant pca_mean: data = x / mean exactly, and the oracle's whole `test` is
  reproducible bit for bit;
* one shared reference list per chromosome, drawn from bins that never carry a planted span: every bin of a
  chromosome is divided by the same reference mean, so equal read counts give bit-equal ratios and the multiset
  of counts written into a span is the multiset the median sees;
* a Poisson(30) background with a fixed seed (|Stouffer| of every background window below the threshold; the CPU
  test holds that with the oracle on `short`), gain spans with counts of 100 and more (z of +13 and more);
* loss spans and spans of mixed sign through pca_mean < 0 on the span's bins (0 / negative gives -0.0).

Span coordinates and lengths are in KEPT bins: what is left after the mask and after the minrefbins filter, the
coordinates of the reference's segmentation.
"""
import collections
import functools

import numpy as np

from oracle import wc_oracle as wo

K = 32                       # reference list length
THR, MINREF, REPEATS = 5.0, 25, 2
BINSIZE = 1e6
BACKGROUND = 30.0
N1 = {"short": 150, "mid": 2048, "long": 5400}      # masked bins of chromosome 1 (the others: 40)
DROP_EVERY = {"short": 512, "mid": 512, "long": 131}  # chromosome 1: masked bin i is short of references where i % this == 57
POOL = list(range(11, 21))   # (0-based) chromosomes 12..21: reference bins, never planted
INF_CHROM, DEAD_CHROM = 8, 21  # chromosome 9 refers to the first K bins of chromosome 22 alone, nobody else does
# the shared list's counts: mean exactly BACKGROUND (no bias of the long chromosome's z), sd 5.52
POOL_COUNTS = np.array([30 + s * d for d in list(range(1, 9)) + list(range(2, 10)) for s in (1, -1)], dtype=np.int64)
SEED = {"short": 3, "mid": 3, "long": 3}


@functools.lru_cache(maxsize=None)
def layout(name):
    """Sizes, mask, masked sizes, idx, dst, pca_mean, zero-row components, binsize of a layout, the background
    counts and the maps kept bin -> genomic bin; read-only arrays."""
    n1 = N1[name]
    sizes, mask_parts = [], []
    for c in range(22):
        if c == 0:                                   # genomic bins p % 97 == 13 are masked out, n1 bins stay
            m = []
            while sum(m) < n1:
                m.append(len(m) % 97 != 13)
        else:
            m = [True] * 40
            if c == 1:
                m.insert(5, False)                   # a masked bin inside chromosome 2
            if c == 2:
                m.append(False)                      # ... and at the end of chromosome 3
        sizes.append(len(m))
        mask_parts.append(np.array(m, dtype=bool))
    sizes = np.array(sizes, dtype=np.int64)
    mask = np.concatenate(mask_parts)
    msizes = np.array([int(m.sum()) for m in mask_parts], dtype=np.int64)
    moff = np.concatenate([[0], np.cumsum(msizes)])
    B = int(moff[-1])
    rng = np.random.RandomState(SEED[name])
    pool_bins = np.concatenate([np.arange(moff[c], moff[c + 1]) for c in POOL])
    shared = np.sort(rng.choice(pool_bins, K, replace=False))
    dead = np.arange(moff[DEAD_CHROM], moff[DEAD_CHROM] + K)
    row_dst = np.sort(rng.uniform(0.5, 1.0, K))
    idx = np.empty((B, K), dtype=np.int32)
    dst = np.tile(row_dst, (B, 1))
    refs_of = []
    for c in range(22):
        lo, hi = int(moff[c]), int(moff[c + 1])
        if c == INF_CHROM:
            bins = dead
        elif c in POOL:
            bins = np.sort(rng.choice(pool_bins[(pool_bins < lo) | (pool_bins >= hi)], K, replace=False))
        else:
            bins = shared
        refs_of.append(bins)
        idx[lo:hi] = np.where(bins < lo, bins, bins - (hi - lo))      # the reference's "other chromosomes" numbering
    short_ref = np.zeros(B, dtype=bool)              # bins whose list tail lies beyond the cutoff: 20 references < MINREF
    short_ref[[i for i in range(n1) if i % DROP_EVERY[name] == 57]] = True
    short_ref[moff[1] + 20] = True
    dst[short_ref, 20:] = 1e3
    background = rng.poisson(BACKGROUND, B).astype(np.int64)
    background[shared] = POOL_COUNTS
    keep = ~short_ref
    masked_to_genomic = np.flatnonzero(mask)
    goff = np.concatenate([[0], np.cumsum(sizes)])
    kept_genomic = [masked_to_genomic[np.flatnonzero(keep[moff[c]:moff[c + 1]]) + moff[c]] for c in range(22)]
    out = dict(name=name, sizes=sizes, mask=mask, msizes=msizes, moff=moff, goff=goff, n_bins=B, idx=idx, dst=dst,
               pca_mean=np.full(B, 1.0 / B), pca_components=np.zeros((0, B)), binsize=BINSIZE, background=background,
               keep=keep, kept_genomic=kept_genomic, kept_sizes=[len(g) for g in kept_genomic], refs_of=refs_of,
               masked_to_genomic=masked_to_genomic)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def sample(lay, spans):
    """One sample: the background with each span's counts written over it.  A span is (chromosome (1-based), first
    kept bin, list of counts, per-bin signs of pca_mean or None).  Returns dict(counts=the sample dict '1'..'22',
    pca_mean=the reference's mean for this sample, planted=[(chrom, x, y)] in kept-bin coordinates, ascending)."""
    g2m = np.full(int(lay["sizes"].sum()), -1, dtype=np.int64)
    g2m[lay["masked_to_genomic"]] = np.arange(lay["n_bins"])
    counts = np.zeros(int(lay["sizes"].sum()), dtype=np.int64)
    counts[lay["masked_to_genomic"]] = lay["background"]
    counts[~lay["mask"]] = 7                         # masked-out bins hold reads too: they count in the total only
    mean = lay["pca_mean"].copy()
    planted = []
    for chrom, x, cnts, signs in spans:
        kept = lay["kept_genomic"][chrom - 1]
        assert 0 <= x and x + len(cnts) <= len(kept), (chrom, x, len(cnts), len(kept))
        where = kept[x:x + len(cnts)]
        counts[where] = cnts
        if signs is not None:
            mean[g2m[where]] *= np.asarray(signs, dtype=np.float64)
        planted.append((chrom, x, x + len(cnts) - 1))
    goff = lay["goff"]
    as_dict = {str(c + 1): counts[goff[c]:goff[c + 1]].astype(np.int32) for c in range(22)}
    return dict(counts=as_dict, pca_mean=mean, planted=sorted(planted))


def reference_of(lay, smp):
    """The mapping wo.test_sample takes as a reference .npz, with the sample's pca_mean."""
    return dict(binsize=np.float64(lay["binsize"]), indexes=lay["idx"], distances=lay["dst"], chromosome_sizes=lay["sizes"],
                mask=lay["mask"], masked_sizes=lay["msizes"], pca_mean=smp["pca_mean"],
                pca_components=lay["pca_components"])


def call_rows_want(lay, smp, thr, minrefbins, repeats, segments):
    """THE REFERENCE: rows [chrom, start, end, value, effect] of the given (chrom, x, y) segments (kept-bin
    coordinates), from the oracle's z-score stage, the keep filter and the survivor walk of wo.test_sample (restated,
    lines 482-513), value = the window's entry of fill_tri, effect = np.median(clean_r[lo + x:lo + y + 1]) - 1.
    Returns (rows, clean_r, clean_sums)."""
    sizes = [int(v) for v in lay["sizes"]]
    msizes = [int(v) for v in lay["msizes"]]
    msums = [sum(msizes[:i + 1]) for i in range(22)]
    data = wo.to_numpy_ref_format(smp["counts"], sizes, lay["mask"])
    data = wo.apply_pca(data, smp["pca_mean"], lay["pca_components"])
    cutoff, _ = wo.get_optimal_cutoff(lay["dst"], 3)
    z, r, ref_sizes, _ = wo.repeat_test(np.copy(data), lay["idx"], lay["dst"], msizes, msums, cutoff, thr, repeats)
    keep = ref_sizes >= minrefbins
    clean_r, clean_z = r[keep], z[keep]
    clean_sums = [int(np.sum(keep[:v])) for v in msums]
    survivors = wo.inflate_array_multi(np.ones(clean_r.shape, dtype=bool), [lay["mask"], keep])
    rows = []
    for chrom, x, y in segments:
        c = chrom - 1
        lo = clean_sums[c - 1] if c else 0
        assert lo + y < clean_sums[c], (chrom, x, y)
        base = sum(sizes[:c])
        pos, filled = base, 0
        while filled <= x:
            filled += survivors[pos] != 0
            pos += 1
        pos -= 1
        end = pos
        while filled <= y:
            filled += survivors[end] != 0
            end += 1
        with np.errstate(all="ignore"):
            value = np.sum(clean_z[lo + x:lo + y + 1]) / np.sqrt(y - x + 1)
            effect = np.median(clean_r[lo + x:lo + y + 1]) - 1
        rows.append([chrom, pos - base, end - base, value, effect])
    return np.array(rows, dtype=np.float64).reshape(-1, 5), clean_r, clean_sums


# ------------------------------------------------------------------------------- classes of a multiset ----
MedianClass = collections.namedtuple("MedianClass", "name neg zero_pm inf run distinct")


def ordered_keys(values):
    """The total order a radix selection sees: the 64-bit image with negative values reversed (-0.0 below +0.0)."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))


def median_class(values):
    """name: odd / even_distinct (middle pair differs, lower value unique) / even_tie (middle pair bit-equal) /
    even_run_ends_at_k (lower middle value repeated, its run ends at rank k, the upper one is the next distinct value)
    / has_nan; flags neg (a value below zero), zero_pm (+0.0 and -0.0), inf; run: how often the lower middle value
    occurs; distinct: no value occurs twice."""
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    n = len(v)
    assert n >= 1
    bits = v.view(np.uint64)
    flags = dict(neg=bool(np.any(v < 0)),
                 zero_pm=bool(np.any(bits == np.uint64(0)) and np.any(bits == np.uint64(1 << 63))),
                 inf=bool(np.any(np.isinf(v))))
    if np.any(np.isnan(v)):
        return MedianClass("has_nan", run=0, distinct=False, **flags)
    keys = np.sort(ordered_keys(v))
    k = (n - 1) // 2
    run = int(np.sum(keys == keys[k]))
    distinct = len(np.unique(keys)) == n
    if n & 1:
        name = "odd"
    elif keys[k] == keys[k + 1]:
        name = "even_tie"
    else:
        name = "even_distinct" if run == 1 else "even_run_ends_at_k"
    return MedianClass(name, run=run, distinct=distinct, **flags)


def kind_of(cls, length):
    """What the coverage table asks for at every length: `tied` (even_tie or even_run_ends_at_k; odd lengths: the
    median value at least three times) and `distinct` (all values differ)."""
    if cls.distinct:
        return "distinct"
    if cls.name in ("even_tie", "even_run_ends_at_k") or (cls.name == "odd" and cls.run >= 3):
        return "tied"
    return "other"


# --------------------------------------------------------------------------------- the spans' counts ----
def arrange(counts, signs=None):
    """The strongest bins (largest |z|) at the edges, weaker ones towards the middle: every prefix and suffix of the
    span is then stronger than the span's mean, so the best Stouffer window is the whole span."""
    counts = np.asarray(counts, dtype=np.int64)
    sg = np.ones(len(counts), dtype=np.int64) if signs is None else np.asarray(signs, dtype=np.int64)
    strength = np.where(sg < 0, counts + BACKGROUND, np.abs(counts - BACKGROUND))
    order = np.argsort(-strength, kind="stable")
    at = np.empty(len(counts), dtype=np.int64)
    at[0::2] = np.arange((len(counts) + 1) // 2)
    at[1::2] = len(counts) - 1 - np.arange(len(counts) // 2)
    out_c, out_s = np.empty_like(counts), np.empty_like(sg)
    out_c[at] = counts[order]
    out_s[at] = sg[order]
    return [int(v) for v in out_c], (None if signs is None else [int(v) for v in out_s])


def distinct(n):
    """n different counts: 100 .. 170 where that many exist, else n .. 2 n - 1."""
    base = 100 if n <= 71 else n
    return arrange(base + np.arange(n))


def _three_levels(n, first_mid, n_mid):
    low = [105 + i % 15 for i in range(first_mid)]
    high = [141 + i % 29 for i in range(n - first_mid - n_mid)]
    return arrange(low + [130] * n_mid + high)


def tied(n):
    """The median value (130) three times (more in long spans) around the middle ranks: even_tie, or an odd span
    whose median is repeated."""
    if n <= 3:
        return [130] * n, None
    n_mid = 3 + 2 * (n // 16)
    return _three_levels(n, (n - n_mid) // 2, n_mid)


def run_ends(n):
    """Even n >= 4: the run of 130 ends exactly at the lower middle rank, the upper middle value is the next one."""
    assert n % 2 == 0 and n >= 4
    k = n // 2 - 1
    n_run = min(3 + n // 16, k + 1)
    return _three_levels(n, k + 1 - n_run, n_run)


def equal(n):
    return [130] * n, None


def loss(n):
    """All ratios negative and different: the counts of distinct(n) under a negative pca_mean."""
    return arrange(distinct(n)[0], [-1] * n)


def mixed(n):
    """Negative ratios (counts 1 .. 40 under a negative pca_mean), -0.0, +0.0 and small positive ones: every |z| is
    between 4.5 and 13, so no bin is weaker than half the span's mean.  Even n: the run of -0.0 ends at the lower middle rank and +0.0 follows (even_run_ends_at_k
    across the two zeros); odd n: the median is a -0.0 that occurs twice."""
    if n == 2:
        return [0, 0], [-1, 1]
    assert n >= 5
    k = (n - 1) // 2
    if n % 2 == 0:
        n_mz = min(3, k)
        n_neg = k + 1 - n_mz
    else:
        n_mz, n_neg = 2, k - 1
    n_pos = n - n_neg - n_mz - 1
    counts = [1 + i % 40 for i in range(n_neg)] + [0] * n_mz + [0] + [1 + i % 5 for i in range(n_pos)]
    signs = [-1] * (n_neg + n_mz) + [1] * (1 + n_pos)
    return arrange(counts, signs)


MAKERS = dict(distinct=distinct, tied=tied, run_ends=run_ends, equal=equal, loss=loss, mixed=mixed)


def span(chrom, x, maker, n):
    counts, signs = MAKERS[maker](n)
    return (chrom, x, counts, signs)


# ------------------------------------------------------------------------------------------ the cases ----
# a case: (name, layout, spans as (chrom, first kept bin, maker, length), chromosomes whose calls are not planted
# finite spans).  Chromosome 1 carries the main span, chromosomes 2..8 two or three short ones (regions with 0, 1 and
# several calls); chromosome 3's span is sometimes the whole region.
def _small(i):
    """Two or three short spans on chromosomes 2..8, rotating through lengths 1, 2, 3, 5 and the plain makers."""
    sets = [[(2, 10, "distinct", 1), (4, 20, "tied", 2), (5, 4, "distinct", 3)],
            [(2, 30, "distinct", 2), (6, 0, "tied", 3), (7, 35, "distinct", 5)],
            [(3, 0, "tied", 40), (8, 17, "distinct", 1)],
            [(4, 8, "tied", 5), (5, 39, "distinct", 1), (6, 21, "equal", 2)],
            [(3, 0, "distinct", 40), (7, 12, "equal", 5), (2, 18, "tied", 3)]]
    return sets[i % len(sets)]


def _cases():
    cases = []

    def add(name, lay, spans, nonfinite=(), repeats=REPEATS):
        cases.append(dict(name=name, layout=lay, spans=list(spans), nonfinite=tuple(nonfinite), repeats=repeats))

    n = 0
    # short: every value class at lengths 2, 5, 64, 65 and 130, the plain classes also at 1, 3 and 63
    for length in (63, 64, 65, 130):
        for maker in ("tied", "distinct", "run_ends", "equal", "loss", "mixed"):
            if maker == "run_ends" and length % 2:
                continue
            add("short-%s-%d" % (maker, length), "short", [(1, 13 if length < 130 else 9, maker, length)] + _small(n))
            n += 1
    add("short-signed-small", "short", [(1, 40, "loss", 2), (1, 100, "loss", 5), (4, 10, "mixed", 5), (6, 20, "mixed", 2)])
    # (chromosome 2: a masked-out bin between the first span's two bins -- its end is the position of survivor y - 1,
    #  plus one -- and the second span starts right behind the bin that is short of references)
    add("short-plain-small", "short", [(1, 30, "run_ends", 4), (1, 108, "equal", 5), (5, 10, "run_ends", 6),
                                       (2, 4, "distinct", 2), (2, 20, "tied", 2)])
    # three calls in chromosome 1 whose list order (strongest first) differs from position order; two on chromosome 2
    add("short-order", "short", [(1, 8, "distinct", 5), (1, 40, "tied", 2), (1, 100, "distinct", 30),
                                 (2, 4, "tied", 3), (2, 25, "distinct", 5)])
    # chromosome 9's reference bins (the first K bins of chromosome 22) empty: ratio +inf, effect +inf; and with empty
    # test bins as well: 0 / 0, effect NaN.  (The emptied bins of chromosome 22 are a finite span of equal ratios +0.0.)
    # One repeat: a second one flags the emptied bins (z = -5.4) and leaves chromosome 9 without references.
    add("short-inf", "short", [(22, 0, "zeros", K), (2, 10, "tied", 5)], nonfinite=[9], repeats=1)
    add("short-nan", "short", [(22, 0, "zeros", K), (9, 7, "zeros", 3), (9, 30, "zeros", 1), (4, 10, "distinct", 2)],
        nonfinite=[9], repeats=1)
    # mid: chromosome 1 has 2 048 masked bins (latency mode's limit), 2 044 kept
    for length in (1023, 1024, 1025, 1026, 2040):
        for maker in ("tied" if length % 2 else ("run_ends" if length % 4 == 0 else "tied"), "distinct"):
            add("mid-%s-%d" % (maker, length), "mid", [(1, 2 if length == 2040 else 500, maker, length)] + _small(n))
            n += 1
    # long: chromosome 1 has 5 400 masked bins, 5 358 kept; the staging limit of k_walk_rows is 5 120
    for length in (2048, 2049, 4096, 4097, 5119, 5120, 5121, 5122):
        for maker in ("tied" if length % 2 else ("run_ends" if length % 4 == 0 else "tied"), "distinct"):
            add("long-%s-%d" % (maker, length), "long", [(1, 100, maker, length)] + _small(n))
            n += 1
    for maker in ("tied", "distinct"):
        add("long-%s-several" % maker, "long", [(1, 100, maker, 257), (1, 1200, maker, 256), (1, 2300, maker, 255),
                                                (1, 3400, "run_ends" if maker == "tied" else maker, 66),
                                                (1, 3800, maker, 65)] + _small(n))
        n += 1
    for maker in ("equal", "loss", "mixed"):
        for length in (300, 5130):
            add("long-%s-%d" % (maker, length), "long", [(1, 100, maker, length)] + _small(n))
            n += 1
    return cases


MAKERS["zeros"] = lambda n: ([0] * n, None)
CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]

# lengths (in kept bins) that must be seen on each route, each as `tied` and as `distinct` (length 1: one class)
REQUIRED = {
    "latency": [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2040],
    "walker": [1, 2, 63, 64, 65, 66, 255, 256, 257, 2048, 2049, 5119, 5120, 5121, 5122],
    "host": [1, 2, 64, 65, 1023, 1024, 1025, 1026, 4096, 4097, 5121],
}


def required(route):
    return {(n, kind) for n in REQUIRED[route] for kind in (("distinct",) if n == 1 else ("tied", "distinct"))}


@functools.lru_cache(maxsize=None)
def case_sample(name):
    case = CASES[CASE_NAMES.index(name)]
    lay = layout(case["layout"])
    smp = sample(lay, [span(*s) for s in case["spans"]])
    smp["finite"] = [p for p in smp["planted"] if p[0] not in case["nonfinite"]]
    return smp


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """wo.test_sample of a `short` case, computed once."""
    case = CASES[CASE_NAMES.index(name)]
    assert case["layout"] == "short"
    lay, smp = layout("short"), case_sample(name)
    with np.errstate(all="ignore"):
        return wo.test_sample(smp["counts"], BINSIZE, reference_of(lay, smp), minzscore=THR, minrefbins=MINREF,
                              repeats=case["repeats"])


@functools.lru_cache(maxsize=None)
def want_of(name):
    """(rows [chrom, start, end, value, effect] of the case's finite planted spans, clean ratios, their chromosome ends)."""
    case = CASES[CASE_NAMES.index(name)]
    lay, smp = layout(case["layout"]), case_sample(name)
    with np.errstate(all="ignore"):
        return call_rows_want(lay, smp, THR, MINREF, case["repeats"], smp["finite"])


def span_class(name, segment):
    """median_class of the ratios of one (chrom, x, y) segment of a case."""
    _, clean_r, clean_sums = want_of(name)
    chrom, x, y = segment
    lo = clean_sums[chrom - 2] if chrom > 1 else 0
    return median_class(clean_r[lo + x:lo + y + 1])
