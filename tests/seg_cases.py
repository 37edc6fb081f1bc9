"""Inputs, the CPU reference and a model of the give-up rules for the segmentation-limit tests (a helper module, not a
conftest; modelled on call_cases.py).

The two fixed-capacity walkers of csrc/testpath.hip -- k_seg_walk (every batch) and k_seg_tree (calls of up to eight
samples) -- hand a call back to the host-driven rounds when a region does not fit: more than CJ_REC = CAND_CAP = 64
windows tied for an extreme, more than TREE_SEGS = 128 segments, a job stack beyond WALK_STACK = TREE_STACK = 64, a
non-finite z.  The samples made here put a region exactly AT each of these capacities and exactly ONE PAST it, through the
real wt.test_batch, with call_cases' construction: zero PCA components, a constant pca_mean and one shared reference list
for every planted chromosome, so that z is an affine function of the read count and equal counts give bit-equal z.

What differs from call_cases: the background count is LEVEL = 3 000 and not 30, the reference list's counts are
LEVEL +- 1..9 (sd 5.52, mean exactly LEVEL), so a count c gives z = (c - LEVEL) / 5.52 on BOTH sides of zero, down to
-543.  (call_cases plants negative z through a negative pca_mean; a batch shares ONE pca_mean, and a bin with a
negative mean is loud -- z <= -5.4 -- in every sample of it, so the quiet samples that fill these batches and follow the
give-ups could not ride along.)  A profile is an integer array L, one entry per kept bin of a region: count = LEVEL + L.
Bins outside a profile keep the background LEVEL + uniform{-4 .. 4}, |z| <= 0.73 (the reference bins themselves
LEVEL +- 9): every window of it stays more than 1 below the threshold.

The expected outputs of every case are wo.test_sample of it (oracle_of, cached; the triangles it filled are kept for
the model and for the `direct` route).  walk_model restates the walkers' recursion over such a triangle and gives the
status bits the kernels must raise; test_seg_cases_cpu.py holds every case to its design with both.

Out of scope: status 1 (a region beyond CJ_MAXLEN = 8 192 bins: the triangle is out of reach there, test_fullsize_gpu.py
covers the lengths) and status 32 (a cell queue overflow: no small input is known that causes one).

Layouts: `seg` (chromosome 1: 520 kept bins, chromosome 2: 332, the others 40) for the limit cases; `hot` (150 / 40 /
40 ... and chromosome 11 with 2 100 masked bins of which 40 are kept) for k_seg_walk's early-starter list, which only
exists where a region has more than TREE_MAXLEN = 2 048 masked bins (seg_setup: `walk_path && !fused`, fused =
max_n <= TREE_MAXLEN): chromosome 11's other 2 060 bins refer to a list of which eight bins are loud in every sample, the
first repeat flags those, the last one finds 24 < MINREF references and the bins are dropped -- the oracle's triangle
of that region stays at 40 bins.
"""
import functools

import numpy as np

import call_cases as cc
from oracle import wc_oracle as wo

K, THR, MINREF, REPEATS, BINSIZE = cc.K, cc.THR, cc.MINREF, cc.REPEATS, cc.BINSIZE
MIN_SEARCH = 3
LEVEL = 3000
NOISE = 4                                        # background: LEVEL + uniform{-NOISE .. NOISE}
POOL = cc.POOL                                   # (0-based) chromosomes 12..21: reference bins, never planted
POOL_COUNTS = cc.POOL_COUNTS - 30 + LEVEL
BULK = 10                                        # `hot`: (0-based) chromosome 11 is the one beyond TREE_MAXLEN masked bins
LOUD_CHROM, N_LOUD, LOUD_BY = 20, 8, 100         # `hot`: eight bins of chromosome 21 hold LEVEL + 100 in every sample
SHAPES = {"seg": dict(n1=521, n2=333, bulk=0, seed=11), "hot": dict(n1=150, n2=40, bulk=2100, seed=12)}
BULK_KEPT = 40

# the capacities, as csrc/testpath.hip names them
CJ_REC = CAND_CAP = 64
TREE_SEGS = 128
WALK_STACK = TREE_STACK = 64
TREE_MAXLEN = 2048
HOT_CAP_SMALL, HOT_CAP_BIG, HOT_BIG_FROM = 512, 4096, 4096      # seg_setup: whot.cap
HOT_CUT = 0.75                                   # ... whot.cut = 0.75 * thr


@functools.lru_cache(maxsize=None)
def layout(name):
    """The dict call_cases.layout gives (cc.sample and cc.reference_of take it), for the shapes of this module."""
    shape = SHAPES[name]
    n1, n2, bulk = shape["n1"], shape["n2"], shape["bulk"]
    sizes, mask_parts = [], []
    for c in range(22):
        if c == 0:                                   # genomic bins p % 97 == 13 are masked out, n1 bins stay
            m = []
            while sum(m) < n1:
                m.append(len(m) % 97 != 13)
        else:
            m = [True] * (n2 if c == 1 else bulk if (c == BULK and bulk) else 40)
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
    rng = np.random.RandomState(shape["seed"])
    loud = np.arange(moff[LOUD_CHROM] + 4, moff[LOUD_CHROM] + 4 + N_LOUD) if bulk else np.zeros(0, dtype=np.int64)
    pool_bins = np.setdiff1d(np.concatenate([np.arange(moff[c], moff[c + 1]) for c in POOL]), loud)
    shared = np.sort(rng.choice(pool_bins, K, replace=False))
    row_dst = np.sort(rng.uniform(0.5, 1.0, K))
    idx = np.empty((B, K), dtype=np.int32)
    dst = np.tile(row_dst, (B, 1))
    refs_of = []
    for c in range(22):
        lo, hi = int(moff[c]), int(moff[c + 1])
        if c in POOL:
            bins = np.sort(rng.choice(pool_bins[(pool_bins < lo) | (pool_bins >= hi)], K, replace=False))
        else:
            bins = shared
        refs_of.append(bins)
        idx[lo:hi] = np.where(bins < lo, bins, bins - (hi - lo))      # the reference's "other chromosomes" numbering
    short_ref = np.zeros(B, dtype=bool)              # bins whose list tail lies beyond the cutoff: 20 references < MINREF
    short_ref[[i for i in range(n1) if i % 512 == 57]] = True
    short_ref[moff[1] + 20] = True
    dst[short_ref, 20:] = 1e3
    flagged_out = np.zeros(B, dtype=bool)            # `hot`: bins that lose N_LOUD of their K references to the first repeat
    if bulk:
        lo, hi = int(moff[BULK]), int(moff[BULK + 1])
        flagged_out[lo:hi] = True
        flagged_out[lo + np.arange(BULK_KEPT) * (bulk // BULK_KEPT) + 7] = False
        others = np.setdiff1d(pool_bins, shared)
        bulk_refs = np.sort(np.concatenate([loud, rng.choice(others, K - N_LOUD, replace=False)]))
        idx[flagged_out] = np.where(bulk_refs < lo, bulk_refs, bulk_refs - (hi - lo))
    background = LEVEL + rng.randint(-NOISE, NOISE + 1, B).astype(np.int64)
    background[shared] = POOL_COUNTS
    background[loud] = LEVEL + LOUD_BY
    keep = ~(short_ref | flagged_out)
    masked_to_genomic = np.flatnonzero(mask)
    goff = np.concatenate([[0], np.cumsum(sizes)])
    kept_genomic = [masked_to_genomic[np.flatnonzero(keep[moff[c]:moff[c + 1]]) + moff[c]] for c in range(22)]
    out = dict(name=name, sizes=sizes, mask=mask, msizes=msizes, moff=moff, goff=goff, n_bins=B, idx=idx, dst=dst,
               pca_mean=np.full(B, 1.0 / B), pca_components=np.zeros((0, B)), binsize=BINSIZE, background=background,
               keep=keep, kept_genomic=kept_genomic, kept_sizes=[len(g) for g in kept_genomic], refs_of=refs_of,
               masked_to_genomic=masked_to_genomic, loud=loud)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ the profiles ----
MAG = 2000        # spikes of near-equal magnitude MAG + rank: no window over several spikes beats the strongest one alone
TIE, FILL = 44, -11                              # z = +8 and four bins of z = -2: every group of five sums to zero


def bit_reversed(i, bits=8):
    return int(format(i, "0%db" % bits)[::-1], 2)


def ladder(n, length, gap=5, right_aligned=False):
    """n single-bin spikes of alternating sign and strictly increasing magnitude, `gap` bins apart.  From bin 0 with
    gap 5 (s q q q q) every job's champion is its rightmost spike and the four bins behind it are a right child that
    stays pending while the left child is walked: the stack grows by one per level.  Right-aligned with gap 4 (s q q q
    up to the region's end) no right child is ever pushed."""
    L = np.zeros(length, dtype=np.int64)
    at = length - gap * n if right_aligned else 0
    assert at >= 0
    for i in range(n):
        L[at + i * gap] = (1 if i % 2 == 0 else -1) * (MAG + i)
    return L


def balanced(n, length, gap=4):
    """n alternating-sign spikes four bins apart (s q q q) whose magnitudes run in bit-reversed order: every spike is a
    segment of its own and the recursion stays about log2(n) deep."""
    L = np.zeros(length, dtype=np.int64)
    assert gap * n <= length and n <= 256
    for i in range(n):
        L[i * gap] = (1 if i % 2 == 0 else -1) * (MAG + bit_reversed(i))
    return L


def ties(k, length, sign=1, other=0):
    """k spikes of ONE count five bins apart on a filler that cancels them: the k single-bin windows tie exactly for
    the maximum (sign = -1: the minimum).  other: one stronger spike of the opposite sign behind them."""
    L = np.zeros(length, dtype=np.int64)
    assert 5 * k + (4 if other else 0) <= length
    for i in range(k):
        L[5 * i] = sign * TIE
        L[5 * i + 1:5 * i + 5] = sign * FILL
    if other:
        L[5 * k + 3] = -sign * other
    return L


def spikes_of(L):
    """The bins a profile makes calls of: the single-bin spikes (|L| of a filler stays below the threshold)."""
    return [int(i) for i in np.flatnonzero(np.abs(L) >= TIE)]


def span_levels(n, sign=1):
    """A plain aberration of n bins (call_cases.distinct: stronger towards the edges, the whole span is the call)."""
    return sign * (np.array(cc.distinct(n)[0], dtype=np.int64) - int(cc.BACKGROUND))


# ------------------------------------------------------------------------------------------ the cases ----
# a case: name, layout, profiles {chromosome (1-based): L over the whole region}, spans [(chromosome, first kept bin,
# levels)], repeats, and what it is for: (limit, side) with limit in ties_hi / ties_lo / segments / stack / nonfinite /
# mixed / none and side in at / beyond / below.
def _cases():
    n1, n2 = SHAPES["seg"]["n1"] - 1, SHAPES["seg"]["n2"] - 1          # kept bins of chromosomes 1 and 2
    cases = []

    def add(name, limit, side, profiles=None, spans=(), lay="seg", repeats=REPEATS, wraps=None):
        cases.append(dict(name=name, layout=lay, profiles=profiles or {}, spans=list(spans), repeats=repeats,
                          limit=limit, side=side, wraps=wraps))

    # stack: level k of the ladder tests (k - 1) pending right children + 2 pushes, the last level (the spike at bin 0
    # has no left child) (N - 1) + 1: the largest test value is N for N <= 64, and level 64 of N >= 65 tests 63 + 2
    add("ladder-64", "stack", "at", {2: ladder(64, n2)})
    add("ladder-65", "stack", "beyond", {2: ladder(65, n2)})
    add("ladder-66", "stack", "beyond", {2: ladder(66, n2)})
    # (the control fills its region: a run of quiet bins next to a lone positive spike is thousands of windows tied at
    #  exactly 0.0 for the minimum, which k_seg_tree -- it records both sides -- does not hold)
    assert n2 % 4 == 0
    add("ladder-83-no-right", "stack", "below", {2: ladder(n2 // 4, n2, gap=4, right_aligned=True)})
    add("balanced-128", "segments", "at", {1: balanced(128, n1)})
    add("balanced-129", "segments", "beyond", {1: balanced(129, n1)})
    add("ties-64", "ties_hi", "at", {2: ties(64, n2)})
    add("ties-65", "ties_hi", "beyond", {2: ties(65, n2)})
    add("ties-64-min", "ties_lo", "at", {2: ties(64, n2, sign=-1)})
    add("ties-65-min", "ties_lo", "beyond", {2: ties(65, n2, sign=-1)})
    add("ties-65-champion-below", "ties_hi", "beyond", {2: ties(65, n2, other=100)})     # the champion is the minimum
    add("mixed", "mixed", "beyond", {1: ladder(66, n1), 2: ties(65, n2)})
    add("quiet", "none", "below")
    add("one-span", "none", "below", spans=[(1, 100, span_levels(20)), (2, 40, span_levels(6, -1)), (5, 10, span_levels(3))])
    # non-finite z: call_cases' sample whose chromosome 9 has empty reference bins, and two finite samples of its layout
    add("short-inf", "nonfinite", "beyond", lay="short", repeats=1, wraps="short-inf")
    add("short-order", "none", "below", lay="short", repeats=1, wraps="short-order")
    add("short-plain-small", "none", "below", lay="short", repeats=1, wraps="short-plain-small")
    # `hot`: spans on 12, 12, 11, 10, 9 and 8 of the 13 plantable chromosomes (1..11 and 22; chromosome 21 is loud in
    # every sample), ten bins on chromosome 1 and five elsewhere
    plantable = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 22]
    for i, leave_out in enumerate([(), (), (3,), (1, 22), (2, 6, 11), (4, 5, 9, 10)]):
        spans = [(c, (17 + 3 * i) % 30, span_levels(10 if c == 1 else 5, -1 if (c + i) % 3 == 0 else 1))
                 for c in plantable if c not in leave_out]
        add("hot-%d" % i, "none", "below", spans=spans, lay="hot")
    return cases


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]
FILLERS = {"seg": ["quiet", "one-span"], "short": ["short-order", "short-plain-small"]}
HOT = [n for n in CASE_NAMES if n.startswith("hot-")]


def case_of(name):
    return CASES[CASE_NAMES.index(name)]


def layout_of(name):
    lay = case_of(name)["layout"]
    return cc.layout(lay) if lay == "short" else layout(lay)


@functools.lru_cache(maxsize=None)
def case_sample(name):
    """dict(counts, pca_mean, planted) as call_cases.sample gives it; spikes: [(chromosome, kept bin)] of the profiles."""
    case = case_of(name)
    if case["wraps"]:
        smp = dict(cc.case_sample(case["wraps"]))
        smp["spikes"] = []
        return smp
    lay = layout_of(name)
    spans = []
    for chrom, L in sorted(case["profiles"].items()):
        assert len(L) == lay["kept_sizes"][chrom - 1], (name, chrom, len(L), lay["kept_sizes"][chrom - 1])
        assert L.min() >= -LEVEL
        spans.append((chrom, 0, [int(v) for v in LEVEL + L], None))
    for chrom, x, levels in case["spans"]:
        spans.append((chrom, x, [int(v) for v in LEVEL + levels], None))
    smp = cc.sample(lay, spans)
    assert np.all(smp["pca_mean"] == lay["pca_mean"])                  # one reference for every sample of a layout
    smp["spikes"] = [(chrom, i) for chrom, L in sorted(case["profiles"].items()) for i in spikes_of(L)]
    smp["spans"] = sorted((chrom, x, x + len(levels) - 1) for chrom, x, levels in case["spans"])
    return smp


def oracle_of_sample(lay, smp, repeats=REPEATS, thr=THR):
    """wo.test_sample of one sample of a layout; `tris`: the triangle of every chromosome as test_sample filled it,
    `regions`: the cleaned z of every chromosome (what the triangles were filled from)."""
    tris, regions = [], []
    fill = wo.fill_tri

    def keeping(region):
        regions.append(np.array(region))
        tris.append(fill(region))
        return tris[-1]

    wo.fill_tri = keeping
    try:
        with np.errstate(all="ignore"):
            out = wo.test_sample(smp["counts"], BINSIZE, cc.reference_of(lay, smp), minzscore=thr, minrefbins=MINREF,
                                 repeats=repeats)
    finally:
        wo.fill_tri = fill
    assert len(tris) == 22
    out["tris"], out["regions"] = tris, regions
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """oracle_of_sample of a case, computed once."""
    return oracle_of_sample(layout_of(name), case_sample(name), case_of(name)["repeats"])


def rows_of(out):
    return np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)


# ---------------------------------------------------------------------------- the walkers' rules, restated ----
def walk_model(tri, edge, thr=THR, min_search=MIN_SEARCH, tie_rule="walk"):
    """The recursion of k_seg_walk (testpath.hip, its `while (true)` loop) over the oracle's triangle of one region:
    pop a job; its extremes (np.argmax / np.argmin: the first of equal windows, as the reference); a quiet job ends;
    more than CJ_REC windows bit-equal to an extreme -> 4; the champion is a segment, the 129th -> 8; stack occupancy
    after the pop + the children to push beyond WALK_STACK -> 16, else push right, then left (left is walked first).
    Any status stops the region's walk (s_stop), 8 and 16 can be raised by the same job.

    tie_rule "walk": a side counts only if it can hold a call (k_seg_walk: hi_cut / lo_cut are infinite for a side
    whose extreme stays below the threshold); "tree": both sides of every job that is not quiet (k_seg_tree: hi_cut =
    emax - 2 eps and lo_cut = emin + 2 eps whatever their size; any status there is counters[6] = 1).

    Returns dict(status, segments, stack: the largest occupancy + pushes tested, ties_hi, ties_lo: the most windows
    bit-equal to a job's extreme per side (sides that count), near: the most windows within 1e-6 relative of a job's
    extreme that are NOT bit-equal to it, depth: the most jobs pending)."""
    res = dict(status=0, segments=0, stack=0, ties_hi=0, ties_lo=0, near=0, depth=0)
    if not np.all(np.isfinite(tri)):
        res["status"] = 2                            # (reg_flag: a non-finite z anywhere in the region)
        return res
    stack = [(0, edge)]
    while stack and not res["status"]:
        lo, hi = stack.pop()
        if hi - lo <= 0:
            continue
        sub, n = wo._sub_triangle(tri, edge, lo, hi)
        vmax, vmin = sub.max(), sub.min()
        if max(abs(vmax), abs(vmin)) < thr:
            continue
        for side, v in (("ties_hi", vmax), ("ties_lo", vmin)):
            if tie_rule == "tree" or abs(v) >= thr:
                tied = int(np.sum(sub == v))
                res[side] = max(res[side], tied)
                res["near"] = max(res["near"], int(np.sum(np.abs(sub - v) <= 1e-6 * abs(v))) - tied)
        if max(res["ties_hi"], res["ties_lo"]) > CJ_REC:
            res["status"] |= 4
            continue
        pos, champ = int(sub.argmax()), vmax
        if abs(vmin) > champ:
            pos, champ = int(sub.argmin()), vmin
        assert abs(champ) >= thr
        x, y = wo.lin_to_2d(n, pos)
        res["segments"] += 1
        if res["segments"] > TREE_SEGS:
            res["status"] |= 8
        left, right = x > min_search, y + 1 < n - min_search
        res["stack"] = max(res["stack"], len(stack) + left + right)
        if len(stack) + left + right > WALK_STACK:
            res["status"] |= 16
        else:
            if right:
                stack.append((lo + y + 1, hi))
            if left:
                stack.append((lo, lo + x))
            res["depth"] = max(res["depth"], len(stack))
    return res


@functools.lru_cache(maxsize=None)
def models_of(name, tie_rule="walk"):
    """walk_model of every chromosome of a case."""
    want = oracle_of(name)
    return [walk_model(tri, len(z), tie_rule=tie_rule) for tri, z in zip(want["tris"], want["regions"])]


def expected_status(name, kernel="walk"):
    """The status word k_seg_walk must leave for a call that holds this case (the OR over its regions: bits 2 / 4 / 8 /
    16), or with kernel="tree" whether k_seg_tree must hand the call back (0 or 1)."""
    status = 0
    for m in models_of(name, kernel):
        status |= m["status"]
    return status if kernel == "walk" else int(status != 0)


# what must be seen on a route: (limit, side of the limit).  The walkers have all three capacities; on the host-driven
# rounds only the tie record exists (k_seg_decide sends a job with more than CAND_CAP candidates to k_seg_brute, the
# CJ_GREC second pass), the other cases run there all the same.
_WALKER = {(limit, side) for limit in ("ties_hi", "ties_lo", "segments", "stack") for side in ("at", "beyond")} | \
          {("nonfinite", "beyond"), ("mixed", "beyond"), ("stack", "below")}
_HOST = {(limit, side) for limit in ("ties_hi", "ties_lo") for side in ("at", "beyond")} | {("nonfinite", "beyond")}
REQUIRED = {"latency": _WALKER, "latency_eager": _WALKER, "latency_off": _WALKER, "walker": _WALKER,
            "walker_no_hot": _WALKER, "host": _HOST, "host_one_part": _HOST, "host_row_blocks": _HOST, "direct": _HOST}


# ------------------------------------------------------------------------------------ the early-starter list ----
def hot_regions(name, margin=2.0):
    """k_region_prefix's criterion on the oracle's cleaned z of a case: a region is hot if |sum z| >= cut sqrt(n) or
    one of its aligned 64-bin trips has |sum| >= 8 cut, cut = 0.75 thr.  Returns (regions that are hot with `margin`
    to spare, regions that are not hot even with the cut divided by `margin`): the summation order cannot move a
    region across either."""
    sure, sure_not = 0, 0
    for z in oracle_of(name)["regions"]:
        n = len(z)
        if n == 0 or not np.all(np.isfinite(z)):
            sure_not += 1
            continue
        trips = max(abs(float(np.sum(z[t:t + 64]))) for t in range(0, n, 64))
        whole = abs(float(np.sum(z)))
        cut = HOT_CUT * THR
        if whole >= margin * cut * np.sqrt(n) or trips >= margin * cut * 8.0:
            sure += 1
        elif whole < cut * np.sqrt(n) / margin and trips < cut * 8.0 / margin:
            sure_not += 1
    return sure, sure_not


def hot_list_capacity(n_regions):
    return HOT_CAP_BIG if n_regions >= HOT_BIG_FROM else HOT_CAP_SMALL


# ------------------------------------------------------------------------------------------ the GPU plan ----
# route -> (environment, kind of call): `alone` one sample per call, `batch` PLACES samples, `direct`
# wt.stouffer_segments on the oracle's cleaned z.  Every route runs every case of LIMIT_CASES.
PLACES = 34
ROUTES = {
    "latency": ({}, "alone"),
    "latency_eager": ({"WC_TEST_LATENCY_MODE": "2"}, "alone"),
    "latency_off": ({"WC_TEST_LATENCY_MODE": "0"}, "alone"),            # a lone sample on k_seg_walk
    "walker": ({}, "batch"),
    "walker_no_hot": ({"WC_TEST_WALK_HOT": "0"}, "batch"),
    "host": ({"WC_TEST_WALK": "0"}, "batch"),
    "host_one_part": ({"WC_TEST_WALK": "0", "WC_CELL_PARTS": "1"}, "batch"),
    "host_row_blocks": ({"WC_TEST_WALK": "0", "WC_TEST_CELLS": "0"}, "batch"),
    "direct": ({}, "direct"),
}
LIMIT_CASES = [c["name"] for c in CASES if c["layout"] != "hot"]


def provides(name):
    case = case_of(name)
    return (case["limit"], case["side"])


def places_of(names, n_places):
    """The samples dealt round the places of a call (test_call_rows_gpu.places_of)."""
    return [names[i % len(names)] for i in range(max(n_places, len(names)))]


def batch_calls():
    """[(label, the distinct samples of the call)] of the `batch` routes: every case that must make a walker give up
    in a call of its own between quiet samples, all of them together (the bits OR-ed over the batch), and every case at
    or below a capacity together in a call that must NOT give up."""
    calls = []
    for lay in ("seg", "short"):
        mine = [n for n in LIMIT_CASES if case_of(n)["layout"] == lay and n not in FILLERS[lay]]
        beyond = [n for n in mine if case_of(n)["side"] == "beyond"]
        within = [n for n in mine if case_of(n)["side"] != "beyond"]
        if within:
            calls.append(("%s-within" % lay, within + FILLERS[lay]))
        for n in beyond:
            calls.append((n, [n] + FILLERS[lay]))
        if len(beyond) > 1:
            calls.append(("%s-all-beyond" % lay, beyond + FILLERS[lay]))
    return calls


def call_status(names):
    status = 0
    for n in set(names):
        status |= expected_status(n)
    return status


@functools.lru_cache(maxsize=None)
def segments_of(name):
    """wo.segment_tri of every chromosome of a case, over the triangles test_sample filled."""
    want = oracle_of(name)
    with np.errstate(all="ignore"):
        return [wo.segment_tri(tri, len(z), THR, MIN_SEARCH) for tri, z in zip(want["tris"], want["regions"])]


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))
