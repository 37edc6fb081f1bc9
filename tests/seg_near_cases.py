"""Inputs, expectations and a model for the NEAR-family segmentation tests (a helper module, not a conftest; it builds
on seg_cases.py and shares its `seg` layout, fillers, routes and oracle pattern).

The window search of csrc/testpath.hip ranks windows by prefix-sum differences, (P[y + 1] - P[x]) * rs[len], trusts
window_eps(n, sum |z|) = (2 n + 64) 2^-53 sum |z| as the bound of that estimate against numpy's value, lists every
window within 2 eps of the approximate extreme as a candidate, re-evaluates the candidates in numpy's own summation
order and takes numpy's argmax / argmin among them (larger value, else lower row-major position).  seg_cases.py plants
BIT-EQUAL ties; random data has one candidate per job.  The cases here are the class in between: windows that differ in
numpy's last bits and that no prefix sum can tell apart.

A NEAR FAMILY is the set of windows of one job within eps / 1000 of the job's extreme by the oracle's values, eps =
window_eps of the region.  z is an affine function of the read count (seg_cases' construction), so windows of equal
length and equal count sum are equal in real arithmetic and differ only by how each z and each sum happened to round.

Count-built cases (through wt.test_batch, every route of seg_cases.ROUTES):

    near-hi-40, near-lo-40   forty two-bin windows (a_i, PAIR - a_i), four bins of -PAIR / 4 behind each, on chromosome
                             2, and the mirror image (the family at the minimum).  The count sum is PAIR = 240: the
                             rounding of a single z is 24 ulps of the window value here (data = count / total is rounded
                             at the size of LEVEL, not of the z), the family spreads over 48 ulps = eps / 1 700.  (With a
                             sum of 60 the same 96-ulp grid is eps / 860 wide and the family would reach into the guard
                             band.)
    near-64, near-65         64 / 65 such pairs in groups of eight bins on chromosome 1 (520 kept bins): at and one past
                             CAND_CAP = CJ_REC = 64.  The first of the six filler bins behind a pair has its own depth in
                             every group, so that the MINIMUM of every job is unique and k_seg_tree's two-sided record
                             cannot overflow on the wrong side; three fillers are quiet, so that the segments stay
                             within TREE_SEGS.
    near-long                three bumps of 140 bins that hold one multiset of counts in three orders -- beyond numpy's
                             128-element leaf, so the pairwise split decides the last bits -- with troughs of 30 bins of
                             -25, -27, -29 behind them.
    giant-first, giant-last  (`giant-near` in its two variants) near-hi-40's pairs with one bin of count LEVEL +
                             2 000 000 000 (z = 3.6e8) as the first / the last kept bin of the region: eps grows by six orders of magnitude, and with the giant in
                             front every later prefix entry carries ulp(3.6e8) of rounding.  The fillers are the varied
                             ones here: with groups that sum to exactly zero every pair would start at the same prefix
                             value, all of them would round alike on top of the giant and the forty estimates would
                             coincide in any tree-like scan -- the rounding would never show.
    thr-edge                 near-hi-40's region (champion v*: the largest bit pattern of the family) and a plain loss on
                             chromosome 1 (champion -w*), run at threshold = v*, nextafter(v*), w*, nextafter(w*).

Float-built cases (wt.stouffer_segments only, expectations from wo.fill_tri / wo.fill_tri_min + wo.segment_tri):
ulp-ladder (and its masked variant) and sign-tie, see float_cases().

near_model restates the walkers' give-up rule with CANDIDATES (windows within 2 eps of the extreme by the oracle's
values) where seg_cases.walk_model counts bit-equal ties; test_seg_near_cases_cpu.py shows that the candidate sets do
not depend on the kernels' prefix order (the guard band) and holds every case to its design with the oracle alone.
"""
import functools

import numpy as np

import call_cases as cc
import seg_cases as sc
from oracle import wc_oracle as wo

LEVEL, THR, REPEATS, MIN_SEARCH = sc.LEVEL, sc.THR, sc.REPEATS, sc.MIN_SEARCH
CAND_CAP = sc.CAND_CAP
PAIR = 240                                       # count sum of a pair: the window is 240 / 5.52 / sqrt(2) = 30.7
GIANT = 2_000_000_000                            # LEVEL + GIANT stays inside int32
FAMILY, BAND = 1e-3, 8.0                         # a family: within FAMILY eps; nothing else within BAND eps
N2 = 332                                         # kept bins of chromosome 2 (layout `seg`; chromosome 1: 520)


def window_eps(z):
    """window_eps of csrc/testpath.hip for a region of cleaned z."""
    return (2.0 * len(z) + 64.0) * 2.0 ** -53 * float(np.sum(np.abs(z)))


# ------------------------------------------------------------------------------------------ the profiles ----
def splits(k):
    """The first counts a_i of k pairs: every a and PAIR - a stays below PAIR / sqrt(2) (no single bin beats its pair),
    in a scrambled order."""
    lo, hi = 74, 166
    values = [lo + (i * (hi - lo)) // (k - 1) for i in range(k)]
    return [values[(i * 27 + 11) % k] for i in range(k)]       # (27 is prime to 40, 64 and 65)


QUIET_GROUPS = (9, 30, 51)


def pairs(k, group=6, varied=False, quiet=()):
    """k groups: the pair (a_i, PAIR - a_i) and group - 2 filler bins of -PAIR / (group - 2): every group sums to zero,
    the filler as a whole is one call and the k filler windows are bit-equal.  varied: the first filler bin of group i
    is deeper by u_i, a scrambled 0 .. k - 1 -- every job's minimum is unique, a group sums to -u_i (the whole region:
    -2 080 / sqrt(520), weaker than one filler) and the deepest filler, 304 / 5.52 / sqrt(6) = 22.5, stays below the
    pair (groups of six: 279 / 5.52 / sqrt(4) = 25.3).  quiet: the groups whose fillers are six bins of -7, no call (65 pairs and 62 fillers stay within
    TREE_SEGS = 128 segments; two pairs with a quiet filler between them are 473 / sqrt(10), below the pair's 240 /
    sqrt(2))."""
    L = np.zeros(k * group, dtype=np.int64)
    for i, a in enumerate(splits(k)):
        L[group * i], L[group * i + 1] = a, PAIR - a
        L[group * i + 2:group * (i + 1)] = -PAIR // (group - 2)
        if varied:
            L[group * i + 2] -= (i * 29 + 3) % k         # (29 is prime to 40, 64 and 65)
            if i in quiet:
                L[group * i + 2:group * (i + 1)] = -7
    return L


def bumps(seed, n_bumps=3, length=140, trough=30):
    """n_bumps bumps of one multiset of counts 4 .. 9 (every count above half the mean: the whole bump, 910 / 5.52 /
    sqrt(140) = 13.9, is its best window) in different orders, a trough of -25, -27, -29 ... behind each (deeper than
    910 (2 - sqrt(310 / 140)) = 466 in all: no window over two bumps beats one)."""
    rng = np.random.RandomState(seed)
    base = 4 + np.arange(length) % 6
    parts = []
    for b in range(n_bumps):
        parts += [rng.permutation(base), np.full(trough, -(25 + 2 * b))]
    return np.concatenate(parts).astype(np.int64)


LONG_SEED = 5                # (of the seeds 1 .. 8: 2, 5 and 7 give two distinct values; 5 and 7 put the second bump on top)


# ------------------------------------------------------------------------------------------ the cases ----
# a case: spans [(chromosome, first kept bin, L)] over the `seg` background, the region and side of its family, the
# thresholds it runs at (None: THR), and whether a walker must give up on it.
def _cases():
    hi40, hi40v = pairs(40), pairs(40, varied=True)
    cases = {}

    def add(name, spans, chrom, side, size, beyond=False, thresholds=(None,)):
        cases[name] = dict(name=name, spans=spans, chrom=chrom, side=side, size=size, beyond=beyond, thresholds=thresholds)

    add("near-hi-40", [(2, 0, hi40)], 2, "hi", 40)
    add("near-lo-40", [(2, 0, -hi40)], 2, "lo", 40)
    add("near-64", [(1, 0, pairs(64, 8, True, QUIET_GROUPS))], 1, "hi", 64)
    add("near-65", [(1, 0, pairs(65, 8, True, QUIET_GROUPS))], 1, "hi", 65, beyond=True)
    add("near-long", [(1, 0, bumps(LONG_SEED))], 1, "hi", 3)
    add("giant-first", [(2, 0, np.array([GIANT])), (2, 6, hi40v)], 2, "hi", 40)
    add("giant-last", [(2, 0, hi40v), (2, N2 - 1, np.array([GIANT]))], 2, "hi", 40)
    add("thr-edge", [(1, 100, sc.span_levels(6, -1)), (2, 0, hi40)], 2, "hi", 40, thresholds=("v", "v+", "w", "w+"))
    return cases


CASES = _cases()
COUNT_CASES = [n for n in CASES if n != "thr-edge"]
FILLERS = sc.FILLERS["seg"]
WITHIN = [n for n in COUNT_CASES if not CASES[n]["beyond"]]
THR_EDGE_ROUTES = ("latency", "walker", "host", "host_row_blocks", "direct")


def is_filler(name):
    return name in FILLERS


@functools.lru_cache(maxsize=None)
def case_sample(name):
    if is_filler(name):
        return sc.case_sample(name)
    lay = sc.layout("seg")
    spans = [(chrom, x, [int(v) for v in LEVEL + L], None) for chrom, x, L in CASES[name]["spans"]]
    for _, _, counts, _ in spans:
        assert 0 <= min(counts) and max(counts) < 2 ** 31
    smp = cc.sample(lay, spans)
    assert np.all(smp["pca_mean"] == lay["pca_mean"])
    return smp


@functools.lru_cache(maxsize=None)
def oracle_of(name, thr=THR):
    """seg_cases.oracle_of_sample of a case at a threshold, computed once."""
    if is_filler(name) and thr == THR:
        return sc.oracle_of(name)
    return sc.oracle_of_sample(sc.layout("seg"), case_sample(name), REPEATS, thr)


@functools.lru_cache(maxsize=None)
def segments_of(name, thr=THR):
    want = oracle_of(name, thr)
    return [wo.segment_tri(tri, len(z), thr, MIN_SEARCH) for tri, z in zip(want["tris"], want["regions"])]


@functools.lru_cache(maxsize=None)
def thresholds_of(name):
    """label -> threshold of a case.  thr-edge: v = the champion of the family's region, w = |champion| of the loss on
    chromosome 1, and the next float above each."""
    if CASES[name]["thresholds"] == (None,):
        return {None: THR}
    want = oracle_of(name)
    v = float(want["tris"][1].max())
    w = float(-want["tris"][0].min())
    return {"v": v, "v+": float(np.nextafter(v, np.inf)), "w": w, "w+": float(np.nextafter(w, np.inf))}


# ---------------------------------------------------------------------------- the walkers' rules, restated ----
def jobs_of(tri, edge, thr=THR, min_search=MIN_SEARCH):
    """Every job the reference's recursion visits (wo.segment_tri), in the walkers' order: (lo, hi, sub-triangle, n,
    position of the champion or None for a quiet job, stack occupancy after the pop)."""
    stack = [(0, edge)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo <= 0:
            continue
        sub, n = wo._sub_triangle(tri, edge, lo, hi)
        vmax, vmin = sub.max(), sub.min()
        if max(abs(vmax), abs(vmin)) < thr:
            yield lo, hi, sub, n, None, len(stack)
            continue
        pos = int(sub.argmax())
        if abs(vmin) > vmax:
            pos = int(sub.argmin())
        x, y = wo.lin_to_2d(n, pos)
        yield lo, hi, sub, n, pos, len(stack)
        if y + 1 < n - min_search:
            stack.append((lo + y + 1, hi))
        if x > min_search:
            stack.append((lo, lo + x))


def near_model(tri, z, thr=THR, tie_rule="walk"):
    """seg_cases.walk_model with the record the kernels really keep: per job and per side that counts (tie_rule as
    there), the windows whose oracle value lies within 2 eps of the extreme; more than CAND_CAP of them -> status 4.
    Segments, stack and the order of the walk are walk_model's.  Returns dict(status, segments, stack, cand_hi,
    cand_lo: the most candidates of a job per side)."""
    res = dict(status=0, segments=0, stack=0, cand_hi=0, cand_lo=0)
    edge = len(z)
    if not np.all(np.isfinite(tri)):
        res["status"] = 2
        return res
    eps = window_eps(z)
    pending = 0
    for lo, hi, sub, n, pos, below in jobs_of(tri, edge, thr):
        if pos is None:
            continue
        vmax, vmin = sub.max(), sub.min()
        if tie_rule == "tree" or abs(vmax) >= thr:
            res["cand_hi"] = max(res["cand_hi"], int(np.sum(sub >= vmax - 2 * eps)))
        if tie_rule == "tree" or abs(vmin) >= thr:
            res["cand_lo"] = max(res["cand_lo"], int(np.sum(sub <= vmin + 2 * eps)))
        if max(res["cand_hi"], res["cand_lo"]) > CAND_CAP:
            res["status"] |= 4
            break
        x, y = wo.lin_to_2d(n, pos)
        res["segments"] += 1
        if res["segments"] > sc.TREE_SEGS:
            res["status"] |= 8
        pushes = (x > MIN_SEARCH) + (y + 1 < n - MIN_SEARCH)
        res["stack"] = max(res["stack"], below + pushes)
        if below + pushes > sc.WALK_STACK:
            res["status"] |= 16
        if res["status"]:
            break
    return res


@functools.lru_cache(maxsize=None)
def models_of(name, tie_rule="walk", thr=THR):
    want = oracle_of(name, thr)
    return [near_model(tri, z, thr, tie_rule) for tri, z in zip(want["tris"], want["regions"])]


def expected_status(name, kernel="walk", thr=THR):
    """The word k_seg_walk must leave for a call that holds this case, or (kernel="tree") whether k_seg_tree hands the
    call back."""
    status = 0
    for m in models_of(name, kernel, thr):
        status |= m["status"]
    return status if kernel == "walk" else int(status != 0)


def call_status(names, thr=THR):
    status = 0
    for n in set(names):
        status |= expected_status(n, "walk", thr)
    return status


# ------------------------------------------------------------------------------------------ the families ----
@functools.lru_cache(maxsize=None)
def family_job(name, thr=THR):
    """The first job of the walk over the case's region whose family (on the case's side) has the designed size:
    dict(lo, hi, sub, n, windows, values, nearest, winner: numpy's argmax / argmin of the job, eps, z)."""
    case, want = CASES[name], oracle_of(name, thr)
    z, tri = want["regions"][case["chrom"] - 1], want["tris"][case["chrom"] - 1]
    eps = window_eps(z)
    for lo, hi, sub, n, pos, _ in jobs_of(tri, len(z), thr):
        if pos is None:
            continue
        windows, values, nearest = family_of(sub, n, case["side"], eps)
        if len(windows) == case["size"]:
            winner = wo.lin_to_2d(n, int(sub.argmax() if case["side"] == "hi" else sub.argmin()))
            return dict(lo=lo, hi=hi, sub=sub, n=n, windows=windows, values=values, nearest=nearest, winner=winner,
                        eps=eps, z=z)
    raise AssertionError("%s: no job with a family of %d" % (name, case["size"]))


def family_of(sub, n, side, eps):
    """[(x, y)] of the windows of a job within FAMILY eps of its extreme on a side, in row-major order, their values,
    and the distance (in eps) of the nearest window that is NOT in the family."""
    if side == "hi":
        dist = sub.max() - sub
    else:
        dist = sub - sub.min()
    member = dist <= FAMILY * eps
    at = np.flatnonzero(member)
    rest = dist[~member]
    nearest = float(rest.min()) / eps if len(rest) else np.inf
    return [wo.lin_to_2d(n, int(p)) for p in at], sub[at], nearest


def prefix_orders(z):
    """Prefix arrays P (P[0] = 0, P[i] = z[0] + ... + z[i - 1]) in four orders: np.cumsum, a pairwise (tree) cumulative
    sum, a scan in 64-bin trips with a running carry (np.cumsum inside a trip), and `wave`: k_region_prefix's own
    order, the same trips with a 64-lane shuffle scan (lane i adds lane i - 1, i - 2, i - 4 ... of the step before)
    inside each."""
    z = np.asarray(z, dtype=np.float64)

    def tree(a):
        if len(a) <= 1:
            return a.copy()
        half = len(a) // 2
        left, right = tree(a[:half]), tree(a[half:])
        return np.concatenate([left, left[-1] + right])

    def shuffle_scan(a):
        incl = np.zeros(64)
        incl[:len(a)] = a
        o = 1
        while o < 64:
            incl[o:] = incl[o:] + incl[:-o]
            o *= 2
        return incl

    out = {"cumsum": np.cumsum(z), "pairwise": tree(z)}
    for name, scan in (("trips", np.cumsum), ("wave", shuffle_scan)):
        parts, carry = [], 0.0
        for t in range(0, len(z), 64):
            local = scan(z[t:t + 64])
            parts.append((carry + local)[:len(z) - t])
            carry = carry + local[-1]
        out[name] = np.concatenate(parts)
    return {name: np.concatenate([np.zeros(1), P]) for name, P in out.items()}


def estimates(P, windows, lo=0):
    """The kernels' estimate (P[y + 1] - P[x]) * rs[len] of windows given in a job's own coordinates."""
    return np.array([(P[lo + y + 1] - P[lo + x]) * (1.0 / np.sqrt(y - x + 1.0)) for x, y in windows])


# ------------------------------------------------------------------------------------------ the float cases ----
LADDER_N, LADDER_K, LADDER_AT = 300, 40, 5
SORTED_ENV = {"WC_MINEFFECT": "sorted"}


def ladder_steps():
    """j of spike i: 39 at the spikes 20 and 31 (bit-equal, the first one in the middle of the ladder), a scrambled
    0 .. 37 at the 38 others."""
    order, k = [], 0
    for i in range(LADDER_K):
        if i in (20, 31):
            order.append(39)
        else:
            order.append((k * 17 + 5) % 38)
            k += 1
    return order


@functools.lru_cache(maxsize=None)
def float_cases():
    """name -> dict(z, r, mineffect, thresholds): one region each.

    ulp-ladder: z[0] = 1e12 (the prefix sums behind it have a granularity of 1.2e-4, eps is 0.07), four quiet bins,
    then 40 single-bin spikes 9 + j 2^-49 five bins apart on four bins of -2.25 (every other window is more than 1
    away from 9; a single-bin window is exact in numpy): each job's answer is its largest spike, the first of equals.
    ulp-ladder-masked: ratios of 1.3 and mineffectsize 0.1, with a ratio of 1.0 on numpy's unmasked argmax (spike 20)
    and three more family members: those windows are exactly 0 in fill_tri_min.
    sign-tie: +9 at bin 10, nextafter(9, 0) at bin 30, -9 at bin 50: the root's extremes are bit-equal in magnitude
    (the maximum is taken), the right child's |minimum| is one ulp above its maximum (the minimum is taken)."""
    z = np.zeros(LADDER_N)
    z[0] = 1e12
    z[1:LADDER_AT] = [0.5, -0.25, 0.25, -0.5]
    spikes = [LADDER_AT + 5 * i for i in range(LADDER_K)]
    for i, j in enumerate(ladder_steps()):
        z[spikes[i]] = 9.0 + j * 2.0 ** -49
        z[spikes[i] + 1:spikes[i] + 5] = -2.25
    tail = np.arange(LADDER_AT + 5 * LADDER_K, LADDER_N)
    z[tail] = np.where(tail % 2 == 0, 0.25, -0.375)
    r = np.full(LADDER_N, 1.3)
    masked = [spikes[20], spikes[3], spikes[31], spikes[12]]
    r[masked] = 1.0
    tie = np.zeros(64)
    tie[::2], tie[1::2] = 0.125, -0.25
    tie[10], tie[30], tie[50] = 9.0, np.nextafter(9.0, 0.0), -9.0
    nine_up = float(np.nextafter(9.0, np.inf))
    cases = {
        "ulp-ladder": dict(z=z, r=None, mineffect=0, thresholds=(THR,), spikes=spikes, masked=[]),
        "ulp-ladder-masked": dict(z=z, r=r, mineffect=0.1, thresholds=(THR,), spikes=spikes, masked=masked),
        "sign-tie": dict(z=tie, r=None, mineffect=0, thresholds=(9.0, nine_up), spikes=[10, 30, 50], masked=[]),
    }
    for case in cases.values():
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def float_want(name, thr):
    """(triangle, segments) of a float case: wo.fill_tri / wo.fill_tri_min and wo.segment_tri."""
    case = float_cases()[name]
    z = np.array(case["z"])
    tri = wo.fill_tri_min(z, np.array(case["r"]), case["mineffect"]) if case["mineffect"] else wo.fill_tri(z)
    return tri, wo.segment_tri(tri, len(z), thr, MIN_SEARCH)
