"""seg_cases.py against the oracle, on the CPU: every case gives exactly its planted calls in wo.test_sample, sits
where its design says relative to a capacity of the walkers (walk_model over the oracle's own triangles), its ties are
bit-equal and nothing else comes near an extreme; the early-starter calls have the numbers of hot regions they are for;
and every row of REQUIRED has a case on the route that must see it."""
import numpy as np
import pytest

import seg_cases as sc
from oracle import wc_oracle as wo

# what the model must measure on the region that carries the limit: (key of walk_model, value, status of the case)
DESIGN = {
    "ladder-64": ("stack", sc.WALK_STACK, 0),
    "ladder-65": ("stack", sc.WALK_STACK + 1, 16),
    "ladder-66": ("stack", sc.WALK_STACK + 1, 16),           # (the walk stops at the first job that does not fit)
    "ladder-83-no-right": ("stack", 1, 0),
    "balanced-128": ("segments", sc.TREE_SEGS, 0),
    "balanced-129": ("segments", sc.TREE_SEGS + 1, 8),
    "ties-64": ("ties_hi", sc.CJ_REC, 0),
    "ties-65": ("ties_hi", sc.CJ_REC + 1, 4),
    "ties-64-min": ("ties_lo", sc.CJ_REC, 0),
    "ties-65-min": ("ties_lo", sc.CJ_REC + 1, 4),
    "ties-65-champion-below": ("ties_hi", sc.CJ_REC + 1, 4),
    "mixed": (None, None, 16 | 4),
    "quiet": (None, None, 0),
    "one-span": (None, None, 0),
    "short-inf": (None, None, 2),
    "short-order": (None, None, 0),
    "short-plain-small": (None, None, 0),
}


def test_layouts():
    seg, hot = sc.layout("seg"), sc.layout("hot")
    assert seg["kept_sizes"][:3] == [520, 332, 40] and int(seg["msizes"].max()) <= sc.TREE_MAXLEN
    # the early-starter list exists only beyond the fused set-up's region length; the oracle's region stays small
    assert int(hot["msizes"][sc.BULK]) > sc.TREE_MAXLEN and hot["kept_sizes"][sc.BULK] == sc.BULK_KEPT
    assert hot["kept_sizes"][0] == 149 and sum(hot["kept_sizes"]) == 149 + 39 + 20 * 40
    assert sc.POOL_COUNTS.mean() == sc.LEVEL
    for lay in (seg, hot):
        assert lay["idx"].shape == (lay["n_bins"], sc.K) and int(lay["mask"].sum()) == lay["n_bins"]
        for c in range(22):                              # the lists: other chromosomes only, pool chromosomes only
            lo, hi = lay["moff"][c], lay["moff"][c + 1]
            bins = lay["refs_of"][c]
            assert np.all((bins < lo) | (bins >= hi)) and len(set(bins.tolist())) == sc.K
            assert np.all(bins >= lay["moff"][sc.POOL[0]]) and not np.any(np.isin(bins, lay["loud"]))
    for name in sc.HOT:                                  # the bins that were meant to go are gone, in every sample
        assert [len(z) for z in sc.oracle_of(name)["regions"]] == hot["kept_sizes"], name


@pytest.mark.parametrize("name", sc.LIMIT_CASES)
def test_case_is_what_it_was_designed_to_be(name):
    case, smp, lay = sc.case_of(name), sc.case_sample(name), sc.layout_of(name)
    want = sc.oracle_of(name)
    segs = sc.segments_of(name)
    rows = sc.rows_of(want)
    assert len(rows) == sum(len(s) for s in segs)
    key, value, status = DESIGN[name]
    walk, tree = sc.models_of(name, "walk"), sc.models_of(name, "tree")
    print(name, "status", sc.expected_status(name), "tree", sc.expected_status(name, "tree"),
          [(c + 1, {k: v for k, v in m.items() if v}) for c, m in enumerate(walk) if m["segments"] or m["status"]])
    assert sc.expected_status(name) == status
    assert sc.expected_status(name, "tree") == int(status != 0)         # the two tie rules agree on every case
    assert (status != 0) == (case["side"] == "beyond")
    if case["wraps"]:
        return
    # the calls: every spike of a profile as a window of one bin, the spans as they were planted, nothing else
    for c in range(22):
        got = [(x, y) for _, (x, y) in segs[c]]
        planted = [(i, i) for chrom, i in smp["spikes"] if chrom == c + 1] + [(x, y) for chrom, x, y in smp["spans"] if chrom == c + 1]
        assert got == sorted(planted), (name, c + 1, got)
        if not planted:            # the background stays below the threshold (the reference bins' LEVEL +- 9 come closest)
            assert np.max(np.abs(want["tris"][c])) < sc.THR - 1.0, (name, c + 1)
    for chrom, L in case["profiles"].items():
        z, tri = want["regions"][chrom - 1], want["tris"][chrom - 1]
        # equal counts are bit-equal z; the windows that hold no spike stay below the threshold
        for level in np.unique(L):
            assert len(set(z[L == level].view(np.int64).tolist())) == 1, (name, chrom, level)
        spikes = np.flatnonzero(np.abs(L) >= sc.TIE)
        for a, b in zip(np.concatenate([[-1], spikes]), np.concatenate([spikes, [len(L)]])):
            if b - a > 1:
                sub, _ = wo._sub_triangle(tri, len(L), a + 1, b)
                assert np.max(np.abs(sub)) < sc.THR - 0.5, (name, chrom, a, b)
        # no window within 1e-6 (relative) of a job's extreme that is not bit-equal to it: the kernels' 2 eps record
        # (window_eps: (2 n + 64) 2^-53 sum |z|, far inside that margin) holds the planted ties and nothing else
        assert walk[chrom - 1]["near"] == 0 and tree[chrom - 1]["near"] == 0
        eps = (2 * len(L) + 64) * 2.0 ** -53 * float(np.sum(np.abs(z)))
        assert 2 * eps < 1e-6 * float(np.min(np.abs(z[spikes]))) / 100
    if key:
        (chrom,) = case["profiles"].keys()
        assert walk[chrom - 1][key] == value, (name, walk[chrom - 1])
        if key.startswith("ties"):                       # the ties are among the single-bin windows of ONE value of z
            z = want["regions"][chrom - 1]
            L = case["profiles"][chrom]
            tied = z[np.flatnonzero(np.abs(L) == sc.TIE)]
            assert len(tied) == value and len(set(tied.view(np.int64).tolist())) == 1
            assert abs(tied[0]) > sc.THR + 1
        if name == "ties-65-champion-below":             # the root's champion is the lone minimum, the ties are maxima
            assert segs[chrom - 1][-1][0] < 0 and abs(segs[chrom - 1][-1][0]) > 2 * abs(segs[chrom - 1][0][0])
            assert walk[chrom - 1]["ties_lo"] == 1


def test_at_limit_and_one_past():
    """Both sides of every capacity are there, one apart."""
    by = {}
    for name in sc.LIMIT_CASES:
        key, value, _ = DESIGN[name]
        if key:
            by.setdefault((sc.case_of(name)["limit"], sc.case_of(name)["side"]), []).append(value)
    for limit, cap in (("stack", sc.WALK_STACK), ("segments", sc.TREE_SEGS), ("ties_hi", sc.CJ_REC), ("ties_lo", sc.CJ_REC)):
        assert by[(limit, "at")] == [cap] and set(by[(limit, "beyond")]) == {cap + 1}, (limit, by)
    # the ladder: 64 spikes are the most that fit and 65 the first that do not (every level adds one pending job)
    assert sc.models_of("ladder-64")[1]["depth"] == sc.WALK_STACK and sc.models_of("ladder-65")[1]["status"] == 16


def test_model_on_hand_made_triangles():
    thr = 5.0
    # one loud bin in the middle: a segment, two quiet children pushed (0 pending + 2)
    z = np.zeros(11)
    z[5] = 9.0
    m = sc.walk_model(wo.fill_tri(z), 11, thr)
    assert (m["status"], m["segments"], m["stack"], m["ties_hi"], m["ties_lo"]) == (0, 1, 2, 1, 0)
    # ... at bin 3 / three bins before the end: x > min_search and y + 1 < edge - min_search are both false
    z = np.zeros(7)
    z[3] = 9.0
    assert sc.walk_model(wo.fill_tri(z), 7, thr)["stack"] == 0
    # two equal maxima: the first is taken, the second found in its right child; the tree's rule also counts the
    # windows tied at 0.0 for the minimum
    z = np.zeros(12)
    z[1] = z[7] = 9.0
    m = sc.walk_model(wo.fill_tri(z), 12, thr)
    assert (m["segments"], m["ties_hi"], m["ties_lo"]) == (2, 2, 0)
    assert sc.walk_model(wo.fill_tri(z), 12, thr, tie_rule="tree")["ties_lo"] > 2
    with np.errstate(all="ignore"):
        z[4] = np.inf
        assert sc.walk_model(wo.fill_tri(z), 12, thr)["status"] == 2
    # all quiet
    assert sc.walk_model(wo.fill_tri(np.full(9, 0.3)), 9, thr) == dict(status=0, segments=0, stack=0, ties_hi=0, ties_lo=0,
                                                                       near=0, depth=0)


def test_batch_calls():
    """The calls of the batch routes: a case that must not give up never shares a call with one that must, every
    give-up bit is seen alone, and the bits of a whole batch are OR-ed."""
    calls = dict(sc.batch_calls())
    assert sc.call_status(calls["seg-within"]) == 0 and sc.call_status(calls["short-inf"]) == 2
    assert {sc.call_status(names) for names in calls.values()} >= {0, 2, 4, 8, 16, 20, 28}
    assert sc.call_status(calls["seg-all-beyond"]) == 28
    everything = {n for names in calls.values() for n in names}
    assert everything == set(sc.LIMIT_CASES)
    for lay, fillers in sc.FILLERS.items():
        assert sc.call_status(fillers) == 0
        assert len({sc.case_of(n)["repeats"] for n in sc.LIMIT_CASES if sc.case_of(n)["layout"] == lay}) == 1
    for names in calls.values():                         # one reference per call
        assert len({sc.case_sample(n)["pca_mean"].tobytes() for n in names}) == 1 and len(names) <= sc.PLACES


def test_hot_list_calls():
    """The early-starter list (k_region_prefix fills it): 48 places hold more hot regions than its 512 entries, 9
    places fewer, 192 places (4 224 regions: the 4 096-entry list) more than 512 and fewer than 4 096 -- with a factor
    of two to spare on either side of the cut."""
    sure = {n: sc.hot_regions(n)[0] for n in sc.HOT}
    maybe = {n: 22 - sc.hot_regions(n)[1] for n in sc.HOT}
    print("hot regions per sample (sure, at most):", [(n, sure[n], maybe[n]) for n in sc.HOT])
    call48, call192 = sc.places_of(sc.HOT, 48), sc.places_of(sc.HOT, 192)
    assert sc.hot_list_capacity(48 * 22) == 512 and sum(sure[n] for n in call48) > 512
    assert sum(maybe[n] for n in call48[:9]) < 512
    assert sc.hot_list_capacity(192 * 22) == 4096 and 512 < sum(sure[n] for n in call192)
    assert sum(maybe[n] for n in call192) < 4096
    assert len(set(sure.values())) >= 4                  # samples with different numbers of hot regions
    for n in sc.HOT:
        assert sc.expected_status(n) == 0
        assert len(sc.rows_of(sc.oracle_of(n))) == len(sc.case_sample(n)["spans"]) + 1    # (+ the loud bins of chromosome 21)


def test_every_required_row_has_a_home():
    have = {sc.provides(n) for n in sc.LIMIT_CASES}
    assert set(sc.REQUIRED) == set(sc.ROUTES)
    for route, rows in sc.REQUIRED.items():
        assert rows <= have, (route, sorted(rows - have))
    for limit in ("ties_hi", "ties_lo", "segments", "stack"):
        for side in ("at", "beyond"):
            for route in ("latency", "latency_eager", "latency_off", "walker", "walker_no_hot"):
                assert (limit, side) in sc.REQUIRED[route]
