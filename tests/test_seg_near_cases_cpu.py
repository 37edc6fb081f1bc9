"""seg_near_cases.py against the oracle, on the CPU: every case is what it was designed to be -- a family of the stated
size, with the stated number of distinct bit patterns and numpy's winner at the stated place -- and, which is what makes
the GPU expectations independent of the code under test, the kernels' candidate sets cannot depend on their prefix order:

* the guard band: in every job the recursion visits, on either side, no window lies between eps / 1000 and 8 eps from
  the extreme.  A sound estimate is within eps of numpy's value (window_eps is the bound the kernels trust), so the
  approximate extreme is within eps of the true one, the cut `extreme - 2 eps` lies between 1 eps and 3 eps below it by
  true values, a family member (estimate within eps / 100, measured below) passes it and a window 8 eps away (estimate
  at most 7 eps from the extreme) does not: whatever order the prefix sums are taken in, the record is the family;
* the spread of the estimates, measured for four prefix orders (np.cumsum, a pairwise cumulative sum, a scan in 64-bin
  trips with a running carry, and the same trips with k_region_prefix's shuffle scan inside): |estimate - oracle value| over the family stays below eps / 100 (the giant cases: below
  eps, they predict "no give-up" and not a count).

test_wrong_implementations names, from the same family data, the case that fails under each of three plausible but
wrong candidate rules."""
import numpy as np
import pytest

import seg_cases as sc
import seg_near_cases as nc
from oracle import wc_oracle as wo

# family size, distinct bit patterns in it, members bit-equal to the extreme, place of numpy's winner in row-major order
DESIGN = {
    "near-hi-40": (40, 3, 17, 2),
    "near-lo-40": (40, 6, 3, 23),
    "near-64": (64, 6, 2, 45),
    "near-65": (65, 3, 27, 0),
    "near-long": (3, 2, 1, 1),
    "giant-first": (40, 4, 9, 10),
    "giant-last": (40, 4, 10, 2),
}
ORDERS = ("cumsum", "pairwise", "trips", "wave")


def family_estimates(name):
    """order -> the estimates of the family's windows from that prefix order."""
    fj = nc.family_job(name)
    return {order: nc.estimates(P, fj["windows"], fj["lo"]) for order, P in nc.prefix_orders(fj["z"]).items()}


def top_by_estimate(name, est):
    fj = nc.family_job(name)
    at = int(np.argmax(est)) if nc.CASES[name]["side"] == "hi" else int(np.argmin(est))
    return fj["windows"][at]


@pytest.mark.parametrize("name", nc.COUNT_CASES)
def test_family(name):
    case, fj = nc.CASES[name], nc.family_job(name)
    size, distinct, bit_equal, place = DESIGN[name]
    values, windows = fj["values"], fj["windows"]
    extreme = values.max() if case["side"] == "hi" else values.min()
    got = (len(windows), len(set(values.view(np.int64).tolist())), int(np.sum(values == extreme)), windows.index(fj["winner"]))
    spread = float(np.max(np.abs(values - extreme)))
    print(name, "job [%d, %d)" % (fj["lo"], fj["hi"]), "eps %.3g" % fj["eps"], "family, distinct, bit-equal, winner's place:",
          got, "spread %.3g eps = %.0f ulps" % (spread / fj["eps"], spread / np.spacing(abs(extreme))))
    assert got == (size, distinct, bit_equal, place)
    assert size == case["size"] and spread <= nc.FAMILY * fj["eps"]
    assert values[place] == extreme and not np.any(values[:place] == extreme)      # numpy: the first of the largest
    lengths = {y - x for x, y in windows}
    assert len(lengths) == 1                                                       # one length: equal in real arithmetic
    if name in ("near-hi-40", "near-lo-40"):
        assert distinct >= 3 and 0 < place < size - 1
    if name in ("near-64", "near-65"):             # a mix of bit-equal and near windows, on one side only
        assert bit_equal >= 2 and size - bit_equal >= 2 and size == nc.CAND_CAP + (name == "near-65")
        other = fj["sub"].min()
        assert int(np.sum(fj["sub"] <= other + 2 * fj["eps"])) == 1                # the root's minimum is unique
    if name == "near-long":
        assert lengths == {139} and distinct >= 2 and place > 0                    # beyond numpy's 128-element leaf
    if name.startswith("giant"):
        z = fj["z"]
        at = 0 if name == "giant-first" else len(z) - 1
        assert z[at] > 3.5e8 and np.sum(np.abs(z)) - z[at] < 1e4 and fj["eps"] > 2e-5


@pytest.mark.parametrize("name", list(nc.CASES))
def test_guard_band(name):
    """No window between eps / 1000 and 8 eps from an extreme, in any job, on either side, in any region."""
    worst, widest, n_jobs = np.inf, 0.0, 0
    for thr in nc.thresholds_of(name).values():
        want = nc.oracle_of(name, thr)
        for c, (tri, z) in enumerate(zip(want["tris"], want["regions"])):
            eps = nc.window_eps(z)
            for lo, hi, sub, n, pos, _ in nc.jobs_of(tri, len(z), thr):
                if pos is None:
                    continue
                n_jobs += 1
                for side in ("hi", "lo"):
                    windows, values, nearest = nc.family_of(sub, n, side, eps)
                    assert nearest > nc.BAND, (name, thr, c + 1, lo, hi, side, nearest)
                    worst = min(worst, nearest)
                    widest = max(widest, float(np.max(np.abs(values - values[0]))) / eps)
    print(name, "%d jobs: the widest family spans %.3g eps, the nearest window outside one lies %.3g eps away" % (n_jobs, widest, worst))
    assert widest <= nc.FAMILY and worst > nc.BAND


@pytest.mark.parametrize("name", nc.COUNT_CASES)
def test_estimate_spread(name):
    fj = nc.family_job(name)
    ratios = {order: float(np.max(np.abs(est - fj["values"]))) / fj["eps"] for order, est in family_estimates(name).items()}
    print(name, "largest |estimate - oracle value| over the family, in eps:", {k: "%.3g" % v for k, v in ratios.items()})
    assert set(ratios) == set(ORDERS)
    bound = 1.0 if name.startswith("giant") else 1e-2
    assert max(ratios.values()) < bound, ratios


@pytest.mark.parametrize("name", nc.COUNT_CASES)
def test_model_statuses(name):
    walk, tree = nc.expected_status(name), nc.expected_status(name, "tree")
    models = [m for m in nc.models_of(name) if m["segments"] or m["status"]]
    print(name, "walk", walk, "tree", tree, models)
    assert (walk, tree) == ((4, 1) if name == "near-65" else (0, 0))
    assert (walk != 0) == nc.CASES[name]["beyond"]
    want = nc.oracle_of(name)
    for model in nc.models_of(name) + nc.models_of(name, "tree"):                  # the other capacities stay out of it
        assert model["segments"] <= sc.TREE_SEGS and model["stack"] <= sc.WALK_STACK
    assert sum(len(s) for s in nc.segments_of(name)) == len(sc.rows_of(want)) <= sc.TREE_SEGS
    old = [sc.walk_model(tri, len(z)) for tri, z in zip(want["tris"], want["regions"])]
    if name == "near-65":
        # the bit-equal model sees 27 ties and no reason to give up: why the candidate model is needed
        assert all(m["status"] == 0 for m in old) and max(m["ties_hi"] for m in old) == DESIGN[name][2]
        assert nc.models_of(name)[0]["cand_hi"] == nc.CAND_CAP + 1
    if name == "near-64":
        assert nc.models_of(name)[0]["cand_hi"] == nc.CAND_CAP and nc.models_of(name, "tree")[0]["cand_lo"] <= 3
    assert all(m["status"] == 0 for m in old)


def test_fillers_and_calls():
    for name in nc.FILLERS:
        assert nc.expected_status(name) == 0 and nc.expected_status(name, "tree") == 0
    assert nc.call_status(nc.WITHIN + nc.FILLERS) == 0 and nc.call_status(["near-65"] + nc.FILLERS) == 4
    assert len({nc.case_sample(n)["pca_mean"].tobytes() for n in list(nc.CASES) + nc.FILLERS}) == 1
    assert len(nc.WITHIN) + len(nc.FILLERS) <= sc.PLACES and set(nc.THR_EDGE_ROUTES) <= set(sc.ROUTES)


def test_thr_edge():
    """The reference calls when abs(champion) >= threshold: at v* the champion's row is there, one float higher it is
    not; the cleaned z does not move with the threshold (the reference pool is quiet, nothing is flagged there)."""
    thr = nc.thresholds_of("thr-edge")
    wants = {label: nc.oracle_of("thr-edge", t) for label, t in thr.items()}
    first = wants["v"]
    for label, want in wants.items():
        assert want["threshold_z"] == thr[label]
        for a, b in zip(first["regions"], want["regions"]):
            assert sc.same_bits(a, b), label
        assert nc.expected_status("thr-edge", "walk", thr[label]) == 0 and nc.expected_status("thr-edge", "tree", thr[label]) == 0
    assert thr["v+"] == np.nextafter(thr["v"], np.inf) and thr["w+"] == np.nextafter(thr["w"], np.inf) and thr["v"] != thr["w"]
    fj = nc.family_job("thr-edge", thr["v"])
    assert fj["lo"] == 0 and fj["values"].max() == thr["v"] and len(fj["windows"]) == 40
    x, y = fj["winner"]
    lay = sc.layout("seg")
    start = int(lay["kept_genomic"][1][x] - lay["goff"][1])
    rows = {label: sc.rows_of(want) for label, want in wants.items()}
    print("thr-edge", {label: (repr(t), len(rows[label])) for label, t in thr.items()}, "winner", (x, y))

    def has(label, chrom, value):
        return [r for r in rows[label] if r[0] == chrom and r[3] == value]

    (row,) = has("v", 2, thr["v"])
    assert row[1] == start
    # every pair bit-equal to v* is called at v*, the members a few ulps below are not, the fillers (21.7) are not
    assert len(has("v", 2, thr["v"])) == int(np.sum(fj["values"] == thr["v"])) == sum(r[0] == 2 for r in rows["v"])
    assert not has("v+", 2, thr["v"]) and not any(r[0] == 2 for r in rows["v+"])
    assert len(has("w", 1, -thr["w"])) == 1 and not has("w+", 1, -thr["w"])
    assert thr["w"] > thr["v"] and len(rows["w"]) == 1 and len(rows["w+"]) == 0


def test_float_cases():
    cases = nc.float_cases()
    ladder, masked, tie = cases["ulp-ladder"], cases["ulp-ladder-masked"], cases["sign-tie"]
    steps, spikes = nc.ladder_steps(), ladder["spikes"]
    assert sorted(steps) == list(range(38)) + [39, 39] and steps[20] == steps[31] == 39 and len(spikes) == nc.LADDER_K
    z = ladder["z"]
    assert z[0] == 1e12 and np.spacing(z[0]) > 1e-4 and nc.window_eps(z) > 0.07
    for thr in ladder["thresholds"]:
        tri, segs = nc.float_want("ulp-ladder", thr)
        n = len(z)
        single = np.zeros(len(tri), dtype=bool)
        single[[wo.tri_offset(n, s, s) for s in spikes]] = True
        rest = tri[~single & (tri < 1e6)]                        # (the windows that hold z[0] are 5e10 and more)
        assert np.max(np.abs(rest - 9.0)) > 1.0 and np.min(np.abs(rest - 9.0)) > 1.0
        assert int(np.sum(~single & (tri >= 1e6))) == n
        # every job's answer is its largest spike, the first of equals: the calls are the giant and every spike, exact
        assert [xy for _, xy in segs] == [(0, 0)] + [(s, s) for s in spikes]
        assert sc.same_bits([v for v, _ in segs[1:]], z[spikes])
        jobs = [j for j in nc.jobs_of(tri, n, thr) if j[4] is not None]
        lo, hi, sub, m, pos, _ = jobs[1]                          # the first job behind the giant holds the whole ladder
        assert (lo, hi) == (1, n) and wo.lin_to_2d(m, pos) == (spikes[20] - 1, spikes[20] - 1)
        assert int(np.sum(sub >= sub.max() - 2 * nc.window_eps(z))) == nc.LADDER_K          # all forty are candidates
        mtri, msegs = nc.float_want("ulp-ladder-masked", thr)
        gone = masked["masked"]
        assert spikes[20] in gone and spikes[31] in gone and len(gone) == 4
        assert all(mtri[wo.tri_offset(n, s, s)] == 0.0 for s in gone)
        assert [xy for _, xy in msegs] == [(0, 0)] + [(s, s) for s in spikes if s not in gone]
        mjobs = [j for j in nc.jobs_of(mtri, n, thr) if j[4] is not None]
        winner = wo.lin_to_2d(mjobs[1][3], mjobs[1][4])
        best_left = max((s for s in spikes if s not in gone), key=lambda s: z[s])
        assert winner == (best_left - 1, best_left - 1) and winner != (spikes[20] - 1, spikes[20] - 1)
        assert steps[spikes.index(best_left)] == 37
    v, up = tie["thresholds"]
    assert up == np.nextafter(v, np.inf)
    tri, segs = nc.float_want("sign-tie", v)
    assert tri.max() == v and tri.min() == -v                     # bit-equal in magnitude: the maximum is taken
    assert [(val, xy) for val, xy in segs] == [(9.0, (10, 10)), (-9.0, (50, 50))]
    jobs = [j for j in nc.jobs_of(tri, 64, v) if j[4] is not None]
    lo, hi, sub, m, pos, _ = jobs[1]                              # the right child: |minimum| one ulp above the maximum
    assert (lo, hi) == (11, 64) and sub.max() == np.nextafter(9.0, 0.0) and sub.min() == -9.0
    assert wo.lin_to_2d(m, pos) == (50 - 11, 50 - 11)
    assert nc.float_want("sign-tie", up)[1] == []


def test_wrong_implementations():
    """Three plausible but wrong candidate rules, and the cases whose expectations they miss (from the oracle's values
    and the three prefix orders alone):
    (a) the first candidate in row-major order: every case whose winner is not the first family member;
    (b) the candidate with the best prefix estimate: a case where ALL the prefix orders put another member on top;
    (c) eps without the sum |z| of the giant bin: in giant-first the estimates behind the giant move in steps of
        ulp(3.6e8) / sqrt(2) = 148 of that eps, and in every prefix order there are jobs whose numpy winner lies more
        than two of it below the best estimate and would not be listed at all."""
    first_wrong = [n for n in nc.COUNT_CASES if DESIGN[n][3] != 0]
    assert {"near-hi-40", "near-lo-40", "near-64", "near-long"} <= set(first_wrong)
    fooled = []
    for name in nc.COUNT_CASES:
        fj = nc.family_job(name)
        tops = {order: top_by_estimate(name, est) for order, est in family_estimates(name).items()}
        if all(top != fj["winner"] for top in tops.values()):
            fooled.append(name)
        print(name, "numpy's winner", fj["winner"], "top by estimate", tops)
    print("(a) fails:", first_wrong, "(b) fails in every prefix order:", fooled)
    assert fooled
    fj = nc.family_job("giant-first")
    z = fj["z"]
    small_eps = (2.0 * len(z) + 64.0) * 2.0 ** -53 * float(np.sum(np.abs(z)) - np.max(np.abs(z)))
    want = nc.oracle_of("giant-first")
    dropped = dict.fromkeys(ORDERS, 0)
    worst = dict.fromkeys(ORDERS, 0.0)
    n_jobs = 0
    prefixes = nc.prefix_orders(z)
    for lo, hi, sub, n, pos, _ in nc.jobs_of(want["tris"][1], len(z)):
        if pos is None or sub.max() < nc.THR:
            continue
        windows, values, _ = nc.family_of(sub, n, "hi", fj["eps"])
        if len(windows) < 2:
            continue
        n_jobs += 1
        at = windows.index(wo.lin_to_2d(n, int(sub.argmax())))
        for order in ORDERS:
            est = nc.estimates(prefixes[order], windows, lo)
            behind = float(est.max() - est[at]) / small_eps
            worst[order] = max(worst[order], behind)
            dropped[order] += behind > 2.0
    print("(c) giant-first: eps %.3g, without the giant %.3g; of %d jobs with a family, those whose numpy winner lies more than"
          " 2 small eps below the best estimate:" % (fj["eps"], small_eps, n_jobs), dropped,
          "the farthest, in the small eps:", {k: "%.3g" % v for k, v in worst.items()})
    assert fj["eps"] > 1e4 * small_eps and n_jobs >= 30
    assert min(dropped.values()) >= 1
