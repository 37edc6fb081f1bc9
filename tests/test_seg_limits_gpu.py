"""The segmentation at the capacities of its fixed-size kernels, by BITS against the oracle, on every route
(csrc/testpath.hip):

    latency / latency_eager   k_seg_tree (seg_tree_region): one sample per call, launched, captured, replayed
    latency_off               a lone sample on k_seg_walk + k_walk_rows
    walker / walker_no_hot    k_seg_walk + k_walk_rows, 34 places
    host / host_one_part / host_row_blocks   the host-driven rounds (WC_TEST_WALK=0; k_seg_job / k_seg_merge /
                              k_seg_decide, with WC_TEST_CELLS=0 k_seg_seed / k_seg_bound / k_seg_bcollect; k_seg_brute)
    direct                    wt.stouffer_segments on the oracle's cleaned z (the host-driven rounds without call rows)

The inputs (seg_cases.py, held to their design on the CPU by test_seg_cases_cpu.py) put a region exactly at and exactly
one past each capacity: 64 / 65 windows tied for an extreme (either side), 128 / 129 segments, a job stack of 64 / 65,
a non-finite region, and two regions of one sample that fail for different reasons.  Every output of every sample --
call rows, results_z, results_r, results_cwz -- is held against wo.test_sample; with WC_TEST_VERBOSE the routes say when
a walker handed a call back, and that must happen exactly where seg_cases.walk_model says, with exactly its status bits;
a call of quiet samples right after a give-up must show none.  test_hot_list: k_seg_walk's early-starter list with more
hot regions than it holds."""
import contextlib
import re

import numpy as np
import pytest

import seg_cases as sc
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
SWITCHES = ("WC_TEST_LATENCY_MODE", "WC_TEST_WALK", "WC_TEST_WALK_HOT", "WC_TEST_CELLS", "WC_CELL_PARTS", "WC_TEST_VERBOSE")
WALK_LINE = re.compile(r"repeated on the host-driven rounds \(walk status (\d+)")
LAT_LINE = re.compile(r"call repeated on the general path \(latency status: walk (\d+), tail (\d+), sd (\d+)\)")
TREE_ROUTES = ("latency", "latency_eager")
WALK_ROUTES = ("latency_off", "walker", "walker_no_hot")


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@contextlib.contextmanager
def references(wt):
    """layout name -> the open reference, opened when first asked for."""
    opened = {}

    def get(name):
        lay_name = sc.case_of(name)["layout"]
        if lay_name not in opened:
            lay = sc.layout_of(name)
            opened[lay_name] = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"],
                                            sc.case_sample(name)["pca_mean"], lay["pca_components"], binsize=sc.BINSIZE)
        return opened[lay_name]

    try:
        yield get
    finally:
        for reference in opened.values():
            reference.close()


def run(wt, get, names, capfd):
    """One wt.test_batch of the named samples; returns (outputs, stderr of the call)."""
    repeats = {sc.case_of(n)["repeats"] for n in names}
    assert len(repeats) == 1
    capfd.readouterr()
    outs = wt.test_batch(get(names[0]), [sc.case_sample(n)["counts"] for n in names], sc.THR, minrefbins=sc.MINREF,
                         repeats=repeats.pop())
    return outs, capfd.readouterr().err


def check(name, out, what):
    want = sc.oracle_of(name)
    got = sc.rows_of(out)
    assert sc.same_bits(got, sc.rows_of(want)), (what, name, "calls", got.shape, sc.rows_of(want).shape)
    assert sc.same_bits(np.concatenate(out["results_z"]), np.concatenate(want["results_z"])), (what, name, "z")
    assert sc.same_bits(np.concatenate(out["results_r"]), np.concatenate(want["results_r"])), (what, name, "r")
    assert sc.same_bits(out["results_cwz"], want["results_cwz"]), (what, name, "cwz")
    return len(got)


def check_lines(route, names, err, what):
    """The give-up lines of one call: there exactly when the model says so, with the model's status bits."""
    walk = [int(n) for n in WALK_LINE.findall(err)]
    lat = [tuple(int(v) for v in m) for m in LAT_LINE.findall(err)]
    status = sc.call_status(names)
    if route in TREE_ROUTES:
        tree = max(sc.expected_status(n, "tree") for n in names)
        assert len(lat) == tree, (what, lat, err)
        if tree:                                         # k_seg_tree's word, not the late repeats' or stdDevAvg's
            assert lat[0][0] != 0 and lat[0][1:] == (0, 0), (what, lat)
        assert walk == ([status] if status else []), (what, walk, status)       # (the general path then asks k_seg_walk)
    elif route in WALK_ROUTES:
        assert lat == [] and walk == ([status] if status else []), (what, walk, status, lat)
    else:
        assert lat == [] and walk == [], (what, walk, lat)
    return walk[0] if walk else 0


@pytest.mark.parametrize("route", list(sc.ROUTES))
def test_seg_limits(wt, monkeypatch, capfd, route):
    env, kind = sc.ROUTES[route]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("WC_TEST_VERBOSE", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    seen, gave_up, n_calls, n_rows = set(), [], 0, 0
    with references(wt) as get:
        if kind == "alone":
            for name in sc.LIMIT_CASES:
                for attempt in range(3):                 # launched, captured, replayed
                    outs, err = run(wt, get, [name], capfd)
                    n_rows += check(name, outs[0], (route, "attempt %d" % attempt))
                    status = check_lines(route, [name], err, (route, name, attempt))
                    n_calls += 1
                if status:
                    gave_up.append((name, status))
                    for filler in sc.FILLERS[sc.case_of(name)["layout"]]:      # nothing of the give-up is left behind
                        outs, err = run(wt, get, [filler], capfd)
                        check(filler, outs[0], (route, "after", name))
                        assert check_lines(route, [filler], err, (route, filler, "after", name)) == 0
                seen.add(sc.provides(name))
        elif kind == "batch":
            for label, names in sc.batch_calls():
                call = sc.places_of(names, sc.PLACES)
                outs, err = run(wt, get, call, capfd)
                for at, name in enumerate(call):
                    n_rows += check(name, outs[at], (route, label, "place %d" % at))
                status = check_lines(route, call, err, (route, label))
                n_calls += 1
                if status:
                    gave_up.append((label, status))
                if sc.call_status(call):
                    fillers = sc.places_of(sc.FILLERS[sc.case_of(names[0])["layout"]], sc.PLACES)
                    outs, err = run(wt, get, fillers, capfd)
                    for at, name in enumerate(fillers):
                        check(name, outs[at], (route, "after", label, "place %d" % at))
                    assert check_lines(route, fillers, err, (route, "after", label)) == 0
                seen |= {sc.provides(n) for n in names}
        else:
            for name in sc.LIMIT_CASES:
                want = sc.oracle_of(name)
                whole, segs = wt.stouffer_segments(want["regions"], sc.THR, sc.MIN_SEARCH)
                n_calls += 1
                for c, (z, tri, wsegs) in enumerate(zip(want["regions"], want["tris"], sc.segments_of(name))):
                    assert [xy for _, xy in segs[c]] == [xy for _, xy in wsegs], (name, c + 1)
                    assert sc.same_bits([v for v, _ in segs[c]], [v for v, _ in wsegs]), (name, c + 1)
                    assert sc.same_bits(whole[c], tri[wo.tri_offset(len(z), 0, len(z) - 1)]), (name, c + 1)
                    n_rows += len(wsegs)
                seen.add(sc.provides(name))
    print(route, "%d calls, %d call rows checked, gave up:" % (n_calls, n_rows), gave_up, "seen", sorted(seen))
    assert sc.REQUIRED[route] <= seen, sorted(sc.REQUIRED[route] - seen)
    if route in TREE_ROUTES + WALK_ROUTES:
        assert {s for _, s in gave_up} >= {2, 4, 8, 16, 20}


def test_hot_list(wt, monkeypatch, capfd):
    """k_seg_walk's early starters (WalkHot, filled by k_region_prefix; only where a region has more than 2 048 masked
    bins): 48 places x 22 regions with more hot regions than the list's 512 entries, the same call without the list, a
    call of 9 straight after, and 192 places (4 224 regions: the 4 096-entry list)."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("WC_TEST_VERBOSE", "1")
    call48, call192 = sc.places_of(sc.HOT, 48), sc.places_of(sc.HOT, 192)
    sure = {n: sc.hot_regions(n)[0] for n in sc.HOT}
    assert sum(sure[n] for n in call48) > sc.hot_list_capacity(48 * 22)
    n_rows = 0
    with references(wt) as get:
        for label, call, switch in (("48 places", call48, None), ("48 places, no list", call48, "0"),
                                    ("48 places again", call48, None), ("9 places", call48[:9], None),
                                    ("192 places", call192, None), ("9 places after 192", call48[:9], None)):
            if switch is None:
                monkeypatch.delenv("WC_TEST_WALK_HOT", raising=False)
            else:
                monkeypatch.setenv("WC_TEST_WALK_HOT", switch)
            outs, err = run(wt, get, call, capfd)
            for at, name in enumerate(call):
                n_rows += check(name, outs[at], (label, "place %d" % at))
            assert check_lines("walker", call, err, label) == 0
    print("hot list: hot regions per sample", sorted(sure.values()), "of 22; %d in 48 places, %d in 192; %d call rows checked"
          % (sum(sure[n] for n in call48), sum(sure[n] for n in call192), n_rows))
