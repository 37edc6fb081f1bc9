"""The window search where prefix sums cannot tell windows apart, by BITS against the oracle, on every route of
seg_cases.ROUTES (csrc/testpath.hip; the routes are described in test_seg_limits_gpu.py).

Every search kernel ranks windows by (P[y + 1] - P[x]) * rs[len], lists what lies within 2 window_eps of the approximate
extreme, re-scores the list in numpy's summation order (window_exact, window_exact_wave) and takes numpy's argmax /
argmin of it (better_max, better_min).  The inputs of seg_near_cases.py (held to their design on the CPU by
test_seg_near_cases_cpu.py) are families of 3 .. 65 windows that are equal in real arithmetic and differ in numpy's last
bits: only a list that holds the whole family, scored exactly and ranked by numpy's rule, gives the reference's calls.
One family is one past the record (near-65): there, and nowhere else in this module, a walker hands the call back, with
status exactly 4; the candidate path itself must decide everything else.  Two cases put one z of 3.6e8 into the
family's region; thr-edge runs at thresholds equal to and one float above a champion; the float-built cases go through
wt.stouffer_segments alone."""
import contextlib
import re

import numpy as np
import pytest

import seg_cases as sc
import seg_near_cases as nc
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
SWITCHES = ("WC_TEST_LATENCY_MODE", "WC_TEST_WALK", "WC_TEST_WALK_HOT", "WC_TEST_CELLS", "WC_CELL_PARTS", "WC_TEST_VERBOSE",
            "WC_MINEFFECT")
WALK_LINE = re.compile(r"repeated on the host-driven rounds \(walk status (\d+)")
LAT_LINE = re.compile(r"call repeated on the general path \(latency status: walk (\d+), tail (\d+), sd (\d+)\)")
TREE_ROUTES = ("latency", "latency_eager")
WALK_ROUTES = ("latency_off", "walker", "walker_no_hot")
ALONE = [r for r, (_, kind) in sc.ROUTES.items() if kind == "alone"]
BATCH = [r for r, (_, kind) in sc.ROUTES.items() if kind == "batch"]


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@contextlib.contextmanager
def reference(wt):
    """The open reference of the `seg` layout (one pca_mean for every sample of this module)."""
    lay = sc.layout("seg")
    ref = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], lay["pca_mean"],
                       lay["pca_components"], binsize=sc.BINSIZE)
    try:
        yield ref
    finally:
        ref.close()


def route_env(monkeypatch, route):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("WC_TEST_VERBOSE", "1")
    for name, value in sc.ROUTES[route][0].items():
        monkeypatch.setenv(name, value)


def run(wt, ref, names, capfd, thr=nc.THR):
    """One wt.test_batch of the named samples; returns (outputs, stderr of the call)."""
    capfd.readouterr()
    outs = wt.test_batch(ref, [nc.case_sample(n)["counts"] for n in names], thr, minrefbins=sc.MINREF, repeats=sc.REPEATS)
    return outs, capfd.readouterr().err


def check(name, out, what, thr=nc.THR):
    want = nc.oracle_of(name, thr)
    got = sc.rows_of(out)
    assert sc.same_bits(got, sc.rows_of(want)), (what, name, "calls", got.shape, sc.rows_of(want).shape)
    assert sc.same_bits(np.concatenate(out["results_z"]), np.concatenate(want["results_z"])), (what, name, "z")
    assert sc.same_bits(np.concatenate(out["results_r"]), np.concatenate(want["results_r"])), (what, name, "r")
    assert sc.same_bits(out["results_cwz"], want["results_cwz"]), (what, name, "cwz")
    return len(got)


def check_lines(route, names, err, what, thr=nc.THR):
    """The give-up lines of one call: there exactly when near_model says so, with its status bits."""
    walk = [int(n) for n in WALK_LINE.findall(err)]
    lat = [tuple(int(v) for v in m) for m in LAT_LINE.findall(err)]
    status = nc.call_status(names, thr)
    if route in TREE_ROUTES:
        tree = max(nc.expected_status(n, "tree", thr) for n in names)
        assert len(lat) == tree, (what, lat, err)
        if tree:                                         # k_seg_tree's word, not the late repeats' or stdDevAvg's
            assert lat[0][0] != 0 and lat[0][1:] == (0, 0), (what, lat)
        assert walk == ([status] if status else []), (what, walk, status)       # (the general path then asks k_seg_walk)
    elif route in WALK_ROUTES:
        assert lat == [] and walk == ([status] if status else []), (what, walk, status, lat)
    else:
        assert lat == [] and walk == [], (what, walk, lat)
    return walk[0] if walk else 0


def check_direct(wt, name, thr=nc.THR):
    """wt.stouffer_segments on the oracle's cleaned z against wo.segment_tri and the triangle."""
    want = nc.oracle_of(name, thr)
    whole, segs = wt.stouffer_segments(want["regions"], thr, sc.MIN_SEARCH)
    n_rows = 0
    for c, (z, tri, wsegs) in enumerate(zip(want["regions"], want["tris"], nc.segments_of(name, thr))):
        assert [xy for _, xy in segs[c]] == [xy for _, xy in wsegs], (name, thr, c + 1)
        assert sc.same_bits([v for v, _ in segs[c]], [v for v, _ in wsegs]), (name, thr, c + 1)
        assert sc.same_bits(whole[c], tri[wo.tri_offset(len(z), 0, len(z) - 1)]), (name, thr, c + 1)
        n_rows += len(wsegs)
    return n_rows


@pytest.mark.parametrize("route", ALONE)
def test_near_alone(wt, monkeypatch, capfd, route):
    """One sample per call, three attempts each (launched, captured, replayed)."""
    route_env(monkeypatch, route)
    gave_up, n_rows = [], 0
    with reference(wt) as ref:
        for name in nc.COUNT_CASES:
            for attempt in range(3):
                outs, err = run(wt, ref, [name], capfd)
                n_rows += check(name, outs[0], (route, "attempt %d" % attempt))
                status = check_lines(route, [name], err, (route, name, attempt))
            if status:
                gave_up.append((name, status))
                for filler in nc.FILLERS:                # nothing of the give-up is left behind
                    outs, err = run(wt, ref, [filler], capfd)
                    check(filler, outs[0], (route, "after", name))
                    assert check_lines(route, [filler], err, (route, filler, "after", name)) == 0
    print(route, "%d call rows checked, gave up:" % n_rows, gave_up)
    assert gave_up == [("near-65", 4)]


@pytest.mark.parametrize("route", BATCH)
def test_near_batch(wt, monkeypatch, capfd, route):
    """34 places: every case between the fillers, and every case that must not give up in one call."""
    route_env(monkeypatch, route)
    gave_up, n_rows = [], 0
    calls = [(name, [name] + nc.FILLERS) for name in nc.COUNT_CASES] + [("within", nc.WITHIN + nc.FILLERS)]
    with reference(wt) as ref:
        for label, names in calls:
            call = sc.places_of(names, sc.PLACES)
            outs, err = run(wt, ref, call, capfd)
            for at, name in enumerate(call):
                n_rows += check(name, outs[at], (route, label, "place %d" % at))
            status = check_lines(route, call, err, (route, label))
            if status:
                gave_up.append((label, status))
            if nc.call_status(call):
                fillers = sc.places_of(nc.FILLERS, sc.PLACES)
                outs, err = run(wt, ref, fillers, capfd)
                for at, name in enumerate(fillers):
                    check(name, outs[at], (route, "after", label, "place %d" % at))
                assert check_lines(route, fillers, err, (route, "after", label)) == 0
    print(route, "%d call rows checked, gave up:" % n_rows, gave_up)
    assert gave_up == ([("near-65", 4)] if route in WALK_ROUTES else [])


def test_near_direct(wt, monkeypatch):
    route_env(monkeypatch, "direct")
    n_rows = sum(check_direct(wt, name) for name in nc.COUNT_CASES)
    print("direct: %d segments checked" % n_rows)


@pytest.mark.parametrize("route", nc.THR_EDGE_ROUTES)
def test_thr_edge(wt, monkeypatch, capfd, route):
    """abs(champion) < threshold means no call: at a threshold EQUAL to the champion's numpy value the call is there
    (and so is every family member bit-equal to it, and none of those a few ulps below), one float higher it is not."""
    route_env(monkeypatch, route)
    kind = sc.ROUTES[route][1]
    rows = {}
    with reference(wt) as ref:
        for label, thr in nc.thresholds_of("thr-edge").items():
            if kind == "direct":
                rows[label] = check_direct(wt, "thr-edge", thr)
            elif kind == "alone":
                for attempt in range(3):
                    outs, err = run(wt, ref, ["thr-edge"], capfd, thr)
                    rows[label] = check("thr-edge", outs[0], (route, label, attempt), thr)
                    assert check_lines(route, ["thr-edge"], err, (route, label, attempt), thr) == 0
            else:
                call = sc.places_of(["thr-edge"] + nc.FILLERS, sc.PLACES)
                outs, err = run(wt, ref, call, capfd, thr)
                for at, name in enumerate(call):
                    n = check(name, outs[at], (route, label, "place %d" % at), thr)
                    if name == "thr-edge":
                        rows[label] = n
                assert check_lines(route, call, err, (route, label), thr) == 0
    print(route, "thr-edge rows per threshold:", rows)
    assert rows["v"] == rows["v+"] + 1 and rows["w"] == 1 and rows["w+"] == 0


FLOAT_ENVS = [{}, {"WC_TEST_CELLS": "0"}, {"WC_CELL_PARTS": "1"}]


@pytest.mark.parametrize("env", FLOAT_ENVS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_float_cases(wt, monkeypatch, env):
    """ulp-ladder (forty spikes one ulp apart behind a z of 1e12), its masked variant (counting kernel and
    WC_MINEFFECT=sorted) and sign-tie (at v and one float above), through wt.stouffer_segments."""
    n_runs = 0
    for name, case in nc.float_cases().items():
        for extra in ([{}, nc.SORTED_ENV] if case["mineffect"] else [{}]):
            for switch in SWITCHES:
                monkeypatch.delenv(switch, raising=False)
            for switch, value in {**env, **extra}.items():
                monkeypatch.setenv(switch, value)
            for thr in case["thresholds"]:
                tri, wsegs = nc.float_want(name, thr)
                z = np.array(case["z"])
                ratios = [np.array(case["r"])] if case["mineffect"] else None
                whole, segs = wt.stouffer_segments([z], thr, sc.MIN_SEARCH, ratios=ratios, mineffectsize=case["mineffect"])
                what = (name, thr, env, extra)
                assert [xy for _, xy in segs[0]] == [xy for _, xy in wsegs], what
                assert sc.same_bits([v for v, _ in segs[0]], [v for v, _ in wsegs]), what
                assert sc.same_bits(whole[0], tri[wo.tri_offset(len(z), 0, len(z) - 1)]), what
                n_runs += 1
    assert n_runs == 1 + 2 + 2


def test_run_to_run(wt, monkeypatch, capfd):
    """The walker batch of near-hi-40 + the giants + near-long three times: the same bits every time."""
    route_env(monkeypatch, "walker")
    call = sc.places_of(["near-hi-40", "giant-first", "giant-last", "near-long"], sc.PLACES)
    seen = []
    with reference(wt) as ref:
        for attempt in range(3):
            outs, err = run(wt, ref, call, capfd)
            for at, name in enumerate(call):
                check(name, outs[at], ("run %d" % attempt, "place %d" % at))
            assert check_lines("walker", call, err, ("run", attempt)) == 0
            seen.append(b"".join(np.ascontiguousarray(out[key], dtype=np.float64).tobytes() for out in outs
                                 for key in ("results_calls", "results_cwz"))
                        + b"".join(np.concatenate(out[key]).tobytes() for out in outs for key in ("results_z", "results_r")))
    assert seen[0] == seen[1] == seen[2]
