"""The call rows of wt.test_batch -- position order, genomic start / end, value, effect = np.median of the call's
ratios - 1 -- by BITS against numpy, on every route that computes them and at every length at which a route changes
its median algorithm (csrc/testpath.hip):

    latency   k_seg_tree's tail            counting median at every length (regions up to 2 048 bins)
    walker    k_walk_rows                  <= 64: a wave; <= 5 120: staged in LDS + block_select_pair; longer: global
    host      k_seg_gather + k_call_post   <= 1 024: counting median in LDS; longer: two block_select runs
              (WC_TEST_WALK=0, and with WC_TEST_CELLS=0 the row-block searches in front of it)

The inputs (call_cases.py, checked on the CPU by test_call_cases_cpu.py) plant spans whose length and whose multiset of
ratios the case chooses: middle pair tied, the lower run ending exactly at the middle rank, all distinct, all equal,
negative, -0.0 next to +0.0, +inf, NaN.  On `short` every output is held against the oracle's test_sample; on `mid` and
`long` the rows against call_cases.call_rows_want.  Each (route, layout) asserts that it has seen every (length, kind)
of call_cases.REQUIRED that lives on that layout."""
import collections

import numpy as np
import pytest

import call_cases as cc

pytestmark = pytest.mark.gpu
SWITCHES = ("WC_TEST_LATENCY_MODE", "WC_TEST_WALK", "WC_TEST_CELLS", "WC_TEST_VERBOSE")
# route -> (the row of REQUIRED it answers for, environment, samples per call)
ROUTES = {
    "latency": ("latency", {}, 1),
    "latency_eager": ("latency", {"WC_TEST_LATENCY_MODE": "2"}, 1),
    "latency_off": (None, {"WC_TEST_LATENCY_MODE": "0"}, 1),            # the general path for a lone sample
    "walker": ("walker", {"WC_TEST_VERBOSE": "1"}, 34),
    "host": ("host", {"WC_TEST_WALK": "0"}, 34),
    "host_row_blocks": ("host", {"WC_TEST_WALK": "0", "WC_TEST_CELLS": "0"}, 34),
}
PLAN = [(r, lay) for r in ("latency", "latency_eager", "latency_off") for lay in ("short", "mid")] + \
       [(r, lay) for r in ("walker", "host", "host_row_blocks") for lay in ("short", "mid", "long")]
GAVE_UP = "repeated on the host-driven rounds"


def home(length):
    """The layout that plants a required length."""
    return "short" if length <= 65 else "mid" if length in (1023, 1024, 1025, 1026, 2040) else "long"


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


def rows_of(out):
    return np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)


def assert_same_results(a, b, what):
    assert same_bits(np.concatenate(a["results_z"]), np.concatenate(b["results_z"])), (what, "z")
    assert same_bits(np.concatenate(a["results_r"]), np.concatenate(b["results_r"])), (what, "r")
    assert same_bits(a["results_cwz"], b["results_cwz"]), (what, "cwz")
    assert same_bits(rows_of(a), rows_of(b)), (what, rows_of(a), rows_of(b))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


def groups_of(layout_name):
    """The cases of a layout that can share a call: the same pca_mean (the signs of the loss spans) and repeat count."""
    by = collections.OrderedDict()
    for case in cc.CASES:
        if case["layout"] == layout_name:
            key = (cc.case_sample(case["name"])["pca_mean"].tobytes(), case["repeats"])
            by.setdefault(key, []).append(case["name"])
    return [(names, key[1]) for key, names in by.items()]


def open_reference(wt, layout_name, name):
    lay = cc.layout(layout_name)
    return wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], cc.case_sample(name)["pca_mean"],
                        lay["pca_components"], binsize=cc.BINSIZE)


def run(wt, reference, names, repeats):
    return wt.test_batch(reference, [cc.case_sample(n)["counts"] for n in names], cc.THR, minrefbins=cc.MINREF,
                         repeats=repeats)


ALONE = {}


def alone_outputs(wt, layout_name):
    """Every sample of a layout in a call of its own with no switch set, once per module: latency mode on `short` and
    `mid`, the general path (k_seg_walk + k_walk_rows) on `long`.  What every other route and place is compared with."""
    if layout_name not in ALONE:
        outs = {}
        for names, repeats in groups_of(layout_name):
            reference = open_reference(wt, layout_name, names[0])
            try:
                for name in names:
                    outs[name] = run(wt, reference, [name], repeats)[0]
            finally:
                reference.close()
        ALONE[layout_name] = outs
    return ALONE[layout_name]


def check_against_numpy(layout_name, name, out):
    """`short`: every output against the oracle's toolTest.  `mid` / `long`: the calls are the planted spans, and their
    rows are call_rows_want's.  Returns the (length, kind) of the calls that were checked."""
    smp = cc.case_sample(name)
    got = rows_of(out)
    if layout_name == "short":
        want = cc.oracle_of(name)
        assert same_bits(got, np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5)), (name, got)
        assert same_bits(np.concatenate(out["results_z"]), np.concatenate(want["results_z"])), name
        assert same_bits(np.concatenate(out["results_r"]), np.concatenate(want["results_r"])), name
        assert same_bits(out["results_cwz"], want["results_cwz"]), name
    else:
        rows, _, _ = cc.want_of(name)
        assert len(got) == len(smp["planted"]), (name, got[:, :3], smp["planted"])
        assert same_bits(got, rows), (name, got, rows)
    return {(y - x + 1, cc.kind_of(cc.span_class(name, (c, x, y)), y - x + 1)) for c, x, y in smp["finite"]}


def places_of(names, n_places):
    """The group's samples dealt round the places of a call: every sample is there, the first, the last and both sides
    of place 32 (the sample tile of the batch kernels) hold one."""
    return [names[i % len(names)] for i in range(max(n_places, len(names)))]


@pytest.mark.parametrize("route,layout_name", PLAN, ids=["%s-%s" % p for p in PLAN])
def test_call_rows(wt, monkeypatch, capfd, route, layout_name):
    answers_for, env, n_places = ROUTES[route]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    alone = alone_outputs(wt, layout_name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    seen, n_samples, n_rows = set(), 0, 0
    for names, repeats in groups_of(layout_name):
        finite = not any(cc.CASES[cc.CASE_NAMES.index(n)]["nonfinite"] for n in names)
        reference = open_reference(wt, layout_name, names[0])
        try:
            capfd.readouterr()
            if n_places == 1:
                # each sample alone three times (latency mode: launched, captured, replayed) with a call of eight
                # between them, and the calls of eight twice
                eights = [places_of(names[i:i + 8], 8) for i in range(0, len(names), 8)]
                first = [run(wt, reference, [n], repeats)[0] for n in names]
                first8 = [run(wt, reference, call, repeats) for call in eights]
                again = [[run(wt, reference, [n], repeats)[0] for n in names] for _ in range(2)]
                again8 = [run(wt, reference, call, repeats) for call in eights]
                for i, name in enumerate(names):
                    for other in again:
                        assert_same_results(first[i], other[i], (name, "run to run"))
                    assert_same_results(first[i], alone[name], (name, "against the call with no switch set"))
                for call, a, b in zip(eights, first8, again8):
                    for at, name in enumerate(call):
                        assert_same_results(a[at], b[at], (name, "place %d of 8, run to run" % at))
                        assert_same_results(a[at], alone[name], (name, "place %d of 8" % at))
                outs = dict(zip(names, first))
            else:
                call = places_of(names, n_places)
                a = run(wt, reference, call, repeats)
                run(wt, reference, call[:9], repeats)                   # a call of another shape in between
                b = run(wt, reference, call, repeats)
                for at, name in enumerate(call):
                    assert_same_results(a[at], b[at], (name, "place %d, run to run" % at))
                    assert_same_results(a[at], alone[name], (name, "place %d of %d against the sample alone" % (at, len(call))))
                outs = {name: a[at] for at, name in enumerate(call)}
            if route == "walker" and finite:                       # k_walk_rows wrote these rows, not a repeat of the batch
                assert GAVE_UP not in capfd.readouterr().err
        finally:
            reference.close()
        for name in names:
            seen |= check_against_numpy(layout_name, name, outs[name])
            n_samples += 1
            n_rows += len(rows_of(outs[name]))
    print(route, layout_name, "%d samples, %d calls checked, seen" % (n_samples, n_rows), sorted(seen))
    if answers_for:
        want = {(n, kind) for n, kind in cc.required(answers_for) if home(n) == layout_name}
        assert want <= seen, sorted(want - seen)


def test_every_required_length_has_a_home():
    for route, (answers_for, _, _) in ROUTES.items():
        if answers_for:
            for n, _ in cc.required(answers_for):
                assert (route, home(n)) in PLAN, (route, n)
