"""call_cases.py against the oracle, on the CPU: every `short` case gives exactly its planted spans in wo.test_sample
and call_rows_want restates test_sample's rows bit for bit; median_class on hand-written multisets; every planted
span of every layout has the class its maker declares and no reference list points into it."""
import time

import numpy as np
import pytest

import call_cases as cc
from oracle import wc_oracle as wo

SHORT = [c["name"] for c in cc.CASES if c["layout"] == "short"]
NEG0 = -0.0


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


def test_layouts():
    for name in ("short", "mid", "long"):
        lay = cc.layout(name)
        assert int(lay["msizes"][0]) == cc.N1[name] and int(lay["mask"].sum()) == lay["n_bins"]
        assert lay["idx"].shape == (lay["n_bins"], cc.K) and 30 <= cc.K <= 60
        assert int((~lay["mask"]).sum()) >= 3 and int((~lay["keep"]).sum()) >= 2
        for c in range(22):                              # the lists: other chromosomes only, never a spans' chromosome
            lo, hi = lay["moff"][c], lay["moff"][c + 1]
            bins = lay["refs_of"][c]
            assert np.all((bins < lo) | (bins >= hi)) and len(set(bins.tolist())) == cc.K
            assert np.all(bins >= lay["moff"][cc.POOL[0]])
    assert int(cc.layout("short")["n_bins"]) == 150 + 21 * 40 and int((~cc.layout("short")["keep"][:150]).sum()) == 1
    assert cc.POOL_COUNTS.mean() == cc.BACKGROUND


@pytest.mark.parametrize("name", SHORT)
def test_short_cases_against_the_oracle(name):
    """The oracle's calls are the planted spans (outside the chromosome without finite ratios), and call_rows_want
    gives the oracle's rows: chromosome, start, end, value and effect by bits."""
    case = cc.CASES[cc.CASE_NAMES.index(name)]
    smp = cc.case_sample(name)
    want = cc.oracle_of(name)
    calls = np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5)
    finite = calls[~np.isin(calls[:, 0], case["nonfinite"])]
    rows, _, _ = cc.want_of(name)
    assert len(finite) == len(smp["finite"]), (finite[:, :3], smp["finite"])
    assert same_bits(rows, finite), (rows, finite)
    if case["nonfinite"]:
        other = calls[np.isin(calls[:, 0], case["nonfinite"])]
        assert len(other) >= 1 and not np.any(np.isfinite(other[:, 4]))
        assert np.any(np.isnan(other[:, 4])) == (name == "short-nan")


def test_short_cases_see_both_signs_of_zero_and_the_order_case():
    cls = cc.span_class("short-mixed-64", (1, 13, 76))
    assert cls.name == "even_run_ends_at_k" and cls.neg and cls.zero_pm
    _, clean_r, _ = cc.want_of("short-mixed-64")
    keys = np.sort(cc.ordered_keys(clean_r[13:77]))
    assert keys[31] == cc.ordered_keys([NEG0])[0] and keys[32] == cc.ordered_keys([0.0])[0]
    cls = cc.span_class("short-signed-small", (6, 20, 21))
    assert cls.name == "even_distinct" and cls.zero_pm and not cls.neg
    # a masked-out bin inside a call of two bins (genomic 4 and 6): end = position of survivor y - 1, plus one; and a
    # call that starts behind a bin dropped for its few references (kept bin 20 is masked bin 21, genomic 22)
    second = np.asarray(cc.oracle_of("short-plain-small")["results_calls"]).reshape(-1, 5)
    second = second[second[:, 0] == 2]
    assert second[:, 1:3].tolist() == [[4.0, 5.0], [22.0, 23.0]]
    # three calls in chromosome 1, the strongest one rightmost: the list order of a search differs from position order
    calls = np.asarray(cc.oracle_of("short-order")["results_calls"]).reshape(-1, 5)
    first = calls[calls[:, 0] == 1]
    assert len(first) == 3 and np.argmax(np.abs(first[:, 3])) == 2


def test_median_class_by_hand():
    mc = cc.median_class
    assert mc([3.0, 1.0, 2.0])[:1] == ("odd",) and mc([3.0, 1.0, 2.0]).distinct and mc([3.0, 1.0, 2.0]).run == 1
    assert mc([2.0, 2.0, 1.0, 2.0, 5.0]).run == 3 and cc.kind_of(mc([2.0, 2.0, 1.0, 2.0, 5.0]), 5) == "tied"
    assert mc([4.0, 1.0, 2.0, 3.0]).name == "even_distinct" and cc.kind_of(mc([4.0, 1.0, 2.0, 3.0]), 4) == "distinct"
    assert mc([1.0, 1.0, 2.0, 3.0]).name == "even_run_ends_at_k" and mc([1.0, 1.0, 2.0, 3.0]).run == 2
    assert mc([1.0, 2.0, 2.0, 3.0]).name == "even_tie" and mc([2.0, 2.0]).name == "even_tie"
    assert mc([1.0, 2.0, 3.0, 3.0]).name == "even_distinct" and cc.kind_of(mc([1.0, 2.0, 3.0, 3.0]), 4) == "other"
    assert mc([1.0, np.nan]).name == "has_nan" and mc([np.nan]).name == "has_nan"
    assert mc([-1.0, 2.0]).neg and not mc([1.0, 2.0]).neg and not mc([NEG0, 2.0]).neg
    assert mc([NEG0, 0.0]).zero_pm and not mc([0.0, 0.0]).zero_pm and not mc([NEG0, NEG0]).zero_pm
    assert mc([NEG0, 0.0]).name == "even_distinct"                   # the two zeros are different bit images ...
    assert mc([NEG0, NEG0, 0.0, 1.0]).name == "even_run_ends_at_k"   # ... and -0.0 sorts below +0.0
    assert mc([1.0, np.inf]).inf and mc([-np.inf, 1.0, 2.0]).inf and not mc([1.0, 2.0]).inf
    assert mc([-2.0, -3.0, -1.0, 4.0]).name == "even_distinct" and mc([-2.0, -2.0, -3.0, -1.0]).name == "even_tie"
    assert mc([7.0]).name == "odd" and cc.kind_of(mc([7.0]), 1) == "distinct"


DECLARED = {
    "distinct": lambda c, n: c.distinct and c.name == ("odd" if n % 2 else "even_distinct") and not c.neg,
    "tied": lambda c, n: cc.kind_of(c, n) == "tied" and (c.name in ("odd", "even_tie")) and (n < 3 or c.run >= 3),
    "run_ends": lambda c, n: c.name == "even_run_ends_at_k" and c.run >= 2,
    "equal": lambda c, n: c.run == n and c.name == ("odd" if n % 2 else "even_tie"),
    "zeros": lambda c, n: c.run == n,
    "loss": lambda c, n: c.distinct and c.neg and not c.zero_pm,
    "mixed": lambda c, n: c.zero_pm and (c.neg or n == 2) and
    c.name == ("even_distinct" if n == 2 else "even_run_ends_at_k" if n % 2 == 0 else "odd"),
}


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_planted_spans_have_their_declared_class(name):
    """The counts of a span, with the sign of pca_mean (0 under a negative mean is -0.0), are ordered like its ratios."""
    case = cc.CASES[cc.CASE_NAMES.index(name)]
    lay = cc.layout(case["layout"])
    for chrom, x, maker, n in case["spans"]:
        _, _, counts, signs = cc.span(chrom, x, maker, n)
        assert len(counts) == n
        values = np.asarray(counts, dtype=np.float64) * (1.0 if signs is None else np.asarray(signs, dtype=np.float64))
        cls = cc.median_class(values)
        assert DECLARED[maker](cls, n), (maker, n, cls)
        if maker != "zeros":                             # (the emptied reference bins of chromosome 9 are the exception)
            genomic = lay["kept_genomic"][chrom - 1][x:x + n]
            assert chrom - 1 not in cc.POOL and chrom - 1 != cc.DEAD_CHROM
            for bins in lay["refs_of"]:
                assert not np.any(np.isin(lay["masked_to_genomic"][bins], genomic))


def test_required_lengths_are_planted():
    """Every (length, kind) the GPU test asserts as seen on a route is planted on a layout that route runs."""
    routes = {"latency": ("short", "mid"), "walker": ("short", "long"), "host": ("short", "mid", "long")}
    for route, lays in routes.items():
        have = set()
        for case in cc.CASES:
            if case["layout"] in lays:
                for chrom, x, maker, n in case["spans"]:
                    _, _, counts, signs = cc.span(chrom, x, maker, n)
                    values = np.asarray(counts, dtype=np.float64) * (1.0 if signs is None else np.asarray(signs, float))
                    have.add((n, cc.kind_of(cc.median_class(values), n)))
        assert cc.required(route) <= have, (route, sorted(cc.required(route) - have))


def test_long_reference_is_quick():
    name = "long-tied-5121"
    t0 = time.time()
    rows, clean_r, clean_sums = cc.want_of(name)
    took = time.time() - t0
    print("call_rows_want of a long sample: %.2f s" % took)
    assert took < 10.0
    assert clean_sums[0] == 5400 - 41 and len(rows) == len(cc.case_sample(name)["finite"])
    assert cc.kind_of(cc.span_class(name, (1, 100, 5220)), 5121) == "tied"
    assert wo.get_optimal_cutoff(cc.layout("long")["dst"], 3)[0] < 1e3
