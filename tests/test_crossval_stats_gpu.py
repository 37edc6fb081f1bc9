"""wc_crossval_stats (csrc/crossval.hip) against crossval_restated.py, integers equal and doubles by bits: the hand-written
matrices of crossval_cases.py (held on the CPU by test_crossval_cases_cpu.py), every sample count around a wave, every
window regime of a chromosome, and every refusal with the outputs untouched."""
import numpy as np
import pytest

import crossval_cases as cc
import crossval_restated as cr

pytestmark = pytest.mark.gpu


def run(case):
    from wisecondor_amd import crossval
    return crossval.crossvalStats(case["Z"], case["sizes"], case["thr"], case["asdef"], case["calls"], case["n_calls"],
                                  chromosomes=case["sel"], windows=case["lengths"])


def agree(case):
    got, want = run(case), cr.stats(**case)
    assert cr.same(got, want) is None, cr.same(got, want)
    return got


@pytest.mark.parametrize("case, want", [(cc.HAND_EDGES, cc.HAND_EDGES_WANT), (cc.HAND_NONFINITE, cc.HAND_NONFINITE_WANT)],
                         ids=["edges", "nonfinite"])
def test_hand_written_matrices(case, want):
    """The second has a row skipped for a nonfinite value beside nothing, and a clean sample beside it."""
    got = run(case)
    assert cr.same(got, cc.hand_want(want)) is None, cr.same(got, cc.hand_want(want))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_sample_counts_around_a_wave(n):
    """65 samples x 5 selected chromosomes and 65 x 4 call rows are more than one workgroup of every kernel; the chromosome
    of 300 bins is more than one workgroup of bins and more windows than a workgroup has lanes."""
    got = agree(cc.random_case(n, n, [9, 0, 300, 13, 70, 5], max_calls=4, lengths=(1, 2, 7), sel=[6, 1, 3, 4, 5]))
    assert got["rec_i"][:, 7].sum() >= 1


def test_a_skipped_row_beside_a_clean_row_of_the_same_sample():
    Z = np.arange(1, 13, dtype=np.float64).reshape(1, 12) / 4
    Z[0, 5] = cc.INF
    got = agree(cc.hand(Z, [4, 4, 4], [2.0], lengths=(1, 2, 4)))
    assert got["rec_i"][0, 7] == 1 and got["win_n"].tolist() == [[8, 6, 2]] and got["win_i"][:, 0].tolist() == [2, 2, 2]


def test_every_window_regime_of_a_chromosome():
    """L = 3 against chromosomes with 0 tested bins, n = 2 < L, n = L (one window), n = L + 1 (two), and one of no bins."""
    Z = [[0.0, -0.0, 0.0, 0.0, 0.0, 0.0,
          1.5, 0.0, 0.0, -2.5, 0.0, 0.0,
          1.0, 0.0, 2.0, 0.0, 0.0, 3.0,
          0.5, 1.5, 0.0, 2.5, 3.5, 0.0]]
    got = agree(cc.hand(Z, [6, 6, 0, 6, 6], [2.0], lengths=(3,)))
    assert got["win_n"].tolist() == [[3]] and got["win_i"].tolist() == [[2, 3, 3, 0]] and got["rec_i"][0, 7] == 0
    assert got["win_hist"].sum() == 3


def test_sixteen_lengths():
    lengths = list(range(1, 16)) + [40]
    got = agree(cc.random_case(3, 4, [70, 17, 3], lengths=lengths, nonfinite=False))
    assert got["win_i"].shape == (16, 4) and got["win_hist"].shape == (16, 130) and got["win_i"][15, 1] > 0


def test_calls_at_a_chromosomes_first_and_last_bin():
    calls = [(0, 1, 0, 0, 7.0, 0.1), (0, 1, 4, 4, -7.0, -0.1), (0, 2, 0, 2, 8.0, 0.2), (1, 3, 0, 0, cc.NAN, 0.0), (1, 2, 2, 2, 6.0, 0.1)]
    got = agree(cc.hand(np.ones((2, 9)), [5, 3, 1], [3.0, 3.0], calls=calls, lengths=(1,)))
    assert got["bins_i"][:, 4].tolist() == [1, 0, 0, 0, 0, 1, 1, 2, 0] and got["bins_i"][:, 5].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert got["rec_i"][:, 1].tolist() == [3, 2] and got["rec_i"][:, 6].tolist() == [5, 2]


def test_every_call_row_used():
    case = cc.random_case(11, 5, [20, 9, 31], max_calls=7, full_calls=True)
    assert case["n_calls"].tolist() == [7] * 5
    agree(case)


def test_a_row_stride_beyond_the_bins():
    wide, tight = cc.random_case(12, 3, [20, 9, 31], stride=77), cc.random_case(12, 3, [20, 9, 31])
    assert wide["Z"].shape == (3, 77) and np.array_equal(wide["Z"][:, :60], tight["Z"], equal_nan=True)
    assert cr.same(agree(wide), run(tight)) is None


def test_the_same_bits_twice_and_after_a_larger_job():
    small = cc.random_case(13, 4, [20, 9, 31])
    first = run(small)
    assert cr.same(run(small), first) is None
    agree(cc.random_case(14, 40, [200, 90, 31, 64], lengths=(1, 2, 3, 50)))
    assert cr.same(run(small), first) is None
    assert cr.same(first, cr.stats(**small)) is None


# -------------------------------------------------------------------------------------------------- refusals ----
def raw(case, fill=-7):
    """wc_crossval_stats itself on outputs filled with `fill`: (return code, the outputs)."""
    from wisecondor_amd import _lib
    from wisecondor_amd.crossval import STATS_KEYS, _stats_args
    lib = _lib.load()
    sizes = np.ascontiguousarray(case["sizes"], dtype=np.int64)
    sel = np.ascontiguousarray(case["sel"], dtype=np.int32)
    lengths = np.ascontiguousarray(case["lengths"], dtype=np.int32)
    Z, calls = np.ascontiguousarray(case["Z"]), np.ascontiguousarray(case["calls"])
    n = Z.shape[0]
    shapes = _stats_args(n, np.abs(sizes), sel, lengths if len(lengths) else np.zeros(1, dtype=np.int32))
    out = {key: np.full(shape, fill, dtype=dtype) for key, (shape, dtype) in shapes.items()}
    rc = lib.wc_crossval_stats(_lib.context(0), _lib.ptr(Z), Z.shape[1], n, _lib.ptr(sizes), len(sizes), _lib.ptr(case["thr"]),
                               _lib.ptr(case["asdef"]), _lib.ptr(calls), _lib.ptr(case["n_calls"]), calls.shape[1], _lib.ptr(sel), len(sel),
                               _lib.ptr(lengths), len(lengths), *[_lib.ptr(out[key]) for key in STATS_KEYS])
    return rc, out


def refused(case):
    from wisecondor_amd import _lib
    rc, out = raw(case)
    assert rc == _lib.E_ARG, (rc, _lib.load().wc_last_error())
    for key, value in out.items():
        assert (value == -7).all(), key
    with pytest.raises(cr.Refused):
        cr.stats(**case)


@pytest.mark.parametrize("change", [dict(lengths=[]), dict(lengths=list(range(1, 18))), dict(lengths=[0, 1]), dict(lengths=[2, 2]),
                                    dict(lengths=[3, 2]), dict(sel=[]), dict(sel=[0]), dict(sel=[3]), dict(sel=[1, 1]),
                                    dict(sizes=[2, -1, 4]), dict(sizes=[4, 4])])
def test_bad_arguments_are_refused_with_the_outputs_untouched(change):
    case = dict(cc.HAND_NONFINITE)
    case.update(change)
    refused(case)


@pytest.mark.parametrize("row", [(0, 0, 0, 0), (0, 3, 0, 0), (0, 1.5, 0, 0), (0, 1, -1, 0), (0, 1, 2, 1), (0, 1, 0, 3), (0, 2, 0, 2),
                                 (0, 1, 0.5, 1), (0, cc.NAN, 0, 0), (0, 1, 0, cc.INF)])
def test_a_call_row_outside_the_layout_is_refused_with_the_outputs_untouched(row):
    from wisecondor_amd import _lib
    case = cc.hand([[1.0, 2.0, 3.0, 4.0, 5.0], [1.0, 2.0, 3.0, 4.0, 5.0]], [3, 2], [3.0, 3.0],
                   calls=[(0, 1, 0, 2, 6.0, 0.1), (1, 2, 1, 1, 6.0, 0.1), (1,) + row[1:] + (6.0, 0.1)])
    refused(case)
    assert b"call row 1 of sample 1" in _lib.load().wc_last_error()


def test_rows_behind_n_calls_are_not_judged():
    """The same bad row behind n_calls is never read; and the good job runs after a refusal."""
    case = cc.hand([[1.0, 2.0, 3.0, 4.0, 5.0]], [3, 2], [3.0], calls=[(0, 1, 0, 2, 6.0, 0.1), (0, 9, 0, 0, 6.0, 0.1)])
    refused(case)
    case["n_calls"][0] = 1
    rc, out = raw(case)
    assert rc == 0 and cr.same(out, cr.stats(**case)) is None


def test_null_pointers_and_counts_are_refused():
    from wisecondor_amd import _lib
    lib = _lib.load()
    case = cc.HAND_EDGES
    sizes, sel, lengths = (np.ascontiguousarray(case[k], dtype=t) for k, t in (("sizes", np.int64), ("sel", np.int32), ("lengths", np.int32)))
    outs = [np.zeros(64, dtype=np.int64) for _ in range(7)]
    args = [_lib.context(0), _lib.ptr(case["Z"]), case["Z"].shape[1], 1, _lib.ptr(sizes), 2, _lib.ptr(case["thr"]), _lib.ptr(case["asdef"]),
            _lib.ptr(case["calls"]), _lib.ptr(case["n_calls"]), 1, _lib.ptr(sel), 2, _lib.ptr(lengths), 2] + [_lib.ptr(o) for o in outs]
    for at, value in ((1, None), (6, None), (18, None), (3, 0), (2, 6), (10, 0), (5, 0), (5, 65)):
        bad = list(args)
        bad[at] = value
        assert lib.wc_crossval_stats(*bad) == _lib.E_ARG, at
