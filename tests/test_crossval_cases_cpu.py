"""The rules of wc_crossval_stats as crossval_restated.py states them, on the hand-written matrices of crossval_cases.py
with the answers written out by hand, and the designed cohort through the oracle: what test_crossval_stats_gpu.py and
test_crossval_gpu.py rely on."""
import numpy as np
import pytest

import crossval_cases as cc
import crossval_restated as cr


@pytest.mark.parametrize("case, want", [(cc.HAND_EDGES, cc.HAND_EDGES_WANT), (cc.HAND_NONFINITE, cc.HAND_NONFINITE_WANT)],
                         ids=["edges", "nonfinite"])
def test_restatement_on_hand_written_matrices(case, want):
    assert cr.same(cr.stats(**case), cc.hand_want(want)) is None


def test_slots_at_the_edges():
    assert cr.slot_of(0.25) == 66 and cr.slot_of(0.2499) == 65
    assert cr.slot_of(-16.0) == 1 and cr.slot_of(float(np.nextafter(-16.0, -17))) == 0
    assert cr.slot_of(16.0) == 129 and cr.slot_of(15.99) == 128
    assert cr.slot_of(float("nan")) == 129 and cr.slot_of(float("inf")) == 129 and cr.slot_of(float("-inf")) == 0
    assert cr.slot_of(0.0) == 65 and cr.slot_of(-0.0) == 65


def test_minus_zero_is_untested_and_nan_is_tested():
    got = cr.stats(**cc.hand([[-0.0, 0.0, cc.NAN, 1.0]], [4], [3.0], lengths=(1,)))
    assert got["bins_i"][:, 0].tolist() == [0, 0, 1, 1] and got["bins_i"][:, 1].tolist() == [0, 0, 1, 0]
    assert got["rec_i"][0].tolist() == [0, 0, 2, 1, 0, 0, 0, 1] and got["win_n"].tolist() == [[0]]
    assert got["rec_f"][0, 2:].tolist() == [1.0, 1.0]
    none = cr.stats(**cc.hand([[cc.INF, 0.0]], [2], [3.0], lengths=(1,)))
    assert np.isnan(none["rec_f"][0, 2:]).all() and none["win_i"].tolist() == [[0, 0, 0, 0]]


def test_length_one_windows_agree_with_the_bin_counts():
    """Values that are multiples of 1 / 64 make every prefix sum exact, so a window of one bin is that bin's z: win_i[0]'s
    hi / lo equal the over_hi / over_lo of the selected chromosomes' rows that are not skipped."""
    rng = np.random.RandomState(5)
    sizes, sel = [7, 0, 12, 5, 9], [1, 3, 5]
    Z = rng.randint(-400, 401, size=(6, sum(sizes))) / 64.0
    Z[rng.random_sample(Z.shape) < 0.2] = 0.0
    Z[2, 8] = cc.NAN                          # chromosome 3 of sample 2 is skipped
    case = cc.hand(Z, sizes, [3.0, 3.5, 2.0, 4.0, 3.0, 6.25], sel=sel, lengths=(1, 4))
    got = cr.stats(**case)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    hi = lo = windows = 0
    for i in range(6):
        for c in sel:
            row = Z[i, offs[c - 1]:offs[c]]
            if not np.isfinite(row).all():
                continue
            t = row[row != 0]
            hi, lo, windows = hi + int((t >= case["thr"][i]).sum()), lo + int((t <= -case["thr"][i]).sum()), windows + len(t)
    assert got["win_i"][0, 1:].tolist() == [windows, hi, lo] and hi > 0 and lo > 0
    assert got["rec_i"][2, 7] == 1 and got["rec_i"][:, 7].sum() == 1
    assert got["win_hist"].sum(axis=1).tolist() == got["win_i"][:, 1].tolist() == got["win_n"].sum(axis=0).tolist()


@pytest.mark.parametrize("change", [dict(lengths=[]), dict(lengths=list(range(1, 18))), dict(lengths=[0, 1]), dict(lengths=[2, 2]),
                                    dict(lengths=[3, 2]), dict(sel=[]), dict(sel=[0]), dict(sel=[3]), dict(sel=[1, 1]),
                                    dict(sizes=[2, -1, 4]), dict(sizes=[4, 4])])
def test_restatement_refuses_bad_arguments(change):
    case = dict(cc.HAND_NONFINITE)
    case.update(change)
    with pytest.raises(cr.Refused):
        cr.stats(**case)


@pytest.mark.parametrize("row", [(0, 0, 0, 0), (0, 3, 0, 0), (0, 1.5, 0, 0), (0, 1, -1, 0), (0, 1, 2, 1), (0, 1, 0, 3), (0, 2, 0, 2),
                                 (0, 1, 0.5, 1), (0, cc.NAN, 0, 0), (0, 1, 0, cc.INF)])
def test_restatement_refuses_a_call_row_outside_the_layout(row):
    with pytest.raises(cr.Refused):
        cr.stats(**cc.hand([[1.0, 2.0, 3.0, 4.0, 5.0]], [3, 2], [3.0], calls=[row + (6.0, 0.1)]))


# ------------------------------------------------------------------------------------------------ the cohort ----
def loo(i):
    return cc.oracle_held_out(i, tuple(cc.training_of(list(range(cc.N)), i)))


def test_the_planted_sample_is_called_on_its_span_and_nobody_else_is():
    lo, hi = cc.PLANTED_SPAN
    for i in range(cc.N):
        calls = np.asarray(loo(i)["results_calls"], dtype=np.float64).reshape(-1, 5)
        assert len(calls) == cc.LOO_CALLS[i], (i, calls)
        on_span = [c for c in calls if c[0] == cc.PLANTED_CHROM and c[1] <= hi and c[2] >= lo]
        if i == cc.PLANTED:
            assert len(on_span) == 1 and tuple(on_span[0][:3]) == (cc.PLANTED_CHROM, lo, hi) and on_span[0][3] > 0
        else:
            assert not on_span
        z = np.concatenate(loo(i)["results_z"])
        assert np.isfinite(z).all() and z.shape == (cc.N_TOTAL,)
        for c in calls:                                             # every call row lies inside the layout
            assert 0 <= c[1] <= c[2] < cc.SIZES[int(c[0]) - 1]


def test_the_once_bin_is_masked_in_one_fold_only_and_removed_in_the_others():
    once = int(cc.OFFS[cc.ONCE_CHROM - 1] + cc.ONCE_BIN)
    for i in range(cc.N):
        training = tuple(cc.training_of(list(range(cc.N)), i))
        assert bool(cc.oracle_reference(training)["mask"][once]) == (i != cc.ONCE_SAMPLE)
        assert np.concatenate(loo(i)["results_z"])[once] == 0.0
        if i != cc.ONCE_SAMPLE:                                     # it passes the mask and falls to minrefbins
            mask = cc.oracle_reference(training)["mask"]
            assert loo(i)["ref_sizes"][int(mask[:once].sum())] < cc.MINREF
    counts = cc.counts()
    assert (counts[:, once] > 0).tolist() == [i == cc.ONCE_SAMPLE for i in range(cc.N)]
    assert counts.shape == (cc.N, cc.N_TOTAL) and cc.N_TOTAL % 64 != 0 and min(cc.SIZES) >= 15 and max(cc.SIZES) <= 60
