"""The inputs of the sensitivity tests, held on the CPU: the oracle finds nothing in the two base samples and exactly the
designed call for every designed plan row, the restated score gives the designed record for each, and the restated
spike agrees with exact rational arithmetic on the rounding ties and at the saturation edge."""
import numpy as np
import pytest

import spike_cases as sc
import spike_restated as sr


def test_both_base_samples_are_clean():
    for base in (0, 1):
        assert len(sc.oracle_calls((base, 1, 0, 1, 0))) == 0, base


@pytest.mark.parametrize("row", sc.ROWS, ids=["%d-%d-%d-%d" % r[0] for r in sc.ROWS])
def test_designed_row_gives_the_designed_call_and_record(row):
    trial, want, record, _ = row
    calls = sc.oracle_calls((0,) + trial)
    if want is None:
        assert len(calls) == 0
    else:
        assert len(calls) == 1, calls
        chrom, start, end, z, _ = calls[0]
        assert (int(chrom), int(start), int(end)) == (trial[0],) + want
        assert (z > 0) == (trial[3] > 0) and z != 0
    rec_i, rec_f = sr.score_lists(sc.plan_of([trial]), [calls])
    assert tuple(rec_i[0, :4]) == (len(calls),) + record
    if want is None:
        assert tuple(rec_i[0, 4:]) == (-1, -1, -1, 0) and np.isnan(rec_f[0]).all()
    else:
        assert tuple(rec_i[0, 4:]) == (0,) + want + (0,)
        assert rec_f[0, 0] == calls[0][3] and rec_f[0, 1] == calls[0][4]


def test_listed_figures_of_the_first_rows():
    """z and effect of the issue's table, to the digits it gives."""
    for trial, z, effect in (((1, 20, 5, 2500000), 38.4, 3.33), ((1, 20, 5, -1000000), -12.1, -1.0)):
        call = sc.oracle_calls((0,) + trial)[0]
        assert abs(call[3] - z) < 0.05 and abs(call[4] - effect) < 0.005
    for trial, z in (((1, 10, 7, 2500000), 33.9), ((1, 20, 5, -700000), -7.9), ((1, 20, 1, 2500000), 18.7)):
        assert abs(sc.oracle_calls((0,) + trial)[0][3] - z) < 0.05


def test_control_trial_matches_nothing():
    calls = np.array([[1.0, 0.0, 0.0, 9.0, 1.0], [1.0, 0.0, 0.0, -9.0, -1.0]])
    rec_i, rec_f = sr.score_lists(np.array([[0, 1, 0, 1, 0]], dtype=np.int32), [calls])
    assert tuple(rec_i[0]) == (2, 0, 0, 0, -1, -1, -1, 0) and np.isnan(rec_f[0]).all()


@pytest.mark.parametrize("c, ppm, want", [(1, 500000, 2), (1, -500000, 1), (3, -500000, 2), (0, 2500000, 0), (7, -1000000, 0),
                                          (21262214, 100000000, 2147483614), (21474837, 100000000, sr.INT_MAX),
                                          (sr.INT_MAX, 1, sr.INT_MAX), (sr.INT_MAX, 0, sr.INT_MAX), (sr.INT_MAX, -1, 2147481500)])
def test_rounding_ties_and_the_saturation_edge(c, ppm, want):
    value, clipped = sr.spike_value(c, ppm)
    assert value == want == sr.spike_value_fraction(c, ppm)
    base = np.array([[c, 5]], dtype=np.int32)
    out, saturated = sr.spike(base, [2], np.array([[0, 1, 0, 1, ppm]], dtype=np.int32))
    assert out.tolist() == [[want if ppm else c, 5]]
    assert saturated == int(clipped and ppm != 0)
    assert clipped == ((c, ppm) in ((21474837, 100000000), (sr.INT_MAX, 1)))


def test_negative_counts_and_bins_outside_the_span_are_copied():
    rng = np.random.RandomState(5)
    base = rng.randint(-3, 1000, size=(2, 30)).astype(np.int32)
    plan = np.array([[1, 2, 3, 4, 2500000], [0, 1, 0, 10, -300000], [1, 3, 9, 1, 1], [0, 2, 0, 1, 0]], dtype=np.int32)
    out, saturated = sr.spike(base, [10, 10, 10], plan)
    assert saturated == 0
    for i, (b, chrom, first, bins, ppm) in enumerate(plan.tolist()):
        lo = 10 * (chrom - 1) + first
        for j in range(30):
            inside = lo <= j < lo + bins and ppm != 0
            assert out[i, j] == (sr.spike_value_fraction(int(base[b, j]), ppm) if inside and base[b, j] >= 0 else base[b, j])
