"""The one-launch prepare (k_prepare_fused, up to 128 samples) beside the two-launch one (k_col_centre + k_convert).

Every workgroup of the fused kernel derives the per-sample centre and mean absolute deviation itself from CENTRE_ROWS
strided rows before it converts its own rows; 129 samples and more keep the two launches.  Every case holds the whole
`newref` against the oracle bit for bit; the bounds cases hold the exported keys to `key <= d <= key + slack_i +
slack_j` with d the pair's float64 distance, and `get_bounds` to a numpy restatement of the centre rule and of the row
rule (restated_bounds below).  The state cases run several jobs in ONE context: the smallest norm of a clamped row
lives in one of two slots that the prepares use in turn, and a fused prepare must find its slot at +inf whatever ran
before it.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

CENTRE_ROWS = 32                    # FUSED_CENTRE_ROWS of csrc/newref.hip
CENTRE_PHASES = 4                   # FUSED_THREADS / 128
BINS = np.array([90, 110, 100], dtype=np.int64)
FUSED = [1, 7, 63, 64, 65, 100, 127, 128]
TWO_LAUNCH = [129, 600]
ORDERS = ["F", "C"]
K = 100
SPREAD = 0.03
# bin layouts: fewer bins than sampled centre rows; one fewer and one more than their number; a count that is a
# multiple of neither 8 nor 128
LAYOUTS = {"fewer": [5, 4, 6], "one_fewer": [10, 11, 10], "one_more": [11, 11, 11], "odd": [101, 77, 45]}
_data = {}


def data_of(n_samples, bins=BINS):
    key = (n_samples, tuple(int(b) for b in bins))
    if key not in _data:
        rng = np.random.RandomState(700 + n_samples + 7 * int(np.sum(bins)))
        _data[key] = 1.0 + SPREAD * rng.standard_normal((int(np.sum(bins)), n_samples))
    return _data[key].copy()


def laid_out(data, order):
    return np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def assert_oracle(data, bins, order, k=K):
    from wisecondor_amd import wisetools
    bins = np.asarray(bins, dtype=np.int64)
    lay = laid_out(data, order)
    sums = np.cumsum(bins)
    idx, dst = wisetools.getReference(lay, bins, sums, k)
    with np.errstate(all="ignore"):
        want_i, want_d = wo.get_reference(lay, bins, sums, k, 1, 1, fast=True)
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    return wisetools.newref_stats()


def centre_rows(n_bins):
    """Every fourth of the 128 strided rows the two-launch path takes; with fewer than 128 bins, CENTRE_ROWS evenly."""
    n = min(n_bins, CENTRE_ROWS)
    return np.arange(n) * ((128 // CENTRE_ROWS) * (n_bins // 128) if n_bins >= 128 else n_bins // n)


# ------------------------------------------------------------------ the rules, restated in numpy ----
def restated_centre(data):
    """Centre and mean absolute deviation per sample from the sampled rows: mean, 8 x MAD window, trimmed mean, all
    over finite values, in float32 as the kernel does it: CENTRE_PHASES row phases (sampled row q belongs to phase
    q % CENTRE_PHASES) summed in row order, then added in phase order.  float32 add, subtract and divide are correctly
    rounded on both sides, so this is the kernel's centre to the bit."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        v = data[centre_rows(data.shape[0])].astype(f32)
        fin = np.isfinite(v)
        S = v.shape[1]

        def mean_of(w, ok):
            part = [np.zeros(S, dtype=f32) for _ in range(CENTRE_PHASES)]
            cnt = [np.zeros(S, dtype=f32) for _ in range(CENTRE_PHASES)]
            for q in range(v.shape[0]):
                part[q % CENTRE_PHASES] = part[q % CENTRE_PHASES] + np.where(ok[q], w[q], f32(0))
                cnt[q % CENTRE_PHASES] = cnt[q % CENTRE_PHASES] + ok[q].astype(f32)
            a, b = np.zeros(S, dtype=f32), np.zeros(S, dtype=f32)
            for r in range(CENTRE_PHASES):
                a, b = a + part[r], b + cnt[r]
            return np.where(b > 0, a / np.where(b > 0, b, f32(1)), f32(0)).astype(f32)
        c0 = mean_of(v, fin)
        mad = mean_of(np.abs(v - c0), fin)
        c = mean_of(v, fin & (np.abs(v - c0) <= f32(8) * mad))
    return c.astype(np.float64), mad.astype(np.float64)


def round_f32(x, up):
    """float64 -> float32 rounded down (up=False) or up."""
    with np.errstate(all="ignore"):
        r = np.asarray(x, dtype=np.float64).astype(np.float32)
        if up:
            return np.where(r.astype(np.float64) < x, np.nextafter(r, np.float32(np.inf)), r)
        return np.where(r.astype(np.float64) > x, np.nextafter(r, np.float32(-np.inf)), r)


def restated_bounds(data):
    """(norm_lo, slack, clamped) per row as the row rule gives them from the restated centre: the float16 image
    scaled by the power of two that puts the mean MAD into [4, 8), clamped to +-65504, subnormals flushed; e2 the
    squared representation error, lo = |a|^2 - (e2 / tau + tau m)(1 + 1e-9) - beta m rounded down with m = max(|a|^2,
    |h|^2), slack = 2 (|a|^2 - lo)(1 + 1e-6) rounded up; a row with a clamped or non-finite value has infinite bounds."""
    S = data.shape[1]
    c, mad = restated_centre(data)
    with np.errstate(all="ignore"):
        good = np.isfinite(mad) & (mad > 0)
        gam = 1.0
        if good.any() and np.isfinite(mad[good].sum()):
            e = int(np.floor(np.log2(mad[good].sum() / good.sum())))
            gam = 2.0 ** (2 - min(max(e, -60), 60))
        a = (data - c).astype(np.float32).astype(np.float64)
        sd = a * gam
        clamped = (np.abs(sd) > 65504.0).any(axis=1)
        h = np.clip(sd, -65504.0, 65504.0).astype(np.float32).astype(np.float16).astype(np.float64)
        h = np.where(np.abs(h) < 6.103515625e-05, 0.0, h)
        back = h / gam
        acc, e2, hn = (a * a).sum(1), ((a - back) ** 2).sum(1), (back * back).sum(1)
        beta = float(np.float32(2.0 * (S + 16) * 2.0 ** -24 * 1.001))
        tau = 2.0 ** -12
        m = np.maximum(acc, hn)
        lo = round_f32(acc - (e2 / tau + tau * m) * (1.0 + 1e-9) - beta * m - 1e-37, up=False)
        hi = round_f32(2.0 * (acc - lo.astype(np.float64)) * (1.0 + 1e-6) + 1e-37, up=True)
        usable = np.isfinite(acc) & (acc < 1e37) & np.isfinite(e2) & np.isfinite(hn) & ~clamped
    inf = np.float32(np.inf)
    return np.where(usable, lo, inf), np.where(usable, hi, inf), clamped


# ------------------------------------------------------------------ device side ----
def stages_of(data, bins, order, k=K):
    import torch
    from wisecondor_amd import _lib, distributed
    X = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    return distributed.HipStages(_lib.context(0), X, np.asarray(bins, dtype=np.int64), k,
                                 _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)


def bounds_of(st):
    import torch
    B = st.n_bins
    lo = torch.zeros(B, dtype=torch.float32, device="cuda")
    slack = torch.zeros(B, dtype=torch.float32, device="cuda")
    st.get_bounds(0, B, lo, slack)
    torch.cuda.synchronize()
    return lo.cpu().numpy(), slack.cpu().numpy()


def check_keys(data, bins, order):
    """prepare -> thresholds -> collect -> export: every listed key is at or below the pair's float64 distance and
    key + slack_i + slack_j at or above it."""
    import torch
    st = stages_of(data, bins, order)
    B = st.n_bins
    st.prepare()
    st.thresholds(0, B)
    st.collect(0, B, 0, 1)
    cap = st.cap
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    lst = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
    st.export(0, B, cap, cnt, lst)
    _, slack = bounds_of(st)
    cnt = cnt.cpu().numpy()
    ent = lst.cpu().numpy().view(np.uint64)
    lay = laid_out(data, order)
    chrom = np.repeat(np.arange(len(bins)), bins)
    slack = slack.astype(np.float64)
    listed = 0
    for i in range(B):
        n = int(cnt[i])
        assert n <= cap, (i, n)
        e = ent[i, :n]
        j = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
        u = (e >> np.uint64(32)).astype(np.uint32)
        key = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
        assert (chrom[j] != chrom[i]).all(), i
        with np.errstate(all="ignore"):
            dist = np.sum(np.power(laid_out(lay[j, :], order) - lay[i, :], 2), 1)
        assert (key.astype(np.float64) <= dist).all(), (order, i)
        assert (key.astype(np.float64) + slack[i] + slack[j] >= dist).all(), (order, i)
        listed += n
    return listed


def assert_bounds_restated(data, bins, order, skip=()):
    """get_bounds of a prepared job against the restatement.  norm_lo to 1e-6 (float32 rounding of a value that the two
    sides sum in different orders); the slack to 1e-3: it is 2 (|a|^2 - lo), about 4e-4 |a|^2, and one float32 step of
    lo, 6e-8 |a|^2, is 1.5e-4 of it."""
    st = stages_of(data, bins, order)
    st.prepare()
    lo, slack = bounds_of(st)
    want_lo, want_slack, clamped = restated_bounds(data)
    keep = np.ones(len(lo), dtype=bool)
    keep[list(skip)] = False
    assert np.array_equal(np.isfinite(lo[keep]), np.isfinite(want_lo[keep]))
    assert np.array_equal(np.isfinite(slack[keep]), np.isfinite(want_slack[keep]))
    f = keep & np.isfinite(want_lo)
    assert np.allclose(lo[f], want_lo[f], rtol=1e-6, atol=0)
    assert np.allclose(slack[f], want_slack[f], rtol=1e-3, atol=0)
    return lo, slack, clamped


# ------------------------------------------------------------------ sample counts ----
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_samples", FUSED + TWO_LAUNCH)
def test_newref_matches_the_oracle(n_samples, order):
    stats = assert_oracle(data_of(n_samples), BINS, order)
    assert stats["fallback_rows"] == 0, stats


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_samples", FUSED + TWO_LAUNCH)
def test_keys_and_slacks_bound_the_distance(n_samples, order):
    assert check_keys(data_of(n_samples), BINS, order) > 0


@pytest.mark.parametrize("n_samples", FUSED)
def test_bounds_follow_the_restated_rules(n_samples):
    assert_bounds_restated(data_of(n_samples), BINS, "F")


# ------------------------------------------------------------------ bin counts ----
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bin_counts_around_the_centre_rows(layout, order):
    bins = np.array(LAYOUTS[layout], dtype=np.int64)
    data = data_of(100, bins)
    assert_oracle(data, bins, order)
    check_keys(data, bins, order)
    assert_bounds_restated(data, bins, order)


# ------------------------------------------------------------------ sampled rows that go wrong ----
def test_outlier_in_a_sampled_row_leaves_the_centre_at_the_bulk():
    """One value 1e6 spreads off in a sampled row: the 8 x MAD window drops it (one of 32 values sits at 31 c' from
    the mean where the window is 15.5 c' wide), the centre of that column stays within a spread of the bulk, and every
    other row's slack is what the clean matrix gives times the ratio of the two restatements."""
    clean = data_of(100)
    dirty = clean.copy()
    row = int(centre_rows(dirty.shape[0])[3])
    dirty[row, 5] += 1e6 * SPREAD
    c, _ = restated_centre(dirty)
    assert abs(c[5] - 1.0) < SPREAD
    _, slack_clean, _ = assert_bounds_restated(clean, BINS, "F")
    _, slack_dirty, _ = assert_bounds_restated(dirty, BINS, "F", skip=[row])
    _, want_clean, _ = restated_bounds(clean)
    _, want_dirty, _ = restated_bounds(dirty)
    others = np.arange(dirty.shape[0]) != row
    assert np.isfinite(slack_dirty[others]).all()
    ratio = want_dirty[others].astype(np.float64) / want_clean[others]
    assert (slack_dirty[others] <= slack_clean[others] * ratio * (1.0 + 2e-3)).all()
    for order in ORDERS:
        assert_oracle(dirty, BINS, order)
        check_keys(dirty, BINS, order)


@pytest.mark.parametrize("order", ORDERS)
def test_column_nan_in_every_sampled_row(order):
    data = data_of(100)
    data[centre_rows(data.shape[0]), 17] = np.nan
    c, mad = restated_centre(data)
    assert c[17] == 0.0 and mad[17] == 0.0
    assert_oracle(data, BINS, order)
    check_keys(data, BINS, order)


@pytest.mark.parametrize("order", ORDERS)
def test_constant_column(order):
    data = data_of(100)
    data[:, 40] = 1.25
    _, mad = restated_centre(data)
    assert mad[40] == 0.0
    stats = assert_oracle(data, BINS, order)
    assert stats["fallback_rows"] == 0, stats
    check_keys(data, BINS, order)
    assert_bounds_restated(data, BINS, order)


@pytest.mark.parametrize("order", ORDERS)
def test_clamped_rows_take_the_exact_path(order):
    """Rows with a value beyond the float16 range of the scaled image: infinite bounds, never listed, the exact path
    for exactly these rows.  (A SAMPLED row cannot clamp at up to 128 samples: its value v raises the column's MAD to
    at least v / 32 and the mean MAD to v / (32 S), the scale puts the mean MAD below 8, so v lands below 8 x 32 x 128 =
    32 768 < 65 504.  The wild sampled row of the test above is such a row; the rows planted here are not sampled.)"""
    data = data_of(100)
    sampled = set(int(r) for r in centre_rows(data.shape[0]))
    planted = [r for r in (50, 151, 290) if r not in sampled]
    assert len(planted) == 3
    for r in planted:
        data[r, 3] = 1.0 + 1e6 * SPREAD
    _, _, clamped = restated_bounds(data)
    assert sorted(np.nonzero(clamped)[0]) == planted
    stats = assert_oracle(data, BINS, order)
    assert stats["fallback_rows"] == len(planted), stats
    lo, slack, _ = assert_bounds_restated(data, BINS, order)
    assert np.isinf(lo[planted]).all() and np.isinf(slack[planted]).all()
    check_keys(data, BINS, order)


# ------------------------------------------------------------------ state carried between calls ----
def clamped_matrix(n_samples):
    data = data_of(n_samples)
    data[151, 0] = 1.0 + 1e6 * SPREAD
    return data


def test_clamped_then_clean_reports_no_fallback_rows():
    assert assert_oracle(clamped_matrix(100), BINS, "F")["fallback_rows"] == 1
    assert assert_oracle(data_of(100), BINS, "F")["fallback_rows"] == 0
    assert assert_oracle(clamped_matrix(64), BINS, "C")["fallback_rows"] == 1
    assert assert_oracle(data_of(64), BINS, "C")["fallback_rows"] == 0


def test_fused_two_launch_fused():
    assert assert_oracle(clamped_matrix(100), BINS, "F")["fallback_rows"] == 1
    assert assert_oracle(clamped_matrix(129), BINS, "F")["fallback_rows"] == 1
    assert assert_oracle(data_of(100), BINS, "F")["fallback_rows"] == 0
    assert assert_oracle(data_of(129), BINS, "F")["fallback_rows"] == 0
    assert assert_oracle(clamped_matrix(128), BINS, "F")["fallback_rows"] == 1
    assert assert_oracle(data_of(128), BINS, "F")["fallback_rows"] == 0


def run_staged(data, order, exact_first=False):
    import torch
    st = stages_of(data, BINS, order)
    B = st.n_bins
    idx = torch.zeros((B, K), dtype=torch.int32, device="cuda")
    dst = torch.zeros((B, K), dtype=torch.float64, device="cuda")
    st.prepare()
    if exact_first:
        st.exact(0, B, idx, dst)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()
    st.thresholds(0, B)
    st.collect(0, B, 0, 1)
    st.finish(0, B, idx, dst)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dst.cpu().numpy()


def oracle_of(data, order):
    lay = laid_out(data, order)
    with np.errstate(all="ignore"):
        return wo.get_reference(lay, BINS, np.cumsum(BINS), K, 1, 1, fast=True)


def test_prepare_exact_then_a_full_pass():
    from wisecondor_amd import wisetools
    data = clamped_matrix(100)
    want_i, want_d = oracle_of(data, "F")
    idx, dst = run_staged(data, "F", exact_first=True)
    assert np.array_equal(idx, want_i) and same_bits(dst, want_d)
    assert assert_oracle(data_of(100), BINS, "F")["fallback_rows"] == 0
    assert assert_oracle(data, BINS, "F")["fallback_rows"] == 1
    assert wisetools.newref_stats()["fast_rows"] == int(BINS.sum()) - 1


def test_staged_pass_between_two_full_passes():
    from wisecondor_amd import wisetools
    assert assert_oracle(clamped_matrix(100), BINS, "F")["fallback_rows"] == 1
    clean = data_of(100)
    want_i, want_d = oracle_of(clean, "F")
    idx, dst = run_staged(clean, "F")
    assert np.array_equal(idx, want_i) and same_bits(dst, want_d)
    assert wisetools.newref_stats()["fallback_rows"] == 0
    data = clamped_matrix(100)
    want_i, want_d = oracle_of(data, "F")
    idx, dst = run_staged(data, "F")
    assert np.array_equal(idx, want_i) and same_bits(dst, want_d)
    assert wisetools.newref_stats()["fallback_rows"] == 1
    assert assert_oracle(clean, BINS, "F")["fallback_rows"] == 0
