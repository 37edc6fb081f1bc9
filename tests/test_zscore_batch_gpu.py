"""The production z-score route of a batch -- wt.test_batch from 113 samples on, where the padded sample count reaches
128: k_pca_apply_t writes the repeats' arrays, the first repeat is k_zscore_tiled<12, 1, 25, true> with its lane
permutation, sample-major outputs and threshold-hit list, k_flag_hits sets the flags, k_zscore_pairs / k_flag_pairs
and the one-workgroup tail k_lat_repeats run the later repeats over sample-major outputs, k_sd_fast and k_inflate read
them -- against numpy's bits at EVERY number of kept references, list strides of every residue, and sample counts
with 0, 1 and 7 leftover tiles.  wt.repeatTest (every other bit-for-bit z-score test) never takes this route.

Inputs and the expectation: zscore_batch_cases.py (checked on the CPU by test_zscore_batch_cases_cpu.py).  The
reference is the numpy oracle alone (wo.to_numpy_ref_format, wo.apply_pca, wo.repeat_test), computed for the samples
zscore_batch_cases.checked() names; z and ratio are compared bit for bit (NaN equals NaN), the sd average bit for
bit, the zero patterns with np.array_equal.  No tolerance anywhere in this file.

What pins what (csrc/testpath.hip):
* the tail slots of k_zscore_tiled (`e < (n & 7)`, slots 8 ng ..): the quiet variant, where no wave leaves the kernel
  and every kept count 0 .. k, so every n & 7 at every ng, occurs -- test_every_kept_count_first_repeat;
* its `ng <= G` boundary (G = 12: 104 kept references and more take zscore_one): k = 104 and 128, kept counts 103
  against 104, quiet variant;
* the `src` lane permutation of z, ratio, kept count and sd: every sample-major k; a permuted kept count shows in
  test_zero_pattern_is_the_kept_count (the zeros are exactly n < minrefbins), a permuted sd in asdef;
* note_hit's `>=` and k_flag_hits' `>=` and sample-major z index: test_flags_at_the_thresholds_edge, and every
  later-repeat test (a pair missing from the hit list is a flag numpy sets and the batch does not);
* the sample-major index of zscore_pair8 and flag_wave (k_zscore_pairs / k_flag_pairs with osm, k_lat_repeats):
  test_later_repeats_launch_pairs and test_later_repeats_one_workgroup.
"""
import os
import re

import numpy as np
import pytest

import zscore_batch_cases as zc
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
SWEEP = int(os.environ.get("WC_SWEEP", "1"))      # WC_SWEEP=8: eight times the seeds of the first-repeat sweep


def bits_differ(a, b):
    """Where two float64 vectors differ in their bits (NaN equals NaN)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero(~((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


def make_reference(wt, c):
    return wt.Reference(c.idx, c.dst, c.sizes, c.sizes, np.ones(c.B, dtype=np.uint8), c.mean, c.comps, binsize=1e6,
                        cutoff=zc.CUTOFF)


def run_call(wt, reference, c, n_samples, thr, repeats, minrefbins=0, chromosomes=()):
    outs = wt.test_batch(reference, [zc.sample_dict(c, s) for s in range(n_samples)], thr, minrefbins=minrefbins,
                         repeats=repeats, chromosomes=list(chromosomes))
    assert len(outs) == n_samples
    return outs


def assert_call_matches(outs, c, thr, repeats, minrefbins, what, run=None):
    """Every checked sample of a call against the oracle.  run: the oracle ran `run` repeats and the call is held to
    its first `repeats` (repeat_test's result after `repeats` repeats is what its repeat number `repeats` returned)."""
    n_samples = len(outs)
    for s in zc.checked(n_samples):
        _, passes = zc.expect(c.k, c.variant, c.seed, s, thr, run or repeats)
        want = passes[repeats - 1]
        wz, wr, wsd = zc.results_of(want, minrefbins)
        gz, gr = np.concatenate(outs[s]["results_z"]), np.concatenate(outs[s]["results_r"])
        where = (what, "samples %d" % n_samples, "sample %d" % s)
        for name, g, w in (("z", gz, wz), ("ratio", gr, wr)):
            bad = bits_differ(g, w)
            assert len(bad) == 0, (where, name, "first differing bins", bad[:8], "got", g[bad[:8]], "want", w[bad[:8]],
                                   "kept references of those bins after each repeat", [p[2][bad[:8]] for p in passes[:repeats]],
                                   "below the cutoff", c.cnt[bad[:8]])
            assert np.array_equal(g == 0, w == 0), (where, name, "zero pattern")
        assert len(bits_differ([outs[s]["asdef"]], [wsd])) == 0, (where, "sd average", outs[s]["asdef"], wsd)
        assert len(outs[s]["results_calls"]) == 0 or what[0] == "tail"


def assert_same_calls(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        for key in ("results_z", "results_r"):
            assert len(bits_differ(np.concatenate(x[key]), np.concatenate(y[key]))) == 0, (what, s, key)
        assert len(bits_differ(x["results_cwz"], y["results_cwz"])) == 0, (what, s)
        assert len(bits_differ(np.asarray(x["results_calls"]).reshape(-1), np.asarray(y["results_calls"]).reshape(-1))) == 0, (what, s)
        assert len(bits_differ([x["asdef"]], [y["asdef"]])) == 0, (what, s)


# ------------------------------------------------------------------ a. every kept count, first repeat ----
def first_repeat_calls(wt, c, what, sizes=zc.CALL_SIZES):
    reference = make_reference(wt, c)
    try:
        for n_samples in sizes:
            outs = run_call(wt, reference, c, n_samples, np.inf, 1)
            assert_call_matches(outs, c, np.inf, 1, 0, what)
    finally:
        reference.close()


@pytest.mark.parametrize("variant", ["quiet", "special"])
@pytest.mark.parametrize("k,seed", [(k, s) for k in zc.ALL_K for s in range(SWEEP)])
def test_every_kept_count_first_repeat(wt, k, seed, variant):
    """Lists of every length 0 .. k in one call of 113 (padded to 128 with copies of sample 0), 128, 144 (one leftover
    tile, dealt to all XCDs) and 232 (seven leftover tiles) samples.  k = 100, 96, 64, 52, 12, 8, 4: the sample-major
    form (k = 4: the 128-slot list reads of the last bins reach furthest into the padding behind the lists);
    k = 99, 97, 10, 7, 1: zscore_one with sample-major outputs; k = 101, 103, 104, 128: bin-major outputs and the
    transposes, 26 list groups, kept counts 103 and 104 on either side of the slot limit.  B % 4 is 3 or 1."""
    c = zc.case(k, variant, seed)
    if variant == "quiet":
        for s in zc.checked(zc.N_SAMPLES):
            assert np.array_equal(zc.expect(k, variant, seed, s, np.inf, 1)[0][2], c.cnt)
        assert set(int(v) for v in c.cnt) == set(range(k + 1))
    first_repeat_calls(wt, c, ("first repeat", k, variant, seed))


@pytest.mark.parametrize("k", [100, 99, 104])
def test_zero_pattern_is_the_kept_count(wt, k):
    """minrefbins 1, 8 and k at one k of each family, special variant (the kept count differs between the samples of a
    tile): results_z and results_r are zero exactly where the oracle's kept count is below minrefbins -- the only
    view of the kept counts behind the tiled kernel's lane permutation."""
    c = zc.case(k, "special")
    reference = make_reference(wt, c)
    try:
        for minrefbins in (1, 8, k):
            for n_samples in (113, 144):
                outs = run_call(wt, reference, c, n_samples, np.inf, 1, minrefbins=minrefbins)
                assert_call_matches(outs, c, np.inf, 1, minrefbins, ("minrefbins", k, minrefbins))
                for s in zc.checked(n_samples):
                    wn = zc.expect(k, "special", 0, s, np.inf, 1)[0][2]
                    gz, gr = np.concatenate(outs[s]["results_z"]), np.concatenate(outs[s]["results_r"])
                    assert np.array_equal((gz == 0) & (gr == 0), wn < minrefbins), (k, minrefbins, n_samples, s)
    finally:
        reference.close()


# ------------------------------------------------------------------ b. the other forms, same expectation ----
@pytest.mark.parametrize("variant", ["quiet", "special"])
@pytest.mark.parametrize("switch,k", [("WC_ZSCORE_SM", 100), ("WC_ZSCORE_TILED", 100), ("WC_ZSCORE_TILED", 10)])
def test_other_forms_give_the_same_bits(wt, monkeypatch, switch, k, variant):
    """WC_ZSCORE_SM=0 (the tiled kernel with bin-major outputs and the transposes) and WC_ZSCORE_TILED=0 (k_zscore, a
    wave per bin) against the expectation test_every_kept_count_first_repeat holds the production form to."""
    monkeypatch.setenv(switch, "0")
    first_repeat_calls(wt, zc.case(k, variant), (switch + "=0", k, variant))


# ------------------------------------------------------------------ c. later repeats, sample-major outputs ----
@pytest.mark.parametrize("k", zc.K_LATE)
def test_later_repeats_launch_pairs(wt, k):
    """Special variant, a low threshold, no chromosome selected: the first repeat's hit list goes through k_flag_hits,
    every later repeat is k_zscore_pairs + k_flag_pairs over sample-major outputs with thousands of pairs (the oracle's
    counts: test_zscore_batch_cases_cpu.py).  2 and 5 repeats, 128 and 144 samples."""
    c = zc.case(k, "special")
    reference = make_reference(wt, c)
    try:
        for n_samples in (128, 144):
            for repeats in (2, zc.LATE_REPEATS):
                outs = run_call(wt, reference, c, n_samples, zc.LOW_THR, repeats)
                assert_call_matches(outs, c, zc.LOW_THR, repeats, 0, ("launch pairs", k, repeats), run=zc.LATE_REPEATS)
    finally:
        reference.close()


def assert_tail_outputs(outs, c, thr, what):
    """The selected chromosome's whole-region value against the oracle's fillTri of the same sample."""
    lo, hi = int(c.sums[zc.TAIL_CHROM - 1] - c.sizes[zc.TAIL_CHROM - 1]), int(c.sums[zc.TAIL_CHROM - 1])
    for s in zc.checked(len(outs)):
        (z, _, _, _), _ = zc.expect(c.k, c.variant, c.seed, s, thr, zc.LATE_REPEATS)
        tri = wo.fill_tri(z[lo:hi])
        assert len(bits_differ(outs[s]["results_cwz"], [tri[hi - lo - 1]])) == 0, (what, s)


@pytest.mark.parametrize("k", zc.K_LATE)
def test_later_repeats_one_workgroup(wt, monkeypatch, capfd, k):
    """`quiet22` with chromosome 22 selected (all of its z-scores finite): repeats 3 .. run as ONE workgroup
    (k_lat_repeats with sample-major outputs).  Repeats 3 and 4 have pairs queued and the form does not overflow;
    the same call with a launch pair per late repeat (WC_TEST_TAIL_REPEATS=0) and with the forced overflow
    (WC_TEST_TAIL_CAP=0: the batch is repeated) -- all three against the oracle, and against each other in every
    sample."""
    seed, thr = zc.TAIL_SEED[k], zc.TAIL_THR[k]
    c = zc.case(k, "quiet22", seed)
    what = ("tail", k)
    reference = make_reference(wt, c)
    try:
        for n_samples in (128, 144):
            outs = run_call(wt, reference, c, n_samples, thr, 2, chromosomes=[zc.TAIL_CHROM])
            assert_call_matches(outs, c, thr, 2, 0, what, run=zc.LATE_REPEATS)
            monkeypatch.setenv("WC_TEST_VERBOSE", "1")
            capfd.readouterr()
            got = run_call(wt, reference, c, n_samples, thr, zc.LATE_REPEATS, chromosomes=[zc.TAIL_CHROM])
            err = capfd.readouterr().err
            queued = [int(v) for v in re.findall(r"pairs queued per repeat:((?: \d+)+)", err)[-1].split()]
            assert queued[2] > 0 and queued[3] > 0, queued          # repeats 3 and 4 had work
            assert max(queued[2:zc.LATE_REPEATS]) <= zc.TAIL_PAIR_CAP, queued
            assert "batch repeated with a launch pair" not in err
            monkeypatch.setenv("WC_TEST_TAIL_REPEATS", "0")
            pairs = run_call(wt, reference, c, n_samples, thr, zc.LATE_REPEATS, chromosomes=[zc.TAIL_CHROM])
            monkeypatch.delenv("WC_TEST_TAIL_REPEATS")
            monkeypatch.setenv("WC_TEST_TAIL_CAP", "0")
            capfd.readouterr()
            again = run_call(wt, reference, c, n_samples, thr, zc.LATE_REPEATS, chromosomes=[zc.TAIL_CHROM])
            assert "batch repeated with a launch pair" in capfd.readouterr().err
            monkeypatch.delenv("WC_TEST_TAIL_CAP")
            monkeypatch.delenv("WC_TEST_VERBOSE")
            for name, call in (("one workgroup", got), ("launch pairs", pairs), ("forced overflow", again)):
                assert_call_matches(call, c, thr, zc.LATE_REPEATS, 0, what + (name,))
                assert_tail_outputs(call, c, thr, what + (name,))
            assert_same_calls(got, pairs, what + ("one workgroup against launch pairs",))
            assert_same_calls(got, again, what + ("one workgroup against forced overflow",))
    finally:
        reference.close()


# ------------------------------------------------------------------ d. flags at the threshold's edge ----
@pytest.mark.parametrize("k", [100, 99, 104])
def test_flags_at_the_thresholds_edge(wt, k):
    """The threshold IS abs(z) of a finite first-repeat z-score of the oracle (sample 130: a leftover tile of the call
    of 144; sample 0 in the call of 128, which the padding copies): numpy's `>=` flags that bin, and the second
    repeat shows it in the bins that keep it (the CPU test holds that the next larger threshold gives other bits).
    k = 100: note_hit and k_flag_hits; k = 99: note_hit behind zscore_one; k = 104: k_flag."""
    c = zc.case(k, "special")
    reference = make_reference(wt, c)
    try:
        for n_samples, s in zc.EDGE_CALLS:
            thr, _ = zc.edge_case(k, "special", 0, s)
            outs = run_call(wt, reference, c, n_samples, thr, 2)
            assert_call_matches(outs, c, thr, 2, 0, ("edge", k, thr))
    finally:
        reference.close()
