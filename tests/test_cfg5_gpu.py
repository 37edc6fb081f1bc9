"""BASELINE config 5 (batched `test`, 50 kb bins), one GPU's share: 125 samples.

* The real reference's fillTri + segmentTri on the three longest 50 kb chromosomes of sample 0
  (tests/golden/cfg5_50kb.npz; about 11 M windows each, minutes of np.sum per chromosome --
  tools/make_goldens.py --only cfg5): segment bounds exact, segment values, the whole-chromosome
  z and 400 random window values per chromosome bit-equal.
* The 125-sample batch (tools/cfg5_case.py): sample 0's cleaned z vectors reproduce the golden
  inputs, its calls on chromosomes 1-3 are the reference's segments mapped to genomic bins, the
  CPU oracle's repeat_test agrees bit for bit with three samples of the batch, and the oracle's
  own segmentation agrees on the short chromosomes (19-22) of those samples.
* WHOLE samples (tests/golden/cfg5_whole.npz, tools/make_cfg5_whole.py): samples 0 and 5 went
  through the real reference's toolTest end to end (all 22 chromosomes, 90 M windows each), ten
  samples through the CPU oracle's test_sample; every call of the batch is compared with them.
  No member of either fixture was computed by the HIP `test` path.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@pytest.fixture(scope="module")
def g(golden):
    return golden("cfg5_50kb.npz")


@pytest.fixture(scope="module")
def gw(golden):
    return golden("cfg5_whole.npz")


@pytest.fixture(scope="module")
def case(wt):
    import cfg5_case
    from wisecondor_amd import synth
    c = cfg5_case.build(wt, synth)
    yield c
    c["reference"].close()


def test_segments_of_the_longest_50kb_chromosomes(wt, g):
    thr = float(g["threshold"])
    zs = [g["z_chr%d" % c] for c in (1, 2, 3)]
    assert [len(z) for z in zs] == [4722, 4609, 3747]
    whole, segs = wt.stouffer_segments(zs, thr, 3)
    for j, c in enumerate((1, 2, 3)):
        want = g["seg_chr%d" % c]
        got = np.array([[v, x, y] for v, (x, y) in segs[j]], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(got[:, 1:], want[:, 1:]), (c, got, want)
        assert same_bits(got[:, 0], want[:, 0]), c
        assert same_bits([whole[j]], [g["whole_chr%d" % c]]), c
    assert len(g["seg_chr1"]) >= 1 and len(g["seg_chr2"]) >= 1          # the planted gain / loss are there


def test_window_values_of_the_triangle(wt, g):
    """fillTri's values (wisetools.py:471) at 400 random windows per chromosome: getValue of the mirror."""
    from wisecondor_amd.triarray import TriArr
    for c in (1, 3):
        tri = TriArr.from_region(g["z_chr%d" % c])
        xs, ys, vs = g["tri_x_chr%d" % c], g["tri_y_chr%d" % c], g["tri_v_chr%d" % c]
        # one batched call: every window as its own region
        regions = [g["z_chr%d" % c][int(x):int(y) + 1] for x, y in zip(xs, ys)]
        whole, _ = wt.stouffer_segments(regions, np.inf, 3)
        assert same_bits(whole, vs), c
        assert same_bits([tri.getValue(int(xs[0]), int(ys[0]))], [vs[0]])


def test_batch_of_125_samples(wt, g, case):
    import cfg5_case
    thr = case["threshold"]
    assert thr == float(g["threshold"])
    assert np.array_equal(case["masked_bins"], g["masked_bins"])
    outs = wt.test_batch(case["reference"], case["tests"], thr)
    assert len(outs) == 125
    # sample 0: the pipeline of this build reproduces the golden's input vectors, and its calls on
    # chromosomes 1-3 are the reference's segments in genomic coordinates.  The stored z vectors were
    # made with the prep (exact PCA) of the build that wrote the fixture; the PCA is pinned to 1e-9 / 1e-10
    # (tests/test_prep_gpu.py), not to bits, so a different summation order in the prep moves these z
    # values in their last digits: they are compared to 1e-6, the coordinates exactly.  (Bits of the
    # segmentation itself: test_segments_of_the_longest_50kb_chromosomes runs on the STORED vectors.)
    zs, rs, xpca, (z, r, n, sd) = cfg5_case.cleaned_regions(wt, case, 0)
    for c in (1, 2, 3):
        assert zs[c - 1].shape == g["z_chr%d" % c].shape, c
        assert np.allclose(zs[c - 1], g["z_chr%d" % c], rtol=0, atol=1e-6, equal_nan=True), c
    calls0 = np.asarray(outs[0]["results_calls"], dtype=np.float64).reshape(-1, 5)
    for c in (1, 2, 3):
        mine = calls0[calls0[:, 0] == c]
        want = g["seg_chr%d" % c]
        assert len(mine) == len(want), c
        assert np.allclose(mine[:, 3], want[:, 0], rtol=1e-6, atol=0), c    # the call's z is the segment's value
        for row, (v, x, y) in zip(mine, want):                          # effect = median(ratio[x..y]) - 1
            assert row[4] == np.median(rs[c - 1][int(x):int(y) + 1]) - 1, c
    planted = [row for row in calls0 if row[0] in (1.0, 2.0) and row[2] - row[1] > 300]
    assert len(planted) >= 2
    # three samples' z-scores against the CPU oracle's repeat_test, all bins: cleaned_regions runs wt.repeatTest on ONE
    # sample, the lone-sample route (k_zscore_pairs, bin-major outputs), not the batch's -- the batch route
    # (k_zscore_tiled with sample-major outputs and what follows it) is held to numpy's bits by test_zscore_batch_gpu.py
    ref = case["reference"]
    ms = [int(v) for v in case["masked_bins"]]
    msum = [int(v) for v in np.cumsum(ms)]
    for i in (0, 5, 124):
        zs_i, rs_i, xp, (zg, rg, ng, sdg) = cfg5_case.cleaned_regions(wt, case, i)
        with np.errstate(all="ignore"):
            zo, ro, no, sdo = wo.repeat_test(np.copy(xp), ref.indexes, ref.distances, ms, msum, ref.cutoff, thr, 5)
        assert np.array_equal(ng, no), i
        assert same_bits(zg, zo) and same_bits(rg, ro), i
        assert sdg == sdo, i
        # and the oracle's fillTri + segmentTri on the short chromosomes of this sample
        calls = np.asarray(outs[i]["results_calls"], dtype=np.float64).reshape(-1, 5)
        for c in (19, 20, 21, 22):
            tri = wo.fill_tri(zs_i[c - 1])
            want = wo.segment_tri(tri, len(zs_i[c - 1]), thr, 3)
            mine = calls[calls[:, 0] == c]
            assert len(mine) == len(want), (i, c)
            assert same_bits(mine[:, 3], [v for v, _ in want]), (i, c)
            assert same_bits([outs[i]["results_cwz"][c - 1]], [tri[len(zs_i[c - 1]) - 1]]), (i, c)


def test_whole_samples_against_the_reference_and_the_oracle(wt, gw, case):
    """Every call of whole 50 kb samples: two samples against the real reference's toolTest output,
    ten against the oracle's.  Coordinates exact.  Values: the reference applies the PCA through
    BLAS and this build's prep is pinned to 1e-9, not to bits, so z / effect / chromosome-wide z
    are compared to 1e-6 relative -- and to 1e-9 when this build's `newref` output is bit for bit
    the one the fixture was made from (distances_sha256)."""
    thr = case["threshold"]
    assert thr == float(gw["threshold"])
    assert np.array_equal(case["masked_bins"], gw["masked_sizes"])
    ref = case["reference"]
    same_ref = hashlib.sha256(ref.distances.tobytes()).hexdigest() == str(gw["distances_sha256"])
    rtol = 1e-9 if same_ref else 1e-6
    if same_ref:
        assert ref.cutoff == float(gw["cutoff"])
    wanted = sorted(set(int(i) for i in gw["ref_samples"]) | set(int(i) for i in gw["oracle_samples"]))
    assert len(wanted) >= 8
    samples = [case["tests"][i] for i in wanted]
    outs = wt.test_batch(ref, samples, thr)
    stride = int(gw["stride"])
    n_calls = 0
    for i, out in zip(wanted, outs):
        calls = np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)
        for kind in ("ref", "oracle"):
            key = "%s%d_results_calls" % (kind, i)
            if key not in gw:
                continue
            want = gw[key].reshape(-1, 5)
            assert np.array_equal(calls[:, :3], want[:, :3]), (kind, i, calls[:, :3], want[:, :3])
            assert np.allclose(calls[:, 3:], want[:, 3:], rtol=rtol, atol=1e-12), (kind, i)
            assert np.allclose(out["results_cwz"], gw["%s%d_results_cwz" % (kind, i)], rtol=rtol, atol=1e-9), (kind, i)
            assert np.isclose(out["asdef"], float(gw["%s%d_asdef" % (kind, i)]), rtol=rtol, atol=0), (kind, i)
            n_calls += len(want)
        if "ref%d_results_z_sampled" % i in gw:
            z = np.concatenate(out["results_z"])
            r = np.concatenate(out["results_r"])
            assert int(np.count_nonzero(z)) == int(gw["ref%d_results_z_nonzero" % i]), i
            zs, rs = gw["ref%d_results_z_sampled" % i], gw["ref%d_results_r_sampled" % i]
            assert np.array_equal(z[::stride] == 0, zs == 0), i            # the masked / dropped bins are zeros
            assert np.allclose(z[::stride], zs, rtol=rtol, atol=1e-9 if same_ref else 1e-6), i
            assert np.allclose(r[::stride], rs, rtol=rtol, atol=1e-12 if same_ref else 1e-9), i
            assert float(gw["ref%d_threshold_z" % i]) == thr
    assert n_calls >= 50


def test_the_walker_gives_the_same_calls_on_every_call(wt, case, monkeypatch):
    """k_seg_walk + k_walk_rows on the 125 x 50 kb batch, 40 calls against ONE run of the host-driven levels: every
    call row and chromosome-wide value bit for bit, every time.  Round 5 found the call rows' medians wrong in about
    one region of 14 000 -- one call in five at this size -- while they were computed at the end of k_seg_walk's
    workgroup: a run-to-run difference that no single comparison shows (tools/gpu_repeatability.py is the same
    check at up to 1 000 samples)."""
    thr = case["threshold"]
    monkeypatch.setenv("WC_TEST_WALK", "0")
    want = wt.test_batch(case["reference"], case["tests"], thr)
    monkeypatch.delenv("WC_TEST_WALK")
    for _ in range(40):
        got = wt.test_batch(case["reference"], case["tests"], thr)
        for i, (a, b) in enumerate(zip(want, got)):
            ca = np.asarray(a["results_calls"], dtype=np.float64).reshape(-1, 5)
            cb = np.asarray(b["results_calls"], dtype=np.float64).reshape(-1, 5)
            assert ca.shape == cb.shape and same_bits(ca, cb), i
            assert same_bits(a["results_cwz"], b["results_cwz"]), i


def test_the_early_start_list_is_per_batch(wt, case, monkeypatch):
    """k_seg_walk starts the regions k_region_prefix has listed (an aberration of some length) first; the list's count is
    reset by the launch behind the walk and an entry only counts if THIS batch's index points back at it.  Different
    batches alternating on one context -- the whole 125 samples, a third of them in another order, the quiet ones
    alone -- give the calls of the same batches without the list (WC_TEST_WALK_HOT=0), bit for bit, every time."""
    thr = case["threshold"]
    tests = case["tests"]
    batches = [tests, tests[80:40:-1], tests[::5], tests[:33]]
    monkeypatch.setenv("WC_TEST_WALK_HOT", "0")
    want = [wt.test_batch(case["reference"], b, thr) for b in batches]
    monkeypatch.delenv("WC_TEST_WALK_HOT")
    for rnd in range(3):
        for q in (0, 1, 2, 3, 1, 0, 3, 2):
            got = wt.test_batch(case["reference"], batches[q], thr)
            for i, (a, b) in enumerate(zip(want[q], got)):
                ca = np.asarray(a["results_calls"], dtype=np.float64).reshape(-1, 5)
                cb = np.asarray(b["results_calls"], dtype=np.float64).reshape(-1, 5)
                assert ca.shape == cb.shape and same_bits(ca, cb), (rnd, q, i)
                assert same_bits(a["results_cwz"], b["results_cwz"]), (rnd, q, i)
