"""The test path's PCA apply (k_pca_project, k_pca_apply, k_pca_apply_t, k_lat_project, k_lat_apply in
csrc/testpath.hip) at 0..8 components and at bin counts on either side of the projection's slice and trip sizes
(8 slices; 256 x 4 bins per trip in k_pca_project, 256 x 8 in k_lat_project): wt.applyPCA against a
np.longdouble restatement, wc_prepare_samples against applyPCA bit for bit, and the three routes of
wt.test_batch (latency, batch, general path for a lone sample) against each other bit for bit and against the
oracle.  Inputs and the longdouble reference: prep_cases.py (checked on the CPU by test_prep_cases_cpu.py)."""
import numpy as np
import pytest

import prep_cases as pc
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@pytest.mark.parametrize("n_bins", pc.APPLY_BINS)
@pytest.mark.parametrize("n_comp", pc.APPLY_COMPS)
def test_apply_pca_against_longdouble(wt, n_comp, n_bins):
    """1, 3 and 33 rows; rtol 1e-12 (float64 numpy stays within 1e-13 of the same reference)."""
    x, mean, comps = pc.apply_case(n_comp, n_bins)
    want = pc.apply_want(n_comp, n_bins)
    for rows in pc.APPLY_ROWS:
        got = wt.applyPCA(np.ascontiguousarray(x[:rows]), mean, comps)
        assert got.shape == (rows, n_bins)
        print("n_comp %d, bins %d, rows %d: %.3e" % (n_comp, n_bins, rows, np.abs(got / want[:rows] - 1).max()))
        assert np.allclose(got, want[:rows], rtol=1e-12, atol=0)
        if n_comp == 0:
            assert same_bits(got, x[:rows] / mean)
    assert same_bits(wt.applyPCA(x[2], mean, comps), got[2])          # a lone vector: the same bits as in a call of 33


def masked_layout(rng, n_bins):
    """22 chromosome sizes of at least one bin with about a tenth more bins than n_bins, a mask that keeps n_bins."""
    n_total = 22 + n_bins + n_bins // 10
    sizes = (1 + rng.multinomial(n_total - 22, np.full(22, 1.0 / 22))).astype(np.int64)
    mask = np.zeros(n_total, dtype=bool)
    mask[rng.choice(n_total, n_bins, replace=False)] = True
    offs = np.concatenate([[0], np.cumsum(sizes)])
    msizes = np.array([int(mask[offs[c]:offs[c + 1]].sum()) for c in range(22)], dtype=np.int64)
    return sizes, mask, msizes


@pytest.mark.parametrize("n_bins", [7, 2047, 2049, 8193])
@pytest.mark.parametrize("n_comp", pc.APPLY_COMPS)
def test_prepare_samples_equals_apply_pca(wt, n_comp, n_bins):
    """wc_prepare_samples (k_sample_totals, k_normalize, k_pca_project, k_pca_apply) on a layout with masked
    bins: raw is counts / total in one division, out is what applyPCA makes of raw."""
    from wisecondor_amd import _lib
    rng = np.random.RandomState(31 * n_bins + n_comp)
    _, mean, comps = pc.apply_case(n_comp, n_bins)
    sizes, mask, msizes = masked_layout(rng, n_bins)
    counts = rng.poisson(3000.0 * (1 + 0.02 * rng.standard_normal((3, len(mask)))).clip(0.5)).astype(np.int32)
    ref = wt.Reference(np.zeros((n_bins, 1), np.int32), np.full((n_bins, 1), 1e10), sizes, msizes, mask, mean, comps,
                       cutoff=0.0)
    try:
        out, raw = np.empty((3, n_bins)), np.empty((3, n_bins))
        _lib.check(_lib.load().wc_prepare_samples(ref.ctx, ref.handle, _lib.ptr(counts), 3, _lib.ptr(out), _lib.ptr(raw)))
    finally:
        ref.close()
    assert same_bits(raw, counts[:, mask] / counts.sum(axis=1, keepdims=True).astype(np.float64))
    assert same_bits(out, wt.applyPCA(raw, mean, comps))


# ------------------------------------------------------------------------------- the three routes ----
N_FILL = 33
# where the five samples sit in the longer calls: first and last place, and in the call of 33 both sides of
# k_pca_apply_t's 32-sample tile (a call of 33 is padded to 48 samples with copies of sample 0)
PLACES = {8: [0, 2, 3, 6, 7], 9: [0, 1, 4, 7, 8], 33: [0, 7, 16, 31, 32]}


def make_reference(wt, layout_id):
    """A reference as in test_random_gpu.test_whole_test_path_random, without the PCA part."""
    rng = np.random.RandomState(4100 + layout_id)
    lo, hi = [(25, 70), (80, 125)][layout_id]                            # the second layout: about 2 100 bins
    sizes = rng.randint(lo, hi, size=22).astype(np.int64)
    total = int(sizes.sum())
    mask = rng.rand(total) > 0.06
    offs = np.concatenate([[0], np.cumsum(sizes)])
    msizes = np.array([int(mask[offs[i]:offs[i + 1]].sum()) for i in range(22)], dtype=np.int64)
    n_bins = int(msizes.sum())
    corrected = 1.0 + 0.02 * rng.standard_normal((n_bins, 20))
    idx, dst = wt.getReference(np.asfortranarray(corrected), msizes, np.cumsum(msizes), 30, 1, 1)
    samples = []
    for _ in range(5 + N_FILL):
        lam = np.full(total, 3000.0) * (1 + 0.02 * rng.standard_normal(total)).clip(0.5)
        c = rng.randint(0, 22)
        a = offs[c] + rng.randint(0, max(1, sizes[c] - 12))
        lam[a:a + rng.randint(4, 12)] *= rng.choice([0.6, 1.4, 1.08])
        counts = rng.poisson(lam).astype(np.int32)
        samples.append({str(c + 1): counts[offs[c]:offs[c + 1]] for c in range(22)})
    return dict(sizes=sizes, mask=mask, msizes=msizes, n_bins=n_bins, idx=idx, dst=dst, samples=samples)


@pytest.fixture(scope="module")
def layouts(wt):
    made = {}

    def get(layout_id):
        if layout_id not in made:
            made[layout_id] = make_reference(wt, layout_id)
        return made[layout_id]
    return get


def assert_same_results(a, b, what):
    assert same_bits(np.concatenate(a["results_z"]), np.concatenate(b["results_z"])), what
    assert same_bits(np.concatenate(a["results_r"]), np.concatenate(b["results_r"])), what
    assert same_bits(a["results_cwz"], b["results_cwz"]), what
    assert same_bits(np.asarray(a["results_calls"]).reshape(-1, 5), np.asarray(b["results_calls"]).reshape(-1, 5)), what


# (eight components first: the slots of the projection's workspace beyond a later case's count then hold values)
@pytest.mark.parametrize("n_comp", [8, 0, 1, 2, 5])
@pytest.mark.parametrize("layout_id", [0, 1])
def test_routes_agree_and_match_oracle(wt, layouts, monkeypatch, layout_id, n_comp):
    """Five samples alone (k_lat_project + k_lat_apply), in a call of 8 (the same kernels, eight samples), of 9 and
    of 33 (k_pca_project from the counts + k_pca_apply_t) and alone on the general path: the same bits in z, ratios,
    chromosome-wide z and calls; and each sample against the oracle's toolTest."""
    lay = layouts(layout_id)
    n_bins = lay["n_bins"]
    rng = np.random.RandomState(977 * layout_id + n_comp)
    comps = pc.pca_basis(rng, n_bins, n_comp)
    mean = np.full(n_bins, 1.0 / n_bins) * (1 + 0.01 * rng.standard_normal(n_bins))
    ref = dict(binsize=np.float64(1e6), indexes=lay["idx"], distances=lay["dst"], chromosome_sizes=lay["sizes"],
               mask=lay["mask"], masked_sizes=lay["msizes"], pca_mean=mean, pca_components=comps)
    five, fill = lay["samples"][:5], lay["samples"][5:]
    thr, minref, repeats = 4.2, 5, 4
    monkeypatch.delenv("WC_TEST_LATENCY_MODE", raising=False)
    reference = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], mean, comps, binsize=1e6)
    try:
        def run(samples):
            return wt.test_batch(reference, samples, thr, minrefbins=minref, repeats=repeats)
        alone = [run([s])[0] for s in five]
        for n, places in sorted(PLACES.items()):
            call = list(fill[:n])
            for s, at in zip(five, places):
                call[at] = s
            outs = run(call)
            for i, at in enumerate(places):
                assert_same_results(outs[at], alone[i], "sample %d at place %d of %d" % (i, at, n))
        monkeypatch.setenv("WC_TEST_LATENCY_MODE", "0")
        for i, s in enumerate(five):
            assert_same_results(run([s])[0], alone[i], "sample %d alone on the general path" % i)
    finally:
        reference.close()
    for sample, out in zip(five, alone):
        with np.errstate(all="ignore"):
            want = wo.test_sample(sample, 1e6, ref, minzscore=thr, minrefbins=minref, repeats=repeats)
        wc_ = np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5)
        gc_ = out["results_calls"].reshape(-1, 5)
        assert np.array_equal(gc_[:, :3], wc_[:, :3]), (gc_, wc_)
        assert np.allclose(gc_[:, 3:], wc_[:, 3:], rtol=1e-8, equal_nan=True)
        assert np.allclose(np.concatenate(out["results_z"]), np.concatenate(want["results_z"]),
                           rtol=1e-8, atol=1e-10, equal_nan=True)
        assert np.allclose(np.concatenate(out["results_r"]), np.concatenate(want["results_r"]),
                           rtol=1e-8, atol=1e-10, equal_nan=True)
        assert np.allclose(out["results_cwz"], want["results_cwz"], rtol=1e-8, atol=1e-9, equal_nan=True)
        if n_comp == 0:                                   # no projection: data = x / mean, every later step is bit-exact
            assert same_bits(gc_, wc_), (gc_, wc_)
            assert same_bits(np.concatenate(out["results_z"]), np.concatenate(want["results_z"]))
            assert same_bits(np.concatenate(out["results_r"]), np.concatenate(want["results_r"]))
            assert same_bits(out["results_cwz"], want["results_cwz"])
