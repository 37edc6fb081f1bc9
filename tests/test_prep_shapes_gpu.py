"""newref prep (csrc/prep.hip) against the oracle at the sample, bin and component counts where its kernels take
another branch: the pairwise mean's branches, the widths of k_prep_norm_centre's tile, the 1 024-thread strides
of k_prep_sign / k_prep_transform, 1..8 components, both eigen-solvers and the one-call C entry point with its
host Jacobi.  The inputs and the expected values come from prep_cases.py (seeded counts, wo.to_numpy_array and
wo.train_pca); test_prep_cases_cpu.py shows that they are well conditioned and that the method alone agrees
with the oracle a thousand times closer than the tolerances here."""
import ctypes

import numpy as np
import pytest

import prep_cases as pc

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def prep(case, device_out=False):
    from wisecondor_amd import wisetools as wt
    n_s, n_b, n_comp = case
    counts, sizes = pc.make_case(n_s, n_b)
    return wt.prepReference(None, pcacomp=n_comp, counts=counts, chrom_bins=sizes, device_out=device_out)


def assert_matches_oracle(case, masked, mask, corrected, comps, mean, mbins):
    """The assertions every route shares; prints the two measured errors first."""
    n_s, n_b, n_comp = case
    want = pc.oracle(*case)
    pc.check_conditions(want, n_comp)
    assert np.array_equal(np.asarray(mask).astype(bool), want["mask"])
    assert [int(v) for v in mbins] == want["masked_chrom_bins"]
    assert masked.shape == (n_b, n_s) == want["masked"].shape
    assert same_bits(masked, want["masked"])                                     # one IEEE division per element
    assert same_bits(mean, np.mean(want["masked"].T, axis=0))                    # numpy's pairwise sum per bin
    assert comps.shape == (n_comp, n_b) and corrected.shape == (n_b, n_s)
    comp_err, corr_err = pc.errors(corrected, comps, want)
    print("%s: components %.3e, correctedData %.3e (relative)" % (pc.case_id(case), comp_err, corr_err))
    assert np.allclose(comps, want["comps"], rtol=0, atol=pc.COMP_ATOL)          # signs included
    assert np.allclose(corrected, want["corrected"], rtol=pc.CORRECTED_RTOL, atol=0)


def check_both_forms(case):
    import torch
    want = pc.oracle(*case)
    masked, bins, mask, corrected, comps, mean, mbins = prep(case)
    assert [int(v) for v in bins] == [int(v) for v in want["chrom_bins"]]
    assert_matches_oracle(case, masked, mask, corrected, comps, mean, mbins)
    dev = prep(case, device_out=True)
    assert isinstance(dev[3], torch.Tensor) and dev[3].is_cuda and dev[3].is_contiguous()
    assert same_bits(dev[0].cpu().numpy(), masked)
    assert same_bits(dev[3].cpu().numpy(), corrected)            # k_prep_correct_bs against k_prep_correct
    assert same_bits(dev[4], comps) and same_bits(dev[5], mean)
    assert list(dev[6]) == list(mbins) and np.array_equal(dev[2], mask)


@pytest.mark.parametrize("case", pc.MEAN_CASES, ids=pc.case_id)
def test_prep_pairwise_mean_branches(case):
    """Sample counts on every branch of the pairwise mean of k_prep_norm_centre: fewer than 8 (3, 7), 8, a tail
    of one (9) and of four (100), 128 / 129 / 130 on either side of the recursion, 257, and 600 (split at
    296 / 304; tile of 16 bins, more than 48 KB of LDS, odd bin count).  257 x 31: fewer bins than one tile or
    one 64-bin group of k_prep_components."""
    check_both_forms(case)


@pytest.mark.parametrize("case", pc.NB_CASES + [pc.BIG_CASE], ids=pc.case_id)
def test_prep_tile_width_switches(case):
    """k_prep_norm_centre's tile is 32 bins up to 383 samples, then 16, 8 up to 1 535, 4 up to 3 071, then 2:
    the last and first sample count of a width (the row stride is S | 1, the sample step 256 / NB)."""
    check_both_forms(case)


@pytest.mark.parametrize("case", pc.BIN_CASES, ids=pc.case_id)
def test_prep_bin_count_edges(case):
    """1 023, 1 024 and 1 025 masked bins: the strides of the 1 024-thread k_prep_sign and k_prep_transform."""
    assert pc.oracle(*case)["masked"].shape[0] == case[1]
    check_both_forms(case)


@pytest.mark.parametrize("case", pc.COMP_CASES, ids=pc.case_id)
def test_prep_component_counts(case):
    """1, 2, 4 and 8 components (the C ABI's range; every other test asks for 3)."""
    check_both_forms(case)


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_prep_both_solvers(monkeypatch, mode):
    """The GPU eigen-solver and LAPACK on the fetched Gram matrix, eight pairs at the headline sample count."""
    monkeypatch.setenv("WC_PREP_EIG", mode)
    case = (100, 1025, 8)
    masked, bins, mask, corrected, comps, mean, mbins = prep(case)
    assert_matches_oracle(case, masked, mask, corrected, comps, mean, mbins)


def one_call(counts, sizes, n_comp):
    """wc_newref_prep as a C caller uses it: the size query, then the call with every output.
    Returns (status, message, mask, maskedChromBins, maskedData, correctedData [B, S], components, mean)."""
    from wisecondor_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    n_s, n_total = counts.shape
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    mask, mbins, nb = np.empty(n_total, dtype=np.uint8), np.empty(22, dtype=np.int64), ctypes.c_int64()
    _lib.check(lib.wc_newref_prep(ctx, _lib.ptr(counts), n_s, n_total, _lib.ptr(sizes), 22, n_comp, _lib.ptr(mask),
                                  _lib.ptr(mbins), ctypes.byref(nb), None, None, None, None))
    n_b = nb.value
    masked, ct, comps, mean = np.empty((n_b, n_s)), np.empty((n_s, n_b)), np.empty((max(n_comp, 1), n_b)), np.empty(n_b)
    rc = lib.wc_newref_prep(ctx, _lib.ptr(counts), n_s, n_total, _lib.ptr(sizes), 22, n_comp, _lib.ptr(mask),
                            _lib.ptr(mbins), ctypes.byref(nb), _lib.ptr(masked), _lib.ptr(ct), _lib.ptr(comps),
                            _lib.ptr(mean))
    return rc, lib.wc_last_error().decode(), mask, mbins, masked, ct.T, comps[:n_comp], mean


@pytest.mark.parametrize("case", pc.ONE_CALL_CASES, ids=pc.case_id)
def test_prep_one_call_against_oracle(case):
    """wc_newref_prep through ctypes: nine samples (the GPU solver) and two (the host Jacobi, which nothing
    else reaches; with two samples the centred data has rank one and the reconstruction is exact)."""
    counts, sizes = pc.make_case(case[0], case[1])
    rc, msg, mask, mbins, masked, corrected, comps, mean = one_call(counts, sizes, case[2])
    assert rc == 0, msg
    assert_matches_oracle(case, masked, mask, corrected, comps, mean, mbins)


@pytest.mark.parametrize("n_s,n_comp,text", [(1, 1, "rank below"), (2, 3, "components"), (3, 4, "components")])
def test_prep_one_call_refuses(n_s, n_comp, text):
    """One sample has no variance to take a component from; more components than samples do not exist."""
    from wisecondor_amd import _lib
    counts, sizes = pc.make_case(n_s, 300)
    rc, msg = one_call(counts, sizes, n_comp)[:2]
    assert rc == _lib.E_ARG and text in msg, (rc, msg)
