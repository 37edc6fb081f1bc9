"""Inputs and CPU references shared by the prep and PCA-apply shape tests (a helper module, not a conftest).

Count matrices on which a comparison of newref prep with the oracle means something: the leading
singular values are separated (an eigenvector's error grows with the inverse of the gap to its
neighbours) and no reconstruction comes near zero (a ratio's error grows with the inverse of its
denominator).  Both properties are asserted by the tests from the oracle alone, see check_conditions().

    counts[s, b] ~ Poisson(depth_s * profile_b * (1 + sum_j a_j u[j, s] v[j, b]))

with eight planted components of geometrically falling amplitude.  About a tenth of the bins are zero
in every sample; the 22-chromosome layout is ragged, has one chromosome that loses every bin to the
mask and one of a single bin.  Everything is seeded by the case.
"""
import functools

import numpy as np

from oracle import wc_oracle as wo

N_PLANTED = 8
DEPTH = 20000.0
RATIO_MIN = 1.15          # s[j] / s[j + 1] for every j < n_comp
CORRECTED_MAX = 0.5       # abs(correctedData - 1) everywhere
COMP_ATOL = 1e-9          # the project's tolerances (README, test_prep_gpu.py)
CORRECTED_RTOL = 1e-10
ZERO_CHROM, ONE_CHROM = 13, 20      # (0-based) the chromosome without a kept bin, the one of a single bin

# (samples, masked bins, components): see the docstrings of the tests for what each one is there for
MEAN_CASES = [(3, 300, 1), (7, 300, 3), (8, 300, 3), (9, 65, 5), (100, 1025, 8), (128, 999, 3), (129, 999, 3),
              (130, 999, 5), (257, 31, 8), (600, 2049, 8)]
NB_CASES = [(383, 63, 3), (385, 65, 3), (1535, 150, 8), (1537, 150, 8)]
BIG_CASE = (3073, 120, 3)
BIN_CASES = [(40, 1023, 2), (40, 1024, 2), (40, 1025, 2)]
COMP_CASES = [(40, 700, 1), (40, 700, 2), (40, 700, 4), (40, 700, 8)]
ONE_CALL_CASES = [(9, 65, 3), (2, 300, 1)]
ALL_CASES = MEAN_CASES + NB_CASES + [BIG_CASE] + BIN_CASES + COMP_CASES + ONE_CALL_CASES

# cases whose default seed gave a singular-value ratio below RATIO_MIN: a steeper amplitude decay
DECAY = {(100, 1025): 0.65}


def case_id(case):
    return "S%d-B%d-n%d" % case


def layout(n_masked, rng):
    """22 ragged chromosome sizes and the bins (genomic positions) that are zero in every sample.

    n_masked bins stay; about n_masked / 9 more are empty: all of chromosome ZERO_CHROM + 1 and the rest
    scattered.  Chromosome ONE_CHROM + 1 has one bin, a kept one."""
    n_zero = max(2, int(round(n_masked / 9.0)))
    zero_len = max(1, n_zero // 3)
    n_total = n_masked + n_zero
    spare = n_total - zero_len - 1 - 20           # beyond one bin for each of the twenty ordinary chromosomes
    assert spare >= 0
    sizes = np.ones(22, dtype=np.int64)
    ordinary = [c for c in range(22) if c not in (ZERO_CHROM, ONE_CHROM)]
    sizes[ordinary] += rng.multinomial(spare, rng.dirichlet(np.full(20, 1.5)))
    sizes[ZERO_CHROM] = zero_len
    offs = np.concatenate([[0], np.cumsum(sizes)])
    empty = np.zeros(n_total, dtype=bool)
    empty[offs[ZERO_CHROM]:offs[ZERO_CHROM + 1]] = True
    free = np.flatnonzero(~empty)
    free = free[free != offs[ONE_CHROM]]
    empty[rng.choice(free, n_zero - zero_len, replace=False)] = True
    assert int((~empty).sum()) == n_masked
    return sizes, empty


@functools.lru_cache(maxsize=None)
def make_case(n_samples, n_masked, seed=0):
    """(counts int32 [S, n_total], chromosome sizes [22]); the arrays are shared: read-only."""
    rng = np.random.RandomState(100003 * n_samples + 17 * n_masked + seed)
    sizes, empty = layout(n_masked, rng)
    n_total = int(sizes.sum())
    decay = DECAY.get((n_samples, n_masked), 0.7)
    amp = 0.10 * decay ** np.arange(N_PLANTED)
    u = np.clip(rng.standard_normal((N_PLANTED, n_samples)), -2.5, 2.5)
    v = rng.uniform(-1.0, 1.0, (N_PLANTED, n_total))
    depth = DEPTH * rng.uniform(0.5, 2.0, n_samples)
    profile = rng.uniform(0.5, 1.5, n_total)
    lam = depth[:, None] * profile[None, :] * (1.0 + np.einsum("j,js,jb->sb", amp, u, v))
    counts = rng.poisson(lam).astype(np.int32)
    counts[:, empty] = 0
    counts.setflags(write=False)
    sizes.setflags(write=False)
    return counts, sizes


def as_samples(counts, sizes):
    """The dict form of the rows (keys '1'..'22'), what the oracle's to_numpy_array takes."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [{str(c + 1): row[offs[c]:offs[c + 1]] for c in range(22)} for row in counts]


@functools.lru_cache(maxsize=None)
def oracle(n_samples, n_masked, n_comp):
    """The expected values of a case, computed once: dict of read-only arrays."""
    counts, sizes = make_case(n_samples, n_masked)
    masked, chrom_bins, mask = wo.to_numpy_array(as_samples(counts, sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    masked_chrom_bins = [int(mask[offs[c]:offs[c + 1]].sum()) for c in range(22)]
    with np.errstate(all="ignore"):
        corrected, comps, mean = wo.train_pca(masked, n_comp)
    t = masked.T
    sing = np.linalg.svd(t - np.mean(t, axis=0), compute_uv=False)
    out = dict(counts=counts, sizes=sizes, masked=masked, chrom_bins=chrom_bins, mask=mask,
               masked_chrom_bins=masked_chrom_bins, corrected=corrected, comps=comps, mean=mean, sing=sing)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_conditions(want, n_comp):
    """The two fixed conditions on a case, from the oracle's values alone; a case that violates one fails."""
    s = want["sing"]
    assert len(s) > n_comp
    ratios = s[:n_comp] / s[1:n_comp + 1]
    assert np.all(ratios >= RATIO_MIN), ratios
    assert np.all(np.abs(want["corrected"] - 1.0) <= CORRECTED_MAX), np.abs(want["corrected"] - 1.0).max()
    assert want["masked_chrom_bins"][ZERO_CHROM] == 0 and want["masked_chrom_bins"][ONE_CHROM] == 1


def gram_route(masked, n_comp):
    """trainPCA the way prep does it, in plain numpy float64: eigh of the [samples, samples] Gram matrix of
    the centred data, the components from the eigenvectors, svd_flip, projection, division.
    Returns (correctedData [B, S], components [n, B], mean [B])."""
    t = masked.T
    mean = np.mean(t, axis=0)
    xc = t - mean
    vals, vecs = np.linalg.eigh(xc @ xc.T)
    order = np.argsort(vals)[::-1][:n_comp]
    comps = (vecs[:, order].T / np.sqrt(vals[order])[:, None]) @ xc
    at = np.argmax(np.abs(comps), axis=1)
    comps = comps * np.sign(comps[np.arange(n_comp), at])[:, None]
    tr = xc @ comps.T
    with np.errstate(all="ignore"):
        corrected = t / (tr @ comps + mean)
    return corrected.T, comps, mean


def errors(corrected, comps, want):
    """(largest absolute component error, largest relative correctedData error) against the oracle."""
    comp_err = float(np.abs(np.asarray(comps) - want["comps"]).max())
    corr_err = float(np.abs(np.asarray(corrected) / want["corrected"] - 1.0).max())
    return comp_err, corr_err


# ------------------------------------------------------------------ PCA apply (the test path) ----
APPLY_COMPS = [0, 1, 2, 3, 5, 8]
APPLY_BINS = [1, 7, 8, 9, 2047, 2048, 2049, 8191, 8193, 16391]
APPLY_ROWS = [1, 3, 33]


def pca_basis(rng, n_bins, n_comp):
    """n_comp unit rows: the first ones an orthonormal basis from np.linalg.qr, and where there are fewer bins
    than components (the kernels do not care) further random unit rows."""
    k = min(n_bins, n_comp)
    comps = np.linalg.qr(rng.standard_normal((n_bins, k)))[0].T.reshape(k, n_bins)
    if n_comp > k:
        extra = rng.standard_normal((n_comp - k, n_bins))
        comps = np.concatenate([comps, extra / np.linalg.norm(extra, axis=1, keepdims=True)])
    return np.ascontiguousarray(comps)


@functools.lru_cache(maxsize=None)
def apply_case(n_comp, n_bins):
    """(x [33, B] unit-sum rows of Poisson counts, mean ~ 1/B with 1 % jitter, comps [n_comp, B]); read-only."""
    rng = np.random.RandomState(7919 * n_comp + n_bins)
    comps = pca_basis(rng, n_bins, n_comp)
    mean = np.full(n_bins, 1.0 / n_bins) * (1 + 0.01 * rng.standard_normal(n_bins))
    lam = 3000.0 * (1 + 0.02 * rng.standard_normal((max(APPLY_ROWS), n_bins))).clip(0.5)
    counts = rng.poisson(lam)
    x = counts / counts.sum(axis=1, keepdims=True).astype(np.float64)
    for a in (x, mean, comps):
        a.setflags(write=False)
    return x, mean, comps


def apply_pca_longdouble(x, mean, comps):
    """applyPCA (wisetools.py:104-113) for the rows of x in np.longdouble, rounded to float64 at the end."""
    xl, ml, cl = (np.asarray(a, dtype=np.longdouble) for a in (x, mean, comps))
    transform = np.dot(xl - ml, cl.T)
    reconstructed = np.dot(transform, cl) + ml
    return np.asarray(xl / reconstructed, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def apply_want(n_comp, n_bins):
    x, mean, comps = apply_case(n_comp, n_bins)
    want = apply_pca_longdouble(x, mean, comps)
    want.setflags(write=False)
    return want
