"""The inputs of the robust-spread and blacklist tests (a helper module, not a conftest).

THE HAND-WRITTEN COLUMNS (COLUMNS): short columns at the edges of the rule of wc_column_robust, each with a name; matrix()
lays them side by side, padded with both zeros, so that the lanes of one wave see different counts, 0 and 1 among them.

THE PLANTED COHORT: N = 40 synth.make_sample samples of READS reads on a layout of 22 chromosomes of 8 .. 22 bins (307
bins, no multiple of 64), tested leave-one-out with refsize 12, minrefbins 4, two repeats and a fixed |z| cut of 5.  Every
fifth bin (PLANTED, 61 bins) is noisy: its count in sample i is multiplied by 1 + TAU * u, u the i-th entry of a
permutation, the bin's own, of N evenly spaced values in -1 .. 1 -- every planted bin carries the same amount of noise, so
either all of them pass a reference's distance cutoff or none does.  ONE noisy bin among quiet ones is not a test of a
blacklist: its distances to every other bin lie far above the cutoff (mean + 3 sd over all bins), the test path finds fewer
than minrefbins reference bins for it and fills its z with 0.0 -- the pipeline drops it by itself.  A fifth of the bins
being noisy is what widens the cutoff until such bins are tested, and then their held-out z-scores are wide.
test_robust_cases_cpu.py holds on the CPU, through the oracle alone, that every planted bin has a robust spread of
2 * MAXSPREAD at least and every other bin that MINCOVER of the samples tested one of MAXSPREAD / 2 at most (measured when
the cohort was designed: 13.8 at least against 1.95 at most); the GPU test demands the planted set exactly on that ground.
"""
import functools
import os

import numpy as np

from oracle import wc_oracle as wo
from wisecondor_amd import synth

NAN, INF = float("nan"), float("inf")
TINY = 5e-324
UP = float(np.nextafter(1.0, 2.0))
UP2 = float(np.nextafter(UP, 2.0))

COLUMNS = [
    ("none", []),
    ("one", [-3.25]),
    ("two", [1.0, 4.0]),
    ("all equal", [2.5] * 6),
    ("all equal, odd", [-2.5] * 5),
    ("ties across the middle pair", [3.0, 2.0, 1.0, 2.0]),
    ("the lower run ends at the middle rank", [3.0, 1.0, 2.0, 1.0]),
    ("the lower run ends at the middle rank, long", [7.0, 1.0, 1.0, 9.0, 1.0, 8.0]),
    ("one ulp apart", [UP2, 1.0, UP, 1.0, UP2, UP]),
    ("one ulp apart, odd", [UP2, 1.0, UP]),
    ("negatives only", [-1.0, -2.5, -3.0, -0.125]),
    ("signs around zero", [-1e-3, 2e-3, -5e-3, 1e-3, 3e-3, -TINY]),
    ("pairs -x and +x", [-2.0, 2.0, 3.0, -3.0]),                    # the median is +0.0 and the deviations tie
    ("pairs -x and +x and one more", [-2.0, 2.0, 3.0, -3.0, 2.0, -2.0]),
    ("1e300 beside 5e-324", [1e300, TINY, -TINY, 1e300, TINY]),
    ("subnormals", [TINY, 2 * TINY, 3 * TINY, -TINY]),
    ("the middle pair overflows", [1.7e308, 1.7e308, -1.0, 1.6e308]),        # median inf, mad NaN
    ("the middle pair overflows downwards", [-1.7e308, -1.7e308, 1.0, -1.6e308]),
    ("a deviation overflows", [-1.5e308, 1.5e308, 1.6e308, 1.7e308, -1.5e308]),
    ("the deviations' middle pair overflows", [-1.7e308, -1.7e308, 1.0e308, 1.7e308]),      # mad inf
    ("nonfinite and zeros kept out", [INF, -INF, NAN, 0.0, -0.0, 1.5, -2.5, 3.5]),
    ("nonfinite only", [INF, NAN, -INF, -0.0]),
    ("zeros only", [0.0, -0.0, 0.0]),
]


def matrix(columns=None, stride=None):
    """The named columns side by side as a float64 matrix [longest, stride], the rest filled with +0.0 and -0.0 in turn."""
    columns = [values for _, values in COLUMNS] if columns is None else columns
    rows = max(1, max(len(v) for v in columns))
    Z = np.zeros((rows, len(columns) if stride is None else stride))
    Z[1::2] = -0.0
    if stride is not None:
        Z[:, len(columns):] = 777.0                    # what lies behind a row's columns is never read
    for b, values in enumerate(columns):
        Z[:len(values), b] = values
    return Z


def random_matrix(seed, n_rows, n_cols, stride=None):
    """Random rows with ties, untested bins, a few nonfinite values, a wide range of magnitudes, and columns that differ in how
    many values they hold."""
    rng = np.random.RandomState(seed)
    kind = rng.randint(4, size=n_cols)
    Z = rng.standard_normal((n_rows, n_cols)) * 3
    Z = np.where(kind == 1, np.round(Z), Z)                                        # ties, and zeros from the rounding
    Z = np.where(kind == 2, Z * 10.0 ** rng.randint(-300, 300, size=(n_rows, n_cols)), Z)
    Z = np.where(kind == 3, np.ldexp(np.round(Z), -1074), Z)                       # subnormals
    Z[rng.random_sample((n_rows, n_cols)) < rng.random_sample(n_cols) * 0.5] = 0.0     # a share of its own per column
    Z[rng.random_sample((n_rows, n_cols)) < 0.02] = -0.0
    for value in (NAN, INF, -INF):
        Z[rng.randint(n_rows), rng.randint(n_cols)] = value
    if n_cols > 2:
        Z[:, 1] = 0.0                                                              # nothing
        Z[1:, 2] = -0.0                                                            # one value at most
    if stride is not None:
        wide = np.full((n_rows, stride), 777.0)
        wide[:, :n_cols] = Z
        Z = wide
    return Z


# ------------------------------------------------------------------------------------------ the planted cohort ----
N = 40
SIZES = [22, 21, 20, 19, 18, 17, 16, 15, 15, 14, 14, 13, 13, 12, 12, 11, 11, 10, 9, 9, 8, 8]
N_TOTAL = 307
BINSIZE = 1000000
READS = 2e6
REFSIZE, MINREF, REPEATS, THR = 12, 4, 2, 5.0
TAU = 0.4
PLANTED = list(range(2, N_TOTAL, 5))                   # flat bin indexes
MAXSPREAD, MINCOVER = 5.0, 0.5
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
PREP_N = 24                                            # the samples of the prepReference(drop=...) tests: the first 24


def place(flat):
    """(chromosome 1-based, bin) of a flat bin index."""
    c = int(np.searchsorted(OFFS, flat, side="right")) - 1
    return c + 1, int(flat - OFFS[c])


@functools.lru_cache(maxsize=None)
def samples():
    """The forty sample dicts '1' .. '22'."""
    assert sum(SIZES) == N_TOTAL and N_TOTAL % 64 and len(SIZES) == 22
    profile = synth.bin_profile(BINSIZE, SIZES)
    factors = [np.linspace(-1.0, 1.0, N)[np.random.RandomState(900 + k).permutation(N)] for k in range(len(PLANTED))]
    out = []
    for i in range(N):
        smp = synth.make_sample(profile, 300 + i, reads=READS)
        for k, flat in enumerate(PLANTED):
            c, g = place(flat)
            assert profile[c - 1][g] > 0.0
            smp[str(c)][g] = int(round(smp[str(c)][g] * (1.0 + TAU * factors[k][i])))
        out.append(smp)
    return out


def counts(n=N):
    """int32 [n, 307]: the dense image of the first n samples (wt.samples_to_counts without the package)."""
    return np.stack([np.concatenate([s[str(c)] for c in range(1, 23)]) for s in samples()[:n]]).astype(np.int32)


def planted_drop():
    drop = np.zeros(N_TOTAL, dtype=np.uint8)
    drop[PLANTED] = 1
    return drop


def oracle_reference(training, drop=None, refsize=REFSIZE):
    """The reference the oracle builds from the samples `training`, as a mapping with the keys of a reference file.  With
    `drop` the mask is restated: wo.to_numpy_array, the rows of its masked data whose bin drop leaves, then wo.train_pca and
    wo.get_reference as ever."""
    with np.errstate(all="ignore"):
        masked, chrom_bins, mask = wo.to_numpy_array([samples()[i] for i in training])
        mask = np.asarray(mask).astype(bool)
        if drop is not None:
            keep = ~np.asarray(drop).astype(bool)
            masked = masked[keep[mask]]
            mask = mask & keep
        corrected, comps, mean = wo.train_pca(masked)
        masked_sizes = [int(mask[OFFS[c]:OFFS[c + 1]].sum()) for c in range(22)]
        idx, dst = wo.get_reference(corrected, masked_sizes, np.cumsum(masked_sizes), select_ref_amount=refsize, fast=True)
    return dict(binsize=BINSIZE, indexes=idx, distances=dst, chromosome_sizes=np.array(chrom_bins), mask=mask,
                masked_sizes=np.array(masked_sizes), pca_mean=mean, pca_components=comps, masked=masked, corrected=corrected)


@functools.lru_cache(maxsize=None)
def oracle_loo():
    """float64 [40, 307]: every sample's results_z from wo.test_sample against the oracle's reference of the other 39."""
    Z = np.zeros((N, N_TOTAL))
    with np.errstate(all="ignore"):
        for i in range(N):
            reference = oracle_reference([j for j in range(N) if j != i])
            out = wo.test_sample(samples()[i], BINSIZE, reference, minzscore=THR, minrefbins=MINREF, repeats=REPEATS)
            Z[i] = np.concatenate(out["results_z"])
    Z.setflags(write=False)
    return Z


def write_cli_files(folder, n=N):
    """The first n sample files as `convert` writes them, under `folder`."""
    paths = []
    for i, smp in enumerate(samples()[:n]):
        paths.append(os.path.join(str(folder), "healthy_%02d.npz" % i))
        total = int(sum(int(v.sum()) for v in smp.values()))
        quality = dict(mapped=total, unmapped=0, no_coordinate=0, filter_rmdup=0, filter_mapq=0, pre_retro=total, post_retro=total)
        np.savez_compressed(paths[-1], arguments={"binsize": float(BINSIZE)}, runtime={}, sample=smp, quality=quality)
    return paths
