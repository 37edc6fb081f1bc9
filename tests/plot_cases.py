"""The cases `plotbatch` is held to: small chromosomes, every kind of z-score row, calls around every threshold of
upstream plotLines (wisetools.py:527-662), panel grids with a last row that is not full, a cytoband table with every
stain.  tools/make_plot_golden.py records what the reference draws for them (tests/golden/plot_primitives.npz);
tests/test_plot_cases_cpu.py and tests/test_plot_gpu.py hold the restatement and the kernels against that."""
import numpy as np

N_CHROM = 22
LENGTHS = (40, 43, 3, 2, 1, 0)
nan, inf = np.nan, np.inf


def _row(kind, n, seed):
    rng = np.random.RandomState(seed)
    z = np.round(rng.standard_normal(n) * 2.5, 3)
    z[z == 0] = 0.25
    if kind == 'all_zero':
        z[:] = 0.0
    elif kind == 'zeros_at_ends':
        z[:min(3, n)] = 0.0
        z[max(0, n - 2):] = 0.0
    elif kind == 'alternating':            # single zeros one bin apart: the most stretches a row can have
        z[::2] = 0.0
    elif kind == 'negative_zero':
        z[1::3] = -0.0
        if n > 7:
            z[5:8] = [0.0, -0.0, 0.0]
    elif kind == 'specials':
        for at, v in ((0, nan), (2, inf), (5, -inf), (6, 0.0), (7, nan), (8, 0.0), (n - 1, inf)):
            if 0 <= at < n:
                z[at] = v
    elif kind == 'one_finite':
        z[:] = nan
        if n:
            z[n // 2] = -7.5
    return z


KINDS = ('no_zero', 'all_zero', 'zeros_at_ends', 'alternating', 'negative_zero', 'specials', 'one_finite')


def zscores(shift=0):
    """22 chromosomes: the lengths and the row kinds cycle with different periods, so every pair of them occurs."""
    return [_row(KINDS[(c + shift) % len(KINDS)], LENGTHS[(c + 2 * shift) % len(LENGTHS)], 100 + c + 31 * shift)
            for c in range(N_CHROM)]


def _calls(z, mineffect):
    """Calls around every threshold: rows (chromosome, start, end, z, effect)."""
    e = mineffect / 100.0
    below, above = np.nextafter(e, 0.0), np.nextafter(e, 1.0)
    rows = [(1, 3, 9, 6.25, 0.30), (1, 12, 12, -6.35, -0.05),                      # a one-bin call
            (1, 0, len(z[0]) - 1, 0.0, 0.12),                                      # the whole chromosome, z exactly 0
            (1, 20, 25, 7.05, below), (1, 20, 25, 7.15, e), (1, 20, 25, -7.25, -above),
            (2, 1, 4, 5.55, np.nextafter(0.1, 0.0)), (2, 5, 8, -5.65, -0.1), (2, 9, 12, 5.75, np.nextafter(0.1, 1.0)),
            (2, 13, 16, 8.45, np.nextafter(0.2, 0.0)), (2, 17, 20, -8.55, 0.2), (2, 21, 24, 8.65, -np.nextafter(0.2, 1.0)),
            (2, 30, 35, 9.0, nan),                                                 # a NaN effect draws nothing
            (3, 0, 2, -4.449999, 1.5), (4, 0, 1, 12.0, 0.5), (5, 0, 0, -0.04, 0.5),
            (23, 1, 5, 9.0, 0.5)]                                                  # a chromosome that is never plotted
    for c in range(6, N_CHROM + 1):
        if len(z[c - 1]) > 4 and c % 3 == 0:
            rows.append((c, 1, len(z[c - 1]) - 2, (-1) ** c * (4.0 + c), 0.02 * c))
    return np.array(rows, dtype=np.float64)


CYTO_TEXT = "\n".join([
    "chr1\t0\t2300000\tp36.33\tgneg", "chr1\t2300000\t5400000\tp36.32\tgpos25", "chr1\t5400000\t7200000\tp36.31\tgpos100",
    "chr1\t7200000\t8100000\tp11.1\tacen", "chr1\t8100000\t9150000\tq12\tgvar", "chr1\t9150000\t10000000\tq21\tstalk",
    "chr3\t0\t300000\tp26\tgpos50", "chr3\t300000\t750000\tq11\tgneg",
    "chr4\t0\t500000\tp16\tgneg",
    "chr5\t0\t250000\tp15\tgpos75",
    "chr9\t0\t1000000\tp24\tgpos100"]) + "\n"       # chr9 is the table's last: the reference never stores it; chr2 is absent


def _case(name, chromosomes, columns, thr, mineffect, shift=0, cyto=False, calls=True, size=(4.0, 3.0), dpi=100):
    z = zscores(shift)
    table = _calls(z, mineffect)
    return dict(name=name, zscores=z, calls=table if calls else np.array([]), threshold=thr, binsize=250000, mineffect=mineffect,
                chromosomes=list(chromosomes), columns=columns, cyto=cyto, size=size, dpi=dpi, sample="sample_%s" % name)


def cases():
    out = [_case("all22_c2", range(1, 23), 2, 5.8, 1.5),
           _case("all22_c3", range(1, 23), 3, 4.25, 25.0, shift=1),
           _case("one_c1", [1], 1, 5.8, 0),
           _case("one_c2", [2], 2, 3.0, 10.0, shift=3),
           _case("two_c1", [2, 1], 1, 5.8, 1.5, shift=2),
           _case("two_c3", [1, 2], 3, 5.8, 20.0, shift=4),
           _case("five_c2", [1, 2, 3, 4, 5], 2, 5.1, 1.5, shift=5),
           _case("five_c3", [5, 4, 3, 2, 1], 3, 5.1, 1.5, shift=6),
           _case("five_c1", [1, 2, 3, 4, 5], 1, 5.1, 12.0),
           _case("nocalls", [1, 2, 3], 2, 5.8, 1.5, calls=False, shift=1),
           # with the cytoband table: the reference can only plot chromosomes its loader stored (not 2, not 9)
           _case("cyto", [1, 3, 4, 5], 2, 5.8, 1.5, cyto=True),
           _case("cyto_c3", [5, 1, 3], 3, 4.4, 0, cyto=True, shift=2)]
    return out


def build_only_cases():
    """Cases the reference dies on (KeyError in its cytoband table): held against the restatement alone."""
    return [_case("cyto_missing", [1, 2, 9, 3], 2, 5.8, 1.5, cyto=True)]
