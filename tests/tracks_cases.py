"""Inputs of the exporttracks tests, named.  The kernels' sizes (csrc/tracks.hip, csrc/deflate.hip): a tile is 256 bins,
a BGZF block 16 384 input bytes.  Rows have at most about 3 000 bins.  Everything here is made once and shared
(functools.lru_cache); callers do not modify it."""
import functools

import numpy as np

TILE = 256
LONGEST = -1.2345678901234567e-308      # 24 bytes
NAN_A = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
NAN_B = np.array([0xfff4000000abcdef], dtype=np.uint64).view(np.float64)[0]
NAN_C = np.array([0x7ff0000000000001], dtype=np.uint64).view(np.float64)[0]
INF = float("inf")


def distinct(n, seed):
    """n finite non-zero values, no two neighbours equal."""
    v = np.random.RandomState(seed).standard_normal(n) * 3.0
    assert np.all(v[1:] != v[:-1]) and np.all(v != 0)
    return v


def _with(n, seed, *runs):
    """distinct(n) with the stretches (from, to, value) overwritten."""
    v = distinct(n, seed)
    for lo, hi, value in runs:
        v[lo:hi] = value
    return v


def case(name, sizes, rows, binsize=50000, prefix="chr", clip=None, nozero=False):
    rows = np.ascontiguousarray(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
    assert rows.shape[1] == max(sum(sizes), 1), name
    rows.setflags(write=False)
    return dict(name=name, sizes=list(sizes), rows=rows, binsize=binsize, prefix=prefix, clip=clip, nozero=nozero)


@functools.lru_cache(maxsize=None)
def cases():
    T = TILE
    out = []
    out.append(case("runs_at_tile_edges", [3 * T], [
        _with(3 * T, 1, (200, T, 1.5)),                 # ends on a tile's last bin
        _with(3 * T, 2, (T, 300, 2.5)),                 # starts on a tile's first bin
        _with(3 * T, 3, (250, 262, -3.25)),             # across one tile edge
        _with(3 * T, 4, (0, T, 4.0), (T, 2 * T, 5.0), (2 * T, 3 * T, 4.0)),    # every run one whole tile
    ]))
    out.append(case("run_across_three_tiles", [5 * T], [_with(5 * T, 5, (100, 900, 0.1)), _with(5 * T, 6, (0, 5 * T, 7.0))]))
    out.append(case("one_run_per_chromosome", [300, 1, 700], [np.concatenate([np.full(300, 1.25), [2.0], np.full(700, -1e-5)])]))
    out.append(case("no_equal_neighbours", [T + 3, 2 * T - 1], [distinct(3 * T + 2, 7)]))
    out.append(case("one_bin", [1], [[0.5]]))
    out.append(case("no_bins", [0, 0], [[7e77]]))
    out.append(case("equal_across_a_chromosome_boundary", [10, 10], [np.full(20, 1.0)]))
    out.append(case("boundary_on_a_tile_edge", [T, T, 100], [np.full(2 * T + 100, 2.0), _with(2 * T + 100, 8, (T - 3, T + 3, 9.0))]))
    out.append(case("empty_chromosomes", [0, 5, 0, 0, 0, 300, 0, 2, 0, 0],
                    [np.concatenate([np.full(5, 1.0), np.full(300, 1.0), np.full(2, 1.0)]), distinct(307, 9)]))
    out.append(case("twelve_chromosomes", [3] * 12, [np.repeat(np.arange(1.0, 13.0), 3), distinct(36, 10)]))
    out.append(case("sixty_four_chromosomes", [1] * 64, [np.full(64, 1.0)]))
    out.append(case("specials", [14], [[0.0, -0.0, 0.0, NAN_A, NAN_B, NAN_A, NAN_C, INF, -INF, INF, 1.0, 1.0, -0.0, -0.0]]))
    out.append(case("specials_nozero", [14], [[0.0, -0.0, 0.0, NAN_A, NAN_B, NAN_A, NAN_C, INF, -INF, INF, 1.0, 1.0, -0.0, -0.0]], nozero=True))
    out.append(case("everything_left_out", [2 * T + 5], [np.full(2 * T + 5, NAN_A), np.full(2 * T + 5, INF),
                                                          np.where(np.arange(2 * T + 5) % 2 == 0, NAN_A, NAN_B)]))
    out.append(case("everything_left_out_nozero", [T, T + 5], [np.zeros(2 * T + 5), -np.zeros(2 * T + 5), np.full(2 * T + 5, NAN_B)], nozero=True))
    out.append(case("nozero_run_spans_tiles", [4 * T], [_with(4 * T, 11, (100, 700, 0.0)), _with(4 * T, 12, (T, 2 * T, -0.0), (2 * T, 3 * T, 0.0))],
                    nozero=True))
    out.append(case("zero_runs_kept", [4 * T], [_with(4 * T, 11, (100, 700, 0.0)), _with(4 * T, 12, (T, 2 * T, -0.0), (2 * T, 3 * T, 0.0))]))
    out.append(case("non_finite_run_spans_a_tile_edge", [2 * T + 9], [_with(2 * T + 9, 13, (250, 260, INF)), _with(2 * T + 9, 14, (500, 521, NAN_C))]))
    out.append(case("shortest_and_longest_values", [3 * T], [_with(3 * T, 15, (250, 262, 0.0), (500, 530, LONGEST)), np.full(3 * T, LONGEST),
                                                            np.where(np.arange(3 * T) % 2 == 0, LONGEST, 0.0)]))
    out.append(case("clip_last_lines", [300, 5, 0, 1], [_with(306, 16, (290, 300, 1.0)), distinct(306, 17)], binsize=1000,
                    clip=[299 * 1000 + 1, 5000, 77, 1]))
    out.append(case("binsize_one", [T + 1, 3], [_with(T + 4, 18, (T - 2, T + 1, 6.0))], binsize=1))
    out.append(case("fifteen_digits", [3, 1], [[1.0, 1.0, 2.0, 3.0], [LONGEST, 0.5, LONGEST, LONGEST]], binsize=333333333333333))
    out.append(case("no_prefix", [T + 1, 2], [distinct(T + 3, 19)], prefix=""))
    out.append(case("sixteen_byte_prefix", [T + 1] + [1] * 10, [distinct(T + 11, 20), np.full(T + 11, LONGEST)], prefix="chromosome_name_",
                    binsize=99999999999))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


SIZES = [37, 0, 1, 255, 256, 257, 12, 5, 9, 30, 2, 3, 511, 512, 513, 7, 7, 7, 1, 4, 8, 16]      # 22 chromosomes, 2 213 bins


@functools.lru_cache(maxsize=None)
def result_like_rows(n_rows):
    """n_rows rows on SIZES as result files hold them: noise, stretches of 0.0 (masked bins) across tiles and chromosome
    boundaries, a few values that are not finite."""
    rng = np.random.RandomState(100 + n_rows)
    total = sum(SIZES)
    rows = rng.standard_normal((n_rows, total)) * 2.0
    for i in range(n_rows):
        for _ in range(6):
            lo = rng.randint(0, total - 1)
            rows[i, lo:lo + rng.randint(1, 600)] = 0.0
        rows[i, rng.randint(0, total, size=3)] = (NAN_A, INF, -0.0)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def random_rows(n=300):
    """[(sizes, row, binsize, prefix)]: values drawn from a small set, so that runs occur."""
    rng = np.random.RandomState(77)
    pool = np.array([0.0, -0.0, 1.0, LONGEST, NAN_A, NAN_B, INF, -INF, 0.1, 1e22, 123456789012345.6, 5e-324])
    out = []
    for _ in range(n):
        sizes = [int(rng.randint(0, 40)) if rng.rand() < 0.8 else 0 for _ in range(rng.randint(1, 13))]
        row = pool[rng.randint(0, rng.randint(1, len(pool) + 1), size=max(sum(sizes), 1))]
        out.append((sizes, row, int(rng.choice([1, 7, 50000, 250000, 10 ** 12])), "chr"[:rng.randint(0, 4)]))
    return out


def padded(rows, stride):
    """rows [n, total] -> [n, stride], the padding filled with a value that must not show."""
    out = np.full((rows.shape[0], stride), 7e77, dtype=np.float64)
    out[:, :rows.shape[1]] = rows
    return out
