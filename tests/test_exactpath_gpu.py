"""newref's exact path in its normal form (the one launch k_exact_dev, row count known to the device only) at
chosen row counts, shapes and layouts.

The lever: wc_newref_import_lists_dev marks a row for the exact path when the imported count exceeds the source
capacity (include/wisecondor_hip.h: "A source row with more than `cap` entries marks the row for the exact fallback
path"), so  prepare -> thresholds -> collect -> import(src_cap = 1, cnt = 2 for the chosen rows, 0 elsewhere) ->
finish  sends exactly the chosen rows (plus whatever the fast path hands over by itself: N0 of a clean run) through
k_exact_dev.  Every case asserts
  * every row of the output, forced or not, equals the numpy oracle (indexes equal, distances bit for bit, the
    -1 / 1e10 padding included); above 2048 samples the forced rows plus 64 fixed unforced rows (wo.oracle_rows);
  * max(N, N0) <= fallback_rows <= N + N0 and fast_rows + fallback_rows == B; N0 == 0 on the plain-noise datasets,
    where the count is therefore exactly N;
  * wc_newref_exact_dev (the host-counted form) on the same prepared state gives the same bits.
Regimes of k_exact_dev (newref.hip): EX_DEV_CAP = 256 rows are filled by tile workgroups (64 x 64 sequential,
32 x 32 pairwise), rows beyond by fb_fill in one of 64 select workgroups (second trip from 256 + 64), rows of a
"lone" chromosome by fb_fill whatever their slot.  Which row lands in which slot changes from run to run (atomicAdd).
"""
import numpy as np
import pytest

from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu

SAMPLE_UNFORCED = 64         # unforced rows compared where the whole-matrix oracle is too dear


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


# ------------------------------------------------------------------ datasets ----
def _hg19_sizes(binsize):
    """22 chromosomes at `binsize`, chr21 cut to a single bin."""
    from wisecondor_amd import synth
    sizes = synth.chrom_bins(binsize)
    sizes[20] = 1
    return sizes


def _noise(sizes, samples, seed):
    from wisecondor_amd import synth
    data, bins, _ = synth.corrected_matrix(0, samples, seed=seed, sizes=sizes)
    return data, bins


def _dups():
    """Exact duplicate rows across chromosomes: one cluster of 150 (more than k = 100: a target that is itself a
    member sees ~140 candidates at distance 0, and any target sees 150 equal keys in a row, which straddle rank k
    for the targets that rank the cluster near it), one of 40, and 30 pairs."""
    data, bins = _noise(_hg19_sizes(1000000), 24, 21)
    rng = np.random.RandomState(22)
    perm = rng.permutation(data.shape[0])
    clusters = [perm[:150], perm[150:190]] + [perm[190 + 2 * i:192 + 2 * i] for i in range(30)]
    for members in clusters:
        data[members] = data[members[0]]
    members = np.concatenate([clusters[0][:25], clusters[1][:10]] + clusters[2:12])
    return data, bins, members


SPECIAL_ROWS = {"nan": 500, "inf": 900, "big": 1300, "zero": 1700}     # four different chromosomes of the 1 Mb layout


def _specials():
    """A NaN entry, an inf entry, a row times 1e6 (every distance to it >= 1e10) and an all-zero row."""
    data, bins = _noise(_hg19_sizes(1000000), 24, 23)
    data[SPECIAL_ROWS["nan"], 5] = np.nan
    data[SPECIAL_ROWS["inf"], 23] = np.inf
    data[SPECIAL_ROWS["big"]] *= 1e6
    data[SPECIAL_ROWS["zero"]] = 0.0
    return data, bins, np.array(sorted(SPECIAL_ROWS.values()))


# name -> (builder, default k, plain noise: a clean run must leave every row on the fast path,
#          whole-matrix oracle affordable)
DATASETS = {
    "noise24": (lambda: _noise(_hg19_sizes(1000000), 24, 3), 100, True, True),
    "noise5": (lambda: _noise(_hg19_sizes(2000000), 5, 5), 100, True, True),
    "noise8": (lambda: _noise(_hg19_sizes(2000000), 8, 8), 100, True, True),
    "noise129": (lambda: _noise(_hg19_sizes(2000000), 129, 129), 100, True, True),
    "noise257": (lambda: _noise(_hg19_sizes(2000000), 257, 257), 100, True, True),
    "wide2100": (lambda: _noise([130, 100, 80, 1, 59, 30], 2100, 2100), 100, True, False),
    "smallk": (lambda: _noise([200, 60, 50, 20], 24, 31), 200, True, True),
    "small300": (lambda: _noise([110, 90, 1, 60, 39], 24, 33), 50, True, True),
    "lone[1,300,1]": (lambda: _noise([1, 300, 1], 40, 41), 20, False, True),
    "lone[1,300]": (lambda: _noise([1, 300], 40, 42), 20, False, True),
    "lone[1,0,300,1]": (lambda: _noise([1, 0, 300, 1], 40, 43), 20, False, True),
    "dups": (_dups, 100, False, True),
    "specials": (_specials, 100, False, True),
}
_data = {}
_oracle = {}
_clean = {}


def dataset(name):
    """(data [B, S] C-ordered, bins, rows the case must force besides the drawn ones)."""
    if name not in _data:
        made = DATASETS[name][0]()
        _data[name] = (made[0], np.asarray(made[1], dtype=np.int64), made[2] if len(made) > 2 else np.zeros(0, dtype=np.int64))
    return _data[name]


def laid_out(data, order):
    return np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)


def reference(name, order, k, rows):
    """The oracle's (idx, dst) for `rows` of dataset `name`: cut from the whole-matrix oracle (computed once per
    dataset, order and k), or row by row (cached per row) where that is too dear."""
    data, bins, _ = dataset(name)
    lay = laid_out(data, order)
    sums = np.cumsum(bins)
    key = (name, order, k)
    with np.errstate(all="ignore"):
        if DATASETS[name][3]:
            if key not in _oracle:
                _oracle[key] = wo.get_reference(lay, bins, sums, k, 1, 1, fast=True)
            return _oracle[key][0][rows], _oracle[key][1][rows]
        have = _oracle.setdefault(key, {})
        todo = [int(r) for r in rows if int(r) not in have]
        if todo:
            got_i, got_d = wo.oracle_rows(lay, bins, sums, k, todo)
            for n, r in enumerate(todo):
                have[r] = (got_i[n], got_d[n])
    return np.array([have[int(r)][0] for r in rows]), np.array([have[int(r)][1] for r in rows])


def pick_rows(bins, n, seed, extra=()):
    """`n` target rows, fixed by `seed`: the rows in `extra`, row 0, row B - 1, the first and the last row of a long
    chromosome, every one-bin chromosome, a run of 70 consecutive rows (longer than a tile of either order) across
    the end of that chromosome, and scattered rows.  Fewer than that many rows: a rotating choice of the edge rows."""
    bins = np.asarray(bins, dtype=np.int64)
    sums = np.cumsum(bins)
    B = int(sums[-1])
    if n >= B:
        return np.arange(B, dtype=np.int64)
    big = int(np.argmax(bins[1:])) + 1
    first, last = int(sums[big] - bins[big]), int(sums[big] - 1)
    musts = list(dict.fromkeys([0, B - 1, first, last] + [int(sums[c] - 1) for c in np.flatnonzero(bins == 1)]))
    if n < len(musts):
        musts = musts[n % len(musts):] + musts[:n % len(musts)]
    run_len = min(70, max(0, (n - len(musts) - len(extra)) // 2))
    run_start = max(0, min(B - run_len, last - run_len // 2))
    scattered = np.random.RandomState(seed).permutation(B)
    chosen = list(dict.fromkeys([int(r) for r in extra] + musts + list(range(run_start, run_start + run_len))
                                + [int(r) for r in scattered]))[:n]
    rows = np.array(sorted(chosen), dtype=np.int64)
    assert len(rows) == n and len(set(chosen)) == n
    if n >= 150 + len(extra):
        assert set(musts) <= set(chosen) and run_len == 70 and set(range(run_start, run_start + 70)) <= set(chosen)
    return rows


# ------------------------------------------------------------ the forcing helper ----
class Forced(object):
    """One prepared newref state on context 0 with chosen rows marked for the exact path."""

    def __init__(self, name, order, k=None):
        import torch
        from wisecondor_amd import _lib, distributed
        self.torch = torch
        self.name, self.order = name, order
        data, self.bins, self.extra = dataset(name)
        self.k = DATASETS[name][1] if k is None else k
        self.B = data.shape[0]
        self.X = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        self.st = distributed.HipStages(_lib.context(0), self.X, self.bins, self.k,
                                        _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)
        self.rows = np.zeros(0, dtype=np.int64)

    def prepare(self, rows=None):
        """prepare -> thresholds -> collect -> import that marks `rows` (None: a clean run, no import)."""
        torch, st, B = self.torch, self.st, self.B
        st.prepare()
        st.thresholds(0, B)
        st.collect(0, B, 0, 1)
        self.rows = np.zeros(0, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        if len(self.rows):
            cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
            cnt[torch.from_numpy(self.rows).cuda()] = 2        # > src_cap = 1: "entries were lost"; 0 adds nothing
            lst = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
            st.import_(0, B, 1, cnt, lst)
            torch.cuda.synchronize()
        return self

    def _run(self, call, bands):
        torch, B, k = self.torch, self.B, self.k
        idx = torch.full((B, k), -7, dtype=torch.int32, device="cuda")           # never a valid output
        dst = torch.full((B, k), float("nan"), dtype=torch.float64, device="cuda")
        for rb, re in bands or [(0, B)]:
            if re > rb:
                call(rb, re, idx[rb:re], dst[rb:re])
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()

    def finish(self, bands=None):
        """wc_newref_finish_dev over all rows, or band by band (rb > 0) into one output."""
        return self._run(self.st.finish, bands)

    def exact(self):
        """wc_newref_exact_dev: every row by the host-counted form of the exact path."""
        return self._run(self.st.exact, None)

    def stats(self, wt):
        return wt.newref_stats(0)

    def compared_rows(self):
        if DATASETS[self.name][3]:
            return np.arange(self.B, dtype=np.int64)
        unforced = np.setdiff1d(np.arange(self.B), self.rows)
        take = np.random.RandomState(64).permutation(len(unforced))[:SAMPLE_UNFORCED]
        assert len(unforced) == 0 or len(take) == min(SAMPLE_UNFORCED, len(unforced))
        return np.union1d(self.rows, unforced[take])

    def assert_oracle(self, idx, dst, what):
        rows = self.compared_rows()
        assert set(self.rows.tolist()) <= set(rows.tolist())             # every forced row is compared
        want_i, want_d = reference(self.name, self.order, self.k, rows)
        bad = (idx[rows] != want_i).any(axis=1)
        a, b = dst[rows], np.asarray(want_d, dtype=np.float64)
        bad |= ~((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))).all(axis=1)
        if bad.any():
            forced = set(self.rows.tolist())
            wrong = rows[bad]
            pytest.fail("%s: %s order %s k=%d: %d of %d compared rows differ from the oracle (%d of them forced); first: %s"
                        % (what, self.name, self.order, self.k, len(wrong), len(rows),
                           sum(int(r) in forced for r in wrong), wrong[:12].tolist()))
        assert np.array_equal(idx[rows], want_i) and same_bits(dst[rows], want_d)


def clean_count(wt, name, order, k):
    """N0: rows a clean run (no import) hands to the exact path by itself; its output is held against the oracle too."""
    key = (name, order, k)
    if key not in _clean:
        job = Forced(name, order, k).prepare(None)
        idx, dst = job.finish()
        stats = job.stats(wt)
        assert stats["fast_rows"] + stats["fallback_rows"] == job.B, stats
        job.assert_oracle(idx, dst, "clean run")
        print("N0 %s order %s k=%d B=%d: %d" % (name, order, k, job.B, stats["fallback_rows"]))
        _clean[key] = stats["fallback_rows"]
    if DATASETS[name][2]:
        assert _clean[key] == 0, "plain noise %s order %s k=%d: a clean run sent %d rows to the exact path" % (
            name, order, k, _clean[key])
    return _clean[key]


def assert_count(stats, n_forced, n0, B):
    assert stats["fast_rows"] + stats["fallback_rows"] == B, stats
    assert max(n_forced, n0) <= stats["fallback_rows"] <= n_forced + n0, (stats, n_forced, n0)


def forced_case(wt, name, order, n, k=None, seed=1):
    """The whole check of one case; returns the finished output."""
    job = Forced(name, order, k)
    n0 = clean_count(wt, name, order, job.k)
    rows = pick_rows(job.bins, n, seed, extra=job.extra)
    job.prepare(rows)
    idx, dst = job.finish()
    stats = job.stats(wt)                       # before exact(): that marks every row
    print("case %s order %s k=%d N=%d: %s" % (name, order, job.k, len(rows), stats))
    assert_count(stats, len(rows), n0, job.B)
    job.assert_oracle(idx, dst, "forced finish")
    ex_i, ex_d = job.exact()
    assert np.array_equal(ex_i, idx) and same_bits(ex_d, dst), "host-counted exact path differs from the forced finish"
    return job, idx, dst


# ------------------------------------------------------------------ the cases ----
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 319, 320, 321, 700, "B"])
def test_row_count_regimes(wt, n, order):
    """2 849 bins (1 Mb, chr21 cut to one bin; not a multiple of 32 or 64) x 24 samples, k = 100: tile edges of both
    orders, the cap (255 / 256 / 257: the last row filled by tiles, the first row filled by its select workgroup),
    the select workgroups' second trip (319 / 320 / 321), far beyond, every row.  C: pairwise order, 32 x 32 tiles;
    F: sequential order, 64 x 64 tiles."""
    B = dataset("noise24")[0].shape[0]
    assert B == 2849
    forced_case(wt, "noise24", order, B if n == "B" else n, seed=100 + (0 if n == "B" else n))


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [100, 500], ids=["N100-tiles", "N500-tiles+fb_fill"])
@pytest.mark.parametrize("samples", [5, 8, 129, 257])
def test_sample_counts(wt, samples, n, order):
    """Fewer than 8 samples (sequential code under either order), one chunk, pairwise leaves beyond 128 samples
    and chunk remainders (129 = 128 + 1, 257 = 2 x 128 + 1), on 1 434 bins (2 Mb).  24 samples: test_row_count_regimes."""
    forced_case(wt, "noise%d" % samples, order, n, seed=samples)


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [50, 350], ids=["N50-tiles", "N350-tiles+fb_fill_global_target"])
def test_more_than_2048_samples(wt, n, order):
    """2 100 samples x 400 bins: k_finish hands the rows over instead of k_pick, and rows beyond the cap read their
    target row from global memory.  Oracle: the forced rows and 64 fixed unforced rows (wo.oracle_rows)."""
    forced_case(wt, "wide2100", order, n, seed=7)


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [64, 700], ids=["N64-tiles", "N700-tiles+fb_fill"])
@pytest.mark.parametrize("k", [1, 256])
def test_k_edges(wt, k, n, order):
    """k = 1 and k = 256 (the largest k of this path) on the 1 Mb matrix; k = 100 is everywhere else."""
    forced_case(wt, "noise24", order, n, k=k, seed=k)


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [64, "B"], ids=["N64-tiles", "NB330-tiles+fb_fill"])
def test_k_above_the_candidate_count(wt, n, order):
    """Chromosomes of 200 / 60 / 50 / 20 bins, k = 200: rows of the first chromosome have 130 candidates, so the
    selection pads with -1 / 1e10 (fb_select)."""
    job, idx, dst = forced_case(wt, "smallk", order, 330 if n == "B" else n, seed=9)
    assert (idx[0, 130:] == -1).all() and (dst[0, 130:] == 1e10).all() and (idx[0, :130] >= 0).all()


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [40, "B"], ids=["N40-fill_below_cap", "NB-fill_below_and_beyond_cap"])
@pytest.mark.parametrize("layout", ["lone[1,300,1]", "lone[1,300]", "lone[1,0,300,1]"])
def test_lone_chromosome(wt, layout, n, order):
    """A long chromosome with at most one bin before and after it: in a Fortran-ordered file its rows are "lone"
    (lone_mask) -- numpy sums their distances pairwise although the file is sequential, and inside k_exact_dev they are
    filled by fb_fill in their select workgroup, below the cap (slot < 256) and beyond it, never by the tiles.  C order
    has no lone rows: there the ids read "tiles" and "tiles + fb_fill"."""
    B = dataset(layout)[0].shape[0]
    job, idx, dst = forced_case(wt, layout, order, B if n == "B" else n, seed=13)
    if order == "F":
        assert _clean[(layout, order, job.k)] >= 300          # the lone rows take the exact path in a clean run as well


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [120, 700], ids=["N120-tiles", "N700-tiles+fb_fill"])
def test_duplicate_rows_and_ties_at_rank_k(wt, n, order):
    """Exact duplicates among the forced rows and among their candidates, clusters that straddle rank k: the selection
    keeps the stable (distance, position) order when the k-th key is tied."""
    job, idx, dst = forced_case(wt, "dups", order, n, seed=17)
    # the data must really tie at rank k for forced rows (the premise of the case): a forced member of the
    # 150-cluster has more than k candidates at distance 0
    members = job.extra[:25]
    assert set(members.tolist()) <= set(job.rows.tolist())
    assert (dst[members] == 0.0).all() and (idx[members] >= 0).all()
    assert (np.diff(idx[members], axis=1) > 0).all()           # equal keys: ascending position


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [60, 700], ids=["N60-tiles", "N700-tiles+fb_fill"])
def test_special_values(wt, n, order):
    """A NaN entry, an inf entry, a row times 1e6 and an all-zero row, each as a forced target and as a candidate of
    the other forced rows: `d < 1e10` admission in both fill codes, specials propagate as numpy's do."""
    job, idx, dst = forced_case(wt, "specials", order, n, seed=19)
    assert set(SPECIAL_ROWS.values()) <= set(job.rows.tolist())
    for tag in ("nan", "inf", "big"):
        row = SPECIAL_ROWS[tag]
        assert (idx[row] == -1).all() and (dst[row] == 1e10).all(), tag         # no candidate is admitted
    assert (idx[SPECIAL_ROWS["zero"]] >= 0).all()


# --------------------------------------------------- state on one context ----
BANDS = [(0, 700), (700, 1400), (1400, 2100), (2100, 2849)]
BAND_FORCED = [300, 3, 0, 256]


def _band_rows(bins):
    rows = []
    for (rb, re), n in zip(BANDS, BAND_FORCED):
        inside = pick_rows(bins, 900, seed=23)
        inside = inside[(inside >= rb) & (inside < re)]
        more = np.setdiff1d(np.arange(rb, re), inside)
        take = np.concatenate([inside, np.random.RandomState(rb).permutation(more)])[:n]
        rows.append(np.sort(take))
    return rows


@pytest.mark.parametrize("order", ["C", "F"])
def test_banded_finishes_with_changing_counts(wt, order):
    """Four bands of ONE prepared state with 300, 3, 0 and 256 forced rows, finished band by band into one output,
    then once more in reverse order: the counter reset between launches (sync[0..1], fb_dirty) and the rb > 0
    addressing of the handed-over rows.  wc_newref_stats walks the per-row status of the whole matrix, so after the
    last band it holds the sum over the bands."""
    n0 = clean_count(wt, "noise24", order, 100)
    job = Forced("noise24", order)
    per_band = _band_rows(job.bins)
    assert [len(r) for r in per_band] == BAND_FORCED
    rows = np.concatenate(per_band)
    job.prepare(rows)
    idx, dst = job.finish(BANDS)
    assert_count(job.stats(wt), len(rows), n0, job.B)
    job.assert_oracle(idx, dst, "bands in order")
    idx2, dst2 = job.finish(BANDS[::-1])
    assert_count(job.stats(wt), len(rows), n0, job.B)
    job.assert_oracle(idx2, dst2, "bands in reverse order")
    ex_i, ex_d = job.exact()
    assert np.array_equal(ex_i, idx) and same_bits(ex_d, dst)


@pytest.mark.parametrize("order", ["C", "F"])
def test_same_finish_twice_then_exact_then_finish(wt, order):
    """finish, finish, exact, finish on one prepared state: four equal results, equal to the oracle."""
    n0 = clean_count(wt, "noise24", order, 100)
    job = Forced("noise24", order)
    rows = pick_rows(job.bins, 400, seed=29)
    job.prepare(rows)
    first = job.finish()
    assert_count(job.stats(wt), len(rows), n0, job.B)
    job.assert_oracle(first[0], first[1], "first finish")
    second = job.finish()
    assert_count(job.stats(wt), len(rows), n0, job.B)
    third = job.exact()
    fourth = job.finish()
    assert_count(job.stats(wt), len(rows), n0, job.B)
    for n, (i, d) in enumerate((second, third, fourth)):
        assert np.array_equal(i, first[0]) and same_bits(d, first[1]), "result %d differs from the first" % (n + 2)


@pytest.mark.parametrize("order", ["C", "F"])
def test_small_job_after_a_large_one(wt, order):
    """2 849 bins, then 300 bins on the same context (scratch and the row list keep the large job's contents),
    then the large one again."""
    large, _, _ = forced_case(wt, "noise24", order, 700, seed=31)
    forced_case(wt, "small300", order, 280, seed=37)
    idx, dst = large.prepare(large.rows).finish()
    assert_count(large.stats(wt), len(large.rows), 0, large.B)
    large.assert_oracle(idx, dst, "the large job again")


@pytest.mark.parametrize("order", ["C", "F"])
def test_run_to_run(wt, order):
    """N = 700 three times in one process, a fresh prepare each time: which row gets which tile slot or beyond-cap
    slot differs between runs by construction, the results may not."""
    n0 = clean_count(wt, "noise24", order, 100)
    job = Forced("noise24", order)
    rows = pick_rows(job.bins, 700, seed=100 + 700)
    results = []
    for trip in range(3):
        job.prepare(rows)
        idx, dst = job.finish()
        assert_count(job.stats(wt), len(rows), n0, job.B)
        job.assert_oracle(idx, dst, "trip %d" % trip)
        results.append((idx, dst))
    for idx, dst in results[1:]:
        assert np.array_equal(idx, results[0][0]) and same_bits(dst, results[0][1])
