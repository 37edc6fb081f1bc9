"""newref's fast path (k_pick + k_rescore) at every workgroup shape a refsize selects.  newref_finish_part launches
k_rescore with ps = max(128, min(512, round_up(k + 28, 64))) threads: two waves up to k = 100 -- the one shape
test_pick_entry_slack_gpu.py, test_pick_batched_gpu.py, test_rescore_rows_gpu.py and test_rescore_need_gpu.py walk --
three up to 164, four up to 228, five up to 256.  Here the wave slabs of a third to fifth wave, the trip loop's stride,
the pass / DMA-group switch on those waves' pair counts, the strided loops of the counting order, its tie sweep and
the output, pick_row's bisection against k (and its LEAN form), and the largest dynamic LDS request are each run with
a pair count that the layout fixes (refsize_cases.py; held to the oracle on the CPU by test_refsize_cases_cpu.py).

Every case: a few chromosomes, every threshold at FLT_MAX; the output is held against the oracle bit for bit
(indexes equal, distances by their int64 view) in both orders -- F: k_rescore<true, false>, register staging in passes
of eight rows; C: k_rescore<false, true>, LDS-DMA groups of sixteen -- and the counters against the design: which rows
took the fast path, and how many pairs were re-scored.  A case whose count is off has not reached its boundary."""
import numpy as np
import pytest

import refsize_cases as rc
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
ORDERS = ["F", "C"]


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


class Job(object):
    """prepare / thresholds / every threshold FLT_MAX / collect on one input at refsize k; finish() as often as a test
    wants."""

    def __init__(self, data, bins, k, order="F"):
        import torch
        from wisecondor_amd import _lib, distributed
        self.torch = torch
        self.B, self.k = data.shape[0], k
        self.X = torch.from_numpy(np.array(data, order="C")).cuda()          # (a copy: the cached input is read-only)
        self.st = distributed.HipStages(_lib.context(0), self.X, np.asarray(bins, dtype=np.int64), k,
                                        _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)
        self.st.prepare()
        self.st.thresholds(0, self.B)
        self.st.set_thr(0, self.B, torch.full((self.B,), float(FMAX), dtype=torch.float32, device="cuda"))
        self.st.collect(0, self.B, 0, 1)

    def finish(self, rb=0, re=None):
        """-> (idx, dst) of the whole job after finish(rb, re); rows outside the band keep -7 / NaN."""
        torch = self.torch
        re = self.B if re is None else re
        idx = torch.full((self.B, self.k), -7, dtype=torch.int32, device="cuda")
        dst = torch.full((self.B, self.k), float("nan"), dtype=torch.float64, device="cuda")
        self.st.finish(rb, re, idx[rb:re], dst[rb:re])
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()

    def stats(self):
        from wisecondor_amd import wisetools
        return wisetools.newref_stats(0)


def check(got, want):
    assert np.array_equal(got[0], want[0])
    assert same_bits(got[1], want[1])


def check_padding(got, rows, n, k):
    """The rows `rows` have n candidates: n answers, then the sentinels."""
    if n < k:
        assert (got[0][rows, :n] >= 0).all() and (got[0][rows, n:] == -1).all()
        assert (got[1][rows, :n] < 1e10).all() and (got[1][rows, n:] == 1e10).all()


def run_designed(family, args, k, order):
    """One full finish of the layout; output, padding and counters as designed.  Returns the output."""
    data, bins = rc.MAKERS[family](*args)
    B = data.shape[0]
    rescored, fallback = rc.designed(family, args, k)
    job = Job(data, bins, k, order)
    got = job.finish()
    stats = job.stats()
    print("%s%s k %d (ps %d) order %s: %s, designed %d pairs" % (family, args, k, rc.ps_of(k), order, stats, rescored))
    check(got, rc.oracle(family, args, k, order))
    check_padding(got, slice(0, bins[0]), bins[1], k)
    check_padding(got, slice(bins[0], B), bins[0], k)
    assert stats["fallback_rows"] == fallback and stats["fast_rows"] == B - fallback, stats
    assert stats["rescored"] == rescored, (stats, rescored)
    return got


# --------------------------------------------------------------- first trip, waves 2 to 3, pair count exact ----
# few(70, b): the 70 rows of the first chromosome re-score exactly b pairs, one trip; the last wave in use (the third
# at k = 164, the fourth at k = 228 and 256) holds b - 128 resp. b - 192 of them: none, 1, 7, 8, 9, 15, 16, 17 ... --
# either side of every pass of eight and every DMA group of sixteen
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k,b", [(k, b) for k, bs in rc.FEW_B.items() for b in bs])
def test_pass_boundaries_of_the_last_wave(k, b, order):
    run_designed("few", (rc.T_ROWS, b), k, order)


# ------------------------------------------------- fifth wave, second and third trips, the RMAX edge ----
# near(m): the 70 target rows re-score exactly m pairs.  m - ps pairs go into a second trip (a third from 2 ps on: 385
# and more at k = 101), whose wave w starts at pair ps + 64 w; 512 fills the row's pair slots, 513 is one too many: the
# target rows take the exact path, the same bits
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k,m", [(k, m) for k, ms in rc.NEAR_M.items() for m in ms])
def test_trips_and_waves_of_a_cluster(k, m, order):
    run_designed("near", (m,), k, order)


# k = 1 and 2: two waves, and the 70 target rows are k or more candidates for the rows of chromosome 2, which then
# re-score what their bound admits -- the target rows' count is taken from a finish of their band alone
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k,m", [(k, m) for k, ms in rc.NEAR_M_SMALL.items() for m in ms])
def test_smallest_refsizes(k, m, order):
    data, bins = rc.near(m)
    B, T = data.shape[0], bins[0]
    want = rc.oracle("near", (m,), k, order)
    job = Job(data, bins, k, order)
    part = job.finish(0, T)
    stats = job.stats()
    print("near(%d) k %d order %s, target rows: %s" % (m, k, order, stats))
    assert np.array_equal(part[0][:T], want[0][:T]) and same_bits(part[1][:T], want[1][:T])
    assert (part[0][T:] == -7).all() and np.isnan(part[1][T:]).all()
    assert stats["fast_rows"] == T and stats["fallback_rows"] == 0, stats
    assert stats["rescored"] == T * m, stats
    check(job.finish(), want)
    stats = job.stats()
    assert stats["fast_rows"] == B and stats["fallback_rows"] == 0, stats
    assert T * m + (B - T) * k <= stats["rescored"] <= T * m + (B - T) * T, stats


# ------------------------------------------------------------------ ties with a strided second sweep ----
# m bit-identical nearest rows: every target row's m distances tie, the counting order leaves holes and its second
# sweep (position as the tie-break) runs over more pairs than the workgroup has threads
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k,m", rc.COPIES_KM)
def test_ties_beyond_one_trip(k, m, order):
    got = run_designed("copies", (m,), k, order)
    assert np.array_equal(got[0][:rc.T_ROWS], np.tile(np.arange(k, dtype=np.int32), (rc.T_ROWS, 1)))
    assert (got[1][:rc.T_ROWS] == got[1][:rc.T_ROWS, :1]).all()


# ---------------------------------------------------------- pick_row's LEAN form away from k = 100 ----
# 600 candidates per target row (more than 512 list entries): the bisection counts against k over sixteen entries per
# lane, and the candidate words are read again behind it
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", rc.LEAN_K)
def test_long_lists(k, order):
    assert rc.designed("near", rc.LEAN_ARGS, k)[0] == 70 * 300 + 600 * 70
    run_designed("near", rc.LEAN_ARGS, k, order)


# ----------------------------------------------------------------------- the largest LDS request ----
# 2 048 samples at five waves: 16 384 bytes of target row and 40 960 of wave slabs, the most k_rescore ever asks for;
# 2 047 samples are padded to the same.  A refused launch comes back as an error from finish()
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("args", rc.BIG_LDS_ARGS, ids=lambda a: "%d_samples" % a[3])
def test_largest_lds_request(args, order):
    run_designed("near", args, rc.BIG_LDS_K, order)


# --------------------------------------------------------------------------- stale slabs at five waves ----
@pytest.mark.parametrize("order", ORDERS)
def test_stale_slabs_of_five_waves_never_reach_an_output(order):
    """512 pairs first (both trips fill every slab row of the five waves), then twice a job of 257 pairs: a first
    trip of four full waves and one pair on the fifth, whose passes 2 .. 8 (DMA groups 2 .. 4) write nothing -- those
    slab rows hold what the job before left there.  No second trip."""
    k = rc.STALE_K
    run_designed("near", rc.STALE_ARGS[0], k, order)
    first = run_designed("near", rc.STALE_ARGS[1], k, order)
    second = run_designed("near", rc.STALE_ARGS[1], k, order)
    assert np.array_equal(first[0], second[0]) and same_bits(first[1], second[1])


# ----------------------------------------------------------------------------------- natural thresholds ----
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", rc.NATURAL_K)
def test_natural_thresholds(k, order):
    """The whole getReference with its own thresholds on plain noise (the 1 Mb layout, 24 samples): the rows are shared
    between the fast and the exact path as the thresholds decide (the list length aimed at does not follow k, so the
    exact path's share grows towards 256: printed, not bounded)."""
    from wisecondor_amd import synth
    from wisecondor_amd import wisetools as wt
    data, bins, sums = synth.corrected_matrix(1000000, 24, seed=k)
    if order == "F":
        data = np.asfortranarray(data)
    idx, dst = wt.getReference(data, bins, sums, k, 1, 1)
    stats = wt.newref_stats()
    print("natural thresholds k %d order %s: %s, exact-path share %.4f"
          % (k, order, stats, stats["fallback_rows"] / float(data.shape[0])))
    want_i, want_d = wo.get_reference(data, bins, sums, k, 1, 1, fast=True)
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    assert stats["fast_rows"] + stats["fallback_rows"] == data.shape[0], stats
    assert stats["fast_rows"] > 0, stats


# ------------------------------------------------------------------------------------- k_select_thr<32> ----
def test_threshold_selection_of_32_keys_per_lane():
    """15 400 rows give 1 152 sampled columns, 18 per lane: the k_select_thr<32> instance (up to 14 336 rows it is
    <16>, at the 50 kb matrix <64>).  One part of about 500 rows against the oracle's same part."""
    from wisecondor_amd import synth
    from wisecondor_amd import wisetools as wt
    data, bins, sums = synth.corrected_matrix(0, 8, seed=32, sizes=[700] * 22)
    part, parts = 16, 31
    idx, dst = wt.getReference(data, bins, sums, 100, part, parts)
    stats = wt.newref_stats()
    rows = idx.shape[0]
    print("15 400 rows x 8 samples, part %d of %d (%d rows): %s" % (part, parts, rows, stats))
    want_i, want_d = wo.get_reference(data, bins, sums, 100, part, parts, fast=True)
    assert 450 <= rows <= 550
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    assert stats["sample_cols"] == 1152, stats
    assert stats["fast_rows"] + stats["fallback_rows"] == rows, stats
    assert stats["fallback_rows"] <= rows // 20, stats
