"""The candidate's slack in the list entry: k_convert packs (row | slack code << index bits), k_gram_glds copies that
word into the entry, k_pick forms its upper bound from it without a gather, the exchange format stays (key, plain row).

Matrices as in test_pick_batched_gpu.py (1 + 0.03 N(0, 1)), three chromosomes whose sizes put the last padded row
number at 255, 511 and 1 279, so that "exactly the bits the problem needs" is 8, 9 and 11 index bits and the highest row
numbers sit directly under the code field.  Every case runs at the automatic width (17 index bits, a 15-bit code), at
exactly the needed width (the widest code) and at 24 (an 8-bit, exponent-only code).  Lists on both sides of 512
entries -- the two forms of k_pick's selection -- come from the two threshold modes: the sampled thresholds list about
384 candidates, every threshold at FLT_MAX lists all rows of the other chromosomes (up to 979 here)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (chromosome sizes, bits the last padded row number needs)
LAYOUTS = {"pad256": ([90, 70, 85], 8), "pad512": ([200, 150, 155], 9), "pad1280": ([560, 300, 419], 11)}
SAMPLES = [16, 100]
ORDERS = ["F", "C"]            # F: sequential sums, C: numpy's pairwise sums
K = 100
FMAX = np.finfo(np.float32).max
CASES = [(n, s, o) for n in sorted(LAYOUTS) for s in SAMPLES for o in ORDERS]
MARKED = 5                     # rows handed to the exact path through the import's marker


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def stats_of(ctx):
    from wisecondor_amd import _lib
    out = np.zeros(8, dtype=np.int64)
    _lib.check(_lib.load().wc_newref_stats(ctx, _lib.ptr(out)))
    return dict(fast_rows=int(out[0]), fallback_rows=int(out[1]), rescored=int(out[4]))


class _Case(object):
    """One matrix on the GPU; everything the tests share is computed once and kept unchanged."""

    def __init__(self, name, n_samples, order):
        import torch
        from wisecondor_amd import _lib, distributed
        self.torch = torch
        self.name, self.order = name, order
        sizes, self.need = LAYOUTS[name]
        self.bins = np.asarray(sizes, dtype=np.int64)
        self.B = int(self.bins.sum())
        assert ((self.B + 127) // 128 * 128 - 1).bit_length() == self.need
        self.widths = [0, self.need, 24]
        rng = np.random.RandomState(1000 * sorted(LAYOUTS).index(name) + 10 * n_samples + ORDERS.index(order))
        self.data = 1.0 + 0.03 * rng.standard_normal((self.B, n_samples))
        self.chrom = np.repeat(np.arange(len(self.bins)), self.bins)
        self.X = torch.from_numpy(np.ascontiguousarray(self.data)).cuda()
        self.sum_order = _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE
        self.ctx = _lib.context(0)
        self.st = distributed.HipStages(self.ctx, self.X, self.bins, K, self.sum_order)
        self._oracle = None
        self._passes = {}

    def oracle(self):
        if self._oracle is None:
            lay = np.asfortranarray(self.data) if self.order == "F" else np.ascontiguousarray(self.data)
            with np.errstate(all="ignore"):
                self._oracle = wo.get_reference(lay, self.bins, np.cumsum(self.bins), K, 1, 1, fast=True)
        return self._oracle

    def collect(self, st, bits, thr):
        """prepare at `bits` index bits / thresholds (thr: None = the sampled ones, else per-row values) / collect.
        The requested width is taken back at once: the context is shared with every other test of the session."""
        torch, B = self.torch, self.B
        st.set_index_bits(bits)
        try:
            st.prepare()
        finally:
            st.set_index_bits(0)
        assert st.index_bits() == (bits or 17)
        st.thresholds(0, B)
        if thr is not None:
            st.set_thr(0, B, torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).cuda())
        st.collect(0, B, 0, 1)

    def exports(self, st):
        """(cnt, plain entries, raw entries, slack per row) of the lists as they stand."""
        torch, B, cap = self.torch, self.B, st.cap
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        cnt_raw = torch.zeros(B, dtype=torch.int32, device="cuda")
        plain = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
        raw = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
        st.export(0, B, cap, cnt, plain)
        st.export_raw(0, B, cap, cnt_raw, raw)
        lo = torch.zeros(B, dtype=torch.float32, device="cuda")
        slack = torch.zeros(B, dtype=torch.float32, device="cuda")
        st.get_bounds(0, B, lo, slack)
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), cnt_raw.cpu().numpy())
        return (cnt.cpu().numpy(), plain.cpu().numpy().view(np.uint64), raw.cpu().numpy().view(np.uint64),
                slack.cpu().numpy())

    def finish(self, st):
        torch, B = self.torch, self.B
        idx = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
        dst = torch.full((B, K), float("nan"), dtype=torch.float64, device="cuda")
        st.finish(0, B, idx, dst)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dst.cpu().numpy()

    def full_pass(self, bits, admit_all):
        """(idx, dst, counters) of a whole pass at `bits` index bits, computed once."""
        key = (bits, admit_all)
        if key not in self._passes:
            self.collect(self.st, bits, np.full(self.B, FMAX, np.float32) if admit_all else None)
            idx, dst = self.finish(self.st)
            self._passes[key] = (idx, dst, stats_of(self.ctx))
        return self._passes[key]


_cases = {}


def _case(name, n_samples, order):
    key = (name, n_samples, order)
    if key not in _cases:
        _cases[key] = _Case(name, n_samples, order)
    return _cases[key]


def _check_lists(c, bits, cnt, plain, raw, slack, want_rows):
    """The statements about one set of exported lists; returns the sorted plain entries per row."""
    ib = bits or 17
    cb = 32 - ib
    mask = np.uint64((1 << ib) - 1)
    cap = plain.shape[1]
    hi = slack.astype(np.float64)
    out = []
    for i in range(c.B):
        n = int(cnt[i])
        assert n <= cap, (i, n)
        p, r = plain[i, :n], raw[i, :n]
        # the plain export is the raw one with the code bits cleared, word for word
        assert np.array_equal(p, r & (np.uint64(0xFFFFFFFF00000000) | mask)), (c.name, bits, i)
        assert np.all((p & np.uint64(0xFFFFFFFF)) <= mask)
        rows = (r & mask).astype(np.int64)
        assert np.array_equal(np.sort(rows), np.sort((p & np.uint64(0xFFFFFFFF)).astype(np.int64)))
        if want_rows is not None:
            assert np.array_equal(np.sort(rows), want_rows[i]), (c.name, bits, i)
        # the code decodes to a slack within [slack_j, slack_j (1 + 2^-(cb - 8))] of the candidate row j
        code = ((r & np.uint64(0xFFFFFFFF)) >> np.uint64(ib)).astype(np.uint32)
        s = (code << np.uint32(31 - cb)).view(np.float32).astype(np.float64)
        assert np.all(hi[rows] <= s), (c.name, bits, i)
        assert np.all(s <= hi[rows] * (1.0 + 2.0 ** -(cb - 8))), (c.name, bits, i)
        out.append(np.sort(p))
    return out


@pytest.mark.parametrize("name,n_samples,order", [x for x in CASES if x[2] == "F"])
def test_raw_lists_carry_row_and_slack(name, n_samples, order):
    """(the lists do not depend on the sum order: one order)"""
    c = _case(name, n_samples, order)
    fin = None
    base_all = base_thr = thr = None
    for bits in c.widths:
        # every threshold at FLT_MAX: a row lists exactly the rows of the other chromosomes
        c.collect(c.st, bits, np.full(c.B, FMAX, np.float32))
        cnt, plain, raw, slack = c.exports(c.st)
        assert np.isfinite(slack).all() and (slack >= np.finfo(np.float32).tiny).all()
        want = [np.flatnonzero(c.chrom != c.chrom[i]) for i in range(c.B)]
        assert max(len(w) for w in want) <= plain.shape[1]
        got = _check_lists(c, bits, cnt, plain, raw, slack, want)
        if base_all is None:
            base_all = got
            # thresholds out of the keys: the 5th smallest key itself, the median, just below the smallest
            thr = np.zeros(c.B, np.float32)
            for i, e in enumerate(got):
                u = (e >> np.uint64(32)).astype(np.uint32)
                kb = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
                key = np.sort(kb.view(np.float32))
                thr[i] = key[4] if i % 3 == 0 else (key[len(key) // 2] if i % 3 == 1
                                                    else np.nextafter(key[0], np.float32(-np.inf), dtype=np.float32))
        else:
            assert all(np.array_equal(a, b) for a, b in zip(got, base_all)), (name, bits)
        c.collect(c.st, bits, thr)
        cnt, plain, raw, slack = c.exports(c.st)
        got = _check_lists(c, bits, cnt, plain, raw, slack, None)
        assert all((len(g) >= 5) if i % 3 == 0 else (len(g) >= len(base_all[i]) // 2 if i % 3 == 1 else len(g) == 0)
                   for i, g in enumerate(got))
        if base_thr is None:
            base_thr = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(got, base_thr)), (name, bits)


@pytest.mark.parametrize("admit_all", [False, True])
@pytest.mark.parametrize("name,n_samples,order", CASES)
def test_full_passes_at_every_width(name, n_samples, order, admit_all):
    c = _case(name, n_samples, order)
    want_i, want_d = c.oracle()
    auto = c.full_pass(0, admit_all)
    for bits in c.widths:
        idx, dst, stats = c.full_pass(bits, admit_all)
        print("%s S=%d %s admit_all=%s index bits %d: %s" % (name, n_samples, order, admit_all, bits or 17, stats))
        assert np.array_equal(idx, want_i), (name, bits)
        assert same_bits(dst, want_d), (name, bits)
        assert np.array_equal(idx, auto[0]) and same_bits(dst, auto[1])
        assert stats["fast_rows"] + stats["fallback_rows"] == c.B, stats
        # (the results above are the oracle's at every width, so a differing count would be rows that only a
        # coarser code sends to the exact path; none here)
        assert stats["fallback_rows"] == auto[2]["fallback_rows"], (bits, stats, auto[2])
    # a coarser code never lowers a decoded slack, so U and with it the number of re-scores can only grow
    assert c.full_pass(24, admit_all)[2]["rescored"] >= auto[2]["rescored"]
    assert auto[2]["rescored"] >= c.full_pass(c.need, admit_all)[2]["rescored"]
    if admit_all and name == "pad1280":
        assert auto[2]["fast_rows"] == c.B          # lists of 719 .. 979 entries: the long form, certified


@pytest.mark.parametrize("name,n_samples,order", CASES)
def test_export_import_into_a_second_context(name, n_samples, order):
    """The plain export of one context, imported into a second one prepared at each width, finishes to the direct
    pass's results; a source count above the source capacity still hands the row to the exact path."""
    import torch
    from wisecondor_amd import _lib, distributed
    c = _case(name, n_samples, order)
    direct = c.full_pass(0, False)
    c.collect(c.st, 0, None)
    cap = c.st.cap
    cnt = torch.zeros(c.B, dtype=torch.int32, device="cuda")
    lst = torch.zeros((c.B, cap), dtype=torch.int64, device="cuda")
    thr = torch.zeros(c.B, dtype=torch.float32, device="cuda")
    c.st.export(0, c.B, cap, cnt, lst)
    c.st.get_thr(0, c.B, thr)
    torch.cuda.synchronize()
    marked = np.random.RandomState(5).permutation(c.B)[:MARKED]
    cnt_marked = cnt.clone()
    cnt_marked[torch.from_numpy(marked).cuda()] = cap + 1
    ctx2 = _lib.new_context(0)
    try:
        st2 = distributed.HipStages(ctx2, c.X, c.bins, K, c.sum_order)
        for bits in c.widths:
            for counts, n_marked in ((cnt, 0), (cnt_marked, MARKED)):
                st2.set_index_bits(bits)
                st2.prepare()
                assert st2.index_bits() == (bits or 17)
                st2.set_thr(0, c.B, thr)
                st2.import_(0, c.B, cap, counts, lst)
                idx, dst = c.finish(st2)
                stats = stats_of(ctx2)
                assert np.array_equal(idx, direct[0]) and same_bits(dst, direct[1]), (name, bits, n_marked)
                assert stats["fast_rows"] + stats["fallback_rows"] == c.B, stats
                # (a marked row may be one the direct pass had handed over already)
                fb0 = direct[2]["fallback_rows"]
                assert max(fb0, n_marked) <= stats["fallback_rows"] <= fb0 + n_marked, (stats, direct[2])
                if n_marked == 0:
                    assert stats["fallback_rows"] == fb0
                    if bits == 24:
                        assert stats["rescored"] >= direct[2]["rescored"]
    finally:
        _lib.destroy_context(ctx2)


def test_too_few_index_bits_are_refused():
    """7 bits for 256 padded rows: the prepare says so and the automatic width works again afterwards."""
    from wisecondor_amd import _lib
    c = _case("pad256", 16, "F")
    c.st.set_index_bits(c.need - 1)
    try:
        with pytest.raises(_lib.WisecondorHipError):
            c.st.prepare()
    finally:
        c.st.set_index_bits(0)
    with pytest.raises(_lib.WisecondorHipError):
        c.st.set_index_bits(25)
    c.st.prepare()
    assert c.st.index_bits() == 17
