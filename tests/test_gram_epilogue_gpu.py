"""The candidate lists of the distance tiles (k_gram_glds and its epilogue), held against themselves:
with every threshold at FLT_MAX a row's list must be exactly the rows of the other chromosomes that have a
finite norm bound, and with any other thresholds it must be the sub-level set of those same keys, bit for bit.
Nothing here depends on how the epilogue is organised: the statements are about the exported lists alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = {
    # boundaries off every multiple of 4 / 32 / 64 / 128, chromosomes of 1 and 3 rows, chromosomes across panel edges
    "ragged": [70, 3, 129, 1, 60, 200],
    # aligned: the diagonal tiles are all same-chromosome and skipped
    "aligned": [128, 128, 128],
    # 770 rows: the last panel holds 2
    "tail2": [5, 250, 5, 250, 5, 250, 5],
    # lists of 23 and of 1 000 entries, just under the capacity
    "nearcap": [1000, 23],
}
SAMPLES = [16, 40, 100]           # one 32-sample slab, two with a short last one, four
# rows that must never be listed and never list anything: one holds a NaN, one 1e300.  (Neither is among the
# rows the per-sample centre is taken from -- every third row here -- so that the other rows keep their bounds.)
SPECIAL = {"ragged": (71, 200)}
CASES = [(name, s) for name in LAYOUTS for s in SAMPLES]
FMAX = np.finfo(np.float32).max


def _decode(entries):
    """Packed list entries -> (float32 keys, ordered key codes, candidate rows)."""
    e = np.asarray(entries).view(np.uint64)
    j = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
    u = (e >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return bits.view(np.float32), u, j


class _Case(object):
    """One matrix on the GPU, its admit-all lists (test 1) and the thresholded ones (test 2), computed once."""

    def __init__(self, name, n_samples):
        import torch
        from wisecondor_amd import _lib, distributed
        self.torch = torch
        self.name = name
        self.bins = np.asarray(LAYOUTS[name], dtype=np.int64)
        self.B = int(self.bins.sum())
        rng = np.random.RandomState(100 * sorted(LAYOUTS).index(name) + n_samples)
        data = 1.0 + 0.03 * rng.standard_normal((self.B, n_samples))
        if name in SPECIAL:
            data[SPECIAL[name][0], n_samples // 2] = np.nan
            data[SPECIAL[name][1], 1] = 1e300
        self.chrom = np.repeat(np.arange(len(self.bins)), self.bins)
        self.X = torch.from_numpy(data).cuda()
        self.job = distributed.NewrefJob(_lib.context(0), self.X, self.bins, 100, _lib.SUM_SEQUENTIAL)
        self.st = self.job.st
        self.admit = None
        self.thr = None
        self.listed = None

    def lists(self, thr, rb=0, re=None, tile_rank=0, tile_ranks=1):
        """prepare / thresholds / set_thr / collect / export -> (cnt, entries[B][cap] as uint64, cap, lower bounds)."""
        torch, st, B = self.torch, self.st, self.B
        st.prepare()
        st.thresholds(0, B)
        t = torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).cuda()
        st.set_thr(0, B, t)
        st.collect(rb, B if re is None else re, tile_rank, tile_ranks)
        cap = st.cap
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        lst = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
        st.export(0, B, cap, cnt, lst)
        lo = torch.zeros(B, dtype=torch.float32, device="cuda")
        slack = torch.zeros(B, dtype=torch.float32, device="cuda")
        st.get_bounds(0, B, lo, slack)
        torch.cuda.synchronize()
        return cnt.cpu().numpy(), lst.cpu().numpy().view(np.uint64), cap, lo.cpu().numpy()

    def expected_candidates(self, lo):
        fin = np.isfinite(lo)
        return [np.flatnonzero(fin & (self.chrom != self.chrom[i])) if fin[i] else np.zeros(0, np.int64)
                for i in range(self.B)]

    def admit_all(self):
        """Test 1's lists, checked on the way, and the key table they define: K[i] = (keys, codes, rows) of row i,
        sorted by candidate row."""
        if self.admit is not None:
            return self.admit
        cnt, lst, cap, lo = self.lists(np.full(self.B, FMAX, np.float32))
        want = self.expected_candidates(lo)
        assert max(len(w) for w in want) <= cap
        n_special = len(SPECIAL.get(self.name, ()))
        assert int(np.isfinite(lo).sum()) == self.B - n_special       # the plain rows all have bounds
        for r in SPECIAL.get(self.name, ()):
            assert not np.isfinite(lo[r]) and cnt[r] == 0, (self.name, r)
        K = []
        for i in range(self.B):
            assert cnt[i] == len(want[i]), (self.name, i, int(cnt[i]), len(want[i]))
            key, code, j = _decode(lst[i, :cnt[i]])
            at = np.argsort(j, kind="stable")
            assert np.array_equal(j[at], want[i]), (self.name, i)      # exactly that set, each once
            assert np.isfinite(key).all(), (self.name, i)
            K.append((key[at], code[at], j[at]))
        self.admit = K
        return K

    def thresholds(self):
        """Per-row thresholds out of the key table and the lists they must produce (sorted packed entries)."""
        if self.thr is not None:
            return self.thr, self.listed
        K = self.admit_all()
        thr = np.zeros(self.B, np.float32)
        listed = []
        for i, (key, code, j) in enumerate(K):
            if len(key):
                s = np.sort(key)
                if i % 3 == 0:
                    thr[i] = s[4]                       # the 5th smallest key exactly: equality must pass
                elif i % 3 == 1:
                    thr[i] = s[len(s) // 2]
                else:
                    thr[i] = np.nextafter(s[0], np.float32(-np.inf), dtype=np.float32)
            keep = key <= thr[i]
            listed.append(np.sort((code[keep].astype(np.uint64) << np.uint64(32)) | j[keep].astype(np.uint64)))
            if len(key):
                n = int(keep.sum())
                assert (n >= 5) if i % 3 == 0 else (n >= len(key) // 2 if i % 3 == 1 else n == 0)
        self.thr, self.listed = thr, listed
        return thr, listed


_cases = {}


def _case(name, n_samples):
    key = (name, n_samples)
    if key not in _cases:
        _cases[key] = _Case(name, n_samples)
    return _cases[key]


def _row_entries(cnt, lst, cap, i):
    assert cnt[i] <= cap, (i, int(cnt[i]))
    return np.sort(lst[i, :cnt[i]])


@pytest.mark.parametrize("name,n_samples", CASES)
def test_admit_all_lists_are_complete_and_exact(name, n_samples):
    """Every threshold at FLT_MAX: cnt is the number of rows on other chromosomes with a finite lower bound, the
    listed candidates are exactly those rows, each once; a row without a finite bound of its own lists nothing."""
    K = _case(name, n_samples).admit_all()
    assert sum(len(k[0]) for k in K) > 0


@pytest.mark.parametrize("name,n_samples", CASES)
def test_thresholded_lists_are_sublevel_sets(name, n_samples):
    """Per-row thresholds taken from the admit-all keys (the 5th smallest key itself, the median, just below the
    smallest): every list is {(K[i][j], j) : K[i][j] <= thr_i} with the key bits of the admit-all pass."""
    c = _case(name, n_samples)
    thr, listed = c.thresholds()
    cnt, lst, cap, _ = c.lists(thr)
    for i in range(c.B):
        assert cnt[i] == len(listed[i]), (name, i, int(cnt[i]), len(listed[i]))
        assert np.array_equal(_row_entries(cnt, lst, cap, i), listed[i]), (name, i)


@pytest.mark.parametrize("n_samples", SAMPLES)
def test_row_bands_and_tile_ranks(n_samples):
    """collect over a row band fills that band's lists completely; the tiles dealt to three ranks give three
    disjoint parts of every list."""
    c = _case("tail2", n_samples)
    thr, listed = c.thresholds()
    cnt, lst, cap, _ = c.lists(thr, 100, 300)
    for i in range(100, 300):
        assert np.array_equal(_row_entries(cnt, lst, cap, i), listed[i]), i
    parts = [c.lists(thr, 0, c.B, r, 3) for r in range(3)]
    for i in range(c.B):
        got = np.concatenate([_row_entries(p[0], p[1], cap, i) for p in parts])
        assert len(got) == len(listed[i]), i                       # disjoint ...
        assert np.array_equal(np.sort(got), listed[i]), i          # ... and their union is the whole list


def test_overflow_keeps_the_count():
    """More passing entries than the list holds: cnt still counts them all (that is what sends the row to the
    exact path) and the slots below the capacity hold distinct rows of the other chromosome."""
    import torch
    from wisecondor_amd import _lib, distributed
    bins = np.array([1200, 1200], dtype=np.int64)
    B = 2400
    rng = np.random.RandomState(77)
    X = torch.from_numpy(1.0 + 0.03 * rng.standard_normal((B, 16))).cuda()
    job = distributed.NewrefJob(_lib.context(0), X, bins, 100, _lib.SUM_SEQUENTIAL)
    st = job.st
    st.prepare()
    st.thresholds(0, B)
    st.set_thr(0, B, torch.full((B,), float(FMAX), dtype=torch.float32, device="cuda"))
    st.collect(0, B, 0, 1)
    cap = st.cap
    assert cap < 1200
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    lst = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
    st.export(0, B, cap, cnt, lst)
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    assert (cnt == 1200).all(), (int(cnt.min()), int(cnt.max()))
    j = (lst.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    other_lo = np.where(np.arange(B) < 1200, 1200, 0)[:, None]
    assert ((j >= other_lo) & (j < other_lo + 1200)).all()
    js = np.sort(j, axis=1)
    assert (js[:, 1:] != js[:, :-1]).all()
