"""k_pick at chosen list lengths: two chromosomes, every threshold at FLT_MAX, so that a row's list is exactly the
other chromosome.  The sizes put a wave of the short form (lists up to 512 entries, eight per lane), of the long form
(up to the capacity, sixteen per lane) and of the hand-over to the exact path (more entries than the list holds) in
front of an empty, a partly filled and a full group of 64 entries: every gather of the selection is an unconditional
load of a selected index, and these are the lengths at which a wrong selection reads a slot that was never written.
The output is held against the oracle bit for bit and the number of exact-path rows against what the sizes imply."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(100, 101), (127, 129), (128, 384), (511, 513), (512, 577), (640, 1023), (1024, 1025)]
S = 100
K = 100
FMAX = np.finfo(np.float32).max


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def run_admit_all(data, bins):
    """prepare / thresholds / every threshold FLT_MAX / collect / finish -> (idx, dst, counters, list capacity)."""
    import torch
    from wisecondor_amd import _lib, distributed, wisetools
    B = data.shape[0]
    X = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    st = distributed.HipStages(_lib.context(0), X, np.asarray(bins, dtype=np.int64), K, _lib.SUM_SEQUENTIAL)
    st.prepare()
    st.thresholds(0, B)
    st.set_thr(0, B, torch.full((B,), float(FMAX), dtype=torch.float32, device="cuda"))
    st.collect(0, B, 0, 1)
    idx = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    dst = torch.full((B, K), float("nan"), dtype=torch.float64, device="cuda")
    st.finish(0, B, idx, dst)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dst.cpu().numpy(), wisetools.newref_stats(0), st.cap


def oracle(data, bins):
    with np.errstate(all="ignore"):
        return wo.get_reference(np.asfortranarray(data), np.asarray(bins), np.cumsum(bins), K, 1, 1, fast=True)


@pytest.mark.parametrize("a,b", SIZES)
def test_list_lengths_around_the_groups(a, b):
    rng = np.random.RandomState(1000 * a + b)
    data = 1.0 + 0.03 * rng.standard_normal((a + b, S))
    idx, dst, stats, cap = run_admit_all(data, [a, b])
    print("sizes (%d, %d): %s, capacity %d" % (a, b, stats, cap))
    want_i, want_d = oracle(data, [a, b])
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    # a row of the first chromosome lists the b rows of the second and the other way round; a list of more
    # entries than the capacity has lost some, and only such a row is handed to the exact path
    implied = (a if b > cap else 0) + (b if a > cap else 0)
    assert stats["fast_rows"] + stats["fallback_rows"] == a + b, stats
    assert stats["fallback_rows"] == implied, (stats, implied)


def test_clamped_row_takes_the_bad_norm_branch():
    """One value of 1e9: that row has no float16 image, is listed nowhere and goes to the exact path by itself;
    every other row is certified against its norm (the bad_norm test behind the bisection) and stays fast."""
    a, b = 100, 101
    rng = np.random.RandomState(7)
    data = 1.0 + 0.03 * rng.standard_normal((a + b, S))
    data[150, 40] = 1e9            # (not among the rows the per-sample centre is taken from: the first 128 here)
    idx, dst, stats, cap = run_admit_all(data, [a, b])
    print("clamped row: %s" % (stats,))
    want_i, want_d = oracle(data, [a, b])
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)
    assert (idx[150] == -1).all()                      # its distances are beyond the sentinel
    assert stats["fast_rows"] + stats["fallback_rows"] == a + b, stats
    assert stats["fallback_rows"] == 1, stats
