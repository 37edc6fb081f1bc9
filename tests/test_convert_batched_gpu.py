"""k_convert at every block shape of its sample loop: half a wave reads a row in blocks of four iterations of 32
samples, so 1 / 7 / 8 / 31 samples are a part of the first iteration, 32 / 33 its end and the start of the second,
100 / 127 / 128 / 129 the end of the first block and the start of the second, 600 five blocks with a short last one.
The whole `newref` is held against the oracle bit for bit in both memory orders, and the exported lists against the
bound that k_convert's norms exist for: a listed key is a LOWER bound of the pair's float64 distance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wc_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

BINS = np.array([90, 110, 100], dtype=np.int64)
SAMPLES = [1, 7, 8, 31, 32, 33, 100, 127, 128, 129, 600]
ORDERS = ["F", "C"]
K = 100
_data = {}


def data_of(n_samples):
    if n_samples not in _data:
        rng = np.random.RandomState(300 + n_samples)
        _data[n_samples] = 1.0 + 0.03 * rng.standard_normal((int(BINS.sum()), n_samples))
    return _data[n_samples]


def laid_out(data, order):
    return np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_samples", SAMPLES)
def test_newref_matches_the_oracle(n_samples, order):
    from wisecondor_amd import wisetools
    lay = laid_out(data_of(n_samples), order)
    sums = np.cumsum(BINS)
    idx, dst = wisetools.getReference(lay, BINS, sums, K)
    with np.errstate(all="ignore"):
        want_i, want_d = wo.get_reference(lay, BINS, sums, K, 1, 1, fast=True)
    assert np.array_equal(idx, want_i)
    assert same_bits(dst, want_d)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_samples", SAMPLES)
def test_listed_keys_are_lower_bounds(n_samples, order):
    """The lists at the thresholds the pass itself takes from its sampled keys: every listed key (float32) is at or
    below the float64 distance of its pair as the oracle sums it."""
    import torch
    from wisecondor_amd import _lib, distributed
    data = data_of(n_samples)
    B = data.shape[0]
    X = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    st = distributed.HipStages(_lib.context(0), X, BINS, K, _lib.SUM_SEQUENTIAL if order == "F" else _lib.SUM_PAIRWISE)
    st.prepare()
    st.thresholds(0, B)
    st.collect(0, B, 0, 1)
    cap = st.cap
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    lst = torch.zeros((B, cap), dtype=torch.int64, device="cuda")
    st.export(0, B, cap, cnt, lst)
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    ent = lst.cpu().numpy().view(np.uint64)
    lay = laid_out(data, order)
    chrom = np.repeat(np.arange(len(BINS)), BINS)
    listed = 0
    for i in range(B):
        n = int(cnt[i])
        assert n <= cap, (i, n)
        e = ent[i, :n]
        j = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
        u = (e >> np.uint64(32)).astype(np.uint32)
        key = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
        assert (chrom[j] != chrom[i]).all(), i
        dist = np.sum(np.power(laid_out(lay[j, :], order) - lay[i, :], 2), 1)
        assert (key.astype(np.float64) <= dist).all(), (n_samples, order, i)
        listed += n
    assert listed > 0
