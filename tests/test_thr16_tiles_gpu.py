"""Tile t of a threshold call on the row band [rb, re) is row panel ib + t / mb x panel t % mb of the sampled rows, with ib
the band's first 128-row panel and mb the number of sampled-row panels (a table today; a form of k_gram_thr16 that
derives the tile from its number was tried beside it: EXPERIMENTS.md).  Whatever spells the tiles out, the thresholds of
a band must be the thresholds the same rows get from a whole-matrix call, bit for bit, wherever the band starts and ends: off every
multiple of 128, one row long, inside the last, partly padded, panel.  Two operand depths (64 samples and fewer: one
k-slab, up to 128: two) and two layouts: 900 bins (M at its floor of 512 sampled rows, four panels, eight row panels)
and 300 bins (M = 384 > bins: the slots beyond the real rows are k_pad_samples')."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

LAYOUTS = {900: [300, 350, 250], 300: [90, 110, 100]}
SAMPLES = [40, 100]        # k_pad16 64 and 128
K = 100
_whole = {}


def bands_of(B):
    last = (B - 1) // 128 * 128           # first row of the last panel
    cand = [(1, 2), (5, 131), (127, 129), (130, 257), (200, B - 23), (B - 1, B), (B - 3, B), (last + 1, B),
            (last - 1, last + 1), (0, 1)]
    return [(rb, re) for rb, re in cand if 0 <= rb < re <= B]


def job(n_bins, n_samples):
    import torch
    from wisecondor_amd import _lib, distributed
    key = (n_bins, n_samples)
    if key not in _whole:
        rng = np.random.RandomState(900 + n_bins + n_samples)
        data = 1.0 + 0.03 * rng.standard_normal((n_bins, n_samples))
        X = torch.from_numpy(data).cuda()
        st = distributed.HipStages(_lib.context(0), X, np.array(LAYOUTS[n_bins], dtype=np.int64), K, _lib.SUM_PAIRWISE)
        st.prepare()
        st.thresholds(0, n_bins)
        out = torch.zeros(n_bins, dtype=torch.float32, device="cuda")
        st.get_thr(0, n_bins, out)
        torch.cuda.synchronize()
        _whole[key] = (X, out.cpu().numpy())
    return _whole[key]


@pytest.mark.parametrize("n_samples", SAMPLES)
@pytest.mark.parametrize("n_bins", sorted(LAYOUTS))
def test_band_thresholds_equal_the_whole_call(n_bins, n_samples):
    import torch
    from wisecondor_amd import _lib, distributed
    X, whole = job(n_bins, n_samples)
    assert np.isfinite(whole).all()
    # (with 512 candidates or fewer a row admits everything, FLT_MAX: every row of the 300-bin layout; the 900-bin
    # rows have 550 .. 650 and take their threshold, a decoded 16-bit key code, from their keys)
    fmax = np.finfo(np.float32).max
    assert (whole == fmax).all() if n_bins < 512 else ((whole < fmax).all() and len(np.unique(whole)) > 1)
    st = distributed.HipStages(_lib.context(0), X, np.array(LAYOUTS[n_bins], dtype=np.int64), K, _lib.SUM_PAIRWISE)
    for rb, re in bands_of(n_bins):
        st.prepare()                       # every row's threshold back at -inf
        st.thresholds(rb, re)
        out = torch.zeros(n_bins, dtype=torch.float32, device="cuda")
        st.get_thr(0, n_bins, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[rb:re].view(np.int32), whole[rb:re].view(np.int32)), (rb, re)
        rest = np.ones(n_bins, dtype=bool)
        rest[rb:re] = False
        assert np.isneginf(got[rest]).all(), (rb, re)
