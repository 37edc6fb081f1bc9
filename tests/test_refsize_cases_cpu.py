"""refsize_cases.py held to what test_newref_refsize_shapes_gpu.py relies on, from the oracle alone: the workgroup
sizes, the pair counts the layouts are designed for, and for every near / copies layout in use that the cluster holds
the k nearest rows of every target row, at distinct distances, in an order that is not the rows' own, with the far rows
well outside."""
import numpy as np
import pytest

import refsize_cases as rc

ORDERS = ("F", "C")


def test_ps_of_on_the_table_edges():
    want = {1: 128, 100: 128, 101: 192, 164: 192, 165: 256, 228: 256, 229: 320, 256: 320}
    assert {k: rc.ps_of(k) for k in want} == want
    assert [rc.ps_of(k) // 64 for k in (100, 164, 228, 256)] == [2, 3, 4, 5]
    # every refsize of the fast path: ps is whole waves, holds k pairs in one trip, and RMAX pairs in at most four
    for k in range(1, 257):
        ps = rc.ps_of(k)
        assert ps % 64 == 0 and ps >= k + 28 and -(-rc.RMAX // ps) <= 4
    # the refsizes in use sit on both edges of every workgroup size
    used = set(rc.FEW_B) | set(rc.NEAR_M) | set(rc.NEAR_M_SMALL)
    assert {100, 101, 164, 165, 228, 229, 256} <= used


def test_few_cases_are_below_k_on_both_sides():
    # the first pair of the last wave in use, and the pass / DMA-group edges of that wave with a case on either side
    last_wave = {164: (128, (8, 16)), 228: (192, (8, 16)), 256: (192, (8, 16, 32, 48))}
    assert set(rc.FEW_B) == set(last_wave)
    for k, bs in rc.FEW_B.items():
        for b in bs:
            assert rc.T_ROWS < k and b < k and b < rc.ps_of(k)                 # one trip
            assert rc.designed("few", (rc.T_ROWS, b), k) == (2 * rc.T_ROWS * b, 0)
            data, bins = rc.few(rc.T_ROWS, b)
            assert data.shape == (rc.T_ROWS + b, 100) and bins == (rc.T_ROWS, b) and not data.flags.writeable
        first, edges = last_wave[k]
        assert first == 64 * ((k - 1) // 64)                                   # the wave of the last pair below k
        pairs = {b - first for b in bs}
        for e in edges:
            assert {e, e + 1} <= pairs, (k, e)
        assert 1 in pairs and k - 1 in bs


@pytest.mark.parametrize("k,args", rc.near_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_near_layouts(k, args):
    m = args[0]
    far = args[1] if len(args) > 1 else rc.FAR
    T = args[2] if len(args) > 2 else rc.T_ROWS
    data, bins = rc.near(*args)
    assert bins == (T, m + far) and data.shape[0] == T + m + far and not data.flags.writeable
    assert m >= k
    if k in rc.NEAR_M_SMALL:
        assert T >= k                                # no designed count for the rows of chromosome 2
    else:
        rescored, fallback = rc.designed("near", args, k)
        assert T < k and fallback == (T if m > rc.RMAX else 0)
        assert rescored == (T * m if m <= rc.RMAX else 0) + (m + far) * T
    seen_unordered = 0
    for order in ORDERS:
        pos, dst = rc.target_view("near", args, order)
        idx, dist = rc.oracle("near", args, k, order)
        # the view is the oracle's own answer, carried on to every candidate
        assert np.array_equal(idx[:T], pos[:, :k]) and np.array_equal(dist[:T], dst[:, :k])
        # the cluster holds the answer: the m nearest of every target row are the cluster, so the k nearest are in it
        assert (pos[:, :m] < m).all() and (pos[:, m:] >= m).all()
        assert (idx[:T] < m).all() and (idx[:T] >= 0).all()
        # distinct distances, among the k and among the whole cluster
        assert (np.diff(dst[:, :m], axis=1) > 0).all()
        # far rows stay outside
        ratio = float((dst[:, m] / dst[:, m - 1]).min())
        spread = float(((dst[:, m - 1] - dst[:, 0]) / dst[:, 0]).max())
        print("k %d %s order %s: far ratio %.3f, cluster spread %.2e" % (k, args, order, ratio, spread))
        assert ratio >= rc.FAR_RATIO
        assert spread < 1e-3                         # far below the float16 allowance of the bound (2^-12 per row)
        # the order is not by position
        if m >= 2:
            if k >= 8:                               # no target row's answer is in ascending position
                asc = np.array([np.array_equal(r, np.sort(r)) for r in idx[:T]])
                assert not asc.any()
            else:                                    # (k = 1, 2) the answer is not the cluster's first rows
                asc = (idx[:T] == np.arange(k)).all(axis=1)
                assert not asc.all()
            seen_unordered += int((~asc).sum())
        # the rows of chromosome 2 see the T target rows
        if T < k:
            assert (idx[T:, :T] >= 0).all() and (idx[T:, T:] == -1).all() and (dist[T:, T:] == 1e10).all()
    assert seen_unordered > 0 or m == 1


@pytest.mark.parametrize("k,m", rc.COPIES_KM)
def test_copies_layouts(k, m):
    data, bins = rc.copies(m)
    T = rc.T_ROWS
    assert bins == (T, m + rc.FAR) and (data[T:T + m] == 1.0).all() and not data.flags.writeable
    assert np.array_equal(data[:T], rc.near(m)[0][:T]) and np.array_equal(data[T + m:], rc.near(m)[0][T + m:])
    assert T < k < m <= rc.RMAX and m > rc.ps_of(k)          # a second trip, and a strided tie sweep
    assert rc.designed("copies", (m,), k) == (T * m + (m + rc.FAR) * T, 0)
    for order in ORDERS:
        pos, dst = rc.target_view("copies", (m,), order)
        idx, dist = rc.oracle("copies", (m,), k, order)
        assert np.array_equal(idx[:T], np.tile(np.arange(k), (T, 1)))      # ties: the first k positions of the cluster
        assert (dst[:, :m] == dst[:, :1]).all()
        assert np.array_equal(pos[:, :m], np.tile(np.arange(m), (T, 1)))
        assert float((dst[:, m] / dst[:, m - 1]).min()) >= rc.FAR_RATIO


def test_case_tables():
    assert rc.NEAR_M[100] == (385,)
    for k, ms in list(rc.NEAR_M.items()) + list(rc.NEAR_M_SMALL.items()):
        assert min(ms) == k or k == 100
    # RMAX and one pair more at the first refsize of every workgroup size above two waves, and at the last
    for k in (101, 165, 229, 256):
        assert 512 in rc.NEAR_M[k] and 513 in rc.NEAR_M[k]
    # the largest dynamic LDS request of k_rescore: the target row and five wave slabs
    m, far, T, samples = rc.BIG_LDS_ARGS[0]
    assert samples == 2048 and rc.ps_of(rc.BIG_LDS_K) == 320 and 8 * samples + (320 // 64) * 8192 == 16384 + 40960
    assert rc.BIG_LDS_ARGS[1][3] == 2047
    # LEAN: more than 512 list entries
    assert rc.LEAN_ARGS[0] + rc.LEAN_ARGS[1] > 512 and rc.LEAN_ARGS[0] <= rc.RMAX
    assert rc.designed("near", rc.LEAN_ARGS, 101) == (70 * 300 + 600 * 70, 0)
