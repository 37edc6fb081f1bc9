"""The 32-bit rank image of a row's distance keys on the host (wc_order_key_host: order_key32 of csrc/common.h, the
function k_rescore's counting order ranks on, compiled for the host).  The order of a row is decided on the image
alone wherever all images differ, so the image must never invert two keys; equal images only cost a second sweep."""
import numpy as np
import pytest

TOP = 0xFFFFFFFF                          # an entry without a distance (key ~0: NaN or >= 1e10)
SAT = 0xFFFFFFFE                          # every key 2^(32 + shift) or more above the anchor
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SHIFTS = [-1, 0, 1, 8, 23, 24, 25, 31, 32]


def image(key, shift=-1):
    from wisecondor_amd import _lib
    key = np.ascontiguousarray(key, dtype=np.uint64)
    out = np.zeros(key.shape, dtype=np.uint32)
    mn = np.zeros(1, dtype=np.uint32)
    _lib.check(_lib.load().wc_order_key_host(_lib.ptr(key), key.size, shift, _lib.ptr(out), _lib.ptr(mn)))
    return out, int(mn[0])


def ordered(d):
    """float64 -> the order-preserving key (f64_ordered), ~0 for NaN and >= 1e10 as k_rescore forms it"""
    d = np.ascontiguousarray(d, dtype=np.float64)
    b = d.view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    key[~(d < 1e10)] = NONE
    return key


def rows():
    """key sets: random distances of one row (a few binades), log-uniform over 80 binades, random 64-bit patterns,
    neighbours in the last bits, entries without a distance among them, a row of nothing else, single keys"""
    rng = np.random.RandomState(11)
    out = [ordered(rng.uniform(0.8, 1.3, 500) ** 2 * 0.09),
           ordered(np.exp(rng.uniform(np.log(1e-14), np.log(9.9e9), 500))),
           ordered(np.concatenate([[0.0, 9.9e9, 1e10, np.nan, np.inf], rng.uniform(0, 1e-3, 100)])),
           rng.randint(0, 2 ** 62, 500).astype(np.uint64) * np.uint64(4) + rng.randint(0, 4, 500).astype(np.uint64),
           np.uint64(0x8000000000000000) + np.arange(0, 3000, 7).astype(np.uint64) * np.uint64(2 ** 22 + 1),
           np.array([NONE, NONE, NONE]), np.array([np.uint64(12345)]), np.array([NONE])]
    near = ordered([0.25])[0] + np.concatenate([np.arange(40), 2 ** np.arange(6, 62)]).astype(np.uint64)
    out.append(near)
    mixed = out[0].copy()
    mixed[::9] = NONE
    out.append(mixed)
    return out


def reference(key, sh):
    """the rule in Python integers"""
    mn = min(int(v) >> 32 for v in key)
    ref = []
    for v in key:
        v = int(v)
        ref.append(TOP if v == int(NONE) else min((v - (mn << 32)) >> sh, SAT))
    return np.array(ref, dtype=np.uint64), mn


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_rule(shift):
    sh = 24 if shift < 0 else shift                  # -1 is the kernel's own shift
    for key in rows():
        r, mn = image(key, shift)
        want, want_mn = reference(key, sh)
        assert mn == want_mn and np.array_equal(r.astype(np.uint64), want)
        # monotone: sorted by key, the images never descend
        by_key = np.argsort(key, kind="stable")
        assert np.all(np.diff(r[by_key].astype(np.int64)) >= 0)
        # entries without a distance, and only they, carry the top code
        assert np.array_equal(r == TOP, key == NONE)
        # saturation only at the top: below the held code the image is the shifted offset itself, and whatever
        # carries the held code lies at or beyond it
        valid = key != NONE
        off = np.array([(int(v) - (mn << 32)) >> sh for v in key[valid]], dtype=object)
        assert all((ri == o) if o < SAT else (ri == SAT) for ri, o in zip(r[valid].tolist(), off.tolist()))
        # distinct images imply the order of the keys: ranking on the image IS ranking on the key
        if len(set(r.tolist())) == len(r):
            assert np.array_equal(np.argsort(r, kind="stable"), by_key)
        # ... and in any row, two keys with different images are ordered as their images
        i, j = np.triu_indices(min(len(key), 120), 1)
        differ = r[i] != r[j]
        assert np.array_equal((r[i] < r[j])[differ], (key[i] < key[j])[differ])


def test_the_kernels_shift_is_24():
    """bit 24 of the key is the lowest that moves the image: 2^-28 relative resolution of a float64 distance"""
    base = ordered([5.0])[0]
    key = np.array([base, base + np.uint64(1 << 23), base + np.uint64(1 << 24), base + np.uint64((1 << 24) - 1)])
    r, mn = image(key)
    assert mn == int(base) >> 32
    assert r[0] == r[1] == r[3] and r[2] == r[0] + 1
    # sixteen binades above the anchor's high word the image is held
    far = np.array([ordered([1.0])[0], ordered([2.0 ** 15 * 1.999])[0], ordered([2.0 ** 16])[0], ordered([9.9e9])[0]])
    r, _ = image(far)
    assert r[0] == 0 and r[1] < SAT and r[2] == SAT and r[3] == SAT


def test_arguments_are_checked():
    from wisecondor_amd import _lib
    lib = _lib.load()
    key = np.array([1, 2], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint32)
    mn = np.zeros(1, dtype=np.uint32)
    good = (_lib.ptr(key), 2, 24, _lib.ptr(out), _lib.ptr(mn))
    assert lib.wc_order_key_host(*good) == 0
    for at, bad in ((0, None), (3, None), (4, None), (1, -1), (2, -2), (2, 33)):
        args = list(good)
        args[at] = bad
        assert lib.wc_order_key_host(*args) == _lib.E_ARG
    # an empty row: nothing written but the identity of the minimum
    assert lib.wc_order_key_host(_lib.ptr(key), 0, -1, _lib.ptr(out), _lib.ptr(mn)) == 0 and mn[0] == TOP
