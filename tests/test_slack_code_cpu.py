"""The slack code of a list entry on the host (wc_slack_code_host: the function k_convert packs with, compiled for the
host): a candidate's slack rides above its row number in the entry's low word, rounded UP to the top cb of the float's
31 non-sign bits.  k_pick forms its upper bound U from the decoded value, so the decoded value must never be below the
slack (a larger one only re-scores a few more candidates), must stay within the promised factor, and the two fields of
the word must not touch."""
import numpy as np
import pytest

FMAX = np.finfo(np.float32).max
TINY = np.float32(2.0 ** -126)          # smallest normal
CBS = list(range(8, 16))


def code(x, cb):
    from wisecondor_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.zeros(x.shape, dtype=np.uint32)
    d = np.zeros(x.shape, dtype=np.float32)
    _lib.check(_lib.load().wc_slack_code_host(_lib.ptr(x), x.size, cb, _lib.ptr(c), _lib.ptr(d)))
    return c, d


@pytest.fixture(scope="module")
def values():
    """10^5 positive floats with uniformly drawn bit patterns (every exponent, subnormals included), ascending, with
    0, the smallest subnormal, FLT_MAX and +inf."""
    rng = np.random.RandomState(20)
    bits = rng.randint(1, 0x7F800000, size=100000).astype(np.uint32)
    special = np.array([0, 1, 0x7F7FFFFF, 0x7F800000], dtype=np.uint32)
    return np.sort(np.concatenate([bits, special])).view(np.float32)


@pytest.mark.parametrize("cb", CBS)
def test_decoded_slack_bounds(values, cb):
    c, d = code(values, cb)
    assert c.max() < (1 << cb)
    assert np.all(d >= values)
    assert d[-1] == np.inf and values[-1] == np.inf
    assert c[0] == 0 and d[0] == 0.0
    # monotone (the values ascend)
    assert np.all(np.diff(c.astype(np.int64)) >= 0)
    assert np.all(np.diff(d[np.isfinite(d)].astype(np.float64)) >= 0)
    # at most 1 + 2^-(cb - 8) times a normal slack (cb = 8: 2 x).  The product is formed in float32, the format the
    # decoded value lives in: in the topmost bucket below +inf (FLT_MAX is in it) the bound itself overflows to +inf,
    # which is what the code gives there ("a carry into the exponent is the next power of two").  The rounding of
    # the product cannot hide an excess: decoded <= x + (2^(31 - cb) - 1) ulp(x) and x 2^-(cb - 8) >= 2^(31 - cb)
    # ulp(x), so the exact product lies a whole ulp above any decoded value that obeys the bound.
    normal = (values >= TINY) & np.isfinite(values)
    with np.errstate(over="ignore"):
        bound = values[normal] * np.float32(1.0 + 2.0 ** -(cb - 8))
    assert bound.dtype == np.float32
    assert np.all(d[normal] <= bound)
    finite = np.isfinite(bound)
    assert finite.sum() > 99000          # (the overflow case is the topmost bucket only)
    assert np.all(d[normal][finite].astype(np.float64) <=
                  values[normal][finite].astype(np.float64) * (1.0 + 2.0 ** -(cb - 8)))
    # exactly representable slacks (the low 31 - cb bits clear) are kept as they are
    exact = (values.view(np.uint32) & np.uint32((1 << (31 - cb)) - 1)) == 0
    assert np.array_equal(d[exact], values[exact])


@pytest.mark.parametrize("cb", CBS)
def test_fields_do_not_leak(cb):
    """row | code << index_bits with every index bit set next to EVERY code: both fields come back."""
    index_bits = 32 - cb
    codes = np.arange(1 << cb, dtype=np.uint32)
    # every code is reachable: the decoded value of a code encodes to that code
    d = (codes << np.uint32(31 - cb)).view(np.float32)
    ok = ~np.isnan(d)                    # (codes beyond +inf's are never produced)
    c2, d2 = code(d[ok], cb)
    assert np.array_equal(c2, codes[ok]) and np.array_equal(d2.view(np.uint32), d[ok].view(np.uint32))
    mask = np.uint32((1 << index_bits) - 1)
    for row in (mask, np.uint32(0), np.uint32(1 << (index_bits - 1))):
        word = row | (codes << np.uint32(index_bits))
        assert np.array_equal(word & mask, np.full(codes.shape, row, dtype=np.uint32))
        assert np.array_equal(word >> np.uint32(index_bits), codes)
        # the decode k_pick uses: the code sits one bit left of where the float's bits belong
        assert np.array_equal((word >> np.uint32(1)) & ~(mask >> np.uint32(1)), codes << np.uint32(31 - cb))


def test_arguments_are_checked():
    from wisecondor_amd import _lib
    lib = _lib.load()
    x = np.array([-1.0], dtype=np.float32)
    c = np.zeros(1, dtype=np.uint32)
    d = np.zeros(1, dtype=np.float32)
    assert lib.wc_slack_code_host(_lib.ptr(x), 1, 15, _lib.ptr(c), _lib.ptr(d)) == _lib.E_ARG
    x[0] = 1.0
    assert lib.wc_slack_code_host(_lib.ptr(x), 1, 0, _lib.ptr(c), _lib.ptr(d)) == _lib.E_ARG
    assert lib.wc_slack_code_host(_lib.ptr(x), 1, 32, _lib.ptr(c), _lib.ptr(d)) == _lib.E_ARG
    ctx_free = lib.wc_newref_set_index_bits(None, 17)
    assert ctx_free == _lib.E_ARG
