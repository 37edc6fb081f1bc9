"""Inputs of the exportjson tests: the doubles the digit routine is tried on, what CPython writes for them, and
synthetic result files.  Everything here is made once and shared (functools.lru_cache); callers do not modify it."""
import functools
import json

import numpy as np

SUBNORMAL = 2.0 ** -1074


@functools.lru_cache(maxsize=None)
def digit_inputs():
    """float64 array: the issue's list."""
    rng = np.random.RandomState(20261020)
    parts = []
    # one million uniformly random 64-bit patterns
    lo = rng.randint(0, 1 << 32, size=1000000, dtype=np.uint64)
    hi = rng.randint(0, 1 << 32, size=1000000, dtype=np.uint64)
    parts.append(((hi << np.uint64(32)) | lo).view(np.float64))
    # every power of two of the 2 046 normal exponents with its two neighbours
    p2 = np.ldexp(1.0, np.arange(-1022, 1024))
    assert len(p2) == 2046 and p2[0] == 2.2250738585072014e-308 and np.isfinite(p2[-1])
    parts += [p2, np.nextafter(p2, np.inf), np.nextafter(p2, -np.inf)]
    # every power of ten from 1e-323 to 1e308 with its neighbours
    p10 = np.array([float("1e%d" % e) for e in range(-323, 309)])
    parts += [p10, np.nextafter(p10, np.inf), np.nextafter(p10, -np.inf)]
    named = [SUBNORMAL * k for k in (1, 2, 3, 2 ** 51, 2 ** 52 - 1)]
    named += [1.7976931348623157e308, 2.0 ** 53, 2.0 ** 53 + 2, 0.1 + 0.2, 1e15, 1e16, 1e16 + 2, 1e-4, 1e-5, 1e22, 1e23,
              123456789012345.6, 0.0, -0.0, float("inf"), -float("inf")]
    parts.append(np.array(named, dtype=np.float64))
    # NaN with either sign and a payload
    parts.append(np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff4000000abcdef, 0x7fffffffffffffff],
                          dtype=np.uint64).view(np.float64))
    # 200 000 result-like values: z-scores, ratios near 1, values k / 100, whole numbers
    parts.append(rng.standard_normal(50000))
    parts.append(1.0 + 0.02 * rng.standard_normal(50000))
    parts.append(rng.randint(-100000, 100000, size=50000) / 100.0)
    parts.append(rng.randint(-1000000, 1000000, size=50000).astype(np.float64))
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])


@functools.lru_cache(maxsize=None)
def digit_expected(strict):
    """What CPython writes for digit_inputs(), as a fixed-width bytes array ('S24'); with strict, null where it is not
    finite.  json.dumps of the list is float.__repr__ of every element, the same as json.dumps([x])[1:-1]."""
    values = digit_inputs()
    texts = json.dumps(values.tolist(), separators=(",", ":"))[1:-1].split(",")
    assert len(texts) == len(values) and max(len(t) for t in texts) <= 24
    for x in (0.1 + 0.2, -0.0, 5e-324):
        assert json.dumps([x])[1:-1] == repr(x)
    if strict:
        texts = ["null" if t in ("NaN", "Infinity", "-Infinity") else t for t in texts]
    return np.array([t.encode("ascii") for t in texts], dtype="S24")


SIZES = [37, 0, 1, 255, 256, 257, 12, 5, 9, 30, 2, 3, 511, 512, 513, 7, 7, 7, 1, 4, 8, 16]      # 22 chromosomes


def _function_stored_by_reference(args):
    return args


def synthetic_result(seed, sizes=None, n_calls=3):
    """A result file's content as a dict: 22 chromosomes by default, one of length 0 and one of length 1, calls, and -0.0,
    inf and NaN among the values."""
    sizes = SIZES if sizes is None else sizes
    rng = np.random.RandomState(seed)
    z = [rng.standard_normal(n) * 2.0 for n in sizes]
    r = [0.03 * rng.standard_normal(n) for n in sizes]
    big = [c for c in range(len(sizes)) if sizes[c] >= 5]
    if big:
        z[big[0]][1] = -0.0
        z[big[0]][2] = float("inf")
        z[big[0]][3] = float("nan")
        z[big[-1]][0] = -float("inf")
        z[big[-1]][4] = 0.0
        r[big[0]][0] = float("nan")
        r[big[-1]][2] = 25.0
    calls = np.array([[1 + k, 3 * k, 3 * k + 2, 5.5 + k, -0.031 * (k + 1)] for k in range(n_calls)], dtype=np.float64).reshape(-1, 5)
    arguments = {"func": _function_stored_by_reference, "infile": "s%d.npz" % seed, "minzscore": None, "multitest": 1000.0,
                 "repeats": np.int64(5), "chromosomes": list(range(1, len(sizes) + 1)), "flag": True,
                 "nested": {"a": 1}, "mixed": [1, {"b": 2}]}
    cwz = rng.standard_normal(len(sizes))
    cwz[1 % len(sizes)] = float("nan")
    return dict(binsize=250000, threshold_z=np.float64(4.75 + seed), asdef=np.float64(0.8125), aasdef=np.float64(0.8125 * (4.75 + seed)),
                arguments=arguments, results_cwz=cwz, results_calls=calls if n_calls else np.array([]), results_z=z, results_r=r)


def dense(arrays, stride=None):
    """Per-chromosome arrays of several samples -> rows [n, stride] (padding filled with a value that must not show)."""
    total = sum(len(c) for c in arrays[0])
    stride = max(total, 1) if stride is None else stride
    rows = np.full((len(arrays), stride), 7e77, dtype=np.float64)
    for i, chroms in enumerate(arrays):
        if total:
            rows[i, :total] = np.concatenate([np.asarray(c, dtype=np.float64) for c in chroms])
    return rows
