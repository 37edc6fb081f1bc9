"""exportjson restated with json.dumps alone: the text of a dense row and the whole file.  Nothing of the product is
used here; CPython's float.__repr__ is the reference for every number."""
import json

import numpy as np

KEYS = ("binsize", "threshold_z", "asdef", "aasdef", "arguments", "results_cwz", "results_calls", "results_z", "results_r")


def _finite_or_none(x):
    return x if x - x == 0 else None


def row_text(row, sizes, strict=False):
    """bytes: [[v,v,...],[...],...] of the dense row cut at the chromosome sizes."""
    chroms, at = [], 0
    for n in sizes:
        values = [float(v) for v in row[at:at + n]]
        chroms.append([_finite_or_none(v) for v in values] if strict else values)
        at += n
    return json.dumps(chroms, separators=(",", ":"), allow_nan=not strict).encode("ascii")


def plain(value):
    """(kept, value) of an `arguments` entry: bool, int, float, str, None, lists or tuples of those; numpy scalars through
    .item()."""
    if isinstance(value, np.generic):
        value = value.item()
    if value is None or isinstance(value, (bool, int, float, str)):
        return True, value
    if isinstance(value, (list, tuple)):
        inner = [plain(v) for v in value]
        return all(k for k, _ in inner), [v for _, v in inner]
    return False, None


def file_object(result, strict=False):
    """The file as one Python object, keys in the file's order."""
    def numbers(a):
        values = [float(v) for v in np.asarray(a, dtype=np.float64).ravel()]
        return [_finite_or_none(v) for v in values] if strict else values
    obj = {}
    for key in KEYS[:4]:
        value = np.asarray(result[key]).item()
        obj[key] = _finite_or_none(value) if strict and isinstance(value, float) else value
    kept = {}
    for key in sorted(result["arguments"]):
        ok, value = plain(result["arguments"][key])
        if ok:
            if strict:
                value = json.loads(json.dumps(value), parse_constant=lambda name: None)
            kept[key] = value
    obj["arguments"] = kept
    obj["results_cwz"] = numbers(result["results_cwz"])
    calls = np.asarray(result["results_calls"], dtype=np.float64).reshape(-1, 5)
    obj["results_calls"] = [[int(c[0]), int(c[1]), int(c[2])] + numbers(c[3:]) for c in calls]
    obj["results_z"] = [numbers(c) for c in result["results_z"]]
    obj["results_r"] = [numbers(c) for c in result["results_r"]]
    return obj


def file_text(result, strict=False):
    return json.dumps(file_object(result, strict), separators=(",", ":"), allow_nan=not strict).encode("ascii")


def same_bits(a, b):
    """float arrays equal bit for bit, except that any NaN equals any NaN (JSON has one NaN)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))
