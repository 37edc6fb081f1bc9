"""The rules of `sensitivity` restated without the library (a helper module, not a conftest): the spike in plain numpy,
the score in plain Python, the table in plain Python.  DESIGN.md 6h has the rules.

    spike     inside the span every count c >= 0 becomes min(2^31 - 1, (c * (1 000 000 + ppm) + 500 000) // 1 000 000)
    score     a call [chrom, start, end, z, effect] matches a trial with span [s, e] on chromosome c when its chromosome
              is c, its z has the effect's sign and min(e, end) - max(s, start) + 1 >= 1
    table     detected: n_match >= 1 and overlap_bins >= ceil(minoverlap * bins)
"""
import math
from fractions import Fraction

import numpy as np

INT_MAX = 2 ** 31 - 1


def spike_value(c, ppm):
    """One count by the rule, in Python's integers; (value, clipped)."""
    if c < 0:
        return c, False
    v = (c * (1000000 + ppm) + 500000) // 1000000
    return min(INT_MAX, v), v > INT_MAX


def spike_value_fraction(c, ppm):
    """The same by exact rational arithmetic: c * (1 + ppm / 10^6) rounded half up, clipped."""
    exact = Fraction(c) * (1 + Fraction(ppm, 1000000))
    return min(INT_MAX, math.floor(exact + Fraction(1, 2)))


def spike(base, chrom_sizes, plan):
    """(int32 [n_trials, n_total], saturated) of base int32 [n_base, n_total] and plan rows {base row, chromosome, first
    bin, bins, ppm}.  ppm == 0: a control trial, nothing is planted."""
    base = np.asarray(base, dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(np.asarray(chrom_sizes, dtype=np.int64))])
    out = np.empty((len(plan), base.shape[1]), dtype=np.int32)
    saturated = 0
    for i, (b, chrom, first, bins, ppm) in enumerate(np.asarray(plan, dtype=np.int64).tolist()):
        out[i] = base[b]
        if ppm == 0:
            continue
        lo = int(offs[chrom - 1]) + first
        seg = base[b, lo:lo + bins].astype(np.int64)
        val = (seg * (1000000 + ppm) + 500000) // 1000000          # (below 2^63: 2^31 * 101 000 000 = 2.2e17)
        over = (seg >= 0) & (val > INT_MAX)
        saturated += int(over.sum())
        out[i, lo:lo + bins] = np.where(seg < 0, seg, np.minimum(val, INT_MAX)).astype(np.int32)
    return out, saturated


def score_one(row, calls):
    """One trial's record of its call rows (a sequence of [chrom, start, end, z, effect]): (eight ints, two floats)."""
    _, chrom, first, bins, ppm = [int(v) for v in row]
    s, e = first, first + bins - 1
    n_match = overlap = length = 0
    best, best_ov = -1, 0
    for r, call in enumerate(calls):
        z = float(call[3])
        sign = (z > 0) if ppm > 0 else (z < 0) if ppm < 0 else False
        if not sign or float(call[0]) != float(chrom):
            continue
        cs, ce = int(call[1]), int(call[2])
        ov = min(e, ce) - max(s, cs) + 1
        if ov < 1:
            continue
        n_match += 1
        overlap += ov
        length += ce - cs + 1
        if ov > best_ov:
            best, best_ov = r, ov
    clip = lambda v: min(v, INT_MAX)                                 # noqa: E731
    if best < 0:
        return [len(calls), 0, 0, 0, -1, -1, -1, 0], [float("nan"), float("nan")]
    return ([len(calls), clip(n_match), clip(overlap), clip(length), best, int(calls[best][1]), int(calls[best][2]), 0],
            [float(calls[best][3]), float(calls[best][4])])


def score(plan, calls, n_calls):
    """(rec_i int32 [n, 8], rec_f float64 [n, 2]) of calls [n, max_calls, 5] and n_calls [n]; rows at and behind
    n_calls[i] are not looked at."""
    rec_i = np.empty((len(plan), 8), dtype=np.int32)
    rec_f = np.empty((len(plan), 2), dtype=np.float64)
    for i, row in enumerate(np.asarray(plan).tolist()):
        n = max(0, min(int(n_calls[i]), len(calls[i])))
        rec_i[i], rec_f[i] = score_one(row, [list(c) for c in np.asarray(calls[i], dtype=np.float64)[:n]])
    return rec_i, rec_f


def score_lists(plan, call_lists):
    """The same of a list of per-trial call arrays [n_i, 5]."""
    rec_i = np.empty((len(plan), 8), dtype=np.int32)
    rec_f = np.empty((len(plan), 2), dtype=np.float64)
    for i, row in enumerate(np.asarray(plan).tolist()):
        rec_i[i], rec_f[i] = score_one(row, [list(c) for c in np.asarray(call_lists[i], dtype=np.float64).reshape(-1, 5)])
    return rec_i, rec_f


def median(values):
    v = sorted(values)
    if not v:
        return float("nan")
    m = len(v) // 2
    return v[m] if len(v) % 2 else float(np.float64(v[m - 1]) + np.float64(v[m])) / 2.0


def table(plan, rec_i, rec_f, lengths_bins, effects_ppm, minoverlap=0.5):
    """Lines [bins, ppm, trials, detected, sensitivity, median best z, median effect, mean jaccard, calls elsewhere] per
    (length, effect), and the control line [0, 0, controls, 0, nan, nan, nan, nan, calls per unspiked sample]."""
    nan = float("nan")
    lines = []
    plan = np.asarray(plan).tolist()
    rec_i = np.asarray(rec_i).tolist()
    rec_f = np.asarray(rec_f).tolist()
    for length in lengths_bins:
        for effect in effects_ppm:
            rows = [i for i, p in enumerate(plan) if p[3] == length and p[4] == effect and effect != 0]
            hit = [i for i in rows if rec_i[i][1] >= 1 and rec_i[i][2] >= math.ceil(minoverlap * length)]
            n = len(rows)
            jac = [rec_i[i][2] / float(length + rec_i[i][3] - rec_i[i][2]) for i in rows]
            away = [rec_i[i][0] - rec_i[i][1] for i in rows]
            lines.append([length, effect, n, len(hit), len(hit) / n if n else nan, median([rec_f[i][0] for i in hit]),
                          median([rec_f[i][1] for i in hit]), float(np.mean(jac)) if n else nan, float(np.mean(away)) if n else nan])
    control = [i for i, p in enumerate(plan) if p[4] == 0]
    lines.append([0, 0, len(control), 0, nan, nan, nan, nan, float(np.mean([rec_i[i][0] for i in control])) if control else nan])
    return np.array(lines, dtype=np.float64)
