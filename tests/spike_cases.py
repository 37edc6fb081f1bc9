"""The designed trials of the `sensitivity` tests (a helper module, not a conftest).  Everything builds on call_cases:
layout("short") (22 chromosomes, 994 bins, chromosome 1 with masked bins at p % 97 == 13, a masked bin 5 inside
chromosome 2, a masked last bin on chromosome 3, a Poisson(30) background), the unspiked sample(lay, []) and
reference_of.  The oracle (wo.test_sample with THR = 5, MINREF = 25, REPEATS = 2) finds no call in the unspiked sample
and exactly one call for every plan row below but the last, which is a designed miss; test_spike_cases_cpu.py holds
that, the GPU tests build on it.
"""
import functools

import numpy as np

import call_cases as cc
import spike_restated as sr
from oracle import wc_oracle as wo

# (chromosome, first bin, bins, ppm), the call the oracle gives as (start, end) or None, the designed record
# (n_match, overlap_bins, match_bins), what the row is there for
ROWS = [
    ((1, 20, 5, 2500000), (20, 24), (1, 5, 5), "a short gain"),
    ((1, 10, 7, 2500000), (10, 16), (1, 7, 7), "over masked bin 13"),
    ((1, 20, 5, -1000000), (20, 24), (1, 5, 5), "everything lost"),
    ((1, 20, 5, -700000), (20, 24), (1, 5, 5), "a loss"),
    ((1, 20, 1, 2500000), (20, 20), (1, 1, 1), "one bin"),
    ((1, 0, 4, 2500000), (0, 3), (1, 4, 4), "the chromosome's first bins"),
    ((1, 147, 5, 2500000), (147, 151), (1, 5, 5), "the chromosome's last bins"),
    ((2, 3, 6, 2500000), (3, 8), (1, 6, 6), "over masked bin 5 of chromosome 2"),
    ((3, 35, 6, 2500000), (35, 38), (1, 4, 4), "ends on the masked last bin: overlap 4 of 6"),
    ((1, 20, 40, 200000), (20, 60), (1, 40, 41), "a weak gain: the call runs one bin past the span"),
    ((1, 20, 40, -200000), (26, 57), (1, 32, 32), "a weak loss: the call lies inside the span"),
    ((5, 0, 40, 300000), (0, 39), (1, 40, 40), "a whole chromosome"),
    ((12, 5, 5, 2500000), (5, 9), (1, 5, 5), "a chromosome the shared reference list draws from"),
    ((1, 20, 3, 100000), None, (0, 0, 0), "a designed miss"),
]
SECOND_SEED = 4              # the second base sample: the same layout with this seed's background


def lay():
    return cc.layout("short")


@functools.lru_cache(maxsize=None)
def base_samples():
    """[the unspiked sample of call_cases, the same with another seed's background]; both as cc.sample gives them."""
    first = cc.sample(lay(), [])
    other = dict(lay())
    background = np.random.RandomState(SECOND_SEED).poisson(cc.BACKGROUND, lay()["n_bins"]).astype(np.int64)
    background[lay()["refs_of"][0]] = cc.POOL_COUNTS          # the shared list keeps its counts, as in call_cases.layout
    other["background"] = background
    return [first, cc.sample(other, [])]


def base_counts():
    """int32 [2, n_total]: the dense image of the two base samples."""
    return np.stack([np.concatenate([s["counts"][str(c)] for c in range(1, 23)]) for s in base_samples()]).astype(np.int32)


def plan_of(rows, base=0):
    return np.array([(base,) + tuple(r) for r in rows], dtype=np.int32).reshape(-1, 5)


def designed_plan():
    """The fourteen rows on base sample 0, a control on either base, and four of the rows again on base sample 1."""
    rows = [(0,) + r[0] for r in ROWS] + [(0, 1, 0, 1, 0), (1, 1, 0, 1, 0)] + [(1,) + ROWS[i][0] for i in (0, 2, 9, 13)]
    return np.array(rows, dtype=np.int32)


def spiked_sample(plan_row):
    """The sample dict '1'..'22' of one plan row, spiked by the restated rule."""
    counts = sr.spike(base_counts(), lay()["sizes"], np.asarray([plan_row], dtype=np.int32))[0][0]
    goff = lay()["goff"]
    return {str(c + 1): counts[goff[c]:goff[c + 1]].copy() for c in range(22)}


@functools.lru_cache(maxsize=None)
def oracle_calls(plan_row):
    """The oracle's call rows [n, 5] of one plan row (a tuple), computed once."""
    smp = base_samples()[plan_row[0]]
    with np.errstate(all="ignore"):
        out = wo.test_sample(spiked_sample(plan_row), cc.BINSIZE, cc.reference_of(lay(), smp), minzscore=cc.THR,
                             minrefbins=cc.MINREF, repeats=cc.REPEATS)
    rows = np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)
    rows.setflags(write=False)
    return rows


# ---------------------------------------------------------------------------------- the command line's grid ----
CLI_SEEDS = (None, SECOND_SEED, 5, 7)       # four sample files: the two base samples and two more backgrounds
CLI_LENGTHS_BP, CLI_EFFECTS_PERCENT, CLI_TRIALS = "5e6,40e6", "250,-100,10", 3
CLI_LENGTHS_BINS, CLI_EFFECTS_PPM = [5, 40], [2500000, -1000000, 100000]


@functools.lru_cache(maxsize=None)
def cli_samples():
    out = list(base_samples())
    for seed in CLI_SEEDS[2:]:
        other = dict(lay())
        background = np.random.RandomState(seed).poisson(cc.BACKGROUND, lay()["n_bins"]).astype(np.int64)
        background[lay()["refs_of"][0]] = cc.POOL_COUNTS
        other["background"] = background
        out.append(cc.sample(other, []))
    return out


def write_cli_files(folder):
    """(four sample files, a reference file) as `convert` and `newref` write them, under `folder`."""
    import os
    paths = []
    for i, smp in enumerate(cli_samples()):
        paths.append(os.path.join(str(folder), "healthy_%d.npz" % i))
        np.savez_compressed(paths[-1], arguments={"binsize": float(cc.BINSIZE)}, runtime={}, sample=smp["counts"], quality={})
    ref = os.path.join(str(folder), "reference.npz")
    np.savez_compressed(ref, **cc.reference_of(lay(), cli_samples()[0]))
    return paths, ref
