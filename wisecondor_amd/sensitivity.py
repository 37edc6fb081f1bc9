"""sensitivity: how small and how weak an aberration a reference still finds, and how often.

Healthy converted samples go to the device once; a kernel writes every trial's spiked copy, the batched `test` runs on
them, a second kernel judges every trial's calls against what was planted, and a few dozen bytes per trial come back
(spike.hip).  The plan maker and the table are host work on small arrays.  The read-depth axis (thinCounts, depths_ppm) and
the binomial spike (draw) are reproducible draws made on the device (draw.hip; DESIGN.md 6h "Draws").

A PLAN is int32 [n_trials, 5]: rows {base row, chromosome (1-based), first bin, bins, effect in ppm}; bins are the
chromosome's own bins in the reference's chromosome_sizes layout, the coordinates of results_calls.  An effect is parts
per million of the read depth, PPM_MIN .. PPM_MAX; 0 is a control trial.  How an effect in percent relates to a fetal
fraction is the reader's own model: nothing here assumes one.
"""
import math

import numpy as np

from . import _lib
from . import wisetools as wt

PPM_MIN, PPM_MAX = -1000000, 100000000
MAX_DEPTHS = 8                    # depths of one thinning (wc_thin_counts)
MAX_CALLS = wt.MAX_CALLS          # per trial, the room of the first attempt
#: the table's columns; the last line is the control line (bins 0, ppm 0: trials = the unspiked samples, and the last
#: column their calls per sample)
TABLE_COLUMNS = ('bins', 'effect_ppm', 'trials', 'detected', 'sensitivity', 'median_best_z', 'median_effect', 'mean_jaccard',
                 'calls_elsewhere')
DEPTH_COLUMN = 'depth_ppm'        # leads the table's columns when the table has depths


def _layout_of(reference):
    """(chromosome sizes, mask) of a wt.Reference, an opened reference file or a mapping with those two keys."""
    if hasattr(reference, 'chromosome_sizes'):
        return np.asarray(reference.chromosome_sizes, dtype=np.int64), np.asarray(reference.mask).astype(bool)
    return np.asarray(reference['chromosome_sizes'], dtype=np.int64), np.asarray(reference['mask']).astype(bool)


def _as_plan(plan):
    plan = np.ascontiguousarray(plan, dtype=np.int32)
    if plan.ndim != 2 or plan.shape[1] != 5:
        raise ValueError('a plan is int32 [n_trials, 5], got shape %s' % (plan.shape,))
    return plan


def parseGrid(lengths_text, effects_text, binsize):
    """The command line's grid: lengths in bp, comma separated, become ceil(length / binsize) bins; effects in percent
    become round(percent * 10 000) ppm.  ValueError for an empty grid, a length below one bp or an effect out of range."""
    def numbers(text, what):
        try:
            return [float(token) for token in str(text).split(',') if token.strip()]
        except ValueError:
            raise ValueError('%s: %r is not a comma separated list of numbers' % (what, text))
    lengths, effects = numbers(lengths_text, '-lengths'), numbers(effects_text, '-effects')
    if not lengths or not effects:
        raise ValueError('an empty grid: -lengths and -effects need one value each at least')
    lengths_bins = []
    for length in lengths:
        if not length >= 1 or not math.isfinite(length):
            raise ValueError('a length of %r bp' % length)
        lengths_bins.append(int(math.ceil(length / float(binsize))))
    effects_ppm = []
    for percent in effects:
        ppm = int(round(percent * 10000)) if math.isfinite(percent) else None
        if ppm is None or ppm < PPM_MIN or ppm > PPM_MAX:
            raise ValueError('an effect of %r %% is out of range (%g .. %g %%)' % (percent, PPM_MIN / 1e4, PPM_MAX / 1e4))
        if ppm == 0:
            raise ValueError('an effect of 0 %% plants nothing (every sample has its control trial already)')
        effects_ppm.append(ppm)
    return lengths_bins, effects_ppm


def parseDepths(text):
    """The command line's -depths: fractions in (0, 1], comma separated, become round(d * 1e6) ppm >= 1.  ValueError for
    an empty list, more than MAX_DEPTHS, a fraction out of range or one that rounds to 0 ppm, and a duplicate."""
    try:
        depths = [float(token) for token in str(text).split(',') if token.strip()]
    except ValueError:
        raise ValueError('-depths: %r is not a comma separated list of numbers' % (text,))
    if not depths or len(depths) > MAX_DEPTHS:
        raise ValueError('-depths takes 1 .. %d fractions, got %d' % (MAX_DEPTHS, len(depths)))
    ppm = []
    for d in depths:
        if not math.isfinite(d) or not 0 < d <= 1 or int(round(d * 1e6)) < 1:
            raise ValueError('a depth of %r is out of range (a fraction in (0, 1] of 1 ppm at least)' % d)
        ppm.append(int(round(d * 1e6)))
    if len(set(ppm)) != len(ppm):
        raise ValueError('-depths names a depth twice: %s' % text)
    return ppm


def validStarts(reference, bins, chromosomes):
    """Per selected chromosome, the first bins at which a span of `bins` fits and holds ceil(bins / 2) unmasked bins at
    least."""
    sizes, mask = _layout_of(reference)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    need = (int(bins) + 1) // 2
    out = []
    for chrom in chromosomes:
        if chrom < 1 or chrom > len(sizes):
            raise ValueError('chromosome %d is not one of the reference\'s %d' % (chrom, len(sizes)))
        kept = np.concatenate([[0], np.cumsum(mask[offs[chrom - 1]:offs[chrom]])])
        n = int(sizes[chrom - 1]) - int(bins) + 1
        if n < 1:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        inside = kept[int(bins):int(bins) + n] - kept[:n]
        out.append(np.flatnonzero(inside >= need).astype(np.int64))
    return out


def makePlan(reference, n_samples, lengths_bins, effects_ppm, trials, chromosomes=None, seed=1, n_depths=1):
    """The plan of a grid: per base sample one control trial, then per length `trials` placements, each used with every
    effect (a paired design: rows of one length differ in the effect alone).  A placement's chromosome is drawn among
    the selected ones with probability proportional to its number of valid starts (validStarts), its start uniformly
    among them, from np.random.RandomState(seed).  ValueError, before anything runs, for a length without a valid start
    on any selected chromosome.  Row order: sample, (control | length, effect, placement).  With n_depths > 1 a sample's
    block is repeated per depth, its base row d * n_samples + b (the rows of a thinned image, thinCounts), with the SAME
    placements at every depth: the design stays paired, rows differ in depth or effect alone."""
    chromosomes = list(range(1, 23)) if chromosomes is None else [int(c) for c in chromosomes]
    if not chromosomes or n_samples < 1 or trials < 1 or not len(lengths_bins) or not len(effects_ppm) or n_depths < 1:
        raise ValueError('an empty grid: samples, lengths, effects, trials and chromosomes need one each at least')
    for ppm in effects_ppm:
        if ppm == 0 or ppm < PPM_MIN or ppm > PPM_MAX:
            raise ValueError('an effect of %d ppm is out of range (%d .. %d, not 0)' % (ppm, PPM_MIN, PPM_MAX))
    starts = {}
    for bins in lengths_bins:
        if bins < 1:
            raise ValueError('a length of %d bins' % bins)
        starts[bins] = validStarts(reference, bins, chromosomes)
        if sum(len(s) for s in starts[bins]) == 0:
            raise ValueError('a length of %d bins has no valid start on the selected chromosomes (it must fit a chromosome '
                             'with half of its bins unmasked)' % bins)
    rng = np.random.RandomState(seed)
    rows = []
    for b in range(int(n_samples)):
        block = [(b, chromosomes[0], 0, 1, 0)]
        for bins in lengths_bins:
            weight = np.array([len(s) for s in starts[bins]], dtype=np.float64)
            placed = []
            for _ in range(int(trials)):
                k = int(rng.choice(len(chromosomes), p=weight / weight.sum()))
                placed.append((chromosomes[k], int(starts[bins][k][rng.randint(len(starts[bins][k]))])))
            for ppm in effects_ppm:
                block.extend((b, chrom, first, int(bins), int(ppm)) for chrom, first in placed)
        for d in range(int(n_depths)):
            rows.extend((d * int(n_samples) + b,) + row[1:] for row in block)
    return np.array(rows, dtype=np.int32).reshape(-1, 5)


def sensitivityTable(plan, rec_i, rec_f, lengths_bins, effects_ppm, minoverlap=0.5, depths_ppm=None, n_samples=None):
    """Without depths: float64 [len(lengths_bins) * len(effects_ppm) + 1, 9], columns TABLE_COLUMNS, a line per (length, effect) in that
    order and the control line last.  A trial is detected when n_match >= 1 and overlap_bins >= ceil(minoverlap * bins);
    the medians are over the detected trials (NaN without one), mean_jaccard is the mean of overlap_bins / (bins +
    match_bins - overlap_bins) and calls_elsewhere the mean of n_calls - n_match, both over all of the line's trials.
    With depths_ppm (and n_samples, the base rows per depth: a plan row's depth is base row // n_samples): that block of
    lines once per depth, its control line included, under a leading depth_ppm column: [n_depths * (lines + 1), 10]."""
    plan = _as_plan(plan)
    if depths_ppm is not None:
        if n_samples is None or n_samples < 1:
            raise ValueError('a table with depths needs n_samples, the base rows per depth')
        rec_i = np.asarray(rec_i).reshape(-1, 8)
        rec_f = np.asarray(rec_f, dtype=np.float64).reshape(-1, 2)
        if not (len(plan) == len(rec_i) == len(rec_f)):
            raise ValueError('%d plan rows, %d and %d records' % (len(plan), len(rec_i), len(rec_f)))
        depth_of = plan[:, 0] // int(n_samples)
        blocks = []
        for d, ppm_d in enumerate(depths_ppm):
            rows = depth_of == d
            block = sensitivityTable(plan[rows], rec_i[rows], rec_f[rows], lengths_bins, effects_ppm, minoverlap)
            blocks.append(np.concatenate([np.full((len(block), 1), float(ppm_d)), block], axis=1))
        return np.concatenate(blocks)
    rec_i = np.asarray(rec_i).reshape(-1, 8).astype(np.int64)
    rec_f = np.asarray(rec_f, dtype=np.float64).reshape(-1, 2)
    if not (len(plan) == len(rec_i) == len(rec_f)):
        raise ValueError('%d plan rows, %d and %d records' % (len(plan), len(rec_i), len(rec_f)))
    bins, ppm = plan[:, 3].astype(np.int64), plan[:, 4].astype(np.int64)
    n_calls, n_match, overlap, match_bins = rec_i[:, 0], rec_i[:, 1], rec_i[:, 2], rec_i[:, 3]
    detected = (n_match >= 1) & (overlap >= np.ceil(float(minoverlap) * bins))
    jaccard = overlap / (bins + match_bins - overlap).astype(np.float64)
    lines = []
    for length in lengths_bins:
        for effect in effects_ppm:
            rows = (bins == length) & (ppm == effect) & (ppm != 0)
            hit = rows & detected
            n, d = int(rows.sum()), int(hit.sum())
            lines.append([length, effect, n, d, d / n if n else np.nan,
                          np.median(rec_f[hit, 0]) if d else np.nan, np.median(rec_f[hit, 1]) if d else np.nan,
                          jaccard[rows].mean() if n else np.nan, (n_calls - n_match)[rows].mean() if n else np.nan])
    control = ppm == 0
    n = int(control.sum())
    lines.append([0, 0, n, 0, np.nan, np.nan, np.nan, np.nan, n_calls[control].mean() if n else np.nan])
    return np.array(lines, dtype=np.float64).reshape(-1, len(TABLE_COLUMNS))


def tableText(table):
    """The table as tab separated text: a header line, then a line per row; the whole numbers as such, the others as
    repr writes them (float() reads every one back bit for bit).  A table with depths has its depth_ppm column first."""
    table = np.asarray(table, dtype=np.float64)
    lead = table.shape[1] - len(TABLE_COLUMNS) if table.ndim == 2 else 0
    out = ['\t'.join((DEPTH_COLUMN,) * lead + TABLE_COLUMNS)]
    for row in table:
        out.append('\t'.join([str(int(v)) for v in row[:4 + lead]] + [repr(float(v)) for v in row[4 + lead:]]))
    return '\n'.join(out) + '\n'


# ------------------------------------------------------------------------------------- the device's half ----
def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def thinCounts(base, chrom_sizes, keep_ppm, seed=1, device=0):
    """int32 [n_keep, n_base, n_total]: base [n_base, n_total] thinned to every depth of keep_ppm (1 .. 1 000 000 each, at
    most MAX_DEPTHS): every read of a bin is kept with probability keep_ppm / 10^6, the draws a pure function of (seed,
    base row, chromosome, bin, read) and shared by all depths, so a bin never gains as the depth falls and 1 000 000 is a
    copy (include/wisecondor_hip.h has the rule).  Counts below 0 are copied; a bin above 2^24 reads is refused.  Host
    arrays in and out (wc_thin_counts)."""
    lib = _lib.load()
    base = np.ascontiguousarray(base, dtype=np.int32)
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    keep = np.ascontiguousarray(keep_ppm, dtype=np.int32).reshape(-1)
    if base.ndim != 2 or base.shape[1] != int(sizes.sum()):
        raise ValueError('base rows of %s for %d bins' % (base.shape, int(sizes.sum())))
    out = np.empty((len(keep),) + base.shape, dtype=np.int32)
    _lib.check(lib.wc_thin_counts(_lib.context(device), _lib.ptr(base), base.shape[0], _lib.ptr(sizes), len(sizes), _lib.ptr(keep), len(keep),
                                  _seed64(seed), _lib.ptr(out)))
    return out


def spikeCounts(base, chrom_sizes, plan, device=0, draw=False, seed=1, trial0=0):
    """(int32 [n_trials, n_total], saturated): row plan[i][0] of base [n_base, n_total] with trial i's span spiked, every
    count c >= 0 inside it min(2^31 - 1, (c * (1 000 000 + ppm) + 500 000) // 1 000 000); saturated: how many bins the
    minimum clipped.  With draw the binomial spike instead: min(2^31 - 1, c * whole + B(c, frac)), whole and frac the
    quotient and remainder of 1 000 000 + ppm by 1 000 000, drawn under `seed` as plan row trial0 + i.  Host arrays in and
    out (wc_spike_counts, wc_spike_counts_ex)."""
    lib = _lib.load()
    base = np.ascontiguousarray(base, dtype=np.int32)
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    plan = _as_plan(plan)
    if base.ndim != 2 or base.shape[1] != int(sizes.sum()):
        raise ValueError('base rows of %s for %d bins' % (base.shape, int(sizes.sum())))
    out = np.empty((len(plan), base.shape[1]), dtype=np.int32)
    saturated = np.zeros(1, dtype=np.int64)
    if draw:
        _lib.check(lib.wc_spike_counts_ex(_lib.context(device), _lib.ptr(base), base.shape[0], _lib.ptr(sizes), len(sizes), _lib.ptr(plan),
                                          len(plan), 1, _seed64(seed), int(trial0), _lib.ptr(out), _lib.ptr(saturated)))
    else:
        _lib.check(lib.wc_spike_counts(_lib.context(device), _lib.ptr(base), base.shape[0], _lib.ptr(sizes), len(sizes), _lib.ptr(plan),
                                       len(plan), _lib.ptr(out), _lib.ptr(saturated)))
    return out, int(saturated[0])


def scoreTrials(plan, calls, n_calls, device=0):
    """(rec_i int32 [n_trials, 8], rec_f float64 [n_trials, 2]) of calls [n_trials, max_calls, 5] and n_calls [n_trials]:
    {n_calls, n_match, overlap_bins, match_bins, best_row, best_start, best_end, 0} and {best z, best effect}
    (include/wisecondor_hip.h has the rules).  Host arrays in and out (wc_spike_score)."""
    lib = _lib.load()
    plan = _as_plan(plan)
    calls = np.ascontiguousarray(calls, dtype=np.float64)
    n_calls = np.ascontiguousarray(n_calls, dtype=np.int32)
    if calls.ndim != 3 or calls.shape[0] != len(plan) or calls.shape[2] != 5 or n_calls.shape != (len(plan),):
        raise ValueError('calls of %s and counts of %s for %d trials' % (calls.shape, n_calls.shape, len(plan)))
    rec_i = np.empty((len(plan), 8), dtype=np.int32)
    rec_f = np.empty((len(plan), 2), dtype=np.float64)
    _lib.check(lib.wc_spike_score(_lib.context(device), _lib.ptr(plan), len(plan), _lib.ptr(calls), _lib.ptr(n_calls), calls.shape[1],
                                  _lib.ptr(rec_i), _lib.ptr(rec_f)))
    return rec_i, rec_f


def sensitivity_batch(reference, samples, plan, threshold, minrefbins=25, repeats=5, chromosomes=None, mineffectsize=0, batch=1024,
                      keep_calls=False, depths_ppm=None, draw=False, seed=1):
    """The plan's trials on the device: the base image of `samples` (sample dicts at the reference's bin size) is uploaded
    once, the plan runs in batches of at most min(batch, 60000 // selected chromosomes) trials
    (wc_sensitivity_batch_dev: spike, test, score), and a batch whose trial has more than MAX_CALLS calls is run again
    with four times the room, as wt.test_batch does.  Returns (rec_i, rec_f), and with keep_calls a list of every
    trial's call rows [n, 5] as well.  With depths_ppm the uploaded image is thinned once on the device (thinCounts' rule
    under `seed`) into len(depths_ppm) * len(samples) rows, depth-major, and the plan's base rows name those (makePlan's
    n_depths).  With draw the spike is the binomial one under `seed`; every batch passes its global offset, so a trial's
    draws depend on its plan row index and not on the batch size."""
    import torch
    lib = _lib.load()
    plan = _as_plan(plan)
    sel = np.ascontiguousarray(list(range(1, 23)) if chromosomes is None else chromosomes, dtype=np.int32)
    sizes = np.ascontiguousarray(reference.chromosome_sizes, dtype=np.int64)
    counts = wt.samples_to_counts(samples, [int(v) for v in sizes])
    n = len(plan)
    rec_i = np.empty((n, 8), dtype=np.int32)
    rec_f = np.empty((n, 2), dtype=np.float64)
    kept = []
    step = max(1, min(int(batch), 60000 // max(1, len(sel))))
    dev = torch.device('cuda', reference.device)
    with torch.cuda.device(dev):
        base = torch.from_numpy(counts).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        if depths_ppm is not None:
            keep = np.ascontiguousarray(depths_ppm, dtype=np.int32).reshape(-1)
            image = torch.empty((len(keep) * base.shape[0], base.shape[1]), dtype=torch.int32, device=dev)
            _lib.check(lib.wc_thin_counts_dev(reference.ctx, stream, base.data_ptr(), base.shape[0], _lib.ptr(sizes), len(sizes),
                                              _lib.ptr(keep), len(keep), _seed64(seed), image.data_ptr()))
            base = image
        extended = depths_ppm is not None or draw
        for lo in range(0, n, step):
            part = np.ascontiguousarray(plan[lo:lo + step])
            m = len(part)
            max_calls = MAX_CALLS
            while True:
                ri = torch.empty((m, 8), dtype=torch.int32, device=dev)
                rf = torch.empty((m, 2), dtype=torch.float64, device=dev)
                calls = torch.empty((m, max_calls, 5), dtype=torch.float64, device=dev) if keep_calls else None
                n_calls = torch.empty((m,), dtype=torch.int32, device=dev) if keep_calls else None
                head = (reference.ctx, stream, reference.handle, base.data_ptr(), base.shape[0], _lib.ptr(sizes), len(sizes),
                        _lib.ptr(part), m)
                tail = (float(threshold), int(minrefbins), int(repeats), float(mineffectsize), _lib.ptr(sel), len(sel),
                        max_calls, ri.data_ptr(), rf.data_ptr(), calls.data_ptr() if keep_calls else None,
                        n_calls.data_ptr() if keep_calls else None)
                if extended:
                    rc = lib.wc_sensitivity_batch_ex_dev(*(head + (1 if draw else 0, _seed64(seed), lo) + tail))
                else:
                    rc = lib.wc_sensitivity_batch_dev(*(head + tail))
                if rc == _lib.E_LIMIT and b"max_calls" in lib.wc_last_error() and max_calls < reference.n_total:
                    max_calls *= 4
                    continue
                _lib.check(rc)
                break
            rec_i[lo:lo + m] = ri.cpu().numpy()
            rec_f[lo:lo + m] = rf.cpu().numpy()
            if keep_calls:
                rows, counts_of = calls.cpu().numpy(), n_calls.cpu().numpy()
                kept.extend(rows[i, :counts_of[i]].copy() for i in range(m))
    return (rec_i, rec_f, kept) if keep_calls else (rec_i, rec_f)
