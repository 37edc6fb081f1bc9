"""crossval: what the pipeline calls on healthy samples its reference has never seen.

The cohort's counts go to the device once.  Fold after fold a reference is built from every sample but the fold's
(wt.prepReference, distributed.NewrefJob, wt.Reference: the routes `newref` takes) and the fold's samples are tested
against it (wc_test_batch_dev); their z-scores and ratios fill the rows of cohort-sized device tensors.  After the last
fold the kernels of csrc/crossval.hip judge all rows in cohort order: per sample, per bin and per window length
(wc_crossval_stats_dev; include/wisecondor_hip.h has the rules).  The fold plan and the tables are host work on small
arrays.
"""
import math

import numpy as np

from . import _lib
from . import wisetools as wt

MAX_CALLS = wt.MAX_CALLS          # per sample, the room of the first attempt
MAX_TRAINING = 4096               # samples the GPU prep takes (wt.prepReference's eigenproblem)
MIN_TRAINING = 4
MAX_LENGTHS = 16
HIST_SLOTS = 130                  # win_hist: slot 0 below -16, 1 .. 128 quarter units of [-16, 16), 129 at 16, above, or NaN
DEFAULT_WINDOWS = (1, 2, 5, 10, 20, 50, 100)
SAMPLE_COLUMNS = ('sample', 'fold', 'calls', 'call_bins', 'tested', 'over_hi', 'over_lo', 'asdef', 'max_z', 'min_z')
BIN_COLUMNS = ('chromosome', 'start', 'end', 'tested', 'nonfinite', 'median', 'spread', 'mean', 'sd', 'listed')
WINDOW_COLUMNS = ('length', 'rows', 'windows', 'hi', 'lo', 'rate', 'expected', 'spread')
#: the two quantiles whose half distance is a normal distribution's standard deviation
SPREAD_QUANTILES = (0.1587, 0.8413)


def foldPlan(n_samples, folds, seed=1):
    """int32 [n_samples]: the fold of every sample.  folds == n_samples is leave-one-out, fold_of[i] = i, and the seed is not
    used; otherwise perm = np.random.RandomState(seed).permutation(n) and fold_of[perm[j]] = j % folds, so fold sizes
    differ by one at most.  ValueError for folds < 2, folds > n, a fold that leaves fewer than MIN_TRAINING training
    samples, and a training set beyond the GPU prep's MAX_TRAINING."""
    n, folds = int(n_samples), int(folds)
    if folds < 2:
        raise ValueError('%d folds: cross-validation needs two at least' % folds)
    if folds > n:
        raise ValueError('%d folds of %d samples' % (folds, n))
    largest, smallest = -(-n // folds), n // folds
    if n - largest < MIN_TRAINING:
        raise ValueError('%d folds of %d samples leave %d training samples (%d at least)' % (folds, n, n - largest, MIN_TRAINING))
    if n - smallest > MAX_TRAINING:
        raise ValueError('%d folds of %d samples leave %d training samples (the GPU prep takes %d)' % (folds, n, n - smallest,
                                                                                                      MAX_TRAINING))
    if folds == n:
        return np.arange(n, dtype=np.int32)
    perm = np.random.RandomState(seed).permutation(n)
    fold_of = np.empty(n, dtype=np.int32)
    fold_of[perm] = np.arange(n) % folds
    return fold_of


def parseWindows(text):
    """The command line's -windows: whole numbers >= 1, comma separated, strictly ascending, at most MAX_LENGTHS."""
    try:
        lengths = [int(token) for token in str(text).split(',') if token.strip()]
    except ValueError:
        raise ValueError('-windows: %r is not a comma separated list of whole numbers' % (text,))
    return checkWindows(lengths)


def checkWindows(lengths):
    lengths = [int(v) for v in lengths]
    if not 1 <= len(lengths) <= MAX_LENGTHS:
        raise ValueError('%d window lengths (1 .. %d)' % (len(lengths), MAX_LENGTHS))
    for at, length in enumerate(lengths):
        if length < 1 or length > 2 ** 31 - 1 or (at and length <= lengths[at - 1]):
            raise ValueError('window lengths must be >= 1 and strictly ascending: %s' % (lengths,))
    return lengths


# ------------------------------------------------------------------------------------- the device's half ----
def _stats_args(n, sizes, sel, lengths):
    n_total, n_len = int(sizes.sum()), len(lengths)
    return dict(bins_i=((n_total, 6), np.int32), bins_f=((n_total, 2), np.float64), rec_i=((n, 8), np.int32),
                rec_f=((n, 4), np.float64), win_n=((n, n_len), np.int64), win_i=((n_len, 4), np.int64),
                win_hist=((n_len, HIST_SLOTS), np.int64))


STATS_KEYS = ('bins_i', 'bins_f', 'rec_i', 'rec_f', 'win_n', 'win_i', 'win_hist')


def crossvalStats(Z, chrom_sizes, thr, asdef, calls, n_calls, chromosomes=None, windows=DEFAULT_WINDOWS, device=0):
    """The judging alone, host arrays in and out (wc_crossval_stats): Z [n, row_stride >= n_total] float64, thr and asdef [n],
    calls [n, max_calls, 5], n_calls [n].  Returns a dict of bins_i, bins_f, rec_i, rec_f, win_n, win_i, win_hist
    (include/wisecondor_hip.h has the rules); rec_i's first column, the fold, is 0."""
    lib = _lib.load()
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    asdef = np.ascontiguousarray(asdef, dtype=np.float64)
    calls = np.ascontiguousarray(calls, dtype=np.float64)
    n_calls = np.ascontiguousarray(n_calls, dtype=np.int32)
    sel = np.ascontiguousarray(list(range(1, 23)) if chromosomes is None else chromosomes, dtype=np.int32)
    lengths = np.ascontiguousarray(windows, dtype=np.int32)
    n = Z.shape[0]
    if Z.ndim != 2 or calls.ndim != 3 or calls.shape[0] != n or calls.shape[2] != 5 or not (thr.shape == asdef.shape == n_calls.shape == (n,)):
        raise ValueError('Z of %s, calls of %s, thr, asdef and n_calls of %s, %s, %s' % (Z.shape, calls.shape, thr.shape, asdef.shape,
                                                                                         n_calls.shape))
    out = {key: np.zeros(shape, dtype=dtype) for key, (shape, dtype) in _stats_args(n, sizes, sel, lengths).items()}
    _lib.check(lib.wc_crossval_stats(_lib.context(device), _lib.ptr(Z), Z.shape[1], n, _lib.ptr(sizes), len(sizes), _lib.ptr(thr),
                                     _lib.ptr(asdef), _lib.ptr(calls), _lib.ptr(n_calls), calls.shape[1], _lib.ptr(sel), len(sel),
                                     _lib.ptr(lengths), len(lengths), *[_lib.ptr(out[key]) for key in STATS_KEYS]))
    return out


def crossval_batch(counts, chrom_sizes, fold_of, binsize, refsize=100, multitest=1000, minzscore=None, minrefbins=25, repeats=5,
                   chromosomes=None, mineffectsize=0, windows=DEFAULT_WINDOWS, keep_results=False, device=0, stage_ms=None,
                   drop=None, robust=False):
    """Every sample of counts (int32 [n, n_total], the image of ingest.load_counts / wt.samples_to_counts in the layout
    chrom_sizes, which every fold uses) tested against a reference built from the samples of the other folds, and the
    held-out results judged on the device.  fold_of: foldPlan's array.  Folds run in ascending fold number; nothing in a
    sample's results or in the statistics depends on that order.  A fold whose sample has more than MAX_CALLS calls is
    tested again with four times the room, as wt.test_batch does.

    Returns a dict: fold_of; threshold, cutoff float64 [folds] (the per-bin |z| cut and the reference's distance cutoff of
    every fold); calls float64 [n_calls, 6] (sample index, then the five call columns, samples ascending); rec_i, rec_f,
    bins_i, bins_f, win_n, win_i, win_hist (wc_crossval_stats_dev; rec_i's first column is the fold).  With keep_results
    also Z, R float64 [n, n_total] and results_cwz [n, selected chromosomes].

    drop: a blacklist (blacklist.readBlacklist), handed to every fold's wt.prepReference.  robust: after the judging
    wc_column_robust_dev runs once over Z on the same stream, and the result gains robust_i int32 [n_total, 2] {finite,
    nonfinite} and robust_f float64 [n_total, 2] {median, mad} (stage_ms: 'robust').  Without it no key and no launch is new.

    stage_ms (a dict, for the measuring tool): receives device-event times in ms summed over the folds under 'gather',
    'prep', 'newref', 'reference', 'test', 'stats' and, with robust, 'robust'; the events synchronise, so the run is slower with it."""
    import torch
    from .distributed import NewrefJob
    from .wisecondor import zThreshold
    lib = _lib.load()
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    fold_of = np.ascontiguousarray(fold_of, dtype=np.int32).reshape(-1)
    sel = np.ascontiguousarray(list(range(1, 23)) if chromosomes is None else chromosomes, dtype=np.int32)
    lengths = np.ascontiguousarray(checkWindows(windows), dtype=np.int32)
    n, n_total = counts.shape
    if n_total != int(sizes.sum()) or fold_of.shape != (n,):
        raise ValueError('counts of %s for %d bins and %d fold numbers' % (counts.shape, int(sizes.sum()), len(fold_of)))
    folds = int(fold_of.max()) + 1 if n else 0
    sizes_of = np.bincount(fold_of, minlength=folds) if n and fold_of.min() >= 0 else np.zeros(1)
    if folds < 2 or sizes_of.min() < 1 or n - sizes_of.max() < MIN_TRAINING or n - sizes_of.min() > MAX_TRAINING:
        raise ValueError('a fold plan of %d folds over %d samples: every fold 0 .. folds - 1 needs a sample and %d .. %d training '
                         'samples' % (folds, n, MIN_TRAINING, MAX_TRAINING))
    ctx = _lib.context(device)
    dev = torch.device('cuda', device)
    threshold, cutoff = np.empty(folds), np.empty(folds)
    step = max(1, 60000 // max(1, len(sel)))            # wc_test_batch_dev: (sample, chromosome) regions per call
    marks = []

    def mark(name):
        if stage_ms is not None:
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            marks.append((name, event))

    with torch.cuda.device(dev):
        host_counts = torch.from_numpy(counts)
        image = host_counts.to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        f64 = dict(dtype=torch.float64, device=dev)
        Z, R = torch.zeros((n, n_total), **f64), torch.zeros((n, n_total), **f64)
        cwz, asdef = torch.zeros((n, len(sel)), **f64), torch.zeros((n,), **f64)
        max_calls = MAX_CALLS
        calls = torch.zeros((n, max_calls, 5), **f64)
        n_calls = torch.zeros((n,), dtype=torch.int32, device=dev)
        for fold in range(folds):
            held = torch.from_numpy(np.flatnonzero(fold_of == fold))
            rest = torch.from_numpy(np.flatnonzero(fold_of != fold))
            mark(None)
            training = host_counts.index_select(0, rest).numpy()
            held_dev = held.to(dev)
            tested = image.index_select(0, held_dev)
            mark('gather')
            _, _, mask, corrected, components, mean, masked_sizes = wt.prepReference(None, device=device, device_out=True, counts=training,
                                                                                     chrom_bins=sizes, drop=drop)
            mark('prep')
            job = NewrefJob(ctx, corrected, np.ascontiguousarray(masked_sizes, dtype=np.int64), int(refsize), _lib.SUM_SEQUENTIAL)
            indexes, distances = job.run()
            mark('newref')
            reference = wt.Reference(indexes.cpu().numpy(), distances.cpu().numpy(), sizes, masked_sizes, mask, mean, components,
                                     binsize=binsize, device=device)
            mark('reference')
            try:
                threshold[fold] = zThreshold([int(v) for v in masked_sizes], multitest, minzscore)
                cutoff[fold] = reference.cutoff
                for lo in range(0, len(held), step):
                    part, rows = tested[lo:lo + step], held_dev[lo:lo + step]
                    m = part.shape[0]
                    fold_calls = max_calls
                    while True:
                        rz, rr = torch.empty((m, n_total), **f64), torch.empty((m, n_total), **f64)
                        cz, sd = torch.empty((m, len(sel)), **f64), torch.empty((m,), **f64)
                        cl = torch.zeros((m, fold_calls, 5), **f64)
                        nc = torch.zeros((m,), dtype=torch.int32, device=dev)
                        rc = lib.wc_test_batch_dev(reference.ctx, stream, reference.handle, part.data_ptr(), m, float(threshold[fold]),
                                                   int(minrefbins), int(repeats), float(mineffectsize), _lib.ptr(sel), len(sel), fold_calls,
                                                   rz.data_ptr(), rr.data_ptr(), cz.data_ptr(), cl.data_ptr(), nc.data_ptr(), sd.data_ptr())
                        if rc == _lib.E_LIMIT and b"max_calls" in lib.wc_last_error() and fold_calls < reference.n_total:
                            fold_calls *= 4
                            continue
                        _lib.check(rc)
                        break
                    if fold_calls > max_calls:          # the cohort's slots grow to the largest room a fold needed
                        grown = torch.zeros((n, fold_calls, 5), **f64)
                        grown[:, :max_calls] = calls
                        calls, max_calls = grown, fold_calls
                    Z.index_copy_(0, rows, rz)
                    R.index_copy_(0, rows, rr)
                    cwz.index_copy_(0, rows, cz)
                    asdef.index_copy_(0, rows, sd)
                    n_calls.index_copy_(0, rows, nc)
                    calls[:, :fold_calls].index_copy_(0, rows, cl)
                mark('test')
            finally:
                reference.close()
        # the judging: once, over all rows in cohort order
        thr = torch.from_numpy(threshold[fold_of]).to(dev)
        shapes = _stats_args(n, sizes, sel, lengths)
        out = {key: torch.zeros(shape, dtype=torch.int32 if dtype == np.int32 else torch.int64 if dtype == np.int64 else torch.float64,
                                device=dev) for key, (shape, dtype) in shapes.items()}
        mark(None)
        _lib.check(lib.wc_crossval_stats_dev(ctx, stream, Z.data_ptr(), n_total, n, _lib.ptr(sizes), len(sizes), thr.data_ptr(),
                                             asdef.data_ptr(), calls.data_ptr(), n_calls.data_ptr(), max_calls, _lib.ptr(sel), len(sel),
                                             _lib.ptr(lengths), len(lengths), *[out[key].data_ptr() for key in STATS_KEYS]))
        mark('stats')
        if robust:
            robust_i = torch.zeros((n_total, 2), dtype=torch.int32, device=dev)
            robust_f = torch.zeros((n_total, 2), **f64)
            _lib.check(lib.wc_column_robust_dev(ctx, stream, Z.data_ptr(), n_total, n, n_total, robust_i.data_ptr(), robust_f.data_ptr()))
            mark('robust')
        result = {key: out[key].cpu().numpy() for key in STATS_KEYS}
        if robust:
            result.update(robust_i=robust_i.cpu().numpy(), robust_f=robust_f.cpu().numpy())
        counts_of = n_calls.cpu().numpy()
        rows_of = calls.cpu().numpy()
        if stage_ms is not None:
            torch.cuda.synchronize()
            for (_, before), (name, after) in zip(marks, marks[1:]):
                if name is not None:
                    stage_ms[name] = stage_ms.get(name, 0.0) + before.elapsed_time(after)
        if keep_results:
            result.update(Z=Z.cpu().numpy(), R=R.cpu().numpy(), results_cwz=cwz.cpu().numpy())
    result['rec_i'][:, 0] = fold_of
    listed = [np.concatenate([np.full((counts_of[i], 1), float(i)), rows_of[i, :counts_of[i]]], axis=1) for i in range(n)]
    result.update(fold_of=fold_of, threshold=threshold, cutoff=cutoff,
                  calls=np.concatenate(listed).reshape(-1, 6) if listed else np.zeros((0, 6)))
    return result


def heldOutResults(result, chrom_sizes):
    """Per sample the dict wt.test_batch returns (results_z / results_r per chromosome, results_cwz, results_calls, asdef)
    out of a crossval_batch result made with keep_results."""
    sizes = [int(v) for v in chrom_sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    calls = result['calls']
    out = []
    for i in range(len(result['fold_of'])):
        out.append(dict(
            results_z=[result['Z'][i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
            results_r=[result['R'][i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
            results_cwz=result['results_cwz'][i].copy(),
            results_calls=calls[calls[:, 0] == i, 1:].copy(),
            asdef=float(result['rec_f'][i, 0])))
    return out


# ------------------------------------------------------------------------------------------- the tables ----
def samplesText(names, rec_i, rec_f):
    """The per-sample table as tab separated text, columns SAMPLE_COLUMNS: the name, then fold, calls, call_bins, tested,
    over_hi, over_lo as whole numbers and asdef, the largest and the smallest z as repr writes them."""
    rec_i = np.asarray(rec_i).reshape(-1, 8)
    rec_f = np.asarray(rec_f, dtype=np.float64).reshape(-1, 4)
    if not (len(names) == len(rec_i) == len(rec_f)):
        raise ValueError('%d names, %d and %d records' % (len(names), len(rec_i), len(rec_f)))
    out = ['\t'.join(SAMPLE_COLUMNS)]
    for name, ri, rf in zip(names, rec_i, rec_f):
        out.append('\t'.join([str(name)] + [str(int(ri[k])) for k in (0, 1, 6, 2, 4, 5)] + [repr(float(rf[k])) for k in (0, 2, 3)]))
    return '\n'.join(out) + '\n'


def binsText(chrom_sizes, binsize, bins_i, bins_f, robust_f, listed):
    """The per-bin table of -robust as tab separated text, a line per bin of the layout, columns BIN_COLUMNS: the bin's
    chromosome, start and end in base pairs; tested and nonfinite (bins_i); median and spread = 1.4826 * mad (robust_f);
    mean and sd, formed here from bins_f's sums over the bin's n finite samples (sd = sqrt((sum z * z - n * mean * mean) /
    (n - 1)), clipped at 0), NaN below two; listed as 0 or 1.  Doubles as repr writes them."""
    from .blacklist import spreadOf
    bins_i = np.asarray(bins_i).reshape(-1, 6)
    bins_f = np.asarray(bins_f, dtype=np.float64).reshape(-1, 2)
    robust_f = np.asarray(robust_f, dtype=np.float64).reshape(-1, 2)
    spread = spreadOf(robust_f)
    out = ['\t'.join(BIN_COLUMNS)]
    b = 0
    for c, size in enumerate(int(v) for v in chrom_sizes):
        for g in range(size):
            n = int(bins_i[b, 0]) - int(bins_i[b, 1])
            mean = sd = float('nan')
            if n >= 2:
                mean = float(bins_f[b, 0]) / n
                sd = math.sqrt(max(0.0, (float(bins_f[b, 1]) - n * mean * mean) / (n - 1)))
            out.append('\t'.join([str(c + 1), str(g * int(binsize)), str((g + 1) * int(binsize)), str(int(bins_i[b, 0])),
                                  str(int(bins_i[b, 1])), repr(float(robust_f[b, 0])), repr(float(spread[b])), repr(mean), repr(sd),
                                  str(int(bool(listed[b])))]))
            b += 1
    return '\n'.join(out) + '\n'


def histQuantile(hist, q):
    """The q-quantile of one line of win_hist, linearly interpolated inside its slot; NaN when it falls into slot 0 or 129
    (the open ends) or the line is empty.  Slot k (1 .. 128) is [-16 + (k - 1) / 4, -16 + k / 4); the quantile lies in the
    first slot at which the running count reaches q * total."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    total = int(hist.sum())
    if total == 0:
        return float('nan')
    target, below = q * total, 0
    for k in range(len(hist)):
        if hist[k] and below + int(hist[k]) >= target:
            if k == 0 or k == len(hist) - 1:
                return float('nan')
            return -16.0 + (k - 1) / 4.0 + 0.25 * (target - below) / int(hist[k])
        below += int(hist[k])
    return float('nan')


def windowsTable(windows, win_n, win_i, win_hist, thresholds):
    """float64 [len(windows), 8], columns WINDOW_COLUMNS: per length its rows, windows, hi and lo (win_i);
    rate = (hi + lo) / windows; expected = sum_i win_n[i, L] * 2 * norm.sf(thresholds[i]) / windows, what independent N(0, 1)
    bins would give; spread = half the distance between the 15.87 % and 84.13 % quantiles of the histogram (histQuantile), 1
    for N(0, 1).  rate, expected and spread are NaN without windows, spread also when a quantile falls into an open end."""
    from scipy.stats import norm
    win_n = np.asarray(win_n, dtype=np.int64).reshape(-1, len(windows))
    win_i = np.asarray(win_i, dtype=np.int64).reshape(len(windows), 4)
    win_hist = np.asarray(win_hist, dtype=np.int64).reshape(len(windows), -1)
    tail = 2.0 * norm.sf(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    lines = []
    for at, length in enumerate(windows):
        rows, n, hi, lo = (int(v) for v in win_i[at])
        low, high = (histQuantile(win_hist[at], q) for q in SPREAD_QUANTILES)
        lines.append([length, rows, n, hi, lo, (hi + lo) / n if n else np.nan,
                      float((win_n[:, at] * tail).sum()) / n if n else np.nan, (high - low) / 2.0 if n else np.nan])
    return np.array(lines, dtype=np.float64).reshape(-1, len(WINDOW_COLUMNS))


def windowsText(table):
    """windowsTable as tab separated text: a header line, then a line per length; the whole numbers as such, the others
    as repr writes them (float() reads every one back bit for bit)."""
    out = ['\t'.join(WINDOW_COLUMNS)]
    for row in np.asarray(table, dtype=np.float64).reshape(-1, len(WINDOW_COLUMNS)):
        out.append('\t'.join([str(int(v)) for v in row[:5]] + [repr(float(v)) for v in row[5:]]))
    return '\n'.join(out) + '\n'
