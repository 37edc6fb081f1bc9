"""convertBam's filters and binning (tests/convert_restated.py, tests/convert_paired_restated.py) restated for reads that
arrive in SLICES: `feed` takes the carry in and gives the carry out, and the carry is exactly the state csrc/convert.hip
keeps between the slices of a run (wc_convert_begin .. wc_convert_finish):

  raw level     cur, cur_n      the chromosome of the last read fed (-1: none yet) and how many reads it has had: 1 or 2
                                (2: two and more); the first one is the read `sam_iter.next()` consumes
                last_pos        the position of the last read fed
                larp            the last position of the nearest chromosome in front of `cur` with at least two reads
                pe, me          paired mode: (pos, mate_pos) of the previous read that took part, (-1, -1) before the first
  kept level    run_chrom       the chromosome of the last kept read (-1: none yet)
                last_kept       its position
                run_len         the length of the open run, saturated at threshold + 1 (a run that has outgrown the
                                threshold is dead: only its last position matters)
                pend            while run_len <= threshold: the open run's positions, head first (never more than
                                max(threshold, 0)); threshold < 0: every kept read is counted at once, nothing is pending

tests/test_convert_bounded_cpu.py holds it against the whole-input restatements on random inputs and random cuts."""
import numpy as np

PROPER_PAIR, READ1 = 0x2, 0x40
COUNTERS = ("filter_rmdup", "filter_mapq", "pre_retro", "post_retro", "outside", "kept", "pair_fail")


def new_carry():
    return dict(cur=-1, cur_n=0, last_pos=-1, larp=-1, pe=-1, me=-1, run_chrom=-1, last_kept=0, run_len=0, pend=[])


def new_totals(n_bins):
    """(counts per chromosome, the seven counters)"""
    return [np.zeros(b, dtype=np.int32) for b in n_bins], dict((k, 0) for k in COUNTERS)


def _bin(totals, chrom, pos, binsize):
    counts, stats = totals
    b = int(pos / float(binsize))                       # int() truncates towards zero, as the reference's does
    if 0 <= b < len(counts[chrom]):
        counts[chrom][b] += 1
        stats["post_retro"] += 1
    else:
        stats["outside"] += 1                           # the reference raises IndexError here: the status word


def _close_run(carry, totals, binsize, threshold):
    if carry["run_len"] <= threshold:
        for p in carry["pend"]:
            _bin(totals, carry["run_chrom"], p, binsize)
    carry["pend"], carry["run_len"] = [], 0


def feed(carry, totals, reads, binsize, min_shift, threshold, min_mapq=1, paired=False):
    """One slice: reads[c] = (pos, mapq, flag, mate_pos) of chromosome c's reads in this slice (any of them empty).
    Returns the carry for the next slice; `carry` itself is left alone.  ValueError: the slice brings reads for a
    chromosome in front of one that has had reads."""
    s = dict(carry, pend=list(carry["pend"]))
    stats = totals[1]
    for c, (pos, mapq, flag, mate) in enumerate(reads):
        if len(pos) and c < s["cur"]:
            raise ValueError("reads of chromosome %d behind reads of chromosome %d" % (c, s["cur"]))
        for i in range(len(pos)):
            p, q = int(pos[i]), int(mapq[i])
            if c != s["cur"]:                           # the chromosome's first read: consumed
                if s["cur_n"] >= 2:
                    s["larp"] = s["last_pos"]
                s["cur"], s["cur_n"], s["last_pos"] = c, 1, p
                continue
            prev = s["larp"] if s["cur_n"] == 1 else s["last_pos"]
            s["cur_n"], s["last_pos"] = 2, p
            if paired:
                f = int(flag[i])
                if not (f & PROPER_PAIR and f & READ1):
                    stats["pair_fail"] += 1
                    continue
                m = int(mate[i])
                dup = p == s["pe"] and m == s["me"]
                s["pe"], s["me"] = p, m
            else:
                dup = p == prev
            stats["pre_retro"] += 1
            if dup:
                stats["filter_rmdup"] += 1
                continue
            if q < min_mapq:
                stats["filter_mapq"] += 1
                continue
            stats["kept"] += 1
            if threshold < 0:
                _bin(totals, c, p, binsize)
            else:
                if c != s["run_chrom"] or p - s["last_kept"] > min_shift:
                    _close_run(s, totals, binsize, threshold)
                s["run_len"] = min(s["run_len"] + 1, threshold + 1)
                s["pend"] = s["pend"] + [p] if s["run_len"] <= threshold else []
            s["run_chrom"], s["last_kept"] = c, p
    assert len(s["pend"]) <= max(threshold, 0) and (not s["pend"] or len(s["pend"]) == s["run_len"])
    return s


def finish(carry, totals, binsize, threshold):
    """Closes the open run; returns (counts per chromosome, counters)."""
    s = dict(carry, pend=list(carry["pend"]))
    if threshold >= 0:
        _close_run(s, totals, binsize, threshold)
    return totals


def cut(reads_by_chrom, cuts):
    """The slices of the concatenated input between the global read indices `cuts` (ascending, any of them equal):
    a list of per-chromosome lists of (pos, mapq, flag, mate) tuples."""
    sizes = [len(r[0]) for r in reads_by_chrom]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    edges = [0] + [int(c) for c in cuts] + [int(starts[-1])]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        piece = []
        for c, r in enumerate(reads_by_chrom):
            a = min(max(lo - starts[c], 0), sizes[c])
            b = min(max(hi - starts[c], 0), sizes[c])
            piece.append(tuple(np.asarray(x)[a:b] for x in r))
        out.append(piece)
    return out


def convert_sliced(n_bins, slices, binsize, min_shift, threshold, min_mapq=1, paired=False):
    """All slices through feed / finish: (counts per chromosome, counters, the largest number of pending positions)"""
    carry, totals = new_carry(), new_totals(n_bins)
    most = 0
    for piece in slices:
        carry = feed(carry, totals, piece, binsize, min_shift, threshold, min_mapq, paired)
        most = max(most, len(carry["pend"]))
    counts, stats = finish(carry, totals, binsize, threshold)
    return counts, stats, most
