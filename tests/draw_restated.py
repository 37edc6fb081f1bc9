"""The draws of `sensitivity` and `downsample` restated in numpy without the library (a helper module, not a conftest).
DESIGN.md 6h has the rule; integers only, so every statement is by bits.

    generator   Philox4x32-10, key (seed low word, seed high word)
    draw        B(c, f): read r (0 <= r < c) is kept when word r & 3 of block (c0 = bin within its chromosome,
                c1 = chromosome | tag << 16, c2 = r >> 2, c3 = row id) is below T = (f << 32) // 1 000 000; B counts them
    thinning    tag 1, row id = the base row, every depth from the same words
    spike       tag 2, row id = the trial's global plan row; c -> min(2^31 - 1, c * whole + B(c, frac)) with
                whole, frac = divmod(1 000 000 + ppm, 1 000 000)
"""
import numpy as np

INT_MAX = 2 ** 31 - 1
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG_THIN, TAG_SPIKE = 1, 2
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)


def philox(counters, key):
    """uint32 [n, 4] words of uint32 [n, 4] counters under key (k0, k1): two words, or uint32 [n, 2] for a key each."""
    c = np.array(counters, dtype=np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k = np.array(key, dtype=np.uint64).reshape(-1, 2)
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2             # (32 x 32 bits: below 2^64)
        c0, c1, c2, c3 = (p1 >> SHIFT) ^ c1 ^ k0, p1 & MASK, (p0 >> SHIFT) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def key_of(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def threshold(f_ppm):
    return (int(f_ppm) << 32) // 1000000


def kept_of_words(words, c, f_ppm):
    """B of the first c words of a flat word sequence (the rule on words written by hand)."""
    if f_ppm == 0:
        return 0
    return sum(1 for w in list(words)[:c] if int(w) < threshold(f_ppm))


def bin_words(c, bin_in_chrom, chrom, tag, row_id, seed):
    """uint32 [c]: the words of a bin's reads 0 .. c - 1."""
    blocks = (int(c) + 3) // 4
    counters = np.empty((blocks, 4), dtype=np.uint64)
    counters[:, 0] = bin_in_chrom
    counters[:, 1] = chrom | tag << 16
    counters[:, 2] = np.arange(blocks)
    counters[:, 3] = row_id
    return philox(counters, key_of(seed)).reshape(-1)[:int(c)]


def draw_segment(counts, first_bin, chrom, tag, row_id, seed, f_ppms):
    """int64 [len(f_ppms), n]: B(c, f) of counts [n] >= 0, the bins first_bin .. of chromosome `chrom`; one pass over the
    words serves every f."""
    counts = np.asarray(counts, dtype=np.int64)
    out = np.zeros((len(f_ppms), len(counts)), dtype=np.int64)
    blocks = (counts + 3) // 4
    total = int(blocks.sum())
    if total == 0 or all(f == 0 for f in f_ppms):
        return out
    owner = np.repeat(np.arange(len(counts)), blocks)
    begin = np.concatenate([[0], np.cumsum(blocks)])[:-1]
    counters = np.empty((total, 4), dtype=np.uint64)
    counters[:, 0] = first_bin + owner
    counters[:, 1] = chrom | tag << 16
    counters[:, 2] = np.arange(total) - begin[owner]
    counters[:, 3] = row_id
    words = philox(counters, key_of(seed)).astype(np.uint64)
    read = counters[:, 2].astype(np.int64)[:, None] * 4 + np.arange(4)[None, :]
    real = read < counts[owner][:, None]
    for k, f in enumerate(f_ppms):
        if f == 0:
            continue
        kept = ((words < np.uint64(threshold(f))) & real).sum(axis=1)
        out[k] = np.bincount(owner, weights=kept, minlength=len(counts)).astype(np.int64)
    return out


def thin(base, chrom_sizes, keep_ppm, seed, row_ids=None):
    """int32 [n_keep, n_base, n_total] of base int32 [n_base, n_total]; counts below 0 are copied."""
    base = np.asarray(base, dtype=np.int32)
    sizes = np.asarray(chrom_sizes, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    out = np.empty((len(keep_ppm),) + base.shape, dtype=np.int32)
    for b in range(base.shape[0]):
        row_id = b if row_ids is None else row_ids[b]
        for ci in range(len(sizes)):
            seg = base[b, offs[ci]:offs[ci + 1]].astype(np.int64)
            if not len(seg):
                continue
            drawn = draw_segment(np.maximum(seg, 0), 0, ci + 1, TAG_THIN, row_id, seed, list(keep_ppm))
            out[:, b, offs[ci]:offs[ci + 1]] = np.where(seg[None, :] < 0, seg[None, :], drawn)
    return out


def spike_draw(base, chrom_sizes, plan, seed, trial0=0):
    """(int32 [n_trials, n_total], saturated): the binomial spike of plan rows {base row, chromosome, first bin, bins, ppm},
    trial i drawing as row id trial0 + i."""
    base = np.asarray(base, dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(np.asarray(chrom_sizes, dtype=np.int64))])
    out = np.empty((len(plan), base.shape[1]), dtype=np.int32)
    saturated = 0
    for i, (b, chrom, first, bins, ppm) in enumerate(np.asarray(plan, dtype=np.int64).tolist()):
        out[i] = base[b]
        if ppm == 0:
            continue
        whole, frac = divmod(1000000 + ppm, 1000000)
        lo = int(offs[chrom - 1]) + first
        seg = base[b, lo:lo + bins].astype(np.int64)
        drawn = draw_segment(np.maximum(seg, 0), first, chrom, TAG_SPIKE, trial0 + i, seed, [frac])[0]
        val = np.maximum(seg, 0) * whole + drawn
        over = (seg >= 0) & (val > INT_MAX)
        saturated += int(over.sum())
        out[i, lo:lo + bins] = np.where(seg < 0, seg, np.minimum(val, INT_MAX)).astype(np.int32)
    return out, saturated

