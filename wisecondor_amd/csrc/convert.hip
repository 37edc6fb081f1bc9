// `convert`: the numeric part of convertBam (wisetools.py:116-217) for one BAM file's reads, all chromosomes in one call.
//
// What the reference's per-read loop computes, restated (tests/convert_restated.py; the reads of a chromosome are
// pos[ro[c] .. ro[c+1]), the first one is consumed uncounted by `sam_iter.next()`):
//   prev[i]  = pos[i - 1], and for the second read of a chromosome `larp`: the position of the last read of the nearest
//              earlier chromosome with at least two reads (-1 if none)
//   dup[i]   = pos[i] == prev[i];   keep[i] = !dup[i] && mapq[i] >= 1
//   k[]      = the kept positions in order; a run starts at the chromosome's first kept read and wherever
//              k[j] - k[j-1] > min_shift; a run of L reads is counted iff threshold < 0 || L <= threshold
//   counts[(int64)((double)pos / binsize)] += 1 for every counted read
// Everything is integer, so the order of accumulation is free.  Order between workgroups comes from kernel boundaries
// only (no workgroup waits for another one):
//   k_cv_tables   larp per chromosome from the offsets table                               (1 workgroup)
//   k_cv_flags    classes of CV_TILE reads per workgroup: kept count per tile, the filter counters
//   k_cv_scan<0>  exclusive sum of the tile counts                                          (1 workgroup)
//   k_cv_compact  kept positions -> kpos[], and the kept rank of every chromosome's first read -> koff[]
//   k_cv_heads    run heads of a tile of kpos[]: the tile's first and last head
//   k_cv_scan<1>, <2>  last head before / first head after every tile                       (1 workgroup each)
//   k_cv_count    run start / end of every kept read -> run length -> bin -> histogram
// Inside a tile everything is a wave ballot: reads are striped (round r, thread t -> tile_base + r * CV_BLOCK + t), so
// a (round, wave) pair is a SEGMENT of 64 consecutive reads, ranks are popcounts below the lane and the nearest head
// is a count of leading / trailing zeros of the head mask; 32 segment values per tile go through LDS.
// Positions are sorted, so the lanes of a segment hit one or two bins: equal bins are matched within the wave and
// one lane issues one atomicAdd per (segment, bin).
//
// The two other parameters of convertBam: `min_mapq` replaces the 1 of keep[i]; `demandPair` (paired mode,
// wisetools.py:160-183, tests/convert_paired_restated.py) is a second instance of the first kernels:
//   elig[i]  = flag[i] has 0x2 (proper pair) and 0x40 (first in pair); a counted read that is not eligible adds one to
//              pair_fail and touches nothing else
//   e(i)     = the nearest earlier eligible counted read, in ANY earlier chromosome (none: (-1, -1) is compared)
//   dup[i]   = pos[i] == pos[e] && mate_pos[i] == mate_pos[e];   keep[i] = elig[i] && !dup[i] && mapq[i] >= min_mapq
// so `larp` is not used; instead
//   k_cv_elig         the last eligible counted read of every tile
//   k_cv_scan<1>      the last eligible counted read before every tile                      (1 workgroup)
//   k_cv_flags<true>  e(i) from the segment's ballot, the tile's 32 segment values or that carry; gathers pos[e] and
//                     mate_pos[e]; writes the class of every read as a byte, which k_cv_compact<true> reads back
//                     (the plain mode recomputes the class there: it needs one neighbouring load, not a scan)
// From kpos[] on the two modes are the same kernels.
//
// The resumable form (wc_convert_begin / feed / finish; tests/convert_sliced_restated.py): the reads arrive in slices, in
// file order, and every kernel above has a second instance, CARRY, that reads the state the slices before left in
// device memory (CvCarry) -- the whole call launches the instances without it, as before:
//   raw level    cur, cur_n   the chromosome of the last read fed and its reads so far (1, or 2 for more): a slice's reads
//                             of `cur` continue it, none of them is the consumed first read
//                last_pos, larp   prev[] of the slice's first read of `cur`: larp while cur_n == 1, else last_pos; larp is
//                             the last position of the nearest chromosome in front of `cur` with at least two reads
//                pe, me       paired mode: pos and mate_pos of e(i) where the slice has no eligible counted read in front
//   kept level   run_chrom, last_kept   the chromosome and position of the last kept read
//                n_pend       the OPEN run (the last kept read's) waits, head first, at the front of the slice's kpos[] while
//                             it is no longer than the threshold: the slice's kept reads are ranked behind it and
//                             koff[c] = 0 up to run_chrom, so heads, run lengths and bins come out of the same ballots.
//                             A longer open run is dead: n_pend = 0, a kept read that continues it (k[j] - last_kept <=
//                             min_shift in run_chrom) is no head, finds no head in front of itself and is not counted.
//                             threshold < 0: every kept read is counted at once, nothing waits.
//   k_cv_slice   the slice's offsets table, a kernel argument, into device memory               (1 workgroup)
//   k_cv_count<CARRY>   leaves the reads of the open run (no head behind them) uncounted unless the slice is the closing one
//   k_cv_carry   the state for the next slice; the open run to the front of the OTHER kpos[]      (1 workgroup)
// The carry is at most min(longest run, max(threshold, 0)) positions; the seven counters are 64-bit sums over the slices.
#include "ctx.h"

#include <limits.h>

#include <algorithm>

#define CV_BLOCK 256
#define CV_ROUNDS 8
#define CV_TILE (CV_BLOCK * CV_ROUNDS)      // reads per workgroup; exported by wc_convert_tile_reads()
#define CV_SEGS (CV_TILE / 64)
#define CV_SCAN_BLOCK 1024
static_assert(CV_BLOCK == 256 && CV_SEGS == 32, "segment = (round, wave): 4 waves per round, 32 segments fit half a wave");

namespace {

// device image of the small tables (int32 each)
struct CvTab {
    int ro[WC_CV_MAX_CHROM + 1];      // first read of chromosome c; ro[n_chrom] = number of reads
    int bo[WC_CV_MAX_CHROM + 1];      // first bin of chromosome c in counts_out
    int larp[WC_CV_MAX_CHROM + 1];    // `prev` of the chromosome's second read
    int koff[WC_CV_MAX_CHROM + 1];    // kept reads in front of chromosome c; koff[n_chrom] = kept reads in all
};

// the state a run (wc_convert_begin .. wc_convert_finish) carries from one slice of reads to the next, in device memory:
// read by the slice's kernels, written by the last one (k_cv_carry) only
struct CvCarry {
    int cur;          // chromosome of the last read fed (-1: none yet); a slice's reads of it continue it
    int cur_n;        // reads it has had: 1, or 2 for two and more
    int last_pos;     // position of the last read fed
    int larp;         // last position of the nearest chromosome in front of `cur` with at least two reads (-1: none)
    int pe, me;       // paired mode: (pos, mate_pos) of the previous read that took part, (-1, -1) before the first
    int run_chrom;    // chromosome of the last kept read (-1: none yet)
    int last_kept;    // its position
    int n_pend;       // kept reads of the open run waiting at the front of the next slice's kpos[] (the whole run, its
                      // head first); 0 with run_chrom >= 0: the open run has outgrown the threshold and is dead
    int m_slice;      // kept reads of the slice in flight (k_cv_scan<0>'s total)
    int max_pend;     // the largest n_pend so far
};

// largest c in [0, n] with tab[c] <= i (tab ascending, tab[0] <= i): with equal entries (empty chromosomes) the last
__device__ __forceinline__ int cv_find(const int *tab, int n, int i) {
    int lo = 0, hi = n + 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int cv_lane() { return (int)(threadIdx.x & 63); }

// class of read i: 0 not a counted read (a chromosome's consumed first read, or past the end), 1 duplicate,
// 2 mapping quality below min_mapq, 3 kept (paired mode adds 4: not eligible); p = its position
// CARRY (a slice of a run): the reads of chromosome `cont` continue it, the first of them follows cont_prev
template <bool CARRY>
__device__ __forceinline__ int cv_class(const int32_t *__restrict__ pos, const uint8_t *__restrict__ mapq, const int *s_ro,
                                        const int *s_larp, int n_chrom, int i, int n, int min_mapq, int cont, int cont_prev,
                                        int &p) {
    p = 0;
    if (i >= n) return 0;
    const int c = cv_find(s_ro, n_chrom, i);
    const int first = s_ro[c];
    int prev;
    if (CARRY && c == cont) {
        p = pos[i];
        prev = i == first ? cont_prev : pos[i - 1];
    } else {
        if (i == first) return 0;
        p = pos[i];
        prev = i == first + 1 ? s_larp[c] : pos[i - 1];
    }
    if (p == prev) return 1;
    return (int)mapq[i] < min_mapq ? 2 : 3;
}

// paired mode: is read i an eligible counted read?  counted: is it a counted read at all
template <bool CARRY>
__device__ __forceinline__ bool cv_elig(const uint16_t *__restrict__ flag, const int *s_ro, int n_chrom, int i, int n, int cont,
                                        bool &counted) {
    counted = false;
    if (i >= n) return false;
    const int c = cv_find(s_ro, n_chrom, i);
    if (i == s_ro[c] && !(CARRY && c == cont)) return false;
    counted = true;
    const unsigned f = flag[i];
    return (f & 0x2u) && (f & 0x40u);
}

// CARRY: chromosome carry->cur has had carry->cur_n reads already and the chromosomes in front of it have none in the
// slice: behind them the search ends at carry->larp
template <bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_tables(const int32_t *__restrict__ pos, CvTab *tab, int n_chrom,
                                                       const CvCarry *__restrict__ carry) {
    const int cur = CARRY ? carry->cur : 0;
    for (int cc = (int)threadIdx.x; cc <= n_chrom; cc += CV_BLOCK) {
        int l = CARRY ? carry->larp : -1;
        for (int e = cc - 1; e >= (CARRY && cur > 0 ? cur : 0); --e) {
            const int here = tab->ro[e + 1] - tab->ro[e];
            if (here + (CARRY && e == cur ? carry->cur_n : 0) >= 2) {
                l = !CARRY || here ? pos[tab->ro[e + 1] - 1] : carry->last_pos;
                break;
            }
        }
        tab->larp[cc] = l;
    }
}

__device__ __forceinline__ void cv_load_tab(const int *src, int *dst, int n) {
    for (int i = (int)threadIdx.x; i < n; i += CV_BLOCK) dst[i] = src[i];
}

template <int MODE, bool REVERSE> __device__ __forceinline__ void cv_seg_scan(const int *s_in, int *s_out, int seed);

// paired mode: the last eligible counted read of the tile (-1: none)
template <bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_elig(const uint16_t *__restrict__ flag, const CvTab *__restrict__ tab,
                                                     int n_chrom, int n, const CvCarry *__restrict__ carry,
                                                     int *__restrict__ tile_elast) {
    const int cont = CARRY ? carry->cur : -1;
    __shared__ int s_ro[WC_CV_MAX_CHROM + 1];
    __shared__ int s_last;
    cv_load_tab(tab->ro, s_ro, n_chrom + 1);
    if (threadIdx.x == 0) s_last = -1;
    wc_sync();
    if (CARRY) n = s_ro[n_chrom];                       // a slice's table may be born on the device: `n` is a bound then
    const int base = (int)blockIdx.x * CV_TILE;
    const int w = (int)threadIdx.x >> 6;
    int last = -1;                                  // wave-uniform; the rounds ascend, so the latest hit is the largest
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int seg_base = base + r * CV_BLOCK + w * 64;
        bool counted;
        const unsigned long long mk = __ballot(cv_elig<CARRY>(flag, s_ro, n_chrom, seg_base + cv_lane(), n, cont, counted));
        if (mk) last = seg_base + 63 - __clzll((long long)mk);
    }
    if (cv_lane() == 0 && last >= 0) atomicMax(&s_last, last);
    wc_sync();
    if (threadIdx.x == 0) tile_elast[blockIdx.x] = s_last;
}

// PAIRED: flag, mate, carry_e (the last eligible counted read before the tile) and cls_out (a byte per read of the
// tile, reads past the end included) are used; otherwise they may be NULL.  CARRY: a slice of a run
template <bool PAIRED, bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_flags(const int32_t *__restrict__ pos, const uint8_t *__restrict__ mapq,
                                                      const uint16_t *__restrict__ flag, const int32_t *__restrict__ mate,
                                                      const CvTab *__restrict__ tab, int n_chrom, int n, int min_mapq,
                                                      const int *__restrict__ carry_e, uint8_t *__restrict__ cls_out,
                                                      int *__restrict__ tile_keep, unsigned long long *stats,
                                                      const CvCarry *__restrict__ carry) {
    const int cont = CARRY ? carry->cur : -1;
    const int cont_prev = CARRY && !PAIRED ? (carry->cur_n == 1 ? carry->larp : carry->last_pos) : -1;
    __shared__ int s_ro[WC_CV_MAX_CHROM + 1], s_larp[WC_CV_MAX_CHROM + 1];
    __shared__ int s_elast[CV_SEGS], s_ebefore[CV_SEGS];
    __shared__ int s_cnt[4];
    cv_load_tab(tab->ro, s_ro, n_chrom + 1);
    if (!PAIRED) cv_load_tab(tab->larp, s_larp, n_chrom + 1);
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    wc_sync();
    if (CARRY) n = s_ro[n_chrom];
    const int base = (int)blockIdx.x * CV_TILE;
    int n_dup = 0, n_low = 0, n_keep = 0, n_fail = 0;       // wave-uniform: popcounts of ballots
    if (PAIRED) {
        const int lane = cv_lane(), w = (int)threadIdx.x >> 6;
        unsigned long long emask[CV_ROUNDS];
        unsigned counted_bits = 0;
#pragma unroll
        for (int r = 0; r < CV_ROUNDS; ++r) {
            const int seg_base = base + r * CV_BLOCK + w * 64;
            bool counted;
            emask[r] = __ballot(cv_elig<CARRY>(flag, s_ro, n_chrom, seg_base + lane, n, cont, counted));
            if (counted) counted_bits |= 1u << r;
            if (lane == 0) s_elast[r * (CV_BLOCK / 64) + w] = emask[r] ? seg_base + 63 - __clzll((long long)emask[r]) : -1;
        }
        wc_sync();
        if (w == 0) cv_seg_scan<1, false>(s_elast, s_ebefore, carry_e[blockIdx.x]);
        wc_sync();
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int r = 0; r < CV_ROUNDS; ++r) {
            const int seg_base = base + r * CV_BLOCK + w * 64;
            const int i = seg_base + lane;
            int cls = ((counted_bits >> r) & 1u) ? 4 : 0;
            if ((emask[r] >> lane) & 1ull) {
                const unsigned long long lo = emask[r] & below;
                const int e = lo ? seg_base + 63 - __clzll((long long)lo) : s_ebefore[r * (CV_BLOCK / 64) + w];
                int pe = -1, me = -1;                       // no earlier eligible read: (-1, -1) is compared as it stands
                if (e >= 0) {
                    pe = pos[e];
                    me = mate[e];
                } else if (CARRY) {                         // it lies in an earlier slice
                    pe = carry->pe;
                    me = carry->me;
                }
                cls = (pos[i] == pe && mate[i] == me) ? 1 : ((int)mapq[i] < min_mapq ? 2 : 3);
            }
            cls_out[i] = (uint8_t)cls;
            n_dup += __popcll(__ballot(cls == 1));
            n_low += __popcll(__ballot(cls == 2));
            n_keep += __popcll(__ballot(cls == 3));
            n_fail += __popcll(__ballot(cls == 4));
        }
    } else {
#pragma unroll
        for (int r = 0; r < CV_ROUNDS; ++r) {
            const int i = base + r * CV_BLOCK + (int)threadIdx.x;
            int p;
            const int cls = cv_class<CARRY>(pos, mapq, s_ro, s_larp, n_chrom, i, n, min_mapq, cont, cont_prev, p);
            n_dup += __popcll(__ballot(cls == 1));
            n_low += __popcll(__ballot(cls == 2));
            n_keep += __popcll(__ballot(cls == 3));
        }
    }
    if (cv_lane() == 0) {
        atomicAdd(&s_cnt[0], n_dup);
        atomicAdd(&s_cnt[1], n_low);
        atomicAdd(&s_cnt[2], n_keep);
        if (PAIRED) atomicAdd(&s_cnt[3], n_fail);
    }
    wc_sync();
    if (threadIdx.x == 0) {
        tile_keep[blockIdx.x] = s_cnt[2];
        if (s_cnt[0]) atomicAdd(&stats[0], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&stats[1], (unsigned long long)s_cnt[1]);
        // pre_retro: every read but the consumed first one of each chromosome (paired: every eligible one of them)
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2];
        if (total) atomicAdd(&stats[2], (unsigned long long)total);
        if (PAIRED && s_cnt[3]) atomicAdd(&stats[6], (unsigned long long)s_cnt[3]);
    }
}

// One workgroup walks `in` in chunks.  MODE 0: out[t] = sum of in[0 .. t), *total = the whole sum; MODE 1: out[t] = max of
// in[0 .. t) (-1 when empty); MODE 2: out[t] = min of in(t .. n) (INT_MAX when empty).
template <int MODE> __device__ __forceinline__ int cv_op(int a, int b) {
    if (MODE == 0) return a + b;
    if (MODE == 1) return a > b ? a : b;
    return a < b ? a : b;
}
template <int MODE>
__global__ void __launch_bounds__(CV_SCAN_BLOCK) k_cv_scan(const int *__restrict__ in, int n, int *__restrict__ out,
                                                          int *total) {
    __shared__ int s_wave[CV_SCAN_BLOCK / 64];
    __shared__ int s_vals[CV_SCAN_BLOCK];
    const int ident = MODE == 0 ? 0 : (MODE == 1 ? -1 : INT_MAX);
    const int tid = (int)threadIdx.x, lane = cv_lane(), w = tid >> 6;
    int carry = ident;
    for (int base = 0; base < n; base += CV_SCAN_BLOCK) {
        const int k = base + tid;
        const int idx = MODE == 2 ? n - 1 - k : k;
        int v = k < n ? in[idx] : ident;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v = cv_op<MODE>(v, t);
        }
        if (lane == 63) s_wave[w] = v;
        wc_sync();
        int pre = ident;
        for (int g = 0; g < w; ++g) pre = cv_op<MODE>(pre, s_wave[g]);
        v = cv_op<MODE>(v, pre);
        s_vals[tid] = v;
        wc_sync();
        const int excl = cv_op<MODE>(tid ? s_vals[tid - 1] : ident, carry);
        if (k < n) out[idx] = excl;
        carry = cv_op<MODE>(carry, s_vals[CV_SCAN_BLOCK - 1]);
        wc_sync();                                  // the next chunk overwrites s_wave / s_vals
    }
    if (MODE == 0 && tid == 0 && total) *total = carry;
}

// exclusive prefix of the 32 segment values of a tile by one whole wave (lanes 0..31 hold a segment each), seeded with
// `seed`; REVERSE: suffix (the segments behind the lane's own)
template <int MODE, bool REVERSE> __device__ __forceinline__ void cv_seg_scan(const int *s_in, int *s_out, int seed) {
    const int lane = cv_lane();
    const int ident = MODE == 0 ? 0 : (MODE == 1 ? -1 : INT_MAX);
    const int at = (REVERSE ? CV_SEGS - 1 - lane : lane) & (CV_SEGS - 1);
    int v = lane < CV_SEGS ? s_in[at] : ident;
#pragma unroll
    for (int d = 1; d < CV_SEGS; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v = cv_op<MODE>(v, t);
    }
    int excl = __shfl_up(v, 1);
    if (lane == 0) excl = ident;
    if (lane < CV_SEGS) s_out[at] = cv_op<MODE>(excl, seed);
}

// PAIRED: the class comes from cls_in (k_cv_flags<true>), mapq and min_mapq are not used.  CARRY: the open run's
// carry->n_pend positions are in kpos[] already, the slice's kept reads go behind them; they belong to chromosome
// carry->run_chrom, which lies at or in front of the slice's first
template <bool PAIRED, bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_compact(const int32_t *__restrict__ pos, const uint8_t *__restrict__ mapq,
                                                        const uint8_t *__restrict__ cls_in, CvTab *tab, int n_chrom, int n,
                                                        int min_mapq, const int *__restrict__ tile_off,
                                                        int32_t *__restrict__ kpos, const CvCarry *__restrict__ carry) {
    const int cont = CARRY ? carry->cur : -1;
    const int cont_prev = CARRY && !PAIRED ? (carry->cur_n == 1 ? carry->larp : carry->last_pos) : -1;
    const int n_pend = CARRY ? carry->n_pend : 0, run_chrom = CARRY ? carry->run_chrom : -1;
    __shared__ int s_ro[WC_CV_MAX_CHROM + 1], s_larp[WC_CV_MAX_CHROM + 1];
    __shared__ int s_seg[CV_SEGS], s_segoff[CV_SEGS];
    cv_load_tab(tab->ro, s_ro, n_chrom + 1);
    if (!PAIRED) cv_load_tab(tab->larp, s_larp, n_chrom + 1);
    wc_sync();
    if (CARRY) n = s_ro[n_chrom];
    const int base = (int)blockIdx.x * CV_TILE;
    const int lane = cv_lane(), w = (int)threadIdx.x >> 6;
    int p[CV_ROUNDS];
    unsigned long long mask[CV_ROUNDS];
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int i = base + r * CV_BLOCK + (int)threadIdx.x;
        int cls;
        if (PAIRED) {
            cls = cls_in[i];
            p[r] = cls == 3 ? pos[i] : 0;
        } else {
            cls = cv_class<CARRY>(pos, mapq, s_ro, s_larp, n_chrom, i, n, min_mapq, cont, cont_prev, p[r]);
        }
        mask[r] = __ballot(cls == 3);
        if (lane == 0) s_seg[r * (CV_BLOCK / 64) + w] = __popcll(mask[r]);
    }
    wc_sync();
    if (w == 0) cv_seg_scan<0, false>(s_seg, s_segoff, tile_off[blockIdx.x] + n_pend);
    wc_sync();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int i = base + r * CV_BLOCK + (int)threadIdx.x;
        const int rank = s_segoff[r * (CV_BLOCK / 64) + w] + __popcll(mask[r] & below);     // kept reads in front of i
        if ((mask[r] >> lane) & 1ull) kpos[rank] = p[r];
        if (i <= n) {
            // i opens a chromosome (or several empty ones and one more; i == n: the end of the table)
            for (int c = cv_find(s_ro, n_chrom, i); c >= 0 && s_ro[c] == i; --c)
                tab->koff[c] = CARRY && c <= run_chrom ? 0 : rank;
        }
    }
}

// is kept read j (< the number of kept reads) the head of a run?  c = its chromosome.  CARRY: with no pending
// positions in front, the first kept read of chromosome run_chrom follows last_kept (and then belongs to a dead run)
template <bool CARRY>
__device__ __forceinline__ bool cv_head(const int32_t *__restrict__ kpos, const int *s_koff, int n_chrom, int j, int min_shift,
                                        int run_chrom, int n_pend, int last_kept, int &c) {
    c = cv_find(s_koff, n_chrom, j);
    if (j == s_koff[c]) {
        if (CARRY && c == run_chrom && n_pend == 0) return (long long)kpos[j] - (long long)last_kept > (long long)min_shift;
        return true;
    }
    return (long long)kpos[j] - (long long)kpos[j - 1] > (long long)min_shift;
}

template <bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_heads(const int32_t *__restrict__ kpos, const CvTab *__restrict__ tab,
                                                      int n_chrom, int min_shift, int *__restrict__ tile_last,
                                                      int *__restrict__ tile_first, const CvCarry *__restrict__ carry) {
    const int run_chrom = CARRY ? carry->run_chrom : -1, n_pend = CARRY ? carry->n_pend : 0;
    const int last_kept = CARRY ? carry->last_kept : 0;
    __shared__ int s_koff[WC_CV_MAX_CHROM + 1];
    __shared__ int s_last[CV_SEGS], s_first[CV_SEGS];
    cv_load_tab(tab->koff, s_koff, n_chrom + 1);
    wc_sync();
    const int m = s_koff[n_chrom];
    const int base = (int)blockIdx.x * CV_TILE;
    const int lane = cv_lane(), w = (int)threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int seg_base = base + r * CV_BLOCK + w * 64;
        const int j = seg_base + lane;
        int c = 0;
        const bool head = j < m && cv_head<CARRY>(kpos, s_koff, n_chrom, j, min_shift, run_chrom, n_pend, last_kept, c);
        const unsigned long long mk = __ballot(head);
        if (lane == 0) {
            s_last[r * (CV_BLOCK / 64) + w] = mk ? seg_base + 63 - __clzll((long long)mk) : -1;
            s_first[r * (CV_BLOCK / 64) + w] = mk ? seg_base + __ffsll((long long)mk) - 1 : INT_MAX;
        }
    }
    wc_sync();
    if (threadIdx.x == 0) {
        int last = -1, first = INT_MAX;
        for (int g = 0; g < CV_SEGS; ++g) {
            last = s_last[g] > last ? s_last[g] : last;
            first = s_first[g] < first ? s_first[g] : first;
        }
        tile_last[blockIdx.x] = last;
        tile_first[blockIdx.x] = first;
    }
}

// CARRY: a read without a head in front of it (start < 0) continues a dead run; a run without a head behind it is
// open: unless the slice is the closing one (`closing`), its reads are left to k_cv_carry and the next slice
template <bool CARRY>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_count(const int32_t *__restrict__ kpos, const CvTab *__restrict__ tab,
                                                      int n_chrom, int min_shift, int threshold, double binsize,
                                                      const int *__restrict__ carry_last, const int *__restrict__ carry_next,
                                                      int32_t *counts, unsigned long long *stats,
                                                      const CvCarry *__restrict__ carry, int closing) {
    const int run_chrom = CARRY ? carry->run_chrom : -1, n_pend = CARRY ? carry->n_pend : 0;
    const int last_kept = CARRY ? carry->last_kept : 0;
    __shared__ int s_koff[WC_CV_MAX_CHROM + 1], s_bo[WC_CV_MAX_CHROM + 1];
    __shared__ int s_last[CV_SEGS], s_first[CV_SEGS], s_before[CV_SEGS], s_after[CV_SEGS];
    __shared__ int s_cnt[2];
    cv_load_tab(tab->koff, s_koff, n_chrom + 1);
    cv_load_tab(tab->bo, s_bo, n_chrom + 1);
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    wc_sync();
    const int m = s_koff[n_chrom];
    const int base = (int)blockIdx.x * CV_TILE;
    if (base >= m) return;                              // (the whole workgroup: m is uniform)
    const int lane = cv_lane(), w = (int)threadIdx.x >> 6;
    unsigned long long mask[CV_ROUNDS];
    int chrom[CV_ROUNDS];
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int seg_base = base + r * CV_BLOCK + w * 64;
        const int j = seg_base + lane;
        chrom[r] = 0;
        const bool head = j < m && cv_head<CARRY>(kpos, s_koff, n_chrom, j, min_shift, run_chrom, n_pend, last_kept, chrom[r]);
        mask[r] = __ballot(head);
        if (lane == 0) {
            s_last[r * (CV_BLOCK / 64) + w] = mask[r] ? seg_base + 63 - __clzll((long long)mask[r]) : -1;
            s_first[r * (CV_BLOCK / 64) + w] = mask[r] ? seg_base + __ffsll((long long)mask[r]) - 1 : INT_MAX;
        }
    }
    wc_sync();
    if (w == 0) cv_seg_scan<1, false>(s_last, s_before, carry_last[blockIdx.x]);
    if (w == 1) cv_seg_scan<2, true>(s_first, s_after, carry_next[blockIdx.x]);
    wc_sync();
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;     // this lane and the ones below
    int n_counted = 0, n_outside = 0;
#pragma unroll
    for (int r = 0; r < CV_ROUNDS; ++r) {
        const int seg = r * (CV_BLOCK / 64) + w;
        const int seg_base = base + r * CV_BLOCK + w * 64;
        const int j = seg_base + lane;
        const unsigned long long lo = mask[r] & upto, hi = mask[r] & ~upto;
        const int start = lo ? seg_base + 63 - __clzll((long long)lo) : s_before[seg];
        int end = hi ? seg_base + __ffsll((long long)hi) - 1 : s_after[seg];
        end = end < m ? end : m;
        int key = -1;                                   // the read's bin in counts[], -1: nothing to add
        bool outside = false;
        bool counted = threshold < 0 || end - start <= threshold;
        if (CARRY && threshold >= 0 && (start < 0 || (end == m && !closing))) counted = false;
        if (j < m && counted) {
            const int c = chrom[r];
            const double q = (double)kpos[j] / binsize;
            const int n_bins = s_bo[c + 1] - s_bo[c];
            if (q >= 0.0 && q < (double)n_bins) key = s_bo[c] + (int)(long long)q;
            else if (q > -1.0 && q < 0.0 && n_bins > 0) key = s_bo[c];      // int() truncates towards zero
            else outside = true;
        }
        n_outside += __popcll(__ballot(outside));
        unsigned long long todo = __ballot(key >= 0);
        n_counted += __popcll(todo);
        while (todo) {                                  // (wave-uniform) one atomic per distinct bin of the segment
            const int leader = __ffsll((long long)todo) - 1;
            const int b = __shfl(key, leader);
            const unsigned long long same = __ballot(key == b);
            if (lane == leader) atomicAdd(&counts[b], (int)__popcll(same));
            todo &= ~same;
        }
    }
    if (lane == 0) {
        atomicAdd(&s_cnt[0], n_counted);
        atomicAdd(&s_cnt[1], n_outside);
    }
    wc_sync();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&stats[3], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&stats[4], (unsigned long long)s_cnt[1]);
    }
}

// The first kernel of a slice whose offsets table comes from the host: the table travels as a kernel argument, so the
// feed neither waits for a copy nor keeps host memory alive
struct CvRo {
    int ro[WC_CV_MAX_CHROM + 1];
};
__global__ void __launch_bounds__(CV_BLOCK) k_cv_slice(CvTab *tab, const CvRo table, int n_chrom) {
    for (int c = (int)threadIdx.x; c <= n_chrom; c += CV_BLOCK) tab->ro[c] = table.ro[c];
}

// The last kernel of a slice, one workgroup: the carry for the next slice.  Every thread reads the old state, then
// thread 0 alone writes the new one (plain vector stores).  The open run -- from the slice's last head h to its last
// kept read -- moves to the front of the next slice's kpos[] while it is no longer than the threshold; a longer one is
// dead: only its last position is kept.
template <bool PAIRED>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_carry(const int32_t *__restrict__ pos, const int32_t *__restrict__ mate,
                                                      const CvTab *__restrict__ tab, int n_chrom, int threshold,
                                                      const int *__restrict__ tile_last, int n_ktiles,
                                                      const int *__restrict__ tile_elast, int n_tiles,
                                                      const int32_t *__restrict__ kpos, int32_t *__restrict__ kpos_next,
                                                      CvCarry *carry, unsigned long long *stats) {
    __shared__ int s_h, s_e;
    if (threadIdx.x == 0) {
        s_h = -1;
        s_e = -1;
    }
    wc_sync();
    int h = -1, e = -1;
    for (int t = (int)threadIdx.x; t < n_ktiles; t += CV_BLOCK) h = tile_last[t] > h ? tile_last[t] : h;
    if (PAIRED)
        for (int t = (int)threadIdx.x; t < n_tiles; t += CV_BLOCK) e = tile_elast[t] > e ? tile_elast[t] : e;
    if (h >= 0) atomicMax(&s_h, h);
    if (PAIRED && e >= 0) atomicMax(&s_e, e);
    const CvCarry old = *carry;
    const int n = tab->ro[n_chrom], m = tab->koff[n_chrom];
    wc_sync();
    h = s_h;
    e = s_e;
    const int open = m - h;                             // (h >= 0) reads of the open run, the pending ones included
    const bool alive = threshold >= 0 && m > 0 && h >= 0 && open <= threshold;
    if (alive)
        for (int k = (int)threadIdx.x; k < open; k += CV_BLOCK) kpos_next[k] = kpos[h + k];
    if (threadIdx.x != 0) return;
    CvCarry next = old;
    if (n > 0) {
        const int c = cv_find(tab->ro, n_chrom, n - 1);     // the chromosome of the slice's last read
        const int total = tab->ro[c + 1] - tab->ro[c] + (c == old.cur ? old.cur_n : 0);
        next.cur = c;
        next.cur_n = total < 2 ? total : 2;
        next.last_pos = pos[n - 1];
        if (!PAIRED) next.larp = tab->larp[c];
    }
    if (PAIRED && e >= 0) {
        next.pe = pos[e];
        next.me = mate[e];
    }
    if (m > 0) {
        next.run_chrom = cv_find(tab->koff, n_chrom, m - 1);
        next.last_kept = kpos[m - 1];
        next.n_pend = alive ? open : 0;
        next.max_pend = next.n_pend > old.max_pend ? next.n_pend : old.max_pend;
    }
    next.m_slice = 0;
    *carry = next;
    stats[5] += (unsigned long long)(m - old.n_pend);   // kept by the first two filters: 64-bit over the slices
}

}  // namespace

// A resumable convert (wc_convert_begin): its own tables, tile words, class bytes and two kpos[] (a slice's kept reads
// go behind the open run that the slice before left at the front of the other one), the counts, the counters, the carry
struct wc_convert_run {
    wc_ctx *ctx = nullptr;
    int n_chrom = 0, min_shift = 0, threshold = 0, min_mapq = 0;
    bool paired = false, finished = false;
    double binsize = 0.0;
    int64_t bins = 0;
    int host_cur = -1;              // the last chromosome that got reads (the order check of the host-table feeds)
    int64_t pend_bound = 0;         // no more than this many positions are pending: min(max(threshold, 0), reads fed)
    int64_t slices = 0;             // slices that went through the kernels
    int at = 0;                     // which kpos[] holds the pending positions
    wc::DevBuf tab, tiles, cls, kpos[2], out, carry;        // out: 8 counters, then the counts
    wc::DevBuf st_pos, st_mapq, st_flag, st_mate;           // staging of the host form
    int64_t device_bytes() const {
        return (int64_t)(tab.bytes + tiles.bytes + cls.bytes + kpos[0].bytes + kpos[1].bytes + out.bytes + carry.bytes +
                         st_pos.bytes + st_mapq.bytes + st_flag.bytes + st_mate.bytes);
    }
    ~wc_convert_run() {
        for (wc::DevBuf *b : {&tab, &tiles, &cls, &kpos[0], &kpos[1], &out, &carry, &st_pos, &st_mapq, &st_flag, &st_mate})
            b->release();
    }
};

namespace {

// grow `buf` to `want` bytes and keep its first `keep` bytes (the pending positions); rare: the buffers are reserved
// for the largest slice so far
int cv_grow_keep(wc::DevBuf &buf, size_t want, size_t keep, hipStream_t stream) {
    if (want <= buf.bytes) return WC_OK;
    if (!buf.p || !keep) return buf.reserve(want);
    wc::DevBuf bigger;
    int rc;
    if ((rc = bigger.reserve(want))) return rc;
    keep = keep < buf.bytes ? keep : buf.bytes;
    WC_HIP(hipMemcpyAsync(bigger.p, buf.p, keep, hipMemcpyDeviceToDevice, stream));
    WC_HIP(hipStreamSynchronize(stream));
    buf.release();
    buf = bigger;
    return WC_OK;
}

struct CvTiles {                     // the eight words per tile of a pass: n ints each, side by side in one buffer
    int *keep, *off, *last, *first, *carry_last, *carry_next, *elast, *carry_e;
};
CvTiles cv_tiles(int *b, int n) { return {b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n, b + 6 * n, b + 7 * n}; }

// One pass of the kernels over a whole call's or a slice's reads; buffers, tables and zeroed outputs are the caller's
struct CvPass {
    hipStream_t stream;
    const int32_t *pos;
    const uint8_t *mapq;
    const uint16_t *flag;           // flag, mate_pos: the paired mode only
    const int32_t *mate_pos;
    CvTab *tab;
    int n_chrom, n, n_tiles, n_ktiles;  // tiles of the reads (read n is the end marker); of the kept reads and the pending ones
    CvTiles tiles;                  // of n_ktiles
    uint8_t *cls;                  // paired mode: a byte for every read of n_tiles whole tiles (no bound in the kernels)
    int32_t *kpos, *counts;
    int min_mapq, min_shift, threshold;
    double binsize;
    bool paired;
    unsigned long long *stats;
    int *kept_total;                // where k_cv_scan<0> leaves the number of kept reads
    const CvCarry *carry;           // CARRY: the state the slices before left; NULL without
    int closing;                    // CARRY: 1 for the empty slice of wc_convert_finish, which counts the open run
};

// the launch sequence of the file's head comment; CARRY: the instances that read the carry
template <bool CARRY> int cv_launch(const CvPass &p) {
    const int n_chrom = p.n_chrom, n = p.n, n_tiles = p.n_tiles, n_ktiles = p.n_ktiles;
    const hipStream_t stream = p.stream;
    const CvTab *tab = p.tab;
    const CvCarry *cin = p.carry;
    const CvTiles &t = p.tiles;
    if (p.paired) {
        hipLaunchKernelGGL(k_cv_elig<CARRY>, dim3(n_tiles), dim3(CV_BLOCK), 0, stream, p.flag, tab, n_chrom, n, cin, t.elast);
        hipLaunchKernelGGL(k_cv_scan<1>, dim3(1), dim3(CV_SCAN_BLOCK), 0, stream, (const int *)t.elast, n_tiles, t.carry_e,
                           (int *)nullptr);
        hipLaunchKernelGGL((k_cv_flags<true, CARRY>), dim3(n_tiles), dim3(CV_BLOCK), 0, stream, p.pos, p.mapq, p.flag,
                           p.mate_pos, tab, n_chrom, n, p.min_mapq, (const int *)t.carry_e, p.cls, t.keep, p.stats, cin);
    } else {
        hipLaunchKernelGGL(k_cv_tables<CARRY>, dim3(1), dim3(CV_BLOCK), 0, stream, p.pos, p.tab, n_chrom, cin);
        hipLaunchKernelGGL((k_cv_flags<false, CARRY>), dim3(n_tiles), dim3(CV_BLOCK), 0, stream, p.pos, p.mapq,
                           (const uint16_t *)nullptr, (const int32_t *)nullptr, tab, n_chrom, n, p.min_mapq,
                           (const int *)nullptr, (uint8_t *)nullptr, t.keep, p.stats, cin);
    }
    hipLaunchKernelGGL(k_cv_scan<0>, dim3(1), dim3(CV_SCAN_BLOCK), 0, stream, (const int *)t.keep, n_tiles, t.off,
                       p.kept_total);
    if (p.paired)
        hipLaunchKernelGGL((k_cv_compact<true, CARRY>), dim3(n_tiles), dim3(CV_BLOCK), 0, stream, p.pos, p.mapq,
                           (const uint8_t *)p.cls, p.tab, n_chrom, n, p.min_mapq, (const int *)t.off, p.kpos, cin);
    else
        hipLaunchKernelGGL((k_cv_compact<false, CARRY>), dim3(n_tiles), dim3(CV_BLOCK), 0, stream, p.pos, p.mapq,
                           (const uint8_t *)nullptr, p.tab, n_chrom, n, p.min_mapq, (const int *)t.off, p.kpos, cin);
    hipLaunchKernelGGL(k_cv_heads<CARRY>, dim3(n_ktiles), dim3(CV_BLOCK), 0, stream, (const int32_t *)p.kpos, tab, n_chrom,
                       p.min_shift, t.last, t.first, cin);
    hipLaunchKernelGGL(k_cv_scan<1>, dim3(1), dim3(CV_SCAN_BLOCK), 0, stream, (const int *)t.last, n_ktiles, t.carry_last,
                       (int *)nullptr);
    hipLaunchKernelGGL(k_cv_scan<2>, dim3(1), dim3(CV_SCAN_BLOCK), 0, stream, (const int *)t.first, n_ktiles, t.carry_next,
                       (int *)nullptr);
    hipLaunchKernelGGL(k_cv_count<CARRY>, dim3(n_ktiles), dim3(CV_BLOCK), 0, stream, (const int32_t *)p.kpos, tab, n_chrom,
                       p.min_shift, p.threshold, p.binsize, (const int *)t.carry_last, (const int *)t.carry_next, p.counts,
                       p.stats, cin, p.closing);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

// one slice through the kernels.  Its offsets table is so_host (HOST int64 [n_chrom + 1]) or, where that is NULL, so_dev
// (DEVICE int [n_chrom + 1]) with n64 a bound of its last entry: the grids are sized by n64, the kernels take the
// number of reads from the table.  closing: the empty slice of wc_convert_finish, which counts the open run
int cv_feed(wc_convert_run *run, hipStream_t stream, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
            const int32_t *mate_pos, const int64_t *so_host, const int *so_dev, int64_t n64, bool closing) {
    const int n_chrom = run->n_chrom;
    const int64_t keep_after = run->threshold > 0 ? std::min<int64_t>(run->threshold, run->pend_bound + n64) : 0;
    WC_CHECK(n64 + keep_after <= (int64_t)INT_MAX - 2 * CV_TILE, WC_E_LIMIT,
             "convert: %lld reads in one slice behind %lld pending ones (limit %d)", (long long)n64, (long long)keep_after,
             INT_MAX - 2 * CV_TILE);
    const int n = (int)n64;
    const int n_tiles = (n + 1 + CV_TILE - 1) / CV_TILE;                              // read n is the end marker
    const int n_ktiles = (int)((n64 + run->pend_bound + 1 + CV_TILE - 1) / CV_TILE);  // kept reads behind the pending ones
    int rc;
    if ((rc = run->tiles.reserve(sizeof(int) * 8 * (size_t)n_ktiles))) return rc;
    if (run->paired && (rc = run->cls.reserve((size_t)n_tiles * CV_TILE))) return rc;
    const size_t kbytes = sizeof(int32_t) * (size_t)(n64 + keep_after + 1);
    if ((rc = cv_grow_keep(run->kpos[run->at], kbytes, sizeof(int32_t) * (size_t)run->pend_bound, stream))) return rc;
    if ((rc = run->kpos[run->at ^ 1].reserve(kbytes))) return rc;
    CvTab *tab = run->tab.as<CvTab>();
    CvCarry *carry = run->carry.as<CvCarry>();
    int32_t *kpos = run->kpos[run->at].as<int32_t>(), *kpos_next = run->kpos[run->at ^ 1].as<int32_t>();
    unsigned long long *stats = run->out.as<unsigned long long>();
    if (so_host) {                                      // ro; bo is there since wc_convert_begin
        CvRo table;
        for (int c = 0; c <= WC_CV_MAX_CHROM; ++c) table.ro[c] = c <= n_chrom ? (int)so_host[c] : 0;
        hipLaunchKernelGGL(k_cv_slice, dim3(1), dim3(CV_BLOCK), 0, stream, tab, table, n_chrom);
    } else {
        WC_HIP(hipMemcpyAsync(tab->ro, so_dev, sizeof(int) * ((size_t)n_chrom + 1), hipMemcpyDeviceToDevice, stream));
    }
    const CvPass pass = {stream, pos, mapq, flag, mate_pos, tab, n_chrom, n, n_tiles, n_ktiles,
                         cv_tiles(run->tiles.as<int>(), n_ktiles), run->cls.as<uint8_t>(), kpos,
                         reinterpret_cast<int32_t *>(stats + 8), run->min_mapq, run->min_shift, run->threshold, run->binsize,
                         run->paired, stats, &carry->m_slice, carry, closing ? 1 : 0};
    if ((rc = cv_launch<true>(pass))) return rc;
    if (run->paired)
        hipLaunchKernelGGL(k_cv_carry<true>, dim3(1), dim3(CV_BLOCK), 0, stream, pos, mate_pos, (const CvTab *)tab, n_chrom,
                           run->threshold, (const int *)pass.tiles.last, n_ktiles, (const int *)pass.tiles.elast, n_tiles,
                           (const int32_t *)kpos, kpos_next, carry, stats);
    else
        hipLaunchKernelGGL(k_cv_carry<false>, dim3(1), dim3(CV_BLOCK), 0, stream, pos, (const int32_t *)nullptr,
                           (const CvTab *)tab, n_chrom, run->threshold, (const int *)pass.tiles.last, n_ktiles,
                           (const int *)nullptr, n_tiles, (const int32_t *)kpos, kpos_next, carry, stats);
    WC_HIP(hipGetLastError());
    run->at ^= 1;
    run->pend_bound = keep_after;
    ++run->slices;
    return WC_OK;
}

// the slice's table: ascending, starting at 0, and no reads for a chromosome in front of one that has had some
int cv_check_slice(wc_convert_run *run, const int64_t *so) {
    WC_CHECK(run && so, WC_E_ARG, "convert: NULL argument");
    WC_CHECK(!run->finished, WC_E_ARG, "convert: the run is finished");
    WC_CHECK(so[0] == 0, WC_E_ARG, "convert: the offset tables must start at 0");
    int last = run->host_cur;
    for (int c = 0; c < run->n_chrom; ++c) {
        WC_CHECK(so[c + 1] >= so[c], WC_E_ARG, "convert: offsets of chromosome %d decrease", c);
        if (so[c + 1] > so[c]) {
            WC_CHECK(c >= run->host_cur, WC_E_ARG, "convert: a slice brings reads for chromosome %d behind reads of chromosome %d",
                     c, run->host_cur);
            last = c;
        }
    }
    run->host_cur = last;
    return WC_OK;
}

// The arguments of wc_convert_reads_ex_dev, of wc_convert_begin (read_offsets NULL: it takes no reads) and, with `host`,
// what wc_convert_reads_ex must know before it stages the arrays (have_reads: pos and mapq; have_pair: flag and mate_pos)
// and hands everything to the device form.  It sizes the staging by the tables' last entries: one below 0 is WC_E_LIMIT
// there, with a text of its own, and WC_E_ARG (the table decreases) from the two others; tests/test_convert_refusals_gpu.py
int cv_check_args(int n_chrom, double binsize, const int64_t *read_offsets, const int64_t *bin_offsets, bool host,
                  bool have_reads, bool paired, bool have_pair) {
    WC_CHECK(n_chrom >= 1 && n_chrom <= WC_CV_MAX_CHROM, WC_E_LIMIT, "convert: %d chromosomes (1..%d supported)", n_chrom,
             WC_CV_MAX_CHROM);
    const int64_t n = read_offsets ? read_offsets[n_chrom] : 0, bins = bin_offsets[n_chrom];
    if (host) {
        WC_CHECK(n >= 0 && bins >= 0 && n <= (int64_t)INT_MAX && bins <= (int64_t)INT_MAX, WC_E_LIMIT,
                 "convert: %lld reads, %lld bins in one call", (long long)n, (long long)bins);
    } else {
        WC_CHECK(binsize > 0.0 && binsize <= DBL_MAX, WC_E_ARG, "convert: bin size %g is not a positive finite number", binsize);
        WC_CHECK((!read_offsets || read_offsets[0] == 0) && bin_offsets[0] == 0, WC_E_ARG,
                 "convert: the offset tables must start at 0");
        for (int c = 0; c < n_chrom; ++c)
            WC_CHECK((!read_offsets || read_offsets[c + 1] >= read_offsets[c]) && bin_offsets[c + 1] >= bin_offsets[c],
                     WC_E_ARG, "convert: offsets of chromosome %d decrease", c);
        WC_CHECK(n <= (int64_t)INT_MAX - 2 * CV_TILE, WC_E_LIMIT, "convert: %lld reads in one call (limit %d)", (long long)n,
                 INT_MAX - 2 * CV_TILE);
        WC_CHECK(bins <= (int64_t)INT_MAX, WC_E_LIMIT, "convert: %lld bins in one call", (long long)bins);
    }
    WC_CHECK(!read_offsets || n == 0 || have_reads, WC_E_ARG, "convert: NULL read arrays");
    WC_CHECK(!read_offsets || !paired || have_pair, WC_E_ARG,
             "convert: the paired mode needs the flag and mate position arrays");
    return WC_OK;
}

// n reads from the four HOST arrays to device memory that the caller has reserved (flag_dev, mate_dev: NULL unless paired)
int cv_stage(int64_t n, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag, const int32_t *mate_pos,
             int32_t *pos_dev, uint8_t *mapq_dev, uint16_t *flag_dev, int32_t *mate_dev) {
    if (!n) return WC_OK;
    WC_HIP(hipMemcpy(pos_dev, pos, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    WC_HIP(hipMemcpy(mapq_dev, mapq, (size_t)n, hipMemcpyHostToDevice));
    if (mate_dev) {
        WC_HIP(hipMemcpy(mate_dev, mate_pos, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        WC_HIP(hipMemcpy(flag_dev, flag, sizeof(uint16_t) * (size_t)n, hipMemcpyHostToDevice));
    }
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_convert_tile_reads(void) { return CV_TILE; }

int wc_convert_reads_ex_dev(wc_ctx *ctx, void *stream_, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                            const int32_t *mate_pos, const int64_t *read_offsets, int n_chrom, double binsize, int min_shift,
                            int threshold, int min_mapq, int demand_pair, const int64_t *bin_offsets, int32_t *counts_out,
                            int64_t *stats_out) {
    WC_CHECK(ctx && read_offsets && bin_offsets && counts_out && stats_out, WC_E_ARG, "convert: NULL argument");
    const bool paired = demand_pair != 0;
    int rc;
    if ((rc = cv_check_args(n_chrom, binsize, read_offsets, bin_offsets, false, pos && mapq, paired, flag && mate_pos))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    ConvertState &cv = ctx->cv;
    const int n = (int)read_offsets[n_chrom];
    const int n_tiles = (n + 1 + CV_TILE - 1) / CV_TILE;         // read n is the end marker that closes the koff table
    if ((rc = cv.tab.reserve(sizeof(CvTab)))) return rc;
    if ((rc = cv.tiles.reserve(sizeof(int) * 8 * (size_t)n_tiles))) return rc;
    if ((rc = cv.kpos.reserve(sizeof(int32_t) * ((size_t)n + 1)))) return rc;
    if (paired && (rc = cv.cls.reserve((size_t)n_tiles * CV_TILE))) return rc;      // whole tiles: no bound in the kernels
    CvTab *tab = cv.tab.as<CvTab>();
    std::vector<int> host(2 * (WC_CV_MAX_CHROM + 1), 0);
    for (int c = 0; c <= n_chrom; ++c) {
        host[c] = (int)read_offsets[c];
        host[WC_CV_MAX_CHROM + 1 + c] = (int)bin_offsets[c];
    }
    WC_HIP(hipMemcpyAsync(tab, host.data(), sizeof(int) * host.size(), hipMemcpyHostToDevice, stream));   // ro, bo
    WC_HIP(hipMemsetAsync(stats_out, 0, sizeof(int64_t) * 8, stream));
    if (bin_offsets[n_chrom]) WC_HIP(hipMemsetAsync(counts_out, 0, sizeof(int32_t) * (size_t)bin_offsets[n_chrom], stream));
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(stats_out);
    // the whole input in one call: the instances without a carry; [5]: kept reads (low word; the high word is zero)
    const CvPass pass = {stream, pos, mapq, flag, mate_pos, tab, n_chrom, n, n_tiles, n_tiles,
                         cv_tiles(cv.tiles.as<int>(), n_tiles), cv.cls.as<uint8_t>(), cv.kpos.as<int32_t>(), counts_out, min_mapq,
                         min_shift, threshold, binsize, paired, stats, reinterpret_cast<int *>(stats + 5), nullptr, 0};
    return cv_launch<false>(pass);
}

int wc_convert_reads_dev(wc_ctx *ctx, void *stream, const int32_t *pos, const uint8_t *mapq, const int64_t *read_offsets,
                         int n_chrom, double binsize, int min_shift, int threshold, const int64_t *bin_offsets,
                         int32_t *counts_out, int64_t *stats_out) {
    return wc_convert_reads_ex_dev(ctx, stream, pos, mapq, nullptr, nullptr, read_offsets, n_chrom, binsize, min_shift,
                                   threshold, 1, 0, bin_offsets, counts_out, stats_out);
}

int wc_convert_reads_ex(wc_ctx *ctx, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag, const int32_t *mate_pos,
                        const int64_t *read_offsets, int n_chrom, double binsize, int min_shift, int threshold, int min_mapq,
                        int demand_pair, const int64_t *bin_offsets, int32_t *counts_out, int64_t *stats_out) {
    WC_CHECK(ctx && read_offsets && bin_offsets && counts_out && stats_out, WC_E_ARG, "convert: NULL argument");
    const bool paired = demand_pair != 0;
    int rc;
    if ((rc = cv_check_args(n_chrom, binsize, read_offsets, bin_offsets, true, pos && mapq, paired, flag && mate_pos))) return rc;
    const int64_t n = read_offsets[n_chrom], bins = bin_offsets[n_chrom];
    WC_HIP(hipSetDevice(ctx->device));
    if ((rc = ctx->tmp_a.reserve(sizeof(int32_t) * (size_t)(n + 1)))) return rc;
    if ((rc = ctx->tmp_b.reserve((size_t)n + 1))) return rc;
    if ((rc = ctx->tmp_c.reserve(sizeof(int32_t) * (size_t)(bins + 1) + 64))) return rc;
    if (paired && (rc = ctx->tmp_d.reserve((sizeof(int32_t) + sizeof(uint16_t)) * (size_t)(n + 1)))) return rc;
    int64_t *stats_dev = ctx->tmp_c.as<int64_t>();               // 8 words, then the counts
    int32_t *mate_dev = paired ? ctx->tmp_d.as<int32_t>() : nullptr;      // n + 1 mate positions, then the flags
    uint16_t *flag_dev = paired ? reinterpret_cast<uint16_t *>(mate_dev + n + 1) : nullptr;
    rc = cv_stage(n, pos, mapq, flag, mate_pos, ctx->tmp_a.as<int32_t>(), ctx->tmp_b.as<uint8_t>(), flag_dev, mate_dev);
    if (rc) return rc;
    rc = wc_convert_reads_ex_dev(ctx, nullptr, ctx->tmp_a.as<int32_t>(), ctx->tmp_b.as<uint8_t>(), flag_dev, mate_dev,
                                 read_offsets, n_chrom, binsize, min_shift, threshold, min_mapq, demand_pair, bin_offsets,
                                 reinterpret_cast<int32_t *>(stats_dev + 8), stats_dev);
    if (rc) return rc;
    WC_HIP(hipDeviceSynchronize());
    return wc::convert_result(nullptr, stats_dev, bins, counts_out, stats_out, true);
}

int wc_convert_reads(wc_ctx *ctx, const int32_t *pos, const uint8_t *mapq, const int64_t *read_offsets, int n_chrom,
                     double binsize, int min_shift, int threshold, const int64_t *bin_offsets, int32_t *counts_out,
                     int64_t *stats_out) {
    return wc_convert_reads_ex(ctx, pos, mapq, nullptr, nullptr, read_offsets, n_chrom, binsize, min_shift, threshold, 1, 0,
                               bin_offsets, counts_out, stats_out);
}

int wc_convert_begin(wc_ctx *ctx, int n_chrom, double binsize, int min_shift, int threshold, int min_mapq, int demand_pair,
                     const int64_t *bin_offsets, wc_convert_run **out) {
    WC_CHECK(ctx && bin_offsets && out, WC_E_ARG, "convert: NULL argument");
    *out = nullptr;
    int rc;
    if ((rc = cv_check_args(n_chrom, binsize, nullptr, bin_offsets, false, false, false, false))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    wc_convert_run *run = new wc_convert_run;
    run->ctx = ctx;
    run->n_chrom = n_chrom;
    run->binsize = binsize;
    run->min_shift = min_shift;
    run->threshold = threshold;
    run->min_mapq = min_mapq;
    run->paired = demand_pair != 0;
    run->bins = bin_offsets[n_chrom];
    const size_t out_bytes = sizeof(int64_t) * 8 + sizeof(int32_t) * (size_t)run->bins;
    const CvCarry start = {/* cur, cur_n */ -1, 0, /* last_pos, larp, pe, me */ -1, -1, -1, -1, /* run_chrom */ -1,
                           /* last_kept, n_pend, m_slice, max_pend */ 0, 0, 0, 0};
    std::vector<int> bo(WC_CV_MAX_CHROM + 1, 0);
    for (int c = 0; c <= n_chrom; ++c) bo[(size_t)c] = (int)bin_offsets[c];
    rc = run->out.reserve(out_bytes);
    if (!rc) rc = run->carry.reserve(sizeof(CvCarry));
    if (!rc) rc = run->tab.reserve(sizeof(CvTab));
    if (!rc && (hipMemset(run->out.p, 0, out_bytes) != hipSuccess ||
                hipMemcpy(run->tab.as<CvTab>()->bo, bo.data(), sizeof(int) * bo.size(), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(run->carry.p, &start, sizeof(start), hipMemcpyHostToDevice) != hipSuccess ||
                hipDeviceSynchronize() != hipSuccess)) {
        wc::set_error("convert: could not set up the run's device state");
        rc = WC_E_HIP;
    }
    if (rc) {
        delete run;
        return rc;
    }
    *out = run;
    return WC_OK;
}

int wc_convert_feed_dev(wc_convert_run *run, void *stream, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                        const int32_t *mate_pos, const int64_t *slice_offsets) {
    WC_CHECK(run && slice_offsets, WC_E_ARG, "convert: NULL argument");
    const int64_t n = slice_offsets[run->n_chrom];
    WC_CHECK(n == 0 || (pos && mapq), WC_E_ARG, "convert: NULL read arrays");
    WC_CHECK(n == 0 || !run->paired || (flag && mate_pos), WC_E_ARG,
             "convert: the paired mode needs the flag and mate position arrays");
    int rc;
    if ((rc = cv_check_slice(run, slice_offsets))) return rc;
    if (n == 0) return WC_OK;                           // nothing to carry on
    WC_HIP(hipSetDevice(run->ctx->device));
    return cv_feed(run, (hipStream_t)stream, pos, mapq, flag, mate_pos, slice_offsets, nullptr, n, false);
}

int wc_convert_feed(wc_convert_run *run, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                    const int32_t *mate_pos, const int64_t *slice_offsets) {
    WC_CHECK(run && slice_offsets, WC_E_ARG, "convert: NULL argument");
    const int64_t n = slice_offsets[run->n_chrom];
    WC_CHECK(n >= 0 && n <= (int64_t)INT_MAX, WC_E_LIMIT, "convert: %lld reads in one slice", (long long)n);
    WC_CHECK(n == 0 || (pos && mapq), WC_E_ARG, "convert: NULL read arrays");
    WC_CHECK(n == 0 || !run->paired || (flag && mate_pos), WC_E_ARG,
             "convert: the paired mode needs the flag and mate position arrays");
    WC_HIP(hipSetDevice(run->ctx->device));
    int rc;
    if ((rc = run->st_pos.reserve(sizeof(int32_t) * (size_t)(n + 1)))) return rc;
    if ((rc = run->st_mapq.reserve((size_t)n + 1))) return rc;
    if (run->paired && (rc = run->st_mate.reserve(sizeof(int32_t) * (size_t)(n + 1)))) return rc;
    if (run->paired && (rc = run->st_flag.reserve(sizeof(uint16_t) * (size_t)(n + 1)))) return rc;
    uint16_t *flag_dev = run->paired ? run->st_flag.as<uint16_t>() : nullptr;
    int32_t *mate_dev = run->paired ? run->st_mate.as<int32_t>() : nullptr;
    rc = cv_stage(n, pos, mapq, flag, mate_pos, run->st_pos.as<int32_t>(), run->st_mapq.as<uint8_t>(), flag_dev, mate_dev);
    if (rc) return rc;
    rc = wc_convert_feed_dev(run, nullptr, run->st_pos.as<int32_t>(), run->st_mapq.as<uint8_t>(), flag_dev, mate_dev,
                             slice_offsets);
    if (rc) return rc;
    return wc::convert_result(nullptr, run->out.as<int64_t>(), 0, nullptr, nullptr, false);      // waits for the slice
}

static int cv_close(wc_convert_run *run, hipStream_t stream) {
    WC_CHECK(run, WC_E_ARG, "convert: NULL argument");
    WC_CHECK(!run->finished, WC_E_ARG, "convert: the run is finished");
    WC_HIP(hipSetDevice(run->ctx->device));
    std::vector<int64_t> nothing((size_t)run->n_chrom + 1, 0);
    const int rc = cv_feed(run, stream, nullptr, nullptr, nullptr, nullptr, nothing.data(), nullptr, 0, true);
    if (rc) return rc;
    run->finished = true;
    return WC_OK;
}

int wc_convert_finish_dev(wc_convert_run *run, void *stream_, int32_t *counts_out, int64_t *stats_out) {
    WC_CHECK(run && counts_out && stats_out, WC_E_ARG, "convert: NULL argument");
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if ((rc = cv_close(run, stream))) return rc;
    const int64_t *stats = run->out.as<int64_t>();
    WC_HIP(hipMemcpyAsync(stats_out, stats, sizeof(int64_t) * 8, hipMemcpyDeviceToDevice, stream));
    if (run->bins)
        WC_HIP(hipMemcpyAsync(counts_out, stats + 8, sizeof(int32_t) * (size_t)run->bins, hipMemcpyDeviceToDevice, stream));
    return WC_OK;
}

int wc_convert_finish(wc_convert_run *run, int32_t *counts_out, int64_t *stats_out) {
    WC_CHECK(run && counts_out && stats_out, WC_E_ARG, "convert: NULL argument");
    int rc;
    if ((rc = cv_close(run, nullptr))) return rc;
    return wc::convert_result(nullptr, run->out.as<int64_t>(), run->bins, counts_out, stats_out, false);
}

int wc_convert_run_info(const wc_convert_run *run, int64_t out[8]) {
    WC_CHECK(run && out, WC_E_ARG, "convert: NULL argument");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = run->slices;
    out[1] = run->device_bytes();
    out[2] = run->pend_bound;
    return WC_OK;
}

void wc_convert_end(wc_convert_run *run) {
    if (!run) return;
    (void)hipDeviceSynchronize();                       // the last slice's kernels still use the buffers
    delete run;
}

}  // extern "C"

namespace wc {

int convert_feed_table_dev(wc_convert_run *run, hipStream_t stream, const int32_t *pos, const uint8_t *mapq,
                           const uint16_t *flag, const int32_t *mate_pos, const int *slice_offsets_dev, int64_t most) {
    WC_CHECK(run && slice_offsets_dev && most >= 0, WC_E_ARG, "convert: NULL argument");
    WC_CHECK(!run->finished, WC_E_ARG, "convert: the run is finished");
    if (most == 0) return WC_OK;
    return cv_feed(run, stream, pos, mapq, flag, mate_pos, nullptr, slice_offsets_dev, most, false);
}

int convert_run_max_pending(const wc_convert_run *run, hipStream_t stream, int64_t *out) {
    int v = 0;
    WC_HIP(hipMemcpyAsync(&v, &run->carry.as<CvCarry>()->max_pend, sizeof(v), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    *out = v;
    return WC_OK;
}

int convert_result(hipStream_t stream, const int64_t *image_dev, int64_t bins, int32_t *counts_out, int64_t *stats_out,
                   bool counts_when_refused) {
    int64_t word = 0;
    if (stats_out) WC_HIP(hipMemcpyAsync(stats_out, image_dev, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, stream));
    else WC_HIP(hipMemcpyAsync(&word, image_dev + 4, sizeof(word), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    const int64_t outside = stats_out ? stats_out[4] : word;
    if (counts_out && bins && (outside == 0 || counts_when_refused)) {
        WC_HIP(hipMemcpyAsync(counts_out, image_dev + 8, sizeof(int32_t) * (size_t)bins, hipMemcpyDeviceToHost, stream));
        WC_HIP(hipStreamSynchronize(stream));
    }
    WC_CHECK(outside == 0, WC_E_ARG,
             "convert: %lld read(s) lie beyond their chromosome's last bin (a position past the header's length)",
             (long long)outside);
    return WC_OK;
}

}  // namespace wc
