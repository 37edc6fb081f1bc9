// newref: reference-bin selection on gfx950.
//
// Replaces getReference/getRefForBins (wisetools.py:298-325, 364-398): for every
// target bin, squared-L2 distance across the sample axis to every bin on another
// chromosome, keep the k nearest in stable (distance, position) order.
//
// Pipeline:
//   prepare     robust per-sample centre; float64 -> ONE float16 operand image (values scaled by a
//               power of two) for the threshold estimate and the distance tiles, a padded float64
//               image for the re-score; per-row norm bounds that carry the row's representation error
//   thresholds  f16-MFMA Gram tiles of all rows x M pseudo-random sample rows -> 16-bit key codes ->
//               per-row admission threshold from an order statistic
//   collect     symmetric f16-MFMA Gram tiles over the cross-chromosome triangle, operand slabs by
//               LDS-DMA; the epilogue turns dot products into LOWER BOUNDS of the true distance and
//               appends the few that pass the row threshold
//   re-score    k_pick: per row (one wave) a separator for the k-th lower bound, the upper bound U,
//               the certificate, the candidates with bound <= U as pairs; k_rescore: their exact
//               float64 distances in numpy's summation order, counting order, output.  Rows whose
//               certificate fails (and every row beyond refsize 256) take the exact path on the GPU
//               (k_exact_tile + k_exact_select).  More than 2048 samples: k_finish, one workgroup per row.
#include <cstring>
#include "ctx.h"

#include <algorithm>
#include <stdlib.h>

namespace {

constexpr int TB = 128;        // tile edge (rows and cols)
constexpr int BK = 32;         // k-slab depth
constexpr int LDA = 36;        // LDS row stride of a staged slab, floats (144 B keeps b128 reads conflict free)
constexpr int LDT = 68;        // the 64 x 128 dot tile of the threshold epilogue is column-major: stride of a column, floats
constexpr int ROLE_ROWS = 1;   // targets are the tile's rows (P side)
constexpr int ROLE_COLS = 2;   // targets are the tile's columns (Q side)
constexpr int MAX_SAMPLE_COLS = 4096;
constexpr int LIST_CAP = 1024;
constexpr int K_MAX = 1024;       // largest refsize (the exact path's selection buffers); above LIST_CAP / 4 every row takes the exact path
constexpr int GL_ROW = 16;            // LDS-DMA tile kernels: floats per LDS row (64 bytes = 32 float16)
constexpr int GL_STAGE = 2 * TB * GL_ROW;   // floats per stage: A rows then B rows
#define WC_ADMIT_ALL FLT_MAX
constexpr double SENTINEL_DISTANCE = 1e10;  // wisetools.py:306

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2_u __attribute__((ext_vector_type(2), aligned(8)));   // rows of an odd sample count start 8-byte aligned
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void_t;          // operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(1))) const void glb_void_t;
typedef __attribute__((address_space(3))) char lds_char_t;          // LDS addresses kept as such (32 bits, one register)
typedef __attribute__((address_space(3))) f64x2 lds_f64x2_t;

// ------------------------------------------------------------------ prepare ----
// Robust per-sample centre from a strided subset of rows: mean -> 8 x mean absolute
// deviation window -> trimmed mean (all over finite values).  Any centre is valid
// (distances are translation invariant per sample); a good one keeps the float32
// norms, and with them the error interval of the MFMA distances, small even when
// a few bins are wild outliers.  One block owns 64 samples end to end.
__global__ __launch_bounds__(1024) void k_col_centre(const double *__restrict__ X, int64_t B, int64_t S,
                                                     int64_t n_rows, int64_t row_step,
                                                     double *__restrict__ centre, int *__restrict__ bad_norm) {
    __shared__ double sh_s[16][64];
    __shared__ double sh_c[16][64];
    __shared__ double sh_v[64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * 64 + tx;
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad_norm = 0x7F800000;   // +inf: no row with a clamped value yet (k_convert)
    // the (at most 128) sampled rows of this sample are read ONCE into registers: the three
    // passes were three dependent memory round trips before (10 us for a kernel that moves 100 KB)
    constexpr int PER = 8;                      // n_rows <= 128 = 16 row phases x 8
    double val[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int64_t q = ty + 16 * e;
        val[e] = (s < S && q < n_rows) ? X[(q * row_step) * S + s] : NAN;
    }
    double c = 0.0, rad = 0.0;
    for (int pass = 0; pass < 3; ++pass) {
        double sum = 0.0, cnt = 0.0;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const double v = val[e];
            const bool ok = isfinite(v) && (pass != 2 || fabs(v - c) <= rad);
            sum += ok ? ((pass == 1) ? fabs(v - c) : v) : 0.0;
            cnt += ok ? 1.0 : 0.0;
        }
        sh_s[ty][tx] = sum;
        sh_c[ty][tx] = cnt;
        wc_sync();
        if (ty == 0) {
            double a = 0.0, b = 0.0;
            for (int r = 0; r < 16; ++r) { a += sh_s[r][tx]; b += sh_c[r][tx]; }
            sh_v[tx] = b > 0.0 ? a / b : 0.0;
        }
        wc_sync();
        if (pass == 0) c = sh_v[tx];
        else if (pass == 1) {
            rad = 8.0 * sh_v[tx];
            if (ty == 0 && s < S) centre[S + s] = sh_v[tx];   // mean absolute deviation: the f16 image's scale comes from it
        } else if (ty == 0 && s < S) centre[s] = sh_v[tx];
        wc_sync();
    }
}

// Layout of the float16 image A16 (bins_pad rows x Kpad16 samples): the 128 rows of a tile panel and the 32
// samples of a k-slab form one contiguous 8 KB block (row-major inside, 64 bytes per row), blocks ordered by
// (panel, slab).  A tile's operand slab is then ONE contiguous stretch: every 128-byte line the LDS-DMA touches is
// used whole (rows of Kpad16 halfs put a slab on half a line of each of 128 rows: measured 16 % slower tile loop).
__device__ __host__ inline int64_t a16_index(int64_t row, int64_t s, int64_t Kpad16) {
    return (((row >> 7) * (Kpad16 >> 5) + (s >> 5)) << 12) + ((row & 127) << 5) + (s & 31);
}

// float32 -> float16 bits for the one-product tiles: value * gam (a power of two) clamped to the
// finite float16 range, rounded to nearest even, subnormal results flushed to zero (so that the
// image is exactly what any matrix-core denormal mode sees).  NaN stays NaN.
__device__ inline unsigned short f32_to_f16_scaled(float a, double gam, double inv_gam, double &back, bool &clamped) {
    double sd = (double)a * gam;
    clamped = clamped || sd > 65504.0 || sd < -65504.0;
    sd = sd > 65504.0 ? 65504.0 : (sd < -65504.0 ? -65504.0 : sd);
    _Float16 h = (_Float16)(float)sd;           // (float)sd is exact: a has 24 bits, gam is a power of two
    if (fabs((double)(float)h) < 6.103515625e-05) h = (_Float16)0.f;
    back = (double)(float)h * inv_gam;          // the value the tiles multiply, exactly
    unsigned short bits;
    __builtin_memcpy(&bits, &h, 2);
    return bits;
}

// A row's slack as a short code in the free high bits of a list entry's candidate word (row | code << index_bits,
// cb = 32 - index_bits code bits): the top cb of the float's 31 non-sign bits, rounded UP, so that the decoded
// slack is never below the true one -- a larger slack only raises k_pick's U (a few more re-scores, a marginally
// stricter certificate; every delivered index and distance is decided in float64).  A carry into the exponent is
// the next power of two, +inf stays +inf (its dropped bits are zero), a NaN counts as +inf.  With eight exponent
// bits and cb - 8 mantissa bits the decoded value is at most 1 + 2^-(cb - 8) times the slack.
__host__ __device__ inline unsigned int slack_encode(float slack, int cb) {
    unsigned int u;
    __builtin_memcpy(&u, &slack, 4);
    u = u > 0x7F800000u ? 0x7F800000u : u;        // (negative values do not occur: a slack is a rounded-up norm gap)
    const int sh = 31 - cb;
    return (u + ((1u << sh) - 1u)) >> sh;
}
__host__ __device__ inline float slack_decode(unsigned int code, int cb) {
    const unsigned int u = code << (31 - cb);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// the slack of a candidate word: its code sits one bit left of where the float's bits belong
__device__ __forceinline__ float slack_of_word(unsigned int word, unsigned int index_mask) {
    return __uint_as_float((word >> 1) & ~(index_mask >> 1));
}

// Half a wave per row: centred operand image, norm interval, chromosome id.
// ONE float16 image (A16; values scaled by the power of two gam) serves the threshold estimate and
// the distance tiles.  The row's representation error e = |a - h| and |h|^2 are accumulated in
// float64, and the lower bound loses w = e^2 / tau + tau max(|a|^2, |h|^2) on top of the float32
// accumulation chain: 2 |a_i.a_j - h_i.h_j| <= 2 (e_i |a_j| + |h_i| e_j) <= w_i + w_j for any tau > 0
// ("one product per multiply").
// norm_hi holds the row's SLACK: key <= true distance <= key + slack_i + slack_j.
// A row with a CLAMPED value (beyond +-65504 / gam: thousands of times the typical spread) has no usable
// image: as a listed candidate its huge slack would void the certificate of every row that lists it.  Such a
// row gets infinite bounds -- never listed, its own row takes the exact path -- and leaves the smallest
// norm among such rows in *bad_norm; k_pick certifies a row only if (|a_bad| - |a_i|)^2, a lower bound of
// its distance to any of them, stays above U.
// The row body of k_convert (NT = 256 threads, centre and scale from global memory: `mean`, the scale terms S doubles
// on) and of k_prepare_fused (LDS: `mean` points there, the scale terms 128 doubles on).
template <bool CENTRE_IN_LDS, int NT>
__device__ __forceinline__ void convert_row(const double *__restrict__ X, int64_t B, int64_t S, int64_t Bpad,
                                            const double *mean, double beta, double tau,
                                            const int64_t *__restrict__ chrom_off, int n_chrom,
                                            unsigned short *__restrict__ A16, int64_t Kpad16,
                                            float *__restrict__ norm_lo, float *__restrict__ norm_hi,
                                            int *__restrict__ chrom_of_row, int2 *__restrict__ chrom_range,
                                            const int *__restrict__ sample_slot, unsigned short *__restrict__ S16,
                                            float *__restrict__ s_norm_lo, int *__restrict__ s_chrom,
                                            int2 *__restrict__ s_range, float *__restrict__ thr, int *__restrict__ cnt,
                                            int *__restrict__ row_stat, double *__restrict__ X64, int64_t Sp,
                                            float *__restrict__ m2_out, int *__restrict__ bad_norm,
                                            int *__restrict__ fb_zero, int n_fb_zero,
                                            unsigned int *__restrict__ cand_word, int index_bits) {
    // Half a wave per row (lane hl of 32, `half` picks the row): a row's life here is a few dependent round trips,
    // and with a wave per row the 11 087 rows of a 250 kb problem were 1.35 rounds of what fits the chip -- two rounds
    // of ~5 us.  Two rows per wave make it one.
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const int64_t row = ((int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6)) * 2 + half;
    // the exact path's counter and tickets of the job that starts here (was a memset launch in front of
    // the pick stage of every pass)
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < n_fb_zero; i += NT) fb_zero[i] = 0;
    if (row >= Bpad) return;                   // (Bpad is a multiple of 128: whole waves)
    // The half wave reads its row ONCE, samples hl + 32 i in blocks of CB: every load of a block -- the row's values,
    // mean[s] and the scale terms mean[S + s] -- is an unconditional load of a selected index (element 0 always exists)
    // issued before the block's first use, so a block is one memory round trip.  (One load and one wait per iteration
    // of three loops, two of which read again what the first had read, were twelve dependent trips at 100 samples.)
    constexpr int CB = 4;
    const int64_t scale_off = CENTRE_IN_LDS ? 128 : S;
    const int64_t xrow = (row < B ? row : 0) * S;
    auto load_x = [&](int64_t s0, double (&xv)[CB], double (&mv)[CB]) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const int64_t s = s0 + 32 * j, sc = s < S ? s : 0;
            xv[j] = X[xrow + sc];
            mv[j] = mean[sc];
        }
    };
    // (the empty statements pin a batch behind its loads: a load whose only use is under a lane condition is
    // otherwise sunk into that block, with a wait of its own)
    auto pin = [&](double (&v)[CB]) {
#pragma unroll
        for (int j = 0; j < CB; ++j) asm volatile("" : "+v"(v[j]));
    };
    auto load_scale = [&](int64_t s0, double (&sv)[CB]) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const int64_t s = s0 + 32 * j;
            sv[j] = mean[scale_off + (s < S ? s : 0)];
        }
    };
    // the first block of the row and of the centre rides with the first block of the scale terms, the row's sample
    // slot and the chromosome ends: at up to 128 samples that is everything this half wave reads, in one trip
    // (up to WC_MAX_CHROM = 64 chromosomes: two ends per lane of the half)
    double xv[CB], mv[CB], sv[CB];
    load_scale(hl, sv);
    load_x(hl, xv, mv);
    int slot_w = sample_slot[row < B ? row : 0];
    int64_t end0_w = chrom_off[hl < n_chrom ? hl + 1 : 0], end1_w = chrom_off[hl + 32 < n_chrom ? hl + 33 : 0];
    asm volatile("" : "+v"(slot_w), "+v"(end0_w), "+v"(end1_w));
    pin(sv);
    pin(xv);
    pin(mv);
    const int slot = row < B ? slot_w : -1;    // >= 0: this row is one of the sampled rows
    // chromosome of the row: lane c of the half holds the end of chromosome c (at most 32 of them), the row's
    // chromosome is the number of ends at or below it (the serial search was up to 22 dependent loads on lane 0)
    int ch_w = -1;
    int2 range_w = make_int2(0, 0);
    {
        const int64_t none = (int64_t)0x7FFFFFFFFFFFFFFFll;
        const int64_t end0 = hl < n_chrom ? end0_w : none, end1 = hl + 32 < n_chrom ? end1_w : none;
        const unsigned long long b0 = __ballot(row < B && hl < n_chrom - 1 && row >= end0);
        const unsigned long long b1 = __ballot(row < B && hl + 32 < n_chrom - 1 && row >= end1);
        const int c = __popc((unsigned int)(b0 >> (32 * half))) + __popc((unsigned int)(b1 >> (32 * half)));
        auto end_of = [&](int i) {             // end of chromosome i, from whichever lane of this half holds it
            const int64_t a0 = __shfl(end0, (lane & 32) + (i & 31)), a1 = __shfl(end1, (lane & 32) + (i & 31));
            return i < 32 ? a0 : a1;
        };
        const int64_t e_lo = end_of(c ? c - 1 : 0), e_hi = end_of(c);
        if (row < B) {
            ch_w = c;
            range_w = make_int2((int)(c ? e_lo : 0), (int)e_hi);
        }
    }
    double gam = 1.0, inv_gam = 1.0;
    {
        // every half wave derives the same scale: typical |a| * gam lands in [4, 8) (float16 keeps
        // 2^13 above that and 2^16 below it in its normal range)
        double t = 0.0, c = 0.0;
        for (int64_t s0 = hl; s0 < S; s0 += 32 * CB) {
            if (s0 != hl) { load_scale(s0, sv); pin(sv); }
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                const double m = sv[j];
                if (s0 + 32 * j < S && isfinite(m) && m > 0.0) { t += m; c += 1.0; }
            }
        }
        for (int o = 16; o > 0; o >>= 1) { t += __shfl_xor(t, o); c += __shfl_xor(c, o); }
        if (c > 0.0 && isfinite(t)) {
            int e = ilogb(t / c);
            e = e < -60 ? -60 : (e > 60 ? 60 : e);
            gam = ldexp(1.0, 2 - e);
            inv_gam = ldexp(1.0, e - 2);
        }
        if (row == 0 && hl == 0) *m2_out = (float)(-2.0 * inv_gam * inv_gam);
    }
    double acc = 0.0, e2 = 0.0, hn = 0.0;
    bool clamped = false;
    // (Kpad16 is a multiple of 64 and the padded float64 row is no longer: a block of four may run past Kpad16, never
    // an iteration inside it that is used)
    for (int64_t s0 = hl; s0 < Kpad16; s0 += 32 * CB) {
        if (s0 != hl) { load_x(s0, xv, mv); pin(xv); pin(mv); }
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const int64_t s = s0 + 32 * j;
            if (s < Kpad16) {
                // float64 image with rows padded to whole 16-sample chunks (128-byte aligned rows, zero
                // padding): the re-score gathers read it with aligned 16-byte loads and no tail cases
                if (X64 && row < B && s < Sp) X64[row * Sp + s] = s < S ? xv[j] : 0.0;
                float a = 0.f;
                if (row < B && s < S) a = (float)(xv[j] - mv[j]);
                double back;
                const unsigned short h = f32_to_f16_scaled(a, gam, inv_gam, back, clamped);
                const double err = (double)a - back;
                e2 += err * err;
                hn += back * back;
                A16[a16_index(row, s, Kpad16)] = h;
                if (slot >= 0) S16[(int64_t)slot * Kpad16 + s] = h;
                acc += (double)a * (double)a;
            }
        }
    }
    for (int o = 16; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o);
        e2 += __shfl_xor(e2, o);
        hn += __shfl_xor(hn, o);
    }
    clamped = ((unsigned int)(__ballot(clamped) >> (32 * half))) != 0u;
    if (hl == 0) {
        float lo = INFINITY, hi = INFINITY;
        int ch = -1;
        int2 range = make_int2(0, 0);   // rows of this row's chromosome (padding rows: none)
        if (row < B) {
            if (isfinite(acc) && acc < 1e37 && isfinite(e2) && isfinite(hn) && clamped) {
                // positive floats order like their bit patterns
                atomicMin(bad_norm, __float_as_int(__double2float_rd(sqrt(acc) * (1.0 - 1e-6))));
            } else if (isfinite(acc) && acc < 1e37 && isfinite(e2) && isfinite(hn)) {
                // key = lo_i + lo_j - 2 dot must never exceed the true distance
                const double m = fmax(acc, hn);
                lo = __double2float_rd(acc - (e2 / tau + tau * m) * (1.0 + 1e-9) - beta * m - 1e-37);
                hi = __double2float_ru(2.0 * (acc - (double)lo) * (1.0 + 1e-6) + 1e-37);
            }
            ch = ch_w;
            range = range_w;
        }
        chrom_range[row] = range;
        norm_lo[row] = lo;
        norm_hi[row] = hi;
        // the row as a listed candidate: its number with its slack's code above it (k_gram_glds copies the word into
        // the entry, k_pick needs no gather of norm_hi)
        cand_word[row] = (unsigned int)row | (slack_encode(hi, 32 - index_bits) << index_bits);
        chrom_of_row[row] = ch;
        if (slot >= 0) {
            s_norm_lo[slot] = lo;
            s_chrom[slot] = ch;
            s_range[slot] = range;
        }
        // per-row state of a new job: nothing admitted, no candidates, not finished
        thr[row] = -INFINITY;
        cnt[row] = 0;
        row_stat[row] = (int)0xFEFEFEFE;
    }
}

#define WC_CONVERT_PARAMS                                                                                            \
    const double *__restrict__ X, int64_t B, int64_t S, int64_t Bpad, const double *__restrict__ mean, double beta, \
        double tau, const int64_t *__restrict__ chrom_off, int n_chrom, unsigned short *__restrict__ A16,           \
        int64_t Kpad16, float *__restrict__ norm_lo, float *__restrict__ norm_hi, int *__restrict__ chrom_of_row,   \
        int2 *__restrict__ chrom_range, const int *__restrict__ sample_slot, unsigned short *__restrict__ S16,      \
        float *__restrict__ s_norm_lo, int *__restrict__ s_chrom, int2 *__restrict__ s_range,                       \
        float *__restrict__ thr, int *__restrict__ cnt, int *__restrict__ row_stat, double *__restrict__ X64,       \
        int64_t Sp, float *__restrict__ m2_out, int *__restrict__ bad_norm, int *__restrict__ fb_zero,              \
        int n_fb_zero, unsigned int *__restrict__ cand_word, int index_bits
#define WC_CONVERT_ARGS(mean_)                                                                                        \
    X, B, S, Bpad, mean_, beta, tau, chrom_off, n_chrom, A16, Kpad16, norm_lo, norm_hi, chrom_of_row, chrom_range,   \
        sample_slot, S16, s_norm_lo, s_chrom, s_range, thr, cnt, row_stat, X64, Sp, m2_out, bad_norm, fb_zero,       \
        n_fb_zero, cand_word, index_bits

// centre and scale from `mean` (k_col_centre's 2 S numbers); more than 128 samples
__global__ __launch_bounds__(256) void k_convert(WC_CONVERT_PARAMS) {
    convert_row<false, 256>(WC_CONVERT_ARGS(mean));
}

// Up to 128 samples: prepare in ONE launch.  Every workgroup derives centre and scale itself, in LDS, from the same
// n_crows <= CR sampled rows (rows q * crow_step) with k_col_centre's three passes -- the same loads, the same sums in
// the same order, so the same bits in every workgroup (rows compared with each other must share a centre) -- and then
// converts its NT / 32 rows as k_convert does.  k_col_centre was a dependent launch of two workgroups for 2 S numbers
// that any later stage tolerates in any reasonable value; the CR rows are 25 KB at 100 samples, read from L2 by all but
// the first workgroups.  Thread = sample (threadIdx & 127) x row phase (threadIdx >> 7), CR / (NT / 128) rows each, ONE
// batch of unconditional loads of selected indices; the row's own loads follow the centre (requested with it they made
// the pass slower: EXPERIMENTS.md).  Workgroup 0 writes `mean_out` for the callers that read the centres back.
// *bad_norm must be +inf at entry (k_col_centre reset it itself, this kernel's rows take minima into it from the
// start); the kernel leaves *bad_spare, the slot of the prepare before this one, at +inf for the prepare after it.
constexpr int FUSED_CENTRE_ROWS = 32;
constexpr int FUSED_MAX_SAMPLES = 128;
constexpr int FUSED_THREADS = 512;      // 16 rows per workgroup: the centre phase is done 693 times at cfg2, not 1 386
constexpr int FUSED_WGS_PER_CU = 3;     // cfg2: 693 workgroups on 256 CUs are one round
template <int CR, int NT>
__global__ __launch_bounds__(NT, FUSED_WGS_PER_CU) void k_prepare_fused(WC_CONVERT_PARAMS, double *__restrict__ mean_out,
                                                                       int64_t n_crows, int64_t crow_step,
                                                                       int *__restrict__ bad_spare) {
    constexpr int NPH = NT / 128, PER = CR / NPH;   // row phases, sampled rows per thread
    static_assert(CR % NPH == 0, "whole rows per phase");
    __shared__ float sh_part[2][2][NPH][128];   // [pass parity][sum, count][row phase][sample]
    __shared__ double sh_cs[2 * 128];           // centre, then scale (mean absolute deviation), per sample
    // (the row phase is the same for a whole wave: as a scalar it leaves the sampled rows' addresses in scalar registers)
    const int tx = threadIdx.x & 127, ty = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad_spare = 0x7F800000;
    double val[PER];
    {
        const unsigned int sc = tx < S ? tx : 0;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int64_t q = ty + NPH * e;
            const double *__restrict__ xq = X + ((q < n_crows ? q : 0) * crow_step) * S;
            val[e] = xq[sc];
        }
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) asm volatile("" : "+v"(val[e]));
    // The three passes in float32: a centre needs no more (the values are centred in float64, whatever it is), and the
    // phase is repeated by every workgroup -- in float64 its arithmetic cost what the launch it replaces did.  A value
    // beyond the float32 range counts as not finite.
    float fv[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) fv[e] = (tx < S && ty + NPH * e < n_crows) ? (float)val[e] : NAN;
    float c = 0.f, rad = 0.f, mad = 0.f;
    for (int pass = 0; pass < 3; ++pass) {
        float sum = 0.f, n = 0.f;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const float v = fv[e];
            const bool ok = isfinite(v) && (pass != 2 || fabsf(v - c) <= rad);
            sum += ok ? ((pass == 1) ? fabsf(v - c) : v) : 0.f;
            n += ok ? 1.f : 0.f;
        }
        // (pass 2 writes the block of pass 0 again: every thread has read that one before the barrier of pass 1)
        float (*part)[NPH][128] = sh_part[pass & 1];
        part[0][ty][tx] = sum;
        part[1][ty][tx] = n;
        wc_sync();
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int r = 0; r < NPH; ++r) { a += part[0][r][tx]; b += part[1][r][tx]; }
        const float v = b > 0.f ? a / b : 0.f;
        if (pass == 1) { mad = v; rad = 8.f * v; }
        else c = v;
    }
    if (ty == 0) {
        sh_cs[tx] = (double)c;
        sh_cs[128 + tx] = (double)mad;
        if (blockIdx.x == 0 && tx < S) {
            mean_out[tx] = (double)c;
            mean_out[S + tx] = (double)mad;
        }
    }
    wc_sync();
    convert_row<true, NT>(WC_CONVERT_ARGS((const double *)sh_cs));
}
#undef WC_CONVERT_PARAMS
#undef WC_CONVERT_ARGS

// Sample slots beyond the real rows (problems with fewer bins than sample columns): zero
// rows that can never be candidates.
__global__ void k_pad_samples(int64_t Kpad16, int64_t first, unsigned short *__restrict__ S16,
                              float *__restrict__ s_norm_lo, int *__restrict__ s_chrom,
                              int2 *__restrict__ s_range) {
    int64_t m = first + blockIdx.x;
    for (int64_t s = threadIdx.x; s < Kpad16; s += blockDim.x) S16[m * Kpad16 + s] = (unsigned short)0;
    if (threadIdx.x == 0) {
        s_norm_lo[m] = INFINITY;
        s_chrom[m] = -2;
        s_range[m] = make_int2(0, 0);
    }
}


// --------------------------------------------------------------- Gram tiles ----
struct GramArgs {
    const float *P, *Q;          // blocked float16 image (a16_index) viewed as 32-bit words, rows padded to 128
    int64_t ld;                  // row stride in 32-bit words (padded sample count / 2)
    const float *m2;             // -2 / gam^2 (the operand image is scaled by gam)
    int nslab32, last_steps32;   // 32-sample slabs, 16-sample MFMA steps of the last one that hold samples (1..2)
    const float *nbP, *nbQ;      // lower norm bounds
    const unsigned int *cwP, *cwQ;   // candidate words: row | slack code << index_bits (k_convert)
    const int2 *range;           // per row: [first, last+1) row of its chromosome (never candidates)
    const int4 *tiles;           // {I, J, roles, 0}
    int ntiles;
    const float *thr;            // admission threshold per target row
    int *cnt;
    unsigned long long *list;
    int cap;
};

// 16-bit image of a non-negative float32 key for the threshold estimate: exponent and 8
// mantissa bits, truncated (the estimate adds the bucket width back); 0xFFFF = not a candidate
// (infinite / NaN lower bound).  Negative keys (near-identical rows) count as 0.
__device__ inline unsigned int key_code16(float key) {
    const unsigned int code = __float_as_uint(fmaxf(key, 0.f)) >> 15;
    return key < INFINITY ? code : 0xFFFFu;
}
__device__ inline float key_from_code16(unsigned int code) {   // upper edge of the bucket
    return __uint_as_float((code << 15) | 0x7FFFu);
}

// bits [a, b) of a 32-bit mask, a and b clipped to [0, 32]
__device__ inline unsigned int run_mask(int a, int b) {
    a = a < 0 ? 0 : a;
    b = b > 32 ? 32 : b;
    if (a >= b) return 0u;
    const unsigned int upto_b = b == 32 ? ~0u : ((1u << b) - 1u);
    return upto_b & ~((1u << a) - 1u);
}

// pack_entry for a key that has passed `key <= thr` (not a NaN: f32_ordered without its NaN case, same bits)
// (the low word is the candidate's word: its row number under its slack's code)
__device__ inline unsigned long long pack_passed(float key, unsigned int word) {
    const unsigned int b = __float_as_uint(key);
    return ((unsigned long long)((b & 0x80000000u) ? ~b : (b | 0x80000000u)) << 32) | word;
}

// mask = 2 mask + (key <= thr): the compare and an add-with-carry (the compiler makes three instructions of it)
__device__ __forceinline__ void shift_in_le(unsigned int &mask, float key, float thr) {
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(key), "v"(thr) : "vcc");
}

// orders one wave's LDS writes before its other lanes' reads of them (no workgroup barrier)
__device__ inline void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline unsigned long long pack_entry(float key, int j) {
    return ((unsigned long long)wc::f32_ordered(key) << 32) | (unsigned int)j;
}

// Distance tiles: 128 x 128 outputs per 256-thread workgroup, each wave a 64 x 64 block as 2 x 2
// v_mfma_f32_32x32x16_f16 accumulators.  The operand image is float16 (11 significant bits, values
// scaled by one power of two), a k-slab row is 32 samples = 64 bytes, and the representation error
// of every row is known exactly (k_convert) and charged to that row's norm bounds: ONE matrix-core
// product per multiply, rigorous lower bounds out.

// The tile's epilogue: dot products -> lower-bound keys -> the few that pass a target's threshold appended
// to that target's list.  Every wave finishes its own 64 x 64 block; the workgroup meets once, before the
// dot blocks overwrite the operand stages.
//
// 1. Sweep in the accumulator layout.  Element 4 r4 + e of acc[m][n] is row wr*64 + m*32 + 8 r4 + 4 lh + e,
//    column wc*64 + n*32 + li: a lane holds two columns x 32 of the wave's 64 rows.  Each key is evaluated once.
//    Against the column target's threshold it sets one bit of the lane's mask of that column (bit 16 m + 4 r4 + e:
//    ascending in the row).  Against the ROW targets' thresholds -- the lane's four rows of a register group,
//    one 16-byte read -- it is one v_cmp whose 64-bit result holds the 32-column masks of two rows (lh = 0, 1);
//    it goes to the wave's mask table as one 8-byte write, word lh landing in its row's slot.
// 2. Reservations, once per tile: the two lanes of a column add their counts (one cross-lane move each way),
//    lane L finishes row L of the wave's 64 (two mask words, the row's own chromosome cleared as a run).  Both
//    sets of atomics are issued back to back; their round trip is covered by the barrier and the staging.
// 3. Appends, per 32-row half m: the wave writes its 32 x 64 dot block column-major into its own quarter of the
//    operand stages (16-byte writes, the four-row chunks of a column XOR-swizzled by the column: an unpadded
//    column is 128 bytes), and the two data-dependent append loops rebuild the keys of the set bits from it.
constexpr int EP_LD = 32;                    // floats per column of a wave's dot block (32 rows, no padding)
constexpr int EP_BLOCK = 64 * EP_LD;         // floats per wave
constexpr int EP_MASKS = 128;                // 32-bit words of a wave's row-mask table: [n][m][r4][e][lh]
static_assert(4 * EP_BLOCK <= 2 * GL_STAGE, "the four dot blocks alias the two operand stages");

__device__ __forceinline__ int ep_at(int col, int row) {      // float offset of (row 0..31, column 0..63) in a dot block
    return col * EP_LD + ((((row >> 2) ^ col) & 7) << 2) + (row & 3);
}

__device__ __forceinline__ void gram_epilogue(const GramArgs &g, float *sm, const float *nbPs, const float *nbQs,
                                              const float *thPs, const float *thQs, const unsigned int *cwPs,
                                              const unsigned int *cwQs, f32x16 (&acc)[2][2], const int I,
                                              const int J, const int roles, const float m2, const int lane, const int w,
                                              const int wr, const int wc, const int li, const int lh) {
    __builtin_amdgcn_s_setprio(0);
    const int row0 = I * TB + wr * 64, col0 = J * TB + wc * 64;           // the wave's block
    const int2 rgq0 = g.range[(int64_t)col0 + li], rgq1 = g.range[(int64_t)col0 + 32 + li];
    const int2 rgr = g.range[(int64_t)row0 + lane];
    unsigned int *maskw = reinterpret_cast<unsigned int *>(sm + 2 * GL_STAGE) + w * EP_MASKS;
    unsigned long long *mask2 = reinterpret_cast<unsigned long long *>(maskw);
    const bool cols = (roles & ROLE_COLS) != 0, rows = (roles & ROLE_ROWS) != 0;
    const float nbc0 = nbQs[wc * 64 + li], nbc1 = nbQs[wc * 64 + 32 + li];
    const float thc0 = cols ? thQs[wc * 64 + li] : -INFINITY, thc1 = cols ? thQs[wc * 64 + 32 + li] : -INFINITY;
    unsigned int mc0 = 0u, mc1 = 0u;
    // (descending, so that the masks can take their bits by shifting them in: bit b is the key of step b)
#pragma unroll
    for (int m = 1; m >= 0; --m)
#pragma unroll
        for (int r4 = 3; r4 >= 0; --r4) {
            const f32x4 nb4 = *(const f32x4 *)&nbPs[wr * 64 + m * 32 + 8 * r4 + 4 * lh];
            const f32x4 th4 = *(const f32x4 *)&thPs[wr * 64 + m * 32 + 8 * r4 + 4 * lh];
#pragma unroll
            for (int e = 3; e >= 0; --e) {
                const float key0 = fmaf(m2, acc[m][0][4 * r4 + e], nb4[e] + nbc0);
                const float key1 = fmaf(m2, acc[m][1][4 * r4 + e], nb4[e] + nbc1);
                shift_in_le(mc0, key0, thc0);
                shift_in_le(mc1, key1, thc1);
                // every lane stores the (uniform) pair of masks: one LDS write, no exec games
                mask2[(m * 4 + r4) * 4 + e] = __ballot(key0 <= th4[e]);
                mask2[32 + (m * 4 + r4) * 4 + e] = __ballot(key1 <= th4[e]);
            }
        }
    // Column role: the own-chromosome rows leave as a run (the lane's 32 rows ascend with the bit number: of the
    // rows below t, 4 per whole group of eight and the group's first or second four are this lane's)
    auto below = [&](int t) {
        t = t < 0 ? 0 : (t > 64 ? 64 : t);
        const int part = (t & 7) - 4 * lh;
        return 4 * (t >> 3) + (part < 0 ? 0 : (part > 4 ? 4 : part));
    };
    mc0 &= ~run_mask(below(rgq0.x - row0), below(rgq0.y - row0));
    mc1 &= ~run_mask(below(rgq1.x - row0), below(rgq1.y - row0));
    const int mine_c = __popc(mc0) | (__popc(mc1) << 16);
    const int other_c = __shfl_xor(mine_c, 32);
    // lane lh = 0 reserves for column li, lane lh = 1 for column 32 + li; the lh = 0 lane's entries go first
    const int cnt_a = lh ? (other_c >> 16) : (mine_c & 0xFFFF), cnt_b = lh ? (mine_c >> 16) : (other_c & 0xFFFF);
    const int64_t gq0 = (int64_t)col0 + li;
    int res_c = 0;
    if (cnt_a + cnt_b > 0) res_c = atomicAdd(&g.cnt[gq0 + 32 * lh], cnt_a + cnt_b);
    // Row role: lane L owns row L of the wave's 64
    unsigned int mr0 = 0u, mr1 = 0u;
    int res_r = 0;
    const int64_t gp = (int64_t)row0 + lane;
    if (rows) {
        wave_lds_fence();
        const int at = (((lane >> 3) * 4 + (lane & 3)) << 1) + ((lane >> 2) & 1);
        mr0 = maskw[at];
        mr1 = maskw[64 + at];
        mr0 &= ~run_mask(rgr.x - col0, rgr.y - col0);
        mr1 &= ~run_mask(rgr.x - (col0 + 32), rgr.y - (col0 + 32));
        const int n_r = __popc(mr0) + __popc(mr1);
        if (n_r > 0) res_r = atomicAdd(&g.cnt[gp], n_r);
    }
    // The one workgroup barrier: every wave has its last fragment reads back (waited for before the epilogue) and
    // its DMA landed; after it the operand stages are the waves' dot blocks.
    // (as inline assembly: before the builtin barrier the compiler waits for EVERY counter, the reservations'
    // round trip included; their first use is after the first half's staging)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float *D = sm + w * EP_BLOCK;
    int base0 = 0, base1 = 0;                                // first free slot of this lane in its two columns' lists
    unsigned long long *dstc0 = g.list + gq0 * g.cap, *dstc1 = g.list + (gq0 + 32) * g.cap;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m) wave_lds_fence();                             // the first half's reads are done
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                f32x4 v4;
                v4[0] = acc[m][n][4 * r4]; v4[1] = acc[m][n][4 * r4 + 1];
                v4[2] = acc[m][n][4 * r4 + 2]; v4[3] = acc[m][n][4 * r4 + 3];
                *(f32x4 *)&D[ep_at(n * 32 + li, 8 * r4 + 4 * lh)] = v4;
            }
        wave_lds_fence();
        if (m == 0) {                                        // (the reservations have had the barrier and the staging to come back)
            const int res_o = __shfl_xor(res_c, 32);
            base0 = lh ? res_o + (other_c & 0xFFFF) : res_c;
            base1 = lh ? res_c + (other_c >> 16) : res_o;
        }
        // Column role: bits 0-15 are column li, bits 16-31 column 32 + li, 16 rows each; two entries per trip
        // (their LDS reads fly together)
        {
            const unsigned int h0 = (mc0 >> (16 * m)) & 0xFFFFu, h1 = (mc1 >> (16 * m)) & 0xFFFFu;
            unsigned int mm = h0 | (h1 << 16);
            const int c0 = __popc(h0);
            const int off0 = base0, off1 = base1 - c0;       // the t-th set bit goes to slot off + t of its column
            int t = 0;
            while (mm) {
                const int p0 = __ffs((int)mm) - 1;
                mm &= mm - 1;
                const bool two = mm != 0u;
                const int p1 = two ? __ffs((int)mm) - 1 : p0;
                mm &= mm - 1;                                   // (0 stays 0)
                const int n0 = p0 >> 4, n1 = p1 >> 4;
                const int l0 = 8 * ((p0 >> 2) & 3) + 4 * lh + (p0 & 3), l1 = 8 * ((p1 >> 2) & 3) + 4 * lh + (p1 & 3);
                const float d0 = D[ep_at(n0 * 32 + li, l0)], d1 = D[ep_at(n1 * 32 + li, l1)];
                const float q0 = nbPs[wr * 64 + m * 32 + l0], q1 = nbPs[wr * 64 + m * 32 + l1];
                const float key0 = fmaf(m2, d0, q0 + (n0 ? nbc1 : nbc0)), key1 = fmaf(m2, d1, q1 + (n1 ? nbc1 : nbc0));
                const int s0 = (n0 ? off1 : off0) + t, s1 = (n1 ? off1 : off0) + t + 1;
                const unsigned int cw0 = cwPs[wr * 64 + m * 32 + l0], cw1 = cwPs[wr * 64 + m * 32 + l1];
                if (s0 < g.cap) (n0 ? dstc1 : dstc0)[s0] = pack_passed(key0, cw0);
                if (two && s1 < g.cap) (n1 ? dstc1 : dstc0)[s1] = pack_passed(key1, cw1);
                t += 2;
            }
            base0 += c0;
            base1 += __popc(h1);
        }
        // Row role: two lanes per row of this half, one per 32-column word
        if (rows) {
            const int rr = lane & 31, own = m * 32 + rr;
            const unsigned int w0 = (unsigned int)__shfl((int)mr0, own), w1 = (unsigned int)__shfl((int)mr1, own);
            int base_r = __shfl(res_r, own) + (lh ? __popc(w0) : 0);
            unsigned int mm = lh ? w1 : w0;
            if (mm) {
                const float nbr = nbPs[wr * 64 + own];
                unsigned long long *dst = g.list + ((int64_t)row0 + own) * g.cap;
                while (mm) {
                    const int ca = 32 * lh + (__ffs((int)mm) - 1);
                    mm &= mm - 1;
                    const bool two = mm != 0u;
                    const int cb = two ? 32 * lh + (__ffs((int)mm) - 1) : ca;
                    mm &= mm - 1;
                    const float d0 = D[ep_at(ca, rr)], d1 = D[ep_at(cb, rr)];
                    const float n0 = nbQs[wc * 64 + ca], n1 = nbQs[wc * 64 + cb];
                    const float key0 = fmaf(m2, d0, nbr + n0), key1 = fmaf(m2, d1, nbr + n1);
                    const unsigned int cw0 = cwQs[wc * 64 + ca], cw1 = cwQs[wc * 64 + cb];
                    if (base_r < g.cap) dst[base_r] = pack_passed(key0, cw0);
                    if (two && base_r + 1 < g.cap) dst[base_r + 1] = pack_passed(key1, cw1);
                    base_r += 2;
                }
            }
        }
    }
}

// ------------------------------------------------ LDS-DMA tile kernel (float16) ----
// The operand slabs are brought in by global_load_lds_dwordx4
// (global -> LDS directly: no staging registers, no ds_write pass).  A slab is 32 samples = 64 bytes per row;
// a wave's DMA instruction fills 16 rows x 64 B = 1 KB lane-linearly, so the row padding of the
// register-staged kernel is not available: the 16-byte chunk g of row r sits in slot g ^ ((r >> 2) & 3)
// (swizzled on the SOURCE address and again on the fragment read), which keeps the sixteen rows a
// ds_read_b128 group touches on distinct banks.  Two slabs of LDS (32 KB), which the epilogue's four wave-private
// dot blocks alias: four workgroups per CU.  The loop is software pipelined: the fragments of k-step t + 1 are read from LDS
// while the matrix cores work on step t (two fragment sets), across the slab boundary as well; the ONE barrier per
// slab sits between the two k-steps of a slab -- there every wave has its reads of the slab back and its DMA of the
// next slab landed (waited for explicitly: a bare s_barrier, __syncthreads()'s fence would add nothing), after it
// the freed stage is refilled with the slab after next.
__global__ __launch_bounds__(256, 4) void k_gram_glds(GramArgs g) {
    __shared__ __attribute__((aligned(16))) float sm[2 * GL_STAGE + 4 * EP_MASKS + 6 * TB];   // operand stages (then the waves' dot blocks) + row masks + bounds / thresholds / candidate words
    float *nbPs = sm + 2 * GL_STAGE + 4 * EP_MASKS;
    float *nbQs = nbPs + TB;
    float *thPs = nbQs + TB;
    float *thQs = thPs + TB;
    unsigned int *cwPs = reinterpret_cast<unsigned int *>(thQs + TB);
    unsigned int *cwQs = cwPs + TB;
    const int chunk = (g.ntiles + 7) >> 3;
    const int t_id = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (t_id >= g.ntiles) return;
    const int4 tile = g.tiles[t_id];
    const int I = tile.x, J = tile.y, roles = tile.z;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), wr = w >> 1, wc = w & 1;
    const int li = lane & 31, lh = lane >> 5;
    const float m2 = *g.m2;
    // DMA sources: wave w fills rows [32 w, 32 w + 32) of A and of B, 16 rows per instruction; lane l
    // lands in row (l >> 2), slot (l & 3) and therefore fetches chunk (l & 3) ^ ((row >> 2) & 3)
    const float *srcA[2], *srcB[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = w * 32 + j * 16 + (lane >> 2);
        const int gch = (lane & 3) ^ ((row >> 2) & 3);
        // (the panel's block of slab 0: a16_index in 32-bit words)
        srcA[j] = g.P + (int64_t)I * TB * g.ld + row * GL_ROW + gch * 4;
        srcB[j] = g.Q + (int64_t)J * TB * g.ld + row * GL_ROW + gch * 4;
    }
    constexpr int slab_stride = TB * GL_ROW;      // the next slab's block
    auto dma = [&](int slab, int stage) {
        float *base = sm + stage * GL_STAGE + (w * 32) * GL_ROW;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            __builtin_amdgcn_global_load_lds((glb_void_t *)(srcA[j] + slab * slab_stride), (lds_void_t *)(base + j * 16 * GL_ROW), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_void_t *)(srcB[j] + slab * slab_stride),
                                             (lds_void_t *)(base + TB * GL_ROW + j * 16 * GL_ROW), 16, 0, 0);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // fragment read offsets (floats) of this lane: rows li and li + 32 of its wave's 64, chunk 2 t + lh swizzled
    const int ra0 = wr * 64 + li, ra1 = ra0 + 32, rb0 = wc * 64 + li, rb1 = rb0 + 32;
    int offA[2][2], offB[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        offA[t][0] = ra0 * GL_ROW + (((2 * t + lh) ^ ((ra0 >> 2) & 3)) << 2);
        offA[t][1] = ra1 * GL_ROW + (((2 * t + lh) ^ ((ra1 >> 2) & 3)) << 2);
        offB[t][0] = (TB + rb0) * GL_ROW + (((2 * t + lh) ^ ((rb0 >> 2) & 3)) << 2);
        offB[t][1] = (TB + rb1) * GL_ROW + (((2 * t + lh) ^ ((rb1 >> 2) & 3)) << 2);
    }
    const int nslab = g.nslab32;          // 32-sample slabs
    f16x8 fa[2][2], fb[2][2];
    auto rd = [&](const float *st, int t) {
        fa[t][0] = *(const f16x8 *)&st[offA[t][0]]; fa[t][1] = *(const f16x8 *)&st[offA[t][1]];
        fb[t][0] = *(const f16x8 *)&st[offB[t][0]]; fb[t][1] = *(const f16x8 *)&st[offB[t][1]];
    };
    auto mm = [&](int t) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[t][0], fb[t][0], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[t][0], fb[t][1], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[t][1], fb[t][0], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[t][1], fb[t][1], acc[1][1], 0, 0, 0);
    };
    dma(0, 0);
    // (the bounds, thresholds and candidate words of the tile's rows and columns: their loads fly with the first slab)
    if (tid < TB) {
        int64_t gp = (int64_t)I * TB + tid;
        nbPs[tid] = g.nbP[gp];
        thPs[tid] = g.thr[gp];
        cwPs[tid] = g.cwP[gp];
    } else {
        int c = tid - TB;
        int64_t gq = (int64_t)J * TB + c;
        nbQs[c] = g.nbQ[gq];
        thQs[c] = g.thr[gq];
        cwQs[c] = g.cwQ[gq];
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    if (nslab > 1) dma(1, 1);
    rd(sm, 0);
    rd(sm, 1);
    __builtin_amdgcn_s_setprio(2);
    for (int slab = 0; slab + 1 < nslab; ++slab) {
        mm(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0070);   // my reads of slab `slab` are back, my DMA of slab + 1 has landed
        __builtin_amdgcn_s_barrier();
        if (slab + 2 < nslab) dma(slab + 2, slab & 1);
        const float *st = sm + ((slab + 1) & 1) * GL_STAGE;
        rd(st, 0);
        __builtin_amdgcn_sched_barrier(0);
        mm(1);
        __builtin_amdgcn_sched_barrier(0);
        rd(st, 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    mm(0);
    if (g.last_steps32 > 1) mm(1);
    __builtin_amdgcn_s_waitcnt(0x0070);   // nothing of this wave in flight into the LDS the dot tile is about to alias
    gram_epilogue(g, sm, nbPs, nbQs, thPs, thQs, cwPs, cwQs, acc, I, J, roles, m2, lane, w, wr, wc, li, lh);
}

// ----------------------------------------------- threshold-estimate Gram (f16) ----
// The admission thresholds only have to put a few hundred candidates per row on the
// lists; they decide nothing (every stored index and distance is re-derived exactly).
// The distances to the M sampled rows come from the same float16 image as the distance
// tiles.  128x128 tile / 4 waves, operand slabs staged global -> registers -> LDS (row
// stride LDA); a slab is 64 float16 (128 B) deep.  (LDS-DMA staging measured slower here:
// this kernel's time is its key-code stores.)

// epilogue of the threshold-estimate tiles: dot products -> 16-bit key codes of every (row, sampled column)
__device__ __forceinline__ void thr_epilogue(float *D, const float *nbPs, const float *nbQs, f32x16 (&acc)[2][2],
                                             const int2 *__restrict__ rangeQ, unsigned int *__restrict__ keys,
                                             const int64_t ldo, const int I, const int J, const float m2, const int tid,
                                             const int wr, const int wc, const int li, const int lh) {
    const int cp = tid & 63, rq = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float nbc0 = nbQs[2 * cp], nbc1 = nbQs[2 * cp + 1];
    const int2 rg0 = rangeQ[(int64_t)J * TB + 2 * cp], rg1 = rangeQ[(int64_t)J * TB + 2 * cp + 1];
    for (int h = 0; h < 2; ++h) {
        wc_sync();
        if (wr == h) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {    // column-major tile, 16-byte writes (see k_gram)
                        const int row = m * 32 + 8 * r4 + 4 * lh;
                        const int col = wc * 64 + n * 32 + li;
                        f32x4 v4;
                        v4[0] = acc[m][n][4 * r4]; v4[1] = acc[m][n][4 * r4 + 1];
                        v4[2] = acc[m][n][4 * r4 + 2]; v4[3] = acc[m][n][4 * r4 + 3];
                        *(f32x4 *)&D[col * LDT + row] = v4;
                    }
        }
        wc_sync();
        // thread = column pair (2cp, 2cp+1) x 16 rows: one 32-bit store carries two 16-bit keys, a
        // wave writes 256 contiguous bytes per row
        const int base_row = I * TB + h * 64 + rq * 16;
        float d0[16], d1[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 a4 = *(const f32x4 *)&D[(2 * cp) * LDT + rq * 16 + 4 * g4];
            const f32x4 b4 = *(const f32x4 *)&D[(2 * cp + 1) * LDT + rq * 16 + 4 * g4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { d0[4 * g4 + e] = a4[e]; d1[4 * g4 + e] = b4[e]; }
        }
        const f32x4 *nbv = (const f32x4 *)&nbPs[h * 64 + rq * 16];
        const unsigned int ex0 = run_mask(rg0.x - base_row, rg0.y - base_row);
        const unsigned int ex1 = run_mask(rg1.x - base_row, rg1.y - base_row);
        unsigned int *out = keys + (((int64_t)base_row * ldo + (int64_t)J * TB) >> 1) + cp;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 nb4 = nbv[g4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int rr = 4 * g4 + e;
                unsigned int c0 = key_code16(fmaf(m2, d0[rr], nb4[e] + nbc0));
                unsigned int c1 = key_code16(fmaf(m2, d1[rr], nb4[e] + nbc1));
                if ((ex0 >> rr) & 1u) c0 = 0xFFFFu;     // same chromosome: never a candidate
                if ((ex1 >> rr) & 1u) c1 = 0xFFFFu;
                out[(int64_t)rr * (ldo >> 1)] = c0 | (c1 << 16);
            }
        }
    }
}

// operands are float16 (scaled by gam, *m2 = -2 / gam^2)
__global__ __launch_bounds__(256, 4) void k_gram_thr16(const unsigned short *__restrict__ P16,
                                                       const unsigned short *__restrict__ Q16, int64_t ld16,
                                                       int nslab, const float *__restrict__ nbP,
                                                       const float *__restrict__ nbQ,
                                                       const int2 *__restrict__ rangeQ,
                                                       const int4 *__restrict__ tiles, int ntiles,
                                                       unsigned int *__restrict__ keys, int64_t ldo,
                                                       const float *__restrict__ m2p) {
    __shared__ __attribute__((aligned(16))) float sm[2 * TB * LDA + 2 * TB];
    float *As = sm;
    float *Bs = sm + TB * LDA;
    float *D = sm;
    float *nbPs = sm + 2 * TB * LDA;
    float *nbQs = nbPs + TB;

    const int chunk = (ntiles + 7) >> 3;
    const int t_id = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (t_id >= ntiles) return;
    const int4 tile = tiles[t_id];
    const int I = tile.x, J = tile.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int li = lane & 31, lh = lane >> 5;
    if (tid < TB) nbPs[tid] = nbP[(int64_t)I * TB + tid];
    else nbQs[tid - TB] = nbQ[(int64_t)J * TB + tid - TB];
    const int lrow = tid >> 3, lcol = (tid & 7) * 8;   // 8 bf16 = 16 bytes per thread and row
    // P is the blocked image (a16_index: a 64-sample slab here is two of its 32-sample blocks), Q the sampled rows
    // as plain rows of ld16 halfs
    const unsigned short *Pg = P16 + a16_index((int64_t)I * TB + lrow, lcol, ld16);
    const unsigned short *Qg = Q16 + ((int64_t)J * TB + lrow) * ld16 + lcol;
    f32x4 pa[4], qb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        pa[p] = *(const f32x4 *)(Pg + p * 32 * 32);
        qb[p] = *(const f32x4 *)(Qg + (int64_t)p * 32 * ld16);
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int lcolf = (tid & 7) * 4;   // the same 16 bytes, in float units of the LDS row
    for (int slab = 0; slab < nslab; ++slab) {
        wc_sync();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *(f32x4 *)&As[(lrow + 32 * p) * LDA + lcolf] = pa[p];
            *(f32x4 *)&Bs[(lrow + 32 * p) * LDA + lcolf] = qb[p];
        }
        wc_sync();
        {
            const int64_t ko = (int64_t)(slab + 1 < nslab ? slab + 1 : slab) * 64;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                pa[p] = *(const f32x4 *)(Pg + ko * TB + p * 32 * 32);      // 64 samples on = two blocks of TB x 32
                qb[p] = *(const f32x4 *)(Qg + ko + (int64_t)p * 32 * ld16);
            }
        }
        // MFMA step t covers k = 16 t .. 16 t + 15; lane half h supplies 8 consecutive k.
        // A and B use the same slots, so the pairing of k is right whatever the hardware order.
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int off = t * 8 + lh * 4;   // float units: (16 t + 8 h) halfs = 32 t + 16 h bytes
            const f16x8 a0 = *(const f16x8 *)&As[(wr * 64 + li) * LDA + off];
            const f16x8 a1 = *(const f16x8 *)&As[(wr * 64 + 32 + li) * LDA + off];
            const f16x8 b0 = *(const f16x8 *)&Bs[(wc * 64 + li) * LDA + off];
            const f16x8 b1 = *(const f16x8 *)&Bs[(wc * 64 + 32 + li) * LDA + off];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    thr_epilogue(D, nbPs, nbQs, acc, rangeQ, keys, ldo, I, J, *m2p, tid, wr, wc, li, lh);
}

__device__ inline uint32_t umed3(uint32_t x, uint32_t y, uint32_t z) {   // v_med3_u32
    const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
    const uint32_t m = hi < z ? hi : z;
    return lo > m ? lo : m;
}

template <int NV>   // keys per lane (M / 64 rounded up to 16 / 32 / 64), two per 32-bit word
__global__ __launch_bounds__(256) void k_select_thr(const unsigned int *__restrict__ keys, int64_t ldo, int M,
                                                    const int2 *__restrict__ chrom_range, int64_t B,
                                                    int64_t row_begin, int64_t row_end, int expect, int cap,
                                                    float *__restrict__ thr) {
    const int lane = threadIdx.x & 63;
    int64_t row = row_begin + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row_end) return;
    // the rows of this row's chromosome (k_convert wrote them): requested WITH the keys -- chrom_of_row -> chrom_off was
    // two more dependent round trips at the end of a wave's life
    const int2 own = chrom_range[row];
    const int words = M / 128;            // 32-bit words per lane
    uint32_t u[NV];
    const uint32_t FIN = 0xFEFFu;         // largest code of a finite key
    // per lane: how many keys are finite, and its four smallest keys (sorted a <= b <= c <= d)
    int myvalid = 0;
    uint32_t a4 = 0xFFFFu, b4 = 0xFFFFu, c4 = 0xFFFFu, d4 = 0xFFFFu;
    const unsigned int *kr = keys + row * (ldo >> 1) + lane;
#pragma unroll
    for (int e = 0; e < NV / 2; ++e) {
        const uint32_t w = e < words ? kr[(int64_t)e * 64] : 0xFFFFFFFFu;
        u[2 * e] = w & 0xFFFFu;
        u[2 * e + 1] = w >> 16;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t x = u[2 * e + t];
            myvalid += x <= FIN;
            d4 = umed3(c4, d4, x);
            c4 = umed3(b4, c4, x);
            b4 = umed3(a4, b4, x);
            a4 = a4 < x ? a4 : x;
        }
    }
    int mvalid = myvalid;
    for (int o = 32; o > 0; o >>= 1) mvalid += __shfl_xor(mvalid, o);
    int64_t nvalid = B - (int64_t)(own.y - own.x);
    float result;
    if (nvalid <= cap / 2) {
        result = WC_ADMIT_ALL;
    } else if (mvalid == 0) {
        result = -INFINITY;
    } else {
        int64_t q = ((int64_t)expect * mvalid + nvalid - 1) / nvalid;
        if (q < 1) q = 1;
        if (q > mvalid) q = mvalid;
        // bitwise search for the q-th smallest 16-bit key code; the threshold is only an
        // admission cut, so the code's bucket is rounded UP, which can only admit more candidates
        uint32_t res = 0;
        if (q <= 48) {
            // The q smallest of the row are spread over 64 lanes (mean q/64 <= 0.75 per lane): the
            // lanes' four smallest hold them all but for a ~3e-4 chance per lane, and then the
            // cut only moves up by one order statistic -- a few more candidates, nothing else.
            for (int bit = 15; bit >= 0; --bit) {
                const uint32_t trial = res | (1u << bit);
                const int c = __popcll(__ballot(a4 < trial)) + __popcll(__ballot(b4 < trial)) +
                              __popcll(__ballot(c4 < trial)) + __popcll(__ballot(d4 < trial));
                if (c < q) res = trial;
            }
        } else {
            for (int bit = 15; bit >= 0; --bit) {
                uint32_t trial = res | (1u << bit);
                int c = 0;
#pragma unroll
                for (int e = 0; e < NV; ++e) c += __popcll(__ballot(u[e] < trial));
                if (c < q) res = trial;
            }
        }
        result = res > FIN ? FLT_MAX : key_from_code16(res);   // never beyond the largest finite key
    }
    if (lane == 0) thr[row] = result;
}

// ------------------------------------------------------------------- finish ----
struct FinishArgs {
    const double *X;
    int64_t B, S;
    const float *norm_lo, *norm_hi, *thr;
    const int *cnt;
    const unsigned long long *list;   // entries: ordered key << 32 | candidate word (row | slack code << index bits)
    unsigned int index_mask;          // the row number's bits of a candidate word
    int cap, k;
    double beta;
    const int *chrom_of_row;
    const int64_t *chrom_off;
    const int2 *chrom_range;   // per row: [first, end) rows of its chromosome
    int64_t row_begin, row_end;
    int32_t *idx_out;
    double *dist_out;
    int *fb_rows, *fb_count;
    const float *bad_norm;   // smallest norm among the rows without a usable float16 image (+inf: none)
    int *row_stat;
    int sum_order;
    int xs_in_lds;
    const int2 *pw_prog;   // pairwise leaf table: {leaf end, adds after it}
    int pw_leaves;
    // Sequential order only: chromosomes with at most ONE bin before them and at most one after.
    // The reference's chromData = concatenate(rows before, rows after) (wisetools.py:386-387) is
    // Fortran ordered only if one of the two pieces has two or more rows; single-row pieces carry
    // no layout, the result comes out C ordered and numpy reduces its rows pairwise whatever the
    // layout of correctedData (found by the seed sweep: 3 bins in 1 + 2, 4 bins in 1 + 2 + 1).
    unsigned long long lone_mask;
};

constexpr int RMAX = 512;       // most candidates re-scored on the fast path (more -> exact fallback)
constexpr int ST_CH = 16;       // samples per staged chunk of the sequential re-score
constexpr int ST_LD = 18;       // LDS row stride of the staged chunk, doubles (even: 16-byte reads; 36 dwords: conflict free)

// k-th smallest (0-based rank kk) 32-bit ordered key among ent[0..n), n <= LIST_CAP.
// Wave 0 holds up to 16 keys per lane and runs a bitwise binary search with wave-wide
// counts (no LDS atomics: the keys of one row share their leading bits, so a histogram
// would serialise on a few addresses).  The result reaches every thread through s_tmp.
template <int NT>
__device__ inline uint32_t select_key(const unsigned long long *ent, int n, int kk, int *s_tmp, int tid) {
    if (tid < 64) {
        // the k-th key only gates a SUPERSET of the k smallest entries, so its 20 leading bits
        // (rounded up) are enough; most rows list <= 512 entries = 8 keys per lane
        uint32_t res = 0;
        if (n <= 512) {
            uint32_t key[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int t = e * 64 + tid;
                key[e] = t < n ? (uint32_t)(ent[t] >> 32) : 0xFFFFFFFFu;
            }
            for (int bit = 31; bit >= 12; --bit) {
                const uint32_t trial = res | (1u << bit);
                int c = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) c += __popcll(__ballot(key[e] < trial));
                if (c <= kk) res = trial;
            }
        } else {
            uint32_t key[LIST_CAP / 64];
#pragma unroll
            for (int e = 0; e < LIST_CAP / 64; ++e) {
                int t = e * 64 + tid;
                key[e] = t < n ? (uint32_t)(ent[t] >> 32) : 0xFFFFFFFFu;
            }
            for (int bit = 31; bit >= 12; --bit) {
                const uint32_t trial = res | (1u << bit);
                int c = 0;
#pragma unroll
                for (int e = 0; e < LIST_CAP / 64; ++e) c += __popcll(__ballot(key[e] < trial));
                if (c <= kk) res = trial;     // fewer than kk+1 keys below trial: the answer is >= trial
            }
        }
        res |= 0xFFFu;
        if (tid == 0) s_tmp[0] = (int)res;
    }
    wc_sync();
    const uint32_t out = (uint32_t)s_tmp[0];
    wc_sync();
    return out;
}

// One workgroup per target row: pick the candidates that can still be among the k
// nearest, re-score them exactly, order them, write the reference's output row.
// NT threads per row: 256 (candidate batches of 128) or 128 (batches of 64, half the LDS,
// twice the rows in flight per CU -- better when the per-row latency dominates, S small).
template <bool SEQ, int NT>
__global__ __launch_bounds__(NT, 4) void k_finish(FinishArgs a) {
    constexpr int CB = NT / 2;        // candidates re-scored per batch (one lane each)
    constexpr int RP = NT / 8;        // candidate rows staged per pass (8 lanes x 16 bytes = one 16-sample chunk row)
    constexpr int NP = CB / RP;       // passes per chunk
    extern __shared__ double xs_dyn[];                     // the target row (S doubles) when it fits
    __shared__ __attribute__((aligned(16))) unsigned long long ent[LIST_CAP > CB * ST_LD ? LIST_CAP : CB * ST_LD];
    __shared__ __attribute__((aligned(16))) unsigned long long dk[RMAX + 2];
    __shared__ __attribute__((aligned(16))) int jv[RMAX + 2];
    __shared__ int cj[RMAX];
    __shared__ double red[4];
    __shared__ int s_tmp[4];
    double *stage = reinterpret_cast<double *>(ent);       // aliases ent once the candidates are compacted
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t row = a.row_begin + blockIdx.x;
    if (row >= a.row_end) return;
    // the first 384 list slots (the expected length) are requested before the count is known:
    // one round trip instead of two before the row's work can start
    constexpr int SPEC = (LIST_CAP * 3 / 8) / NT;
    unsigned long long spec[SPEC];
#pragma unroll
    for (int e = 0; e < SPEC; ++e) spec[e] = a.list[row * a.cap + tid + e * NT];
    const int c = a.cnt[row];
    const float thr_f = a.thr[row];
    const float nhi_f = a.norm_hi[row];           // needed only later: requested now
    const int ch = a.chrom_of_row[row];
    const bool admit_all = (thr_f == WC_ADMIT_ALL);
    bool fallback = c > a.cap || ((a.lone_mask >> ch) & 1ull);   // C-ordered chromData: exact path, pairwise order
    const int n = fallback ? 0 : c;
    // the candidates' upper norm bounds are requested together with the list: the gather's
    // round trip runs under the k-th key search instead of inside the bound computation
    constexpr int EPT = LIST_CAP / NT;     // list entries per thread
    float nh[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int t = tid + e * NT;
        nh[e] = 0.f;
        if (t < n) {
            const unsigned long long en = e < SPEC ? spec[e] : a.list[row * a.cap + t];
            ent[t] = en;
            nh[e] = a.norm_hi[(int)((uint32_t)en & a.index_mask)];
        }
    }
    const double *xi = a.X + row * a.S;
    if (a.xs_in_lds) {
        for (int64_t s = tid; s < a.S; s += NT) xs_dyn[s] = xi[s];
        xi = xs_dyn;
    }
    if (tid == 0) s_tmp[2] = 0;
    wc_sync();

    int R = 0;
    if (!fallback) {
        double U = INFINITY;  // admit-all rows with fewer than k candidates re-score everything
        if (n < a.k) {
            if (!admit_all) fallback = true;
        } else {
            // upper bound of the k-th true distance: the largest upper bound among the
            // entries whose lower bound is within the k smallest
            const uint32_t kth = select_key<NT>(ent, n, a.k - 1, s_tmp, tid);
            const double nhi = (double)nhi_f;
            double my = -INFINITY;
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int t = tid + e * NT;
                if (t < n) {
                    uint32_t ku = (uint32_t)(ent[t] >> 32);
                    if (ku <= kth) {
                        double ub = (double)wc::f32_from_ordered(ku) + (nhi + (double)nh[e]) + 1e-36;
                        my = fmax(my, ub);
                    }
                }
            }
            for (int o = 32; o > 0; o >>= 1) my = fmax(my, __shfl_xor(my, o));
            if (lane == 0) red[tid >> 6] = my;
            wc_sync();
            U = red[0];
            for (int q = 1; q < NT / 64; ++q) U = fmax(U, red[q]);
            // every candidate that was never listed has a lower bound > thr: need thr >= U
            if (!(U == U) || (!admit_all && !(U <= (double)thr_f))) fallback = true;
        }
        {
            // rows with clamped values are never listed: see pick_row
            const float bad = *a.bad_norm;
            if (bad < INFINITY) {
                const double ni = sqrt(fmax((double)a.norm_lo[row] + (double)nhi_f, 0.0));
                if (!((sqrt(fmax(U, 0.0)) + ni) * (1.0 + 1e-3) < (double)bad * (1.0 - 1e-3))) fallback = true;
            }
        }
        if (!fallback) {
            // compact the survivors (order is irrelevant: they are sorted exactly below)
            for (int t0 = 0; t0 < n; t0 += NT) {
                int t = t0 + tid;
                bool keep = false;
                int j = 0;
                if (t < n) {
                    j = (int)((uint32_t)ent[t] & a.index_mask);
                    keep = (double)wc::f32_from_ordered((uint32_t)(ent[t] >> 32)) <= U;
                }
                unsigned long long m = __ballot(keep);
                int base = 0;
                if (lane == 0 && m) base = atomicAdd(&s_tmp[2], __popcll(m));
                base = __shfl(base, 0);
                int at = base + __popcll(m & ((1ull << lane) - 1ull));
                if (keep && at < RMAX) cj[at] = j;
            }
            wc_sync();
            R = s_tmp[2];
            if (R > RMAX) fallback = true;
        }
    }
    if (fallback) {
        if (tid == 0) {
            int at = atomicAdd(a.fb_count, 1);
            a.fb_rows[at] = (int)row;
            a.row_stat[row] = -1;  // exact fallback path
        }
        return;
    }

    {
        // Exact float64 distances (wisetools.py:302) with numpy's rounding order.  16-sample
        // chunks of the candidate rows arrive with coalesced 128-byte loads (the next chunk in
        // flight during the sums), are subtracted and squared by the loading lanes and staged
        // through LDS; one lane per candidate then adds them in numpy's order.
        //   sequential order: one running sum per lane;
        //   pairwise order:   numpy's eight strided accumulators per leaf (<= 128
        //                     samples, boundaries from the host-built leaf table),
        //                     leaf sums folded with a small value stack.
        constexpr bool seq = SEQ;  // sequential order, or fewer than 8 samples (numpy sums those left to right too)
        const int l8 = tid & 7, r0 = tid >> 3;
        for (int b0 = 0; b0 < R; b0 += CB) {
            const int nb = (R - b0) < CB ? (R - b0) : CB;
            // element offsets fit 32 bits whenever the matrix is below 32 GB (checked by the host).
            // Staging rows beyond nb re-read the batch's first candidate; their lanes' sums are dropped.
            unsigned int src[NP];
            f64x2 pre[NP];
            auto fetch = [&](unsigned int so) {     // 16 samples from `so` of every staged row, two per lane
                if ((int64_t)so + ST_CH <= a.S) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) pre[p] = *(const f64x2_u *)&a.X[src[p] + so];
                } else {
                    const int64_t s0 = (int64_t)so + 2 * l8;
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        pre[p].x = s0 < a.S ? a.X[src[p] + so] : 0.0;
                        pre[p].y = s0 + 1 < a.S ? a.X[src[p] + so + 1] : 0.0;
                    }
                }
            };
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                int rr = r0 + RP * p;
                src[p] = (unsigned int)cj[b0 + (rr < nb ? rr : 0)] * (unsigned int)a.S + 2u * (unsigned int)l8;
            }
            fetch(0u);
            double acc = 0.0;                     // sequential sum / tail sum of the last leaf
            double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            double vs[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int sp = 0, leaf = 0;
            bool in_tail = false;
            int2 lf = seq ? make_int2(0, 0) : a.pw_prog[0];   // {leaf end, adds after the leaf}
            for (int64_t c0 = 0; c0 < a.S; c0 += ST_CH) {
                wc_sync();
                {
                    // the staging lanes subtract and square (every lane busy, the target's two
                    // samples read once per chunk); the candidate lanes below only add
                    f64x2 x2;
                    if (c0 + ST_CH <= a.S && a.xs_in_lds) {
                        x2 = *(const f64x2 *)&xi[c0 + 2 * l8];
                    } else {
                        const int64_t s0 = c0 + 2 * l8;
                        x2.x = s0 < a.S ? xi[s0] : 0.0;
                        x2.y = s0 + 1 < a.S ? xi[s0 + 1] : 0.0;
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const double d0 = pre[p].x - x2.x, d1 = pre[p].y - x2.y;
                        f64x2 sq2;
                        sq2.x = d0 * d0;
                        sq2.y = d1 * d1;
                        *(f64x2 *)&stage[(r0 + RP * p) * ST_LD + 2 * l8] = sq2;
                    }
                }
                wc_sync();
                if (c0 + ST_CH < a.S) fetch((unsigned int)(c0 + ST_CH));
                if (SEQ && tid < CB && c0 + ST_CH <= a.S && a.xs_in_lds) {
                    // full chunk, left-to-right sum: 16-byte LDS reads, no per-element control flow
                    const double *sp_ = &stage[tid * ST_LD];
#pragma unroll
                    for (int e = 0; e < ST_CH; e += 2) {
                        const f64x2 v = *(const f64x2 *)(sp_ + e);
                        acc = acc + v.x;
                        acc = acc + v.y;
                    }
                } else if (tid < CB) {
                    const bool full = c0 + ST_CH <= a.S && a.xs_in_lds;
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const int64_t base = c0 + 8 * g;
                        if (base >= a.S) break;
                        const int cntg = (a.S - base) < 8 ? (int)(a.S - base) : 8;
                        double sq[8];
                        if (full) {   // 16-byte LDS reads, no per-element guards
                            const double *sp_ = &stage[tid * ST_LD + 8 * g];
#pragma unroll
                            for (int e = 0; e < 8; e += 2) {
                                const f64x2 v = *(const f64x2 *)(sp_ + e);
                                sq[e] = v.x;
                                sq[e + 1] = v.y;
                            }
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) sq[e] = (e < cntg) ? stage[tid * ST_LD + 8 * g + e] : 0.0;
                        }
                        if (seq || in_tail || cntg < 8) {
                            for (int e = 0; e < cntg; ++e) acc = acc + sq[e];
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) r[e] = r[e] + sq[e];
                            if (base + 8 == (int64_t)(lf.x - (lf.x & 7))) {   // body of the current leaf complete
                                double val = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
                                for (int e = 0; e < 8; ++e) r[e] = 0.0;
                                if (lf.x & 7) {          // last leaf with a tail: added after the combine
                                    acc = val;
                                    in_tail = true;
                                } else {
                                    wc::stack_set(vs, sp++, val);
                                    for (int q = 0; q < lf.y; ++q) {
                                        double right = wc::stack_get(vs, --sp), left = wc::stack_get(vs, sp - 1);
                                        wc::stack_set(vs, sp - 1, left + right);
                                    }
                                    ++leaf;
                                    if (leaf < a.pw_leaves) lf = a.pw_prog[leaf];
                                }
                            }
                        }
                    }
                }
            }
            if (!seq) {
                if (in_tail) {
                    wc::stack_set(vs, sp++, acc);
                    for (int q = 0; q < lf.y; ++q) {
                        double right = wc::stack_get(vs, --sp), left = wc::stack_get(vs, sp - 1);
                        wc::stack_set(vs, sp - 1, left + right);
                    }
                }
                acc = vs[0];
            }
            if (tid < nb) {
                bool ok = acc < SENTINEL_DISTANCE;  // NaN and >= 1e10 are never admitted (wisetools.py:314)
                dk[b0 + tid] = ok ? wc::f64_ordered(acc) : ~0ull;
                jv[b0 + tid] = ok ? cj[b0 + tid] : 0x40000000 + b0 + tid;   // unique, after every real index
            }
        }
    }
    const int64_t cs = a.chrom_off[ch], ce = a.chrom_off[ch + 1];
    const int64_t orow = row - a.row_begin;
    wc_sync();
    {
        // Order by counting: element t goes to slot #{u : (d_u, j_u) < (d_t, j_t)}.  Every thread
        // streams the same (broadcast) LDS pairs, no round-to-round dependencies; the few
        // hundred comparisons per element beat the 28 dependent rounds of a bitonic network.
        if (tid == 0 && (R & 1)) { dk[R] = ~0ull; jv[R] = 0x7FFFFFFF; }
        wc_sync();
        for (int t = tid; t < R; t += NT) {
            const unsigned long long mine = dk[t];
            const int myj = jv[t];
            int rank = 0;
            for (int u = 0; u < R; u += 2) {
                const u64x2 kk = *(const u64x2 *)&dk[u];
                const int2 jj = *(const int2 *)&jv[u];
                rank += (kk.x < mine) | ((kk.x == mine) & (jj.x < myj));
                rank += (kk.y < mine) | ((kk.y == mine) & (jj.y < myj));
            }
            if (rank < a.k) {
                int32_t oi = -1;
                double od = SENTINEL_DISTANCE;
                if (mine != ~0ull) {
                    oi = (int32_t)(myj < cs ? myj : myj - (ce - cs));
                    od = wc::f64_from_ordered(mine);
                }
                a.idx_out[orow * a.k + rank] = oi;
                a.dist_out[orow * a.k + rank] = od;
            }
        }
        for (int t = R + tid; t < a.k; t += NT) {     // fewer candidates than k: sentinels (wisetools.py:305-306)
            a.idx_out[orow * a.k + t] = -1;
            a.dist_out[orow * a.k + t] = SENTINEL_DISTANCE;
        }
    }
    if (tid == 0) a.row_stat[row] = R;  // >= 0: fast path, number of float64 re-scores
}

// ------------------------------------------------------- pair engine (finish) ----
// The same stage D as k_finish, cut into a light per-row pass and a throughput pass:
//   k_pick     one WAVE per row (no workgroup barriers): k-th key by a bitwise search with
//              ballot counts, upper bound U of the k-th true distance, certificate, and the
//              candidates with key <= U written as (row, candidate) pairs into the row's
//              RMAX pair slots; rows without a certificate (or with more pairs) go to the
//              exact path;
//   k_rescore  one wave per 64 pairs of a row (a row with more than `ps` pairs, ps = the
//              workgroup's thread count, takes several trips): float64 distances in numpy's order with all
//              lanes busy -- 16-sample chunks staged through a wave-private LDS slab (the
//              wave's own DS operations complete in order: no barrier inside the loop) --
//              then, after the one barrier that joins the row's waves, the counting order and
//              the output row.
// k_finish needs six dependent phases with workgroup barriers per row (26.6 us per row at
// 100 samples); here the selection runs at full lane occupancy for four rows per workgroup and
// the re-score loop never waits for another wave.
constexpr int PS_MAX = 512;       // most threads of a k_rescore workgroup (pairs re-scored per trip)

struct PickArgs {
    FinishArgs f;
    int *pairs;                   // [rows, RMAX] candidate rows of the fast path
    int ps;                       // threads per k_rescore workgroup: k + margin rounded up to whole waves
};

// Element `i` of a wave-uniform table through a 32-bit byte offset: the load takes its base from scalar registers and
// one address register instead of two; every table here is far below 4 GB.  The offset is made opaque, or a selected
// index is widened before the selection and the address is a 64-bit sum in vector registers again.
template <class T>
__device__ __forceinline__ T at_u32(const T *base, uint32_t i) {
    uint32_t off = i * (uint32_t)sizeof(T);
    asm volatile("" : "+v"(off));
    return *(const T *)((const char *)base + off);
}

// Selection for one row by one wave; NE list entries per lane.  Returns the number of pairs, -1
// when the row has no certificate (exact path).
// A candidate's slack rides in its entry (the code above the row number, slack_of_word): nothing is gathered per
// candidate, the wave's first trip is all it needs on the short form.
// LEAN (the lists beyond 512 entries): only the KEYS stay in registers through the bisection; the candidate words
// are read again behind it (the list is L2-hot) -- the full form of sixteen entries per lane took 77 registers and
// with them the whole kernel's occupancy (six waves per SIMD).
// Every gather here is an UNCONDITIONAL load of a selected index (slot 0 of the list always exists): a load under a
// lane condition is compiled into an exec-masked block with a wait of its own, one memory round trip per entry where
// a batch in front of one wait pays a single trip.
template <int NE, bool LEAN>
__device__ inline int pick_row(const PickArgs &p, int64_t row, int lane, int n, bool admit_all, float thr_f,
                               float nhi_f, float nlo_f, float bad, const unsigned long long (&spec)[8]) {
    const FinishArgs &a = p.f;
    const unsigned long long *lst = a.list + row * a.cap;
    unsigned long long ent[LEAN ? 1 : NE];
    uint32_t key[LEAN ? NE : 1];
    uint32_t cand[LEAN ? NE - 8 : 1];         // candidate words of the entries beyond `spec`
    if constexpr (LEAN) {
        unsigned long long far[NE - 8];
#pragma unroll
        for (int e = 8; e < NE; ++e) far[e - 8] = at_u32(lst, e * 64 + lane < n ? (uint32_t)(e * 64 + lane) : 0u);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int t = e * 64 + lane;
            key[e] = t < n ? (uint32_t)((e < 8 ? spec[e] : far[e < 8 ? 0 : e - 8]) >> 32) : 0xFFFFFFFFu;
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int t = e * 64 + lane;
            ent[e] = t < n ? (e < 8 ? spec[e] : lst[t]) : ~0ull;
        }
    }
    auto KU = [&](int e) -> uint32_t { if constexpr (LEAN) return key[e]; else return (uint32_t)(ent[e] >> 32); };
    auto IDX = [&](int e) -> uint32_t { if constexpr (LEAN) return e < 8 ? (uint32_t)spec[e] : cand[e < 8 ? 0 : e - 8]; else return (uint32_t)ent[e]; };
    double U = INFINITY;   // admit-all rows with fewer than k candidates re-score everything
    if (n < a.k) {
        if (!admit_all) return -1;
    } else {
        // A separator `res` with at least k keys <= res: bisection of the key VALUES between the smallest
        // and the largest listed key (ordered float bits).  It stops as soon as exactly k keys lie at
        // or below the trial -- after about log2(n) + 2 steps, when the interval is narrower than the
        // gap behind the k-th key -- or when the interval is down to 4096 codes (ties, near ties: a
        // superset of the k smallest, as good for the bound below).
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (e * 64 + lane < n) {
                const uint32_t ku = KU(e);
                kmin = ku < kmin ? ku : kmin;
                kmax = ku > kmax ? ku : kmax;
            }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t a2 = (uint32_t)__shfl_xor((int)kmin, o), b2 = (uint32_t)__shfl_xor((int)kmax, o);
            kmin = a2 < kmin ? a2 : kmin;
            kmax = b2 > kmax ? b2 : kmax;
        }
        // invariant: #(key <= lo) < k <= #(key <= hi); lo starts one below the smallest key
        // (as a 33-bit value: kmin may be 0)
        long long lo = (long long)kmin - 1, hi = (long long)kmax;
        uint32_t res = kmax;
        while (hi - lo > 4096) {
            const uint32_t trial = (uint32_t)(lo + ((hi - lo) >> 1));
            int c = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) c += __popcll(__ballot(KU(e) <= trial));
            // entries beyond n carry ~0 keys: never counted (trial < 2^32 - 1 whenever the loop runs)
            if (c >= a.k) { hi = (long long)trial; res = trial; if (c == a.k) break; }
            else lo = (long long)trial;
        }
        // upper bound of the k-th true distance: the largest upper bound among those entries
        const double nhi = (double)nhi_f;
        double my = -INFINITY;
        if constexpr (LEAN) {
            // the candidate words beyond `spec` (whose own ride in its registers) in one batch, kept for the output
            // step; they carry the slacks of the entries at or below the separator.  (The lane number is made opaque
            // here: with the key loads' own addresses these loads are merged into them, and the candidate words -- or
            // their addresses -- live through the bisection in registers the kernel does not have.)
            int ln = lane;
            asm volatile("" : "+v"(ln));
#pragma unroll
            for (int e = 8; e < NE; ++e) cand[e - 8] = (uint32_t)at_u32(lst, e * 64 + ln < n ? (uint32_t)(e * 64 + ln) : 0u);
#pragma unroll
            for (int e = 8; e < NE; ++e) asm volatile("" : "+v"(cand[e - 8]));
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const uint32_t ku = KU(e);
            if (e * 64 + lane < n && ku <= res) {
                const double sl = (double)slack_of_word(IDX(e), a.index_mask);
                const double ub = (double)wc::f32_from_ordered(ku) + (nhi + sl) + 1e-36;
                my = fmax(my, ub);
            }
        }
        for (int o = 32; o > 0; o >>= 1) my = fmax(my, __shfl_xor(my, o));
        U = my;
        // every candidate that was never listed has a lower bound > thr: need thr >= U
        if (!(U == U) || (!admit_all && !(U <= (double)thr_f))) return -1;
    }
    {
        // rows with clamped values are never listed (k_convert): their distance to this row is at least
        // (|a_bad| - |a_i|)^2, which must stay above U (|a_i|^2 <= lo_i + slack_i); an admit-all row with
        // fewer than k candidates (U infinite) cannot tell and takes the exact path
        if (bad < INFINITY) {
            const double ni = sqrt(fmax((double)nlo_f + (double)nhi_f, 0.0));
            if (!((sqrt(fmax(U, 0.0)) + ni) * (1.0 + 1e-3) < (double)bad * (1.0 - 1e-3))) return -1;
        }
    }
    int base = 0;
    int *out = p.pairs + row * RMAX;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const bool keep = e * 64 + lane < n && (double)wc::f32_from_ordered(KU(e)) <= U;
        const unsigned long long m = __ballot(keep);
        const int at = base + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && at < RMAX) out[at] = (int)(IDX(e) & a.index_mask);
        base += __popcll(m);
    }
    return base;
}

__global__ __launch_bounds__(256, 7) void k_pick(PickArgs p) {   // (seven waves per SIMD, 66 registers: the 11 087 rows of cfg2 are 1.55 rounds of the chip instead of 1.8; held to 64 for eight waves one register spills -- 8 bytes of scratch, no faster: EXPERIMENTS.md)
    const FinishArgs &a = p.f;
    const int lane = threadIdx.x & 63;
    // (the wave's number through readfirstlane: the row and every address derived from it are wave-uniform, which
    // the compiler cannot see in threadIdx.x >> 6 -- the row's list, its output and its scalars then take scalar
    // registers and the gathers one address register each)
    const int64_t row = a.row_begin + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= a.row_end) return;
    // The row's scalars -- with the two that the clamped-row test behind the bisection reads, norm_lo and bad_norm --
    // and the first 512 list slots (the expected length is 384; slots beyond the count are never used) are requested
    // together: one round trip before the row's work can start.  The scalars go through VECTOR loads (an opaque zero
    // in the index) and readfirstlane: as scalar loads each is waited for together with the next kernel argument,
    // a chain of trips in front of the list.
    int zl = 0;
    asm volatile("" : "+v"(zl));
    const int c_w = a.cnt[row + zl];
    const float thr_w = a.thr[row + zl], nhi_w = a.norm_hi[row + zl], nlo_w = a.norm_lo[row + zl], bad_w = a.bad_norm[zl];
    const int ch_w = a.chrom_of_row[row + zl];
    unsigned long long spec[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) spec[e] = a.list[row * a.cap + e * 64 + lane];
    // (pinned here: the list loads are otherwise sunk behind the wave-uniform branch on the count, a second trip)
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(spec[e]));
    auto uniform_f = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const int c = __builtin_amdgcn_readfirstlane(c_w), ch = __builtin_amdgcn_readfirstlane(ch_w);
    const float thr_f = uniform_f(thr_w), nhi_f = uniform_f(nhi_w), nlo_f = uniform_f(nlo_w), bad = uniform_f(bad_w);
    const bool admit_all = (thr_f == WC_ADMIT_ALL);
    const bool exact = c > a.cap || ((a.lone_mask >> ch) & 1ull);   // lost entries / C-ordered chromData: exact path
    int R = -1;
    if (!exact) R = c <= 512 ? pick_row<8, false>(p, row, lane, c, admit_all, thr_f, nhi_f, nlo_f, bad, spec)
                             : pick_row<LIST_CAP / 64, true>(p, row, lane, c, admit_all, thr_f, nhi_f, nlo_f, bad, spec);
    if (lane != 0) return;
    if (R < 0 || R > RMAX) {
        const int at = atomicAdd(a.fb_count, 1);
        a.fb_rows[at] = (int)row;
        a.row_stat[row] = -1;              // exact fallback path
        return;
    }
    a.row_stat[row] = R;                   // >= 0: fast path, number of float64 re-scores
}

// Sum of a candidate's squared differences in numpy's order, fed chunk by chunk (ST_CH samples,
// one lane per candidate): the sequential order is one running sum; the pairwise order keeps
// numpy's eight strided accumulators per leaf (<= 128 samples, boundaries from the host-built
// leaf table) and folds the leaf sums with a small value stack.
// value stack of the pairwise fold, addressed by a wave-uniform index through a switch (stays in
// registers); numpy's tree over S <= 8192 samples nests at most seven leaves deep
__device__ inline void vs_set(double (&v)[8], int i, double x) {
    switch (i) {
        case 0: v[0] = x; break; case 1: v[1] = x; break; case 2: v[2] = x; break; case 3: v[3] = x; break;
        case 4: v[4] = x; break; case 5: v[5] = x; break; case 6: v[6] = x; break; default: v[7] = x; break;
    }
}
__device__ inline double vs_get(const double (&v)[8], int i) {
    switch (i) {
        case 0: return v[0]; case 1: return v[1]; case 2: return v[2]; case 3: return v[3];
        case 4: return v[4]; case 5: return v[5]; case 6: return v[6]; default: return v[7];
    }
}

template <bool SEQ>
struct RowSum {
    double acc;
    double r[8];
    double vs[8];
    int sp, leaf;
    bool in_tail;
    int2 lf;
    __device__ inline void init(const FinishArgs &a) {
        acc = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) vs[e] = 0.0;
        sp = 0; leaf = 0; in_tail = false;
        lf = SEQ ? make_int2(0, 0) : a.pw_prog[0];
    }
    // v[0..15] = this candidate's squares of samples c0 .. c0 + 15 (registers: every index below is
    // a compile-time constant); full: all sixteen are real samples
    __device__ inline void chunk_regs(const FinishArgs &a, const double (&v)[ST_CH], int64_t c0, bool full) {
        if (SEQ) {
#pragma unroll
            for (int e = 0; e < ST_CH; ++e) acc = acc + v[e];
            return;
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t base = c0 + 8 * g;
            if (base >= a.S) break;
            const int cntg = full ? 8 : ((a.S - base) < 8 ? (int)(a.S - base) : 8);
            if (in_tail || cntg < 8) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < cntg) acc = acc + v[8 * g + e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) r[e] = r[e] + v[8 * g + e];
                leaf_end(a, base);
            }
        }
    }
    // the same for one group of eight samples starting at `base` (cntg of them real), pairwise order
    __device__ inline void group_regs(const FinishArgs &a, const double (&v)[8], int64_t base, int cntg) {
        if (in_tail || cntg < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < cntg) acc = acc + v[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = r[e] + v[e];
            leaf_end(a, base);
        }
    }
    // after a complete group of eight at `base`: close the leaf when its body ends here
    __device__ inline void leaf_end(const FinishArgs &a, int64_t base) {
        if (base + 8 == (int64_t)(lf.x - (lf.x & 7))) {   // body of the current leaf complete
            const double val = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = 0.0;
            if (lf.x & 7) {          // last leaf with a tail: added after the combine
                acc = val;
                in_tail = true;
            } else {
                vs_set(vs, sp++, val);
                for (int q = 0; q < lf.y; ++q) {
                    const double right = vs_get(vs, --sp), left = vs_get(vs, sp - 1);
                    vs_set(vs, sp - 1, left + right);
                }
                ++leaf;
                if (leaf < a.pw_leaves) lf = a.pw_prog[leaf];
            }
        }
    }
    __device__ inline double result() {
        if (SEQ) return acc;
        if (in_tail) {
            vs_set(vs, sp++, acc);
            for (int q = 0; q < lf.y; ++q) {
                const double right = vs_get(vs, --sp), left = vs_get(vs, sp - 1);
                vs_set(vs, sp - 1, left + right);
            }
        }
        return vs[0];
    }
};

// One workgroup (ps threads = ps / 64 waves) per row; see the header of this section.
// Xp is the padded float64 image (rows of Sp = 16 n samples, zero padded, 128-byte aligned): every
// chunk of every candidate row is one aligned cache line, fetched by eight lanes with 16-byte loads,
// and there are no tail cases -- the zero padding adds +0.0 to sums that are >= +0 (or NaN), which is exact.
// Addresses of the gathers: the chunk's base is wave uniform and lives in scalar registers, a lane's part is one
// 32-bit byte offset per load (the image is below 4 GB), made opaque in front of every load: left alone the compiler
// hoists base + offset out of the chunk loop as eight 64-bit lane addresses and advances each of them per chunk
// (eight v_lshl_add_u64 per chunk and eight more registers).
// Wave slab: 64 candidate rows x 128 bytes, the 16-byte pieces of a row XOR-swizzled by
// f(row) = bits {1, 2, 4} of the row number, which makes the transposing writes (eight lanes
// fill one row) and the per-candidate reads (sixteen lanes, sixteen rows) conflict free without
// padding; the piece addresses are loop invariants held in registers.
// Dynamic LDS: [target row: Sp doubles][wave slabs: 8 KB each]; after the sums (one barrier) the
// slab memory holds dk / jv (distances and candidates as computed), sd / sj (in order) and rk (the rank keys).
constexpr int SLAB_DOUBLES = 64 * ST_CH;
// A wave's passes follow its pairs: the nb pairs of a trip fill (nb + 7) / 8 passes of eight candidate rows ((nb + 15) / 16
// DMA groups of sixteen), and the chunk loop is instantiated on that count -- the staging registers of a pass keep
// compile-time indexes, a pass left out issues no gather, forms no squares and writes no slab piece.  The slab rows of
// such a pass keep whatever an earlier trip, row or kernel left there: only lanes >= nb read them, and their sums are
// dropped where the trip's result is formed.
// GLDS: the candidates' chunks arrive by LDS-DMA (global_load_lds_dwordx4) instead of through staging
// registers + a ds_write pass: the XOR swizzle moves to the source address, the owning lane forms
// (candidate - target)^2 itself from the raw values (the same two roundings per element), and the next
// chunk's DMA runs under the sums of this one.
// The slab as two halves of 64 rows x 64 B: samples 0-7 and 8-15 of the chunk.  A DMA instruction
// covers 16 rows (lane l: row 16 j + (l >> 2), slot l & 3, piece slot ^ ((row >> 2) & 3)); as soon as
// a half has been read into registers the same half of the NEXT chunk is requested, so the DMA runs
// under this chunk's arithmetic without a second slab (LDS per wave as in the register-staged form)
template <bool SEQ, int NGRP>
__device__ __forceinline__ void rescore_chunks_dma(const FinishArgs &a, RowSum<SEQ> &sum, const char *base, const double *xs,
                                                   char *slab, int cj, int Sp, int nchunk, int lane) {
    const int l4 = lane & 3, rq = lane >> 2;
    unsigned int src[NGRP];                              // byte offset of this lane's 16 bytes in chunk 0 of row 16 j + rq
#pragma unroll
    for (int j = 0; j < NGRP; ++j) {
        const int rw = 16 * j + rq;
        src[j] = ((unsigned int)__shfl(cj, rw) * (unsigned int)Sp + 2u * (unsigned int)(l4 ^ ((rw >> 2) & 3))) * 8u;
    }
    int rd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rd[q] = lane * 64 + ((q ^ ((lane >> 2) & 3)) << 4);
    auto dma = [&](int c, int half) {
        const char *cb = base + (size_t)c * (ST_CH * 8) + half * 64;
        char *dst = slab + half * 4096;
#pragma unroll
        for (int j = 0; j < NGRP; ++j)
            __builtin_amdgcn_global_load_lds((glb_void_t *)(cb + src[j]), (lds_void_t *)(dst + j * 1024), 16, 0, 0);
    };
    dma(0, 0);
    dma(0, 1);
    for (int c = 0; c < nchunk; ++c) {
        __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0): both halves of chunk c have landed
        __builtin_amdgcn_wave_barrier();
        f64x2 t[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = *(const f64x2 *)(slab + rd[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) t[4 + q] = *(const f64x2 *)(slab + 4096 + rd[q]);
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) only: the reads are in registers
        __builtin_amdgcn_wave_barrier();
        if (c + 1 < nchunk) { dma(c + 1, 0); dma(c + 1, 1); }
        double v[ST_CH];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f64x2 x2 = *(const f64x2 *)&xs[c * ST_CH + 2 * q];     // wave-uniform: a broadcast read
            const double d0 = t[q].x - x2.x, d1 = t[q].y - x2.y;
            v[2 * q] = d0 * d0;
            v[2 * q + 1] = d1 * d1;
        }
        sum.chunk_regs(a, v, (int64_t)c * ST_CH, (c + 1) * ST_CH <= a.S);
    }
}

// the register-staged form; a lane reads all eight pieces of its own slab row whatever NPASS is
template <bool SEQ, int NPASS>
__device__ __forceinline__ void rescore_chunks_staged(const FinishArgs &a, RowSum<SEQ> &sum, const char *base, const double *xs,
                                                      int cj, int Sp, int nchunk, int lane,
                                                      lds_char_t *const (&wptr)[8], lds_char_t *const (&rptr)[8]) {
    const int l8 = lane & 7, r0 = lane >> 3;
    unsigned int src[NPASS];                             // byte offset of this lane's 16 bytes in chunk 0 of row r0 + 8 q
#pragma unroll
    for (int q = 0; q < NPASS; ++q)
        src[q] = ((unsigned int)__shfl(cj, r0 + 8 * q) * (unsigned int)Sp + 2u * (unsigned int)l8) * 8u;
    f64x2 pre[NPASS];
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
        asm volatile("" : "+v"(src[q]));                 // (see the header: the base stays in scalar registers)
        pre[q] = *(const f64x2 *)(base + src[q]);
    }
    for (int c = 0; c < nchunk; ++c) {
        const f64x2 x2 = *(const f64x2 *)&xs[c * ST_CH + 2 * l8];
        wave_lds_fence();                                // the previous chunk's reads are done
#pragma unroll
        for (int q = 0; q < NPASS; ++q) {
            const double d0 = pre[q].x - x2.x, d1 = pre[q].y - x2.y;
            f64x2 sq2;
            sq2.x = d0 * d0;
            sq2.y = d1 * d1;
            *(lds_f64x2_t *)wptr[q] = sq2;
        }
        wave_lds_fence();
        if (c + 1 < nchunk) {
            const char *cb = base + (size_t)(c + 1) * (ST_CH * 8);      // wave-uniform chunk base
#pragma unroll
            for (int q = 0; q < NPASS; ++q) {
                asm volatile("" : "+v"(src[q]));
                pre[q] = *(const f64x2 *)(cb + src[q]);
            }
        }
        double v[ST_CH];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f64x2 t2 = *(const lds_f64x2_t *)rptr[q];
            v[2 * q] = t2.x;
            v[2 * q + 1] = t2.y;
        }
        sum.chunk_regs(a, v, (int64_t)c * ST_CH, (c + 1) * ST_CH <= a.S);
    }
}

// -- the order of a row's pairs (the tail of k_rescore) --------------------------------------
// Smallest value of a wave (all 64 lanes active): four v_min_u32 over DPP row shifts leave a row's minimum in its last
// lane (a lane without a source keeps the identity), the four rows meet in scalar registers.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#define WC_MIN_SHR(N)                                                                                              \
    {                                                                                                              \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFF, (int)v, 0x110 + N, 0xF, 0xF, false); \
        v = o < v ? o : v;                                                                                         \
    }
    WC_MIN_SHR(1) WC_MIN_SHR(2) WC_MIN_SHR(4) WC_MIN_SHR(8)
#undef WC_MIN_SHR
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 47), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

constexpr int ORDER_OVERREAD = 64;                      // bytes behind the rank keys that order_rank may read
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;

// #{u : rk[u] < mine} over n16 x 16 rank keys (the row's, padded with the top code to whole trips): a trip is four
// 16-byte reads and sixteen 32-bit compares; the next trip's reads are issued in front of this trip's compares.
__device__ __forceinline__ int order_rank(const uint32_t *rk, int n16, uint32_t mine) {
    // Two register sets in turn, and the reads volatile: with one set and a copy, or with plain reads, the compiler
    // moves every read down to the compares that use it and the trip waits out its whole LDS latency.  The read in
    // front of the last trip's compares goes one trip beyond the keys, inside the slab memory (ORDER_OVERREAD); it is
    // never counted.
    const volatile lds_u32x4_t *rp = (const volatile lds_u32x4_t *)rk;
    u32x4 a0 = rp[0], a1 = rp[1], a2 = rp[2], a3 = rp[3], b0, b1, b2, b3;
    int rank = 0;
    auto count = [&](const u32x4 &k) { rank += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine); };
    for (int u = 1;; u += 2) {
        b0 = rp[4], b1 = rp[5], b2 = rp[6], b3 = rp[7];
        count(a0); count(a1); count(a2); count(a3);
        if (u >= n16) break;
        rp += 8;
        a0 = rp[0], a1 = rp[1], a2 = rp[2], a3 = rp[3];
        count(b0); count(b1); count(b2); count(b3);
        if (u + 1 >= n16) break;
    }
    return rank;
}

// The row's R pairs, (my_d[t], my_j[t]) of trip t in the thread that re-scored them (pair t * ps + tid), in stable
// (distance, position) order -> output row (wisetools.py:305-324).  `lds` is the slab memory behind the row's own
// values, which every wave has left; `min_hi` the smallest high word among the row's keys.
// Order by counting on the 32-bit image of the key (order_key32): element t goes to slot #{u : r_u < r_t}.  Equal
// images -- equal distances, distances closer than the image resolves or both beyond its range, entries without a
// distance -- are rare; they land on one slot, one of them finds the other's index there, and the row goes through a
// second sweep on the full key with the index as tie-break.  TRIPS: the most pairs a thread may hold.
template <int TRIPS>
__device__ __forceinline__ void rescore_order(const PickArgs &p, double *lds, int64_t row, int R, int tid, int2 own,
                                              uint32_t min_hi, int *clash, const unsigned long long *my_d,
                                              const int *my_j) {
    const FinishArgs &a = p.f;
    asm volatile("" : "+v"(tid));       // opaque: nothing formed from the thread number lives through the chunk loop for this
    unsigned long long *dk = reinterpret_cast<unsigned long long *>(lds);
    unsigned long long *sd = dk + RMAX + 2;
    int *jv = reinterpret_cast<int *>(sd + RMAX);
    int *sj = jv + RMAX + 2;
    uint32_t *rk = reinterpret_cast<uint32_t *>(sj + RMAX + 2);       // 16-byte aligned; RMAX is whole trips
    uint32_t my_r[TRIPS];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
        const int e = t * p.ps + tid;
        if (e < R) {
            my_r[t] = wc::order_key32(my_d[t], min_hi, wc::ORDER_KEY_SH);
            dk[e] = my_d[t];
            jv[e] = my_j[t];
            rk[e] = my_r[t];
        }
    }
    const int n16 = __builtin_amdgcn_readfirstlane((R + 15) >> 4);
    if (tid < 16 && R + tid < 16 * n16) rk[R + tid] = 0xFFFFFFFFu;    // never below a real one
    wc_sync();
    int slot[TRIPS];
    {
        int t2 = 0;
        for (int e = tid; e < R; e += p.ps, ++t2) {
            uint32_t mine = 0;
            unsigned long long d = 0;
            int j = 0;
#pragma unroll
            for (int t = 0; t < TRIPS; ++t)
                if (t == t2) { mine = my_r[t]; d = my_d[t]; j = my_j[t]; }
            const int rank = order_rank(rk, n16, mine);
            sd[rank] = d;
            sj[rank] = j;
#pragma unroll
            for (int t = 0; t < TRIPS; ++t)
                if (t == t2) slot[t] = rank;
        }
    }
    wc_sync();
    // (a flag and one barrier: __syncthreads_or is a reduction, an LDS atomic and three barriers)
#pragma unroll
    for (int t = 0; t < TRIPS; ++t)
        if (t * p.ps + tid < R && sj[slot[t]] != my_j[t]) *clash = 1;  // the indexes are unique
    wc_sync();
    if (__builtin_amdgcn_readfirstlane(*clash)) {
        for (int t = tid; t < R; t += p.ps) {
            const unsigned long long mine = dk[t];
            const int myj = jv[t];
            int rank = 0;
            for (int u = 0; u < R; ++u) rank += (dk[u] < mine) | ((dk[u] == mine) & (jv[u] < myj));
            sd[rank] = mine;
            sj[rank] = myj;
        }
        wc_sync();
    }
    const int cs = own.x, ce = own.y;
    const int64_t orow = row - a.row_begin;
    for (int t = tid; t < a.k; t += p.ps) {
        int32_t oi = -1;                                 // fewer candidates than k: sentinels (wisetools.py:305-306)
        double od = SENTINEL_DISTANCE;
        if (t < R && sd[t] != ~0ull) {
            const int myj = sj[t];
            oi = (int32_t)(myj < cs ? myj : myj - (ce - cs));
            od = wc::f64_from_ordered(sd[t]);
        }
        a.idx_out[orow * a.k + t] = oi;
        a.dist_out[orow * a.k + t] = od;
    }
}

template <bool SEQ, bool GLDS>
__global__ __launch_bounds__(PS_MAX, (SEQ && !GLDS) ? 4 : (SEQ ? 5 : 3)) void k_rescore(PickArgs p, const double *__restrict__ Xp, int Sp) {
    const FinishArgs &a = p.f;
    extern __shared__ __attribute__((aligned(16))) double rs_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row = a.row_begin + blockIdx.x;
    // the row's state, its own values, the first trip's pairs and -- for the output -- the rows of its
    // chromosome are requested together: one round trip where there were three in front of the chunks and
    // two more (chrom_of_row -> chrom_off) behind the order (the pair slots beyond the row's count hold
    // stale indexes; they are replaced below before anything is gathered)
    const int cj_first = p.pairs[row * RMAX + tid];      // tid < ps <= RMAX
    const int R = a.row_stat[row];
    const int2 own = a.chrom_range[row];                 // [first, end) rows of the row's chromosome
    double *xs = rs_dyn;
    char *slab = reinterpret_cast<char *>(rs_dyn + Sp + w * SLAB_DOUBLES);
    {
        const double *xi = Xp + row * Sp;
        for (int s = tid; s < Sp; s += p.ps) xs[s] = xi[s];
    }
    if (R < 0) return;                                   // exact path (workgroup-uniform)
    __shared__ uint32_t s_min_hi;
    __shared__ int s_clash;                              // two pairs on one slot of the order (rescore_order)
    if (tid == 0) { s_min_hi = 0xFFFFFFFFu; s_clash = 0; }
    wc_sync();
    const int l8 = lane & 7, r0 = lane >> 3;
    constexpr int NP = 8;                                // 8 rows per pass x 8 passes = the wave's 64 candidates
    constexpr int TRIPS = RMAX / 128;                    // a wave's trips with the smallest workgroup (two waves)
    auto swz = [](int r) { return ((r >> 1) & 3) | (((r >> 4) & 1) << 2); };
    // LDS addresses of the written and of the read pieces in the wave's slab, pinned in registers: left to itself the
    // compiler keeps a common part and the piece parts apart and adds them per piece and chunk in every instance of the
    // chunk loop (ten address adds beside the 48 float64 operations of a chunk).  The written pieces of passes q and
    // q + 2 differ by a constant (bit 4 of the row is bit 1 of q), which goes into the instruction's offset.
    lds_char_t *wptr[NP], *rptr[NP], *wbase[2];
    lds_char_t *slab3 = (lds_char_t *)slab;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        wbase[h] = slab3 + r0 * 128 + ((l8 ^ swz(r0 + 16 * h)) << 4);
        asm volatile("" : "+v"(wbase[h]));
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        wptr[q] = wbase[(q >> 1) & 1] + q * 1024;        // row r0 + 8 q
        rptr[q] = slab3 + lane * 128 + ((q ^ swz(lane)) << 4);
        asm volatile("" : "+v"(rptr[q]));
    }
    unsigned long long my_d[TRIPS];
    int my_j[TRIPS];
    int trip = 0;
    const int nchunk = Sp / ST_CH;
    const char *base = reinterpret_cast<const char *>(Xp);
    for (int b0 = w * 64; b0 < R; b0 += p.ps, ++trip) {
        const int nb = R - b0 < 64 ? R - b0 : 64;        // pairs of this wave in this trip
        const int *cjp = p.pairs + row * RMAX + b0;
        int cj = trip == 0 ? cj_first : cjp[lane < nb ? lane : 0];
        if (trip == 0) cj = __shfl(cj, lane < nb ? lane : 0);   // lanes beyond nb take the trip's first candidate; their sums are dropped
        RowSum<SEQ> sum;
        sum.init(a);
        // the chunk loop on the number of passes (DMA groups) the wave's nb pairs fill
        if constexpr (GLDS) {
            switch (__builtin_amdgcn_readfirstlane((nb + 15) >> 4)) {
                case 1: rescore_chunks_dma<SEQ, 1>(a, sum, base, xs, slab, cj, Sp, nchunk, lane); break;
                case 2: rescore_chunks_dma<SEQ, 2>(a, sum, base, xs, slab, cj, Sp, nchunk, lane); break;
                case 3: rescore_chunks_dma<SEQ, 3>(a, sum, base, xs, slab, cj, Sp, nchunk, lane); break;
                default: rescore_chunks_dma<SEQ, 4>(a, sum, base, xs, slab, cj, Sp, nchunk, lane); break;
            }
        } else {
            switch (__builtin_amdgcn_readfirstlane((nb + 7) >> 3)) {
                case 1:                                  // (with case 2: one gather in front of a wait is a lone round trip per chunk)
                case 2: rescore_chunks_staged<SEQ, 2>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                case 3: rescore_chunks_staged<SEQ, 3>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                case 4: rescore_chunks_staged<SEQ, 4>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                case 5: rescore_chunks_staged<SEQ, 5>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                case 6: rescore_chunks_staged<SEQ, 6>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                case 7: rescore_chunks_staged<SEQ, 7>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
                default: rescore_chunks_staged<SEQ, 8>(a, sum, base, xs, cj, Sp, nchunk, lane, wptr, rptr); break;
            }
        }
        const double d = sum.result();
        const bool ok = lane < nb && d < SENTINEL_DISTANCE;  // NaN and >= 1e10 are never admitted (wisetools.py:314)
        const unsigned long long dd = ok ? wc::f64_ordered(d) : ~0ull;
        const int jj = ok ? cj : 0x40000000 + b0 + lane;      // unique, after every real index
        // the smallest high word of the row's keys, for the rank image: the wave's into LDS (~0 carries the identity)
        const uint32_t hmin = wave_min_u32((uint32_t)(dd >> 32));
        if (lane == 0) atomicMin(&s_min_hi, hmin);
#pragma unroll
        for (int t = 0; t < TRIPS; ++t)
            if (t == trip) { my_d[t] = dd; my_j[t] = jj; }
    }
    wc_sync();                                    // every wave is through with its slab
    // (TRIPS = 1, the rows with a pair per thread at most: no selection among the trips' registers)
    if (R <= p.ps) rescore_order<1>(p, rs_dyn + Sp, row, R, tid, own, s_min_hi, &s_clash, my_d, my_j);
    else rescore_order<TRIPS>(p, rs_dyn + Sp, row, R, tid, own, s_min_hi, &s_clash, my_d, my_j);
}

// -- exact path: the slow filler and the selection ------------------------------------------
// fb_fill: float64 distance keys of `row` to the candidates [j0, j1) into sc[j], one thread per
// candidate (its 128-byte chunks are whole cache lines), numpy's order by RowSum; same chromosome /
// NaN / >= 1e10 -> ~0.  Only the rows the tiled kernel leaves out come here: rows of a "lone"
// chromosome (pairwise order whatever the layout) and targets beyond EX_CAP.
template <bool SEQ>
__device__ inline void fb_fill_order(const FinishArgs &a, int64_t row, const double *xi, int64_t j0, int64_t j1,
                                     unsigned long long *__restrict__ sc, int tid) {
    const int ch = a.chrom_of_row[row];
    const int64_t cs = a.chrom_off[ch], ce = a.chrom_off[ch + 1];
    for (int64_t base = j0; base < j1; base += 256) {
        const int64_t j = base + tid;
        const bool in = j < j1;
        const double *xj = a.X + (in ? j : row) * a.S;
        RowSum<SEQ> sum;
        sum.init(a);
        for (int64_t c0 = 0; c0 < a.S; c0 += ST_CH) {
            double v[ST_CH];
#pragma unroll
            for (int e = 0; e < ST_CH; ++e) {
                const double d = c0 + e < a.S ? xj[c0 + e] - xi[c0 + e] : 0.0;   // zero padding: adds +0.0 to sums >= +0
                v[e] = d * d;
            }
            sum.chunk_regs(a, v, c0, c0 + ST_CH <= a.S);
        }
        const double d = sum.result();
        if (in) {
            const bool ok = !(j >= cs && j < ce) && d < SENTINEL_DISTANCE;
            sc[j] = ok ? wc::f64_ordered(d) : ~0ull;
        }
    }
}
__device__ inline void fb_fill(const FinishArgs &a, int64_t row, const double *xi, int64_t j0, int64_t j1,
                               unsigned long long *__restrict__ sc, int tid) {
    const bool lone = (a.lone_mask >> a.chrom_of_row[row]) & 1ull;
    // fewer than eight samples: numpy's pairwise sum is the plain left-to-right one
    if (a.S < 8 || (!lone && a.sum_order == WC_SUM_SEQUENTIAL)) fb_fill_order<true>(a, row, xi, j0, j1, sc, tid);
    else fb_fill_order<false>(a, row, xi, j0, j1, sc, tid);
}

// Radix selection (8-bit digits, most significant first) of the element of 0-based rank `want`
// among the values v(j), j in [0, n), for which use(j) holds.  All 256 threads take part.
template <int BITS, class V, class U>
__device__ inline unsigned long long fb_radix_select(int64_t n, int want, V v, U use, unsigned int *hist,
                                                     unsigned long long *s_pref, int *s_want, int tid) {
    unsigned long long prefix = 0ull, mask = 0ull;
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        wc_sync();
        for (int64_t j = tid; j < n; j += 256) {
            if (!use(j)) continue;
            const unsigned long long key = v(j);
            if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        wc_sync();
        if (tid == 0) {
            int kk = want, d = 0;
            for (; d < 255; ++d) {
                if (kk < (int)hist[d]) break;
                kk -= (int)hist[d];
            }
            *s_want = kk;
            *s_pref = prefix | ((unsigned long long)d << shift);
        }
        wc_sync();
        want = *s_want;
        prefix = *s_pref;
        mask |= 0xFFull << shift;
        wc_sync();
    }
    return prefix;
}

// fb_select: the k smallest (distance, position) pairs of sc[0..B) in order -> output row.
// The k-th smallest key by radix selection; everything below it is taken, of the entries that
// tie with it the lowest positions (a second selection over the positions when there are more
// ties than places); the <= 256 chosen entries are ordered by counting.
__device__ inline void fb_select(const FinishArgs &a, int64_t row, const unsigned long long *sc,
                                 unsigned long long *selk, int *selj, unsigned int *hist, int tid) {
    __shared__ unsigned long long s_pref;
    __shared__ int s_int[4];
    const int ch = a.chrom_of_row[row];
    const int64_t cs = a.chrom_off[ch], ce = a.chrom_off[ch + 1];
    const int64_t orow = row - a.row_begin;
    // how many candidates carry a distance at all
    if (tid < 4) s_int[tid] = 0;
    wc_sync();
    {
        int mine = 0;
        for (int64_t j = tid; j < a.B; j += 256) mine += sc[j] != ~0ull;
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if ((tid & 63) == 0) atomicAdd(&s_int[0], mine);
    }
    wc_sync();
    const int n_valid = s_int[0];
    const int take = n_valid < a.k ? n_valid : a.k;        // entries that exist; the rest is padding
    wc_sync();
    unsigned long long kth = ~0ull;
    int jth = 0x7FFFFFFF;
    if (take > 0) {
        kth = fb_radix_select<64>(a.B, take - 1, [&](int64_t j) { return sc[j]; }, [&](int64_t) { return true; },
                                  hist, &s_pref, &s_int[1], tid);
        // entries below the k-th key, and entries equal to it
        if (tid < 4) s_int[tid] = 0;
        wc_sync();
        int below = 0, equal = 0;
        for (int64_t j = tid; j < a.B; j += 256) {
            const unsigned long long v = sc[j];
            below += v < kth;
            equal += v == kth;
        }
        for (int o = 32; o > 0; o >>= 1) { below += __shfl_xor(below, o); equal += __shfl_xor(equal, o); }
        if ((tid & 63) == 0) { atomicAdd(&s_int[2], below); atomicAdd(&s_int[3], equal); }
        wc_sync();
        const int n_below = s_int[2], n_equal = s_int[3], places = take - n_below;
        wc_sync();
        if (n_equal > places)      // more ties than places: the lowest positions win (stable order)
            jth = (int)fb_radix_select<32>(a.B, places - 1, [&](int64_t j) { return (unsigned long long)j; },
                                           [&](int64_t j) { return sc[j] == kth; }, hist, &s_pref, &s_int[1], tid);
    }
    if (tid == 0) s_int[0] = 0;
    wc_sync();
    for (int64_t j = tid; j < a.B; j += 256) {
        const unsigned long long v = sc[j];
        if (take > 0 && (v < kth || (v == kth && (int)j <= jth))) {
            const int at = atomicAdd(&s_int[0], 1);
            if (at < K_MAX) { selk[at] = v; selj[at] = (int)j; }
        }
    }
    wc_sync();
    // order the chosen entries by counting, write the row
    for (int t = tid; t < a.k; t += 256) {
        int32_t oi = -1;
        double od = SENTINEL_DISTANCE;
        if (t < take) {
            const unsigned long long mine = selk[t];
            const int myj = selj[t];
            int rank = 0;
            for (int u = 0; u < take; ++u) rank += (selk[u] < mine) | ((selk[u] == mine) & (selj[u] < myj));
            oi = (int32_t)(myj < cs ? myj : myj - (ce - cs));
            od = wc::f64_from_ordered(mine);
            a.idx_out[orow * a.k + rank] = oi;
            a.dist_out[orow * a.k + rank] = od;
        } else {
            a.idx_out[orow * a.k + t] = -1;
            a.dist_out[orow * a.k + t] = SENTINEL_DISTANCE;
        }
    }
    wc_sync();
}

// ------------------------------------------------------------ exact path, tiled ----
// Float64 distances of a SET of target rows to every candidate, in numpy's rounding order, then the
// k smallest per row.  Who takes it: rows whose certificate failed (ties at the boundary, outlier rows,
// lost list entries), every row when refsize > 256, and wc_newref_exact_dev -- the entry point the
// full-size tests use to check the fast path row by row.
//   k_exact_tile    EX_T x EX_T (target, candidate) pairs per 256-thread workgroup, every thread a
//                   TR x TR block of pairs: 16-sample chunks of the 2 EX_T rows are staged through LDS
//                   (sample-major, so a thread's TR targets are 16-byte reads and the candidates of the
//                   sixteen lanes of a row of threads are consecutive), the next chunk's loads in flight;
//                   a pair's squared differences are added in numpy's order -- sequential: one
//                   running sum per pair (4 x 4 pairs per thread, sixteen independent chains);
//                   pairwise: RowSum<false> per pair (2 x 2 pairs per thread).  Ordered keys of the
//                   distances go to scratch[target slot][candidate] (~0: same chromosome, NaN, >= 1e10).
//   k_exact_select  one workgroup per target: radix selection of the k-th key, counting order, output row
//                   (fb_select).  The launch boundary between the two is the only synchronisation.
// Up to EX_CAP targets per launch pair; a normal pass does not know the number of certificate failures
// on the host (no read-back), so the grid is sized for EX_CAP and surplus workgroups leave at once; targets
// beyond EX_CAP (pathological inputs) are filled and selected by one workgroup each in k_exact_select.
// Rows of a "lone" chromosome (FinishArgs::lone_mask: pairwise order whatever the layout) are filled by
// their select workgroup as well.
constexpr int EX_CAP = 1024;     // targets per launch pair when the host knows their number (scratch: EX_CAP rows of Bpad keys)
constexpr int EX_DEV_CAP = 256;  // ... when only the device does (the normal pass: scratch 2 EX_DEV_CAP rows)
constexpr int EX_LD = 130;       // doubles per staged sample: 128 values + 2 (16-byte aligned rows, spread banks)

constexpr int EXACT_TILE_LDS = ST_CH * EX_LD * 8 + 64 * 4 + 64 * 8;     // buf + s_row + s_rng (64 = the largest EX_T)
// (bx, by, ny): this workgroup's candidate tile, its first row group and the row groups in flight; nf: rows of this launch
template <bool SEQ>
__device__ inline void exact_tile_body(const FinishArgs &a, const int *__restrict__ rows, int nf, int first,
                                       unsigned long long *__restrict__ scratch, int64_t Bpad, int bx, int by, int ny,
                                       char *smem) {
    constexpr int TR = SEQ ? 4 : 2;            // pairs per thread: TR targets x TR candidates
    constexpr int EX_T = 16 * TR;              // targets (and candidates) per tile
    constexpr int NLD = 2 * EX_T * ST_CH / 256;   // staged values per thread and chunk
    double *buf = reinterpret_cast<double *>(smem);
    int *s_row = reinterpret_cast<int *>(smem + ST_CH * EX_LD * 8);
    int2 *s_rng = reinterpret_cast<int2 *>(smem + ST_CH * EX_LD * 8 + 64 * 4);
    const int tid = threadIdx.x;
    const int tr = tid >> 4, tc = tid & 15;
    const int64_t j0 = (int64_t)bx * EX_T;
    for (int rg = by; rg * EX_T < nf; rg += ny) {
        wc_sync();
        if (tid < EX_T) {
            const int f = rg * EX_T + tid;
            const int row = rows[first + (f < nf ? f : rg * EX_T)];      // slots beyond nf repeat the group's first row
            s_row[tid] = row;
            const int ch = a.chrom_of_row[row];
            const bool lone = (a.lone_mask >> ch) & 1ull;                // filled by k_exact_select instead
            s_rng[tid] = (f < nf && !lone) ? make_int2((int)a.chrom_off[ch], (int)a.chrom_off[ch + 1]) : make_int2(0, 0x7FFFFFFF);
        }
        wc_sync();
        // staging: value e = tid + 256 q of a chunk is sample e & 15 of staged row e >> 4 (targets, then candidates)
        int64_t src[NLD];
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int rr = (tid + 256 * q) >> 4;
            int64_t row = rr < EX_T ? (int64_t)s_row[rr] : j0 + (rr - EX_T);
            row = row < a.B ? row : a.B - 1;
            src[q] = row * a.S + (tid & 15);
        }
        double pre[NLD];
        auto fetch = [&](int64_t c0) {
            const bool in = c0 + (tid & 15) < a.S;
#pragma unroll
            for (int q = 0; q < NLD; ++q) pre[q] = in ? a.X[src[q] + c0] : 0.0;     // zero padding: adds +0.0 to sums >= +0
        };
        fetch(0);
        RowSum<SEQ> sum[TR][TR];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int q = 0; q < TR; ++q) sum[i][q].init(a);
        for (int64_t c0 = 0; c0 < a.S; c0 += ST_CH) {
            wc_sync();                       // the previous chunk's reads are done
#pragma unroll
            for (int q = 0; q < NLD; ++q) buf[(tid & 15) * EX_LD + ((tid + 256 * q) >> 4)] = pre[q];
            wc_sync();
            if (c0 + ST_CH < a.S) fetch(c0 + ST_CH);
            if constexpr (SEQ) {
#pragma unroll
                for (int s = 0; s < ST_CH; ++s) {
                    const f64x2 ra = *(const f64x2 *)&buf[s * EX_LD + 4 * tr], rb = *(const f64x2 *)&buf[s * EX_LD + 4 * tr + 2];
                    const double xr[4] = {ra.x, ra.y, rb.x, rb.y};
                    double xc[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) xc[q] = buf[s * EX_LD + EX_T + tc + 16 * q];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double d = xc[q] - xr[i];
                            const double sq = d * d;
                            sum[i][q].acc = sum[i][q].acc + sq;
                        }
                }
            } else {
#pragma unroll 1
                for (int g = 0; g < 2; ++g) {
                    const int64_t base = c0 + 8 * g;
                    if (base >= a.S) break;
                    double xr[2][8], xc[2][8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const f64x2 r2 = *(const f64x2 *)&buf[(8 * g + e) * EX_LD + 2 * tr];
                        xr[0][e] = r2.x; xr[1][e] = r2.y;
                        xc[0][e] = buf[(8 * g + e) * EX_LD + EX_T + tc];
                        xc[1][e] = buf[(8 * g + e) * EX_LD + EX_T + tc + 16];
                    }
                    const int cntg = (a.S - base) < 8 ? (int)(a.S - base) : 8;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            double v[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const double d = xc[q][e] - xr[i][e];
                                v[e] = d * d;
                            }
                            sum[i][q].group_regs(a, v, base, cntg);
                        }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            const int rl = TR * tr + i, f = rg * EX_T + rl;
            if (f >= nf) continue;
            const int2 rng = s_rng[rl];
            if (rng.y == 0x7FFFFFFF) continue;      // lone chromosome: filled by k_exact_select
            unsigned long long *sc = scratch + (int64_t)f * Bpad;
#pragma unroll
            for (int q = 0; q < TR; ++q) {
                const int64_t j = j0 + tc + 16 * q;
                if (j >= a.B) continue;
                const double d = sum[i][q].result();
                const bool ok = !(j >= rng.x && j < rng.y) && d < SENTINEL_DISTANCE;   // NaN and >= 1e10 are never admitted (wisetools.py:314)
                sc[j] = ok ? wc::f64_ordered(d) : ~0ull;
            }
        }
    }
}

template <bool SEQ>
__global__ __launch_bounds__(256) void k_exact_tile(FinishArgs a, const int *__restrict__ rows,
                                                    const int *__restrict__ n_rows_dev, int n_rows_host, int first,
                                                    unsigned long long *__restrict__ scratch, int64_t Bpad, int cap) {
    __shared__ __attribute__((aligned(16))) char smem[EXACT_TILE_LDS];
    int nf = (n_rows_dev ? *n_rows_dev : n_rows_host) - first;
    nf = nf > cap ? cap : nf;
    if (nf <= 0) return;
    exact_tile_body<SEQ>(a, rows, nf, first, scratch, Bpad, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y, smem);
}

constexpr int EXACT_SELECT_LDS = K_MAX * 8 + K_MAX * 4 + 256 * 4 + 2048 * 8;    // rk + rj + hist + xs
// bx of nx select workgroups; count: rows listed (first .. ), of which the first `cap` were filled by the tiles;
// beyond_cap: also take the rows beyond the cap (the count was only known on the device)
__device__ inline void exact_select_body(const FinishArgs &a, const int *__restrict__ rows, int count, int first,
                                         unsigned long long *__restrict__ scratch, int64_t Bpad, int cap, int bx, int nx,
                                         bool beyond_cap, char *smem) {
    unsigned long long *rk = reinterpret_cast<unsigned long long *>(smem);
    int *rj = reinterpret_cast<int *>(smem + K_MAX * 8);
    unsigned int *hist = reinterpret_cast<unsigned int *>(smem + K_MAX * 12);
    double *xs = reinterpret_cast<double *>(smem + K_MAX * 12 + 256 * 4);
    const int tid = threadIdx.x;
    const int nf = count > cap ? cap : count;
    if (bx < nf) {
        const int64_t row = rows[first + bx];
        unsigned long long *sc = scratch + (int64_t)bx * Bpad;
        if ((a.lone_mask >> a.chrom_of_row[row]) & 1ull) fb_fill(a, row, a.X + row * a.S, 0, a.B, sc, tid);
        wc_sync();
        fb_select(a, row, sc, rk, rj, hist, tid);
    }
    // targets beyond the cap (only when the host does not know the count: it loops over bands otherwise)
    if (!beyond_cap) return;
    unsigned long long *own = scratch + ((int64_t)cap + bx) * Bpad;
    for (int f = cap + bx; f < count; f += nx) {
        const int64_t row = rows[first + f];
        const double *xi = a.X + row * a.S;
        wc_sync();
        if (a.S <= 2048) {
            for (int64_t s = tid; s < a.S; s += 256) xs[s] = xi[s];
            xi = xs;
        }
        wc_sync();
        fb_fill(a, row, xi, 0, a.B, own, tid);
        wc_sync();
        fb_select(a, row, own, rk, rj, hist, tid);
    }
}

__global__ __launch_bounds__(256) void k_exact_select(FinishArgs a, const int *__restrict__ rows, int n_rows_host, int first,
                                                      unsigned long long *__restrict__ scratch, int64_t Bpad, int cap) {
    __shared__ __attribute__((aligned(16))) char smem[EXACT_SELECT_LDS];
    exact_select_body(a, rows, n_rows_host - first, first, scratch, Bpad, cap, (int)blockIdx.x, (int)gridDim.x, false, smem);
}

// The normal pass: the number of rows without a certificate is only known on the device (usually NONE), and the two
// stages were two launches that both found nothing to do -- 9.1 us = 4.6 % of a 100 x 250 kb pass.  ONE launch: the
// first n_tile workgroups are the tiles (ctiles x row groups), the next n_sel the selections; with no row listed every
// workgroup leaves at once.  With rows: a tile workgroup publishes its keys (agent-scope fence: the selections run on
// other XCDs) and counts itself in sync[0]; a selection waits for all n_tile of them.  Workgroups are dispatched in
// index order and the tiles wait for nobody, so the wait cannot starve them; the last selection to finish clears the two
// counters for the next launch on the same prepared state.  (The fences make the rare path slower than two launches;
// launches with a host-known count -- refsize > 256, wc_newref_exact_dev -- keep the two kernels.)
template <bool SEQ>
__global__ __launch_bounds__(256) void k_exact_dev(FinishArgs a, const int *__restrict__ rows,
                                                   const int *__restrict__ n_rows_dev, int *__restrict__ sync,
                                                   unsigned long long *__restrict__ scratch, int64_t Bpad, int cap,
                                                   int ctiles, int rgroups, int n_sel) {
    constexpr int LDS = EXACT_TILE_LDS > EXACT_SELECT_LDS ? EXACT_TILE_LDS : EXACT_SELECT_LDS;
    __shared__ __attribute__((aligned(16))) char smem[LDS];
    const int count = *n_rows_dev;
    if (count <= 0) return;
    // (the grid is small -- EXD_TILE_WGS + EXD_SEL_WGS workgroups that loop over the tiles / rows: an empty launch costs
    //  what its workgroups cost to dispatch, and this launch is empty in every normal pass)
    const int tid = threadIdx.x, n_tile = (int)gridDim.x - n_sel, id = (int)blockIdx.x;
    if (id < n_tile) {
        for (int t = id; t < ctiles * rgroups; t += n_tile) {
            wc_sync();
            exact_tile_body<SEQ>(a, rows, count > cap ? cap : count, 0, scratch, Bpad, t % ctiles, t / ctiles, rgroups, smem);
        }
        __threadfence();                               // this workgroup's keys are visible to the other XCDs ...
        wc_sync();
        if (tid == 0) atomicAdd(&sync[0], 1);          // ... before it counts itself in
        return;
    }
    if (tid == 0) {
        while (__hip_atomic_load(&sync[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n_tile) __builtin_amdgcn_s_sleep(8);
        __threadfence();                               // (acquire: the tiles' keys)
    }
    wc_sync();
    for (int bx = id - n_tile; bx < cap; bx += n_sel) {
        wc_sync();
        exact_select_body(a, rows, count, 0, scratch, Bpad, cap, bx, n_sel, bx < n_sel, smem);
    }
    wc_sync();
    if (tid == 0 && atomicAdd(&sync[1], 1) == n_sel - 1) {
        atomicExch(&sync[0], 0);
        atomicExch(&sync[1], 0);
    }
}

// refsize above LIST_CAP / 4 (the candidate lists are sized for refsize <= 256): every row of the
// range takes the exact path.
__global__ void k_all_exact(FinishArgs a) {
    const int64_t row = a.row_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.row_end) return;
    a.fb_rows[row - a.row_begin] = (int)row;
    a.row_stat[row] = -1;
    if (row == a.row_begin) *a.fb_count = (int)(a.row_end - a.row_begin);
}

// Multi-GPU exchange helpers: pack / merge per-row candidate lists.  The exchange format is (ordered key << 32 |
// plain row number): the export clears the slack code above the row number (`keep` = the row number's bits; all
// ones: the entries as they are), the import puts the importing context's own word of that row back -- every rank
// prepares the whole matrix and so holds the whole table.
__global__ __launch_bounds__(64) void k_export_lists(const int *__restrict__ cnt,
                                                     const unsigned long long *__restrict__ list, int cap,
                                                     int64_t row_begin, int dst_cap, int *__restrict__ dst_cnt,
                                                     unsigned long long *__restrict__ dst_list, unsigned int keep) {
    const int64_t r = blockIdx.x, row = row_begin + r;
    const int c = cnt[row];
    const int n = c < dst_cap ? c : dst_cap;
    const unsigned long long keep64 = 0xFFFFFFFF00000000ull | keep;
    for (int t = threadIdx.x; t < n; t += 64) dst_list[r * dst_cap + t] = list[row * cap + t] & keep64;
    if (threadIdx.x == 0) dst_cnt[r] = c;  // the true count: > dst_cap tells the owner entries were lost
}

__global__ __launch_bounds__(64) void k_import_lists(int *__restrict__ cnt, unsigned long long *__restrict__ list,
                                                     int cap, int64_t row_begin, int src_cap,
                                                     const int *__restrict__ src_cnt,
                                                     const unsigned long long *__restrict__ src_list,
                                                     const unsigned int *__restrict__ cand_word,
                                                     unsigned int index_mask, unsigned int n_words) {
    const int64_t r = blockIdx.x, row = row_begin + r;
    const int c = src_cnt[r];
    const int base = cnt[row];
    if (c > src_cap || base > cap) {
        wc_sync();
        if (threadIdx.x == 0) cnt[row] = cap + 1;  // lost entries: the row takes the exact path
        return;
    }
    for (int t = threadIdx.x; t < c; t += 64)
        if (base + t < cap) {
            const unsigned long long e = src_list[r * src_cap + t];
            const unsigned int j = (unsigned int)e & index_mask;
            list[row * cap + base + t] = (e & 0xFFFFFFFF00000000ull) | cand_word[j < n_words ? j : 0u];
        }
    wc_sync();
    if (threadIdx.x == 0) cnt[row] = base + c;
}

// ----------------------------------------------------------------- host side ----
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

void build_pairwise_leaves(int n, int off, std::vector<int2> &prog) {
    if (n <= 128) {
        prog.push_back(make_int2(off + n, 0));
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    build_pairwise_leaves(n2, off, prog);
    build_pairwise_leaves(n - n2, off + n2, prog);
    prog.back().y += 1;
}

int build_tiles(NewrefState &st, int64_t row_begin, int64_t row_end, int rank, int ranks,
                std::vector<int4> &tiles) {
    const int nb = (int)(st.bins_pad / TB);
    const int ib = (int)(row_begin / TB), ie = (int)((row_end + TB - 1) / TB);
    auto chrom_at = [&](int64_t row) {
        if (row >= st.n_bins) row = st.n_bins - 1;
        int c = 0;
        while (c + 1 < st.n_chrom && row >= st.chrom_off[c + 1]) ++c;
        return c;
    };
    std::vector<int> clo(nb), chi(nb);
    for (int b = 0; b < nb; ++b) {
        clo[b] = chrom_at((int64_t)b * TB);
        chi[b] = chrom_at((int64_t)b * TB + TB - 1);
    }
    // Order: 8x8 super-tiles (8 row panels x 8 column panels).  An XCD runs 64 workgroups
    // at a time over a contiguous stretch of this list, i.e. one super-tile: its 64 tiles
    // share 16 operand panels in that XCD's L2 instead of streaming 64 different ones.
    // Ranks are dealt whole super-tiles when there are plenty, single tiles otherwise.
    constexpr int ST = 8;
    const int64_t n_super = (int64_t)((ie - ib + ST - 1) / ST) * ((nb + ST - 1) / ST);
    const bool deal_super = n_super >= 32ll * ranks;
    int64_t serial = 0, super_serial = -1;
    for (int I0 = ib; I0 < ie; I0 += ST)
        for (int J0 = 0; J0 < nb; J0 += ST) {
            ++super_serial;
            for (int I = I0; I < std::min(I0 + ST, ie); ++I)
                for (int J = J0; J < std::min(J0 + ST, nb); ++J) {
                    int roles;
                    bool in = J >= ib && J < ie;
                    if (in) {
                        if (J < I) continue;
                        roles = (J == I) ? ROLE_COLS : (ROLE_ROWS | ROLE_COLS);
                    } else {
                        roles = ROLE_ROWS;
                    }
                    // a tile whose rows and columns all sit on one chromosome has no candidates
                    if (clo[I] == chi[I] && clo[J] == chi[J] && clo[I] == clo[J]) continue;
                    if (((deal_super ? super_serial : serial++) % ranks) != rank) continue;
                    tiles.push_back(make_int4(I, J, roles, 0));
                }
        }
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_newref_prepare_dev(wc_ctx *ctx, void *stream_, const double *corrected, int64_t n_bins,
                          int64_t n_samples, const int64_t *chrom_bins_host, int n_chrom, int k,
                          int sum_order) {
    WC_CHECK(ctx && corrected && chrom_bins_host, WC_E_ARG, "newref: NULL argument");
    WC_CHECK(n_bins > 0 && n_samples > 0 && k > 0, WC_E_ARG, "newref: empty problem");
    WC_CHECK(n_chrom > 0 && n_chrom <= WC_MAX_CHROM, WC_E_ARG, "newref: n_chrom out of range");
    WC_CHECK(n_samples <= 8192, WC_E_LIMIT, "newref: more than 8192 samples not supported");
    WC_CHECK(k <= K_MAX, WC_E_LIMIT, "newref: refsize above %d not supported", K_MAX);
    WC_CHECK(n_bins < (1ll << 31) - 256, WC_E_LIMIT, "newref: too many bins");
    WC_CHECK(n_bins * n_samples < (1ll << 32), WC_E_LIMIT, "newref: more than 2^32 matrix elements not supported");
    WC_CHECK(sum_order == WC_SUM_PAIRWISE || sum_order == WC_SUM_SEQUENTIAL, WC_E_ARG, "newref: bad sum_order");
    hipStream_t stream = (hipStream_t)stream_;
    WC_HIP(hipSetDevice(ctx->device));
    NewrefState &st = ctx->nr;
    st.prepared = false;
    st.n_bins = n_bins;
    st.n_samples = n_samples;
    st.n_chrom = n_chrom;
    st.k = k;
    st.corrected = corrected;
    st.sum_order = sum_order;
    st.exact_only = k > LIST_CAP / 4;      // the lists hold ~4 k candidates per row: beyond 256 every row is scanned exactly
    st.chrom_off[0] = 0;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_bins_host[c] >= 0, WC_E_ARG, "newref: negative chromosome size");
        st.chrom_off[c + 1] = st.chrom_off[c] + chrom_bins_host[c];
    }
    WC_CHECK(st.chrom_off[n_chrom] == n_bins, WC_E_ARG, "newref: chromosome sizes sum to %lld, expected %lld",
             (long long)st.chrom_off[n_chrom], (long long)n_bins);
    st.bins_pad = round_up(n_bins, TB);
    {
        // a list entry's candidate word: the row number in its low index_bits bits, the candidate's slack as a
        // code of 32 - index_bits bits above it (slack_encode).  At least 17 index bits: 8 exponent + 7 mantissa
        // bits of slack up to 131 072 padded rows, fewer mantissa bits beyond, exponent only at 2^24 rows; more
        // rows than that (lists of 137 GB) have no fast path.
        int need = 1;
        while (need < 31 && ((st.bins_pad - 1) >> need) != 0) ++need;
        if (need > 24) st.exact_only = true;
        WC_CHECK(st.index_bits_req == 0 || st.exact_only || st.index_bits_req >= need, WC_E_ARG,
                 "newref: %d index bits requested, %lld padded rows need %d", st.index_bits_req,
                 (long long)st.bins_pad, need);
        st.index_bits = st.index_bits_req ? st.index_bits_req : std::min(24, std::max(17, need));
    }
    st.k_pad16 = round_up(n_samples, 64);
    st.cap = LIST_CAP;
    st.expect = LIST_CAP * 3 / 8;     // 384: k = 100 is 4 sigma of the sampled order statistic away, the cap 6
    // relative half-width of the key error interval: the float32 accumulation chain, doubled because
    // nothing is assumed about the rounding inside the matrix cores' dot products beyond 2^-23 per
    // term.  The float16 representation error is charged per row (k_convert, tau).
    const double chain = (double)(n_samples + 16) * 5.9604644775390625e-08;
    st.beta = (float)(2.0 * chain * 1.001);
    st.tau = 2.44140625e-04;      // 2^-12: round-to-nearest float16 leaves |a - h| ~ 1.9e-4 |a| (rms)
    int64_t M = round_up((n_bins + 13) / 14, TB);
    if (M < 512) M = 512;
    if (M > MAX_SAMPLE_COLS) M = MAX_SAMPLE_COLS;
    if (M > st.bins_pad) M = st.bins_pad;
    st.n_sample_cols = M;  // padded count; real sample rows = min(M, n_bins)

    int rc;
    if ((rc = st.col_mean.reserve(sizeof(double) * 3 * n_samples))) return rc;
    // padded float64 image for the pair engine's gathers (32-bit byte offsets: below 4 GB; the
    // target row and two chunk slabs per wave must fit the LDS: up to 2048 samples)
    st.s_pad = round_up(n_samples, 16);
    st.x64_pad = n_samples <= 2048 && st.bins_pad * st.s_pad * 8 < (1ll << 32);
    if (st.x64_pad && (rc = st.x64.reserve(sizeof(double) * st.bins_pad * st.s_pad))) return rc;
    if ((rc = st.m2.reserve(sizeof(float) * 4))) return rc;
    if ((rc = st.norm_lo.reserve(sizeof(float) * st.bins_pad))) return rc;
    if ((rc = st.norm_hi.reserve(sizeof(float) * st.bins_pad))) return rc;
    if ((rc = st.cand_word.reserve(sizeof(unsigned int) * st.bins_pad))) return rc;
    if ((rc = st.chrom_of_row.reserve(sizeof(int) * st.bins_pad))) return rc;
    if ((rc = st.chrom_range.reserve(sizeof(int2) * st.bins_pad))) return rc;
    if ((rc = st.chrom_off_dev.reserve(sizeof(int64_t) * (WC_MAX_CHROM + 1)))) return rc;
    if ((rc = st.sample_rows.reserve(sizeof(int) * M))) return rc;
    if ((rc = st.sample_slot.reserve(sizeof(int) * st.bins_pad))) return rc;
    if ((rc = st.a16.reserve(sizeof(unsigned short) * st.bins_pad * st.k_pad16))) return rc;
    if ((rc = st.s16.reserve(sizeof(unsigned short) * M * st.k_pad16))) return rc;
    if ((rc = st.s_norm_lo.reserve(sizeof(float) * M))) return rc;
    if ((rc = st.s_chrom.reserve(sizeof(int) * M))) return rc;
    if ((rc = st.s_range.reserve(sizeof(int2) * M))) return rc;
    if ((rc = st.keys1.reserve(sizeof(unsigned short) * st.bins_pad * M))) return rc;
    if ((rc = st.thr.reserve(sizeof(float) * st.bins_pad))) return rc;
    if ((rc = st.cnt.reserve(sizeof(int) * st.bins_pad))) return rc;
    if ((rc = st.list.reserve(sizeof(uint64_t) * st.bins_pad * st.cap))) return rc;
    if ((rc = st.fb_rows.reserve(sizeof(int) * st.bins_pad))) return rc;
    if ((rc = st.fb_count.reserve(sizeof(int) * 4))) return rc;
    if ((rc = st.stats.reserve(sizeof(int) * st.bins_pad))) return rc;

    {
        std::vector<int64_t> ckey(st.chrom_off, st.chrom_off + n_chrom + 1);
        if (ckey != st.chrom_key) {     // the device copy is uploaded once per layout
            WC_HIP(hipMemcpyAsync(st.chrom_off_dev.p, st.chrom_off, sizeof(int64_t) * (n_chrom + 1),
                                  hipMemcpyHostToDevice, stream));
            WC_HIP(hipStreamSynchronize(stream));
            st.chrom_key = ckey;
        }
    }
    if (st.pw_for != n_samples) {
        // numpy's pairwise split tree over n_samples, flattened: leaves in order with the
        // number of pending "add the two top partial sums" steps after each
        std::vector<int2> prog;
        build_pairwise_leaves((int)n_samples, 0, prog);
        if ((rc = st.pw_prog.reserve(sizeof(int2) * prog.size()))) return rc;
        WC_HIP(hipMemcpyAsync(st.pw_prog.p, prog.data(), sizeof(int2) * prog.size(), hipMemcpyHostToDevice, stream));
        WC_HIP(hipStreamSynchronize(stream));
        st.pw_leaves = (int)prog.size();
        st.pw_for = n_samples;
    }
    // fixed pseudo-random sample of rows (partial Fisher-Yates on a 64-bit LCG), ascending;
    // depends on (n_bins, M) only, so it is uploaded once per layout
    std::vector<int64_t> skey = {n_bins, M};
    if (skey != st.sample_key) {
        int64_t real = std::min<int64_t>(M, n_bins);
        std::vector<int> perm(n_bins);
        for (int64_t i = 0; i < n_bins; ++i) perm[i] = (int)i;
        uint64_t s = 0x9E3779B97F4A7C15ull;
        for (int64_t i = 0; i < real; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            int64_t pick = i + (int64_t)((s >> 33) % (uint64_t)(n_bins - i));
            std::swap(perm[i], perm[pick]);
        }
        std::sort(perm.begin(), perm.begin() + real);
        std::vector<int> slot((size_t)n_bins, -1);   // row -> sample slot
        for (int64_t i = 0; i < real; ++i) slot[perm[i]] = (int)i;
        WC_HIP(hipMemcpyAsync(st.sample_rows.p, perm.data(), sizeof(int) * real, hipMemcpyHostToDevice, stream));
        WC_HIP(hipMemcpyAsync(st.sample_slot.p, slot.data(), sizeof(int) * n_bins, hipMemcpyHostToDevice, stream));
        WC_HIP(hipStreamSynchronize(stream));  // perm and slot go out of scope
        st.sample_key = skey;
        st.tiles0_key.clear();
        st.tiles1_key.clear();
    }

    double *mean2 = st.col_mean.as<double>();
    if (n_samples <= FUSED_MAX_SAMPLES) {
        // one launch.  The smallest norm of a clamped row lives in one of two slots, m2[1] and m2[2]: the fused kernel
        // takes minima into one from its first workgroup on, so it cannot reset that one itself; it resets the OTHER,
        // which no kernel of this job reads, for the prepare after this one.  bad_spare_clean says that it has; a
        // prepare that does not find it (the first of a context) sets its slot from the host.
        const int slot = 1 - st.bad_slot;
        int *bad = st.m2.as<int>() + 1 + slot, *spare = st.m2.as<int>() + 1 + st.bad_slot;
        if (!st.bad_spare_clean) WC_HIP(hipMemsetD32Async((hipDeviceptr_t)bad, 0x7F800000, 1, stream));
        // the sampled rows: every fourth of the 128 strided rows k_col_centre takes (a row that is none of those is
        // none of these); with fewer than 128 bins, FUSED_CENTRE_ROWS of them evenly
        const int64_t n_crows = std::min<int64_t>(n_bins, FUSED_CENTRE_ROWS);
        const int64_t crow_step = n_bins >= 128 ? (128 / FUSED_CENTRE_ROWS) * (n_bins / 128) : n_bins / n_crows;
        hipLaunchKernelGGL((k_prepare_fused<FUSED_CENTRE_ROWS, FUSED_THREADS>),
                           dim3((unsigned)(st.bins_pad / (FUSED_THREADS / 32))), dim3(FUSED_THREADS),
                           0, stream, corrected, n_bins, n_samples, st.bins_pad, (const double *)nullptr,
                           (double)st.beta, st.tau, st.chrom_off_dev.as<int64_t>(), n_chrom,
                           st.a16.as<unsigned short>(), st.k_pad16, st.norm_lo.as<float>(), st.norm_hi.as<float>(),
                           st.chrom_of_row.as<int>(), st.chrom_range.as<int2>(),
                           (const int *)st.sample_slot.as<int>(), st.s16.as<unsigned short>(),
                           st.s_norm_lo.as<float>(), st.s_chrom.as<int>(), st.s_range.as<int2>(), st.thr.as<float>(),
                           st.cnt.as<int>(), st.stats.as<int>(), st.x64_pad ? st.x64.as<double>() : (double *)nullptr,
                           st.s_pad, st.m2.as<float>(), bad, st.fb_count.as<int>(), 4,
                           st.cand_word.as<unsigned int>(), st.index_bits, mean2, n_crows, crow_step, spare);
        WC_HIP(hipGetLastError());
        st.bad_slot = slot;
        st.bad_spare_clean = true;
    } else {
        // more samples than the fused kernel holds per workgroup: the centres first, in a launch of their own
        // (k_col_centre resets the slot in use itself; the spare one stays as it is)
        int64_t n_rows = std::min<int64_t>(n_bins, 128);
        int64_t row_step = n_bins / n_rows;
        int *bad = st.m2.as<int>() + 1 + st.bad_slot;
        hipLaunchKernelGGL(k_col_centre, dim3((unsigned)((n_samples + 63) / 64)), dim3(1024), 0, stream, corrected,
                           n_bins, n_samples, n_rows, row_step, mean2, bad);
        hipLaunchKernelGGL(k_convert, dim3((unsigned)(st.bins_pad / 8)), dim3(256), 0, stream, corrected, n_bins,
                           n_samples, st.bins_pad, (const double *)mean2, (double)st.beta, st.tau,
                           st.chrom_off_dev.as<int64_t>(), n_chrom, st.a16.as<unsigned short>(),
                           st.k_pad16, st.norm_lo.as<float>(), st.norm_hi.as<float>(), st.chrom_of_row.as<int>(),
                           st.chrom_range.as<int2>(), (const int *)st.sample_slot.as<int>(),
                           st.s16.as<unsigned short>(), st.s_norm_lo.as<float>(), st.s_chrom.as<int>(),
                           st.s_range.as<int2>(), st.thr.as<float>(), st.cnt.as<int>(), st.stats.as<int>(),
                           st.x64_pad ? st.x64.as<double>() : (double *)nullptr, st.s_pad, st.m2.as<float>(),
                           bad, st.fb_count.as<int>(), 4, st.cand_word.as<unsigned int>(), st.index_bits);
    }
    st.fb_dirty = false;
    if (M > n_bins)
        hipLaunchKernelGGL(k_pad_samples, dim3((unsigned)(M - n_bins)), dim3(256), 0, stream, st.k_pad16, n_bins,
                           st.s16.as<unsigned short>(), st.s_norm_lo.as<float>(), st.s_chrom.as<int>(),
                           st.s_range.as<int2>());
    WC_HIP(hipGetLastError());
    st.prepared = true;
    return WC_OK;
}

int wc_newref_thresholds_dev(wc_ctx *ctx, void *stream_, int64_t row_begin, int64_t row_end) {
    WC_CHECK(ctx && ctx->nr.prepared, WC_E_ARG, "newref: prepare has not run");
    NewrefState &st = ctx->nr;
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= st.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_begin == row_end || st.exact_only) return WC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int ib = (int)(row_begin / TB), ie = (int)((row_end + TB - 1) / TB);
    const int mb = (int)(st.n_sample_cols / TB);
    std::vector<int64_t> key = {st.bins_pad, st.n_sample_cols, ib, ie};
    if (key != st.tiles0_key) {
        std::vector<int4> tiles;
        tiles.reserve((size_t)(ie - ib) * mb);
        for (int I = ib; I < ie; ++I)
            for (int J = 0; J < mb; ++J) tiles.push_back(make_int4(I, J, 0, 0));
        int rc;
        if ((rc = st.tiles0.reserve(sizeof(int4) * tiles.size()))) return rc;
        WC_HIP(hipMemcpyAsync(st.tiles0.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, stream));
        WC_HIP(hipStreamSynchronize(stream));
        st.tiles0_key = key;
        st.tiles0_n = (int64_t)tiles.size();
    }
    {
        const int ntiles = (int)st.tiles0_n;
        unsigned grid = (unsigned)(((ntiles + 7) / 8) * 8);
        // (LDS-DMA staging was tried here too: 0.554 vs 0.518 ms at 600 x 50 kb -- this kernel's time is its
        // 472 MB of key-code stores, not its operand path; EXPERIMENTS.md)
        hipLaunchKernelGGL(k_gram_thr16, dim3(grid), dim3(256), 0, stream,
                           (const unsigned short *)st.a16.as<unsigned short>(),
                           (const unsigned short *)st.s16.as<unsigned short>(), st.k_pad16, (int)(st.k_pad16 / 64),
                           (const float *)st.norm_lo.as<float>(), (const float *)st.s_norm_lo.as<float>(),
                           (const int2 *)st.s_range.as<int2>(), (const int4 *)st.tiles0.as<int4>(), ntiles,
                           st.keys1.as<unsigned int>(), st.n_sample_cols, (const float *)st.m2.as<float>());
    }
    unsigned sg = (unsigned)((row_end - row_begin + 3) / 4);
    {
        const unsigned int *kp = st.keys1.as<unsigned int>();
        const int2 *cr = st.chrom_range.as<int2>();
        const int per_lane = (int)(st.n_sample_cols / 64);
#define WC_SELECT(NV)                                                                                          \
    hipLaunchKernelGGL(k_select_thr<NV>, dim3(sg), dim3(256), 0, stream, kp, st.n_sample_cols,                \
                       (int)st.n_sample_cols, cr, st.n_bins, row_begin, row_end, (int)st.expect, (int)st.cap, \
                       st.thr.as<float>())
        if (per_lane <= 16) WC_SELECT(16);
        else if (per_lane <= 32) WC_SELECT(32);
        else WC_SELECT(64);
#undef WC_SELECT
    }
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int64_t wc_newref_list_capacity(wc_ctx *ctx) { return ctx ? ctx->nr.cap : 0; }

int wc_newref_get_thresholds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, float *out) {
    WC_CHECK(ctx && ctx->nr.prepared && out, WC_E_ARG, "newref: bad argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= ctx->nr.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_end > row_begin)
        WC_HIP(hipMemcpyAsync(out, ctx->nr.thr.as<float>() + row_begin, sizeof(float) * (row_end - row_begin),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WC_OK;
}

int wc_newref_get_bounds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, float *lo_out,
                             float *slack_out) {
    WC_CHECK(ctx && ctx->nr.prepared && lo_out && slack_out, WC_E_ARG, "newref: bad argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= ctx->nr.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_end > row_begin) {
        WC_HIP(hipMemcpyAsync(lo_out, ctx->nr.norm_lo.as<float>() + row_begin, sizeof(float) * (row_end - row_begin),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
        WC_HIP(hipMemcpyAsync(slack_out, ctx->nr.norm_hi.as<float>() + row_begin, sizeof(float) * (row_end - row_begin),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return WC_OK;
}

int wc_newref_set_thresholds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, const float *in) {
    WC_CHECK(ctx && ctx->nr.prepared && in, WC_E_ARG, "newref: bad argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= ctx->nr.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_end > row_begin)
        WC_HIP(hipMemcpyAsync(ctx->nr.thr.as<float>() + row_begin, in, sizeof(float) * (row_end - row_begin),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WC_OK;
}

static int newref_export(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int64_t dst_cap,
                         int32_t *dst_cnt, uint64_t *dst_list, bool raw) {
    WC_CHECK(ctx && ctx->nr.prepared && dst_cnt && dst_list && dst_cap > 0, WC_E_ARG, "newref: bad argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= ctx->nr.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_end == row_begin) return WC_OK;
    NewrefState &st = ctx->nr;
    hipLaunchKernelGGL(k_export_lists, dim3((unsigned)(row_end - row_begin)), dim3(64), 0, (hipStream_t)stream,
                       (const int *)st.cnt.as<int>(), (const unsigned long long *)st.list.as<unsigned long long>(),
                       (int)st.cap, row_begin, (int)dst_cap, dst_cnt, (unsigned long long *)dst_list,
                       raw ? ~0u : (1u << st.index_bits) - 1u);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_newref_export_lists_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int64_t dst_cap,
                               int32_t *dst_cnt, uint64_t *dst_list) {
    return newref_export(ctx, stream, row_begin, row_end, dst_cap, dst_cnt, dst_list, false);
}

int wc_newref_export_raw_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int64_t dst_cap,
                             int32_t *dst_cnt, uint64_t *dst_list) {
    return newref_export(ctx, stream, row_begin, row_end, dst_cap, dst_cnt, dst_list, true);
}

int wc_newref_index_bits(wc_ctx *ctx) { return ctx && ctx->nr.prepared ? ctx->nr.index_bits : 0; }

int wc_newref_set_index_bits(wc_ctx *ctx, int bits) {
    WC_CHECK(ctx, WC_E_ARG, "newref: NULL context");
    WC_CHECK(bits == 0 || (bits >= 1 && bits <= 24), WC_E_ARG, "newref: index bits must be 0 (automatic) or 1..24");
    ctx->nr.index_bits_req = bits;      // the next prepare checks it against the problem's rows
    return WC_OK;
}

int wc_slack_code_host(const float *slack, int64_t n, int code_bits, uint32_t *code_out, float *decoded_out) {
    WC_CHECK(slack && code_out && decoded_out && n >= 0, WC_E_ARG, "slack code: bad argument");
    WC_CHECK(code_bits >= 1 && code_bits <= 31, WC_E_ARG, "slack code: 1..31 code bits");
    for (int64_t i = 0; i < n; ++i) {
        WC_CHECK(!(slack[i] < 0.f), WC_E_ARG, "slack code: negative value at %lld", (long long)i);
        code_out[i] = slack_encode(slack[i], code_bits);
        decoded_out[i] = slack_decode(code_out[i], code_bits);
    }
    return WC_OK;
}

int wc_order_key_host(const uint64_t *key, int64_t n, int shift, uint32_t *image_out, uint32_t *min_hi_out) {
    WC_CHECK(key && image_out && min_hi_out && n >= 0, WC_E_ARG, "order key: bad argument");
    WC_CHECK(shift >= -1 && shift <= 32, WC_E_ARG, "order key: shift -1 (the kernel's) or 0..32");
    const int sh = shift < 0 ? wc::ORDER_KEY_SH : shift;
    uint32_t min_hi = 0xFFFFFFFFu;          // as the kernel: over every key (an entry without a distance has the top word)
    for (int64_t i = 0; i < n; ++i) min_hi = std::min(min_hi, (uint32_t)(key[i] >> 32));
    for (int64_t i = 0; i < n; ++i) image_out[i] = wc::order_key32(key[i], min_hi, sh);
    *min_hi_out = min_hi;
    return WC_OK;
}

int wc_newref_import_lists_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int64_t src_cap,
                               const int32_t *src_cnt, const uint64_t *src_list) {
    WC_CHECK(ctx && ctx->nr.prepared && src_cnt && src_list && src_cap > 0, WC_E_ARG, "newref: bad argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= ctx->nr.n_bins, WC_E_ARG, "newref: bad row range");
    if (row_end == row_begin) return WC_OK;
    NewrefState &st = ctx->nr;
    hipLaunchKernelGGL(k_import_lists, dim3((unsigned)(row_end - row_begin)), dim3(64), 0, (hipStream_t)stream,
                       st.cnt.as<int>(), st.list.as<unsigned long long>(), (int)st.cap, row_begin, (int)src_cap,
                       src_cnt, (const unsigned long long *)src_list,
                       (const unsigned int *)st.cand_word.as<unsigned int>(), (1u << st.index_bits) - 1u,
                       (unsigned int)st.bins_pad);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_newref_collect_dev(wc_ctx *ctx, void *stream_, int64_t row_begin, int64_t row_end, int tile_rank,
                          int tile_ranks) {
    WC_CHECK(ctx && ctx->nr.prepared, WC_E_ARG, "newref: prepare has not run");
    NewrefState &st = ctx->nr;
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= st.n_bins, WC_E_ARG, "newref: bad row range");
    WC_CHECK(tile_ranks >= 1 && tile_rank >= 0 && tile_rank < tile_ranks, WC_E_ARG, "newref: bad tile rank");
    if (row_begin == row_end || st.exact_only) return WC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<int64_t> key = {st.n_bins, row_begin, row_end, tile_rank, tile_ranks};
    for (int c = 0; c <= st.n_chrom; ++c) key.push_back(st.chrom_off[c]);
    if (key != st.tiles1_key) {
        std::vector<int4> tiles;
        build_tiles(st, row_begin, row_end, tile_rank, tile_ranks, tiles);
        int rc;
        if ((rc = st.tiles.reserve(sizeof(int4) * std::max<size_t>(tiles.size(), 1)))) return rc;
        if (!tiles.empty()) {
            WC_HIP(hipMemcpyAsync(st.tiles.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, stream));
            WC_HIP(hipStreamSynchronize(stream));
        }
        st.tiles1_key = key;
        st.tiles1_n = (int64_t)tiles.size();
    }
    ctx->last_stats[2] = st.tiles1_n;
    ctx->last_stats[3] = st.n_sample_cols;
    if (st.tiles1_n == 0) return WC_OK;
    GramArgs g{};
    // the float16 image the threshold estimate used (blocked: a16_index), 32 samples per slab
    g.P = g.Q = st.a16.as<float>();
    g.ld = st.k_pad16 / 2;
    g.m2 = st.m2.as<float>();
    g.nslab32 = (int)((st.n_samples + 31) / 32);
    g.last_steps32 = (int)(((st.n_samples - (int64_t)(g.nslab32 - 1) * 32) + 15) / 16);
    g.nbP = g.nbQ = st.norm_lo.as<float>();
    g.cwP = g.cwQ = st.cand_word.as<unsigned int>();
    g.range = st.chrom_range.as<int2>();
    g.tiles = st.tiles.as<int4>();
    g.ntiles = (int)st.tiles1_n;
    g.thr = st.thr.as<float>();
    g.cnt = st.cnt.as<int>();
    g.list = st.list.as<unsigned long long>();
    g.cap = (int)st.cap;
    const unsigned grid = (unsigned)(((g.ntiles + 7) / 8) * 8);
    hipLaunchKernelGGL(k_gram_glds, dim3(grid), dim3(256), 0, stream, g);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

// the arguments every kernel of stage D shares
static void finish_args(NewrefState &st, int64_t row_begin, int64_t row_end, int32_t *idx_out, double *dist_out,
                        FinishArgs &a) {
    a.X = st.corrected;
    a.B = st.n_bins;
    a.S = st.n_samples;
    a.norm_lo = st.norm_lo.as<float>();
    a.norm_hi = st.norm_hi.as<float>();
    a.thr = st.thr.as<float>();
    a.cnt = st.cnt.as<int>();
    a.list = st.list.as<unsigned long long>();
    a.index_mask = (1u << st.index_bits) - 1u;
    a.cap = (int)st.cap;
    a.k = st.k;
    a.beta = (double)st.beta;
    a.chrom_of_row = st.chrom_of_row.as<int>();
    a.chrom_off = st.chrom_off_dev.as<int64_t>();
    a.chrom_range = st.chrom_range.as<int2>();
    a.row_begin = row_begin;
    a.row_end = row_end;
    a.idx_out = idx_out;
    a.dist_out = dist_out;
    a.fb_rows = st.fb_rows.as<int>();
    a.fb_count = st.fb_count.as<int>();
    a.bad_norm = st.m2.as<float>() + 1 + st.bad_slot;
    a.row_stat = st.stats.as<int>();
    a.sum_order = st.sum_order;
    a.lone_mask = 0ull;
    if (st.sum_order == WC_SUM_SEQUENTIAL)
        for (int c = 0; c < st.n_chrom; ++c)
            if (st.chrom_off[c] <= 1 && st.n_bins - st.chrom_off[c + 1] <= 1) a.lone_mask |= 1ull << c;
    a.xs_in_lds = st.n_samples <= 2048;
    a.pw_prog = st.pw_prog.as<int2>();
    a.pw_leaves = st.pw_leaves;
}

// The exact path over the rows listed in fb_rows: `n_host` < 0 -- the count is on the device (the rows the fast
// path handed over; ONE launch pair sized for EX_CAP rows, no read-back); otherwise the host knows it and loops
// over bands of EX_CAP rows.
static int launch_exact(NewrefState &st, hipStream_t stream, const FinishArgs &a, int64_t n_host) {
    int rc;
    // scratch: one row of keys per target of a launch pair.  Count on the device (the normal pass, usually no row at
    // all): a launch pair for EX_DEV_CAP targets plus one row per select workgroup for the rows beyond (16 KB per bin
    // in all: 0.23 GB at 50 kb bins); count on the host: EX_CAP targets per pair, no second half.
    const int cap = n_host < 0 ? EX_DEV_CAP : EX_CAP;
    if ((rc = st.fb_scratch.reserve(sizeof(uint64_t) * (n_host < 0 ? 2 : 1) * cap * st.bins_pad))) return rc;
    const bool seq = st.sum_order == WC_SUM_SEQUENTIAL || st.n_samples < 8;
    const int edge = seq ? 64 : 32;                                  // targets / candidates per tile
    const unsigned ctiles = (unsigned)((st.n_bins + edge - 1) / edge);
    unsigned long long *scratch = st.fb_scratch.as<unsigned long long>();
    const int *rows = st.fb_rows.as<int>();
    if (n_host < 0) {
        // count on the device: one launch (k_exact_dev); fb_count[1..2] are its two counters (zero between launches)
        const int rgroups = 4;                         // row groups in flight per candidate tile
        int *sync = st.fb_count.as<int>() + 1;
        constexpr int EXD_TILE_WGS = 192, EXD_SEL_WGS = 64;
        const int n_tile = (int)std::min<int64_t>((int64_t)ctiles * rgroups, EXD_TILE_WGS);
        const unsigned grid = (unsigned)(n_tile + EXD_SEL_WGS);
        if (seq) hipLaunchKernelGGL((k_exact_dev<true>), dim3(grid), dim3(256), 0, stream, a, rows,
                                    (const int *)st.fb_count.as<int>(), sync, scratch, st.bins_pad, cap, (int)ctiles, rgroups, EXD_SEL_WGS);
        else hipLaunchKernelGGL((k_exact_dev<false>), dim3(grid), dim3(256), 0, stream, a, rows,
                                (const int *)st.fb_count.as<int>(), sync, scratch, st.bins_pad, cap, (int)ctiles, rgroups, EXD_SEL_WGS);
        return WC_OK;
    }
    for (int64_t first = 0; first < n_host; first += cap) {
        const int64_t nf = std::min<int64_t>(cap, n_host - first);
        const unsigned rgroups = (unsigned)((nf + edge - 1) / edge);
        if (seq) hipLaunchKernelGGL((k_exact_tile<true>), dim3(ctiles, rgroups), dim3(256), 0, stream, a, rows,
                                    (const int *)nullptr, (int)n_host, (int)first, scratch, st.bins_pad, cap);
        else hipLaunchKernelGGL((k_exact_tile<false>), dim3(ctiles, rgroups), dim3(256), 0, stream, a, rows,
                                (const int *)nullptr, (int)n_host, (int)first, scratch, st.bins_pad, cap);
        hipLaunchKernelGGL(k_exact_select, dim3((unsigned)nf), dim3(256), 0, stream, a, rows, (int)n_host, (int)first,
                           scratch, st.bins_pad, cap);
    }
    return WC_OK;
}

// stage D in parts: `which` bit 0 = the per-row fast path (k_pick + k_rescore; k_finish beyond 2048 samples),
// bit 1 = the exact path for the rows it handed over (two idle launches when there are none), bit 2 = k_pick
// alone, bit 3 = k_rescore alone
static int newref_finish_part(wc_ctx *ctx, void *stream_, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                              double *dist_out, int which) {
    WC_CHECK(ctx && ctx->nr.prepared, WC_E_ARG, "newref: prepare has not run");
    NewrefState &st = ctx->nr;
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= st.n_bins, WC_E_ARG, "newref: bad row range");
    WC_CHECK(idx_out && dist_out, WC_E_ARG, "newref: NULL output");
    if (row_begin == row_end) return WC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if (which & 5) {
        // the counter of exact rows: k_convert zeroed it for the first pick of a prepared job; a second
        // finish on the same prepared state starts from a memset
        if (st.fb_dirty) WC_HIP(hipMemsetAsync(st.fb_count.p, 0, sizeof(int) * 4, stream));
        st.fb_dirty = true;
    }
    FinishArgs a{};
    finish_args(st, row_begin, row_end, idx_out, dist_out, a);
    // pair engine: workgroups of k + margin threads (whole waves); refsize beyond PS_MAX - 28 takes several trips
    const int ps = (int)std::max<int64_t>(128, std::min<int64_t>(PS_MAX, round_up(st.k + 28, 64)));
    const bool pair_engine = st.x64_pad && !st.exact_only;
    if ((which & 12) && !pair_engine) which = (which & ~12) | ((which & 4) ? 1 : 0);   // no halves outside the pair engine: all of it in the first call
    const bool seq = st.sum_order == WC_SUM_SEQUENTIAL || st.n_samples < 8;
    const unsigned rows = (unsigned)(row_end - row_begin);
    if ((which & 1) && st.exact_only) {
        hipLaunchKernelGGL(k_all_exact, dim3((rows + 255) / 256), dim3(256), 0, stream, a);
    } else if ((which & 13) && pair_engine) {
        if ((rc = st.pairs.reserve(sizeof(int) * st.bins_pad * RMAX))) return rc;
        PickArgs p{a, st.pairs.as<int>(), ps};
        if (which & 5) hipLaunchKernelGGL(k_pick, dim3((rows + 3) / 4), dim3(256), 0, stream, p);
        // wave slabs; after the sums the same memory holds dk / sd / jv / sj / rk of the counting order (rescore_order).
        // Chunk staging: LDS-DMA for the pairwise order (100 samples x 250 kb: 0.099 vs 0.131 ms, no staging
        // registers), registers for the sequential order (0.076 vs 0.083 ms: the DMA of the next chunk can only
        // be issued after this chunk's LDS reads have returned)
        const size_t slabs = sizeof(double) * (size_t)(ps / 64) * SLAB_DOUBLES;
        const size_t order = (sizeof(unsigned long long) + sizeof(int)) * (2 * RMAX + 4) + sizeof(uint32_t) * (RMAX + 2) + ORDER_OVERREAD;
        const size_t dyn = sizeof(double) * st.s_pad + std::max(slabs, order);
        if (!(which & 9)) {
        } else if (seq) hipLaunchKernelGGL((k_rescore<true, false>), dim3(rows), dim3(ps), dyn, stream, p,
                                           (const double *)st.x64.as<double>(), (int)st.s_pad);
        else hipLaunchKernelGGL((k_rescore<false, true>), dim3(rows), dim3(ps), dyn, stream, p,
                                (const double *)st.x64.as<double>(), (int)st.s_pad);
    } else if (which & 1) {
        // more than 2048 samples (the pair engine's LDS holds the target row and its chunk slabs up to there):
        // one 128-thread workgroup per row does selection, re-score and order
        const size_t dyn = a.xs_in_lds ? sizeof(double) * st.n_samples : 0;
        if (seq) hipLaunchKernelGGL((k_finish<true, 128>), dim3(rows), dim3(128), dyn, stream, a);
        else hipLaunchKernelGGL((k_finish<false, 128>), dim3(rows), dim3(128), dyn, stream, a);
    }
    if (which & 2) {
        if (st.exact_only) rc = launch_exact(st, stream, a, (int64_t)rows);
        else rc = launch_exact(st, stream, a, -1);
        if (rc) return rc;
    }
    WC_HIP(hipGetLastError());
    return WC_OK;
}

// The exact path for EVERY row of [row_begin, row_end) on a prepared job (wc_newref_prepare_dev): float64
// distances to all candidates in numpy's order, stable selection -- no matrix cores, no bounds, no lists.
// The full-size tests hold the fast path against it row by row; it is also what refsize > 256 runs.
int wc_newref_exact_dev(wc_ctx *ctx, void *stream_, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                        double *dist_out) {
    WC_CHECK(ctx && ctx->nr.prepared, WC_E_ARG, "newref: prepare has not run");
    NewrefState &st = ctx->nr;
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= st.n_bins, WC_E_ARG, "newref: bad row range");
    WC_CHECK(idx_out && dist_out, WC_E_ARG, "newref: NULL output");
    if (row_begin == row_end) return WC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    FinishArgs a{};
    finish_args(st, row_begin, row_end, idx_out, dist_out, a);
    const unsigned rows = (unsigned)(row_end - row_begin);
    hipLaunchKernelGGL(k_all_exact, dim3((rows + 255) / 256), dim3(256), 0, stream, a);
    st.fb_dirty = true;
    const int rc = launch_exact(st, stream, a, (int64_t)rows);
    if (rc) return rc;
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_newref_finish_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                         double *dist_out) {
    return newref_finish_part(ctx, stream, row_begin, row_end, idx_out, dist_out, 3);
}

int wc_newref_rescore_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                          double *dist_out) {
    return newref_finish_part(ctx, stream, row_begin, row_end, idx_out, dist_out, 1);
}

int wc_newref_fallback_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                           double *dist_out) {
    return newref_finish_part(ctx, stream, row_begin, row_end, idx_out, dist_out, 2);
}

int wc_newref_pick_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                       double *dist_out) {
    return newref_finish_part(ctx, stream, row_begin, row_end, idx_out, dist_out, 4);
}

int wc_newref_rescore_pairs_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                                double *dist_out) {
    return newref_finish_part(ctx, stream, row_begin, row_end, idx_out, dist_out, 8);
}

__global__ void k_noop(int *p) {
    if (p && threadIdx.x == 9999) *p = 0;
}

// Launch floor of this box: a chain of `n` dependent empty launches on `stream`, timed with events
// over `reps` repetitions; out[0] = microseconds per chain.  What a series of n tiny kernels costs
// before any of them does work (bench.py prices the one-sample latency path against it).
int wc_launch_floor_us(wc_ctx *ctx, void *stream_, int n, int reps, double *out) {
    WC_CHECK(ctx && out && n > 0 && reps > 0, WC_E_ARG, "launch floor: bad argument");
    WC_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    hipEvent_t e0, e1;
    WC_HIP(hipEventCreate(&e0));
    WC_HIP(hipEventCreate(&e1));
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, stream, (int *)nullptr);
    WC_HIP(hipStreamSynchronize(stream));
    WC_HIP(hipEventRecord(e0, stream));
    for (int r = 0; r < reps; ++r)
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, stream, (int *)nullptr);
    WC_HIP(hipEventRecord(e1, stream));
    WC_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    WC_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    out[0] = 1e3 * (double)ms / (double)reps;
    return WC_OK;
}

static int newref_pass(wc_ctx *ctx, void *stream, const double *corrected, int64_t n_bins, int64_t n_samples,
                       const int64_t *chrom_bins_host, int n_chrom, int k, int sum_order, int64_t row_begin,
                       int64_t row_end, int32_t *idx_out, double *dist_out) {
    int rc = wc_newref_prepare_dev(ctx, stream, corrected, n_bins, n_samples, chrom_bins_host, n_chrom, k,
                                   sum_order);
    if (rc) return rc;
    if ((rc = wc_newref_thresholds_dev(ctx, stream, row_begin, row_end))) return rc;
    if ((rc = wc_newref_collect_dev(ctx, stream, row_begin, row_end, 0, 1))) return rc;
    return wc_newref_finish_dev(ctx, stream, row_begin, row_end, idx_out, dist_out);
}

int wc_get_reference_dev(wc_ctx *ctx, void *stream_, const double *corrected, int64_t n_bins, int64_t n_samples,
                         const int64_t *chrom_bins_host, int n_chrom, int k, int sum_order,
                         int64_t row_begin, int64_t row_end, int32_t *idx_out, double *dist_out) {
    WC_CHECK(ctx && corrected && chrom_bins_host, WC_E_ARG, "newref: NULL argument");
    return newref_pass(ctx, stream_, corrected, n_bins, n_samples, chrom_bins_host, n_chrom, k, sum_order,
                       row_begin, row_end, idx_out, dist_out);
}

int wc_get_reference(wc_ctx *ctx, const double *corrected, int64_t n_bins, int64_t n_samples,
                     const int64_t *chrom_bins, int n_chrom, int k, int sum_order, int64_t row_begin,
                     int64_t row_end, int32_t *idx_out, double *dist_out) {
    WC_CHECK(ctx && corrected && idx_out && dist_out, WC_E_ARG, "getReference: NULL argument");
    WC_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= n_bins, WC_E_ARG, "getReference: bad row range");
    WC_HIP(hipSetDevice(ctx->device));
    int64_t rows = row_end - row_begin;
    int rc;
    if ((rc = ctx->tmp_a.reserve(sizeof(double) * n_bins * n_samples))) return rc;
    if ((rc = ctx->tmp_b.reserve(sizeof(int32_t) * std::max<int64_t>(rows, 1) * k))) return rc;
    if ((rc = ctx->tmp_c.reserve(sizeof(double) * std::max<int64_t>(rows, 1) * k))) return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, corrected, sizeof(double) * n_bins * n_samples, hipMemcpyHostToDevice));
    rc = wc_get_reference_dev(ctx, nullptr, ctx->tmp_a.as<double>(), n_bins, n_samples, chrom_bins, n_chrom, k,
                              sum_order, row_begin, row_end, ctx->tmp_b.as<int32_t>(), ctx->tmp_c.as<double>());
    if (rc) return rc;
    WC_HIP(hipDeviceSynchronize());
    if (rows > 0) {
        WC_HIP(hipMemcpy(idx_out, ctx->tmp_b.p, sizeof(int32_t) * rows * k, hipMemcpyDeviceToHost));
        WC_HIP(hipMemcpy(dist_out, ctx->tmp_c.p, sizeof(double) * rows * k, hipMemcpyDeviceToHost));
    }
    return WC_OK;
}

int wc_newref_stats(wc_ctx *ctx, int64_t out[8]) {
    WC_CHECK(ctx && out, WC_E_ARG, "stats: NULL argument");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    NewrefState &st = ctx->nr;
    if (st.stats.p && st.prepared) {
        WC_HIP(hipSetDevice(ctx->device));
        WC_HIP(hipDeviceSynchronize());
        std::vector<int> rows(st.n_bins);
        WC_HIP(hipMemcpy(rows.data(), st.stats.p, sizeof(int) * st.n_bins, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < st.n_bins; ++r) {
            if (rows[r] >= 0) { out[0] += 1; out[4] += rows[r]; }
            else if (rows[r] == -1) out[1] += 1;
        }
    }
    out[2] = ctx->last_stats[2];
    out[3] = ctx->last_stats[3];
    return WC_OK;
}

}  // extern "C"
