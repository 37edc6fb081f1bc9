// crossval: the held-out z-scores of a healthy cohort, judged on the device.
// Z is [n_samples, row_stride] float64 in the layout wc_test_batch_dev leaves (n_total bins of a row are read), calls and
// n_calls likewise, thr and asdef one double per sample.  A bin is TESTED when z != 0 (+-0.0 is the fill of masked and
// removed bins; NaN is tested), NONFINITE when tested and not finite, else FINITE.
//   k_cx_check    a lane per (sample, call row below n_calls): a row whose chromosome or span lies outside the layout, or
//                 whose three leading doubles are no whole numbers, leaves the smallest such flat row index in the status
//                 word; the host waits for that word and refuses the call before any output is written.
//   k_cx_bins     a lane per bin walks the samples in ascending order: loads are coalesced across bins and the float64
//                 sums {sum z, sum z * z} are sequential by construction.  Every product is rounded before it is added
//                 (__dmul_rn, __dadd_rn: no FMA contraction, whatever the compiler's flags), so a Python loop over
//                 np.float64 is the definition, bit for bit.  The call rows are the same in every lane (scalar loads):
//                 a row covers the bin when the bin's flat index lies in its flat span.
//   k_cx_prefix   a lane per (sample, selected chromosome): the chromosome's tested values t in bin order and
//                 P[0] = 0, P[j + 1] = P[j] + t[j], sequentially (a parallel scan rounds differently and is not the
//                 rule), to a scratch array in global memory -- a chromosome's length is not bounded by LDS.  row_n
//                 receives the number of tested values, or -1 for a row with a nonfinite value (skipped).
//   k_cx_rec      a wave per sample: the row's class counts and its largest and smallest finite z by a wave reduction
//                 (integers, max and min: no order in them), call_bins over the call rows, rows_skipped and win_n from
//                 row_n.
//   k_cx_windows  a workgroup per (sample, length L): lanes stride over the windows a of every selected chromosome,
//                 w = (P[a + L] - P[a]) / sqrt((double)L) (the root comes from the host, correctly rounded), into a
//                 histogram of 130 slots in LDS; hi / lo by a wave reduction.  The workgroup adds its nonzero slots to
//                 the int64 outputs with 64-bit integer atomics: integer counts make the order free.
// The only LDS is k_cx_windows' histogram; its barriers are wc_sync().  No kernel indexes by a call row's or a
// caller's value that the host or k_cx_check has not bounded.
#include <limits.h>

#include "ctx.h"

namespace {

const int CX_T = 256;                   // lanes per workgroup
const int CX_SLOTS = 130;               // win_hist: slot 0 below -16, 1 .. 128 quarter units of [-16, 16), 129 above or NaN
const int CX_MAX_LENGTHS = 16;

struct CxTab {                          // the small tables of a call, checked on the host and uploaded once
    long long status;                   // k_cx_check: the first bad call row, sample * max_calls + row (LLONG_MAX: none)
    long long off[WC_MAX_CHROM + 1];    // first flat bin of chromosome c (0-based), off[n_chrom] = n_total
    long long poff[WC_MAX_CHROM + 1];   // first element of selected chromosome s in a sample's stretch of P
    int sel[WC_MAX_CHROM];              // selected chromosomes, 0-based
    int len[CX_MAX_LENGTHS];            // window lengths
    double root[CX_MAX_LENGTHS];        // sqrt((double)len), rounded on the host
    int n_chrom, n_sel, n_len, pad;
};

__device__ __forceinline__ bool cx_finite(double z) { return fabs(z) <= DBL_MAX; }     // false for NaN and the infinities
__device__ __forceinline__ bool cx_whole(double v, double lo, double hi) { return v >= lo && v <= hi && v == floor(v); }

__global__ __launch_bounds__(CX_T) void k_cx_check(CxTab *__restrict__ tab, const double *__restrict__ calls,
                                                   const int *__restrict__ n_calls, int max_calls, long long n_samples) {
    const long long g = (long long)blockIdx.x * CX_T + threadIdx.x;
    if (g >= n_samples * max_calls) return;
    const long long i = g / max_calls;
    const int r = (int)(g - i * max_calls);
    if (r >= n_calls[i]) return;
    const double *c = calls + g * 5;
    bool ok = cx_whole(c[0], 1.0, (double)tab->n_chrom);
    if (ok) {
        const long long size = tab->off[(int)c[0]] - tab->off[(int)c[0] - 1];
        ok = cx_whole(c[1], 0.0, (double)size - 1.0) && cx_whole(c[2], c[1], (double)size - 1.0);
    }
    if (!ok) atomicMin(&tab->status, g);
}

__global__ __launch_bounds__(CX_T) void k_cx_bins(const CxTab *__restrict__ tab, const double *__restrict__ Z, long long row_stride,
                                                  long long n_samples, const double *__restrict__ thr,
                                                  const double *__restrict__ calls, const int *__restrict__ n_calls, int max_calls,
                                                  int *__restrict__ bins_i, double *__restrict__ bins_f) {
    const long long b = (long long)blockIdx.x * CX_T + threadIdx.x, n_total = tab->off[tab->n_chrom];
    if (b >= n_total) return;
    int tested = 0, nonfinite = 0, over_hi = 0, over_lo = 0, in_gain = 0, in_loss = 0;
    double s1 = 0.0, s2 = 0.0;
    for (long long i = 0; i < n_samples; ++i) {
        const double z = Z[i * row_stride + b], t = thr[i];
        if (z != 0.0) {
            ++tested;
            if (cx_finite(z)) {
                over_hi += z >= t;
                over_lo += z <= -t;
                // each product is rounded before it is added: no FMA contraction
                s1 = __dadd_rn(s1, z);
                s2 = __dadd_rn(s2, __dmul_rn(z, z));
            } else {
                ++nonfinite;
            }
        }
        int n = n_calls[i];
        n = n < 0 ? 0 : (n > max_calls ? max_calls : n);
        const double *mine = calls + i * (long long)max_calls * 5;
        for (int r = 0; r < n; ++r) {                   // (the same rows in every lane; k_cx_check has bounded them)
            const double *c = mine + (long long)r * 5;
            const long long first = tab->off[(int)c[0] - 1];
            const bool covers = b >= first + (long long)c[1] && b <= first + (long long)c[2];
            in_gain += covers && c[3] > 0.0;
            in_loss += covers && c[3] < 0.0;
        }
    }
    int *bi = bins_i + b * 6;
    bi[0] = tested;
    bi[1] = nonfinite;
    bi[2] = over_hi;
    bi[3] = over_lo;
    bi[4] = in_gain;
    bi[5] = in_loss;
    bins_f[b * 2] = s1;
    bins_f[b * 2 + 1] = s2;
}

__global__ __launch_bounds__(CX_T) void k_cx_prefix(const CxTab *__restrict__ tab, const double *__restrict__ Z, long long row_stride,
                                                    long long n_samples, double *__restrict__ P, int *__restrict__ row_n) {
    const long long g = (long long)blockIdx.x * CX_T + threadIdx.x;
    const int n_sel = tab->n_sel;
    if (g >= n_samples * n_sel) return;
    const long long i = g / n_sel;
    const int s = (int)(g - i * n_sel), c = tab->sel[s];
    const double *z = Z + i * row_stride;
    double *p = P + i * tab->poff[n_sel] + tab->poff[s];
    double sum = 0.0;
    int n = 0;
    bool bad = false;
    p[0] = 0.0;
    for (long long b = tab->off[c]; b < tab->off[c + 1]; ++b) {
        const double v = z[b];
        if (v == 0.0) continue;
        bad = bad || !cx_finite(v);
        sum = __dadd_rn(sum, v);                        // sequential: P[j + 1] = P[j] + t[j]
        p[++n] = sum;
    }
    row_n[g] = bad ? -1 : n;
}

__global__ __launch_bounds__(CX_T) void k_cx_rec(const CxTab *__restrict__ tab, const double *__restrict__ Z, long long row_stride,
                                                 long long n_samples, const double *__restrict__ thr, const double *__restrict__ asdef,
                                                 const double *__restrict__ calls, const int *__restrict__ n_calls, int max_calls,
                                                 const int *__restrict__ row_n, int *__restrict__ rec_i, double *__restrict__ rec_f,
                                                 long long *__restrict__ win_n) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (CX_T / 64) + (threadIdx.x >> 6);
    if (i >= n_samples) return;
    const long long n_total = tab->off[tab->n_chrom];
    const double *z = Z + i * row_stride;
    const double t = thr[i];
    long long tested = 0, nonfinite = 0, over_hi = 0, over_lo = 0, call_bins = 0;
    double hi = -INFINITY, lo = INFINITY;               // (of finite values: neither infinity is one of them)
    for (long long b = lane; b < n_total; b += 64) {
        const double v = z[b];
        if (v == 0.0) continue;
        ++tested;
        if (!cx_finite(v)) { ++nonfinite; continue; }
        over_hi += v >= t;
        over_lo += v <= -t;
        hi = v > hi ? v : hi;
        lo = v < lo ? v : lo;
    }
    int n = n_calls[i];
    n = n < 0 ? 0 : (n > max_calls ? max_calls : n);
    const double *mine = calls + i * (long long)max_calls * 5;
    for (int r = lane; r < n; r += 64) call_bins += (long long)mine[(long long)r * 5 + 2] - (long long)mine[(long long)r * 5 + 1] + 1;
    for (int d = 32; d >= 1; d >>= 1) {
        tested += __shfl_xor(tested, d, 64);
        nonfinite += __shfl_xor(nonfinite, d, 64);
        over_hi += __shfl_xor(over_hi, d, 64);
        over_lo += __shfl_xor(over_lo, d, 64);
        call_bins += __shfl_xor(call_bins, d, 64);
        const double o_hi = __shfl_xor(hi, d, 64), o_lo = __shfl_xor(lo, d, 64);
        hi = o_hi > hi ? o_hi : hi;
        lo = o_lo < lo ? o_lo : lo;
    }
    const int n_sel = tab->n_sel, n_len = tab->n_len;
    const int *rows = row_n + i * n_sel;
    if (lane < n_len) {                                 // win_n: lane l owns length l (at most 16)
        const int L = tab->len[lane];
        long long w = 0;
        for (int s = 0; s < n_sel; ++s) w += rows[s] >= L ? rows[s] - L + 1 : 0;
        win_n[i * n_len + lane] = w;
    }
    if (lane != 0) return;
    int skipped = 0;
    for (int s = 0; s < n_sel; ++s) skipped += rows[s] < 0;
    auto clip = [](long long v) { return (int)(v > INT_MAX ? INT_MAX : v); };
    int *ri = rec_i + i * 8;
    double *rf = rec_f + i * 4;
    const bool any = tested > nonfinite;
    ri[0] = 0;                                          // the fold: the caller's to fill in
    ri[1] = n;
    ri[2] = clip(tested);
    ri[3] = clip(nonfinite);
    ri[4] = clip(over_hi);
    ri[5] = clip(over_lo);
    ri[6] = clip(call_bins);
    ri[7] = skipped;
    rf[0] = asdef[i];
    rf[1] = t;
    rf[2] = any ? hi : (double)NAN;
    rf[3] = any ? lo : (double)NAN;
}

__global__ __launch_bounds__(CX_T) void k_cx_windows(const CxTab *__restrict__ tab, long long n_samples, const double *__restrict__ thr,
                                                     const double *__restrict__ P, const int *__restrict__ row_n,
                                                     unsigned long long *__restrict__ win_i, unsigned long long *__restrict__ win_hist) {
    __shared__ unsigned hist[CX_SLOTS];
    __shared__ unsigned over[2];
    const long long i = blockIdx.x;
    const int l = blockIdx.y, n_sel = tab->n_sel, L = tab->len[l];
    const double root = tab->root[l], t = thr[i];
    for (int k = threadIdx.x; k < CX_SLOTS; k += CX_T) hist[k] = 0;
    if (threadIdx.x < 2) over[threadIdx.x] = 0;
    wc_sync();
    const int *rows = row_n + i * n_sel;
    const double *mine = P + i * tab->poff[n_sel];
    unsigned n_hi = 0, n_lo = 0;
    unsigned long long n_rows = 0, n_windows = 0;       // (the same in every lane)
    for (int s = 0; s < n_sel; ++s) {
        const int n = rows[s];
        if (n < L) continue;                            // skipped (-1) or too short for a window
        ++n_rows;
        n_windows += (unsigned long long)(n - L + 1);
        const double *p = mine + tab->poff[s];
        for (int a = threadIdx.x; a <= n - L; a += CX_T) {
            const double w = __ddiv_rn(__dsub_rn(p[a + L], p[a]), root);
            n_hi += w >= t;
            n_lo += w <= -t;
            int slot;
            if (w < -16.0) slot = 0;
            else if (!(w < 16.0)) slot = CX_SLOTS - 1;  // w >= 16 or NaN
            else slot = 1 + (int)floor(__dmul_rn(__dadd_rn(w, 16.0), 4.0));
            atomicAdd(&hist[slot < CX_SLOTS - 1 ? slot : CX_SLOTS - 1], 1u);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        n_hi += __shfl_xor(n_hi, d, 64);
        n_lo += __shfl_xor(n_lo, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_hi) atomicAdd(&over[0], n_hi);
        if (n_lo) atomicAdd(&over[1], n_lo);
    }
    wc_sync();
    for (int k = threadIdx.x; k < CX_SLOTS; k += CX_T)
        if (hist[k]) atomicAdd(win_hist + (long long)l * CX_SLOTS + k, (unsigned long long)hist[k]);
    if (threadIdx.x == 0) {
        unsigned long long *wi = win_i + (long long)l * 4;
        if (n_rows) atomicAdd(wi, n_rows);
        if (n_windows) atomicAdd(wi + 1, n_windows);
        if (over[0]) atomicAdd(wi + 2, (unsigned long long)over[0]);
        if (over[1]) atomicAdd(wi + 3, (unsigned long long)over[1]);
    }
}

// the arguments the host can judge, and the call's tables
int cx_tables(const double *Z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom, const double *thr,
              const double *asdef, const double *calls, const int32_t *n_calls, int max_calls, const int32_t *sel, int n_sel,
              const int32_t *lengths, int n_lengths, CxTab &tab) {
    WC_CHECK(Z && chrom_sizes && thr && asdef && calls && n_calls && sel && lengths, WC_E_ARG, "crossval stats: NULL argument");
    WC_CHECK(n_samples >= 1 && n_samples <= INT_MAX, WC_E_ARG, "crossval stats: %lld samples", (long long)n_samples);
    WC_CHECK(n_chrom >= 1 && n_chrom <= WC_MAX_CHROM, WC_E_ARG, "crossval stats: %d chromosomes (1 .. %d)", n_chrom, WC_MAX_CHROM);
    memset(&tab, 0, sizeof(tab));
    tab.status = LLONG_MAX;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_sizes[c] >= 0 && chrom_sizes[c] <= INT_MAX - 8 - tab.off[c], WC_E_ARG,
                 "crossval stats: chromosome %d has %lld bins (a row holds fewer than 2^31)", c + 1, (long long)chrom_sizes[c]);
        tab.off[c + 1] = tab.off[c] + chrom_sizes[c];
    }
    WC_CHECK(tab.off[n_chrom] >= 1, WC_E_ARG, "crossval stats: a row without bins");
    WC_CHECK(row_stride >= tab.off[n_chrom], WC_E_ARG, "crossval stats: a row stride of %lld for %lld bins", (long long)row_stride,
             (long long)tab.off[n_chrom]);
    WC_CHECK(max_calls >= 1 && n_samples * (int64_t)max_calls <= (int64_t)INT_MAX * CX_T, WC_E_ARG, "crossval stats: max_calls = %d", max_calls);
    WC_CHECK(n_sel >= 1 && n_sel <= n_chrom, WC_E_ARG, "crossval stats: %d selected chromosomes of %d", n_sel, n_chrom);
    bool seen[WC_MAX_CHROM] = {false};
    for (int s = 0; s < n_sel; ++s) {
        WC_CHECK(sel[s] >= 1 && sel[s] <= n_chrom && !seen[sel[s] - 1], WC_E_ARG,
                 "crossval stats: selected chromosome %d (1 .. %d, each once)", (int)sel[s], n_chrom);
        seen[sel[s] - 1] = true;
        tab.sel[s] = sel[s] - 1;
        tab.poff[s + 1] = tab.poff[s] + chrom_sizes[sel[s] - 1] + 1;
    }
    WC_CHECK(n_lengths >= 1 && n_lengths <= CX_MAX_LENGTHS, WC_E_ARG, "crossval stats: %d window lengths (1 .. %d)", n_lengths, CX_MAX_LENGTHS);
    for (int l = 0; l < n_lengths; ++l) {
        WC_CHECK(lengths[l] >= 1 && (l == 0 || lengths[l] > lengths[l - 1]), WC_E_ARG,
                 "crossval stats: window length %d at place %d (each >= 1, strictly ascending)", (int)lengths[l], l);
        tab.len[l] = lengths[l];
        tab.root[l] = sqrt((double)lengths[l]);
    }
    tab.n_chrom = n_chrom;
    tab.n_sel = n_sel;
    tab.n_len = n_lengths;
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_crossval_stats_dev(wc_ctx *ctx, void *stream_, const double *Z, int64_t row_stride, int64_t n_samples,
                          const int64_t *chrom_sizes_host, int n_chrom, const double *thr, const double *asdef, const double *calls,
                          const int32_t *n_calls, int max_calls, const int32_t *sel_host, int n_sel, const int32_t *lengths_host,
                          int n_lengths, int32_t *bins_i, double *bins_f, int32_t *rec_i, double *rec_f, int64_t *win_n, int64_t *win_i,
                          int64_t *win_hist) {
    WC_CHECK(ctx && bins_i && bins_f && rec_i && rec_f && win_n && win_i && win_hist, WC_E_ARG, "crossval stats: NULL argument");
    CxTab tab;
    int rc;
    if ((rc = cx_tables(Z, row_stride, n_samples, chrom_sizes_host, n_chrom, thr, asdef, calls, n_calls, max_calls, sel_host, n_sel,
                        lengths_host, n_lengths, tab)))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    WC_HIP(hipSetDevice(ctx->device));
    const long long n_total = tab.off[n_chrom], p_row = tab.poff[n_sel];
    if ((rc = ctx->cx_tab.reserve(sizeof(CxTab))) || (rc = ctx->cx_prefix.reserve(sizeof(double) * (size_t)n_samples * (size_t)p_row)) ||
        (rc = ctx->cx_rows.reserve(sizeof(int) * (size_t)n_samples * (size_t)n_sel)) || (rc = ctx->ensure_pinned(sizeof(long long))))
        return rc;
    CxTab *dtab = ctx->cx_tab.as<CxTab>();
    // (a pageable source: the call returns with the tables read)
    WC_HIP(hipMemcpyAsync(dtab, &tab, sizeof(CxTab), hipMemcpyHostToDevice, stream));
    auto blocks = [](long long n) { return dim3((unsigned)((n + CX_T - 1) / CX_T)); };
    hipLaunchKernelGGL(k_cx_check, blocks(n_samples * max_calls), dim3(CX_T), 0, stream, dtab, calls, (const int *)n_calls, max_calls,
                       (long long)n_samples);
    WC_HIP(hipGetLastError());
    // the call's one wait: a bad call row is refused before any output is written
    long long *status = (long long *)ctx->pinned;
    WC_HIP(hipMemcpyAsync(status, &dtab->status, sizeof(long long), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    WC_CHECK(*status == LLONG_MAX, WC_E_ARG,
             "crossval stats: call row %lld of sample %lld lies outside the layout (a chromosome 1 .. %d, whole 0 <= start <= end < its bins)",
             *status % max_calls, *status / max_calls, n_chrom);
    WC_HIP(hipMemsetAsync(win_i, 0, sizeof(int64_t) * 4 * (size_t)n_lengths, stream));
    WC_HIP(hipMemsetAsync(win_hist, 0, sizeof(int64_t) * CX_SLOTS * (size_t)n_lengths, stream));
    double *P = ctx->cx_prefix.as<double>();
    int *row_n = ctx->cx_rows.as<int>();
    hipLaunchKernelGGL(k_cx_bins, blocks(n_total), dim3(CX_T), 0, stream, (const CxTab *)dtab, Z, (long long)row_stride, (long long)n_samples, thr,
                       calls, (const int *)n_calls, max_calls, (int *)bins_i, bins_f);
    WC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cx_prefix, blocks(n_samples * n_sel), dim3(CX_T), 0, stream, (const CxTab *)dtab, Z, (long long)row_stride,
                       (long long)n_samples, P, row_n);
    WC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cx_rec, dim3((unsigned)((n_samples + CX_T / 64 - 1) / (CX_T / 64))), dim3(CX_T), 0, stream, (const CxTab *)dtab, Z,
                       (long long)row_stride, (long long)n_samples, thr, asdef, calls, (const int *)n_calls, max_calls, (const int *)row_n,
                       (int *)rec_i, rec_f, (long long *)win_n);
    WC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cx_windows, dim3((unsigned)n_samples, (unsigned)n_lengths), dim3(CX_T), 0, stream, (const CxTab *)dtab,
                       (long long)n_samples, thr, (const double *)P, (const int *)row_n, (unsigned long long *)win_i,
                       (unsigned long long *)win_hist);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_crossval_stats(wc_ctx *ctx, const double *Z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                      const double *thr, const double *asdef, const double *calls, const int32_t *n_calls, int max_calls, const int32_t *sel,
                      int n_sel, const int32_t *lengths, int n_lengths, int32_t *bins_i, double *bins_f, int32_t *rec_i, double *rec_f,
                      int64_t *win_n, int64_t *win_i, int64_t *win_hist) {
    WC_CHECK(ctx && bins_i && bins_f && rec_i && rec_f && win_n && win_i && win_hist, WC_E_ARG, "crossval stats: NULL argument");
    CxTab tab;
    int rc;
    if ((rc = cx_tables(Z, row_stride, n_samples, chrom_sizes, n_chrom, thr, asdef, calls, n_calls, max_calls, sel, n_sel, lengths,
                        n_lengths, tab)))
        return rc;
    WC_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n_samples, T = (size_t)tab.off[n_chrom], nl = (size_t)n_lengths;
    // inputs: Z | calls | thr | asdef | n_calls; outputs: bins_f | rec_f | win_n | win_i | win_hist | bins_i | rec_i (8-byte items first)
    const size_t in_bytes[5] = {8 * N * (size_t)row_stride, 8 * N * (size_t)max_calls * 5, 8 * N, 8 * N, 4 * N};
    const size_t out_bytes[7] = {8 * T * 2, 8 * N * 4, 8 * N * nl, 8 * nl * 4, 8 * nl * CX_SLOTS, 4 * T * 6, 4 * N * 8};
    const void *in_host[5] = {Z, calls, thr, asdef, n_calls};
    void *out_host[7] = {bins_f, rec_f, win_n, win_i, win_hist, bins_i, rec_i};
    size_t in_at[5], out_at[7], total = 0;
    for (int k = 0; k < 5; ++k) { in_at[k] = total; total += (in_bytes[k] + 255) & ~(size_t)255; }
    for (int k = 0; k < 7; ++k) { out_at[k] = total; total += (out_bytes[k] + 255) & ~(size_t)255; }
    if ((rc = ctx->tmp_a.reserve(total))) return rc;
    unsigned char *d = ctx->tmp_a.as<unsigned char>();
    for (int k = 0; k < 5; ++k) WC_HIP(hipMemcpy(d + in_at[k], in_host[k], in_bytes[k], hipMemcpyHostToDevice));
    if ((rc = wc_crossval_stats_dev(ctx, nullptr, (const double *)(d + in_at[0]), row_stride, n_samples, chrom_sizes, n_chrom,
                                    (const double *)(d + in_at[2]), (const double *)(d + in_at[3]), (const double *)(d + in_at[1]),
                                    (const int32_t *)(d + in_at[4]), max_calls, sel, n_sel, lengths, n_lengths, (int32_t *)(d + out_at[5]),
                                    (double *)(d + out_at[0]), (int32_t *)(d + out_at[6]), (double *)(d + out_at[1]), (int64_t *)(d + out_at[2]),
                                    (int64_t *)(d + out_at[3]), (int64_t *)(d + out_at[4]))))
        return rc;
    WC_HIP(hipDeviceSynchronize());
    for (int k = 0; k < 7; ++k) WC_HIP(hipMemcpy(out_host[k], d + out_at[k], out_bytes[k], hipMemcpyDeviceToHost));
    return WC_OK;
}

}  // extern "C"
