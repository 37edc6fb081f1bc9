// What plot.hip (the rasteriser) and pdf.hip (the content stream) share.  On the device: decimal digits without a buffer,
// the exact "{:.1f}" label of a call, rounding to whole units and a panel's y range.  On the host (defined in plot.hip):
// the page plan -- one pinned block of small tables per call with a tail of the back end's own -- the launch of
// k_plot_list, and what the two host-array entry points do around their stages.
#pragma once
#include "ctx.h"

#if defined(__HIPCC__)
// decimal digits of v >= 0 (at least one)
__device__ __forceinline__ int pl_digits(unsigned long long v) {
    int n = 1;
    while (v >= 10ull) {
        v /= 10ull;
        ++n;
    }
    return n;
}
// digit `k` (0 = the most significant) of the `n`-digit number v
__device__ __forceinline__ int pl_digit(unsigned long long v, int n, int k) {
    for (int i = n - 1; i > k; --i) v /= 10ull;
    return '0' + (int)(v % 10ull);
}
// "{:.1f}".format(z) without a buffer: tenths = the correctly rounded abs(z) * 10 (ties to even on the exact value, which
// v * 8 + v * 2 with the error of the one addition gives); false: the label is "?" (not finite, or abs(z) >= 1e9)
__device__ __forceinline__ bool pl_label_tenths(double zc, unsigned long long &tenths, int &neg) {
    const double v = fabs(zc);
    neg = __builtin_signbit(zc) ? 1 : 0;
    if (!(v < 1e9)) return false;
    const double a = v * 8.0, b = v * 2.0, sum = a + b, bb = sum - a;
    const double err = (a - (sum - bb)) + (b - bb);
    const double whole = floor(sum), r = (sum - whole) - 0.5;
    unsigned long long n = (unsigned long long)whole;
    if (r > 0.0 || (r == 0.0 && (err > 0.0 || (err == 0.0 && (n & 1ull))))) ++n;
    tenths = n;
    return true;
}
__device__ __forceinline__ int pl_label_len(bool ok, unsigned long long tenths, int neg) {
    return ok ? neg + pl_digits(tenths / 10ull) + 2 : 1;
}
__device__ __forceinline__ int pl_label_char(bool ok, unsigned long long tenths, int neg, int n, int k) {
    if (!ok) return '?';
    if (neg && k == 0) return '-';
    if (k == n - 1) return '0' + (int)(tenths % 10ull);
    if (k == n - 2) return '.';
    return pl_digit(tenths / 10ull, n - neg - 2, k - neg);
}
// floor(v + 0.5) and floor(v) as int; values beyond +-1e9 stop there, NaN lies nowhere
__device__ __forceinline__ int pl_rnd(double v) {
    if (!(v == v)) return -2000000000;
    v = v < -1e9 ? -1e9 : (v > 1e9 ? 1e9 : v);
    return (int)floor(v + 0.5);
}
__device__ __forceinline__ int pl_flr(double v) {
    if (!(v == v)) return -2000000000;
    v = v < -1e9 ? -1e9 : (v > 1e9 ? 1e9 : v);
    return (int)floor(v);
}
__device__ __forceinline__ int pl_alpha(double alpha) {
    const int a = pl_rnd(255.0 * alpha);
    return a < 0 ? 0 : (a > 255 ? 255 : a);
}
// a panel's y range from the finite z range of its list's first entry (mn, mx): the threshold lines and, on a page with
// cytobands, their strip stay inside, 5 % of the range is added at either end
__device__ __forceinline__ void pl_yrange(double mn, double mx, double thr, int has_cyto, double &yhi, double &yspan) {
    const double cyto_y = -thr - thr / 2.0, base = has_cyto ? cyto_y : -thr;
    const double lo = mn < base ? mn : base, hi = mx > thr ? mx : thr;
    const double pad = (hi - lo) * 0.05, ylo = lo - pad;
    yhi = hi + pad;
    yspan = yhi - ylo;
}
#endif

namespace wc {
// The small tables of one call -- chromosome offsets and lengths, bands, panel chromosomes, boxes, band offsets, names --
// in ctx->pl_host (pinned) and, once sent, in ctx->pl_tab, followed by a tail of the back end's own (the rasteriser's
// arguments and font, the content kernel's sections and arguments).
struct PagePlan {
    int n_panels = 0, cap = 0, has_cyto = 0, name_cap = 0;       // cap: entries of a panel's list, the worst case
    size_t tail = 0, bytes = 0;                                  // the tail is [tail, bytes) of the block
    // the tables on the device; band_off is NULL on a page without cytobands
    const long long *chrom_off = nullptr, *chrom_len = nullptr;
    const double *bands = nullptr;
    const int *panel_chrom = nullptr, *boxes = nullptr, *band_off = nullptr;
    const char *names = nullptr;
    unsigned char *tail_host = nullptr;                          // the tail in the pinned block, for the back end to fill
    const unsigned char *tail_dev = nullptr;                     // and where its kernel finds it
};

// chromosomes, panels and the band offsets of a page, with `who` ("plot", "pdf") in front of the band table's message
int plot_check_page(const char *who, const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels,
                    int64_t row_stride, const int32_t *band_off);
// Checks the page, lays its panels out (columns >= 1; 0: no boxes), works the lists' capacity out, waits until the
// previous call's block has left the pinned memory and fills it again.  bands, band_off and names may be absent.
int page_plan(wc_ctx *ctx, const char *who, const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels,
              int64_t row_stride, int max_calls, int columns, int width, int height, const double *bands, const int32_t *band_off,
              const char *names, int64_t n_samples, int name_cap, size_t tail_bytes, PagePlan &P);
// enqueues the copy of bytes [from, to) of the block and records ctx->pl_sent behind it: the one event the next
// page_plan waits for (it waits for these small copies only, not for the call's kernels)
int page_send(wc_ctx *ctx, hipStream_t stream, size_t from, size_t to);
// k_plot_list on the plan's tables into ctx->pl_list / pl_counts / pl_status (the status word is cleared first)
int plot_list_launch(wc_ctx *ctx, hipStream_t stream, const PagePlan &P, const double *z, int64_t row_stride, int64_t n_samples,
                     const double *calls, const int32_t *n_calls, int max_calls, double thr, double mineffect, int cap);

// What wc_plot_batch and wc_plot_pdf_batch do around their stages.  Device memory: tmp_a holds z rows | calls | call
// counts, tmp_b the streams, tmp_c their lengths, tmp_d the Adler-32 words.  Events: [5] in front of the copy in, [0] .. [4]
// behind the tables' copy and the four stages (the back end records them), [6] behind the copy out.
struct HostBatch {
    Events<7> events;
    hipEvent_t *ev = nullptr;                                    // NULL: no times were asked for
    const double *z = nullptr, *calls = nullptr;                 // the device's copies (NULL where the host gave none)
    const int32_t *n_calls = nullptr;
    int stage(wc_ctx *ctx, const double *z_host, int64_t row_stride, int64_t n_samples, const double *calls_host,
              const int32_t *n_calls_host, int max_calls, bool timed);
    // the status word, the lengths and the Adler-32 words, then stream i from tmp_b + i * dev_stride
    int collect(wc_ctx *ctx, const char *who, int64_t n_samples, int64_t dev_stride, unsigned char *streams_out, int64_t out_stride,
                int64_t *out_len, uint32_t *adler_out);
    void times(double *times_ms);                                // [0] copy in [1] .. [4] the stages [5] copy out; [6], [7] zero
};

inline void put32(unsigned char *p, uint32_t v) {                // big-endian, as PNG chunks and zlib's Adler-32 have it
    p[0] = (unsigned char)(v >> 24);
    p[1] = (unsigned char)(v >> 16);
    p[2] = (unsigned char)(v >> 8);
    p[3] = (unsigned char)v;
}
}  // namespace wc
