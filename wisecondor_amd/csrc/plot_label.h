// What plot.hip (the rasteriser) and pdf.hip (the content stream) share: decimal digits without a buffer and the exact
// "{:.1f}" label of a call, on the device; on the host the checks and the launch of k_plot_list (defined in plot.hip).
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
#endif

namespace wc {
// plot.hip: the argument checks every plot call shares, and k_plot_list enqueued on `stream` with the three small tables
// already on the device (the status word is cleared first)
int plot_check_panels(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, int64_t row_stride);
int plot_list_launch(hipStream_t stream, const double *z, int64_t row_stride, int64_t n_samples, const long long *chrom_off_dev,
                     const long long *chrom_len_dev, const int *panel_chrom_dev, const double *calls, const int32_t *n_calls,
                     int max_calls, double thr, double mineffect, int n_panels, int cap, double *entries, int *counts, int *status);
}  // namespace wc
