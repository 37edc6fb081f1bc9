// Robust column statistics: the median and the median absolute deviation of every column of a [n_rows, row_stride]
// float64 matrix, by exact selection (include/wisecondor_hip.h has the rule).  The classes are crossval's:
// a value is TESTED when z != 0, NONFINITE when tested and not finite, else FINITE; only FINITE values take part.
//   k_rb_cols   a lane per column, as k_cx_bins: a wave reads 512 contiguous bytes of every row.  A value's order-preserving
//               64-bit key is its bits, all of them flipped for a negative value and the sign bit flipped otherwise.  The
//               k-th smallest key comes from a radix descent, most significant digit first: per digit the lane reads its
//               column again (from L2: a wave's strip of the matrix is n_rows * 512 bytes), counts the digits of the keys
//               that share the prefix found so far, and walks the counts to the digit that holds rank k.  The descent also
//               leaves how many values are smaller than the k-th and how many equal it, so the upper middle value of an
//               even count is the same value when enough are equal, and otherwise the smallest larger key: one more pass.
//               The deviation's selection is the same descent over d = |z - median|, formed on the fly (__dsub_rn).
//               The digit counters are the lane's own: RB_BITS-bit digits, 16-bit counters (n_rows <= 8192) packed into
//               64-bit registers, so there is no LDS, no barrier and nothing shared between lanes; lanes of a wave differ in
//               their counts and ranks, and only the row loop has the same trip count in all of them.
#include <limits.h>

#include "ctx.h"

namespace {

const int RB_T = 64;                    // lanes per workgroup: a wave, so that few columns still spread over the CUs
const int RB_BITS = 4;                  // digit width; 64 % RB_BITS == 0
const int RB_DIGITS = 1 << RB_BITS;
const int RB_WORDS = (RB_DIGITS + 3) / 4;          // four 16-bit counters to a 64-bit word
const int RB_MAX_ROWS = 8192;           // the project's sample limit; a 16-bit counter holds it

typedef unsigned long long rb_key;

__device__ __forceinline__ bool rb_finite(double z) { return fabs(z) <= DBL_MAX; }     // false for NaN and the infinities
__device__ __forceinline__ rb_key rb_to_key(double v) {
    const rb_key u = (rb_key)__double_as_longlong(v);
    return u ^ ((u >> 63) ? ~0ull : 1ull << 63);
}
__device__ __forceinline__ double rb_to_value(rb_key k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 1ull << 63 : ~0ull)));
}

struct RbPick {                         // what a descent leaves
    rb_key key;                         // the key of rank k
    int less, equal;                    // values with a smaller key, values with this key
};

// The key of rank k (0-based, k < the column's FINITE values) among value(z) of the column's FINITE z.
template <class F>
__device__ __forceinline__ RbPick rb_descend(const double *__restrict__ col, long long row_stride, int n_rows, int k, F value) {
    rb_key prefix = 0;
    int less = 0, equal = 0;
    for (int shift = 64 - RB_BITS; shift >= 0; shift -= RB_BITS) {
        rb_key cnt[RB_WORDS];
        for (int w = 0; w < RB_WORDS; ++w) cnt[w] = 0;
        // the keys that share the digits above `shift` with the prefix (every key in the first pass)
        const rb_key high = shift + RB_BITS < 64 ? ~0ull << ((shift + RB_BITS) & 63) : 0ull;
#pragma unroll 4
        for (int i = 0; i < n_rows; ++i) {
            const double z = col[(long long)i * row_stride];
            if (z != 0.0 && rb_finite(z)) {
                const rb_key key = rb_to_key(value(z));
                if ((key & high) == prefix) {
                    const int d = (int)(key >> shift) & (RB_DIGITS - 1);
                    const rb_key one = 1ull << ((d & 3) * 16);
                    for (int w = 0; w < RB_WORDS; ++w) cnt[w] += (d >> 2) == w ? one : 0ull;     // (registers: no indexing by d)
                }
            }
        }
        int rank = k - less, digit = 0;
        bool found = false;
        for (int d = 0; d < RB_DIGITS; ++d) {
            const int c = (int)(cnt[d >> 2] >> ((d & 3) * 16)) & 0xFFFF;
            if (!found && rank < c) { found = true; digit = d; equal = c; }
            if (!found) { rank -= c; less += c; }
        }
        prefix |= (rb_key)digit << shift;
    }
    return {prefix, less, equal};
}

// med() of the rule over value(z) of the column's n >= 1 FINITE z.
template <class F>
__device__ __forceinline__ double rb_median(const double *__restrict__ col, long long row_stride, int n_rows, int n, F value) {
    const RbPick lo = rb_descend(col, row_stride, n_rows, (n - 1) / 2, value);
    if (n & 1) return rb_to_value(lo.key);
    rb_key hi = lo.key;
    if (lo.less + lo.equal <= n / 2) {  // the upper middle rank lies behind the run of equal values: the smallest larger key
        hi = ~0ull;
        for (int i = 0; i < n_rows; ++i) {
            const double z = col[(long long)i * row_stride];
            if (z != 0.0 && rb_finite(z)) {
                const rb_key key = rb_to_key(value(z));
                hi = key > lo.key && key < hi ? key : hi;
            }
        }
    }
    return __ddiv_rn(__dadd_rn(rb_to_value(lo.key), rb_to_value(hi)), 2.0);      // the sum is rounded first
}

__global__ __launch_bounds__(RB_T) void k_rb_cols(const double *__restrict__ Z, long long row_stride, int n_rows, long long n_cols,
                                                  int *__restrict__ col_i, double *__restrict__ col_f) {
    const long long b = (long long)blockIdx.x * RB_T + threadIdx.x;
    if (b >= n_cols) return;
    const double *col = Z + b;
    int finite = 0, nonfinite = 0;
    for (int i = 0; i < n_rows; ++i) {
        const double z = col[(long long)i * row_stride];
        if (z != 0.0) {
            if (rb_finite(z)) ++finite;
            else ++nonfinite;
        }
    }
    double median = (double)NAN, mad = (double)NAN;
    if (finite > 0) {
        median = rb_median(col, row_stride, n_rows, finite, [](double z) { return z; });
        if (rb_finite(median)) {
            const double centre = median;
            mad = rb_median(col, row_stride, n_rows, finite, [centre](double z) { return fabs(__dsub_rn(z, centre)); });
        }
    }
    col_i[b * 2] = finite;
    col_i[b * 2 + 1] = nonfinite;
    col_f[b * 2] = median;
    col_f[b * 2 + 1] = mad;
}

int rb_check(wc_ctx *ctx, const double *Z, int64_t row_stride, int64_t n_rows, int64_t n_cols, const int32_t *col_i, const double *col_f) {
    WC_CHECK(ctx && Z && col_i && col_f, WC_E_ARG, "column robust: NULL argument");
    WC_CHECK(n_rows >= 1 && n_cols >= 1 && n_cols <= (int64_t)INT_MAX && row_stride >= n_cols, WC_E_ARG,
             "column robust: %lld rows of %lld columns at a row stride of %lld", (long long)n_rows, (long long)n_cols, (long long)row_stride);
    WC_CHECK(n_rows <= RB_MAX_ROWS, WC_E_LIMIT, "column robust: %lld rows (%d at most)", (long long)n_rows, RB_MAX_ROWS);
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_column_robust_dev(wc_ctx *ctx, void *stream, const double *Z, int64_t row_stride, int64_t n_rows, int64_t n_cols, int32_t *col_i,
                         double *col_f) {
    int rc;
    if ((rc = rb_check(ctx, Z, row_stride, n_rows, n_cols, col_i, col_f))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_rb_cols, dim3((unsigned)((n_cols + RB_T - 1) / RB_T)), dim3(RB_T), 0, (hipStream_t)stream, Z, (long long)row_stride,
                       (int)n_rows, (long long)n_cols, (int *)col_i, col_f);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_column_robust(wc_ctx *ctx, const double *Z, int64_t row_stride, int64_t n_rows, int64_t n_cols, int32_t *col_i, double *col_f) {
    int rc;
    if ((rc = rb_check(ctx, Z, row_stride, n_rows, n_cols, col_i, col_f))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    // Z (the last row only as far as its columns go) | col_f | col_i
    const size_t z_bytes = 8 * ((size_t)(n_rows - 1) * (size_t)row_stride + (size_t)n_cols), f_bytes = 16 * (size_t)n_cols, i_bytes = 8 * (size_t)n_cols;
    const size_t f_at = (z_bytes + 255) & ~(size_t)255, i_at = f_at + ((f_bytes + 255) & ~(size_t)255);
    if ((rc = ctx->tmp_a.reserve(i_at + i_bytes))) return rc;
    unsigned char *d = ctx->tmp_a.as<unsigned char>();
    WC_HIP(hipMemcpy(d, Z, z_bytes, hipMemcpyHostToDevice));
    if ((rc = wc_column_robust_dev(ctx, nullptr, (const double *)d, row_stride, n_rows, n_cols, (int32_t *)(d + i_at), (double *)(d + f_at))))
        return rc;
    WC_HIP(hipDeviceSynchronize());
    WC_HIP(hipMemcpy(col_f, d + f_at, f_bytes, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(col_i, d + i_at, i_bytes, hipMemcpyDeviceToHost));
    return WC_OK;
}

}  // extern "C"
