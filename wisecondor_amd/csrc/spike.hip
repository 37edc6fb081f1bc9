// sensitivity: planted aberrations, spiked and judged on the device.
// A trial is a plan row {base row, chromosome (1-based), first bin, bins, effect in ppm}; the host checks every row, turns
// it into a SpRow (the base row's offset and the span as flat bins of a row) and only then uploads it.
//   k_spike        the trials' count rows: a copy of the base row, and inside the span every count c >= 0 becomes
//                  min(2^31 - 1, (c * (1 000 000 + ppm) + 500 000) div 1 000 000) in 64-bit integers.  The output is ONE flat
//                  int32 array cut into quads of four elements at 16-byte addresses, a lane per quad and SP_U quads per
//                  lane, their loads issued together.  A workgroup belongs to one trial (blockIdx.x), so the plan row is
//                  the same in every lane.  A quad's four sources lie together in the base row, but begin at any multiple
//                  of four bytes: they are read by ONE load of 16 bytes that is aligned to four (global_load_dwordx4; gfx950
//                  global loads take any dword alignment, a wave's load then touches one 128-byte line more).  A quad that
//                  reaches beyond its trial's row (trial * n_total is no multiple of four when n_total % 4 != 0), in front
//                  of the array or behind it goes element by element and finds each element's own trial.  The span test
//                  and the multiply run only in lanes whose quad meets the span; the divide is by a constant.
//   k_spike_score  a wave per trial: lanes stride over the trial's n_calls rows [chrom, start, end, z, effect]; a call
//                  matches when its chromosome is the trial's, its z has the effect's sign and it overlaps the span by a bin
//                  at least.  Counts and sums by a wave reduction, the best call (largest overlap, earliest row) by an
//                  arg-max; lane 0 copies that row's doubles.  Sums are kept in 64 bits and stored clipped to 2^31 - 1.
// Nothing synchronises inside a workgroup and no kernel uses LDS.  The host's half (checked rows, upload, launches) is
// declared in spike.h: draw.hip, which holds the binomial spike and the _ex entry points, calls it too.
#include <limits.h>

#include "spike.h"

namespace {

const int SP_T = 256;                   // lanes per workgroup
const int SP_U = 4;                     // quads per lane in k_spike
const int SP_PPM_MIN = -1000000, SP_PPM_MAX = 100000000;

__device__ __forceinline__ int sp_value(int c, int ppm, int &clipped) {
    if (c < 0) return c;
    const unsigned long long v = ((unsigned long long)c * (unsigned long long)(1000000 + ppm) + 500000ull) / 1000000ull;
    if (v > 2147483647ull) {
        ++clipped;
        return INT_MAX;
    }
    return (int)v;
}

// out: the flat array; a = (address of out / 4) & 3: quad q holds flat elements 4 q - a .. 4 q - a + 3
__global__ __launch_bounds__(SP_T) void k_spike(const int *__restrict__ base, long long n_total, const SpRow *__restrict__ rows,
                                                long long n_trials, int *__restrict__ out, int a,
                                                unsigned long long *__restrict__ saturated) {
    const long long t = blockIdx.x, F = t * n_total, total = n_trials * n_total;
    const SpRow row = rows[t];
    // the quads whose first element lies in this trial's row (trial 0 also takes the quad that begins in front of the array)
    const long long q_lo = t == 0 ? 0 : (F + a + 3) >> 2, q_hi = (F + n_total + a + 3) >> 2;
    const long long q0 = q_lo + (long long)blockIdx.y * (SP_T * SP_U) + threadIdx.x;
    int4 v[SP_U];
    bool whole[SP_U];
    int clipped = 0;
#pragma unroll
    for (int u = 0; u < SP_U; ++u) {
        const long long q = q0 + (long long)u * SP_T, j0 = 4 * q - a - F;
        whole[u] = q < q_hi && j0 >= 0 && j0 + 3 < n_total;
        if (!whole[u]) continue;
        // (the four sources begin at any multiple of four bytes: a load of 16 bytes that is aligned to four)
        __builtin_memcpy(&v[u], base + row.src + j0, 16);
    }
#pragma unroll
    for (int u = 0; u < SP_U; ++u) {
        const long long q = q0 + (long long)u * SP_T, j0 = 4 * q - a - F;
        if (whole[u]) {
            if (j0 + 3 >= row.lo && j0 < row.hi) {
                if (j0 >= row.lo && j0 < row.hi) v[u].x = sp_value(v[u].x, row.ppm, clipped);
                if (j0 + 1 >= row.lo && j0 + 1 < row.hi) v[u].y = sp_value(v[u].y, row.ppm, clipped);
                if (j0 + 2 >= row.lo && j0 + 2 < row.hi) v[u].z = sp_value(v[u].z, row.ppm, clipped);
                if (j0 + 3 >= row.lo && j0 + 3 < row.hi) v[u].w = sp_value(v[u].w, row.ppm, clipped);
            }
            *reinterpret_cast<int4 *>(out + (4 * q - a)) = v[u];
        } else if (q < q_hi) {
            // an edge quad: each element finds its own trial (several rows fit a quad when n_total < 4)
            for (int k = 0; k < 4; ++k) {
                const long long e = 4 * q - a + k;
                if (e < F || e >= total) continue;
                const long long tt = e / n_total, j = e - tt * n_total;
                const SpRow r = rows[tt];
                int c = base[r.src + j];
                if (j >= r.lo && j < r.hi) c = sp_value(c, r.ppm, clipped);
                out[e] = c;
            }
        }
    }
    if (saturated) {
        for (int d = 32; d >= 1; d >>= 1) clipped += __shfl_down(clipped, d, 64);
        if ((threadIdx.x & 63) == 0 && clipped) atomicAdd(saturated, (unsigned long long)clipped);
    }
}

__global__ __launch_bounds__(SP_T) void k_spike_score(const SpRow *__restrict__ rows, long long n_trials,
                                                      const double *__restrict__ calls, const int *__restrict__ n_calls,
                                                      int max_calls, int *__restrict__ rec_i, double *__restrict__ rec_f) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * (SP_T / 64) + (threadIdx.x >> 6);
    if (t >= n_trials) return;
    const SpRow row = rows[t];
    const long long s = row.first, e = (long long)row.first + row.bins - 1;
    int n = n_calls[t];
    n = n < 0 ? 0 : (n > max_calls ? max_calls : n);
    const double *mine = calls + t * (long long)max_calls * 5;
    long long n_match = 0, overlap = 0, length = 0, best_ov = 0;
    int best_row = INT_MAX;
    for (int r = lane; r < n; r += 64) {                // (rows ascend in a lane: a later row wins with a LARGER overlap only)
        const double *c = mine + (long long)r * 5;
        const double z = c[3];
        const bool sign = row.ppm > 0 ? z > 0.0 : (row.ppm < 0 ? z < 0.0 : false);
        if (!sign || c[0] != (double)row.chrom) continue;
        const long long cs = (long long)c[1], ce = (long long)c[2];
        const long long ov = (e < ce ? e : ce) - (s > cs ? s : cs) + 1;
        if (ov < 1) continue;
        ++n_match;
        overlap += ov;
        length += ce - cs + 1;
        if (ov > best_ov) { best_ov = ov; best_row = r; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        n_match += __shfl_xor(n_match, d, 64);
        overlap += __shfl_xor(overlap, d, 64);
        length += __shfl_xor(length, d, 64);
        const long long o_ov = __shfl_xor(best_ov, d, 64);
        const int o_row = __shfl_xor(best_row, d, 64);
        if (o_ov > best_ov || (o_ov == best_ov && o_row < best_row)) { best_ov = o_ov; best_row = o_row; }
    }
    if (lane != 0) return;
    auto clip = [](long long v) { return (int)(v > INT_MAX ? INT_MAX : v); };
    int *ri = rec_i + t * 8;
    double *rf = rec_f + t * 2;
    const bool have = n_match > 0;
    const double *b = mine + (long long)(have ? best_row : 0) * 5;
    ri[0] = n;
    ri[1] = clip(n_match);
    ri[2] = clip(overlap);
    ri[3] = clip(length);
    ri[4] = have ? best_row : -1;
    ri[5] = have ? (int)(long long)b[1] : -1;
    ri[6] = have ? (int)(long long)b[2] : -1;
    ri[7] = 0;
    rf[0] = have ? b[3] : (double)NAN;
    rf[1] = have ? b[4] : (double)NAN;
}

}  // namespace

// ---- the host's half (spike.h: draw.hip calls it too) -------------------------------------------------------------------
// every plan row checked (the first bad one named) and turned into a SpRow; chrom_sizes == NULL: the score's checks alone
int sp_rows(const char *who, const int32_t *plan, int64_t n_trials, int64_t n_base, const int64_t *chrom_sizes, int n_chrom,
            std::vector<SpRow> &rows, int64_t *n_total_out) {
    WC_CHECK(n_trials >= 1 && plan, WC_E_ARG, "%s: %lld trials, or no plan", who, (long long)n_trials);
    int64_t off[WC_MAX_CHROM + 1] = {0};
    if (chrom_sizes) {
        WC_CHECK(n_chrom >= 1 && n_chrom <= WC_MAX_CHROM, WC_E_ARG, "%s: %d chromosomes (1 .. %d)", who, n_chrom, WC_MAX_CHROM);
        for (int c = 0; c < n_chrom; ++c) {
            WC_CHECK(chrom_sizes[c] >= 0 && chrom_sizes[c] <= INT_MAX - 8 - off[c], WC_E_ARG,
                     "%s: chromosome %d has %lld bins (a row holds fewer than 2^31)", who, c + 1, (long long)chrom_sizes[c]);
            off[c + 1] = off[c] + chrom_sizes[c];
        }
        WC_CHECK(off[n_chrom] >= 1, WC_E_ARG, "%s: a row without bins", who);
        WC_CHECK(n_base >= 1, WC_E_ARG, "%s: %lld base rows", who, (long long)n_base);
    }
    rows.resize((size_t)n_trials);
    for (int64_t i = 0; i < n_trials; ++i) {
        const int32_t *p = plan + 5 * i;
        const int64_t b = p[0], c = p[1], first = p[2], bins = p[3], ppm = p[4];
        WC_CHECK(ppm >= SP_PPM_MIN && ppm <= SP_PPM_MAX, WC_E_ARG, "%s: plan row %lld: an effect of %lld ppm (%d .. %d)", who,
                 (long long)i, (long long)ppm, SP_PPM_MIN, SP_PPM_MAX);
        WC_CHECK(first >= 0, WC_E_ARG, "%s: plan row %lld: first bin %lld", who, (long long)i, (long long)first);
        WC_CHECK(bins >= 1, WC_E_ARG, "%s: plan row %lld: %lld bins", who, (long long)i, (long long)bins);
        WC_CHECK(first + bins <= INT_MAX, WC_E_ARG, "%s: plan row %lld: bins %lld .. %lld", who, (long long)i, (long long)first,
                 (long long)(first + bins - 1));
        SpRow &r = rows[(size_t)i];
        r.src = 0;
        r.lo = r.hi = 0;
        if (chrom_sizes) {
            WC_CHECK(b >= 0 && b < n_base, WC_E_ARG, "%s: plan row %lld: base row %lld of %lld", who, (long long)i, (long long)b,
                     (long long)n_base);
            WC_CHECK(c >= 1 && c <= n_chrom, WC_E_ARG, "%s: plan row %lld: chromosome %lld of %d", who, (long long)i, (long long)c,
                     n_chrom);
            WC_CHECK(first + bins <= chrom_sizes[c - 1], WC_E_ARG, "%s: plan row %lld: bins %lld .. %lld of chromosome %lld, which has %lld",
                     who, (long long)i, (long long)first, (long long)(first + bins - 1), (long long)c, (long long)chrom_sizes[c - 1]);
            r.src = b * off[n_chrom];
            if (ppm != 0) {
                r.lo = (int)(off[c - 1] + first);
                r.hi = (int)(off[c - 1] + first + bins);
            }
        } else {
            WC_CHECK(c >= 1, WC_E_ARG, "%s: plan row %lld: chromosome %lld", who, (long long)i, (long long)c);
        }
        r.ppm = (int)ppm;
        r.chrom = (int)c;
        r.first = (int)first;
        r.bins = (int)bins;
    }
    if (n_total_out) *n_total_out = chrom_sizes ? off[n_chrom] : 0;
    return WC_OK;
}

int sp_upload(wc_ctx *ctx, hipStream_t stream, const std::vector<SpRow> &rows) {
    int rc;
    if ((rc = ctx->sp_plan.reserve(rows.size() * sizeof(SpRow)))) return rc;
    // (a pageable source: the call returns with the rows read, the vector may go)
    WC_HIP(hipMemcpyAsync(ctx->sp_plan.p, rows.data(), rows.size() * sizeof(SpRow), hipMemcpyHostToDevice, stream));
    return WC_OK;
}

int sp_spike_launch(wc_ctx *ctx, hipStream_t stream, const int32_t *base, int64_t n_total, int64_t n_trials, int32_t *out,
                    unsigned long long *saturated_dev, size_t slot) {
    WC_CHECK(((uintptr_t)base & 3) == 0 && ((uintptr_t)out & 3) == 0, WC_E_ARG, "spike: counts not aligned to four bytes");
    WC_CHECK(n_trials <= INT_MAX, WC_E_LIMIT, "spike: more than 2^31 - 1 trials per call");
    if (saturated_dev) WC_HIP(hipMemsetAsync(saturated_dev, 0, sizeof(unsigned long long), stream));
    const int64_t quads = n_total / 4 + 2;
    const dim3 grid((unsigned)n_trials, (unsigned)((quads + SP_T * SP_U - 1) / (SP_T * SP_U)));
    hipLaunchKernelGGL(k_spike, grid, dim3(SP_T), 0, stream, (const int *)base, (long long)n_total,
                       (const SpRow *)ctx->sp_plan.as<SpRow>() + slot, (long long)n_trials, (int *)out, (int)(((uintptr_t)out >> 2) & 3),
                       saturated_dev);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int sp_score_launch(wc_ctx *ctx, hipStream_t stream, int64_t n_trials, const double *calls, const int32_t *n_calls, int max_calls,
                    int32_t *rec_i, double *rec_f) {
    const int per = SP_T / 64;
    hipLaunchKernelGGL(k_spike_score, dim3((unsigned)((n_trials + per - 1) / per)), dim3(SP_T), 0, stream,
                       (const SpRow *)ctx->sp_plan.as<SpRow>(), (long long)n_trials, calls, (const int *)n_calls, max_calls,
                       (int *)rec_i, rec_f);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

extern "C" {

// the deterministic rule under its first names: the _ex entry points (draw.hip) with draw = 0
int wc_spike_counts_dev(wc_ctx *ctx, void *stream, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                        const int32_t *plan_host, int64_t n_trials, int32_t *out, int64_t *saturated) {
    return wc_spike_counts_ex_dev(ctx, stream, base, n_base, chrom_sizes_host, n_chrom, plan_host, n_trials, 0, 0, 0, out, saturated);
}

int wc_spike_counts(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *plan,
                    int64_t n_trials, int32_t *out, int64_t *saturated) {
    return wc_spike_counts_ex(ctx, base, n_base, chrom_sizes, n_chrom, plan, n_trials, 0, 0, 0, out, saturated);
}

int wc_spike_score_dev(wc_ctx *ctx, void *stream_, const int32_t *plan_host, int64_t n_trials, const double *calls, const int32_t *n_calls,
                       int max_calls, int32_t *rec_i, double *rec_f) {
    WC_CHECK(ctx && calls && n_calls && rec_i && rec_f, WC_E_ARG, "spike score: NULL argument");
    WC_CHECK(max_calls >= 1, WC_E_ARG, "spike score: max_calls = %d", max_calls);
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<SpRow> rows;
    int rc;
    if ((rc = sp_rows("spike score", plan_host, n_trials, 0, nullptr, 0, rows, nullptr))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    if ((rc = sp_upload(ctx, stream, rows))) return rc;
    return sp_score_launch(ctx, stream, n_trials, calls, n_calls, max_calls, rec_i, rec_f);
}

int wc_spike_score(wc_ctx *ctx, const int32_t *plan, int64_t n_trials, const double *calls, const int32_t *n_calls, int max_calls,
                   int32_t *rec_i, double *rec_f) {
    WC_CHECK(ctx && calls && n_calls && rec_i && rec_f, WC_E_ARG, "spike score: NULL argument");
    WC_CHECK(max_calls >= 1, WC_E_ARG, "spike score: max_calls = %d", max_calls);
    std::vector<SpRow> rows;
    int rc;
    if ((rc = sp_rows("spike score", plan, n_trials, 0, nullptr, 0, rows, nullptr))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    const size_t cb = sizeof(double) * (size_t)n_trials * max_calls * 5, nb = sizeof(int32_t) * (size_t)n_trials;
    if ((rc = ctx->tmp_a.reserve(cb)) || (rc = ctx->tmp_b.reserve(nb)) || (rc = ctx->tmp_c.reserve(nb * 8)) ||
        (rc = ctx->tmp_d.reserve(sizeof(double) * (size_t)n_trials * 2)) || (rc = sp_upload(ctx, nullptr, rows)))
        return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, calls, cb, hipMemcpyHostToDevice));
    WC_HIP(hipMemcpy(ctx->tmp_b.p, n_calls, nb, hipMemcpyHostToDevice));
    if ((rc = sp_score_launch(ctx, nullptr, n_trials, ctx->tmp_a.as<double>(), ctx->tmp_b.as<int32_t>(), max_calls,
                              ctx->tmp_c.as<int32_t>(), ctx->tmp_d.as<double>())))
        return rc;
    WC_HIP(hipDeviceSynchronize());
    WC_HIP(hipMemcpy(rec_i, ctx->tmp_c.p, nb * 8, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(rec_f, ctx->tmp_d.p, sizeof(double) * (size_t)n_trials * 2, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_sensitivity_batch_dev(wc_ctx *ctx, void *stream, const wc_reference *ref, const int32_t *base, int64_t n_base,
                             const int64_t *chrom_sizes_host, int n_chrom, const int32_t *plan_host, int64_t n_trials, double threshold,
                             int min_ref_bins, int repeats, double min_effect, const int32_t *chromosomes_host, int n_sel, int max_calls,
                             int32_t *rec_i, double *rec_f, double *calls, int32_t *n_calls) {
    return wc_sensitivity_batch_ex_dev(ctx, stream, ref, base, n_base, chrom_sizes_host, n_chrom, plan_host, n_trials, 0, 0, 0, threshold,
                                       min_ref_bins, repeats, min_effect, chromosomes_host, n_sel, max_calls, rec_i, rec_f, calls, n_calls);
}

}  // extern "C"
