// sensitivity: reproducible Binomial(c, f) per bin, drawn on the device.  Read r of a bin with c reads is
// kept when its 32-bit Philox word (philox.h) is below T = (f << 32) div 1 000 000; the word is word r & 3 of the block
// with counter (bin within its chromosome, chromosome | tag << 16, r >> 2, row id) under the key (seed low, seed high).
// B(c, f) counts the kept reads: a sum of integers, so the order in which blocks are visited cannot show.
//   k_thin_check   tag 1's refusal: the first bin (smallest flat index) with more than 2^24 reads goes to a status word by
//                  atomicMin; the host reads the word before k_thin is launched, so a refused call writes nothing.
//   k_thin<NK>     base [n_base, n_total] -> out [NK, n_base, n_total].  A lane per bin; ONE pass over a bin's blocks
//                  serves all NK depths: every word is compared against every threshold.  A bin below DR_CUT reads is
//                  walked by its lane (neighbouring bins have similar counts: a wave's trip count is its largest); the
//                  bins at and above it are then taken one after another by the whole wave, blocks strided over the 64
//                  lanes and the kept reads summed by a butterfly.  The chromosome of a flat bin is counted from the
//                  offsets (at most WC_MAX_CHROM, cached loads).  Counts below 0 are copied.
//   k_draw_patch   tag 2: the binomial spike.  k_spike first writes the trials' rows as plain copies; this kernel then
//                  rewrites the span's bins alone, a wave per span bin in the strided form, so that one heavy bin cannot
//                  hold a lane: c >= 0 becomes min(2^31 - 1, c * whole + B(c, frac)), whole and frac the quotient and
//                  remainder of (1 000 000 + ppm) by 1 000 000.  Lane 0 stores the bin and counts a clipped one.
//   k_philox       the known-answer kernel: px_block of given counters and keys.
//   k_philox_spin  the rounds alone over registers, for the rate k_thin is held against.
// Nothing synchronises inside a workgroup and no kernel uses LDS; the waves of a workgroup are independent.
#include <limits.h>

#include "philox.h"
#include "spike.h"

namespace {

const int DR_T = 256;                   // lanes per workgroup
const int DR_CUT = 4096;                // reads: at and above, a wave takes the bin together (64 blocks a lane at the least)
const int DR_MAX_KEEP = 8;
const int DR_MAX_READS = 1 << 24;       // thinning: one bin's reads (a wave's 65 536 trips)
const uint32_t DR_TAG_THIN = 1u << 16, DR_TAG_SPIKE = 2u << 16;

struct DrKeep {                         // the thresholds of the depths.  T = 2^32 (f = 1 000 000) is above every word: such a
    uint32_t t[DR_MAX_KEEP];            // depth has its bit in `full` and keeps the count; every other T fits 32 bits, so
    uint32_t full;                      // the 64-bit comparison of the rule is one of 32 bits
};

struct DrTab {                          // ctx->dr_tab
    unsigned long long status;          // k_thin_check: ~0, or the flat index of the first bin beyond DR_MAX_READS
    int off[WC_MAX_CHROM + 1];
};

// kept[k] += the reads of blocks j0, j0 + stride, .. of a bin with c reads whose words are below keep.t[k]
template <int NK>
__device__ __forceinline__ void dr_blocks(uint32_t c0, uint32_t c1, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t c, uint32_t j0,
                                          uint32_t stride, const DrKeep &keep, uint32_t (&kept)[NK]) {
    const uint32_t blocks = (c >> 2) + ((c & 3) != 0);
    for (uint32_t j = j0; j < blocks; j += stride) {
        uint32_t w[4];
        px_block(c0, c1, j, c3, k0, k1, w);
        const uint32_t have = c - 4 * j;            // the block's reads: 1 .. 3 in the last block, else 4 or more
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool real = (uint32_t)q < have;
#pragma unroll
            for (int k = 0; k < NK; ++k) kept[k] += (real && w[q] < keep.t[k]) ? 1u : 0u;
        }
    }
}

template <int NK>
__device__ __forceinline__ void dr_wave_sum(uint32_t (&kept)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
        for (int d = 32; d >= 1; d >>= 1) kept[k] += __shfl_xor(kept[k], d, 64);
}

__global__ __launch_bounds__(DR_T) void k_thin_check(const int *__restrict__ base, long long total, DrTab *__restrict__ tab) {
    const long long i = (long long)blockIdx.x * DR_T + threadIdx.x;
    if (i < total && base[i] > DR_MAX_READS) atomicMin(&tab->status, (unsigned long long)i);
}

template <int NK>
__global__ __launch_bounds__(DR_T) void k_thin(const int *__restrict__ base, long long total, int n_total, const DrTab *__restrict__ tab,
                                               int n_chrom, DrKeep keep, uint32_t k0, uint32_t k1, int *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * DR_T + threadIdx.x;
    const bool live = i < total;                    // (no lane leaves early: the wave's shuffles below need all of them)
    const int c = live ? base[i] : -1;
    const long long row = live ? i / n_total : 0;
    const int j = (int)(i - row * n_total);
    int chrom = 0;
    for (int k = 1; k < n_chrom; ++k) chrom += j >= tab->off[k] ? 1 : 0;
    const uint32_t c0 = (uint32_t)(j - tab->off[chrom]), c1 = (uint32_t)(chrom + 1) | DR_TAG_THIN, c3 = (uint32_t)row;
    uint32_t kept[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) kept[k] = 0;
    if (c > 0 && c < DR_CUT) dr_blocks<NK>(c0, c1, c3, k0, k1, (uint32_t)c, 0, 1, keep, kept);
    unsigned long long tall = __ballot(c >= DR_CUT);
    while (tall) {                                  // (wave-uniform: every lane sees the same mask)
        const int src = __ffsll((long long)tall) - 1;
        tall &= tall - 1;
        uint32_t part[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) part[k] = 0;
        dr_blocks<NK>(__shfl(c0, src, 64), __shfl(c1, src, 64), __shfl(c3, src, 64), k0, k1, (uint32_t)__shfl(c, src, 64), (uint32_t)lane, 64,
                      keep, part);
        dr_wave_sum<NK>(part);
        if (lane == src) {
#pragma unroll
            for (int k = 0; k < NK; ++k) kept[k] = part[k];
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < NK; ++k) out[(long long)k * total + i] = c < 0 || ((keep.full >> k) & 1u) ? c : (int)kept[k];
}

// a wave per span bin: blockIdx.x the trial, the workgroup's four waves and gridDim.y stride over the span
__global__ __launch_bounds__(DR_T) void k_draw_patch(const int *__restrict__ base, long long n_total, const SpRow *__restrict__ rows,
                                                     uint32_t trial0, uint32_t k0, uint32_t k1, int *__restrict__ out,
                                                     unsigned long long *__restrict__ saturated) {
    const int lane = threadIdx.x & 63;
    const long long t = blockIdx.x;
    const SpRow row = rows[t];
    const int span = row.hi - row.lo;               // 0: a control trial
    const uint32_t m = (uint32_t)(1000000 + row.ppm), whole = m / 1000000u, frac = m % 1000000u;
    DrKeep keep;
    keep.t[0] = (uint32_t)px_threshold(frac);       // (frac < 1 000 000: T is below 2^32)
    for (int sb = (int)blockIdx.y * (DR_T / 64) + (threadIdx.x >> 6); sb < span; sb += (int)gridDim.y * (DR_T / 64)) {
        const int c = base[row.src + row.lo + sb];
        if (c < 0) continue;                        // (the copy stands)
        uint32_t kept[1] = {0};
        if (frac) {
            dr_blocks<1>((uint32_t)(row.first + sb), (uint32_t)row.chrom | DR_TAG_SPIKE, trial0 + (uint32_t)t, k0, k1, (uint32_t)c,
                         (uint32_t)lane, 64, keep, kept);
            dr_wave_sum<1>(kept);
        }
        if (lane == 0) {
            const unsigned long long v = (unsigned long long)c * whole + kept[0];
            out[t * n_total + row.lo + sb] = v > 2147483647ull ? INT_MAX : (int)v;
            if (v > 2147483647ull && saturated) atomicAdd(saturated, 1ull);
        }
    }
}

__global__ __launch_bounds__(DR_T) void k_philox(const uint32_t *__restrict__ counters, const uint32_t *__restrict__ keys, long long n,
                                                 uint32_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * DR_T + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4];
    px_block(counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3], keys[2 * i], keys[2 * i + 1], w);
    for (int q = 0; q < 4; ++q) out[4 * i + q] = w[q];
}

// the rounds alone: every lane runs `blocks` blocks over registers and stores the exclusive-or of their words (the store keeps
// the loop alive); what k_thin's rate is held against (tools/gpu_sensitivity_depth_time.py)
__global__ __launch_bounds__(DR_T) void k_philox_spin(uint32_t blocks, uint32_t k0, uint32_t k1, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * DR_T + threadIdx.x;
    uint32_t acc = 0;
    for (uint32_t j = 0; j < blocks; ++j) {
        uint32_t w[4];
        px_block(i, DR_TAG_THIN, j, 0, k0, k1, w);
        acc ^= w[0] ^ w[1] ^ w[2] ^ w[3];
    }
    out[i] = acc;
}

// ---- the host's half ----------------------------------------------------------------------------------------------------
int dr_offsets(const char *who, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, DrTab &tab, int64_t *n_total) {
    WC_CHECK(n_base >= 1 && n_base <= INT_MAX, WC_E_ARG, "%s: %lld base rows", who, (long long)n_base);
    WC_CHECK(n_chrom >= 1 && n_chrom <= WC_MAX_CHROM, WC_E_ARG, "%s: %d chromosomes (1 .. %d)", who, n_chrom, WC_MAX_CHROM);
    int64_t off = 0;
    tab.off[0] = 0;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_sizes[c] >= 0 && chrom_sizes[c] <= INT_MAX - 8 - off, WC_E_ARG, "%s: chromosome %d has %lld bins (a row holds fewer than 2^31)",
                 who, c + 1, (long long)chrom_sizes[c]);
        off += chrom_sizes[c];
        tab.off[c + 1] = (int)off;
    }
    WC_CHECK(off >= 1, WC_E_ARG, "%s: a row without bins", who);
    *n_total = off;
    return WC_OK;
}

int dr_keep(const char *who, const int32_t *keep_ppm, int n_keep, DrKeep &keep) {
    WC_CHECK(keep_ppm && n_keep >= 1 && n_keep <= DR_MAX_KEEP, WC_E_ARG, "%s: %d depths (1 .. %d), or no keep_ppm", who, n_keep, DR_MAX_KEEP);
    for (int k = 0; k < DR_MAX_KEEP; ++k) keep.t[k] = 0;
    keep.full = 0;
    for (int k = 0; k < n_keep; ++k) {
        WC_CHECK(keep_ppm[k] >= 1 && keep_ppm[k] <= 1000000, WC_E_ARG, "%s: depth %d keeps %d ppm (1 .. 1000000)", who, k, keep_ppm[k]);
        if (keep_ppm[k] == 1000000) keep.full |= 1u << k;
        else keep.t[k] = (uint32_t)px_threshold((uint32_t)keep_ppm[k]);
    }
    return WC_OK;
}

template <int NK>
void dr_thin_launch(hipStream_t stream, const int32_t *base, long long total, int n_total, const DrTab *tab, int n_chrom, const DrKeep &keep,
                    uint64_t seed, int32_t *out) {
    hipLaunchKernelGGL(k_thin<NK>, dim3((unsigned)((total + DR_T - 1) / DR_T)), dim3(DR_T), 0, stream, (const int *)base, total, n_total, tab,
                       n_chrom, keep, (uint32_t)seed, (uint32_t)(seed >> 32), (int *)out);
}

// the check, its read-back (the one wait of the call) and the thinning of DEVICE rows; tab and keep are checked already
int dr_thin(wc_ctx *ctx, hipStream_t stream, const int32_t *base, int64_t n_base, int64_t n_total, int n_chrom, DrTab &tab, const DrKeep &keep,
            int n_keep, uint64_t seed, int32_t *out) {
    const long long total = n_base * n_total;
    WC_CHECK(total <= (long long)INT_MAX * DR_T, WC_E_LIMIT, "thin: %lld bins in one call", total);
    int rc;
    if ((rc = ctx->dr_tab.reserve(sizeof(DrTab)))) return rc;
    tab.status = ~0ull;
    WC_HIP(hipMemcpyAsync(ctx->dr_tab.p, &tab, sizeof(DrTab), hipMemcpyHostToDevice, stream));
    DrTab *dev = ctx->dr_tab.as<DrTab>();
    hipLaunchKernelGGL(k_thin_check, dim3((unsigned)((total + DR_T - 1) / DR_T)), dim3(DR_T), 0, stream, (const int *)base, total, dev);
    WC_HIP(hipGetLastError());
    unsigned long long status = 0;
    WC_HIP(hipMemcpyAsync(&status, &dev->status, sizeof(status), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    WC_CHECK(status == ~0ull, WC_E_LIMIT, "thin: base row %lld, bin %lld has more than %d reads", (long long)(status / (unsigned long long)n_total),
             (long long)(status % (unsigned long long)n_total), DR_MAX_READS);
    // (an instance per width: a wider one would spend compares on depths nobody asked for)
    switch (n_keep) {
    case 1: dr_thin_launch<1>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 2: dr_thin_launch<2>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 3: dr_thin_launch<3>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 4: dr_thin_launch<4>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 5: dr_thin_launch<5>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 6: dr_thin_launch<6>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    case 7: dr_thin_launch<7>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    default: dr_thin_launch<8>(stream, base, total, (int)n_total, dev, n_chrom, keep, seed, out); break;
    }
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int dr_draw_args(const char *who, int draw, int64_t trial0, int64_t n_trials) {
    WC_CHECK(draw == 0 || draw == 1, WC_E_ARG, "%s: draw = %d (0 or 1)", who, draw);
    WC_CHECK(trial0 >= 0 && trial0 + n_trials <= 4294967296ll, WC_E_ARG, "%s: trial0 = %lld with %lld trials (row ids are 32 bits)", who,
             (long long)trial0, (long long)n_trials);
    return WC_OK;
}

// the checked rows to the device and the trials' rows to `out`: the deterministic rule (draw == 0: k_spike as it always ran) or
// the copy and the patch.  ctx->sp_plan begins with the rows as the score reads them in either case.
int dr_spike(wc_ctx *ctx, hipStream_t stream, const int32_t *base, int64_t n_total, std::vector<SpRow> &rows, int draw, uint64_t seed,
             int64_t trial0, int32_t *out, unsigned long long *saturated_dev) {
    const int64_t n = (int64_t)rows.size();
    int rc;
    if (!draw) {
        if ((rc = sp_upload(ctx, stream, rows))) return rc;
        return sp_spike_launch(ctx, stream, base, n_total, n, out, saturated_dev);
    }
    int max_span = 0;
    rows.resize((size_t)(2 * n));
    for (int64_t i = 0; i < n; ++i) {               // the second half: the same rows as controls, which k_spike copies
        SpRow r = rows[(size_t)i];
        max_span = std::max(max_span, r.hi - r.lo);
        r.lo = r.hi = 0;
        rows[(size_t)(n + i)] = r;
    }
    if ((rc = sp_upload(ctx, stream, rows)) || (rc = sp_spike_launch(ctx, stream, base, n_total, n, out, saturated_dev, (size_t)n))) return rc;
    if (max_span == 0) return WC_OK;
    const int per = DR_T / 64;
    const dim3 grid((unsigned)n, (unsigned)std::min((max_span + per - 1) / per, 1024));
    hipLaunchKernelGGL(k_draw_patch, grid, dim3(DR_T), 0, stream, (const int *)base, (long long)n_total, (const SpRow *)ctx->sp_plan.as<SpRow>(),
                       (uint32_t)trial0, (uint32_t)seed, (uint32_t)(seed >> 32), (int *)out, saturated_dev);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_thin_wave_cutoff(void) { return DR_CUT; }

int wc_philox4x32_host(const uint32_t *counters, const uint32_t *keys, int64_t n, uint32_t *out) {
    WC_CHECK(counters && keys && out && n >= 0, WC_E_ARG, "philox: NULL argument or n = %lld", (long long)n);
    for (int64_t i = 0; i < n; ++i)
        px_block(counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3], keys[2 * i], keys[2 * i + 1], out + 4 * i);
    return WC_OK;
}

int wc_philox4x32(wc_ctx *ctx, const uint32_t *counters, const uint32_t *keys, int64_t n, uint32_t *out) {
    WC_CHECK(ctx && counters && keys && out && n >= 1, WC_E_ARG, "philox: NULL argument or n = %lld", (long long)n);
    WC_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->tmp_a.reserve(16 * (size_t)n)) || (rc = ctx->tmp_b.reserve(8 * (size_t)n)) || (rc = ctx->tmp_c.reserve(16 * (size_t)n))) return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, counters, 16 * (size_t)n, hipMemcpyHostToDevice));
    WC_HIP(hipMemcpy(ctx->tmp_b.p, keys, 8 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_philox, dim3((unsigned)((n + DR_T - 1) / DR_T)), dim3(DR_T), 0, nullptr, (const uint32_t *)ctx->tmp_a.as<uint32_t>(),
                       (const uint32_t *)ctx->tmp_b.as<uint32_t>(), (long long)n, ctx->tmp_c.as<uint32_t>());
    WC_HIP(hipGetLastError());
    WC_HIP(hipDeviceSynchronize());
    WC_HIP(hipMemcpy(out, ctx->tmp_c.p, 16 * (size_t)n, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_philox_spin_dev(wc_ctx *ctx, void *stream_, int64_t lanes, int64_t blocks, uint64_t seed, uint32_t *out) {
    WC_CHECK(ctx && out && lanes >= DR_T && lanes % DR_T == 0 && lanes <= (1ll << 30) && blocks >= 0 && blocks <= (1ll << 24), WC_E_ARG,
             "philox spin: %lld lanes (a multiple of %d, at most 2^30) x %lld blocks (at most 2^24), or no output", (long long)lanes, DR_T,
             (long long)blocks);
    WC_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_philox_spin, dim3((unsigned)(lanes / DR_T)), dim3(DR_T), 0, (hipStream_t)stream_, (uint32_t)blocks, (uint32_t)seed,
                       (uint32_t)(seed >> 32), out);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int wc_thin_counts_dev(wc_ctx *ctx, void *stream_, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                       const int32_t *keep_ppm_host, int n_keep, uint64_t seed, int32_t *out) {
    WC_CHECK(ctx && base && out && chrom_sizes_host, WC_E_ARG, "thin: NULL argument");
    DrTab tab;
    DrKeep keep;
    int64_t n_total = 0;
    int rc;
    if ((rc = dr_offsets("thin", n_base, chrom_sizes_host, n_chrom, tab, &n_total)) || (rc = dr_keep("thin", keep_ppm_host, n_keep, keep))) return rc;
    WC_CHECK(((uintptr_t)base & 3) == 0 && ((uintptr_t)out & 3) == 0, WC_E_ARG, "thin: counts not aligned to four bytes");
    WC_HIP(hipSetDevice(ctx->device));
    return dr_thin(ctx, (hipStream_t)stream_, base, n_base, n_total, n_chrom, tab, keep, n_keep, seed, out);
}

int wc_thin_counts(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *keep_ppm, int n_keep,
                   uint64_t seed, int32_t *out) {
    WC_CHECK(ctx && base && out && chrom_sizes, WC_E_ARG, "thin: NULL argument");
    DrTab tab;
    DrKeep keep;
    int64_t n_total = 0;
    int rc;
    if ((rc = dr_offsets("thin", n_base, chrom_sizes, n_chrom, tab, &n_total)) || (rc = dr_keep("thin", keep_ppm, n_keep, keep))) return rc;
    WC_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = sizeof(int32_t) * (size_t)(n_base * n_total), out_bytes = in_bytes * (size_t)n_keep;
    if ((rc = ctx->tmp_a.reserve(in_bytes)) || (rc = ctx->tmp_b.reserve(out_bytes))) return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, base, in_bytes, hipMemcpyHostToDevice));
    if ((rc = dr_thin(ctx, nullptr, ctx->tmp_a.as<int32_t>(), n_base, n_total, n_chrom, tab, keep, n_keep, seed, ctx->tmp_b.as<int32_t>()))) return rc;
    WC_HIP(hipDeviceSynchronize());
    WC_HIP(hipMemcpy(out, ctx->tmp_b.p, out_bytes, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_spike_counts_ex_dev(wc_ctx *ctx, void *stream_, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                           const int32_t *plan_host, int64_t n_trials, int draw, uint64_t seed, int64_t trial0, int32_t *out, int64_t *saturated) {
    WC_CHECK(ctx && base && out && chrom_sizes_host, WC_E_ARG, "spike: NULL argument");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<SpRow> rows;
    int64_t n_total = 0;
    int rc;
    if ((rc = sp_rows("spike", plan_host, n_trials, n_base, chrom_sizes_host, n_chrom, rows, &n_total)) ||
        (rc = dr_draw_args("spike", draw, trial0, n_trials)))
        return rc;
    WC_HIP(hipSetDevice(ctx->device));
    return dr_spike(ctx, stream, base, n_total, rows, draw, seed, trial0, out, (unsigned long long *)saturated);
}

int wc_spike_counts_ex(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *plan,
                       int64_t n_trials, int draw, uint64_t seed, int64_t trial0, int32_t *out, int64_t *saturated) {
    WC_CHECK(ctx && base && out && chrom_sizes, WC_E_ARG, "spike: NULL argument");
    std::vector<SpRow> rows;
    int64_t n_total = 0;
    int rc;
    if ((rc = sp_rows("spike", plan, n_trials, n_base, chrom_sizes, n_chrom, rows, &n_total)) || (rc = dr_draw_args("spike", draw, trial0, n_trials)))
        return rc;
    WC_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = sizeof(int32_t) * (size_t)(n_base * n_total), out_bytes = sizeof(int32_t) * (size_t)(n_trials * n_total);
    if ((rc = ctx->tmp_a.reserve(in_bytes)) || (rc = ctx->tmp_b.reserve(out_bytes)) || (rc = ctx->tmp_c.reserve(8))) return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, base, in_bytes, hipMemcpyHostToDevice));
    if ((rc = dr_spike(ctx, nullptr, ctx->tmp_a.as<int32_t>(), n_total, rows, draw, seed, trial0, ctx->tmp_b.as<int32_t>(),
                       ctx->tmp_c.as<unsigned long long>())))
        return rc;
    WC_HIP(hipDeviceSynchronize());
    WC_HIP(hipMemcpy(out, ctx->tmp_b.p, out_bytes, hipMemcpyDeviceToHost));
    if (saturated) WC_HIP(hipMemcpy(saturated, ctx->tmp_c.p, 8, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_sensitivity_batch_ex_dev(wc_ctx *ctx, void *stream_, const wc_reference *ref, const int32_t *base, int64_t n_base,
                                const int64_t *chrom_sizes_host, int n_chrom, const int32_t *plan_host, int64_t n_trials, int draw, uint64_t seed,
                                int64_t trial0, double threshold, int min_ref_bins, int repeats, double min_effect,
                                const int32_t *chromosomes_host, int n_sel, int max_calls, int32_t *rec_i, double *rec_f, double *calls,
                                int32_t *n_calls) {
    WC_CHECK(ctx && ref && base && chrom_sizes_host && rec_i && rec_f, WC_E_ARG, "sensitivity: NULL argument");
    WC_CHECK(max_calls >= 1 && n_sel >= 0, WC_E_ARG, "sensitivity: max_calls = %d, %d chromosomes selected", max_calls, n_sel);
    WC_CHECK(n_trials <= 60000 && n_trials * std::max(n_sel, 1) <= 60000, WC_E_LIMIT,
             "sensitivity: trials x chromosomes = %lld exceeds 60000 per call; split the plan", (long long)(n_trials * std::max(n_sel, 1)));
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<SpRow> rows;
    int64_t n_total = 0;
    int rc;
    if ((rc = sp_rows("sensitivity", plan_host, n_trials, n_base, chrom_sizes_host, n_chrom, rows, &n_total)) ||
        (rc = dr_draw_args("sensitivity", draw, trial0, n_trials)))
        return rc;
    WC_HIP(hipSetDevice(ctx->device));
    TestState &ts = ctx->ts;
    // the spiked rows and everything the test writes besides the calls live in the workspaces of the host-array test
    if ((rc = ts.counts.reserve(sizeof(int32_t) * (size_t)(n_trials * n_total))) ||
        (rc = ts.res_z.reserve(sizeof(double) * (size_t)(n_trials * n_total))) ||
        (rc = ts.res_r.reserve(sizeof(double) * (size_t)(n_trials * n_total))) ||
        (rc = ts.cwz.reserve(sizeof(double) * (size_t)(n_trials * std::max(n_sel, 1)))) || (rc = ts.n.reserve(sizeof(double) * (size_t)n_trials)))
        return rc;
    if (!calls) {
        if ((rc = ts.calls.reserve(sizeof(double) * (size_t)n_trials * max_calls * 5))) return rc;
        calls = ts.calls.as<double>();
    }
    if (!n_calls) {
        if ((rc = ts.n_calls.reserve(sizeof(int32_t) * (size_t)n_trials))) return rc;
        n_calls = ts.n_calls.as<int32_t>();
    }
    if ((rc = dr_spike(ctx, stream, base, n_total, rows, draw, seed, trial0, ts.counts.as<int32_t>(), nullptr))) return rc;
    if ((rc = wc_test_batch_dev(ctx, stream_, ref, ts.counts.as<int32_t>(), n_trials, threshold, min_ref_bins, repeats, min_effect,
                                chromosomes_host, n_sel, max_calls, ts.res_z.as<double>(), ts.res_r.as<double>(), ts.cwz.as<double>(), calls,
                                n_calls, ts.n.as<double>())))
        return rc;
    return sp_score_launch(ctx, stream, n_trials, calls, n_calls, max_calls, rec_i, rec_f);
}

}  // extern "C"
