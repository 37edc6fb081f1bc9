// The host's half that export.hip and tracks.hip share (the kernels' half is tile_text.h): the checks of a call's
// arguments, the working memory of the three launches, and the entry that takes HOST arrays.  A file brings its table
// (make_tab, bound_of) and its three launches as a callable
//     launch(stream, work, call, mid)
// on a call whose pointers are DEVICE memory: the length kernel, the scan kernel, `mid` recorded where it is not NULL,
// the bytes kernel.
#pragma once
#include "ctx.h"
#include "tile_text.h"

namespace wc {

struct TextWork {                       // the call's working memory and grid
    uint4 *slots;                       // 16 bytes per value: its digits between the two passes
    void *sums;                         // per tile, sum_size bytes: what the length kernel leaves the scan
    long long *tile_off;
    long long n_tiles;
    dim3 grid;                          // (tiles, rows)
};

struct TextRows {                       // a call as both files' entries take it
    const char *name, *unit;            // the messages' words: "json" / "values", "bedgraph" / "bins"
    wc_ctx *ctx;
    const double *rows;
    int64_t row_stride, n_rows;
    unsigned char *text;
    int64_t text_stride;
    int n_counts;                       // per-row int64 counters the scan leaves: text_len, and with 2 one more
    int64_t *counts[2];

    int begin() const {
        WC_CHECK(ctx && n_rows >= 0, WC_E_ARG, "%s: unusable argument (%lld rows)", name, (long long)n_rows);
        return WC_OK;
    }

    // behind the file's make_tab.  total: values of a row; dev: the _dev form, whose kernels store whole 16-byte lines
    int check(int64_t total, int64_t bound, bool dev) const {
        WC_CHECK(n_rows <= 65535, WC_E_LIMIT, "%s: %lld rows in one call (at most 65535); split the batch", name, (long long)n_rows);
        WC_CHECK(row_stride >= total && (rows || total == 0 || n_rows == 0), WC_E_ARG, "%s: rows %lld values apart hold %lld %s", name,
                 (long long)row_stride, (long long)total, unit);
        WC_CHECK(n_rows == 0 || (counts[0] && (n_counts < 2 || counts[1]) && (text || bound == 0)), WC_E_ARG, "%s: NULL output", name);
        WC_CHECK(text_stride >= bound, WC_E_ARG, "%s: %lld bytes per text row, wc_%s_row_bound is %lld", name, (long long)text_stride, name,
                 (long long)bound);
        WC_CHECK(!dev || (text_stride % 16 == 0 && ((uintptr_t)text & 15) == 0), WC_E_ARG,
                 "%s: text rows %lld bytes apart (a multiple of 16, from an address that is one)", name, (long long)text_stride);
        return WC_OK;
    }

    // the three kernels, enqueued (this call's pointers are DEVICE memory); ev (may be NULL): [0] in front, [1] behind
    // the scan, [2] behind the bytes
    template <class Launch> int enqueue(hipStream_t stream, int64_t total, size_t sum_size, hipEvent_t *ev, Launch launch) const {
        if (n_rows == 0) return WC_OK;
        WC_HIP(hipSetDevice(ctx->device));
        const int64_t n_tiles = total > 0 ? (total + TT_T - 1) / TT_T : 1;
        int rc;
        // the slots | the tiles' sums | their offsets (one call in flight per context)
        const size_t slot_bytes = (size_t)n_rows * (size_t)total * 16, sum_bytes = ((size_t)n_rows * n_tiles * sum_size + 15) & ~(size_t)15;
        if ((rc = ctx->js_slots.reserve(slot_bytes + 16)) || (rc = ctx->js_tiles.reserve(sum_bytes + (size_t)n_rows * n_tiles * 8))) return rc;
        const TextWork work = {ctx->js_slots.as<uint4>(), ctx->js_tiles.p,
                               reinterpret_cast<long long *>(ctx->js_tiles.as<unsigned char>() + sum_bytes), (long long)n_tiles,
                               dim3((unsigned)n_tiles, (unsigned)n_rows)};
        if (ev) WC_HIP(hipEventRecord(ev[0], stream));
        if ((rc = launch(stream, work, *this, ev ? ev[1] : nullptr))) return rc;
        if (ev) WC_HIP(hipEventRecord(ev[2], stream));
        return WC_OK;
    }

    // The same for a call whose pointers are HOST memory, synchronising: only counts[0][i] bytes of a row are copied,
    // and a length outside min_len .. bound is WC_E_INTERNAL.  times_ms (may be NULL) [4]: copy in, lengths and scan,
    // bytes, copy out.
    template <class Launch>
    int stage(int64_t total, int64_t bound, int64_t min_len, size_t sum_size, double *times_ms, Launch launch) const {
        if (times_ms)
            for (int i = 0; i < 4; ++i) times_ms[i] = 0.0;
        if (n_rows == 0) return WC_OK;
        WC_HIP(hipSetDevice(ctx->device));
        const int64_t dev_stride = (bound + 15) / 16 * 16;
        const size_t in_bytes = ((size_t)(n_rows - 1) * row_stride + (size_t)total) * 8;
        int rc;
        if ((rc = ctx->tmp_a.reserve(in_bytes + 16)) || (rc = ctx->tmp_b.reserve((size_t)n_rows * dev_stride + 16)) ||
            (rc = ctx->tmp_c.reserve((size_t)n_rows * 16)))
            return rc;
        Events<5> events;
        hipEvent_t *ev = events.e;
        if (times_ms && (rc = events.create())) return rc;
        if (times_ms) (void)hipEventRecord(ev[3], nullptr);
        if (in_bytes) WC_HIP(hipMemcpy(ctx->tmp_a.p, rows, in_bytes, hipMemcpyHostToDevice));
        int64_t *d_counts = ctx->tmp_c.as<int64_t>();
        const TextRows dev = {name, unit, ctx, ctx->tmp_a.as<double>(), row_stride, n_rows, ctx->tmp_b.as<unsigned char>(), dev_stride,
                              n_counts, {d_counts, d_counts + n_rows}};
        if ((rc = dev.enqueue(nullptr, total, sum_size, times_ms ? ev : nullptr, launch))) return rc;
        for (int k = 0; k < n_counts; ++k) WC_HIP(hipMemcpy(counts[k], dev.counts[k], (size_t)n_rows * 8, hipMemcpyDeviceToHost));
        const int64_t *text_len = counts[0];
        for (int64_t i = 0; i < n_rows; ++i) {
            WC_CHECK(text_len[i] >= min_len && text_len[i] <= bound, WC_E_INTERNAL, "%s: a row of %lld bytes, the bound is %lld", name,
                     (long long)text_len[i], (long long)bound);
            if (text_len[i]) WC_HIP(hipMemcpy(text + i * text_stride, dev.text + i * dev_stride, (size_t)text_len[i], hipMemcpyDeviceToHost));
        }
        if (times_ms) {
            (void)hipEventRecord(ev[4], nullptr);
            (void)hipEventSynchronize(ev[4]);
            const int from[4] = {3, 0, 1, 2}, to[4] = {0, 1, 2, 4};
            events.elapsed(4, from, to, times_ms);
        }
        return WC_OK;
    }
};

}  // namespace wc
