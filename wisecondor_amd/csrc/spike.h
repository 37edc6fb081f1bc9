// What spike.hip and draw.hip share: the checked plan row and the host helpers that check, upload and launch.
#pragma once
#include <vector>

#include "ctx.h"

struct SpRow {                          // 32 bytes: a checked plan row as the kernels read it
    long long src;                      // the base row's first element
    int lo, hi;                         // the span as flat bins of a row, hi exclusive (lo == hi: a control trial)
    int ppm, chrom, first, bins;        // chrom 1-based
};
static_assert(sizeof(SpRow) == 32, "a plan row is two 16-byte loads");

// every plan row checked (the first bad one named) and turned into a SpRow; chrom_sizes == NULL: the score's checks alone
int sp_rows(const char *who, const int32_t *plan, int64_t n_trials, int64_t n_base, const int64_t *chrom_sizes, int n_chrom,
            std::vector<SpRow> &rows, int64_t *n_total_out);
// rows to ctx->sp_plan (a pageable source: the call returns with the rows read)
int sp_upload(wc_ctx *ctx, hipStream_t stream, const std::vector<SpRow> &rows);
// k_spike over the n_trials rows that begin at row `slot` of ctx->sp_plan
int sp_spike_launch(wc_ctx *ctx, hipStream_t stream, const int32_t *base, int64_t n_total, int64_t n_trials, int32_t *out,
                    unsigned long long *saturated_dev, size_t slot = 0);
int sp_score_launch(wc_ctx *ctx, hipStream_t stream, int64_t n_trials, const double *calls, const int32_t *n_calls, int max_calls,
                    int32_t *rec_i, double *rec_f);
