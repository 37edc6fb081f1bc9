// Per-device context: cached workspaces for the newref and test paths.
#pragma once
#include "common.h"

#define WC_MAX_CHROM 64

struct NewrefState {
    // problem
    int64_t n_bins = 0, n_samples = 0;
    int64_t bins_pad = 0;   // rows padded to the 128-row tile
    int64_t k_pad16 = 0;    // samples padded to the 64-wide float16 k-slab of the threshold tiles
    int n_chrom = 0, k = 0, sum_order = 0;
    int64_t chrom_off[WC_MAX_CHROM + 1] = {0};
    const double *corrected = nullptr;  // device, caller owned
    // tuning
    int64_t n_sample_cols = 0;      // M, multiple of 128
    int64_t cap = 0;                // candidate-list capacity per row
    int64_t expect = 0;             // expected candidates per row under the sampled threshold
    float beta = 0.f;               // relative half-width of the key error interval
    bool prepared = false;
    double tau = 0.0;               // weight of the float16 representation-error split (k_convert)
    // device buffers
    wc::DevBuf col_partial, col_mean, norm_lo, norm_hi, chrom_of_row, chrom_range, chrom_off_dev;
    wc::DevBuf sample_rows, sample_slot, s32, s_norm_lo, s_chrom, s_range, a16, s16;
    wc::DevBuf keys1, thr, cnt, list, tiles;
    wc::DevBuf fb_rows, fb_count, fb_scratch, stats, tiles0, pw_prog, pairs, x64, m2;
    bool fb_dirty = true;       // fb_count holds a finished pass's counts (k_convert zeroes it for the next job)
    // m2[1 + bad_slot] is the smallest norm among the rows with a clamped value (+inf: none) of the prepared job;
    // bad_spare_clean: the other slot holds +inf, left there by the one-launch prepare for the prepare after it
    int bad_slot = 0;
    bool bad_spare_clean = false;
    int64_t s_pad = 0;      // samples padded to whole 16-sample chunks (x64 row stride)
    bool exact_only = false; // refsize beyond the candidate lists' design size: every row takes the exact path
    wc::DevBuf cand_word;    // per row: row | slack code << index_bits, the low word of the row's entries in other rows' lists
    int index_bits = 17;     // bits of the row number in a candidate word (prepare: max(17, what bins_pad needs))
    int index_bits_req = 0;  // wc_newref_set_index_bits: 0 = automatic
    bool x64_pad = false;   // the padded float64 image exists (pair engine usable)
    int pw_leaves = 0;
    int64_t pw_for = -1;
    // host-side caches so that repeated calls on the same layout enqueue kernels only
    std::vector<int64_t> sample_key, tiles0_key, tiles1_key, chrom_key;
    int64_t tiles0_n = 0, tiles1_n = 0;
};

// Workspaces of the batched test path (grow-only, reused across calls).
struct TestState {
    std::vector<int> sel_host;      // chromosome selection currently held by `sel`
    wc::DevBuf counts, totals, raw, proj, data, xt, xc, zt, rt, nt, sdt, z, r, n, sd_avg;
    wc::DevBuf zc, rc, gpos, regions, sel;
    wc::DevBuf res_z, res_r, cwz, calls, n_calls;
    // Stouffer search
    wc::DevBuf zs, rs2, ns2, sds, sub, tmin, tmax, tmin2, tmax2, cell_state, cell_rec, prefix, reg_abs, reg_flag, rs, jobs_a, jobs_b, job_cnt, partial, cbound, cuts, job_res, hot, cand, cand_cnt;
    wc::DevBuf seg, out_val, out_x, out_y, out_n, whole, effect, misc, misc2, reduce_tmp, win_bits, bit_off, pairs_a, pairs_b, cut_vals;
    wc::DevBuf walk_hot;             // k_seg_walk's early starters: [0] count, [16 ..] the list, [16 + 4096 ..] every region's place in it
    int64_t rs_len = 0;
    // latency mode: the captured call (hipGraph), the arguments it was captured for, and whether
    // an eager call of that shape has sized the workspaces
    hipGraphExec_t lat_exec = nullptr;
    std::vector<int64_t> lat_key, lat_fail_key;   // lat_fail_key: a shape whose capture failed stays on the eager latency kernels
    bool lat_warm = false;
    unsigned long long lat_epoch = 0;   // wc::realloc_epoch() at capture time
    // optional stage timing of wc_test_batch_dev (wc_test_profile): events on the launch stream
    // between the stages, and counts of the window evaluations the search kernels executed
    bool profile = false;
    std::vector<hipEvent_t> prof_ev;    // event pool, grown on demand
    std::vector<int> prof_tag;          // tag of every mark of the last batch, in record order
    wc::DevBuf sd_fail;                 // per-sample flags of k_sd_fast (1: the serial kernel takes the sample)
    wc::DevBuf prof_work;               // u64[2]: windows evaluated by k_seg_search, evaluations by k_seg_quiet
    void mark(int tag, hipStream_t stream) {
        if (!profile) return;
        const size_t at = prof_tag.size();
        if (at >= prof_ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return;
            prof_ev.push_back(e);
        }
        if (hipEventRecord(prof_ev[at], stream) == hipSuccess) prof_tag.push_back(tag);
    }
};

// state carried from wc_newref_prep_gram to wc_newref_prep_finish.  The arrays are the prep step's own: no other
// entry point writes them, so _eig and _finish* compute from what _gram left whatever ran on the context in between.
struct PrepState {
    int64_t S = 0, Btot = 0, B = 0;
    bool ready = false;
    wc::DevBuf eig_ws;          // eigh.hip: working copy, reflectors, tridiagonal, vectors
    wc::DevBuf counts, totals, sel;     // the counts [S, Btot], the samples' totals, the kept bins' places
    wc::DevBuf raw, data, xt, xc;       // maskedData [B, S]; tdata, centred and corrected_t [S, B]
    wc::DevBuf z;                       // Gram matrix [S, S] | scaled eigenvectors [8, S] | components [8, B] | mean [B]
    wc::DevBuf proj;                    // projection [S, 8]
    wc::DevBuf misc, zt;                // the Gram tiles' list; their slices' partial tiles
};

// workspaces of `convert` (convert.hip): the small tables, the per-tile words, the kept positions, and in paired mode
// the class byte of every read
struct ConvertState {
    wc::DevBuf tab, tiles, kpos, cls;
};

struct wc_ctx {
    int device = 0;
    PrepState prep;
    ConvertState cv;
    NewrefState nr;
    TestState ts;
    wc::DevBuf tmp_a, tmp_b, tmp_c, tmp_d;  // host-pointer API staging
    wc::DevBuf df_scratch, df_meta;         // deflate.hip: the blocks' slots before they are gathered; their lengths and CRC shares
    wc::DevBuf js_slots, js_tiles;          // export.hip: the values' decimal digits between the passes; the tiles' sums and offsets
    wc::DevBuf sp_plan;                     // spike.hip: the checked plan rows of the call in flight
    wc::DevBuf dr_tab;                      // draw.hip: the thinning's status word and chromosome offsets
    wc::DevBuf cx_tab, cx_prefix, cx_rows;  // crossval.hip: the call's tables and status word; the prefix sums P; tested values per row
    // plot.hip: display lists and their counts, the small tables of a call (and the host block they are copied from),
    // the scanline images, the Adler-32 block sums, the status word
    wc::DevBuf pl_list, pl_counts, pl_tab, pl_img, pl_part, pl_status;
    // the tables' host block is pinned, so its copy is truly asynchronous; pl_sent is recorded behind that copy and
    // waited for before the block is written again (it waits for the small copy only, not for the call's kernels)
    unsigned char *pl_host = nullptr;
    size_t pl_host_bytes = 0;
    hipEvent_t pl_sent = nullptr;
    int pl_host_reserve(size_t bytes) {
        if (!pl_sent) WC_HIP(hipEventCreateWithFlags(&pl_sent, hipEventDisableTiming));
        else WC_HIP(hipEventSynchronize(pl_sent));
        if (bytes <= pl_host_bytes) return WC_OK;
        if (pl_host) (void)hipHostFree(pl_host);
        pl_host = nullptr;
        pl_host_bytes = 0;
        const size_t ask = bytes + (bytes >> 1) + 256;
        WC_HIP(hipHostMalloc((void **)&pl_host, ask, hipHostMallocDefault));
        pl_host_bytes = ask;
        return WC_OK;
    }
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    int64_t last_stats[8] = {0};
    // side stream for work that only feeds an output (overlaps with the main stream)
    hipStream_t lat_stream = nullptr;      // latency-mode calls of the test path run (and are captured) here
    hipEvent_t ev_lat_in = nullptr, ev_lat_out = nullptr;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_pending = false;
    hipStream_t side2 = nullptr;           // big batches: the inflated arrays and the whole-region values beside stdDevAvg, not behind it
    hipEvent_t ev_join2 = nullptr;
    bool side2_pending = false;
    bool side_fresh = false;               // the side stream was forked from the launch stream and NOTHING has been enqueued on the
                                           // launch stream since: the next side_begin needs no second event record + wait
    // small pinned host block for count read-backs (a pageable destination costs a staged copy).  The latency-mode
    // graph of the test path bakes this block's address in (k_assemble_calls' host_status), so a block that moves
    // counts as a reallocation like a DevBuf's: whoever cached the address compares wc::realloc_epoch().
    int ensure_pinned(size_t bytes) {
        if (pinned_bytes >= bytes) return WC_OK;
        ++wc::realloc_epoch();
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
        pinned_bytes = 0;
        WC_HIP(hipHostMalloc(&pinned, bytes, hipHostMallocDefault));
        pinned_bytes = bytes;
        return WC_OK;
    }
    int ensure_side_stream() {
        if (side) return WC_OK;
        // lowest priority: what runs here only feeds outputs (stdDevAvg, the inflated arrays, whole-region values) and
        // must not take CUs from the launch stream's critical path
        int prio_least = 0, prio_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_least = 0;
        WC_HIP(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio_least));
        WC_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        WC_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        WC_HIP(hipStreamCreateWithPriority(&side2, hipStreamNonBlocking, prio_least));
        WC_HIP(hipEventCreateWithFlags(&ev_join2, hipEventDisableTiming));
        return WC_OK;
    }

    std::vector<wc::DevBuf *> all_buffers() {
        return {&nr.col_partial, &nr.col_mean, &nr.norm_lo, &nr.norm_hi, &nr.cand_word, &nr.chrom_of_row, &nr.chrom_range,
                &nr.chrom_off_dev, &nr.sample_rows, &nr.sample_slot, &nr.s32, &nr.s_norm_lo, &nr.s_chrom, &nr.s_range, &nr.keys1,
                &nr.thr, &nr.cnt, &nr.list, &nr.tiles, &nr.fb_rows, &nr.fb_count, &nr.fb_scratch,
                &nr.stats, &nr.tiles0, &nr.pw_prog, &nr.pairs, &nr.x64, &nr.m2, &nr.a16, &nr.s16, &tmp_a, &tmp_b, &tmp_c, &tmp_d,
                &ts.counts, &ts.totals, &ts.raw, &ts.proj, &ts.data, &ts.xt, &ts.xc, &ts.zt, &ts.rt, &ts.nt,
                &ts.sdt, &ts.z, &ts.r, &ts.n, &ts.sd_avg, &ts.zc, &ts.rc, &ts.gpos, &ts.regions,
                &ts.sel, &ts.res_z, &ts.res_r, &ts.cwz, &ts.calls, &ts.n_calls, &ts.zs, &ts.rs2, &ts.ns2, &ts.sds, &ts.sub, &ts.tmin, &ts.tmax, &ts.tmin2, &ts.tmax2, &ts.cell_state, &ts.cell_rec, &ts.prefix, &ts.reg_abs,
                &ts.reg_flag, &ts.rs, &ts.jobs_a, &ts.jobs_b, &ts.job_cnt, &ts.partial, &ts.cbound, &ts.cuts, &ts.job_res, &ts.hot,
                &ts.cand, &ts.cand_cnt, &ts.seg, &ts.out_val, &ts.out_x, &ts.out_y, &ts.out_n,
                &ts.whole, &ts.effect, &ts.misc, &ts.misc2, &ts.reduce_tmp, &ts.win_bits, &ts.bit_off, &ts.pairs_a, &ts.pairs_b, &ts.cut_vals, &ts.prof_work, &ts.sd_fail, &ts.walk_hot, &prep.eig_ws, &prep.counts, &prep.totals, &prep.sel, &prep.raw, &prep.data,
                &prep.xt, &prep.xc, &prep.z, &prep.proj, &prep.misc, &prep.zt,
                &cv.tab, &cv.tiles, &cv.kpos, &cv.cls, &df_scratch, &df_meta, &js_slots, &js_tiles, &sp_plan, &dr_tab, &cx_tab, &cx_prefix, &cx_rows, &pl_list, &pl_counts, &pl_tab, &pl_img, &pl_part, &pl_status};
    }
};

namespace wc {
// N events for the stage times of a host-array call, destroyed on every way out of it
template <int N> struct Events {
    hipEvent_t e[N] = {};
    ~Events() {
        for (int i = 0; i < N; ++i)
            if (e[i]) (void)hipEventDestroy(e[i]);
    }
    int create() {
        for (int i = 0; i < N; ++i) WC_HIP(hipEventCreate(&e[i]));
        return WC_OK;
    }
    // ms[i] = the time from event from[i] to event to[i], for n stages
    void elapsed(int n, const int *from, const int *to, double *ms) const {
        for (int i = 0; i < n; ++i) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, e[from[i]], e[to[i]]);
            ms[i] = t;
        }
    }
};

// eigh.hip: leading eigenpairs of a device-resident symmetric matrix (host outputs)
int sym_eigh_leading(wc_ctx *ctx, const double *matrix_dev, int64_t n, int n_pairs, double *eigvals_out,
                     double *eigvecs_out);

// convert.hip, for the streamed BAM route (bamgpu.hip): one slice of a run whose offsets table is born on the device
// (DEVICE int [n_chrom + 1]); `most`: a bound of its last entry, by which the grids and the working memory are sized.
// The order of the chromosomes is the caller's to keep (the reader's order check does).  convert_run_max_pending: the
// most positions the run has carried from one slice to the next (waits for the stream).
int convert_feed_table_dev(wc_convert_run *run, hipStream_t stream, const int32_t *pos, const uint8_t *mapq,
                           const uint16_t *flag, const int32_t *mate_pos, const int *slice_offsets_dev, int64_t most);
int convert_run_max_pending(const wc_convert_run *run, hipStream_t stream, int64_t *out);
// A convert's result from its device image -- 8 counters, then `bins` counts -- to HOST memory, on `stream` and waiting
// for it: the counters, the counts, and the refusal (WC_E_ARG) of a status word, counter 4, that is not 0.  Behind a
// refusal the entries differ and both ways are kept: the whole calls (wc_convert_reads_ex, wc_convert_bam_dev) have always
// written the counts all the same (counts_when_refused; tests/test_convert_bounded_gpu.py compares them), a run's finish
// leaves counts_out alone, as include/wisecondor_hip.h says.  stats_out NULL: the status word alone is read and checked
// (a run between two slices).
int convert_result(hipStream_t stream, const int64_t *image_dev, int64_t bins, int32_t *counts_out, int64_t *stats_out,
                   bool counts_when_refused);
}  // namespace wc
