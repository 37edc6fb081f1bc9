/*
 * wisecondor_hip.h -- C ABI of the MI355X (gfx950) implementation of WISECONDOR's
 * numeric hot path: `newref` reference-bin selection and the `test` path
 * (PCA-apply, masked z-score repeats, Stouffer window segmentation).
 *
 * The reference (VUmcCGP/wisecondor) is pure Python/numpy and has no FFI of its
 * own; each entry point below replaces one numpy function of the reference and
 * cites it as file:line under the upstream tree.  INTEGRATION.md shows the
 * ctypes stub a maintainer would add to wisetools.py to bind them.
 *
 * Conventions
 *   - plain C, no C++/torch types; every array is a dense row-major buffer.
 *   - functions ending in `_dev` take DEVICE pointers and enqueue work on the
 *     given hipStream_t (passed as void*; NULL = default stream) without
 *     synchronising; the others take HOST pointers, copy, run and synchronise.
 *   - return value 0 = success, negative = WC_E_* below; wc_last_error() gives
 *     a message.  Nothing here falls back to a CPU implementation.
 *   - IEEE specials propagate as in the reference (np.seterr('ignore'),
 *     wisetools.py:34): NaN/inf inputs yield NaN/inf outputs, never a trap.
 */
#ifndef WISECONDOR_HIP_H
#define WISECONDOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WC_OK 0
#define WC_E_ARG (-1)      /* invalid argument (shape, range, NULL)            */
#define WC_E_HIP (-2)      /* a HIP runtime call failed                        */
#define WC_E_LIMIT (-3)    /* size beyond a documented implementation limit    */
#define WC_E_INTERNAL (-4) /* internal consistency check failed                */

/* Summation order of the float64 distance, which numpy derives from the memory
 * layout of correctedData (wisetools.py:302): a C-contiguous [bins, samples]
 * array is reduced row by row with numpy's pairwise summation; the
 * Fortran-contiguous array that np.load returns for a prep file (trainPCA
 * returns corrected.T, wisetools.py:101) is reduced sample by sample, i.e. a
 * plain left-to-right sum.  The buffers handed to this library are always
 * row-major [bins, samples]; the flag only selects the rounding order.        */
#define WC_SUM_PAIRWISE 0
#define WC_SUM_SEQUENTIAL 1

typedef struct wc_ctx wc_ctx; /* per-device context: workspaces, scratch, counters */

/* ---- context -------------------------------------------------------------- */
wc_ctx *wc_create(int device);
void wc_destroy(wc_ctx *ctx);
const char *wc_last_error(void);
const char *wc_version(void);
/* counters of the last newref call: [0] rows finished by the fast path,
 * [1] rows that took the exact fallback path, [2] symmetric tiles launched,
 * [3] sample columns M, [4] candidates re-scored in float64 (sum over rows)   */
int wc_newref_stats(wc_ctx *ctx, int64_t out[8]);

/* ---- newref: reference-bin selection -------------------------------------- */
/* getPart, wisetools.py:358-361: rows [start,end) of zero-based part p of n.  */
void wc_get_part(int64_t partnum, int64_t outof, int64_t bincount, int64_t *start, int64_t *end);

/*
 * getReference + getRefForBins, wisetools.py:298-325 and :364-398.
 * corrected      [n_bins, n_samples] float64 (the prep file's correctedData)
 * chrom_bins     [n_chrom] bins per chromosome (maskedChromBins); sum == n_bins
 * k              selectRefAmount (reference default 100)
 * sum_order      WC_SUM_PAIRWISE / WC_SUM_SEQUENTIAL (see above)
 * row_begin/end  target rows to produce (getPart of part, splitParts)
 * idx_out        [row_end-row_begin, k] int32: positions in the
 *                "all bins not on the target's chromosome" concatenation
 *                (wisetools.py:386-387), -1 padded
 * dist_out       [row_end-row_begin, k] float64 ascending, 1e10 padded
 * Results equal the reference bit for bit (stable (distance, position) order,
 * numpy pairwise-summed float64 distances).  k <= 1024; above 256 every row is
 * scanned exactly (the candidate lists are sized for refsize <= 256): slower, same bits.
 */
int wc_get_reference(wc_ctx *ctx, const double *corrected, int64_t n_bins, int64_t n_samples,
                     const int64_t *chrom_bins, int n_chrom, int k, int sum_order,
                     int64_t row_begin, int64_t row_end, int32_t *idx_out, double *dist_out);
int wc_get_reference_dev(wc_ctx *ctx, void *stream, const double *corrected, int64_t n_bins,
                         int64_t n_samples, const int64_t *chrom_bins_host, int n_chrom, int k,
                         int sum_order, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                         double *dist_out);

/*
 * Multi-GPU building blocks of the same computation (one process per GPU; the
 * host exchanges `thr` / candidate lists with RCCL between the calls).
 *   stage A  wc_newref_prepare_dev    centre + float16 operand image + norm bounds (all rows)
 *   stage B  wc_newref_thresholds_dev per-row admission thresholds for rows
 *            [row_begin,row_end) from a fixed pseudo-random column sample
 *   stage C  wc_newref_collect_dev    symmetric MFMA distance tiles
 *            `tile_rank` of `tile_ranks` (round-robin), appending candidates
 *            whose lower-bound distance passes the row threshold
 *   stage D  wc_newref_finish_dev     float64 re-score in numpy order, stable
 *            sort, certificate, exact fallback -> idx/dist for the row range
 * wc_get_reference_dev == A, B(all), C(0 of 1), D(range).
 */
int wc_newref_prepare_dev(wc_ctx *ctx, void *stream, const double *corrected, int64_t n_bins,
                          int64_t n_samples, const int64_t *chrom_bins_host, int n_chrom, int k,
                          int sum_order);
int wc_newref_thresholds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end);
/* copy thresholds of rows [row_begin,row_end) out of / into the context (device float[rows]) */
int wc_newref_get_thresholds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, float *out);
int wc_newref_set_thresholds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, const float *in);
/* the error interval every decision of the fast path rests on (device float[rows] each): a listed
 * key of the pair (i, j) obeys  key <= distance(i, j) <= key + slack[i] + slack[j];  lo[i] is the
 * row's lower norm bound (key = lo[i] + lo[j] - 2 dot).  For tests of the bound itself. */
int wc_newref_get_bounds_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, float *lo_out,
                             float *slack_out);
int wc_newref_collect_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                          int tile_rank, int tile_ranks);
/* candidate-list exchange: pack the lists of rows [row_begin,row_end) into
 * dst_cnt int32[rows] / dst_list u64[rows, dst_cap] (device), and merge lists
 * received from another rank into this context's lists for those rows.  A source
 * row with more than `cap` entries marks the row for the exact fallback path.  */
int64_t wc_newref_list_capacity(wc_ctx *ctx);
int wc_newref_export_lists_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                               int64_t dst_cap, int32_t *dst_cnt, uint64_t *dst_list);
int wc_newref_import_lists_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                               int64_t src_cap, const int32_t *src_cnt, const uint64_t *src_list);
/* Inside a context a list entry's low word is (row | slack code << index bits): the candidate's slack
 * (wc_newref_get_bounds_dev), rounded UP to a code of 32 - index bits bits, rides above its row number, so that
 * stage D needs no gather per candidate.  The exchange format above stays (ordered key << 32 | plain row):
 * the export clears the code, the import puts the importing context's own code back.  For tests:
 *   wc_newref_export_raw_dev   the export without the clearing
 *   wc_newref_index_bits       the width of the prepared job (0: not prepared)
 *   wc_newref_set_index_bits   0 = automatic (max(17, bits of the padded row count - 1)); otherwise 1..24 and at
 *                              least what the problem needs (checked by the next prepare, where it takes effect)
 *   wc_slack_code_host         the code itself on the host: code_out[i] = code of slack[i] >= 0 in code_bits
 *                              (1..31) bits, decoded_out[i] = the slack it stands for (>= slack[i])            */
int wc_newref_export_raw_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                             int64_t dst_cap, int32_t *dst_cnt, uint64_t *dst_list);
int wc_newref_index_bits(wc_ctx *ctx);
int wc_newref_set_index_bits(wc_ctx *ctx, int bits);
int wc_slack_code_host(const float *slack, int64_t n, int code_bits, uint32_t *code_out, float *decoded_out);
/* For tests: the 32-bit image of a row's float64-ordered distance keys on which k_rescore ranks the row's pairs
 * (csrc/common.h, order_key32), on the host.  key[n] are the row's keys (~0 = no distance); min_hi_out = the smallest
 * high word among them, image_out[i] = min((key[i] - (min_hi << 32)) >> shift, 0xFFFFFFFE), 0xFFFFFFFF for ~0.
 * shift 0..32, or -1 for the kernel's own.                                                                        */
int wc_order_key_host(const uint64_t *key, int64_t n, int shift, uint32_t *image_out, uint32_t *min_hi_out);
int wc_newref_finish_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                         int32_t *idx_out, double *dist_out);
/* stage D in its two halves, for callers that time them apart: the per-row fast path, then
 * the exact path for the rows it handed over (same arguments; finish == rescore + fallback) */
int wc_newref_rescore_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                          int32_t *idx_out, double *dist_out);
int wc_newref_fallback_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                           int32_t *idx_out, double *dist_out);
/* the fast path's own two kernels apart (rescore == pick + rescore_pairs): candidate selection with
 * the certificate, then the exact float64 distances and their order (wisetools.py:302, 305-324) */
int wc_newref_pick_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                       int32_t *idx_out, double *dist_out);
int wc_newref_rescore_pairs_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end,
                                int32_t *idx_out, double *dist_out);
/* The exact path for EVERY row of [row_begin, row_end) of a prepared job (wc_newref_prepare_dev): float64
 * distances to all candidates in numpy's order and the stable selection of wisetools.py:305-321, without
 * matrix cores, bounds or candidate lists.  It is what a row takes when its certificate fails and what
 * refsize > 256 runs for every row; exported so that callers (the full-size tests) can hold the fast path
 * against it row by row. */
int wc_newref_exact_dev(wc_ctx *ctx, void *stream, int64_t row_begin, int64_t row_end, int32_t *idx_out,
                        double *dist_out);
/* measurement helper: microseconds a chain of n dependent empty kernel launches takes on `stream`
 * (mean over reps) -- the launch floor bench.py prices the one-sample `test` latency against */
int wc_launch_floor_us(wc_ctx *ctx, void *stream, int n, int reps, double *out);

/*
 * Native sample ingest and result output for many files (replaces the
 * np.load loop of wisecondor.py:75-80 / 193-196 and the np.savez_compressed of wisecondor.py:270-280
 * for batches).  Host only, plain threads, no GPU.
 *
 * wc_read_samples: file i of `paths` (a converted sample: members `sample` = pickled dict
 *   chromosome -> integer array, `arguments` = pickled dict with 'binsize') -> row i of counts_out
 *   (int32 [n_files, row_stride]): chromosomes '1'..'n_chrom', each padded with zeros / truncated to
 *   chrom_sizes[c] (toNumpyRefFormat, wisetools.py:268-274), bins merged when to_binsize is a whole
 *   multiple of the file's own bin size (scaleSample, wisetools.py:220-237; to_binsize <= 0: keep).
 *   binsize_out[i] = the file's own bin size.  status[i]: WC_OK, or WC_NPZ_* -- then the row is
 *   undefined and the caller reads that file the slow way (np.load), which also words the error.
 * wc_write_test_results: one `test` output file per row (keys / dtypes / shapes of the reference's,
 *   SURVEY.md App. B): arguments (args_npy[i]: the ready-made .npy member bytes, a pickled dict),
 *   runtime (shared bytes), binsize (int64 when binsize_is_int -- the reference stores the Python value it read
 *   from the reference file unchanged --, else float64), results_r / results_z (object arrays of n_chrom float64 arrays cut
 *   from row i of r / z at chrom_sizes), results_cwz [n_sel], results_calls [n, 5] (shape (0,) when
 *   empty), threshold_z, asdef, aasdef = asdef * threshold_z.  level: zlib level of the members
 *   (0 = stored).  status[i]: WC_OK or WC_NPZ_IO.
 * Both return WC_OK unless an argument is unusable; per-file outcomes are in status.
 */
#define WC_NPZ_UNSUPPORTED 1   /* not a file this reader understands (layout, pickle opcode, dtype) */
#define WC_NPZ_IO 2            /* could not read / write the file */
#define WC_NPZ_BINSIZE 3       /* the file's bin size cannot be scaled to to_binsize */
int wc_read_samples(const char *const *paths, int n_files, int n_threads, const int64_t *chrom_sizes, int n_chrom,
                    double to_binsize, int32_t *counts_out, int64_t row_stride, double *binsize_out, int *status);
/* chromosome lengths of every file at to_binsize (int64 [n_files, n_chrom]) and its own bin size: what
 * `newref`'s toNumpyArray needs to size the dense matrix (per-chromosome maximum over the samples,
 * wisetools.py:243-250) before wc_read_samples fills it */
int wc_read_sample_lengths(const char *const *paths, int n_files, int n_threads, int n_chrom, double to_binsize,
                           int64_t *lengths_out, double *binsize_out, int *status);
int wc_write_test_results(int n_files, int n_threads, const char *const *out_paths,
                          const unsigned char *const *args_npy, const int64_t *args_len,
                          const unsigned char *runtime_npy, int64_t runtime_len, double binsize, int binsize_is_int,
                          double threshold_z,
                          const int64_t *chrom_sizes, int n_chrom, const double *z, const double *r,
                          int64_t row_stride, const double *cwz, int n_sel, const double *calls,
                          const int32_t *n_calls, int max_calls, const double *asdef, int level, int *status);

/*
 * newref prep (upstream of the hot path): toNumpyArray's
 * normalisation + all-zero-bin mask (wisetools.py:240-264) and trainPCA
 * (wisetools.py:89-101) as a deterministic exact PCA (float64 Gram matrix on the GPU's float64
 * matrix cores, its [samples, samples] eigenproblem by the direct solver of csrc/eigh.hip on the GPU --
 * wc_newref_prep_eig; callers may also solve the fetched matrix with their own LAPACK --, everything
 * bins-sized on the GPU).
 *   counts [n_samples, n_total_bins] int32: per chromosome padded with zeros to
 *          chromosome_bins[c] (the longest sample, wisetools.py:245-250)
 *   mask_out [n_total_bins], masked_chrom_bins_out [n_chrom], *n_masked_out = B
 *   masked_data_out [B, n_samples]; corrected_t_out [n_samples, B] (the reference's
 *   correctedData is its transpose VIEW, i.e. Fortran-ordered [B, n_samples]);
 *   pca_components_out [n_comp, B]; pca_mean_out [B].
 * Call once with the four data outputs NULL to learn B, then again with buffers.
 * wc_newref_prep is the one-call form.  The steps are also exported: _gram builds the Gram
 * matrix G [n_samples, n_samples] of the centred data in HBM (and copies it to gram_out unless
 * that is NULL), _eig solves its eigenproblem on the GPU for the n_pairs leading pairs
 * (Householder tridiagonalisation, Sturm multisection, inverse iteration: a direct method,
 * 3 <= n_samples <= 4096, n_pairs <= 8; eigenvalues descending, unit eigenvectors as rows, host
 * outputs), _finish takes such pairs -- from _eig or from the caller's own LAPACK on gram_out.
 * wc_sym_eigh_leading_dev is the same solver on any device-resident symmetric float64 matrix
 * (left untouched).
 * What _gram leaves for _eig and _finish* lives in workspaces of the prep step's own: any other entry
 * point may run on the context between the steps, and _finish* may be called any number of times (with
 * other pairs or component counts too) after one _gram; each computes from that _gram's data.  Only the
 * next _gram (or wc_newref_prep, which calls it) replaces the state.  Before the first _gram of a
 * context, or after one that failed, _eig and _finish* return WC_E_ARG ("wc_newref_prep_gram has not
 * run") and write no output.
 */
/* Leaves the state described above; an error return leaves none (_eig / _finish* then refuse). */
int wc_newref_prep_gram(wc_ctx *ctx, const int32_t *counts, int64_t n_samples, int64_t n_total_bins,
                        const int64_t *chromosome_bins, int n_chrom, uint8_t *mask_out,
                        int64_t *masked_chrom_bins_out, int64_t *n_masked_out, double *gram_out);
/* wc_newref_prep_gram with a blacklist: drop_host [n_total_bins] uint8 (HOST, may be NULL).  Once the zero mask has reached
 * the host, mask_out[g] is cleared where drop_host[g] is set; the masked layout and everything behind it follow that mask, so
 * a dropped bin is treated as a bin that is empty in every sample.  Nothing else differs; NULL is wc_newref_prep_gram. */
int wc_newref_prep_gram_ex(wc_ctx *ctx, const int32_t *counts, int64_t n_samples, int64_t n_total_bins,
                           const int64_t *chromosome_bins, int n_chrom, uint8_t *mask_out,
                           int64_t *masked_chrom_bins_out, int64_t *n_masked_out, double *gram_out, const uint8_t *drop_host);
int wc_newref_prep_eig(wc_ctx *ctx, int n_pairs, double *eigvals_out, double *eigvecs_out);
int wc_sym_eigh_leading_dev(wc_ctx *ctx, const double *matrix_dev, int64_t n, int n_pairs, double *eigvals_out,
                            double *eigvecs_out);
/* Reads the state of the context's last wc_newref_prep_gram, whatever ran in between; repeatable. */
int wc_newref_prep_finish(wc_ctx *ctx, int n_comp, const double *eigvecs, const double *eigvals,
                          double *masked_data_out, double *corrected_t_out, double *pca_components_out,
                          double *pca_mean_out);
/* Device-resident finish: the bins-sized results stay in HBM for wc_newref_*_dev (no 2 x B x S x 8 B
 * trip through the host).  corrected_bs_dev [n_masked, n_samples] row-major device memory holding the
 * values of the reference's Fortran-ordered correctedData (wisetools.py:101: pass WC_SUM_SEQUENTIAL
 * to newref); masked_dev [n_masked, n_samples] device memory; pca_components_out / pca_mean_out host
 * memory.  Every output may be NULL.  Like wc_newref_prep_finish it reads the state of the context's last
 * wc_newref_prep_gram, whatever ran in between, and may be repeated. */
int wc_newref_prep_finish_dev(wc_ctx *ctx, int n_comp, const double *eigvecs, const double *eigvals,
                              double *masked_dev, double *corrected_bs_dev, double *pca_components_out,
                              double *pca_mean_out);
int wc_newref_prep(wc_ctx *ctx, const int32_t *counts, int64_t n_samples, int64_t n_total_bins,
                   const int64_t *chromosome_bins, int n_chrom, int n_comp, uint8_t *mask_out,
                   int64_t *masked_chrom_bins_out, int64_t *n_masked_out, double *masked_data_out,
                   double *corrected_t_out, double *pca_components_out, double *pca_mean_out);

/* ---- convert: BAM -> binned sample ----------------------------------------- */
#define WC_E_IO (-5)       /* a file could not be opened or read               */
#define WC_E_FORMAT (-6)   /* a file is damaged or not of the expected format  */
#define WC_CV_MAX_CHROM 256 /* chromosomes per wc_convert_reads call           */

/*
 * Native BAM reader (host only, no GPU; replaces pysam in convertBam, wisetools.py:134-155).  wc_bam_open reads the
 * whole file: BGZF blocks inflated by n_threads threads (1..64), records walked by their block_size chain.  The handle
 * then holds, until wc_bam_close:
 *   wc_bam_info   out[0] references in the header, [1] placed records (refID >= 0), [2] mapped (refID >= 0, flag 0x4
 *                 clear), [3] unmapped (flag 0x4 set), [4] no_coordinate (refID < 0), [5] bytes wc_bam_refs writes to
 *                 names_out.  The three counts stand in for pysam's index statistics (no .bai is read); that mapping
 *                 is not verified against pysam.
 *   wc_bam_refs   names_out: the reference names in header order, each followed by '\n'; lengths_out [n_refs];
 *                 offsets_out [n_refs + 1]: the placed records of reference r are [offsets[r], offsets[r+1]) of
 *   wc_bam_pos    int32, the 0-based position field, and
 *   wc_bam_mapq   uint8, of every placed record in file order (no flag filter), and for the paired mode of convert
 *   wc_bam_flag   uint16, the flag word (0x2 proper pair, 0x40 first in pair: pysam's is_proper_pair / is_read1), and
 *   wc_bam_mate_pos  int32, the 0-based next_pos field (pysam's next_reference_start; -1: none), in the same order.
 *                 That mapping follows the SAM specification; it is not verified against pysam either.
 * Errors (never a crash; wc_last_error has the text): WC_E_IO cannot open; WC_E_FORMAT bad magic, a damaged or
 * truncated BGZF block, a record that overruns its block_size or the data (a missing EOF block is accepted);
 * WC_E_ARG the file is not coordinate-sorted (positions decrease within a reference, or a reference's records are
 * not contiguous in header order); WC_E_LIMIT more than 2^31 - 1 placed records.
 */
typedef struct wc_bam wc_bam;
int wc_bam_open(const char *path, int n_threads, wc_bam **out);
int wc_bam_info(const wc_bam *bam, int64_t out[8]);
int wc_bam_refs(const wc_bam *bam, char *names_out, int64_t names_cap, int64_t *lengths_out, int64_t *offsets_out);
const int32_t *wc_bam_pos(const wc_bam *bam);
const uint8_t *wc_bam_mapq(const wc_bam *bam);
const uint16_t *wc_bam_flag(const wc_bam *bam);
const int32_t *wc_bam_mate_pos(const wc_bam *bam);
void wc_bam_close(wc_bam *bam);

/*
 * The device reader: the same result as the reader above with the four arrays born on the device.  Only the compressed
 * bytes cross to the device; BGZF inflate (one block per wave, CRC-32 checked), the record walk and the field extraction
 * are HIP kernels (csrc/bamgpu.hip).
 *
 * Host stage (no GPU needed): wc_bamfile_open reads the whole file into host memory pinned for `device` (the calling
 * thread's device is set to it; ordinary memory where device < 0 or no device is present), walks the BGZF block directory with the header checks of the reader above, inflates with zlib only
 * the leading blocks the BAM header needs, and parses the header.  Its errors carry the codes the reader above returns
 * for the same file: WC_E_IO cannot open; WC_E_FORMAT not BGZF, a truncated block or block header, an unusable BC field,
 * a bad BAM\1 magic, data that ends inside the header.
 *   wc_bamfile_info   out[0] references, [1] BGZF blocks, [2] the sum of their ISIZE fields (inflated bytes), [3] bytes of
 *                     the file, [4] offset of the first record in the inflated stream, [5] bytes wc_bamfile_refs writes to
 *                     names_out, [6] 1 when the buffer is pinned, [7] microseconds the pinned allocation took
 *   wc_bamfile_refs   names_out / lengths_out as in wc_bam_refs
 *
 * Device stage: wc_bam_open_dev uploads the file of an opened host stage, runs the kernels on `stream` and returns when
 * the arrays are complete; the host-stage handle may be closed afterwards.  The device memory the call needs is computed
 * from the block directory before anything is allocated (compressed and inflated bytes, 2 bytes of record map per
 * inflated byte, 15 bytes per possible record); budget_bytes <= 0 stands for 0.8 of the free device memory.  A need above
 * the budget is WC_E_LIMIT ("needs X bytes, budget Y"): such a file takes the reader above.  Everything but the four
 * arrays is freed before the call returns.  Further errors, with the codes of the reader above: WC_E_FORMAT a BGZF block
 * whose deflate data or CRC is damaged, a record with block_size < 32, with fields that overrun its block_size, with a
 * refID beyond the header, a chain of records that does not end exactly with the data; WC_E_ARG not coordinate-sorted;
 * WC_E_LIMIT more than 2^31 - 1 placed records.  A file with ONE fault gets the code of the reader above.  With several
 * the two may differ: the reader above reports the first fault in file order, this one reports a damaged BGZF block
 * before any record fault, and a record-format fault (the first in file order) before an order fault -- so an unsorted
 * pair followed by a bad record is WC_E_ARG there and WC_E_FORMAT here.
 *   wc_bam_dev_info   as wc_bam_info; out[6] the device bytes the open needed, [7] the budget it was held against
 *   wc_bam_dev_refs   as wc_bam_refs (host outputs)
 *   wc_bam_dev_pos / _mapq / _flag / _mate_pos   DEVICE pointers, valid until wc_bam_dev_close
 *   wc_bam_dev_fetch  copies of the four arrays in HOST memory (a NULL output is skipped); for tests
 *   wc_bam_dev_times  milliseconds of the open's stages between device events: out[0] host to device copy, [1] inflate,
 *                     [2] record starts (per-segment chain maps), [3] segment link, [4] record checks and counts,
 *                     [5] field extraction, [6] order check and offsets; [7] the whole call by the host clock
 * wc_bam_chain_segment: the record chain is resolved in segments of that many inflated bytes, segment s covering the
 * offsets [s * segment, (s + 1) * segment) of the inflated stream (for tests that aim at the boundaries).
 * wc_bgzf_inflate: the inflate kernel on any BGZF byte string (HOST pointers): bgzf_bytes [n] -> out [*out_len], cap the
 * room in out (WC_E_ARG when it is too small); WC_E_FORMAT for a damaged block header, deflate stream or CRC.
 * wc_convert_bam_dev: wc_convert_reads_ex_dev on the device arrays of an opened reader for the references refs[n_chrom]
 * (header indices, ascending), gathered on the device where they are not contiguous; counts_out / stats_out are HOST
 * memory, the call synchronises; a read beyond its chromosome's bins is WC_E_ARG as in wc_convert_reads_ex.
 */
typedef struct wc_bamfile wc_bamfile;
typedef struct wc_bam_dev wc_bam_dev;
int wc_bamfile_open(const char *path, int device, wc_bamfile **out);
int wc_bamfile_info(const wc_bamfile *file, int64_t out[8]);
int wc_bamfile_refs(const wc_bamfile *file, char *names_out, int64_t names_cap, int64_t *lengths_out);
void wc_bamfile_close(wc_bamfile *file);
int wc_bam_open_dev(wc_ctx *ctx, void *stream, const wc_bamfile *file, int64_t budget_bytes, wc_bam_dev **out);
int wc_bam_dev_info(const wc_bam_dev *bam, int64_t out[8]);
int wc_bam_dev_refs(const wc_bam_dev *bam, char *names_out, int64_t names_cap, int64_t *lengths_out, int64_t *offsets_out);
const int32_t *wc_bam_dev_pos(const wc_bam_dev *bam);
const uint8_t *wc_bam_dev_mapq(const wc_bam_dev *bam);
const uint16_t *wc_bam_dev_flag(const wc_bam_dev *bam);
const int32_t *wc_bam_dev_mate_pos(const wc_bam_dev *bam);
int wc_bam_dev_times(const wc_bam_dev *bam, double out[8]);
int wc_bam_dev_fetch(const wc_bam_dev *bam, int32_t *pos_out, uint8_t *mapq_out, uint16_t *flag_out, int32_t *mate_pos_out);
void wc_bam_dev_close(wc_bam_dev *bam);
int wc_bam_chain_segment(void);
int wc_bgzf_inflate(wc_ctx *ctx, const unsigned char *bgzf_bytes, int64_t n, unsigned char *out, int64_t cap, int64_t *out_len);
int wc_convert_bam_dev(wc_ctx *ctx, void *stream, const wc_bam_dev *bam, const int32_t *refs, int n_chrom, double binsize,
                       int min_shift, int threshold, int min_mapq, int demand_pair, const int64_t *bin_offsets,
                       int32_t *counts_out, int64_t *stats_out);

/*
 * The streamed device reader: the same wc_bam_dev handle with host and device working memory bounded by a chunk size
 * and the longest record, not by the file.  Only the four arrays (11 bytes per placed record) grow with the file.
 *
 * Host stage (no GPU needed): wc_bamchunks_open parses the BAM header from as many leading BGZF blocks as it needs (the
 * checks, texts and codes of wc_bamfile_open) and starts a reader thread that fills two staging buffers of
 * min(chunk_bytes, file size) + 65536 + 64 bytes in turn (pinned for `device`, ordinary memory where device < 0 or no
 * device is present); the file is never held whole.  A chunk is the next run of WHOLE BGZF blocks whose compressed bytes
 * total at most chunk_bytes, and at least one block (chunk_bytes = 1: one block per chunk; chunk_bytes <= 0: the default,
 * wc_bam_stream_default_chunk).  The bytes of a block cut by the end of a read go in front of the next read.  A block
 * header defect is reported by the wc_bamchunks_next call that meets it, with the file's block number: an incomplete
 * block is WC_E_FORMAT "truncated" only at the true end of the file.
 *   wc_bamchunks_info   as wc_bamfile_info, except [1] 0, [2] 0 (blocks and inflated bytes are known chunk by chunk) and
 *                       [7] the bytes of the two staging buffers
 *   wc_bamchunks_refs   as wc_bamfile_refs
 *   wc_bamchunks_next   out[0] 1: a chunk, 0: the file is through (the other words are 0); [1] the file's number of the
 *                       chunk's first block, [2] its blocks, [3] its compressed bytes, [4] the sum of its ISIZE fields,
 *                       [5] its offset in the file, [6] 1 for the file's last chunk.  The chunk before is released.
 *
 * Device stage: wc_bam_stream_dev opens the chunk iterator itself and sends every chunk through the kernels of the
 * whole-file reader: the compressed bytes are copied on a second stream while the chunk before is decoded on `stream`;
 * the blocks are inflated behind the bytes carried over from the chunk before (the records that do not end inside their
 * chunk, a cut block_size word included), the records of carry + chunk are walked and their fields appended to the four
 * arrays at a running base kept on the device; the bytes from the first record that does not end inside the chunk are
 * the next carry (a record longer than a chunk keeps accumulating: working memory is O(chunk + longest record)).
 * The counters, the coordinate-order check (the last placed record of a chunk is the predecessor of the next chunk's
 * first) and the per-reference counts accumulate on the device.  The arrays are reserved by the most records a chunk can
 * hold and grow geometrically.  One small status read per chunk, after the copy of the next chunk has been enqueued.
 * Errors carry the codes of wc_bam_open_dev, with block numbers and inflated offsets counted in the whole file; the first
 * defect in file order is reported, so a file with a format defect behind an order defect is WC_E_ARG here and
 * WC_E_FORMAT from wc_bam_open_dev (which checks every record before any order).  Leftover bytes behind the last chunk
 * are the "truncated" error.  There is no budget: the need does not grow with the file.
 *   wc_bam_dev_info          of a streamed handle: out[6] the peak device bytes INCLUDING the four arrays, [7] 0
 *   wc_bam_dev_times         of a streamed handle: out[0] milliseconds the call waited for the reader thread, [1] for
 *                            the device, [7] the whole call by the host clock; the others 0
 *   wc_bam_dev_stream_info   out[0] chunks, [1] / [2] the largest chunk's compressed / inflated bytes, [3] the largest
 *                            carry, [4] the peak device working bytes (everything except the four arrays), [5] the bytes
 *                            of the host staging buffers, [6] times the arrays were regrown, [7] 1 when the staging
 *                            buffers are pinned.  All 0 for a handle of wc_bam_open_dev.
 */
typedef struct wc_bamchunks wc_bamchunks;
int wc_bamchunks_open(const char *path, int device, int64_t chunk_bytes, wc_bamchunks **out);
int wc_bamchunks_info(const wc_bamchunks *chunks, int64_t out[8]);
int wc_bamchunks_refs(const wc_bamchunks *chunks, char *names_out, int64_t names_cap, int64_t *lengths_out);
int wc_bamchunks_next(wc_bamchunks *chunks, int64_t out[8]);
void wc_bamchunks_close(wc_bamchunks *chunks);
int64_t wc_bam_stream_default_chunk(void);
int wc_bam_stream_dev(wc_ctx *ctx, void *stream, const char *path, int64_t chunk_bytes, wc_bam_dev **out);
int wc_bam_dev_stream_info(const wc_bam_dev *bam, int64_t out[8]);

/*
 * The bounded route of `convert`: the loop of wc_bam_stream_dev with another sink.  A chunk's placed records go to a buffer
 * of the chunk's own (reserved by the most records a chunk plus carry can hold, reused by the next chunk), and once the
 * chunk's status read has found it sound, its records of the references refs[n_chrom] (indices into the header,
 * ascending: the rest is skipped) are set side by side and fed to a resumable convert (wc_convert_begin below) on
 * `stream`; the slice's table is made on the device from the chunk's references, so the route adds no host
 * synchronisation to the reader's one status read per chunk.  Device memory does not grow with the read count and the
 * number of placed records is not limited; one chunk is limited as one wc_convert_reads_ex_dev call is.  Errors keep the
 * codes, texts, block numbers and the first-defect-in-file-order rule of wc_bam_stream_dev; a damaged or unsorted chunk
 * is never fed.  counts_out (int32 [bin_offsets[n_chrom]]) and stats_out (int64 [8]) are HOST memory and what
 * wc_convert_bam_dev gives for the same file; on any error counts_out is not written (a read beyond its chromosome's
 * bins: WC_E_ARG, stats_out written).
 *   info_out   int64 [16]: [0] chunks, [1] the largest chunk's compressed bytes, [2] the largest carry of bytes from chunk
 *              to chunk, [3] the most positions the convert carried from slice to slice, [4] the peak device bytes,
 *              everything included, [5] the bytes of the host staging buffers, [6] placed records, [7] the largest
 *              chunk's inflated bytes, [8] / [9] / [10] mapped / unmapped / no_coordinate as wc_bam_dev_info [2..4],
 *              [11] of [4]: the bytes of the convert's own working memory; the others 0
 */
int wc_convert_bam_stream_dev(wc_ctx *ctx, void *stream, const char *path, int64_t chunk_bytes, const int32_t *refs, int n_chrom,
                              double binsize, int min_shift, int threshold, int min_mapq, int demand_pair,
                              const int64_t *bin_offsets, int32_t *counts_out, int64_t *stats_out, int64_t info_out[16]);

/*
 * The numeric part of convertBam (wisetools.py:116-217) for all chromosomes of one file in one call: the paired-end
 * selection, duplicate removal, mapping-quality filter, the tower (RETRO) filter, binning.  wc_convert_reads[_dev] is
 * the function as toolConvert calls it (mapq 1, demandPair False); wc_convert_reads_ex[_dev] takes both parameters.
 *   pos, mapq       the reads of the processed chromosomes, concatenated in header order (device pointers for _dev)
 *   read_offsets    HOST int64 [n_chrom + 1], read_offsets[0] == 0: chromosome c owns [read_offsets[c], [c+1])
 *   bin_offsets     HOST int64 [n_chrom + 1], bin_offsets[0] == 0: its bins in counts_out (int(length / binsize + 1) each)
 *   min_shift, threshold   -retdist / -retthres, any value (threshold < 0: no tower filter)
 *   counts_out      int32 [bin_offsets[n_chrom]], zeroed by the call
 *   stats_out       int64 [8]: [0] filter_rmdup [1] filter_mapq [2] pre_retro [3] post_retro [4] counted reads whose
 *                   bin (int64)((double)pos / binsize) lies outside their chromosome's bins -- the status word: the
 *                   reference raises IndexError there, the host form returns WC_E_ARG, nothing is written out of
 *                   range -- [5] reads kept by the first two filters [6] pair_fail (0 unless demand_pair)
 *   min_mapq        (_ex) a read below it is counted in filter_mapq; any int (<= 0: nothing is filtered, > 255: every
 *                   eligible read that is no duplicate)
 *   demand_pair     (_ex) != 0: the paired-end branch (wisetools.py:160-183).  Only reads whose flag has 0x2 and 0x40 take
 *                   part; every other counted read adds one to pair_fail and nothing else.  A duplicate is a read whose
 *                   pos AND mate_pos equal those of the previous read that took part -- however many reads or
 *                   chromosomes back; before the first one (-1, -1) is compared.  pre_retro counts the reads that took
 *                   part.  flag (uint16) and mate_pos (int32) run parallel to pos; they may be NULL when demand_pair
 *                   == 0 and are WC_E_ARG when it is not.
 * The first read of every chromosome is consumed uncounted and `larp` is carried from chromosome to chromosome on the
 * device, as in the reference.  Where the reference dies (a chromosome without reads: StopIteration) the chromosome
 * gets all-zero counts and leaves `larp` alone; a chromosome with one read likewise.  n_chrom <= WC_CV_MAX_CHROM,
 * fewer than 2^31 - 4096 reads.  In the paired mode the carried state is the previous read that took part, so such a
 * chromosome changes nothing there either.  wc_convert_tile_reads: reads per workgroup of the kernels (their tile
 * boundaries).
 */
int wc_convert_tile_reads(void);
int wc_convert_reads_dev(wc_ctx *ctx, void *stream, const int32_t *pos, const uint8_t *mapq, const int64_t *read_offsets,
                         int n_chrom, double binsize, int min_shift, int threshold, const int64_t *bin_offsets,
                         int32_t *counts_out, int64_t *stats_out);
int wc_convert_reads(wc_ctx *ctx, const int32_t *pos, const uint8_t *mapq, const int64_t *read_offsets, int n_chrom,
                     double binsize, int min_shift, int threshold, const int64_t *bin_offsets, int32_t *counts_out,
                     int64_t *stats_out);
int wc_convert_reads_ex_dev(wc_ctx *ctx, void *stream, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                            const int32_t *mate_pos, const int64_t *read_offsets, int n_chrom, double binsize, int min_shift,
                            int threshold, int min_mapq, int demand_pair, const int64_t *bin_offsets, int32_t *counts_out,
                            int64_t *stats_out);
int wc_convert_reads_ex(wc_ctx *ctx, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag, const int32_t *mate_pos,
                        const int64_t *read_offsets, int n_chrom, double binsize, int min_shift, int threshold, int min_mapq,
                        int demand_pair, const int64_t *bin_offsets, int32_t *counts_out, int64_t *stats_out);

/*
 * The same computation in resumable form: the reads arrive in slices, in file order, and every slice is filtered and
 * binned as it arrives; only a small carry stays on the device between slices (csrc/convert.hip), so the
 * working memory follows the largest slice and not the read count, and the total number of reads is not limited.
 *   wc_convert_begin       the parameters of wc_convert_reads_ex that do not depend on the reads; zeroes the counts
 *   wc_convert_feed_dev    one slice: DEVICE arrays (flag / mate_pos may be NULL unless demand_pair) and slice_offsets,
 *                          HOST int64 [n_chrom + 1], slice_offsets[0] == 0: chromosome c owns [slice_offsets[c], [c+1]) of
 *                          THIS slice's arrays.  A slice may be empty, hold parts of several chromosomes and end anywhere:
 *                          on a chromosome's consumed first read, inside a tower.  Reads for a chromosome in front of one
 *                          that has had reads already are WC_E_ARG.  One slice is limited as one wc_convert_reads_ex_dev
 *                          call is.  The call enqueues kernels on `stream` and returns without waiting; the arrays must
 *                          stay valid until they have run.  Slices of one run go to one stream (or the caller orders them).
 *   wc_convert_feed        the same from HOST arrays; it waits for the slice and returns WC_E_ARG as soon as the status
 *                          word (stats [4]) is not 0
 *   wc_convert_finish_dev  closes the open run and copies the counts (int32 [bin_offsets[n_chrom]]) and stats (int64 [8],
 *                          as stats_out above, every word 64-bit over all slices) to DEVICE memory on `stream`
 *   wc_convert_finish      the same to HOST memory; status word not 0: WC_E_ARG, stats_out written, counts_out untouched
 *   wc_convert_run_info    out[0] slices that ran, [1] device bytes the run holds, [2] an upper bound of the positions carried
 *   wc_convert_end         frees the run (finished or not)
 * After any sequence of slices whose concatenation is the input of wc_convert_reads_ex, counts and stats [0..6] are that
 * call's, bit for bit.  The carry holds at most min(longest open run, max(threshold, 0)) positions.
 */
typedef struct wc_convert_run wc_convert_run;
int wc_convert_begin(wc_ctx *ctx, int n_chrom, double binsize, int min_shift, int threshold, int min_mapq, int demand_pair,
                     const int64_t *bin_offsets, wc_convert_run **out);
int wc_convert_feed_dev(wc_convert_run *run, void *stream, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                        const int32_t *mate_pos, const int64_t *slice_offsets);
int wc_convert_feed(wc_convert_run *run, const int32_t *pos, const uint8_t *mapq, const uint16_t *flag,
                    const int32_t *mate_pos, const int64_t *slice_offsets);
int wc_convert_finish_dev(wc_convert_run *run, void *stream, int32_t *counts_out, int64_t *stats_out);
int wc_convert_finish(wc_convert_run *run, int32_t *counts_out, int64_t *stats_out);
int wc_convert_run_info(const wc_convert_run *run, int64_t out[8]);
void wc_convert_end(wc_convert_run *run);

/* ---- test: per-reference state -------------------------------------------- */
typedef struct wc_reference wc_reference;

/*
 * Everything toolTest derives from the reference file alone
 * (wisecondor.py:177-201): uploads indexes/distances/PCA, computes
 * getOptimalCutoff(distances, cutoff_repeats) (wisetools.py:328-336) on the
 * GPU and the per-bin reference lists `index[i][distances[i] < cutoff]`
 * (wisetools.py:424) once, since they are sample independent.
 *   indexes [n_bins,k] int32, distances [n_bins,k] float64,
 *   chromosome_sizes/masked_sizes [n_chrom] int64, mask [sum(chromosome_sizes)] uint8,
 *   pca_mean [n_bins], pca_components [n_comp, n_bins] float64.
 * cutoff_override: NULL to compute the cutoff, else the value to use (the
 * reference passes it explicitly to repeatTest, wisetools.py:438).
 * Limits: k <= 1024 (lists above 128 entries take a slower generic kernel), n_comp <= 8.
 */
wc_reference *wc_reference_create(wc_ctx *ctx, const int32_t *indexes, const double *distances,
                                  int64_t n_bins, int k, const int64_t *chromosome_sizes,
                                  const int64_t *masked_sizes, int n_chrom, const uint8_t *mask,
                                  const double *pca_mean, const double *pca_components, int n_comp,
                                  int cutoff_repeats, const double *cutoff_override);
void wc_reference_destroy(wc_reference *ref);
double wc_reference_cutoff(const wc_reference *ref);

/* getOptimalCutoff alone, wisetools.py:328-336 (host pointers). */
int wc_optimal_cutoff(wc_ctx *ctx, const double *distances, int64_t count, int repeats, double *cutoff);
/* ... with the function's second return value (wisetools.py:332, :336): mask [count] uint8 =
 * `distances < cutoff of the iteration before the last` (all finite values when repeats == 1).
 * repeats >= 1; the reference's repeats == 0 case (an all-zero float array) is host marshalling. */
int wc_optimal_cutoff_mask(wc_ctx *ctx, const double *distances, int64_t count, int repeats, double *cutoff,
                           uint8_t *mask);

/* applyPCA alone, wisetools.py:104-113, for a batch of already normalised and
 * masked vectors: samples/out [n_samples, n_bins] float64 (host pointers).    */
int wc_apply_pca(wc_ctx *ctx, const double *samples, int64_t n_samples, int64_t n_bins,
                 const double *pca_mean, const double *pca_components, int n_comp, double *out);

/*
 * toNumpyRefFormat + applyPCA, wisetools.py:267-278 and :104-113, for a batch.
 * counts [n_samples, sum(chromosome_sizes)] int32: per chromosome already
 * padded/truncated to the reference length (host marshalling of the dict).
 * out    [n_samples, n_bins] float64 (PCA-corrected, masked, unit-sum).
 * raw    optional [n_samples, n_bins] float64: the vector before PCA.
 */
int wc_prepare_samples(wc_ctx *ctx, const wc_reference *ref, const int32_t *counts,
                       int64_t n_samples, double *out, double *raw);

/*
 * repeatTest/trySample, wisetools.py:407-448, for a batch of samples.
 * data [n_samples, n_bins] float64 -> z, r, ref_sizes [n_samples, n_bins]
 * float64 and sd_avg [n_samples] (stdDevAvg).  Means and standard deviations
 * are summed in numpy's pairwise order.
 */
int wc_repeat_test(wc_ctx *ctx, const wc_reference *ref, const double *data, int64_t n_samples,
                   double threshold, int repeats, double *z, double *r, double *ref_sizes,
                   double *sd_avg);

/*
 * stdDevAvg of trySample alone (wisetools.py:428-435): the mean of the non-NaN per-bin standard
 * deviations, summed bin by bin like the reference's Python loop (sequential float64 rounding).
 * sd [n_samples, n_bins] host -> out [n_samples].  The sum runs as an exact parallel scan
 * (testpath.hip, k_sd_fast); *serial_samples (optional) receives how many samples needed the
 * serial chain instead.
 */
int wc_std_dev_avg(wc_ctx *ctx, const double *sd, int64_t n_samples, int64_t n_bins, double *out,
                   int32_t *serial_samples);

/*
 * fillTri / fillTriMin (wisetools.py:466-487) + TriArr.segmentTri (triarray.py:59-84)
 * on a batch of independent regions without materialising the triangle.
 * z [total] float64: concatenated regions; region_offsets [n_regions+1].
 * min_effect != 0 enables fillTriMin's filter: a window keeps its value only if
 * abs(median(ratio[x..y]) - 1) >= min_effect (ratio laid out like z; may be NULL
 * when min_effect == 0).
 * Outputs per region: whole-region Stouffer z (getValue(0,n-1),
 * wisecondor.py:237) and up to max_calls segments (value, x, y inclusive) in
 * ascending position order; n_calls[region] holds the number found (if it
 * exceeds max_calls the call fails with WC_E_LIMIT).
 */
int wc_stouffer_segments(wc_ctx *ctx, const double *z, const double *ratio, double min_effect,
                         const int64_t *region_offsets, int64_t n_regions, double threshold,
                         int min_search, int max_calls, double *region_z, int32_t *n_calls,
                         double *call_value, int32_t *call_x, int32_t *call_y);

/*
 * The numeric content of toolTest (wisecondor.py:199-268) for a batch:
 * prepare -> repeatTest -> minrefbins cleaning -> Stouffer segmentation ->
 * call coordinate mapping and median effect -> inflated per-bin outputs.
 *   counts        [n_samples, n_total_bins] int32 (see wc_prepare_samples)
 *   chromosomes   [n_sel] 1-based chromosome numbers to segment (-chromosomes)
 *   results_z/r   [n_samples, n_total_bins] float64 (r is ratio-1), zeros at
 *                 masked / removed bins
 *   results_cwz   [n_samples, n_sel]
 *   calls         [n_samples, max_calls, 5] rows [chrom, start, end, z, effect]
 *   n_calls       [n_samples]
 *   asdef         [n_samples]
 * min_effect is -mineffectsize (0 = the reference default, no filter).
 */
int wc_test_batch(wc_ctx *ctx, const wc_reference *ref, const int32_t *counts, int64_t n_samples,
                  double threshold, int min_ref_bins, int repeats, double min_effect,
                  const int32_t *chromosomes, int n_sel, int max_calls, double *results_z,
                  double *results_r, double *results_cwz, double *calls, int32_t *n_calls,
                  double *asdef);

/* Device-resident variant used by bench.py: counts already on the GPU, outputs
 * stay on the GPU (any output pointer may be NULL to skip it).                */
int wc_test_batch_dev(wc_ctx *ctx, void *stream, const wc_reference *ref, const int32_t *counts,
                      int64_t n_samples, double threshold, int min_ref_bins, int repeats,
                      double min_effect, const int32_t *chromosomes_host, int n_sel, int max_calls,
                      double *results_z, double *results_r, double *results_cwz, double *calls,
                      int32_t *n_calls, double *asdef);

/*
 * Optional stage timing of wc_test_batch_dev for the measurement harness (bench.py): with
 * profiling enabled every call records HIP events between its stages on the launch stream.
 * wc_test_profile_read synchronises the device and returns, for the LAST call, milliseconds of
 *   [0] prepare (toNumpyRefFormat + applyPCA)   [1] z-score repeats (repeatTest)
 *   [2] reshaping, inflation, cleaning          [3] Stouffer segmentation (fillTri + segmentTri)
 *   [4] call mapping and outputs                [5] of [3]: the certificate + window-search launches
 * and the work those launches executed: [6] windows evaluated by the search kernel (4 float64
 * operations each), [7] window / bound evaluations of the quiet-job certificate.
 */
int wc_test_profile(wc_ctx *ctx, int enable);
/* Development aid: phase stamps (shader clock) of the latency-mode kernels' workgroup
 * `block_plus_one - 1` (0: off); returns the 64 stamps of the calls since the last request. */
int wc_debug_times(wc_ctx *ctx, int block_plus_one, unsigned long long *out64);
/* Development aid: the process-wide count of workspace (re)allocations -- every device workspace of every context
 * that was allocated, grown or released, and every context's pinned host block that moved.  Read only.  A repeated
 * call of an unchanged shape leaves it unchanged (such calls only enqueue kernels); the latency-mode graph of the
 * test path is dropped and captured again once it differs from its value at capture time. */
unsigned long long wc_realloc_epoch(void);
int wc_test_profile_read(wc_ctx *ctx, double out[8]);

/* ---- result files: raw deflate and CRC-32 on the device (testbatch -encoder gpu) ------------
 * Every row of `src` (n_rows rows of row_bytes bytes, src_stride bytes apart) becomes one complete raw deflate
 * stream (zlib.decompress(x, -15) reads it): out_len[i] bytes at out + i * out_stride, out_stride >=
 * wc_deflate_bound(row_bytes); crc[i] is the CRC-32 of the row's input bytes, as zlib.crc32 gives it.  The bytes of
 * `out` behind a stream are not written.
 * A row is cut into blocks of wc_deflate_block_bytes() input bytes that are coded independently: a run of equal
 * bytes is one literal and distance-1 matches of 3 .. 258 bytes (zlib's Z_RLE strategy; matches do not cross a
 * block cut), the block's own Huffman code (dynamic header; code lengths limited to 15 bits, those of the
 * code-length alphabet to 7), or a stored block where that is not smaller.  Behind every coded block but the last an
 * empty stored block pads to a byte boundary.  wc_deflate_bound(n) = n + 10 * (ceil(n / B) + 1).
 * The streams depend on the input bytes alone.  wc_deflate_rows_dev enqueues on `stream` without synchronising
 * (scratch memory of `ctx`: one call in flight per context).
 * wc_deflate_rows_len_dev: the same for rows of unequal lengths, in the shape of wc_bgzf_rows_dev: the stream of the
 * first row_len[i] (DEVICE int64, read on the device) bytes of row i, an empty row one empty final block; the grid is
 * sized by max_row_bytes, out_stride >= wc_deflate_bound(max_row_bytes).  A row_len[i] outside 0 .. max_row_bytes
 * gives out_len[i] = -1 and nothing else for that row.  A row's stream, length and CRC are those of
 * wc_deflate_rows_dev called on that row alone.                                                           */
int wc_deflate_block_bytes(void);
int64_t wc_deflate_bound(int64_t row_bytes);
int wc_deflate_rows_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, int64_t row_bytes,
                        int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len, uint32_t *crc);
int wc_deflate_rows_len_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, const int64_t *row_len,
                            int64_t max_row_bytes, int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len,
                            uint32_t *crc);
int wc_deflate_rows(wc_ctx *ctx, const unsigned char *src, int64_t n_rows, int64_t row_bytes, int64_t src_stride,
                    unsigned char *out, int64_t out_stride, int64_t *out_len, uint32_t *crc);
/* The encoder's Huffman construction, host only (no GPU needed): len_out[s] = code length of symbol s, 0 where
 * freq[s] == 0, at most `limit` (1 .. 15) bits; n <= 288; a single used symbol gets length 1; with two or more the
 * Kraft sum is exactly 1; sum(freq * len) is the unlimited Huffman cost wherever that tree fits the limit.     */
int wc_huffman_lengths(const uint32_t *freq, int n, int limit, uint8_t *len_out);

/* The members results_r.npy / results_z.npy of a result file are a 1-d object array of n_chrom float64 arrays
 * (protocol 3 pickle, what np.save writes); everything but the values depends on chrom_sizes alone.
 * wc_results_member_bytes: the member's size (-1: unusable argument).  wc_results_member_template: the member with
 * zeros for values into tmpl (cap >= that size), and table [3, n_chrom] int64 = the byte offset of every
 * chromosome's values in the member, its first element in a dense row, its number of elements.  Host only.
 * wc_results_members_dev: image[row, :member_bytes] = the member of rows[row, :] (DEVICE float64, row_stride
 * elements apart); tmpl and table are DEVICE copies of the above; image rows are image_stride bytes apart (a
 * multiple of 4, >= member_bytes, padded with zeros).  Enqueues on `stream`.                               */
int64_t wc_results_member_bytes(const int64_t *chrom_sizes, int n_chrom);
int wc_results_member_template(const int64_t *chrom_sizes, int n_chrom, unsigned char *tmpl, int64_t cap, int64_t *table);
int wc_results_members_dev(wc_ctx *ctx, void *stream, const unsigned char *tmpl, int64_t member_bytes, const int64_t *table,
                           int n_gaps, const double *rows, int64_t row_stride, int64_t n_rows, unsigned char *image,
                           int64_t image_stride);
/* wc_write_test_results with results_z / results_r given as ready-made raw deflate streams (z_len[i] bytes at
 * z_streams + i * z_stride, CRC-32 z_crc[i] of the member_bytes uncompressed bytes; likewise r): stored with
 * method 8 as they are.  The other members are encoded as wc_write_test_results encodes them.               */
int wc_write_test_results_packed(int n_files, int n_threads, const char *const *out_paths, const unsigned char *const *args_npy,
                                 const int64_t *args_len, const unsigned char *runtime_npy, int64_t runtime_len, double binsize,
                                 int binsize_is_int, double threshold_z, const unsigned char *z_streams, int64_t z_stride,
                                 const int64_t *z_len, const uint32_t *z_crc, const unsigned char *r_streams, int64_t r_stride,
                                 const int64_t *r_len, const uint32_t *r_crc, int64_t member_bytes, const double *cwz, int n_sel,
                                 const double *calls, const int32_t *n_calls, int max_calls, const double *asdef, int level,
                                 int *status);

/* ---- plotbatch: result files -> z-score panel PNGs (upstream plotLines, wisetools.py:527-662) -----------
 * What is drawn follows the reference; how it is drawn is this library's own rasteriser ("plotbatch":
 * integer blending, half-open rectangles, a column-wise polyline, a bitmap font), so that the bytes are reproducible.
 *
 * wc_plot_layout (host): the pixel boxes [x0, y0, x1, y1) of n_panels panels in `rows` rows of `columns`, int32
 *   [n_panels, 4], inside the reference's figure margins.  A box may be empty in a very small image.  width and height
 *   are whole units up to 2097152: an image's pixels (wc_plot_image_bytes holds those to 32768) or a PDF page's
 *   centipoints (plotpdf, below).
 * wc_plot_list: the display list a kernel makes of dense z-score rows and calls in the layout wc_test_batch_dev leaves
 *   them in (results_z [n_samples, row_stride], chromosome c at the sum of chrom_sizes before it; calls [n_samples,
 *   max_calls, 5]; n_calls [n_samples]) for the panels panel_chrom[n_panels] (1-based chromosome numbers).  HOST pointers.
 *   entries_out float64 [n_samples, n_panels, capacity, 9], rows (kind, panel, x0, x1, y0, y1, colour id, alpha, value)
 *   in data coordinates, counts_out int32 [n_samples, n_panels] the entries every panel NEEDS.  Per panel: one kind 0
 *   entry (x1 = bins, y0 / y1 = min / max of the finite z-scores, +inf / -inf when there is none, value = the number of
 *   kind 2 entries), one kind 2 entry per stretch of bins whose z == 0 ([first - 0.5, last + 0.5] x [-thr, thr],
 *   colour 7, alpha 0.5), one kind 3 entry per call of the chromosome with abs(effect) * 100 >= mineffect ([start - 0.5,
 *   end + 0.5] x [0, thr], -thr when z < 0; colour 1 below abs(effect) 0.2, else 3; alpha min(1, abs(effect) * 10); value
 *   z).  A panel that needs more than `capacity` entries keeps the first `capacity` and sets bit 0 of *status_out (the
 *   call still returns WC_OK); wc_plot_batch sizes its lists for the worst case, 1 + ceil(bins / 2) + max_calls.
 * wc_plot_batch_dev: list, raster, Adler-32 and deflate for n_samples images of width x height pixels, enqueued on
 *   `stream` without synchronising.  results_z / calls / n_calls are DEVICE pointers, the tables are HOST memory:
 *   bands_host [n_bands, 4] rows (x0, x1, alpha, hatch 0 / 1 '//' / 2 '\' / -1: a band of the table that gets no
 *   rectangle) in bins with band_off_host int32 [n_panels + 1] (NULL: no cytoband file); a panel with any row, drawn or
 *   not, gets the grey line at -1.5 threshold, as the reference draws it once per band of the table; names_host [n_samples, name_cap] NUL-padded sample names.  Outputs, all
 *   DEVICE memory: streams (the raw deflate stream of image i at i * out_stride, out_stride >= wc_deflate_bound(
 *   wc_plot_image_bytes(width, height))), out_len, adler, *status (as wc_plot_list's), and, unless NULL, scanlines: image
 *   i in PNG scanline layout (per row a filter byte 0 and 3 * width bytes) at i * scan_stride, scan_stride a multiple
 *   of 16.  It uses wc_deflate_rows_dev and shares its rule: one call in flight per context.  WC_E_LIMIT: more images
 *   or larger ones than that call accepts, or more than 65535 images.  threshold must be positive and finite.
 *   The tables are copied from pinned memory of the context; the next call waits for that copy (not for the kernels)
 *   before it writes the block again.
 * wc_plot_batch: the same from HOST pointers, synchronising (the bytes of streams_out behind a stream are not
 *   written); scanlines_out (may be NULL) is [n_samples,
 *   wc_plot_image_bytes]; times_ms (may be NULL) double [8]: milliseconds of [0] copy in [1] list [2] raster
 *   [3] Adler-32 [4] deflate [5] copy out.  A list beyond its capacity is WC_E_INTERNAL here.
 * wc_adler32_rows_dev: adler[i] = zlib.adler32 of row i (n_rows <= 65535 rows of row_bytes bytes, src_stride apart),
 *   as blockwise sums modulo 65521 combined in order.  DEVICE pointers, enqueues on `stream`.
 * wc_png_bytes / wc_png_assemble (host): the file of one image: signature, IHDR (8-bit RGB), one IDAT chunk = 78 01 +
 *   the raw deflate stream + the big-endian Adler-32, IEND; wc_png_bytes(deflate_len) is its size.                  */
int wc_plot_layout(int width, int height, int rows, int columns, int n_panels, int32_t *boxes_out);
int64_t wc_plot_image_bytes(int width, int height);
int wc_plot_list(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                 const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                 const int32_t *panel_chrom, int n_panels, int capacity, double *entries_out, int32_t *counts_out, int32_t *status_out);
int wc_plot_batch_dev(wc_ctx *ctx, void *stream, const double *results_z, int64_t row_stride, int64_t n_samples,
                      const int64_t *chrom_sizes_host, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls,
                      double threshold, double mineffect, const int32_t *panel_chrom_host, int n_panels, int columns,
                      const double *bands_host, const int32_t *band_off_host, const char *names_host, int name_cap, int width, int height,
                      int dpi, unsigned char *scanlines, int64_t scan_stride, unsigned char *streams, int64_t out_stride, int64_t *out_len,
                      uint32_t *adler, int32_t *status);
int wc_plot_batch(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                  const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                  const int32_t *panel_chrom, int n_panels, int columns, const double *bands, const int32_t *band_off, const char *names,
                  int name_cap, int width, int height, int dpi, unsigned char *scanlines_out, unsigned char *streams_out,
                  int64_t out_stride, int64_t *out_len, uint32_t *adler_out, double *times_ms);
int wc_adler32_rows_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, int64_t row_bytes, int64_t src_stride,
                        uint32_t *adler);
int64_t wc_png_bytes(int64_t deflate_len);
int wc_png_assemble(int width, int height, const unsigned char *deflate, int64_t deflate_len, uint32_t adler, unsigned char *out,
                    int64_t cap, int64_t *out_len);

/* ---- plotpdf: result files -> vector PDF pages, the content stream written on the device ------
 * The same display list as plotbatch, drawn as PDF operators.  All geometry is in centipoints (1 / 100 pt): the page is
 * width_cp x height_cp, the panel boxes are wc_plot_layout(width_cp, height_cp, ...), the mappings are the rasteriser's
 * with the box in centipoints, q = floor(v + 0.5) limited to +-9 999 999, the flip is height_cp - qy, and every number is
 * one field of 9 bytes (right-aligned: an optional '-', the whole points, '.', two digits).  A page's content is a row of
 * sections; a section is a run of records of one kind and one width, each ending in '\n'; a record with nothing to draw
 * is spaces.  Per panel, in the painter's order: head (q, the box as clip path; 1 x 49 bytes), cytobands (the table's rows
 * x 138), list rectangles (slots x 73: uncallable patches, then calls), the four grey lines (4 x 81), two edge lines per
 * slot (slots x 162), the polyline's head (1 x 57), one vertex per bin (bins x 22), S (1 x 2), labels (slots x 96), frame
 * and Q (1 x 82), the chromosome number (1 x 96); behind the last panel the title (1 x 73 + 2 * (45 + name_cap - 1)) and
 * the legend (4 x 179).  slots of a panel = the longest list among the samples of the call, less its range entry: every
 * sample of a call has the same row_bytes and the same section starts.
 *
 * wc_plot_pdf_sections (host): the section starts for given slots (int32 [n_panels]) into starts_out (may be NULL) int64
 *   [11 * n_panels + 3], the last entry and the return value the row's bytes; -1: unusable arguments.
 * wc_plot_pdf_row_bound (host): the most bytes a page can take: ceil(bins / 2) + max_calls slots in every panel.
 * wc_plot_pdf_batch_dev: list, content, Adler-32 and deflate for n_samples pages.  Inputs as wc_plot_batch_dev's
 *   (results_z / calls / n_calls DEVICE pointers in the layout wc_test_batch_dev leaves them, the tables HOST memory).
 *   IT SYNCHRONISES `stream` ONCE, behind the list kernel, to read the lists' counts back (one small copy): the slot
 *   counts size the sections.  Everything behind that is enqueued without synchronising.  Outputs, DEVICE memory:
 *   content (may be NULL: the context keeps it) page i's uncompressed content at i * content_stride, a multiple of 16 and
 *   at least wc_plot_pdf_row_bound rounded up to one (the bytes from the row's end to the next multiple of 16 are written
 *   as spaces); streams (raw deflate, page i at i * out_stride, out_stride >= wc_deflate_bound(wc_plot_pdf_row_bound));
 *   out_len; adler; *status (as wc_plot_list's).  HOST outputs, valid on return: *row_bytes_host the row_bytes used,
 *   offsets_host (may be NULL) as wc_plot_pdf_sections' starts_out.  It uses wc_deflate_rows_dev and shares its rule: one
 *   call in flight per context.  WC_E_LIMIT, before anything runs: more pages, or a larger bound, than that call accepts,
 *   or more than 65535 pages.  threshold must be positive and finite, the page at most 1 440 000 centipoints each way.
 * wc_plot_pdf_batch: the same from HOST pointers, synchronising.  content_out (may be NULL) [n_samples, content_stride],
 *   row_bytes of every row written; streams_out rows out_stride >= wc_deflate_bound(wc_plot_pdf_row_bound) apart, only
 *   out_len[i] bytes of each written; times_ms (may be NULL) double [8]: milliseconds of [0] copy in [1] list and the
 *   counts' way back [2] content [3] Adler-32 [4] deflate [5] copy out.
 * wc_pdf_bytes / wc_pdf_assemble (host): the file around one content stream: %PDF-1.4 and a binary comment; Catalog,
 *   Pages, Page (MediaBox [0 0 width_cp / 100 height_cp / 100]); the font /Courier; the ExtGState dictionary /A000 ..
 *   /A255 (/ca and /CA = a / 255); the two tiling patterns /P1 ('//') and /P2 ('\'); the content object (/Filter
 *   /FlateDecode /Length n, data = 78 01 + the raw stream + the big-endian Adler-32); a classic xref table with 20-byte
 *   entries; trailer, startxref, %%EOF.  No /Info, no date, no /ID: the bytes depend on the inputs alone, and
 *   wc_pdf_bytes(deflate_len) is the file's size whatever the page (numbers that vary stand in fixed-width fields). */
int64_t wc_plot_pdf_sections(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, const int32_t *band_off,
                             const int32_t *slots, int name_cap, int64_t *starts_out);
int64_t wc_plot_pdf_row_bound(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, const int32_t *band_off,
                              int max_calls, int name_cap);
int wc_plot_pdf_batch_dev(wc_ctx *ctx, void *stream, const double *results_z, int64_t row_stride, int64_t n_samples,
                          const int64_t *chrom_sizes_host, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls,
                          double threshold, double mineffect, const int32_t *panel_chrom_host, int n_panels, int columns,
                          const double *bands_host, const int32_t *band_off_host, const char *names_host, int name_cap, int width_cp,
                          int height_cp, unsigned char *content, int64_t content_stride, unsigned char *streams, int64_t out_stride,
                          int64_t *out_len, uint32_t *adler, int64_t *row_bytes_host, int64_t *offsets_host, int32_t *status);
int wc_plot_pdf_batch(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                      const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                      const int32_t *panel_chrom, int n_panels, int columns, const double *bands, const int32_t *band_off, const char *names,
                      int name_cap, int width_cp, int height_cp, unsigned char *content_out, int64_t content_stride,
                      unsigned char *streams_out, int64_t out_stride, int64_t *out_len, uint32_t *adler_out, int64_t *row_bytes_out,
                      int64_t *offsets_out, double *times_ms);
int64_t wc_pdf_bytes(int64_t deflate_len);
int wc_pdf_assemble(int width_cp, int height_cp, const unsigned char *deflate, int64_t deflate_len, uint32_t adler, unsigned char *out,
                    int64_t cap, int64_t *out_len);

/* ---- exportjson: result rows -> lossless JSON text, the digits made on the device ------------
 * A value's text is what CPython's float.__repr__ / json.dumps gives, byte for byte: the shortest digits that read
 * back to the same double (the closest of them, a tie to even), positional or d.ddde+XX as repr chooses, ".0" behind
 * whole numbers, "-0.0"; at most 24 bytes.  Not finite: Infinity, -Infinity, NaN (sign and payload of a NaN are
 * dropped); with strict != 0 all three are null.  The digits are Ryu's, exact for every double (csrc/fmt_double.h).
 *
 * wc_format_doubles_host (host only, no GPU needed): text [n, 24] = the text of v[i] padded with zero bytes, len[i]
 *   its length.  wc_format_doubles: the same from the device's kernel; HOST pointers, synchronising.  WC_E_LIMIT:
 *   more than INT_MAX / 24 values.
 * wc_json_row_bound (host): the most bytes a row's text takes: 25 per value + 2 per chromosome + 2, and 1 more for
 *   every empty chromosome beyond the first ("[]," is three bytes); -1: a negative size, more than 64 chromosomes or
 *   more than INT_MAX - 512 values.
 * wc_json_rows_dev: row i of `rows` (DEVICE float64, row_stride elements apart, the dense layout wc_test_batch_dev
 *   leaves: chromosome c at the sum of the sizes before it) becomes the compact text [[v,v,...],[...],...]: no white
 *   space, a chromosome of length 0 is [], no chromosome at all is [].  text_len[i] (DEVICE int64) bytes at text +
 *   i * text_stride (DEVICE), dense.  BYTES BEHIND text_len[i] ARE NOT WRITTEN.  text is 16-byte aligned and
 *   text_stride a multiple of 16, at least wc_json_row_bound.  chrom_sizes_host is HOST memory and travels as a kernel
 *   argument.  Enqueues on `stream` without synchronising, except that a call which has to grow the context's working
 *   memory (16 bytes per value, 12 per 256 values) allocates, which waits for the device; one call in flight per
 *   context.  Refused before anything runs, outputs untouched: WC_E_ARG for a negative size or row count, a
 *   row_stride below the row's values, a text_stride below the bound or no multiple of 16, a NULL pointer; WC_E_LIMIT
 *   for more than 65535 rows, more than 64 chromosomes, more than INT_MAX - 512 values in a row.
 * wc_json_rows: the same from HOST pointers, synchronising; text rows need no alignment, only text_len[i] bytes of
 *   each are written.  times_ms (may be NULL) double [4]: milliseconds of [0] copy in [1] lengths and scan [2] bytes
 *   [3] copy out.
 * wc_gzip_bytes / wc_gzip_assemble (host): one gzip member around a raw deflate stream: the fixed header 1f 8b 08 00,
 *   no time, no name, XFL 0, OS 255; the stream; CRC-32 and ISIZE (input_len modulo 2^32), little-endian.
 *   wc_gzip_bytes(deflate_len) = deflate_len + 18 is its size; a smaller cap is WC_E_ARG.  The bytes depend on the
 *   arguments alone.  Members in a row read as one stream.                                                       */
int wc_format_doubles_host(const double *v, int64_t n, int strict, char *text, uint8_t *len);
int wc_format_doubles(wc_ctx *ctx, const double *v, int64_t n, int strict, char *text, uint8_t *len);
int64_t wc_json_row_bound(const int64_t *chrom_sizes, int n_chrom);
int wc_json_rows_dev(wc_ctx *ctx, void *stream, const double *rows, int64_t row_stride, int64_t n_rows,
                     const int64_t *chrom_sizes_host, int n_chrom, int strict, unsigned char *text, int64_t text_stride,
                     int64_t *text_len);
int wc_json_rows(wc_ctx *ctx, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes, int n_chrom,
                 int strict, unsigned char *text, int64_t text_stride, int64_t *text_len, double *times_ms);
int64_t wc_gzip_bytes(int64_t deflate_len);
int wc_gzip_assemble(const unsigned char *deflate, int64_t deflate_len, uint32_t crc, int64_t input_len, unsigned char *out,
                     int64_t cap, int64_t *out_len);

/* ---- exporttracks: result rows -> bedGraph text, BGZF on the device ---------------------------------
 * A row is the dense layout of wc_json_rows_dev.  Chromosome c (0-based) is named prefix + decimal(c + 1); inside a
 * chromosome a RUN is a maximal stretch of bins a..b whose doubles have the same 64 bits (-0.0 beside 0.0: two runs).
 * A run is one line
 *     name \t a * binsize \t min((b + 1) * binsize, clip_len[c]) \t value \n
 * with the value's text as wc_format_doubles_host writes it (not strict).  A run that is not finite is left out; with
 * bit 0 of flags set (nozero) a run of 0.0 of either sign too.  No header, no track line; a row with nothing kept is
 * 0 bytes.
 *
 * wc_bedgraph_row_bound (host): the most bytes a row's text takes, every bin a line of its own:
 *     sum over the chromosomes with n > 0 bins of
 *         n * (prefix_len + digits(c + 1) + digits((n - 1) * binsize) + digits(n * binsize) + 28)
 *   (28 = three tabs, the newline and 24 bytes of value).  -1 for arguments wc_bedgraph_rows_dev refuses.
 * wc_bedgraph_rows_dev: text_len[i] (DEVICE int64) bytes at text + i * text_stride (DEVICE), dense; dropped[i]
 *   (DEVICE int64) the row's bins that are not finite.  BYTES BEHIND text_len[i] ARE NOT WRITTEN.  text is 16-byte
 *   aligned and text_stride a multiple of 16, at least the bound.  chrom_sizes_host, clip_len_host (may be NULL:
 *   nothing is clipped) and prefix are HOST memory and travel as a kernel argument.  Three kernel launches on
 *   `stream`, no synchronisation, except that a call which has to grow the context's working memory (shared with
 *   wc_json_rows_dev: 16 bytes per value, 16 per 256 values) allocates, which waits for the device; one call in flight
 *   per context.  Refused before anything runs, outputs untouched: WC_E_ARG for a negative size or row count, a
 *   binsize below 1, a row_stride below the row's values, a text_stride below the bound or no multiple of 16, a NULL
 *   pointer, a prefix of more than 16 bytes or with a byte that is 0, a tab, a newline or not ASCII, a flag bit other
 *   than bit 0, a clip_len[c] at or below the start of chromosome c's last bin; WC_E_LIMIT for more than 65535 rows,
 *   more than 64 chromosomes, more than INT_MAX - 512 bins in a row, a chromosome whose bins * binsize reaches 10^15
 *   (every coordinate has at most 15 digits).
 * wc_bedgraph_rows: the same from HOST pointers, synchronising; text rows need no alignment, only text_len[i] bytes
 *   of each are written.  times_ms (may be NULL) double [4]: milliseconds of [0] copy in [1] lengths and scan
 *   [2] bytes [3] copy out.
 *
 * wc_bgzf_rows_dev: the first row_len[i] (DEVICE int64, read on the device) bytes of row i of src (DEVICE, src_stride
 *   apart) become a BGZF file (the SAM specification, section 4.1) of out_len[i] (DEVICE int64) bytes at out +
 *   i * out_stride: the bytes are cut into blocks of wc_deflate_block_bytes input bytes, each coded as
 *   wc_deflate_rows_dev codes a row's last block (the same tokens and Huffman code, a stored block where that is
 *   shorter, the final bit set) and framed by the 18-byte header with the BC extra field and BSIZE - 1, the block's
 *   own CRC-32 and its ISIZE; the 28-byte end-of-file block closes the row, and is all of a row of 0 bytes.  The grid
 *   is sized by max_row_bytes and the blocks behind a row's end do nothing: one call serves rows of unequal lengths
 *   without a read-back.  A row_len[i] outside 0 .. max_row_bytes gives out_len[i] = -1 and nothing else for that
 *   row.  out_stride is at least wc_bgzf_bound of max_row_bytes: row_bytes + 31 per block + 28.  Bytes behind
 *   out_len[i] are not written.  Two kernel launches, no synchronisation unless the working memory grows (shared
 *   with wc_deflate_rows_dev, 16 400 bytes per block of the grid).
 * wc_bgzf_rows: the same from HOST pointers, synchronising; a row_len[i] outside 0 .. max_row_bytes is WC_E_ARG.    */
int64_t wc_bedgraph_row_bound(const int64_t *chrom_sizes, int n_chrom, int64_t binsize, int prefix_len);
int wc_bedgraph_rows_dev(wc_ctx *ctx, void *stream, const double *rows, int64_t row_stride, int64_t n_rows,
                         const int64_t *chrom_sizes_host, int n_chrom, int64_t binsize, const int64_t *clip_len_host, const char *prefix,
                         int prefix_len, int flags, unsigned char *text, int64_t text_stride, int64_t *text_len, int64_t *dropped);
int wc_bedgraph_rows(wc_ctx *ctx, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes, int n_chrom,
                     int64_t binsize, const int64_t *clip_len, const char *prefix, int prefix_len, int flags, unsigned char *text,
                     int64_t text_stride, int64_t *text_len, int64_t *dropped, double *times_ms);
int64_t wc_bgzf_bound(int64_t row_bytes);
int wc_bgzf_rows_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t max_row_bytes,
                     int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len);
int wc_bgzf_rows(wc_ctx *ctx, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t max_row_bytes, int64_t src_stride,
                 unsigned char *out, int64_t out_stride, int64_t *out_len);

/* ---- sensitivity: planted aberrations, spiked and judged on the device --------------------------------
 * A PLAN is HOST memory in every call, int32 [n_trials, 5]: rows {base row, chromosome (1-based), first bin, bins, effect
 *   in ppm}.  Bins are the chromosome's own bins in the chromosome_sizes layout (masked bins count); the span is
 *   first .. first + bins - 1.  The effect is parts per million of the read depth, -1 000 000 .. +100 000 000; 0 is a
 *   control trial, in which nothing is planted and nothing can match.  Every call checks every row before anything is
 *   uploaded or launched and returns WC_E_ARG with the first bad row named in the error text, outputs untouched:
 *   a base row outside 0 .. n_base - 1, a chromosome outside 1 .. n_chrom, first < 0, bins < 1, first + bins beyond the
 *   chromosome's size, an effect out of range.  (The score has no sizes: it checks first, bins and the effect, and a
 *   chromosome >= 1.)  One call in flight per context: the checked plan lives in the context.
 * wc_spike_counts_dev: out [n_trials, n_total] int32 (DEVICE, n_total = sum(chrom_sizes)) = row plan[i][0] of base
 *   [n_base, n_total] int32 (DEVICE), and inside the span every count c >= 0 becomes
 *   min(2^31 - 1, (c * (1 000 000 + ppm) + 500 000) div 1 000 000) in 64-bit integers (half up, exact, no float); counts
 *   below 0 and every bin outside the span are copied bit for bit.  saturated (DEVICE int64, may be NULL): how many bins
 *   the minimum clipped.  base and out must not overlap and are aligned to 4 bytes; out need not be aligned to 16.
 *   Enqueued on `stream`, nothing is waited for.  At most 2^31 - 9 bins in a row.
 * wc_spike_counts: the same from HOST pointers (saturated: HOST int64, may be NULL), synchronising.
 * wc_spike_score_dev: calls [n_trials, max_calls, 5] float64 rows [chrom, start, end, z, effect] and n_calls [n_trials]
 *   int32 (DEVICE, the layout wc_test_batch_dev leaves; rows at and behind n_calls[i] are not read, n_calls is taken
 *   as clipped to 0 .. max_calls).  start and end are compared as int64.  A call MATCHES trial i with span [s, e] on
 *   chromosome c when its chromosome is c, its z has the effect's sign (z > 0 for a gain, z < 0 for a loss; NaN, +0.0 and
 *   -0.0 match nothing) and min(e, end) - max(s, start) + 1 >= 1.
 *   rec_i [n_trials, 8] int32 (DEVICE): {n_calls, n_match, overlap_bins (the sum of the matching calls' overlaps),
 *   match_bins (the sum of their lengths end - start + 1), best_row (the matching call with the largest overlap, the
 *   earliest row on a tie; -1: none), best_start, best_end (that call's; -1: none), 0}; the sums are formed in 64 bits
 *   and stored clipped to 2^31 - 1.  rec_f [n_trials, 2] float64 (DEVICE): {best z, best effect}, copies of the stored
 *   doubles, NaN when there is none.  Nothing in a record depends on a summation order.
 * wc_spike_score: the same from HOST pointers, synchronising.
 * wc_sensitivity_batch_dev: spike, then wc_test_batch_dev on the spiked rows, then the score, all on `stream` and on the
 *   context's workspaces, with no wait between the stages besides those of wc_test_batch_dev.  chrom_sizes MUST be the
 *   chromosome_sizes the reference was created with (the handle is opaque here, so, like the row length of the counts
 *   wc_test_batch_dev takes, this is not checked).  threshold .. max_calls are passed on as they are, and so is every
 *   error of that call (WC_E_LIMIT "max_calls": run the trials again with more room).  At most 60000 trials x selected
 *   chromosomes per call.  rec_i, rec_f: as above; calls, n_calls (DEVICE, either may be NULL: the context's own) receive
 *   what the test found.  The dense per-bin outputs of the test go to the context's workspaces and are not returned.      */
int wc_spike_counts_dev(wc_ctx *ctx, void *stream, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                        const int32_t *plan_host, int64_t n_trials, int32_t *out, int64_t *saturated);
int wc_spike_counts(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *plan,
                    int64_t n_trials, int32_t *out, int64_t *saturated);
int wc_spike_score_dev(wc_ctx *ctx, void *stream, const int32_t *plan_host, int64_t n_trials, const double *calls, const int32_t *n_calls,
                       int max_calls, int32_t *rec_i, double *rec_f);
int wc_spike_score(wc_ctx *ctx, const int32_t *plan, int64_t n_trials, const double *calls, const int32_t *n_calls, int max_calls,
                   int32_t *rec_i, double *rec_f);
int wc_sensitivity_batch_dev(wc_ctx *ctx, void *stream, const wc_reference *ref, const int32_t *base, int64_t n_base,
                             const int64_t *chrom_sizes_host, int n_chrom, const int32_t *plan_host, int64_t n_trials, double threshold,
                             int min_ref_bins, int repeats, double min_effect, const int32_t *chromosomes_host, int n_sel, int max_calls,
                             int32_t *rec_i, double *rec_f, double *calls, int32_t *n_calls);

/* ---- sensitivity: reproducible binomial draws on the device ---------------------------------------------
 * The generator is Philox4x32-10 (Random123: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten
 *   rounds) under the key (seed low 32 bits, seed high 32 bits).  B(c, f), c >= 0 reads and f parts per million
 *   (0 .. 1 000 000): read r (0 <= r < c) is kept when its 32-bit word, as 64 bits, is below T = (f << 32) div 1 000 000;
 *   B counts the kept reads (f = 1 000 000 keeps all, f = 0 none).  Read r takes word r & 3 of the block with counter
 *   (c0 = bin within its chromosome, c1 = chromosome (1-based) | tag << 16, c2 = r >> 2, c3 = row id).  Tag 1 is thinning,
 *   tag 2 the spike.  The counter names chromosome and bin, never a flat index or a batch position.
 * wc_philox4x32_host (no GPU needed): out [n, 4] = the block of counters [n, 4] under keys [n, 2], all uint32 HOST.
 * wc_philox4x32: the same by the device function, through a kernel; HOST pointers, synchronising, n >= 1.
 * wc_philox_spin_dev (a measuring aid): every one of `lanes` lanes (a multiple of 256, at most 2^30) runs `blocks` (at most
 *   2^24) blocks over registers and stores the exclusive-or of their words to out [lanes] uint32 (DEVICE); enqueued on
 *   `stream`.  The rate of the rounds with no memory in the loop: what the thinning kernel's rate is held against.
 * wc_thin_counts_dev: out [n_keep, n_base, n_total] int32 (DEVICE) of base [n_base, n_total] int32 (DEVICE): depth d holds
 *   B(c, keep_ppm[d]) with tag 1 and row id b in every bin of base row b; counts below 0 are copied.  The depth is NOT in
 *   the counter: all depths of a base row use the same words, so a bin's count never rises as keep_ppm falls, and a
 *   depth of 1 000 000 is a copy.  Checked on the host first, the first bad argument named (WC_E_ARG): n_base >= 1,
 *   1 .. WC_MAX_CHROM (64) chromosomes of >= 0 bins and fewer than 2^31 - 8 in a row, n_keep 1 .. 8, every keep_ppm
 *   1 .. 1 000 000 (HOST int32).  A bin with more than 2^24 reads is refused with WC_E_LIMIT, the base row and the flat bin
 *   named and NOTHING written to out: a kernel looks for one first and the call waits on `stream` for its status word
 *   (the call's one wait); the thinning itself is enqueued and not waited for.  base and out must not overlap.
 * wc_thin_counts: the same from HOST pointers, synchronising.
 * wc_thin_wave_cutoff: the reads from which the thinning kernel's wave takes a bin together instead of leaving it to its
 *   lane (for tests that stand on either side of it; the result does not depend on which form ran).
 * wc_spike_counts_ex_dev / wc_spike_counts_ex: wc_spike_counts_dev / wc_spike_counts with the rule chosen.  draw == 0: the
 *   deterministic rule above, bit for bit (seed and trial0 are not looked at beyond their check).  draw == 1: the binomial
 *   spike: with m = 1 000 000 + ppm, whole = m div 1 000 000 and frac = m mod 1 000 000, a count c >= 0 inside the span
 *   becomes min(2^31 - 1, c * whole + B(c, frac)) with tag 2 and row id trial0 + i for plan row i, so a plan cut into
 *   batches gives the uncut plan's rows when every batch passes its global offset.  Its expectation is the deterministic
 *   rule's value, and a ppm that is a multiple of 1 000 000 gives that rule's bits.  WC_E_ARG for draw outside {0, 1},
 *   trial0 < 0 or trial0 + n_trials > 2^32.  A span bin costs ceil(c / 4) blocks spread over a wave.
 * wc_sensitivity_batch_ex_dev: wc_sensitivity_batch_dev likewise.  The first names call these with draw = 0.          */
int wc_philox4x32_host(const uint32_t *counters, const uint32_t *keys, int64_t n, uint32_t *out);
int wc_philox4x32(wc_ctx *ctx, const uint32_t *counters, const uint32_t *keys, int64_t n, uint32_t *out);
int wc_philox_spin_dev(wc_ctx *ctx, void *stream, int64_t lanes, int64_t blocks, uint64_t seed, uint32_t *out);
int wc_thin_counts_dev(wc_ctx *ctx, void *stream, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                       const int32_t *keep_ppm_host, int n_keep, uint64_t seed, int32_t *out);
int wc_thin_counts(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *keep_ppm, int n_keep,
                   uint64_t seed, int32_t *out);
int wc_thin_wave_cutoff(void);
int wc_spike_counts_ex_dev(wc_ctx *ctx, void *stream, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes_host, int n_chrom,
                           const int32_t *plan_host, int64_t n_trials, int draw, uint64_t seed, int64_t trial0, int32_t *out, int64_t *saturated);
int wc_spike_counts_ex(wc_ctx *ctx, const int32_t *base, int64_t n_base, const int64_t *chrom_sizes, int n_chrom, const int32_t *plan,
                       int64_t n_trials, int draw, uint64_t seed, int64_t trial0, int32_t *out, int64_t *saturated);
int wc_sensitivity_batch_ex_dev(wc_ctx *ctx, void *stream, const wc_reference *ref, const int32_t *base, int64_t n_base,
                                const int64_t *chrom_sizes_host, int n_chrom, const int32_t *plan_host, int64_t n_trials, int draw, uint64_t seed,
                                int64_t trial0, double threshold, int min_ref_bins, int repeats, double min_effect,
                                const int32_t *chromosomes_host, int n_sel, int max_calls, int32_t *rec_i, double *rec_f, double *calls,
                                int32_t *n_calls);

/* ---- crossval: the held-out z-scores of a healthy cohort, judged on the device --------------------------
 * wc_crossval_stats_dev: Z [n_samples, row_stride] float64 (DEVICE; n_total = sum(chrom_sizes) <= row_stride bins of a row
 *   are read: the dense layout wc_test_batch_dev leaves), thr and asdef [n_samples] float64 (DEVICE: the per-bin |z| cut
 *   and the asdef of every sample), calls [n_samples, max_calls, 5] float64 rows [chrom, start, end, z, effect] and n_calls
 *   [n_samples] int32 (DEVICE; rows at and behind n_calls[i] are not read, n_calls is taken as clipped to 0 .. max_calls).
 *   chrom_sizes, sel (the selected chromosomes, 1-based, each once) and lengths (the window lengths) are HOST memory.
 *   With z = Z[i][b], i ascending:
 *   Classes: a bin is TESTED when z != 0 (so +0.0 and -0.0, the fill of masked and removed bins, are untested and NaN is
 *     tested), NONFINITE when tested and not finite, else FINITE.
 *   bins_i [n_total, 6] int32: {tested, nonfinite, over_hi (finite and z >= thr[i]), over_lo (finite and z <= -thr[i]),
 *     in_gain, in_loss}: the call rows whose [start, end] (inclusive, the chromosome's own bins) covers the bin, a row with
 *     z > 0 a gain and one with z < 0 a loss.
 *   bins_f [n_total, 2] float64: {sum z, sum z * z} over the bin's finite samples, added one sample after the other in
 *     ascending i from 0.0, every product rounded before it is added (no fused multiply-add).
 *   rec_i [n_samples, 8] int32: {0 (the caller's: the sample's fold), n_calls, tested, nonfinite, over_hi, over_lo,
 *     call_bins = sum(end - start + 1), rows_skipped}, the sums formed in 64 bits and stored clipped to 2^31 - 1.
 *   rec_f [n_samples, 4] float64: {asdef[i], thr[i], the largest finite z, the smallest finite z}; the last two are NaN
 *     when the sample has no finite z.
 *   Windows: for sample i and selected chromosome c, t = the chromosome's tested values in bin order, n of them.  A row with
 *     a nonfinite value is skipped and counted in rows_skipped.  Otherwise P[0] = 0, P[j + 1] = P[j] + t[j], sequentially,
 *     and for every length L and every a in 0 .. n - L: w = (P[a + L] - P[a]) / sqrt((double)L).
 *   win_n [n_samples, n_lengths] int64: windows per sample and length.
 *   win_i [n_lengths, 4] int64: {rows (not skipped, with a window of this length at least: n >= L), windows,
 *     hi (w >= thr[i]), lo (w <= -thr[i])}.
 *   win_hist [n_lengths, 130] int64: slot 0 for w < -16, slot 129 for w >= 16 or NaN, else 1 + (int)floor((w + 16.0) * 4.0).
 *   Refused with WC_E_ARG before any output is written: NULL pointers, n_samples < 1, a layout outside 1 .. WC_MAX_CHROM
 *     chromosomes of fewer than 2^31 - 8 bins in a row, row_stride < n_total, max_calls < 1, n_sel outside 1 .. n_chrom, a
 *     selected chromosome outside 1 .. n_chrom or named twice, n_lengths outside 1 .. 16, a length < 1 or not above the one
 *     before it -- and a call row whose chromosome is no whole number in 1 .. n_chrom or whose span is not whole numbers
 *     0 <= start <= end < the chromosome's bins: a kernel looks for one and the call waits on `stream` for its status word
 *     (the call's one wait; the first such row is named), so a call row is never clipped silently and never indexed.  The
 *     rest is enqueued and not waited for.  One call in flight per context.
 * wc_crossval_stats: the same from HOST pointers, synchronising.                                                          */
int wc_crossval_stats_dev(wc_ctx *ctx, void *stream, const double *Z, int64_t row_stride, int64_t n_samples,
                          const int64_t *chrom_sizes_host, int n_chrom, const double *thr, const double *asdef, const double *calls,
                          const int32_t *n_calls, int max_calls, const int32_t *sel_host, int n_sel, const int32_t *lengths_host,
                          int n_lengths, int32_t *bins_i, double *bins_f, int32_t *rec_i, double *rec_f, int64_t *win_n, int64_t *win_i,
                          int64_t *win_hist);
int wc_crossval_stats(wc_ctx *ctx, const double *Z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                      const double *thr, const double *asdef, const double *calls, const int32_t *n_calls, int max_calls, const int32_t *sel,
                      int n_sel, const int32_t *lengths, int n_lengths, int32_t *bins_i, double *bins_f, int32_t *rec_i, double *rec_f,
                      int64_t *win_n, int64_t *win_i, int64_t *win_hist);

/* ---- robust column statistics: the median and the median absolute deviation of every column ------------
 * wc_column_robust_dev: Z [n_rows, row_stride] float64 (DEVICE; n_cols <= row_stride columns of a row are read), col_i
 *   [n_cols, 2] int32 and col_f [n_cols, 2] float64 (DEVICE).  For column b, with z = Z[i * row_stride + b], i = 0 .. n_rows - 1:
 *   Classes: crossval's.  TESTED when z != 0 (so +0.0 and -0.0 are untested and NaN is tested), NONFINITE when tested and
 *     not finite, else FINITE.
 *   col_i[b] = {finite, nonfinite}.
 *   Median: v = the column's FINITE values, n of them, s = the same in ascending order.  med(s) = s[(n - 1) / 2] for odd n and
 *     (s[n / 2 - 1] + s[n / 2]) / 2.0 for even n, the sum rounded first.
 *   col_f[b][0] = med(s), NaN when n == 0.
 *   col_f[b][1] = med of d_i = fabs(v_i - col_f[b][0]), every difference rounded, sorted ascending; NaN when n == 0 or the
 *     median is not finite (the two middle values overflowed).  d can be zero, and then +0.0; it can be +inf.
 *   For nonzero finite input this is np.median(v) and np.median(np.abs(v - np.median(v))) bit for bit.  The selection is
 *   exact (a radix selection over the values' bits): no sum enters but the one of the middle pair.
 *   Refused before anything is written: WC_E_ARG for NULL pointers, n_rows < 1, n_cols < 1 (or above 2^31 - 1),
 *     row_stride < n_cols; WC_E_LIMIT for n_rows > 8192.  The work is enqueued on `stream` and not waited for.
 * wc_column_robust: the same from HOST pointers, synchronising (of Z's last row only n_cols values are read).           */
int wc_column_robust_dev(wc_ctx *ctx, void *stream, const double *Z, int64_t row_stride, int64_t n_rows, int64_t n_cols,
                         int32_t *col_i, double *col_f);
int wc_column_robust(wc_ctx *ctx, const double *Z, int64_t row_stride, int64_t n_rows, int64_t n_cols, int32_t *col_i,
                     double *col_f);

#ifdef __cplusplus
}
#endif
#endif /* WISECONDOR_HIP_H */
