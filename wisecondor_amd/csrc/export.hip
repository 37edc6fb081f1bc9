// exportjson: dense float64 rows -> the compact JSON text [[v,v,...],[...],...] of every row, the digits made on the
// device (the digit routine is fmt_double.h).  A row's values are cut into tiles of JS_T values, a
// workgroup per tile and a lane per value; a value's FIELD is its text and what follows it up to the next value: a
// comma inside a chromosome, behind a chromosome's last value the brackets and commas up to the next value or the
// row's end.  What stands in front of the first value is the row's HEAD; it depends on the chromosome sizes alone.
//   k_js_len     the decimal digits of every value (16 bytes: an integer of up to 17 digits, its power of ten, class and
//                sign) into the call's slots, and the sum of the tile's field lengths
//   k_js_scan    a workgroup per row: the exclusive sum of the tile sums, and text_len = head + their total
//   k_js_bytes   the tile's fields from the slots: an exclusive sum of the field lengths inside the tile, every lane
//                writes its field into the tile's image in LDS, and after one barrier the image goes out in aligned
//                16-byte stores; the image's first and last 16 bytes, which a neighbouring tile shares, go out byte by
//                byte.  Tile 0 writes the head.  Bytes behind text_len[i] are NOT written.
//   k_js_format  wc_format_doubles: a lane per value, text [n, 24] padded with zero bytes, and the lengths
// Nothing synchronises; the chromosome table travels as a kernel argument.
#include <limits.h>

#include "ctx.h"
#include "fmt_double.h"
#include "text_rows.h"
#include "tile_text.h"

namespace {

const int JS_T = TT_T;                  // values per tile = lanes per workgroup (the kernels' one tile and trip size; tile_text.h)
const int JS_IMG = 32 * JS_T;           // bytes of a tile's image: two 16-byte lines per lane
// the most a tile's image holds: up to 15 bytes in front (the image starts on a multiple of 16), the head (tile 0), JS_T
// fields of 24 bytes and a comma or bracket each, and at most once per call the rest of the brackets and commas
const int JS_STRUCT = 3 * WC_MAX_CHROM + 1;
static_assert(15 + JS_STRUCT + JS_T * (FD_MAX_TEXT + 1) + JS_STRUCT <= JS_IMG, "a tile's fields fit its image");

struct JsTab {
    int n_chrom, head;
    long long total;                    // values of a row
    long long off[WC_MAX_CHROM + 1];    // chromosome c is values off[c] .. off[c + 1]
};

// The structure between chromosome a's last value (a = -1: the row's start) and the next value or the row's end; returns
// its length and writes it unless dst is NULL.
__host__ __device__ inline int js_gap(const long long *off, int n_chrom, int a, unsigned char *dst) {
    int k = 0;
    if (dst) dst[k] = a >= 0 ? ']' : '[';
    ++k;
    for (int c = a + 1; c < n_chrom; ++c) {
        if (c > 0) {
            if (dst) dst[k] = ',';
            ++k;
        }
        if (dst) dst[k] = '[';
        ++k;
        if (off[c + 1] > off[c]) return k;
        if (dst) dst[k] = ']';
        ++k;
    }
    if (dst) dst[k] = ']';
    return k + 1;
}

__device__ __forceinline__ void js_load_tab(const JsTab &tab, long long *s_off) {
    for (int i = threadIdx.x; i <= tab.n_chrom; i += JS_T) s_off[i] = tab.off[i];
    wc_sync();
}

__global__ __launch_bounds__(JS_T) void k_js_len(const double *__restrict__ rows, long long row_stride, const JsTab tab, int strict,
                                                 uint4 *__restrict__ slots, int *__restrict__ sums) {
    __shared__ long long s_off[WC_MAX_CHROM + 1];
    __shared__ int s_part[JS_T / 64];
    js_load_tab(tab, s_off);
    const int t = threadIdx.x;
    const long long row = blockIdx.y, j = (long long)blockIdx.x * JS_T + t;
    int w = 0;
    if (j < tab.total) {
        const FdDec d = fd_decimal((uint64_t)__double_as_longlong(rows[row * row_stride + j]));
        slots[row * tab.total + j] = make_uint4((unsigned)d.digits, (unsigned)(d.digits >> 32), (unsigned)d.exp, d.kind);
        const int c = tt_chrom_of(s_off, tab.n_chrom, j);
        w = fd_length(d, strict) + (j + 1 < s_off[c + 1] ? 1 : js_gap(s_off, tab.n_chrom, c, nullptr));
    }
    for (int d = 32; d >= 1; d >>= 1) w += __shfl_down(w, d, 64);
    if ((t & 63) == 0) s_part[t >> 6] = w;
    wc_sync();
    if (t == 0) {
        int sum = 0;
        for (int k = 0; k < JS_T / 64; ++k) sum += s_part[k];
        sums[row * gridDim.x + blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(JS_T) void k_js_scan(const int *__restrict__ sums, long long n_tiles, int head, long long *__restrict__ tile_off,
                                                  long long *__restrict__ text_len) {
    __shared__ int s_buf[JS_T];
    const int t = threadIdx.x;
    const long long row = blockIdx.x;
    long long carry = 0;
    for (long long base = 0; base < n_tiles; base += JS_T) {
        const long long b = base + t;
        const int v = b < n_tiles ? sums[row * n_tiles + b] : 0;
        const int incl = tt_scan(v, s_buf);
        if (b < n_tiles) tile_off[row * n_tiles + b] = carry + incl - v;
        carry += s_buf[JS_T - 1];
        wc_sync();                              // (the next trip writes s_buf again)
    }
    if (t == 0) text_len[row] = head + carry;
}

__global__ __launch_bounds__(JS_T) void k_js_bytes(const uint4 *__restrict__ slots, const long long *__restrict__ tile_off, const JsTab tab,
                                                   int strict, unsigned char *__restrict__ text, long long text_stride) {
    __shared__ __attribute__((aligned(16))) unsigned char image[JS_IMG];
    __shared__ long long s_off[WC_MAX_CHROM + 1];
    __shared__ int s_buf[JS_T];
    js_load_tab(tab, s_off);
    const int t = threadIdx.x;
    const long long row = blockIdx.y, j = (long long)blockIdx.x * JS_T + t;
    FdDec d;
    d.digits = 0; d.exp = 0; d.kind = 0;
    int w = 0, gap = 0, c = 0;
    if (j < tab.total) {
        const uint4 s = slots[row * tab.total + j];
        d.digits = (uint64_t)s.x | ((uint64_t)s.y << 32);
        d.exp = (int32_t)s.z;
        d.kind = s.w;
        c = tt_chrom_of(s_off, tab.n_chrom, j);
        gap = j + 1 < s_off[c + 1] ? 0 : js_gap(s_off, tab.n_chrom, c, nullptr);
        w = fd_length(d, strict) + (gap ? gap : 1);
    }
    const int incl = tt_scan(w, s_buf);
    const long long start = tab.head + tile_off[row * gridDim.x + blockIdx.x];      // where the tile's first field begins
    const long long r0 = blockIdx.x == 0 ? 0 : start, r1 = start + s_buf[JS_T - 1], a0 = r0 & ~15ll;
    if (j < tab.total) {
        unsigned char *p = image + (start + incl - w - a0);
        p += fd_write(d, strict, p);
        if (gap) js_gap(s_off, tab.n_chrom, c, p);
        else *p = ',';
    }
    if (blockIdx.x == 0 && t == 0) js_gap(s_off, tab.n_chrom, -1, image);
    wc_sync();
    tt_store(image, a0, r0, r1, text + row * text_stride);
}

__global__ __launch_bounds__(JS_T) void k_js_format(const double *__restrict__ v, long long n, int strict, unsigned char *__restrict__ text,
                                                    unsigned char *__restrict__ len) {
    __shared__ __attribute__((aligned(16))) unsigned char image[JS_T * FD_MAX_TEXT];
    const int t = threadIdx.x;
    const long long j = (long long)blockIdx.x * JS_T + t;
    for (int line = t; line < JS_T * FD_MAX_TEXT / 16; line += JS_T) reinterpret_cast<uint4 *>(image)[line] = make_uint4(0u, 0u, 0u, 0u);
    wc_sync();
    if (j < n) {
        const FdDec d = fd_decimal((uint64_t)__double_as_longlong(v[j]));
        len[j] = (unsigned char)fd_write(d, strict, image + FD_MAX_TEXT * t);
    }
    wc_sync();
    const long long r0 = (long long)blockIdx.x * JS_T * FD_MAX_TEXT, end = n * FD_MAX_TEXT;
    tt_store(image, r0, r0, r0 + JS_T * FD_MAX_TEXT < end ? r0 + JS_T * FD_MAX_TEXT : end, text);
}

// ---- the host's half ----------------------------------------------------------------------------------------------------
int make_tab(const int64_t *chrom_sizes, int n_chrom, JsTab *tab) {
    WC_CHECK(n_chrom >= 0 && (chrom_sizes || n_chrom == 0), WC_E_ARG, "json: unusable chromosome sizes");
    WC_CHECK(n_chrom <= WC_MAX_CHROM, WC_E_LIMIT, "json: %d chromosomes (at most %d)", n_chrom, WC_MAX_CHROM);
    memset(tab, 0, sizeof *tab);
    tab->n_chrom = n_chrom;
    const long long most = (long long)INT_MAX - 2 * JS_T;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_sizes[c] >= 0, WC_E_ARG, "json: chromosome %d has %lld values", c + 1, (long long)chrom_sizes[c]);
        WC_CHECK(chrom_sizes[c] <= most - tab->off[c], WC_E_LIMIT, "json: more than %lld values in a row", most);
        tab->off[c + 1] = tab->off[c] + chrom_sizes[c];
    }
    tab->total = tab->off[n_chrom];
    tab->head = js_gap(tab->off, n_chrom, -1, nullptr);
    return WC_OK;
}

// 25 per value + 2 per chromosome + 2, and one more for every empty chromosome after the first ("[]," is three bytes)
int64_t bound_of(const JsTab &tab) {
    int empty = 0;
    for (int c = 0; c < tab.n_chrom; ++c) empty += tab.off[c + 1] == tab.off[c];
    return 25 * (int64_t)tab.total + 2 * tab.n_chrom + 2 + (empty > 1 ? empty - 1 : 0);
}

// a call's three launches, as wc::TextRows takes them (text_rows.h)
auto launches(const JsTab &tab, int strict) {
    return [&tab, strict](hipStream_t stream, const wc::TextWork &w, const wc::TextRows &call, hipEvent_t mid) -> int {
        int *sums = static_cast<int *>(w.sums);
        hipLaunchKernelGGL(k_js_len, w.grid, dim3(JS_T), 0, stream, call.rows, (long long)call.row_stride, tab, strict, w.slots, sums);
        WC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_js_scan, dim3(w.grid.y), dim3(JS_T), 0, stream, (const int *)sums, w.n_tiles, tab.head, w.tile_off,
                           (long long *)call.counts[0]);
        WC_HIP(hipGetLastError());
        if (mid) WC_HIP(hipEventRecord(mid, stream));
        hipLaunchKernelGGL(k_js_bytes, w.grid, dim3(JS_T), 0, stream, (const uint4 *)w.slots, (const long long *)w.tile_off, tab, strict,
                           call.text, (long long)call.text_stride);
        WC_HIP(hipGetLastError());
        return WC_OK;
    };
}

}  // namespace

extern "C" {

int wc_format_doubles_host(const double *v, int64_t n, int strict, char *text, uint8_t *len) {
    WC_CHECK(n >= 0 && (n == 0 || (v && text && len)), WC_E_ARG, "format: unusable argument");
    if (n) memset(text, 0, (size_t)n * FD_MAX_TEXT);
    for (int64_t i = 0; i < n; ++i) {
        uint64_t bits;
        memcpy(&bits, &v[i], 8);
        len[i] = (uint8_t)fd_write(fd_decimal(bits), strict, (unsigned char *)text + FD_MAX_TEXT * i);
    }
    return WC_OK;
}

int wc_format_doubles(wc_ctx *ctx, const double *v, int64_t n, int strict, char *text, uint8_t *len) {
    WC_CHECK(ctx && n >= 0 && (n == 0 || (v && text && len)), WC_E_ARG, "format: unusable argument");
    WC_CHECK(n <= (int64_t)INT_MAX / FD_MAX_TEXT, WC_E_LIMIT, "format: %lld values in one call", (long long)n);
    if (n == 0) return WC_OK;
    WC_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->tmp_a.reserve((size_t)n * 8)) || (rc = ctx->tmp_b.reserve((size_t)n * FD_MAX_TEXT + 16)) || (rc = ctx->tmp_c.reserve((size_t)n)))
        return rc;
    WC_HIP(hipMemcpy(ctx->tmp_a.p, v, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_js_format, dim3((unsigned)((n + JS_T - 1) / JS_T)), dim3(JS_T), 0, nullptr, (const double *)ctx->tmp_a.as<double>(),
                       (long long)n, strict, ctx->tmp_b.as<unsigned char>(), ctx->tmp_c.as<unsigned char>());
    WC_HIP(hipGetLastError());
    WC_HIP(hipMemcpy(text, ctx->tmp_b.p, (size_t)n * FD_MAX_TEXT, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(len, ctx->tmp_c.p, (size_t)n, hipMemcpyDeviceToHost));
    return WC_OK;
}

int64_t wc_json_row_bound(const int64_t *chrom_sizes, int n_chrom) {
    JsTab tab;
    if (make_tab(chrom_sizes, n_chrom, &tab)) return -1;
    return bound_of(tab);
}

int wc_json_rows_dev(wc_ctx *ctx, void *stream, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes_host,
                     int n_chrom, int strict, unsigned char *text, int64_t text_stride, int64_t *text_len) {
    const wc::TextRows call = {"json", "values", ctx, rows, row_stride, n_rows, text, text_stride, 1, {text_len, nullptr}};
    JsTab tab;
    int rc;
    if ((rc = call.begin()) || (rc = make_tab(chrom_sizes_host, n_chrom, &tab)) || (rc = call.check(tab.total, bound_of(tab), true))) return rc;
    return call.enqueue((hipStream_t)stream, tab.total, sizeof(int), nullptr, launches(tab, strict != 0));
}

int wc_json_rows(wc_ctx *ctx, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes, int n_chrom, int strict,
                 unsigned char *text, int64_t text_stride, int64_t *text_len, double *times_ms) {
    const wc::TextRows call = {"json", "values", ctx, rows, row_stride, n_rows, text, text_stride, 1, {text_len, nullptr}};
    JsTab tab;
    int rc;
    if ((rc = call.begin()) || (rc = make_tab(chrom_sizes, n_chrom, &tab)) || (rc = call.check(tab.total, bound_of(tab), false))) return rc;
    return call.stage(tab.total, bound_of(tab), 2, sizeof(int), times_ms, launches(tab, strict != 0));
}

int64_t wc_gzip_bytes(int64_t deflate_len) { return deflate_len < 0 ? -1 : deflate_len + 18; }

int wc_gzip_assemble(const unsigned char *deflate, int64_t deflate_len, uint32_t crc, int64_t input_len, unsigned char *out, int64_t cap,
                     int64_t *out_len) {
    WC_CHECK(deflate && deflate_len >= 1 && input_len >= 0 && out && out_len, WC_E_ARG, "gzip: unusable argument");
    WC_CHECK(cap >= wc_gzip_bytes(deflate_len), WC_E_ARG, "gzip: room for %lld bytes, wc_gzip_bytes(%lld) is %lld", (long long)cap,
             (long long)deflate_len, (long long)wc_gzip_bytes(deflate_len));
    // magic, method 8, no flags, no time, no extra flags, operating system unknown
    const unsigned char head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255};
    memcpy(out, head, 10);
    memcpy(out + 10, deflate, (size_t)deflate_len);
    unsigned char *p = out + 10 + deflate_len;
    const uint32_t isize = (uint32_t)((uint64_t)input_len & 0xffffffffu);
    for (int k = 0; k < 4; ++k) {
        p[k] = (unsigned char)(crc >> (8 * k));
        p[4 + k] = (unsigned char)(isize >> (8 * k));
    }
    *out_len = deflate_len + 18;
    return WC_OK;
}

}  // extern "C"
