// exporttracks: dense float64 rows -> bedGraph text, one line per run of bins with the same 64 bits inside a chromosome
// (the digit routine is fmt_double.h).  A row's bins are cut into tiles of BT_T bins, a workgroup per tile
// and a lane per bin, as export.hip does.  A line  name \t start \t end \t value \n  belongs to a run, and a run can span
// many tiles, so the line is written in two halves, each from what a bin sees of its two neighbours:
//   the run's FIRST bin (its left neighbour differs in bits, or it opens a chromosome) owns  name \t start \t
//   the run's LAST bin (its right neighbour differs, or it closes a chromosome) owns        end \t value \n
//   every other bin owns nothing.
// Both ends hold the same 64 bits, so both take the same decision to keep or drop the run (not finite: always dropped;
// a zero of either sign: dropped with BT_NOZERO), and between a kept run's two halves no other bin owns a byte: in the
// order of the bins the halves are adjacent, whatever lies between them.  No bin looks further than one bin away.
//   k_bt_len     the value's decimal digits, made by a kept run's last bin only (16 bytes into the call's slots), the sum
//                of the tile's bytes and the number of its bins that are not finite
//   k_bt_scan    a workgroup per row: the exclusive sum of the tile sums, text_len and dropped
//   k_bt_bytes   an exclusive sum of the lanes' bytes inside the tile, every lane writes its halves into the tile's image
//                in LDS, and after one barrier the image goes out in aligned 16-byte stores; the image's first and last
//                16 bytes, which a neighbouring tile shares, go out byte by byte.  Bytes behind text_len[i] are NOT written.
// Nothing synchronises; the chromosome table, the bin size, the clip lengths and the name prefix travel as a kernel
// argument.
#include <limits.h>

#include "ctx.h"
#include "fmt_double.h"
#include "text_rows.h"
#include "tile_text.h"

namespace {

const int BT_T = TT_T;                  // bins per tile = lanes per workgroup (tile_text.h)
const int BT_PREFIX = 16;               // bytes of the name prefix at most
const int BT_COORD = 15;                // digits of a coordinate at most
const long long BT_COORD_END = 1000000000000000ll;      // 10^15: every coordinate is below it
const int BT_FIRST = BT_PREFIX + 2 + 1 + BT_COORD + 1;  // name \t start \t        (at most 64 chromosomes: two digits)
const int BT_LAST = BT_COORD + 1 + FD_MAX_TEXT + 1;     // end \t value \n
const int BT_IMG = 80 * BT_T;           // bytes of a tile's image: five 16-byte lines per lane
static_assert(WC_MAX_CHROM < 100, "a chromosome's number has two digits");
static_assert(15 + BT_T * (BT_FIRST + BT_LAST) <= BT_IMG, "a tile's halves fit its image");
const int BT_NOZERO = 1;

struct BtTab {
    int n_chrom, prefix_len, flags;
    long long total, binsize;           // bins of a row
    long long off[WC_MAX_CHROM + 1];    // chromosome c is bins off[c] .. off[c + 1]
    long long clip[WC_MAX_CHROM];       // no end beyond it (LLONG_MAX: nothing is clipped)
    unsigned char prefix[BT_PREFIX];
};

struct BtShared {
    long long off[WC_MAX_CHROM + 1];
    long long clip[WC_MAX_CHROM];
    unsigned long long v[BT_T + 2];     // the tile's bins and one neighbour on either side
    unsigned char prefix[BT_PREFIX];
};

__host__ __device__ inline int bt_digits(long long v) {       // 0 <= v < 10^15
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

__device__ __forceinline__ int bt_put(long long v, unsigned char *p) {
    const int n = bt_digits(v);
    for (int i = n - 1; i >= 0; --i) {
        p[i] = (unsigned char)('0' + (int)(v % 10));
        v /= 10;
    }
    return n;
}

struct BtBin {                          // what a lane knows of its bin
    unsigned long long bits;
    long long start, end;               // the bin's own coordinates, the end clipped
    int chrom;
    bool first, last, keep, finite;
};

// The tables and the tile's bins with their two neighbours into LDS (the neighbour across a tile edge is one more
// global load), and this lane's bin; false for a lane behind the row's end.
__device__ __forceinline__ bool bt_load(const BtTab &tab, const double *__restrict__ row, BtShared &S, BtBin &b) {
    const int t = threadIdx.x;
    for (int i = t; i <= tab.n_chrom; i += BT_T) S.off[i] = tab.off[i];
    for (int i = t; i < tab.n_chrom; i += BT_T) S.clip[i] = tab.clip[i];
    if (t < BT_PREFIX) S.prefix[t] = tab.prefix[t];
    const long long j = (long long)blockIdx.x * BT_T + t;
    if (j < tab.total) S.v[t + 1] = (unsigned long long)__double_as_longlong(row[j]);
    if (t == 0 && j > 0 && j < tab.total) S.v[0] = (unsigned long long)__double_as_longlong(row[j - 1]);
    if (t == BT_T - 1 && j + 1 < tab.total) S.v[BT_T + 1] = (unsigned long long)__double_as_longlong(row[j + 1]);
    wc_sync();
    if (j >= tab.total) return false;
    b.bits = S.v[t + 1];
    b.chrom = tt_chrom_of(S.off, tab.n_chrom, j);
    const long long p = j - S.off[b.chrom];
    b.first = p == 0 || S.v[t] != b.bits;
    b.last = j + 1 == S.off[b.chrom + 1] || S.v[t + 2] != b.bits;
    b.finite = ((b.bits >> 52) & 0x7ffu) != 0x7ffu;
    b.keep = b.finite && !((tab.flags & BT_NOZERO) && (b.bits << 1) == 0);
    b.start = p * tab.binsize;
    const long long end = b.start + tab.binsize, clip = S.clip[b.chrom];
    b.end = end < clip ? end : clip;
    return true;
}

__device__ __forceinline__ int bt_first_len(const BtTab &tab, const BtBin &b) {
    return tab.prefix_len + (b.chrom + 1 >= 10 ? 2 : 1) + 1 + bt_digits(b.start) + 1;
}

__global__ __launch_bounds__(BT_T) void k_bt_len(const double *__restrict__ rows, long long row_stride, const BtTab tab,
                                                 uint4 *__restrict__ slots, int2 *__restrict__ sums) {
    __shared__ BtShared S;
    __shared__ int s_part[2 * (BT_T / 64)];
    const int t = threadIdx.x;
    const long long row = blockIdx.y, j = (long long)blockIdx.x * BT_T + t;
    BtBin b;
    int w = 0, lost = 0;
    if (bt_load(tab, rows + row * row_stride, S, b)) {
        lost = !b.finite;
        if (b.keep && b.first) w = bt_first_len(tab, b);
        if (b.keep && b.last) {
            const FdDec d = fd_decimal((uint64_t)b.bits);
            slots[row * tab.total + j] = make_uint4((unsigned)d.digits, (unsigned)(d.digits >> 32), (unsigned)d.exp, d.kind);
            w += bt_digits(b.end) + 1 + fd_length(d, 0) + 1;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        w += __shfl_down(w, d, 64);
        lost += __shfl_down(lost, d, 64);
    }
    if ((t & 63) == 0) {
        s_part[t >> 6] = w;
        s_part[BT_T / 64 + (t >> 6)] = lost;
    }
    wc_sync();
    if (t == 0) {
        int sum = 0, gone = 0;
        for (int k = 0; k < BT_T / 64; ++k) {
            sum += s_part[k];
            gone += s_part[BT_T / 64 + k];
        }
        sums[row * gridDim.x + blockIdx.x] = make_int2(sum, gone);
    }
}

__global__ __launch_bounds__(BT_T) void k_bt_scan(const int2 *__restrict__ sums, long long n_tiles, long long *__restrict__ tile_off,
                                                  long long *__restrict__ text_len, long long *__restrict__ dropped) {
    __shared__ int s_buf[BT_T];
    const int t = threadIdx.x;
    const long long row = blockIdx.x;
    long long carry = 0, gone = 0;
    for (long long base = 0; base < n_tiles; base += BT_T) {
        const long long b = base + t;
        const int2 v = b < n_tiles ? sums[row * n_tiles + b] : make_int2(0, 0);
        const int incl = tt_scan(v.x, s_buf);
        if (b < n_tiles) tile_off[row * n_tiles + b] = carry + incl - v.x;
        carry += s_buf[BT_T - 1];
        wc_sync();                              // (the next scan writes s_buf again)
        gone += tt_scan(v.y, s_buf);            // (lane BT_T - 1 holds the trip's whole sum)
        wc_sync();
    }
    if (t == BT_T - 1) {
        text_len[row] = carry;
        dropped[row] = gone;
    }
}

__global__ __launch_bounds__(BT_T) void k_bt_bytes(const double *__restrict__ rows, long long row_stride, const uint4 *__restrict__ slots,
                                                   const long long *__restrict__ tile_off, const BtTab tab,
                                                   unsigned char *__restrict__ text, long long text_stride) {
    __shared__ __attribute__((aligned(16))) unsigned char image[BT_IMG];
    __shared__ BtShared S;
    __shared__ int s_buf[BT_T];
    const int t = threadIdx.x;
    const long long row = blockIdx.y, j = (long long)blockIdx.x * BT_T + t;
    BtBin b;
    FdDec d;
    d.digits = 0; d.exp = 0; d.kind = 0;
    int w = 0;
    const bool live = bt_load(tab, rows + row * row_stride, S, b);
    const bool head = live && b.keep && b.first, tail = live && b.keep && b.last;
    if (head) w = bt_first_len(tab, b);
    if (tail) {
        const uint4 s = slots[row * tab.total + j];
        d.digits = (uint64_t)s.x | ((uint64_t)s.y << 32);
        d.exp = (int32_t)s.z;
        d.kind = s.w;
        w += bt_digits(b.end) + 1 + fd_length(d, 0) + 1;
    }
    const int incl = tt_scan(w, s_buf);
    const long long r0 = tile_off[row * gridDim.x + blockIdx.x], r1 = r0 + s_buf[BT_T - 1], a0 = r0 & ~15ll;
    unsigned char *p = image + (r0 + incl - w - a0);
    if (head) {
        for (int k = 0; k < tab.prefix_len; ++k) p[k] = S.prefix[k];
        p += tab.prefix_len;
        p += bt_put(b.chrom + 1, p);
        *p++ = '\t';
        p += bt_put(b.start, p);
        *p++ = '\t';
    }
    if (tail) {
        p += bt_put(b.end, p);
        *p++ = '\t';
        p += fd_write(d, 0, p);
        *p = '\n';
    }
    wc_sync();
    tt_store(image, a0, r0, r1, text + row * text_stride);
}

// ---- the host's half ----------------------------------------------------------------------------------------------------
int make_tab(const int64_t *chrom_sizes, int n_chrom, int64_t binsize, const int64_t *clip_len, const char *prefix, int prefix_len,
             int flags, BtTab *tab) {
    WC_CHECK(n_chrom >= 0 && (chrom_sizes || n_chrom == 0), WC_E_ARG, "bedgraph: unusable chromosome sizes");
    WC_CHECK(n_chrom <= WC_MAX_CHROM, WC_E_LIMIT, "bedgraph: %d chromosomes (at most %d)", n_chrom, WC_MAX_CHROM);
    WC_CHECK(binsize >= 1, WC_E_ARG, "bedgraph: a bin size of %lld", (long long)binsize);
    WC_CHECK(prefix_len >= 0 && prefix_len <= BT_PREFIX && (prefix || prefix_len == 0), WC_E_ARG,
             "bedgraph: a name prefix of %d bytes (at most %d)", prefix_len, BT_PREFIX);
    WC_CHECK((flags & ~BT_NOZERO) == 0, WC_E_ARG, "bedgraph: flags %d (bit 0 alone is defined)", flags);
    memset(tab, 0, sizeof *tab);
    tab->n_chrom = n_chrom;
    tab->prefix_len = prefix_len;
    tab->flags = flags;
    tab->binsize = binsize;
    for (int k = 0; k < prefix_len; ++k) {
        const unsigned char ch = (unsigned char)prefix[k];
        WC_CHECK(ch < 128 && ch != '\t' && ch != '\n' && ch != 0, WC_E_ARG, "bedgraph: byte %d of the name prefix is 0x%02x", k, ch);
        tab->prefix[k] = ch;
    }
    const long long most = (long long)INT_MAX - 2 * BT_T;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_sizes[c] >= 0, WC_E_ARG, "bedgraph: chromosome %d has %lld bins", c + 1, (long long)chrom_sizes[c]);
        WC_CHECK(chrom_sizes[c] <= most - tab->off[c], WC_E_LIMIT, "bedgraph: more than %lld bins in a row", most);
        WC_CHECK(chrom_sizes[c] <= (BT_COORD_END - 1) / binsize, WC_E_LIMIT,
                 "bedgraph: chromosome %d ends at %lld bins of %lld; coordinates stay below 10^%d", c + 1, (long long)chrom_sizes[c],
                 (long long)binsize, BT_COORD);
        tab->off[c + 1] = tab->off[c] + chrom_sizes[c];
        tab->clip[c] = LLONG_MAX;
        if (clip_len) {
            WC_CHECK(chrom_sizes[c] == 0 || clip_len[c] > (chrom_sizes[c] - 1) * binsize, WC_E_ARG,
                     "bedgraph: chromosome %d is %lld long, its last bin starts at %lld", c + 1, (long long)clip_len[c],
                     (long long)((chrom_sizes[c] - 1) * binsize));
            tab->clip[c] = clip_len[c];
        }
    }
    tab->total = tab->off[n_chrom];
    return WC_OK;
}

// every bin a line of its own, every coordinate as long as its chromosome's longest:
// the sum over the chromosomes of bins * (prefix + digits(number) + digits((bins - 1) * binsize) + digits(bins * binsize) + 28)
int64_t bound_of(const BtTab &tab) {
    int64_t bound = 0;
    for (int c = 0; c < tab.n_chrom; ++c) {
        const long long n = tab.off[c + 1] - tab.off[c];
        if (n > 0) bound += n * (tab.prefix_len + bt_digits(c + 1) + bt_digits((n - 1) * tab.binsize) + bt_digits(n * tab.binsize) + 4 + FD_MAX_TEXT);
    }
    return bound;
}

// a call's three launches, as wc::TextRows takes them (text_rows.h); counts: text_len, dropped
auto launches(const BtTab &tab) {
    return [&tab](hipStream_t stream, const wc::TextWork &w, const wc::TextRows &call, hipEvent_t mid) -> int {
        int2 *sums = static_cast<int2 *>(w.sums);
        hipLaunchKernelGGL(k_bt_len, w.grid, dim3(BT_T), 0, stream, call.rows, (long long)call.row_stride, tab, w.slots, sums);
        WC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bt_scan, dim3(w.grid.y), dim3(BT_T), 0, stream, (const int2 *)sums, w.n_tiles, w.tile_off,
                           (long long *)call.counts[0], (long long *)call.counts[1]);
        WC_HIP(hipGetLastError());
        if (mid) WC_HIP(hipEventRecord(mid, stream));
        hipLaunchKernelGGL(k_bt_bytes, w.grid, dim3(BT_T), 0, stream, call.rows, (long long)call.row_stride, (const uint4 *)w.slots,
                           (const long long *)w.tile_off, tab, call.text, (long long)call.text_stride);
        WC_HIP(hipGetLastError());
        return WC_OK;
    };
}

}  // namespace

extern "C" {

int64_t wc_bedgraph_row_bound(const int64_t *chrom_sizes, int n_chrom, int64_t binsize, int prefix_len) {
    BtTab tab;
    if (make_tab(chrom_sizes, n_chrom, binsize, nullptr, "cccccccccccccccc", prefix_len, 0, &tab)) return -1;      // (any BT_PREFIX bytes)
    return bound_of(tab);
}

int wc_bedgraph_rows_dev(wc_ctx *ctx, void *stream, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes_host,
                         int n_chrom, int64_t binsize, const int64_t *clip_len_host, const char *prefix, int prefix_len, int flags,
                         unsigned char *text, int64_t text_stride, int64_t *text_len, int64_t *dropped) {
    const wc::TextRows call = {"bedgraph", "bins", ctx, rows, row_stride, n_rows, text, text_stride, 2, {text_len, dropped}};
    BtTab tab;
    int rc;
    if ((rc = call.begin()) || (rc = make_tab(chrom_sizes_host, n_chrom, binsize, clip_len_host, prefix, prefix_len, flags, &tab)) ||
        (rc = call.check(tab.total, bound_of(tab), true)))
        return rc;
    return call.enqueue((hipStream_t)stream, tab.total, sizeof(int2), nullptr, launches(tab));
}

int wc_bedgraph_rows(wc_ctx *ctx, const double *rows, int64_t row_stride, int64_t n_rows, const int64_t *chrom_sizes, int n_chrom,
                     int64_t binsize, const int64_t *clip_len, const char *prefix, int prefix_len, int flags, unsigned char *text,
                     int64_t text_stride, int64_t *text_len, int64_t *dropped, double *times_ms) {
    const wc::TextRows call = {"bedgraph", "bins", ctx, rows, row_stride, n_rows, text, text_stride, 2, {text_len, dropped}};
    BtTab tab;
    int rc;
    if ((rc = call.begin()) || (rc = make_tab(chrom_sizes, n_chrom, binsize, clip_len, prefix, prefix_len, flags, &tab)) ||
        (rc = call.check(tab.total, bound_of(tab), false)))
        return rc;
    return call.stage(tab.total, bound_of(tab), 0, sizeof(int2), times_ms, launches(tab));
}



}  // extern "C"
