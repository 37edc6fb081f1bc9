// plotbatch: result files -> z-score panel PNGs (DESIGN.md "plotbatch").  Three kernels and the host framing:
//   k_plot_list     one workgroup per (sample, panel): the display list of upstream plotLines (wisetools.py:527-662)
//                   in data coordinates -- the panel's finite z range, one entry per stretch of bins whose z == 0
//                   (positionsToStretches(zeros, 1): an ordered compaction of the stretch starts and ends across the
//                   waves), one entry per call of the panel's chromosome with abs(effect) * 100 >= mineffect
//   k_plot_raster   the image in PNG scanline layout (filter byte 0, then RGB), a lane per pixel column: it works out the
//                   polyline's min-max span of its column once per panel and walks the panel's list for every pixel of
//                   a band of rows, in the painter's order of DESIGN.md.  Every data-to-pixel mapping is float64 in
//                   one fixed operation order (the unit is compiled with contraction off, like the rest of the
//                   library): tests/plot_restated.py repeats it in numpy and the tests compare the bytes.
//   k_adler_blocks / k_adler_rows   Adler-32 of every image: per block of PL_ADLER_B bytes the two sums modulo 65521,
//                   then the blocks of a row combined in order
// The deflate stream of an image is wc_deflate_rows_dev's (deflate.hip) with the image as one row; the host puts the
// PNG chunks around it (wc_png_assemble) and computes the chunk CRCs over the compressed bytes.
#include <limits.h>
#include <zlib.h>

#include "ctx.h"
#include "plot_font.h"
#include "plot_label.h"

namespace {

const int PL_T = 256;               // lanes per workgroup of every kernel here
const int PL_F = 9;                 // fields of a list entry: kind, panel, x0, x1, y0, y1, colour id, alpha, value
const int PL_RANGE = 0, PL_ZERO = 2, PL_CALL = 3;     // (kind 1, a cytoband, exists on the host only)
const int PL_BAND_ROWS = 16;        // image rows per workgroup of the raster kernel
const int PL_ADLER_B = 65536;       // bytes per Adler-32 block
const unsigned PL_ADLER_M = 65521u;
const int PL_TITLE_PREFIX = 45;     // strlen("Z-score versus chromosomal position - Sample ")

// the reference's palette (wisetools.py:531-541) and its line grey, each channel int(c * 255 + 0.5)
__device__ const unsigned char PL_PALETTE[9][3] = {{0, 0, 0},      {230, 153, 0},  {89, 179, 230}, {0, 153, 128}, {242, 230, 64},
                                                   {0, 115, 179},  {204, 102, 0},  {204, 153, 179}, {179, 179, 179}};
const int PL_GREY = 8;

struct ListShared {
    int cs[PL_T / 64], ce[PL_T / 64];
    double mn[PL_T / 64], mx[PL_T / 64];
};

// ---- the display list ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_T) void k_plot_list(const double *__restrict__ z, long long row_stride,
                                                    const long long *__restrict__ chrom_off,
                                                    const long long *__restrict__ chrom_len, const int *__restrict__ panel_chrom,
                                                    const double *__restrict__ calls, const int *__restrict__ n_calls,
                                                    int max_calls, double thr, double mineffect, int cap,
                                                    double *__restrict__ entries, int *__restrict__ counts, int *status) {
    __shared__ ListShared S;
    const int p = blockIdx.x, P = gridDim.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long s = blockIdx.y;
    const int chrom = panel_chrom[p];
    const long long len = chrom_len[chrom - 1];
    const double *zr = z + s * row_stride + chrom_off[chrom - 1];
    double *out = entries + (s * P + p) * (long long)cap * PL_F;
    const unsigned long long below = (1ull << lane) - 1ull;

    // zero stretches: the k-th start and the k-th end belong to stretch k
    int base_s = 0, base_e = 0;
    double mn = INFINITY, mx = -INFINITY;
    for (long long tile = 0; tile < len; tile += PL_T) {
        const long long i = tile + t;
        const bool in = i < len;
        const double v = in ? zr[i] : 1.0;
        const bool isz = in && v == 0.0;                                    // -0.0 counts, NaN does not
        const bool st = isz && (i == 0 || zr[i - 1] != 0.0);
        const bool en = isz && (i == len - 1 || zr[i + 1] != 0.0);
        if (in && __builtin_isfinite(v)) {
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        const unsigned long long bs = __ballot(st), be = __ballot(en);
        if (lane == 0) {
            S.cs[w] = __popcll(bs);
            S.ce[w] = __popcll(be);
        }
        wc_sync();
        int off_s = base_s, off_e = base_e, tot_s = 0, tot_e = 0;
        for (int k = 0; k < PL_T / 64; ++k) {
            if (k < w) {
                off_s += S.cs[k];
                off_e += S.ce[k];
            }
            tot_s += S.cs[k];
            tot_e += S.ce[k];
        }
        if (st) {
            const long long at = 1 + off_s + __popcll(bs & below);
            if (at < cap) {
                double *e = out + at * PL_F;
                e[0] = PL_ZERO; e[1] = p; e[2] = (double)i - 0.5; e[4] = -thr; e[5] = thr; e[6] = 7; e[7] = 0.5; e[8] = 0.0;
            }
        }
        if (en) {
            const long long at = 1 + off_e + __popcll(be & below);
            if (at < cap) out[at * PL_F + 3] = (double)i + 0.5;
        }
        base_s += tot_s;
        base_e += tot_e;
        wc_sync();                                                          // the counts are rewritten by the next tile
    }
    const int nz = base_s;

    // the range of the finite z-scores
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane == 0) {
        S.mn[w] = mn;
        S.mx[w] = mx;
    }
    wc_sync();
    if (t == 0 && cap > 0) {
        for (int k = 0; k < PL_T / 64; ++k) {
            mn = S.mn[k] < mn ? S.mn[k] : mn;
            mx = S.mx[k] > mx ? S.mx[k] : mx;
        }
        out[0] = PL_RANGE; out[1] = p; out[2] = 0.0; out[3] = (double)len; out[4] = mn; out[5] = mx; out[6] = 0; out[7] = 0.0;
        out[8] = (double)nz;
    }
    wc_sync();

    // the calls of this chromosome, in their order
    int nc = n_calls ? n_calls[s] : 0;
    nc = nc < 0 ? 0 : (nc > max_calls ? max_calls : nc);
    int base_c = 0;
    for (int tile = 0; tile < nc; tile += PL_T) {
        const int j = tile + t;
        const bool in = j < nc;
        const double *c = calls + (s * max_calls + (in ? j : 0)) * 5;
        const double ch = in ? c[0] : 0.0, eff = in ? c[4] : 0.0;
        const double ae = fabs(eff);
        const bool keep = in && ch == (double)chrom && ae * 100.0 >= mineffect;      // a NaN effect draws nothing
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) S.cs[w] = __popcll(bk);
        wc_sync();
        int off = base_c, tot = 0;
        for (int k = 0; k < PL_T / 64; ++k) {
            if (k < w) off += S.cs[k];
            tot += S.cs[k];
        }
        if (keep) {
            const long long at = 1 + (long long)nz + off + __popcll(bk & below);
            if (at < cap) {
                double *e = out + at * PL_F;
                const double zc = c[3], a10 = ae * 10.0;
                e[0] = PL_CALL; e[1] = p; e[2] = c[1] - 0.5; e[3] = c[2] + 0.5; e[4] = 0.0; e[5] = zc < 0.0 ? -thr : thr;
                e[6] = ae >= 0.2 ? 3 : 1; e[7] = a10 < 1.0 ? a10 : 1.0; e[8] = zc;
            }
        }
        base_c += tot;
        wc_sync();
    }
    if (t == 0) {
        const long long total = 1 + (long long)nz + base_c;
        counts[s * P + p] = (int)total;
        if (total > cap) atomicOr(status, 1);                               // never a silently shorter list
    }
}

// ---- the rasteriser --------------------------------------------------------------------------------------------------
struct RasterArgs {
    int W, H, s, P, cap, has_cyto, name_cap;
    long long row_stride, img_stride;
    double thr;
    const double *z;
    const long long *chrom_off, *chrom_len;
    const int *panel_chrom, *boxes, *band_off;
    const double *bands, *entries;
    const int *counts;
    const char *names;
    const unsigned char *font;
    unsigned char *out;
};

struct Rgb {
    int r, g, b;
};
__device__ __forceinline__ void pl_blend(Rgb &c, int col, int a) {
    c.r = (c.r * (255 - a) + PL_PALETTE[col][0] * a + 127) / 255;
    c.g = (c.g * (255 - a) + PL_PALETTE[col][1] * a + 127) / 255;
    c.b = (c.b * (255 - a) + PL_PALETTE[col][2] * a + 127) / 255;
}
__device__ __forceinline__ bool pl_glyph(const unsigned char *font, int ch, int dx, int dy, int s) {
    if (ch < 32 || ch > 126) ch = '?';
    return (font[(ch - 32) * WC_FONT_H + dy / s] >> (7 - (dx / s) % WC_FONT_W)) & 1;
}
// (the arguments are read from the call's table block where they are needed: held in registers for the whole kernel
//  they did not fit the scalar file)
__global__ __launch_bounds__(PL_T) void k_plot_raster(const RasterArgs *args) {
    const RasterArgs &A = *args;
    __shared__ unsigned char font[WC_FONT_N * WC_FONT_H];
    for (int i = threadIdx.x; i < WC_FONT_N * WC_FONT_H; i += PL_T) font[i] = A.font[i];
    wc_sync();
    const int ix = blockIdx.x * PL_T + threadIdx.x;
    if (ix >= A.W) return;
    const long long smp = blockIdx.z;
    const int s = A.s, W = A.W, H = A.H;
    const int row0 = blockIdx.y * PL_BAND_ROWS, row1 = row0 + PL_BAND_ROWS < H ? row0 + PL_BAND_ROWS : H;
    unsigned char *img = A.out + smp * A.img_stride;
    const long long line = 1 + 3ll * W;
    const char *name = A.names + smp * A.name_cap;
    int name_len = 0;
    while (name_len < A.name_cap && name[name_len]) ++name_len;
    const double cx = (double)ix + 0.5;

    // the state of this lane's column inside the panel it is crossing
    int cur = -1, bx0 = 0, by0 = 0, bx1 = 0, by1 = 0, n_ent = 0, nz = 0, span_lo = 0, span_hi = -1, has_bands = 0;
    double bw = 1.0, bh = 1.0, xmax = 1.0, yhi = 1.0, yspan = 1.0;
    const double *ent = A.entries;
    const double thr = A.thr, cyto_y = -thr - thr / 2.0;

    for (int iy = row0; iy < row1; ++iy) {
        if (ix == 0) img[iy * line] = 0;                                     // the scanline's filter byte
        const double cy = (double)iy + 0.5;
        Rgb c = {255, 255, 255};
        if (!(cur >= 0 && ix >= bx0 && ix < bx1 && iy >= by0 && iy < by1)) {
            cur = -1;
            for (int p = 0; p < A.P; ++p) {
                const int *b = A.boxes + 4 * p;
                if (ix >= b[0] && ix < b[2] && iy >= b[1] && iy < b[3]) cur = p;
            }
            if (cur >= 0) {
                const int *b = A.boxes + 4 * cur;
                bx0 = b[0]; by0 = b[1]; bx1 = b[2]; by1 = b[3];
                bw = (double)(bx1 - bx0);
                bh = (double)(by1 - by0);
                const int chrom = A.panel_chrom[cur];
                const long long len = A.chrom_len[chrom - 1];
                const double *zr = A.z + smp * A.row_stride + A.chrom_off[chrom - 1];
                xmax = len > 0 ? (double)len : 1.0;
                ent = A.entries + (smp * A.P + cur) * (long long)A.cap * PL_F;
                n_ent = A.counts[smp * A.P + cur];
                n_ent = n_ent > A.cap ? A.cap : n_ent;
                nz = (int)ent[8];
                has_bands = A.band_off && A.band_off[cur + 1] > A.band_off[cur];
                pl_yrange(ent[4], ent[5], thr, A.has_cyto, yhi, yspan);
                // the polyline in this column: min and max of the segments that cross it, taken at the column's edges
                span_lo = INT_MAX;
                span_hi = INT_MIN;
                const double xl = (double)ix, xr = (double)ix + 1.0;
                long long i_lo = (long long)pl_flr(((xl - bx0) * xmax) / bw) - 2, i_hi = (long long)pl_flr(((xr - bx0) * xmax) / bw) + 2;
                i_lo = i_lo < 0 ? 0 : i_lo;
                i_hi = i_hi > len - 2 ? len - 2 : i_hi;
                for (long long i = i_lo; i <= i_hi; ++i) {
                    const double za = zr[i], zb = zr[i + 1];
                    if (!__builtin_isfinite(za) || !__builtin_isfinite(zb)) continue;     // a gap breaks the line
                    const double xa = ((double)i * bw) / xmax + bx0, xb = ((double)(i + 1) * bw) / xmax + bx0;
                    if (!(xa < xr && xb > xl)) continue;
                    const double t0 = xa > xl ? xa : xl, t1 = xb < xr ? xb : xr, dx = xb - xa;
                    const double ya = ((yhi - za) * bh) / yspan + by0, yb = ((yhi - zb) * bh) / yspan + by0;
                    const double y0 = ya + (yb - ya) * ((t0 - xa) / dx), y1 = ya + (yb - ya) * ((t1 - xa) / dx);
                    if (!(y0 == y0) || !(y1 == y1)) continue;
                    const int r0 = pl_flr(y0 < y1 ? y0 : y1), r1 = pl_flr(y0 < y1 ? y1 : y0);
                    span_lo = r0 < span_lo ? r0 : span_lo;
                    span_hi = r1 > span_hi ? r1 : span_hi;
                }
                if (span_lo <= span_hi) {
                    span_lo -= (s - 1) / 2;
                    span_hi += s / 2;
                }
            }
        }
        if (cur >= 0) {
#define PL_FX(x) (((x) * bw) / xmax + bx0)
#define PL_FY(y) (((yhi - (y)) * bh) / yspan + by0)
            // 2. cytobands
            if (has_bands) {
                const double top = PL_FY(-thr), bot = PL_FY(cyto_y);
                if (top <= cy && cy < bot) {
                    for (int k = A.band_off[cur]; k < A.band_off[cur + 1]; ++k) {
                        const double *bd = A.bands + 4 * k;
                        if (bd[3] >= 0.0 && PL_FX(bd[0]) <= cx && cx < PL_FX(bd[1])) {      // (hatch -1: a band without a rectangle)
                            const int a = pl_alpha(bd[2]), hatch = (int)bd[3], period = 6 * s;
                            pl_blend(c, 0, a);
                            if ((hatch == 1 && (ix + iy) % period < s) || (hatch == 2 && (((ix - iy) % period) + period) % period < s))
                                pl_blend(c, 0, a);
                        }
                    }
                }
            }
            // 3. uncallable patches, 4. call rectangles (the list holds them in this order)
            for (int k = 1; k < n_ent; ++k) {
                const double *e = ent + k * PL_F;
                const double ya = e[4], yb = e[5];
                if (PL_FX(e[2]) <= cx && cx < PL_FX(e[3]) && PL_FY(ya > yb ? ya : yb) <= cy && cy < PL_FY(ya > yb ? yb : ya))
                    pl_blend(c, (int)e[6], pl_alpha(e[7]));
            }
            // 5. grey lines
            const int lw0 = s / 2;
            for (int k = 0; k < (has_bands ? 4 : 3); ++k) {
                const double y = k == 0 ? 0.0 : k == 1 ? thr : k == 2 ? -thr : cyto_y;
                const int r = pl_rnd(PL_FY(y)) - lw0;
                if (iy >= r && iy < r + s) pl_blend(c, PL_GREY, 255);
            }
            // 6. call edge lines
            for (int k = 1 + nz; k < n_ent; ++k) {
                const double *e = ent + k * PL_F;
                const int c0 = pl_rnd(PL_FX(e[2])) - lw0, c1 = pl_rnd(PL_FX(e[3])) - lw0;
                if ((ix >= c0 && ix < c0 + s) || (ix >= c1 && ix < c1 + s)) pl_blend(c, (int)e[6], 255);
            }
            // 7. the polyline
            if (iy >= span_lo && iy <= span_hi) pl_blend(c, 5, 255);
            // 8. labels
            for (int k = 1 + nz; k < n_ent; ++k) {
                const double *e = ent + k * PL_F;
                const double zc = e[8];
                unsigned long long tenths = 0;
                int neg = 0;
                const bool ok = pl_label_tenths(zc, tenths, neg);
                const int n = pl_label_len(ok, tenths, neg), wpx = n * WC_FONT_W * s;
                const int tx = pl_rnd(PL_FX(e[2] + (e[3] - e[2]) / 2.0)) - (wpx >> 1);
                const int edge = pl_rnd(PL_FY(e[5]));
                const int ty = zc > 0.0 ? edge + s : edge - s - WC_FONT_H * s;            // anchored top / bottom
                const int dx = ix - tx, dy = iy - ty;
                if (dx >= 0 && dx < wpx && dy >= 0 && dy < WC_FONT_H * s &&
                    pl_glyph(font, pl_label_char(ok, tenths, neg, n, dx / (WC_FONT_W * s)), dx % (WC_FONT_W * s), dy, s))
                    pl_blend(c, 0, 255);
            }
            // 9. the frame
            if (ix - bx0 < s || bx1 - ix <= s || iy - by0 < s || by1 - iy <= s) pl_blend(c, 0, 255);
#undef PL_FX
#undef PL_FY
        } else {
            // the chromosome number to the left of every panel
            for (int p = 0; p < A.P; ++p) {
                const int *b = A.boxes + 4 * p;
                const unsigned long long chrom = (unsigned long long)A.panel_chrom[p];
                const int n = pl_digits(chrom), wpx = n * WC_FONT_W * s;
                const int tx = b[0] - 4 * s - wpx, ty = b[1] + ((b[3] - b[1] - WC_FONT_H * s) >> 1);
                const int dx = ix - tx, dy = iy - ty;
                if (b[2] > b[0] && b[3] > b[1] && dx >= 0 && dx < wpx && dy >= 0 && dy < WC_FONT_H * s &&
                    pl_glyph(font, pl_digit(chrom, n, dx / (WC_FONT_W * s)), dx % (WC_FONT_W * s), dy, s))
                    pl_blend(c, 0, 255);
            }
        }
        // 10. title and legend
        {
            const char *prefix = "Z-score versus chromosomal position - Sample ";
            const int n = PL_TITLE_PREFIX + name_len, wpx = n * WC_FONT_W * s;
            const int tx = (W - wpx) >> 1, ty = (H * 7) / 100 - WC_FONT_H * s;
            const int dx = ix - tx, dy = iy - ty;
            if (dx >= 0 && dx < wpx && dy >= 0 && dy < WC_FONT_H * s) {
                const int k = dx / (WC_FONT_W * s);
                const int ch = k < PL_TITLE_PREFIX ? prefix[k] : (unsigned char)name[k - PL_TITLE_PREFIX];
                if (pl_glyph(font, ch, dx % (WC_FONT_W * s), dy, s)) pl_blend(c, 0, 255);
            }
            // two columns of two entries, filled column by column as the reference's ncol=2 legend
            const int ew = 21 * WC_FONT_W * s, eh = 16 * s, lx = (W - 2 * ew) >> 1, ly = H - 34 * s;
            const int ldx = ix - lx, ldy = iy - ly;
            if (ldx >= 0 && ldx < 2 * ew && ldy >= 0 && ldy < 2 * eh) {
                const int which = (ldx / ew) * 2 + ldy / eh, ex = ldx % ew, ey = ldy % eh;
                const char *text = which == 0 ? "Called region" : which == 1 ? "Uncallable region" : which == 2 ? "Z-score per bin" : "Z-score threshold";
                const int tn = which == 0 ? 13 : which == 1 ? 17 : which == 2 ? 15 : 17;
                const int col = which == 0 ? 1 : which == 1 ? 7 : which == 2 ? 5 : PL_GREY;
                if (ex < 2 * WC_FONT_W * s && ey >= 3 * s && ey < 11 * s) pl_blend(c, col, 255);
                const int dx2 = ex - 3 * WC_FONT_W * s;
                if (dx2 >= 0 && dx2 < tn * WC_FONT_W * s && ey < WC_FONT_H * s &&
                    pl_glyph(font, text[dx2 / (WC_FONT_W * s)], dx2 % (WC_FONT_W * s), ey, s))
                    pl_blend(c, 0, 255);
            }
        }
        unsigned char *px = img + iy * line + 1 + 3ll * ix;
        px[0] = (unsigned char)c.r;
        px[1] = (unsigned char)c.g;
        px[2] = (unsigned char)c.b;
    }
}

// ---- Adler-32 ---------------------------------------------------------------------------------------------------------
// Block b of a row: A = sum of its bytes, B = sum of (n - i) * byte i over its n bytes, both modulo 65521.  Appending the
// block to a prefix with the sums (a, b) gives (a + A, b + n * a + B).
__global__ __launch_bounds__(PL_T) void k_adler_blocks(const unsigned char *__restrict__ src, long long row_bytes, long long stride,
                                                       int n_blk, unsigned *__restrict__ part) {
    __shared__ unsigned long long sa[PL_T / 64], sb[PL_T / 64];
    const int blk = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long row = blockIdx.y, start = (long long)blk * PL_ADLER_B;
    const int n = (int)(row_bytes - start < PL_ADLER_B ? row_bytes - start : PL_ADLER_B);      // <= 0: an empty row's one block
    const unsigned char *p = src + row * stride + start;
    unsigned long long a = 0, b = 0;
    for (int i = t; i < n; i += PL_T) {
        const unsigned v = p[i];
        a += v;
        b += (unsigned long long)(n - i) * v;                               // < 2^16 * 2^8 per term, 256 terms per lane
    }
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    if (lane == 0) {
        sa[w] = a;
        sb[w] = b;
    }
    wc_sync();
    if (t == 0) {
        a = 0;
        b = 0;
        for (int k = 0; k < PL_T / 64; ++k) {
            a += sa[k];
            b += sb[k];
        }
        part[(row * n_blk + blk) * 2] = (unsigned)(a % PL_ADLER_M);
        part[(row * n_blk + blk) * 2 + 1] = (unsigned)(b % PL_ADLER_M);
    }
}

__global__ void k_adler_rows(const unsigned *__restrict__ part, long long row_bytes, int n_blk, long long n_rows,
                             unsigned *__restrict__ adler) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    unsigned long long a = 1, b = 0;
    for (int blk = 0; blk < n_blk; ++blk) {
        const long long start = (long long)blk * PL_ADLER_B;
        const long long n = row_bytes - start < PL_ADLER_B ? row_bytes - start : PL_ADLER_B;
        const unsigned *q = part + (row * n_blk + blk) * 2;
        b = (b + (unsigned long long)(n > 0 ? n : 0) * a + q[1]) % PL_ADLER_M;
        a = (a + q[0]) % PL_ADLER_M;
    }
    adler[row] = (unsigned)((b << 16) | a);
}

int64_t adler_blocks_of(int64_t row_bytes) { return row_bytes <= 0 ? 1 : (row_bytes + PL_ADLER_B - 1) / PL_ADLER_B; }

int check_panels(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, int64_t row_stride) {
    WC_CHECK(chrom_sizes && n_chrom >= 1 && n_chrom <= WC_CV_MAX_CHROM && panel_chrom && n_panels >= 1 && n_panels <= 1024, WC_E_ARG,
             "plot: %d chromosomes (1 .. %d), %d panels (1 .. 1024)", n_chrom, WC_CV_MAX_CHROM, n_panels);
    int64_t total = 0;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(chrom_sizes[c] >= 0 && chrom_sizes[c] < (1ll << 30), WC_E_ARG, "plot: chromosome %d has %lld bins", c + 1,
                 (long long)chrom_sizes[c]);
        total += chrom_sizes[c];
    }
    WC_CHECK(row_stride >= total, WC_E_ARG, "plot: rows of %lld values for %lld bins", (long long)row_stride, (long long)total);
    for (int p = 0; p < n_panels; ++p)
        WC_CHECK(panel_chrom[p] >= 1 && panel_chrom[p] <= n_chrom, WC_E_ARG, "plot: panel %d asks for chromosome %d of %d", p,
                 panel_chrom[p], n_chrom);
    return WC_OK;
}

}  // namespace

namespace wc {
int plot_check_page(const char *who, const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels,
                    int64_t row_stride, const int32_t *band_off) {
    int rc;
    if ((rc = check_panels(chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride))) return rc;
    if (band_off) {
        WC_CHECK(band_off[0] == 0, WC_E_ARG, "%s: unusable cytoband table", who);
        for (int p = 0; p < n_panels; ++p) WC_CHECK(band_off[p + 1] >= band_off[p], WC_E_ARG, "%s: unusable cytoband table", who);
    }
    return WC_OK;
}

int page_plan(wc_ctx *ctx, const char *who, const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels,
              int64_t row_stride, int max_calls, int columns, int width, int height, const double *bands, const int32_t *band_off,
              const char *names, int64_t n_samples, int name_cap, size_t tail_bytes, PagePlan &P) {
    int rc;
    if ((rc = plot_check_page(who, chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, band_off))) return rc;
    WC_CHECK(!band_off || bands || band_off[n_panels] == 0, WC_E_ARG, "%s: unusable cytoband table", who);
    std::vector<int32_t> boxes(4 * (size_t)n_panels);
    if (columns >= 1 && (rc = wc_plot_layout(width, height, (n_panels + columns - 1) / columns, columns, n_panels, boxes.data()))) return rc;
    int64_t longest = 0;
    for (int p = 0; p < n_panels; ++p) longest = chrom_sizes[panel_chrom[p] - 1] > longest ? chrom_sizes[panel_chrom[p] - 1] : longest;
    const int64_t cap64 = 1 + (longest + 1) / 2 + max_calls;             // alternating zeros: ceil(bins / 2) stretches
    WC_CHECK(cap64 <= INT_MAX / 2, WC_E_LIMIT, "%s: lists of %lld entries", who, (long long)cap64);
    P.n_panels = n_panels; P.cap = (int)cap64; P.has_cyto = band_off ? 1 : 0; P.name_cap = name_cap;
    // the block, 8-byte fields first
    const size_t n_bands = band_off ? band_off[n_panels] : 0, name_bytes = names ? (size_t)n_samples * name_cap : 0;
    const size_t off_chrom_off = 0, off_chrom_len = off_chrom_off + 8 * (size_t)n_chrom, off_bands = off_chrom_len + 8 * (size_t)n_chrom,
                 off_panel = off_bands + 32 * n_bands, off_boxes = off_panel + 4 * (size_t)n_panels,
                 off_band_off = off_boxes + 16 * (size_t)n_panels, off_names = off_band_off + 4 * (size_t)(n_panels + 1);
    P.tail = (off_names + name_bytes + 7) & ~(size_t)7;
    P.bytes = (P.tail + tail_bytes + 7) & ~(size_t)7;
    WC_HIP(hipSetDevice(ctx->device));
    if ((rc = ctx->pl_host_reserve(P.bytes)) || (rc = ctx->pl_tab.reserve(P.bytes))) return rc;
    unsigned char *h = ctx->pl_host;
    memset(h, 0, P.bytes);
    int64_t run = 0;
    for (int c = 0; c < n_chrom; ++c) {
        memcpy(h + off_chrom_off + 8 * c, &run, 8);
        memcpy(h + off_chrom_len + 8 * c, &chrom_sizes[c], 8);
        run += chrom_sizes[c];
    }
    if (n_bands) memcpy(h + off_bands, bands, 32 * n_bands);
    memcpy(h + off_panel, panel_chrom, 4 * (size_t)n_panels);
    if (columns >= 1) memcpy(h + off_boxes, boxes.data(), 16 * (size_t)n_panels);
    if (band_off) memcpy(h + off_band_off, band_off, 4 * (size_t)(n_panels + 1));
    if (name_bytes) memcpy(h + off_names, names, name_bytes);
    const unsigned char *tab = ctx->pl_tab.as<unsigned char>();
    P.chrom_off = (const long long *)(tab + off_chrom_off); P.chrom_len = (const long long *)(tab + off_chrom_len);
    P.bands = (const double *)(tab + off_bands); P.panel_chrom = (const int *)(tab + off_panel);
    P.boxes = (const int *)(tab + off_boxes); P.band_off = band_off ? (const int *)(tab + off_band_off) : nullptr;
    P.names = (const char *)(tab + off_names);
    P.tail_host = h + P.tail; P.tail_dev = tab + P.tail;
    return WC_OK;
}

int page_send(wc_ctx *ctx, hipStream_t stream, size_t from, size_t to) {
    WC_HIP(hipMemcpyAsync(ctx->pl_tab.as<unsigned char>() + from, ctx->pl_host + from, to - from, hipMemcpyHostToDevice, stream));
    WC_HIP(hipEventRecord(ctx->pl_sent, stream));
    return WC_OK;
}

int plot_list_launch(wc_ctx *ctx, hipStream_t stream, const PagePlan &P, const double *z, int64_t row_stride, int64_t n_samples,
                     const double *calls, const int32_t *n_calls, int max_calls, double thr, double mineffect, int cap) {
    WC_HIP(hipMemsetAsync(ctx->pl_status.p, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_plot_list, dim3((unsigned)P.n_panels, (unsigned)n_samples), dim3(PL_T), 0, stream, z, (long long)row_stride,
                       P.chrom_off, P.chrom_len, P.panel_chrom, calls, (const int *)n_calls, max_calls, thr, mineffect, cap,
                       ctx->pl_list.as<double>(), ctx->pl_counts.as<int>(), ctx->pl_status.as<int>());
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int HostBatch::stage(wc_ctx *ctx, const double *z_host, int64_t row_stride, int64_t n_samples, const double *calls_host,
                     const int32_t *n_calls_host, int max_calls, bool timed) {
    const size_t zb = (size_t)n_samples * row_stride * 8, cb = (size_t)n_samples * max_calls * 40, nb = (size_t)n_samples * 4;
    const size_t off_calls = (zb + 15) & ~(size_t)15, off_n = off_calls + ((cb + 15) & ~(size_t)15);
    int rc;
    if ((rc = ctx->tmp_a.reserve(off_n + nb + 16)) || (rc = ctx->tmp_c.reserve((size_t)n_samples * 8)) ||
        (rc = ctx->tmp_d.reserve((size_t)n_samples * 4)) || (timed && (rc = events.create())))
        return rc;
    unsigned char *base = ctx->tmp_a.as<unsigned char>();
    if (timed) (void)hipEventRecord((ev = events.e)[5], nullptr);
    if (zb && z_host) WC_HIP(hipMemcpy(base, z_host, zb, hipMemcpyHostToDevice));
    if (cb && calls_host) WC_HIP(hipMemcpy(base + off_calls, calls_host, cb, hipMemcpyHostToDevice));
    if (max_calls && n_calls_host) WC_HIP(hipMemcpy(base + off_n, n_calls_host, nb, hipMemcpyHostToDevice));
    z = z_host ? (const double *)base : nullptr;
    calls = calls_host ? (const double *)(base + off_calls) : nullptr;
    n_calls = n_calls_host ? (const int32_t *)(base + off_n) : nullptr;
    return WC_OK;
}

int HostBatch::collect(wc_ctx *ctx, const char *who, int64_t n_samples, int64_t dev_stride, unsigned char *streams_out,
                       int64_t out_stride, int64_t *out_len, uint32_t *adler_out) {
    int status = 0;
    WC_HIP(hipMemcpy(&status, ctx->pl_status.p, 4, hipMemcpyDeviceToHost));
    WC_CHECK(!status, WC_E_INTERNAL, "%s: a display list outgrew its capacity (status %d)", who, status);
    WC_HIP(hipMemcpy(out_len, ctx->tmp_c.p, (size_t)n_samples * 8, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(adler_out, ctx->tmp_d.p, (size_t)n_samples * 4, hipMemcpyDeviceToHost));
    // only the streams cross, each in a transfer of its own: one strided transfer as wide as the longest stream
    // (hipMemcpy2D) measured a quarter slower into the same pageable destination
    for (int64_t i = 0; i < n_samples; ++i) {
        WC_CHECK(out_len[i] >= 0 && out_len[i] <= dev_stride, WC_E_INTERNAL, "%s: a stream of %lld bytes in a slot of %lld", who,
                 (long long)out_len[i], (long long)dev_stride);
        if (out_len[i] > 0)
            WC_HIP(hipMemcpy(streams_out + i * out_stride, ctx->tmp_b.as<unsigned char>() + i * dev_stride, (size_t)out_len[i],
                             hipMemcpyDeviceToHost));
    }
    return WC_OK;
}

void HostBatch::times(double *times_ms) {
    if (!ev) return;
    (void)hipEventRecord(ev[6], nullptr);
    (void)hipEventSynchronize(ev[6]);
    const int from[6] = {5, 0, 1, 2, 3, 4}, to[6] = {0, 1, 2, 3, 4, 6};
    events.elapsed(6, from, to, times_ms);
    times_ms[6] = times_ms[7] = 0.0;
}
}  // namespace wc

extern "C" {

int wc_plot_layout(int width, int height, int rows, int columns, int n_panels, int32_t *boxes_out) {
    WC_CHECK(width >= 1 && height >= 1 && rows >= 1 && columns >= 1 && n_panels >= 0 && n_panels <= rows * columns && boxes_out &&
                 width <= (1 << 21) && height <= (1 << 21),
             WC_E_ARG, "plot layout: %d x %d units (at most 2097152 each), %d panels in %d rows of %d", width, height, n_panels, rows, columns);
    // the figure margins of the reference's subplots (left 0.125, right 0.9, top 0.88, bottom 0.11), in whole units: the
    // pixels of an image (wc_plot_image_bytes holds those to 32768) or the centipoints of a PDF page
    const int gx0 = width * 125 / 1000, gx1 = width - width / 10, gy0 = height * 12 / 100, gy1 = height - height * 11 / 100;
    const int cw = (gx1 - gx0) / columns, ch = (gy1 - gy0) / rows;
    for (int p = 0; p < n_panels; ++p) {
        const int r = p / columns, c = p % columns, cx = gx0 + c * cw, cy = gy0 + r * ch;
        boxes_out[4 * p + 0] = cx + cw * 12 / 100;      // room for the chromosome number
        boxes_out[4 * p + 1] = cy;
        boxes_out[4 * p + 2] = cx + cw;
        boxes_out[4 * p + 3] = cy + ch - ch * 15 / 100;
    }
    return WC_OK;
}

int wc_plot_list(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                 const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                 const int32_t *panel_chrom, int n_panels, int capacity, double *entries_out, int32_t *counts_out, int32_t *status_out) {
    WC_CHECK(ctx && n_samples >= 1 && n_samples <= 65535 && max_calls >= 0 && (max_calls == 0 || (calls && n_calls)) && capacity >= 0 &&
                 entries_out && counts_out && status_out && (results_z || row_stride == 0),
             WC_E_ARG, "plot list: unusable argument (1 .. 65535 samples)");
    int rc;
    wc::PagePlan P;                                       // no bands, boxes or names; the capacity is the caller's
    if ((rc = wc::page_plan(ctx, "plot", chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0,
                            0, 0, P)) ||
        (rc = wc::page_send(ctx, nullptr, 0, P.bytes)))
        return rc;
    const size_t zb = (size_t)n_samples * row_stride * 8, cb = (size_t)n_samples * max_calls * 40, nb = (size_t)n_samples * 4;
    const size_t eb = (size_t)n_samples * n_panels * capacity * PL_F * 8, kb = (size_t)n_samples * n_panels * 4;
    if ((rc = ctx->tmp_a.reserve(zb + 8)) || (rc = ctx->tmp_b.reserve(cb + 8)) || (rc = ctx->tmp_c.reserve(nb + 8)) ||
        (rc = ctx->pl_list.reserve(eb + 8)) || (rc = ctx->pl_counts.reserve(kb)) || (rc = ctx->pl_status.reserve(8)))
        return rc;
    if (zb) WC_HIP(hipMemcpy(ctx->tmp_a.p, results_z, zb, hipMemcpyHostToDevice));
    if (cb) WC_HIP(hipMemcpy(ctx->tmp_b.p, calls, cb, hipMemcpyHostToDevice));
    if (max_calls) WC_HIP(hipMemcpy(ctx->tmp_c.p, n_calls, nb, hipMemcpyHostToDevice));
    if (eb) WC_HIP(hipMemset(ctx->pl_list.p, 0, eb));
    if ((rc = wc::plot_list_launch(ctx, nullptr, P, ctx->tmp_a.as<double>(), row_stride, n_samples, ctx->tmp_b.as<double>(),
                                   max_calls ? ctx->tmp_c.as<int32_t>() : nullptr, max_calls, threshold, mineffect, capacity)))
        return rc;
    if (eb) WC_HIP(hipMemcpy(entries_out, ctx->pl_list.p, eb, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(counts_out, ctx->pl_counts.p, kb, hipMemcpyDeviceToHost));
    WC_HIP(hipMemcpy(status_out, ctx->pl_status.p, 4, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_adler32_rows_dev(wc_ctx *ctx, void *stream_, const unsigned char *src, int64_t n_rows, int64_t row_bytes, int64_t src_stride,
                        uint32_t *adler) {
    WC_CHECK(ctx && n_rows >= 0 && row_bytes >= 0 && src_stride >= row_bytes && (src || n_rows == 0 || row_bytes == 0) &&
                 (n_rows == 0 || adler),
             WC_E_ARG, "adler32: unusable argument");
    if (n_rows == 0) return WC_OK;
    const int64_t n_blk = adler_blocks_of(row_bytes);
    WC_CHECK(n_rows <= 65535 && n_blk <= INT_MAX / 4, WC_E_LIMIT, "adler32: %lld rows (at most 65535) of %lld blocks", (long long)n_rows,
             (long long)n_blk);
    WC_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if ((rc = ctx->pl_part.reserve((size_t)n_rows * n_blk * 8))) return rc;
    hipLaunchKernelGGL(k_adler_blocks, dim3((unsigned)n_blk, (unsigned)n_rows), dim3(PL_T), 0, stream, src, (long long)row_bytes,
                       (long long)src_stride, (int)n_blk, ctx->pl_part.as<unsigned>());
    WC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_adler_rows, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, stream, (const unsigned *)ctx->pl_part.as<unsigned>(),
                       (long long)row_bytes, (int)n_blk, (long long)n_rows, (unsigned *)adler);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

int64_t wc_plot_image_bytes(int width, int height) {
    if (width < 1 || height < 1 || width > 32768 || height > 32768) return -1;
    return (int64_t)height * (1 + 3 * (int64_t)width);
}

// ev: NULL, or six events recorded behind the tables' copy and the four stages
static int plot_batch_enqueue(wc_ctx *ctx, hipStream_t stream, const double *results_z, int64_t row_stride, int64_t n_samples,
                              const int64_t *chrom_sizes, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls,
                              double threshold, double mineffect, const int32_t *panel_chrom, int n_panels, int columns,
                              const double *bands, const int32_t *band_off, const char *names, int name_cap, int width, int height,
                              int dpi, unsigned char *scanlines, int64_t scan_stride, unsigned char *streams, int64_t out_stride,
                              int64_t *out_len, uint32_t *adler, hipEvent_t *ev) {
    WC_CHECK(ctx && n_samples >= 1 && max_calls >= 0 && (max_calls == 0 || (calls && n_calls)) && names && name_cap >= 1 && columns >= 1 &&
                 dpi >= 1 && dpi <= 100000 && streams && out_len && adler && (results_z || row_stride == 0),
             WC_E_ARG, "plot: unusable argument");
    WC_CHECK(threshold > 0.0 && threshold <= DBL_MAX, WC_E_ARG, "plot: threshold_z %g is not a positive finite number", threshold);
    const int64_t img = wc_plot_image_bytes(width, height);
    WC_CHECK(img > 0, WC_E_ARG, "plot: %d x %d pixels (1 .. 32768 each)", width, height);
    // what the deflate stage takes in one call (wc_deflate_rows_dev), held up front
    const int64_t n_blk = (img + wc_deflate_block_bytes() - 1) / wc_deflate_block_bytes();
    WC_CHECK(n_samples <= 65535 && n_blk <= INT_MAX / 2 && n_samples <= (int64_t)INT_MAX / n_blk, WC_E_LIMIT,
             "plot: %lld images of %lld bytes in one call; split the batch", (long long)n_samples, (long long)img);
    WC_CHECK(out_stride >= wc_deflate_bound(img), WC_E_ARG, "plot: %lld bytes per stream, wc_deflate_bound(%lld) is %lld",
             (long long)out_stride, (long long)img, (long long)wc_deflate_bound(img));
    WC_CHECK(!scanlines || (scan_stride >= img && scan_stride % 16 == 0), WC_E_ARG, "plot: scanline stride %lld (a multiple of 16, at least %lld)",
             (long long)scan_stride, (long long)img);
    int rc;
    wc::PagePlan P;                                       // the tail: the raster kernel's arguments, then the font
    if ((rc = wc::page_plan(ctx, "plot", chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, max_calls, columns, width, height, bands,
                            band_off, names, n_samples, name_cap, sizeof(RasterArgs) + sizeof(WC_FONT_ROWS), P)))
        return rc;
    const int cap = P.cap;
    const int64_t stride = scanlines ? scan_stride : (img + 15) / 16 * 16;     // the stride is padded, never the row
    if ((rc = ctx->pl_list.reserve((size_t)n_samples * n_panels * cap * PL_F * 8)) || (rc = ctx->pl_counts.reserve((size_t)n_samples * (n_panels + 1) * 4)) ||
        (rc = ctx->pl_status.reserve(8)) || (!scanlines && (rc = ctx->pl_img.reserve((size_t)n_samples * stride))))
        return rc;
    unsigned char *image = scanlines ? scanlines : ctx->pl_img.as<unsigned char>();
    RasterArgs A;
    A.W = width; A.H = height; A.s = (2 * dpi + 100) / 200 > 1 ? (2 * dpi + 100) / 200 : 1;       // max(1, round(dpi / 100))
    A.P = n_panels; A.cap = cap; A.has_cyto = P.has_cyto; A.name_cap = name_cap;
    A.row_stride = row_stride; A.img_stride = stride; A.thr = threshold; A.z = results_z;
    A.chrom_off = P.chrom_off; A.chrom_len = P.chrom_len; A.panel_chrom = P.panel_chrom; A.boxes = P.boxes; A.band_off = P.band_off;
    A.bands = P.bands; A.entries = ctx->pl_list.as<double>(); A.counts = ctx->pl_counts.as<int>(); A.names = P.names;
    A.font = P.tail_dev + sizeof(RasterArgs); A.out = image;
    memcpy(P.tail_host, &A, sizeof(RasterArgs));
    memcpy(P.tail_host + sizeof(RasterArgs), WC_FONT_ROWS, sizeof(WC_FONT_ROWS));
    if ((rc = wc::page_send(ctx, stream, 0, P.bytes))) return rc;      // the whole block in one transfer
    if (ev) WC_HIP(hipEventRecord(ev[0], stream));
    if ((rc = wc::plot_list_launch(ctx, stream, P, results_z, row_stride, n_samples, calls, n_calls, max_calls, threshold, mineffect, cap)))
        return rc;
    if (ev) WC_HIP(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(k_plot_raster, dim3((unsigned)((width + PL_T - 1) / PL_T), (unsigned)((height + PL_BAND_ROWS - 1) / PL_BAND_ROWS), (unsigned)n_samples),
                       dim3(PL_T), 0, stream, (const RasterArgs *)P.tail_dev);
    WC_HIP(hipGetLastError());
    if (ev) WC_HIP(hipEventRecord(ev[2], stream));
    if ((rc = wc_adler32_rows_dev(ctx, stream, image, n_samples, img, stride, adler))) return rc;
    if (ev) WC_HIP(hipEventRecord(ev[3], stream));
    // the CRC-32 words of the deflate call are not needed (the PNG's checksums are Adler-32 and the chunk CRCs); they go
    // behind the lists' counts
    if ((rc = wc_deflate_rows_dev(ctx, stream, image, n_samples, img, stride, streams, out_stride, out_len,
                                  ctx->pl_counts.as<uint32_t>() + n_samples * n_panels)))
        return rc;
    if (ev) WC_HIP(hipEventRecord(ev[4], stream));
    return WC_OK;
}

int wc_plot_batch_dev(wc_ctx *ctx, void *stream, const double *results_z, int64_t row_stride, int64_t n_samples,
                      const int64_t *chrom_sizes_host, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls,
                      double threshold, double mineffect, const int32_t *panel_chrom_host, int n_panels, int columns,
                      const double *bands_host, const int32_t *band_off_host, const char *names_host, int name_cap, int width, int height,
                      int dpi, unsigned char *scanlines, int64_t scan_stride, unsigned char *streams, int64_t out_stride, int64_t *out_len,
                      uint32_t *adler, int32_t *status) {
    WC_CHECK(status, WC_E_ARG, "plot: NULL status word");
    int rc = plot_batch_enqueue(ctx, (hipStream_t)stream, results_z, row_stride, n_samples, chrom_sizes_host, n_chrom, calls, n_calls,
                                max_calls, threshold, mineffect, panel_chrom_host, n_panels, columns, bands_host, band_off_host, names_host,
                                name_cap, width, height, dpi, scanlines, scan_stride, streams, out_stride, out_len, adler, nullptr);
    if (rc) return rc;
    WC_HIP(hipMemcpyAsync(status, ctx->pl_status.p, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WC_OK;
}

int wc_plot_batch(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                  const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                  const int32_t *panel_chrom, int n_panels, int columns, const double *bands, const int32_t *band_off, const char *names,
                  int name_cap, int width, int height, int dpi, unsigned char *scanlines_out, unsigned char *streams_out,
                  int64_t out_stride, int64_t *out_len, uint32_t *adler_out, double *times_ms) {
    WC_CHECK(ctx && n_samples >= 1 && max_calls >= 0 && streams_out && out_len && adler_out, WC_E_ARG, "plot: unusable argument");
    const int64_t img = wc_plot_image_bytes(width, height);
    WC_CHECK(img > 0, WC_E_ARG, "plot: %d x %d pixels (1 .. 32768 each)", width, height);
    WC_CHECK(out_stride >= wc_deflate_bound(img), WC_E_ARG, "plot: %lld bytes per stream, wc_deflate_bound(%lld) is %lld",
             (long long)out_stride, (long long)img, (long long)wc_deflate_bound(img));
    WC_CHECK(n_samples <= 65535 && (double)n_samples * (double)out_stride < 1e12, WC_E_LIMIT, "plot: %lld images of %lld bytes in one call; split the batch",
             (long long)n_samples, (long long)img);
    WC_HIP(hipSetDevice(ctx->device));
    const int64_t stride = (img + 15) / 16 * 16;
    int rc;
    wc::HostBatch B;
    if ((rc = ctx->tmp_b.reserve((size_t)n_samples * out_stride)) || (rc = ctx->pl_img.reserve((size_t)n_samples * stride)) ||
        (rc = B.stage(ctx, results_z, row_stride, n_samples, calls, n_calls, max_calls, times_ms != nullptr)) ||
        (rc = plot_batch_enqueue(ctx, nullptr, B.z, row_stride, n_samples, chrom_sizes, n_chrom, B.calls, B.n_calls, max_calls, threshold,
                                 mineffect, panel_chrom, n_panels, columns, bands, band_off, names, name_cap, width, height, dpi,
                                 ctx->pl_img.as<unsigned char>(), stride, ctx->tmp_b.as<unsigned char>(), out_stride,
                                 ctx->tmp_c.as<int64_t>(), ctx->tmp_d.as<uint32_t>(), B.ev)) ||
        (rc = B.collect(ctx, "plot", n_samples, out_stride, streams_out, out_stride, out_len, adler_out)))
        return rc;
    if (scanlines_out)
        WC_HIP(hipMemcpy2D(scanlines_out, (size_t)img, ctx->pl_img.p, (size_t)stride, (size_t)img, (size_t)n_samples, hipMemcpyDeviceToHost));
    B.times(times_ms);      // [1] list [2] raster [3] Adler-32 [4] deflate
    return WC_OK;
}

int64_t wc_png_bytes(int64_t deflate_len) { return deflate_len < 0 ? -1 : deflate_len + 63; }

int wc_png_assemble(int width, int height, const unsigned char *deflate, int64_t deflate_len, uint32_t adler, unsigned char *out,
                    int64_t cap, int64_t *out_len) {
    WC_CHECK(width >= 1 && height >= 1 && deflate && deflate_len >= 1 && out && out_len, WC_E_ARG, "png: unusable argument");
    WC_CHECK(deflate_len <= (int64_t)INT_MAX - 6, WC_E_LIMIT, "png: a stream of %lld bytes does not fit one IDAT chunk", (long long)deflate_len);
    WC_CHECK(cap >= wc_png_bytes(deflate_len), WC_E_ARG, "png: room for %lld bytes, wc_png_bytes(%lld) is %lld", (long long)cap,
             (long long)deflate_len, (long long)wc_png_bytes(deflate_len));
    using wc::put32;
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    unsigned char *p = out;
    memcpy(p, sig, 8);
    p += 8;
    put32(p, 13);
    memcpy(p + 4, "IHDR", 4);
    put32(p + 8, (uint32_t)width);
    put32(p + 12, (uint32_t)height);
    p[16] = 8;      // bits per channel
    p[17] = 2;      // RGB
    p[18] = p[19] = p[20] = 0;
    put32(p + 21, (uint32_t)crc32(0, p + 4, 17));
    p += 25;
    put32(p, (uint32_t)(deflate_len + 6));
    memcpy(p + 4, "IDAT", 4);
    p[8] = 0x78;    // zlib header: deflate, 32 KiB window, fastest
    p[9] = 0x01;
    memcpy(p + 10, deflate, (size_t)deflate_len);
    put32(p + 10 + deflate_len, adler);
    put32(p + 14 + deflate_len, (uint32_t)crc32(0, p + 4, (unsigned)(deflate_len + 10)));
    p += 18 + deflate_len;
    put32(p, 0);
    memcpy(p + 4, "IEND", 4);
    put32(p + 8, (uint32_t)crc32(0, p + 4, 4));
    p += 12;
    *out_len = p - out;
    return WC_OK;
}

}  // extern "C"
