// plotpdf: result files -> vector PDF pages.  The page's content stream is text; one kernel writes it:
//   k_pdf_content   a workgroup per span of PD_CHUNK bytes of a sample's row.  The row is a run of sections (the table the
//                   host makes: start, record kind, record count, record width), every record of a kind as wide as every
//                   other, so the records that overlap a span follow from two divisions.  A lane writes one record at a
//                   time, byte by byte, into the span's image in LDS (a record that crosses the span's end writes the part
//                   inside); after one barrier every lane stores 16 aligned bytes of the image.  Every byte of the row, and
//                   of the padding up to the next multiple of 16, is written by every call.
// The display list is k_plot_list's (plot.hip), the checksum wc_adler32_rows_dev's, the compression
// wc_deflate_rows_dev's.  The sections' slot counts come from the lists' counts, which the host reads back: THE CALL
// SYNCHRONISES ONCE, between the list kernel and the content kernel.  Every coordinate is an integer number of
// centipoints, written as a fixed field of 9 bytes; tests/pdf_restated.py repeats the stream in numpy and the tests compare
// the bytes.  wc_pdf_assemble (host) puts the file's objects around one compressed stream.
#include <float.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "plot_label.h"

namespace {

const int PD_T = 256;
const int PD_CHUNK = 16 * PD_T;     // bytes of a row per workgroup
const int PD_LIM = 9999999;         // a coordinate's limit in centipoints
const int PD_F = 9;                 // fields of a list entry (plot.hip)
const int PD_CALL = 3;
const int PD_LABEL_CAP = 12;        // "-999999999.9"
const int PD_TITLE_PREFIX = 45;     // strlen("Z-score versus chromosomal position - Sample ")
const int PD_LEGEND_CAP = 17;
const int PD_PER_PANEL = 11;        // sections of a panel

enum { K_HEAD, K_BAND, K_LIST, K_GREY, K_EDGE, K_POLYHEAD, K_VERTEX, K_STROKE, K_LABEL, K_FRAMEQ, K_CHROM, K_TITLE, K_LEGEND };
// bytes of a record of every kind (the title's grows with the longest name: 2 hex digits per character)
const int PD_WIDTH[13] = {49, 138, 73, 81, 162, 57, 22, 2, 96, 82, 96, 73, 179};

struct PdfSec {
    long long start;
    int kind, panel, count, width;
};

struct PdfArgs {
    int Wc, Hc, P, cap, has_cyto, name_cap, n_sec, title_cap;
    long long row_stride, row_bytes, out_stride;
    double thr;
    const double *z;
    const long long *chrom_off, *chrom_len;
    const int *panel_chrom, *boxes, *band_off;
    const double *bands, *entries;
    const int *counts;
    const char *names;
    const PdfSec *secs;
};

// the reference's palette and its line grey in hundredths (wisetools.py:531-541)
__device__ const unsigned char PD_CENTS[9][3] = {{0, 0, 0},   {90, 60, 0}, {35, 70, 90}, {0, 60, 50}, {95, 90, 25},
                                                 {0, 45, 70}, {80, 40, 0}, {80, 60, 70}, {70, 70, 70}};
const int PD_GREY = 8;

// pl_rnd limited to +-PD_LIM; NaN lies at the lower limit (where pl_rnd's own value for it would end up: the test is
// spelled out because without it k_pdf_content takes 90 vector registers instead of 83)
__device__ __forceinline__ int pd_rnd(double v) {
    if (!(v == v)) return -PD_LIM;
    const int q = pl_rnd(v);
    return q < -PD_LIM ? -PD_LIM : (q > PD_LIM ? PD_LIM : q);
}

// pl_alpha's value through pd_rnd: with pl_alpha itself the kernel's instructions change and the content stage measured
// 0.6 - 1.1 % slower; this form compiles to the instructions it had before
__device__ __forceinline__ int pd_alpha(double alpha) {
    const int a = pd_rnd(255.0 * alpha);
    return a < 0 ? 0 : (a > 255 ? 255 : a);
}

// ---- the records' templates ---------------------------------------------------------------------------------------------
// A record is one or two lines of template text; a text record's last line is a head, the hex string and a tail.  A
// template byte >= 0x80 is a placeholder: with n = its low four bits and f = bits 4 .. 6, n = 0 .. 8 is byte n of number
// field f, n = 9 digit f of the graphics state's alpha, n = 10 digit f & 1 of colour channel f >> 1, n = 11 digit f of the
// line width, n = 12 the path operator, n = 13 the pattern's number.
#define PD_N0 "\x80" "\x81" "\x82" "\x83" "\x84" "\x85" "\x86" "\x87" "\x88"
#define PD_N1 "\x90" "\x91" "\x92" "\x93" "\x94" "\x95" "\x96" "\x97" "\x98"
#define PD_N2 "\xa0" "\xa1" "\xa2" "\xa3" "\xa4" "\xa5" "\xa6" "\xa7" "\xa8"
#define PD_N3 "\xb0" "\xb1" "\xb2" "\xb3" "\xb4" "\xb5" "\xb6" "\xb7" "\xb8"
#define PD_N4 "\xc0" "\xc1" "\xc2" "\xc3" "\xc4" "\xc5" "\xc6" "\xc7" "\xc8"
#define PD_N5 "\xd0" "\xd1" "\xd2" "\xd3" "\xd4" "\xd5" "\xd6" "\xd7" "\xd8"
#define PD_N6 "\xe0" "\xe1" "\xe2" "\xe3" "\xe4" "\xe5" "\xe6" "\xe7" "\xe8"
#define PD_N7 "\xf0" "\xf1" "\xf2" "\xf3" "\xf4" "\xf5" "\xf6" "\xf7" "\xf8"
#define PD_GS " /A" "\x89" "\x99" "\xa9" " gs "
#define PD_RGB "0." "\x8a" "\x9a" " 0." "\xaa" "\xba" " 0." "\xca" "\xda"
#define PD_LW " /A255 gs " "\x8b" "." "\x9b" "\xab" " w "
#define PD_T_FILL PD_GS PD_RGB " rg " PD_N0 " " PD_N1 " " PD_N2 " " PD_N3 " re f\n"
#define PD_T_PAT "/Pattern cs /P" "\x8d" " scn " PD_N4 " " PD_N5 " " PD_N6 " " PD_N7 " re f\n"
#define PD_T_LINE_A PD_LW PD_RGB " RG " PD_N0 " " PD_N1 " m " PD_N2 " " PD_N3 " l S\n"
#define PD_T_LINE_B PD_LW PD_RGB " RG " PD_N4 " " PD_N5 " m " PD_N6 " " PD_N7 " l S\n"
#define PD_T_HEAD "q " PD_N0 " " PD_N1 " " PD_N2 " " PD_N3 " re W n\n"
#define PD_T_POLY " /A255 gs 0.50 w 0.00 0.45 0.70 RG " PD_N0 " " PD_N1 " m\n"
#define PD_T_VERT PD_N0 " " PD_N1 " " "\x8c" "\n"
#define PD_T_STROKE "S\n"
#define PD_T_FRAMEQ " /A255 gs 1.00 w 0.00 0.00 0.00 RG " PD_N0 " " PD_N1 " " PD_N2 " " PD_N3 " re S\nQ\n"
#define PD_T_TEXT8 " /A255 gs 0.00 0.00 0.00 rg BT /F1 8 Tf " PD_N4 " " PD_N5 " Td <"
#define PD_T_TEXT12 " /A255 gs 0.00 0.00 0.00 rg BT /F1 12 Tf " PD_N4 " " PD_N5 " Td <"
#define PD_T_TAIL "> Tj ET\n"
#define PD_LEN(t) ((int)sizeof(t) - 1)

__device__ const unsigned char PD_TAB[] = PD_T_FILL PD_T_PAT PD_T_LINE_A PD_T_LINE_B PD_T_HEAD PD_T_POLY PD_T_VERT PD_T_STROKE PD_T_FRAMEQ
    PD_T_TEXT8 PD_T_TEXT12 PD_T_TAIL;
const int O_FILL = 0, O_PAT = O_FILL + PD_LEN(PD_T_FILL), O_LINE_A = O_PAT + PD_LEN(PD_T_PAT), O_LINE_B = O_LINE_A + PD_LEN(PD_T_LINE_A),
          O_HEAD = O_LINE_B + PD_LEN(PD_T_LINE_B), O_POLY = O_HEAD + PD_LEN(PD_T_HEAD), O_VERT = O_POLY + PD_LEN(PD_T_POLY),
          O_STROKE = O_VERT + PD_LEN(PD_T_VERT), O_FRAMEQ = O_STROKE + PD_LEN(PD_T_STROKE), O_TEXT8 = O_FRAMEQ + PD_LEN(PD_T_FRAMEQ),
          O_TEXT12 = O_TEXT8 + PD_LEN(PD_T_TEXT8), O_TAIL = O_TEXT12 + PD_LEN(PD_T_TEXT12);
const int L_FILL = PD_LEN(PD_T_FILL), L_PAT = PD_LEN(PD_T_PAT), L_LINE = PD_LEN(PD_T_LINE_A), L_TEXT8 = PD_LEN(PD_T_TEXT8),
          L_TEXT12 = PD_LEN(PD_T_TEXT12), L_TAIL = PD_LEN(PD_T_TAIL);
static_assert(L_FILL == 73 && L_PAT == 65 && L_LINE == 81 && PD_LEN(PD_T_LINE_B) == 81 && PD_LEN(PD_T_HEAD) == 49 && PD_LEN(PD_T_POLY) == 57 &&
                  PD_LEN(PD_T_VERT) == 22 && PD_LEN(PD_T_STROKE) == 2 && PD_LEN(PD_T_FRAMEQ) == 82 && L_TEXT8 == 64 && L_TEXT12 == 65 &&
                  L_TAIL == 8,
              "the records' widths are the section table's (PD_WIDTH)");
static_assert(L_FILL + L_PAT == 138 && 2 * L_LINE == 162 && L_TEXT8 + 2 * PD_LABEL_CAP + L_TAIL == 96 && L_TEXT12 + L_TAIL == 73 &&
                  L_FILL + L_TEXT8 + 2 * PD_LEGEND_CAP + L_TAIL == 179,
              "the records' widths are the section table's (PD_WIDTH)");

__device__ const char PD_TITLE[] = "Z-score versus chromosomal position - Sample ";
__device__ const char PD_LEGEND[4][PD_LEGEND_CAP + 1] = {"Called region", "Uncallable region", "Z-score per bin", "Z-score threshold"};

// byte j of the fixed field of 9 bytes: right-aligned, an optional '-', the whole points, '.', two digits
__device__ __forceinline__ int pd_num_char(int q, int j) {
    q = q < -PD_LIM ? -PD_LIM : (q > 99999999 ? 99999999 : q);
    const bool neg = q < 0;
    const unsigned a = (unsigned)(neg ? -q : q), whole = a / 100u;
    if (j == 6) return '.';
    if (j == 7) return '0' + (int)(a / 10u % 10u);
    if (j == 8) return '0' + (int)(a % 10u);
    const int nd = 1 + (whole >= 10u) + (whole >= 100u) + (whole >= 1000u) + (whole >= 10000u) + (whole >= 100000u);
    const int k = j - (6 - nd);                         // the digit's index, -1: the sign's place
    if (k < 0) return k == -1 && neg ? '-' : ' ';
    const unsigned div = j == 0 ? 100000u : j == 1 ? 10000u : j == 2 ? 1000u : j == 3 ? 100u : j == 4 ? 10u : 1u;
    return '0' + (int)(whole / div % 10u);
}

// a panel's box and mappings (the box in centipoints)
struct Panel {
    int bx0, by0, bx1, by1, n_ent, nb, chrom;
    long long len;
    double bw, bh, xmax, yhi, yspan;
    const double *ent, *zr;
    __device__ __forceinline__ int qx(double x) const { return pd_rnd((x * bw) / xmax + bx0); }
    __device__ __forceinline__ int qy(double y) const { return pd_rnd(((yhi - y) * bh) / yspan + by0); }
};

__device__ __forceinline__ Panel pd_panel(const PdfArgs &A, long long smp, int p) {
    Panel Q;
    const int *b = A.boxes + 4 * p;
    Q.bx0 = b[0]; Q.by0 = b[1]; Q.bx1 = b[2]; Q.by1 = b[3];
    Q.bw = (double)(Q.bx1 - Q.bx0);
    Q.bh = (double)(Q.by1 - Q.by0);
    Q.chrom = A.panel_chrom[p];
    Q.len = A.chrom_len[Q.chrom - 1];
    Q.zr = A.z + smp * A.row_stride + A.chrom_off[Q.chrom - 1];
    Q.xmax = Q.len > 0 ? (double)Q.len : 1.0;
    Q.ent = A.entries + (smp * A.P + p) * (long long)A.cap * PD_F;
    const int n = A.counts[smp * A.P + p];
    Q.n_ent = n > A.cap ? A.cap : n;
    Q.nb = A.band_off ? A.band_off[p + 1] - A.band_off[p] : 0;
    pl_yrange(Q.ent[4], Q.ent[5], A.thr, A.has_cyto, Q.yhi, Q.yspan);
    return Q;
}

// Record r of a section: its numbers first, then its bytes inside the span [c0, c0 + PD_CHUNK) from the templates.  A part
// that draws nothing (on == false) keeps its line ends and is spaces otherwise.
__device__ __forceinline__ void pd_record(const PdfArgs &A, long long smp, const PdfSec &sec, long long r, unsigned char *lds,
                                          long long c0) {
    int v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0, v6 = 0, v7 = 0;       // the number fields
    int a8 = 255, colour = 0, lw = 50, op = 'l', pat = '1';
    bool on1 = true, on2 = true;
    int t1 = 0, len1 = 0, t2 = 0, len2 = 0, hexcap = 0;                       // the two parts' templates; a text part's characters
    int tkind = 0, tn = 0, neg = 0, which = 0;                                // the text: 0 a label, 1 a number, 2 the title, 3 legend
    bool ok = false;
    unsigned long long tenths = 0, number = 0;
    const char *name = A.names + smp * A.name_cap;
    const int Hc = A.Hc, Wc = A.Wc;
    const double thr = A.thr, cyto_y = -thr - thr / 2.0;
    if (sec.kind == K_TITLE) {
        int name_len = 0;
        while (name_len < A.name_cap - 1 && name[name_len]) ++name_len;
        tkind = 2; tn = PD_TITLE_PREFIX + name_len;
        t2 = O_TEXT12; len2 = L_TEXT12; hexcap = A.title_cap;
        v4 = (Wc >> 1) - tn * 360; v5 = Hc - (Hc * 7) / 100;
    } else if (sec.kind == K_LEGEND) {
        // two columns of two entries, filled column by column as the reference's ncol=2 legend
        which = (int)r;
        const int ew = 21 * 480, ex = ((Wc - 2 * ew) >> 1) + (which >> 1) * ew, by = 2400 - (which & 1) * 1600;
        tkind = 3; tn = which == 0 ? 13 : which == 2 ? 15 : 17;
        colour = which == 0 ? 1 : which == 1 ? 7 : which == 2 ? 5 : PD_GREY;
        t1 = O_FILL; len1 = L_FILL; t2 = O_TEXT8; len2 = L_TEXT8; hexcap = PD_LEGEND_CAP;
        v0 = ex; v1 = by; v2 = 960; v3 = 600; v4 = ex + 1440; v5 = by;
    } else {
        const Panel Q = pd_panel(A, smp, sec.panel);
        switch (sec.kind) {
        case K_HEAD:
            t1 = O_HEAD; len1 = PD_LEN(PD_T_HEAD);
            v0 = Q.bx0; v1 = Hc - Q.by1; v2 = Q.bx1 - Q.bx0; v3 = Q.by1 - Q.by0;
            break;
        case K_BAND: {
            const double *bd = A.bands + 4 * (A.band_off[sec.panel] + r);
            const int hatch = (int)bd[3], top = Q.qy(-thr), bot = Q.qy(cyto_y), x0 = Q.qx(bd[0]), x1 = Q.qx(bd[1]);
            t1 = O_FILL; len1 = L_FILL; t2 = O_PAT; len2 = L_PAT;
            on1 = hatch >= 0;                                               // (hatch -1: a band without a rectangle)
            on2 = hatch == 1 || hatch == 2;
            pat = hatch == 2 ? '2' : '1';
            a8 = pd_alpha(bd[2]);
            v0 = v4 = x0; v1 = v5 = Hc - bot; v2 = v6 = x1 - x0; v3 = v7 = bot - top;
            break;
        }
        case K_LIST: {
            const bool have = r + 1 < Q.n_ent;
            const double *e = Q.ent + (have ? r + 1 : 0) * PD_F;
            const double ya = e[4], yb = e[5];
            const int qt = Q.qy(ya > yb ? ya : yb), qb = Q.qy(ya > yb ? yb : ya), x0 = Q.qx(e[2]), x1 = Q.qx(e[3]);
            t1 = O_FILL; len1 = L_FILL;
            on1 = have;
            colour = (int)e[6];
            a8 = pd_alpha(e[7]);
            v0 = x0; v1 = Hc - qb; v2 = x1 - x0; v3 = qb - qt;
            break;
        }
        case K_GREY: {
            const double y = r == 0 ? 0.0 : r == 1 ? thr : r == 2 ? -thr : cyto_y;
            t1 = O_LINE_A; len1 = L_LINE;
            on1 = r < 3 || Q.nb > 0;
            lw = r == 0 ? 100 : 75;
            colour = PD_GREY;
            v0 = Q.bx0; v2 = Q.bx1; v1 = v3 = Hc - Q.qy(y);
            break;
        }
        case K_EDGE: {
            const bool have = r + 1 < Q.n_ent && Q.ent[(r + 1) * PD_F] == (double)PD_CALL;
            const double *e = Q.ent + (have ? r + 1 : 0) * PD_F;
            t1 = O_LINE_A; len1 = L_LINE; t2 = O_LINE_B; len2 = L_LINE;
            on1 = on2 = have;
            colour = (int)e[6];
            v0 = v2 = Q.qx(e[2]); v4 = v6 = Q.qx(e[3]);
            v1 = v5 = Hc - Q.by1; v3 = v7 = Hc - Q.by0;
            break;
        }
        case K_POLYHEAD:
            t1 = O_POLY; len1 = PD_LEN(PD_T_POLY);
            v0 = Q.bx0; v1 = Hc - Q.by1;
            break;
        case K_VERTEX: {
            const double v = Q.zr[r];
            const bool fin = __builtin_isfinite(v);
            t1 = O_VERT; len1 = PD_LEN(PD_T_VERT);
            on1 = fin;
            op = r == 0 || !__builtin_isfinite(Q.zr[r - 1]) ? 'm' : 'l';
            v0 = Q.qx((double)r); v1 = Hc - Q.qy(fin ? v : 0.0);
            break;
        }
        case K_STROKE:
            t1 = O_STROKE; len1 = PD_LEN(PD_T_STROKE);
            break;
        case K_LABEL: {
            const bool have = r + 1 < Q.n_ent && Q.ent[(r + 1) * PD_F] == (double)PD_CALL;
            const double *e = Q.ent + (have ? r + 1 : 0) * PD_F;
            const double zc = e[8];
            ok = pl_label_tenths(zc, tenths, neg);
            tkind = 0; tn = pl_label_len(ok, tenths, neg);
            t2 = O_TEXT8; len2 = L_TEXT8; hexcap = PD_LABEL_CAP;
            on2 = have;
            const int edge = Hc - Q.qy(e[5]);
            v4 = Q.qx(e[2] + (e[3] - e[2]) / 2.0) - tn * 240;
            v5 = zc > 0.0 ? edge - 700 : edge + 300;                        // anchored top / bottom
            break;
        }
        case K_FRAMEQ:
            t1 = O_FRAMEQ; len1 = PD_LEN(PD_T_FRAMEQ);
            v0 = Q.bx0 + 50; v1 = Hc - Q.by1 + 50; v2 = Q.bx1 - Q.bx0 - 100; v3 = Q.by1 - Q.by0 - 100;
            break;
        case K_CHROM:
            number = (unsigned long long)Q.chrom;
            tkind = 1; tn = pl_digits(number);
            t2 = O_TEXT8; len2 = L_TEXT8; hexcap = PD_LABEL_CAP;
            v4 = Q.bx0 - 400 - tn * 480; v5 = Hc - ((Q.by0 + Q.by1) >> 1) - 250;
            break;
        default:
            break;
        }
    }
    colour = colour < 0 || colour > 8 ? 0 : colour;
    const long long start = sec.start + r * sec.width;
    const int b0 = c0 > start ? (int)(c0 - start) : 0;
    const int b1 = start + sec.width > c0 + PD_CHUNK ? (int)(c0 + PD_CHUNK - start) : sec.width;
    for (int b = b0; b < b1; ++b) {
        int c;
        bool on = on1;
        if (b < len1) {
            c = PD_TAB[t1 + b];
        } else {
            const int d = b - len1, h = d - len2;
            on = on2;
            if (h < 0) {
                c = PD_TAB[t2 + d];
            } else if (h < 2 * hexcap) {
                const int k = h >> 1;
                int ch = ' ';
                if (k < tn) {
                    if (tkind == 0) ch = pl_label_char(ok, tenths, neg, tn, k);
                    else if (tkind == 1) ch = pl_digit(number, tn, k);
                    else if (tkind == 2) ch = k < PD_TITLE_PREFIX ? PD_TITLE[k] : (unsigned char)name[k - PD_TITLE_PREFIX];
                    else ch = PD_LEGEND[which][k];
                    if (ch < 32 || ch > 126) ch = '?';
                }
                const int nib = h & 1 ? ch & 15 : ch >> 4;
                c = nib < 10 ? '0' + nib : 'A' + nib - 10;
            } else {
                c = PD_TAB[O_TAIL + h - 2 * hexcap];
            }
        }
        if (c & 0x80) {
            const int n = c & 15, f = (c >> 4) & 7;
            if (n <= 8) {
                const int q = f == 0 ? v0 : f == 1 ? v1 : f == 2 ? v2 : f == 3 ? v3 : f == 4 ? v4 : f == 5 ? v5 : f == 6 ? v6 : v7;
                c = pd_num_char(q, n);
            } else if (n == 9) {
                c = '0' + (f == 0 ? a8 / 100 : f == 1 ? a8 / 10 % 10 : a8 % 10);
            } else if (n == 10) {
                const int cents = PD_CENTS[colour][f >> 1];
                c = '0' + (f & 1 ? cents % 10 : cents / 10);
            } else if (n == 11) {
                c = '0' + (f == 0 ? lw / 100 : f == 1 ? lw / 10 % 10 : lw % 10);
            } else {
                c = n == 12 ? op : pat;
            }
        }
        lds[start + b - c0] = (unsigned char)((on || c == '\n') ? c : ' ');
    }
}

// (the arguments are read from the call's table block, as k_plot_raster's; the rows' address comes as an argument of its
//  own, which makes the final stores global ones)
__global__ __launch_bounds__(PD_T) void k_pdf_content(const PdfArgs *__restrict__ args, unsigned char *__restrict__ out) {
    const PdfArgs &A = *args;
    __shared__ __attribute__((aligned(16))) unsigned char image[PD_CHUNK];
    const int t = threadIdx.x;
    const long long smp = blockIdx.y, c0 = (long long)blockIdx.x * PD_CHUNK, c1 = c0 + PD_CHUNK;
    // the bytes between the row's end and the next multiple of 16 are spaces; every other byte is a record's
    reinterpret_cast<uint4 *>(image)[t] = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
    wc_sync();
    for (int s = 0; s < A.n_sec; ++s) {
        const PdfSec sec = A.secs[s];
        const long long end = sec.start + (long long)sec.count * sec.width;
        if (sec.count <= 0 || end <= c0 || sec.start >= c1) continue;
        const long long r0 = c0 > sec.start ? (c0 - sec.start) / sec.width : 0;
        const long long r1 = c1 < end ? (c1 - 1 - sec.start) / sec.width : (long long)sec.count - 1;
        for (long long r = r0 + t; r <= r1; r += PD_T) pd_record(A, smp, sec, r, image, c0);
    }
    wc_sync();
    const long long at = c0 + 16ll * t;
    if (at < ((A.row_bytes + 15) & ~15ll))
        *reinterpret_cast<uint4 *>(out + smp * A.out_stride + at) = reinterpret_cast<const uint4 *>(image)[t];
}

// ---- the host's half ----------------------------------------------------------------------------------------------------
int title_cap_of(int name_cap) { return PD_TITLE_PREFIX + (name_cap > 1 ? name_cap - 1 : 0); }

// the section table of a page whose panel p has slots[p] list slots; returns the row's bytes
int64_t build_sections(const int64_t *chrom_sizes, const int32_t *panel_chrom, int n_panels, const int32_t *band_off,
                       const int32_t *slots, int name_cap, std::vector<PdfSec> *out) {
    int64_t at = 0;
    auto add = [&](int kind, int panel, int64_t count, int width) {
        if (out) out->push_back(PdfSec{(long long)at, kind, panel, (int)count, width});
        at += count * width;
    };
    for (int p = 0; p < n_panels; ++p) {
        const int64_t bins = chrom_sizes[panel_chrom[p] - 1], n = slots[p];
        add(K_HEAD, p, 1, PD_WIDTH[K_HEAD]);
        add(K_BAND, p, band_off ? band_off[p + 1] - band_off[p] : 0, PD_WIDTH[K_BAND]);
        add(K_LIST, p, n, PD_WIDTH[K_LIST]);
        add(K_GREY, p, 4, PD_WIDTH[K_GREY]);
        add(K_EDGE, p, n, PD_WIDTH[K_EDGE]);
        add(K_POLYHEAD, p, 1, PD_WIDTH[K_POLYHEAD]);
        add(K_VERTEX, p, bins, PD_WIDTH[K_VERTEX]);
        add(K_STROKE, p, 1, PD_WIDTH[K_STROKE]);
        add(K_LABEL, p, n, PD_WIDTH[K_LABEL]);
        add(K_FRAMEQ, p, 1, PD_WIDTH[K_FRAMEQ]);
        add(K_CHROM, p, 1, PD_WIDTH[K_CHROM]);
    }
    add(K_TITLE, 0, 1, PD_WIDTH[K_TITLE] + 2 * title_cap_of(name_cap));
    add(K_LEGEND, 0, 4, PD_WIDTH[K_LEGEND]);
    return at;
}

int check_page(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, int64_t row_stride,
               const int32_t *band_off, int name_cap) {
    int rc;
    if ((rc = wc::plot_check_page("pdf", chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, band_off))) return rc;
    WC_CHECK(name_cap >= 1 && name_cap <= 4096, WC_E_ARG, "pdf: names of %d bytes (1 .. 4096)", name_cap);
    return WC_OK;
}

// a call's page plan (plot_label.h) -- its tail is the section table, then the content kernel's arguments, sent once the
// lists' counts are known -- and what pdf_lists leaves for pdf_pages
struct Plan {
    wc::PagePlan page;
    int n_sec = 0, Wc = 0, Hc = 0;
    int64_t n_samples = 0, row_stride = 0, row_bytes = 0;
    double thr = 0.0;
    const double *z = nullptr;
    std::vector<int32_t> slots;
    std::vector<PdfSec> secs;
};

// the arguments and, for the worst case, what the deflate stage takes in one call: held before anything is touched
int pdf_check(const wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
              const double *calls, const int32_t *n_calls, int max_calls, double threshold, const int32_t *panel_chrom, int n_panels,
              int columns, const int32_t *band_off, const char *names, int name_cap, int width_cp, int height_cp, int64_t *bound_out) {
    WC_CHECK(ctx && n_samples >= 1 && max_calls >= 0 && (max_calls == 0 || (calls && n_calls)) && names && columns >= 1 &&
                 row_stride >= 0 && (results_z || row_stride == 0),
             WC_E_ARG, "pdf: unusable argument");
    WC_CHECK(threshold > 0.0 && threshold <= DBL_MAX, WC_E_ARG, "pdf: threshold_z %g is not a positive finite number", threshold);
    WC_CHECK(width_cp >= 1 && height_cp >= 1 && width_cp <= 1440000 && height_cp <= 1440000, WC_E_ARG,
             "pdf: a page of %d x %d centipoints (1 .. 1440000 each)", width_cp, height_cp);
    int rc;
    if ((rc = check_page(chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, band_off, name_cap))) return rc;
    const int64_t bound = wc_plot_pdf_row_bound(chrom_sizes, n_chrom, panel_chrom, n_panels, band_off, max_calls, name_cap);
    WC_CHECK(bound > 0, WC_E_LIMIT, "pdf: the page's content does not fit a row");
    const int64_t n_blk = (bound + wc_deflate_block_bytes() - 1) / wc_deflate_block_bytes();
    WC_CHECK(n_samples <= 65535 && n_blk <= INT_MAX / 2 && n_samples <= (int64_t)INT_MAX / n_blk, WC_E_LIMIT,
             "pdf: %lld pages of up to %lld bytes in one call; split the batch", (long long)n_samples, (long long)bound);
    *bound_out = bound;
    return WC_OK;
}

// tables, the display lists, and the read-back of their counts (the call's one synchronise); `bound` is pdf_check's
int pdf_lists(wc_ctx *ctx, hipStream_t stream, const double *results_z, int64_t row_stride, int64_t n_samples,
              const int64_t *chrom_sizes, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls, double threshold,
              double mineffect, const int32_t *panel_chrom, int n_panels, int columns, const double *bands, const int32_t *band_off,
              const char *names, int name_cap, int width_cp, int height_cp, int64_t bound, Plan &L, hipEvent_t *ev) {
    int rc;
    wc::PagePlan &P = L.page;
    L.n_sec = PD_PER_PANEL * n_panels + 2; L.Wc = width_cp; L.Hc = height_cp; L.n_samples = n_samples; L.row_stride = row_stride;
    L.thr = threshold; L.z = results_z;
    if ((rc = wc::page_plan(ctx, "pdf", chrom_sizes, n_chrom, panel_chrom, n_panels, row_stride, max_calls, columns, width_cp, height_cp,
                            bands, band_off, names, n_samples, name_cap, sizeof(PdfSec) * (size_t)L.n_sec + sizeof(PdfArgs), P)) ||
        (rc = ctx->pl_list.reserve((size_t)n_samples * n_panels * P.cap * PD_F * 8)) ||
        (rc = ctx->pl_counts.reserve((size_t)n_samples * (n_panels + 1) * 4)) || (rc = ctx->pl_status.reserve(8)) ||
        (rc = ctx->ensure_pinned((size_t)n_samples * n_panels * 4)) || (rc = wc::page_send(ctx, stream, 0, P.tail)))
        return rc;
    if (ev) WC_HIP(hipEventRecord(ev[0], stream));
    if ((rc = wc::plot_list_launch(ctx, stream, P, results_z, row_stride, n_samples, calls, n_calls, max_calls, threshold, mineffect, P.cap)))
        return rc;
    // the slot counts of the sections: per panel the largest list among the samples
    WC_HIP(hipMemcpyAsync(ctx->pinned, ctx->pl_counts.p, (size_t)n_samples * n_panels * 4, hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    const int *counts = (const int *)ctx->pinned;
    L.slots.assign(n_panels, 0);
    for (int64_t s = 0; s < n_samples; ++s)
        for (int p = 0; p < n_panels; ++p) {
            int n = counts[s * n_panels + p] - 1;
            n = n > P.cap - 1 ? P.cap - 1 : n;
            L.slots[p] = n > L.slots[p] ? n : L.slots[p];
        }
    L.row_bytes = build_sections(chrom_sizes, panel_chrom, n_panels, band_off, L.slots.data(), name_cap, &L.secs);
    WC_CHECK((int)L.secs.size() == L.n_sec && L.row_bytes <= bound, WC_E_INTERNAL, "pdf: %lld bytes of content, the bound is %lld",
             (long long)L.row_bytes, (long long)bound);
    if (ev) WC_HIP(hipEventRecord(ev[1], stream));
    return WC_OK;
}

// the content kernel, Adler-32 and deflate, enqueued
int pdf_pages(wc_ctx *ctx, hipStream_t stream, const Plan &L, unsigned char *content, int64_t content_stride, unsigned char *streams,
              int64_t out_stride, int64_t *out_len, uint32_t *adler, hipEvent_t *ev) {
    const wc::PagePlan &P = L.page;
    const int64_t padded = (L.row_bytes + 15) / 16 * 16;
    WC_CHECK(content_stride >= padded && content_stride % 16 == 0 && ((uintptr_t)content & 15) == 0, WC_E_ARG,
             "pdf: content rows %lld bytes apart (a multiple of 16, at least %lld, from an address that is one)", (long long)content_stride,
             (long long)padded);
    WC_CHECK(out_stride >= wc_deflate_bound(L.row_bytes), WC_E_ARG, "pdf: %lld bytes per stream, wc_deflate_bound(%lld) is %lld",
             (long long)out_stride, (long long)L.row_bytes, (long long)wc_deflate_bound(L.row_bytes));
    const size_t sec_bytes = sizeof(PdfSec) * L.secs.size();
    PdfArgs A;
    A.Wc = L.Wc; A.Hc = L.Hc; A.P = P.n_panels; A.cap = P.cap; A.has_cyto = P.has_cyto; A.name_cap = P.name_cap; A.n_sec = L.n_sec;
    A.title_cap = title_cap_of(P.name_cap); A.row_stride = L.row_stride; A.row_bytes = L.row_bytes; A.out_stride = content_stride;
    A.thr = L.thr; A.z = L.z;
    A.chrom_off = P.chrom_off; A.chrom_len = P.chrom_len; A.panel_chrom = P.panel_chrom; A.boxes = P.boxes; A.band_off = P.band_off;
    A.bands = P.bands; A.entries = ctx->pl_list.as<double>(); A.counts = ctx->pl_counts.as<int>(); A.names = P.names;
    A.secs = (const PdfSec *)P.tail_dev;
    memcpy(P.tail_host, L.secs.data(), sec_bytes);
    memcpy(P.tail_host + sec_bytes, &A, sizeof(PdfArgs));
    int rc;
    if ((rc = wc::page_send(ctx, stream, P.tail, P.bytes))) return rc;
    hipLaunchKernelGGL(k_pdf_content, dim3((unsigned)((padded + PD_CHUNK - 1) / PD_CHUNK), (unsigned)L.n_samples), dim3(PD_T), 0, stream,
                       (const PdfArgs *)(P.tail_dev + sec_bytes), content);
    WC_HIP(hipGetLastError());
    if (ev) WC_HIP(hipEventRecord(ev[2], stream));
    if ((rc = wc_adler32_rows_dev(ctx, stream, content, L.n_samples, L.row_bytes, content_stride, adler))) return rc;
    if (ev) WC_HIP(hipEventRecord(ev[3], stream));
    // the CRC-32 words of the deflate call are not needed; they go behind the lists' counts
    if ((rc = wc_deflate_rows_dev(ctx, stream, content, L.n_samples, L.row_bytes, content_stride, streams, out_stride, out_len,
                                  ctx->pl_counts.as<uint32_t>() + L.n_samples * P.n_panels)))
        return rc;
    if (ev) WC_HIP(hipEventRecord(ev[4], stream));
    return WC_OK;
}

void report(const Plan &L, int64_t *row_bytes_host, int64_t *offsets_host) {
    if (row_bytes_host) *row_bytes_host = L.row_bytes;
    if (offsets_host) {
        for (size_t i = 0; i < L.secs.size(); ++i) offsets_host[i] = L.secs[i].start;
        offsets_host[L.secs.size()] = L.row_bytes;
    }
}

void append(std::string &s, const char *fmt, ...) {
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    s += line;
}

// the file's objects 1 .. 7, everything before the content object: offsets[i] = where object i + 1 begins
std::string pdf_front(int Wc, int Hc, size_t *offsets) {
    std::string s = "%PDF-1.4\n%\xe2\xe3\xcf\xd3\n";
    offsets[0] = s.size();
    s += "1 0 obj\n<< /Type /Catalog /Pages 2 0 R >>\nendobj\n";
    offsets[1] = s.size();
    s += "2 0 obj\n<< /Type /Pages /Kids [3 0 R] /Count 1 >>\nendobj\n";
    offsets[2] = s.size();
    append(s, "3 0 obj\n<< /Type /Page /Parent 2 0 R /MediaBox [0 0 %9d.%02d %9d.%02d] /Contents 8 0 R\n", Wc / 100, Wc % 100, Hc / 100, Hc % 100);
    s += "/Resources << /Font << /F1 4 0 R >> /ExtGState 5 0 R /Pattern << /P1 6 0 R /P2 7 0 R >> >> >>\nendobj\n";
    offsets[3] = s.size();
    s += "4 0 obj\n<< /Type /Font /Subtype /Type1 /BaseFont /Courier >>\nendobj\n";
    offsets[4] = s.size();
    s += "5 0 obj\n<<\n";
    for (int a = 0; a < 256; ++a) {
        const int v = (a * 10000 + 127) / 255;          // alpha a / 255 to four decimals
        append(s, "/A%03d << /ca %d.%04d /CA %d.%04d >>\n", a, v / 10000, v % 10000, v / 10000, v % 10000);
    }
    s += ">>\nendobj\n";
    // the hatches '//' and '\\' as coloured tiling patterns: a black diagonal, 1 pt wide, every 6 pt
    const char *strokes[2] = {"0 0 0 RG 1 w -1 -1 m 7 7 l -4 2 m 4 10 l 2 -4 m 10 4 l S\n", "0 0 0 RG 1 w -1 7 m 7 -1 l -4 4 m 4 -4 l 2 10 m 10 2 l S\n"};
    for (int k = 0; k < 2; ++k) {
        offsets[5 + k] = s.size();
        append(s, "%d 0 obj\n<< /Type /Pattern /PatternType 1 /PaintType 1 /TilingType 1 /BBox [0 0 6 6] /XStep 6 /YStep 6 /Resources << >> "
                  "/Length %d >>\nstream\n",
               6 + k, (int)strlen(strokes[k]));
        s += strokes[k];
        s += "endstream\nendobj\n";
    }
    return s;
}

const char PD_CONTENT_HEAD[] = "8 0 obj\n<< /Filter /FlateDecode /Length %10lld >>\nstream\n";
const char PD_CONTENT_TAIL[] = "\nendstream\nendobj\n";

}  // namespace

extern "C" {

int64_t wc_plot_pdf_sections(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, const int32_t *band_off,
                             const int32_t *slots, int name_cap, int64_t *starts_out) {
    if (!slots || check_page(chrom_sizes, n_chrom, panel_chrom, n_panels, LLONG_MAX, band_off, name_cap)) return -1;
    double most = 0.0;                                       // held in floating point first: the sum below must not wrap
    for (int p = 0; p < n_panels; ++p) {
        if (slots[p] < 0) return -1;
        most += 22.0 * (double)chrom_sizes[panel_chrom[p] - 1] + 331.0 * slots[p] + 138.0 * (band_off ? band_off[p + 1] - band_off[p] : 0) + 1000.0;
    }
    if (most > 4e18) return -1;
    std::vector<PdfSec> secs;
    const int64_t bytes = build_sections(chrom_sizes, panel_chrom, n_panels, band_off, slots, name_cap, starts_out ? &secs : nullptr);
    if (starts_out) {
        for (size_t i = 0; i < secs.size(); ++i) starts_out[i] = secs[i].start;
        starts_out[secs.size()] = bytes;
    }
    return bytes;
}

int64_t wc_plot_pdf_row_bound(const int64_t *chrom_sizes, int n_chrom, const int32_t *panel_chrom, int n_panels, const int32_t *band_off,
                              int max_calls, int name_cap) {
    if (max_calls < 0 || check_page(chrom_sizes, n_chrom, panel_chrom, n_panels, LLONG_MAX, band_off, name_cap)) return -1;
    std::vector<int32_t> slots((size_t)n_panels);
    for (int p = 0; p < n_panels; ++p) {
        const int64_t n = (chrom_sizes[panel_chrom[p] - 1] + 1) / 2 + max_calls;      // alternating zeros: ceil(bins / 2) patches
        if (n > INT_MAX / 2) return -1;
        slots[p] = (int32_t)n;
    }
    return wc_plot_pdf_sections(chrom_sizes, n_chrom, panel_chrom, n_panels, band_off, slots.data(), name_cap, nullptr);
}

int wc_plot_pdf_batch_dev(wc_ctx *ctx, void *stream_, const double *results_z, int64_t row_stride, int64_t n_samples,
                          const int64_t *chrom_sizes_host, int n_chrom, const double *calls, const int32_t *n_calls, int max_calls,
                          double threshold, double mineffect, const int32_t *panel_chrom_host, int n_panels, int columns,
                          const double *bands_host, const int32_t *band_off_host, const char *names_host, int name_cap, int width_cp,
                          int height_cp, unsigned char *content, int64_t content_stride, unsigned char *streams, int64_t out_stride,
                          int64_t *out_len, uint32_t *adler, int64_t *row_bytes_host, int64_t *offsets_host, int32_t *status) {
    WC_CHECK(streams && out_len && adler && status && row_bytes_host, WC_E_ARG, "pdf: NULL output");
    hipStream_t stream = (hipStream_t)stream_;
    Plan L;
    int rc;
    int64_t bound = 0;
    if ((rc = pdf_check(ctx, results_z, row_stride, n_samples, chrom_sizes_host, n_chrom, calls, n_calls, max_calls, threshold,
                        panel_chrom_host, n_panels, columns, band_off_host, names_host, name_cap, width_cp, height_cp, &bound)) ||
        (rc = pdf_lists(ctx, stream, results_z, row_stride, n_samples, chrom_sizes_host, n_chrom, calls, n_calls, max_calls, threshold,
                        mineffect, panel_chrom_host, n_panels, columns, bands_host, band_off_host, names_host, name_cap, width_cp,
                        height_cp, bound, L, nullptr)))
        return rc;
    const int64_t padded = (L.row_bytes + 15) / 16 * 16;
    if (!content) {
        if ((rc = ctx->pl_img.reserve((size_t)n_samples * padded))) return rc;
        content = ctx->pl_img.as<unsigned char>();
        content_stride = padded;
    }
    if ((rc = pdf_pages(ctx, stream, L, content, content_stride, streams, out_stride, out_len, adler, nullptr))) return rc;
    WC_HIP(hipMemcpyAsync(status, ctx->pl_status.p, 4, hipMemcpyDeviceToDevice, stream));
    report(L, row_bytes_host, offsets_host);
    return WC_OK;
}

int wc_plot_pdf_batch(wc_ctx *ctx, const double *results_z, int64_t row_stride, int64_t n_samples, const int64_t *chrom_sizes, int n_chrom,
                      const double *calls, const int32_t *n_calls, int max_calls, double threshold, double mineffect,
                      const int32_t *panel_chrom, int n_panels, int columns, const double *bands, const int32_t *band_off, const char *names,
                      int name_cap, int width_cp, int height_cp, unsigned char *content_out, int64_t content_stride,
                      unsigned char *streams_out, int64_t out_stride, int64_t *out_len, uint32_t *adler_out, int64_t *row_bytes_out,
                      int64_t *offsets_out, double *times_ms) {
    WC_CHECK(streams_out && out_len && adler_out && row_bytes_out, WC_E_ARG, "pdf: NULL output");
    int rc;
    int64_t bound = 0;
    // (with the host's pointers standing in for the device's: only whether they are there is looked at)
    if ((rc = pdf_check(ctx, results_z, row_stride, n_samples, chrom_sizes, n_chrom, calls, n_calls, max_calls, threshold, panel_chrom,
                        n_panels, columns, band_off, names, name_cap, width_cp, height_cp, &bound)))
        return rc;
    WC_HIP(hipSetDevice(ctx->device));
    wc::HostBatch B;
    Plan L;
    if ((rc = B.stage(ctx, results_z, row_stride, n_samples, calls, n_calls, max_calls, times_ms != nullptr)) ||
        (rc = pdf_lists(ctx, nullptr, B.z, row_stride, n_samples, chrom_sizes, n_chrom, B.calls, B.n_calls, max_calls, threshold, mineffect,
                        panel_chrom, n_panels, columns, bands, band_off, names, name_cap, width_cp, height_cp, bound, L, B.ev)))
        return rc;
    // the device's rows and streams are sized by what this batch needs, the caller's by the bound it could know
    const int64_t padded = (L.row_bytes + 15) / 16 * 16, dev_stride = wc_deflate_bound(L.row_bytes);
    WC_CHECK(out_stride >= dev_stride && (!content_out || content_stride >= L.row_bytes), WC_E_ARG,
             "pdf: %lld bytes per stream and %lld per content row, %lld and %lld are needed", (long long)out_stride,
             (long long)content_stride, (long long)dev_stride, (long long)L.row_bytes);
    if ((rc = ctx->pl_img.reserve((size_t)n_samples * padded)) || (rc = ctx->tmp_b.reserve((size_t)n_samples * dev_stride)) ||
        (rc = pdf_pages(ctx, nullptr, L, ctx->pl_img.as<unsigned char>(), padded, ctx->tmp_b.as<unsigned char>(), dev_stride,
                        ctx->tmp_c.as<int64_t>(), ctx->tmp_d.as<uint32_t>(), B.ev)) ||
        (rc = B.collect(ctx, "pdf", n_samples, dev_stride, streams_out, out_stride, out_len, adler_out)))
        return rc;
    if (content_out && L.row_bytes > 0)
        WC_HIP(hipMemcpy2D(content_out, (size_t)content_stride, ctx->pl_img.p, (size_t)padded, (size_t)L.row_bytes, (size_t)n_samples,
                           hipMemcpyDeviceToHost));
    report(L, row_bytes_out, offsets_out);
    B.times(times_ms);      // [1] list and the counts' way back [2] content [3] Adler-32 [4] deflate
    return WC_OK;
}

int64_t wc_pdf_bytes(int64_t deflate_len) {
    if (deflate_len < 0) return -1;
    size_t offsets[7];
    const std::string front = pdf_front(100, 100, offsets);          // (its size does not depend on the page)
    char head[96];
    const int n = snprintf(head, sizeof head, PD_CONTENT_HEAD, 0ll);
    // header and objects 1 .. 7 | the content object | xref: a line, a count line, 9 entries | trailer
    const std::string trailer = "trailer\n<< /Size 9 /Root 1 0 R >>\nstartxref\n          \n%%EOF\n";
    return (int64_t)front.size() + n + 2 + deflate_len + 4 + (int64_t)strlen(PD_CONTENT_TAIL) + 5 + 4 + 9 * 20 + (int64_t)trailer.size();
}

int wc_pdf_assemble(int width_cp, int height_cp, const unsigned char *deflate, int64_t deflate_len, uint32_t adler, unsigned char *out,
                    int64_t cap, int64_t *out_len) {
    WC_CHECK(width_cp >= 1 && height_cp >= 1 && width_cp <= 1440000 && height_cp <= 1440000 && deflate && deflate_len >= 1 && out && out_len,
             WC_E_ARG, "pdf: unusable argument (a page of 1 .. 1440000 centipoints each way)");
    WC_CHECK(deflate_len <= 9999999990ll - 6, WC_E_LIMIT, "pdf: a stream of %lld bytes", (long long)deflate_len);
    WC_CHECK(cap >= wc_pdf_bytes(deflate_len), WC_E_ARG, "pdf: room for %lld bytes, wc_pdf_bytes(%lld) is %lld", (long long)cap,
             (long long)deflate_len, (long long)wc_pdf_bytes(deflate_len));
    size_t offsets[8];
    const std::string front = pdf_front(width_cp, height_cp, offsets);
    unsigned char *p = out;
    memcpy(p, front.data(), front.size());
    p += front.size();
    offsets[7] = (size_t)(p - out);
    p += snprintf((char *)p, 96, PD_CONTENT_HEAD, (long long)(deflate_len + 6));
    p[0] = 0x78;    // zlib header: deflate, 32 KiB window, fastest
    p[1] = 0x01;
    memcpy(p + 2, deflate, (size_t)deflate_len);
    p += 2 + deflate_len;
    wc::put32(p, adler);
    p += 4;
    memcpy(p, PD_CONTENT_TAIL, strlen(PD_CONTENT_TAIL));
    p += strlen(PD_CONTENT_TAIL);
    const long long xref = p - out;
    std::string tail = "xref\n0 9\n0000000000 65535 f \n";
    for (int i = 0; i < 8; ++i) append(tail, "%010lld 00000 n \n", (long long)offsets[i]);
    append(tail, "trailer\n<< /Size 9 /Root 1 0 R >>\nstartxref\n%-10lld\n%%%%EOF\n", xref);
    memcpy(p, tail.data(), tail.size());
    p += tail.size();
    *out_len = p - out;
    WC_CHECK(*out_len == wc_pdf_bytes(deflate_len), WC_E_INTERNAL, "pdf: %lld bytes written, wc_pdf_bytes says %lld", (long long)*out_len,
             (long long)wc_pdf_bytes(deflate_len));
    return WC_OK;
}

}  // extern "C"
