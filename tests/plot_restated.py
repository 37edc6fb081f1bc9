"""`plotbatch` restated in numpy: what is drawn (the display list of upstream plotLines, wisetools.py:527-662) and how
(the rasteriser's rules, DESIGN.md "plotbatch").  The kernels of csrc/plot.hip are held to this bit for bit.

The rules, in the order the code below applies them:
  image     RGB, 8 bits, PNG scanline layout: per row a filter byte 0, then 3 W bytes
  s         max(1, round(dpi / 100)) = max(1, (2 dpi + 100) // 200): the width of every line, the factor of every glyph
  boxes     wc_plot_layout: margins left W * 125 // 1000, right W // 10, top H * 12 // 100, bottom H * 11 // 100; cells
            of (grid // columns) x (grid // rows) pixels; a panel leaves cell_w * 12 // 100 on the left of its cell and
            cell_h * 15 // 100 below
  mapping   float64, in this order: fx(x) = (x * box_w) / max(bins, 1) + box_x0; fy(y) = ((yhi - y) * box_h) / (yhi - ylo) +
            box_y0 with lo = min(min finite z, -thr - thr / 2 with a cytoband file, else -thr), hi = max(max finite z, thr),
            pad = (hi - lo) * 0.05, ylo = lo - pad, yhi = hi + pad
  rnd / flr floor(v + 0.5) / floor(v) of v limited to +-1e9; NaN lies nowhere
  blend     c = (c * (255 - a) + colour * a + 127) // 255, a = rnd(255 * alpha) limited to 0 .. 255
  rectangle covers the pixels whose centre (ix + 0.5, iy + 0.5) lies in [fx(x0), fx(x1)) x [fy(y top), fy(y bottom))
  order     white; cytobands (hatch '//' : a second blend where (ix + iy) % (6 s) < s, '\\': where (ix - iy) mod (6 s) < s);
            uncallable patches; call rectangles; grey lines at 0, thr, -thr (and -1.5 thr where the panel's chromosome has
            bands in the table, drawn or not): rows rnd(fy(y)) - s // 2 + [0, s); call edge lines: columns rnd(fx(x)) - s // 2 + [0, s); the polyline; labels; the frame
            (s pixels inside the box); outside the boxes the chromosome numbers; the title; the legend
  polyline  for every pair of neighbouring finite bins (i, z[i]) - (i + 1, z[i + 1]) and every pixel column [ix, ix + 1) with
            fx(i) < ix + 1 and fx(i + 1) > ix: y at the clipped ends t = max(fx(i), ix), min(fx(i + 1), ix + 1) is
            ya + (yb - ya) * ((t - xa) / (xb - xa)); the column is filled from flr(min) - (s - 1) // 2 to flr(max) + s // 2
  text      8 x 14 glyphs of csrc/plot_font.h times s; characters outside ASCII 32..126 draw '?'; a call's label is
            "{:.1f}".format(z), '?' when abs(z) >= 1e9 or z is not finite, centred on rnd(fx(centre)) and s pixels below
            (z > 0) or above the rectangle's far edge; labels and everything above are clipped to the box
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE, BAND, ZERO, CALL = 0, 1, 2, 3
_REF_PALETTE = [(0, 0, 0), (0.90, 0.60, 0), (0.35, 0.70, 0.90), (0, 0.60, 0.50), (0.95, 0.90, 0.25), (0, 0.45, 0.70),
                (0.80, 0.40, 0), (0.80, 0.60, 0.70), (0.7, 0.7, 0.7)]          # wisetools.py:531-541, then the line grey
PALETTE = np.array([[int(v * 255 + 0.5) for v in c] for c in _REF_PALETTE], dtype=np.int64)
GREY = 8
FONT_W, FONT_H = 8, 14
TITLE = "Z-score versus chromosomal position - Sample "
LEGEND = (("Called region", 1), ("Uncallable region", 7), ("Z-score per bin", 5), ("Z-score threshold", GREY))


def font_table():
    """The 95 glyphs of csrc/plot_font.h as a uint8 array [95, 14]."""
    text = open(os.path.join(ROOT, "wisecondor_amd", "csrc", "plot_font.h")).read()
    body = text[text.index("WC_FONT_ROWS["):]
    rows = [[int(v, 16) for v in re.findall(r"0x[0-9a-f]{2}", line.split("//")[0])] for line in body.splitlines()[1:]]
    rows = [r for r in rows if r]
    return np.array(rows, dtype=np.uint8)


# ------------------------------------------------------------------------------------ what is drawn ----
def load_cytobands(path):
    """chromosome name -> [(start, end, stain)], every chromosome of the table (the reference drops the last one)."""
    table = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if parts:
                table.setdefault(parts[0][3:], []).append((parts[1], parts[2], parts[4]))
    return table


def band_rows(table, chromosomes, binsize):
    """bands float64 [n, 4] rows (x0, x1, alpha, hatch; hatch -1: a band of the table that gets no rectangle) and offsets
    int32 [panels + 1].  A panel with any row has the -1.5 thr line: the reference draws it once per band of the table."""
    rows, offs = [], [0]
    for chrom in chromosomes:
        for start, end, stain in table.get(str(chrom), []):
            x0, x1 = float(start) / binsize, float(end) / binsize
            if stain[1:4] == 'pos':
                rows.append((x0, x1, float(stain[4:]) / 100 * 0.5, 0.0))
            elif stain == 'acen':
                rows.append((x0, x1, 1 * 0.5, 1.0))
            elif stain == 'gvar':
                rows.append((x0, x1, 0.75 * 0.5, 2.0))
            else:
                rows.append((x0, x1, 0.0, -1.0))
        offs.append(len(rows))
    return np.array(rows, dtype=np.float64).reshape(-1, 4), np.array(offs, dtype=np.int32)


def display_list(zscores, calls, thr, chromosomes, mineffect=0):
    """Per panel a float64 array [n, 9]: (kind, panel, x0, x1, y0, y1, colour, alpha, value), as wc_plot_list gives it."""
    thr = float(thr)
    calls = np.asarray(calls, dtype=np.float64).reshape(-1, 5)
    out = []
    for p, chrom in enumerate(chromosomes):
        z = np.asarray(zscores[chrom - 1], dtype=np.float64)
        fin = z[np.isfinite(z)]
        zeros = [i for i, v in enumerate(z) if v == 0]
        stretches = []
        if zeros:
            start = zeros[0]
            for i, val in enumerate(zeros[:-1]):
                if zeros[i + 1] - val > 1:
                    stretches.append((start, val))
                    start = zeros[i + 1]
            stretches.append((start, zeros[-1]))
        rows = [(RANGE, p, 0.0, float(len(z)), fin.min() if len(fin) else np.inf, fin.max() if len(fin) else -np.inf, 0, 0.0,
                 float(len(stretches)))]
        for a, b in stretches:
            rows.append((ZERO, p, a - 0.5, b + 0.5, -thr, thr, 7, 0.5, 0.0))
        for mark in calls:
            if mark[0] == chrom and abs(mark[4]) * 100 >= mineffect:
                colour = 3 if abs(mark[4]) >= 0.2 else 1
                rows.append((CALL, p, mark[1] - 0.5, mark[2] + 0.5, 0.0, -thr if mark[3] < 0 else thr, colour,
                             min(1, abs(mark[4]) * 10), mark[3]))
        out.append(np.array(rows, dtype=np.float64).reshape(-1, 9))
    return out


def label_text(z):
    return "{:.1f}".format(z) if abs(z) < 1e9 else "?"


# ------------------------------------------------------------------------------------ how it is drawn ----
def image_size(size, dpi):
    return int(np.floor(size[0] * dpi + 0.5)), int(np.floor(size[1] * dpi + 0.5))


def line_scale(dpi):
    return max(1, (2 * int(dpi) + 100) // 200)


def layout(W, H, rows, columns, n_panels):
    gx0, gx1, gy0, gy1 = W * 125 // 1000, W - W // 10, H * 12 // 100, H - H * 11 // 100
    cw, ch = (gx1 - gx0) // columns, (gy1 - gy0) // rows
    boxes = []
    for p in range(n_panels):
        r, c = divmod(p, columns)
        cx, cy = gx0 + c * cw, gy0 + r * ch
        boxes.append((cx + cw * 12 // 100, cy, cx + cw, cy + ch - ch * 15 // 100))
    return np.array(boxes, dtype=np.int32).reshape(-1, 4)


def _lim(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(v < -1e9, -1e9, np.where(v > 1e9, 1e9, v))


def rnd(v):
    v = _lim(v)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), -2000000000, np.floor(v + 0.5)).astype(np.int64)


def flr(v):
    v = _lim(v)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), -2000000000, np.floor(v)).astype(np.int64)


def alpha8(alpha):
    return int(min(255, max(0, rnd(255.0 * np.float64(alpha)))))


def _blend(img, mask, colour, a):
    img[mask] = (img[mask] * (255 - a) + PALETTE[colour] * a + 127) // 255


def _text(img, allowed, font, text, tx, ty, s):
    H, W = allowed.shape
    for k, ch in enumerate(text):
        code = ord(ch) if 32 <= ord(ch) <= 126 else ord('?')
        for gy in range(FONT_H):
            bits = int(font[code - 32, gy])
            for gx in range(FONT_W):
                if (bits >> (7 - gx)) & 1:
                    x0, y0 = tx + (k * FONT_W + gx) * s, ty + gy * s
                    xa, xb, ya, yb = max(x0, 0), min(x0 + s, W), max(y0, 0), min(y0 + s, H)
                    if xa < xb and ya < yb:
                        m = allowed[ya:yb, xa:xb]
                        img[ya:yb, xa:xb][m] = 0


def raster(lists, zscores, chromosomes, columns, thr, name, W, H, dpi, bands=None, band_off=None, font=None):
    """The scanline image, uint8 [H, 1 + 3 W], of one sample: `lists` as display_list (or wc_plot_list) gives them,
    bands / band_off as band_rows gives them (None: no cytoband file)."""
    font = font_table() if font is None else font
    thr = np.float64(thr)
    s = line_scale(dpi)
    n = len(chromosomes)
    boxes = layout(W, H, (n + columns - 1) // columns, columns, n)
    img = np.full((H, W, 3), 255, dtype=np.int64)
    inbox = np.zeros((H, W), dtype=bool)
    cyto_y = -thr - thr / 2.0
    with np.errstate(all='ignore'):
        for p, chrom in enumerate(chromosomes):
            bx0, by0, bx1, by1 = (int(v) for v in boxes[p])
            if bx1 <= bx0 or by1 <= by0:
                continue
            inbox[by0:by1, bx0:bx1] = True
            sub = img[by0:by1, bx0:bx1]
            ent = np.asarray(lists[p], dtype=np.float64).reshape(-1, 9)
            z = np.asarray(zscores[chrom - 1], dtype=np.float64)
            ixs, iys = np.arange(bx0, bx1), np.arange(by0, by1)
            cx, cy = ixs + 0.5, iys + 0.5
            bw, bh, xmax = np.float64(bx1 - bx0), np.float64(by1 - by0), np.float64(max(len(z), 1))
            nz = int(ent[0, 8])
            base = cyto_y if band_off is not None else -thr
            lo, hi = (ent[0, 4] if ent[0, 4] < base else base), (ent[0, 5] if ent[0, 5] > thr else thr)
            pad = (hi - lo) * 0.05
            ylo, yhi = lo - pad, hi + pad
            yspan = yhi - ylo

            def fx(x):
                return (x * bw) / xmax + bx0

            def fy(y):
                return ((yhi - y) * bh) / yspan + by0

            def rect(x0, x1, ya, yb):
                top, bot = (ya, yb) if ya > yb else (yb, ya)
                return np.outer((fy(top) <= cy) & (cy < fy(bot)), (fx(x0) <= cx) & (cx < fx(x1)))

            has_bands = band_off is not None and band_off[p + 1] > band_off[p]
            if has_bands:
                for x0, x1, alpha, hatch in bands[band_off[p]:band_off[p + 1]]:
                    if hatch < 0:
                        continue
                    m = rect(x0, x1, -thr, cyto_y)
                    a = alpha8(alpha)
                    _blend(sub, m, 0, a)
                    if hatch == 1:
                        _blend(sub, m & (np.add.outer(iys, ixs) % (6 * s) < s), 0, a)
                    elif hatch == 2:
                        _blend(sub, m & (np.mod(np.subtract.outer(-iys, -ixs), 6 * s) < s), 0, a)
            for e in ent[1:]:
                _blend(sub, rect(e[2], e[3], e[4], e[5]), int(e[6]), alpha8(e[7]))
            for y in [np.float64(0.0), thr, -thr] + ([cyto_y] if has_bands else []):
                r = int(rnd(fy(y))) - s // 2
                _blend(sub, np.outer((iys >= r) & (iys < r + s), np.ones(len(ixs), bool)), GREY, 255)
            for e in ent[1 + nz:]:
                for x in (e[2], e[3]):
                    c = int(rnd(fx(x))) - s // 2
                    _blend(sub, np.outer(np.ones(len(iys), bool), (ixs >= c) & (ixs < c + s)), int(e[6]), 255)
            span_lo = np.full(len(ixs), np.iinfo(np.int64).max)
            span_hi = np.full(len(ixs), np.iinfo(np.int64).min)
            xl, xr = ixs.astype(np.float64), ixs + 1.0
            for i in range(len(z) - 1):
                if not (np.isfinite(z[i]) and np.isfinite(z[i + 1])):
                    continue
                xa, xb = fx(np.float64(i)), fx(np.float64(i + 1))
                m = (xa < xr) & (xb > xl)
                if not m.any():
                    continue
                t0, t1, dx = np.maximum(xa, xl), np.minimum(xb, xr), xb - xa
                ya, yb = fy(z[i]), fy(z[i + 1])
                y0, y1 = ya + (yb - ya) * ((t0 - xa) / dx), ya + (yb - ya) * ((t1 - xa) / dx)
                m &= ~(np.isnan(y0) | np.isnan(y1))
                span_lo = np.where(m, np.minimum(span_lo, flr(np.minimum(y0, y1))), span_lo)
                span_hi = np.where(m, np.maximum(span_hi, flr(np.maximum(y0, y1))), span_hi)
            have = span_lo <= span_hi
            span_lo = np.where(have, span_lo - (s - 1) // 2, span_lo)
            span_hi = np.where(have, span_hi + s // 2, span_hi)
            _blend(sub, (iys[:, None] >= span_lo[None, :]) & (iys[:, None] <= span_hi[None, :]), 5, 255)
            clip = np.zeros((H, W), dtype=bool)
            clip[by0:by1, bx0:bx1] = True
            for e in ent[1 + nz:]:
                text = label_text(e[8])
                wpx = len(text) * FONT_W * s
                tx = int(rnd(fx(e[2] + (e[3] - e[2]) / 2.0))) - (wpx >> 1)
                edge = int(rnd(fy(e[5])))
                _text(img, clip, font, text, tx, edge + s if e[8] > 0 else edge - s - FONT_H * s, s)
            frame = np.zeros((by1 - by0, bx1 - bx0), dtype=bool)
            frame[:s, :] = frame[-s:, :] = True
            frame[:, :s] = frame[:, -s:] = True
            _blend(sub, frame, 0, 255)
    outside = ~inbox
    for p, chrom in enumerate(chromosomes):
        bx0, by0, bx1, by1 = (int(v) for v in boxes[p])
        if bx1 > bx0 and by1 > by0:
            text = str(int(chrom))
            _text(img, outside, font, text, bx0 - 4 * s - len(text) * FONT_W * s, by0 + ((by1 - by0 - FONT_H * s) >> 1), s)
    everywhere = np.ones((H, W), dtype=bool)
    title = TITLE + name
    _text(img, everywhere, font, title, (W - len(title) * FONT_W * s) >> 1, (H * 7) // 100 - FONT_H * s, s)
    ew, eh = 21 * FONT_W * s, 16 * s
    lx, ly = (W - 2 * ew) >> 1, H - 34 * s
    for which, (text, colour) in enumerate(LEGEND):
        ex, ey = lx + (which // 2) * ew, ly + (which % 2) * eh
        xa, xb, ya, yb = max(ex, 0), min(ex + 2 * FONT_W * s, W), max(ey + 3 * s, 0), min(ey + 11 * s, H)
        if xa < xb and ya < yb:
            img[ya:yb, xa:xb] = PALETTE[colour]
        # the entry's cell bounds its text (21 characters wide: nothing here is longer)
        _text(img, everywhere, font, text, ex + 3 * FONT_W * s, ey, s)
    scan = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    scan[:, 1:] = img.reshape(H, 3 * W).astype(np.uint8)
    return scan


def png_chunks(data):
    """[(type, payload)] of a PNG byte string; raises on a bad signature or chunk CRC."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload) & 0xffffffff
        out.append((kind, payload))
        at += 12 + n
    return out
