"""`plotpdf` restated in Python: the page's content stream and the file around it, made of the display
list of tests/plot_restated.py.  The kernel of csrc/pdf.hip and wc_pdf_assemble are held to this byte for byte.

The rules, in the order the code below applies them:
  units     centipoints (1 / 100 pt): the page is round(size * 7200) each way; boxes = plot_restated.layout of the page
  mapping   plot_restated's fx / fy with the box in centipoints (float64, the same operation order), the same y range
  rnd       q = floor(v + 0.5) of v limited to +-1e9, then limited to +-9 999 999; NaN gives -9 999 999
  flip      PDF's y axis points up: y = Hc - qy; a rectangle's width and height are differences of the integer corners
  number    a field of 9 bytes, right-aligned: an optional '-', the whole points, '.', two digits (-99999.99 .. 999999.99)
  colour    the palette's two decimals; alpha a8 = rnd(255 * alpha) limited to 0 .. 255, the graphics state /A<a8>
  records   of a fixed width per kind, each line ending in '\\n'; one that draws nothing is spaces (the line ends stay)
              head      49  q <x y w h> re W n                          the box as clip path
              band     138  a fill line (73) and '/Pattern cs /P<n> scn <x y w h> re f' (65; spaces without a hatch)
              fill      73  ' /A<a8> gs <r g b> rg <x y w h> re f'      patches, then calls, in the list's order
              line      81  ' /A255 gs <width> w <r g b> RG <x y> m <x y> l S'   the four grey lines: 1, 0.75, 0.75, 0.75 pt
              edge     162  two lines of 0.5 pt, the call's colour, over the box's height
              polyhead  57  ' /A255 gs 0.50 w 0.00 0.45 0.70 RG <x y> m'  (the box's lower left corner: a path always begins)
              vertex    22  '<x y> m' for the first bin and after a bin that is not finite, else '<x y> l'
              stroke     2  'S'
              text      96  ' /A255 gs 0.00 0.00 0.00 rg BT /F1 8 Tf <x y> Td <hex, 12 characters padded with 20> Tj ET'
              frame     82  ' /A255 gs 1.00 w 0.00 0.00 0.00 RG <x y w h> re S', half a point inside the box, then 'Q'
              title     73 + 2 cap  as text, 12 pt; cap = 45 + the longest name of the call
              legend   179  a fill line (a swatch of 9.6 x 6 pt) and a text of 17 characters
  sections  per panel: head, bands (the table's rows), fills (slots), lines (4), edges (slots), polyhead, vertices (bins),
            stroke, labels (slots), frame, the chromosome number (text); then the title and the legend (4).  slots = the
            longest list among the samples of the call, less the range entry; a slot that holds no call has blank edges
            and a blank label
  text      Courier, 600 / 1000 wide: a label of n characters at 8 pt starts n * 240 left of rnd(fx(centre)); its baseline
            lies 700 below the far edge (z > 0, 'top') or 300 above it ('bottom'); the chromosome number ends 400 left of
            the box, baseline 250 below the box's middle; the title is centred at Wc >> 1, baseline Hc - Hc * 7 // 100;
            characters outside ASCII 32 .. 126 are '?'
  legend    entry `which` at x = ((Wc - 2 * 10080) >> 1) + (which >> 1) * 10080, baseline 2400 - (which & 1) * 1600: the swatch
            960 x 600 from there, the text 1440 to the right
"""
import struct
import zlib

import numpy as np

import plot_restated as pr

LIM = 9999999
CENTS = [[int(round(v * 100)) for v in c] for c in pr._REF_PALETTE]
LABEL_CAP, LEGEND_CAP = 12, 17


def page_size(size):
    return int(np.floor(size[0] * 7200 + 0.5)), int(np.floor(size[1] * 7200 + 0.5))


def rnd(v):
    v = float(v)
    if v != v:
        return -LIM
    v = min(max(v, -1e9), 1e9)
    return int(min(max(np.floor(np.float64(v) + 0.5), -LIM), LIM))


def alpha8(alpha):
    return min(255, max(0, rnd(255.0 * np.float64(alpha))))


def num(q):
    q = min(max(int(q), -LIM), 99999999)
    text = ('-' if q < 0 else '') + '%d.%02d' % (abs(q) // 100, abs(q) % 100)
    assert len(text) <= 9
    return text.rjust(9)


def field(v):
    """The 9 bytes a coordinate v (float64, centipoints) is written as."""
    return num(rnd(v))


def _rgb(colour):
    return ' '.join('0.%02d' % c for c in CENTS[colour])


def _blank(text, on):
    return text if on else ''.join(c if c == '\n' else ' ' for c in text)


def _fill(a8, colour, x, y, w, h, on=True):
    return _blank(' /A%03d gs %s rg %s %s %s %s re f\n' % (a8, _rgb(colour), num(x), num(y), num(w), num(h)), on)


def _line(cents, colour, x0, y0, x1, y1, on=True):
    return _blank(' /A255 gs %d.%02d w %s RG %s %s m %s %s l S\n' % (cents // 100, cents % 100, _rgb(colour), num(x0), num(y0), num(x1), num(y1)), on)


def _text(size, x, y, text, cap, on=True):
    text = ''.join(c if 32 <= ord(c) <= 126 else '?' for c in text)
    assert len(text) <= cap
    hexed = ''.join('%02X' % ord(c) for c in text.ljust(cap))
    return _blank(' /A255 gs 0.00 0.00 0.00 rg BT /F1 %d Tf %s %s Td <%s> Tj ET\n' % (size, num(x), num(y), hexed), on)


def slots_of(lists_per_sample):
    """Per panel the longest list among the samples, less the range entry."""
    return [max(len(lists[p]) - 1 for lists in lists_per_sample) for p in range(len(lists_per_sample[0]))]


def content(lists, zscores, chromosomes, columns, thr, name, Wc, Hc, slots=None, bands=None, band_off=None, name_cap=None,
            sections=None):
    """The content stream (bytes) of one sample.  slots / name_cap default to what this sample alone needs; `sections`, a
    list, receives (kind, panel, start) of every section and at last ('end', 0, bytes)."""
    thr = np.float64(thr)
    n = len(chromosomes)
    boxes = pr.layout(Wc, Hc, (n + columns - 1) // columns, columns, n)
    slots = slots_of([lists]) if slots is None else slots
    cyto_y = -thr - thr / 2.0
    out = []
    size = [0]

    def section(kind, p, text):
        if sections is not None:
            sections.append((kind, p, size[0]))
        out.append(text)
        size[0] += len(text)

    with np.errstate(all='ignore'):
        for p, chrom in enumerate(chromosomes):
            bx0, by0, bx1, by1 = (int(v) for v in boxes[p])
            ent = np.asarray(lists[p], dtype=np.float64).reshape(-1, 9)
            z = np.asarray(zscores[chrom - 1], dtype=np.float64)
            bw, bh, xmax = np.float64(bx1 - bx0), np.float64(by1 - by0), np.float64(max(len(z), 1))
            base = cyto_y if band_off is not None else -thr
            lo, hi = (ent[0, 4] if ent[0, 4] < base else base), (ent[0, 5] if ent[0, 5] > thr else thr)
            pad = (hi - lo) * 0.05
            ylo, yhi = lo - pad, hi + pad
            yspan = yhi - ylo

            def qx(x):
                return rnd((np.float64(x) * bw) / xmax + bx0)

            def qy(y):
                return rnd(((yhi - np.float64(y)) * bh) / yspan + by0)

            section('head', p, 'q %s %s %s %s re W n\n' % (num(bx0), num(Hc - by1), num(bx1 - bx0), num(by1 - by0)))
            rows = bands[band_off[p]:band_off[p + 1]] if band_off is not None else []
            text = ''
            for x0, x1, alpha, hatch in rows:
                top, bot, a, b = qy(-thr), qy(cyto_y), qx(x0), qx(x1)
                text += _fill(alpha8(alpha), 0, a, Hc - bot, b - a, bot - top, hatch >= 0)
                text += _blank('/Pattern cs /P%d scn %s %s %s %s re f\n' % (2 if hatch == 2 else 1, num(a), num(Hc - bot), num(b - a),
                                                                             num(bot - top)), hatch in (1, 2))
            section('band', p, text)
            text = ''
            for k in range(slots[p]):
                if k + 1 < len(ent):
                    e = ent[k + 1]
                    top, bot = (e[4], e[5]) if e[4] > e[5] else (e[5], e[4])
                    qt, qb, a, b = qy(top), qy(bot), qx(e[2]), qx(e[3])
                    text += _fill(alpha8(e[7]), int(e[6]), a, Hc - qb, b - a, qb - qt)
                else:
                    text += _fill(0, 0, 0, 0, 0, 0, False)
            section('fill', p, text)
            text = ''
            for k, y in enumerate((np.float64(0.0), thr, -thr, cyto_y)):
                py = Hc - qy(y)
                text += _line(100 if k == 0 else 75, pr.GREY, bx0, py, bx1, py, k < 3 or len(rows) > 0)
            section('line', p, text)
            text = ''
            for k in range(slots[p]):
                if k + 1 < len(ent) and ent[k + 1, 0] == pr.CALL:
                    e = ent[k + 1]
                    for x in (qx(e[2]), qx(e[3])):
                        text += _line(50, int(e[6]), x, Hc - by1, x, Hc - by0)
                else:
                    text += 2 * _line(0, 0, 0, 0, 0, 0, False)
            section('edge', p, text)
            section('polyhead', p, ' /A255 gs 0.50 w %s RG %s %s m\n' % (_rgb(5), num(bx0), num(Hc - by1)))
            text = ''
            for i, v in enumerate(z):
                if np.isfinite(v):
                    text += '%s %s %s\n' % (num(qx(i)), num(Hc - qy(v)), 'm' if i == 0 or not np.isfinite(z[i - 1]) else 'l')
                else:
                    text += ' ' * 21 + '\n'
            section('vertex', p, text)
            section('stroke', p, 'S\n')
            text = ''
            for k in range(slots[p]):
                if k + 1 < len(ent) and ent[k + 1, 0] == pr.CALL:
                    e = ent[k + 1]
                    label = pr.label_text(e[8])
                    edge = Hc - qy(e[5])
                    text += _text(8, qx(e[2] + (e[3] - e[2]) / 2.0) - len(label) * 240, edge - 700 if e[8] > 0 else edge + 300, label,
                                  LABEL_CAP)
                else:
                    text += _text(8, 0, 0, '', LABEL_CAP, False)
            section('label', p, text)
            section('frame', p, ' /A255 gs 1.00 w %s RG %s %s %s %s re S\nQ\n' % (_rgb(0), num(bx0 + 50), num(Hc - by1 + 50), num(bx1 - bx0 - 100),
                                                                        num(by1 - by0 - 100)))
            number = str(int(chrom))
            section('chrom', p, _text(8, bx0 - 400 - len(number) * 480, Hc - ((by0 + by1) >> 1) - 250, number, LABEL_CAP))
    raw = name.encode('latin1', 'replace')
    title = pr.TITLE + raw.decode('latin1')
    cap = len(pr.TITLE) + (len(raw) if name_cap is None else name_cap - 1)
    section('title', 0, _text(12, (Wc >> 1) - len(title) * 360, Hc - (Hc * 7) // 100, title, cap))
    text = ''
    for which, (label, colour) in enumerate(pr.LEGEND):
        ex, by = ((Wc - 2 * 10080) >> 1) + (which >> 1) * 10080, 2400 - (which & 1) * 1600
        text += _fill(255, colour, ex, by, 960, 600) + _text(8, ex + 1440, by, label, LEGEND_CAP)
    section('legend', 0, text)
    if sections is not None:
        sections.append(('end', 0, size[0]))
    return ''.join(out).encode('latin1')


# ------------------------------------------------------------------------------------ the file ----
PATTERNS = (b"0 0 0 RG 1 w -1 -1 m 7 7 l -4 2 m 4 10 l 2 -4 m 10 4 l S\n", b"0 0 0 RG 1 w -1 7 m 7 -1 l -4 4 m 4 -4 l 2 10 m 10 2 l S\n")


def assemble(Wc, Hc, deflate, adler):
    """The PDF file around one raw deflate stream of a content whose Adler-32 is `adler`."""
    objects = [b"<< /Type /Catalog /Pages 2 0 R >>\n",
               b"<< /Type /Pages /Kids [3 0 R] /Count 1 >>\n",
               ("<< /Type /Page /Parent 2 0 R /MediaBox [0 0 %9d.%02d %9d.%02d] /Contents 8 0 R\n/Resources << /Font << /F1 4 0 R >> "
                "/ExtGState 5 0 R /Pattern << /P1 6 0 R /P2 7 0 R >> >> >>\n" % (Wc // 100, Wc % 100, Hc // 100, Hc % 100)).encode(),
               b"<< /Type /Font /Subtype /Type1 /BaseFont /Courier >>\n",
               b"<<\n" + b"".join(("/A%03d << /ca %d.%04d /CA %d.%04d >>\n" % ((a,) + 2 * divmod((a * 10000 + 127) // 255, 10000))).encode()
                                  for a in range(256)) + b">>\n"]
    for stroke in PATTERNS:
        objects.append(("<< /Type /Pattern /PatternType 1 /PaintType 1 /TilingType 1 /BBox [0 0 6 6] /XStep 6 /YStep 6 /Resources << >> "
                        "/Length %d >>\nstream\n" % len(stroke)).encode() + stroke + b"endstream\n")
    data = b"\x78\x01" + bytes(deflate) + struct.pack(">I", adler & 0xffffffff)
    objects.append(("<< /Filter /FlateDecode /Length %10d >>\nstream\n" % len(data)).encode() + data + b"\nendstream\n")
    out = b"%PDF-1.4\n%\xe2\xe3\xcf\xd3\n"
    offsets = []
    for i, body in enumerate(objects):
        offsets.append(len(out))
        out += ("%d 0 obj\n" % (i + 1)).encode() + body + b"endobj\n"
    xref = len(out)
    out += b"xref\n0 9\n0000000000 65535 f \n" + b"".join(("%010d 00000 n \n" % o).encode() for o in offsets)
    out += ("trailer\n<< /Size 9 /Root 1 0 R >>\nstartxref\n%-10d\n%%%%EOF\n" % xref).encode()
    return out


def deflate_raw(data, level=6):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    return comp.compress(data) + comp.flush()


# ------------------------------------------------------------------------------------ the sweep ----
def sweep():
    """One-panel pages over 0 .. 33 bins and 0 .. 3 calls whose zero stretches change from page to page (none, single
    zeros one bin apart, zeros at both ends), so that the slot counts, and with them the section starts, take every
    residue modulo 16: dicts of zscores (one chromosome), calls, threshold, name."""
    out = []
    for bins in range(34):
        for n_calls in range(4):
            rng = np.random.RandomState(1000 + 4 * bins + n_calls)
            z = np.round(rng.standard_normal(bins) * 2.0, 2)
            z[z == 0] = 0.5
            kind = (bins + n_calls) % 3
            if kind == 0:
                z[::2] = 0.0
            elif kind == 2:
                z[:1] = 0.0
                z[max(0, bins - 2):] = 0.0
            calls = [(1, 2 * k, min(2 * k + 3, max(bins - 1, 0)), (-1) ** k * (5.5 + k), 0.04 * (k + 1) * (-1) ** k) for k in range(n_calls)]
            out.append(dict(zscores=[z], calls=np.array(calls, dtype=np.float64).reshape(-1, 5), threshold=5.0,
                            name="b%d_c%d" % (bins, n_calls)))
    return out
