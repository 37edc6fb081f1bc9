"""`plotpdf` without a GPU: the tests' own PDF reader (tests/pdf_reader.py) proven on a file matplotlib's PDF backend
writes; the restated content stream (tests/pdf_restated.py), read back through that reader and mapped to data coordinates,
against what the reference's plotLines drew (tests/golden/plot_primitives.npz); the number field; the file's structure,
wc_pdf_assemble against the restated file; the section table (wc_plot_pdf_sections) and the residues its starts take on
the sweep the GPU test runs; the command line."""
import io
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pdf_reader as rd  # noqa: E402
import pdf_restated as pd  # noqa: E402
import plot_cases  # noqa: E402
import plot_restated as pr  # noqa: E402

CASES = plot_cases.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "plot_primitives.npz"))


@pytest.fixture(scope="module")
def cyto_table(tmp_path_factory):
    path = tmp_path_factory.mktemp("cyto") / "cytoBand.txt"
    path.write_text(plot_cases.CYTO_TEXT)
    return pr.load_cytobands(str(path))


# ---- (a) the reader, on an independent writer -------------------------------------------------------------------------
def test_the_reader_opens_what_matplotlibs_pdf_backend_writes():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(4, 3))
    ax = fig.add_subplot(111)
    ax.plot([0, 1, 2], [1, 3, 2])
    ax.add_patch(plt.Rectangle((0.5, 1.5), 1, 1))
    buf = io.BytesIO()
    fig.savefig(buf, format="pdf")
    plt.close(fig)
    doc = rd.Document(buf.getvalue())
    page, content = doc.page()
    assert [float(v) for v in page["MediaBox"]] == [0, 0, 288, 216]
    assert len(content) > 500                                          # (inflated: the file holds it compressed)
    value, raw = doc.obj(page["Contents"].num)
    assert value["Filter"] == "FlateDecode" and isinstance(value["Length"], rd.Ref) and zlib.decompress(raw) == content
    ops = [op for _, op in rd.tokenize(content)]
    assert any(ops[i:i + 4] == ["m", "l", "l", "S"] for i in range(len(ops))), ops          # the three-point line
    # the interpreter takes this build's operators only: matplotlib's stream has others
    with pytest.raises(ValueError):
        rd.interpret(content)


# ---- (b) the restated stream against the reference's primitives ------------------------------------------------------
def _page(case, cyto_table, size=(4.0, 3.0)):
    Wc, Hc = pd.page_size(size)
    chroms = case['chromosomes']
    lists = pr.display_list(case['zscores'], case['calls'], case['threshold'], chroms, case['mineffect'])
    bands = offs = None
    if case['cyto']:
        bands, offs = pr.band_rows(cyto_table, chroms, case['binsize'])
    content = pd.content(lists, case['zscores'], chroms, case['columns'], case['threshold'], case['sample'], Wc, Hc, bands=bands,
                         band_off=offs)
    return Wc, Hc, lists, bands, offs, content


@pytest.mark.parametrize("case", CASES, ids=[c['name'] for c in CASES])
def test_restated_stream_read_back_equals_the_reference_primitives(case, golden, cyto_table):
    g = {k.split("__", 1)[1]: golden[k] for k in golden.files if k.startswith(case['name'] + "__")}
    Wc, Hc, lists, bands, offs, content = _page(case, cyto_table)
    thr = np.float64(case['threshold'])
    chroms = case['chromosomes']
    prims = rd.interpret(content)
    boxes = pr.layout(Wc, Hc, (len(chroms) + case['columns'] - 1) // case['columns'], case['columns'], len(chroms))
    cyto_y = -thr - thr / 2.0
    rgb100 = lambda rgb: tuple(int(round(float(v) * 100)) for v in rgb)
    at_y = 0
    for p, chrom in enumerate(chroms):
        bx0, by0, bx1, by1 = (int(v) for v in boxes[p])
        clip = (bx0, Hc - by1, bx1 - bx0, by1 - by0)
        mine = [q for q in prims if q['clip'] == clip]
        ent = lists[p]
        z = case['zscores'][chrom - 1]
        bins = max(len(z), 1)
        base = cyto_y if offs is not None else -thr
        lo, hi = min(ent[0, 4], base), max(ent[0, 5], thr)
        pad = (hi - lo) * 0.05
        ylo, yhi = lo - pad, hi + pad
        bw, bh = float(bx1 - bx0), float(by1 - by0)
        # Half a centipoint: q = floor(v + 0.5) moves a coordinate by at most that, which is 0.5 * bins / box_w in x and
        # 0.5 * (yhi - ylo) / box_h in y (derived, not measured).  The comparison is made on the page, where that bound
        # is the number 0.5 itself; EPS covers the rounding of the mapping's own four float64 operations on values below
        # 1e7 (a few 1e-9) and of the golden's x + w, nothing else.
        EPS = 1e-6
        near_x = lambda qx, x: abs(qx - ((x * bw) / bins + bx0)) <= 0.5 + EPS
        near_y = lambda py, y: abs((Hc - py) - (((yhi - y) * bh) / (yhi - ylo) + by0)) <= 0.5 + EPS
        # rectangles, in the reference's order: bands, uncallable stretches, calls
        fills = [q for q in mine if q['kind'] == 'fill' and q['pattern'] is None]
        got = g['rect'][g['rect'][:, 0] == p]
        assert len(fills) == len(got)
        for q, r in zip(fills, got):
            x, y, w, h = q['rect']
            rx0, rx1 = r[1], r[1] + r[3]
            ry0, ry1 = sorted((r[2], r[2] + r[4]))
            assert near_x(x, rx0) and near_x(x + w, rx1) and near_y(y, ry0) and near_y(y + h, ry1), (q, r)
            assert q['rgb'] == rgb100(r[5:8]) and q['a8'] == pr.alpha8(r[8]) == pd.alpha8(r[8]), (q, r)
        hatched = [q for q in mine if q['kind'] == 'fill' and q['pattern'] is not None]
        want = [r for r in got if r[9] > 0]
        assert [q['pattern'] for q in hatched] == ["P%d" % r[9] for r in want]
        for q, r in zip(hatched, want):
            assert near_x(q['rect'][0], r[1]) and q['a8'] == pd.alpha8(r[8])
        # lines: the grey ones (0, +-thr and -1.5 thr exactly where the golden has it), then two edges per call
        strokes = [q for q in mine if q['kind'] == 'stroke']
        lines = [q for q in strokes if len(q['path']) == 2 and q['path'][0][0] == 'm']
        horizontal = [q for q in lines if q['path'][0][2] == q['path'][1][2]]
        vertical = [q for q in lines if q['path'][0][1] == q['path'][1][1]]
        assert len(horizontal) + len(vertical) == len(lines)
        want_h = g['hline'][g['hline'][:, 0] == p]
        levels = sorted(set(want_h[:, 1].tolist()), key=lambda y: [0.0, float(thr), float(-thr), float(cyto_y)].index(y))
        assert len(horizontal) == len(levels)
        assert (float(cyto_y) in levels) == (offs is not None and offs[p + 1] > offs[p])
        for q, y in zip(horizontal, levels):
            (_, x0, y0), (_, x1, y1) = q['path']
            assert (x0, x1) == (bx0, bx1) and near_y(y0, y), (q, y)
            assert q['rgb'] == rgb100(want_h[0][2:]) and q['width'] == (100 if y == 0 else 75) and q['a8'] == 255
        want_v = g['vline'][g['vline'][:, 0] == p]
        assert len(vertical) == len(want_v)
        for q, r in zip(vertical, want_v):
            (_, x0, y0), (_, x1, y1) = q['path']
            assert near_x(x0, r[1]) and (y0, y1) == (Hc - by1, Hc - by0), (q, r)
            assert q['rgb'] == rgb100(r[2:]) and q['width'] == 50
        # the polyline: one vertex per finite bin, a new subpath exactly behind the bins that are not finite
        poly = [q for q in strokes if q not in lines and q['path'][0][0] != 're']
        assert [q['path'] for q in strokes if q['path'][0][0] == 're'] == [[('re', bx0 + 50, Hc - by1 + 50, bx1 - bx0 - 100, by1 - by0 - 100)]]
        finite = np.isfinite(z)
        runs = [i for i in range(len(z)) if finite[i] and (i == 0 or not finite[i - 1])]
        drawn = [i for i in runs if i + 1 < len(z) and finite[i + 1]]
        if not drawn:
            assert not poly
        else:
            assert len(poly) == 1 and poly[0]['rgb'] == rgb100(g['plot_len'][p][2:]) and poly[0]['width'] == 50
            path = poly[0]['path'][1:]                                  # (behind the head's own moveto)
            assert len(path) == int(finite.sum())
            for seg, i in zip(path, np.nonzero(finite)[0]):
                assert seg[0] == ('m' if i in runs else 'l'), (i, seg)
                assert near_x(seg[1], float(i)) and near_y(seg[2], g['plot_y'][at_y + i]), (i, seg)
        at_y += len(z)
        # labels
        sel = g['text_at'][:, 0] == p
        texts = [q for q in mine if q['kind'] == 'text']
        assert [q['text'].rstrip() for q in texts] == list(g['text_s'][sel])
        for q, (_, tx, ty), va in zip(texts, g['text_at'][sel], g['text_va'][sel]):
            n = len(q['text'].rstrip())
            assert near_x(q['x'] + n * 240, tx) and near_y(q['y'] + (700 if va == 'top' else -300), ty), (q, tx, ty)
            assert q['size'] == 8 and q['rgb'] == (0, 0, 0)
    outside = [q for q in prims if q['clip'] is None and q['kind'] == 'text']
    assert [q['text'].rstrip() for q in outside[:len(chroms)]] == [str(c) for c in chroms]
    assert outside[len(chroms)]['text'].rstrip() == str(g['title']) and outside[len(chroms)]['size'] == 12
    assert [q['text'].rstrip() for q in outside[len(chroms) + 1:]] == list(g['legend'])
    swatches = [q for q in prims if q['clip'] is None and q['kind'] == 'fill']
    assert [q['rgb'] for q in swatches] == [rgb100(c) for c in g['legend_rgb']]


# ---- (c) the number field ------------------------------------------------------------------------------------------
def test_the_number_field():
    want = {0: "     0.00", 5: "     0.05", -5: "    -0.05", 99: "     0.99", -99: "    -0.99", 100: "     1.00", -100: "    -1.00",
            9999999: " 99999.99", -9999999: "-99999.99", 123456: "  1234.56"}
    for q, text in want.items():
        assert pd.num(q) == text == pd.field(float(q)) and len(text) == 9
    # beyond the limit: clamped
    for v in (1e7, 1e300, np.inf, 9999999.5):
        assert pd.field(v) == " 99999.99"
    for v in (-1e7, -1e300, -np.inf, np.nan):
        assert pd.field(v) == "-99999.99"
    # ties x.5 go up (floor(v + 0.5))
    # (the float64 below 0.5 too: v + 0.5 rounds to 1.0 before the floor, as in the rasteriser)
    assert [pd.rnd(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 0.4999999)] == [1, 2, 3, 0, -1, -2, 1, 0]
    assert [pd.field(v) for v in (12.5, -12.5, 99.5, -100.5)] == ["     0.13", "    -0.12", "     1.00", "    -1.00"]
    # a sum of a flipped coordinate may pass the limit upwards: the field holds six digits in front of the point
    assert pd.num(9999999 + 84240) == "100842.39" and pd.num(10 ** 9) == "999999.99"


# ---- (d) the file ---------------------------------------------------------------------------------------------------
def test_the_file_is_what_the_restatement_writes_and_its_structure_holds(cyto_table):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    case = [c for c in CASES if c['name'] == 'cyto'][0]
    Wc, Hc, lists, bands, offs, content = _page(case, cyto_table, (11.7, 8.3))
    assert (Wc, Hc) == (84240, 59760) == wt.pdfPageSize((11.7, 8.3))
    stream = pd.deflate_raw(content)
    adler = zlib.adler32(content)
    data = wt.pdfAssemble(Wc, Hc, stream, adler)
    assert data == pd.assemble(Wc, Hc, stream, adler)
    assert len(data) == _lib.load().wc_pdf_bytes(len(stream))
    assert len(wt.pdfAssemble(100, 100, stream, adler)) == len(data)           # whatever the page
    assert data.startswith(b"%PDF-1.4\n%") and data[10] >= 128 and data.endswith(b"%%EOF\n")
    for word in (b"/Info", b"/ID", b"/CreationDate", b"/Producer"):
        assert word not in data
    doc = rd.Document(data)
    assert data[doc.startxref:doc.startxref + 5] == b"xref\n" and sorted(doc.offsets) == list(range(1, 9))
    for num, at in doc.offsets.items():
        assert data[at:].startswith(b"%d 0 obj\n" % num)                        # every xref offset lands on its object
        doc.obj(num)
    page, got = doc.page()
    assert [float(v) for v in page["MediaBox"]] == [0, 0, 842.4, 597.6]
    value, raw = doc.obj(8)
    assert value["Length"] == len(raw) == len(stream) + 6 and raw[:2] == b"\x78\x01"
    assert zlib.decompress(raw) == content == got
    assert doc.get(page["Resources"]["Font"]["F1"])["BaseFont"] == "Courier"
    states = doc.get(page["Resources"]["ExtGState"])
    assert len(states) == 256 and all(round(float(states["A%03d" % a]["ca"]) * 255) == a for a in range(256))
    for name in ("P1", "P2"):
        pattern, strokes = doc.obj(page["Resources"]["Pattern"][name].num)
        assert pattern["PatternType"] == 1 and pattern["Length"] == len(strokes)
        rd.interpret(strokes)
    # through the file's own resources the drawing is the one read from the bare stream
    assert rd.interpret(got, doc, page["Resources"]) == rd.interpret(content)
    # one Adler byte changed: zlib refuses the content
    bad = rd.Document(wt.pdfAssemble(Wc, Hc, stream, adler ^ 0x100))
    with pytest.raises(zlib.error):
        bad.page()
    with pytest.raises(Exception):
        wt.pdfAssemble(0, Hc, stream, adler)


# ---- (e) the section table ------------------------------------------------------------------------------------------
def test_section_starts_on_the_sweep_take_every_residue_modulo_16():
    from wisecondor_amd import wisetools as wt
    Wc, Hc = pd.page_size((4.0, 3.0))
    seen = {}
    for job in pd.sweep():
        lists = pr.display_list(job['zscores'], job['calls'], job['threshold'], [1], 0)
        secs = []
        content = pd.content(lists, job['zscores'], [1], 1, job['threshold'], job['name'], Wc, Hc, sections=secs)
        starts = wt.pdfSections([len(job['zscores'][0])], [1], None, pd.slots_of([lists]), len(job['name']) + 1)
        assert [s[2] for s in secs] == list(starts) and starts[-1] == len(content)
        for kind, _, start in secs:
            seen.setdefault(kind, set()).add(start % 16)
    # the first three sections of a one-panel page begin at fixed offsets (0, 49 and, without a cytoband table, 49 again):
    # nothing of the sample stands in front of them.  Every other section, and the row's end, is asserted
    fixed = {'head': {0}, 'band': {1}, 'fill': {1}}
    assert set(seen) == {'head', 'band', 'fill', 'line', 'edge', 'polyhead', 'vertex', 'stroke', 'label', 'frame', 'chrom', 'title',
                         'legend', 'end'}
    for kind, residues in seen.items():
        assert residues == fixed.get(kind, set(range(16))), (kind, sorted(residues))


def test_row_bound_is_the_worst_case_of_the_section_table():
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    sizes = np.array([40, 43, 3, 0], dtype=np.int64)
    panels = np.array([2, 1, 4, 3], dtype=np.int32)
    band_off = np.array([0, 2, 2, 3, 3], dtype=np.int32)
    lib = _lib.load()
    bound = lib.wc_plot_pdf_row_bound(_lib.ptr(sizes), 4, _lib.ptr(panels), 4, _lib.ptr(band_off), 5, 9)
    slots = [(sizes[c - 1] + 1) // 2 + 5 for c in panels]
    starts = wt.pdfSections(sizes, panels, band_off, slots, 9)
    assert bound == starts[-1]
    widths = np.diff(starts)
    assert widths[1] == 2 * 138 and widths[2] == slots[0] * 73 and widths[6] == 43 * 22 and widths[-2] == 73 + 2 * (45 + 8)
    assert lib.wc_plot_pdf_row_bound(_lib.ptr(sizes), 4, _lib.ptr(np.array([5], dtype=np.int32)), 1, None, 5, 9) == -1


# ---- (f) the command line -------------------------------------------------------------------------------------------
def test_plotpdf_options_defaults_and_output_names(tmp_path, capsys):
    from wisecondor_amd import ingest
    from wisecondor_amd import wisecondor as cli
    args = cli.buildParser().parse_args(["plotpdf", "a_test.npz", "b_test.npz", "out"])
    assert args.func is cli.toolPlotPdf and args.infiles == ["a_test.npz", "b_test.npz"] and args.outdir == "out"
    assert args.cytofile is None and args.chromosomes == list(range(1, 23)) and args.columns == 2
    assert args.size == [11.7, 8.3] and args.mineffect == 1.5 and args.batch == 64 and args.io == 8
    assert not hasattr(args, "dpi") and not hasattr(args, "filetype")
    args = cli.buildParser().parse_args(["plotpdf", "a", "out", "-chromosomes", "1,5,22", "-columns", "3", "-size", "6", "4", "-mineffect", "0",
                                         "-cytofile", "c.txt", "-batch", "7", "-io", "2"])
    assert (args.chromosomes, args.columns, args.size, args.mineffect, args.cytofile, args.batch, args.io) == \
        ([1, 5, 22], 3, [6.0, 4.0], 0.0, "c.txt", 7, 2)
    with pytest.raises(SystemExit):
        cli.buildParser().parse_args(["plotpdf", "a", "out", "-dpi", "200"])
    capsys.readouterr()
    assert ingest.plot_output_names(["d/a_test.npz", "b.x"], "o", "pdf", "plotpdf") == [os.path.join("o", "a_test_z.pdf"),
                                                                                       os.path.join("o", "b.x_z.pdf")]
    outdir = tmp_path / "out"
    with pytest.raises(SystemExit) as stop:
        cli.main(["plotpdf", str(tmp_path / "a" / "s_test.npz"), str(tmp_path / "b" / "s_test.npz"), str(outdir)])
    assert stop.value.code == 2 and "ERROR: plotpdf:" in capsys.readouterr().out and not outdir.exists()
    # a chromosome the files do not hold: found when the first file is read, before anything is drawn
    args = cli.buildParser().parse_args(["test", "in.npz", "out.npz", "ref.npz"])
    result = dict(results_z=[np.zeros(3), np.ones(2)], results_r=[np.zeros(3), np.ones(2)], results_cwz=np.zeros(2),
                  results_calls=np.zeros((0, 5)), asdef=0.01)
    path = str(tmp_path / "two_test.npz")
    cli.writeTestOutput(path, args, 250000.0, result, 5.8)
    with pytest.raises(SystemExit) as stop:
        cli.main(["plotpdf", path, str(outdir), "-chromosomes", "1,2,3"])
    said = capsys.readouterr().out
    assert stop.value.code == 2 and "ERROR: plotpdf: -chromosomes names 3" in said and not os.listdir(str(outdir))
