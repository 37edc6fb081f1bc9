"""`plotbatch` without a GPU: the restated display list (tests/plot_restated.py) against what the reference's plotLines
drew for every case of tests/plot_cases.py (tests/golden/plot_primitives.npz, recorded by tools/make_plot_golden.py), as
exact float64; the restated rasteriser's pixels where the rules name them; the glyph table; the host half of the PNG
path (wc_plot_layout, wc_png_assemble); the command line; the listing of csrc/plot.hip."""
import io
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _rgb8(rgb):
    return [int(v * 255 + 0.5) for v in rgb]


def test_the_cases_cover_what_they_should():
    lengths, kinds = set(), set()
    for shift in range(7):
        for c, z in enumerate(plot_cases.zscores(shift)):
            lengths.add(len(z))
    assert lengths == {0, 1, 2, 3, 40, 43}
    grids = {(len(c['chromosomes']), c['columns']) for c in CASES}
    assert {(1, 1), (1, 2), (2, 1), (2, 3), (5, 1), (5, 2), (5, 3), (22, 2), (22, 3)} <= grids
    assert any(len(c['chromosomes']) % c['columns'] for c in CASES)                 # a last row that is not full
    assert any(np.asarray(c['calls']).shape == (0,) for c in CASES)                 # upstream's empty call list
    z = plot_cases.zscores(0)
    assert any(np.signbit(v[v == 0]).any() for v in z) and any(np.isnan(v).any() for v in z)
    assert any(np.isposinf(v).any() for v in z) and any(np.isneginf(v).any() for v in z)


@pytest.mark.parametrize("case", CASES, ids=[c['name'] for c in CASES])
def test_restated_list_equals_the_reference_primitives(case, golden, cyto_table):
    g = {k.split("__", 1)[1]: golden[k] for k in golden.files if k.startswith(case['name'] + "__")}
    thr = np.float64(case['threshold'])
    chroms = case['chromosomes']
    lists = pr.display_list(case['zscores'], case['calls'], thr, chroms, case['mineffect'])
    bands = offs = None
    if case['cyto']:
        bands, offs = pr.band_rows(cyto_table, chroms, case['binsize'])
    rows = int(np.ceil(len(chroms) / float(case['columns'])))
    assert _eq(g['grid'], [(p, rows, case['columns']) for p in range(len(chroms))])
    assert str(g['title']) == pr.TITLE + case['sample']
    assert list(g['legend']) == [t for t, _ in pr.LEGEND]
    assert [_rgb8(c) for c in g['legend_rgb']] == [list(pr.PALETTE[c]) for _, c in pr.LEGEND]
    at = 0
    for p, chrom in enumerate(chroms):
        ent = lists[p]
        z = case['zscores'][chrom - 1]
        assert _eq(g['xlim'][p], (p, ent[0, 2], ent[0, 3])) and ent[0, 3] == len(z)
        assert _eq(g['ylabel'][p], (p, chrom))
        assert _eq(g['plot_len'][p][:2], (p, len(z))) and _rgb8(g['plot_len'][p][2:]) == list(pr.PALETTE[5])
        assert _eq(g['plot_y'][at:at + len(z)], z)
        at += len(z)
        fin = z[np.isfinite(z)]
        assert _eq(ent[0, 4:6], (fin.min(), fin.max()) if len(fin) else (np.inf, -np.inf))
        # grey lines: 0 and +-thr, and -1.5 thr once per band of the table (whatever its stain): the rasteriser draws it
        # where the panel has rows in the band table it is given
        has_line = bands is not None and offs[p + 1] > offs[p]
        got = g['hline'][g['hline'][:, 0] == p]
        assert all(_rgb8(r[2:]) == list(pr.PALETTE[pr.GREY]) for r in got)
        want = [0.0, thr, -thr] + ([-thr - thr / 2] if has_line else [])
        assert sorted(set(got[:, 1].tolist())) == sorted(want)
        # rectangles, in the reference's order: bands, uncallable stretches, calls
        want = []
        if bands is not None:
            for x0, x1, alpha, hatch in bands[offs[p]:offs[p + 1]]:
                if hatch < 0:
                    continue
                want.append((p, x0, -thr - thr / 2, x1 - x0, thr / 2, 0, 0, 0, alpha, hatch))
        for e in ent[1:]:
            want.append((p, e[2], e[4] if e[0] == pr.ZERO else 0.0, e[3] - e[2], thr * 2 if e[0] == pr.ZERO else e[5])
                        + tuple(pr.PALETTE[int(e[6])]) + (e[7], 0))
        got = g['rect'][g['rect'][:, 0] == p]
        assert len(got) == len(want)
        for r, w in zip(got, want):
            assert _eq(r[:5], w[:5]) and _rgb8(r[5:8]) == list(w[5:8]) and _eq(r[8:], w[8:]), (r, w)
        calls = ent[ent[:, 0] == pr.CALL]
        got = g['vline'][g['vline'][:, 0] == p]
        assert _eq(got[:, 1], calls[:, 2:4].reshape(-1))
        assert [_rgb8(r[2:]) for r in got] == [list(pr.PALETTE[int(c)]) for c in np.repeat(calls[:, 6], 2)]
        sel = g['text_at'][:, 0] == p
        assert _eq(g['text_at'][sel][:, 1], calls[:, 2] + (calls[:, 3] - calls[:, 2]) / 2.0)
        assert _eq(g['text_at'][sel][:, 2], calls[:, 5])
        assert list(g['text_s'][sel]) == [pr.label_text(v) for v in calls[:, 8]]
        assert list(g['text_va'][sel]) == ['top' if v > 0 else 'bottom' for v in calls[:, 8]]
    assert at == len(g['plot_y'])


def test_a_chromosome_absent_from_the_table_has_no_bands(cyto_table):
    case = plot_cases.build_only_cases()[0]
    bands, offs = pr.band_rows(cyto_table, case['chromosomes'], case['binsize'])
    per = dict(zip(case['chromosomes'], np.diff(offs)))
    assert per[2] == 0 and per[9] == 1 and per[1] == 6 and per[3] == 2      # 9 is the table's last: kept here
    drawn = [int((bands[offs[i]:offs[i + 1], 3] >= 0).sum()) for i in range(len(per))]
    assert drawn == [4, 0, 1, 1]


def _hand_made(W, H, dpi=100):
    """One panel of 8 bins: a call rectangle over bins 2..4 (alpha 0.5, orange), a zero stretch at bin 6."""
    thr = np.float64(4.0)
    z = [np.array([1.0, 2.0, 6.0, 5.0, 3.0, -1.0, 0.0, -2.0])]
    calls = np.array([[1, 2, 4, 5.5, 0.05]])
    lists = pr.display_list(z, calls, thr, [1], 0)
    return thr, z, lists, pr.raster(lists, z, [1], 1, thr, "x", W, H, dpi)


@pytest.mark.parametrize("W,H", [(20, 10), (100, 75), (400, 300)])
def test_restated_image_has_the_pixels_the_rules_name(W, H):
    thr, z, lists, scan = _hand_made(W, H)
    assert scan.shape == (H, 1 + 3 * W) and scan.dtype == np.uint8 and not scan[:, 0].any()
    img = scan[:, 1:].reshape(H, W, 3).astype(np.int64)
    bx0, by0, bx1, by1 = (int(v) for v in pr.layout(W, H, 1, 1, 1)[0])
    assert 0 <= bx0 < bx1 <= W and 0 <= by0 < by1 <= H
    bw, bh = np.float64(bx1 - bx0), np.float64(by1 - by0)
    lo, hi = -thr, np.float64(6.0)
    pad = (hi - lo) * 0.05
    ylo, yhi = lo - pad, hi + pad
    fx = lambda x: (x * bw) / np.float64(8) + bx0
    fy = lambda y: ((yhi - y) * bh) / (yhi - ylo) + by0
    xs, ys = np.arange(bx0, bx1) + 0.5, np.arange(by0, by1) + 0.5
    # the call rectangle [1.5, 4.5) x (0, thr] and the uncallable patch [5.5, 6.5) x (-thr, thr]: half-open in both
    # directions, by pixel centres.  Every pixel of the box that nothing opaque was drawn over (lines, polyline, label,
    # frame) has the stated blend inside them, a = round(255 * 0.5) = 128 over white, and is white outside them.
    call = np.outer((fy(thr) <= ys) & (ys < fy(0.0)), (fx(1.5) <= xs) & (xs < fx(4.5)))
    patch = np.outer((fy(thr) <= ys) & (ys < fy(-thr)), (fx(5.5) <= xs) & (xs < fx(6.5)))
    assert call.any() and patch.any() and not (call & patch).any()
    white = np.array([255, 255, 255])
    orange, purple = ((white * (255 - 128) + pr.PALETTE[c] * 128 + 127) // 255 for c in (1, 7))
    box = img[by0:by1, bx0:bx1]
    opaque = np.zeros(call.shape, dtype=bool)
    for colour in (pr.PALETTE[5], pr.PALETTE[pr.GREY], pr.PALETTE[0], pr.PALETTE[1]):
        opaque |= (box == colour).all(axis=2)
    for mask, colour in ((call, orange), (patch, purple), (~call & ~patch, white)):
        seen = mask & ~opaque
        assert seen.any(), "nothing of this region is left to see at %d x %d" % (W, H)
        assert (box[seen] == colour).all()
    # the right end of the rectangle is where the half-open rule says
    last = np.nonzero(call.any(axis=0))[0][-1] + bx0
    assert last + 0.5 < fx(4.5) <= last + 1.5
    assert (img[by0:by1, bx0] == 0).all()         # the frame
    if bx1 - bx0 < 12 or by1 - by0 < 12:          # the smallest box: the label covers the polyline's peak, the legend the top
        return
    # a polyline column spans the min - max of what crosses it: the column of bin 2's peak reaches up to fy(6)
    peak_col = int(np.floor(fx(2.0)))
    blue = pr.PALETTE[5]
    blue_rows = np.nonzero((img[by0:by1, peak_col] == blue).all(axis=1))[0] + by0
    assert blue_rows.min() == int(np.floor(fy(6.0)))
    seg_lo = min(fy(2.0) + (fy(6.0) - fy(2.0)) * ((peak_col - fx(1.0)) / (fx(2.0) - fx(1.0))), fy(6.0))
    assert blue_rows.min() == int(np.floor(seg_lo))
    # the frame
    assert (img[by0, bx0:bx1] == 0).all() and (img[by0:by1, bx1 - 1] == 0).all()


def test_a_panel_with_undrawn_bands_only_still_has_the_line_below(cyto_table):
    """Chromosome 4 of the table has one gneg band: no rectangle, but the reference draws the -1.5 thr line for it."""
    case = [c for c in CASES if c['name'] == 'cyto'][0]
    chroms, thr = case['chromosomes'], np.float64(case['threshold'])
    p = chroms.index(4)
    W, H = 400, 300
    lists = pr.display_list(case['zscores'], np.array([]), thr, chroms, 0)
    images = {}
    for name, table in (("with", cyto_table), ("without", {k: v for k, v in cyto_table.items() if k != '4'})):
        bands, offs = pr.band_rows(table, chroms, case['binsize'])
        assert offs[p + 1] - offs[p] == (1 if name == "with" else 0)
        images[name] = pr.raster(lists, case['zscores'], chroms, 2, thr, "x", W, H, 100, bands, offs)[:, 1:].reshape(H, W, 3)
    bx0, by0, bx1, by1 = (int(v) for v in pr.layout(W, H, 2, 2, 4)[p])
    ent = lists[p][0]
    cyto_y = -thr - thr / 2
    lo, hi = min(ent[4], cyto_y), max(ent[5], thr)
    pad = (hi - lo) * 0.05
    row = int(np.floor(((hi + pad - cyto_y) * np.float64(by1 - by0)) / ((hi + pad) - (lo - pad)) + by0 + 0.5))
    assert by0 < row < by1 - 1
    inner = slice(bx0 + 1, bx1 - 1)
    assert (images["with"][row, inner] == pr.PALETTE[pr.GREY]).all()
    assert (images["without"][row, inner] == 255).all()
    differ = np.nonzero((images["with"] != images["without"]).any(axis=(1, 2)))[0]
    assert list(differ) == [row]                                      # nothing else: a gneg band has no rectangle


def test_line_width_and_scale_follow_dpi():
    assert [pr.line_scale(d) for d in (1, 50, 100, 149, 150, 200, 250)] == [1, 1, 1, 1, 2, 2, 3]
    assert pr.image_size((11.7, 8.3), 100) == (1170, 830) and pr.image_size((4.0, 3.0), 50) == (200, 150)


def test_glyph_table_has_95_glyphs_and_only_the_space_is_empty():
    font = pr.font_table()
    assert font.shape == (95, 14)
    empty = [i for i in range(95) if not font[i].any()]
    assert empty == [0]
    assert len({font[i].tobytes() for i in range(95)}) == 95
    # (tools/make_plot_font.py --check compares the header with a fresh rendering; that depends on the FreeType at hand)
    header = open(os.path.join(ROOT, "wisecondor_amd", "csrc", "plot_font.h")).read()
    assert "#define WC_FONT_W 8" in header and "#define WC_FONT_H 14" in header and "#define WC_FONT_N 95" in header


def test_layout_matches_the_library(lib_plot):
    from wisecondor_amd import wisetools as wt
    for W, H, rows, cols, n in [(1170, 830, 11, 2, 22), (20, 10, 1, 1, 1), (400, 300, 2, 3, 5), (100, 75, 8, 3, 22), (585, 415, 5, 1, 5)]:
        assert np.array_equal(wt.plotLayout(W, H, rows, cols, n), pr.layout(W, H, rows, cols, n))
    with pytest.raises(Exception):
        wt.plotLayout(100, 100, 1, 2, 3)


@pytest.fixture(scope="module")
def lib_plot():
    from wisecondor_amd import _lib
    return _lib.load()


def test_png_assemble_with_zlibs_own_stream(lib_plot):
    from PIL import Image
    from wisecondor_amd import wisetools as wt
    thr, z, lists, scan = _hand_made(100, 75)
    raw = scan.tobytes()
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = comp.compress(raw) + comp.flush()
    adler = zlib.adler32(raw)
    png = wt.pngAssemble(100, 75, stream, adler)
    assert len(png) == lib_plot.wc_png_bytes(len(stream)) == len(stream) + 63
    kinds = [k for k, _ in pr.png_chunks(png)]
    assert kinds == [b"IHDR", b"IDAT", b"IEND"]
    idat = pr.png_chunks(png)[1][1]
    assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == raw and struct.unpack(">I", idat[-4:])[0] == adler
    im = Image.open(io.BytesIO(png))
    assert im.size == (100, 75) and im.mode == "RGB"
    assert np.array_equal(np.asarray(im), scan[:, 1:].reshape(75, 100, 3))
    # one Adler byte changed (the chunk CRC made right again): no reader accepts the image data
    bad = wt.pngAssemble(100, 75, stream, adler ^ 0x100)
    assert bad != png
    with pytest.raises(Exception):
        Image.open(io.BytesIO(bad)).load()
    with pytest.raises(Exception):
        wt.pngAssemble(0, 75, stream, adler)


def test_the_three_assemblers_size_their_files_and_keep_the_stream(lib_plot):
    """pngAssemble, pdfAssemble and gzipAssemble share one wrapper: each on a zlib stream of its own, the file as long as
    the library's wc_*_bytes says and the stream read back out of it."""
    import gzip
    import pdf_reader as rd
    from wisecondor_amd import wisetools as wt
    raws, streams = [], []
    for k in range(3):
        raws.append(bytes(bytearray((7 * i * (k + 1) + i // 5) % 251 for i in range(303 + 100 * k))))      # (303: 3 scanlines of 100 pixels)
        comp = zlib.compressobj(1 + 4 * k, zlib.DEFLATED, -15)
        streams.append(comp.compress(raws[k]) + comp.flush())
    assert len({len(s) for s in streams}) == 3
    png = wt.pngAssemble(100, 3, streams[0], zlib.adler32(raws[0]))
    assert len(png) == lib_plot.wc_png_bytes(len(streams[0]))
    assert zlib.decompress(pr.png_chunks(png)[1][1]) == raws[0]
    pdf = wt.pdfAssemble(28800, 21600, streams[1], zlib.adler32(raws[1]))
    assert len(pdf) == lib_plot.wc_pdf_bytes(len(streams[1]))
    assert rd.Document(pdf).page()[1] == raws[1]
    assert rd.Document(pdf).obj(8)[1][2:-4] == streams[1]
    gz = wt.gzipAssemble(streams[2], zlib.crc32(raws[2]), len(raws[2]))
    assert len(gz) == lib_plot.wc_gzip_bytes(len(streams[2]))
    assert gzip.decompress(gz) == raws[2] and gz[10:-8] == streams[2]


def _parse(argv):
    from wisecondor_amd import wisecondor as cli
    return cli.buildParser().parse_args(argv)


def test_plotbatch_options_and_defaults():
    from wisecondor_amd import wisecondor as cli
    args = _parse(["plotbatch", "a_test.npz", "b_test.npz", "out"])
    assert args.func is cli.toolPlotBatch and args.infiles == ["a_test.npz", "b_test.npz"] and args.outdir == "out"
    # upstream's defaults (wisecondor.py:483-502) for its five options
    assert args.cytofile is None and args.chromosomes == list(range(1, 23)) and args.columns == 2
    assert args.size == [11.7, 8.3] and args.mineffect == 1.5
    assert args.filetype == "png" and args.dpi == 100
    args = _parse(["plotbatch", "a", "out", "-chromosomes", "1,5,22", "-columns", "3", "-size", "6", "4", "-mineffect", "0", "-dpi", "200",
                   "-cytofile", "c.txt", "-batch", "7", "-io", "2"])
    assert (args.chromosomes, args.columns, args.size, args.mineffect, args.dpi, args.cytofile, args.batch, args.io) == \
        ([1, 5, 22], 3, [6.0, 4.0], 0.0, 200, "c.txt", 7, 2)
    from wisecondor_amd import ingest
    assert ingest.plot_output_names(["d/a_test.npz", "b.x"], "o") == [os.path.join("o", "a_test_z.png"), os.path.join("o", "b.x_z.png")]
    with pytest.raises(ValueError):
        ingest.plot_output_names(["d/a.npz", "e/a.npz"], "o")


def test_filetype_pdf_is_refused_and_plot_stays_refused(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *argv: subprocess.run([sys.executable, "-m", "wisecondor_amd.wisecondor"] + list(argv), cwd=str(tmp_path), env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    got = run("plotbatch", "a_test.npz", str(tmp_path / "out"), "-filetype", "pdf")
    assert got.returncode == 2 and "png only" in got.stdout and not (tmp_path / "out").exists()
    got = run("plot", "x", "y")
    assert got.returncode == 2 and "PDF" in got.stdout and "plotbatch" in got.stdout
    assert run("plot", "x").returncode == 2


def test_argument_errors_are_error_lines_with_status_2(tmp_path, capsys):
    """Two inputs with one stem, and a -chromosomes entry the files do not hold: an ERROR line and status 2, no
    traceback, nothing drawn (neither needs a GPU: both are found before the first batch is made)."""
    from wisecondor_amd import wisecondor as cli
    outdir = tmp_path / "out"
    with pytest.raises(SystemExit) as stop:
        cli.main(["plotbatch", str(tmp_path / "a" / "s_test.npz"), str(tmp_path / "b" / "s_test.npz"), str(outdir)])
    assert stop.value.code == 2 and "ERROR: plotbatch:" in capsys.readouterr().out and not outdir.exists()
    args = cli.buildParser().parse_args(["test", "in.npz", "out.npz", "ref.npz"])
    result = dict(results_z=[np.zeros(3), np.ones(2)], results_r=[np.zeros(3), np.ones(2)], results_cwz=np.zeros(2),
                  results_calls=np.zeros((0, 5)), asdef=0.01)
    path = str(tmp_path / "two_test.npz")
    cli.writeTestOutput(path, args, 250000.0, result, 5.8)
    with pytest.raises(SystemExit) as stop:
        cli.main(["plotbatch", path, str(outdir), "-chromosomes", "1,2,3"])
    said = capsys.readouterr().out
    assert stop.value.code == 2 and "ERROR: plotbatch: -chromosomes names 3" in said and "1..2" in said
    assert not os.listdir(str(outdir))


def test_plot_listing_has_guarded_barriers_and_no_scratch(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "plot.hip" in SOURCES and "-ffp-contract=off" in FLAGS
    out = str(tmp_path / "plot.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "plot.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total >= 8, total
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    for want in ("k_plot_list", "k_plot_raster", "k_adler_blocks", "k_adler_rows"):
        assert any(want in n for n in names), (want, names)
    for name, k in zip(names, kernels):
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.sgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
