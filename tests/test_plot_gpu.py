"""`plotbatch` on the GPU: the kernels of csrc/plot.hip against the numpy restatement (tests/plot_restated.py), bit for
bit -- the display list of every case of tests/plot_cases.py, the scanline bytes at three image sizes and three
resolutions and in batches, the Adler-32 against zlib, the whole PNG through zlib and PIL, the command line."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plot_cases  # noqa: E402
import plot_restated as pr  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = plot_cases.cases() + plot_cases.build_only_cases()
BY_NAME = {c['name']: c for c in CASES}
SIZES = ((20, 10), (100, 75), (400, 300))


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@pytest.fixture(scope="module")
def cyto_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("cyto") / "cytoBand.txt"
    path.write_text(plot_cases.CYTO_TEXT)
    return str(path)


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=[c['name'] for c in CASES])
def test_plot_list_equals_the_restated_list(case, wt):
    want = pr.display_list(case['zscores'], case['calls'], case['threshold'], case['chromosomes'], case['mineffect'])
    entries, counts, status = wt.plotList([case['zscores']], [case['calls']], case['threshold'], case['chromosomes'],
                                          case['mineffect'])
    assert status == 0 and counts.shape == (1, len(want))
    for p, rows in enumerate(want):
        assert counts[0, p] == len(rows)
        assert _same(entries[0, p, :len(rows)], rows), (p, entries[0, p, :len(rows)], rows)
        assert not entries[0, p, len(rows):].any()


def test_plot_list_of_several_samples_and_a_capacity_that_is_too_small(wt):
    case = BY_NAME["all22_c2"]
    zs = [plot_cases.zscores(s) for s in (0, 6, 12)]                  # (shift 0, 6 and 12 keep chromosome 1 at 40 bins)
    assert len({tuple(len(c) for c in z) for z in zs}) == 1
    calls = [case['calls'], np.array([]), case['calls'][::2]]
    entries, counts, status = wt.plotList(zs, calls, 5.8, case['chromosomes'], 1.5)
    assert status == 0
    need = 0
    for i in range(3):
        for p, rows in enumerate(pr.display_list(zs[i], calls[i], 5.8, case['chromosomes'], 1.5)):
            assert counts[i, p] == len(rows) and _same(entries[i, p, :len(rows)], rows)
            need = max(need, len(rows))
    # a deliberately small capacity: the status word is raised, the counts still say what is needed, nothing beyond the
    # capacity is written and what is written is right
    cap = 5
    assert need > cap
    small, counts2, status = wt.plotList(zs, calls, 5.8, case['chromosomes'], 1.5, capacity=cap)
    assert status == 1 and np.array_equal(counts2, counts) and small.shape[2] == cap
    for i in range(3):
        for p in range(22):
            k = min(cap, counts[i, p])
            assert _same(small[i, p, :k], entries[i, p, :k])      # whole entries: a stretch's start and end share an index
    _, _, status = wt.plotList(zs, calls, 5.8, case['chromosomes'], 1.5, capacity=need)
    assert status == 0


def _results(case, shifts, call_steps):
    out = []
    for shift, step in zip(shifts, call_steps):
        calls = case['calls'] if step == 1 else (np.array([]) if step == 0 else np.asarray(case['calls'])[::step])
        out.append(dict(results_z=plot_cases.zscores(shift), results_calls=calls, threshold_z=case['threshold'],
                        binsize=case['binsize']))
    return out


def _restated(case, res, name, W, H, dpi, table):
    chroms = case['chromosomes']
    lists = pr.display_list(res['results_z'], res['results_calls'], res['threshold_z'], chroms, case['mineffect'])
    bands = offs = None
    if table is not None:
        bands, offs = pr.band_rows(table, chroms, case['binsize'])
    return pr.raster(lists, res['results_z'], chroms, case['columns'], res['threshold_z'], name, W, H, dpi, bands, offs)


def _draw(wt, case, results, names, W, H, dpi, cyto):
    details = {}
    pngs = wt.plot_batch(results, names, cytofile=cyto, chromosomes=case['chromosomes'], columns=case['columns'],
                         size=(W / float(dpi), H / float(dpi)), mineffect=case['mineffect'], dpi=dpi, details=details)
    assert details['size'] == (W, H)
    return pngs, details['scanlines']


SHIFT3 = (0, 6, 12, 18, 24)         # multiples of six: the same chromosome lengths, other rows


@pytest.mark.parametrize("dpi", (50, 100, 200))
@pytest.mark.parametrize("W,H", SIZES)
def test_scanlines_equal_the_restatement(W, H, dpi, wt, cyto_path):
    n = {50: 1, 100: 3, 200: 5}[dpi]
    for name in ("cyto_missing", "five_c3") if (W, H) != SIZES[2] else ("cyto_missing", "all22_c3"):
        case = BY_NAME[name]
        cyto = cyto_path if case['cyto'] else None
        table = pr.load_cytobands(cyto_path) if case['cyto'] else None
        results = _results(case, SHIFT3[:n], (1, 0, 2, 3, 1)[:n])
        names = ["s%d_%s" % (i, "x" * i) for i in range(n)]
        pngs, scan = _draw(wt, case, results, names, W, H, dpi, cyto)
        for i in range(n):
            want = _restated(case, results[i], names[i], W, H, dpi, table)
            if not np.array_equal(scan[i], want):
                bad = np.argwhere(scan[i] != want)
                raise AssertionError("%s sample %d: %d bytes differ, first at row %d byte %d: %d, restated %d"
                                     % (name, i, len(bad), bad[0][0], bad[0][1], scan[i][tuple(bad[0])], want[tuple(bad[0])]))


def test_the_same_bytes_twice_and_after_a_larger_job(wt, cyto_path):
    case = BY_NAME["cyto"]
    results = _results(case, SHIFT3[:3], (1, 2, 0))
    names = ["a", "b\xe9", "c"]                                     # (a character outside the glyph table draws '?')
    first, scan1 = _draw(wt, case, results, names, 100, 75, 100, cyto_path)
    again, scan2 = _draw(wt, case, results, names, 100, 75, 100, cyto_path)
    assert first == again and np.array_equal(scan1, scan2)
    big = BY_NAME["all22_c2"]
    _draw(wt, big, _results(big, SHIFT3, (1, 1, 2, 0, 3)), list("vwxyz"), 400, 300, 100, None)
    third, scan3 = _draw(wt, case, results, names, 100, 75, 100, cyto_path)
    assert first == third and np.array_equal(scan1, scan3)
    want = _restated(case, results[1], "b?", 100, 75, 100, pr.load_cytobands(cyto_path))
    assert np.array_equal(scan1[1], want)


def test_interleaved_thresholds_keep_their_places(wt):
    """Five samples whose thresholds alternate take two GPU calls, samples 0, 2, 4 and samples 1, 3: file and scanlines i
    are those of sample i drawn alone."""
    case = BY_NAME["one_c1"]
    results = _results(case, SHIFT3, (1, 0, 2, 3, 1))
    for res, thr in zip(results, (5.0, 4.0, 5.0, 4.0, 5.0)):
        res['threshold_z'] = thr
    names = ["a", "bb_longer", "ccc", "d_the_longest_name", "ee"]
    W, H = SIZES[0]
    kw = dict(chromosomes=case['chromosomes'], columns=case['columns'], size=(W / 100.0, H / 100.0), mineffect=case['mineffect'], dpi=100)
    details = {}
    pngs = wt.plot_batch(results, names, details=details, **kw)
    assert len(details['times_ms']) == 2 and details['scanlines'].shape == (5, H, 1 + 3 * W)
    for i in range(5):
        one = {}
        alone = wt.plot_batch(results[i:i + 1], names[i:i + 1], details=one, **kw)
        assert pngs[i] == alone[0], i
        assert np.array_equal(details['scanlines'][i], one['scanlines'][0]), i
        assert len(one['times_ms']) == 1
    assert len(set(pngs)) == 5                                     # (a sample in another's place would show)


@pytest.mark.parametrize("n_bytes", (0, 1, 5551, 5552, 5553, 65536, 65537, 200003))
def test_adler32_rows_against_zlib(n_bytes, wt):
    rng = np.random.RandomState(n_bytes % 1000)
    rows = rng.randint(0, 256, size=(3, n_bytes)).astype(np.uint8)
    if n_bytes:
        rows[1] = 0xff                                               # the largest sums a row can have
    got = wt.adler32Rows(rows)
    assert [int(v) for v in got] == [zlib.adler32(rows[i].tobytes()) & 0xffffffff for i in range(3)]


@pytest.mark.parametrize("W,H", (SIZES[0], SIZES[2]))
def test_whole_png_through_zlib_and_pil(W, H, wt, cyto_path):
    from PIL import Image
    from wisecondor_amd import _lib
    assert (H * (1 + 3 * W) < _lib.load().wc_deflate_block_bytes()) == ((W, H) == SIZES[0])      # one deflate block / several
    case = BY_NAME["cyto"]
    results = _results(case, SHIFT3[:2], (1, 2))
    pngs, scan = _draw(wt, case, results, ["p", "q"], W, H, 100, cyto_path)
    table = pr.load_cytobands(cyto_path)
    for i, png in enumerate(pngs):
        chunks = pr.png_chunks(png)
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)
        want = _restated(case, results[i], "pq"[i], W, H, 100, table)
        assert zlib.decompress(chunks[1][1]) == want.tobytes() == scan[i].tobytes()
        im = Image.open(io.BytesIO(png))
        assert im.size == (W, H) and np.array_equal(np.asarray(im.convert("RGB")), want[:, 1:].reshape(H, W, 3))


def test_plotbatch_command_line(tmp_path, wt, cyto_path, golden, capsys):
    """Five result files (written by writeTestOutput from the oracle's result, as tests/test_consumers_cpu.py does) and
    one with other chromosome lengths, in batches of 2."""
    from oracle import wc_oracle as wo
    from wisecondor_amd import wisecondor as cli
    g = golden("cfg1_pipeline.npz")
    keys = [str(c) for c in range(1, len(g["sample_chrom_lengths"]) + 1)]
    offs = np.concatenate([[0], np.cumsum(g["sample_chrom_lengths"])])
    sample = {k: g["t_loss2_sample"][offs[i]:offs[i + 1]] for i, k in enumerate(keys)}
    ref = dict(binsize=g["ref_binsize"], indexes=g["ref_indexes"], distances=g["ref_distances"],
               chromosome_sizes=g["ref_chromosome_sizes"], mask=g["ref_mask"], masked_sizes=g["ref_masked_sizes"],
               pca_mean=g["ref_pca_mean"], pca_components=g["ref_pca_components"])
    out = wo.test_sample(sample, float(g["binsize"]), ref)
    args = cli.buildParser().parse_args(["test", "in.npz", "out.npz", "ref.npz"])
    paths = []
    for i in range(5):
        res = dict(out)
        res["results_z"] = [np.asarray(c, dtype=np.float64) * (1.0 + 0.25 * i) for c in out["results_z"]]
        res["results_calls"] = np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5)[:len(out["results_calls"]) - i]
        paths.append(str(tmp_path / ("s%d_test.npz" % i)))
        cli.writeTestOutput(paths[-1], args, float(g["binsize"]), res, out["threshold_z"])
    odd = dict(out)
    odd["results_z"] = [np.asarray(c)[:-1] for c in out["results_z"]]
    odd_path = str(tmp_path / "odd_test.npz")
    cli.writeTestOutput(odd_path, args, float(g["binsize"]), odd, out["threshold_z"])
    outdir = tmp_path / "plots"
    argv = ["plotbatch"] + paths[:3] + [odd_path] + paths[3:] + [str(outdir), "-batch", "2", "-size", "6", "4.5", "-cytofile", cyto_path]
    with pytest.raises(SystemExit) as stop:
        cli.main(argv)
    assert stop.value.code == 1
    said = capsys.readouterr().out
    assert "odd_test.npz skipped: other chromosome lengths" in said and "5 plots written" in said
    assert sorted(os.listdir(str(outdir))) == ["s%d_test_z.png" % i for i in range(5)]
    from wisecondor_amd import ingest
    for i, path in enumerate(paths):
        alone = wt.plot_batch([ingest._load_result(path)], [wt.sampleNameOf(path)], cytofile=cyto_path, size=(6.0, 4.5),
                              mineffect=1.5)[0]
        assert open(str(outdir / ("s%d_test_z.png" % i)), "rb").read() == alone
    assert len({open(str(outdir / f), "rb").read() for f in os.listdir(str(outdir))}) == 5


def test_labels_round_as_python_formats_them(wt):
    """"{:.1f}".format(z) rounds the exact value to the nearest tenth, ties to even: z values on and beside such ties, at
    the ends of the label's range, signed zeros and values that are not finite, five samples of eight calls each."""
    tricky = [0.25, 0.75, 1.25, 0.05, 0.15, 0.35, -0.45, 2.675, 1e-300, -1e-300, 0.049999999999999996, 0.95, 9.95, 99.95, -99.95,
              999.95, 0.1 + 0.2 - 0.25, 123456.75, 123456.25, 999999999.94, 999999999.96, 1e9, -1e9, np.nextafter(1e9, 0), np.inf,
              -np.inf, -0.0, 0.0, 7.45, 7.55, 8.5e-2, 6.5, 4503599627370.5 / 1e4, 33.35, 33.45, 1.0000000000000002, 0.5, 1.5,
              0.65, 0.85]
    assert len(tricky) == 40
    z = [np.linspace(-3.0, 3.0, 40)] + [np.zeros(0)] * 21
    results = []
    for i in range(5):
        calls = np.array([(1, 5 * k, 5 * k + 4, tricky[8 * i + k], 0.05 + 0.03 * k) for k in range(8)], dtype=np.float64)
        results.append(dict(results_z=z, results_calls=calls, threshold_z=4.0, binsize=250000))
    names = ["r%d" % i for i in range(5)]
    details = {}
    wt.plot_batch(results, names, chromosomes=[1], columns=1, size=(8.0, 3.0), mineffect=0, dpi=100, details=details)
    W, H = details['size']
    for i, res in enumerate(results):
        lists = pr.display_list(z, res['results_calls'], 4.0, [1], 0)
        assert len(lists[0]) == 9
        want = pr.raster(lists, z, [1], 1, 4.0, names[i], W, H, 100)
        assert np.array_equal(details['scanlines'][i], want), (i, [pr.label_text(v) for v in res['results_calls'][:, 3]])


def test_a_batch_beyond_the_deflate_calls_limits_is_refused_up_front(wt):
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = np.array([4], dtype=np.int64)
    panels = np.array([1], dtype=np.int32)
    dummy = np.zeros(64, dtype=np.float64)
    names = np.zeros(8, dtype=np.uint8)
    image = lib.wc_plot_image_bytes(20, 10)
    stride = lib.wc_deflate_bound(image)
    # (the limits are held before any buffer is touched: the small arrays are never read)
    for n_samples, w, h in ((65536, 20, 10), (40000, 32768, 32768)):
        stride = lib.wc_deflate_bound(lib.wc_plot_image_bytes(w, h))
        rc = lib.wc_plot_batch(_lib.context(0), _lib.ptr(dummy), 4, n_samples, _lib.ptr(sizes), 1, _lib.ptr(dummy), _lib.ptr(dummy), 1,
                               4.0, 0.0, _lib.ptr(panels), 1, 1, None, None, _lib.ptr(names), 8, w, h, 100, None, _lib.ptr(dummy),
                               stride, _lib.ptr(dummy), _lib.ptr(dummy), None)
        assert rc == _lib.E_LIMIT, (rc, lib.wc_last_error())
    assert lib.wc_plot_image_bytes(0, 10) == -1 and lib.wc_plot_image_bytes(32769, 10) == -1
    rc = lib.wc_plot_batch(_lib.context(0), _lib.ptr(dummy), 4, 1, _lib.ptr(sizes), 1, _lib.ptr(dummy), _lib.ptr(dummy), 1,
                           float('nan'), 0.0, _lib.ptr(panels), 1, 1, None, None, _lib.ptr(names), 8, 20, 10, 100, None,
                           _lib.ptr(np.zeros(stride + 8, dtype=np.uint8)), lib.wc_deflate_bound(image), _lib.ptr(dummy), _lib.ptr(dummy), None)
    assert rc == _lib.E_ARG and b"threshold" in lib.wc_last_error()


def test_device_form_gives_the_host_forms_streams(wt, cyto_path):
    """wc_plot_batch_dev on device-resident rows and calls (the layout wc_test_batch_dev leaves there): the same
    scanlines, streams, lengths and Adler-32 words as the host form.  Two calls with different names are enqueued on one
    stream without a synchronise between them: the second must not disturb the tables of the first."""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    case = BY_NAME["cyto"]
    results = _results(case, SHIFT3[:3], (1, 0, 2))
    W, H = 100, 75
    rows, sizes, calls, n_calls = wt._dense_results([r['results_z'] for r in results], [r['results_calls'] for r in results])
    bands, band_off = wt.plotBands(wt.loadCytoBands(cyto_path), case['chromosomes'], case['binsize'])
    panels = np.array(case['chromosomes'], dtype=np.int32)
    dev = torch.device("cuda", 0)
    image = int(lib.wc_plot_image_bytes(W, H))
    stride, scan_stride = int(lib.wc_deflate_bound(image)), (image + 15) // 16 * 16 + 32
    d_rows, d_calls, d_n = (torch.from_numpy(a).to(dev) for a in (rows, calls, n_calls))
    name_sets = (["d0", "d1", "d2"], ["e0", "e1", "e2"])
    want = [_draw(wt, case, results, names, W, H, 100, cyto_path) for names in name_sets]
    outs = []
    with torch.cuda.device(dev):
        for names in name_sets:
            name_block = np.zeros((3, 4), dtype=np.uint8)
            for i, n in enumerate(names):
                name_block[i, :2] = np.frombuffer(n.encode(), dtype=np.uint8)
            o = dict(scan=torch.zeros((3, scan_stride), dtype=torch.uint8, device=dev),
                     streams=torch.zeros((3, stride), dtype=torch.uint8, device=dev),
                     len=torch.zeros(3, dtype=torch.int64, device=dev), adler=torch.zeros(3, dtype=torch.int32, device=dev),
                     status=torch.full((1,), -1, dtype=torch.int32, device=dev))
            outs.append(o)
            _lib.check(lib.wc_plot_batch_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), rows.shape[1],
                                             3, _lib.ptr(sizes), len(sizes), d_calls.data_ptr(), d_n.data_ptr(), calls.shape[1],
                                             float(case['threshold']), float(case['mineffect']), _lib.ptr(panels), len(panels),
                                             case['columns'], _lib.ptr(bands), _lib.ptr(band_off), _lib.ptr(name_block), 4, W, H, 100,
                                             o['scan'].data_ptr(), scan_stride, o['streams'].data_ptr(), stride, o['len'].data_ptr(),
                                             o['adler'].data_ptr(), o['status'].data_ptr()))
        torch.cuda.synchronize()
    for o, (pngs, scan) in zip(outs, want):
        assert int(o['status'].cpu()[0]) == 0
        lengths, adlers = o['len'].cpu().numpy(), o['adler'].cpu().numpy().view(np.uint32)
        for i in range(3):
            assert np.array_equal(o['scan'][i, :image].cpu().numpy(), scan[i].reshape(-1))
            assert int(adlers[i]) == zlib.adler32(scan[i].tobytes()) & 0xffffffff
            stream = o['streams'][i, :int(lengths[i])].cpu().numpy().tobytes()
            assert zlib.decompress(stream, -15) == scan[i].tobytes()
            assert wt.pngAssemble(W, H, stream, adlers[i]) == pngs[i]
