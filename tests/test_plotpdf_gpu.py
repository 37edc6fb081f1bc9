"""`plotpdf` on the GPU: the content streams k_pdf_content (csrc/pdf.hip) writes against the restatement
(tests/pdf_restated.py), byte for byte -- every case of tests/plot_cases.py at two page sizes with and without a cytoband
file, the one-panel sweep whose section starts take every residue modulo 16, batches whose samples need different slot
counts, z-scores at and beyond the limits, the labels' rounding; the whole file through the tests' reader; the device form;
the command line."""
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

pytestmark = pytest.mark.gpu
CASES = plot_cases.cases() + plot_cases.build_only_cases()
BY_NAME = {c['name']: c for c in CASES}
SIZES = ((4.0, 3.0), (11.7, 8.3))
SHIFT3 = (0, 6, 12, 18, 24)         # multiples of six: the same chromosome lengths, other rows


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@pytest.fixture(scope="module")
def cyto_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("cyto") / "cytoBand.txt"
    path.write_text(plot_cases.CYTO_TEXT)
    return str(path)


def _restated(results, names, chroms, columns, mineffect, size, table=None, binsize=250000):
    """[content bytes] of a batch, as one GPU call makes them: shared slot counts and title width."""
    Wc, Hc = pd.page_size(size)
    lists = [pr.display_list(r['results_z'], r['results_calls'], r['threshold_z'], chroms, mineffect) for r in results]
    slots = pd.slots_of(lists)
    bands = offs = None
    if table is not None:
        bands, offs = pr.band_rows(table, chroms, binsize)
    name_cap = max(len(n.encode('latin1', 'replace')) for n in names) + 1
    return [pd.content(lists[i], r['results_z'], chroms, columns, r['threshold_z'], names[i], Wc, Hc, slots=slots, bands=bands,
                       band_off=offs, name_cap=name_cap) for i, r in enumerate(results)]


def _first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, restated %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    return "first at byte %d: %r, restated %r" % (at, got[max(0, at - 30):at + 30], want[max(0, at - 30):at + 30])


def _draw(wt, results, names, chroms, columns, mineffect, size, cyto=None):
    details = {}
    files = wt.plot_pdf_batch(results, names, cytofile=cyto, chromosomes=chroms, columns=columns, size=size, mineffect=mineffect,
                              details=details)
    assert details['size'] == pd.page_size(size)
    return files, details


def _case_result(case, shift=0, step=1):
    calls = case['calls'] if step == 1 else (np.array([]) if step == 0 else np.asarray(case['calls'])[::step])
    return dict(results_z=plot_cases.zscores(shift) if shift else case['zscores'], results_calls=calls, threshold_z=case['threshold'],
                binsize=case['binsize'])


@pytest.mark.parametrize("with_cyto", (False, True), ids=("nocyto", "cyto"))
@pytest.mark.parametrize("size", SIZES, ids=("4x3", "a4"))
@pytest.mark.parametrize("case", CASES, ids=[c['name'] for c in CASES])
def test_content_equals_the_restatement(case, size, with_cyto, wt, cyto_path):
    results, names = [_case_result(case)], [case['sample']]
    table = pr.load_cytobands(cyto_path) if with_cyto else None
    files, details = _draw(wt, results, names, case['chromosomes'], case['columns'], case['mineffect'], size,
                           cyto_path if with_cyto else None)
    want = _restated(results, names, case['chromosomes'], case['columns'], case['mineffect'], size, table, case['binsize'])
    assert details['content'][0] == want[0], _first_difference(details['content'][0], want[0])
    assert details['row_bytes'] == [len(want[0])]


def test_content_on_the_sweep_of_section_starts(wt):
    """Every section start at every residue modulo 16 (tests/test_pdf_cases_cpu.py asserts that of this sweep's offsets)."""
    for job in pd.sweep():
        results = [dict(results_z=job['zscores'], results_calls=job['calls'], threshold_z=job['threshold'], binsize=250000)]
        files, details = _draw(wt, results, [job['name']], [1], 1, 0, (4.0, 3.0))
        secs = []
        lists = pr.display_list(job['zscores'], job['calls'], job['threshold'], [1], 0)
        want = pd.content(lists, job['zscores'], [1], 1, job['threshold'], job['name'], 28800, 21600, sections=secs)
        assert details['content'][0] == want, (job['name'], _first_difference(details['content'][0], want))
        assert list(details['offsets'][0]) == [s[2] for s in secs]


def test_a_batch_with_unequal_counts_has_equal_rows_and_every_sample_its_own_list(wt):
    bins = 43
    quiet = np.linspace(-3.0, 3.0, bins)
    quiet[quiet == 0] = 0.5
    striped = quiet.copy()
    striped[::2] = 0.0                                                      # ceil(bins / 2) patches
    many = np.array([(1, k, k + 1, (-1) ** k * (6.0 + k), 0.03 * (k + 1)) for k in range(30)], dtype=np.float64)
    other = [np.arange(5, dtype=np.float64) - 2.0]
    results = [dict(results_z=[quiet] + other, results_calls=np.array([]), threshold_z=5.0, binsize=250000),
               dict(results_z=[striped] + other, results_calls=many[:2], threshold_z=5.0, binsize=250000),
               dict(results_z=[quiet] + other, results_calls=many, threshold_z=5.0, binsize=250000)]      # max_calls calls on one chromosome
    names = ["quiet", "striped_zeros", "calls"]
    files, details = _draw(wt, results, names, [1, 2], 2, 0, (6.0, 4.0))
    want = _restated(results, names, [1, 2], 2, 0, (6.0, 4.0))
    assert len(details['row_bytes']) == 1 and len({len(c) for c in details['content']}) == 1
    lists = [pr.display_list(r['results_z'], r['results_calls'], 5.0, [1, 2], 0) for r in results]
    assert [len(l[0]) - 1 for l in lists] == [0, (bins + 1) // 2 + 2, 30]
    for i in range(3):
        assert details['content'][i] == want[i], (i, _first_difference(details['content'][i], want[i]))
        prims = rd.interpret(details['content'][i])
        fills = [q for q in prims if q['kind'] == 'fill' and q['clip'] is not None]
        assert len(fills) == sum(len(l) - 1 for l in lists[i])                        # its own list, not the batch's slots
        labels = [q['text'].rstrip() for q in prims if q['kind'] == 'text' and q['clip'] is not None]
        assert labels == [pr.label_text(e[8]) for l in lists[i] for e in l if e[0] == pr.CALL]
    # alone, the sample without a patch or a call has a shorter row with the same drawing
    alone, d1 = _draw(wt, results[:1], names[:1], [1, 2], 2, 0, (6.0, 4.0))
    assert d1['row_bytes'][0] < details['row_bytes'][0]
    strip = lambda prims: [{k: v for k, v in q.items() if k != 'text'} if q['kind'] == 'text' and q['size'] == 12 else q for q in prims]
    assert strip(rd.interpret(d1['content'][0])) == strip(rd.interpret(details['content'][0]))


def test_values_at_and_beyond_the_limits(wt):
    nan, inf = np.nan, np.inf
    z = [np.array([1e300, -1e300, 1.0, nan, 2.0, inf, -inf, 3.0, 4.0]),        # clamped; line breaks
         np.array([nan, nan, -7.5, nan]),                                      # a lone finite bin draws nothing
         np.zeros(0),                                                          # a panel without a bin
         np.array([1.7e308, -1.7e308, 0.0])]                                   # a range whose padding overflows
    calls = np.array([(1, 0, 1, 1e300, 0.5), (1, 2, 4, -1e300, -0.5), (1, 5, 6, nan, 0.3), (1, -1e12, 1e12, 7.0, 0.1),     # (far outside the box)
                      (2, 0, 3, inf, 0.2), (3, 0, 0, 5.0, 0.1), (4, 0, 2, -inf, 1e300)])
    results = [dict(results_z=z, results_calls=calls, threshold_z=5.0, binsize=250000)]
    files, details = _draw(wt, results, ["limits"], [1, 2, 3, 4], 2, 0, (4.0, 3.0))
    want = _restated(results, ["limits"], [1, 2, 3, 4], 2, 0, (4.0, 3.0))
    assert details['content'][0] == want[0], _first_difference(details['content'][0], want[0])
    # the far call's corners stop at the limit, its width is their difference; where the mapping is NaN (chromosome 4: inf / inf)
    # a coordinate lies at the lower limit, flipped: Hc + 9 999 999
    assert b"-99999.99    154.73 199999.98" in want[0] and b"100215.99" in want[0]
    prims = rd.interpret(details['content'][0])
    polylines = [q for q in prims if q['kind'] == 'stroke' and len(q['path']) > 2]
    assert len(polylines) == 2                                                 # chromosomes 1 and 4; 2 and 3 stroke nothing
    assert [seg[0] for seg in polylines[0]['path']] == ['m', 'm', 'l', 'l', 'm', 'm', 'l']
    assert [q['text'].rstrip() for q in prims if q['kind'] == 'text' and q['clip'] is not None] == ["?", "?", "?", "7.0", "?", "5.0", "?"]


def test_labels_round_as_python_formats_them(wt):
    tricky = [0.25, 0.75, 1.25, 0.05, 0.15, 0.35, -0.45, 2.675, 1e-300, -1e-300, 0.049999999999999996, 0.95, 9.95, 99.95, -99.95,
              999.95, 0.1 + 0.2 - 0.25, 123456.75, 123456.25, 999999999.94, 999999999.96, 1e9, -1e9, np.nextafter(1e9, 0), np.inf,
              -np.inf, -0.0, 0.0, 7.45, 7.55, 8.5e-2, 6.5, 4503599627370.5 / 1e4, 33.35, 33.45, 1.0000000000000002, 0.5, 1.5,
              0.65, 0.85]                                                      # tests/test_plot_gpu.py's rounding cases
    z = [np.linspace(-3.0, 3.0, 40)] + [np.zeros(0)] * 21
    results = []
    for i in range(5):
        calls = np.array([(1, 5 * k, 5 * k + 4, tricky[8 * i + k], 0.05 + 0.03 * k) for k in range(8)], dtype=np.float64)
        results.append(dict(results_z=z, results_calls=calls, threshold_z=4.0, binsize=250000))
    names = ["r%d" % i for i in range(5)]
    files, details = _draw(wt, results, names, [1], 1, 0, (8.0, 3.0))
    want = _restated(results, names, [1], 1, 0, (8.0, 3.0))
    for i in range(5):
        assert details['content'][i] == want[i], (i, _first_difference(details['content'][i], want[i]))
        labels = [q['text'].rstrip() for q in rd.interpret(details['content'][i]) if q['kind'] == 'text' and q['clip'] is not None]
        assert labels == ["{:.1f}".format(v) if abs(v) < 1e9 else "?" for v in tricky[8 * i:8 * i + 8]]


def test_the_same_bytes_twice_and_after_a_larger_job(wt, cyto_path):
    case = BY_NAME["cyto"]
    results = [_case_result(case, s, step) for s, step in zip(SHIFT3[:3], (1, 2, 0))]
    names = ["a", "b\xe9", "c"]                                             # (a character outside ASCII draws '?')
    chroms = case['chromosomes']
    first, d1 = _draw(wt, results, names, chroms, 2, 1.5, (4.0, 3.0), cyto_path)
    again, d2 = _draw(wt, results, names, chroms, 2, 1.5, (4.0, 3.0), cyto_path)
    assert first == again and d1['content'] == d2['content']
    big = BY_NAME["all22_c2"]
    _draw(wt, [_case_result(big, s) for s in SHIFT3], list("vwxyz"), big['chromosomes'], 2, 1.5, (11.7, 8.3))
    third, d3 = _draw(wt, results, names, chroms, 2, 1.5, (4.0, 3.0), cyto_path)
    assert first == third and d1['content'] == d3['content']
    want = _restated(results, names, chroms, 2, 1.5, (4.0, 3.0), pr.load_cytobands(cyto_path))
    assert d1['content'] == want
    title = [q for q in rd.interpret(d1['content'][1]) if q['kind'] == 'text' and q['size'] == 12][0]
    assert title['text'].rstrip() == pr.TITLE + "b?"


def test_interleaved_thresholds_keep_their_places(wt):
    """Five samples whose thresholds alternate take two GPU calls, samples 0, 2, 4 and samples 1, 3.  A page's bytes
    depend on its call: the title's record is as wide as the whole batch's longest name needs and a section has the slots of
    the call's longest list, so a sample drawn alone has other bytes by design (its title record alone is 2 bytes shorter
    per character its name lacks to the longest).  Byte for byte the batch is therefore held to one call per threshold --
    the longest name's length occurs in both, so those calls' title width is the batch's -- and to the five single-sample
    calls in what the reader draws of them."""
    case = BY_NAME["one_c1"]
    thresholds = (5.0, 4.0, 5.0, 4.0, 5.0)
    results = [_case_result(case, s, step) for s, step in zip(SHIFT3, (1, 0, 2, 3, 1))]
    for res, thr in zip(results, thresholds):
        res['threshold_z'] = thr
    names = ["a", "bb_longer", "c_the_longest_name", "d_the_longest_name", "ee"]
    chroms, size = case['chromosomes'], SIZES[0]
    files, details = _draw(wt, results, names, chroms, case['columns'], case['mineffect'], size)
    assert len(details['times_ms']) == len(details['row_bytes']) == len(details['offsets']) == 2
    assert len(set(files)) == 5 and len(set(details['content'])) == 5     # (a sample in another's place would show)
    for call, thr in enumerate((4.0, 5.0)):                                 # the calls go by ascending threshold
        pick = [i for i, t in enumerate(thresholds) if t == thr]
        part, d = _draw(wt, [results[i] for i in pick], [names[i] for i in pick], chroms, case['columns'], case['mineffect'], size)
        assert d['row_bytes'] == [details['row_bytes'][call]] and np.array_equal(d['offsets'][0], details['offsets'][call])
        for k, i in enumerate(pick):
            assert files[i] == part[k], i
            assert details['content'][i] == d['content'][k], (i, _first_difference(details['content'][i], d['content'][k]))
    rstrip = lambda prims: [dict(q, text=q['text'].rstrip()) if q['kind'] == 'text' else q for q in prims]
    for i in range(5):
        alone, d = _draw(wt, results[i:i + 1], names[i:i + 1], chroms, case['columns'], case['mineffect'], size)
        assert rstrip(rd.interpret(d['content'][0])) == rstrip(rd.interpret(details['content'][i])), i
        assert rd.Document(files[i]).page()[1] == details['content'][i]


def test_the_two_tools_alternate_on_one_context(wt, cyto_path):
    """plotbatch and plotpdf share the context's pinned table block and its device copy, each with a tail of its own
    behind the tables: PNG of two samples at the largest size, PDF of one with cytobands, PNG of one at the smallest size
    without, the PDF again -- each as the same call gives it as the first call on a fresh context."""
    from wisecondor_amd import _lib
    big, cyto, small = BY_NAME["all22_c2"], BY_NAME["cyto"], BY_NAME["one_c1"]

    def png(ctx, case, n, W, H):
        details = {}
        results = [_case_result(case, s) for s in SHIFT3[:n]]
        files = wt.plot_batch(results, ["png%d" % i for i in range(n)], chromosomes=case['chromosomes'], columns=case['columns'],
                              size=(W / 100.0, H / 100.0), mineffect=case['mineffect'], dpi=100, ctx=ctx, details=details)
        return files, details['scanlines'].tobytes()

    def pdf(ctx):
        details = {}
        files = wt.plot_pdf_batch([_case_result(cyto)], ["a_pdf_name"], cytofile=cyto_path, chromosomes=cyto['chromosomes'], columns=2,
                                  size=SIZES[0], mineffect=1.5, ctx=ctx, details=details)
        return files, details['content'], details['row_bytes'], [list(o) for o in details['offsets']]

    steps = (lambda ctx: png(ctx, big, 2, 400, 300), pdf, lambda ctx: png(ctx, small, 1, 20, 10), pdf)
    shared = _lib.new_context(0)
    try:
        got = [step(shared) for step in steps]
    finally:
        _lib.destroy_context(shared)
    for k, step in enumerate(steps):
        fresh = _lib.new_context(0)
        try:
            want = step(fresh)
        finally:
            _lib.destroy_context(fresh)
        assert got[k] == want, k
    assert got[1] == got[3] and got[0] != got[2]


@pytest.mark.parametrize("size", SIZES, ids=("4x3", "a4"))
def test_whole_file_through_the_reader(size, wt, cyto_path):
    case = BY_NAME["cyto"]
    results = [_case_result(case, s, step) for s, step in zip(SHIFT3[:2], (1, 2))]
    files, details = _draw(wt, results, ["p", "q"], case['chromosomes'], 2, 1.5, size, cyto_path)
    Wc, Hc = pd.page_size(size)
    for i, data in enumerate(files):
        doc = rd.Document(data)
        for num, at in doc.offsets.items():
            assert data[at:].startswith(b"%d 0 obj\n" % num)
        page, content = doc.page()
        assert [cents for cents in (int(round(float(v) * 100)) for v in page["MediaBox"])] == [0, 0, Wc, Hc]
        assert content == details['content'][i]
        value, raw = doc.obj(8)
        assert value["Length"] == len(raw) and raw[:2] == b"\x78\x01"
        assert int.from_bytes(raw[-4:], "big") == zlib.adler32(content) & 0xffffffff        # the device's Adler-32 is zlib's
        assert zlib.decompress(raw[2:-4], -15) == content
        assert data == pd.assemble(Wc, Hc, raw[2:-4], zlib.adler32(content))
        assert rd.interpret(content, doc, page["Resources"]) == rd.interpret(content)


def test_device_form_gives_the_host_forms_streams(wt, cyto_path):
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    case = BY_NAME["cyto"]
    results = [_case_result(case, s, step) for s, step in zip(SHIFT3[:3], (1, 0, 2))]
    names = ["d0", "d1", "d2"]
    Wc, Hc = pd.page_size((4.0, 3.0))
    files, details = _draw(wt, results, names, case['chromosomes'], 2, 1.5, (4.0, 3.0), cyto_path)
    rows, sizes, calls, n_calls = wt._dense_results([r['results_z'] for r in results], [r['results_calls'] for r in results])
    bands, band_off = wt.plotBands(wt.loadCytoBands(cyto_path), case['chromosomes'], case['binsize'])
    panels = np.array(case['chromosomes'], dtype=np.int32)
    bound = int(lib.wc_plot_pdf_row_bound(_lib.ptr(sizes), len(sizes), _lib.ptr(panels), len(panels), _lib.ptr(band_off), calls.shape[1], 3))
    assert bound >= details['row_bytes'][0]
    stride, row_stride = int(lib.wc_deflate_bound(bound)), (bound + 15) // 16 * 16 + 32
    dev = torch.device("cuda", 0)
    d_rows, d_calls, d_n = (torch.from_numpy(a).to(dev) for a in (rows, calls, n_calls))
    name_block = np.zeros((3, 3), dtype=np.uint8)
    for i, n in enumerate(names):
        name_block[i, :2] = np.frombuffer(n.encode(), dtype=np.uint8)
    content = torch.full((3, row_stride), 0x55, dtype=torch.uint8, device=dev)
    streams = torch.zeros((3, stride), dtype=torch.uint8, device=dev)
    lengths = torch.zeros(3, dtype=torch.int64, device=dev)
    adler = torch.zeros(3, dtype=torch.int32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    used = np.zeros(1, dtype=np.int64)
    starts = np.zeros(11 * len(panels) + 3, dtype=np.int64)
    with torch.cuda.device(dev):
        _lib.check(lib.wc_plot_pdf_batch_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), rows.shape[1], 3,
                                             _lib.ptr(sizes), len(sizes), d_calls.data_ptr(), d_n.data_ptr(), calls.shape[1],
                                             float(case['threshold']), 1.5, _lib.ptr(panels), len(panels), 2, _lib.ptr(bands),
                                             _lib.ptr(band_off), _lib.ptr(name_block), 3, Wc, Hc, content.data_ptr(), row_stride,
                                             streams.data_ptr(), stride, lengths.data_ptr(), adler.data_ptr(), _lib.ptr(used),
                                             _lib.ptr(starts), status.data_ptr()))
        torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0 and int(used[0]) == details['row_bytes'][0] and np.array_equal(starts, details['offsets'][0])
    n = int(used[0])
    padded = (n + 15) // 16 * 16
    host, lens, adlers = content.cpu().numpy(), lengths.cpu().numpy(), adler.cpu().numpy().view(np.uint32)
    for i in range(3):
        assert host[i, :n].tobytes() == details['content'][i]
        assert (host[i, n:padded] == 0x20).all() and (host[i, padded:] == 0x55).all()      # spaces to the next 16, nothing behind
        assert int(adlers[i]) == zlib.adler32(details['content'][i]) & 0xffffffff
        stream = streams[i, :int(lens[i])].cpu().numpy().tobytes()
        assert zlib.decompress(stream, -15) == details['content'][i]
        assert wt.pdfAssemble(Wc, Hc, stream, adlers[i]) == files[i]


def test_plotpdf_command_line(tmp_path, wt, cyto_path, golden, capsys):
    """Five result files in batches of two with two thresholds, and one that cannot be read."""
    from oracle import wc_oracle as wo
    from wisecondor_amd import ingest
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
        cli.writeTestOutput(paths[-1], args, float(g["binsize"]), res, out["threshold_z"] * (1.5 if i % 2 else 1.0))
    damaged = str(tmp_path / "damaged_test.npz")
    with open(damaged, "wb") as f:
        f.write(open(paths[0], "rb").read()[:200])
    outdir = tmp_path / "plots"
    argv = ["plotpdf"] + paths[:3] + [damaged] + paths[3:] + [str(outdir), "-batch", "2", "-size", "6", "4.5", "-cytofile", cyto_path]
    with pytest.raises(SystemExit) as stop:
        cli.main(argv)
    assert stop.value.code == 1
    said = capsys.readouterr().out
    assert "damaged_test.npz skipped: cannot be read" in said and "5 plots written" in said
    assert sorted(os.listdir(str(outdir))) == ["s%d_test_z.pdf" % i for i in range(5)]
    loaded = [ingest._load_result(p) for p in paths]
    assert len({r['threshold_z'] for r in loaded}) == 2
    # the batches were (s0, s1), (s2), (s3, s4): a file's bytes depend on its batch through the slot counts
    for group in ((0, 1), (2,), (3, 4)):
        want = wt.plot_pdf_batch([loaded[i] for i in group], [wt.sampleNameOf(paths[i]) for i in group], cytofile=cyto_path,
                                 size=(6.0, 4.5), mineffect=1.5)
        for i, data in zip(group, want):
            assert open(str(outdir / ("s%d_test_z.pdf" % i)), "rb").read() == data
            rd.interpret(rd.Document(data).page()[1])
    assert len({open(str(outdir / f), "rb").read() for f in os.listdir(str(outdir))}) == 5


def test_a_batch_beyond_the_deflate_calls_limits_is_refused_up_front(wt):
    from wisecondor_amd import _lib
    lib = _lib.load()
    dummy = np.zeros(64, dtype=np.float64)
    names = np.zeros(8, dtype=np.uint8)
    panels = np.array([1], dtype=np.int32)
    # (the limits are held before any buffer is touched: the small arrays are never read)
    for n_samples, bins in ((65536, 4), (40000, (1 << 30) - 1)):
        sizes = np.array([bins], dtype=np.int64)
        rc = lib.wc_plot_pdf_batch(_lib.context(0), _lib.ptr(dummy), bins, n_samples, _lib.ptr(sizes), 1, _lib.ptr(dummy), _lib.ptr(dummy), 1,
                                   4.0, 0.0, _lib.ptr(panels), 1, 1, None, None, _lib.ptr(names), 8, 28800, 21600, None, 0, _lib.ptr(dummy),
                                   1 << 40, _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), None, None)
        assert rc == _lib.E_LIMIT, (rc, lib.wc_last_error())
    sizes = np.array([4], dtype=np.int64)
    rc = lib.wc_plot_pdf_batch(_lib.context(0), _lib.ptr(dummy), 4, 1, _lib.ptr(sizes), 1, _lib.ptr(dummy), _lib.ptr(dummy), 1,
                               float('nan'), 0.0, _lib.ptr(panels), 1, 1, None, None, _lib.ptr(names), 8, 28800, 21600, None, 0,
                               _lib.ptr(dummy), 1 << 20, _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), None, None)
    assert rc == _lib.E_ARG and b"threshold" in lib.wc_last_error()
