"""What one call leaves behind for the next: every family of entry points after every other on one context.

The suite's other files hold each kernel against numpy, the oracle or a restatement -- on the one shared context, in one
fixed order.  Here every test makes its own context(s), runs the jobs of tests/sequence_cases.py in some order and
compares each with the job's baseline, the same job on a context of its own.  The baselines are anchored once against
the independent reference of each family (the first test), so "equals the baseline" is not the code agreeing with
itself.  The named scenarios are the orders in which something is known to go stale: the pinned host block moving under
the latency graph, workspaces growing under it (in this context and in another one; the allocation counter is
process-wide), the prep step's state with other calls between its steps, growth orders, a reference handle closed and
its address reused.  Then every job after every other, seeded walks, and the steady state: a third call of an unchanged
shape allocates nothing.
"""
import ctypes
import gzip
import os
import zlib

import numpy as np
import pytest

import sequence_cases as sq

pytestmark = pytest.mark.gpu
SWEEP = int(os.environ.get("WC_SWEEP", "1"))        # WC_SWEEP=8: eight times the seeds of the walks
GENERAL_LINE = "repeated on the general path"


@pytest.fixture()
def ctx():
    with sq.context() as handle:
        yield handle


@pytest.fixture()
def ctx2():
    with sq.context() as handle:
        yield handle


def agree(got, name, shape, where=None):
    diff = sq.same(got, sq.baseline(name, shape))
    assert diff is None, "%s %s differs from its baseline%s: %s" % (name, shape, "" if where is None else " (%s)" % (where,), diff)


# ------------------------------------------------------------------------------------- the anchors ----
def _anchor_newref(shape, out):
    from oracle import wc_oracle as wo
    data, sizes = sq.newref_case(shape)
    for order, arr in (("F", np.asfortranarray(data)), ("C", np.ascontiguousarray(data))):
        idx, dst = wo.get_reference(arr, sizes, np.cumsum(sizes), sq.NEWREF_K, 1, 1, fast=True)
        assert np.array_equal(out["idx_" + order], idx) and np.array_equal(out["dst_" + order], dst), order
    assert not np.array_equal(out["dst_F"], out["dst_C"])          # the two summation orders do differ on this data


def _anchor_prep(shape, out):
    import prep_cases as pc
    for n_comp in sq.PREP_COMPS:
        want = pc.oracle(*(sq.PREP_CASES[shape] + (n_comp,)))
        pc.check_conditions(want, n_comp)
        get = lambda key: out["%s_%d" % (key, n_comp)]
        assert np.array_equal(get("mask").astype(bool), want["mask"]) and get("mbins").tolist() == want["masked_chrom_bins"]
        assert sq.same({"m": get("masked")}, {"m": want["masked"]}) is None              # one IEEE division per element
        assert sq.same({"m": get("mean")}, {"m": np.mean(want["masked"].T, axis=0)}) is None
        comp_err, corr_err = pc.errors(get("corrected"), get("comps"), want)
        assert comp_err <= pc.COMP_ATOL and corr_err <= pc.CORRECTED_RTOL, (n_comp, comp_err, corr_err)


def _anchor_batch(out, rows, first):
    """Rows of a test-path job against the oracle's toolTest body: call coordinates exact, values to the PCA's tolerance."""
    from oracle import wc_oracle as wo
    lay, found = sq.tp_layout(), 0
    starts = np.concatenate([[0], np.cumsum(out["n_calls"])])
    for row in rows:
        with np.errstate(all="ignore"):
            want = wo.test_sample(sq.tp_samples()[first + row], 1e6, lay, minzscore=sq.TEST_THR)
        wcalls = np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5)
        calls = out["calls"][starts[row]:starts[row + 1]]
        assert np.array_equal(calls[:, :3], wcalls[:, :3]), (row, calls, wcalls)
        assert np.allclose(calls[:, 3:], wcalls[:, 3:], rtol=1e-8, equal_nan=True), row
        assert np.allclose(out["z"][row], np.concatenate(want["results_z"]), rtol=1e-8, atol=1e-10, equal_nan=True), row
        assert np.allclose(out["cwz"][row], want["results_cwz"], rtol=1e-8, atol=1e-10, equal_nan=True), row
        assert np.isclose(out["asdef"][row], float(want["asdef"]), rtol=1e-8), row
        found += len(wcalls)
    assert found >= 1


def _anchor_test_general(shape, out):
    _anchor_batch(out, (0, 1, sq.TEST_SAMPLES[shape] - 1), 0)
    if shape == sq.LARGE:           # a sample's result does not depend on the batch it is in
        n = sq.TEST_SAMPLES[sq.SMALL]
        small, k = sq.baseline("test_general", sq.SMALL), int(out["n_calls"][:n].sum())
        head = dict(out, z=out["z"][:n], r=out["r"][:n], cwz=out["cwz"][:n], calls=out["calls"][:k], n_calls=out["n_calls"][:n],
                    asdef=out["asdef"][:n])
        assert sq.same(head, small) is None, sq.same(head, small)


def _general_route(ctx, count):
    return sq.tp_call(sq.reference_on(ctx), 20, count, mode="0")


def _anchor_test_latency(shape, out):
    _anchor_batch(out, range(sq.LAT_SAMPLES[shape]), 20)
    general = sq.fresh(_general_route, sq.LAT_SAMPLES[shape])
    assert sq.same(out, general) is None, sq.same(out, general)


def _anchor_small(shape, out):
    import prep_cases as pc
    from oracle import wc_oracle as wo
    case, lay = sq.small_case(shape), sq.tp_layout()
    rows = []
    for r, z in enumerate(case["regions"]):
        tri = wo.fill_tri(z)
        rows += [[r, v, x, y] for v, (x, y) in wo.segment_tri(tri, len(z), 3.0, 3)]
        assert sq.same({"w": out["whole"][r:r + 1]}, {"w": np.array([tri[len(z) - 1]])}) is None
    assert len(rows) >= len(case["regions"])
    assert sq.same({"s": out["segs"]}, {"s": np.array(rows, dtype=np.float64).reshape(-1, 4)}) is None
    cutoff, mask = wo.get_optimal_cutoff(lay["distances"], 3)
    assert out["cutoff"][0] == cutoff and np.array_equal(out["cutoff_mask"], mask)
    for i, row in enumerate(case["sd"]):           # trySample's loop: the values that are not NaN, added one by one
        total, n = 0.0, 0
        for v in row.tolist():
            if v == v:
                total, n = total + v, n + 1
        assert out["sd_avg"][i] == total / n, i
    ms = [int(v) for v in lay["masked_sizes"]]
    for i in range(min(3, len(case["data"]))):
        wz, wr, wn, wsd = wo.repeat_test(np.copy(case["data"][i]), lay["indexes"], lay["distances"], ms, [int(v) for v in np.cumsum(ms)],
                                         cutoff, 4.0, 3)
        assert np.array_equal(out["rep_n"][i], wn) and sq.same({"z": out["rep_z"][i]}, {"z": np.asarray(wz, dtype=np.float64)}) is None, i
    x, mean, comps = pc.apply_case(*sq.SMALL_APPLY[shape])
    assert np.allclose(out["pca"], pc.apply_pca_longdouble(x[:sq.SMALL_ROWS[shape]], mean, comps), rtol=1e-12, atol=0)


def _anchor_eigh(shape, out):
    """np.linalg.eigh with the tolerances of test_eigh_gpu.py (random symmetric matrices)."""
    matrix, (n, k) = sq.eigh_case(shape), sq.EIGH[shape]
    vec_tol, val_tol = (1e-10, 1e-13) if shape == sq.SMALL else (1e-9, 1e-12)
    w, v = np.linalg.eigh(matrix)
    w, v = w[::-1], v[:, ::-1].T
    scale = max(abs(w[0]), abs(w[-1]))
    vals, vecs = out["vals"], out["vecs"]
    assert np.abs(vals - w[:k]).max() <= val_tol * scale
    assert np.abs(matrix @ vecs.T - vecs.T * vals).max() <= 1e-12 * scale * np.sqrt(n)
    assert np.abs(vecs @ vecs.T - np.eye(k)).max() <= 1e-12
    for j in range(k):
        assert np.abs(np.sign(np.dot(vecs[j], v[j])) * vecs[j] - v[j]).max() <= vec_tol


def _anchor_convert(shape, out):
    import bam_writer as bw
    import convert_restated as cr
    names, lengths, pos, mapq = sq.convert_case(shape)
    want, stats = cr.convert(names, lengths, pos, mapq, sq.CONVERT_BINSIZE, 4, 4)
    recs = bw.records_of(list(range(len(names))), pos, mapq, 7)
    extra = dict(no_coordinate=7, unmapped=sum(1 for r in recs if r[3] & 4), mapped=sum(1 for r in recs if r[0] >= 0 and not r[3] & 4))
    assert sum(int(np.sum(want[k])) for k in sq.KEYS24) > 1000 and stats["filter_rmdup"] > 0 and stats["filter_mapq"] > 0
    for tag, info in (("reads", dict(stats)), ("bam", dict(stats, **extra))):
        for key in sq.KEYS24:
            assert np.array_equal(out["%s_%s" % (tag, key)], want[key]), (tag, key)
        assert out[tag + "_info"].tolist() == [int(info[k]) for k in sorted(info)], tag


def _anchor_deflate(shape, out):
    rows = sq.deflate_case(shape)
    for i, row in enumerate(rows):
        assert zlib.decompress(out["stream_%d" % i], -15) == row.tobytes(), i
        assert int(out["crcs"][i]) == zlib.crc32(row.tobytes()) & 0xffffffff and int(out["adler"][i]) == zlib.adler32(row.tobytes())
        assert int(out["lengths"][i]) == len(out["stream_%d" % i])
    assert int(out["lengths"][0]) < rows.shape[1] // 50                 # the long run is found


def _as_bytes(text):
    return text if isinstance(text, bytes) else text.encode("ascii")


def _anchor_export(shape, out):
    import json_cases
    import json_restated as jr
    import tracks_restated as tr
    for i, res in enumerate(sq.export_case(shape)):
        z, r = np.concatenate(res["results_z"]), np.concatenate(res["results_r"])
        assert out["json_row_%d" % i] == _as_bytes(jr.row_text(z, json_cases.SIZES, False)), i
        assert gzip.decompress(out["json_gz_%d" % i]) == _as_bytes(jr.file_text(res)), i
        text, dropped = tr.track_text(z, json_cases.SIZES, 250000)
        assert out["bedgraph_row_%d" % i] == _as_bytes(text) and int(out["bedgraph_dropped"][i]) == dropped, i
        assert gzip.decompress(out["track_%d_0" % i]) == _as_bytes(text), i
        assert gzip.decompress(out["track_%d_1" % i]) == _as_bytes(tr.track_text(r, json_cases.SIZES, 250000)[0]), i
        tr.bgzf_blocks(out["track_%d_0" % i])
        assert out["track_%d_2" % i] == tr.calls_bed(np.asarray(res["results_calls"]).reshape(-1, 5), res["binsize"]), i


def _anchor_plot(shape, out):
    import plot_restated as pr
    case, results, names, dpi = sq.plot_case(shape)
    assert int(out["status"][0]) == 0
    for i, res in enumerate(results):
        lists = pr.display_list(res["results_z"], res["results_calls"], case["threshold"], case["chromosomes"], case["mineffect"])
        for p, rows in enumerate(lists):
            assert out["counts"][i, p] == len(rows)
            assert np.array_equal(out["entries"][i, p, :len(rows)], np.asarray(rows, dtype=np.float64).reshape(len(rows), 9), equal_nan=True)
            assert not out["entries"][i, p, len(rows):].any()
        if i == 0:
            want = pr.raster(lists, res["results_z"], case["chromosomes"], case["columns"], res["threshold_z"], names[i], 4 * dpi, 3 * dpi, dpi)
            assert np.array_equal(out["scanlines"][i], want)
        idat = b"".join(payload for kind, payload in pr.png_chunks(out["png_%d" % i]) if kind == b"IDAT")
        assert zlib.decompress(idat) == out["scanlines"][i].tobytes(), i


def _anchor_pdf(shape, out):
    import pdf_reader as rd
    import pdf_restated as pd
    import plot_restated as pr
    case, results, names = sq.pdf_case(shape)
    chroms = case["chromosomes"]
    Wc, Hc = pd.page_size((4.0, 3.0))
    lists = [pr.display_list(r["results_z"], r["results_calls"], r["threshold_z"], chroms, case["mineffect"]) for r in results]
    slots = pd.slots_of(lists)
    name_cap = max(len(n) for n in names) + 1
    for i in sorted({0, 1, len(results) - 1}):
        want = pd.content(lists[i], results[i]["results_z"], chroms, case["columns"], results[i]["threshold_z"], names[i], Wc, Hc,
                          slots=slots, bands=None, band_off=None, name_cap=name_cap)
        assert out["content_%d" % i] == want, i
    for i in range(len(results)):                          # the file through the reader: the page's content is that stream
        content, data = out["content_%d" % i], out["pdf_%d" % i]
        doc = rd.Document(data)
        assert doc.page()[1] == content, i
        raw = doc.obj(8)[1]
        assert zlib.decompress(raw[2:-4], -15) == content and data == pd.assemble(Wc, Hc, raw[2:-4], zlib.adler32(content)), i


def _anchor_sensitivity(shape, out):
    import draw_restated as dr
    import spike_cases as sc
    import spike_restated as sr
    lay, base, plan = sc.lay(), sc.base_counts(), sq.sens_plan(shape)
    assert np.array_equal(out["thinned"], dr.thin(base, lay["sizes"], list(sq.SENS_KEEP[shape]), sq.SENS_SEED))
    want, saturated = sr.spike(base, lay["sizes"], plan)
    drawn, saturated_drawn = dr.spike_draw(base, lay["sizes"], plan, sq.SENS_SEED, trial0=3)
    assert np.array_equal(out["spiked"], want) and np.array_equal(out["drawn"], drawn)
    assert out["saturated"].tolist() == [saturated, saturated_drawn]
    calls, n_calls = sq.sens_calls(shape)
    want_i, want_f = sr.score(plan, calls, n_calls)
    assert sq.same({"i": out["score_i"], "f": out["score_f"]}, {"i": np.asarray(want_i, dtype=np.int32), "f": np.asarray(want_f, dtype=np.float64)}) is None
    starts = np.concatenate([[0], np.cumsum(out["kept_n"])])
    kept = np.zeros((len(plan), 4, 5))
    for i, row in enumerate(plan.tolist()):                        # the oracle's calls of the spiked sample, by bits
        got = out["kept_calls"][starts[i]:starts[i + 1]]
        assert sq.same({"c": got}, {"c": np.array(sc.oracle_calls(tuple(row)))}) is None, (row, got)
        kept[i, :len(got)] = got
    want_i, want_f = sr.score(plan, kept, out["kept_n"].astype(np.int32))
    assert sq.same({"i": out["rec_i"], "f": out["rec_f"]}, {"i": np.asarray(want_i, dtype=np.int32), "f": np.asarray(want_f, dtype=np.float64)}) is None
    assert int(out["kept_n"].sum()) >= 1


def _anchor_crossval(shape, out):
    import crossval_restated as cr
    diff = cr.same(out, cr.stats(**sq.crossval_case(shape)))
    assert diff is None, diff


ANCHORS = dict(newref=_anchor_newref, prep=_anchor_prep, test_general=_anchor_test_general, test_latency=_anchor_test_latency,
               small_entries=_anchor_small, eigh=_anchor_eigh, convert=_anchor_convert, deflate=_anchor_deflate, export=_anchor_export,
               plot=_anchor_plot, pdf=_anchor_pdf, sensitivity=_anchor_sensitivity, crossval=_anchor_crossval)


@pytest.mark.parametrize("name", sq.NAMES)
def test_baseline_equals_the_independent_reference(name):
    """Each job's baseline, in both shapes, against what the suite already holds that family to: the oracle, the
    restatements, zlib, np.linalg.eigh."""
    assert set(ANCHORS) == set(sq.NAMES)
    for shape in sq.SHAPES:
        ANCHORS[name](shape, sq.baseline(name, shape))


# ------------------------------------------------------------------------------- D1 named scenarios ----
def _latency_after(ctx, capfd, monkeypatch, between):
    """The latency job's three calls on a reference that stays open, `between`, then a fourth and a fifth call: both the
    general path's bits, neither repeated on the general path, the fifth without an allocation."""
    count = sq.LAT_SAMPLES[sq.LARGE]
    reference = sq.reference_on(ctx)
    for _ in range(3):
        got = sq.tp_call(reference, 20, count)
    agree(got, "test_latency", sq.LARGE, "third call")
    before = sq.epoch()
    between()
    moved = sq.epoch()
    monkeypatch.setenv("WC_TEST_VERBOSE", "1")
    capfd.readouterr()
    fourth = sq.tp_call(reference, 20, count)
    at_four = sq.epoch()
    fifth = sq.tp_call(reference, 20, count)
    at_five = sq.epoch()
    err = capfd.readouterr().err
    monkeypatch.delenv("WC_TEST_VERBOSE")
    print("allocation epoch: %d before, %d after what ran in between, %d after the fourth call, %d after the fifth"
          % (before, moved, at_four, at_five))
    agree(fourth, "test_latency", sq.LARGE, "fourth call")
    agree(fifth, "test_latency", sq.LARGE, "fifth call")
    assert GENERAL_LINE not in err, err
    assert at_five == at_four, (at_four, at_five)
    return before, moved


def _prep_agrees(got, n_comp):
    want = {k[:-len("_%d" % n_comp)]: v for k, v in sq.baseline("prep", sq.SMALL).items() if k.endswith("_%d" % n_comp)}
    diff = sq.same(got, want)
    assert diff is None, (n_comp, diff)


def test_pinned_block_grown_by_prep_under_a_latency_graph(ctx, capfd, monkeypatch):
    """Prep with one component, the latency graph, prep of the same counts with eight components: the device arrays are
    sized for eight components either way, so the second prep moves the pinned block (8 B -> 64 B bytes) and the graph's
    status words would land in freed host memory.  The block's move must count as a reallocation."""
    _prep_agrees(sq.run_prep_one(ctx, sq.SMALL, 1), 1)
    before, moved = _latency_after(ctx, capfd, monkeypatch, lambda: _prep_agrees(sq.run_prep_one(ctx, sq.SMALL, 8), 8))
    assert moved == before + 1, (before, moved)         # one move: the pinned block's, and no workspace's


def test_pinned_block_grown_by_pdf_under_a_latency_graph(ctx, capfd, monkeypatch):
    """The same with the 66-page pdf job between: its counts' read-back needs more pinned bytes than prep left."""
    _prep_agrees(sq.run_prep_one(ctx, sq.SMALL, 1), 1)
    before, moved = _latency_after(ctx, capfd, monkeypatch, lambda: agree(sq.run_pdf(ctx, sq.LARGE), "pdf", sq.LARGE))
    assert moved != before, (before, moved)


@pytest.mark.parametrize("grower", ["test_general", "newref", "export"])
def test_workspaces_grown_under_a_latency_graph(ctx, capfd, monkeypatch, grower):
    before, moved = _latency_after(ctx, capfd, monkeypatch, lambda: agree(sq.BY_NAME[grower].run(ctx, sq.LARGE), grower, sq.LARGE))
    assert moved != before


@pytest.mark.parametrize("grower", ["test_general", "crossval"])
def test_workspaces_grown_in_another_context_under_a_latency_graph(ctx, ctx2, capfd, monkeypatch, grower):
    """The allocation counter is process-wide: growth in a second context drops this context's graph too, and the call
    after it is still right and still a latency call."""
    before, moved = _latency_after(ctx, capfd, monkeypatch, lambda: agree(sq.BY_NAME[grower].run(ctx2, sq.LARGE), grower, sq.LARGE))
    assert moved != before


def _prep_steps(ctx, n_comp, between=None, finishes=1):
    """wc_newref_prep_gram, `between`, wc_newref_prep_eig, then wc_newref_prep_finish (`finishes` times) and
    wc_newref_prep_finish_dev; every finish as the dict of run_prep_one, the device one without the mask."""
    import prep_cases as pc
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    counts, sizes = pc.make_case(*sq.PREP_CASES[sq.SMALL])
    counts, sizes = np.ascontiguousarray(counts), np.ascontiguousarray(sizes)
    n_s, n_total = counts.shape
    mask, mbins, n_b = np.empty(n_total, dtype=np.uint8), np.empty(22, dtype=np.int64), ctypes.c_int64()
    _lib.check(lib.wc_newref_prep_gram(ctx, _lib.ptr(counts), n_s, n_total, _lib.ptr(sizes), 22, _lib.ptr(mask), _lib.ptr(mbins),
                                       ctypes.byref(n_b), None))
    if between is not None:
        between()
    evals, evecs = np.empty(n_comp), np.empty((n_comp, n_s))
    _lib.check(lib.wc_newref_prep_eig(ctx, n_comp, _lib.ptr(evals), _lib.ptr(evecs)))
    if between is not None:
        between()
    B = n_b.value
    outs = []
    for _ in range(finishes):
        masked, corrected_t, comps, mean = np.empty((B, n_s)), np.empty((n_s, B)), np.empty((n_comp, B)), np.empty(B)
        _lib.check(lib.wc_newref_prep_finish(ctx, n_comp, _lib.ptr(evecs), _lib.ptr(evals), _lib.ptr(masked), _lib.ptr(corrected_t),
                                             _lib.ptr(comps), _lib.ptr(mean)))
        outs.append({"masked": masked, "mask": mask.astype(bool), "corrected": np.ascontiguousarray(corrected_t.T), "comps": comps,
                     "mean": mean, "mbins": mbins.copy(), "bins": np.asarray(sizes, dtype=np.int64)})
        if between is not None:
            between()
    dev = torch.device("cuda", 0)
    masked_d = torch.empty((B, n_s), dtype=torch.float64, device=dev)
    corrected_d = torch.empty((B, n_s), dtype=torch.float64, device=dev)
    comps, mean = np.empty((n_comp, B)), np.empty(B)
    torch.cuda.synchronize()
    _lib.check(lib.wc_newref_prep_finish_dev(ctx, n_comp, _lib.ptr(evecs), _lib.ptr(evals), ctypes.c_void_p(masked_d.data_ptr()),
                                             ctypes.c_void_p(corrected_d.data_ptr()), _lib.ptr(comps), _lib.ptr(mean)))
    outs.append({"masked": masked_d.cpu().numpy(), "mask": mask.astype(bool), "corrected": corrected_d.cpu().numpy(), "comps": comps,
                 "mean": mean, "mbins": mbins.copy(), "bins": np.asarray(sizes, dtype=np.int64)})
    return outs


@pytest.mark.parametrize("between", ["test_general", "test_latency", "small_entries", "sensitivity"])
def test_prep_steps_with_test_path_calls_between(ctx, between):
    """The prep step's state is its own (include/wisecondor_hip.h): test-path calls between _gram, _eig and the finishes
    -- which used to overwrite the arrays _finish reads -- change nothing."""
    def other():
        agree(sq.BY_NAME[between].run(ctx, sq.LARGE), between, sq.LARGE, "between prep's steps")
    for out in _prep_steps(ctx, 8, other):
        _prep_agrees(out, 8)


def test_prep_finish_twice_and_without_gram(ctx, ctx2):
    """_finish is repeatable after one _gram, also with another component count; on a context that has never seen
    _gram, _eig and both finishes are refused with WC_E_ARG and write nothing."""
    from wisecondor_amd import _lib
    lib = _lib.load()
    for out in _prep_steps(ctx, 8, finishes=2):
        _prep_agrees(out, 8)
    for out in _prep_steps(ctx, 1, finishes=2):
        _prep_agrees(out, 1)
    evals, evecs = np.ones(1), np.ones((1, 40))
    outs = [np.full(16, 7.0) for _ in range(4)]
    for call in (lambda: lib.wc_newref_prep_eig(ctx2, 1, _lib.ptr(outs[0]), _lib.ptr(outs[1])),
                 lambda: lib.wc_newref_prep_finish(ctx2, 1, _lib.ptr(evecs), _lib.ptr(evals), *[_lib.ptr(o) for o in outs]),
                 lambda: lib.wc_newref_prep_finish_dev(ctx2, 1, _lib.ptr(evecs), _lib.ptr(evals), None, None, _lib.ptr(outs[2]),
                                                       _lib.ptr(outs[3]))):
        assert call() == _lib.E_ARG and b"wc_newref_prep_gram has not run" in lib.wc_last_error()
        assert all(np.all(o == 7.0) for o in outs)


@pytest.mark.parametrize("name", sq.NAMES)
def test_growth_orders(ctx, name):
    """SMALL, LARGE, SMALL, LARGE on one context: grown workspaces, then reused ones that are larger than the job."""
    for step, shape in enumerate((sq.SMALL, sq.LARGE, sq.SMALL, sq.LARGE)):
        agree(sq.BY_NAME[name].run(ctx, shape), name, shape, "step %d" % step)


def test_latency_graph_survives_a_closed_reference(ctx, capfd, monkeypatch):
    """A latency graph, reference.close(), a reference of another layout on the same context (its handle may get the freed
    one's address; the graph's key holds the reference's serial number), the latency job again."""
    import call_cases as cc
    import spike_cases as sc
    from wisecondor_amd import wisetools as wt
    agree(sq.run_test_latency(ctx, sq.LARGE), "test_latency", sq.LARGE)
    sq.close_references(ctx)
    lay = sc.lay()
    other = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], sc.base_samples()[0]["pca_mean"],
                         lay["pca_components"], binsize=cc.BINSIZE, ctx=ctx)
    try:
        row = (0,) + sc.ROWS[0][0]
        for _ in range(3):
            outs = wt.test_batch(other, [sc.spiked_sample(row)], cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS)
        got = np.asarray(outs[0]["results_calls"], dtype=np.float64).reshape(-1, 5)
        assert sq.same({"c": got}, {"c": np.array(sc.oracle_calls(row))}) is None, got
        monkeypatch.setenv("WC_TEST_VERBOSE", "1")
        capfd.readouterr()
        agree(sq.run_test_latency(ctx, sq.LARGE), "test_latency", sq.LARGE, "with the other reference open")
        agree(sq.run_test_latency(ctx, sq.SMALL), "test_latency", sq.SMALL, "with the other reference open")
        assert GENERAL_LINE not in capfd.readouterr().err
    finally:
        other.close()
    agree(sq.run_test_latency(ctx, sq.LARGE), "test_latency", sq.LARGE, "after the other reference was closed")


# ------------------------------------------------------------------ D2 every job after every other ----
@pytest.mark.parametrize("first", sq.NAMES)
def test_every_job_after(ctx, first):
    """On one context, for every job B: `first` (SMALL and LARGE in turn), then B (both shapes over the round), and B
    against its baseline."""
    for i, name in enumerate(sq.NAMES):
        a_shape, b_shape = sq.SHAPES[i % 2], sq.SHAPES[(i // 2) % 2]
        sq.BY_NAME[first].run(ctx, a_shape)
        agree(sq.BY_NAME[name].run(ctx, b_shape), name, b_shape, "after %s %s, pair %d of the round" % (first, a_shape, i))


# ------------------------------------------------------------------------------------ D3 seeded walks ----
def _walk(seed, contexts):
    steps = sq.walk_steps(seed)
    for i, (name, shape) in enumerate(steps):
        diff = sq.same(sq.BY_NAME[name].run(contexts[i % len(contexts)], shape), sq.baseline(name, shape))
        if diff is not None:
            listing = ", ".join("%d:%s/%s" % (k, n, s) for k, (n, s) in enumerate(steps[:i + 1]))
            raise AssertionError("walk %d on %d context(s): step %d (%s %s) differs from its baseline: %s\nthe steps so far: %s"
                                 % (seed, len(contexts), i, name, shape, diff, listing))


@pytest.mark.parametrize("seed", range(6 * SWEEP))
def test_seeded_walk(ctx, seed):
    _walk(seed, [ctx])


@pytest.mark.parametrize("seed", range(6 * SWEEP))
def test_seeded_walk_on_two_contexts(ctx, ctx2, seed):
    _walk(100 + seed, [ctx, ctx2])


# ------------------------------------------------------------------------------------ D4 steady state ----
@pytest.mark.parametrize("shape", sq.SHAPES)
@pytest.mark.parametrize("name", sq.NAMES)
def test_third_call_allocates_nothing(ctx, name, shape):
    """The header's promise: repeated calls of an unchanged shape only enqueue kernels."""
    job = sq.BY_NAME[name]
    job.run(ctx, shape)
    job.run(ctx, shape)
    before = sq.epoch()
    agree(job.run(ctx, shape), name, shape, "third call")
    assert sq.epoch() == before, (name, shape, before, sq.epoch())
