"""wt.sensitivity_batch with depths and the binomial spike, `sensitivity -depths -draw` and `downsample`, on the layout and
base samples of spike_cases.py as test_sensitivity_gpu.py uses them: the calls of the device route equal wt.test_batch
on samples thinned and spiked by the restatement (draw_restated.py) bit for bit, the records equal the restated score
of those calls, and neither the batch size nor the new entry point changes a bit of what ran before."""
import numpy as np
import pytest

import call_cases as cc
import draw_restated as dr
import spike_cases as sc
import spike_restated as sr

pytestmark = pytest.mark.gpu
DEPTHS = [1000000, 500000]
SEED = 1


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


@pytest.fixture(scope="module")
def reference(wt):
    lay = sc.lay()
    ref = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], sc.base_samples()[0]["pca_mean"],
                       lay["pca_components"], binsize=cc.BINSIZE)
    yield ref
    ref.close()


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 5)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 5)
    if a.shape != b.shape:
        return False
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def samples():
    return [s["counts"] for s in sc.base_samples()]


def depth_plan():
    """The designed plan once per depth, base rows d * 2 + b."""
    plan = sc.designed_plan()
    parts = []
    for d in range(len(DEPTHS)):
        part = plan.copy()
        part[:, 0] += 2 * d
        parts.append(part)
    return np.concatenate(parts)


def run(wt, reference, plan, **options):
    return wt.sensitivity_batch(reference, samples(), plan, cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS, **options)


ROUTE = {}


def route(wt, reference):
    """The depth plan through the device route, once per module, and the rows the restatement makes of it."""
    if not ROUTE:
        plan = depth_plan()
        rec_i, rec_f, calls = run(wt, reference, plan, keep_calls=True, depths_ppm=DEPTHS, draw=True, seed=SEED)
        sizes = sc.lay()["sizes"]
        image = dr.thin(sc.base_counts(), sizes, DEPTHS, SEED).reshape(len(DEPTHS) * 2, -1)
        spiked, _ = dr.spike_draw(image, sizes, plan, SEED, 0)
        ROUTE.update(plan=plan, rec_i=rec_i, rec_f=rec_f, calls=calls, image=image, spiked=spiked)
    return ROUTE


def test_calls_equal_the_host_route_on_restated_rows(wt, reference):
    got = route(wt, reference)
    plan, goff = got["plan"], sc.lay()["goff"]
    assert len(plan) == 40 and set(plan[:, 0].tolist()) == {0, 1, 2, 3}
    assert np.array_equal(got["image"][:2], sc.base_counts()) and (got["image"][2:] < got["image"][:2]).any()
    dicts = [{str(c + 1): row[goff[c]:goff[c + 1]].copy() for c in range(22)} for row in got["spiked"]]
    outs = wt.test_batch(reference, dicts, cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS)
    want = [np.asarray(o["results_calls"], dtype=np.float64).reshape(-1, 5) for o in outs]
    for i, row in enumerate(plan.tolist()):
        assert same_bits(got["calls"][i], want[i]), (row, got["calls"][i], want[i])
    assert sum(len(w) for w in want) >= 5               # the strong trials are still found: the comparison is of something


def test_records_equal_the_restated_score(wt, reference):
    got = route(wt, reference)
    want_i, want_f = sr.score_lists(got["plan"], got["calls"])
    assert np.array_equal(got["rec_i"], want_i)
    nan = np.isnan(want_f)
    assert np.array_equal(np.isnan(got["rec_f"]), nan)
    assert np.array_equal(got["rec_f"].view(np.int64)[~nan], want_f.view(np.int64)[~nan])


@pytest.mark.parametrize("batch", [1, 5])
def test_batches_give_the_same_records(wt, reference, batch):
    got = route(wt, reference)
    rec_i, rec_f = run(wt, reference, got["plan"], batch=batch, depths_ppm=DEPTHS, draw=True, seed=SEED)
    assert np.array_equal(rec_i, got["rec_i"])
    assert np.array_equal(rec_f.view(np.int64), got["rec_f"].view(np.int64))


def test_depths_without_draw_plant_the_deterministic_spike(wt, reference):
    got = route(wt, reference)
    plan = got["plan"]
    _, _, calls = run(wt, reference, plan, keep_calls=True, depths_ppm=DEPTHS, seed=SEED)
    spiked, _ = sr.spike(got["image"], sc.lay()["sizes"], plan)
    goff = sc.lay()["goff"]
    dicts = [{str(c + 1): row[goff[c]:goff[c + 1]].copy() for c in range(22)} for row in spiked]
    outs = wt.test_batch(reference, dicts, cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS)
    for i in range(len(plan)):
        assert same_bits(calls[i], outs[i]["results_calls"]), plan[i]


def test_without_the_new_arguments_nothing_changes(wt, reference):
    """sensitivity_batch as it always was called (the first entry point) against the _ex entry point with draw = 0 and a
    seed and an offset that must not matter."""
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    plan = sc.designed_plan()
    rec_i, rec_f, calls = run(wt, reference, plan, keep_calls=True)
    sizes = np.ascontiguousarray(reference.chromosome_sizes, dtype=np.int64)
    sel = np.arange(1, 23, dtype=np.int32)
    base = torch.from_numpy(wt.samples_to_counts(samples(), [int(v) for v in sizes])).cuda()
    n, room = len(plan), wt.MAX_CALLS
    ri = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    rf = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    dc_ = torch.empty((n, room, 5), dtype=torch.float64, device="cuda")
    dn = torch.empty((n,), dtype=torch.int32, device="cuda")
    rc = lib.wc_sensitivity_batch_ex_dev(reference.ctx, torch.cuda.current_stream().cuda_stream, reference.handle, base.data_ptr(), 2,
                                         _lib.ptr(sizes), len(sizes), _lib.ptr(plan), n, 0, 0x123456789, 5, float(cc.THR), cc.MINREF, cc.REPEATS,
                                         0.0, _lib.ptr(sel), len(sel), room, ri.data_ptr(), rf.data_ptr(), dc_.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.wc_last_error()
    assert np.array_equal(ri.cpu().numpy(), rec_i)
    assert np.array_equal(rf.cpu().numpy().view(np.int64), rec_f.view(np.int64))
    counts, rows = dn.cpu().numpy(), dc_.cpu().numpy()
    for i in range(n):
        assert same_bits(rows[i, :counts[i]], calls[i])


def test_command_line_with_depths_and_draw(wt, tmp_path, capsys):
    from wisecondor_amd import sensitivity
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    options = ["-lengths", sc.CLI_LENGTHS_BP, "-effects", sc.CLI_EFFECTS_PERCENT, "-trials", str(sc.CLI_TRIALS), "-minzscore", "5",
               "-repeats", "2"]
    cli.main(["sensitivity"] + paths + [str(tmp_path / "out"), ref_path] + options + ["-depths", "1,0.5", "-draw"])
    printed = capsys.readouterr().out
    out = np.load(str(tmp_path / "out.npz"), allow_pickle=True)
    assert sorted(out.files) == sorted(["arguments", "runtime", "binsize", "threshold_z", "samples", "lengths_bins", "effects_ppm",
                                        "plan", "rec_i", "rec_f", "table", "depths_ppm", "draw"])
    per_depth = 4 * (1 + 2 * 3 * 3)
    assert out["plan"].shape == (2 * per_depth, 5) and out["depths_ppm"].tolist() == [1000000, 500000] and bool(out["draw"])
    assert out["arguments"].item()["depths"] == "1,0.5" and out["arguments"].item()["draw"] is True
    reference = cc.reference_of(sc.lay(), sc.cli_samples()[0])
    plan = sensitivity.makePlan(reference, 4, sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, 3, seed=1, n_depths=2)
    assert np.array_equal(out["plan"], plan)
    lines_per_depth = 2 * 3 + 1
    table = out["table"]
    assert table.shape == (2 * lines_per_depth, 1 + len(sensitivity.TABLE_COLUMNS))
    assert table[:, 0].tolist() == [1000000.0] * lines_per_depth + [500000.0] * lines_per_depth
    for d in range(2):
        rows = out["plan"][:, 0] // 4 == d
        block = sr.table(out["plan"][rows], out["rec_i"][rows], out["rec_f"][rows], sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, 0.5)
        assert np.array_equal(table[d * lines_per_depth:(d + 1) * lines_per_depth, 1:], block, equal_nan=True)
        assert table[(d + 1) * lines_per_depth - 1, 1:4].tolist() == [0, 0, 4]          # the depth's control line
    lines = open(str(tmp_path / "out.tsv")).read().strip("\n").split("\n")
    assert lines[0].split("\t") == [sensitivity.DEPTH_COLUMN] + list(sensitivity.TABLE_COLUMNS)
    assert np.array_equal(np.array([[float(v) for v in line.split("\t")] for line in lines[1:]]), table, equal_nan=True)
    assert "\n".join(lines) in printed
    # the records are those of the library's route on the same plan
    from wisecondor_amd import ingest
    stored = wt.Reference.from_npz(np.load(ref_path, allow_pickle=True))
    try:
        smp = [ingest.read_sample(path, stored.binsize)[0] for path in paths]
        rec_i, rec_f = wt.sensitivity_batch(stored, smp, plan, 5.0, minrefbins=25, repeats=2, depths_ppm=[1000000, 500000], draw=True, seed=1,
                                            batch=7)
    finally:
        stored.close()
    assert np.array_equal(out["rec_i"], rec_i) and np.array_equal(out["rec_f"].view(np.int64), rec_f.view(np.int64))
    for bad in ("0", "1.5", "-0.5", "abc", "1e-9", "0.5,0.5", ",".join(["0.%d" % i for i in range(1, 10)]), ""):
        with pytest.raises(SystemExit) as err:
            cli.main(["sensitivity"] + paths + [str(tmp_path / "refused"), ref_path] + options + ["-depths=" + bad])
        assert err.value.code == 2, bad
        assert "ERROR:" in capsys.readouterr().out
    assert not (tmp_path / "refused.npz").exists()


def test_downsample(wt, tmp_path, capsys):
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    counts = sc.cli_samples()[0]["counts"]
    quality = {"mapped": 12, "unmapped": 3, "no_coordinate": 0, "filter_rmdup": 1, "filter_mapq": 2, "pre_retro": 9, "post_retro": 8}
    src = str(tmp_path / "whole.npz")
    np.savez_compressed(src, arguments={"binsize": float(cc.BINSIZE), "retdist": 4}, runtime={}, sample=counts, quality=quality)
    total = int(sum(int(v.sum()) for v in counts.values()))

    def want_of(keep_ppm, seed):
        return {key: dr.draw_segment(np.asarray(v, dtype=np.int64), 0, int(key), dr.TAG_THIN, 0, seed, [keep_ppm])[0] for key, v in counts.items()}

    half = str(tmp_path / "half.npz")
    cli.main(["downsample", src, half, "-fraction", "0.5", "-seed", "3"])
    got = np.load(half, allow_pickle=True)
    assert sorted(got.files) == ["arguments", "quality", "runtime", "sample"]
    want = want_of(500000, 3)
    sample = got["sample"].item()
    assert sorted(sample) == sorted(counts)
    for key in counts:
        assert sample[key].dtype == np.asarray(counts[key]).dtype and np.array_equal(sample[key], want[key]), key
    kept = int(sum(int(v.sum()) for v in want.values()))
    assert got["quality"].item() == dict(quality, downsampled=kept)
    assert abs(kept - total / 2) < 6 * np.sqrt(total / 4)
    assert got["arguments"].item() == {"binsize": float(cc.BINSIZE), "retdist": 4, "fraction": 0.5, "seed": 3}
    # -reads N: whole ppm of the file's total
    some = str(tmp_path / "some.npz")
    cli.main(["downsample", src, some, "-reads", str(total // 3)])
    ppm = (total // 3) * 1000000 // total
    want = want_of(ppm, 1)
    got = np.load(some, allow_pickle=True)
    assert all(np.array_equal(got["sample"].item()[key], want[key]) for key in counts)
    assert got["arguments"].item()["reads"] == total // 3 and "fraction" not in got["arguments"].item()
    # more reads than there are: a copy
    cli.main(["downsample", src, some, "-reads", str(total * 2)])
    assert all(np.array_equal(np.load(some, allow_pickle=True)["sample"].item()[key], counts[key]) for key in counts)
    capsys.readouterr()
    # the output is a converted sample like any other: `test` and `report` take it
    result = str(tmp_path / "half_test.npz")
    with pytest.raises(SystemExit) as done:                           # (`test` ends with status 0, as upstream does)
        cli.main(["test", half, result, ref_path, "-minzscore", "5", "-repeats", "2"])
    assert done.value.code == 0
    assert "results_calls" in np.load(result, allow_pickle=True).files
    cli.main(["report", half, result])
    assert "Reads out:" in capsys.readouterr().out
    for bad in (["-fraction", "0"], ["-fraction", "1.5"], ["-fraction", "1e-9"], ["-reads", "0"], ["-reads", "-4"], [],
                ["-fraction", "0.5", "-reads", "7"]):
        with pytest.raises(SystemExit) as err:
            cli.main(["downsample", src, str(tmp_path / "refused.npz")] + bad)
        assert err.value.code == 2, bad
    assert not (tmp_path / "refused.npz").exists()
