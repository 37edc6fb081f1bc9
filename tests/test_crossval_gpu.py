"""crossval.crossval_batch and the `crossval` sub-command on the designed cohort of crossval_cases.py (held on the CPU by
test_crossval_cases_cpu.py): every held-out sample's results equal, bit for bit, what the public host-array route gives
for its fold's training samples, the statistics equal the restatement of the returned rows, and neither the order of
the folds nor the way the fold count is given changes a bit."""
import os

import numpy as np
import pytest

import crossval_cases as cc
import crossval_restated as cr

pytestmark = pytest.mark.gpu
OPTIONS = dict(refsize=cc.REFSIZE, minzscore=cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS, windows=cc.WINDOWS)
CLI_OPTIONS = ["-refsize", str(cc.REFSIZE), "-minzscore", str(cc.THR), "-minrefbins", str(cc.MINREF), "-repeats", str(cc.REPEATS)]
ONCE = int(cc.OFFS[cc.ONCE_CHROM - 1] + cc.ONCE_BIN)
RUNS, ROUTE, CLI = {}, {}, {}


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.int64(-1), a.view(np.int64))


def batch(fold_of):
    """crossval_batch on the cohort under a fold plan, once per plan."""
    from wisecondor_amd import crossval
    key = tuple(int(v) for v in fold_of)
    if key not in RUNS:
        RUNS[key] = crossval.crossval_batch(cc.counts(), cc.SIZES, np.array(fold_of, dtype=np.int32), cc.BINSIZE, keep_results=True, **OPTIONS)
    return RUNS[key]


def plan(folds):
    from wisecondor_amd import crossval
    return crossval.foldPlan(cc.N, folds, seed=1)


def public_route(training, held):
    """wt.prepReference (host form) -> wt.getReference -> wt.Reference -> wt.test_batch for one fold: (the fold's mask,
    the test_batch dicts of `held`), once per fold."""
    from wisecondor_amd import wisetools as wt
    key = (tuple(training), tuple(held))
    if key not in ROUTE:
        _, chrom_bins, mask, corrected, components, mean, masked_sizes = wt.prepReference([cc.samples()[i] for i in training])
        assert chrom_bins == cc.SIZES
        indexes, distances = wt.getReference(corrected, masked_sizes, np.cumsum(masked_sizes), selectRefAmount=cc.REFSIZE)
        reference = wt.Reference(indexes, distances, chrom_bins, masked_sizes, mask, mean, components, binsize=cc.BINSIZE)
        outs = wt.test_batch(reference, [cc.samples()[i] for i in held], cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS)
        ROUTE[key] = (np.asarray(mask).astype(bool), outs, reference.cutoff)
        reference.close()
    return ROUTE[key]


@pytest.mark.parametrize("folds", [13, 4])
def test_every_held_out_row_equals_the_public_route(folds):
    fold_of = plan(folds)
    got = batch(fold_of)
    assert got["Z"].shape == got["R"].shape == (cc.N, cc.N_TOTAL) and got["results_cwz"].shape == (cc.N, 22)
    assert got["threshold"].tolist() == [cc.THR] * folds and got["fold_of"].tolist() == fold_of.tolist()
    for fold in range(folds):
        held = [i for i in range(cc.N) if fold_of[i] == fold]
        mask, outs, cutoff = public_route(cc.training_of(fold_of, fold), held)
        assert got["cutoff"][fold] == cutoff
        for i, want in zip(held, outs):
            assert np.array_equal(bits(got["Z"][i]), bits(np.concatenate(want["results_z"]))), i
            assert np.array_equal(bits(got["R"][i]), bits(np.concatenate(want["results_r"]))), i
            assert np.array_equal(bits(got["results_cwz"][i]), bits(want["results_cwz"])), i
            mine = got["calls"][got["calls"][:, 0] == i, 1:]
            assert np.array_equal(bits(mine), bits(np.asarray(want["results_calls"], dtype=np.float64).reshape(-1, 5))), i
            assert bits(got["rec_f"][i, 0]) == bits(want["asdef"]), i
            assert got["rec_i"][i, 0] == fold and got["rec_i"][i, 1] == len(mine)


def test_leave_one_out_finds_what_the_oracle_finds():
    got = batch(plan(13))
    assert got["rec_i"][:, 1].tolist() == cc.LOO_CALLS
    assert np.isfinite(got["Z"]).all() and got["rec_i"][:, 3].sum() == 0 and got["rec_i"][:, 7].sum() == 0


def test_the_once_bin_is_masked_in_one_fold_only():
    """The fold that holds ONCE_SAMPLE out masks the bin; every other fold keeps it in its mask, and there the test path
    removes it (minrefbins), so its z is the 0.0 fill in every row (crossval_cases.py says why)."""
    fold_of = plan(13)
    got = batch(fold_of)
    for fold in range(13):
        mask, _, _ = public_route(cc.training_of(fold_of, fold), [fold])
        assert bool(mask[ONCE]) == (fold != cc.ONCE_SAMPLE)
    assert got["Z"][cc.ONCE_SAMPLE, ONCE] == 0.0 and got["R"][cc.ONCE_SAMPLE, ONCE] == 0.0
    assert (got["Z"][:, ONCE] == 0.0).all() and got["bins_i"][ONCE].tolist() == [0, 0, 0, 0, 0, 0]


def restated(got):
    n_calls = got["rec_i"][:, 1].astype(np.int32)
    calls = np.full((cc.N, max(1, int(n_calls.max())), 5), np.nan)
    for i in range(cc.N):
        calls[i, :n_calls[i]] = got["calls"][got["calls"][:, 0] == i, 1:]
    want = cr.stats(got["Z"], cc.SIZES, got["threshold"][got["fold_of"]], got["rec_f"][:, 0], calls, n_calls, lengths=cc.WINDOWS)
    want["rec_i"][:, 0] = got["fold_of"]
    return want


@pytest.mark.parametrize("folds", [13, 4])
def test_statistics_equal_the_restatement_of_the_returned_rows(folds):
    got = batch(plan(folds))
    assert cr.same(got, restated(got)) is None, cr.same(got, restated(got))
    assert got["win_i"][0, 0] == cc.N * 22 and got["win_i"][-1, 1] == 0          # no chromosome has 100 tested bins
    assert got["win_i"][0, 1] == got["rec_i"][:, 2].sum() == got["bins_i"][:, 0].sum()


def test_renumbering_the_folds_changes_no_bit():
    fold_of = plan(4)
    other = np.array([2, 0, 3, 1], dtype=np.int32)[fold_of]
    a, b = batch(fold_of), batch(other)
    for key in ("Z", "R", "results_cwz", "calls", "rec_f", "bins_i", "bins_f", "win_n", "win_i", "win_hist"):
        assert np.array_equal(bits(a[key]) if a[key].dtype == np.float64 else a[key], bits(b[key]) if b[key].dtype == np.float64 else b[key]), key
    assert np.array_equal(a["rec_i"][:, 1:], b["rec_i"][:, 1:]) and b["rec_i"][:, 0].tolist() == other.tolist()
    assert np.array_equal(bits(a["cutoff"]), bits(b["cutoff"][[2, 0, 3, 1]]))


def test_the_planted_sample_alone_is_called_on_its_span():
    got = batch(plan(13))
    lo, hi = cc.PLANTED_SPAN
    on_span = [c for c in got["calls"] if c[1] == cc.PLANTED_CHROM and c[2] <= hi and c[3] >= lo]
    assert len(on_span) == 1 and on_span[0][0] == cc.PLANTED and tuple(on_span[0][1:4]) == (cc.PLANTED_CHROM, lo, hi)
    first = int(cc.OFFS[cc.PLANTED_CHROM - 1])
    assert got["bins_i"][first + lo:first + hi + 1, 4].tolist() == [1] * (hi - lo + 1)
    assert got["bins_i"][first + lo:first + hi + 1, 5].tolist() == [0] * (hi - lo + 1)
    assert got["bins_i"][:, 4].sum() + got["bins_i"][:, 5].sum() == got["rec_i"][:, 6].sum()


def test_a_fold_with_more_calls_than_the_room_is_run_again(monkeypatch):
    from wisecondor_amd import crossval
    want = batch(plan(13))
    assert want["rec_i"][:, 1].max() == 3
    monkeypatch.setattr(crossval, "MAX_CALLS", 1)
    got = crossval.crossval_batch(cc.counts(), cc.SIZES, plan(13), cc.BINSIZE, **OPTIONS)
    for key in ("calls", "rec_f", "bins_f"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    for key in ("rec_i", "bins_i", "win_n", "win_i", "win_hist"):
        assert np.array_equal(got[key], want[key]), key
    assert "Z" not in got


# ------------------------------------------------------------------------------------------- the command line ----
def command_line(folder_factory):
    """`crossval -loo -results` and `crossval -folds 13` on the thirteen files, once per module."""
    if not CLI:
        from wisecondor_amd import wisecondor as cli
        folder = folder_factory.mktemp("crossval_cli")
        paths = cc.write_cli_files(folder)
        cli.main(["crossval"] + paths + [str(folder / "out"), "-loo", "-results", str(folder / "held")] + CLI_OPTIONS)
        cli.main(["crossval"] + paths + [str(folder / "folds13.npz"), "-folds", "13"] + CLI_OPTIONS)
        CLI.update(folder=folder, paths=paths)
    return CLI


def test_command_line_files(tmp_path_factory):
    from wisecondor_amd import crossval
    run = command_line(tmp_path_factory)
    folder, paths = run["folder"], run["paths"]
    out = np.load(str(folder / "out.npz"), allow_pickle=True)
    shapes = dict(fold_of=(13,), threshold=(13,), cutoff=(13,), rec_i=(13, 8), rec_f=(13, 4), bins_i=(cc.N_TOTAL, 6), bins_f=(cc.N_TOTAL, 2),
                  win_n=(13, 7), win_i=(7, 4), win_hist=(7, 130), samples=(13,), chromosome_sizes=(22,), windows=(7,))
    assert sorted(out.files) == sorted(list(shapes) + ["arguments", "runtime", "binsize", "calls"])
    for key, shape in shapes.items():
        assert out[key].shape == shape, key
    assert out["calls"].shape == (sum(cc.LOO_CALLS), 6) and out["samples"].tolist() == paths
    assert out["chromosome_sizes"].tolist() == cc.SIZES and out["windows"].tolist() == list(cc.WINDOWS) and float(out["binsize"]) == cc.BINSIZE
    assert out["arguments"].item()["loo"] is True and out["arguments"].item()["refsize"] == cc.REFSIZE
    want = batch(plan(13))
    for key in ("rec_i", "bins_i", "win_n", "win_i", "win_hist", "fold_of"):
        assert np.array_equal(out[key], want[key]), key
    for key in ("rec_f", "bins_f", "calls", "threshold", "cutoff"):
        assert np.array_equal(bits(out[key]), bits(want[key])), key
    # -loo equals -folds 13
    same = np.load(str(folder / "folds13.npz"), allow_pickle=True)
    for key in shapes:
        if key != "samples":
            assert np.array_equal(bits(out[key]) if out[key].dtype == np.float64 else out[key],
                                  bits(same[key]) if same[key].dtype == np.float64 else same[key]), key
    assert np.array_equal(bits(out["calls"]), bits(same["calls"]))
    # the tables parse back to the arrays
    lines = open(str(folder / "out_samples.tsv")).read().strip("\n").split("\n")
    assert lines[0].split("\t") == list(crossval.SAMPLE_COLUMNS) and len(lines) == 14
    for i, line in enumerate(lines[1:]):
        cells = line.split("\t")
        assert cells[0] == os.path.basename(paths[i])
        assert [int(v) for v in cells[1:7]] == [int(out["rec_i"][i, k]) for k in (0, 1, 6, 2, 4, 5)]
        assert np.array_equal(bits([float(v) for v in cells[7:]]), bits(out["rec_f"][i, [0, 2, 3]]))
    lines = open(str(folder / "out_windows.tsv")).read().strip("\n").split("\n")
    assert lines[0].split("\t") == list(crossval.WINDOW_COLUMNS) and len(lines) == 8
    table = crossval.windowsTable(list(cc.WINDOWS), out["win_n"], out["win_i"], out["win_hist"], out["rec_f"][:, 1])
    assert np.array_equal(bits([[float(v) for v in line.split("\t")] for line in lines[1:]]), bits(table))
    assert np.array_equal(table[:, 1:5], out["win_i"]) and np.isnan(table[-1, 5:]).all() and 0.5 < table[0, 7] < 2.0


@pytest.mark.parametrize("i", range(cc.N))
def test_held_out_result_files_equal_testbatch_on_a_reference_of_the_others(tmp_path_factory, tmp_path, capsys, i):
    from wisecondor_amd import wisecondor as cli
    run = command_line(tmp_path_factory)
    held = str(run["folder"] / "held" / ("healthy_%02d_test.npz" % i))
    others = [p for k, p in enumerate(run["paths"]) if k != i]
    reference = str(tmp_path / "reference.npz")
    cli.main(["newref"] + others + [reference, "-refsize", str(cc.REFSIZE)])
    cli.main(["testbatch", run["paths"][i], str(tmp_path / "single"), reference, "-minzscore", str(cc.THR), "-minrefbins", str(cc.MINREF),
              "-repeats", str(cc.REPEATS)])
    got = np.load(held, allow_pickle=True)
    want = np.load(str(tmp_path / "single" / ("healthy_%02d_test.npz" % i)), allow_pickle=True)
    for key in ("results_z", "results_r"):
        assert len(got[key]) == len(want[key]) == 22
        for a, b in zip(got[key], want[key]):
            assert np.array_equal(bits(a), bits(b)), key
    for key in ("results_cwz", "results_calls", "threshold_z", "asdef", "aasdef", "binsize"):
        assert np.shape(got[key]) == np.shape(want[key]) and np.array_equal(bits(got[key]), bits(want[key])), key
    capsys.readouterr()
    cli.main(["report", run["paths"][i], held])                 # the file loads through `report`
    assert capsys.readouterr().out.strip()
