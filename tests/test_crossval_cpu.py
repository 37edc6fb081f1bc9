"""The host half of `crossval` (wisecondor_amd/crossval.py) and the sub-command's refusals: nothing here needs a GPU."""
import numpy as np
import pytest

import crossval_cases as cc


@pytest.fixture(scope="module")
def cv():
    from wisecondor_amd import crossval
    return crossval


def test_fold_sizes_differ_by_one_at_most(cv):
    for n, folds in ((13, 4), (100, 10), (101, 10), (9, 2), (200, 7)):
        plan = cv.foldPlan(n, folds, seed=3)
        assert plan.dtype == np.int32 and plan.shape == (n,)
        sizes = np.bincount(plan, minlength=folds)
        assert len(sizes) == folds and sizes.max() - sizes.min() <= 1 and sizes.sum() == n


def test_leave_one_out_is_the_identity_whatever_the_seed(cv):
    assert cv.foldPlan(13, 13, seed=1).tolist() == list(range(13))
    assert cv.foldPlan(13, 13, seed=99).tolist() == list(range(13))


def test_same_seed_same_plan_and_the_rule(cv):
    assert np.array_equal(cv.foldPlan(50, 5, seed=4), cv.foldPlan(50, 5, seed=4))
    assert not np.array_equal(cv.foldPlan(50, 5, seed=4), cv.foldPlan(50, 5, seed=5))
    perm = np.random.RandomState(4).permutation(50)
    plan = cv.foldPlan(50, 5, seed=4)
    assert [int(plan[perm[j]]) for j in range(50)] == [j % 5 for j in range(50)]


@pytest.mark.parametrize("n, folds, word", [(13, 1, "two at least"), (13, 0, "two at least"), (13, 14, "14 folds of 13"),
                                            (5, 2, "leave 2 training"), (6, 2, "leave 3 training"), (4, 4, "leave 3 training"),
                                            (8200, 2, "the GPU prep takes 4096"), (4098, 4098, "leave 4097 training")])
def test_fold_plans_that_are_refused(cv, n, folds, word):
    with pytest.raises(ValueError, match=word):
        cv.foldPlan(n, folds)


def test_the_limits_themselves_pass(cv):
    assert len(cv.foldPlan(5, 5)) == 5                      # four training samples
    assert len(cv.foldPlan(8, 2)) == 8
    assert len(cv.foldPlan(4097, 4097)) == 4097             # 4 096 training samples


def test_windows_of_the_command_line(cv):
    assert cv.parseWindows("1,2,5,10,20,50,100") == [1, 2, 5, 10, 20, 50, 100] == list(cv.DEFAULT_WINDOWS)
    assert cv.parseWindows(",".join(str(v) for v in range(1, 17))) == list(range(1, 17))
    for bad in ("", "0,1", "2,2", "3,2", "1,x", "1.5", ",".join(str(v) for v in range(1, 18)), "-1"):
        with pytest.raises(ValueError):
            cv.parseWindows(bad)


def test_quantile_of_a_histogram(cv):
    hist = np.zeros(130, dtype=np.int64)
    hist[65] = 100                                          # [0, 0.25): uniform inside the slot
    assert cv.histQuantile(hist, 0.5) == 0.125 and cv.histQuantile(hist, 0.1) == pytest.approx(0.025)
    hist[61] = 100                                          # [-1, -0.75)
    assert cv.histQuantile(hist, 0.25) == -0.875 and cv.histQuantile(hist, 0.75) == 0.125
    assert cv.histQuantile(hist, 0.5) == -0.75              # the count is reached at the slot's upper edge
    assert np.isnan(cv.histQuantile(np.zeros(130, dtype=np.int64), 0.5))
    hist[0] = 100
    assert np.isnan(cv.histQuantile(hist, 0.1587)) and cv.histQuantile(hist, 0.8413) == pytest.approx(0.25 * 0.5239)
    hist[129] = 1000
    assert np.isnan(cv.histQuantile(hist, 0.8413))


def test_windows_table_and_text_from_fixed_arrays(cv):
    from scipy.stats import norm
    windows = [1, 4, 9]
    win_n = np.array([[30, 10, 0], [70, 30, 0]], dtype=np.int64)
    win_i = np.array([[4, 100, 3, 1], [3, 40, 2, 0], [0, 0, 0, 0]], dtype=np.int64)
    hist = np.zeros((3, 130), dtype=np.int64)
    hist[0, 61], hist[0, 68] = 50, 50                       # half in [-1, -0.75), half in [0.75, 1)
    hist[1, 0], hist[1, 65] = 20, 20                        # the lower quantile falls into the open end
    table = cv.windowsTable(windows, win_n, win_i, hist, [3.0, 4.0])
    assert table.shape == (3, len(cv.WINDOW_COLUMNS))
    assert table[0, :5].tolist() == [1, 4, 100, 3, 1] and table[0, 5] == 0.04
    assert table[0, 6] == pytest.approx((30 * 2 * norm.sf(3.0) + 70 * 2 * norm.sf(4.0)) / 100, rel=1e-14)
    low, high = -1.0 + 0.25 * 15.87 / 50, 0.75 + 0.25 * (84.13 - 50) / 50
    assert table[0, 7] == pytest.approx((high - low) / 2, rel=1e-12)
    assert table[1, :6].tolist() == [4, 3, 40, 2, 0, 0.05] and np.isnan(table[1, 7]) and not np.isnan(table[1, 6])
    assert table[2, :5].tolist() == [9, 0, 0, 0, 0] and np.isnan(table[2, 5:]).all()
    text = cv.windowsText(table)
    lines = text.strip("\n").split("\n")
    assert lines[0].split("\t") == list(cv.WINDOW_COLUMNS) and text.endswith("\n") and len(lines) == 4
    assert lines[1].split("\t")[:6] == ["1", "4", "100", "3", "1", "0.04"] and lines[3].split("\t")[5:] == ["nan", "nan", "nan"]
    back = np.array([[float(v) for v in line.split("\t")] for line in lines[1:]])
    assert np.array_equal(back, table, equal_nan=True)


def test_samples_text_from_fixed_records(cv):
    rec_i = np.array([[2, 1, 700, 0, 3, 4, 12, 0], [0, 0, 650, 1, 0, 0, 0, 1]], dtype=np.int32)
    rec_f = np.array([[0.1, 5.0, 7.25, -6.5], [0.3, 5.0, np.nan, np.nan]])
    lines = cv.samplesText(["a.npz", "b.npz"], rec_i, rec_f).strip("\n").split("\n")
    assert lines[0].split("\t") == list(cv.SAMPLE_COLUMNS)
    assert lines[1].split("\t") == ["a.npz", "2", "1", "12", "700", "3", "4", "0.1", "7.25", "-6.5"]
    assert lines[2].split("\t") == ["b.npz", "0", "0", "0", "650", "0", "0", "0.3", "nan", "nan"]
    with pytest.raises(ValueError):
        cv.samplesText(["a.npz"], rec_i, rec_f)


def test_options_and_defaults():
    from wisecondor_amd import wisecondor as cli
    args = cli.buildParser().parse_args(["crossval", "a.npz", "b.npz", "c.npz", "d.npz", "e.npz", "out"])
    assert args.func is cli.toolCrossval and args.infiles == ["a.npz", "b.npz", "c.npz", "d.npz", "e.npz"] and args.outfile == "out"
    assert (args.folds, args.loo, args.seed, args.refsize, args.binsize, args.windows, args.results) == \
        (10, False, 1, 100, None, "1,2,5,10,20,50,100", None)
    assert (args.minzscore, args.multitest, args.minrefbins, args.repeats, args.mineffectsize) == (None, 1000, 25, 5, 0)
    assert args.chromosomes == list(range(1, 23))
    assert cli.buildParser().parse_args(["crossval", "a.npz", "out", "-loo"]).loo is True
    with pytest.raises(SystemExit) as stop:
        cli.buildParser().parse_args(["crossval", "a.npz", "out", "-loo", "-folds", "3"])
    assert stop.value.code == 2
    assert cli.crossvalOutputs("x/out") == ("x/out.npz", "x/out_samples.tsv", "x/out_windows.tsv") == cli.crossvalOutputs("x/out.npz")


@pytest.mark.parametrize("files, options, word", [
    (4, ["-loo"], "5 healthy samples"),
    (13, ["-folds", "1"], "two at least"),
    (13, ["-folds", "14"], "14 folds of 13"),
    (6, ["-folds", "2"], "training samples"),
    (13, ["-loo", "-windows", "2,1"], "ascending"),
    (13, ["-loo", "-windows", ""], "window lengths"),
    (13, ["-loo", "-windows", "1,two"], "whole numbers"),
    (13, ["-loo", "-binsize", "1500000"], "does not scale"),
    (13, ["-loo", "-refsize", "0"], "-refsize >= 1"),
])
def test_refusals_exit_with_status_2_before_the_library_is_loaded(tmp_path, capsys, monkeypatch, files, options, word):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisecondor as cli

    def no_library():
        raise AssertionError("a refusal loaded the library")
    monkeypatch.setattr(_lib, "load", no_library)
    paths = cc.write_cli_files(tmp_path)[:files]
    with pytest.raises(SystemExit) as stop:
        cli.main(["crossval"] + paths + [str(tmp_path / "out")] + options)
    assert stop.value.code == 2
    out = capsys.readouterr().out
    assert "ERROR:" in out and word in out
    assert not (tmp_path / "out.npz").exists()


def test_samples_binned_at_different_sizes_are_refused(tmp_path, capsys, monkeypatch):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisecondor as cli
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("a refusal loaded the library")))
    paths = cc.write_cli_files(tmp_path)
    odd = str(tmp_path / "odd.npz")
    np.savez_compressed(odd, arguments={"binsize": 300000.0}, runtime={}, sample=cc.samples()[0], quality={})
    for options, word in (([], "different sizes"), (["-binsize", "1000000"], "does not scale")):
        with pytest.raises(SystemExit) as stop:
            cli.main(["crossval", "-loo"] + paths[:6] + [odd, str(tmp_path / "out")] + options)
        assert stop.value.code == 2
        assert word in capsys.readouterr().out
