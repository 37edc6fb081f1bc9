"""The host's half of `sensitivity`: the plan maker, the table, the command line's options and refusals; and the rates the
oracle gives on the exact plan of the GPU tests' command line (test_sensitivity_gpu.py asserts them only because this
test has asked the oracle for them)."""
import math

import numpy as np
import pytest

import call_cases as cc
import spike_cases as sc
import spike_restated as sr
from oracle import wc_oracle as wo


@pytest.fixture(scope="module")
def se():
    from wisecondor_amd import sensitivity
    return sensitivity


@pytest.fixture(scope="module")
def ref():
    return cc.reference_of(sc.lay(), sc.base_samples()[0])


def test_same_seed_same_plan_another_seed_another(se, ref):
    a = se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=1)
    assert a.dtype == np.int32 and a.shape == (3 * (1 + 2 * 2 * 6), 5)
    assert np.array_equal(a, se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=1))
    assert not np.array_equal(a, se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=2))
    from wisecondor_amd import wisetools as wt
    assert np.array_equal(a, wt.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=1))


def test_placements_are_paired_and_every_sample_has_one_control(se, ref):
    effects = [2500000, -50000, 100000]
    plan = se.makePlan(ref, 3, [5, 7], effects, 6, seed=3)
    for b in range(3):
        mine = plan[plan[:, 0] == b]
        assert (mine[:, 4] == 0).sum() == 1 and mine[0, 4] == 0
        for bins in (5, 7):
            places = [mine[(mine[:, 3] == bins) & (mine[:, 4] == e)][:, 1:4] for e in effects]
            assert all(len(p) == 6 for p in places)
            assert all(np.array_equal(places[0], p) for p in places[1:])
    # the samples' placements differ (one stream of draws)
    assert not np.array_equal(plan[plan[:, 0] == 0][:, 1:], plan[plan[:, 0] == 1][:, 1:])


def test_every_span_fits_and_is_half_unmasked(se, ref):
    lay = sc.lay()
    plan = se.makePlan(ref, 2, [1, 2, 5, 9, 40, 41], [2500000], 40, seed=7)
    spiked = plan[plan[:, 4] != 0]
    for _, chrom, first, bins, _ in spiked.tolist():
        assert 0 <= first and first + bins <= lay["sizes"][chrom - 1]
        lo = lay["goff"][chrom - 1] + first
        assert lay["mask"][lo:lo + bins].sum() >= math.ceil(bins / 2)
    # 41 bins fit chromosomes 1, 2 (41 bins) and 3 (41 bins) alone; 150 only chromosome 1
    assert set(spiked[spiked[:, 3] == 41][:, 1].tolist()) <= {1, 2, 3}
    long_plan = se.makePlan(ref, 1, [42], [2500000], 30, seed=1)
    assert set(long_plan[long_plan[:, 4] != 0][:, 1].tolist()) == {1}
    # bins 12 .. 14 of chromosome 1 hold masked bin 13: a start at 13 with one bin is not valid, with two it is
    starts = se.validStarts(ref, 1, [1])[0]
    assert 13 not in starts and 12 in starts and 14 in starts
    assert 13 in se.validStarts(ref, 2, [1])[0]


def test_a_length_without_a_valid_start_is_refused_by_name(se, ref):
    with pytest.raises(ValueError, match="200 bins"):
        se.makePlan(ref, 2, [5, 200], [2500000], 3)
    with pytest.raises(ValueError, match="42 bins"):
        se.makePlan(ref, 2, [42], [2500000], 3, chromosomes=[2, 3, 4])
    with pytest.raises(ValueError, match="empty grid"):
        se.makePlan(ref, 2, [], [2500000], 3)
    with pytest.raises(ValueError, match="out of range"):
        se.makePlan(ref, 2, [5], [100000001], 3)
    with pytest.raises(ValueError, match="out of range"):
        se.makePlan(ref, 2, [5], [-1000001], 3)


def test_table_on_hand_written_records(se):
    # length 5: ceil(0.5 * 5) = 3; length 4: ceil(0.5 * 4) = 2
    plan = np.array([[0, 1, 0, 1, 0],
                     [0, 1, 10, 5, 50000], [0, 1, 20, 5, 50000], [0, 1, 30, 5, 50000], [0, 1, 40, 5, 50000],
                     [0, 1, 10, 4, 50000], [0, 1, 20, 4, 50000],
                     [0, 1, 10, 5, -50000],
                     [1, 2, 0, 1, 0]], dtype=np.int32)
    rec_i = np.array([[2, 0, 0, 0, -1, -1, -1, 0],
                      [1, 1, 3, 3, 0, 10, 12, 0],          # overlap 3 of 5: detected
                      [3, 1, 2, 9, 1, 16, 24, 0],          # overlap 2 of 5: not detected; two calls elsewhere
                      [0, 0, 0, 0, -1, -1, -1, 0],         # no call
                      [2, 2, 5, 6, 0, 38, 42, 0],          # two matching calls: detected
                      [1, 1, 2, 2, 0, 10, 11, 0],          # overlap 2 of 4: detected
                      [1, 1, 1, 1, 0, 20, 20, 0],          # overlap 1 of 4: not detected
                      [1, 1, 5, 5, 0, 10, 14, 0],
                      [1, 0, 0, 0, -1, -1, -1, 0]], dtype=np.int32)
    nan = float("nan")
    rec_f = np.array([[nan, nan], [6.0, 0.05], [5.5, 0.04], [nan, nan], [9.0, 0.07], [7.0, 0.06], [5.1, 0.03], [-8.0, -0.05],
                      [nan, nan]])
    table = se.sensitivityTable(plan, rec_i, rec_f, [5, 4], [50000, -50000], minoverlap=0.5)
    want = np.array([
        [5, 50000, 4, 2, 0.5, 7.5, 0.06, (3 / 5 + 2 / 12 + 0 + 5 / 6) / 4, 0.5],
        [5, -50000, 1, 1, 1.0, -8.0, -0.05, 1.0, 0.0],
        [4, 50000, 2, 1, 0.5, 7.0, 0.06, (2 / 4 + 1 / 4) / 2, 0.0],
        [4, -50000, 0, 0, nan, nan, nan, nan, nan],
        [0, 0, 2, 0, nan, nan, nan, nan, 1.5]])
    assert table.shape == want.shape == (5, len(se.TABLE_COLUMNS))
    assert np.allclose(table, want, rtol=1e-15, atol=0, equal_nan=True), table
    assert np.array_equal(table, sr.table(plan, rec_i, rec_f, [5, 4], [50000, -50000], 0.5), equal_nan=True)
    # 0.4 * 5 = 2 exactly: the second trial is detected too; 0.61 * 5 = 3.05 -> 4: the first no longer
    assert se.sensitivityTable(plan, rec_i, rec_f, [5], [50000], minoverlap=0.4)[0, 3] == 3
    assert se.sensitivityTable(plan, rec_i, rec_f, [5], [50000], minoverlap=0.61)[0, 3] == 1
    text = se.tableText(table)
    lines = text.strip("\n").split("\n")
    assert lines[0].split("\t") == list(se.TABLE_COLUMNS)
    back = np.array([[float(v) for v in line.split("\t")] for line in lines[1:]])
    assert np.array_equal(back, table, equal_nan=True)


def test_grid_of_the_command_line(se):
    assert se.parseGrid("1e6,5e6,20e6", "2.5,5,10,-2.5,-5,-10", 250000) == ([4, 20, 80], [25000, 50000, 100000, -25000, -50000, -100000])
    assert se.parseGrid("1", "-100,10000", 1e6) == ([1], [-1000000, 100000000])
    assert se.parseGrid("1000001", "0.00016,0.00014", 1e6) == ([2], [2, 1])     # ceil; round
    for lengths, effects in (("", "5"), ("5e6", ""), (",", "5"), ("5e6", "-100.01"), ("5e6", "10000.01"), ("5e6", "nan"),
                             ("0", "5"), ("x", "5"), ("5e6", "0")):
        with pytest.raises(ValueError):
            se.parseGrid(lengths, effects, 1e6)


def test_options_and_defaults():
    from wisecondor_amd import wisecondor as cli
    args = cli.buildParser().parse_args(["sensitivity", "a.npz", "b.npz", "out", "ref.npz", "-lengths", "1e6,5e6", "-effects", "2.5,-5"])
    assert args.func is cli.toolSensitivity
    assert (args.infiles, args.outfile, args.reference) == (["a.npz", "b.npz"], "out", "ref.npz")
    assert (args.lengths, args.effects, args.trials, args.seed, args.minoverlap, args.batch) == ("1e6,5e6", "2.5,-5", 20, 1, 0.5, 1024)
    test_args = cli.buildParser().parse_args(["test", "a.npz", "o.npz", "ref.npz"])
    for name in ("chromosomes", "minzscore", "multitest", "minrefbins", "repeats", "mineffectsize"):
        assert getattr(args, name) == getattr(test_args, name), name
    args = cli.buildParser().parse_args(["sensitivity", "a.npz", "out", "ref.npz", "-lengths", "1e6", "-effects=-5,5", "-trials", "3",
                                         "-seed", "9", "-minoverlap", "0.25", "-batch", "7", "-chromosomes", "1,2", "-minzscore", "5",
                                         "-repeats", "2"])
    assert (args.effects, args.trials, args.seed, args.minoverlap, args.batch, args.chromosomes, args.minzscore, args.repeats) == \
        ("-5,5", 3, 9, 0.25, 7, [1, 2], 5.0, 2)
    assert cli.sensitivityOutputs("x/out") == ("x/out.npz", "x/out.tsv") and cli.sensitivityOutputs("out.npz") == ("out.npz", "out.tsv")
    with pytest.raises(SystemExit) as stop:
        cli.buildParser().parse_args(["sensitivity", "a.npz", "out", "ref.npz", "-lengths", "1e6"])
    assert stop.value.code == 2


@pytest.mark.parametrize("options, word", [
    (["-lengths", ",", "-effects", "5"], "empty grid"),
    (["-lengths", "5e6", "-effects", "20000"], "out of range"),
    (["-lengths", "5e6", "-effects=-150"], "out of range"),
    (["-lengths", "5e6,200e6", "-effects", "5"], "200 bins"),
    (["-lengths", "5e6", "-effects", "5", "-trials", "0"], "-trials"),
    (["-lengths", "5e6", "-effects", "5", "-chromosomes", "23"], "chromosome 23"),
])
def test_refusals_exit_with_status_2(tmp_path, capsys, options, word):
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    with pytest.raises(SystemExit) as stop:
        cli.main(["sensitivity"] + paths[:2] + [str(tmp_path / "out"), ref_path] + options)
    assert stop.value.code == 2
    out = capsys.readouterr().out
    assert "ERROR:" in out and word in out, out
    assert not (tmp_path / "out.npz").exists() and not (tmp_path / "out.tsv").exists()


def test_a_sample_whose_bin_size_does_not_scale_is_refused(tmp_path, capsys):
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    odd = str(tmp_path / "odd.npz")
    np.savez_compressed(odd, arguments={"binsize": 300000.0}, runtime={}, sample=sc.cli_samples()[0]["counts"], quality={})
    with pytest.raises(SystemExit) as stop:
        cli.main(["sensitivity", paths[0], odd, str(tmp_path / "out"), ref_path, "-lengths", "5e6", "-effects", "5"])
    assert stop.value.code == 2
    out = capsys.readouterr().out
    assert "ERROR:" in out and "odd.npz" in out and "does not scale" in out


def test_oracle_rates_on_the_command_lines_exact_plan(se, ref):
    """The plan `sensitivity` makes for the GPU test's command line (four samples, -lengths 5e6,40e6 -effects 250,-100,10
    -trials 3, seed 1): at 5 bins the oracle detects every +250 % trial and no +10 % trial."""
    lay = sc.lay()
    plan = se.makePlan(ref, 4, sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, sc.CLI_TRIALS, seed=1)
    assert se.parseGrid(sc.CLI_LENGTHS_BP, sc.CLI_EFFECTS_PERCENT, cc.BINSIZE) == (sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM)
    rows = plan[(plan[:, 3] == 5) & np.isin(plan[:, 4], (2500000, 100000))]
    assert len(rows) == 4 * 3 * 2
    counts = np.stack([np.concatenate([s["counts"][str(c)] for c in range(1, 23)]) for s in sc.cli_samples()]).astype(np.int32)
    lists = []
    for row in rows:
        spiked = sr.spike(counts, lay["sizes"], row[None, :])[0][0]
        as_dict = {str(c + 1): spiked[lay["goff"][c]:lay["goff"][c + 1]] for c in range(22)}
        with np.errstate(all="ignore"):
            out = wo.test_sample(as_dict, cc.BINSIZE, ref, minzscore=cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS)
        lists.append(np.asarray(out["results_calls"], dtype=np.float64).reshape(-1, 5))
    rec_i, rec_f = sr.score_lists(rows, lists)
    table = se.sensitivityTable(rows, rec_i, rec_f, [5], [2500000, 100000])
    assert table[0, 2] == table[1, 2] == 12
    assert table[0, 4] == 1.0 and table[1, 4] == 0.0, table
