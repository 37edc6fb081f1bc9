"""wt.sensitivity_batch and the `sensitivity` sub-command on the designed trials of spike_cases.py (held on the CPU by
test_spike_cases_cpu.py and test_sensitivity_cpu.py): the calls of the device route equal wt.test_batch on host-spiked
samples bit for bit and the oracle's rows for the designed trials, the records equal the restated score of those calls,
and batching changes nothing."""
import numpy as np
import pytest

import call_cases as cc
import spike_cases as sc
import spike_restated as sr

pytestmark = pytest.mark.gpu
TWO_CALLS = (0, 22, 0, 32, 400000)       # a gain on the bins chromosome 9 refers to: a call on 22 and a loss call on 9


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


def run(wt, reference, plan, **options):
    return wt.sensitivity_batch(reference, samples(), plan, cc.THR, minrefbins=cc.MINREF, repeats=cc.REPEATS, **options)


def host_route(wt, reference, plan):
    """wt.test_batch on the sample dicts spiked by the restated rule: every trial's call rows."""
    outs = wt.test_batch(reference, [sc.spiked_sample(tuple(row)) for row in plan.tolist()], cc.THR, minrefbins=cc.MINREF,
                         repeats=cc.REPEATS)
    return [np.asarray(o["results_calls"], dtype=np.float64).reshape(-1, 5) for o in outs]


DESIGNED = {}


def designed(wt, reference):
    """The designed plan through the device route, once per module."""
    if not DESIGNED:
        plan = sc.designed_plan()
        rec_i, rec_f, calls = run(wt, reference, plan, keep_calls=True)
        DESIGNED.update(plan=plan, rec_i=rec_i, rec_f=rec_f, calls=calls)
    return DESIGNED


def test_calls_equal_the_host_route_and_the_oracle(wt, reference):
    got = designed(wt, reference)
    plan = got["plan"]
    assert len(got["calls"]) == len(plan) == 20 and set(plan[:, 0].tolist()) == {0, 1}
    want = host_route(wt, reference, plan)
    for i, row in enumerate(plan.tolist()):
        assert same_bits(got["calls"][i], want[i]), (row, got["calls"][i], want[i])
    for i, (trial, span, _, _) in enumerate(sc.ROWS):
        assert plan[i].tolist() == [0] + list(trial)
        assert same_bits(got["calls"][i], sc.oracle_calls((0,) + trial)), (trial, got["calls"][i])
        assert len(got["calls"][i]) == (0 if span is None else 1)


def test_records_equal_the_restated_score(wt, reference):
    got = designed(wt, reference)
    want_i, want_f = sr.score_lists(got["plan"], got["calls"])
    assert got["rec_i"].dtype == np.int32 and got["rec_i"].shape == (20, 8) and got["rec_f"].shape == (20, 2)
    assert np.array_equal(got["rec_i"], want_i)
    nan = np.isnan(want_f)
    assert np.array_equal(np.isnan(got["rec_f"]), nan)
    assert np.array_equal(got["rec_f"].view(np.int64)[~nan], want_f.view(np.int64)[~nan])
    for i, (_, span, record, _) in enumerate(sc.ROWS):
        assert tuple(got["rec_i"][i, 1:4]) == record
        assert tuple(got["rec_i"][i, 4:7]) == ((-1, -1, -1) if span is None else (0,) + span)
    controls = got["plan"][:, 4] == 0
    assert controls.sum() == 2 and (got["rec_i"][controls] == [0, 0, 0, 0, -1, -1, -1, 0]).all()


@pytest.mark.parametrize("batch", [1, 5])
def test_batches_give_the_same_records(wt, reference, batch):
    got = designed(wt, reference)
    rec_i, rec_f = run(wt, reference, got["plan"], batch=batch)
    assert np.array_equal(rec_i, got["rec_i"])
    assert np.array_equal(rec_f.view(np.int64), got["rec_f"].view(np.int64))


def test_a_trial_with_more_calls_than_the_room_is_run_again(wt, reference, monkeypatch):
    """MAX_CALLS = 1: the whole of chromosome 1 lost (one call: the room holds) and a trial with two calls (the batch is
    run again with four times the room); both equal wt.test_batch."""
    from wisecondor_amd import sensitivity
    n1 = int(sc.lay()["sizes"][0])
    plan = np.array([(0, 1, 0, n1, -1000000), TWO_CALLS, (1, 1, 0, 1, 0)], dtype=np.int32)
    want = host_route(wt, reference, plan)
    assert [len(w) for w in want] == [1, 2, 0]
    monkeypatch.setattr(sensitivity, "MAX_CALLS", 1)
    for batch in (1, 3):
        rec_i, rec_f, calls = run(wt, reference, plan, keep_calls=True, batch=batch)
        for i in range(3):
            assert same_bits(calls[i], want[i]), (batch, i, calls[i], want[i])
        want_i, _ = sr.score_lists(plan, want)
        assert np.array_equal(rec_i, want_i)
        assert rec_i[1].tolist() == [2, 1, 32, 32, 1, 0, 31, 0]          # the loss call on chromosome 9 is a call elsewhere
    assert same_bits(want[0], sc.oracle_calls(tuple(plan[0].tolist())))
    assert same_bits(want[1], sc.oracle_calls(TWO_CALLS))


def test_a_bad_plan_row_is_refused_before_anything_runs(wt, reference):
    from wisecondor_amd import _lib
    plan = sc.designed_plan()
    plan[7, 3] = 500
    with pytest.raises(_lib.WisecondorHipError, match="plan row 7") as err:
        run(wt, reference, plan)
    assert err.value.code == _lib.E_ARG


def test_command_line(wt, tmp_path, capsys):
    from wisecondor_amd import sensitivity
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    options = ["-lengths", sc.CLI_LENGTHS_BP, "-effects", sc.CLI_EFFECTS_PERCENT, "-trials", str(sc.CLI_TRIALS), "-minzscore", "5",
               "-repeats", "2"]
    cli.main(["sensitivity"] + paths + [str(tmp_path / "out"), ref_path] + options)
    printed = capsys.readouterr().out
    cli.main(["sensitivity"] + paths + [str(tmp_path / "again.npz"), ref_path] + options)
    out = np.load(str(tmp_path / "out.npz"), allow_pickle=True)
    again = np.load(str(tmp_path / "again.npz"), allow_pickle=True)
    assert sorted(out.files) == sorted(["arguments", "runtime", "binsize", "threshold_z", "samples", "lengths_bins", "effects_ppm",
                                        "plan", "rec_i", "rec_f", "table"])
    n = 4 * (1 + 2 * 3 * 3)
    assert out["plan"].shape == (n, 5) and out["rec_i"].shape == (n, 8) and out["rec_f"].shape == (n, 2)
    assert out["table"].shape == (2 * 3 + 1, len(sensitivity.TABLE_COLUMNS)) and out["samples"].tolist() == paths
    assert out["lengths_bins"].tolist() == sc.CLI_LENGTHS_BINS and out["effects_ppm"].tolist() == sc.CLI_EFFECTS_PPM
    assert float(out["threshold_z"]) == 5.0 and float(out["binsize"]) == cc.BINSIZE
    assert out["arguments"].item()["trials"] == 3 and out["arguments"].item()["seed"] == 1
    reference = cc.reference_of(sc.lay(), sc.cli_samples()[0])
    assert np.array_equal(out["plan"], sensitivity.makePlan(reference, 4, sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, 3, seed=1))
    table = sensitivity.sensitivityTable(out["plan"], out["rec_i"], out["rec_f"], sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, 0.5)
    assert np.array_equal(out["table"], table, equal_nan=True)
    assert np.array_equal(out["table"], sr.table(out["plan"], out["rec_i"], out["rec_f"], sc.CLI_LENGTHS_BINS, sc.CLI_EFFECTS_PPM, 0.5),
                          equal_nan=True)
    assert np.array_equal(out["rec_i"], again["rec_i"]) and np.array_equal(out["plan"], again["plan"])
    assert np.array_equal(out["rec_f"].view(np.int64), again["rec_f"].view(np.int64))
    lines = open(str(tmp_path / "out.tsv")).read().strip("\n").split("\n")
    assert lines[0].split("\t") == list(sensitivity.TABLE_COLUMNS)
    assert np.array_equal(np.array([[float(v) for v in line.split("\t")] for line in lines[1:]]), out["table"], equal_nan=True)
    assert "\n".join(lines) in printed
    # test_sensitivity_cpu.py::test_oracle_rates_on_the_command_lines_exact_plan asked the oracle for these two on this plan
    by = {(int(r[0]), int(r[1])): r for r in out["table"]}
    assert by[(5, 2500000)][2] == 12 and by[(5, 2500000)][4] == 1.0
    assert by[(5, 100000)][2] == 12 and by[(5, 100000)][4] == 0.0
    assert by[(0, 0)][2] == 4 and by[(0, 0)][8] == 0.0               # the four unspiked samples: no call
