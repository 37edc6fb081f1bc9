"""Blacklists end to end on the planted cohort of robust_cases.py (held on the CPU by test_robust_cases_cpu.py):
wt.prepReference(drop=...) against the oracle route with the mask restated, `newref -blacklist` and `test` against the
reference it writes, `crossval -makeblacklist` finding exactly the planted bins, `crossval -blacklist` against the public
host-array route fold by fold, and a run without the new options leaving what it leaves today."""
import os

import numpy as np
import pytest

import robust_cases as rc
import robust_restated as rr
from oracle import wc_oracle as wo

pytestmark = pytest.mark.gpu
TEST_OPTIONS = ["-minzscore", str(rc.THR), "-minrefbins", str(rc.MINREF), "-repeats", str(rc.REPEATS)]
CLI_OPTIONS = ["-refsize", str(rc.REFSIZE)] + TEST_OPTIONS
OPTIONS = dict(refsize=rc.REFSIZE, minzscore=rc.THR, minrefbins=rc.MINREF, repeats=rc.REPEATS)
COMP_ATOL = CORRECTED_RTOL = 1e-12
BATCH_KEYS = {"bins_i", "bins_f", "rec_i", "rec_f", "win_n", "win_i", "win_hist", "fold_of", "threshold", "cutoff", "calls"}
NPZ_KEYS = BATCH_KEYS | {"arguments", "runtime", "binsize", "samples", "chromosome_sizes", "windows"}
REFERENCE_KEYS = {"arguments", "runtime", "binsize", "indexes", "distances", "chromosome_sizes", "mask", "masked_sizes", "pca_components",
                  "pca_mean"}
NEW_OPTIONS = ("blacklist", "robust", "makeblacklist", "maxspread", "maxshift", "mincover")
CACHE = {}


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.int64(-1), a.view(np.int64))


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def once(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def files(folder_factory):
    """The forty sample files and the planted bins as a BED file, once per module."""
    def make():
        from wisecondor_amd import blacklist
        folder = folder_factory.mktemp("blacklist_files")
        bed = str(folder / "planted.bed")
        blacklist.writeBlacklist(bed, rc.planted_drop(), rc.SIZES, rc.BINSIZE)
        return dict(folder=folder, paths=rc.write_cli_files(folder), bed=bed)
    return once("files", make)


# ------------------------------------------------------------------------------------- wt.prepReference(drop=) ----
def prep(drop, device_out=False):
    from wisecondor_amd import wisetools as wt
    return wt.prepReference(None, counts=rc.counts(rc.PREP_N), chrom_bins=rc.SIZES, drop=drop, device_out=device_out)


def dropped_prep():
    """(the host form's outputs, NewrefJob's indexes and distances on the device form's matrix) under the planted drop."""
    def make():
        import torch
        from wisecondor_amd import _lib
        from wisecondor_amd.distributed import NewrefJob
        host = prep(rc.planted_drop())
        dev = prep(rc.planted_drop(), device_out=True)
        job = NewrefJob(_lib.context(0), dev[3], np.ascontiguousarray(dev[6], dtype=np.int64), rc.REFSIZE, _lib.SUM_SEQUENTIAL)
        indexes, distances = job.run()
        torch.cuda.synchronize()
        return host, dev, indexes.cpu().numpy(), distances.cpu().numpy()
    return once("dropped_prep", make)


def test_prep_with_a_drop_equals_the_oracle_route_with_the_mask_restated():
    host, dev, indexes, distances = dropped_prep()
    masked, bins, mask, corrected, comps, mean, mbins = host
    want = rc.oracle_reference(tuple(range(rc.PREP_N)), drop=rc.planted_drop())
    assert [int(v) for v in bins] == rc.SIZES
    assert np.array_equal(np.asarray(mask).astype(bool), want["mask"]) and not np.asarray(mask)[rc.PLANTED].any()
    assert int(np.asarray(mask).sum()) == rc.N_TOTAL - len(rc.PLANTED)              # this layout has no empty bin
    assert [int(v) for v in mbins] == want["masked_sizes"].tolist() and sum(mbins) == masked.shape[0]
    assert same_bits(masked, want["masked"])                                       # divided by the sum over ALL bins, then gathered
    comp_err = float(np.abs(comps - want["pca_components"]).max())
    corr_err = float(np.abs(np.asarray(corrected) / want["corrected"] - 1.0).max())
    mean_err = float(np.abs(mean / want["pca_mean"] - 1.0).max())
    print("components %.3e (absolute), correctedData %.3e, mean %.3e (relative)" % (comp_err, corr_err, mean_err))
    assert comp_err <= COMP_ATOL and corr_err <= CORRECTED_RTOL and mean_err <= CORRECTED_RTOL
    # the device form holds the same values, and the selection on them is the oracle's on them, bit for bit
    assert same_bits(dev[3].cpu().numpy(), np.ascontiguousarray(corrected)) and list(dev[6]) == list(mbins)
    with np.errstate(all="ignore"):
        want_i, want_d = wo.get_reference(np.asfortranarray(corrected), mbins, np.cumsum(mbins), rc.REFSIZE, 1, 1, fast=True)
    assert np.array_equal(indexes, want_i) and same_bits(distances, want_d)
    assert np.mean(indexes == want["indexes"]) > 0.99                              # and the oracle's own, up to the PCA's rounding


def test_a_drop_of_zeros_is_no_drop():
    a, b = prep(None), prep(np.zeros(rc.N_TOTAL, dtype=np.uint8))
    for k in (0, 3, 4, 5):
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.array_equal(a[2], b[2]) and list(a[6]) == list(b[6]) and a[2].all()
    c = prep(np.zeros(rc.N_TOTAL, dtype=bool).tolist())
    assert same_bits(np.asarray(a[3]), np.asarray(c[3]))


def test_a_drop_that_leaves_nothing_and_one_of_another_length_are_refused():
    from wisecondor_amd import _lib
    with pytest.raises(_lib.WisecondorHipError, match="every bin is empty") as refused:
        prep(np.ones(rc.N_TOTAL, dtype=np.uint8))
    assert refused.value.code == _lib.E_ARG
    for length in (rc.N_TOTAL - 1, rc.N_TOTAL + 1, 0):
        with pytest.raises(ValueError):
            prep(np.zeros(length, dtype=np.uint8))
    assert prep(rc.planted_drop())[0].shape[0] == rc.N_TOTAL - len(rc.PLANTED)      # the context prepares again afterwards


# ------------------------------------------------------------------------------------------ newref -blacklist ----
def reference_file(folder_factory):
    def make():
        from wisecondor_amd import wisecondor as cli
        made = files(folder_factory)
        path = str(made["folder"] / "reference.npz")
        cli.main(["newref"] + made["paths"][:rc.PREP_N] + [path, "-refsize", str(rc.REFSIZE), "-blacklist", made["bed"]])
        return path
    return once("reference", make)


def test_newref_blacklist_writes_the_reference_of_the_dropped_prep(tmp_path_factory):
    path = reference_file(tmp_path_factory)
    ref = np.load(path, allow_pickle=True)
    host, _, indexes, distances = dropped_prep()
    assert set(ref.files) == REFERENCE_KEYS | {"blacklist"}
    assert ref["blacklist"].dtype == np.uint8 and np.array_equal(ref["blacklist"], rc.planted_drop())
    assert ref["arguments"].item()["blacklist"] == files(tmp_path_factory)["bed"]
    assert np.array_equal(ref["mask"], host[2]) and ref["masked_sizes"].tolist() == list(host[6])
    assert np.array_equal(ref["indexes"], indexes) and same_bits(ref["distances"], distances)
    assert same_bits(ref["pca_components"], host[4]) and same_bits(ref["pca_mean"], host[5])
    assert not os.path.exists(path[:-4] + "_prep.npz")


def test_newrefprep_blacklist_keeps_the_dropped_bins_in_the_prep_file(tmp_path_factory, tmp_path, capsys):
    from wisecondor_amd import wisecondor as cli
    made = files(tmp_path_factory)
    cli.main(["newrefprep"] + made["paths"][:rc.PREP_N] + [str(tmp_path / "prep.npz"), "-blacklist", made["bed"]])
    assert "%d of %d bins dropped, 0 lines ignored" % (len(rc.PLANTED), rc.N_TOTAL) in capsys.readouterr().out
    pz = np.load(str(tmp_path / "prep.npz"), allow_pickle=True)
    host = dropped_prep()[0]
    assert np.array_equal(pz["blacklist"], rc.planted_drop()) and np.array_equal(pz["mask"], host[2])
    assert same_bits(pz["correctedData"], host[3]) and pz["arguments"].item()["blacklist"] == made["bed"]


@pytest.mark.parametrize("i", [rc.PREP_N, rc.N - 1])
def test_test_against_the_blacklisted_reference_equals_the_oracle(tmp_path_factory, tmp_path, i):
    from wisecondor_amd import wisecondor as cli
    path = reference_file(tmp_path_factory)
    ref = np.load(path, allow_pickle=True)
    out_path = str(tmp_path / "out.npz")
    with pytest.raises(SystemExit) as stop:
        cli.main(["test", files(tmp_path_factory)["paths"][i], out_path, path] + TEST_OPTIONS)
    assert stop.value.code == 0
    out = np.load(out_path, allow_pickle=True)
    with np.errstate(all="ignore"):
        want = wo.test_sample(rc.samples()[i], rc.BINSIZE, {k: ref[k] for k in ref.files}, minzscore=rc.THR, minrefbins=rc.MINREF,
                              repeats=rc.REPEATS)
    z, r = np.concatenate(list(out["results_z"])), np.concatenate(list(out["results_r"]))
    assert z.shape == (rc.N_TOTAL,)
    # the project's tolerances of `test` against the oracle (test_cli_gpu.py)
    assert np.allclose(z, np.concatenate(want["results_z"]), rtol=1e-9, atol=1e-11)
    assert np.allclose(r, np.concatenate(want["results_r"]), rtol=1e-9, atol=1e-11)
    got_calls, want_calls = np.asarray(out["results_calls"]).reshape(-1, 5), np.asarray(want["results_calls"]).reshape(-1, 5)
    assert np.array_equal(got_calls[:, :3], want_calls[:, :3]) and np.allclose(got_calls[:, 3:], want_calls[:, 3:], rtol=1e-9)
    assert np.array_equal(bits(z[rc.PLANTED]), bits(np.zeros(len(rc.PLANTED)))) and np.array_equal(bits(r[rc.PLANTED]), bits(np.zeros(len(rc.PLANTED))))
    assert np.count_nonzero(z) > 200                                               # (the rest of the sample is tested)


# -------------------------------------------------------------------------------------- crossval -makeblacklist ----
def robust_batch():
    def make():
        from wisecondor_amd import crossval
        return crossval.crossval_batch(rc.counts(), rc.SIZES, crossval.foldPlan(rc.N, rc.N), rc.BINSIZE, keep_results=True, robust=True, **OPTIONS)
    return once("robust_batch", make)


def test_robust_figures_of_a_run_equal_the_restatement_on_its_rows():
    got = robust_batch()
    assert set(got) == BATCH_KEYS | {"robust_i", "robust_f", "Z", "R", "results_cwz"}
    want_i, want_f = rr.robust(got["Z"])
    assert got["robust_i"].dtype == np.int32 and np.array_equal(got["robust_i"], want_i)
    assert rr.same_bits(got["robust_f"], want_f)
    assert np.array_equal(got["robust_i"].sum(axis=1), got["bins_i"][:, 0]) and np.array_equal(got["robust_i"][:, 1], got["bins_i"][:, 1])
    spread = 1.4826 * got["robust_f"][:, 1]
    rest = np.setdiff1d(np.arange(rc.N_TOTAL), rc.PLANTED)
    print("planted: spread %.3f at least; others: %.3f at most" % (spread[rc.PLANTED].min(), np.nanmax(spread[rest])))
    stage_ms = {}
    from wisecondor_amd import crossval
    crossval.crossval_batch(rc.counts(rc.PREP_N), rc.SIZES, crossval.foldPlan(rc.PREP_N, 4), rc.BINSIZE, robust=True, stage_ms=stage_ms, **OPTIONS)
    assert set(stage_ms) == {"gather", "prep", "newref", "reference", "test", "stats", "robust"} and stage_ms["robust"] > 0


def test_crossval_makeblacklist_writes_exactly_the_planted_bins(tmp_path_factory, capsys):
    from wisecondor_amd import blacklist
    from wisecondor_amd import crossval
    from wisecondor_amd import wisecondor as cli
    made = files(tmp_path_factory)
    folder = tmp_path_factory.mktemp("make")
    bed = str(folder / "bl.bed")
    cli.main(["crossval"] + made["paths"] + [str(folder / "out"), "-loo", "-makeblacklist", bed, "-maxspread", str(rc.MAXSPREAD)] + CLI_OPTIONS)
    assert "%d bins in %d runs listed" % (len(rc.PLANTED), len(rc.PLANTED)) in capsys.readouterr().out
    drop, ignored = blacklist.readBlacklist(bed, rc.SIZES, rc.BINSIZE)
    assert ignored == 0 and np.flatnonzero(drop).tolist() == rc.PLANTED
    head = open(bed).readline()
    assert head.startswith("#") and str(rc.BINSIZE) in head and "maxspread=5.0" in head and "mincover=0.5" in head
    assert sorted(os.listdir(str(folder))) == ["bl.bed", "out.npz", "out_bins.tsv", "out_samples.tsv", "out_windows.tsv"]
    out = np.load(str(folder / "out.npz"), allow_pickle=True)
    want = robust_batch()
    assert set(out.files) == NPZ_KEYS | {"robust_i", "robust_f"}
    assert np.array_equal(out["robust_i"], want["robust_i"]) and rr.same_bits(out["robust_f"], want["robust_f"])
    arguments = out["arguments"].item()
    assert arguments["makeblacklist"] == bed and arguments["maxspread"] == rc.MAXSPREAD and "robust" not in arguments and "maxshift" not in arguments
    # out_bins.tsv: a line per bin of the layout, and the doubles read back bit for bit
    lines = open(str(folder / "out_bins.tsv")).read().strip("\n").split("\n")
    assert lines[0].split("\t") == list(crossval.BIN_COLUMNS) and len(lines) == 1 + rc.N_TOTAL
    cells = [line.split("\t") for line in lines[1:]]
    places = [rc.place(b) for b in range(rc.N_TOTAL)]
    assert [[int(v) for v in row[:3]] for row in cells] == [[c, g * rc.BINSIZE, (g + 1) * rc.BINSIZE] for c, g in places]
    assert np.array_equal(np.array([[int(row[3]), int(row[4])] for row in cells]), out["bins_i"][:, :2])
    assert rr.same_bits([float(row[5]) for row in cells], out["robust_f"][:, 0])
    assert rr.same_bits([float(row[6]) for row in cells], 1.4826 * out["robust_f"][:, 1])
    assert [int(row[9]) for row in cells] == rc.planted_drop().tolist()
    finite = out["robust_i"][:, 0]
    mean = np.array([float(row[7]) for row in cells])
    sd = np.array([float(row[8]) for row in cells])
    assert np.array_equal(np.isnan(mean), finite < 2) and np.array_equal(np.isnan(sd), finite < 2)
    rows = want["Z"]
    full = np.flatnonzero(finite == rc.N)
    assert len(full) > 200 and np.allclose(mean[full], rows[:, full].mean(axis=0), rtol=1e-9, atol=1e-12)
    assert np.allclose(sd[full], rows[:, full].std(axis=0, ddof=1), rtol=1e-7)


# ------------------------------------------------------------------------------------------ crossval -blacklist ----
def test_crossval_blacklist_equals_the_public_route_with_the_same_drop(tmp_path_factory):
    from wisecondor_amd import crossval
    from wisecondor_amd import wisecondor as cli
    from wisecondor_amd import wisetools as wt
    made = files(tmp_path_factory)
    folder = tmp_path_factory.mktemp("apply")
    n, folds = rc.PREP_N, 4
    cli.main(["crossval"] + made["paths"][:n] + [str(folder / "out"), "-folds", str(folds), "-blacklist", made["bed"], "-results", str(folder / "held")]
             + CLI_OPTIONS)
    out = np.load(str(folder / "out.npz"), allow_pickle=True)
    assert set(out.files) == NPZ_KEYS | {"blacklist"} and np.array_equal(out["blacklist"], rc.planted_drop())
    assert not os.path.exists(str(folder / "out_bins.tsv"))
    fold_of = crossval.foldPlan(n, folds, seed=1)
    assert out["fold_of"].tolist() == fold_of.tolist()
    assert (out["bins_i"][rc.PLANTED, :4] == 0).all()                              # no fold tested a dropped bin (calls may span one)
    drop = rc.planted_drop()
    for fold in range(folds):
        held = [i for i in range(n) if fold_of[i] == fold]
        training = [rc.samples()[i] for i in range(n) if fold_of[i] != fold]
        _, chrom_bins, mask, corrected, components, mean, masked_sizes = wt.prepReference(training, drop=drop)
        indexes, distances = wt.getReference(corrected, masked_sizes, np.cumsum(masked_sizes), selectRefAmount=rc.REFSIZE)
        reference = wt.Reference(indexes, distances, chrom_bins, masked_sizes, mask, mean, components, binsize=rc.BINSIZE)
        outs = wt.test_batch(reference, [rc.samples()[i] for i in held], rc.THR, minrefbins=rc.MINREF, repeats=rc.REPEATS)
        reference.close()
        for i, want in zip(held, outs):
            got = np.load(str(folder / "held" / ("healthy_%02d_test.npz" % i)), allow_pickle=True)
            for key in ("results_z", "results_r"):
                assert same_bits(np.concatenate(list(got[key])), np.concatenate(want[key])), (i, key)
            assert same_bits(got["results_cwz"], want["results_cwz"]), i
            assert (np.concatenate(list(got["results_z"]))[rc.PLANTED] == 0.0).all()


# ------------------------------------------------------------------------------------ a run without the options ----
def test_a_run_without_the_new_options_leaves_what_it_leaves_today(tmp_path_factory):
    from wisecondor_amd import crossval
    from wisecondor_amd import wisecondor as cli
    made = files(tmp_path_factory)
    folder = tmp_path_factory.mktemp("plain")
    n, folds = rc.PREP_N, 4
    cli.main(["crossval"] + made["paths"][:n] + [str(folder / "out"), "-folds", str(folds)] + CLI_OPTIONS)
    assert sorted(os.listdir(str(folder))) == ["out.npz", "out_samples.tsv", "out_windows.tsv"]
    out = np.load(str(folder / "out.npz"), allow_pickle=True)
    assert set(out.files) == NPZ_KEYS
    assert not any(name in out["arguments"].item() for name in NEW_OPTIONS)
    got = crossval.crossval_batch(rc.counts(n), rc.SIZES, crossval.foldPlan(n, folds), rc.BINSIZE, **OPTIONS)
    assert set(got) == BATCH_KEYS
    for key in ("bins_i", "rec_i", "win_i", "win_hist"):
        assert np.array_equal(got[key], out[key]), key
    assert same_bits(got["bins_f"], out["bins_f"])
    stage_ms = {}
    crossval.crossval_batch(rc.counts(n), rc.SIZES, crossval.foldPlan(n, folds), rc.BINSIZE, stage_ms=stage_ms, **OPTIONS)
    assert set(stage_ms) == {"gather", "prep", "newref", "reference", "test", "stats"}
    # and `newref` without -blacklist writes the keys it writes today
    ref_path = str(folder / "ref.npz")
    cli.main(["newref"] + made["paths"][:n] + [ref_path, "-refsize", str(rc.REFSIZE)])
    ref = np.load(ref_path, allow_pickle=True)
    assert set(ref.files) == REFERENCE_KEYS and "blacklist" not in ref["arguments"].item()
