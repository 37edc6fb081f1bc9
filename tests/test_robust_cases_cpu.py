"""What the robust-spread and blacklist tests stand on, held on the CPU: the restatement of wc_column_robust against
np.median, blacklist.listedBins and the BED reader and writer on hand-written figures, the new command line options, the
compiled kernel's resources, and the planted cohort of robust_cases.py through the oracle alone."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import robust_cases as rc
import robust_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the restatement ----
def numpy_route(values):
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(all="ignore"):
        median = np.median(v)
        return median, np.median(np.abs(v - median))


def test_restatement_equals_numpy_on_random_nonzero_finite_columns():
    rng = np.random.RandomState(11)
    for trial in range(4000):
        n = rng.randint(1, 40)
        v = rng.standard_normal(n) * 10.0 ** rng.randint(-300, 300, size=n)
        if trial % 3 == 0:
            v = np.ldexp(np.round(rng.standard_normal(n) * 20) * 2 + 1, -1074)       # subnormals, with ties
        if trial % 5 == 0:
            v = np.round(rng.standard_normal(n) * 2) + 0.5                         # ties
        assert np.isfinite(v).all() and (v != 0).all()
        finite, nonfinite, median, mad = rr.column(v)
        assert (finite, nonfinite) == (n, 0)
        assert rr.same_bits([median, mad], numpy_route(v)), v


@pytest.mark.parametrize("name,values", rc.COLUMNS, ids=[name for name, _ in rc.COLUMNS])
def test_restatement_on_the_hand_written_columns(name, values):
    finite, nonfinite, median, mad = rr.column(values)
    v = [x for x in values if x != 0 and math.isfinite(x)]
    assert finite == len(v) and nonfinite == sum(1 for x in values if x != 0 and not math.isfinite(x))
    if not v:
        assert math.isnan(median) and math.isnan(mad)
        return
    want_median, want_mad = numpy_route(v)
    assert rr.same_bits(median, want_median)
    assert rr.same_bits(mad, want_mad) if math.isfinite(median) else math.isnan(mad)


def test_hand_written_answers():
    answers = {"one": (-3.25, 0.0), "two": (2.5, 1.5), "all equal": (2.5, 0.0), "ties across the middle pair": (2.0, 0.5),
               "the lower run ends at the middle rank": (1.5, 0.5), "the lower run ends at the middle rank, long": (4.0, 3.0),
               "one ulp apart": (rc.UP, rc.UP - 1.0), "one ulp apart, odd": (rc.UP, rc.UP - 1.0), "negatives only": (-1.75, 1.0),
               "pairs -x and +x": (0.0, 2.5), "pairs -x and +x and one more": (0.0, 2.0), "1e300 beside 5e-324": (rc.TINY, 2 * rc.TINY),
               "subnormals": (2 * rc.TINY, rc.TINY), "nonfinite and zeros kept out": (1.5, 2.0),
               "the deviations' middle pair overflows": ((-1.7e308 + 1.0e308) / 2.0, rc.INF)}
    columns = dict(rc.COLUMNS)
    for name, (median, mad) in answers.items():
        got = rr.column(columns[name])
        assert rr.same_bits(got[2:], [median, mad]), (name, got)
    assert math.copysign(1.0, rr.column(columns["pairs -x and +x"])[2]) == 1.0          # +0.0
    for name in ("the middle pair overflows", "the middle pair overflows downwards"):
        got = rr.column(columns[name])
        assert got[0] == 4 and math.isinf(got[2]) and math.isnan(got[3])
    assert rr.column(columns["a deviation overflows"])[2:] == (1.5e308, 1.7e308 - 1.5e308)
    for name in ("none", "nonfinite only", "zeros only"):
        assert rr.column(columns[name])[0] == 0 and all(math.isnan(v) for v in rr.column(columns[name])[2:])
    assert rr.column(columns["nonfinite only"])[1] == 3


def test_restatement_refuses_what_the_library_refuses():
    for shape in ((0, 3), (3, 0)):
        with pytest.raises(rr.Refused):
            rr.robust(np.zeros(shape))
    with pytest.raises(rr.Refused):
        rr.robust(np.zeros((2, 3)), n_cols=4)
    with pytest.raises(rr.TooLarge):
        rr.robust(np.zeros((8193, 1)))
    assert rr.robust(np.ones((8192, 1)))[0].tolist() == [[8192, 0]]


# ----------------------------------------------------------------------------------------------- listedBins ----
def test_listed_bins_cover_spread_and_shift():
    from wisecondor_amd import blacklist
    n = 9                                               # ceil(0.5 * 9) = 5
    cut = blacklist.MAD_TO_SD * 2.0                     # the spread of a mad of 2.0, as listedBins forms it
    above = float(np.nextafter(2.0, 9.0))               # the next mad; its spread is the next double or the one after
    assert cut < blacklist.MAD_TO_SD * above <= float(np.nextafter(np.nextafter(cut, 9.0), 9.0))
    col_i = np.array([[5, 0], [4, 5], [9, 0], [9, 0], [9, 0], [0, 9], [0, 0], [9, 0]], dtype=np.int32)
    col_f = np.array([[0.0, 10.0],                      # wide, cover exactly at ceil(mincover * n): listed
                      [0.0, 10.0],                      # wide, one below: not listed (the nonfinite samples do not count)
                      [0.0, 2.0],                       # a spread equal to maxspread: not listed
                      [0.0, above],                     # one ulp of the mad above it: listed
                      [-2.5, 0.1],                      # quiet but shifted
                      [rc.NAN, rc.NAN],                 # tested by all, finite in none
                      [rc.NAN, rc.NAN],                 # no fold tested it
                      [rc.INF, rc.NAN]])                # a median that overflowed
    got = blacklist.listedBins(col_i, col_f, n, cut)
    assert got.dtype == bool and got.tolist() == [True, False, False, True, False, False, False, False]
    got = blacklist.listedBins(col_i, col_f, n, cut, maxshift=2.0)
    assert got.tolist() == [True, False, False, True, True, False, False, True]
    assert blacklist.listedBins(col_i, col_f, n, cut, maxshift=2.5).tolist()[4] is False          # > is the test
    assert blacklist.listedBins(col_i, col_f, n, cut, mincover=4 / 9.0).tolist()[1] is True
    assert blacklist.listedBins(col_i, col_f, n, cut, mincover=0.0).tolist()[5:7] == [False, False]
    with pytest.raises(TypeError):
        blacklist.listedBins(col_i, col_f, n)           # maxspread has no default


# ------------------------------------------------------------------------------------------------------ BED ----
SIZES_BED = [4, 3] + [2] * 20


def test_bed_writer_then_reader(tmp_path):
    from wisecondor_amd import blacklist
    listed = np.zeros(sum(SIZES_BED), dtype=bool)
    listed[[0, 1, 3, 4, 6, 7, 8, 46]] = True            # 3 | 4: a run that ends with chromosome 1 and one that begins chromosome 2
    path = str(tmp_path / "bl.bed")
    runs = blacklist.writeBlacklist(path, listed, SIZES_BED, 1000, note="maxspread=3.0")
    lines = open(path).read().split("\n")
    assert lines[0].startswith("#") and "1000" in lines[0] and "maxspread=3.0" in lines[0] and lines[-1] == ""
    assert lines[1:-1] == ["chr1\t0\t2000", "chr1\t3000\t4000", "chr2\t0\t1000", "chr2\t2000\t3000", "chr3\t0\t2000", "chr22\t1000\t2000"]
    assert runs == 6                                    # runs do not cross chromosomes
    drop, ignored = blacklist.readBlacklist(path, SIZES_BED, 1000)
    assert drop.dtype == np.uint8 and ignored == 0 and np.array_equal(drop.astype(bool), listed)
    # at a bin size that divides it: every listed bin becomes its four quarters
    fine, ignored = blacklist.readBlacklist(path, [4 * s for s in SIZES_BED], 250)
    assert ignored == 0 and np.array_equal(fine.astype(bool), np.repeat(listed, 4))
    blacklist.writeBlacklist(path, listed, SIZES_BED, 1000, prefix="")
    assert open(path).read().split("\n")[1] == "1\t0\t2000"
    assert np.array_equal(blacklist.readBlacklist(path, SIZES_BED, 1000)[0].astype(bool), listed)
    with pytest.raises(ValueError):
        blacklist.writeBlacklist(path, listed[:-1], SIZES_BED, 1000)


def test_bed_reader_names_edges_and_clipping(tmp_path):
    from wisecondor_amd import blacklist
    path = str(tmp_path / "in.bed")
    with open(path, "w") as handle:
        handle.write("track name=x\nbrowser position chr1\n# a comment\n\n"
                     "chr1\t1999\t2000\tname\t0\t+\n"       # touches bin 1 by its last base pair
                     "1 3000 3001\n"                         # spaces, no prefix: touches bin 3 by its first
                     "chr2\t0\t1000\n"                       # ends exactly at the start of bin 1: bin 0 alone
                     "chr2\t2999\t9000000\n"                 # clipped to the chromosome's last bin
                     "chr3\t5000\t6000\n"                    # wholly beyond the layout: nothing
                     "chrX\t0\t5000\nY\t0\t10\nchrM\t1\t2\nchrUn_gl000220\t0\t100\nchr23\t0\t10\nchr0\t0\t10\n")
    drop, ignored = blacklist.readBlacklist(path, SIZES_BED, 1000)
    assert ignored == 6
    assert np.flatnonzero(drop).tolist() == [1, 3, 4, 6]
    # the same file at 500 bp bins of the same genome
    drop, _ = blacklist.readBlacklist(path, [2 * s for s in SIZES_BED], 500)
    assert np.flatnonzero(drop).tolist() == [3, 6, 8, 9, 13]


@pytest.mark.parametrize("line", ["chr1\t5", "chr1", "chr1\ta\t5", "chr1\t1\t5.5", "chr1\t-1\t5", "chr1\t5\t5", "chr1\t6\t5", "chrX\t5\t1"])
def test_bed_reader_names_the_malformed_line(tmp_path, line):
    from wisecondor_amd import blacklist
    path = str(tmp_path / "bad.bed")
    with open(path, "w") as handle:
        handle.write("# header\nchr1\t0\t10\n\n" + line + "\n")
    with pytest.raises(ValueError, match="line 4"):
        blacklist.readBlacklist(path, SIZES_BED, 1000)


# -------------------------------------------------------------------------------------------------- options ----
def test_options_are_parsed_and_absent_unless_given():
    from wisecondor_amd import wisecondor as cli
    parser = cli.buildParser()
    new = ("blacklist", "robust", "makeblacklist", "maxspread", "maxshift", "mincover")
    plain = parser.parse_args(["crossval", "a", "b", "c", "d", "e", "out"])
    assert not any(hasattr(plain, name) for name in new)
    for tool, tail in (("newref", ["a", "ref.npz"]), ("newrefprep", ["a", "prep.npz"])):
        assert not hasattr(parser.parse_args([tool] + tail), "blacklist")
        assert parser.parse_args([tool] + tail + ["-blacklist", "bl.bed"]).blacklist == "bl.bed"
    full = parser.parse_args(["crossval", "a", "b", "c", "d", "e", "out", "-blacklist", "in.bed", "-makeblacklist", "bl.bed", "-maxspread", "2.5",
                              "-maxshift", "1.5", "-mincover", "0.75"])
    assert (full.blacklist, full.makeblacklist, full.maxspread, full.maxshift, full.mincover) == ("in.bed", "bl.bed", 2.5, 1.5, 0.75)
    assert not hasattr(full, "robust")                  # implied, not set
    assert cli.crossvalRobustPlan(full) == (True, dict(maxspread=2.5, maxshift=1.5, mincover=0.75))
    assert cli.crossvalRobustPlan(plain) == (False, None)
    only = parser.parse_args(["crossval", "a", "b", "c", "d", "e", "out", "-robust"])
    assert only.robust is True and cli.crossvalRobustPlan(only) == (True, None)
    assert cli.crossvalRobustPlan(parser.parse_args(["crossval", "a", "out", "-maxspread", "3"])) == \
        (True, dict(maxspread=3.0, maxshift=None, mincover=0.5))
    for tool in ("test", "testbatch", "sensitivity", "report"):
        with pytest.raises(SystemExit):
            parser.parse_args([tool, "-blacklist", "x"] + ["a"] * 4)


def test_makeblacklist_without_maxspread_exits_2_before_the_gpu(tmp_path, capsys, monkeypatch):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisecondor as cli
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    paths = rc.write_cli_files(tmp_path, n=5)
    for extra in (["-makeblacklist", str(tmp_path / "bl.bed")], ["-robust", "-mincover", "0.3"], ["-maxspread", "-1"]):
        with pytest.raises(SystemExit) as stop:
            cli.main(["crossval"] + paths + [str(tmp_path / "out")] + extra)
        assert stop.value.code == 2
        assert "ERROR" in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / "bl.bed")) and not os.path.exists(str(tmp_path / "out.npz"))


# --------------------------------------------------------------------------------------- the compiled kernel ----
def test_robust_listing_has_the_recorded_resources():
    """The kernel of csrc/robust.hip (gfx950 assembly, cross-compiled here): registers, scratch, spills and LDS are what
    profiles/robust_kernel_resources.txt records, and every workgroup barrier, if there is one, is reached with the wave's
    own LDS operations complete (tools/barrier_scan.py).  The listing is searched for nothing else."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "robust.hip" in SOURCES
    import tempfile
    with tempfile.TemporaryDirectory() as folder:
        out = os.path.join(folder, "robust.s")
        flags = [f for f in FLAGS if f != "-fPIC"]
        subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "robust.hip")],
                              stderr=subprocess.DEVNULL)
        total, bad = barrier_scan.scan(out)
        text = open(out).read()
    assert not bad, bad[:5]
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in meta.split("  - .agpr_count:")[1:]:
        k = ".agpr_count:" + k
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))      # noqa: E731
        short = re.search(r"k_rb_[a-z]+", re.search(r"\.name:\s+(\S+)", k).group(1)).group(0)
        seen[short] = dict(vgpr=get("vgpr_count"), agpr=get("agpr_count"), spill=get("vgpr_spill_count"),
                           scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"), sgpr=get("sgpr_count"))
        assert get("sgpr_spill_count") == 0, short
    recorded = {}
    for line in open(os.path.join(ROOT, "profiles", "robust_kernel_resources.txt")):
        m = re.match(r"(k_rb_\w+)\s+vgpr\s+(\d+) agpr\s+(\d+) spill\s+(\d+) scratch\s+(\d+) lds\s+(\d+) sgpr\s+(\d+)", line)
        if m:
            recorded[m.group(1)] = dict(zip(("vgpr", "agpr", "spill", "scratch", "lds", "sgpr"), (int(v) for v in m.groups()[1:])))
    assert sorted(seen) == ["k_rb_cols"]
    assert seen == recorded
    for name, figures in seen.items():
        assert figures["scratch"] == 0 and figures["spill"] == 0, name


# ---------------------------------------------------------------------------------------- the planted cohort ----
def test_planted_cohort_through_the_oracle_alone():
    """Leave-one-out through wo.test_sample, the restatement on the resulting matrix: every planted bin has a robust spread
    of twice MAXSPREAD at least, every other bin that MINCOVER of the samples tested has half of it at most, so a route that
    agrees with the oracle to a part in a thousand lists the planted bins and no other."""
    from wisecondor_amd import blacklist
    Z = rc.oracle_loo()
    assert Z.shape == (rc.N, rc.N_TOTAL) and np.isfinite(Z).all()
    col_i, col_f = rr.robust(Z)
    spread = 1.4826 * col_f[:, 1]
    need = int(math.ceil(rc.MINCOVER * rc.N))
    planted = np.zeros(rc.N_TOTAL, dtype=bool)
    planted[rc.PLANTED] = True
    assert len(rc.PLANTED) == 61
    print("planted: cover %d at least, spread %.3f at least; others: %d covered, spread %.3f at most"
          % (col_i[planted, 0].min(), spread[planted].min(), int((col_i[~planted, 0] >= need).sum()), np.nanmax(spread[~planted])))
    assert (col_i[planted, 0] >= need).all()
    assert (spread[planted] >= 2 * rc.MAXSPREAD).all()
    others = ~planted & (col_i[:, 0] >= need)
    assert others.sum() >= 200 and (spread[others] <= rc.MAXSPREAD / 2).all()
    assert ((col_i[:, 0] >= need) | (col_i[:, 0] == 0)).all()          # no bin sits near the cover criterion
    listed = blacklist.listedBins(col_i, col_f, rc.N, rc.MAXSPREAD, mincover=rc.MINCOVER)
    assert np.flatnonzero(listed).tolist() == rc.PLANTED
