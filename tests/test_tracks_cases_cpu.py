"""exporttracks without a GPU: the restatement (tests/tracks_restated.py) against hand-written texts, one rule at a time;
the cases (tests/tracks_cases.py) expanded back to their bins by bits; the two bounds; the calls file; the BGZF walker
on strings made with zlib and on damaged ones; the command line's options."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracks_cases as tc  # noqa: E402
import tracks_restated as tr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from wisecondor_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def test_the_restatement_rule_by_rule():
    text = lambda *a, **k: tr.track_text(*a, **k)[0]        # noqa: E731
    # a run is one line; values as repr writes them
    assert text([1.5, 1.5, 0.1 + 0.2], [3], 100) == b"chr1\t0\t200\t1.5\nchr1\t200\t300\t0.30000000000000004\n"
    # no run crosses a chromosome, and chromosome i is named prefix + (i + 1); an empty chromosome has no line
    assert text([2.0, 2.0, 2.0], [1, 0, 2], 10) == b"chr1\t0\t10\t2.0\nchr3\t0\t20\t2.0\n"
    assert text([2.0], [1], 10, prefix="") == b"1\t0\t10\t2.0\n" and text([2.0], [1], 10, prefix="Chr_") == b"Chr_1\t0\t10\t2.0\n"
    # the same 64 bits, not the same value: -0.0 beside 0.0 are two runs
    assert text([0.0, -0.0, -0.0], [3], 5) == b"chr1\t0\t5\t0.0\nchr1\t5\t15\t-0.0\n"
    # not finite: left out and counted, a gap in the track
    assert tr.track_text([1.0, float("inf"), tc.NAN_A, tc.NAN_B, -float("inf"), 1.0], [6], 5) == (b"chr1\t0\t5\t1.0\nchr1\t25\t30\t1.0\n", 4)
    # nozero: zeros of either sign too, but they are not counted
    assert tr.track_text([0.0, -0.0, 3.0, tc.NAN_A], [4], 5, nozero=True) == (b"chr1\t10\t15\t3.0\n", 1)
    assert tr.track_text([0.0, tc.NAN_A], [2], 5, nozero=True) == (b"", 1)
    # clipping shortens a chromosome's last line only
    assert text([1.0, 2.0, 2.0, 4.0], [3, 1], 100, clip=[250, 100]) == b"chr1\t0\t100\t1.0\nchr1\t100\t250\t2.0\nchr2\t0\t100\t4.0\n"
    # the shortest and the longest value
    assert text([0.0, tc.LONGEST], [2], 1) == b"chr1\t0\t1\t0.0\nchr1\t1\t2\t-1.2345678901234567e-308\n"
    assert tr.bits_of(tc.NAN_A) != tr.bits_of(tc.NAN_B) != tr.bits_of(tc.NAN_C) and tr.bits_of(-0.0) == 1 << 63
    assert tr.expand(b"chr2\t100\t250\t2.0\n", 100) == {(1, 1): 2.0, (1, 2): 2.0}
    with pytest.raises(AssertionError):
        tr.expand(b"chr1\t0\t200\t2.0\nchr1\t100\t200\t2.0\n", 100)


def test_every_case_expands_back_to_its_bins(lib):
    from wisecondor_amd import wisetools as wt
    assert len(tc.cases()) >= 20
    for case in tc.cases():
        bound = wt.bedgraphRowBound(case["sizes"], case["binsize"], len(case["prefix"]))
        for row in case["rows"]:
            text, dropped = tr.track_text(row, case["sizes"], case["binsize"], case["prefix"], case["clip"], case["nozero"])
            assert len(text) <= bound, case["name"]
            bins = tr.expand(text, case["binsize"], case["prefix"])           # (raises where a bin is covered twice)
            left_out = 0
            for c, lo, hi in tr.chrom_ranges(case["sizes"]):
                for j in range(lo, hi):
                    value = float(row[j])
                    if not np.isfinite(value) or (case["nozero"] and value == 0.0):
                        assert (c, j - lo) not in bins, (case["name"], c, j)
                        left_out += not np.isfinite(value)
                    else:
                        assert tr.bits_of(bins[(c, j - lo)]) == tr.bits_of(value), (case["name"], c, j)
            assert left_out == dropped and len(bins) + sum(1 for v in row[:sum(case["sizes"])] if not np.isfinite(v) or (case["nozero"] and v == 0)) \
                == sum(case["sizes"]), case["name"]
    # what the names promise
    assert tr.track_text(tc.by_name("equal_across_a_chromosome_boundary")["rows"][0], [10, 10], 50000)[0].count(b"\n") == 2
    assert tr.track_text(tc.by_name("one_run_per_chromosome")["rows"][0], [300, 1, 700], 50000)[0].count(b"\n") == 3
    assert all(tr.track_text(row, [2 * tc.TILE + 5], 50000)[0] == b"" for row in tc.by_name("everything_left_out")["rows"])
    case = tc.by_name("fifteen_digits")
    assert b"\t999999999999999\t" in tr.track_text(case["rows"][0], case["sizes"], case["binsize"])[0]
    case = tc.by_name("clip_last_lines")
    assert tr.track_text(case["rows"][0], case["sizes"], 1000, clip=case["clip"])[0].splitlines()[-1] == b"chr4\t0\t1\t" + repr(float(case["rows"][0][-1])).encode()


def test_row_bound(lib):
    from wisecondor_amd import wisetools as wt
    # bins * (prefix + digits of the number + digits of the last start + digits of the end + 28), chromosome by chromosome
    assert wt.bedgraphRowBound([], 1, 3) == 0 and wt.bedgraphRowBound([0, 0], 50000, 3) == 0
    assert wt.bedgraphRowBound([1], 1, 0) == 1 * (0 + 1 + 1 + 1 + 28)
    assert wt.bedgraphRowBound([3, 0, 1] + [0] * 8 + [100], 50000, 3) == 3 * (3 + 1 + 6 + 6 + 28) + 1 * (3 + 1 + 1 + 5 + 28) + 100 * (3 + 2 + 7 + 7 + 28)
    # it is reached: every bin a line of the longest value, every coordinate as long as the chromosome's longest
    assert len(tr.track_text([tc.LONGEST], [1], 25)[0]) == wt.bedgraphRowBound([1], 25, 3) == 3 + 1 + 1 + 2 + 28
    assert len(tr.track_text([tc.LONGEST, 2 * tc.LONGEST] * 2, [4], 25)[0]) == 4 * (3 + 1 + 28) + (1 + 2 + 2 + 2) + (2 + 2 + 2 + 3)
    assert wt.bedgraphRowBound([4], 25, 3) == 4 * (3 + 1 + 2 + 3 + 28)
    for sizes, row, binsize, prefix in tc.random_rows():
        for nozero in (False, True):
            text, _ = tr.track_text(row, sizes, binsize, prefix, nozero=nozero)
            assert len(text) <= wt.bedgraphRowBound(sizes, binsize, len(prefix))
    assert len(tc.random_rows()) == 300 and any(b"\n" in tr.track_text(r, s, b, p)[0] for s, r, b, p in tc.random_rows())
    runs = sum(tr.track_text(r, s, b, p)[0].count(b"\n") for s, r, b, p in tc.random_rows())
    assert runs < sum(sum(s) for s, _, _, _ in tc.random_rows())         # runs occurred
    for bad in (dict(sizes=[3, -1]), dict(sizes=[1] * 65), dict(binsize=0), dict(prefix_len=17), dict(prefix_len=-1),
                dict(sizes=[3], binsize=333333333333334), dict(sizes=[1], binsize=10 ** 15)):
        with pytest.raises(ValueError):
            wt.bedgraphRowBound(bad.get("sizes", [3]), bad.get("binsize", 1), bad.get("prefix_len", 3))
    assert wt.bedgraphRowBound([3], 333333333333333, 16) == 3 * (16 + 1 + 15 + 15 + 28)
    assert wt.bedgraphRowBound([1], 10 ** 15 - 1, 0) == 1 + 1 + 15 + 28


def test_bgzf_bound(lib):
    B = lib.wc_deflate_block_bytes()
    assert B == 16384
    assert lib.wc_bgzf_bound(-1) == -1 and lib.wc_bgzf_bound(0) == 28
    # a stored block is 5 bytes longer than its input, the frame 26, and the end-of-file block 28
    for n, blocks in ((1, 1), (B - 1, 1), (B, 1), (B + 1, 2), (2 * B + 1, 3), (10 * B, 10)):
        assert lib.wc_bgzf_bound(n) == n + 31 * blocks + 28
    assert 18 + 5 + B + 8 <= 65536          # a block's BSIZE - 1 fits 16 bits


def _calls():
    return np.array([[3, 10, 12, 5.25, 0.031],
                     [1, 4, 4, float("nan"), -0.02],
                     [1, 0, 3, float("inf"), 0.05],
                     [1, 0, 3, -float("inf"), -0.05],         # a tie with the line before: the file's order stays
                     [2, 7, 9, -123.456, -0.015],            # |z| * 10 beyond 1000
                     [1, 0, 2, 4.449, 0.015],
                     [2, 7, 9, 0.25, 0.0151],
                     [22, 1, 299, -7.04, 1e-9]], dtype=np.float64)


def test_calls_bed(lib):
    from wisecondor_amd import wisetools as wt
    calls = _calls()
    text = wt.callsBed(calls, 1000)
    assert text == tr.calls_bed(calls, 1000)
    lines = text.decode().splitlines()
    assert len(lines) == 8
    assert lines[0] == "chr1\t0\t3000\tz=4.45;effect=1.50%\t44\t.\t0\t3000\t213,94,0"
    assert lines[1] == "chr1\t0\t4000\tz=inf;effect=5.00%\t1000\t.\t0\t4000\t213,94,0"
    assert lines[2] == "chr1\t0\t4000\tz=-inf;effect=-5.00%\t1000\t.\t0\t4000\t0,114,178"
    assert lines[3] == "chr1\t4000\t5000\tz=nan;effect=-2.00%\t0\t.\t4000\t5000\t0,114,178"
    assert lines[4].startswith("chr2\t7000\t10000\tz=-123.46;effect=-1.50%\t1000\t")
    assert lines[7] == "chr22\t1000\t300000\tz=-7.04;effect=0.00%\t70\t.\t1000\t300000\t213,94,0"
    assert [line.split("\t")[0] for line in lines] == ["chr1"] * 4 + ["chr2"] * 2 + ["chr3", "chr22"]
    # -mineffect is report's rule, abs(effect * 100) > mineffect: a call exactly on it is left out
    on_it = abs(calls[5, 4] * 100)
    kept = wt.callsBed(calls, 1000, mineffect=on_it)
    assert kept == tr.calls_bed(calls, 1000, mineffect=on_it) and kept.count(b"\n") == 5
    assert b"effect=1.50%" not in kept and b"effect=-1.50%" not in kept and b"effect=1.51%" in kept
    # clipping and the prefix
    clip = [4500] + [10 ** 9] * 21
    clipped = wt.callsBed(calls, 1000, prefix="", chrom_lengths=clip)
    assert clipped == tr.calls_bed(calls, 1000, prefix="", clip=clip)
    assert clipped.startswith(b"1\t0\t3000\t") and b"1\t4000\t4500\tz=nan;effect=-2.00%\t0\t.\t4000\t4500\t" in clipped
    assert wt.callsBed(np.array([]), 1000) == b"" == tr.calls_bed([], 1000)
    with pytest.raises(ValueError):
        wt.callsBed(calls, 1000, prefix="a\tb")


def test_bgzf_blocks_on_strings_made_with_zlib():
    rng = np.random.RandomState(3)
    data = bytes(rng.randint(48, 58, size=150000).astype(np.uint8))
    whole = tr.bgzf_of(data)
    blocks = tr.bgzf_blocks(whole)
    assert len(blocks) == 4 and blocks[-1] == (b"\x03\x00", 0, 0)
    assert [isize for _, _, isize in blocks] == [65280, 65280, 150000 - 2 * 65280, 0]
    assert b"".join(zlib.decompress(p, -15) for p, _, _ in blocks) == data
    assert all(zlib.crc32(zlib.decompress(p, -15)) == crc for p, crc, _ in blocks)
    assert gzip.decompress(whole) == data
    assert tr.bgzf_blocks(tr.bgzf_of(b"")) == [(b"\x03\x00", 0, 0)] and tr.bgzf_of(b"") == tr.BGZF_EOF
    # damaged: a bad magic, a wrong extra field, a size that walks past the end or into a block, no end-of-file block
    for damaged in (b"\x1f\x8c" + whole[2:], whole[:12] + b"XX" + whole[14:], whole[:-1], whole + b"\x00", whole[:-28], b"",
                    whole[:16] + struct.pack("<H", struct.unpack("<H", whole[16:18])[0] + 1) + whole[18:],
                    whole[:16] + struct.pack("<H", 20) + whole[18:]):
        with pytest.raises(ValueError):
            tr.bgzf_blocks(damaged)


def test_options_names_and_refusals(tmp_path, capsys):
    from wisecondor_amd import ingest
    from wisecondor_amd import wisecondor as cli
    p = cli.buildParser()
    a = p.parse_args(["exporttracks", "a_test.npz", "b_test.npz", "out"])
    assert (a.infiles, a.outdir, a.gz, a.nozero, a.only, a.chrprefix, a.chromsizes, a.mineffect, a.batch, a.io) == \
        (["a_test.npz", "b_test.npz"], "out", False, False, None, "chr", None, 0, 64, 8)
    assert a.func is cli.toolExportTracks
    a = p.parse_args(["exporttracks", "a.npz", "out", "-gz", "-nozero", "-only", "r", "-chrprefix", "", "-chromsizes", "hg.sizes",
                      "-mineffect", "1.5", "-batch", "2", "-io", "3"])
    assert (a.gz, a.nozero, a.only, a.chrprefix, a.chromsizes, a.mineffect, a.batch, a.io) == (True, True, "r", "", "hg.sizes", 1.5, 2, 3)
    with pytest.raises(SystemExit):
        p.parse_args(["exporttracks", "a.npz", "out", "-only", "x"])
    capsys.readouterr()
    # the new options stay out of every other command's namespace
    others = {"exportjson": ["a.npz", "out"], "plotbatch": ["a.npz", "out"], "plotpdf": ["a.npz", "out"], "report": ["a.npz", "b.npz"],
              "test": ["a.npz", "b.npz", "ref.npz"], "testbatch": ["a.npz", "out", "ref.npz"], "convert": ["a.bam", "a.npz"],
              "newref": ["a.npz", "ref.npz"]}
    for command, rest in others.items():
        space = vars(p.parse_args([command] + rest))
        assert not {"nozero", "only", "chrprefix", "chromsizes"} & set(space), command
    assert "gz" not in vars(p.parse_args(["plotpdf", "a.npz", "out"]))
    # the names
    J = os.path.join
    assert ingest.tracks_output_names(["x/a_test.npz", "b"], "o") == [(J("o", "a_test_z.bedgraph"), J("o", "a_test_r.bedgraph"), J("o", "a_test_calls.bed")),
                                                                     (J("o", "b_z.bedgraph"), J("o", "b_r.bedgraph"), J("o", "b_calls.bed"))]
    assert ingest.tracks_output_names(["a.npz"], "o", gz=True, only="r") == [(J("o", "a_r.bedgraph.gz"), J("o", "a_calls.bed"))]
    # two inputs with one stem: refused before the directory is made
    outdir = tmp_path / "never"
    with pytest.raises(SystemExit) as stop:
        cli.main(["exporttracks", str(tmp_path / "one" / "s_test.npz"), str(tmp_path / "two" / "s_test.npz"), str(outdir)])
    assert stop.value.code == 2 and not outdir.exists()
    assert "would both be written to s_test_calls.bed" in capsys.readouterr().out
    # a prefix that is too long, a -chromsizes file that is missing or is no such file: the same
    for extra, said in ((["-chrprefix", "x" * 17], "at most 16 ASCII bytes"), (["-chromsizes", str(tmp_path / "none.sizes")], "No such file"),
                        (["-chrprefix", "a\tb"], "at most 16 ASCII bytes")):
        with pytest.raises(SystemExit) as stop:
            cli.main(["exporttracks", str(tmp_path / "s_test.npz"), str(outdir)] + extra)
        assert stop.value.code == 2 and not outdir.exists()
        assert said in capsys.readouterr().out
    bad = tmp_path / "bad.sizes"
    bad.write_text("chr1\t1000\nchr2 2000\n")
    with pytest.raises(SystemExit) as stop:
        cli.main(["exporttracks", str(tmp_path / "s_test.npz"), str(outdir), "-chromsizes", str(bad)])
    assert stop.value.code == 2 and "line 2 is not name<TAB>length" in capsys.readouterr().out


def test_chromosome_sizes_against_the_bins(tmp_path):
    from wisecondor_amd import ingest
    sizes = tmp_path / "hg.sizes"
    sizes.write_text("chr1\t2500\nchr2\t1000\textra\n# a comment\n\nchr3\t1\nchrX\t9\n")
    table = ingest.read_chrom_sizes(str(sizes))
    assert table == {"chr1": 2500, "chr2": 1000, "chr3": 1, "chrX": 9}
    assert ingest.chrom_lengths_for(table, "chr", [3, 1, 0], 1000) == [2500, 1000, 1]
    assert ingest.chrom_lengths_for(table, "chr", [3, 1, 1], 1000) == [2500, 1000, 1]
    with pytest.raises(ValueError, match="no chromosome chr4"):
        ingest.chrom_lengths_for(table, "chr", [3, 1, 0, 0], 1000)
    with pytest.raises(ValueError, match="no chromosome 1"):
        ingest.chrom_lengths_for(table, "", [3], 1000)
    # a chromosome's last bin starts at or beyond its length
    with pytest.raises(ValueError, match="chr2 1000 bases"):
        ingest.chrom_lengths_for(table, "chr", [3, 2, 0], 1000)
    with pytest.raises(ValueError, match="chr1 2500 bases"):
        ingest.chrom_lengths_for(table, "chr", [4, 1, 0], 1000)
