"""`convert` / `report` without a GPU: the numpy restatement of convertBam against what the REAL convertBam returned
(tests/golden/convert.npz, made by tools/make_convert_golden.py), `report`'s text against what the reference's
toolReport printed, the converted file through both sample readers, and the CLI surface."""
import argparse
import contextlib
import io
import os

import numpy as np
import pytest

import convert_restated as cr

KEYS = cr.KEYS


def golden_case(g, name):
    """(names, lengths, pos per reference, mapq per reference, binsize, min_shift, threshold, counts dict, quality)"""
    offs = g[name + "_offsets"]
    pos = [g[name + "_pos"][a:b] for a, b in zip(offs[:-1], offs[1:])]
    mapq = [g[name + "_mapq"][a:b] for a, b in zip(offs[:-1], offs[1:])]
    binsize, min_shift, threshold = g[name + "_params"]
    counts, at = {}, 0
    for key, present, bins in zip(KEYS, g[name + "_present"], g[name + "_bins"]):
        counts[key] = g[name + "_counts"][at:at + bins] if present else None
        at += int(bins) if present else 0
    quality = dict(zip([str(k) for k in g["quality_keys"]], [int(v) for v in g[name + "_quality"]]))
    return ([str(n) for n in g[name + "_names"]], [int(v) for v in g[name + "_lengths"]], pos, mapq, float(binsize),
            int(min_shift), int(threshold), counts, quality)


def same_sample(got, want):
    for key in KEYS:
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key] is not None and got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key


def test_golden_covers_what_it_should(golden):
    g = golden("convert.npz")
    names, _, pos, mapq, _, _, _, counts, quality = golden_case(g, "defaults")
    assert {"chr1", "2", "CHR3", "chrM", "GL000207.1", "chrX", "Y"} <= set(names)
    assert counts["5"] is None and counts["X"] is not None and counts["Y"] is not None and not counts["Y"].any()
    two, three, four = names.index("2"), names.index("CHR3"), names.index("chr4")
    assert pos[two][1] == pos[two][0] and pos[three][1] == pos[two][-1]
    assert len(pos[four]) > 3000 and (mapq[four] == 0).sum() > 20
    params = {tuple(g[str(c) + "_params"]) for c in g["cases"]}
    assert {t for _, _, t in params} >= {-1, 0, 1, 4, 7} and {m for _, m, _ in params} >= {-1, 0, 4, 10}
    assert {b for b, _, _ in params} >= {1e6, 1000.0, 333.0, 777.25}


def test_restatement_equals_the_reference(golden):
    g = golden("convert.npz")
    assert len(g["cases"]) >= 12
    for name in g["cases"]:
        names, lengths, pos, mapq, binsize, min_shift, threshold, counts, quality = golden_case(g, str(name))
        got, stats = cr.convert(names, lengths, pos, mapq, binsize, min_shift, threshold)
        same_sample(got, counts)
        for key, value in stats.items():
            assert value == quality[key], (name, key)


def _convert_file(tmp_path, g):
    from wisecondor_amd import wisecondor as cli
    _, _, _, _, binsize, min_shift, threshold, counts, quality = golden_case(g, "defaults")
    args = argparse.Namespace(infile="x.bam", outfile="sample.npz", binsize=binsize, retdist=min_shift, retthres=threshold)
    path = str(tmp_path / "sample.npz")
    cli.writeConvertOutput(path, args, counts, quality)
    return path, counts, binsize


def test_report_prints_the_reference_text(tmp_path, golden):
    from wisecondor_amd import wisecondor as cli
    g = golden("convert.npz")
    converted, _, binsize = _convert_file(tmp_path, g)
    _, z, asdef, aasdef = g["report_scalars"]
    result = str(tmp_path / "result.npz")
    np.savez_compressed(result, arguments={"infile": "sample.npz", "repeats": 5}, runtime={}, binsize=binsize,
                        results_calls=g["report_calls"], threshold_z=np.float64(z), asdef=np.float64(asdef),
                        aasdef=np.float64(aasdef))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["report", converted, result])
    printed = buf.getvalue()
    printed = printed[printed.index("\n# Arguments used in convert"):]       # (main echoes its own arguments first)
    assert printed == str(g["report_text"])


def test_converted_file_loads_through_both_readers(tmp_path, golden):
    from wisecondor_amd import ingest
    g = golden("convert.npz")
    path, counts, binsize = _convert_file(tmp_path, g)
    back = np.load(path, allow_pickle=True)
    assert sorted(back.files) == [str(k) for k in g["file_keys"]]
    assert sorted(back["sample"].item()) == [str(k) for k in g["file_sample_keys"]]
    assert set(str(k) for k in g["file_argument_keys"]) <= set(back["arguments"].item())
    sample, own = ingest.read_sample(path)
    assert own == binsize
    same_sample(sample, counts)
    # the native reader: chromosomes 1..22 padded / truncated to the given sizes (an absent one cannot be read)
    full = {k: (v if v is not None else np.zeros(3, dtype=np.int32)) for k, v in counts.items()}
    path2 = str(tmp_path / "full.npz")
    from wisecondor_amd import wisecondor as cli
    cli.writeConvertOutput(path2, argparse.Namespace(infile="x.bam", outfile=path2, binsize=binsize, retdist=4, retthres=4,
                                                    func=cli.toolConvert), full, {})
    sizes = [len(full[str(c)]) for c in range(1, 23)]
    rows = np.full((1, sum(sizes)), -1, dtype=np.int32)
    slow = []
    own = ingest.read_counts([path2], sizes, binsize, rows, threads=2, fallbacks=slow)
    assert slow == [] and own[0] == binsize
    assert np.array_equal(rows[0], np.concatenate([full[str(c)] for c in range(1, 23)]))


def test_cli_surface_of_the_new_sub_commands():
    from wisecondor_amd import wisecondor as cli
    p = cli.buildParser()
    a = p.parse_args(["convert", "in.bam", "out.npz"])
    assert (a.infile, a.outfile, a.binsize, a.retdist, a.retthres) == ("in.bam", "out.npz", 1e6, 4, 4)
    assert isinstance(a.binsize, float) and a.func is cli.toolConvert
    a = p.parse_args(["convert", "in.bam", "out.npz", "-binsize", "50000", "-retdist", "2", "-retthres", "-1"])
    assert (a.binsize, a.retdist, a.retthres) == (50000.0, 2, -1)
    a = p.parse_args(["convertbatch", "a.bam", "b.bam", "outdir", "-io", "3", "-binsize", "250000"])
    assert (a.infiles, a.outdir, a.io, a.binsize, a.retdist, a.retthres) == (["a.bam", "b.bam"], "outdir", 3, 250000.0, 4, 4)
    assert a.func is cli.toolConvertBatch
    a = p.parse_args(["report", "t.npz", "r.npz"])
    assert (a.testfile, a.resultfile, a.mineffect) == ("t.npz", "r.npz", 1.5) and a.func is cli.toolReport
    assert cli.convert_output_names(["x/a.bam", "y/b.BAM", "c"], "o") == [os.path.join("o", n) for n in ("a.npz", "b.npz", "c.npz")]
    with pytest.raises(ValueError):
        cli.convert_output_names(["x/a.bam", "y/a.bam"], "o")
    with pytest.raises(SystemExit) as e:
        p.parse_args(["plot", "x"]).func(None)
    assert e.value.code == 2
