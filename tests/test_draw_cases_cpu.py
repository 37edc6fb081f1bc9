"""The draw rule without a GPU: the generator's known answers (the restatement and wc_philox4x32_host), the properties of
the rule on the restatement, the conditions the designed input of draw_cases.py meets, the plan maker, the table and the
command line with depths, and the resources of the compiled kernels of csrc/draw.hip."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import call_cases as cc
import draw_cases as dc
import draw_restated as dr
import spike_cases as sc
import spike_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


def hexed(words):
    return [" ".join("%08x" % w for w in row) for row in words]


def host_words(counters, keys):
    from wisecondor_amd import _lib
    counters = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros_like(counters)
    assert _lib.load().wc_philox4x32_host(_lib.ptr(counters), _lib.ptr(keys), len(counters), _lib.ptr(out)) == 0
    return out


# ------------------------------------------------------------------------------------------ the generator ----
def test_known_answers():
    counters, keys = [k[0] for k in KNOWN], [k[1] for k in KNOWN]
    assert hexed(dr.philox(counters, keys)) == [k[2] for k in KNOWN]
    assert hexed(host_words(counters, keys)) == [k[2] for k in KNOWN]


def test_host_generator_equals_the_restatement():
    rng = np.random.RandomState(11)
    counters = rng.randint(0, 2 ** 32, size=(10000, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.randint(0, 2 ** 32, size=(10000, 2), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(host_words(counters, keys), dr.philox(counters, keys))
    assert dr.key_of(dc.HIGH_SEED) == (0x7F4A7C15, 0x9E3779B9) and dr.key_of(-1) == (0xFFFFFFFF, 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the rule ----
def test_draw_on_hand_written_words():
    # T(1) = 4294, T(999 999) = 2^32 - 4295 (floor), T(1 000 000) = 2^32: above every word
    assert [dr.threshold(f) for f in (0, 1, 999999, 1000000)] == [0, 4294, 2 ** 32 - 4295, 2 ** 32]
    words = [0, 4293, 4294, 2 ** 32 - 4296, 2 ** 32 - 4295, 2 ** 32 - 1, 5]
    want = {0: [0, 0, 0, 0, 0], 1: [0, 1, 2, 2, 2], 999999: [0, 1, 3, 4, 4], 1000000: [0, 1, 3, 4, 5]}
    for f, kept in want.items():
        assert [dr.kept_of_words(words, c, f) for c in (0, 1, 3, 4, 5)] == kept, f
    # the vectorised draw is that count on the bin's own words, read r taking word r & 3 of block r >> 2
    for c in (0, 1, 3, 4, 5, 9):
        mine = dr.bin_words(c, 17, 3, dr.TAG_THIN, 2, 99)
        assert len(mine) == c
        blocks = dr.philox([[17, 3 | 1 << 16, j, 2] for j in range((c + 3) // 4)] or np.zeros((0, 4)), dr.key_of(99)).reshape(-1)
        assert np.array_equal(mine, blocks[:c])
        for f in (0, 1, 400000, 999999, 1000000):
            counts = np.array([7, c, 2])
            got = dr.draw_segment(counts, 16, 3, dr.TAG_THIN, 2, 99, [f])[0]
            assert got[1] == dr.kept_of_words(mine, c, f), (c, f)
    # the tag, the chromosome, the bin, the row and the seed each change the words
    first = dr.bin_words(8, 17, 3, dr.TAG_THIN, 2, 99)
    for other in (dr.bin_words(8, 17, 3, dr.TAG_SPIKE, 2, 99), dr.bin_words(8, 17, 4, dr.TAG_THIN, 2, 99), dr.bin_words(8, 18, 3, dr.TAG_THIN, 2, 99),
                  dr.bin_words(8, 17, 3, dr.TAG_THIN, 3, 99), dr.bin_words(8, 17, 3, dr.TAG_THIN, 2, 99 + 2 ** 32)):
        assert not np.array_equal(first, other)


def test_thinned_rows_are_nested_and_the_whole_depth_is_a_copy():
    base, sizes = dc.thin_base(3, 1), dc.thin_sizes(1)
    keep = [1000000, 750000, 500000, 100000, 1]
    out = dr.thin(base, sizes, keep, 1)
    assert np.array_equal(out[0], base)
    for k in range(4):
        assert (out[k + 1] <= out[k]).all()
    assert (out[1] < out[0]).any() and (out[4][base >= 0] <= 1).all()
    negative = base < 0
    assert negative.any() and all(np.array_equal(out[k][negative], base[negative]) for k in range(5))
    # a draw names chromosome and bin, not the layout: the same chromosome behind another one gives the same counts
    moved = dr.thin(np.concatenate([base[:, 8:], base[:, :8]], axis=1), np.array([0, 0, sizes[2], 7, 1]), keep, 1)
    assert np.array_equal(moved[:, :, :sizes[2]], out[:, :, 8:])
    assert not np.array_equal(moved[1, :, sizes[2]:], out[1, :, :8])


def test_spike_with_a_whole_multiple_is_the_deterministic_rule():
    for n_base, r in ((1, 0), (3, 3)):
        base, sizes, plan = dc.spike_base(n_base, r), dc.spike_sizes(r), dc.spike_plan(n_base, r)
        got, saturated = dc.spike_want(n_base, r, 1, 0)
        fixed = np.isin(plan[:, 4], [2000000, -1000000, 100000000, 0])
        want, want_saturated = sr.spike(base, sizes, plan[fixed])
        assert fixed.sum() >= 20 and np.array_equal(got[fixed], want)
        assert saturated == want_saturated == 1                     # the clip and its count: CLIP_COUNT x 101
        clip = [i for i, row in enumerate(plan.tolist()) if row[1:] == [4, 498, 5, 100000000]][0]
        assert got[clip, 9 + 500] == 2 ** 31 - 1 and got[clip + 1, 9 + 500] == 3 * dc.CLIP_COUNT
        lost = plan[:, 4] == -1000000                                # the loss of everything is 0 (negative counts stay)
        for i in np.flatnonzero(lost):
            b, _, first, bins, _ = plan[i].tolist()
            lo = int(np.concatenate([[0], np.cumsum(sizes)])[plan[i, 1] - 1]) + first
            seg = base[b, lo:lo + bins]
            assert np.array_equal(got[i, lo:lo + bins], np.where(seg < 0, seg, 0))
        # between the whole multiples the value lies between them, and the rows outside the span are copies
        weak = [i for i, row in enumerate(plan.tolist()) if row[3] == 300 and row[4] == 25000][0]
        b = plan[weak, 0]
        added = got[weak].astype(np.int64) - base[b]
        assert (added[:109] == 0).all() and (added[409:] == 0).all()
        assert (added[109:409] >= 0).all() and (added[109:409] <= base[b, 109:409]).all()
    # the row id is the GLOBAL plan row: trial0 moves every draw
    assert not np.array_equal(dc.spike_want(3, 1, 1, 0)[0], dc.spike_want(3, 1, 1, 7)[0])
    part = dr.spike_draw(dc.spike_base(3, 1), dc.spike_sizes(1), dc.spike_plan(3, 1)[7:], 1, 7)[0]
    assert np.array_equal(part, dc.spike_want(3, 1, 1, 0)[0][7:])


def test_the_designed_input_meets_its_conditions():
    """Conditions on the INPUT (draw_cases.DESIGNED), by the restatement: a different seed or input is checked the same
    way before it is used.  Measured with this input: -0.04, -0.76, -0.17 standard deviations; 1.013, 1.000, 0.995."""
    counts, thinned = dc.designed_counts(), dc.designed_thinned()
    total = int(counts.sum())
    for f, row in zip(dc.DESIGNED["depths"], thinned):
        p = f / 1e6
        off = (int(row.sum()) - total * p) / np.sqrt(total * p * (1 - p))
        z = (row - counts * p) / np.sqrt(counts * p * (1 - p))
        print("depth %d ppm: total %+.3f sd, per bin mean %+.4f sd %.4f" % (f, off, z.mean(), z.std()))
        assert abs(off) < 6
        assert abs(z.mean()) < 0.1 and 0.9 < z.std() < 1.1
    assert (thinned[1] <= thinned[0]).all() and (thinned[2] <= thinned[1]).all()


# --------------------------------------------------------------------------- plan, table, command line ----
@pytest.fixture(scope="module")
def se():
    from wisecondor_amd import sensitivity
    return sensitivity


@pytest.fixture(scope="module")
def ref():
    return cc.reference_of(sc.lay(), sc.base_samples()[0])


def test_plan_with_depths_repeats_the_same_placements(se, ref):
    one = se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=4)
    assert np.array_equal(one, se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=4, n_depths=1))
    many = se.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=4, n_depths=4)
    block = len(one) // 3
    assert many.dtype == np.int32 and many.shape == (4 * len(one), 5)
    for b in range(3):
        for d in range(4):
            mine = many[(b * 4 + d) * block:(b * 4 + d + 1) * block]
            assert (mine[:, 0] == d * 3 + b).all()
            assert np.array_equal(mine[:, 1:], one[b * block:(b + 1) * block, 1:])
    from wisecondor_amd import wisetools as wt
    assert np.array_equal(many, wt.makePlan(ref, 3, [5, 40], [2500000, -50000], 6, seed=4, n_depths=4))
    with pytest.raises(ValueError, match="empty grid"):
        se.makePlan(ref, 3, [5], [2500000], 6, n_depths=0)


def test_table_with_depths_on_hand_written_records(se):
    # two samples, two depths: base rows 0, 1 at depth 0 and 2, 3 at depth 1; length 4: ceil(0.5 * 4) = 2
    plan = np.array([[0, 1, 0, 1, 0], [0, 1, 10, 4, 50000], [2, 1, 0, 1, 0], [2, 1, 10, 4, 50000],
                     [1, 1, 0, 1, 0], [1, 1, 20, 4, 50000], [3, 1, 0, 1, 0], [3, 1, 20, 4, 50000]], dtype=np.int32)
    rec_i = np.array([[0, 0, 0, 0, -1, -1, -1, 0], [1, 1, 4, 4, 0, 10, 13, 0], [3, 0, 0, 0, -1, -1, -1, 0], [2, 1, 1, 1, 0, 10, 10, 0],
                      [2, 0, 0, 0, -1, -1, -1, 0], [1, 1, 2, 2, 0, 20, 21, 0], [1, 0, 0, 0, -1, -1, -1, 0], [0, 0, 0, 0, -1, -1, -1, 0]],
                     dtype=np.int32)
    nan = float("nan")
    rec_f = np.array([[nan, nan], [8.0, 0.05], [nan, nan], [5.5, 0.02], [nan, nan], [6.0, 0.04], [nan, nan], [nan, nan]])
    table = se.sensitivityTable(plan, rec_i, rec_f, [4], [50000], minoverlap=0.5, depths_ppm=[1000000, 250000], n_samples=2)
    want = np.array([
        [1000000, 4, 50000, 2, 2, 1.0, 7.0, (0.05 + 0.04) / 2, (4 / 4 + 2 / 4) / 2, 0.0],
        [1000000, 0, 0, 2, 0, nan, nan, nan, nan, 1.0],
        [250000, 4, 50000, 2, 0, 0.0, nan, nan, (1 / 4 + 0) / 2, 0.5],
        [250000, 0, 0, 2, 0, nan, nan, nan, nan, 2.0]])
    assert table.shape == (4, 1 + len(se.TABLE_COLUMNS))
    assert np.allclose(table, want, rtol=1e-15, atol=0, equal_nan=True), table
    for d, rows in enumerate((plan[:, 0] < 2, plan[:, 0] >= 2)):
        assert np.array_equal(table[2 * d:2 * d + 2, 1:], sr.table(plan[rows], rec_i[rows], rec_f[rows], [4], [50000], 0.5), equal_nan=True)
    lines = se.tableText(table).strip("\n").split("\n")
    assert lines[0].split("\t") == [se.DEPTH_COLUMN] + list(se.TABLE_COLUMNS) and lines[1].split("\t")[:5] == ["1000000", "4", "50000", "2", "2"]
    assert np.array_equal(np.array([[float(v) for v in line.split("\t")] for line in lines[1:]]), table, equal_nan=True)
    # without depths: the table and its text as they always were
    plain = se.sensitivityTable(plan[:2], rec_i[:2], rec_f[:2], [4], [50000])
    assert plain.shape == (2, len(se.TABLE_COLUMNS)) and se.tableText(plain).split("\n")[0].split("\t") == list(se.TABLE_COLUMNS)
    with pytest.raises(ValueError, match="n_samples"):
        se.sensitivityTable(plan, rec_i, rec_f, [4], [50000], depths_ppm=[1000000, 250000])


def test_depths_of_the_command_line(se):
    assert se.parseDepths("1,0.5,0.25") == [1000000, 500000, 250000]
    assert se.parseDepths("0.000001,0.1234567") == [1, 123457]
    assert len(se.parseDepths(",".join("0.%d" % i for i in range(1, 9)))) == 8
    for bad in ("", ",", "0", "-0.5", "1.0000001", "nan", "inf", "x", "0.0000004", "0.5,0.5", "0.5,0.5000001",
                ",".join("0.%d" % i for i in range(1, 10))):
        with pytest.raises(ValueError):
            se.parseDepths(bad)


def test_new_options_stay_out_of_the_namespace_unless_given():
    from wisecondor_amd import wisecondor as cli
    base = ["sensitivity", "a.npz", "out", "ref.npz", "-lengths", "1e6", "-effects", "5"]
    args = cli.buildParser().parse_args(base)
    assert not hasattr(args, "depths") and not hasattr(args, "draw")
    args = cli.buildParser().parse_args(base + ["-depths", "1,0.5,0.25", "-draw", "-seed", "7"])
    assert args.depths == "1,0.5,0.25" and args.draw is True and args.seed == 7
    args = cli.buildParser().parse_args(["downsample", "in.npz", "out.npz", "-fraction", "0.25"])
    assert args.func is cli.toolDownsample and (args.infile, args.outfile, args.fraction, args.seed) == ("in.npz", "out.npz", 0.25, 1)
    assert not hasattr(args, "reads")
    args = cli.buildParser().parse_args(["downsample", "in.npz", "out.npz", "-reads", "5000000", "-seed", "3"])
    assert args.reads == 5000000 and args.seed == 3 and not hasattr(args, "fraction")
    for bad in ([], ["-fraction", "0.5", "-reads", "7"], ["-fraction", "x"]):
        with pytest.raises(SystemExit) as stop:
            cli.buildParser().parse_args(["downsample", "in.npz", "out.npz"] + bad)
        assert stop.value.code == 2
    sub = [a for a in cli.buildParser()._actions if hasattr(a, "choices") and a.choices][0].choices["downsample"]
    assert "draw around N" in " ".join(sub.format_help().split())


@pytest.mark.parametrize("options, word", [
    (["-depths", "0"], "a depth of 0.0"), (["-depths", "1.5"], "a depth of 1.5"), (["-depths=-0.5"], "a depth of -0.5"),
    (["-depths", "abc"], "not a comma separated list"), (["-depths", "0.0000004"], "a depth of 4e-07"), (["-depths", "0.5,0.5"], "twice"),
    (["-depths", ",".join("0.%d" % i for i in range(1, 10))], "got 9"), (["-depths", ","], "got 0"),
])
def test_depth_refusals_exit_with_status_2(tmp_path, capsys, options, word):
    from wisecondor_amd import wisecondor as cli
    paths, ref_path = sc.write_cli_files(tmp_path)
    with pytest.raises(SystemExit) as stop:
        cli.main(["sensitivity"] + paths[:2] + [str(tmp_path / "out"), ref_path, "-lengths", "5e6", "-effects", "5"] + options)
    assert stop.value.code == 2
    out = capsys.readouterr().out
    assert "ERROR:" in out and word in out, out
    assert not (tmp_path / "out.npz").exists() and not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("options, word", [
    (["-fraction", "0"], "-fraction 0.0"), (["-fraction", "1.5"], "-fraction 1.5"), (["-fraction", "0.0000004"], "-fraction 4e-07"),
    (["-reads", "0"], "-reads 0"), (["-reads", "-3"], "-reads -3"),
])
def test_downsample_refusals_exit_with_status_2(tmp_path, capsys, options, word):
    from wisecondor_amd import wisecondor as cli
    paths, _ = sc.write_cli_files(tmp_path)
    with pytest.raises(SystemExit) as stop:
        cli.main(["downsample", paths[0], str(tmp_path / "out.npz")] + options)
    assert stop.value.code == 2
    out = capsys.readouterr().out
    assert "ERROR:" in out and word in out, out
    assert not (tmp_path / "out.npz").exists()


def test_downsample_refuses_a_key_that_is_no_chromosome_number(tmp_path, capsys):
    from wisecondor_amd import wisecondor as cli
    for key, word in (("X", "not a number"), ("65", "outside 1 .. 64"), ("0", "outside 1 .. 64")):
        odd = str(tmp_path / "odd.npz")
        np.savez_compressed(odd, arguments={"binsize": 1e6}, runtime={}, sample={"1": np.arange(5), key: np.arange(3)}, quality={})
        with pytest.raises(SystemExit) as stop:
            cli.main(["downsample", odd, str(tmp_path / "out.npz"), "-fraction", "0.5"])
        assert stop.value.code == 2 and word in capsys.readouterr().out


# ------------------------------------------------------------------------------------------- the listing ----
def test_draw_listing_has_guarded_barriers_and_the_recorded_resources(tmp_path):
    """As test_spike_isa_cpu.py does for spike.hip: every workgroup barrier guarded (the kernels have none), no scratch, no
    spill, no LDS, and the figures profiles/spike_kernel_resources.txt records.  The listing is searched for nothing else."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "draw.hip" in SOURCES
    out = str(tmp_path / "draw.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "draw.hip")], stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total == 0 and not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in meta.split("  - .agpr_count:")[1:]:
        k = ".agpr_count:" + k
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))      # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", k).group(1)
        short = re.search(r"k_(thin_check|thin|draw_patch|philox_spin|philox)", name).group(0)
        if short == "k_thin":
            short += "<%s>" % re.search(r"k_thinILi(\d+)E", name).group(1)
        seen[short] = dict(vgpr=get("vgpr_count"), agpr=get("agpr_count"), spill=get("vgpr_spill_count"),
                           scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"), sgpr=get("sgpr_count"))
        assert get("sgpr_spill_count") == 0, short
    recorded = {}
    for line in open(os.path.join(ROOT, "profiles", "spike_kernel_resources.txt")):
        m = re.match(r"(k_(?:thin|draw|philox)\S*)\s+vgpr\s+(\d+) agpr\s+(\d+) spill\s+(\d+) scratch\s+(\d+) lds\s+(\d+) sgpr\s+(\d+)", line)
        if m:
            recorded[m.group(1)] = dict(zip(("vgpr", "agpr", "spill", "scratch", "lds", "sgpr"), (int(v) for v in m.groups()[1:])))
    assert sorted(seen) == sorted(["k_thin_check", "k_draw_patch", "k_philox", "k_philox_spin"] + ["k_thin<%d>" % n for n in range(1, 9)])
    assert seen == recorded
    for name, figures in seen.items():
        assert figures["scratch"] == 0 and figures["spill"] == 0 and figures["lds"] == 0, name
