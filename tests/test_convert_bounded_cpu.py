"""The bounded `convert` without a GPU: the numpy restatement of the sliced rule (tests/convert_sliced_restated.py: the
carry in, the carry out, exactly the state csrc/convert.hip keeps between the slices of a run) against the whole-input
restatements -- which tests/golden/convert.npz and convert_paired.npz pin to the real convertBam -- on random inputs
and random cuts in both modes; and the `-bounded` option of the command line."""
import numpy as np
import pytest

import convert_paired_restated as cpr
import convert_restated as cr
import convert_sliced_restated as csr
from test_convert_paired_cpu import random_paired_stream

NAMES = ["chr%s" % k for k in cr.KEYS[:7]]


def random_input(rng):
    """seven chromosomes, empty and one-read ones among them, towers of every length around the thresholds"""
    lengths = [int(rng.randint(3000, 40000)) for _ in NAMES]
    cols = []
    for length in lengths:
        n = [0, 1, 2, 30, 120][rng.randint(0, 5)]
        towers = [(int(rng.randint(0, length)), int(rng.randint(2, 9)), int(rng.randint(0, 6))) for _ in range(n // 15)]
        if n > 1:
            cols.append(random_paired_stream(rng, length, n, float(rng.choice([0.0, 0.3, 0.9, 1.0])), towers))
        else:
            cols.append((rng.randint(0, length, n), np.full(n, 60), np.full(n, 0x43), rng.randint(0, length, n)))
    return lengths, cols


def whole(lengths, cols, binsize, min_shift, threshold, min_mapq, paired):
    pos, mapq, flag, mate = ([c[i] for c in cols] for i in range(4))
    counts, stats = cpr.convert(NAMES, lengths, pos, mapq, flag, mate, binsize, min_shift, threshold, min_mapq, paired)
    return [counts[cr.chrom_key(n)] for n in NAMES], stats


@pytest.mark.parametrize("block", range(10))
def test_sliced_rule_equals_the_whole_rule_at_random_cuts(block):
    for seed in range(30 * block, 30 * block + 30):
        one_random_input(seed)


def one_random_input(seed):
    rng = np.random.RandomState(9000 + seed)
    lengths, cols = random_input(rng)
    n = sum(len(c[0]) for c in cols)
    binsize = float(rng.choice([100.0, 333.0, 777.25]))
    min_shift, threshold = int(rng.choice([-1, 0, 1, 4, 10])), int(rng.choice([-1, 0, 1, 3, 4, 7, 500]))
    min_mapq, paired = int(rng.choice([0, 1, 20, 61])), bool(seed % 2)
    n_bins = [cr.n_bins(l, binsize) for l in lengths]
    want, want_stats = whole(lengths, cols, binsize, min_shift, threshold, min_mapq, paired)
    if not paired and min_mapq == 1:
        plain = cr.convert(NAMES, lengths, [c[0] for c in cols], [c[1] for c in cols], binsize, min_shift, threshold)
        assert plain[1] == want_stats
    cut_sets = [[], [0], [n], sorted(rng.randint(0, n + 1, 3)), sorted(rng.randint(0, n + 1, int(rng.randint(1, 40)))),
                list(range(n + 1))]
    for cuts in cut_sets:
        got, stats, most = csr.convert_sliced(n_bins, csr.cut(cols, cuts), binsize, min_shift, threshold, min_mapq, paired)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), cuts
        for key in ("filter_rmdup", "filter_mapq", "pre_retro", "post_retro", "pair_fail"):
            assert stats[key] == want_stats[key], (key, cuts)
        assert stats["outside"] == 0
        assert stats["kept"] == stats["pre_retro"] - stats["filter_rmdup"] - stats["filter_mapq"]
        assert most <= max(threshold, 0)


def test_the_carry_is_what_the_design_says():
    """A tower cut inside: the pending positions while it fits the threshold, nothing but its last position once it is
    dead; a chromosome's consumed first read as the last read of a slice; larp skips a one-read chromosome."""
    pos = [np.array([5, 100, 101, 102, 103, 104, 105, 900]), np.array([7]), np.array([50, 900, 900])]
    cols = [(p, np.full(len(p), 60), np.full(len(p), 0x43), np.arange(len(p))) for p in pos]
    n_bins = [1, 1, 1]
    carry, totals = csr.new_carry(), csr.new_totals(n_bins)
    pieces = csr.cut(cols, [4, 6, 9, 10])
    carry = csr.feed(carry, totals, pieces[0], 1000.0, 4, 4)            # 5 | 100 101 102
    assert carry["pend"] == [100, 101, 102] and carry["run_len"] == 3 and (carry["cur"], carry["cur_n"]) == (0, 2)
    carry = csr.feed(carry, totals, pieces[1], 1000.0, 4, 4)            # 103 104: the run is five long, dead
    assert carry["pend"] == [] and carry["run_len"] == 5 and carry["last_kept"] == 104 and totals[1]["post_retro"] == 0
    carry = csr.feed(carry, totals, pieces[2], 1000.0, 4, 4)            # 105 900 | 7: ends on chr2's consumed read
    assert (carry["cur"], carry["cur_n"], carry["larp"]) == (1, 1, 900) and carry["pend"] == [900]
    carry = csr.feed(carry, totals, pieces[3], 1000.0, 4, 4)            # chr3's consumed read alone in a slice
    assert (carry["cur"], carry["cur_n"], carry["larp"]) == (2, 1, 900)  # chr2 had one read: larp is still chr1's
    carry = csr.feed(carry, totals, pieces[4], 1000.0, 4, 4)            # 900 (== larp: a duplicate), 900 (a duplicate)
    counts, stats = csr.finish(carry, totals, 1000.0, 4)
    assert stats["filter_rmdup"] == 2 and stats["post_retro"] == 1 and [int(c.sum()) for c in counts] == [1, 0, 0]
    with pytest.raises(ValueError):
        csr.feed(carry, csr.new_totals(n_bins), pieces[0], 1000.0, 4, 4)


def parse(argv):
    from wisecondor_amd import wisecondor as cli
    return cli.buildParser().parse_args(argv)


def test_bounded_option_parses_and_stays_out_of_the_namespace_unless_given(tmp_path):
    from wisecondor_amd import wisecondor as cli
    for command, rest in (("convert", ["in.bam", "out.npz"]), ("convertbatch", ["a.bam", "b.bam", "outdir"])):
        plain = parse([command] + rest)
        assert not hasattr(plain, "bounded") and not hasattr(plain, "chunk") and not hasattr(plain, "stream")
        args = parse([command] + rest + ["-bounded"])
        assert args.bounded is True and not hasattr(args, "chunk")
        assert cli._convert_route(args) == "bounded"
        args = parse([command] + rest + ["-bounded", "-chunk", "4096"])
        assert args.bounded is True and args.chunk == 4096 and cli._convert_route(args) == "bounded"
        args = parse([command] + rest + ["-stream", "-chunk", "4096"])
        assert cli._convert_route(args) == "stream"
        with pytest.raises(ValueError):
            cli._convert_route(parse([command] + rest + ["-chunk", "4096"]))        # -chunk alone is still refused
        assert cli._convert_route(plain) == "whole"
