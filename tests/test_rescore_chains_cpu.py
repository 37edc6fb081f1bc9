"""Dependent load chains of k_rescore in the compiled code (gfx950 assembly, cross-compiled here), by
tools/load_chain_scan.py as in test_load_chains_cpu.py.

A row's life in k_rescore is a chain of memory round trips.  Behind the counting order there used to be two more, each a
load with a wait of its own: chrom_of_row[row], then chrom_off[] through the number it returned.  The chromosome's range
now comes with the row's first batch (chrom_range[row]), and the only load the register-staged instantiation still
waits for alone is the pair reload of a trip beyond the first (rows with more pairs than the workgroup has threads).
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEQ_STAGED = "9k_rescoreILb1ELb0EE"        # k_rescore<true, false> in the mangled name


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from wisecondor_amd.build import CSRC, FLAGS, _hipcc
    out = str(tmp_path_factory.mktemp("rescore_chains") / "newref.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "newref.hip")],
                          stderr=subprocess.DEVNULL)
    return out


def kernel_text(listing, symbol):
    lines = open(listing).read().split("\n")
    first = [i for i, ln in enumerate(lines) if ln.startswith(symbol + ":")]
    assert len(first) == 1
    last = next(i for i in range(first[0], len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines, first[0], last


def test_one_lone_wait_and_none_behind_the_order(listing):
    import load_chain_scan
    found = {sym: r for sym, r in load_chain_scan.scan(listing).items() if SEQ_STAGED in sym}
    assert len(found) == 1
    sym, r = next(iter(found.items()))
    print("\n".join(load_chain_scan.report(listing, ["k_rescore"])))
    assert len(r["waits"]) <= 1
    # the order ends with the last workgroup barrier of the row: no load of the row that is ordered there may be
    # issued behind it and waited for alone (the output rows are stores).  The lone wait that is left sits in the
    # trip loop, in front of every barrier but the one behind the row's own values.  (The position test reads the
    # TEXT order of the listing, which follows the source here but is the compiler's layout, not control flow: the
    # count above and the shape of the load below carry the claim, the position only says where to look if it moves.)
    lines, first, last = kernel_text(listing, sym)
    barriers = [i + 1 for i in range(first, last) if lines[i].strip().startswith("s_barrier")]
    assert len(barriers) >= 4
    for wait_line, load_line, text in r["waits"]:
        assert wait_line < barriers[1], (wait_line, barriers, text)
        assert re.match(r"global_load_dword\s", text), text          # one pair index per lane


def test_no_scratch_and_the_register_budgets(listing):
    """k_rescore<true, false>: four waves per SIMD (128 registers); k_rescore<false, true>: three (168).  Nothing spilled:
    scratch in the chunk loop costs more than the occupancy it buys."""
    text = open(listing).read()
    meta = text[text.index("amdhsa.kernels:"):]
    for name, budget in ((SEQ_STAGED, 128), ("9k_rescoreILb0ELb1EE", 168)):
        blocks = [b for b in meta.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+\S*%s" % name, b)]
        assert len(blocks) == 1

        def get(key):
            return int(re.search(r"\.%s:\s+(\d+)" % key, blocks[0]).group(1))
        print(name, get("vgpr_count"), get("vgpr_spill_count"), get("private_segment_fixed_size"))
        assert get("vgpr_count") <= budget
        assert get("vgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0
