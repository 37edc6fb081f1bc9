"""Dependent load chains of k_pick and k_convert in the compiled code (gfx950 assembly, cross-compiled here).

Both kernels move almost nothing and run as one or two rounds of waves: their time is the number of memory round trips
a wave makes one after the other.  tools/load_chain_scan.py counts, per kernel, the `s_waitcnt vmcnt(0)` that wait for a
single load (a round trip of its own) and the loops that hold a load and such a wait (a round trip per iteration).  The
source batches its loads -- unconditional loads of selected indices, pinned by empty asm statements -- and this test
keeps the compiler from quietly undoing that: a load under a lane condition comes back as an exec-masked block with a
wait of its own.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (lone waits, loops with a load and a lone wait) as tools/load_chain_scan.py reports them
PARENT = {"k_pick": (45, 1), "k_convert": (1, 1)}      # commit 83dbf1e (before the batched loads)
CHANGE = {"k_pick": (0, 0), "k_convert": (0, 0)}       # read from the listing of the batched form


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from wisecondor_amd.build import CSRC, FLAGS, _hipcc
    out = str(tmp_path_factory.mktemp("chains") / "newref.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "newref.hip")],
                          stderr=subprocess.DEVNULL)
    return out


@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_fewer_lone_round_trips_than_the_parent(listing, kernel):
    import load_chain_scan
    waits, loops = load_chain_scan.counts(listing)[kernel]
    print("%s: %d lone waits, %d loops (parent %s, recorded %s)" % (kernel, waits, loops, PARENT[kernel], CHANGE[kernel]))
    assert waits + loops < sum(PARENT[kernel])
    assert waits <= CHANGE[kernel][0] and loops <= CHANGE[kernel][1]


def test_scan_reads_a_listing(tmp_path):
    """The scan itself on a hand-written listing: one lone wait in a loop, one batch of two, one counted wait."""
    import load_chain_scan
    text = """
_ZN12_GLOBAL__N_16k_demoEPf:
\tglobal_load_dword v1, v[2:3], off
\tglobal_load_dword v4, v[2:3], off offset:4
\ts_waitcnt vmcnt(0)
.LBB0_1:
\tglobal_load_dword v5, v0, s[0:1]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\ts_cbranch_scc1 .LBB0_1
\tglobal_load_dword v6, v0, s[0:1]
\ts_waitcnt vmcnt(1)
\ts_waitcnt vmcnt(0)
\ts_cbranch_scc1 .LBB0_2
.LBB0_2:
\ts_endpgm
"""
    path = tmp_path / "demo.s"
    path.write_text(text)
    assert load_chain_scan.counts(str(path)) == {"k_demo": (1, 1)}
    found = load_chain_scan.scan(str(path))["_ZN12_GLOBAL__N_16k_demoEPf"]
    assert [w[:2] for w in found["waits"]] == [(8, 7)]
    assert [lp[0] for lp in found["loops"]] == [".LBB0_1"]


def test_k_pick_keeps_its_occupancy(listing):
    """Seven waves per SIMD: at most 72 vector registers, nothing spilled, no scratch."""
    text = open(listing).read()
    meta = text[text.index("amdhsa.kernels:"):]
    blocks = [b for b in meta.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+\S*6k_pickE", b)]
    assert len(blocks) == 1

    def get(key):
        return int(re.search(r"\.%s:\s+(\d+)" % key, blocks[0]).group(1))
    assert get("vgpr_count") <= 72
    assert get("vgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0
