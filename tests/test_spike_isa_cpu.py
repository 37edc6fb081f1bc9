"""The compiled kernels of csrc/spike.hip (gfx950 assembly, cross-compiled here): every workgroup barrier is reached
with the wave's own LDS operations complete (tools/barrier_scan.py; the two kernels have none, and the scan says so), and
registers, scratch, spills and LDS are what profiles/spike_kernel_resources.txt records.  The listing is searched for
nothing else."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_spike_listing_has_guarded_barriers_and_the_recorded_resources(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "spike.hip" in SOURCES
    out = str(tmp_path / "spike.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "spike.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total == 0                       # a wave per trial, a lane per quad: neither kernel synchronises a workgroup
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in meta.split("  - .agpr_count:")[1:]:
        k = ".agpr_count:" + k
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))      # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", k).group(1)
        short = re.search(r"k_spike(_score)?", name).group(0)
        seen[short] = dict(vgpr=get("vgpr_count"), agpr=get("agpr_count"), spill=get("vgpr_spill_count"),
                           scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"), sgpr=get("sgpr_count"))
        assert get("sgpr_spill_count") == 0, short
    recorded = {}
    for line in open(os.path.join(ROOT, "profiles", "spike_kernel_resources.txt")):
        m = re.match(r"(k_spike\w*)\s+vgpr\s+(\d+) agpr\s+(\d+) spill\s+(\d+) scratch\s+(\d+) lds\s+(\d+) sgpr\s+(\d+)", line)
        if m:
            recorded[m.group(1)] = dict(zip(("vgpr", "agpr", "spill", "scratch", "lds", "sgpr"), (int(v) for v in m.groups()[1:])))
    assert sorted(seen) == ["k_spike", "k_spike_score"]
    assert seen == recorded
    for name, figures in seen.items():
        assert figures["scratch"] == 0 and figures["spill"] == 0 and figures["lds"] == 0, name
