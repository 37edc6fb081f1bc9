"""The compiled kernels of csrc/bamgpu.hip (gfx950 assembly, cross-compiled here), as tests/test_convert_isa_cpu.py does
for convert.hip: every workgroup barrier is reached with the wave's own LDS operations complete (tools/barrier_scan.py),
no kernel uses scratch memory or spills a register, and the kernels of the device reader are all there."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_bamgpu_listing_has_guarded_barriers_and_no_scratch(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "bamgpu.hip" in SOURCES
    out = str(tmp_path / "bamgpu.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "bamgpu.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    # the kernels of one wave per workgroup (inflate, chain, link) keep the fences of their barriers and need no s_barrier
    assert total >= 2, total
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    for want in ("k_bg_inflate", "k_bg_chain", "k_bg_link", "k_bg_begin", "k_bg_walkILb0", "k_bg_walkILb1", "k_bg_scan",
                 "k_bg_order", "k_bg_offsets", "k_bg_advance"):
        assert any(want in n for n in names), (want, names)
    for name, k in zip(names, kernels):
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.sgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.uses_dynamic_stack:\s+(\S+)", k).group(1) == "false", name
    # the Huffman tables live in LDS: about 5 KiB per wave, so the register file and not the LDS bounds the occupancy
    inflate = kernels[[i for i, n in enumerate(names) if "k_bg_inflate" in n][0]]
    assert 4096 <= int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", inflate).group(1)) <= 8192
