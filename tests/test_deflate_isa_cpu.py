"""The compiled kernels of csrc/deflate.hip (gfx950 assembly, cross-compiled here): every workgroup barrier is reached
with the wave's own LDS operations complete (tools/barrier_scan.py, as tests/test_convert_isa_cpu.py does for
convert.hip), and no kernel uses scratch memory or spills -- the Huffman construction's work arrays and the encoder's
tables live in LDS, where a runtime subscript costs nothing."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_deflate_listing_has_guarded_barriers_and_no_scratch(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "deflate.hip" in SOURCES
    out = str(tmp_path / "deflate.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "deflate.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total >= 10, total
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    for want in ("k_df_encode", "k_df_gather", "k_df_assemble"):
        assert any(want in n for n in names), (want, names)
    for name, k in zip(names, kernels):
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.sgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        # the encoder's LDS (input, coded block, tables, Huffman work space) leaves room for three workgroups per CU
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", k).group(1)) <= 48 * 1024, name
