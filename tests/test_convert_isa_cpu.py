"""The compiled kernels of csrc/convert.hip (gfx950 assembly, cross-compiled here): every workgroup barrier is
reached with the wave's own LDS operations complete (tools/barrier_scan.py, as tests/test_isa_cpu.py does for the
other sources), and no kernel uses scratch memory or spills."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_convert_listing_has_guarded_barriers_and_no_scratch(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, _hipcc
    out = str(tmp_path / "convert.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "convert.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total >= 12, total
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    for want in ("k_cv_tables", "k_cv_flags", "k_cv_scan", "k_cv_compact", "k_cv_heads", "k_cv_count"):
        assert any(want in n for n in names), (want, names)
    for name, k in zip(names, kernels):
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
