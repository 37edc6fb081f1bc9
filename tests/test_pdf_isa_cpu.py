"""The compiled kernel of csrc/pdf.hip (gfx950 assembly, cross-compiled here), in the manner of
tests/test_deflate_isa_cpu.py: every workgroup barrier is reached with the wave's own LDS operations complete
(tools/barrier_scan.py), no scratch memory, no spills; the rows leave LDS in 16-byte global stores."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_pdf_listing_has_guarded_barriers_and_no_scratch(tmp_path):
    import barrier_scan
    from wisecondor_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "pdf.hip" in SOURCES and "-ffp-contract=off" in FLAGS
    out = str(tmp_path / "pdf.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.check_call([_hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "pdf.hip")],
                          stderr=subprocess.DEVNULL)
    total, bad = barrier_scan.scan(out)
    assert total == 2, total
    assert not bad, bad[:5]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    assert len(names) == 1 and "k_pdf_content" in names[0], names
    for name, k in zip(names, kernels):
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert re.search(r"\.sgpr_spill_count:\s+(\d+)", k).group(1) == "0", name
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", k).group(1)) == 4096, name
    body = text[:text.index("amdhsa.kernels:")]
    # a span's image is filled and read 16 bytes at a time, and nothing else is stored to global memory
    stores = re.findall(r"^\s+((?:global|flat|buffer)_store_\w+)", body, flags=re.M)
    assert stores == ["global_store_dwordx4"], stores
    assert "ds_write_b128" in body and "ds_read_b128" in body and "ds_write_b8" in body
    # the label digits are the rasteriser's: one routine in one header
    for unit in ("plot.hip", "pdf.hip"):
        source = open(os.path.join(CSRC, unit)).read()
        assert '#include "plot_label.h"' in source and "pl_label_tenths(double" not in source
