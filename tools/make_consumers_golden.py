#!/usr/bin/env python3
"""Generate tests/golden/consumers.npz by RUNNING the upstream reference's `report` and `plot` on the test .npz
files this build writes (dev container only, like make_goldens.py).

tests/test_consumers_cpu.py writes the same two files (the Python writer and the native batch writer) and holds
them against what is recorded here: the text `report` printed for each, whether `plot` read its inputs, the
layout of each file as the reference loaded it, and the values `report` prints from.  Only data is written
under tests/golden/; no reference source text is.

Run:  python tools/make_consumers_golden.py      (needs the reference sources, see ref_loader.py)
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402
import test_consumers_cpu as tc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    tmp = tempfile.mkdtemp(prefix="wc_consumers_")
    files, sample, _, _ = tc.write_outputs(tmp, lambda name: np.load(os.path.join(GOLD, name), allow_pickle=False))
    _, wc, _ = ref_loader.load()
    convert_out = os.path.join(tmp, "sample.npz")
    quality = dict(mapped=1, unmapped=0, no_coordinate=0, filter_rmdup=0, filter_mapq=0, pre_retro=1,
                   post_retro=1, pair_fail=0)
    binsize = float(np.load(files["python"], allow_pickle=True)["binsize"])
    np.savez_compressed(convert_out, arguments={"binsize": binsize}, runtime={}, sample=sample, quality=quality)
    rec = {}
    for writer, path in sorted(files.items()):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            wc.toolReport(argparse.Namespace(testfile=convert_out, resultfile=path, mineffect=1.5))
        rec["report_" + writer] = np.array(buf.getvalue())
        rec["layout_" + writer] = np.array(tc.layout(path))
        back = np.load(path, allow_pickle=True)
        for key in tc.PRINTED:
            rec["%s_%s" % (writer, key)] = np.asarray(back[key])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            wc.toolPlot(argparse.Namespace(infile=files["python"], outfile=os.path.join(tmp, "plot"), cytofile=None,
                                           chromosomes=list(range(1, 23)), columns=2, filetype="png",
                                           size=[11.7, 8.3], mineffect=1.5))
        assert os.path.getsize(os.path.join(tmp, "plot_z.png")) > 10000
        rec["plot"] = np.array("drawn")
    except AttributeError as e:
        assert "label" in str(e)
        rec["plot"] = np.array("read; stopped at Tick.label")
    np.savez_compressed(os.path.join(GOLD, "consumers.npz"), **rec)
    print("wrote tests/golden/consumers.npz:", ", ".join(sorted(rec)))


if __name__ == "__main__":
    main()
