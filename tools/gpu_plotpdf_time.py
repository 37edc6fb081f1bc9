#!/usr/bin/env python3
"""Time `plotpdf`'s GPU path on the cohorts of tools/gpu_plot_time.py (22 panels of human autosomes at 250 kb and at 50 kb
bins, the default page of 11.7 x 8.3 inches, batches of 64 and 256 samples) and, in the same session, `plotbatch` on them.

    timeout -k 10 900 python tools/gpu_plotpdf_time.py --out profiles/plotpdf_times.json

Per shape, after one warm-up call, `--repeats` (20) calls of wisetools.plot_pdf_batch (host arrays in, PDF bytes out) followed
by the write of the files by the I/O thread pool: every time, median and spread (max - min) of
  the stages of wc_plot_pdf_batch between device events: copy in, list (with the counts' way back), content, Adler-32,
  deflate, copy out
  the whole call, the file write, and files per second end to end (call + write)
then row_bytes, the bytes per second k_pdf_content writes, the file's size beside zlib level 6 of the same content (for the
sample with the most calls), the same number of plot_batch calls (whole call only), and -- where matplotlib is present --
the time one host core takes to draw that sample's display list with matplotlib's PDF backend (median of three).  No figure
is asserted anywhere."""
import argparse
import concurrent.futures
import io
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_plot_time import cohort, summary  # noqa: E402


def matplotlib_pdf_time(result, repeats=3):
    try:
        import matplotlib
        matplotlib.use("agg")
        import matplotlib.patches
        import matplotlib.pyplot as plt
    except Exception:
        return None
    import plot_restated as pr
    lists = pr.display_list(result['results_z'], result['results_calls'], result['threshold_z'], range(1, 23), 1.5)
    thr = result['threshold_z']
    times, size = [], 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        fig = plt.figure(figsize=(11.7, 8.3))
        for p, ent in enumerate(lists):
            ax = fig.add_subplot(11, 2, p + 1)
            ax.set_xlim(0, ent[0, 3])
            for y in (0, thr, -thr):
                ax.axhline(y=y, linewidth=0.75, color=(0.7, 0.7, 0.7))
            ax.xaxis.set_ticklabels([])
            for e in ent[1:]:
                colour = tuple(v / 255.0 for v in pr.PALETTE[int(e[6])])
                ax.add_patch(matplotlib.patches.Rectangle((e[2], min(e[4], e[5])), e[3] - e[2], abs(e[5] - e[4]), color=colour,
                                                          alpha=e[7]))
                if e[0] == pr.CALL:
                    ax.axvline(x=e[2], linewidth=0.5, color=colour)
                    ax.axvline(x=e[3], linewidth=0.5, color=colour)
                    ax.text(e[2] + (e[3] - e[2]) / 2, e[5], pr.label_text(e[8]), fontsize=8,
                            verticalalignment='top' if e[8] > 0 else 'bottom', horizontalalignment='center')
            ax.plot(result['results_z'][p], color=(0, 0.45, 0.70), linewidth=0.5)
            ax.set_ylabel(p + 1)
        fig.text(0.5, 0.93, pr.TITLE + 'sample000', ha='center', va='bottom')
        fig.legend([plt.Rectangle((0, 0), 1, 1, fc=tuple(v / 255.0 for v in pr.PALETTE[c])) for _, c in pr.LEGEND],
                   [text for text, _ in pr.LEGEND], loc='lower center', prop={'size': 8}, ncol=2)
        buf = io.BytesIO()
        fig.savefig(buf, format="pdf")
        plt.close(fig)
        times.append(time.perf_counter() - t0)
        size = len(buf.getvalue())
    return {"seconds": summary(times, 3), "pdf_bytes": size, "matplotlib": matplotlib.__version__}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plotpdf_times.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--binsizes", type=int, nargs="+", default=[250000, 50000])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--io", type=int, default=8)
    ap.add_argument("--keep", default=None, help="directory that receives one PDF per bin size (to look at)")
    args = ap.parse_args()
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    stage_names = ["copy_in", "list", "content", "adler32", "deflate", "copy_out"]
    shapes = []
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.io)

    def write(path, data):
        with open(path, "wb") as f:
            f.write(data)

    for binsize in args.binsizes:
        for batch in args.batches:
            results = cohort(batch, binsize, seed=batch)
            names = ["sample%03d" % i for i in range(batch)]
            wt.plot_pdf_batch(results, names, mineffect=1.5)                          # the warm-up
            stages, calls, writes, rates = [], [], [], []
            with tempfile.TemporaryDirectory() as tmp:
                for _ in range(args.repeats):
                    details = {'want_content': False}
                    t0 = time.perf_counter()
                    pdfs = wt.plot_pdf_batch(results, names, mineffect=1.5, details=details)
                    t1 = time.perf_counter()
                    list(pool.map(write, [os.path.join(tmp, "%s_z.pdf" % n) for n in names], pdfs))
                    t2 = time.perf_counter()
                    stages.append(details['times_ms'][0])
                    calls.append(t1 - t0)
                    writes.append(t2 - t1)
                    rates.append(batch / (t2 - t0))
            # plotbatch on the same cohort in the same session: figures of different sessions do not compare
            wt.plot_batch(results, names, mineffect=1.5)
            png_calls = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                pngs = wt.plot_batch(results, names, mineffect=1.5, details={'want_scanlines': False})
                png_calls.append(time.perf_counter() - t0)
            pick = int(np.argmax([len(r['results_calls']) for r in results]))
            row_bytes = details['row_bytes'][0]
            one = {}
            alone = wt.plot_pdf_batch(results[pick:pick + 1], names[pick:pick + 1], mineffect=1.5, details=one)[0]
            content = one['content'][0]
            shape = {"binsize": binsize, "batch": batch, "bins": int(sum(len(c) for c in results[0]['results_z'])),
                     "page_centipoints": list(details['size']), "row_bytes": row_bytes,
                     "stage_milliseconds": {n: summary([s[i] for s in stages]) for i, n in enumerate(stage_names)},
                     "call_seconds": summary(calls, 4), "file_write_seconds": summary(writes, 4),
                     "files_per_second_end_to_end": summary(rates, 1),
                     "plotbatch_call_seconds_same_session": summary(png_calls, 4)}
            med = {n: shape["stage_milliseconds"][n]["median"] for n in stage_names}
            shape["largest_device_stage"] = max(("list", "content", "adler32", "deflate"), key=lambda n: med[n])
            shape["content_gigabytes_per_second"] = round(batch * row_bytes / (med["content"] * 1e-3) / 1e9, 2)
            shape["deflate_gigabytes_per_second"] = round(batch * row_bytes / (med["deflate"] * 1e-3) / 1e9, 2)
            shape.update({"compared_sample": pick, "its_calls": len(results[pick]['results_calls']), "pdf_bytes": len(pdfs[pick]), "pdf_bytes_drawn_alone": len(alone),
                          "png_bytes": len(pngs[pick]), "content_bytes": len(content),
                          "zlib_level6_bytes": len(zlib.compress(content, 6)), "matplotlib_pdf_one_core": matplotlib_pdf_time(results[pick])})
            if args.keep:
                os.makedirs(args.keep, exist_ok=True)
                write(os.path.join(args.keep, "plot_%d_%d.pdf" % (binsize, batch)), pdfs[pick])
            shapes.append(shape)
            print(json.dumps(shape), flush=True)
    result = {"shapes": shapes, "repeats": args.repeats, "io_threads": args.io, "library": _lib.load().wc_version().decode(),
              "note": "end to end = wisetools.plot_pdf_batch from host arrays to PDF bytes (only the compressed streams leave the "
                      "device) plus the write of the files; reading the result files is not in it.  pdf_bytes, png_bytes, the zlib "
                      "size and the matplotlib time belong to one sample of the shape's own cohort (compared_sample).  The "
                      "plotbatch calls ran in this session, behind the plotpdf calls of the same shape"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
