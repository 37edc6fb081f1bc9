#!/usr/bin/env python3
"""Time `plotbatch`'s GPU path on cohorts a user would plot: 22 panels of human autosomes at 250 kb and at 50 kb bins,
the default figure (11.7 x 8.3 inches at 100 dpi), batches of 64 and 256 samples.

    timeout -k 10 900 python tools/gpu_plot_time.py --out profiles/plot_times.json

Per shape, after one warm-up call, `--repeats` (20) calls of wisetools.plot_batch (host arrays in, PNG bytes out) followed by
the write of the files by the I/O thread pool: every time, median and spread (max - min) of
  the stages of wc_plot_batch between device events: copy in, list, raster, Adler-32, deflate, copy out
  the whole call, the file write, and images per second end to end (call + write)
and, for the sample with the most calls of every shape's cohort: the PNG's size beside zlib levels 1 and 6 of the same scanlines, and
-- where matplotlib is present on the measuring machine -- the time one host core takes to draw the same display list
with it (grey lines, patches, call edge lines and labels, polyline, chromosome numbers, title and legend; Agg, to a PNG
in memory, median of three).  The synthetic samples have runs of masked bins (z == 0) and a few calls each.  No figure is asserted anywhere."""
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

HG19 = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663, 146364022, 141213431, 135534747, 135006516,
        133851895, 115169878, 107349540, 102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566]


def cohort(n, binsize, seed):
    rng = np.random.RandomState(seed)
    sizes = [int(length / binsize + 1) for length in HG19]
    out = []
    for _ in range(n):
        zs, calls = [], []
        for c, bins in enumerate(sizes):
            z = rng.standard_normal(bins)
            for _ in range(max(1, bins // 200)):                       # masked runs, the centromere among them
                at = rng.randint(0, bins)
                z[at:at + rng.randint(1, max(2, bins // 50))] = 0.0
            zs.append(z)
        for _ in range(rng.randint(0, 5)):
            c = rng.randint(0, 22)
            a = rng.randint(0, sizes[c] - 2)
            b = min(sizes[c] - 1, a + rng.randint(1, max(2, sizes[c] // 10)))
            zc = rng.choice([-1, 1]) * rng.uniform(5, 12)
            zs[c][a:b + 1] += np.sign(zc) * 3.0
            calls.append((c + 1, a, b, zc, np.sign(zc) * rng.uniform(0.02, 0.3)))
        out.append(dict(results_z=zs, results_calls=np.array(calls, dtype=np.float64), threshold_z=5.8, binsize=binsize))
    return out


def summary(values, digits=3):
    return {"runs": [round(float(v), digits) for v in values], "median": round(float(np.median(values)), digits),
            "spread": round(float(max(values) - min(values)), digits)}


def matplotlib_time(result, repeats=3):
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
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fig = plt.figure(figsize=(11.7, 8.3), dpi=100)
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
        fig.savefig(io.BytesIO(), format="png")
        plt.close(fig)
        times.append(time.perf_counter() - t0)
    return {"seconds": summary(times, 3), "matplotlib": matplotlib.__version__}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plot_times.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--binsizes", type=int, nargs="+", default=[250000, 50000])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--io", type=int, default=8)
    ap.add_argument("--keep", default=None, help="directory that receives one PNG per bin size (to look at)")
    args = ap.parse_args()
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    stage_names = ["copy_in", "list", "raster", "adler32", "deflate", "copy_out"]
    shapes = []
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.io)

    def write(path, data):
        with open(path, "wb") as f:
            f.write(data)

    for binsize in args.binsizes:
        for batch in args.batches:
            results = cohort(batch, binsize, seed=batch)
            names = ["sample%03d" % i for i in range(batch)]
            wt.plot_batch(results, names, mineffect=1.5)                             # the warm-up
            stages, calls, writes, rates = [], [], [], []
            with tempfile.TemporaryDirectory() as tmp:
                for _ in range(args.repeats):
                    details = {'want_scanlines': False}
                    t0 = time.perf_counter()
                    pngs = wt.plot_batch(results, names, mineffect=1.5, details=details)
                    t1 = time.perf_counter()
                    list(pool.map(write, [os.path.join(tmp, "%s_z.png" % n) for n in names], pngs))
                    t2 = time.perf_counter()
                    stages.append(details['times_ms'][0])
                    calls.append(t1 - t0)
                    writes.append(t2 - t1)
                    rates.append(batch / (t2 - t0))
            # the sample of this cohort with the most calls: its file beside zlib on the same scanlines, and matplotlib on
            # its display list
            pick = int(np.argmax([len(r['results_calls']) for r in results]))
            one = {}
            wt.plot_batch(results[pick:pick + 1], names[pick:pick + 1], mineffect=1.5, details=one)
            scan = one['scanlines'][0].tobytes()
            per_size = {"compared_sample": pick, "its_calls": len(results[pick]['results_calls']), "png_bytes": len(pngs[pick]),
                        "scanline_bytes": len(scan), "zlib_level6_bytes": len(zlib.compress(scan, 6)),
                        "zlib_level1_bytes": len(zlib.compress(scan, 1)), "matplotlib_one_core": matplotlib_time(results[pick])}
            if args.keep:
                os.makedirs(args.keep, exist_ok=True)
                write(os.path.join(args.keep, "plot_%d_%d.png" % (binsize, batch)), pngs[pick])
            shape = {"binsize": binsize, "batch": batch, "bins": int(sum(len(c) for c in results[0]['results_z'])),
                     "image": list(details['size']),
                     "stage_milliseconds": {n: summary([s[i] for s in stages]) for i, n in enumerate(stage_names)},
                     "call_seconds": summary(calls, 4), "file_write_seconds": summary(writes, 4),
                     "images_per_second_end_to_end": summary(rates, 1)}
            med = {n: shape["stage_milliseconds"][n]["median"] for n in stage_names}
            shape["largest_device_stage"] = max(("list", "raster", "adler32", "deflate"), key=lambda n: med[n])
            shape["deflate_gigabytes_per_second"] = round(batch * per_size["scanline_bytes"] / (med["deflate"] * 1e-3) / 1e9, 2)
            shape.update(per_size)
            shapes.append(shape)
            print(json.dumps(shape), flush=True)
    result = {"shapes": shapes, "repeats": args.repeats, "io_threads": args.io, "library": _lib.load().wc_version().decode(),
              "note": "end to end = wisetools.plot_batch from host arrays to PNG bytes (only the compressed streams leave the device) "
                      "plus the write of the files; reading the result files is not in it.  png_bytes, the zlib sizes and the "
                      "matplotlib time belong to one sample of the shape's own cohort (compared_sample)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
