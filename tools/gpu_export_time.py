#!/usr/bin/env python3
"""Time `exportjson`'s GPU path on the cohorts of tools/gpu_plot_time.py (22 human autosomes at 250 kb and at 50 kb bins,
batches of 64 and 256 files) and, in the same session, json.dumps of the same arrays on the host.

    timeout -k 10 900 python tools/gpu_export_time.py --out profiles/export_times.json

Per shape, after one warm-up call each, `--repeats` (5) times:
  wisetools.jsonRows on the batch's z rows: the stages of wc_json_rows between device events (copy in, lengths and scan,
  bytes, copy out)
  wisetools.export_json_batch without and with gz (host arrays in, the files' bytes out; its stages between device events:
  copy in, text, deflate, copy out) followed by the write of the files by the I/O thread pool: files per second end to end
then the files' sizes, the .json.gz size beside gzip level 6 of the same text (first sample), and the baseline:
json.dumps(..., separators=(',', ':')) of the z and r lists of `--baseline-files` (8) of the same files on one core and in
the `--io` thread pool, as files per second.  No figure is asserted anywhere; the baseline is json.dumps, never the code
under test."""
import argparse
import concurrent.futures
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_plot_time import cohort, summary  # noqa: E402


def full_results(batch, binsize):
    rng = np.random.RandomState(batch + 1)
    out = []
    for res in cohort(batch, binsize, seed=batch):
        res = dict(res)
        res['results_r'] = [0.01 * z + 0.001 * rng.standard_normal(len(z)) for z in res['results_z']]
        res['results_cwz'] = rng.standard_normal(len(res['results_z']))
        res['asdef'] = 0.9
        res['aasdef'] = 0.9 * res['threshold_z']
        res['arguments'] = {'binsize': binsize, 'repeats': 5}
        out.append(res)
    return out


def host_dumps(res):
    return len(json.dumps([c.tolist() for c in res['results_z']], separators=(',', ':'))) + \
        len(json.dumps([c.tolist() for c in res['results_r']], separators=(',', ':')))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_times.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--binsizes", type=int, nargs="+", default=[250000, 50000])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--io", type=int, default=8)
    ap.add_argument("--baseline-files", type=int, default=8)
    args = ap.parse_args()
    import torch
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    if not torch.cuda.is_available():
        raise SystemExit("gpu_export_time: no GPU visible; nothing is measured without one")
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.io)

    def write(path, data):
        with open(path, "wb") as f:
            f.write(data)

    shapes = []
    for binsize in args.binsizes:
        for batch in args.batches:
            results = full_results(batch, binsize)
            sizes = [len(c) for c in results[0]['results_z']]
            z_rows = np.stack([np.concatenate(r['results_z']) for r in results])
            wt.jsonRows(z_rows, sizes)                                             # the warm-ups
            wt.export_json_batch(results)
            wt.export_json_batch(results, gz=True)
            row_stages = []
            for _ in range(args.repeats):
                times = []
                wt.jsonRows(z_rows, sizes, times=times)
                row_stages.append(times)
            shape = {"binsize": binsize, "batch": batch, "values_per_row": int(sum(sizes)),
                     "rows_stage_milliseconds": {n: summary([s[i] for s in row_stages]) for i, n in
                                                 enumerate(["copy_in", "lengths_and_scan", "bytes", "copy_out"])}}
            with tempfile.TemporaryDirectory() as tmp:
                for gz in (False, True):
                    stages, calls, writes, rates = [], [], [], []
                    for _ in range(args.repeats):
                        details = {}
                        t0 = time.perf_counter()
                        files = wt.export_json_batch(results, gz=gz, details=details)
                        t1 = time.perf_counter()
                        list(pool.map(write, [os.path.join(tmp, "s%03d.json%s" % (i, ".gz" if gz else "")) for i in range(batch)], files))
                        t2 = time.perf_counter()
                        stages.append(details['times_ms'][0])
                        calls.append(t1 - t0)
                        writes.append(t2 - t1)
                        rates.append(batch / (t2 - t0))
                    key = "gz" if gz else "plain"
                    shape[key] = {"stage_milliseconds": {n: summary([s[i] for s in stages]) for i, n in
                                                         enumerate(["copy_in", "text", "deflate", "copy_out"])},
                                  "call_seconds": summary(calls, 4), "file_write_seconds": summary(writes, 4),
                                  "files_per_second_end_to_end": summary(rates, 1), "file_bytes_first_sample": len(files[0])}
                    if gz:
                        packed = files[0]
                    else:
                        plain = files[0]
            level6 = zlib.compressobj(6, zlib.DEFLATED, 31)
            shape["gzip_level6_bytes_first_sample"] = len(level6.compress(plain) + level6.flush())
            shape["device_gz_over_gzip_level6"] = round(len(packed) / shape["gzip_level6_bytes_first_sample"], 3)
            text_bytes = sum(details['text_bytes'][0])
            shape["text_bytes_first_sample"] = text_bytes
            # the baseline, in this session: json.dumps of the same arrays
            subset = results[:min(args.baseline_files, batch)]
            t0 = time.perf_counter()
            for res in subset:
                host_dumps(res)
            one_core = time.perf_counter() - t0
            t0 = time.perf_counter()
            list(pool.map(host_dumps, subset))
            pooled = time.perf_counter() - t0
            shape["json_dumps_baseline"] = {"files": len(subset), "one_core_seconds": round(one_core, 4),
                                            "one_core_files_per_second": round(len(subset) / one_core, 2),
                                            "io_pool_seconds": round(pooled, 4), "io_pool_files_per_second": round(len(subset) / pooled, 2)}
            shapes.append(shape)
            print(json.dumps({k: v for k, v in shape.items() if k != "rows_stage_milliseconds"})[:600], flush=True)
    result = {"shapes": shapes, "repeats": args.repeats, "io_threads": args.io, "library": _lib.load().wc_version().decode(),
              "note": "end to end = wisetools.export_json_batch from host arrays to the files' bytes plus the write of the files; reading "
                      "the result files is not in it.  rows_stage_milliseconds is wc_json_rows on the batch's z rows alone.  The "
                      "baseline ran in this session on the first files of the same cohort; it makes the text of results_z and "
                      "results_r only.  Figures of different sessions do not compare"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
