#!/usr/bin/env python3
"""Time `exporttracks`' GPU path on the cohorts of tools/gpu_plot_time.py (22 human autosomes at 250 kb and at 50 kb bins,
batches of 64 and 256 files) and, in the same session, `exportjson -gz`'s deflate stage on the same files and the Python
restatement (tests/tracks_restated.py) of the same tracks on the host.

    timeout -k 10 1100 python tools/gpu_tracks_time.py --out profiles/tracks_times.json

Per shape, after one warm-up call each, `--repeats` (5) times:
  wisetools.bedgraphRows on the batch's z rows: the stages of wc_bedgraph_rows between device events (copy in, lengths and
  scan, bytes, copy out)
  wisetools.export_tracks_batch plain and gz, each without and with nozero (host arrays in, the files' bytes out; its
  stages between device events: copy in, text, BGZF, copy out) followed by the write of the files by the I/O thread
  pool: files per second end to end
  wisetools.export_json_batch with gz: its deflate stage, the same encoder in its raw framing (one call per GPU call,
  the lengths read on the device), beside the BGZF stage above, per batch
then the .bedgraph.gz size beside zlib level 6 of the same text cut into BGZF blocks of 65 280 bytes on the host (first
sample), and the baseline: tracks_restated.track_text of the z and r rows of `--baseline-files` (8) of the same files on
one core, as files per second.  No figure is asserted anywhere; the baseline is the restatement, never the code under test."""
import argparse
import concurrent.futures
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gpu_export_time import full_results  # noqa: E402
from gpu_plot_time import summary  # noqa: E402
import tracks_restated as tr  # noqa: E402


def host_tracks(res, sizes):
    return sum(len(tr.track_text(np.concatenate(res['results_' + key]), sizes, res['binsize'])[0]) for key in ('z', 'r'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_times.json"))
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
        raise SystemExit("gpu_tracks_time: no GPU visible; nothing is measured without one")
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.io)

    def write(path, data):
        with open(path, "wb") as f:
            for part in data:
                f.write(part)

    shapes = []
    for binsize in args.binsizes:
        for batch in args.batches:
            results = full_results(batch, binsize)
            sizes = [len(c) for c in results[0]['results_z']]
            z_rows = np.stack([np.concatenate(r['results_z']) for r in results])
            wt.bedgraphRows(z_rows, sizes, binsize)                                 # the warm-ups
            for gz in (False, True):
                wt.export_tracks_batch(results, gz=gz)
            wt.export_json_batch(results, gz=True)
            row_stages = []
            for _ in range(args.repeats):
                times = []
                wt.bedgraphRows(z_rows, sizes, binsize, times=times)
                row_stages.append(times)
            shape = {"binsize": binsize, "batch": batch, "bins_per_row": int(sum(sizes)),
                     "row_bound_bytes": wt.bedgraphRowBound(sizes, binsize, 3),
                     "rows_stage_milliseconds": {n: summary([s[i] for s in row_stages]) for i, n in
                                                 enumerate(["copy_in", "lengths_and_scan", "bytes", "copy_out"])}}
            with tempfile.TemporaryDirectory() as tmp:
                for gz in (False, True):
                    for nozero in (False, True):
                        stages, calls, writes, rates, gpu_calls = [], [], [], [], 0
                        for _ in range(args.repeats):
                            details = {}
                            t0 = time.perf_counter()
                            files = wt.export_tracks_batch(results, gz=gz, nozero=nozero, details=details)
                            t1 = time.perf_counter()
                            list(pool.map(write, [os.path.join(tmp, "s%03d.tracks" % i) for i in range(batch)], files))
                            t2 = time.perf_counter()
                            gpu_calls = len(details['times_ms'])
                            stages.append(np.sum(details['times_ms'], axis=0))      # a batch beyond the byte budget is several GPU calls
                            calls.append(t1 - t0)
                            writes.append(t2 - t1)
                            rates.append(batch / (t2 - t0))
                        key = ("gz" if gz else "plain") + ("_nozero" if nozero else "")
                        shape[key] = {"stage_milliseconds_per_batch": {n: summary([s[i] for s in stages]) for i, n in
                                                                       enumerate(["copy_in", "text", "bgzf", "copy_out"])},
                                      "gpu_calls_per_batch": gpu_calls, "call_seconds": summary(calls, 4),
                                      "file_write_seconds": summary(writes, 4), "files_per_second_end_to_end": summary(rates, 1),
                                      "track_bytes_first_sample": [len(files[0][0]), len(files[0][1])],
                                      "text_bytes_first_sample": list(details['text_bytes'][0])}
                        if gz and not nozero:
                            packed = files[0][0]
                        if not gz and not nozero:
                            plain = files[0][0]
            # exportjson -gz's deflate stage on the same files: the raw framing of the same encoder
            json_stages = []
            for _ in range(args.repeats):
                details = {}
                wt.export_json_batch(results, gz=True, details=details)
                json_stages.append(np.sum(details['times_ms'], axis=0))
            shape["exportjson_gz_stage_milliseconds_per_batch"] = {n: summary([s[i] for s in json_stages]) for i, n in
                                                                   enumerate(["copy_in", "text", "deflate", "copy_out"])}
            shape["exportjson_text_bytes_first_sample"] = list(details['text_bytes'][0])
            host = tr.bgzf_of(plain, block=65280, level=6)
            shape["bgzf_zlib_level6_bytes_first_sample"] = len(host)
            shape["device_bgzf_over_zlib_level6"] = round(len(packed) / len(host), 3)
            subset = results[:min(args.baseline_files, batch)]
            t0 = time.perf_counter()
            for res in subset:
                host_tracks(res, sizes)
            one_core = time.perf_counter() - t0
            shape["python_restatement_baseline"] = {"files": len(subset), "one_core_seconds": round(one_core, 4),
                                                    "one_core_files_per_second": round(len(subset) / one_core, 2)}
            shapes.append(shape)
            print(json.dumps({k: v for k, v in shape.items() if k != "rows_stage_milliseconds"})[:900], flush=True)
    result = {"shapes": shapes, "repeats": args.repeats, "io_threads": args.io, "library": _lib.load().wc_version().decode(),
              "note": "end to end = wisetools.export_tracks_batch from host arrays to the files' bytes (two tracks and the calls per "
                      "file) plus the write of the files; reading the result files is not in it.  rows_stage_milliseconds is "
                      "wc_bedgraph_rows on the batch's z rows alone.  bgzf (exporttracks, one call per GPU call for all rows) and "
                      "deflate (exportjson -gz, the raw framing, one call too) are the two stages the same session puts side by side; their "
                      "inputs differ: bedGraph text of merged runs against JSON text of every value.  The baseline ran in this "
                      "session on the first files of the same cohort.  Figures of different sessions do not compare"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
