#!/usr/bin/env python3
"""Time the three routes of `convert` on the synthetic 5-million-record BAM of tools/gpu_convert_time.py (its `make`
step writes the file), all in ONE session on one machine:

    timeout -k 10 900 python tools/gpu_convert_time.py make /tmp/wc_convert_time.bam --records 5000000 &&
    timeout -k 10 900 python tools/gpu_convert_bounded_time.py time /tmp/wc_convert_time.bam [--parent-root DIR]

  default   the whole convertBam call through the default reader (the whole-file device reader)
  stream    the same through `-stream` (BamReadsStream, then the filters on the whole arrays) at every chunk size
  bounded   the same through `-bounded` (wc_convert_bam_stream_dev: reader AND filters chunk by chunk)
  parent    the yardstick: `-stream` of another build of the package (--parent-root: a tree with its own built
            wisecondor_amd, e.g. `git archive` of the parent commit); without it the yardstick is this tree's own `-stream`

Every (route, chunk size) is a process of its own under its own time limit (`one`: a warm-up, then --repeats timed calls
ending in a device synchronise; the results of all routes are compared through a digest before anything is written), so a
route that fails ends the measurement.  Per route: every time, the median, the route's own run-to-run spread (max - min)
and the peak device bytes.  `time` writes profiles/convert_bounded_times.json; only figures inside that one file compare."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(result):
    chromosomes, quality = result
    h = hashlib.sha256()
    for key in sorted(chromosomes):
        h.update(key.encode())
        h.update(b"-" if chromosomes[key] is None else np.ascontiguousarray(chromosomes[key]).tobytes())
    h.update(json.dumps(sorted(quality.items())).encode())
    return h.hexdigest()


def one(args):
    """One route in this process: prints a JSON line."""
    sys.path.insert(0, args.root)
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    seen = {}

    def default_call():
        with wt.openBamReads(args.path) as bam:
            seen["peak_device_bytes"] = getattr(bam, "device_bytes", 0)
            seen["reader"] = type(bam).__name__
            return wt.convertBamReads(bam, args.binsize)

    def stream_call():
        with wt.BamReadsStream(args.path, chunk=args.chunk) as bam:
            seen["peak_device_bytes"] = bam.device_bytes
            seen["info"] = bam.stream_info
            return wt.convertBamReads(bam, args.binsize)

    def bounded_call():
        info = {}
        out = wt.convertBamBounded(args.path, args.binsize, chunk=args.chunk, info=info)
        seen["peak_device_bytes"] = info["peak_device_bytes"]
        seen["info"] = info
        return out

    call = {"default": default_call, "stream": stream_call, "bounded": bounded_call}[args.route]
    digest = _digest(call())                            # the warm-up
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        call()                                          # ends in a device synchronise
        times.append(time.perf_counter() - t0)
    print(json.dumps({"route": args.route, "chunk_bytes": args.chunk, "seconds": [round(t, 4) for t in times],
                      "median": round(float(np.median(times)), 4), "spread": round(max(times) - min(times), 4),
                      "peak_device_bytes": int(seen["peak_device_bytes"]), "info": seen.get("info"), "digest": digest,
                      "library": _lib.load().wc_version().decode(), "root": os.path.relpath(args.root, ROOT)}))


def timing(args):
    def child(route, chunk, root):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "one", args.path, "--route", route,
               "--chunk", str(chunk), "--repeats", str(args.repeats), "--binsize", str(args.binsize), "--root", root]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                        # a route that failed, faulted or ran out of time ends the session
            raise SystemExit("%s at chunk %d ended with status %d: nothing is written" % (route, chunk, done.returncode))
        return json.loads(done.stdout.strip().splitlines()[-1])

    legs = [child("default", 0, ROOT)]
    for chunk in args.chunks:
        leg = {"chunk_bytes": chunk}
        if args.parent_root:
            leg["parent_stream"] = child("stream", chunk, os.path.abspath(args.parent_root))
        leg["stream"] = child("stream", chunk, ROOT)
        leg["bounded"] = child("bounded", chunk, ROOT)
        yardstick = leg.get("parent_stream", leg["stream"])
        leg["yardstick"] = "parent_stream" if args.parent_root else "stream"
        leg["bounded_minus_yardstick_seconds"] = round(leg["bounded"]["median"] - yardstick["median"], 4)
        leg["bounded_within_the_yardsticks_spread_or_better"] = bool(
            leg["bounded"]["median"] - yardstick["median"] <= yardstick["spread"])
        legs.append(leg)
    digests = {legs[0]["digest"]} | {leg[k]["digest"] for leg in legs[1:] for k in ("parent_stream", "stream", "bounded") if k in leg}
    if len(digests) != 1:
        raise SystemExit("the routes disagree: nothing is written")
    result = {"file": {"compressed_bytes": os.path.getsize(args.path),
                       "records_placed": legs[1]["bounded"]["info"]["placed_records"]},
              "binsize": args.binsize, "repeats": args.repeats, "default_reader": legs[0], "chunk_sizes": legs[1:],
              "note": "one session, one machine; every route a process of its own: warm-up, then the timed calls"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("path")
    t.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_bounded_times.json"))
    t.add_argument("--repeats", type=int, default=7)
    t.add_argument("--binsize", type=int, default=1000000)
    t.add_argument("--chunks", type=int, nargs="+", default=[8 << 20, 32 << 20, 256 << 20])
    t.add_argument("--parent-root", default=None)
    t.add_argument("--limit", type=int, default=120, help="seconds every route's process may take")
    t.set_defaults(func=timing)
    o = sub.add_parser("one")
    o.add_argument("path")
    o.add_argument("--route", choices=["default", "stream", "bounded"], required=True)
    o.add_argument("--chunk", type=int, default=0)
    o.add_argument("--repeats", type=int, default=7)
    o.add_argument("--binsize", type=int, default=1000000)
    o.add_argument("--root", default=ROOT)
    o.set_defaults(func=one)
    args = ap.parse_args()
    args.func(args)


if __name__ == "__main__":
    main()
