#!/usr/bin/env python3
"""Time `convert` on a synthetic BAM of a size a user would run: the host reader (BamReads, 16 threads: what convertBam
used before the device reader) against the device reader (BamReadsDevice), and the device reader's stages.

Two steps, each a process of its own, chained with && and each under its own time limit:

    timeout -k 10 600 python tools/gpu_convert_time.py make /tmp/wc_convert_time.bam --records 5000000 &&
    timeout -k 10 600 python tools/gpu_convert_time.py time /tmp/wc_convert_time.bam --out profiles/convert_times.json &&
    timeout -k 10 600 python tools/gpu_convert_time.py stream /tmp/wc_convert_time.bam --out profiles/convert_stream_times.json

`make` needs no GPU: a seeded BAM, coordinate-sorted over chr1..chr22, X, Y, records of 100 and 151 bases with names,
CIGAR, 4-bit sequence, qualities and tags (about 230 and 310 bytes), compressed at zlib level 6 in BGZF blocks of 65 280
bytes by a pool of processes.  `time` writes the JSON:
  leg 1  wall time of the whole call (reader + filters + binning, ending in a device synchronise) of both readers,
         alternating, after one warm-up of each: every time, median, spread (max - min)
  leg 2  the device reader's stages: the host stage by the host clock, the device stages between device events
         (wc_bam_dev_times), the convert kernels by the host clock around the synchronous call; inflated bytes per second
         of the inflate kernel; the sum of the walk's stages (checks, fields, order) per run, its median and spread
The two readers' results are compared (dict and quality) before anything is written.
`stream` writes its own JSON: per chunk size (8, 32 and 256 MiB unless --chunks names others) the wall time of the whole
call through the whole-file device reader and through the streamed reader (BamReadsStream), alternating, five times each
after one warm-up of each, results compared first; the streamed reader's stream_info (chunks, peak device working bytes,
host staging bytes) beside the whole-file reader's device_bytes; and whether the streamed reader beats the whole-file
reader by more than that reader's own spread."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHROMS = [("chr%d" % c, int(2.4e8 - 8e6 * c)) for c in range(1, 23)] + [("chrX", 155000000), ("chrY", 57000000)]
BLOCK = 65280


def _records(ref, pos, l_seq, rng, serial):
    """len(pos) records of reference `ref` with l_seq bases as one byte string (a fixed layout, filled by columns)."""
    n = len(pos)
    half = (l_seq + 1) // 2
    tags = b"NMC\x01MDZ%dA\x00ASC\x60" % (l_seq - 1)
    dt = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                   ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("mref", "<i4"), ("mpos", "<i4"), ("tlen", "<i4"),
                   ("name", "S24"), ("cigar", "<u4"), ("seq", "u1", (half,)), ("qual", "u1", (l_seq,)),
                   ("tags", "S%d" % len(tags))])
    a = np.zeros(n, dtype=dt)
    a["bs"] = dt.itemsize - 4
    a["ref"], a["pos"], a["l_name"], a["n_cigar"], a["l_seq"] = ref, pos, 24, 1, l_seq
    a["mapq"] = rng.choice([0, 1, 20, 37, 60, 60, 60, 60], n)
    a["flag"] = rng.choice([0, 16, 0, 16, 1024, 256, 4], n)
    a["bin"] = 4680
    a["mref"], a["mpos"] = -1, -1
    a["name"] = np.char.add(b"SIM:1:FC:%d:" % (ref + 1), (serial + np.arange(n)).astype("S9"))
    a["cigar"] = (l_seq << 4) | 0
    a["seq"] = rng.randint(0, 256, (n, half), dtype=np.uint8)
    q = rng.choice(np.array([2, 11, 25, 37, 37, 37, 37, 37], dtype=np.uint8), (n, l_seq))
    a["qual"] = q
    a["tags"] = tags
    return a.tobytes()


def _bgzf_block(piece):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cd = c.compress(piece) + c.flush()
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cd) + 25) + cd
            + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))


def make(args):
    import concurrent.futures
    rng = np.random.RandomState(args.seed)
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    head = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(CHROMS))]
    for name, length in CHROMS:
        head += [struct.pack("<i", len(name) + 1), name.encode() + b"\0", struct.pack("<i", length)]
    total_len = float(sum(l for _, l in CHROMS))
    inflated = compressed = records = 0
    began = time.time()
    with open(args.path, "wb") as out, concurrent.futures.ProcessPoolExecutor(max_workers=args.workers) as pool:
        carry = b"".join(head)
        for ref, (_, length) in enumerate(CHROMS):
            n = int(round(args.records * length / total_len))
            pos = np.sort(rng.randint(0, length - 200, n)).astype(np.int32)
            parts = [carry]
            for lo in range(0, n, 4000):                # runs of one read length, as lanes of a flow cell would give
                parts.append(_records(ref, pos[lo:lo + 4000], 151 if (lo // 4000) % 3 else 100, rng, records + lo))
            records += n
            data = b"".join(parts)
            whole = len(data) - len(data) % BLOCK if ref + 1 < len(CHROMS) else len(data)
            pieces = [data[i:i + BLOCK] for i in range(0, whole, BLOCK)]
            carry = data[whole:]
            for blob in pool.map(_bgzf_block, pieces, chunksize=16):
                out.write(blob)
                compressed += len(blob)
            inflated += whole
        eof = _bgzf_block(b"")
        out.write(eof)
        compressed += len(eof)
    print(json.dumps({"path": args.path, "records": records, "inflated_bytes": inflated, "compressed_bytes": compressed,
                      "ratio": round(inflated / compressed, 3), "seconds": round(time.time() - began, 1)}))


def _same(a, b):
    (da, qa), (db, qb) = a, b
    return qa == qb and set(da) == set(db) and all(
        (da[k] is None and db[k] is None) or np.array_equal(da[k], db[k]) for k in da)


def timing(args):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt

    def host_call():
        with wt.BamReads(args.path, threads=args.threads) as bam:
            return wt.convertBamReads(bam, args.binsize)

    def device_call():
        with wt.BamReadsDevice(args.path) as bam:
            return wt.convertBamReads(bam, args.binsize)

    want, got = host_call(), device_call()                      # the warm-up of both, and the comparison
    if not _same(want, got):
        raise SystemExit("the two readers disagree: nothing is written")
    times = {"host_reader": [], "device_reader": []}
    for _ in range(args.repeats):
        for name, call in (("host_reader", host_call), ("device_reader", device_call)):
            t0 = time.perf_counter()
            call()                                              # ends in a device synchronise (wc_convert_*)
            times[name].append(time.perf_counter() - t0)
    leg1 = {name: {"seconds": [round(t, 4) for t in ts], "median": round(float(np.median(ts)), 4),
                   "spread": round(max(ts) - min(ts), 4)} for name, ts in times.items()}
    stages = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        bamfile = wt.BamFile(args.path)
        t1 = time.perf_counter()
        with bamfile, wt.BamReadsDevice(bamfile) as bam:
            t2 = time.perf_counter()
            wt.convertBamReads(bam, args.binsize)
            t3 = time.perf_counter()
            row = {"host_stage": (t1 - t0) * 1e3, "host_stage_pinning": bamfile.pin_ms, "device_open_call": (t2 - t1) * 1e3, "convert_kernels_call": (t3 - t2) * 1e3}
            row.update(bam.stage_ms)
            row["inflated_bytes"], row["compressed_bytes"] = bamfile.inflated_bytes, bamfile.compressed_bytes
            row["blocks"], row["placed_records"], row["pinned"] = bamfile.n_blocks, bam.n_reads, bamfile.pinned
            stages.append(row)
    keys = ["host_stage", "host_stage_pinning", "h2d", "inflate", "record_starts", "link", "checks", "fields", "order", "device_open_call",
            "convert_kernels_call"]
    med = {k: round(float(np.median([r[k] for r in stages])), 3) for k in keys}
    walk = [r["checks"] + r["fields"] + r["order"] for r in stages]         # both walk passes and what follows them
    last = stages[-1]
    result = {
        "file": {"records_placed": last["placed_records"], "bgzf_blocks": last["blocks"], "inflated_bytes": last["inflated_bytes"],
                 "compressed_bytes": last["compressed_bytes"],
                 "compression_ratio": round(last["inflated_bytes"] / last["compressed_bytes"], 3), "pinned_host_buffer": last["pinned"]},
        "binsize": args.binsize, "host_reader_threads": args.threads, "repeats": args.repeats,
        "leg1_whole_call_seconds": leg1,
        "device_reader_beats_host_reader_by_more_than_its_spread":
            bool(leg1["host_reader"]["median"] - leg1["device_reader"]["median"] > leg1["host_reader"]["spread"]),
        "leg2_stage_milliseconds_median": med,
        "leg2_walk_stages_sum_milliseconds": {"runs": [round(w, 3) for w in walk], "median": round(float(np.median(walk)), 3),
                                              "spread": round(max(walk) - min(walk), 3)},
        "leg2_inflate_gigabytes_per_second": round(last["inflated_bytes"] / (med["inflate"] * 1e-3) / 1e9, 3),
        "leg2_h2d_gigabytes_per_second": round(last["compressed_bytes"] / (med["h2d"] * 1e-3) / 1e9, 3),
        "library": _lib.load().wc_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def stream_timing(args):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt

    seen = {}

    def device_call():
        with wt.BamReadsDevice(args.path) as bam:
            seen["device_bytes"], seen["placed"] = bam.device_bytes, bam.n_reads
            return wt.convertBamReads(bam, args.binsize)

    def stream_call(chunk):
        with wt.BamReadsStream(args.path, chunk=chunk) as bam:
            seen["stream_info"], seen["stream_ms"], seen["stream_bytes"] = bam.stream_info, bam.stage_ms, bam.device_bytes
            return wt.convertBamReads(bam, args.binsize)

    def summary(ts):
        return {"seconds": [round(t, 4) for t in ts], "median": round(float(np.median(ts)), 4), "spread": round(max(ts) - min(ts), 4)}

    want = device_call()                                        # the warm-up of the whole-file reader
    legs = []
    for chunk in args.chunks:
        if not _same(want, stream_call(chunk)):                 # the warm-up at this size, and the comparison
            raise SystemExit("the two readers disagree at chunk %d: nothing is written" % chunk)
        times = {"device_reader": [], "stream_reader": []}
        for _ in range(args.repeats):
            for name, call in (("device_reader", device_call), ("stream_reader", lambda: stream_call(chunk))):
                t0 = time.perf_counter()
                call()                                          # ends in a device synchronise (wc_convert_*)
                times[name].append(time.perf_counter() - t0)
        leg = {"chunk_bytes": chunk, "device_reader": summary(times["device_reader"]),
               "stream_reader": summary(times["stream_reader"]), "stream_info": seen["stream_info"],
               "stream_reader_wait_ms": {k: round(v, 3) for k, v in seen["stream_ms"].items()},
               "stream_reader_peak_device_bytes_with_arrays": seen["stream_bytes"],
               "device_reader_device_bytes": seen["device_bytes"]}
        leg["stream_reader_beats_device_reader_by_more_than_its_spread"] = bool(
            leg["device_reader"]["median"] - leg["stream_reader"]["median"] > leg["device_reader"]["spread"])
        leg["device_reader_beats_stream_reader_by_more_than_its_spread"] = bool(
            leg["stream_reader"]["median"] - leg["device_reader"]["median"] > leg["stream_reader"]["spread"])
        legs.append(leg)
    best = min(legs, key=lambda leg: leg["stream_reader"]["median"])
    result = {"file": {"records_placed": seen["placed"], "compressed_bytes": os.path.getsize(args.path)},
              "binsize": args.binsize, "repeats": args.repeats, "chunk_sizes": legs,
              "fastest_chunk_bytes": best["chunk_bytes"],
              "library_default_chunk_bytes": int(_lib.load().wc_bam_stream_default_chunk()),
              "library": _lib.load().wc_version().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("make")
    m.add_argument("path")
    m.add_argument("--records", type=int, default=5000000)
    m.add_argument("--seed", type=int, default=1)
    m.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    m.set_defaults(func=make)
    t = sub.add_parser("time")
    t.add_argument("path")
    t.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_times.json"))
    t.add_argument("--repeats", type=int, default=5)
    t.add_argument("--threads", type=int, default=16)
    t.add_argument("--binsize", type=int, default=1000000)
    t.set_defaults(func=timing)
    st = sub.add_parser("stream")
    st.add_argument("path")
    st.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_stream_times.json"))
    st.add_argument("--repeats", type=int, default=5)
    st.add_argument("--binsize", type=int, default=1000000)
    st.add_argument("--chunks", type=int, nargs="+", default=[8 << 20, 32 << 20, 256 << 20])
    st.set_defaults(func=stream_timing)
    args = ap.parse_args()
    args.func(args)


if __name__ == "__main__":
    main()
