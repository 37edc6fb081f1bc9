#!/usr/bin/env python3
"""What the GPU result encoder (testbatch -encoder gpu, csrc/deflate.hip) takes and what it buys.  Run on the GPU box.

1. Device time of wc_deflate_rows_dev (device events around the call: its two kernels) for 512 result-like rows of
   92 000 and of 460 000 bytes (the 250 kb and 50 kb bin sizes' rows), the GB/s of input, and the compressed size
   against zlib's Z_RLE level 1 on the same rows.
2. `testbatch` files/s end to end, N files at 250 kb in batches of 512 with 16 I/O threads, -encoder host and
   -encoder gpu alternating in the same process (one warm-up run of each first), every run listed.
Writes the figures as JSON (default profiles/deflate_times.json) and prints them."""
import argparse
import contextlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wisecondor_amd import synth  # noqa: E402
from wisecondor_amd import wisecondor as cli  # noqa: E402
from wisecondor_amd import wisetools as wt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, default=8192)
ap.add_argument("--binsize", type=int, default=250000)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--io", type=int, default=16)
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--repeats", type=int, default=20, help="timed calls of the primitive per shape")
ap.add_argument("--runs", type=int, default=3, help="timed testbatch runs per encoder")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_times.json"))
a = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("gpu_encode_rate: no GPU visible (nothing is measured without one)")


def result_rows(n_rows, n_bins, seed):
    """Rows like results_z and results_r: float64 noise (z in the even rows, ratio - 1 in the odd ones), 3 % of the bins
    zeroed singly and 12 runs of 5 .. 200 zeros per row."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n_rows, n_bins))
    mask = (rng.uniform(size=(n_rows, n_bins)) >= 0.03).astype(np.float64)
    for i in range(n_rows):
        for _ in range(12):
            at = int(rng.randint(0, n_bins - 200))
            mask[i, at:at + int(rng.randint(5, 201))] = 0.0
    out = z * mask
    out[1::2] = (1.0 + 0.03 * z[1::2]) * mask[1::2] - mask[1::2]
    return out


def zlib_rle(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    return len(co.compress(data) + co.flush())


out = {"block_bytes": int(wt._lib.load().wc_deflate_block_bytes()), "primitive": {}, "testbatch": {}}
for n_bins in (11500, 57500):
    host = result_rows(a.rows, n_bins, 77)
    rows = torch.from_numpy(host).cuda().view(torch.uint8)
    for _ in range(3):                                      # code objects, the context's scratch buffers
        streams, lengths, crcs = wt.deflateRows(rows)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        streams, lengths, crcs = wt.deflateRows(rows)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    lengths = lengths.cpu().numpy()
    sample = range(0, a.rows, max(1, a.rows // 32))
    want = [zlib_rle(host[i].tobytes()) for i in sample]
    t0 = time.time()
    for i in sample:
        zlib_rle(host[i].tobytes())
    zlib_s = (time.time() - t0) / len(sample)
    got = streams.cpu().numpy()
    for i in list(sample)[:4]:
        assert zlib.decompress(got[i, :lengths[i]].tobytes(), -15) == host[i].tobytes()
    in_bytes = a.rows * n_bins * 8
    med = statistics.median(times)
    out["primitive"]["%d_rows_of_%d_bytes" % (a.rows, 8 * n_bins)] = {
        "device_s_median": med, "device_s_min": min(times), "device_s_max": max(times), "calls": a.repeats,
        "input_GB_per_s_median": in_bytes / med / 1e9,
        "size_over_zlib_rle_level1": float(np.sum(lengths[list(sample)])) / float(np.sum(want)),
        "size_over_raw": float(np.sum(lengths)) / in_bytes,
        "zlib_rle_level1_s_per_row_one_host_thread": zlib_s}
    del rows, streams

tmp = tempfile.mkdtemp(prefix="wc_encode_")
profile = synth.bin_profile(a.binsize)
refs = [synth.make_sample(profile, seed=i) for i in range(40)]
_, chrom_bins, mask, corrected, comps, mean, masked_bins = wt.prepReference(refs)
masked_bins = np.asarray(masked_bins, dtype=np.int64)
idx, dst = wt.getReference(corrected, masked_bins, np.cumsum(masked_bins), 100, 1, 1)
refpath = os.path.join(tmp, "reference.npz")
np.savez_compressed(refpath, arguments={}, runtime={}, binsize=float(a.binsize), indexes=idx, distances=dst,
                    chromosome_sizes=np.asarray(chrom_bins), mask=mask, masked_sizes=masked_bins,
                    pca_components=comps, pca_mean=mean)
paths = []
for i in range(a.files):
    p = os.path.join(tmp, "s_%05d.npz" % i)
    if i < 64:
        np.savez_compressed(p, arguments={"binsize": float(a.binsize)}, runtime={}, sample=synth.make_sample(profile, seed=3000 + i),
                            quality={})
    else:
        shutil.copyfile(paths[i % 64], p)       # (neither the decode nor the encode cost depends on the counts)
    paths.append(p)
runs = {"host": [], "gpu": []}
order = ["host", "gpu"] + ["host", "gpu"] * a.runs             # the first of each: warm-up, listed but not summarised
for k, encoder in enumerate(order):
    outdir = os.path.join(tmp, "out_%d" % k)
    argv = ["testbatch"] + paths + [outdir, refpath, "-batch", str(a.batch), "-io", str(a.io), "-encoder", encoder]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(argv)
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("rank 0")][-1]
    rate = float(line.split("(")[1].split(" files/s")[0])
    size = sum(os.path.getsize(os.path.join(outdir, f)) for f in os.listdir(outdir)) / max(1, len(os.listdir(outdir)))
    runs[encoder].append({"files_per_s": rate, "report": line, "bytes_per_result_file": size, "warm_up": k < 2})
    shutil.rmtree(outdir, ignore_errors=True)
for encoder, got in runs.items():
    timed = [r["files_per_s"] for r in got if not r["warm_up"]]
    out["testbatch"][encoder] = {"runs": got, "files_per_s_median": statistics.median(timed), "files_per_s_min": min(timed),
                                 "files_per_s_max": max(timed)}
out["testbatch"].update(files=a.files, binsize=a.binsize, batch=a.batch, io_threads=a.io)
shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
