#!/usr/bin/env python3
"""Time `sensitivity` on synthetic data of the bench's kind (22 human autosomes at 250 kb and at 50 kb bins, a reference of
40 samples with refsize 100, 8 healthy samples) at 256 and 4 096 trials, and write profiles/sensitivity_times.json.

    python tools/gpu_sensitivity_time.py --out profiles/sensitivity_times.json

The command itself never touches the GPU: it starts one child per bin size (`--step BINSIZE`), one after the other, each
under its own `timeout`, and starts nothing more after a child that failed.  A child measures, in ONE process so that
the figures of a shape share a session, per trial count:
  device   wt.sensitivity_batch end to end (base image up, records back), `--repeats` (3) runs after a warm-up: trials
           per second; and its three stages called one by one through the C ABI with a device synchronise between them
           (wc_spike_counts_dev, wc_test_batch_dev with every output, wc_spike_score_dev), batches of 1 024 trials
  k_spike  the spike of all trials in one call between device events, beside a device-to-device hipMemcpyAsync of the
           bytes the spike WRITES (trials x bins x 4): both as written bytes per second, median of `--copies` (10)
  host     the same plan through numpy spiking (tests/spike_restated.py) -> wt.test_batch on sample dicts -> the Python
           restatement of the score, `--repeats` runs: trials per second
No figure is asserted anywhere.  The host route is the restatement, never the code under test."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRIALS = (256, 4096)
LENGTHS_BP, EFFECTS_PPM = (1e6, 5e6, 20e6), (25000, 50000, 100000, -25000, -50000, -100000)
N_HEALTHY, BATCH = 8, 1024


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": list(values)}


def step(binsize, repeats, copies):
    import torch
    import spike_restated as sr
    from wisecondor_amd import _lib, sensitivity, synth
    from wisecondor_amd import wisecondor as cli
    from wisecondor_amd import wisetools as wt
    from wisecondor_amd.distributed import TestBatch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_sensitivity_time: no GPU visible; nothing is measured without one")
    lib = _lib.load()
    profile = synth.bin_profile(binsize)
    refs = [synth.make_sample(profile, seed=i) for i in range(40)]
    _, chrom_bins, mask, corrected, comps, mean, masked_bins = wt.prepReference(refs)
    masked_bins = np.asarray(masked_bins, dtype=np.int64)
    idx, dst = wt.getReference(corrected, masked_bins, np.cumsum(masked_bins), 100, 1, 1)
    reference = wt.Reference(idx, dst, np.asarray(chrom_bins, dtype=np.int64), masked_bins, mask, mean, comps, binsize=binsize)
    cut = cli.zThreshold([int(v) for v in masked_bins], 1000, None)
    healthy = [synth.make_sample(profile, seed=3000 + i) for i in range(N_HEALTHY)]
    sizes = reference.chromosome_sizes
    n_total = reference.n_total
    lengths_bins = [int(np.ceil(length / binsize)) for length in LENGTHS_BP]
    sel = np.arange(1, 23, dtype=np.int32)
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    shapes = []
    for n_trials in TRIALS:
        per = -(-n_trials // (N_HEALTHY * len(lengths_bins) * len(EFFECTS_PPM)))
        plan = sensitivity.makePlan(reference, N_HEALTHY, lengths_bins, list(EFFECTS_PPM), per, seed=1)[:n_trials]
        assert len(plan) == n_trials
        shape = {"binsize": binsize, "trials": n_trials, "bins_per_row": n_total, "lengths_bins": lengths_bins,
                 "effects_ppm": list(EFFECTS_PPM), "healthy_samples": N_HEALTHY, "threshold_z": float(cut), "batch": BATCH}
        # ---- device route, end to end
        rec_i, rec_f = sensitivity.sensitivity_batch(reference, healthy, plan, cut, batch=BATCH)          # warm-up
        walls = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            began = time.perf_counter()
            got_i, got_f = sensitivity.sensitivity_batch(reference, healthy, plan, cut, batch=BATCH)
            walls.append(time.perf_counter() - began)
            assert np.array_equal(got_i, rec_i)
        shape["device_wall_s"] = spread(walls)
        shape["device_trials_per_s"] = n_trials / spread(walls)["median"]
        table = sensitivity.sensitivityTable(plan, rec_i, rec_f, lengths_bins, list(EFFECTS_PPM))
        shape["table"] = [[None if v != v else v for v in row] for row in table.tolist()]
        # ---- the three stages one by one
        base = torch.from_numpy(wt.samples_to_counts(healthy, [int(v) for v in sizes])).cuda()
        stage = {"spike_s": [], "test_s": [], "score_s": []}
        for _ in range(repeats + 1):
            took = [0.0, 0.0, 0.0]
            for lo in range(0, n_trials, BATCH):
                part = np.ascontiguousarray(plan[lo:lo + BATCH])
                m = len(part)
                counts = torch.empty((m, n_total), dtype=torch.int32, device="cuda")
                tb = TestBatch(reference, counts, cut, chromosomes=sel, max_calls=wt.MAX_CALLS)
                ri = torch.empty((m, 8), dtype=torch.int32, device="cuda")
                rf = torch.empty((m, 2), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _lib.check(lib.wc_spike_counts_dev(reference.ctx, None, base.data_ptr(), N_HEALTHY, _lib.ptr(sizes), len(sizes),
                                                   _lib.ptr(part), m, counts.data_ptr(), None))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                tb.run()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                _lib.check(lib.wc_spike_score_dev(reference.ctx, None, _lib.ptr(part), m, tb.calls.data_ptr(), tb.n_calls.data_ptr(),
                                                  wt.MAX_CALLS, ri.data_ptr(), rf.data_ptr()))
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                took = [took[0] + t1 - t0, took[1] + t2 - t1, took[2] + t3 - t2]
                assert np.array_equal(ri.cpu().numpy(), rec_i[lo:lo + m])
            for key, value in zip(("spike_s", "test_s", "score_s"), took):
                stage[key].append(value)
        shape["stages"] = {key: spread(values[1:]) for key, values in stage.items()}          # (the first pass warms up)
        # ---- k_spike beside a device-to-device copy of the bytes it writes
        written = n_trials * n_total * 4
        out = torch.empty((n_trials, n_total), dtype=torch.int32, device="cuda")
        src = torch.randint(0, 100, (n_trials, n_total), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        spike_ms, copy_ms = [], []
        for i in range(copies + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            _lib.check(lib.wc_spike_counts_dev(reference.ctx, stream, base.data_ptr(), N_HEALTHY, _lib.ptr(sizes), len(sizes),
                                               _lib.ptr(plan), n_trials, out.data_ptr(), None))
            ev[1].record()
            ev[2].record()
            assert hip.hipMemcpyAsync(out.data_ptr(), src.data_ptr(), written, 3, stream) == 0       # 3: device to device
            ev[3].record()
            torch.cuda.synchronize()
            if i:
                spike_ms.append(ev[0].elapsed_time(ev[1]))
                copy_ms.append(ev[2].elapsed_time(ev[3]))
        shape["k_spike"] = {"written_bytes": written, "ms": spread(spike_ms), "copy_ms": spread(copy_ms),
                            "written_gb_per_s": written / spread(spike_ms)["median"] / 1e6,
                            "copy_written_gb_per_s": written / spread(copy_ms)["median"] / 1e6,
                            "note": "the spike's interval holds the plan's check and upload on the host as well as the kernel"}
        del out, src
        # ---- host route: numpy spiking -> wt.test_batch -> the Python restatement of the score
        dense = base.cpu().numpy()
        offs = np.concatenate([[0], np.cumsum(sizes)])
        host_walls, host_parts = [], []
        for _ in range(repeats):
            began = time.perf_counter()
            spiked, _ = sr.spike(dense, sizes, plan)
            dicts = [{str(c + 1): row[offs[c]:offs[c + 1]] for c in range(len(sizes))} for row in spiked]
            t1 = time.perf_counter()
            outs = wt.test_batch(reference, dicts, cut)
            t2 = time.perf_counter()
            host_i, _ = sr.score_lists(plan, [o["results_calls"] for o in outs])
            t3 = time.perf_counter()
            host_walls.append(t3 - began)
            host_parts.append([t1 - began, t2 - t1, t3 - t2])
            assert np.array_equal(host_i, rec_i)
            del outs, dicts, spiked
        shape["host_wall_s"] = spread(host_walls)
        shape["host_parts_s_spike_test_score"] = host_parts
        shape["host_trials_per_s"] = n_trials / spread(host_walls)["median"]
        shapes.append(shape)
        print("gpu_sensitivity_time: %d kb, %d trials: device %.0f trials/s, host %.0f trials/s" %
              (binsize // 1000, n_trials, shape["device_trials_per_s"], shape["host_trials_per_s"]), flush=True)
    reference.close()
    return shapes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_times.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--copies", type=int, default=10)
    ap.add_argument("--binsizes", type=int, nargs="+", default=[250000, 50000])
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--step", type=int, default=None, help="(a child) measure this bin size and print its shapes as JSON")
    args = ap.parse_args()
    if args.step is not None:
        print("SHAPES " + json.dumps(step(args.step, args.repeats, args.copies)))
        return
    shapes = []
    for binsize in args.binsizes:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(binsize),
               "--repeats", str(args.repeats), "--copies", str(args.copies)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("SHAPES ")]
        for ln in done.stdout.splitlines():
            if not ln.startswith("SHAPES "):
                print(ln, flush=True)
        if done.returncode != 0 or not lines:
            raise SystemExit("gpu_sensitivity_time: the %d bp step ended with status %d; nothing more is started"
                             % (binsize, done.returncode))
        shapes.extend(json.loads(lines[-1][len("SHAPES "):]))
    with open(args.out, "w") as f:
        json.dump({"what": "sensitivity: device route, its stages, k_spike beside hipMemcpyAsync, the host route",
                   "repeats": args.repeats, "copies": args.copies, "shapes": shapes}, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
