#!/usr/bin/env python3
"""Time the robust stage of `crossval` (wc_column_robust_dev, csrc/robust.hip) on synthetic data of the bench's kind
(22 human autosomes, synth.make_sample) and write profiles/crossval_robust_times.json.

    python tools/gpu_robust_time.py --out profiles/crossval_robust_times.json

Shapes: those of profiles/crossval_times.json, leave-one-out on 100 samples x 250 kb and 10 folds on 200 samples x 50 kb,
both at refsize 100.  The command itself never touches the GPU: it starts one child per shape (`--step NAME`), one after
the other, each under its own `timeout`, and starts nothing more after a child that failed.  A child measures, in ONE
process, `--repeats` (3) runs after a warm-up of each:
  plain / robust   crossval.crossval_batch end to end without and with robust=True, alternating, wall time
  stages           robust=True with device events around the stages: 'stats' and 'robust' of every run
  kernel           wc_column_robust_dev alone on the run's held-out Z, resident on the device, between device events
  host             np.median over the samples and np.median of the absolute deviations from it, on the same matrix, on one
                   core (numpy's median does not thread): what the stage would cost on the host, the copy of Z not counted
and says whether the two acceptance lines of the stage hold:
  call_within      median(robust) - median(plain) <= max(spread of the robust runs, the robust stage's time)
  stage_below_host the robust stage's median lies below the host route's median by more than the host route's spread
No figure is asserted; a line that does not hold is reported as false.  WC_LIB_PATH selects another build of the library
(tools/build_variant.py): that is how digit widths were compared."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"loo_100x250kb": dict(binsize=250000, samples=100, folds=100, refsize=100),
          "folds10_200x50kb": dict(binsize=50000, samples=200, folds=10, refsize=100)}


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": list(values)}


def step(name, repeats):
    import torch
    from wisecondor_amd import _lib, crossval, synth
    from wisecondor_amd import wisetools as wt
    if not torch.cuda.is_available():
        raise SystemExit("gpu_robust_time: no GPU visible; nothing is measured without one")
    shape = dict(SHAPES[name])
    binsize, n, folds, refsize = shape["binsize"], shape["samples"], shape["folds"], shape["refsize"]
    profile = synth.bin_profile(binsize)
    samples = [synth.make_sample(profile, seed=7000 + i) for i in range(n)]
    sizes = synth.chrom_bins(binsize)
    counts = wt.samples_to_counts(samples, sizes)
    fold_of = crossval.foldPlan(n, folds, seed=1)
    shape.update(name=name, bins_per_row=int(sum(sizes)), library=os.environ.get("WC_LIB_PATH") or "the built library")

    def run(robust, stage_ms=None, keep=False):
        torch.cuda.synchronize()
        began = time.perf_counter()
        extra = dict(robust=True) if robust else {}
        out = crossval.crossval_batch(counts, sizes, fold_of, binsize, refsize=refsize, stage_ms=stage_ms, keep_results=keep, **extra)
        return time.perf_counter() - began, out

    run(False)
    _, warm = run(True, keep=True)
    plain_s, robust_s = [], []
    for _ in range(repeats):
        plain_s.append(run(False)[0])
        took, out = run(True)
        robust_s.append(took)
        assert np.array_equal(out["robust_i"], warm["robust_i"])
        assert np.array_equal(out["robust_f"], warm["robust_f"], equal_nan=True)
    stage_runs = []
    for _ in range(repeats):
        stage_ms = {}
        run(True, stage_ms=stage_ms)
        stage_runs.append(stage_ms)
    # the kernel alone, on the rows of the run
    Z = warm["Z"]
    lib, ctx = _lib.load(), _lib.context(0)
    dev = torch.device("cuda", 0)
    kernel_ms = []
    with torch.cuda.device(dev):
        z = torch.from_numpy(Z).to(dev)
        col_i = torch.zeros((Z.shape[1], 2), dtype=torch.int32, device=dev)
        col_f = torch.zeros((Z.shape[1], 2), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(repeats + 1):
            before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before.record()
            _lib.check(lib.wc_column_robust_dev(ctx, stream, z.data_ptr(), Z.shape[1], Z.shape[0], Z.shape[1], col_i.data_ptr(), col_f.data_ptr()))
            after.record()
            torch.cuda.synchronize()
            if at:                                      # (the first is the warm-up)
                kernel_ms.append(before.elapsed_time(after))
        assert np.array_equal(col_i.cpu().numpy(), warm["robust_i"])
    host_ms = []
    for at in range(repeats + 1):
        began = time.perf_counter()
        centre = np.median(Z, axis=0)
        np.median(np.abs(Z - centre), axis=0)
        if at:
            host_ms.append(1e3 * (time.perf_counter() - began))
    p, r, h, k = spread(plain_s), spread(robust_s), spread(host_ms), spread(kernel_ms)
    stage = spread([s["robust"] for s in stage_runs])
    stats = spread([s["stats"] for s in stage_runs])
    over = r["median"] - p["median"]
    allowed = max(r["max"] - r["min"], stage["median"] / 1e3)
    shape.update(plain_wall_s=p, robust_wall_s=r, robust_stage_ms=stage, stats_stage_ms=stats, robust_kernel_ms=k, host_median_twice_ms=h,
                 call_over_plain_s=over, call_allowed_s=allowed, call_within=bool(over <= allowed),
                 stage_below_host=bool(stage["median"] < h["median"] - (h["max"] - h["min"])),
                 bins_listed_at_spread_2=int(np.count_nonzero(1.4826 * warm["robust_f"][:, 1] > 2.0)))
    print("gpu_robust_time: %s: robust stage %.3f ms (kernel %.3f ms) beside stats %.3f ms; call %.3f s against %.3f s; np.median twice %.1f ms"
          % (name, stage["median"], k["median"], stats["median"], r["median"], p["median"], h["median"]), flush=True)
    return shape


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossval_robust_times.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--step", default=None, help="(a child) measure this shape and print it as JSON")
    args = ap.parse_args()
    if args.step is not None:
        print("SHAPE " + json.dumps(step(args.step, args.repeats)))
        return
    shapes = []
    for name in args.shapes:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--repeats",
               str(args.repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("SHAPE ")]
        for ln in done.stdout.splitlines():
            if not ln.startswith("SHAPE ") and not ln.startswith("Working on part"):
                print(ln, flush=True)
        if done.returncode != 0 or not lines:
            raise SystemExit("gpu_robust_time: the %s step ended with status %d; nothing more is started" % (name, done.returncode))
        shapes.append(json.loads(lines[-1][len("SHAPE "):]))
    with open(args.out, "w") as f:
        json.dump({"what": "crossval: the robust stage (wc_column_robust_dev) beside the stats stage, the whole call with and without it, "
                           "and np.median twice over the same matrix on one host core",
                   "repeats": args.repeats, "not_measured": "real samples; file I/O; the copy of Z to the host that the host route would need",
                   "shapes": shapes}, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
