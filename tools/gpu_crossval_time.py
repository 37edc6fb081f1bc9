#!/usr/bin/env python3
"""Time `crossval` on synthetic data of the bench's kind (22 human autosomes, synth.make_sample) and write
profiles/crossval_times.json.

    python tools/gpu_crossval_time.py --out profiles/crossval_times.json

Shapes: leave-one-out on 100 samples x 250 kb at refsize 100, and 10 folds on 200 samples x 50 kb at refsize 100.
The command itself never touches the GPU: it starts one child per shape (`--step NAME`), one after the other, each
under its own `timeout`, and starts nothing more after a child that failed.  A child measures, in ONE process and
alternating so that the two routes share a session, `--repeats` (3) runs after a warm-up of each:
  device   crossval.crossval_batch end to end (counts up, statistics back), wall time
  host     the same folds one at a time through the public host-array route: wt.prepReference (host form) ->
           wt.getReference -> wt.Reference -> wt.test_batch on the fold's sample dicts, wall time; its calls per sample
           must equal the device route's
and then one more device run with device events between the stages of every fold (training gather, prep, newref,
reference creation -- which holds the round trip of indexes / distances through the host that wc_reference_create needs
-- test, and the statistics kernels): per-stage sums and the share of reference creation.  `within_spread` says
whether the device route's median is not above the host route's by more than the host route's own run-to-run spread
(max - min); no figure is asserted.  Real samples and file I/O are not measured."""
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
    from wisecondor_amd import crossval, synth
    from wisecondor_amd import wisecondor as cli
    from wisecondor_amd import wisetools as wt
    if not torch.cuda.is_available():
        raise SystemExit("gpu_crossval_time: no GPU visible; nothing is measured without one")
    shape = dict(SHAPES[name])
    binsize, n, folds, refsize = shape["binsize"], shape["samples"], shape["folds"], shape["refsize"]
    profile = synth.bin_profile(binsize)
    samples = [synth.make_sample(profile, seed=7000 + i) for i in range(n)]
    sizes = synth.chrom_bins(binsize)
    counts = wt.samples_to_counts(samples, sizes)
    fold_of = crossval.foldPlan(n, folds, seed=1)
    shape.update(name=name, bins_per_row=int(sum(sizes)), windows=list(crossval.DEFAULT_WINDOWS))

    def device(stage_ms=None):
        torch.cuda.synchronize()
        began = time.perf_counter()
        out = crossval.crossval_batch(counts, sizes, fold_of, binsize, refsize=refsize, stage_ms=stage_ms)
        return time.perf_counter() - began, out

    def host():
        torch.cuda.synchronize()
        began = time.perf_counter()
        n_calls = np.zeros(n, dtype=np.int64)
        for fold in range(folds):
            rest, held = np.flatnonzero(fold_of != fold), np.flatnonzero(fold_of == fold)
            _, chrom_bins, mask, corrected, comps, mean, masked = wt.prepReference(None, counts=counts[rest], chrom_bins=sizes)
            idx, dst = wt.getReference(corrected, masked, np.cumsum(masked), refsize, 1, 1)
            reference = wt.Reference(idx, dst, chrom_bins, masked, mask, mean, comps, binsize=binsize)
            outs = wt.test_batch(reference, [samples[i] for i in held], cli.zThreshold(masked, 1000, None))
            reference.close()
            n_calls[held] = [len(o["results_calls"]) for o in outs]
        return time.perf_counter() - began, n_calls

    _, warm = device()
    _, warm_calls = host()
    assert np.array_equal(warm["rec_i"][:, 1], warm_calls), "the two routes disagree on the calls per sample"
    device_s, host_s = [], []
    for _ in range(repeats):
        took, out = device()
        device_s.append(took)
        assert np.array_equal(out["rec_i"], warm["rec_i"])
        took, calls = host()
        host_s.append(took)
        assert np.array_equal(calls, warm_calls)
    stage_ms = {}
    staged_s, _ = device(stage_ms)
    d, h = spread(device_s), spread(host_s)
    total = sum(stage_ms.values())
    shape.update(device_wall_s=d, host_route_wall_s=h, host_route_spread_s=h["max"] - h["min"],
                 within_spread=bool(d["median"] <= h["median"] + (h["max"] - h["min"])),
                 device_wall_with_events_s=staged_s, stage_ms_summed_over_folds=stage_ms,
                 reference_creation_share_of_stages=stage_ms.get("reference", 0.0) / total if total else None,
                 samples_with_calls=int((warm["rec_i"][:, 1] > 0).sum()), calls=int(warm["rec_i"][:, 1].sum()),
                 windows_table=[[None if v != v else v for v in row] for row in crossval.windowsTable(
                     list(crossval.DEFAULT_WINDOWS), warm["win_n"], warm["win_i"], warm["win_hist"], warm["rec_f"][:, 1]).tolist()])
    print("gpu_crossval_time: %s: device %.3f s, host route %.3f s (spread %.3f s), reference creation %.0f %% of the stages"
          % (name, d["median"], h["median"], h["max"] - h["min"], 100 * (shape["reference_creation_share_of_stages"] or 0)), flush=True)
    return shape


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossval_times.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
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
            raise SystemExit("gpu_crossval_time: the %s step ended with status %d; nothing more is started" % (name, done.returncode))
        shapes.append(json.loads(lines[-1][len("SHAPE "):]))
    with open(args.out, "w") as f:
        json.dump({"what": "crossval: crossval_batch end to end, its stages, and the public host-array route fold by fold",
                   "repeats": args.repeats, "not_measured": "real samples; file I/O (loading the samples, writing the outputs)",
                   "shapes": shapes}, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
