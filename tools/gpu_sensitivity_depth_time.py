#!/usr/bin/env python3
"""Time `sensitivity` with depths and the binomial spike at the shapes of profiles/sensitivity_times.json (synthetic data of
the bench's kind, a reference of 40 samples with refsize 100, 8 healthy samples, 256 and 4 096 trials per depth) and
write profiles/sensitivity_depth_times.json.

    python tools/gpu_sensitivity_depth_time.py --binsizes 250000 [--parent-lib PATH] --out profiles/sensitivity_depth_times.json

The command itself never touches the GPU: per bin size it starts one child (`--step BINSIZE`) under its own `timeout`,
and with --parent-lib (the parent commit's build of the library) two more that measure the unchanged deterministic route
alone, on that build and on this one, one after the other in the same session; it starts nothing more after a child that
failed.  A child measures in ONE process, `--repeats` (3) runs after a warm-up each, per trial count:
  (a) fixed          wt.sensitivity_batch as it always was called: the deterministic route, trials per second
  (b) draw           the same plan with draw=True
  (c) depths         depths 1, 0.5, 0.25, 0.1 (four times the plan's rows) without and with draw
  stages             the thinning of the 8 samples to 4 depths (wc_thin_counts_dev) and the spike of one batch, deterministic
                     and drawn (wc_spike_counts_ex_dev), each between device synchronises
  k_thin             Philox blocks per second of the thinning (ceil(c / 4) per bin, one pass for all depths), of the same
                     kernel on bins of equal counts that fill the machine, and of a bare loop of the same rounds over
                     registers (wc_philox_spin_dev, between device events): the kernel's roofline is ALU work
  host               (c) with draw through the numpy restatement (tests/draw_restated.py) -> wt.test_batch -> the Python
                     score: ONE run (the restated thinning of 80 M reads takes tens of seconds)
No figure is asserted anywhere.  The host route is the restatement, never the code under test."""
import argparse
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
DEPTHS = [1000000, 500000, 250000, 100000]
NEW_SYMBOLS = ("wc_philox_spin_dev", "wc_philox4x32_host", "wc_philox4x32", "wc_thin_counts_dev", "wc_thin_counts", "wc_thin_wave_cutoff",
               "wc_spike_counts_ex_dev", "wc_spike_counts_ex", "wc_sensitivity_batch_ex_dev")


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": list(values)}


def timed(fn, repeats):
    import torch
    fn()                                                        # warm-up
    walls = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        began = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - began)
    return spread(walls), out


def setup(binsize):
    import torch
    from wisecondor_amd import synth
    from wisecondor_amd import wisecondor as cli
    from wisecondor_amd import wisetools as wt
    if not torch.cuda.is_available():
        raise SystemExit("gpu_sensitivity_depth_time: no GPU visible; nothing is measured without one")
    profile = synth.bin_profile(binsize)
    refs = [synth.make_sample(profile, seed=i) for i in range(40)]
    _, chrom_bins, mask, corrected, comps, mean, masked_bins = wt.prepReference(refs)
    masked_bins = np.asarray(masked_bins, dtype=np.int64)
    idx, dst = wt.getReference(corrected, masked_bins, np.cumsum(masked_bins), 100, 1, 1)
    reference = wt.Reference(idx, dst, np.asarray(chrom_bins, dtype=np.int64), masked_bins, mask, mean, comps, binsize=binsize)
    cut = cli.zThreshold([int(v) for v in masked_bins], 1000, None)
    healthy = [synth.make_sample(profile, seed=3000 + i) for i in range(N_HEALTHY)]
    lengths_bins = [int(np.ceil(length / binsize)) for length in LENGTHS_BP]
    return reference, cut, healthy, lengths_bins


def plan_of(sensitivity, reference, lengths_bins, n_trials, n_depths=1):
    per = -(-n_trials // (N_HEALTHY * len(lengths_bins) * len(EFFECTS_PPM)))
    return sensitivity.makePlan(reference, N_HEALTHY, lengths_bins, list(EFFECTS_PPM), per, seed=1, n_depths=n_depths)


def step_fixed(binsize, repeats):
    """(a) alone; runs on either build of the library (the new symbols are not asked of the parent's)."""
    from wisecondor_amd import _lib
    if os.environ.get("WC_LIB_PATH"):
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    from wisecondor_amd import sensitivity
    reference, cut, healthy, lengths_bins = setup(binsize)
    shapes = []
    for n_trials in TRIALS:
        plan = plan_of(sensitivity, reference, lengths_bins, n_trials)[:n_trials]
        walls, _ = timed(lambda: sensitivity.sensitivity_batch(reference, healthy, plan, cut, batch=BATCH), repeats)
        shapes.append({"binsize": binsize, "trials": n_trials, "library": os.environ.get("WC_LIB_PATH") and "parent" or "change",
                       "fixed_wall_s": walls, "fixed_trials_per_s": n_trials / walls["median"]})
    reference.close()
    return shapes


def step(binsize, repeats):
    import torch
    import draw_restated as dr
    import spike_restated as sr
    from wisecondor_amd import _lib, sensitivity
    from wisecondor_amd import wisetools as wt
    lib = _lib.load()
    reference, cut, healthy, lengths_bins = setup(binsize)
    sizes = np.ascontiguousarray(reference.chromosome_sizes, dtype=np.int64)
    n_total = reference.n_total
    dense = wt.samples_to_counts(healthy, [int(v) for v in sizes])
    base = torch.from_numpy(dense).cuda()
    keep = np.array(DEPTHS, dtype=np.int32)
    shapes = []
    # ---- the thinning stage and k_thin's rate
    image = torch.empty((len(DEPTHS) * N_HEALTHY, n_total), dtype=torch.int32, device="cuda")
    thin_walls, _ = timed(lambda: _lib.check(lib.wc_thin_counts_dev(reference.ctx, None, base.data_ptr(), N_HEALTHY, _lib.ptr(sizes), len(sizes),
                                                                    _lib.ptr(keep), len(keep), 1, image.data_ptr())), repeats)
    blocks = int(((np.maximum(dense, 0).astype(np.int64) + 3) // 4).sum())
    # the same kernel on bins that fill the machine, every bin with the cohort's mean count: every lane runs the same trips
    mean_c = int(np.maximum(dense, 0).mean())
    even = torch.full((1, 256 * 256 * 8), mean_c, dtype=torch.int32, device="cuda")
    even_out = torch.empty((len(DEPTHS),) + tuple(even.shape), dtype=torch.int32, device="cuda")
    even_sizes = np.array([even.shape[1]], dtype=np.int64)
    even_walls, _ = timed(lambda: _lib.check(lib.wc_thin_counts_dev(reference.ctx, None, even.data_ptr(), 1, _lib.ptr(even_sizes), 1, _lib.ptr(keep),
                                                                    len(keep), 1, even_out.data_ptr())), repeats)
    bare_blocks = even.shape[1] * ((mean_c + 3) // 4)
    lanes, spin_blocks = 256 * 256 * 8 * 4, 4096
    spin_out = torch.empty((lanes,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    spin_ms = []
    for i in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        _lib.check(lib.wc_philox_spin_dev(reference.ctx, stream, lanes, spin_blocks, 1, spin_out.data_ptr()))
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            spin_ms.append(ev[0].elapsed_time(ev[1]))
    spin = {"lanes": lanes, "blocks_per_lane": spin_blocks, "ms": spread(spin_ms), "blocks_per_s": lanes * spin_blocks / spread(spin_ms)["median"] * 1e3}
    thin = {"wall_s": thin_walls, "spin": spin, "philox_blocks": blocks, "blocks_per_s": blocks / thin_walls["median"],
            "even_bins": {"bins": even.shape[1], "reads_per_bin": mean_c, "wall_s": even_walls, "philox_blocks": bare_blocks,
                          "blocks_per_s": bare_blocks / even_walls["median"]},
            "note": "both intervals hold the host's checks, the check kernel and its read-back as well as k_thin"}
    print("gpu_sensitivity_depth_time: %d kb: thinning %.2f ms, %.3g blocks/s; even bins %.3g blocks/s; bare rounds %.3g blocks/s"
          % (binsize // 1000, thin_walls["median"] * 1e3, thin["blocks_per_s"], thin["even_bins"]["blocks_per_s"], spin["blocks_per_s"]), flush=True)
    del even, even_out
    for n_trials in TRIALS:
        plan = plan_of(sensitivity, reference, lengths_bins, n_trials)[:n_trials]
        deep = plan_of(sensitivity, reference, lengths_bins, n_trials, len(DEPTHS))
        shape = {"binsize": binsize, "trials": n_trials, "trials_with_depths": len(deep), "bins_per_row": n_total, "depths_ppm": DEPTHS,
                 "healthy_samples": N_HEALTHY, "batch": BATCH, "thinning": thin}
        run = lambda rows, **kw: sensitivity.sensitivity_batch(reference, healthy, rows, cut, batch=BATCH, **kw)       # noqa: E731
        for name, rows, kw in (("fixed", plan, {}), ("draw", plan, dict(draw=True)), ("depths", deep, dict(depths_ppm=DEPTHS)),
                               ("depths_draw", deep, dict(depths_ppm=DEPTHS, draw=True))):
            walls, (rec_i, rec_f) = timed(lambda: run(rows, **kw), repeats)
            shape[name + "_wall_s"] = walls
            shape[name + "_trials_per_s"] = len(rows) / walls["median"]
            if name == "depths_draw":
                table = sensitivity.sensitivityTable(rows, rec_i, rec_f, lengths_bins, list(EFFECTS_PPM), depths_ppm=DEPTHS, n_samples=N_HEALTHY)
                shape["table_depths_draw"] = [[None if v != v else v for v in row] for row in table.tolist()]
                deep_i = rec_i
        # ---- the spike stage of one batch on its own, deterministic and drawn
        part = np.ascontiguousarray(plan[:BATCH])
        counts = torch.empty((len(part), n_total), dtype=torch.int32, device="cuda")
        for name, flag in (("spike_fixed_s", 0), ("spike_draw_s", 1)):
            walls, _ = timed(lambda: _lib.check(lib.wc_spike_counts_ex_dev(reference.ctx, None, base.data_ptr(), N_HEALTHY, _lib.ptr(sizes), len(sizes),
                                                                           _lib.ptr(part), len(part), flag, 1, 0, counts.data_ptr(), None)), repeats)
            shape[name] = walls
        shape["spike_stage_trials"] = len(part)
        # ---- host route of (c) with draw, once
        offs = np.concatenate([[0], np.cumsum(sizes)])
        began = time.perf_counter()
        thinned = dr.thin(dense, sizes, DEPTHS, 1).reshape(len(DEPTHS) * N_HEALTHY, -1)
        t1 = time.perf_counter()
        spiked, _ = dr.spike_draw(thinned, sizes, deep, 1, 0)
        dicts = [{str(c + 1): row[offs[c]:offs[c + 1]] for c in range(len(sizes))} for row in spiked]
        t2 = time.perf_counter()
        outs = wt.test_batch(reference, dicts, cut)
        t3 = time.perf_counter()
        host_i, _ = sr.score_lists(deep, [o["results_calls"] for o in outs])
        t4 = time.perf_counter()
        assert np.array_equal(host_i, deep_i)
        shape["host_parts_s_thin_spike_test_score"] = [t1 - began, t2 - t1, t3 - t2, t4 - t3]
        shape["host_wall_s"] = t4 - began
        shape["host_trials_per_s"] = len(deep) / (t4 - began)
        del outs, dicts, spiked, thinned
        shapes.append(shape)
        print("gpu_sensitivity_depth_time: %d kb, %d trials: fixed %.0f, draw %.0f, depths %.0f, depths+draw %.0f, host %.0f trials/s"
              % (binsize // 1000, n_trials, shape["fixed_trials_per_s"], shape["draw_trials_per_s"], shape["depths_trials_per_s"],
                 shape["depths_draw_trials_per_s"], shape["host_trials_per_s"]), flush=True)
    reference.close()
    return shapes


def child(args, binsize, mode, env=None):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(binsize), "--mode", mode,
           "--repeats", str(args.repeats)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("SHAPES ")]
    for ln in done.stdout.splitlines():
        if not ln.startswith("SHAPES "):
            print(ln, flush=True)
    if done.returncode != 0 or not lines:
        raise SystemExit("gpu_sensitivity_depth_time: the %d bp %s step ended with status %d; nothing more is started"
                         % (binsize, mode, done.returncode))
    return json.loads(lines[-1][len("SHAPES "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_depth_times.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--binsizes", type=int, nargs="+", default=[250000, 50000])
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build of the library: (a) is measured on it too")
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--step", type=int, default=None, help="(a child) measure this bin size and print its shapes as JSON")
    ap.add_argument("--mode", choices=("all", "fixed"), default="all")
    ap.add_argument("--merge", action="store_true", help="keep the bin sizes --out already has and is not asked for again")
    args = ap.parse_args()
    if args.step is not None:
        print("SHAPES " + json.dumps(step(args.step, args.repeats) if args.mode == "all" else step_fixed(args.step, args.repeats)))
        return
    shapes, builds = [], []
    if args.merge and os.path.exists(args.out):
        old = json.load(open(args.out))
        shapes = [s for s in old["shapes"] if s["binsize"] not in args.binsizes]
        builds = [s for s in old["parent_and_change"] if s["binsize"] not in args.binsizes]
    for binsize in args.binsizes:
        if args.parent_lib:
            builds.extend(child(args, binsize, "fixed", dict(os.environ, WC_LIB_PATH=os.path.abspath(args.parent_lib))))
            builds.extend(child(args, binsize, "fixed"))
        shapes.extend(child(args, binsize, "all"))
    with open(args.out, "w") as f:
        json.dump({"what": "sensitivity with depths and the binomial spike: the routes, the thinning and spike stages, k_thin's rate, "
                           "the host route once; parent_and_change: the deterministic route on the parent commit's library and on this one",
                   "repeats": args.repeats, "parent_and_change": builds, "shapes": shapes}, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
