"""Largest component and correctedData error of the GPU newref prep against the oracle for every case of
tests/prep_cases.py (the cases of tests/test_prep_shapes_gpu.py), next to the error of numpy's float64 Gram route
on the same case, and the wall time of one prepReference call.  A GPU error more than about 1 000 times the CPU
route's is worth a look even where it passes the tests' tolerances.
    python3 tools/gpu_prep_shapes.py [--out profiles/prep_shapes_errors.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import prep_cases as pc                                  # noqa: E402
from wisecondor_amd import wisetools as wt               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "prep_shapes_errors.json"))
    args = ap.parse_args()
    runs = [(case, "auto") for case in pc.ALL_CASES if case[0] >= 3]
    runs += [((100, 1025, 8), "gpu"), ((100, 1025, 8), "host")]
    rows = []
    for case, eig in runs:
        n_s, n_b, n_comp = case
        os.environ["WC_PREP_EIG"] = eig
        counts, sizes = pc.make_case(n_s, n_b)
        want = pc.oracle(*case)
        wt.prepReference(None, pcacomp=n_comp, counts=counts, chrom_bins=sizes)          # (sizes the workspaces)
        t0 = time.perf_counter()
        got = wt.prepReference(None, pcacomp=n_comp, counts=counts, chrom_bins=sizes)
        ms = 1e3 * (time.perf_counter() - t0)
        comp_err, corr_err = pc.errors(got[3], got[4], want)
        cpu_corrected, cpu_comps, _ = pc.gram_route(want["masked"], n_comp)
        cpu_comp_err, cpu_corr_err = pc.errors(cpu_corrected, cpu_comps, want)
        ratios = want["sing"][:n_comp] / want["sing"][1:n_comp + 1]
        rows.append(dict(samples=n_s, masked_bins=n_b, n_comp=n_comp, eig=eig, components_max_abs_err=comp_err,
                         corrected_max_rel_err=corr_err, cpu_gram_components_max_abs_err=cpu_comp_err,
                         cpu_gram_corrected_max_rel_err=cpu_corr_err, smallest_singular_ratio=float(ratios.min()),
                         prep_ms=round(ms, 2)))
        print("%-18s eig %-4s components %.2e (numpy Gram route %.2e)  correctedData %.2e (%.2e)  %.1f ms"
              % (pc.case_id(case), eig, comp_err, cpu_comp_err, corr_err, cpu_corr_err, ms), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(tolerances=dict(components_abs=pc.COMP_ATOL, corrected_rel=pc.CORRECTED_RTOL), cases=rows), f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
