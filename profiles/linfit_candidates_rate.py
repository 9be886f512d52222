"""What a mechanism grid costs through kiwi_hip_linear_fit_candidates, on configuration 2's set-up as bench.py makes it (50 receivers
x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 = 12 960 double couples at 10 degrees
as candidates, for ngroup = 1, 16 and 2 160 locations, under the outer l1norm, the outer l2norm and the outer l2norm with a free
moment per mechanism (free_scale).  Per case: the whole `linear_fit_candidates_params` call by the host clock, best of `reps` after
a warm-up, every run listed, with the four HIP-event times (evaluation, Gram + solve, candidate kernels, downloads;
kiwi_hip_get_linear_fit_candidates_ms); candidate-receiver pairs per second of the candidate kernels; and their fp64 operation
rate from the counted operations (2 K^2 + 4 K + 8 per pair under l1norm: the products and sums of x.b, G x, x.G.x, the value, its
root and the two weighted sums; under l2norm a "pair" is a candidate and the folded row, twice the sums with free_scale).
For ngroup = 1 and 16 the full misfit array [ngroup, 12 960] is returned; for 2 160 only the best mechanism per location.

The yardstick is what the library offered before: `misfits_for_params` of the same ngroup x 12 960 `moment_tensor` rows on the same
context in the same run, for ngroup = 1 and 16; its time for 2 160 locations is SCALED from 16 (x 135) and marked so.
The gate: at ngroup = 16 every candidate call takes less time than the yardstick (96 syntheses against 207 360).

    python profiles/linfit_candidates_rate.py [out.json] [--commit=<id>] [--reps=3]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

L = 4096
K = 6
GRID = (range(0, 360, 10), range(0, 91, 10), range(-180, 180, 10))
MOMENT, UNIT = 7e18, 1e18
CASES = (("l1norm", False), ("l2norm", False), ("l2norm", True))
EVENTS = ("evaluation_ms", "gram_and_solve_ms", "candidate_kernels_ms", "download_ms")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    import torch
    import bench
    from kiwi_amd import mtfit, synthetic
    from linfit_rate import cfg2_locations
    wl = synthetic.workload("cfg2", 512, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    p.set_misfit_method("l2norm")
    basis = cfg2_locations(wl)
    nrec = wl["nrec"]
    unit_dc, _ = mtfit.double_couple_candidates(*GRID)
    ncand = len(unit_dc)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, window_samples=L, reps=reps,
               candidates_per_workgroup=p.linear_fit_candidates_shape(K)[0], receivers_per_stage=p.linear_fit_candidates_shape(K)[1],
               fp64_operations_per_pair=2 * K * K + 4 * K + 8, by_ngroup={})
    for ngroup in (1, 16, 2160):
        rows = basis[:ngroup * K]
        entry = dict(syntheses=ngroup * K, trial_sources=ngroup * ncand, full_misfit_array=ngroup <= 16)
        for norm, free in CASES:
            cand = unit_dc if free else unit_dc * (MOMENT / UNIT)
            kw = dict(outer_norm=norm, free_scale=free, misfit=ngroup <= 16)
            p.linear_fit_candidates_params("moment_tensor", rows, K, cand, **kw)
            runs = []
            for _ in range(reps):
                t = time.perf_counter()
                scan = p.linear_fit_candidates_params("moment_tensor", rows, K, cand, **kw)
                runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.linear_fit_candidates_ms()))))
            best = min(runs, key=lambda r: r["call_s"])
            pairs = ngroup * ncand * (nrec if norm == "l1norm" else 1)
            ops = pairs * (2 * K * K + 4 * K + 8) * (2 if free else 1)
            kernel_s = min(r["candidate_kernels_ms"] for r in runs) * 1e-3
            entry[norm + ("_free_scale" if free else "")] = dict(
                runs=runs, best_call_s=best["call_s"], trial_sources_per_s=ngroup * ncand / best["call_s"],
                candidate_receiver_pairs=pairs, pairs_per_s_of_the_candidate_kernels=pairs / kernel_s,
                fp64_gflops_of_the_candidate_kernels=ops / kernel_s * 1e-9,
                status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                best_misfit_range=[float(np.nanmin(scan.best_misfit)), float(np.nanmax(scan.best_misfit))])
        if ngroup <= 16:
            grid = synthetic.mt_sdr_grid()
            trials = np.tile(grid, (ngroup, 1))
            trials[:, :4] = np.repeat(rows[::K, :4], ncand, axis=0)
            trials[:, 10] = rows[0, 10]
            p.misfits_for_params("moment_tensor", trials)
            runs = []
            for _ in range(reps):
                t = time.perf_counter()
                p.misfits_for_params("moment_tensor", trials)
                runs.append(time.perf_counter() - t)
            entry["yardstick_misfits_for_params"] = dict(runs_s=runs, best_call_s=min(runs), syntheses=len(trials), measured=True)
        else:
            y16 = res["by_ngroup"]["16"]["yardstick_misfits_for_params"]["best_call_s"]
            entry["yardstick_misfits_for_params"] = dict(best_call_s=y16 * ngroup / 16.0, syntheses=ngroup * ncand, measured=False,
                                                         note="scaled from the measured ngroup = 16 by %g; not run" % (ngroup / 16.0))
        y = entry["yardstick_misfits_for_params"]["best_call_s"]
        for norm, free in CASES:
            c = entry[norm + ("_free_scale" if free else "")]
            c["yardstick_over_this_call"] = y / c["best_call_s"]
        res["by_ngroup"][str(ngroup)] = entry
        print(ngroup, json.dumps(entry), flush=True)
    p.close()
    e16 = res["by_ngroup"]["16"]
    res["gate_ngroup_16_faster_than_the_yardstick"] = all(e16[n + ("_free_scale" if f else "")]["best_call_s"] < e16["yardstick_misfits_for_params"]["best_call_s"]
                                                          for n, f in CASES)
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    print(json.dumps(res))
    if args:
        with open(args[0], "w") as fh:
            json.dump(res, fh, indent=1)
    if not res["gate_ngroup_16_faster_than_the_yardstick"]:
        sys.exit("gate: a candidate call at ngroup = 16 took longer than misfits_for_params of the same trial sources")


if __name__ == "__main__":
    main()
