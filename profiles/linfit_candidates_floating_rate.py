"""What a mechanism grid with per-receiver shifts costs through kiwi_hip_linear_fit_candidates_floating, on configuration 2's set-up
as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 =
12 960 double couples at 10 degrees as candidates, for ngroup = 1 and 16 locations, shift ranges of 5 and of 21 samples on all
receivers, under the outer l1norm and l2norm.  Per case: the whole `linear_fit_candidates_floating_params` call by the host clock,
best of `reps` after a warm-up, every run listed, with the four HIP-event times (evaluation, Gram + cross-correlation kernels,
candidate kernels, downloads; kiwi_hip_get_linear_fit_candidates_floating_ms); candidate-receiver-shift triples per second of the
candidate kernels.  Beside the Gram + cross-correlation time stands the Gram + solve time of `linear_fit_candidates_params` under
l2norm on the same rows in the same run (the same Gram kernel on the same inputs); their difference is what the cross-correlation
kernel adds, to the extent the solve kernel's time is small.

The yardstick is what the library offered before: `misfits_for_params` of the same ngroup x 12 960 `moment_tensor` rows under
floating_l2norm with the same ranges, same context, same run.  The gate: at ngroup = 16 every call takes less time than the yardstick.

    python profiles/linfit_candidates_floating_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
EVENTS = ("evaluation_ms", "gram_and_xcorr_ms", "candidate_kernels_ms", "download_ms")


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
    dt = gf["dt"]
    basis = cfg2_locations(wl)
    nrec = wl["nrec"]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    shape = p.linear_fit_candidates_floating_shape(K)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, window_samples=L, reps=reps, candidates_per_workgroup=shape[0],
               shifts_per_pass=shape[1], shifts_per_stage=shape[2], cases=[],
               not_timed=["several devices", "K other than 6", "cand_shift and receiver_misfit at this size"])
    gate = True
    for ngroup in (1, 16):
        rows = basis[:ngroup * K]
        p.set_misfit_method("l2norm")
        p.set_floating_shiftrange(0, 0.0, 0.0)
        p.linear_fit_candidates_params("moment_tensor", rows, K, cand, outer_norm="l2norm", misfit=False)
        gram_solve = []
        for _ in range(reps):
            p.linear_fit_candidates_params("moment_tensor", rows, K, cand, outer_norm="l2norm", misfit=False)
            gram_solve.append(p.linear_fit_candidates_ms()[1])
        grid = synthetic.mt_sdr_grid()
        trials = np.tile(grid, (ngroup, 1))
        trials[:, :4] = np.repeat(rows[::K, :4], ncand, axis=0)
        trials[:, 10] = rows[0, 10]
        for half in (2, 10):
            ns = 2 * half + 1
            p.set_misfit_method("floating_l2norm")
            p.set_floating_shiftrange(0, -half * dt, half * dt)
            p.misfits_for_params("moment_tensor", trials)
            yruns = []
            for _ in range(reps):
                t = time.perf_counter()
                p.misfits_for_params("moment_tensor", trials)
                yruns.append(time.perf_counter() - t)
            y = min(yruns)
            for norm in ("l1norm", "l2norm"):
                kw = dict(outer_norm=norm, misfit=True)
                p.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, **kw)
                runs = []
                for _ in range(reps):
                    t = time.perf_counter()
                    scan = p.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, **kw)
                    runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.linear_fit_candidates_floating_ms()))))
                best = min(runs, key=lambda r: r["call_s"])
                triples = ngroup * ncand * nrec * ns
                kernel_s = min(r["candidate_kernels_ms"] for r in runs) * 1e-3
                gx = min(r["gram_and_xcorr_ms"] for r in runs)
                case = dict(ngroup=ngroup, shifts=ns, outer_norm=norm, syntheses=ngroup * K, trial_sources=ngroup * ncand, runs=runs,
                            best_call_s=best["call_s"], trial_sources_per_s=ngroup * ncand / best["call_s"],
                            candidate_receiver_shift_triples=triples, triples_per_s_of_the_candidate_kernels=triples / kernel_s,
                            gram_and_xcorr_ms=gx, gram_and_solve_ms_of_linear_fit_candidates_same_rows=min(gram_solve),
                            xcorr_ms_as_their_difference=gx - min(gram_solve),
                            yardstick_misfits_for_params=dict(runs_s=yruns, best_call_s=y, syntheses=len(trials)),
                            yardstick_over_this_call=y / best["call_s"],
                            status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                            best_misfit_range=[float(np.nanmin(scan.best_misfit)), float(np.nanmax(scan.best_misfit))])
                if ngroup == 16 and not best["call_s"] < y:
                    gate = False
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    p.close()
    res["gate_ngroup_16_faster_than_the_yardstick"] = gate
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
    if not gate:
        sys.exit("gate: a call at ngroup = 16 took longer than misfits_for_params of the same trial sources under floating_l2norm")


if __name__ == "__main__":
    main()
