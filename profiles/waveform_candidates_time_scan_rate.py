"""What a mechanism grid x origin times under l1norm / l2norm costs through kiwi_hip_waveform_candidates_time_scan, on configuration
2's set-up as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the
36 x 10 x 36 = 12 960 double couples at 10 degrees as candidates, for 1 and 16 locations, 5 and 21 origin times, under l1norm inside
and outside and l2norm inside and outside.  Per case: the whole `waveform_candidates_time_scan_params` call by the host clock, best
of `reps` after a warm-up, every run listed, with the four HIP-event times (evaluation, rows + scan kernel, fold kernels, downloads;
kiwi_hip_get_waveform_candidates_time_scan_ms).

The yardstick is what the library offered before: the nk separate `waveform_candidates_params` calls with the rows' times moved by
k dt, on the same context in the same run.  The gate: at 16 locations and 21 origin times under l1norm the scan takes less time than
the yardstick.

    python profiles/waveform_candidates_time_scan_rate.py [out.json] [--commit=<id>] [--reps=3] [--groups=1,16] [--offsets=5,21]"""
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
EVENTS = ("evaluation_ms", "scan_kernels_ms", "fold_kernels_ms", "download_ms")
SETUPS = (("l1norm", "l1norm"), ("l2norm", "l2norm"))       # (inside, outside)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    groups = [int(g) for g in opt.get("groups", "1,16").split(",")]
    noffsets = [int(g) for g in opt.get("offsets", "5,21").split(",")]
    import torch
    import bench
    from kiwi_amd import mtfit, synthetic
    from linfit_rate import cfg2_locations
    wl = synthetic.workload("cfg2", 512, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    dt = float(p.dt)
    basis = cfg2_locations(wl)
    nrec = wl["nrec"]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    shape = p.waveform_candidates_time_scan_shape(K)
    samples = int(sum(len(p.get_reference(ir + 1, k + 1, 2, maxn=1 << 14)[1]) for ir in range(nrec) for k in range(len(p.components[ir]))))
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, window_samples=L, window_samples_per_location=samples, reps=reps,
               candidates_per_workgroup=shape[0], samples_per_stage=shape[1], offsets_per_pass=shape[2], cases=[],
               not_measured=["several devices", "K other than 6", "cand_misfit, misfit, slot_misfit and rows at this size (the call returns the "
                             "bests per offset only here)", "offset steps other than one sample", "hardware counters"])
    gate = True
    for inner, outer in SETUPS:
        p.set_misfit_method(inner)
        for nk in noffsets:
            k0 = -((nk - 1) // 2)
            for ngroup in groups:
                rows = basis[:ngroup * K]
                pairs = ngroup * ncand * samples

                def scan_call():
                    return p.waveform_candidates_time_scan_params("moment_tensor", rows, K, k0, 1, nk, cand, outer_norm=outer, cand_misfit=False,
                                                                  cand_offset=False)
                scan_call()                                   # (warm-up)
                runs = []
                for _ in range(reps):
                    t = time.perf_counter()
                    scan = scan_call()
                    runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.waveform_candidates_time_scan_ms()))))
                best = min(runs, key=lambda r: r["call_s"])
                kernel_s = min(r["scan_kernels_ms"] for r in runs) * 1e-3

                # the yardstick: one plain call per origin time, the rows' times moved by k dt
                def separate():
                    out, slot_ms = [], 0.0
                    for j in range(nk):
                        moved = rows.copy()
                        moved[:, 0] += np.float32((k0 + j) * dt)
                        out.append(p.waveform_candidates_params("moment_tensor", moved, K, cand, outer_norm=outer, misfit=False))
                        slot_ms += p.waveform_candidates_ms()[1]
                    return out, slot_ms
                separate()
                yruns, yslot = [], []
                for _ in range(reps):
                    t = time.perf_counter()
                    plain, slot_ms = separate()
                    yruns.append(time.perf_counter() - t)
                    yslot.append(slot_ms)
                y = min(yruns)
                sep = np.stack([s.best_misfit for s in plain], 1)
                case = dict(ngroup=ngroup, inner_norm=inner, outer_norm=outer, offsets=nk, k0=k0, kstep=1, syntheses=ngroup * K,
                            trial_sources=ngroup * ncand * nk, runs=runs, best_call_s=best["call_s"],
                            trial_sources_per_s=ngroup * ncand * nk / best["call_s"], candidate_sample_pairs=pairs,
                            seconds_per_candidate_sample_offset=kernel_s / (pairs * nk),
                            yardstick_separate_waveform_candidates_params=dict(runs_s=yruns, best_call_s=y, slot_kernel_ms_summed=yslot, calls=nk,
                                                                               syntheses=ngroup * K * nk),
                            yardstick_over_this_call=y / best["call_s"],
                            scan_kernels_over_the_yardsticks_slot_kernels=kernel_s / (min(yslot) * 1e-3),
                            status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                            best_offset_counts=np.bincount(scan.best_offset[scan.best_offset >= 0], minlength=nk).tolist(),
                            largest_best_misfit_difference_to_the_separate_calls=float(np.nanmax(np.abs(scan.best_misfit - sep))))
                if inner == "l1norm" and ngroup == 16 and nk == 21 and not best["call_s"] < y:
                    gate = False
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    p.close()
    res["gate_16_locations_21_offsets_l1norm_faster_than_the_separate_calls"] = gate
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
        sys.exit("gate: the scan at 16 locations and 21 origin times under l1norm took longer than the 21 separate waveform_candidates_params calls")


if __name__ == "__main__":
    main()
