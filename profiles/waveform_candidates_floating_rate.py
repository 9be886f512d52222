"""What a mechanism grid under floating_l1norm / floating_l2norm costs through kiwi_hip_waveform_candidates_floating, on configuration
2's set-up as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the
36 x 10 x 36 = 12 960 double couples at 10 degrees as candidates, for 1 and 16 locations, 5 and 21 shifts per receiver, under
floating_l1norm inside with l1norm outside and floating_l2norm inside with l2norm outside.  Per case: the whole
`waveform_candidates_floating_params` call by the host clock, best of `reps` after a warm-up, every run listed, with the four
HIP-event times (evaluation, floating slot kernel, fold kernels, downloads; kiwi_hip_get_waveform_candidates_floating_ms).

The yardstick is what the library offered before: `misfits_for_params` of the same ngroup x 12 960 `moment_tensor` rows under the
same floating method and ranges, same context, same run, unscaled at both sizes.  The gate: at 16 locations and 21 shifts the call
takes less time than the yardstick in both set-ups.  Beside it `waveform_candidates_params` on the same traces under the plain norm
(no shifts): the slot kernels' times give what a shift costs, seconds per (candidate, sample, shift) against seconds per
(candidate, sample).

    python profiles/waveform_candidates_floating_rate.py [out.json] [--commit=<id>] [--reps=3] [--groups=1,16] [--shifts=5,21]"""
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
EVENTS = ("evaluation_ms", "slot_kernel_ms", "fold_kernels_ms", "download_ms")
SETUPS = (("l1norm", "l1norm"), ("l2norm", "l2norm"))       # (inside: floating_<it>, outside)


def timed(reps, call, ms):
    call()                                                    # (warm-up)
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, ms()))))
    return out, runs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    groups = [int(g) for g in opt.get("groups", "1,16").split(",")]
    nshifts = [int(g) for g in opt.get("shifts", "5,21").split(",")]
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
    shape = p.waveform_candidates_floating_shape(K)
    samples = int(sum(len(p.get_reference(ir + 1, k + 1, 2, maxn=1 << 14)[1]) for ir in range(nrec) for k in range(len(p.components[ir]))))
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, window_samples=L, window_samples_per_location=samples, reps=reps,
               candidates_per_workgroup=shape[0], samples_per_stage=shape[1], shifts_per_pass=shape[2], cases=[],
               not_measured=["several devices", "K other than 6", "cand_shift and slot_misfit at this size", "hardware counters"])
    gate = True
    for inner, outer in SETUPS:
        for ns in nshifts:
            half = (ns - 1) // 2
            for ngroup in groups:
                rows = basis[:ngroup * K]
                pairs = ngroup * ncand * samples
                # beside it: the plain norm on the same traces, no shifts
                p.set_floating_shiftrange(0, 0.0, 0.0)
                p.set_misfit_method(inner)
                _, plain = timed(reps, lambda: p.waveform_candidates_params("moment_tensor", rows, K, cand, outer_norm=outer, misfit=False),
                                 p.waveform_candidates_ms)
                p.set_misfit_method("floating_" + inner)
                p.set_floating_shiftrange(0, -half * dt, (ns - 1 - half) * dt)
                scan, runs = timed(reps, lambda: p.waveform_candidates_floating_params("moment_tensor", rows, K, cand, outer_norm=outer, misfit=False),
                                   p.waveform_candidates_floating_ms)
                best = min(runs, key=lambda r: r["call_s"])
                kernel_s = min(r["slot_kernel_ms"] for r in runs) * 1e-3
                plain_s = min(r["slot_kernel_ms"] for r in plain) * 1e-3
                case = dict(ngroup=ngroup, inner_norm="floating_" + inner, outer_norm=outer, shifts_per_receiver=ns, syntheses=ngroup * K,
                            trial_sources=ngroup * ncand, runs=runs, best_call_s=best["call_s"], trial_sources_per_s=ngroup * ncand / best["call_s"],
                            candidate_sample_pairs=pairs, seconds_per_candidate_sample_shift=kernel_s / (pairs * ns),
                            plain_norm_waveform_candidates=dict(runs=plain, best_call_s=min(r["call_s"] for r in plain),
                                                                seconds_per_candidate_sample=plain_s / pairs),
                            slot_kernel_over_the_plain_slot_kernel=kernel_s / plain_s,
                            status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                            best_misfit_range=[float(np.nanmin(scan.best_misfit)), float(np.nanmax(scan.best_misfit))],
                            best_shift_range=[int(scan.best_shift.min()), int(scan.best_shift.max())])
                grid = synthetic.mt_sdr_grid()
                trials = np.tile(grid, (ngroup, 1))
                trials[:, :4] = np.repeat(rows[::K, :4], ncand, axis=0)
                trials[:, 10] = rows[0, 10]
                p.misfits_for_params("moment_tensor", trials[:ncand])
                yruns = []
                for _ in range(reps):
                    t = time.perf_counter()
                    p.misfits_for_params("moment_tensor", trials)
                    yruns.append(time.perf_counter() - t)
                y = min(yruns)
                case["yardstick_misfits_for_params"] = dict(runs_s=yruns, best_call_s=y, syntheses=len(trials), scaled=False)
                case["yardstick_over_this_call"] = y / best["call_s"]
                if ngroup == 16 and ns == 21 and not best["call_s"] < y:
                    gate = False
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    p.close()
    res["gate_16_locations_21_shifts_faster_than_the_yardstick"] = gate
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
        sys.exit("gate: the call at 16 locations and 21 shifts took longer than misfits_for_params of the same trial sources under the same method")


if __name__ == "__main__":
    main()
