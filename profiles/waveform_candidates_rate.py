"""What a mechanism grid under l1norm inside costs through kiwi_hip_waveform_candidates, on configuration 2's set-up as bench.py makes
it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 = 12 960 double
couples at 10 degrees as candidates, for ngroup = 1, 16 and 2160 locations, under l1norm inside with both outer norms and under
l2norm inside once.  Per case: the whole `waveform_candidates_params` call by the host clock, best of `reps` after a warm-up,
every run listed, with the four HIP-event times (evaluation, slot kernel, fold kernels, downloads;
kiwi_hip_get_waveform_candidates_ms) and the (candidate, sample) pairs per second of the slot kernel, which spends about 15
vector instructions on a pair at K = 6 (11 multiplies and adds, the difference, |.|, a conversion and an fp64 add; two LDS reads).

The yardstick is what the library offered before: `misfits_for_params` of the same ngroup x 12 960 `moment_tensor` rows under the
same method, same context, same run -- at 1 and 16 locations; at 2160 it is scaled from 16 and marked as scaled.  The gate: at
ngroup = 16 the call takes less time than the yardstick in every set-up.  The one-location row is reported whichever way it falls.

    python profiles/waveform_candidates_rate.py [out.json] [--commit=<id>] [--reps=3] [--groups=1,16,2160]"""
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
SETUPS = (("l1norm", "l1norm"), ("l1norm", "l2norm"), ("l2norm", "l2norm"))       # (inside, outside)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    groups = [int(g) for g in opt.get("groups", "1,16,2160").split(",")]
    import torch
    import bench
    from kiwi_amd import mtfit, synthetic
    from linfit_rate import cfg2_locations
    wl = synthetic.workload("cfg2", 512, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    basis = cfg2_locations(wl)
    nrec = wl["nrec"]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    shape = p.waveform_candidates_shape(K)
    samples = int(sum(len(p.get_reference(ir + 1, k + 1, 2, maxn=1 << 14)[1]) for ir in range(nrec) for k in range(len(p.components[ir]))))
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, window_samples=L, window_samples_per_location=samples, reps=reps,
               candidates_per_workgroup=shape[0], samples_per_stage=shape[1], counted_vector_instructions_per_pair=15, cases=[],
               not_timed=["several devices", "K other than 6", "slot_misfit at this size", "hardware counters",
                          "the yardstick at 2160 locations (scaled from 16)"])
    gate = True
    for inner, outer in SETUPS:
        p.set_misfit_method(inner)
        yard16 = None
        for ngroup in groups:
            rows = basis[:ngroup * K]
            kw = dict(outer_norm=outer, misfit=False)
            p.waveform_candidates_params("moment_tensor", rows, K, cand, **kw)          # (warm-up)
            runs = []
            for _ in range(reps):
                t = time.perf_counter()
                scan = p.waveform_candidates_params("moment_tensor", rows, K, cand, **kw)
                runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.waveform_candidates_ms()))))
            best = min(runs, key=lambda r: r["call_s"])
            pairs = ngroup * ncand * samples
            kernel_s = min(r["slot_kernel_ms"] for r in runs) * 1e-3
            case = dict(ngroup=ngroup, inner_norm=inner, outer_norm=outer, syntheses=ngroup * K, trial_sources=ngroup * ncand, runs=runs,
                        best_call_s=best["call_s"], trial_sources_per_s=ngroup * ncand / best["call_s"],
                        candidate_sample_pairs=pairs, pairs_per_s_of_the_slot_kernel=pairs / kernel_s,
                        status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                        best_misfit_range=[float(np.nanmin(scan.best_misfit)), float(np.nanmax(scan.best_misfit))])
            if ngroup <= 16:
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
                if ngroup == 16:
                    yard16 = y
                    if not best["call_s"] < y:
                        gate = False
            elif yard16 is not None:
                y = yard16 * ngroup / 16.0
                case["yardstick_misfits_for_params"] = dict(best_call_s=y, syntheses=ngroup * ncand, scaled=True, scaled_from_ngroup=16)
            else:
                y = None
            if y is not None:
                case["yardstick_over_this_call"] = y / best["call_s"]
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
        sys.exit("gate: the call at ngroup = 16 took longer than misfits_for_params of the same trial sources under the same method")


if __name__ == "__main__":
    main()
