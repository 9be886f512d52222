"""What the joint bootstrap of a mechanism grid under ampspec_l2norm inside and l2norm outside costs through
kiwi_hip_spectral_candidates_bootstrap, on configuration 2's set-up as bench.py makes it (50 receivers x 3 components x 4096
samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 = 12 960 double couples at 10 degrees as candidates.  Rows:
16 locations with a pass band (corners 0.05, 0.1, 0.3, 0.4 of Nyquist) on every receiver at 100 and 1000 draws, 16 locations
without a filter at 100 draws, ONE location without a filter at 100 draws (draw 0 of ones, the others resampling counts).  Per row:
the whole `spectral_candidates_bootstrap_params` call by the host clock, best of `reps` after a warm-up, every run listed, with the
five HIP-event times (evaluation, spectra kernel, slot kernel, bootstrap kernels, downloads;
kiwi_hip_get_spectral_candidates_bootstrap_ms).

The yardstick is what the library offered before, on the same context in the same run:
`spectral_candidates_params(..., slot_misfit=True)`, which downloads slot_misfit [ngroup, 12 960, 150], then
`Engine.outer_misfits_slots` on it, which uploads it again; its candidate kernel (speccand_kernel, one workgroup per location and
tile, the slots one behind the other) is timed by kiwi_hip_get_spectral_candidates_ms in the same calls.  The gate: at 16
locations with the pass band and 100 draws the new call takes less time than that route.  The ratio of every row and the rates of
the two candidate kernels per (candidate, kept bin) are reported, not promised.  In the same run best_value, best_group and
best_cand of every row are compared with the host route's bits.

    python profiles/spectral_candidates_bootstrap_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
CORNERS = (0.05, 0.1, 0.3, 0.4)
EVENTS = ("evaluation_ms", "spectra_kernel_ms", "slot_kernel_ms", "bootstrap_kernels_ms", "download_ms")
NORM = "l2norm"
CASES = ((16, True, 100), (16, True, 1000), (16, False, 100), (1, False, 100))      # (locations, pass band, draws)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    import torch
    import bench
    from kiwi_amd import mtfit, synthetic
    from kiwi_amd.engine import bootstrap_draw_weights
    from linfit_rate import cfg2_locations
    wl = synthetic.workload("cfg2", 512, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    dt = gf["dt"]
    p.set_misfit_method("ampspec_l2norm")
    nrec = wl["nrec"]
    basis = cfg2_locations(wl)
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    slot_receiver = np.repeat(np.arange(nrec, dtype=np.int32), [len(c) for c in p.components])
    nmis = len(slot_receiver)
    C, T, Rmax = p.spectral_candidates_bootstrap_shape(K)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, receivers=nrec, slots=nmis, window_samples=L, inner_norm="ampspec_l2norm", outer_norm=NORM,
               reps=reps, candidates_per_workgroup=C, draws_per_tile=T, max_receivers=Rmax,
               bins_per_stage=p.spectral_candidates_shape(K, context=False)[1], rows=[])

    def flush():
        if args:
            with open(args[0], "w") as fh:
                json.dump(res, fh, indent=1)

    filtered_now = False
    for ngroup, filtered, ndraw in CASES:
        if filtered != filtered_now:
            for ir in range(1, nrec + 1):
                p.set_misfit_filter(ir, *(([c * 0.5 / dt for c in CORNERS], [0., 1., 1., 0.]) if filtered else ([], [])))
            filtered_now = filtered
        rows = basis[:ngroup * K]
        draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw - 1, np.random.default_rng(ndraw))])
        one = p.spectral_candidates_params("moment_tensor", rows[:K], K, cand[:1], outer_norm=NORM, spectra=True)      # (the kept bins)
        kept = int(np.sum(one.spectra_range[0, :, 1] - one.spectra_range[0, :, 0] + 1))
        new_call = lambda: p.spectral_candidates_bootstrap_params("moment_tensor", rows, K, cand, draws, outer_norm=NORM)   # noqa: E731

        def host_route():
            scan = p.spectral_candidates_params("moment_tensor", rows, K, cand, outer_norm=NORM, misfit=False, slot_misfit=True)
            parent_ms = p.spectral_candidates_ms()
            m = scan.slot_misfit.reshape(ngroup * ncand, nmis)
            n = np.repeat(scan.slot_norm, ncand, axis=0)
            bv, bi, _ = p.outer_misfits_slots(m, n, slot_receiver, nrec, outer_norm=NORM, draw_weights=draws)
            return bv, bi, parent_ms

        new_call()
        host_route()
        runs, host_runs, parent_kernel_ms = [], [], []
        for _ in range(reps):                                 # alternating: the two sides share the machine's moods
            t = time.perf_counter()
            boot = new_call()
            runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.spectral_candidates_bootstrap_ms()))))
            t = time.perf_counter()
            bv, bi, parent_ms = host_route()
            host_runs.append(time.perf_counter() - t)
            parent_kernel_ms.append(parent_ms[2])
        best = min(r["call_s"] for r in runs)
        hbest = min(host_runs)
        slot_s = min(r["slot_kernel_ms"] for r in runs) * 1e-3
        parent_s = min(parent_kernel_ms) * 1e-3
        pairs = ngroup * ncand * kept
        has = boot.best_cand >= 0
        flat = boot.best_group.astype(np.int64) * ncand + boot.best_cand
        hh = ~np.isnan(bv)
        same = bool(np.array_equal(boot.best_value, bv, equal_nan=True) and np.array_equal(has, hh) and np.array_equal(flat[hh], bi[hh]))
        row = dict(locations=ngroup, pass_band=filtered, ndraw=ndraw, runs=runs, best_call_s=best, kept_bins_per_location=kept,
                   transform_lengths=sorted(set(int(v) for v in one.spectra_range[0, :, 2])),
                   slot_misfit_bytes_of_the_host_route=ngroup * ncand * nmis * 4,
                   slot_kernel_workgroups=ngroup * nmis * ((ncand + C - 1) // C), speccand_kernel_workgroups=ngroup * ((ncand + C - 1) // C),
                   candidate_bin_pairs=pairs, pairs_per_s_of_the_slot_kernel=pairs / slot_s,
                   speccand_kernel_ms_in_the_host_route=parent_kernel_ms, pairs_per_s_of_speccand_kernel=pairs / parent_s,
                   slot_kernel_faster_per_pair_than_speccand_kernel=bool(slot_s < parent_s),
                   candidate_draws_per_s_of_the_bootstrap_kernels=ngroup * ncand * ndraw / (min(r["bootstrap_kernels_ms"] for r in runs) * 1e-3),
                   draws_with_a_winner=int(np.sum(has)), distinct_winners=len(set(flat[has].tolist())),
                   status_counts={str(k): int(np.sum(boot.status == k)) for k in (0, 1, 2)},
                   host_route_runs_s=host_runs, host_route_best_s=hbest, host_route_over_this_call=hbest / best,
                   best_equal_the_host_routes_bits=same)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        flush()
    p.close()
    gate_rows = [r for r in res["rows"] if r["locations"] == 16 and r["pass_band"] and r["ndraw"] == 100]
    res["gate_16_locations_pass_band_100_draws_faster_than_the_host_route"] = all(r["host_route_over_this_call"] > 1.0 for r in gate_rows)
    res["equality_at_size"] = all(r["best_equal_the_host_routes_bits"] for r in res["rows"])
    res["not_measured"] = ["several devices", "K other than 6", "ampspec_l1norm at this size", "hardware counters"]
    res["arithmetic"] = os.environ.get("KIWI_HIP_ARITH", "exact")
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    flush()
    if not res["equality_at_size"]:
        sys.exit("equality at size: a row's best_* differ from the host route's bits")
    if not res["gate_16_locations_pass_band_100_draws_faster_than_the_host_route"]:
        sys.exit("gate: the call at 16 locations with the pass band and 100 draws took longer than the host route")


if __name__ == "__main__":
    main()
