"""What the joint bootstrap of a mechanism grid under l1norm inside and outside costs through kiwi_hip_waveform_candidates_bootstrap,
on configuration 2's set-up as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial
location, the 36 x 10 x 36 = 12 960 double couples at 10 degrees as candidates, 16 locations, nk = 1 and nk = 5 origin times one
sample apart, 100 and 1000 draws (draw 0 of ones, the others resampling counts).  Per row: the whole
`waveform_candidates_bootstrap_params` call by the host clock, best of `reps` after a warm-up, every run listed, with the five
HIP-event times (evaluation, rows + scan kernels, fold kernels, bootstrap kernels, downloads;
kiwi_hip_get_waveform_candidates_bootstrap_ms).

The yardstick is what the library offered before, on the same context in the same run:
`waveform_candidates_time_scan_params(..., slot_misfit=True)`, which downloads slot_misfit [16, nk, 12 960, 150], then
`Engine.outer_misfits_slots` on it, which uploads it again.  The gate: at nk = 5 with 100 draws the new call takes less time than
that route.  The ratio of every row is reported, not promised.  In the same run best_value, best_group, best_offset and best_cand of
every row are compared with the host route's bits.  At nk = 21 the yardstick's array is 2.6 GB each way: the new call is timed alone
there.

    python profiles/waveform_candidates_bootstrap_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
NGROUP = 16
GRID = (range(0, 360, 10), range(0, 91, 10), range(-180, 180, 10))
MOMENT, UNIT = 7e18, 1e18
EVENTS = ("evaluation_ms", "scan_kernels_ms", "fold_kernels_ms", "bootstrap_kernels_ms", "download_ms")
NORM = "l1norm"                                               # inside and outside
GRAM_SIBLING_PAIRS_PER_S = 3.3e10                            # profiles/linfit_candidates_bootstrap_rate.json, the bootstrap kernels alone


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
    p.set_misfit_method(NORM)
    nrec = wl["nrec"]
    rows = cfg2_locations(wl)[:NGROUP * K]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    slot_receiver = np.repeat(np.arange(nrec, dtype=np.int32), [len(c) for c in p.components])
    nmis = len(slot_receiver)
    C, T, Rmax = p.waveform_candidates_bootstrap_shape(K)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, locations=NGROUP, receivers=nrec, slots=nmis, window_samples=L, inner_norm=NORM, outer_norm=NORM,
               reps=reps, candidates_per_workgroup=C, draws_per_tile=T, max_receivers=Rmax, rows=[])

    def flush():
        if args:
            with open(args[0], "w") as fh:
                json.dump(res, fh, indent=1)

    for nk in (1, 5, 21):
        k0 = -(nk // 2)
        for ndraw in (100, 1000):
            draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw - 1, np.random.default_rng(ndraw))])
            new_call = lambda: p.waveform_candidates_bootstrap_params("moment_tensor", rows, K, cand, draws, k0, 1, nk, outer_norm=NORM)   # noqa: E731

            def host_route():
                scan = p.waveform_candidates_time_scan_params("moment_tensor", rows, K, k0, 1, nk, cand, outer_norm=NORM, cand_misfit=False,
                                                              cand_offset=False, slot_misfit=True)
                m = scan.slot_misfit.reshape(NGROUP * nk * ncand, nmis)
                n = np.repeat(scan.slot_norm, nk * ncand, axis=0)
                bv, bi, _ = p.outer_misfits_slots(m, n, slot_receiver, nrec, outer_norm=NORM, draw_weights=draws)
                return bv, bi

            with_host = nk != 21                              # (2.6 GB each way: the new call alone)
            new_call()
            if with_host:
                host_route()
            runs, host_runs = [], []
            for _ in range(reps):                             # alternating: the two sides share the machine's moods
                t = time.perf_counter()
                boot = new_call()
                runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.waveform_candidates_bootstrap_ms()))))
                if with_host:
                    t = time.perf_counter()
                    bv, bi = host_route()
                    host_runs.append(time.perf_counter() - t)
            best = min(r["call_s"] for r in runs)
            kernel_s = min(r["bootstrap_kernels_ms"] for r in runs) * 1e-3
            has = boot.best_cand >= 0
            flat = (boot.best_group.astype(np.int64) * nk + boot.best_offset) * ncand + boot.best_cand
            row = dict(nk=nk, offsets=[k0, 1, nk], ndraw=ndraw, runs=runs, best_call_s=best,
                       slot_misfit_bytes_of_the_host_route=NGROUP * nk * ncand * nmis * 4,
                       candidate_draws_per_s_of_the_call=NGROUP * nk * ncand * ndraw / best,
                       candidate_draws_per_s_of_the_bootstrap_kernels=NGROUP * nk * ncand * ndraw / kernel_s,
                       gram_sibling_candidate_draws_per_s_of_its_bootstrap_kernels=GRAM_SIBLING_PAIRS_PER_S,
                       draws_with_a_winner=int(np.sum(has)), distinct_winners=len(set(flat[has].tolist())),
                       status_counts={str(k): int(np.sum(boot.status == k)) for k in (0, 1, 2)})
            if with_host:
                hbest = min(host_runs)
                hh = ~np.isnan(bv)
                same = bool(np.array_equal(boot.best_value, bv, equal_nan=True) and np.array_equal(has, hh) and np.array_equal(flat[hh], bi[hh]))
                row.update(host_route_runs_s=host_runs, host_route_best_s=hbest, host_route_over_this_call=hbest / best,
                           best_equal_the_host_routes_bits=same)
            else:
                row.update(host_route="not run: its slot_misfit array is %.1f GB each way" % (NGROUP * nk * ncand * nmis * 4 / 1e9))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            flush()
    p.close()
    gate_rows = [r for r in res["rows"] if r["nk"] == 5 and r["ndraw"] == 100]
    res["gate_nk_5_ndraw_100_faster_than_the_host_route"] = all(r["host_route_over_this_call"] > 1.0 for r in gate_rows)
    res["equality_at_size"] = all(r["best_equal_the_host_routes_bits"] for r in res["rows"] if "best_equal_the_host_routes_bits" in r)
    res["not_measured"] = ["several devices", "K other than 6", "l2norm inside or outside at this size", "hardware counters of the bootstrap kernel",
                           "what bounds the bootstrap kernel (its slot sums read the slab once per draw pass, the Gram sibling's phase 1 reads rows of sums)"]
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
    if not res["gate_nk_5_ndraw_100_faster_than_the_host_route"]:
        sys.exit("gate: the call at nk = 5 with 100 draws took longer than the host route")


if __name__ == "__main__":
    main()
