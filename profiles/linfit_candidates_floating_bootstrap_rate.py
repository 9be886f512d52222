"""What the joint bootstrap of a mechanism grid with per-receiver shifts costs through kiwi_hip_linear_fit_candidates_floating_bootstrap,
on configuration 2's set-up as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial
location, the 36 x 10 x 36 = 12 960 double couples at 10 degrees as candidates, 16 locations, shift ranges of 5 and of 21 samples on
all receivers, 100 and 1000 draws (draw 0 of ones, the others resampling counts), under the outer l1norm and the outer l2norm.  Per
row: the whole `linear_fit_candidates_floating_bootstrap_params` call by the host clock, best of `reps` after a warm-up, every run
listed, with the four HIP-event times (evaluation, Gram and cross-correlation kernels, bootstrap kernels, downloads;
kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms) and the (candidate, draw) pairs per second of the bootstrap kernels.

The yardstick is what the library offered before, on the same context in the same run: `linear_fit_candidates_floating_params(...,
cand_shift=True, receiver_misfit=True)`, which downloads receiver_misfit and cand_shift [16, 12 960, 50], then `Engine.outer_misfits`
on the first, which uploads it again, and the winner's row of the second.  The gate: with 21 shifts and 1000 draws the new call takes
less time than that route, under both norms.  The ratio of every row is reported, not promised.  In the same run best_value,
best_group, best_cand and best_shift of every row are compared with the host route's bits.

    python profiles/linfit_candidates_floating_bootstrap_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
EVENTS = ("evaluation_ms", "gram_xcorr_kernels_ms", "bootstrap_kernels_ms", "download_ms")
GRAM_SIBLING_PAIRS_PER_S = 3.3e10                             # profiles/linfit_candidates_bootstrap_rate.json: a comparison, not a threshold


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    reps = int(opt.get("reps", 3))
    out_file = args[0] if args else os.path.join(ROOT, "profiles", "linfit_candidates_floating_bootstrap_rate.json")
    import torch
    import bench
    from kiwi_amd import mtfit, synthetic
    from kiwi_amd.engine import bootstrap_draw_weights
    from linfit_rate import cfg2_locations
    wl = synthetic.workload("cfg2", 512, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    dt = gf["dt"]
    nrec = wl["nrec"]
    rows = cfg2_locations(wl)[:NGROUP * K]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    C, T, Rmax = p.linear_fit_candidates_floating_bootstrap_shape(K)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, locations=NGROUP, receivers=nrec, window_samples=L, reps=reps, candidates_per_workgroup=C,
               draws_per_tile=T, max_receivers=Rmax, gram_sibling_candidate_draws_per_s=GRAM_SIBLING_PAIRS_PER_S, rows=[])

    def flush():
        with open(out_file, "w") as fh:
            json.dump(res, fh, indent=1)

    p.set_misfit_method("floating_l2norm")
    for half in (2, 10):
        ns = 2 * half + 1
        p.set_floating_shiftrange(0, -half * dt, half * dt)
        for ndraw in (100, 1000):
            draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw - 1, np.random.default_rng(ndraw))])
            for norm in ("l1norm", "l2norm"):
                new_call = lambda: p.linear_fit_candidates_floating_bootstrap_params("moment_tensor", rows, K, cand, draws, outer_norm=norm)   # noqa: E731

                def host_route():
                    scan = p.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, outer_norm=norm, misfit=True, cand_shift=True,
                                                                   receiver_misfit=True)
                    m = scan.receiver_misfit.reshape(NGROUP * ncand, nrec, 1)
                    n = np.repeat(scan.receiver_norm, ncand, axis=0)[:, :, None]
                    bv, bi, _ = p.outer_misfits(m, n, outer_norm=norm, draw_weights=draws, ncomponents=[1] * nrec)
                    has = ~np.isnan(bv)
                    bs = np.where(has[:, None], scan.cand_shift.reshape(NGROUP * ncand, nrec)[np.where(has, bi, 0)].astype(np.int32), 0)
                    return bv, bi, bs

                new_call()
                host_route()
                runs, host_runs = [], []
                for _ in range(reps):                         # alternating: the two sides share the machine's moods
                    t = time.perf_counter()
                    boot = new_call()
                    runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.linear_fit_candidates_floating_bootstrap_ms()))))
                    t = time.perf_counter()
                    bv, bi, bs = host_route()
                    host_runs.append(time.perf_counter() - t)
                best, hbest = min(r["call_s"] for r in runs), min(host_runs)
                kernel_s = 1e-3 * min(r["bootstrap_kernels_ms"] for r in runs)
                has = ~np.isnan(bv)
                flat = boot.best_group.astype(np.int64) * ncand + boot.best_cand
                same = bool(np.array_equal(boot.best_value, bv, equal_nan=True) and np.array_equal(flat[has], bi[has]) and
                            np.all(boot.best_cand[~has] == -1) and np.array_equal(boot.best_shift, bs))
                row = dict(shifts=ns, ndraw=ndraw, outer_norm=norm, runs=runs, best_call_s=best, host_route_runs_s=host_runs,
                           host_route_best_s=hbest, host_route_over_this_call=hbest / best,
                           receiver_misfit_bytes_of_the_host_route=NGROUP * ncand * nrec * 4,
                           cand_shift_bytes_of_the_host_route=NGROUP * ncand * nrec * 2,
                           candidate_draws_per_s_of_the_bootstrap_kernels=NGROUP * ncand * ndraw / kernel_s,
                           candidate_draws_per_s_of_the_call=NGROUP * ncand * ndraw / best, best_and_shifts_equal_the_host_routes_bits=same,
                           draws_with_a_winner=int(np.sum(has)), distinct_winners=len(set(flat[has].tolist())),
                           distinct_shift_rows=len(set(map(tuple, boot.best_shift[has].tolist()))),
                           status_counts={str(k): int(np.sum(boot.status == k)) for k in (0, 1, 2)})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                flush()
    p.close()
    gate_rows = [r for r in res["rows"] if r["shifts"] == 21 and r["ndraw"] == 1000]
    res["gate_21_shifts_1000_draws_faster_than_the_host_route"] = all(r["host_route_over_this_call"] > 1.0 for r in gate_rows)
    res["equality_at_size"] = all(r["best_and_shifts_equal_the_host_routes_bits"] for r in res["rows"])
    res["not_measured"] = ["several devices", "K other than 6", "group_shift at size", "hardware counters"]
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
        sys.exit("equality at size: a row's best_* or best_shift differ from the host route's bits")
    if not res["gate_21_shifts_1000_draws_faster_than_the_host_route"]:
        sys.exit("gate: the call with 21 shifts and 1000 draws took longer than the host route")


if __name__ == "__main__":
    main()
