"""What the joint bootstrap of a mechanism grid costs through kiwi_hip_linear_fit_candidates_bootstrap, on configuration 2's set-up
as bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 =
12 960 double couples at 10 degrees as candidates, 16 locations, nk = 1 and nk = 5 origin times one sample apart, 100 and 1000
draws (draw 0 of ones, the others resampling counts), under the outer l1norm and the outer l2norm.  Per row: the whole
`linear_fit_candidates_bootstrap_params` call by the host clock, best of `reps` after a warm-up, every run listed, with the five
HIP-event times (evaluation, Gram-scan kernel, solve kernels, bootstrap kernels, downloads;
kiwi_hip_get_linear_fit_candidates_bootstrap_ms).

The yardstick is what the library offered before, on the same context in the same run: `linear_fit_candidates_params(...,
receiver_misfit=True)` (nk = 1) or `linear_fit_candidates_time_scan_params(..., receiver_misfit=True)` (nk = 5), which downloads
receiver_misfit [16, nk, 12 960, 50], then `Engine.outer_misfits` on it, which uploads it again.  The gate: at nk = 1 with 1000
draws the new call takes less time than that route, under both norms.  The ratio of every row is reported, not promised.  In the
same run best_value, best_group, best_offset and best_cand of every row are compared with the host route's bits.
`--bench-before=<files>` / `--bench-after=<files>` (comma-separated): the outputs of bench.py's default line run from a checkout of
the parent commit and from this one in the same session, alternating, copied into the result.

    python profiles/linfit_candidates_bootstrap_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
EVENTS = ("evaluation_ms", "gram_scan_kernel_ms", "solve_kernels_ms", "bootstrap_kernels_ms", "download_ms")


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
    p.set_misfit_method("l2norm")
    nrec = wl["nrec"]
    rows = cfg2_locations(wl)[:NGROUP * K]
    cand = mtfit.double_couple_candidates(*GRID)[0] * (MOMENT / UNIT)
    ncand = len(cand)
    C, T, Rmax = p.linear_fit_candidates_bootstrap_shape(K)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, locations=NGROUP, receivers=nrec, window_samples=L, reps=reps, candidates_per_workgroup=C,
               draws_per_tile=T, max_receivers=Rmax, rows=[])

    def flush():
        if args:
            with open(args[0], "w") as fh:
                json.dump(res, fh, indent=1)

    for nk in (1, 5):
        k0 = -(nk // 2)
        for ndraw in (100, 1000):
            draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw - 1, np.random.default_rng(ndraw))])
            for norm in ("l1norm", "l2norm"):
                new_call = lambda: p.linear_fit_candidates_bootstrap_params("moment_tensor", rows, K, cand, draws, k0, 1, nk, outer_norm=norm)   # noqa: E731

                def host_route():
                    if nk == 1:
                        scan = p.linear_fit_candidates_params("moment_tensor", rows, K, cand, outer_norm=norm, receiver_misfit=True)
                    else:
                        scan = p.linear_fit_candidates_time_scan_params("moment_tensor", rows, K, cand, k0, 1, nk, outer_norm=norm, marginal=False,
                                                                        receiver_misfit=True)
                    m = scan.receiver_misfit.reshape(NGROUP * nk * ncand, nrec, 1)
                    n = np.repeat(scan.receiver_norm, nk * ncand, axis=0)[:, :, None]
                    bv, bi, _ = p.outer_misfits(m, n, outer_norm=norm, draw_weights=draws, ncomponents=[1] * nrec)
                    return bv, bi

                new_call()
                host_route()
                runs, host_runs = [], []
                for _ in range(reps):                         # alternating: the two sides share the machine's moods
                    t = time.perf_counter()
                    boot = new_call()
                    runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.linear_fit_candidates_bootstrap_ms()))))
                    t = time.perf_counter()
                    bv, bi = host_route()
                    host_runs.append(time.perf_counter() - t)
                best, hbest = min(r["call_s"] for r in runs), min(host_runs)
                has = ~np.isnan(bv)
                flat = (boot.best_group.astype(np.int64) * nk + boot.best_offset) * ncand + boot.best_cand
                same = bool(np.array_equal(boot.best_value, bv, equal_nan=True) and np.array_equal(flat[has], bi[has]) and
                            np.all(boot.best_cand[~has] == -1))
                row = dict(nk=nk, offsets=[k0, 1, nk], ndraw=ndraw, outer_norm=norm, runs=runs, best_call_s=best, host_route_runs_s=host_runs,
                           host_route_best_s=hbest, host_route_over_this_call=hbest / best,
                           receiver_misfit_bytes_of_the_host_route=NGROUP * nk * ncand * nrec * 4,
                           candidate_draws_per_s=NGROUP * nk * ncand * ndraw / best, best_equal_the_host_routes_bits=same,
                           draws_with_a_winner=int(np.sum(has)), distinct_winners=len(set(flat[has].tolist())),
                           status_counts={str(k): int(np.sum(boot.status == k)) for k in (0, 1, 2)})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                flush()
    p.close()
    gate_rows = [r for r in res["rows"] if r["nk"] == 1 and r["ndraw"] == 1000]
    res["gate_nk_1_ndraw_1000_faster_than_the_host_route"] = all(r["host_route_over_this_call"] > 1.0 for r in gate_rows)
    res["equality_at_size"] = all(r["best_equal_the_host_routes_bits"] for r in res["rows"])
    res["not_measured"] = ["several devices", "K other than 6", "hardware counters of the bootstrap kernel", "what bounds phase 2 of the bootstrap kernel"]
    res["arithmetic"] = os.environ.get("KIWI_HIP_ARITH", "exact")
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    if "bench-before" in opt and "bench-after" in opt:       # files (comma-separated) whose last line is bench.py's JSON result line
        def lines(names):
            out = []
            for fn in names.split(","):
                with open(fn) as fh:
                    b = json.loads([ln for ln in fh.read().splitlines() if ln.strip().startswith("{")][-1])
                out.append({k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup")})
            return out
        a, b = lines(opt["bench-before"]), lines(opt["bench-after"])
        va, vb = [x["value"] for x in a], [x["value"] for x in b]
        res["bench_default_line"] = dict(how="bench.py --gpus 1 --steps 30 --warmup 5 in one session, in the order parent, this build, parent, "
                                             "this build; the parent is a checkout of the parent commit with its own library",
                                         parent_library=a, this_library=b, this_over_parent=(sum(vb) / len(vb)) / (sum(va) / len(va)),
                                         parent_spread=max(va) - min(va), this_spread=max(vb) - min(vb))
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    flush()
    if not res["equality_at_size"]:
        sys.exit("equality at size: a row's best_* differ from the host route's bits")
    if not res["gate_nk_1_ndraw_1000_faster_than_the_host_route"]:
        sys.exit("gate: the call at nk = 1 with 1000 draws took longer than the host route")


if __name__ == "__main__":
    main()
