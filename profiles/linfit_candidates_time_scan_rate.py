"""What a mechanism grid at nk origin times costs through kiwi_hip_linear_fit_candidates_time_scan, on configuration 2's set-up as
bench.py makes it (50 receivers x 3 components x 4096 samples): K = 6 elementary tensors per trial location, the 36 x 10 x 36 =
12 960 double couples at 10 degrees as candidates, 16 locations, nk = 5 and 21 origin times one sample apart, under the outer
l1norm, the outer l2norm and the outer l2norm with a free moment per mechanism (free_scale).  Per case: the whole
`linear_fit_candidates_time_scan_params` call by the host clock, best of `reps` after a warm-up, every run listed, with the five
HIP-event times (evaluation, Gram-scan kernel, solve kernels, candidate-scan kernels, downloads;
kiwi_hip_get_linear_fit_candidates_time_scan_ms).  The call returns the best mechanism per (location, origin time) and the
mechanism cube with the origin time profiled out (cand_misfit, cand_offset), not the full [16, nk, 12 960] array.

The yardstick is what the library offered before: the nk separate `linear_fit_candidates_params` calls with the basis sources'
times moved by k dt (each returning its full misfit array [16, 12 960], which the caller needs to profile the time out himself), on
the same context in the same run.  The gate: at nk = 21 the scan call takes less time than those separate calls, in every case.
The ratio itself is reported, not promised.  `--bench-before=<files>` / `--bench-after=<files>` (comma-separated): the outputs of
bench.py's default line run from a checkout of the parent commit and from this one in the same session, alternating, copied into
the result with the ratio of the means and the spread of either side.

    python profiles/linfit_candidates_time_scan_rate.py [out.json] [--commit=<id>] [--reps=3]"""
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
CASES = (("l1norm", False), ("l2norm", False), ("l2norm", True))
EVENTS = ("evaluation_ms", "gram_scan_kernel_ms", "solve_kernels_ms", "candidate_scan_kernels_ms", "download_ms")


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
    dt = float(gf["dt"])
    rows = cfg2_locations(wl)[:NGROUP * K]
    unit_dc, _ = mtfit.double_couple_candidates(*GRID)
    ncand = len(unit_dc)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), workload=wl["name"],
               K=K, candidates=ncand, locations=NGROUP, receivers=wl["nrec"], window_samples=L, reps=reps,
               candidates_per_workgroup=p.linear_fit_candidates_time_scan_shape(K)[0],
               receivers_per_stage=p.linear_fit_candidates_time_scan_shape(K)[1], by_nk={})

    def flush():
        if args:
            with open(args[0], "w") as fh:
                json.dump(res, fh, indent=1)

    for nk in (5, 21):
        k0 = -(nk // 2)
        entry = dict(offsets=[k0, 1, nk], syntheses_of_the_scan=NGROUP * K, syntheses_of_the_separate_calls=NGROUP * K * nk,
                     mechanism_time_nodes=NGROUP * nk * ncand)
        for norm, free in CASES:
            cand = unit_dc if free else unit_dc * (MOMENT / UNIT)
            kw = dict(outer_norm=norm, free_scale=free)
            scan_call = lambda: p.linear_fit_candidates_time_scan_params("moment_tensor", rows, K, cand, k0, 1, nk, marginal=True, **kw)   # noqa: E731

            def separate():
                out = []
                for j in range(nk):
                    moved = rows.copy()
                    moved[:, 0] += np.float32((k0 + j) * dt)
                    out.append(p.linear_fit_candidates_params("moment_tensor", moved, K, cand, misfit=True, **kw))
                return out

            scan_call()
            separate()
            runs, sep_runs = [], []
            for _ in range(reps):                             # alternating: the two sides share the machine's moods
                t = time.perf_counter()
                scan = scan_call()
                runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(EVENTS, p.linear_fit_candidates_time_scan_ms()))))
                t = time.perf_counter()
                sep = separate()
                sep_runs.append(time.perf_counter() - t)
            best, ybest = min(r["call_s"] for r in runs), min(sep_runs)
            sep_best = np.stack([s.best_misfit for s in sep], 1)
            entry[norm + ("_free_scale" if free else "")] = dict(
                runs=runs, best_call_s=best, mechanism_time_nodes_per_s=NGROUP * nk * ncand / best,
                separate_calls_runs_s=sep_runs, separate_calls_best_s=ybest, separate_calls_over_this_call=ybest / best,
                status_counts={str(k): int(np.sum(scan.status == k)) for k in (0, 1, 2)},
                best_misfit_range=[float(np.nanmin(scan.best_misfit)), float(np.nanmax(scan.best_misfit))],
                largest_difference_of_the_best_misfits_against_the_separate_calls=float(np.nanmax(np.abs(scan.best_misfit - sep_best))))
        res["by_nk"][str(nk)] = entry
        print(nk, json.dumps(entry), flush=True)
        flush()
    p.close()
    e21 = res["by_nk"]["21"]
    res["gate_nk_21_faster_than_the_separate_calls"] = all(e21[n + ("_free_scale" if f else "")]["separate_calls_over_this_call"] > 1.0
                                                           for n, f in CASES)
    res["not_timed"] = ["several devices", "K other than 6", "receiver_misfit at size", "hardware counters of the candidate-scan kernel"]
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
    print(json.dumps(res))
    flush()
    if not res["gate_nk_21_faster_than_the_separate_calls"]:
        sys.exit("gate: a scan call at nk = 21 took longer than the 21 separate linear_fit_candidates_params calls")


if __name__ == "__main__":
    main()
