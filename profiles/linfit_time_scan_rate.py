"""What the linear fit's time scan costs against the path the library offered before it: configuration 2's setup
(`synthetic.workload('cfg2')`, set up as bench.py does) read as 2 160 trial locations x 6 elementary tensors x 50 receivers, and
configuration 4's (`mt_eikonal`) with the six elementary tensors of 8 grid locations, as profiles/linfit_rate.py has them.  Per shape
and nk in {1, 5, 21, 81} offsets one sample apart, centred on the sources' own time, in the same run on the same context:
  scan      the whole `linear_fit_time_scan_params` call by the host clock (warm-up, best of three) and its four HIP-event times
            (kiwi_hip_get_linear_fit_time_scan_ms: evaluation, Gram-scan kernel, solve kernels, downloads) of the best run
  separate  nk `linear_fit_params` calls with the times moved by k dt (best of three of the sum) and their summed event times
nk = 1 stands beside one plain `linear_fit_params` call.  The gate: the scan at nk = 5 takes less time than the five separate calls.

    python profiles/linfit_time_scan_rate.py [out.json] [--commit=<id>]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.linfit_rate import L, cfg2_locations, timed  # noqa: E402

NKS = (1, 5, 21, 81)
REPS = 3


def case(name, nsetup, rows_of):
    import bench
    from kiwi_amd import synthetic
    wl = synthetic.workload(name, nsetup, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    rows = rows_of(wl)
    st, K, dt = wl["sourcetype"], 6, gf["dt"]
    ngroup = len(rows) // K
    res = dict(workload=wl["name"], sourcetype=st, groups=ngroup, K=K, sources=len(rows), receivers=wl["nrec"], window_samples=L,
               offsets_per_pass=p.linear_fit_time_scan_shape(K)[0], tile_samples=p.linear_fit_time_scan_shape(K)[1], by_nk={})
    p.linear_fit_params(st, rows[:8 * K], K)                     # code objects, buffers
    p.linear_fit_time_scan_params(st, rows[:8 * K], K, -1, 1, 3)
    for nk in NKS:
        k0 = -(nk // 2)
        scans, seps = [], []
        for _ in range(REPS):
            t, fit = timed(lambda: p.linear_fit_time_scan_params(st, rows, K, k0, 1, nk))
            scans.append(dict(call_s=t, **dict(zip(("evaluation_ms", "gram_scan_ms", "solve_ms", "download_ms"), p.linear_fit_time_scan_ms()))))
        for _ in range(REPS):
            tot, ev, worst = 0.0, np.zeros(3), 0.0
            for j in range(nk):
                moved = rows.copy()
                moved[:, 0] += np.float32((k0 + j) * dt)
                t, one = timed(lambda: p.linear_fit_params(st, moved, K))
                tot += t
                ev += np.array(p.linear_fit_ms())
                ok = (one.status == 0) & (fit.status[:, j] == 0)
                if ok.any():
                    worst = max(worst, float(np.max(np.abs(one.misfit[ok] - fit.misfit[:, j][ok]))))
            seps.append(dict(calls_s=tot, evaluation_ms=float(ev[0]), fit_kernels_ms=float(ev[1]), download_ms=float(ev[2]),
                             max_abs_misfit_difference_to_scan=worst))
        bs, bp = min(scans, key=lambda r: r["call_s"]), min(seps, key=lambda r: r["calls_s"])
        res["by_nk"][str(nk)] = dict(k0=k0, scan=dict(bs, runs_call_s=[r["call_s"] for r in scans]),
                                     separate_calls=dict(bp, runs_calls_s=[r["calls_s"] for r in seps]),
                                     separate_over_scan=bp["calls_s"] / bs["call_s"],
                                     scan_status_counts={str(k): int(np.sum(fit.status == k)) for k in (0, 1, 2)})
        print(name, nk, json.dumps(res["by_nk"][str(nk)]), flush=True)
    g = res["by_nk"]["5"]
    res["gate_scan_at_nk5_faster_than_five_calls"] = bool(g["scan"]["call_s"] < g["separate_calls"]["calls_s"])
    p.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    from kiwi_amd import mtfit
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName))
    res["cfg2"] = case("cfg2", 512, cfg2_locations)
    res["cfg4"] = case("cfg4", 32, lambda wl: mtfit.elementary_params("mt_eikonal", wl["trials"][:8]))
    res["not_measured"] = "several devices, the entry point for an uploaded batch (kiwi_hip_linear_fit_time_scan), kstep > 1, counters of the Gram-scan kernel"
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                    stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    print(json.dumps(res))
    if args:
        with open(args[0], "w") as fh:
            json.dump(res, fh, indent=1)
    ok = res["cfg2"]["gate_scan_at_nk5_faster_than_five_calls"] and res["cfg4"]["gate_scan_at_nk5_faster_than_five_calls"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
