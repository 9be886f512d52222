"""What the linear fit costs on top of the evaluation of its basis sources: configuration 2's setup (`synthetic.workload('cfg2')`,
set up as bench.py does) with its 12 960 evaluations read as 2 160 trial locations x 6 elementary tensors, and configuration 4's (`mt_eikonal`) with the
six elementary tensors of a handful of grid locations.  Per case: the whole `linear_fit_params` call by the host clock; evaluation /
fit kernels / download by HIP events (kiwi_hip_get_linear_fit_ms); `misfits_for_params` of the same sources alone in the same
run (the fit's added cost is stated as a ratio to it); the Gram kernel's compulsory bytes (kept synthetics once + references,
from the shapes) over the fit kernels' time, beside kiwi_hip_measure_read_bandwidth of the same run; and what the same answer
takes without the call -- set_keep_synthetics(2), get_synthetics of every basis trace, numpy Gram and solve -- timed on a
subset of the groups and SCALED to all of them.

    python profiles/linfit_rate.py [out.json] [--commit=<id>]"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 4096
HOST_GROUPS = 4


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def host_path(p, rows, sourcetype, nrec, ngroups):
    """the answer without kiwi_hip_linear_fit: kept tapered synthetics down trace by trace, Gram matrix and solve in numpy"""
    K = 6
    p.set_keep_synthetics(2)
    p.set_source_params(sourcetype, rows[:ngroups * K])
    p.eval()
    ref = [p.get_reference(ir + 1, k + 1, 2, maxn=L + 64)[1].astype(np.float64) for ir in range(nrec) for k in range(3)]
    d = np.concatenate(ref)
    out = []
    for g in range(ngroups):
        A = np.stack([np.concatenate([p.get_synthetics(g * K + i, ir + 1, k + 1, 2, maxn=L + 64)[1].astype(np.float64)
                                      for ir in range(nrec) for k in range(3)]) for i in range(K)], 1)
        out.append(np.linalg.solve(A.T @ A, A.T @ d))
    p.set_keep_synthetics(0)
    return np.array(out)


def cfg2_locations(wl):
    """configuration 2's 12 960 evaluations spent on 2 160 trial locations (12 x 12 x 15 over north, east, depth) x 6 elementary
    tensors instead of 12 960 double couples at one location"""
    from kiwi_amd import mtfit
    base = np.array(wl["true"], np.float32)
    loc = np.array([[0., 400. * (a - 6), 400. * (b - 6), 8000. + 500. * c] for a in range(12) for b in range(12) for c in range(15)], np.float32)
    rows = np.tile(base, (len(loc), 1))
    rows[:, :4] = loc
    return mtfit.elementary_params("moment_tensor", rows)


def case(name, nsetup, rows_of, reps=3):
    import bench
    from kiwi_amd import synthetic
    wl = synthetic.workload(name, nsetup, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    rows = rows_of(wl)
    st, K = wl["sourcetype"], 6
    ngroup, nrec = len(rows) // K, wl["nrec"]
    res = dict(workload=wl["name"], sourcetype=st, groups=ngroup, K=K, sources=len(rows), receivers=nrec, window_samples=L)
    p.linear_fit_params(st, rows[:8 * K], K)                     # code objects, buffers
    fits, evals = [], []
    for _ in range(reps):
        t, fit = timed(lambda: p.linear_fit_params(st, rows, K))
        fits.append(dict(call_s=t, **dict(zip(("evaluation_ms", "fit_kernels_ms", "download_ms"), p.linear_fit_ms()))))
        evals.append(timed(lambda: p.misfits_for_params(st, rows))[0])
    best = min(fits, key=lambda r: r["call_s"])
    res["linear_fit_params"] = dict(best, runs_call_s=[r["call_s"] for r in fits])
    res["misfits_for_params_s"] = dict(best=min(evals), runs=evals)
    res["fit_over_evaluation_alone"] = best["call_s"] / min(evals)
    res["fit_kernels_over_evaluation_events"] = best["fit_kernels_ms"] / best["evaluation_ms"]
    res["status_counts"] = {str(k): int(np.sum(fit.status == k)) for k in (0, 1, 2)}
    res["pivot_min_range"] = [float(fit.pivot_min.min()), float(fit.pivot_min.max())]
    # the Gram kernel reads every kept trace once and the references once per group (the latter from cache in practice)
    wsum = 3 * nrec * L
    bytes_syn, bytes_ref = 4.0 * len(rows) * wsum, 4.0 * ngroup * wsum
    res["gram_compulsory_bytes"] = dict(kept_synthetics=bytes_syn, references=bytes_ref)
    res["gram_gbs_over_fit_kernels_time"] = (bytes_syn + bytes_ref) / (best["fit_kernels_ms"] * 1e-3) / 1e9
    gbs = ctypes.c_double(0.0)
    p._ck(p.L.kiwi_hip_measure_read_bandwidth(p.h, 4 << 30, 10, ctypes.byref(gbs)), "measure_read_bandwidth")
    res["pure_read_gbs_same_run"] = float(gbs.value)
    ng = min(HOST_GROUPS, ngroup)
    t, x = timed(lambda: host_path(p, rows, st, nrec, ng))
    ok = fit.status[:ng] == 0
    res["without_the_call"] = dict(groups_timed=ng, seconds=t, scaled_to_all_groups_s=t * ngroup / ng, label="SCALED from %d groups" % ng,
                                   max_rel_difference_of_coefficients=float(np.max(np.abs(x[ok] - fit.coef[:ng][ok]) / np.max(np.abs(x[ok]), 1, keepdims=True))) if ok.any() else None)
    res["without_over_with"] = res["without_the_call"]["scaled_to_all_groups_s"] / best["call_s"]
    p.close()
    print(name, json.dumps(res), flush=True)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    from kiwi_amd import mtfit, synthetic
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName))
    res["cfg2"] = case("cfg2", 512, cfg2_locations)
    res["cfg4"] = case("cfg4", 32, lambda wl: mtfit.elementary_params("mt_eikonal", wl["trials"][:8]))
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


if __name__ == "__main__":
    main()
