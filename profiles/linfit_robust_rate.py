"""What the robust linear fit (kiwi_hip_linear_fit_robust) costs, on the shapes of profiles/linfit_rate.py: configuration 2 read as
2 160 trial locations x 6 elementary tensors, configuration 4 (`mt_eikonal`) as 8 x 6.  Per case and mode -- A: misfit method
l1norm, B: l2norm; outer norm l1norm, niter = 8, eps = 1e-3 --: the whole `linear_fit_robust_params` call by the host clock, the
four HIP-event times (evaluation, l2 start, reweighting passes, download; kiwi_hip_get_linear_fit_robust_ms), and the time per
reweighting pass (mode A: niter + 1 sample passes with their fold-and-solve launches; mode B: one launch of niter + 1 iterations
on the per-receiver normal equations), beside the fit kernels (Gram + solve) of `linear_fit_params` on the same inputs in the same
session -- of this build and, with --parent-lib=<libkiwi_hip.so of the parent commit>, of that library in a child process of its
own, alternating with this build's.  One warm-up call per shape and mode, then `reps` timed calls; every run is listed, the
best is quoted.  The restatement's gap to the linear program's optimum (tests/test_linfit_robust.py gates on it) is measured
on the host and written alongside.

    python profiles/linfit_robust_rate.py [out.json] [--commit=<id>] [--parent-lib=<path>]"""
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
NITER, EPS = 8, 1e-3
METHOD = {"A": "l1norm", "B": "l2norm"}


def setup(name, nsetup):
    import bench
    from kiwi_amd import mtfit, synthetic
    from linfit_rate import cfg2_locations
    wl = synthetic.workload(name, nsetup, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    rows = cfg2_locations(wl) if name == "cfg2" else mtfit.elementary_params("mt_eikonal", wl["trials"][:8])
    return wl, p, rows


CASES = (("cfg2", 512), ("cfg4", 32))


def l2_fit_kernels(reps=3):
    """fit kernels (Gram + solve) [ms] of linear_fit_params per case, of whatever library KIWI_HIP_LIB names: warm-up + reps"""
    out = {}
    for name, nsetup in CASES:
        wl, p, rows = setup(name, nsetup)
        p.linear_fit_params(wl["sourcetype"], rows, 6)
        runs = []
        for _ in range(reps):
            p.linear_fit_params(wl["sourcetype"], rows, 6)
            runs.append(p.linear_fit_ms()[1])
        p.close()
        out[name] = runs
    return out


def l2_fit_kernels_of(lib):
    """the same in a child process that loads `lib`"""
    env = dict(os.environ, KIWI_HIP_LIB=lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--l2-only"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("child with %s failed: %s" % (lib, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def case(name, nsetup, reps=3):
    wl, p, rows = setup(name, nsetup)
    st, K = wl["sourcetype"], 6
    ngroup, nrec = len(rows) // K, wl["nrec"]
    res = dict(workload=wl["name"], sourcetype=st, groups=ngroup, K=K, sources=len(rows), receivers=nrec, window_samples=L, niter=NITER, eps=EPS)
    p.set_misfit_method("l2norm")
    p.linear_fit_params(st, rows, K)
    l2 = []
    for _ in range(reps):
        t = time.perf_counter()
        p.linear_fit_params(st, rows, K)
        l2.append(dict(call_s=time.perf_counter() - t, **dict(zip(("evaluation_ms", "fit_kernels_ms", "download_ms"), p.linear_fit_ms()))))
    res["linear_fit_params_l2"] = l2
    gram_ms = min(r["fit_kernels_ms"] for r in l2)
    for mode in ("A", "B"):
        p.set_misfit_method(METHOD[mode])
        p.linear_fit_robust_params(st, rows, K, niter=NITER, eps=EPS)
        runs = []
        for _ in range(reps):
            t = time.perf_counter()
            fit = p.linear_fit_robust_params(st, rows, K, niter=NITER, eps=EPS)
            runs.append(dict(call_s=time.perf_counter() - t,
                             **dict(zip(("evaluation_ms", "l2_start_ms", "reweighting_ms", "download_ms"), p.linear_fit_robust_ms()))))
        best = min(runs, key=lambda r: r["reweighting_ms"])
        per_pass = best["reweighting_ms"] / (NITER + 1)
        res["mode_" + mode] = dict(runs=runs, best=best, reweighting_ms_per_pass=per_pass, passes=NITER + 1,
                                   pass_over_fit_kernels_of_this_build=per_pass / gram_ms,
                                   status_counts={str(k): int(np.sum(fit.status == k)) for k in (0, 1, 2, 3)},
                                   misfit_l2_start_to_final=[float(np.nanmean(fit.trace[:, 0, 1])), float(np.nanmean(fit.misfit))])
    p.close()
    print(name, json.dumps(res), flush=True)
    return res


def restatement_gap():
    from tests import linfit_robust_restatement as rr
    from tests import test_linfit_robust as t
    syn, ref, receivers, planted = t.outlier_case()
    out = rr.fit(syn, ref, receivers, t.DT, "A", None, False, NITER, EPS)
    x, opt = t.lp_optimum(t.l1_problem(syn, ref, receivers, t.DT))
    return dict(case="tests/test_linfit_robust.py outlier_case: K = 6, 7 receivers x 100 samples, one receiver in noise 20 x its signal, one spike burst",
                eps=EPS, niter=NITER, relative_gap=float(out["misfit"][0] / opt - 1.0))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "--l2-only" in sys.argv[1:]:
        print(json.dumps(l2_fit_kernels()))
        return
    if "--gap-only" in sys.argv[1:]:
        print(json.dumps(restatement_gap()))
        return
    import torch
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName))
    res["restatement_gap_to_lp_optimum"] = restatement_gap()
    for name, nsetup in CASES:
        res[name] = case(name, nsetup)
    if "parent-lib" in opt:
        from kiwi_amd import lib as klib
        ab = dict(parent=[], this_build=[])
        for _ in range(2):                                   # alternating, each in a process of its own
            ab["parent"].append(l2_fit_kernels_of(os.path.abspath(opt["parent-lib"])))
            ab["this_build"].append(l2_fit_kernels_of(klib.LIB_PATH))
        res["fit_kernels_ms_parent_against_this_build"] = ab
        for name, _ in CASES:
            parent = min(v for run in ab["parent"] for v in run[name])
            res[name]["parent_fit_kernels_ms"] = parent
            res[name]["mode_A"]["pass_over_parent_fit_kernels"] = res[name]["mode_A"]["reweighting_ms_per_pass"] / parent
            res[name]["mode_B"]["pass_over_parent_fit_kernels"] = res[name]["mode_B"]["reweighting_ms_per_pass"] / parent
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
