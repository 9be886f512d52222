"""What the wide linear fit (kiwi_hip_linear_fit_wide) costs at its largest size: K = 64 basis sources per group (a 4 x 4 fault,
two rake directions, two time windows: kiwi_amd/slipfit.py), 16 groups (fault orientations) x 50 receivers x 3 components x
4096 samples, on the setup of configuration 2.  Per mode -- free coefficients, and non-negative coefficients with a relative
Laplacian penalty --: the whole `linear_fit_wide_params` call by the host clock and the HIP-event times (evaluation, Gram and
solve kernels, download; kiwi_hip_get_linear_fit_ms) with the Gram kernels and the solve kernel apart
(kiwi_hip_get_linear_fit_wide_ms).  Beside them: the Gram's compulsory bytes (every kept trace and the references once, from the
shapes) over the Gram kernels' time and kiwi_hip_measure_read_bandwidth of the same run, and the same non-negative fit WITHOUT
the call -- kept synthetics down trace by trace, scipy.optimize.nnls on the stacked traces with the penalty as extra rows --
timed on one group and SCALED to all.  One warm-up call, then `reps` timed calls; every run is listed, the best is quoted.  Last:
the figures of examples/invert_slip.py that the documents quote.

    python profiles/linfit_wide_rate.py [out.json] [--commit=<id>]"""
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
NX, NY, NRAKE, NWIN = 4, 4, 2, 2
NGROUP = 16
SMOOTHING = 0.05
NAMES = ("evaluation_ms", "gram_and_solve_kernels_ms", "download_ms")


def fault_rows(ngroup):
    """ngroup fault models of K = 64 basis sources: the same plane at strikes 10 degrees apart"""
    from kiwi_amd import slipfit
    return np.concatenate([slipfit.patch_basis("moment_tensor", origin=(0., 0., 0., 11000.), strike=10.0 * g, dip=30.0, rakes=(55., 145.),
                                               nx=NX, ny=NY, patch_length=3000., patch_width=2000., nwin=NWIN, window=2.0,
                                               rupture_velocity=2800.) for g in range(ngroup)])


def host_path(p, rows, K, nrec, penalty):
    """one group without the call: kept tapered synthetics down trace by trace, scipy's nnls on the stacked traces"""
    import scipy.optimize
    p.set_keep_synthetics(2)
    p.set_source_params("moment_tensor", rows[:K])
    p.eval()
    d = np.concatenate([p.get_reference(ir + 1, k + 1, 2, maxn=L + 64)[1].astype(np.float64) for ir in range(nrec) for k in range(3)])
    A = np.stack([np.concatenate([p.get_synthetics(i, ir + 1, k + 1, 2, maxn=L + 64)[1].astype(np.float64)
                                  for ir in range(nrec) for k in range(3)]) for i in range(K)], 1)
    p.set_keep_synthetics(0)
    full = np.zeros((K, K))
    full[np.triu_indices(K)] = penalty
    full = full + np.triu(full, 1).T
    ev, V = np.linalg.eigh(full * (np.sum(A * A) / K))
    F = (V * np.sqrt(np.clip(ev, 0.0, None))) @ V.T
    x, _ = scipy.optimize.nnls(np.concatenate([A, F], 0), np.concatenate([d, np.zeros(K)]), maxiter=30 * K)
    return x


def example_figures():
    """what examples/invert_slip.py finds, as README.md and CHANGELOG.md quote it"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("invert_slip", os.path.join(ROOT, "examples", "invert_slip.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    r = ex.main(verbose=False)
    return dict(planted_asperities=[list(a[:2]) for a in ex.ASPERITIES], found_asperities=[list(a) for a in r["asperities"]],
                planted_largest_coefficient=float(r["planted"].max()), free_smallest_coefficient=float(r["free"].min()),
                free_misfit=r["free_misfit"], nonneg_misfit=r["misfit"], nonneg_status=r["status"], npositive=r["npositive"],
                nsolves=r["nsolves"])


def main(reps=3):
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    import bench
    from kiwi_amd import slipfit, synthetic
    K = NX * NY * NRAKE * NWIN
    wl = synthetic.workload("cfg2", 64, 0)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    nrec = wl["nrec"]
    rows = fault_rows(NGROUP)
    penalty = SMOOTHING * slipfit.laplacian_penalty(NX, NY, NRAKE, NWIN)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
               workload=wl["name"], groups=NGROUP, K=K, sources=len(rows), receivers=nrec, window_samples=L, smoothing=SMOOTHING)
    modes = dict(free=dict(), nonneg_penalty=dict(nonneg=True, penalty=penalty, penalty_relative=True))
    fit = {}
    for name, kw in modes.items():
        p.linear_fit_wide_params("moment_tensor", rows[:2 * K], K, **kw)       # code objects, buffers
        runs = []
        for _ in range(reps):
            t = time.perf_counter()
            fit[name] = p.linear_fit_wide_params("moment_tensor", rows, K, **kw)
            runs.append(dict(call_s=time.perf_counter() - t, **dict(zip(NAMES, p.linear_fit_ms())),
                             **dict(zip(("gram_kernels_ms", "solve_kernel_ms"), p.linear_fit_wide_ms()))))
        f = fit[name]
        res[name] = dict(best=min(runs, key=lambda r: r["gram_and_solve_kernels_ms"]), runs=runs,
                         status_counts={str(k): int(np.sum(f.status == k)) for k in (0, 1, 2, 4)},
                         nsolves_range=[int(f.nsolves.min()), int(f.nsolves.max())], npositive_range=[int(f.npositive.min()), int(f.npositive.max())],
                         misfit_range=[float(np.nanmin(f.misfit)), float(np.nanmax(f.misfit))],
                         pivot_min_range=[float(f.pivot_min.min()), float(f.pivot_min.max())])
    gram_ms = min(r["gram_kernels_ms"] for m in modes for r in res[m]["runs"])
    res["gram_kernels_ms"] = gram_ms
    res["solve_kernel_ms"] = dict(nonneg_0=min(r["solve_kernel_ms"] for r in res["free"]["runs"]),
                                  nonneg_1=min(r["solve_kernel_ms"] for r in res["nonneg_penalty"]["runs"]))
    wsum = 3 * nrec * L
    bytes_syn, bytes_ref = 4.0 * len(rows) * wsum, 4.0 * NGROUP * wsum
    res["gram_compulsory_bytes"] = dict(kept_synthetics=bytes_syn, references=bytes_ref)
    res["gram_compulsory_gbs"] = (bytes_syn + bytes_ref) / (gram_ms * 1e-3) / 1e9
    gbs = ctypes.c_double(0.0)
    p._ck(p.L.kiwi_hip_measure_read_bandwidth(p.h, 4 << 30, 10, ctypes.byref(gbs)), "measure_read_bandwidth")
    res["pure_read_gbs_same_run"] = float(gbs.value)
    t = time.perf_counter()
    x = host_path(p, rows, K, nrec, penalty)
    t = time.perf_counter() - t
    f = fit["nonneg_penalty"]
    res["without_the_call"] = dict(groups_timed=1, seconds=t, scaled_to_all_groups_s=t * NGROUP, label="SCALED from 1 group",
                                   max_difference_of_coefficients_over_largest=float(np.max(np.abs(x - f.coef[0])) / np.max(np.abs(x))))
    res["without_over_with"] = t * NGROUP / res["nonneg_penalty"]["best"]["call_s"]
    p.close()
    res["example_invert_slip"] = example_figures()
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
