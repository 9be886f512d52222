"""What nk origin times cost from one synthesis (kiwi_hip_time_scan) against nk separate evaluations, on configuration 3's shape
(`synthetic.workload('cfg3')` set up as bench.py does: 4096 sources x 50 receivers x 3 components x 4096 samples) and on
configuration 5's.  Per row -- nk = 1, 5, 21, 81 under unfiltered l2norm; nk = 5, 21 under l2norm with a frequency filter on every
receiver; nk = 5, 21 under ampspec_l2norm --: the whole scan call by the host clock and its three HIP-event times (evaluation, scan
kernels, downloads); in the same run on the same context the nk separate set_source_params (times moved by k dt) + eval +
get_misfits of the interface the call replaces, with the part of it that is evaluation + download alone; whether offset 0 of the
scan is the plain evaluation in bits.  The JSON is rewritten after every row.  `--bench-before=<files>` / `--bench-after=<files>`
(comma-separated): the outputs of bench.py's default line run from a checkout of the parent commit and from this one in the same
session, copied into the result.

    python profiles/time_scan_rate.py [out.json] [--commit=<id>] [--nsrc=4096] [--nsrc5=1024] [--reps=2] [--cases=cfg3,cfg5]"""
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
FILTER = ([0.016, 0.02, 0.4, 0.48], [0., 1., 1., 0.])
ROWS = [("l2norm", None, 1), ("l2norm", None, 5), ("l2norm", None, 21), ("l2norm", None, 81),
        ("l2norm", FILTER, 5), ("l2norm", FILTER, 21), ("ampspec_l2norm", None, 5), ("ampspec_l2norm", None, 21)]


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def case(name, nsrc, reps, res, flush):
    import bench
    from kiwi_amd import synthetic
    wl = synthetic.workload(name, nsrc, 0)
    wl = dict(wl, method="l2norm", filter=None)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    dt = float(gf["dt"])
    trials = np.array(wl["trials"], np.float32)
    out = res[name] = dict(workload=wl["name"], sourcetype=wl["sourcetype"], sources=len(trials), receivers=wl["nrec"], window_samples=L,
                           centroids_per_source=ncent, dt=dt, rows=[])

    def separate(ks):
        """(whole time, evaluation + download part of it, results): the parent's interface, one upload per origin time"""
        t_all, t_dev, got = 0.0, 0.0, []
        for k in ks:
            rows = trials.copy()
            rows[:, 0] += np.float32(k * dt)
            t0 = time.perf_counter()
            p.set_source_params(wl["sourcetype"], rows)
            t1 = time.perf_counter()
            p.eval()
            got.append(p.get_misfits())
            t2 = time.perf_counter()
            t_all += t2 - t0
            t_dev += t2 - t1
        return t_all, t_dev, got

    for method, filt, nk in ROWS:
        p.set_misfit_filter(0, *(filt if filt is not None else ([], [])))
        p.set_misfit_method(method)
        k0 = -(nk // 2)
        ks = [k0 + j for j in range(nk)]
        p.set_source_params(wl["sourcetype"], trials)
        p.time_scan(0, None, k0, 1, nk)                      # tables, reference variants, buffers
        calls = []
        for _ in range(reps):
            p.set_source_params(wl["sourcetype"], trials)
            t, got = timed(lambda: p.time_scan(0, None, k0, 1, nk))
            calls.append(dict(call_s=t, **dict(zip(("evaluation_ms", "scan_kernels_ms", "download_ms"), p.time_scan_ms()))))
        t_up = timed(lambda: p.set_source_params(wl["sourcetype"], trials))[0]
        p.eval()
        plain = p.get_misfits()
        seps = [separate(ks)[:2] for _ in range(1 if nk > 21 else reps)]
        best = min(calls, key=lambda r: r["call_s"])
        sep_all, sep_dev = min(s[0] for s in seps), min(s[1] for s in seps)
        j0 = ks.index(0)
        row = dict(method=method, filter=filt, nk=nk, k0=k0, kstep=1,
                   scan_call=dict(best, runs_call_s=[c["call_s"] for c in calls]), upload_once_s=t_up,
                   scan_call_with_upload_s=best["call_s"] + t_up,
                   separate_evaluations_s=dict(whole=sep_all, evaluation_and_download=sep_dev, runs=[s[0] for s in seps]),
                   separate_over_scan=sep_all / (best["call_s"] + t_up), separate_device_part_over_scan_call=sep_dev / best["call_s"],
                   scan_faster=bool(best["call_s"] + t_up < sep_all),
                   offset0_equals_plain_bits=bool(np.array_equal(got[0][:, j0], plain[0]) and np.array_equal(got[2][:, j0], plain[2])),
                   offset0_largest_rel_difference=float(np.max(np.abs(got[0][:, j0].astype(np.float64) - plain[0]) /
                                                               np.maximum(np.abs(plain[0]), plain[1]))))
        out["rows"].append(row)
        print(name, json.dumps(row), flush=True)
        flush()
    gbs = ctypes.c_double(0.0)
    p._ck(p.L.kiwi_hip_measure_read_bandwidth(p.h, 4 << 30, 10, ctypes.byref(gbs)), "measure_read_bandwidth")
    out["pure_read_gbs_same_run"] = float(gbs.value)
    p.close()
    flush()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    from kiwi_amd import lib
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName))
    buf = ctypes.create_string_buffer(1024)
    lib.load().kiwi_hip_build_flags(buf, 1024)
    res["build_flags_extra"] = buf.value.decode()
    res["arithmetic"] = os.environ.get("KIWI_HIP_ARITH", "exact")
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                    stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    if "bench-before" in opt and "bench-after" in opt:       # files (comma-separated) whose last line is bench.py's JSON result line
        def lines(names):
            out = []
            for fn in names.split(","):
                with open(fn) as fh:
                    b = json.loads([ln for ln in fh.read().splitlines() if ln.strip().startswith("{")][-1])
                out.append({k: b[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup")})
            return out
        a, b = lines(opt["bench-before"]), lines(opt["bench-after"])
        res["bench_default_line"] = dict(parent_library=a, this_library=b,
                                         this_over_parent=(sum(x["value"] for x in b) / len(b)) / (sum(x["value"] for x in a) / len(a)))

    def flush():
        if args:
            with open(args[0], "w") as fh:
                json.dump(res, fh, indent=1)

    reps = int(opt.get("reps", 2))
    which = opt.get("cases", "cfg3,cfg5").split(",")
    if "cfg3" in which:
        case("cfg3", int(opt.get("nsrc", 4096)), reps, res, flush)
    if "cfg5" in which:
        case("cfg5", int(opt.get("nsrc5", 1024)), reps, res, flush)
    print(json.dumps(res))
    flush()


if __name__ == "__main__":
    main()
