"""What B misfit bands cost from one synthesis (kiwi_hip_band_misfits) against B separate evaluations, on configuration 3's
shape (`synthetic.workload('cfg3')` set up as bench.py does: 4096 sources x 50 receivers x 3 components x 4096 samples) and on
configuration 5's.  Per band count B = 1, 2, 4, 8 -- the mix: one unfiltered l2norm, filtered l2norm in distinct pass bands, one
ampspec_l2norm (from B = 2 on) --: the whole band call by the host clock and its three HIP-event times (evaluation, band kernels,
downloads); in the same run on the same context the sum of B separate set_misfit_filter + set_misfit_method + eval + get_misfits
(the path the call replaces); and for B = 1 the plain evaluation beside the band call, which shows what writing the synthetics
to memory costs where the plain evaluation compares inside the accumulate kernel.

    python profiles/band_misfits_rate.py [out.json] [--commit=<id>] [--nsrc=4096]"""
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


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def pass_band(i, n):
    """the i-th of n pass bands between 0.02 and 0.8 Hz, cosine flanks"""
    edges = np.geomspace(0.02, 0.8, n + 1)
    lo, hi = float(edges[i]), float(edges[i + 1])
    return [0.8 * lo, lo, hi, 1.2 * hi], [0., 1., 1., 0.]


def band_mix(B):
    """one unfiltered l2norm, filtered l2norm in distinct pass bands, one ampspec_l2norm"""
    if B == 1:
        return [("l2norm", None, None)]
    nf = B - 2
    return [("l2norm", None, None)] + [("l2norm",) + tuple(pass_band(i, max(nf, 1))) for i in range(nf)] + [("ampspec_l2norm", None, None)]


def separate(p, bands):
    out = []
    for name, fx, fy in bands:
        p.set_misfit_filter(0, [] if fx is None else fx, [] if fx is None else fy)
        p.set_misfit_method(name)
        p.eval()
        out.append(p.get_misfits())
    return out


def case(name, nsrc, reps=3):
    import bench
    from kiwi_amd import synthetic
    wl = synthetic.workload(name, nsrc, 0)
    wl = dict(wl, method="l2norm", filter=None)              # the context's own comparator: the cheapest (it runs inside the band call)
    p, gf, recv, refs, tapers, ncent = bench.setup_product(0, wl, L)
    res = dict(workload=wl["name"], sourcetype=wl["sourcetype"], sources=len(wl["trials"]), receivers=wl["nrec"], window_samples=L,
               centroids_per_source=ncent, bands={})
    for B in (1, 2, 4, 8):
        bands = band_mix(B)
        p.set_misfit_bands(bands)
        p.band_misfits()                                     # tables, reference variants, buffers
        sep = separate(p, bands)
        calls, seps = [], []
        for _ in range(reps):
            t, got = timed(p.band_misfits)
            calls.append(dict(call_s=t, **dict(zip(("evaluation_ms", "band_kernels_ms", "download_ms"), p.band_misfits_ms()))))
            seps.append(timed(lambda: separate(p, bands))[0])
        best = min(calls, key=lambda r: r["call_s"])
        same = all(np.array_equal(got[0][:, b], sep[b][0]) and np.array_equal(got[1][:, b], sep[b][1]) and np.array_equal(got[2][:, b], sep[b][2])
                   for b in range(B))
        r = dict(bands=[dict(method=b[0], filter=b[1]) for b in bands], band_call=dict(best, runs_call_s=[c["call_s"] for c in calls]),
                 separate_evaluations_s=dict(best=min(seps), runs=seps), call_over_one_separate_evaluation=best["call_s"] / (min(seps) / B),
                 separate_over_call=min(seps) / best["call_s"], equal_bit_for_bit=bool(same))
        if B == 1:
            p.set_misfit_filter(0, [], [])
            p.set_misfit_method("l2norm")
            plain = [timed(lambda: (p.eval(), p.get_misfits()))[0] for _ in range(reps)]
            r["plain_evaluation_s"] = dict(best=min(plain), runs=plain)
            r["band_call_over_plain_evaluation"] = best["call_s"] / min(plain)
        res["bands"][str(B)] = r
        print(name, B, json.dumps(r), flush=True)
    gbs = ctypes.c_double(0.0)
    p._ck(p.L.kiwi_hip_measure_read_bandwidth(p.h, 4 << 30, 10, ctypes.byref(gbs)), "measure_read_bandwidth")
    res["pure_read_gbs_same_run"] = float(gbs.value)
    p.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    from kiwi_amd import lib
    nsrc = int(opt.get("nsrc", 4096))
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName))
    buf = ctypes.create_string_buffer(1024)
    lib.load().kiwi_hip_build_flags(buf, 1024)
    res["build_flags_extra"] = buf.value.decode()
    res["arithmetic"] = os.environ.get("KIWI_HIP_ARITH", "exact")
    res["cfg3"] = case("cfg3", nsrc)
    res["cfg5"] = case("cfg5", min(nsrc, 1024))
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
