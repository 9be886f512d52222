"""set_database dbpath nipx nipz on the device: time of the densification of cfg3's database (synthetic.make_gfdb():
128 x 6 x 10 x 4096) at (2,1), (1,2), (2,2), (4,4) -- the cold first call, then the median of 5, each ending in a device
synchronise -- and cfg3 evals/s (synthetic.workload('cfg3'), set up as bench.py does) through the (2,2) database against the stored one.

    python profiles/densify_rate.py [out.json] [--commit=<id>]   (the commit measured; default: git rev-parse HEAD)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kiwi_amd import Engine, synthetic  # noqa: E402


def timed_set(p, gf, f):
    t = time.perf_counter()
    p.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"],
                   nipx=f[0], nipz=f[1])
    p.sync()
    return time.perf_counter() - t


def cfg3_evals_per_s(p, gf, f, reps=5):
    """cfg3 (synthetic.workload('cfg3'): 50 receivers, 256 bilateral trials of 100 centroids, l2norm, whole-trace tapers,
    references = synthetics of the true source) through the database installed at factors f, set up like bench.py's
    setup_product; median of `reps` timed evaluations."""
    wl = synthetic.workload("cfg3")
    pk = synthetic.pack_gfdb(gf)
    p.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], pk["data"], pk["first"], pk["nsamp"],
                   nipx=f[0], nipz=f[1])
    del pk
    lat, lon, depth, comps, dist = synthetic.make_receivers(wl["nrec"])
    p.set_receivers(lat, lon, depth, comps)
    p.set_source_location(40.0, 30.0, 0.0)
    p.set_effective_dt(0.5)
    p.set_local_interpolation("bilinear")
    p.set_misfit_method(wl["method"])
    dt, L = gf["dt"], gf["data"].shape[3]
    firsts = [int(round(d / 6000.0 / dt)) for d in dist]
    for ir in range(wl["nrec"]):
        for k in range(3):
            p.set_ref_seismogram(ir + 1, k + 1, firsts[ir], np.zeros(L, np.float32))
        p.set_misfit_taper(ir + 1, *synthetic.full_taper(firsts[ir], L, dt))
    trials = wl["trials"]
    first = trials.copy()
    first[0] = wl["true"]
    p.set_keep_synthetics(1)
    p.set_source_params(wl["sourcetype"], first)
    p.eval()
    refs = {(ir + 1, k + 1): p.get_synthetics(0, ir + 1, k + 1, 1) for ir in range(wl["nrec"]) for k in range(3)}
    p.set_keep_synthetics(0)
    for (ir, k), (lo, d) in refs.items():
        p.set_ref_seismogram(ir, k, lo, d)
    p.set_source_params(wl["sourcetype"], trials)
    for _ in range(3):
        p.eval()
    p.sync()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        p.eval()
        p.sync()
        times.append(time.perf_counter() - t)
    return len(trials) / float(np.median(times))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--commit=")]
    commit = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")), None)
    out = args[0] if args else None
    gf = synthetic.make_gfdb()
    p = Engine(0)
    res = dict(database="make_gfdb() 128x6x10x4096", set_database_s={})
    for f in [(1, 1), (2, 1), (1, 2), (2, 2), (4, 4)]:
        cold = timed_set(p, gf, f)
        warm = [timed_set(p, gf, f) for _ in range(5)]
        res["set_database_s"]["%d,%d" % f] = dict(cold=cold, median5=float(np.median(warm)))
        print(f, res["set_database_s"]["%d,%d" % f], flush=True)
    res["cfg3_evals_per_s"] = {"1,1": cfg3_evals_per_s(p, gf, (1, 1)), "2,2": cfg3_evals_per_s(p, gf, (2, 2))}
    print(res["cfg3_evals_per_s"], flush=True)
    res["commit"] = commit
    if commit is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                    stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
