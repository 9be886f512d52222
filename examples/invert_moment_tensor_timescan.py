#!/usr/bin/env python3
"""A free moment tensor at every node of a depth x origin-time grid on noisy data, from SIX syntheses per depth.

  1. a Green's function database and a receiver ring (synthetic stand-ins, kiwi_amd/synthetic.py);
  2. "observed" traces = synthetics of a known `moment_tensor` source at a planted depth and origin time + noise, set as
     references with misfit tapers;
  3. a grid over 5 depths x 21 origin times, one sample apart: MisfitGrid.compute_mt_time_scan(engine) synthesises the six
     elementary tensors of every depth at the first time and fits the tensor at every origin time from their inner products
     (Engine.linear_fit_time_scan_params, kiwi_hip_linear_fit_time_scan) -- 30 syntheses instead of 630;
  4. the same fits made time by time (Engine.linear_fit_params per origin time: what the library offered before), with their
     time beside the scan's.

Run on a machine with an MI355X:  python examples/invert_moment_tensor_timescan.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, gridsearch, mtfit  # noqa: E402


def main(nrec=12, L=512, noise=0.03, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=48, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=150e3)
    dt = gf["dt"]
    e = Engine(0)
    e.set_database(dt, gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    depths = np.array([9000., 10000., 11000., 12000., 13000.])
    times = (np.arange(21) - 10) * dt                          # whole samples: gridsearch.split_time_axis takes the axis
    planted_depth, planted_time = depths[3], times[14]
    planted = np.array([4.1e18, -2.3e18, 7.7e18, 3.5e18, -2.9e18, 5.2e18], np.float32)
    true = np.array([planted_time, 0., 0., planted_depth] + list(planted) + [0.5], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            n = rng.standard_normal(len(d)).astype(np.float32)
            n = np.convolve(n, np.hanning(21) / np.hanning(21).sum(), "same")
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * n)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")
    base = true.copy()
    base[0], base[3], base[4:10] = 0.0, depths[0], 1e18
    axes = [("depth", depths), ("time", times)]
    grid = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    grid.compute_mt_time_scan(e)                               # (first call: code objects)
    grid = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    t0 = time.perf_counter()
    grid.compute_mt_time_scan(e, evaluate_fitted=False)
    t_scan = time.perf_counter() - t0
    ms = e.linear_fit_time_scan_ms()
    # time by time: six syntheses per (depth, origin time)
    nodes = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes).sources
    mtfit.fit_moment_tensors(e, "moment_tensor", nodes[:len(times)])
    t0 = time.perf_counter()
    tensors, misfit, status, _ = mtfit.fit_moment_tensors(e, "moment_tensor", nodes)
    t_plain = time.perf_counter() - t0
    best = grid.best_source
    hit = best[0] == np.float32(planted_time) and best[3] == np.float32(planted_depth)
    rel = np.abs(best[4:10] - planted) / np.abs(planted).max()
    if verbose:
        n = len(grid.sources)
        print("%d grid nodes: %d syntheses with the scan, %d syntheses saved" % (n, 6 * n - grid.syntheses_saved, grid.syntheses_saved))
        print("scan %.1f ms (evaluation %.2f, Gram-scan kernel %.2f, solve kernels %.2f, downloads %.2f); time by time %.1f ms" % (
            1e3 * t_scan, ms[0], ms[1], ms[2], ms[3], 1e3 * t_plain))
        print("best node: depth %.0f m, time %.2f s, misfit %.4f; time by time: depth %.0f m, time %.2f s, misfit %.4f" % (
            best[3], best[0], grid.fit_misfits[grid.ibest], nodes[int(np.nanargmin(misfit)), 3], nodes[int(np.nanargmin(misfit)), 0],
            np.nanmin(misfit)))
        print("largest |scan - time by time| of the fit misfits: %.3g" % np.nanmax(np.abs(grid.fit_misfits - misfit)))
        print("fitted tensor against the planted one, relative to its largest component:", np.array2string(rel, precision=3))
        print("planted node found" if hit and np.all(rel < 0.1) else
              "planted node NOT found: planted depth %.0f m, time %.2f s" % (planted_depth, planted_time))
    e.close()
    return best, (planted_time, planted_depth)


if __name__ == "__main__":
    main()
