#!/usr/bin/env python3
"""A moment-tensor grid over depth x origin time on noisy data, the time axis scanned from ONE synthesis per depth.

  1. a Green's function database and a receiver ring (synthetic stand-ins, kiwi_amd/synthetic.py);
  2. "observed" traces = synthetics of a known `moment_tensor` source at a planted depth and origin time + noise, set as
     references with misfit tapers;
  3. a grid over 5 depths x 21 origin times, one sample apart: MisfitGrid.compute(engine, time_scan=True) synthesises the five
     depths at the first time and scans the axis (Engine.time_scan_for_params) -- 5 syntheses instead of 105;
  4. the same grid evaluated node by node, with its time beside the scan's.

Run on a machine with an MI355X:  python examples/invert_timescan.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, gridsearch  # noqa: E402


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
    # (rise time 0.5 s: two centroids at -+ 0.125 s, so that every centroid's time / dt is exact in fp32 and the scan equals the
    # node-by-node evaluation in bits, include/kiwi_hip.h)
    true = np.array([planted_time, 0., 0., planted_depth, 4.1e18, -2.3e18, 7.7e18, 3.5e18, -2.9e18, 5.2e18, 0.5], np.float32)
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
    base[0], base[3] = 0.0, depths[0]
    axes = [("depth", depths), ("time", times)]
    scan = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    scan.compute(e, time_scan=True)                            # (first call: code objects)
    t0 = time.perf_counter()
    scan.compute(e, time_scan=True)
    t_scan = time.perf_counter() - t0
    ms = e.time_scan_ms()
    scan.postprocess(bootstrap_iterations=20, rng=np.random.default_rng(2))
    plain = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    t0 = time.perf_counter()
    plain.compute(e)
    t_plain = time.perf_counter() - t0
    plain.postprocess(bootstrap_iterations=20, rng=np.random.default_rng(2))
    best = scan.best_source
    hit = best[0] == np.float32(planted_time) and best[3] == np.float32(planted_depth)
    if verbose:
        print("%d grid nodes: %d syntheses with the scan, %d syntheses saved" % (len(scan.sources), len(scan.sources) - scan.syntheses_saved,
                                                                               scan.syntheses_saved))
        print("scan %.1f ms (evaluation %.2f, scan kernels %.2f, downloads %.2f); node by node %.1f ms" % (
            1e3 * t_scan, ms[0], ms[1], ms[2], 1e3 * t_plain))
        print("best node: depth %.0f m, time %.2f s, misfit %.4f; node by node: depth %.0f m, time %.2f s" % (
            best[3], best[0], scan.get_best_misfit(), plain.best_source[3], plain.best_source[0]))
        print("largest |scan - node by node| / max(misfit, norm factor): %.3g" % np.max(
            np.abs(scan.misfits_by_src - plain.misfits_by_src) / np.maximum(np.maximum(plain.misfits_by_src, plain.norms_by_src), 1e-300)))
        print("planted time found" if hit else "planted time NOT found: planted depth %.0f m, time %.2f s" % (planted_depth, planted_time))
    e.close()
    return best, (planted_time, planted_depth)


if __name__ == "__main__":
    main()
