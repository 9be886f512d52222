#!/usr/bin/env python3
"""The best double couple, depth and origin time on noisy data, from SIX syntheses per depth.

  1. the setup of examples/invert_double_couple.py: synthetic Green's functions, a receiver ring, "observed" traces = the synthetics
     of a known double couple at a planted depth and origin time + noise;
  2. a grid over depths x origin times, one sample apart, and at every node the mechanisms strike x dip x rake with the planted
     moment: MisfitGrid.compute_dc_time_scan(engine, ...) synthesises the six elementary tensors of every depth at the first time
     and evaluates every mechanism at every origin time from their inner products on the device
     (Engine.linear_fit_candidates_time_scan_params, kiwi_hip_linear_fit_candidates_time_scan), under the l1norm outer norm;
  3. the mechanism cube with the origin time profiled out at the best depth: how many mechanisms come within 10 % of the best one;
  4. the same answers made time by time (mtfit.scan_double_couples per origin time: what the library offered before), with their
     time beside the scan's.

Run on a machine with an MI355X:  python examples/invert_double_couple_timescan.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, gridsearch, mtfit  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def main(nrec=12, L=1024, depths=(9000., 10000., 11000., 12000., 13000.), nk=21, step=10, noise=0.05, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    mech = (range(0, 360, step), range(0, 91, step), range(-180, 180, step))
    gf = synthetic.make_gfdb(nx=96, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=300e3)
    dt = gf["dt"]
    e = Engine(0)
    e.set_database(dt, gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    depths = np.asarray(depths, np.float64)
    times = (np.arange(nk) - nk // 2) * dt                     # whole samples: gridsearch.split_time_axis takes the axis
    planted_depth, planted_time = depths[len(depths) // 2 + 1], times[(2 * nk) // 3]
    true = np.array([planted_time, 2000., -1000., planted_depth] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * rng.standard_normal(len(d)).astype(np.float32))
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")
    base = true.copy()
    base[0], base[3] = 0.0, depths[0]
    axes = [("depth", depths), ("time", times)]
    grid = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    grid.compute_dc_time_scan(e, *mech, moment=PLANTED[3])     # (first call: code objects)
    grid = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes)
    t0 = time.perf_counter()
    grid.compute_dc_time_scan(e, *mech, moment=PLANTED[3], cube=True)
    t_scan = time.perf_counter() - t0
    ms = e.linear_fit_candidates_time_scan_ms()
    # time by time: six syntheses per (depth, origin time)
    nodes = gridsearch.MisfitGrid("moment_tensor", base, param_values=axes).sources
    mtfit.scan_double_couples(e, "moment_tensor", nodes[:len(times)], *mech, moment=PLANTED[3])
    t0 = time.perf_counter()
    plain = mtfit.scan_double_couples(e, "moment_tensor", nodes, *mech, moment=PLANTED[3])
    t_plain = time.perf_counter() - t0
    best = grid.best_source
    found = (float(best[3]), float(best[0])) + tuple(grid.dc_sdr[grid.ibest])
    want = (float(np.float32(planted_depth)), float(np.float32(planted_time))) + PLANTED[:3]
    if verbose:
        n, nmech = len(grid.sources), len(mech[0]) * len(mech[1]) * len(mech[2])
        print("%d grid nodes x %d mechanisms: %d syntheses with the scan, %d syntheses saved" % (n, nmech, nmech * n - grid.syntheses_saved, grid.syntheses_saved))
        print("scan %.1f ms (evaluation %.2f, Gram-scan kernel %.2f, solve kernels %.2f, candidate-scan kernels %.2f, downloads %.2f); "
              "time by time %.1f ms" % ((1e3 * t_scan,) + ms + (1e3 * t_plain,)))
        print("best node: depth %.0f m, time %.2f s, strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (found + (grid.dc_misfits[grid.ibest],)))
        ip = int(np.nanargmin(plain["misfit"]))
        print("time by time: depth %.0f m, time %.2f s, strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (
            nodes[ip, 3], nodes[ip, 0], plain["strike"][ip], plain["dip"][ip], plain["rake"][ip], plain["misfit"][ip]))
        print("largest |scan - time by time| of the best misfits per node: %.3g" % np.nanmax(np.abs(grid.dc_misfits - plain["misfit"])))
        cube = grid.dc_cube[grid.ibest // len(times)]
        print("mechanism cube at the best depth, origin time profiled out: %d of %d mechanisms within 10 %% of the best misfit" % (
            int(np.sum(cube <= 1.1 * np.nanmin(cube))), cube.size))
        print("planted node found" if found == want else
              "planted node NOT found: planted depth %.0f m, time %.2f s, strike %.0f, dip %.0f, rake %.0f" % want)
    e.close()
    return found == want


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(10000., 11000., 12000.), nk=7) if small else main()) else 1)
