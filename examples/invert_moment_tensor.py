#!/usr/bin/env python3
"""Best moment tensor per trial location by linear least squares, on synthetic data.

  1. a Green's function database and a receiver ring (synthetic stand-ins, kiwi_amd/synthetic.py);
  2. "observed" traces = synthetics of a known `moment_tensor` source + noise, set as references with misfit tapers;
  3. a grid over north-shift x east-shift x depth; at every node the six elementary tensors are evaluated and the tensor
     that fits best follows from a 6 x 6 solve on the device (kiwi_amd/mtfit.py, Engine.linear_fit_params) -- six
     evaluations per node instead of a sweep over strike, dip, rake and moment;
  4. the best node, its tensor, and the trace-free (deviatoric) tensor there.

Run on a machine with an MI355X:  python examples/invert_moment_tensor.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, gridsearch, mtfit  # noqa: E402


def main(nrec=24, L=1024, noise=0.05, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=96, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=300e3)
    e = Engine(0)
    e.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    tensor = np.array(synthetic.mt_from_sdr(35., 60., 110., 7e18)) + np.array([1e18, 1e18, 1e18, 0, 0, 0])
    true = np.array([0., 2000., -1000., 11000.] + list(tensor) + [1.0], np.float32)
    # observed data: synthetics of the true source (no references needed for that) + band-limited noise
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    dt = gf["dt"]
    for ir in range(nrec):
        for k in range(3):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            n = rng.standard_normal(len(d)).astype(np.float32)
            n = np.convolve(n, np.hanning(21) / np.hanning(21).sum(), "same")
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * n)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")
    start = true.copy()
    start[4:10] = 1e18                                   # the tensor columns of the grid's base source are not used
    grid = gridsearch.MisfitGrid("moment_tensor", start, param_ranges=[("north-shift", 0, 4000, 1000), ("east-shift", -3000, 1000, 1000),
                                                                        ("depth", 9000, 13000, 1000)])
    t0 = time.perf_counter()
    grid.compute(e, linear_mt=True)
    t_grid = time.perf_counter() - t0
    best = grid.best_source
    dev, dev_misfit, _, _ = mtfit.fit_moment_tensors(e, "moment_tensor", best, deviatoric=True)
    if verbose:
        print("grid: %d nodes x 6 elementary tensors in %.3f s (evaluation %.1f ms, fit kernels %.2f ms, download %.2f ms of the last call)"
              % ((len(grid.sources), t_grid) + e.linear_fit_ms()))
        print("best grid point: north %.0f east %.0f depth %.0f, misfit %.4f (smallest pivot %.2f)"
              % (best[1], best[2], best[3], grid.fit_misfits[grid.ibest], grid.fit_pivot_min[grid.ibest]))
        print("   fitted tensor  [1e18 N m]: " + " ".join("%7.3f" % (v / 1e18) for v in best[4:10]))
        print("   true tensor    [1e18 N m]: " + " ".join("%7.3f" % (v / 1e18) for v in true[4:10]))
        print("   deviatoric fit [1e18 N m]: " + " ".join("%7.3f" % (v / 1e18) for v in dev[0]) + "   misfit %.4f" % dev_misfit[0])
        print("true: north %.0f east %.0f depth %.0f" % (true[1], true[2], true[3]))
    e.close()
    return true, grid


if __name__ == "__main__":
    main()
