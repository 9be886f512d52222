#!/usr/bin/env python3
"""A moment-tensor grid ranked in two frequency bands and by an amplitude-spectrum norm, from ONE synthesis per trial source.

  1. a Green's function database and a receiver ring (synthetic stand-ins, kiwi_amd/synthetic.py);
  2. "observed" traces = synthetics of a known `moment_tensor` source + noise, set as references with misfit tapers;
  3. three bands: l2norm below 0.1 Hz, l2norm between 0.1 and 0.4 Hz, ampspec_l2norm of the unfiltered traces
     (Engine.set_misfit_bands); a grid over strike x dip x rake is evaluated once and compared in all three
     (Engine.band_misfits_for_params), the bands folded into one outer misfit per source (gridsearch.make_band_global_misfits);
  4. the same ranking from three separate evaluations, one per band, with their time beside the band call's.

Run on a machine with an MI355X:  python examples/invert_multiband.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, gridsearch  # noqa: E402

BANDS = [("l2norm", [0.005, 0.01, 0.08, 0.1], [0., 1., 1., 0.]),
         ("l2norm", [0.08, 0.1, 0.35, 0.4], [0., 1., 1., 0.]),
         ("ampspec_l2norm", None, None)]


def main(nrec=12, L=512, noise=0.03, seed=1, step=30, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=48, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=150e3)
    e = Engine(0)
    e.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    grid = synthetic.mt_sdr_grid(step=step, depth=11000.0)
    iplanted = len(grid) // 3 + 7
    true = grid[iplanted].copy()
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    dt = gf["dt"]
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            n = rng.standard_normal(len(d)).astype(np.float32)
            n = np.convolve(n, np.hanning(21) / np.hanning(21).sum(), "same")
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * n)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")
    e.set_misfit_bands(BANDS)
    e.band_misfits_for_params("moment_tensor", grid[:8])          # (first call: transform tables, reference variants)
    t0 = time.perf_counter()
    m, n, g, failings = e.band_misfits_for_params("moment_tensor", grid)
    t_bands = time.perf_counter() - t0
    ms = e.band_misfits_ms()
    mis, nor = gridsearch.band_slots_to_receivers(m, n, comps)
    outer, _ = gridsearch.make_band_global_misfits(mis, nor, band_weights=[1.0, 1.0, 0.5])
    ibest = int(np.nanargmin(outer))
    # the same from three separate evaluations
    t0 = time.perf_counter()
    sep = []
    for name, fx, fy in BANDS:
        e.set_misfit_filter(0, [] if fx is None else fx, [] if fx is None else fy)
        e.set_misfit_method(name)
        sm, sn, sg, _ = e.misfits_for_params("moment_tensor", grid)
        sep.append((sm, sn))
    t_sep = time.perf_counter() - t0
    same = all(np.array_equal(m[:, b], sep[b][0]) and np.array_equal(n[:, b], sep[b][1]) for b in range(len(BANDS)))
    if verbose:
        print("%d trial sources x %d bands: band call %.1f ms (evaluation %.1f, band kernels %.1f, downloads %.1f); "
              "three separate evaluations %.1f ms" % (len(grid), len(BANDS), 1e3 * t_bands, ms[0], ms[1], ms[2], 1e3 * t_sep))
        print("band misfits equal the separate evaluations bit for bit: %s" % same)
        print("best source: index %d, strike dip rake from the grid, outer misfit %.4f; per band %s" % (
            ibest, outer[ibest], " ".join("%.4f" % v for v in g[ibest])))
        # (two (strike, dip, rake) triples of the grid may describe the same tensor: the tensor is what is recovered)
        hit = np.allclose(grid[ibest, 4:10], true[4:10], rtol=1e-5, atol=1e-5 * np.abs(true[4:10]).max())
        print("planted source recovered" if hit else "planted source NOT recovered: planted %d" % iplanted)
    e.close()
    return ibest, iplanted, outer


if __name__ == "__main__":
    main()
