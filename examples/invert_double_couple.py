#!/usr/bin/env python3
"""The best double couple over depth x strike x dip x rake from SIX syntheses per depth, with a bootstrap of the mechanism.

  1. the setup of examples/invert_moment_tensor.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known double couple (a node of the grid below) + noise;
  2. a depth axis; at every depth the 36 x 10 x 36 = 12 960 mechanisms at 10 degrees (strike x dip x rake) with the planted
     moment.  The seismograms are linear in the tensor, so every mechanism is a combination of the six elementary tensors'
     synthetics: `mtfit.scan_double_couples` synthesises those six per depth and evaluates all mechanisms from their normal
     equations on the device (kiwi_hip_linear_fit_candidates), under the l1norm outer norm;
  3. at the best depth, the per-receiver misfits of all 12 960 mechanisms go through `Engine.outer_misfits` with bootstrap
     weights over the receivers: how often each mechanism wins.

Run on a machine with an MI355X:  python examples/invert_double_couple.py [--small]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402

GRID = (range(0, 360, 10), range(0, 91, 10), range(-180, 180, 10))
PLANTED = (40., 60., 110., 7e18)


def main(nrec=12, L=1024, depths=(9000., 10000., 11000., 12000., 13000.), noise=0.05, draws=200, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=96, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=300e3)
    e = Engine(0)
    e.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    true = np.array([0., 2000., -1000., 11000.] + list(synthetic.mt_from_sdr(*PLANTED)) + [1.0], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        for k in range(3):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * rng.standard_normal(len(d)).astype(np.float32))
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), gf["dt"], ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")

    rows = np.tile(true, (len(depths), 1))
    rows[:, 3] = depths
    res = mtfit.scan_double_couples(e, "moment_tensor", rows, *GRID, moment=PLANTED[3], outer_norm="l1norm", receiver_misfit=True)
    ms = e.linear_fit_candidates_ms()
    nmech = len(GRID[0]) * len(GRID[1]) * len(GRID[2])
    ibest = int(np.argmin(res["misfit"]))
    found = (float(depths[ibest]), res["strike"][ibest], res["dip"][ibest], res["rake"][ibest])
    if verbose:
        for i, z in enumerate(depths):
            print("depth %6.0f m: best double couple (%3.0f, %2.0f, %4.0f) misfit %.4f; free tensor (l2norm) misfit %.4f" % (
                z, res["strike"][i], res["dip"][i], res["rake"][i], res["misfit"][i], res["tensor_misfit"][i]))
        print("best: depth %.0f m, strike %.0f, dip %.0f, rake %.0f; planted: depth %.0f m, strike %.0f, dip %.0f, rake %.0f" % (
            found + (true[3],) + PLANTED[:3]))
        print("evaluation %.2f ms, Gram and solve %.2f ms, candidate kernels %.2f ms, downloads %.2f ms" % ms)
        print("%d trial sources from %d syntheses: %d syntheses saved" % (
            len(depths) * nmech, 6 * len(depths), len(depths) * nmech - 6 * len(depths)))

    # bootstrap over the receivers at the best depth: every receiver one slot, its l2 misfit over all its components
    scan = res["scan"]
    m = scan.receiver_misfit[ibest][:, :, None]
    n = np.broadcast_to(scan.receiver_norm[ibest][None, :, None], m.shape)
    weights = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=draws).astype(np.float64)
    _, winner, _ = e.outer_misfits(m, n, outer_norm="l1norm", draw_weights=weights, ncomponents=[1] * nrec)
    _, sdr = mtfit.double_couple_candidates(*GRID)
    share = float(np.mean(winner == res["index"][ibest]))
    if verbose:
        w = sdr[winner]
        print("bootstrap of %d draws at depth %.0f m: the best mechanism wins %.0f %%; strike %.0f .. %.0f, dip %.0f .. %.0f, rake %.0f .. %.0f" % (
            draws, depths[ibest], 100 * share, w[:, 0].min(), w[:, 0].max(), w[:, 1].min(), w[:, 1].max(), w[:, 2].min(), w[:, 2].max()))
    e.close()
    ok = found == (float(true[3]),) + PLANTED[:3]
    if verbose:
        print("planted mechanism found" if ok else "planted mechanism NOT found")
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(10000., 11000., 12000.), draws=50) if small else main()) else 1)
