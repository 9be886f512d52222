#!/usr/bin/env python3
"""The best double couple when every station is mis-timed by the velocity model, from SIX syntheses per location.

  1. the setup of examples/invert_double_couple.py: synthetic Green's functions, a receiver ring, "observed" traces = the synthetics
     of a known double couple + noise -- but every station's data arrive late or early by its own whole number of samples, as a
     velocity model that is wrong along single paths makes them;
  2. mtfit.scan_double_couples under l2norm (no shifts): the mechanism the mis-timed data ask for;
  3. mtfit.scan_double_couples_floating under floating_l2norm with a shift range per station
     (Engine.linear_fit_candidates_floating_params, kiwi_hip_linear_fit_candidates_floating): per mechanism every station takes the
     shift under which it fits best; the planted mechanism and the planted delays come back.

Run on a machine with an MI355X:  python examples/invert_double_couple_station_shifts.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def main(nrec=12, L=1024, step=10, max_delay=4, noise=0.05, seed=1, verbose=True):
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
    true = np.array([0., 2000., -1000., 11000.] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
    delays = rng.integers(-max_delay, max_delay + 1, nrec)        # samples by which a station's data are late
    delays[0], delays[1] = max_delay, -max_delay
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            late = np.zeros(len(d) + 2 * max_delay, np.float32)   # the data cover the taper at every shift of the range
            late[max_delay + delays[ir]:max_delay + delays[ir] + len(d)] = d
            late += noise * np.abs(d).max() * rng.standard_normal(len(late)).astype(np.float32)
            e.set_ref_seismogram(ir + 1, k + 1, lo - max_delay, late)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    row = true.copy()
    e.set_misfit_method("l2norm")
    plain = mtfit.scan_double_couples(e, "moment_tensor", row, *mech, moment=PLANTED[3], outer_norm="l2norm")
    e.set_misfit_method("floating_l2norm")
    e.set_floating_shiftrange(0, -max_delay * dt, max_delay * dt)
    mtfit.scan_double_couples_floating(e, "moment_tensor", row, *mech, moment=PLANTED[3], outer_norm="l2norm")     # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.scan_double_couples_floating(e, "moment_tensor", row, *mech, moment=PLANTED[3], outer_norm="l2norm")
    t_scan = time.perf_counter() - t0
    ms = e.linear_fit_candidates_floating_ms()
    found = (res["strike"][0], res["dip"][0], res["rake"][0])
    shifts = np.rint(res["shifts"][0] / dt).astype(int)
    ok = found == PLANTED[:3] and np.array_equal(shifts, -delays)       # the reference moves back by the delay
    if verbose:
        nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
        print("%d mechanisms x %d stations x %d shifts from 6 syntheses: %.1f ms (evaluation %.2f, Gram and cross-correlation kernels "
              "%.2f, candidate kernels %.2f, downloads %.2f)" % ((nmech, nrec, 2 * max_delay + 1, 1e3 * t_scan) + ms))
        print("without shifts: strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (plain["strike"][0], plain["dip"][0], plain["rake"][0], plain["misfit"][0]))
        print("with shifts:    strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (found + (res["misfit"][0],)))
        print("planted delays [samples]:   %s" % " ".join("%3d" % v for v in delays))
        print("recovered delays [samples]: %s" % " ".join("%3d" % -v for v in shifts))
        print("planted mechanism and delays found" if ok else "planted mechanism or delays NOT found: planted strike %.0f, dip %.0f, rake %.0f" % PLANTED[:3])
    e.close()
    assert ok, "the floating scan did not return the planted mechanism and delays"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, max_delay=3) if small else main()) else 1)
