#!/usr/bin/env python3
"""Confidence on depth, mechanism AND station delays of a double couple whose stations are mis-timed, from ONE call: the joint
bootstrap over the receivers under floating_l2norm.

  1. the setup of examples/invert_double_couple_station_shifts.py: synthetic Green's functions, a receiver ring, "observed" traces =
     the synthetics of a known double couple at a planted depth + noise, every station's data late or early by its own whole number
     of samples;
  2. draw 0 of ones and the draws that resample the receivers (engine.bootstrap_draw_weights);
  3. mtfit.bootstrap_double_couples_floating(engine, ...): the six elementary tensors of every depth are synthesised once; per
     mechanism every station takes the shift under which it fits best; every draw's best (depth, mechanism) and that winner's
     shifts are found on the device (Engine.linear_fit_candidates_floating_bootstrap_params,
     kiwi_hip_linear_fit_candidates_floating_bootstrap): neither the [depth x mechanism, receiver] misfits nor the shifts of every
     candidate, which the host route downloads, are ever written;
  4. how often each (depth, mechanism) wins the resampled draws, and per station the spread of the winner's delay.

Run on a machine with an MI355X:  python examples/invert_double_couple_station_shifts_bootstrap.py [--small]"""
import collections
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402
from kiwi_amd.engine import bootstrap_draw_weights  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def main(nrec=12, L=1024, depths=(9000., 10000., 11000., 12000., 13000.), step=10, max_delay=4, ndraw=200, noise=0.05, seed=1, verbose=True):
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
    ip = len(depths) // 2 + 1                                 # the planted depth index
    true = np.array([0., 2000., -1000., depths[ip]] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
    delays = rng.integers(-max_delay, max_delay + 1, nrec)    # samples by which a station's data are late
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
    e.set_misfit_method("floating_l2norm")
    e.set_floating_shiftrange(0, -max_delay * dt, max_delay * dt)
    rows = np.tile(true, (len(depths), 1))
    rows[:, 3] = depths
    draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw, rng)])
    kw = dict(moment=PLANTED[3], outer_norm="l2norm", per_group=True)
    mtfit.bootstrap_double_couples_floating(e, "moment_tensor", rows, *mech, draws[:2], **kw)        # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.bootstrap_double_couples_floating(e, "moment_tensor", rows, *mech, draws, **kw)
    t_boot = time.perf_counter() - t0
    ms = e.linear_fit_candidates_floating_bootstrap_ms()
    d = slice(1, None)                                        # the resampled draws
    shifts = np.rint(res["shifts"] / dt).astype(int)          # [1 + ndraw, nrec]: the reference moves back by the delay
    wins = collections.Counter(zip(res["row"][d], res["strike"][d], res["dip"][d], res["rake"][d]))
    node = (ip,) + PLANTED[:3]
    modes = np.array([collections.Counter(-shifts[d, r]).most_common(1)[0][0] for r in range(nrec)])
    ok = 2 * wins[node] > ndraw and np.array_equal(modes, delays)
    if verbose:
        nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
        print("%d depths x %d mechanisms x %d shifts x %d draws over %d stations in one call: %.1f ms (evaluation %.2f, Gram and "
              "cross-correlation kernels %.2f, bootstrap kernels %.2f, downloads %.2f)" % (
                  (len(depths), nmech, 2 * max_delay + 1, len(draws), nrec, 1e3 * t_boot) + ms))
        print("draw 0 (all stations once): depth %.0f m, strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (
            depths[res["row"][0]], res["strike"][0], res["dip"][0], res["rake"][0], res["misfit"][0]))
        for (row, s, dd, r), n in wins.most_common(5):
            print("  depth %6.0f m, strike %.0f, dip %.0f, rake %.0f wins %d of %d draws" % (depths[row], s, dd, r, n, ndraw))
        print("station: planted delay, delay of draw 0, mode over the draws, share of the mode, spread [samples]")
        for r in range(nrec):
            got = -shifts[d, r]
            print("  %2d: %3d %3d %3d  %3.0f %%  %.2f" % (r + 1, delays[r], -shifts[0, r], modes[r], 100.0 * np.mean(got == modes[r]), np.std(got)))
        print("planted depth and mechanism win most draws, planted delays are the modes" if ok else
              "planted node or delays NOT found: planted depth index %d, strike %.0f, dip %.0f, rake %.0f" % node)
    e.close()
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(10000., 11000., 12000.), max_delay=3, ndraw=40) if small else main()) else 1)
