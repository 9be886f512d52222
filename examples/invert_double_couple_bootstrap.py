#!/usr/bin/env python3
"""Confidence on depth, origin time and mechanism of a double couple from ONE call: the joint bootstrap over the receivers.

  1. the setup of examples/invert_double_couple_timescan.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known double couple at a planted depth and origin time + noise;
  2. draw 0 of ones and 200 draws that resample the receivers (engine.bootstrap_draw_weights);
  3. mtfit.bootstrap_double_couples(engine, ...): the six elementary tensors of every depth are synthesised once, every mechanism
     strike x dip x rake at every origin time is evaluated from their inner products, and every draw's best (depth, time, mechanism)
     is found on the device (Engine.linear_fit_candidates_bootstrap_params, kiwi_hip_linear_fit_candidates_bootstrap): the
     [depth x time x mechanism, receiver] matrix the host route downloads and uploads again is never written;
  4. how often the planted depth, time and mechanism win, the spread of strike, dip and rake over the draws, and the depth profile
     under resampling: at every depth the misfit of its own best mechanism and time, draw by draw.

Run on a machine with an MI355X:  python examples/invert_double_couple_bootstrap.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402
from kiwi_amd.engine import bootstrap_draw_weights  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def main(nrec=12, L=1024, depths=(9000., 10000., 11000., 12000., 13000.), nk=21, step=10, ndraw=200, noise=0.05, seed=1, verbose=True):
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
    k0 = -(nk // 2)
    jp, ip = (2 * nk) // 3, len(depths) // 2 + 1              # the planted offset index and depth index
    true = np.array([(k0 + jp) * dt, 2000., -1000., depths[ip]] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
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
    rows = np.tile(true, (len(depths), 1))
    rows[:, 0], rows[:, 3] = 0.0, depths
    draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw, rng)])
    kw = dict(moment=PLANTED[3], k0=k0, kstep=1, nk=nk, outer_norm="l1norm", per_group=True)
    mtfit.bootstrap_double_couples(e, "moment_tensor", rows, *mech, draws[:2], **kw)        # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.bootstrap_double_couples(e, "moment_tensor", rows, *mech, draws, **kw)
    t_boot = time.perf_counter() - t0
    ms = e.linear_fit_candidates_bootstrap_ms()
    found = (int(res["row"][0]), int(res["offset"][0]), res["strike"][0], res["dip"][0], res["rake"][0])
    want = (ip, jp) + PLANTED[:3]
    d = slice(1, None)                                        # the resampled draws
    if verbose:
        nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
        print("%d depths x %d origin times x %d mechanisms x %d draws over %d receivers in one call: %.1f ms "
              "(evaluation %.2f, Gram-scan kernel %.2f, solve kernels %.2f, bootstrap kernels %.2f, downloads %.2f)" % (
                  (len(depths), nk, nmech, len(draws), nrec, 1e3 * t_boot) + ms))
        print("draw 0 (all receivers once): depth %.0f m, time %.2f s, strike %.0f, dip %.0f, rake %.0f, misfit %.4f" % (
            depths[found[0]], (k0 + found[1]) * dt, found[2], found[3], found[4], res["misfit"][0]))
        print("planted depth wins %d of %d draws, planted time %d, planted mechanism %d" % (
            int(np.sum(res["row"][d] == ip)), ndraw, int(np.sum(res["offset"][d] == jp)),
            int(np.sum((res["strike"][d] == PLANTED[0]) & (res["dip"][d] == PLANTED[1]) & (res["rake"][d] == PLANTED[2])))))
        print("spread of strike %.1f, dip %.1f, rake %.1f degrees (standard deviation over the draws); depth %.0f m, time %.3f s" % (
            np.std(res["strike"][d]), np.std(res["dip"][d]), np.std(res["rake"][d]), np.std(depths[res["row"][d]]),
            np.std((k0 + res["offset"][d]) * dt)))
        prof = res["rows_misfit"][:, d]
        for i, z in enumerate(depths):
            print("  depth %6.0f m: best misfit over time and mechanism %.4f (all receivers), %.4f +- %.4f over the draws" % (
                z, res["rows_misfit"][i, 0], np.mean(prof[i]), np.std(prof[i])))
        print("planted node found" if found == want else
              "planted node NOT found: planted depth index %d, offset index %d, strike %.0f, dip %.0f, rake %.0f" % want)
    e.close()
    return found == want


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(10000., 11000., 12000.), nk=7, ndraw=40) if small else main()) else 1)
