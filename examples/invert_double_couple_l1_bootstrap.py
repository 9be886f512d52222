#!/usr/bin/env python3
"""How sure are the double couple, the depth AND the origin time under l1norm inside and outside?  The bootstrap over the stations
of the whole search, on the device.

  1. the setup of examples/invert_double_couple_l1_timescan.py: synthetic Green's functions, a receiver ring, "observed" traces =
     the synthetics of a known double couple at a known depth and a known origin time + noise; one station's data are replaced by
     a glitch (a step many times the size of its signal);
  2. mtfit.bootstrap_double_couples_waveform (Engine.waveform_candidates_bootstrap_params,
     kiwi_hip_waveform_candidates_bootstrap): per trial depth the six elementary tensors are synthesised ONCE; the slot misfits of
     every (depth, origin time, mechanism) stay on the device, and every resampled draw of station weights finds its best of ALL
     of them -- not of the best depth only, as examples/invert_double_couple_l1.py has to;
  3. printed: how often each depth, each origin time and the planted mechanism win the draws.  Draw 0 is a row of ones, the plain
     search.

Run on a machine with an MI355X:  python examples/invert_double_couple_l1_bootstrap.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402
from kiwi_amd.engine import bootstrap_draw_weights  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def same_mechanism(a, b):
    ta, tb = (np.array(synthetic.mt_from_sdr(s, d, r, 1.0)) for s, d, r in (a, b))
    return np.max(np.abs(ta - tb)) <= 1e-6


def main(nrec=12, L=1024, step=10, depths=(7000., 9000., 11000., 13000., 15000.), offsets=(-10, 1, 21), late=4, noise=0.02, glitch=30.0,
         ndraw=200, seed=1, verbose=True):
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
    true_depth = depths[len(depths) // 2]
    k0, kstep, nk = offsets
    # the event happens `late` samples after the time the trial sources are given
    true = np.array([late * dt, 2000., -1000., true_depth] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    bad = 1                                  # the station whose data are a glitch
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            obs = d + noise * np.abs(d).max() * rng.standard_normal(len(d)).astype(np.float32)
            if ir == bad:
                obs = (glitch * np.abs(d).max() * (np.arange(len(d)) > len(d) // 3)).astype(np.float32)
            e.set_ref_seismogram(ir + 1, k + 1, lo, obs)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    rows = np.tile(true, (len(depths), 1))
    rows[:, 0] = 0.0
    rows[:, 3] = depths
    e.set_misfit_method("l1norm")
    dw = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw, rng)])
    kw = dict(k0=k0, kstep=kstep, nk=nk, outer_norm="l1norm", per_group=True)
    mtfit.bootstrap_double_couples_waveform(e, "moment_tensor", rows, *mech, PLANTED[3], dw[:2], **kw)      # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.bootstrap_double_couples_waveform(e, "moment_tensor", rows, *mech, PLANTED[3], dw, **kw)
    t_boot = time.perf_counter() - t0
    ms = e.waveform_candidates_bootstrap_ms()
    nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
    plain = (res["strike"][0], res["dip"][0], res["rake"][0])
    ok = bool(same_mechanism(plain, PLANTED[:3]) and depths[res["row"][0]] == true_depth and k0 + res["offset"][0] * kstep == late)
    draws = slice(1, None)
    has = res["row"][draws] >= 0
    nd = int(np.sum(has))
    right = np.array([r >= 0 and same_mechanism((s, d, k), PLANTED[:3])
                      for r, s, d, k in zip(res["row"][draws], res["strike"][draws], res["dip"][draws], res["rake"][draws])])
    depth_wins = int(np.sum(res["row"][draws][has] == depths.index(true_depth)))
    time_wins = int(np.sum(k0 + res["offset"][draws][has] * kstep == late))
    if verbose:
        print("%d draws x %d depths x %d origin times x %d mechanisms from %d syntheses under l1norm inside and outside: %.1f ms (evaluation "
              "%.2f, rows and scan kernels %.2f, fold kernels %.2f, bootstrap kernels %.2f, downloads %.2f); station %d of %d is a glitch" % (
                  (len(dw), len(depths), nk, nmech, 6 * len(depths), 1e3 * t_boot) + ms + (bad + 1, nrec)))
        print("draw of ones: strike %.0f, dip %.0f, rake %.0f at %.0f m, origin time %+.1f s, misfit %.4f" % (
            plain + (depths[res["row"][0]], res["time_shift"][0], res["misfit"][0])))
        for j, z in enumerate(depths):
            print("depth %6.0f m wins %3d of %d draws" % (z, int(np.sum(res["row"][draws][has] == j)), nd))
        for j in range(nk):
            n = int(np.sum(res["offset"][draws][has] == j))
            if n:
                print("origin time %+.1f s wins %3d of %d draws" % ((k0 + j * kstep) * dt, n, nd))
        print("planted depth wins %d, planted origin time %d, planted mechanism %d of %d draws" % (depth_wins, time_wins, int(np.sum(right)), nd))
        print("planted mechanism, depth and origin time found by the draw of ones" if ok else
              "planted mechanism, depth or origin time NOT found by the draw of ones: planted strike %.0f, dip %.0f, rake %.0f at %.0f m, %+.1f s" % (
                  PLANTED[:3] + (true_depth, late * dt)))
    e.close()
    assert ok, "the draw of ones did not return the planted mechanism, depth and origin time"
    assert 2 * depth_wins > nd and 2 * time_wins > nd, "the planted depth and origin time do not win most of the draws"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(9000., 11000., 13000.), offsets=(-4, 1, 9), ndraw=50) if small else main()) else 1)
