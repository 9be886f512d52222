#!/usr/bin/env python3
"""The best double couple, depth and per-station time shifts under floating_l1norm -- a glitched station AND mis-timed stations at
once -- from SIX syntheses per depth.

  1. the setup of examples/invert_double_couple_l1.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known double couple at a known depth + noise; every station's data are late or early by its own whole number
     of samples (a velocity model that mis-times single stations), and one station's data are replaced by a glitch;
  2. mtfit.scan_double_couples_waveform_floating (Engine.waveform_candidates_floating_params,
     kiwi_hip_waveform_candidates_floating): per trial depth the six elementary tensors are synthesised once; every mechanism of the
     grid is a combination of their kept traces, and per mechanism every station slides its data inside its shift range and keeps
     the shift under which the l1 sum over its components is smallest; the receivers are folded under l1norm.  The planted
     mechanism, depth and delays come back;
  3. beside it what the two remedies answer alone on the same data -- mtfit.scan_double_couples_waveform (l1norm, no shifts) and
     mtfit.scan_double_couples_floating (floating_l2norm, the Gram route): printed, not judged.

Run on a machine with an MI355X:  python examples/invert_double_couple_l1_station_shifts.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402

PLANTED = (40., 60., 110., 7e18)


def same_mechanism(a, b):
    ta, tb = (np.array(synthetic.mt_from_sdr(s, d, r, 1.0)) for s, d, r in (a, b))
    return np.max(np.abs(ta - tb)) <= 1e-6


def main(nrec=12, L=1024, step=10, depths=(7000., 9000., 11000., 13000., 15000.), noise=0.02, glitch=30.0, max_delay=4, seed=1, verbose=True):
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
    true = np.array([0., 2000., -1000., true_depth] + list(synthetic.mt_from_sdr(*PLANTED)) + [0.5], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    bad = 1                                  # the station whose data are a glitch
    delays = rng.integers(-max_delay, max_delay + 1, nrec)      # samples by which a station's data are late
    pad = max_delay + 1
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            obs = np.zeros(len(d) + 2 * pad, np.float32)        # (padded: the data cover the taper at every shift of the range)
            obs[pad + delays[ir]:pad + delays[ir] + len(d)] = d
            obs += noise * np.abs(d).max() * rng.standard_normal(len(obs)).astype(np.float32)
            if ir == bad:
                obs = (glitch * np.abs(d).max() * (np.arange(len(obs)) > len(obs) // 3)).astype(np.float32)
            e.set_ref_seismogram(ir + 1, k + 1, lo - pad, obs)
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
    e.set_keep_synthetics(0)
    rows = np.tile(true, (len(depths), 1))
    rows[:, 3] = depths
    e.set_misfit_method("floating_l1norm")
    e.set_floating_shiftrange(0, -max_delay * dt, max_delay * dt)
    kw = dict(moment=PLANTED[3], outer_norm="l1norm")
    mtfit.scan_double_couples_waveform_floating(e, "moment_tensor", rows, *mech, **kw)      # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.scan_double_couples_waveform_floating(e, "moment_tensor", rows, *mech, **kw)
    t_scan = time.perf_counter() - t0
    ms = e.waveform_candidates_floating_ms()
    nmech = len(mtfit.double_couple_candidates(*mech)[1])
    idep = int(np.nanargmin(res["misfit"]))
    found = (res["strike"][idep], res["dip"][idep], res["rake"][idep])
    # the data of a station that is late by d samples fit best when they are moved back: shift -d
    good = np.arange(nrec) != bad
    shifts = np.rint(res["shifts"][idep] / dt).astype(int)
    ok = same_mechanism(found, PLANTED[:3]) and depths[idep] == true_depth and np.array_equal(shifts[good], -delays[good])
    # the two remedies alone
    e.set_floating_shiftrange(0, 0.0, 0.0)
    e.set_misfit_method("l1norm")
    l1 = mtfit.scan_double_couples_waveform(e, "moment_tensor", rows, *mech, **kw)
    e.set_misfit_method("floating_l2norm")
    e.set_floating_shiftrange(0, -max_delay * dt, max_delay * dt)
    l2 = mtfit.scan_double_couples_floating(e, "moment_tensor", rows, *mech, moment=PLANTED[3], outer_norm="l2norm")
    if verbose:
        print("%d depths x %d mechanisms x %d shifts per station from %d syntheses under floating_l1norm inside, l1norm outside: %.1f ms "
              "(evaluation %.2f, floating slot kernel %.2f, fold kernels %.2f, downloads %.2f); station %d of %d is a glitch" % (
                  (len(depths), nmech, 2 * max_delay + 1, 6 * len(depths), 1e3 * t_scan) + ms + (bad + 1, nrec)))
        for j, z in enumerate(depths):
            print("depth %6.0f m: strike %.0f, dip %.0f, rake %.0f, misfit %.4f%s" % (z, res["strike"][j], res["dip"][j], res["rake"][j], res["misfit"][j],
                                                                                       "   <- best" if j == idep else ""))
        print("planted delays [samples]:   %s" % " ".join("%3d" % d for d in delays))
        print("shifts found (= -delay):    %s   (station %d: the glitch)" % (" ".join("%3d" % s for s in shifts), bad + 1))
        for name, r in (("l1norm without shifts (scan_double_couples_waveform)", l1), ("floating_l2norm, Gram route (scan_double_couples_floating)", l2)):
            j = int(np.nanargmin(r["misfit"]))
            print("%s: strike %.0f, dip %.0f, rake %.0f at %.0f m, misfit %.4f" % (name, r["strike"][j], r["dip"][j], r["rake"][j], depths[j], r["misfit"][j]))
        print("planted mechanism, depth and delays found" if ok else "planted mechanism, depth or delays NOT found: planted strike %.0f, dip %.0f, "
              "rake %.0f at %.0f m" % (PLANTED[:3] + (true_depth,)))
    e.close()
    assert ok, "the floating_l1norm scan did not return the planted mechanism, depth and delays"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(9000., 11000., 13000.), max_delay=3) if small else main()) else 1)
