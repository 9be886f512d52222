#!/usr/bin/env python3
"""The best double couple, depth AND origin time under l1norm inside and outside, from SIX syntheses per depth.

  1. the setup of examples/invert_double_couple_l1.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known double couple at a known depth and a known origin time + noise; one station's data are replaced by a
     glitch (a step many times the size of its signal), which is what the l1 norms are chosen against;
  2. mtfit.scan_double_couples_waveform_time_scan (Engine.waveform_candidates_time_scan_params,
     kiwi_hip_waveform_candidates_time_scan): per trial depth the six elementary tensors are synthesised ONCE, at the trial time;
     every mechanism of the grid is a combination of their untapered rows, formed once per sample, read k samples earlier under
     the receivers' tapers for every origin-time offset k and compared with the data under l1norm, the receivers folded under
     l1norm; the planted mechanism, depth and origin time come back;
  3. beside it the l2 / l2 answer of mtfit.scan_double_couples_time_scan (the Gram route) on the same data: printed, not judged.

Run on a machine with an MI355X:  python examples/invert_double_couple_l1_timescan.py [--small]"""
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


def main(nrec=12, L=1024, step=10, depths=(7000., 9000., 11000., 13000., 15000.), offsets=(-10, 1, 21), late=4, noise=0.02, glitch=30.0,
         seed=1, verbose=True):
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
    kw = dict(outer_norm="l1norm")
    mtfit.scan_double_couples_waveform_time_scan(e, "moment_tensor", rows, *mech, PLANTED[3], k0, kstep, nk, **kw)      # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.scan_double_couples_waveform_time_scan(e, "moment_tensor", rows, *mech, PLANTED[3], k0, kstep, nk, **kw)
    t_scan = time.perf_counter() - t0
    ms = e.waveform_candidates_time_scan_ms()
    idep = int(np.nanargmin(res["misfit"]))
    found = (res["strike"][idep], res["dip"][idep], res["rake"][idep])
    nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
    # the same data under l2norm inside and outside, through the Gram sums
    e.set_misfit_method("l2norm")
    l2 = mtfit.scan_double_couples_time_scan(e, "moment_tensor", rows, *mech, k0, kstep, nk, moment=PLANTED[3], outer_norm="l2norm")
    jdep = int(np.nanargmin(l2["misfit"]))
    ok = same_mechanism(found, PLANTED[:3]) and depths[idep] == true_depth and k0 + res["offset"][idep] * kstep == late
    if verbose:
        print("%d depths x %d origin times x %d mechanisms from %d syntheses under l1norm inside and outside: %.1f ms (evaluation %.2f, rows and "
              "scan kernels %.2f, fold kernels %.2f, downloads %.2f); station %d of %d is a glitch" % (
                  (len(depths), nk, nmech, 6 * len(depths), 1e3 * t_scan) + ms + (bad + 1, nrec)))
        for j, z in enumerate(depths):
            print("depth %6.0f m: strike %.0f, dip %.0f, rake %.0f, origin time %+.1f s, misfit %.4f%s" % (
                z, res["strike"][j], res["dip"][j], res["rake"][j], res["time_shift"][j], res["misfit"][j], "   <- best" if j == idep else ""))
        print("l2norm inside and outside on the same data: strike %.0f, dip %.0f, rake %.0f at %.0f m, origin time %+.1f s, misfit %.4f" % (
            l2["strike"][jdep], l2["dip"][jdep], l2["rake"][jdep], depths[jdep], (k0 + l2["offset"][jdep] * kstep) * dt, l2["misfit"][jdep]))
        print("planted mechanism, depth and origin time found" if ok else
              "planted mechanism, depth or origin time NOT found: planted strike %.0f, dip %.0f, rake %.0f at %.0f m, %+.1f s" % (
                  PLANTED[:3] + (true_depth, late * dt)))
    e.close()
    assert ok, "the l1 time scan did not return the planted mechanism, depth and origin time"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(9000., 11000., 13000.), offsets=(-4, 1, 9)) if small else main()) else 1)
