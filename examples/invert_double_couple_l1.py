#!/usr/bin/env python3
"""The best double couple and depth under l1norm inside AND outside -- the fully robust search -- from SIX syntheses per depth.

  1. the setup of examples/invert_double_couple.py: synthetic Green's functions, a receiver ring, "observed" traces = the synthetics
     of a known double couple at a known depth + noise; one station's data are replaced by a glitch (a step many times the size
     of its signal), which is what the l1 norms are chosen against;
  2. mtfit.scan_double_couples_waveform (Engine.waveform_candidates_params, kiwi_hip_waveform_candidates): per trial depth the six
     elementary tensors are synthesised once, every mechanism of the grid is a combination of their kept traces, compared with the
     data sample by sample under l1norm, the receivers folded under l1norm; the planted mechanism and depth come back;
  3. the bootstrap over the receivers at the best depth through Engine.outer_misfits_slots on the call's own per-slot misfits;
  4. beside it the l2 / l2 answer of mtfit.scan_double_couples (the Gram route) on the same data: printed, not judged.

Run on a machine with an MI355X:  python examples/invert_double_couple_l1.py [--small]"""
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


def main(nrec=12, L=1024, step=10, depths=(7000., 9000., 11000., 13000., 15000.), noise=0.02, glitch=30.0, ndraw=200, seed=1, verbose=True):
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
    rows[:, 3] = depths
    e.set_misfit_method("l1norm")
    kw = dict(moment=PLANTED[3], outer_norm="l1norm", slot_misfit=True)
    mtfit.scan_double_couples_waveform(e, "moment_tensor", rows, *mech, **kw)      # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.scan_double_couples_waveform(e, "moment_tensor", rows, *mech, **kw)
    t_scan = time.perf_counter() - t0
    ms = e.waveform_candidates_ms()
    idep = int(np.nanargmin(res["misfit"]))
    found = (res["strike"][idep], res["dip"][idep], res["rake"][idep])
    # bootstrap over the receivers at the best depth: receiver weights drawn with replacement, the best mechanism of every draw
    scan = res["scan"]
    nmech = scan.slot_misfit.shape[1]
    slot_receiver = np.repeat(np.arange(nrec, dtype=np.int32), [len(c) for c in comps])
    draws = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), ndraw).astype(np.float64)
    bv, bi, _ = e.outer_misfits_slots(scan.slot_misfit[idep], np.tile(scan.slot_norm[idep], (nmech, 1)), slot_receiver, nrec,
                                      outer_norm="l1norm", draw_weights=draws)
    sdr = mtfit.double_couple_candidates(*mech)[1]
    mode = int(np.bincount(bi).argmax())
    # the same data under l2norm inside and outside, through the Gram sums
    e.set_misfit_method("l2norm")
    l2 = mtfit.scan_double_couples(e, "moment_tensor", rows, *mech, moment=PLANTED[3], outer_norm="l2norm")
    jdep = int(np.nanargmin(l2["misfit"]))
    ok = same_mechanism(found, PLANTED[:3]) and depths[idep] == true_depth and same_mechanism(tuple(sdr[mode]), PLANTED[:3])
    if verbose:
        print("%d depths x %d mechanisms from %d syntheses under l1norm inside and outside: %.1f ms (evaluation %.2f, slot kernel %.2f, "
              "fold kernels %.2f, downloads %.2f); station %d of %d is a glitch" % ((len(depths), nmech, 6 * len(depths), 1e3 * t_scan) + ms + (bad + 1, nrec)))
        for j, z in enumerate(depths):
            print("depth %6.0f m: strike %.0f, dip %.0f, rake %.0f, misfit %.4f%s" % (z, res["strike"][j], res["dip"][j], res["rake"][j], res["misfit"][j],
                                                                                       "   <- best" if j == idep else ""))
        print("bootstrap over the receivers, %d draws: mode strike %.0f, dip %.0f, rake %.0f in %d draws" % (
            ndraw, sdr[mode, 0], sdr[mode, 1], sdr[mode, 2], int(np.bincount(bi).max())))
        print("l2norm inside and outside on the same data: strike %.0f, dip %.0f, rake %.0f at %.0f m, misfit %.4f" % (
            l2["strike"][jdep], l2["dip"][jdep], l2["rake"][jdep], depths[jdep], l2["misfit"][jdep]))
        print("planted mechanism and depth found" if ok else "planted mechanism or depth NOT found: planted strike %.0f, dip %.0f, rake %.0f at %.0f m" % (
            PLANTED[:3] + (true_depth,)))
    e.close()
    assert ok, "the l1 scan did not return the planted mechanism and depth"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(9000., 11000., 13000.), ndraw=100) if small else main()) else 1)
