#!/usr/bin/env python3
"""How sure are the double couple AND the depth under an amplitude-spectrum norm inside a pass band?  The bootstrap over the
stations of the whole search, on the device.

  1. the setup of examples/invert_double_couple_ampspec.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known double couple at a known depth + noise; every receiver has a pass-band filter and the misfit method is
     ampspec_l2norm;
  2. mtfit.bootstrap_double_couples_spectral (Engine.spectral_candidates_bootstrap_params,
     kiwi_hip_spectral_candidates_bootstrap): per trial depth the six elementary tensors are synthesised and transformed ONCE; the
     slot misfits of every (depth, mechanism) stay on the device, and every resampled draw of station weights finds its best of
     ALL of them -- not of the best depth only, as examples/invert_double_couple_ampspec.py has to;
  3. printed: how often each depth and each mechanism win the draws.  Draw 0 is a row of ones, the plain search.

Amplitude spectra leave the polarity open: a mechanism and its opposite have the same misfit and the lower grid index is returned,
so the wins are counted up to the polarity.

Run on a machine with an MI355X:  python examples/invert_double_couple_ampspec_bootstrap.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402
from kiwi_amd.engine import bootstrap_draw_weights  # noqa: E402

PLANTED = (40., 60., 110., 7e18)
CORNERS = (0.05, 0.1, 0.3, 0.4)          # pass band, of Nyquist


def same_up_to_sign(a, b):
    ta, tb = (np.array(synthetic.mt_from_sdr(s, d, r, 1.0)) for s, d, r in (a, b))
    return min(np.max(np.abs(ta - tb)), np.max(np.abs(ta + tb))) <= 1e-6


def main(nrec=12, L=1024, step=10, depths=(7000., 9000., 11000., 13000., 15000.), noise=0.02, ndraw=200, seed=1, verbose=True):
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
    band = ([c * 0.5 / dt for c in CORNERS], [0., 1., 1., 0.])
    for ir in range(nrec):
        for k in range(len(comps[ir])):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + noise * np.abs(d).max() * rng.standard_normal(len(d)).astype(np.float32))
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), dt, ramp=8.0))
        e.set_misfit_filter(ir + 1, *band)
    e.set_keep_synthetics(0)
    e.set_misfit_method("ampspec_l2norm")
    rows = np.tile(true, (len(depths), 1))
    rows[:, 3] = depths
    dw = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, ndraw - 1, rng)])
    kw = dict(outer_norm="l2norm", per_group=True)
    mtfit.bootstrap_double_couples_spectral(e, "moment_tensor", rows, *mech, PLANTED[3], dw[:2], **kw)      # (first call: code objects)
    t0 = time.perf_counter()
    res = mtfit.bootstrap_double_couples_spectral(e, "moment_tensor", rows, *mech, PLANTED[3], dw, **kw)
    t_boot = time.perf_counter() - t0
    ms = e.spectral_candidates_bootstrap_ms()
    nmech = len(mech[0]) * len(mech[1]) * len(mech[2])
    plain = (res["strike"][0], res["dip"][0], res["rake"][0])
    ok = bool(same_up_to_sign(plain, PLANTED[:3]) and depths[res["row"][0]] == true_depth)
    draws = slice(1, None)
    has = res["row"][draws] >= 0
    nd = int(np.sum(has))
    wins = {}
    for r, s, d, k in zip(res["row"][draws][has], res["strike"][draws][has], res["dip"][draws][has], res["rake"][draws][has]):
        wins[(depths[r], s, d, k)] = wins.get((depths[r], s, d, k), 0) + 1
    right = sum(n for (z, s, d, k), n in wins.items() if same_up_to_sign((s, d, k), PLANTED[:3]))
    depth_wins = int(np.sum(res["row"][draws][has] == depths.index(true_depth)))
    if verbose:
        print("%d draws x %d depths x %d mechanisms from %d syntheses under ampspec_l2norm in a pass band: %.1f ms (evaluation %.2f, spectra "
              "kernel %.2f, slot kernel %.2f, bootstrap kernels %.2f, downloads %.2f)" % ((len(dw), len(depths), nmech, 6 * len(depths), 1e3 * t_boot) + ms))
        print("draw of ones: strike %.0f, dip %.0f, rake %.0f at %.0f m, misfit %.4f" % (plain + (depths[res["row"][0]], res["misfit"][0])))
        for j, z in enumerate(depths):
            print("depth %6.0f m wins %3d of %d draws" % (z, int(np.sum(res["row"][draws][has] == j)), nd))
        for (z, s, d, k), n in sorted(wins.items(), key=lambda kv: -kv[1])[:8]:
            print("strike %3.0f, dip %2.0f, rake %4.0f at %6.0f m wins %3d of %d draws%s" % (
                s, d, k, z, n, nd, "  (the planted one, up to the polarity)" if same_up_to_sign((s, d, k), PLANTED[:3]) and z == true_depth else ""))
        print("planted depth wins %d, planted mechanism (up to the polarity) %d of %d draws" % (depth_wins, right, nd))
        print("planted mechanism and depth found by the draw of ones" if ok else
              "planted mechanism or depth NOT found by the draw of ones: planted strike %.0f, dip %.0f, rake %.0f at %.0f m" % (
                  PLANTED[:3] + (true_depth,)))
    e.close()
    assert ok, "the draw of ones did not return the planted mechanism and depth"
    assert 2 * depth_wins > nd, "the planted depth does not win most of the draws"
    return ok


if __name__ == "__main__":
    small = "--small" in sys.argv[1:]
    sys.exit(0 if (main(nrec=6, L=512, depths=(9000., 11000., 13000.), ndraw=50) if small else main()) else 1)
