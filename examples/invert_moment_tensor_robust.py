#!/usr/bin/env python3
"""One station with gross noise: the moment tensor by the l2 fit against the l1 (robust) fit, on synthetic data.

  1. the setup of examples/invert_moment_tensor.py: synthetic Green's functions, a receiver ring, "observed" traces = the
     synthetics of a known `moment_tensor` source + a little noise;
  2. one station is buried in noise 20 x its signal -- a dead channel, a local storm, a wrong response;
  3. at the true location the tensor is fitted three times from the same six evaluations: l2norm inside and outside
     (Engine.linear_fit_params), l2norm inside with l1norm outside (the reference's default outer norm), and l1norm inside
     and outside (kiwi_hip_linear_fit_robust: iteratively reweighted least squares on the device).

Run on a machine with an MI355X:  python examples/invert_moment_tensor_robust.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, synthetic, mtfit  # noqa: E402


def main(nrec=12, L=1024, noise=0.02, bad_station=5, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=96, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=120e3, dspan=300e3)
    e = Engine(0)
    e.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    tensor = np.array(synthetic.mt_from_sdr(35., 60., 110., 7e18)) + np.array([1e18, 1e18, 1e18, 0, 0, 0])
    true = np.array([0., 2000., -1000., 11000.] + list(tensor) + [1.0], np.float32)
    e.set_source_params("moment_tensor", true[None, :])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        level = 20.0 if ir + 1 == bad_station else noise
        for k in range(3):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            e.set_ref_seismogram(ir + 1, k + 1, lo, d + level * np.abs(d).max() * rng.standard_normal(len(d)).astype(np.float32))
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), gf["dt"], ramp=8.0))
    e.set_keep_synthetics(0)
    fits = {}
    e.set_misfit_method("l2norm")
    fits["l2 fit (l2norm inside, l2norm outside)"] = mtfit.fit_moment_tensors(e, "moment_tensor", true)
    fits["l1 fit (l2norm inside, l1norm outside)"] = mtfit.fit_moment_tensors(e, "moment_tensor", true, outer_norm="l1norm")
    e.set_misfit_method("l1norm")
    fits["l1 fit (l1norm inside, l1norm outside)"] = mtfit.fit_moment_tensors(e, "moment_tensor", true, outer_norm="l1norm", niter=8, eps=1e-3)
    ms = e.linear_fit_robust_ms()
    errors = {}
    for name, (tensors, misfit, status, _) in fits.items():
        errors[name] = float(np.max(np.abs(tensors[0] - true[4:10])) / np.max(np.abs(true[4:10])))
        if verbose:
            print("%s: status %d, misfit %.4f, largest tensor error %.2g of the largest component" % (name, status[0], misfit[0], errors[name]))
            print("   fitted tensor [1e18 N m]: " + " ".join("%7.3f" % (v / 1e18) for v in tensors[0]))
    if verbose:
        print("   true tensor   [1e18 N m]: " + " ".join("%7.3f" % (v / 1e18) for v in true[4:10]))
        print("last call: evaluation %.2f ms, l2 start %.2f ms, reweighting passes %.2f ms, download %.2f ms" % ms)
    e.close()
    return errors


if __name__ == "__main__":
    main()
