#!/usr/bin/env python3
"""Multi-time-window slip inversion of a planted two-asperity moment distribution, on synthetic data.

  1. synthetic Green's functions and a receiver ring as in examples/invert_moment_tensor.py;
  2. a fault plane of 4 x 4 patches of 10 km x 8 km, every patch with two rake directions (45 degrees either side of the
     true rake) and two time windows: K = 64 basis sources (kiwi_amd/slipfit.py patch_basis);
  3. "observed" traces = the synthetics of a planted moment distribution with two asperities + noise;
  4. the moments are fitted twice from the same 64 evaluations (kiwi_hip_linear_fit_wide): free coefficients without smoothing
     -- the solution oscillates between positive and negative moments many times the planted ones --, and non-negative
     coefficients with a Laplacian smoothing term (relative to the mean diagonal of the normal matrix; the problem is
     ill-conditioned, smallest pivot 1e-6, so 1e-4 is already felt and 1e-3 smears the asperities out), which recovers both.

Run on a machine with an MI355X:  python examples/invert_slip.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kiwi_amd import Engine, slipfit, synthetic  # noqa: E402

NX, NY, NWIN = 4, 4, 2
STRIKE, DIP, RAKE = 35.0, 20.0, 100.0
ASPERITIES = ((1, 0, 3.0e18), (2, 3, 2.0e18))            # (iy, ix, moment of the centre patch [N m])
UNIT = 1e18


def planted_moments():
    """[NY, NX, 2, NWIN] N m: per asperity the centre patch and 0.4 of it on its four neighbours; slip along the true rake
    (equal parts on the two rake directions, each 1 / sqrt(2) of the moment); 0.7 of it in the first window"""
    patch = np.zeros((NY, NX))
    for iy, ix, m0 in ASPERITIES:
        patch[iy, ix] += m0
        for jy, jx in ((iy - 1, ix), (iy + 1, ix), (iy, ix - 1), (iy, ix + 1)):
            if 0 <= jy < NY and 0 <= jx < NX:
                patch[jy, jx] += 0.4 * m0
    return patch[:, :, None, None] * np.sqrt(0.5) * np.array([0.7, 0.3])[None, None, None, :] * np.ones((1, 1, 2, 1))


def patch_map(moments):
    """[NY, NX]: the moment of every patch, summed over rakes and windows"""
    return moments.sum(axis=(2, 3))


def found_asperities(moments):
    """the largest patch, and the largest one outside its 3 x 3 neighbourhood: [(iy, ix), (iy, ix)]"""
    m = patch_map(moments).copy()
    a = np.unravel_index(np.argmax(m), m.shape)
    m[max(a[0] - 1, 0):a[0] + 2, max(a[1] - 1, 0):a[1] + 2] = -np.inf
    b = np.unravel_index(np.argmax(m), m.shape)
    return [(int(a[0]), int(a[1])), (int(b[0]), int(b[1]))]


def main(nrec=12, L=1024, noise=0.05, smoothing=1e-4, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    gf = synthetic.make_gfdb(nx=96, nz=6, L=L)
    lat, lon, depth, comps, dist = synthetic.make_receivers(nrec, dmin=130e3, dspan=280e3)
    e = Engine(0)
    e.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    e.set_effective_dt(0.5)
    e.set_local_interpolation("bilinear")
    e.set_receivers(lat, lon, depth, comps)
    e.set_source_location(40.0, 30.0, 0.0)
    rows = slipfit.patch_basis("moment_tensor", origin=(0., 0., 0., 11000.), strike=STRIKE, dip=DIP, rakes=(RAKE - 45., RAKE + 45.),
                               nx=NX, ny=NY, patch_length=10000., patch_width=8000., nwin=NWIN, window=2.0, rupture_velocity=2800.,
                               unit=UNIT)
    K = len(rows)
    planted = planted_moments()
    # the observed traces: the planted combination of the basis sources' synthetics + noise
    x0 = planted.reshape(-1) / UNIT
    used = np.flatnonzero(x0)
    e.set_source_params("moment_tensor", rows[used])
    e.set_keep_synthetics(1)
    e.eval()
    for ir in range(nrec):
        for k in range(3):
            lo, d = e.get_synthetics(0, ir + 1, k + 1, 1)
            d = x0[used[0]] * d.astype(np.float64)
            for i in range(1, len(used)):
                lo_i, d_i = e.get_synthetics(i, ir + 1, k + 1, 1)
                assert lo_i == lo and len(d_i) == len(d)
                d = d + x0[used[i]] * d_i
            d = d + noise * np.abs(d).max() * rng.standard_normal(len(d))
            e.set_ref_seismogram(ir + 1, k + 1, lo, d.astype(np.float32))
        e.set_misfit_taper(ir + 1, *synthetic.full_taper(lo, len(d), gf["dt"], ramp=8.0))
    e.set_keep_synthetics(0)
    e.set_misfit_method("l2norm")
    shape = (NY, NX, 2, NWIN)
    free, free_misfit, free_status, _ = slipfit.fit_slip(e, rows, K, smoothing=0.0, shape=shape, nonneg=False, unit=UNIT)
    smooth, misfit, status, fit = slipfit.fit_slip(e, rows, K, smoothing=smoothing, shape=shape, nonneg=True, unit=UNIT)
    ms = e.linear_fit_ms()
    e.close()
    result = dict(planted=planted, free=free, free_misfit=float(free_misfit[0]), free_status=int(free_status[0]), smooth=smooth,
                  misfit=float(misfit[0]), status=int(status[0]), npositive=int(fit.npositive[0]), nsolves=int(fit.nsolves[0]),
                  asperities=found_asperities(smooth))
    if verbose:
        def show(title, m):
            print(title)
            for row in patch_map(m) / 1e18:
                print("   " + " ".join("%7.2f" % v for v in row))
        show("planted moment per patch [1e18 N m] (rows: down dip, columns: along strike):", planted)
        show("free coefficients, no smoothing: status %d, misfit %.4f, %d of %d coefficients negative, most negative %.2f:" % (
            free_status[0], free_misfit[0], int(np.sum(free < 0)), K, free.min() / 1e18), free)
        show("non-negative coefficients, smoothing %g: status %d, misfit %.4f, %d positive, %d solves:" % (
            smoothing, status[0], misfit[0], fit.npositive[0], fit.nsolves[0]), smooth)
        print("asperities found at (down dip, along strike) %s, planted at %s" % (result["asperities"], [a[:2] for a in ASPERITIES]))
        print("total moment: planted %.3g, free %.3g, non-negative %.3g N m" % (planted.sum(), free.sum(), smooth.sum()))
        print("last call: evaluation %.2f ms, Gram and solve kernels %.2f ms, download %.2f ms" % ms)
    return result


if __name__ == "__main__":
    main()
