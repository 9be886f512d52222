"""Multi-time-window slip inversion: the moment of every patch of a fault plane in every time window by linear least squares
with non-negative coefficients and a smoothing term.

A fault plane is cut into nx x ny patches; a patch, a rake direction and a time window make one basis source (a
`moment_tensor` point source at the patch centre with the double-couple tensor of strike, dip and that rake, its time the
rupture delay of the patch plus the window offset, its rise time the window length).  The seismogram is linear in the moments
of the basis sources, which must not be negative; `Engine.linear_fit_wide_params` (kiwi_hip_linear_fit_wide) evaluates the
K = nx ny nrake nwin basis sources, forms their inner products and runs the active-set solve on the device.

Order of the basis sources, everywhere in this module: patch row iy (down dip) slowest, then ix (along strike), then the rake,
then the window: index ((iy nx + ix) nrake + irake) nwin + iwin -- a moment array is [ny, nx, nrake, nwin]."""
import numpy as np

from . import synthetic
from .lib import KiwiHipError


def patch_centres(origin, strike, dip, nx, ny, patch_length, patch_width):
    """(north [ny, nx], east, depth, along-strike offset, down-dip offset) of the patch centres of a plane centred on
    origin = (time, north, east, depth)"""
    s, d = np.radians(strike), np.radians(dip)
    xs = (np.arange(nx) - 0.5 * (nx - 1)) * float(patch_length)
    yd = (np.arange(ny) - 0.5 * (ny - 1)) * float(patch_width)
    X, Y = np.meshgrid(xs, yd)                                   # [ny, nx]
    north = origin[1] + X * np.cos(s) - Y * np.cos(d) * np.sin(s)
    east = origin[2] + X * np.sin(s) + Y * np.cos(d) * np.cos(s)
    depth = origin[3] + Y * np.sin(d)
    return north, east, depth, X, Y


def patch_basis(sourcetype="moment_tensor", origin=(0., 0., 0., 10000.), strike=0., dip=90., rakes=(0.,), nx=1, ny=1,
                patch_length=1000., patch_width=1000., nwin=1, window=1., rupture_velocity=3000., unit=1e18):
    """Parameter rows [K, 11] float32 of the K = nx ny len(rakes) nwin basis sources (order: module docstring): point sources
    at the patch centres of a plane centred on origin = (time, north-shift, east-shift, depth), rupturing from there at
    `rupture_velocity`; moment `unit` N m each, time = origin time + distance from the origin / rupture_velocity + iwin window,
    rise time = window."""
    if sourcetype not in ("moment_tensor", 6):
        raise KiwiHipError("patch_basis: the basis sources are moment_tensor point sources, not %s" % (sourcetype,))
    rakes = np.atleast_1d(np.asarray(rakes, np.float64))
    if nx < 1 or ny < 1 or nwin < 1 or len(rakes) < 1:
        raise KiwiHipError("patch_basis: need at least one patch, one rake and one window")
    north, east, depth, X, Y = patch_centres(origin, strike, dip, nx, ny, patch_length, patch_width)
    delay = np.sqrt(X * X + Y * Y) / float(rupture_velocity)
    tensors = [synthetic.mt_from_sdr(strike, dip, r, m0=unit) for r in rakes]
    rows = np.zeros((ny, nx, len(rakes), nwin, 11), np.float32)
    for iw in range(nwin):
        rows[:, :, :, iw, 0] = (origin[0] + delay + iw * float(window))[:, :, None]
    rows[..., 1] = north[:, :, None, None]
    rows[..., 2] = east[:, :, None, None]
    rows[..., 3] = depth[:, :, None, None]
    for ir, t in enumerate(tensors):
        rows[:, :, ir, :, 4:10] = np.asarray(t, np.float32)
    rows[..., 10] = float(window)
    return rows.reshape(-1, 11)


def laplacian_matrix(nx, ny):
    """D [nx ny, nx ny]: the 5-point Laplacian of a [ny, nx] grid, patch iy nx + ix; a patch at the rim counts the
    neighbours it has, so that constants are in the null space"""
    D = np.zeros((nx * ny, nx * ny))
    for iy in range(ny):
        for ix in range(nx):
            p = iy * nx + ix
            for jy, jx in ((iy - 1, ix), (iy + 1, ix), (iy, ix - 1), (iy, ix + 1)):
                if 0 <= jy < ny and 0 <= jx < nx:
                    D[p, jy * nx + jx] = 1.0
                    D[p, p] -= 1.0
    return D


def laplacian_penalty(nx, ny, nrake=1, nwin=1):
    """Upper triangle by rows [K (K + 1) / 2] of D^T D, with D the 5-point Laplacian within each (rake, window) layer, in the
    order of the basis sources: the `penalty` of `Engine.linear_fit_wide`."""
    D = laplacian_matrix(nx, ny)
    layers = nrake * nwin
    K = nx * ny * layers
    full = np.zeros((K, K))
    for q in range(layers):
        idx = np.arange(nx * ny) * layers + q
        full[np.ix_(idx, idx)] = D
    P = full.T @ full
    P = 0.5 * (P + P.T)
    return np.ascontiguousarray(P[np.triu_indices(K)])


def fit_slip(engine, rows, K, smoothing=0.0, shape=None, nonneg=True, unit=1e18, sourcetype="moment_tensor", receiver_weights=None,
             anarchy=False, piece=0):
    """The moments of the basis sources `rows` [ngroup K, nparams] (every K consecutive rows one fault model, `patch_basis`)
    under the engine's references and tapers.  shape = (ny, nx, nrake, nwin) with ny nx nrake nwin = K; smoothing > 0 adds
    smoothing x the mean diagonal of the normal matrix x `laplacian_penalty`.  Returns (moments [ngroup, ny, nx, nrake, nwin]
    in N m -- [ny, nx, nrake, nwin] for one group --, misfit [ngroup]: the data misfit, status [ngroup]: 0 solved, 1 no
    solution, 2 a basis source failed to discretise, 4 the cap of 3 K solves was reached; the `WideFit`)."""
    K = int(K)
    if shape is None:
        shape = (1, K, 1, 1)
    ny, nx, nrake, nwin = (int(v) for v in shape)
    if ny * nx * nrake * nwin != K:
        raise KiwiHipError("fit_slip: shape %s does not hold K = %d basis sources" % (tuple(shape), K))
    penalty = None
    if smoothing:
        if not smoothing > 0:
            raise KiwiHipError("fit_slip: smoothing must not be negative")
        penalty = float(smoothing) * laplacian_penalty(nx, ny, nrake, nwin)
    fit = engine.linear_fit_wide_params(sourcetype, rows, K, receiver_weights=receiver_weights, anarchy=anarchy, nonneg=nonneg,
                                        penalty=penalty, penalty_relative=True, piece=piece)
    moments = (fit.coef * float(unit)).reshape(-1, ny, nx, nrake, nwin)
    return (moments[0] if len(moments) == 1 else moments), fit.misfit, fit.status, fit
