"""Best moment tensor per trial location by linear least squares.

The seismograms of a `moment_tensor` or `mt_eikonal` source are linear in the six tensor components (they enter the
centroid table as factors), so under the time-domain `l2norm` the global misfit is a quadratic form in the tensor and its
minimum a 6 x 6 solve.  `elementary_params` turns every trial row into six basis sources (unit tensors), which share their
geometry and run through the engine as one run of geometry-identical sources; `Engine.linear_fit_params` evaluates them,
forms the inner products between their synthetics on the device and solves (kiwi_hip_linear_fit)."""
import numpy as np

from .engine import SOURCE_TYPES
from .lib import KiwiHipError

# first tensor column (mxx, myy, mzz, mxy, mxz, myz follow each other) of the source types whose tensor is free
TENSOR_COLUMN = {6: 4, 5: 13}            # moment_tensor, mt_eikonal (source_moment_tensor.f90, source_mt_eikonal.f90:71-72)
COMPONENTS = ("mxx", "myy", "mzz", "mxy", "mxz", "myz")


def _tensor_column(sourcetype):
    st = SOURCE_TYPES.get(sourcetype, sourcetype)
    if st not in TENSOR_COLUMN:
        raise KiwiHipError("a free moment tensor needs the source type moment_tensor or mt_eikonal, not %s" % (sourcetype,))
    return st, TENSOR_COLUMN[st]


def elementary_params(sourcetype, params, unit=1e18):
    """Every row of params[N, nparams] repeated six times with the tensor columns replaced by `unit` x the six unit tensors
    (order mxx, myy, mzz, mxy, mxz, myz): [6 N, nparams] float32, the six basis sources of a row consecutive."""
    _, c0 = _tensor_column(sourcetype)
    p = np.atleast_2d(np.asarray(params, np.float32))
    out = np.repeat(p, 6, axis=0)
    out[:, c0:c0 + 6] = np.tile(np.eye(6, dtype=np.float32) * np.float32(unit), (len(p), 1))
    return out


# orthonormal basis of the trace-free tensors in the six-component order above: columns of T [6, 5]
_s2, _s6 = np.sqrt(0.5), np.sqrt(1.0 / 6.0)
DEVIATORIC_BASIS = np.array([[_s2, _s6, 0, 0, 0], [-_s2, _s6, 0, 0, 0], [0, -2 * _s6, 0, 0, 0],
                             [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1.]])


def _unpack(normal):
    G = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            G[i, j] = G[j, i] = normal[k]
            k += 1
    return G, np.array(normal[21:27]), float(normal[27])


def solve_deviatoric(normal):
    """Trace-free least squares from one row of `normal` (G upper triangle by rows, b, R of the six unit tensors), on the
    host in fp64: coefficients [6] with mxx + myy + mzz = 0, misfit, status (0 solved, 1 no solution), smallest Cholesky
    pivot of the unit-diagonal 5 x 5 matrix."""
    G, b, R = _unpack(normal)
    T = DEVIATORIC_BASIS
    G5, b5 = T.T @ G @ T, T.T @ b
    d = np.diag(G5)
    nan6 = np.full(6, np.nan)
    if not np.all(d > 0) or not R > 0:
        return nan6, np.nan, 1, 0.0
    s = 1.0 / np.sqrt(d)
    A = G5 * s[:, None] * s[None, :]
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return nan6, np.nan, 1, 0.0
    piv = float(np.min(np.diag(L)) ** 2)
    if not piv > 5 * 2.0 ** -52:
        return nan6, np.nan, 1, piv
    y = np.linalg.solve(L.T, np.linalg.solve(L, b5 * s)) * s
    x = T @ y
    val = R - 2.0 * x @ b + x @ G @ x
    return x, float(np.sqrt(max(val, 0.0) / R)), 0, piv


def fit_moment_tensors(engine, sourcetype, params, unit=1e18, deviatoric=False, receiver_weights=None, anarchy=False, piece=0,
                       outer_norm="l2norm", niter=8, eps=1e-3):
    """The best moment tensor of every row of params[N, nparams] (its own tensor columns are ignored) under the engine's
    references, tapers and filters, l2norm inside and outside.  Returns (tensors[N, 6] in N m, misfit[N] -- the global misfit
    of the fitted tensor --, status[N]: 0 solved, 1 no solution, 2 the row failed to discretise; pivot_min[N]: the smallest
    Cholesky pivot of the unit-diagonal normal matrix, small where the data do not resolve the tensor).  deviatoric=True
    solves the trace-free problem (mxx + myy + mzz = 0) on the host from the device's normal equations.
    outer_norm="l1norm", or an engine whose misfit method is l1norm: the robust fit (`Engine.linear_fit_robust_params`, `niter`
    reweighted solves with the relative bound `eps`) under the engine's method inside and `outer_norm` outside; status 3 then
    marks a reweighted system that broke down (the tensor of the iterate before), pivot_min is NaN, and deviatoric=True is
    refused (the host's trace-free solve works from l2 normal equations)."""
    p = np.atleast_2d(np.asarray(params, np.float32))
    if outer_norm != "l2norm" or getattr(engine, "misfit_method", "l2norm") != "l2norm":
        if deviatoric:
            raise KiwiHipError("fit_moment_tensors: deviatoric=True works from l2 normal equations; not available with a robust fit")
        fit = engine.linear_fit_robust_params(sourcetype, elementary_params(sourcetype, p, unit), 6, outer_norm=outer_norm,
                                              receiver_weights=receiver_weights, anarchy=anarchy, niter=niter, eps=eps, piece=piece)
        return fit.coef * float(unit), fit.misfit, fit.status, np.full(len(p), np.nan)
    fit = engine.linear_fit_params(sourcetype, elementary_params(sourcetype, p, unit), 6, receiver_weights=receiver_weights,
                                   anarchy=anarchy, normal=deviatoric, piece=piece)
    if not deviatoric:
        return fit.coef * float(unit), fit.misfit, fit.status, fit.pivot_min
    tensors, misfit = np.full((len(p), 6), np.nan), np.full(len(p), np.nan)
    status, pivot = np.array(fit.status, np.int32), np.zeros(len(p))
    for g in range(len(p)):
        if fit.status[g] == 2:
            continue
        x, m, st, piv = solve_deviatoric(fit.normal[g])
        tensors[g], misfit[g], status[g], pivot[g] = x * float(unit), m, st, piv
    return tensors, misfit, status, pivot


def fit_moment_tensors_time_scan(engine, sourcetype, params, k0, kstep, nk, unit=1e18, deviatoric=False, receiver_weights=None,
                                 anarchy=False, piece=0):
    """`fit_moment_tensors` at the origin-time offsets (k0 + j kstep) dt, j < nk, of every row of params[N, nparams], from the six
    syntheses per row of a single time (`Engine.linear_fit_time_scan_params`): the best moment tensor of every (row, offset).
    Returns (tensors[N, nk, 6] in N m, misfit[N, nk], status[N, nk], pivot_min[N, nk], best[N]): as `fit_moment_tensors` per
    offset, and the offset index of the smallest misfit among the solved offsets of a row, -1 where there is none.
    deviatoric=True solves the trace-free problem per offset on the host from the device's normal equations
    (`solve_deviatoric`); `best` then follows the trace-free misfits."""
    p = np.atleast_2d(np.asarray(params, np.float32))
    fit = engine.linear_fit_time_scan_params(sourcetype, elementary_params(sourcetype, p, unit), 6, k0, kstep, nk,
                                             receiver_weights=receiver_weights, anarchy=anarchy, normal=deviatoric, piece=piece)
    if not deviatoric:
        return fit.coef * float(unit), fit.misfit, fit.status, fit.pivot_min, fit.best
    nk = fit.status.shape[1]
    tensors, misfit = np.full((len(p), nk, 6), np.nan), np.full((len(p), nk), np.nan)
    status, pivot, best = np.array(fit.status, np.int32), np.zeros((len(p), nk)), np.full(len(p), -1, np.int32)
    for g in range(len(p)):
        for j in range(nk):
            if fit.status[g, j] == 2:
                continue
            x, m, st, piv = solve_deviatoric(fit.normal[g, j])
            tensors[g, j], misfit[g, j], status[g, j], pivot[g, j] = x * float(unit), m, st, piv
        ok = np.nonzero(status[g] == 0)[0]
        if len(ok):
            best[g] = ok[int(np.argmin(misfit[g][ok]))]
    return tensors, misfit, status, pivot, best


def double_couple_candidates(strikes, dips, rakes, moment=1.0):
    """The double couples over strikes x dips x rakes [degrees] (first axis slowest, the order of `synthetic.mt_sdr_grid`) with
    the scalar moment `moment`: (tensors [n, 6] float64 in COMPONENTS order -- `synthetic.mt_from_sdr`'s R m_unrot R^T with
    R = euler(dip, strike, -rake) --, sdr [n, 3] float64: the strike, dip and rake of every row)."""
    s, d, r = (np.asarray(list(a), np.float64) for a in (strikes, dips, rakes))
    sdr = np.stack([g.ravel() for g in np.meshgrid(s, d, r, indexing="ij")], axis=1)
    a, b, g = np.radians(sdr[:, 1]), np.radians(sdr[:, 0]), -np.radians(sdr[:, 2])
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    R = np.array([[cb * cg - ca * sb * sg, -cb * sg - ca * sb * cg, sa * sb],
                  [sb * cg + ca * cb * sg, -sb * sg + ca * cb * cg, -sa * cb],
                  [sa * sg, sa * cg, ca]]).transpose(2, 0, 1)
    mu = np.array([[0, 0, -1.], [0, 0, 0], [-1., 0, 0]])
    m = R @ mu @ R.transpose(0, 2, 1) * float(moment)
    return np.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2], m[:, 0, 1], m[:, 0, 2], m[:, 1, 2]], axis=1), sdr


def scan_double_couples(engine, sourcetype, params, strikes, dips, rakes, moment=None, outer_norm="l1norm", unit=1e18,
                        receiver_weights=None, anarchy=False, piece=0, cube=False, receiver_misfit=False):
    """The best double couple of every row of params[N, nparams] (its own tensor columns are ignored) over the grid strikes x
    dips x rakes, from the SIX syntheses of the row's elementary tensors (`Engine.linear_fit_candidates_params`): every
    mechanism of the grid is a combination of them, so no mechanism is synthesised.  moment=None: the best scalar moment of
    every mechanism is found on the way (outer l2norm only; it may come out negative: the opposite mechanism); otherwise all
    mechanisms have that moment [N m].  Returns a dict: strike, dip, rake, moment, misfit [N] of the best mechanism (NaN where
    there is none), index [N] its row in the grid (-1: none), status [N] (0 evaluated, 1 no data, 2 the row failed to
    discretise), tensor [N, 6] in N m and tensor_misfit [N]: the free tensor of `fit_moment_tensors` (l2norm) of the same
    row, scan: the `CandidateScan`; cube=True adds cube [N, ns, nd, nr], every mechanism's misfit (and moments, the same
    shape, where moment is None)."""
    p = np.atleast_2d(np.asarray(params, np.float32))
    free = moment is None
    if free and outer_norm != "l2norm":
        raise KiwiHipError("scan_double_couples: moment=None (the best moment per mechanism) needs outer_norm l2norm; give a moment")
    s, d, r = list(strikes), list(dips), list(rakes)
    cand, sdr = double_couple_candidates(s, d, r, 1.0 if free else float(moment) / float(unit))
    scan = engine.linear_fit_candidates_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, outer_norm=outer_norm,
                                               receiver_weights=receiver_weights, anarchy=anarchy, free_scale=free,
                                               misfit=cube or free, receiver_misfit=receiver_misfit, piece=piece)
    has = scan.best_index >= 0
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, None], sdr[at], np.nan)
    rows = np.arange(len(p))
    mom = np.where(has, scan.scale[rows, at] * float(unit) if free else float(moment), np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=mom, misfit=scan.best_misfit, index=scan.best_index,
               status=scan.status, tensor=scan.fit_coef * float(unit), tensor_misfit=scan.fit_misfit, scan=scan)
    if cube:
        out["cube"] = scan.misfit.reshape(len(p), len(s), len(d), len(r))
        if free:
            out["moments"] = (scan.scale * float(unit)).reshape(len(p), len(s), len(d), len(r))
    return out


def scan_double_couples_time_scan(engine, sourcetype, params, strikes, dips, rakes, k0, kstep, nk, moment=None, outer_norm="l1norm",
                                  unit=1e18, receiver_weights=None, anarchy=False, piece=0, cube=False, receiver_misfit=False):
    """`scan_double_couples` at the origin-time offsets (k0 + j kstep) dt, j < nk, of every row of params[N, nparams], from the SIX
    syntheses per row of a single time (`Engine.linear_fit_candidates_time_scan_params`): the best double couple AND origin time of
    every row.  moment as in `scan_double_couples` (None: the best scalar moment of every mechanism and offset, outer l2norm only).
    Returns a dict: strike, dip, rake, moment, misfit [N] of the best (mechanism, offset) (NaN where there is none), index [N] the
    mechanism's row in the grid and offset [N] the offset index (-1: none), status [N]; per offset strikes, dips_, rakes_, moments,
    misfits, indices [N, nk]: the best mechanism of every offset; tensor [N, nk, 6] in N m, tensor_misfit and tensor_status
    [N, nk]: the free tensor of `fit_moment_tensors_time_scan` per offset; scan: the `CandidateTimeScan`.  cube=True adds cube
    [N, ns, nd, nr]: every mechanism's smallest misfit over the offsets -- the mechanism cube with the origin time profiled out --,
    cube_offset, the same shape: the offset index of that minimum, and cube_moments where moment is None."""
    p = np.atleast_2d(np.asarray(params, np.float32))
    free = moment is None
    if free and outer_norm != "l2norm":
        raise KiwiHipError("scan_double_couples_time_scan: moment=None (the best moment per mechanism) needs outer_norm l2norm; give a moment")
    s, d, r = list(strikes), list(dips), list(rakes)
    cand, sdr = double_couple_candidates(s, d, r, 1.0 if free else float(moment) / float(unit))
    scan = engine.linear_fit_candidates_time_scan_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, k0, kstep, nk,
                                                         outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                         free_scale=free, marginal=cube, receiver_misfit=receiver_misfit, piece=piece)
    has = scan.best_index >= 0                                                  # [N, nk]
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, :, None], sdr[at], np.nan)                           # [N, nk, 3]
    moms = np.where(has, scan.best_scale * float(unit) if free else float(moment), np.nan)
    rows = np.arange(len(p))
    found = scan.best_offset >= 0
    j = np.where(found, scan.best_offset, 0)
    one = lambda a, none: np.where(found, a[rows, j], none)                     # noqa: E731
    out = dict(strike=one(pick[:, :, 0], np.nan), dip=one(pick[:, :, 1], np.nan), rake=one(pick[:, :, 2], np.nan), moment=one(moms, np.nan),
               misfit=one(scan.best_misfit, np.nan), index=one(scan.best_index, -1), offset=scan.best_offset, status=scan.status,
               strikes=pick[:, :, 0], dips_=pick[:, :, 1], rakes_=pick[:, :, 2], moments=moms, misfits=scan.best_misfit,
               indices=scan.best_index, tensor=scan.fit_coef * float(unit), tensor_misfit=scan.fit_misfit, tensor_status=scan.fit_status,
               scan=scan)
    if cube:
        shape = (len(p), len(s), len(d), len(r))
        out["cube"], out["cube_offset"] = scan.cand_misfit.reshape(shape), scan.cand_offset.reshape(shape)
        if free:
            out["cube_moments"] = (scan.cand_scale * float(unit)).reshape(shape)
    return out


def bootstrap_double_couples(engine, sourcetype, rows, strikes, dips, rakes, draw_weights, moment=1e18, k0=0, kstep=1, nk=1,
                             outer_norm="l1norm", unit=1e18, receiver_weights=None, anarchy=False, piece=0, per_group=False):
    """The bootstrap over the receivers of `scan_double_couples_time_scan`, joint over the rows of rows[N, nparams] (locations),
    the origin-time offsets (k0 + j kstep) dt, j < nk, and the grid strikes x dips x rakes, in ONE call on the device
    (`Engine.linear_fit_candidates_bootstrap_params`).  draw_weights [ndraw, nrec] as `engine.bootstrap_draw_weights` makes them;
    put a row of ones in front to get the plain winner as draw 0.  All mechanisms have the scalar moment `moment` [N m].  Returns a
    dict of arrays [ndraw]: row (index into `rows`), strike, dip, rake, offset (index j), index (the mechanism's row in the
    grid) and misfit of the best (row, offset, mechanism) of every draw -- -1 and NaN for a draw that excludes everything --;
    status [N]; boot: the `CandidateBootstrap`.  per_group=True adds rows_strike, rows_dip, rows_rake, rows_offset, rows_index and
    rows_misfit [N, ndraw]: the same per row, the depth profile under resampling."""
    p = np.atleast_2d(np.asarray(rows, np.float32))
    cand, sdr = double_couple_candidates(list(strikes), list(dips), list(rakes), float(moment) / float(unit))
    boot = engine.linear_fit_candidates_bootstrap_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, draw_weights, k0, kstep,
                                                         nk, outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                         per_group=per_group, piece=piece)

    def angles(cand_index):
        has = cand_index >= 0
        return np.where(has[..., None], sdr[np.where(has, cand_index, 0)], np.nan)
    pick = angles(boot.best_cand)
    out = dict(row=boot.best_group, strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], offset=boot.best_offset, index=boot.best_cand,
               misfit=boot.best_value, status=boot.status, boot=boot)
    if per_group:
        pick = angles(boot.group_cand)
        out.update(rows_strike=pick[..., 0], rows_dip=pick[..., 1], rows_rake=pick[..., 2], rows_offset=boot.group_offset,
                   rows_index=boot.group_cand, rows_misfit=boot.group_value)
    return out


def scan_double_couples_floating(engine, sourcetype, params, strikes, dips, rakes, moment, outer_norm="l1norm", unit=1e18,
                                 receiver_weights=None, anarchy=False, piece=0, cube=False, receiver_misfit=False):
    """`scan_double_couples` with per-receiver time shifts (`Engine.linear_fit_candidates_floating_params`): the engine's misfit
    method is floating_l2norm and every receiver has its own range of whole-sample shifts (`set_floating_shiftrange`); per
    mechanism every receiver takes the shift under which it fits best, still from the SIX syntheses of a row.  All mechanisms
    have the scalar moment `moment` [N m]; moment=None (the best moment per mechanism) is refused: the shifts that win depend on
    the scale, so it has no closed form.  Returns a dict: strike, dip, rake, moment, misfit [N] of the best mechanism (NaN where
    there is none), index [N] its row in the grid (-1: none), status [N] (0 evaluated, 1 no receiver counts, 2 the row failed to
    discretise), shifts [N, nrec]: the best mechanism's shift of every receiver in SECONDS (0 for receivers that do not count),
    scan: the `CandidateFloatingScan`; cube=True adds cube [N, ns, nd, nr], every mechanism's misfit, and cube_shifts
    [N, ns, nd, nr, nrec] in samples (int16)."""
    if moment is None:
        raise KiwiHipError("scan_double_couples_floating: moment=None (the best moment per mechanism) is not defined under "
                           "per-receiver shifts; give a moment")
    p = np.atleast_2d(np.asarray(params, np.float32))
    s, d, r = list(strikes), list(dips), list(rakes)
    cand, sdr = double_couple_candidates(s, d, r, float(moment) / float(unit))
    scan = engine.linear_fit_candidates_floating_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, outer_norm=outer_norm,
                                                        receiver_weights=receiver_weights, anarchy=anarchy, misfit=cube,
                                                        cand_shift=cube, receiver_misfit=receiver_misfit, piece=piece)
    has = scan.best_index >= 0
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, None], sdr[at], np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=np.where(has, float(moment), np.nan), misfit=scan.best_misfit,
               index=scan.best_index, status=scan.status, shifts=scan.best_shift * float(engine.dt), scan=scan)
    if cube:
        out["cube"] = scan.misfit.reshape(len(p), len(s), len(d), len(r))
        out["cube_shifts"] = scan.cand_shift.reshape(len(p), len(s), len(d), len(r), -1)
    return out


def bootstrap_double_couples_floating(engine, sourcetype, rows, strikes, dips, rakes, draw_weights, moment=1e18, outer_norm="l1norm",
                                      unit=1e18, receiver_weights=None, anarchy=False, piece=0, per_group=False):
    """The bootstrap over the receivers of `scan_double_couples_floating`, joint over the rows of rows[N, nparams] (locations) and
    the grid strikes x dips x rakes, in ONE call on the device (`Engine.linear_fit_candidates_floating_bootstrap_params`): the
    engine's misfit method is floating_l2norm and every receiver has its own range of whole-sample shifts.  draw_weights
    [ndraw, nrec] as `engine.bootstrap_draw_weights` makes them; put a row of ones in front to get the plain winner as draw 0.
    All mechanisms have the scalar moment `moment` [N m].  Returns a dict of arrays [ndraw]: row (index into `rows`), strike, dip,
    rake, moment, index (the mechanism's row in the grid) and misfit of the best (row, mechanism) of every draw -- -1 and NaN for
    a draw that excludes everything --; shifts [ndraw, nrec]: that winner's shift of every receiver in SECONDS (0 for receivers
    that do not count): how stable each station's delay is under resampling; status [N]; boot: the `CandidateFloatingBootstrap`.
    per_group=True adds rows_strike, rows_dip, rows_rake, rows_index, rows_misfit [N, ndraw] and rows_shifts [N, ndraw, nrec]: the
    same per row, the depth profile under resampling."""
    p = np.atleast_2d(np.asarray(rows, np.float32))
    cand, sdr = double_couple_candidates(list(strikes), list(dips), list(rakes), float(moment) / float(unit))
    boot = engine.linear_fit_candidates_floating_bootstrap_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, draw_weights,
                                                                  outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                                  per_group=per_group, piece=piece)

    def angles(cand_index):
        has = cand_index >= 0
        return np.where(has[..., None], sdr[np.where(has, cand_index, 0)], np.nan)
    pick = angles(boot.best_cand)
    out = dict(row=boot.best_group, strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2],
               moment=np.where(boot.best_cand >= 0, float(moment), np.nan), index=boot.best_cand, misfit=boot.best_value,
               shifts=boot.best_shift * float(engine.dt), status=boot.status, boot=boot)
    if per_group:
        pick = angles(boot.group_cand)
        out.update(rows_strike=pick[..., 0], rows_dip=pick[..., 1], rows_rake=pick[..., 2], rows_index=boot.group_cand,
                   rows_misfit=boot.group_value, rows_shifts=boot.group_shift * float(engine.dt))
    return out


def scan_double_couples_spectral(engine, sourcetype, params, strikes, dips, rakes, moment=None, outer_norm="l1norm", unit=1e18,
                                 receiver_weights=None, anarchy=False, piece=0, cube=False, slot_misfit=False):
    """`scan_double_couples` under the amplitude-spectrum norms (`Engine.spectral_candidates_params`): the engine's misfit method
    is ampspec_l2norm or ampspec_l1norm, and every mechanism of the grid is a combination of the complex spectra of the SIX
    syntheses of a row, compared in amplitude inside the receivers' pass bands.  moment=None: the best scalar moment of every
    mechanism is found on the way (ampspec_l2norm with outer l2norm only); otherwise all mechanisms have that moment [N m].
    Amplitude spectra leave the polarity open: a mechanism and its opposite (rake + 180) have the same misfit, the lower grid
    index is returned.  Returns a dict: strike, dip, rake, moment, misfit [N] of the best mechanism (NaN where there is none),
    index [N] its row in the grid (-1: none), status [N] (0 evaluated, 1 no receiver counts, 2 the row failed to discretise),
    scan: the `SpectralCandidateScan`; cube=True adds cube [N, ns, nd, nr], every mechanism's misfit (and moments, the same
    shape, where moment is None)."""
    p = np.atleast_2d(np.asarray(params, np.float32))
    free = moment is None
    if free and outer_norm != "l2norm":
        raise KiwiHipError("scan_double_couples_spectral: moment=None (the best moment per mechanism) needs outer_norm l2norm; give a moment")
    s, d, r = list(strikes), list(dips), list(rakes)
    cand, sdr = double_couple_candidates(s, d, r, 1.0 if free else float(moment) / float(unit))
    scan = engine.spectral_candidates_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, outer_norm=outer_norm,
                                             receiver_weights=receiver_weights, anarchy=anarchy, free_scale=free, misfit=cube or free,
                                             slot_misfit=slot_misfit, piece=piece)
    has = scan.best_index >= 0
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, None], sdr[at], np.nan)
    rows = np.arange(len(p))
    mom = np.where(has, scan.scale[rows, at] * float(unit) if free else float(moment), np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=mom, misfit=scan.best_misfit, index=scan.best_index,
               status=scan.status, scan=scan)
    if cube:
        out["cube"] = scan.misfit.reshape(len(p), len(s), len(d), len(r))
        if free:
            out["moments"] = (scan.scale * float(unit)).reshape(len(p), len(s), len(d), len(r))
    return out


def scan_double_couples_waveform(engine, sourcetype, rows, strikes, dips, rakes, moment, outer_norm="l1norm", unit=1e18,
                                 receiver_weights=None, anarchy=False, piece=0, cube=False, slot_misfit=False):
    """`scan_double_couples` under the time-domain l1norm inside (`Engine.waveform_candidates_params`): the engine's misfit method
    is l1norm (or l2norm, evaluated from the residual itself), and every mechanism of the grid is a combination of the kept
    traces of the SIX syntheses of a row, compared with the data sample by sample -- the fully robust search, l1 inside and
    outside, without a synthesis per mechanism.  moment [N m] is a number or a sequence: with a sequence the candidates are
    mechanisms x moments (the moment varies fastest).  moment=None (the best moment per mechanism) is refused: under l1norm the
    best scale of a direction has no closed form; the moment axis is more candidates.  Returns a dict: strike, dip, rake, moment,
    misfit [N] of the best candidate (NaN where there is none), index [N] its row among the candidates (-1: none), status [N]
    (0 evaluated, 1 no receiver counts, 2 the row failed to discretise), scan: the `WaveformCandidateScan`; cube=True adds cube
    [N, ns, nd, nr], every mechanism's misfit ([N, ns, nd, nr, nmoment] where moment is a sequence)."""
    if moment is None:
        raise KiwiHipError("scan_double_couples_waveform: moment=None (the best moment per mechanism) has no closed form under l1norm; "
                           "give a moment, or a sequence of moments as a further axis of candidates")
    p = np.atleast_2d(np.asarray(rows, np.float32))
    s, d, r = list(strikes), list(dips), list(rakes)
    moments = np.atleast_1d(np.asarray(moment, np.float64))
    mech, sdr = double_couple_candidates(s, d, r, 1.0)
    cand = (mech[:, None, :] * (moments / float(unit))[None, :, None]).reshape(-1, 6)
    scan = engine.waveform_candidates_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, outer_norm=outer_norm,
                                             receiver_weights=receiver_weights, anarchy=anarchy, misfit=cube, slot_misfit=slot_misfit,
                                             piece=piece)
    has = scan.best_index >= 0
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, None], sdr[at // len(moments)], np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=np.where(has, moments[at % len(moments)], np.nan),
               misfit=scan.best_misfit, index=scan.best_index, status=scan.status, scan=scan)
    if cube:
        shape = (len(p), len(s), len(d), len(r)) + ((len(moments),) if np.ndim(moment) else ())
        out["cube"] = scan.misfit.reshape(shape)
    return out


def scan_double_couples_waveform_floating(engine, sourcetype, rows, strikes, dips, rakes, moment, outer_norm="l1norm", unit=1e18,
                                          receiver_weights=None, anarchy=False, piece=0, cube=False, slot_misfit=False, bootstrap=None):
    """`scan_double_couples_waveform` with per-receiver time shifts (`Engine.waveform_candidates_floating_params`): the engine's
    misfit method is floating_l1norm (or floating_l2norm) and every receiver has its own range of whole-sample shifts
    (`set_floating_shiftrange`); per mechanism every receiver takes the shift under which the sum over its components is smallest,
    still from the SIX syntheses of a row -- l1 inside and outside against a glitched station, shifts against a mis-timed one.
    moment [N m] is a number or a sequence (mechanisms x moments, the moment fastest); moment=None is refused as in
    `scan_double_couples_waveform`.  Returns a dict: strike, dip, rake, moment, misfit [N] of the best candidate (NaN where there
    is none), index [N] its row among the candidates (-1: none), status [N] (0 evaluated, 1 no receiver counts, 2 the row failed
    to discretise), shifts [N, nrec]: the best candidate's shift of every receiver in SECONDS (0 for a disabled receiver), scan:
    the `WaveformCandidateFloatingScan`; cube=True adds cube [N, ns, nd, nr] ([N, ns, nd, nr, nmoment] where moment is a
    sequence) and cube_shifts, the same with a last axis nrec, in samples (int16).  bootstrap: draw weights [ndraw, nrec]
    (`engine.bootstrap_draw_weights`); adds boot_misfit and boot_index [N, ndraw], the best candidate of every row under every
    draw, through `Engine.outer_misfits_slots` on the scan's slot misfits (every candidate keeps the shifts it chose without weights)."""
    if moment is None:
        raise KiwiHipError("scan_double_couples_waveform_floating: moment=None (the best moment per mechanism) has no closed form under "
                           "l1norm or under shifts; give a moment, or a sequence of moments as a further axis of candidates")
    p = np.atleast_2d(np.asarray(rows, np.float32))
    s, d, r = list(strikes), list(dips), list(rakes)
    moments = np.atleast_1d(np.asarray(moment, np.float64))
    mech, sdr = double_couple_candidates(s, d, r, 1.0)
    cand = (mech[:, None, :] * (moments / float(unit))[None, :, None]).reshape(-1, 6)
    scan = engine.waveform_candidates_floating_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, outer_norm=outer_norm,
                                                      receiver_weights=receiver_weights, anarchy=anarchy, misfit=cube, cand_shift=cube,
                                                      slot_misfit=slot_misfit or bootstrap is not None, piece=piece)
    has = scan.best_index >= 0
    at = np.where(has, scan.best_index, 0)
    pick = np.where(has[:, None], sdr[at // len(moments)], np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=np.where(has, moments[at % len(moments)], np.nan),
               misfit=scan.best_misfit, index=scan.best_index, status=scan.status, shifts=scan.best_shift * float(engine.dt), scan=scan)
    if cube:
        shape = (len(p), len(s), len(d), len(r)) + ((len(moments),) if np.ndim(moment) else ())
        out["cube"] = scan.misfit.reshape(shape)
        out["cube_shifts"] = scan.cand_shift.reshape(shape + (-1,))
    if bootstrap is not None:
        draws = np.atleast_2d(np.asarray(bootstrap, np.float64))
        bm, bi = np.full((len(p), len(draws)), np.nan), np.full((len(p), len(draws)), -1, np.int32)
        nrec = len(engine.components)
        slot_receiver = np.repeat(np.arange(nrec, dtype=np.int32), [len(c) if engine.enabled[ir] else 0 for ir, c in enumerate(engine.components)])
        for g in range(len(p)):
            if scan.status[g] == 0:
                bv, ix, _ = engine.outer_misfits_slots(scan.slot_misfit[g], np.tile(scan.slot_norm[g], (len(cand), 1)), slot_receiver, nrec,
                                                       outer_norm, receiver_weights, anarchy, draws)
                bm[g], bi[g] = bv, np.where(bv == bv, ix, -1)
        out["boot_misfit"], out["boot_index"] = bm, bi
    return out


def scan_double_couples_waveform_time_scan(engine, sourcetype, rows, strikes, dips, rakes, moment, k0, kstep, nk, outer_norm="l1norm",
                                           unit=1e18, receiver_weights=None, anarchy=False, piece=0, cube=False, slot_misfit=False):
    """`scan_double_couples_waveform` at the nk origin times (k0 + j kstep) dt later than the rows' own, from the SIX syntheses of
    a row (`Engine.waveform_candidates_time_scan_params`): the best double couple, depth and origin time under l1norm inside and
    outside.  The engine's misfit method is l1norm (or l2norm); a receiver with a misfit filter is refused.  moment [N m] is a
    number or a sequence (mechanisms x moments, the moment fastest); moment=None is refused as in
    `scan_double_couples_waveform`.  Returns a dict: strike, dip, rake, moment, misfit [N] of the best (candidate, offset) (NaN
    where there is none), offset [N] its index j (-1: none) and time_shift [N] = (k0 + j kstep) dt in seconds, index [N] the
    candidate's row (-1: none), status [N] (0 evaluated, 1 no receiver counts, 2 the row failed to discretise), offsets_misfit
    [N, nk] the best misfit at every offset, scan: the `WaveformCandidateTimeScan`; cube=True adds cube [N, nk, ns, nd, nr]
    ([N, nk, ns, nd, nr, nmoment] where moment is a sequence), every candidate's misfit at every offset."""
    if moment is None:
        raise KiwiHipError("scan_double_couples_waveform_time_scan: moment=None (the best moment per mechanism) has no closed form under "
                           "l1norm; give a moment, or a sequence of moments as a further axis of candidates")
    p = np.atleast_2d(np.asarray(rows, np.float32))
    s, d, r = list(strikes), list(dips), list(rakes)
    moments = np.atleast_1d(np.asarray(moment, np.float64))
    mech, sdr = double_couple_candidates(s, d, r, 1.0)
    cand = (mech[:, None, :] * (moments / float(unit))[None, :, None]).reshape(-1, 6)
    scan = engine.waveform_candidates_time_scan_params(sourcetype, elementary_params(sourcetype, p, unit), 6, k0, kstep, nk, cand,
                                                       outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                       cand_misfit=False, cand_offset=False, misfit=cube, slot_misfit=slot_misfit, piece=piece)
    has = scan.best_offset >= 0
    jb = np.where(has, scan.best_offset, 0)
    n = np.arange(len(p))
    index = np.where(has, scan.best_index[n, jb], -1)
    at = np.where(has, index, 0)
    pick = np.where(has[:, None], sdr[at // len(moments)], np.nan)
    out = dict(strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=np.where(has, moments[at % len(moments)], np.nan),
               misfit=np.where(has, scan.best_misfit[n, jb], np.nan), offset=scan.best_offset,
               time_shift=np.where(has, (int(k0) + jb * int(kstep)) * float(engine.dt), np.nan), index=index, status=scan.status,
               offsets_misfit=scan.best_misfit, scan=scan)
    if cube:
        shape = (len(p), int(nk), len(s), len(d), len(r)) + ((len(moments),) if np.ndim(moment) else ())
        out["cube"] = scan.misfit.reshape(shape)
    return out


def bootstrap_double_couples_waveform(engine, sourcetype, rows, strikes, dips, rakes, moment, draw_weights, k0=0, kstep=1, nk=1,
                                      outer_norm="l1norm", unit=1e18, receiver_weights=None, anarchy=False, piece=0, per_group=False):
    """The bootstrap over the receivers of `scan_double_couples_waveform_time_scan`, joint over the rows of rows[N, nparams]
    (locations), the origin-time offsets (k0 + j kstep) dt, j < nk, and the grid strikes x dips x rakes (x moments), in ONE call on
    the device (`Engine.waveform_candidates_bootstrap_params`): l1norm inside and outside under resampling, the slot misfits never
    leaving the device.  The engine's misfit method is l1norm (or l2norm).  moment [N m] is a number or a sequence (mechanisms x
    moments, the moment fastest); moment=None is refused as in `scan_double_couples_waveform`.  draw_weights [ndraw, nrec] as
    `engine.bootstrap_draw_weights` makes them; put a row of ones in front to get the plain winner as draw 0.  Returns a dict of
    arrays [ndraw]: row (index into `rows`), strike, dip, rake, moment, offset (index j), time_shift [s], index (the candidate's
    row) and misfit of the best (row, offset, candidate) of every draw -- -1 and NaN for a draw that excludes everything --; status
    [N]; boot: the `CandidateBootstrap`.  per_group=True adds rows_strike, rows_dip, rows_rake, rows_moment, rows_offset, rows_index
    and rows_misfit [N, ndraw]: the same per row, the depth profile under resampling."""
    if moment is None:
        raise KiwiHipError("bootstrap_double_couples_waveform: moment=None (the best moment per mechanism) has no closed form under "
                           "l1norm; give a moment, or a sequence of moments as a further axis of candidates")
    p = np.atleast_2d(np.asarray(rows, np.float32))
    moments = np.atleast_1d(np.asarray(moment, np.float64))
    mech, sdr = double_couple_candidates(list(strikes), list(dips), list(rakes), 1.0)
    cand = (mech[:, None, :] * (moments / float(unit))[None, :, None]).reshape(-1, 6)
    boot = engine.waveform_candidates_bootstrap_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, draw_weights, k0, kstep,
                                                       nk, outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                       per_group=per_group, piece=piece)

    def picked(cand_index):
        has = cand_index >= 0
        at = np.where(has, cand_index, 0)
        return np.where(has[..., None], sdr[at // len(moments)], np.nan), np.where(has, moments[at % len(moments)], np.nan)
    pick, mom = picked(boot.best_cand)
    has = boot.best_offset >= 0
    out = dict(row=boot.best_group, strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=mom, offset=boot.best_offset,
               time_shift=np.where(has, (int(k0) + np.where(has, boot.best_offset, 0) * int(kstep)) * float(engine.dt), np.nan),
               index=boot.best_cand, misfit=boot.best_value, status=boot.status, boot=boot)
    if per_group:
        pick, mom = picked(boot.group_cand)
        out.update(rows_strike=pick[..., 0], rows_dip=pick[..., 1], rows_rake=pick[..., 2], rows_moment=mom, rows_offset=boot.group_offset,
                   rows_index=boot.group_cand, rows_misfit=boot.group_value)
    return out


def bootstrap_double_couples_spectral(engine, sourcetype, rows, strikes, dips, rakes, moment, draw_weights, outer_norm="l1norm",
                                      unit=1e18, receiver_weights=None, anarchy=False, piece=0, per_group=False):
    """The bootstrap over the receivers of `scan_double_couples_spectral`, joint over the rows of rows[N, nparams] (locations) and
    the grid strikes x dips x rakes (x moments), in ONE call on the device (`Engine.spectral_candidates_bootstrap_params`): the
    amplitude-spectrum norm inside, `outer_norm` outside under resampling, the slot misfits never leaving the device.  The
    engine's misfit method is ampspec_l2norm or ampspec_l1norm.  moment [N m] is a number or a sequence (mechanisms x moments, the
    moment fastest: the moment axis is more candidates); moment=None is refused, the best moment of a direction belongs to one
    fold, not to a resampled one.  Amplitude spectra leave the polarity open: a mechanism and its opposite (rake + 180) tie, the
    lower grid index is returned.  draw_weights [ndraw, nrec] as `engine.bootstrap_draw_weights` makes them; put a row of ones in
    front to get the plain winner as draw 0.  Returns a dict of arrays [ndraw]: row (index into `rows`), strike, dip, rake,
    moment, index (the candidate's row) and misfit of the best (row, candidate) of every draw -- -1 and NaN for a draw that
    excludes everything --; status [N]; boot: the `CandidateBootstrap`.  per_group=True adds rows_strike, rows_dip, rows_rake,
    rows_moment, rows_index and rows_misfit [N, ndraw]: the same per row, the depth profile under resampling."""
    if moment is None:
        raise KiwiHipError("bootstrap_double_couples_spectral: moment=None (the best moment per mechanism) is not resampled; give a "
                           "moment, or a sequence of moments as a further axis of candidates")
    p = np.atleast_2d(np.asarray(rows, np.float32))
    moments = np.atleast_1d(np.asarray(moment, np.float64))
    mech, sdr = double_couple_candidates(list(strikes), list(dips), list(rakes), 1.0)
    cand = (mech[:, None, :] * (moments / float(unit))[None, :, None]).reshape(-1, 6)
    boot = engine.spectral_candidates_bootstrap_params(sourcetype, elementary_params(sourcetype, p, unit), 6, cand, draw_weights,
                                                       outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                                       per_group=per_group, piece=piece)

    def picked(cand_index):
        has = cand_index >= 0
        at = np.where(has, cand_index, 0)
        return np.where(has[..., None], sdr[at // len(moments)], np.nan), np.where(has, moments[at % len(moments)], np.nan)
    pick, mom = picked(boot.best_cand)
    out = dict(row=boot.best_group, strike=pick[:, 0], dip=pick[:, 1], rake=pick[:, 2], moment=mom, index=boot.best_cand,
               misfit=boot.best_value, status=boot.status, boot=boot)
    if per_group:
        pick, mom = picked(boot.group_cand)
        out.update(rows_strike=pick[..., 0], rows_dip=pick[..., 1], rows_rake=pick[..., 2], rows_moment=mom, rows_index=boot.group_cand,
                   rows_misfit=boot.group_value)
    return out
