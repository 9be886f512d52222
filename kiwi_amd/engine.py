"""Python host side of the C-ABI: one ``Engine`` == one ``minimizer`` process of the reference.

Method names follow the reference's stdin commands / minimizer_engine procedures
(minimizer.f90:1729-1811) so that the calling code reads like python/tunguska/seismosizer.py;
``make_misfits_for_sources`` and ``make_global_misfits`` restate the two Python functions that sit
directly on the path (seismosizer.py:682-722, 843-922)."""
import collections
import ctypes as C

import numpy as np

from . import lib as _lib
from .lib import KiwiHipError, c_float_p, c_int_p, c_double_p

SOURCE_TYPES = {"bilateral": 1, "circular": 2, "point_lp": 3, "eikonal": 4, "mt_eikonal": 5,
                "moment_tensor": 6}          # source_all.f90:88-98
NORMS = {"l2norm": 1, "l1norm": 2, "ampspec_l2norm": 3, "ampspec_l1norm": 4, "scalar_product": 5,
         "peak": 6, "floating_l2norm": 7, "floating_l1norm": 8}      # comparator.f90:137-146

LinearFit = collections.namedtuple("LinearFit", "coef misfit status pivot_min normal by_receiver")
RobustFit = collections.namedtuple("RobustFit", "coef misfit status trace")
ScanFit = collections.namedtuple("ScanFit", "coef misfit status pivot_min best normal")
CandidateScan = collections.namedtuple("CandidateScan", "best_index best_misfit status misfit scale receiver_misfit receiver_norm "
                                                        "fit_coef fit_misfit")
CandidateFloatingScan = collections.namedtuple("CandidateFloatingScan", "best_index best_misfit status best_shift misfit cand_shift "
                                                                        "receiver_misfit receiver_norm")
CandidateTimeScan = collections.namedtuple("CandidateTimeScan", "best_offset best_index best_misfit best_scale status cand_misfit cand_offset "
                                                                "cand_scale misfit scale receiver_misfit receiver_norm fit_coef fit_misfit "
                                                                "fit_status")
CandidateBootstrap = collections.namedtuple("CandidateBootstrap", "best_value best_group best_offset best_cand status group_value group_offset "
                                            "group_cand")
CandidateFloatingBootstrap = collections.namedtuple("CandidateFloatingBootstrap", "best_value best_group best_cand best_shift status group_value "
                                                    "group_cand group_shift")
SpectralCandidateScan = collections.namedtuple("SpectralCandidateScan", "best_index best_misfit status misfit scale slot_misfit slot_norm "
                                                                        "spectra spectra_range spectra_ref")
WaveformCandidateScan = collections.namedtuple("WaveformCandidateScan", "best_index best_misfit status misfit slot_misfit slot_norm")
WaveformCandidateFloatingScan = collections.namedtuple("WaveformCandidateFloatingScan",
                                                       "best_index best_misfit status best_shift misfit cand_shift slot_misfit slot_norm")
WaveformCandidateTimeScan = collections.namedtuple("WaveformCandidateTimeScan",
                                                   "best_offset best_index best_misfit status cand_misfit cand_offset misfit slot_misfit "
                                                   "slot_norm rows shift_halo row_offset")
WideFit = collections.namedtuple("WideFit", "coef misfit status pivot_min normal by_receiver npositive nsolves")

GEOREC = np.dtype([("row", np.int32, 4), ("w", np.float32, 4), ("ishift", np.int32), ("wfrac", np.float32),
                   ("f", np.float32, 6), ("cl", np.float32), ("sl", np.float32), ("flags", np.int32),
                   ("pad", np.int32)])


def _pointer(ctype):
    """array -> pointer of that type for a call; None -> None (NULL: an input left out, an output not asked for)"""
    return lambda a: None if a is None else a.ctypes.data_as(ctype)


_fp, _ip, _dp, _sp = _pointer(c_float_p), _pointer(c_int_p), _pointer(c_double_p), _pointer(C.POINTER(C.c_short))

_K_RANGE = "%s: K = %d basis sources per group; 1 to %d are supported"


def _outer_code(outer_norm):
    code = {"l1norm": 1, "l2norm": 2}.get(outer_norm)
    if code is None:
        raise KiwiHipError("unknown norm method: %s" % outer_norm)
    return code


def discretize(sourcetype, params, effective_dt):
    """psm_set + psm_to_tdsm on the host (kiwi_hip_discretize): (centroids[n,10], moment, risetime)."""
    L = _lib.load()
    st = SOURCE_TYPES.get(sourcetype, sourcetype)
    p = np.ascontiguousarray(params, np.float32)
    n, mo, ri = C.c_int(), C.c_float(), C.c_float()
    rc = L.kiwi_hip_discretize(st, _fp(p), len(p), effective_dt, None, 0, C.byref(n), C.byref(mo), C.byref(ri))
    if rc != 0:
        raise KiwiHipError("discretize failed (rc=%d): unsupported source type or wrong parameter count" % rc)
    cent = np.zeros((n.value, 10), np.float32)
    rc = L.kiwi_hip_discretize(st, _fp(p), len(p), effective_dt, _fp(cent), n.value, C.byref(n), C.byref(mo),
                               C.byref(ri))
    if rc != 0:
        raise KiwiHipError("discretize failed (rc=%d)" % rc)
    return cent, mo.value, ri.value


def principal_axes(sourcetype, params):
    """`get_principal_axes`: ((P azimuth, P polar angle), (T azimuth, T polar angle)) in degrees; bilateral sources only."""
    L = _lib.load()
    p = np.ascontiguousarray(params, np.float32)
    pax, tax = np.zeros(2, np.float32), np.zeros(2, np.float32)
    if L.kiwi_hip_principal_axes(SOURCE_TYPES[sourcetype], _fp(p), _fp(pax), _fp(tax)) != 0:
        raise KiwiHipError("principal axes are defined for bilateral sources only")
    return pax, tax


def pack_crust_profile(vp, vs, rho, thickness):
    """t_crust2x2_1d_profile (crust2x2.f90:45-50) as the 31 floats the C-ABI takes."""
    out = np.concatenate([np.asarray(vp, np.float32), np.asarray(vs, np.float32), np.asarray(rho, np.float32),
                          np.asarray(thickness, np.float32)])
    if out.shape != (31,):
        raise KiwiHipError("a crust profile is vp[8], vs[8], rho[8], thickness[7]")
    return np.ascontiguousarray(out)


_EIKONAL_ERRORS = {5: "Empty rupture area", 6: "position of nucleation point is outside of rupture region"}


def discretize_eikonal(sourcetype, params, effective_dt, rupture_profile, con_points, con_normals):
    """psm_set + psm_to_tdsm of `eikonal` / `mt_eikonal` (kiwi_hip_discretize_eikonal)."""
    L = _lib.load()
    st = SOURCE_TYPES.get(sourcetype, sourcetype)
    p = np.ascontiguousarray(params, np.float32)
    prof = np.ascontiguousarray(rupture_profile, np.float32)
    pts = np.ascontiguousarray(con_points, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(con_normals, np.float32).reshape(-1, 3)
    n, mo, ri = C.c_int(), C.c_float(), C.c_float()

    def call(cent, maxcent):
        rc = L.kiwi_hip_discretize_eikonal(st, _fp(p), len(p), effective_dt, _fp(prof), len(pts), _fp(pts), _fp(nrm),
                                           cent, maxcent, C.byref(n), C.byref(mo), C.byref(ri))
        if rc != 0:
            raise KiwiHipError("discretize failed (rc=%d): %s" % (rc, _EIKONAL_ERRORS.get(rc, "bad arguments")))

    call(None, 0)
    cent = np.zeros((n.value, 10), np.float32)
    call(_fp(cent), n.value)
    return cent, mo.value, ri.value


def fast_marching_grid_ok(nx, ny):
    """Does the host's optimised march / the device march take an nx x ny grid (padded size within an int)?"""
    return bool(_lib.load().kiwi_hip_fast_marching_grid_ok(int(nx), int(ny)))


def fast_marching_batch(speeds, origins, deltas, starts, discards=None, engine=None):
    """Independent fast-marching solves in one call (kiwi_hip_fast_marching_batch): speeds is a list of 2-D float32 arrays
    [ny, nx] of possibly different shapes, origins / deltas / starts one (x, y) pair per solve, discards one speed per solve
    (None, or NaN entries: none).  engine=None: the host's routine, no GPU needed; an Engine: its device.  Returns
    (list of time arrays, number of solves handed on -- by the device to the host, or by the host's march to the plain one)."""
    L = _lib.load()
    n = len(speeds)
    arrs = [np.ascontiguousarray(a, np.float32) for a in speeds]
    for a in arrs:
        if a.ndim != 2:
            raise ValueError("every speed grid is a 2-D array [ny, nx]")
    nx = np.array([a.shape[1] for a in arrs], np.int32)
    ny = np.array([a.shape[0] for a in arrs], np.int32)
    sizes = np.array([a.size for a in arrs], np.int64)
    ofs = np.zeros(max(n, 1), np.int64)
    ofs[1:n] = np.cumsum(sizes)[:-1]
    total = int(sizes.sum())
    packed = np.concatenate([a.ravel() for a in arrs]) if n and total else np.zeros(1, np.float32)
    times = np.zeros(max(total, 1), np.float32)
    org = np.ascontiguousarray(origins, np.float32).reshape(-1, 2)
    dlt = np.ascontiguousarray(deltas, np.float32).reshape(-1, 2)
    sta = np.ascontiguousarray(starts, np.float32).reshape(-1, 2)
    dis = np.full(n, np.nan, np.float32) if discards is None else np.ascontiguousarray(discards, np.float32).reshape(-1)
    if not (len(org) == len(dlt) == len(sta) == len(dis) == n):
        raise ValueError("origins, deltas, starts and discards need one entry per solve")
    fb = C.c_longlong(0)
    h = engine.h if engine is not None else None
    rc = L.kiwi_hip_fast_marching_batch(h, 1 if engine is not None else 0, n, _ip(nx), _ip(ny),
                                        ofs.ctypes.data_as(C.POINTER(C.c_longlong)), _fp(packed), _fp(org), _fp(dlt), _fp(sta),
                                        _fp(dis), _fp(times), C.byref(fb))
    if rc != 0:
        buf = C.create_string_buffer(1024)
        L.kiwi_hip_last_error(h, buf, 1024)
        raise KiwiHipError("fast_marching_batch: nok > %s" % buf.value.decode())
    out = [times[int(ofs[k]):int(ofs[k]) + int(sizes[k])].reshape(arrs[k].shape).copy() for k in range(n)]
    return out, fb.value


def _pieces(n, piece, st):
    """The pieces [first, first + count) kiwi_hip_misfits_for_params cuts a list of n sources into (list order; it works
    from the last to the first): `piece` sources each, and for the eikonal types the last one as a ramp of half, a quarter,
    an eighth and an eighth of it -- worked on in the order eighth, eighth, quarter, half -- so that the device starts early."""
    out = [(s0, min(piece, n - s0)) for s0 in range(0, n, piece)]
    if st in (4, 5) and len(out) >= 2 and out[-1][1] >= 8:
        first, cnt = out.pop()
        e, q = cnt // 8, cnt // 4
        h = cnt - 2 * e - q
        out += [(first, h), (first + h, q), (first + h + q, e), (first + h + q + e, e)]
    return out


class Engine:
    def __init__(self, device=0, ndev=None, eikonal_solver=None):
        """device: the GPU of a one-device engine; ndev: instead, ONE engine over that many devices of this process
        (kiwi_hip_init_multi; 0 = all visible): setters are repeated on every device, misfits_for_params /
        make_misfits_for_sources shard their trial list over them.  eikonal_solver: 'host' or 'device' (set_eikonal_solver);
        None leaves the library's choice (host, or KIWI_HIP_EIK_DEVICE)."""
        self.L = _lib.load()
        self.h = C.c_void_p()
        rc = self.L.kiwi_hip_init(device, C.byref(self.h)) if ndev is None else self.L.kiwi_hip_init_multi(ndev, C.byref(self.h))
        if rc != 0:
            buf = C.create_string_buffer(512)
            self.L.kiwi_hip_last_error(None, buf, 512)
            self.h = None
            raise KiwiHipError("kiwi_hip_init: " + buf.value.decode())
        self.nsrc = 0
        self.misfit_method = "l2norm"      # the library's default
        if eikonal_solver is not None:
            self.set_eikonal_solver(eikonal_solver)

    def set_eikonal_solver(self, where):
        """Where the eikonal discretisers run their fast-marching solves: 'host' (default) or 'device' -- the solves of a
        batch that the solve cache does not answer go to the GPU as one launch, one solve per wavefront; same results."""
        w = {"host": 0, "device": 1, 0: 0, 1: 1}.get(where)
        if w is None:
            raise ValueError("eikonal_solver: 'host' or 'device'")
        self._ck(self.L.kiwi_hip_set_eikonal_solver(self.h, w), "set_eikonal_solver")

    @property
    def eikonal_solver(self):
        w = C.c_int(0)
        self._ck(self.L.kiwi_hip_get_eikonal_solver(self.h, C.byref(w)), "get_eikonal_solver")
        return "device" if w.value == 1 else "host"

    def eikonal_solver_ms(self):
        """(upload, kernel, download) milliseconds of this context's last device batch of fast-marching solves (HIP events)."""
        u, k, d = C.c_double(0), C.c_double(0), C.c_double(0)
        self._ck(self.L.kiwi_hip_get_eikonal_solver_ms(self.h, C.byref(u), C.byref(k), C.byref(d)), "get_eikonal_solver_ms")
        return u.value, k.value, d.value

    def eikonal_solver_stats(self):
        """(kernel launches, largest heap of any solve) of the same batch; the device heap holds 4096 entries."""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self.L.kiwi_hip_get_eikonal_solver_stats(self.h, C.byref(a), C.byref(b)), "get_eikonal_solver_stats")
        return a.value, b.value

    def ndevices(self):
        n = C.c_int(0)
        self._ck(self.L.kiwi_hip_ndevices(self.h, C.byref(n)), "ndevices")
        return n.value

    def set_arithmetic(self, mode):
        """'exact' (default: every fp32 multiply and add of the superposition rounded on its own, as the reference's host does:
        bit-identical to the CPU oracle) or 'fused' (multiply + consuming add as one fused multiply-add: misfits within 1e-6 of
        the norm factor, half the vector instructions); include/kiwi_hip.h KIWI_ARITH_*."""
        m = {"exact": 0, "fused": 1, 0: 0, 1: 1}.get(mode)
        if m is None:
            raise ValueError("arithmetic: 'exact' or 'fused'")
        self._ck(self.L.kiwi_hip_set_arithmetic(self.h, m), "set_arithmetic")

    def arithmetic(self):
        m = C.c_int(0)
        self._ck(self.L.kiwi_hip_get_arithmetic(self.h, C.byref(m)), "get_arithmetic")
        return "fused" if m.value == 1 else "exact"

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc, what):
        if rc != 0:
            buf = C.create_string_buffer(1024)
            self.L.kiwi_hip_last_error(self.h, buf, 1024)
            raise KiwiHipError("%s: nok > %s" % (what, buf.value.decode()))

    def close(self):
        if self.h:
            self.L.kiwi_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ setup commands
    def set_database(self, dt, dx, dz, firstx, firstz, data, first, nsamp, nipx=1, nipz=1):
        """data[nx,nz,ng,L] float32, first/nsamp[nx,nz,ng] int32 (see kiwi_hip_set_gfdb).  nipx, nipz other than 1: the
        database is densified by Gulunay's f-k interpolation on the device (kiwi_hip_set_gfdb_interpolated)."""
        data = np.ascontiguousarray(data, np.float32)
        first = np.ascontiguousarray(first, np.int32)
        nsamp = np.ascontiguousarray(nsamp, np.int32)
        nx, nz, ng, L = data.shape
        assert first.shape == (nx, nz, ng) and nsamp.shape == (nx, nz, ng)
        if nipx == 1 and nipz == 1:
            rc = self.L.kiwi_hip_set_gfdb(self.h, nx, nz, ng, L, dt, dx, dz, firstx, firstz, _fp(data), _ip(first),
                                          _ip(nsamp))
        else:
            rc = self.L.kiwi_hip_set_gfdb_interpolated(self.h, int(nipx), int(nipz), nx, nz, ng, L, dt, dx, dz, firstx,
                                                       firstz, _fp(data), _ip(first), _ip(nsamp))
        self._ck(rc, "set_database")
        self.dt = dt

    def database_shape(self):
        """(nx, nz, ng, maxlen, dx, dz) of the installed database (densified, when it was)."""
        v = [C.c_int() for _ in range(4)] + [C.c_float() for _ in range(2)]
        self._ck(self.L.kiwi_hip_get_gfdb_shape(self.h, *[C.byref(x) for x in v]), "database_shape")
        return tuple(x.value for x in v)

    def get_database_trace(self, ix, iz, ig):
        """(first, samples) of installed trace (ix, iz, ig), 0-based; samples is empty for a trace that is not stored."""
        f, n = C.c_int(), C.c_int()
        self._ck(self.L.kiwi_hip_get_gfdb_trace(self.h, ix, iz, ig, C.byref(f), C.byref(n), None, 0), "get_database_trace")
        out = np.zeros(max(n.value, 1), np.float32)
        self._ck(self.L.kiwi_hip_get_gfdb_trace(self.h, ix, iz, ig, C.byref(f), C.byref(n), _fp(out), len(out)),
                 "get_database_trace")
        return f.value, out[:n.value]

    def set_local_interpolation(self, kind):
        self._interp = (kind in ("bilinear", True, 1))
        self._ck(self.L.kiwi_hip_set_interp(self.h, int(self._interp), getattr(self, "_xus", 1),
                                            getattr(self, "_zus", 1)), "set_local_interpolation")

    def set_spacial_undersampling(self, xus, zus):
        self._xus, self._zus = xus, zus
        self._ck(self.L.kiwi_hip_set_interp(self.h, int(getattr(self, "_interp", False)), xus, zus),
                 "set_spacial_undersampling")

    def set_effective_dt(self, dt):
        self._ck(self.L.kiwi_hip_set_effective_dt(self.h, dt), "set_effective_dt")

    def set_source_location(self, lat_deg, lon_deg, ref_time=0.0):
        self._ck(self.L.kiwi_hip_set_source_location(self.h, lat_deg, lon_deg, ref_time), "set_source_location")

    def set_receivers(self, lat_deg, lon_deg, depth, components):
        n = len(lat_deg)
        lat = np.ascontiguousarray(lat_deg, np.float64)
        lon = np.ascontiguousarray(lon_deg, np.float64)
        dep = np.ascontiguousarray(np.zeros(n) if depth is None else depth, np.float32)
        arr = (C.c_char_p * n)(*[c.encode() for c in components])
        self._ck(self.L.kiwi_hip_set_receivers(self.h, n, _dp(lat), _dp(lon), _fp(dep), arr), "set_receivers")
        self.components = list(components)
        self.enabled = [len(c) > 0 for c in components]

    def switch_receiver(self, irec, state):
        self._ck(self.L.kiwi_hip_switch_receiver(self.h, irec, int(bool(state))), "switch_receiver")
        self.enabled[irec - 1] = bool(state)

    def set_ref_seismogram(self, irec, icomp, first, data):
        d = np.ascontiguousarray(data, np.float32)
        self._ck(self.L.kiwi_hip_set_reference(self.h, irec, icomp, first, len(d), _fp(d)), "set_ref_seismograms")

    def set_misfit_taper(self, irec, x, y):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        self._ck(self.L.kiwi_hip_set_taper(self.h, irec, len(x), _fp(x), _fp(y)), "set_misfit_taper")

    def set_misfit_filter(self, irec, x, y):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        self._ck(self.L.kiwi_hip_set_filter(self.h, irec, len(x), _fp(x), _fp(y)), "set_misfit_filter")

    def set_misfit_method(self, name):
        if not isinstance(name, int) and name not in NORMS:
            raise KiwiHipError("set_misfit_method: nok > unknown norm: %s" % name)   # minimizer.f90:842-873
        self._ck(self.L.kiwi_hip_set_misfit_method(self.h, NORMS.get(name, name)), "set_misfit_method")
        self.misfit_method = {v: k for k, v in NORMS.items()}.get(name, name)

    def shift_ref_seismogram(self, irec, shift):
        """`shift_ref_seismogram ireceiver shift` (seconds)."""
        self._ck(self.L.kiwi_hip_shift_ref_seismogram(self.h, irec, shift), "shift_ref_seismogram")

    def autoshift_ref_seismogram(self, irec, min_shift, max_shift, isrc=0):
        """`autoshift_ref_seismogram ireceiver min-shift max-shift` against uploaded source `isrc`; returns the shifts
        applied, in seconds (one per receiver for irec == 0)."""
        out = np.zeros(len(self.components) if irec == 0 else 1, np.float32)
        self._ck(self.L.kiwi_hip_autoshift_ref_seismogram(self.h, irec, min_shift, max_shift, isrc, _fp(out)),
                 "autoshift_ref_seismogram")
        return out

    def set_floating_shiftrange(self, irec, min_shift, max_shift):
        """`set_floating_shiftrange ireceiver min-shift max-shift` (seconds; ireceiver 0 = all receivers)."""
        self._ck(self.L.kiwi_hip_set_floating_shiftrange(self.h, irec, min_shift, max_shift), "set_floating_shiftrange")

    def get_floating_shifts(self, isrc0=0, nsrc=None):
        """`get_floating_shifts` for a batch: [nsrc, n_enabled_receivers] in seconds."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        nen = sum(1 for e, c in zip(self.enabled, self.components) if e and len(c))
        out = np.zeros((nsrc, nen), np.float32)
        self._ck(self.L.kiwi_hip_get_floating_shifts(self.h, isrc0, nsrc, _fp(out)), "get_floating_shifts")
        return out

    def set_synthetics_factor(self, f):
        self._ck(self.L.kiwi_hip_set_synthetics_factor(self.h, f), "set_synthetics_factor")

    # ------------------------------------------------------------------ trial sources
    def set_sources(self, tables, moments=None, risetimes=None):
        """tables: list of centroid tables [n_i,10]."""
        ofs = np.zeros(len(tables) + 1, np.int32)
        ofs[1:] = np.cumsum([len(t) for t in tables])
        cent = np.ascontiguousarray(np.concatenate(tables, 0) if len(tables) else np.zeros((0, 10)), np.float32)
        mo = np.ascontiguousarray(np.ones(len(tables)) if moments is None else moments, np.float32)
        ri = np.ascontiguousarray(np.zeros(len(tables)) if risetimes is None else risetimes, np.float32)
        self._ck(self.L.kiwi_hip_set_sources(self.h, len(tables), _ip(ofs), _fp(cent), _fp(mo), _fp(ri)),
                 "set_sources")
        self.nsrc = len(tables)

    def set_source_crust(self, rupture_profile, origin_profile):
        """The two CRUST2.0 look-ups of set_source_location (see include/kiwi_hip.h), 31 floats each."""
        a = np.ascontiguousarray(rupture_profile, np.float32)
        b = np.ascontiguousarray(origin_profile, np.float32)
        self._ck(self.L.kiwi_hip_set_source_crust(self.h, _fp(a), _fp(b)), "set_source_location")

    def set_source_crustal_thickness_limit(self, limit):
        self._ck(self.L.kiwi_hip_set_source_crustal_thickness_limit(self.h, limit),
                 "set_source_crustal_thickness_limit")

    def get_source_crustal_thickness(self):
        t = C.c_float()
        self._ck(self.L.kiwi_hip_get_source_crustal_thickness(self.h, C.byref(t)), "get_source_crustal_thickness")
        return t.value

    def set_source_constraints(self, points, normals):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self._ck(self.L.kiwi_hip_set_source_constraints(self.h, len(pts), _fp(pts), _fp(nrm)),
                 "set_source_constraints")

    def set_source_params(self, sourcetype, params):
        """Batch form of `set_source_params type p1..pn`: params[nsrc, nparams]."""
        p = np.ascontiguousarray(np.atleast_2d(params), np.float32)
        st = SOURCE_TYPES.get(sourcetype, sourcetype)
        if p.shape[1] != self.L.kiwi_hip_source_nparams(st):
            raise KiwiHipError("set_source_params: wrong number of source parameters")
        self.nsrc = p.shape[0]          # the batch is uploaded even when the call reports that no source could be discretised
        self._ck(self.L.kiwi_hip_set_sources_params(self.h, st, p.shape[0], _fp(p)), "set_source_params")

    def get_source_status(self, isrc0=0, nsrc=None):
        """Per uploaded source: 0 discretised, else the discretiser's error code (see source_status_message)."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        st = np.zeros(nsrc, np.int32)
        self._ck(self.L.kiwi_hip_get_source_status(self.h, isrc0, nsrc, _ip(st)), "set_source_params")
        return st

    def source_status_message(self, code):
        buf = C.create_string_buffer(256)
        self.L.kiwi_hip_source_status_message(int(code), buf, 256)
        return buf.value.decode()

    # ------------------------------------------------------------------ hot path
    def eval(self, isrc0=0, nsrc=None):
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        self._ck(self.L.kiwi_hip_eval(self.h, isrc0, nsrc), "get_misfits")

    def sync(self):
        self._ck(self.L.kiwi_hip_sync(self.h), "sync")

    def nmisfits(self):
        n = C.c_int()
        self._ck(self.L.kiwi_hip_nmisfits(self.h, C.byref(n)), "get_misfits")
        return n.value

    def get_misfits(self, isrc0=0, nsrc=None):
        """(misfit[nsrc,nmis], norm[nsrc,nmis], global[nsrc]) of already evaluated sources."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        nm = self.nmisfits()
        m = np.zeros((nsrc, nm), np.float32)
        n = np.zeros((nsrc, nm), np.float32)
        g = np.zeros(nsrc, np.float32)
        self._ck(self.L.kiwi_hip_get_misfits(self.h, isrc0, nsrc, _fp(m), _fp(n), _fp(g)), "get_misfits")
        return m, n, g

    def global_misfits_device(self, isrc0=0, nsrc=None):
        """The global misfits of evaluated sources where they lie: an object with `__cuda_array_interface__` (fp32 [nsrc] on this
        engine's device; torch.as_tensor(obj, device=...) wraps it without a copy), valid until the next eval / upload.  What the
        multi-GPU all-gather takes (kiwi_amd/shard.py gather_global_misfits_device)."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        ptr = C.c_void_p()
        self._ck(self.L.kiwi_hip_get_global_misfits_device(self.h, isrc0, nsrc, C.byref(ptr)), "get_global_misfits_device")

        class _DeviceArray:
            __cuda_array_interface__ = {"shape": (nsrc,), "typestr": "<f4", "data": (ptr.value or 0, False), "version": 2, "strides": None}
        return _DeviceArray()

    def set_keep_synthetics(self, which):
        self._ck(self.L.kiwi_hip_set_keep_synthetics(self.h, which), "set_keep_synthetics")

    def get_synthetics(self, isrc, irec, icomp, which=1, maxn=1 << 20):
        out = np.zeros(maxn, np.float32)
        first, n = C.c_int(), C.c_int()
        self._ck(self.L.kiwi_hip_get_synthetics(self.h, isrc, irec, icomp, which, C.byref(first), C.byref(n),
                                                _fp(out), maxn), "output_seismograms")
        return first.value, out[:n.value].copy()

    def get_amp_spectrum(self, irec, icomp, probe="synthetics", filtered=False, isrc=0, maxn=1 << 20):
        """`output_seismogram_spectra` for one receiver component: (df, amplitudes[ntrans / 2 + 1])."""
        out = np.zeros(maxn, np.float32)
        df, n = C.c_float(), C.c_int()
        self._ck(self.L.kiwi_hip_get_amp_spectrum(self.h, isrc, irec, icomp, 0 if probe == "references" else 1, int(bool(filtered)),
                                                  C.byref(df), C.byref(n), _fp(out), maxn), "output_seismogram_spectra")
        return float(df.value), out[:n.value].copy()

    def get_cross_correlations(self, irec, min_shift, max_shift, isrc=0):
        """`output_cross_correlations` for one receiver: (first shift in samples, cc[ncomp, nshift])."""
        dt = self.dt
        ns = int(round(max_shift / dt)) - int(round(min_shift / dt)) + 1
        nc = len(self.components[irec - 1])
        out = np.zeros(max(ns, 1) * max(nc, 1), np.float32)
        first, n = C.c_int(), C.c_int()
        self._ck(self.L.kiwi_hip_get_cross_correlations(self.h, isrc, irec, min_shift, max_shift, C.byref(first), C.byref(n),
                                                        _fp(out), len(out)), "output_cross_correlations")
        return first.value, out[:nc * n.value].reshape(nc, n.value) if n.value else np.zeros((0, 0), np.float32)

    def get_peak_amplitudes(self, differentiate, isrc=0):
        """`get_peak_amplitudes`: per enabled receiver the peak vector norm of the velocity (1) or acceleration (2)."""
        out = np.zeros(sum(1 for e in self.enabled if e), np.float32)
        self._ck(self.L.kiwi_hip_get_peak_amplitudes(self.h, isrc, differentiate, _fp(out)), "get_peak_amplitudes")
        return out

    def get_arias_intensities(self, isrc=0):
        """`get_arias_intensities` per enabled receiver."""
        out = np.zeros(sum(1 for e in self.enabled if e), np.float32)
        self._ck(self.L.kiwi_hip_get_arias_intensities(self.h, isrc, _fp(out)), "get_arias_intensities")
        return out

    def get_source_centroids(self, isrc=0):
        """The discretised source the engine holds for trial `isrc`: centroids[n, 10] (`output_source_model`)."""
        n = C.c_int()
        self._ck(self.L.kiwi_hip_get_source_centroids(self.h, isrc, 0, C.byref(n), None), "output_source_model")
        cent = np.zeros((n.value, 10), np.float32)
        self._ck(self.L.kiwi_hip_get_source_centroids(self.h, isrc, n.value, C.byref(n), _fp(cent)), "output_source_model")
        return cent

    def get_reference(self, irec, icomp, which=1, maxn=1 << 20):
        """(first sample index, samples) of a reference probe: 1 plain, 2 tapered, 3 filtered."""
        first, n = C.c_int(), C.c_int()
        buf = np.zeros(maxn, np.float32)
        self._ck(self.L.kiwi_hip_get_reference(self.h, irec, icomp, which, C.byref(first), C.byref(n), _fp(buf), maxn),
                 "output_seismograms")
        return first.value, buf[:min(n.value, maxn)].copy()

    def kernel_ms(self):
        ms = np.zeros(4, np.float32)
        ln = np.zeros(3, np.int32)
        self._ck(self.L.kiwi_hip_get_kernel_ms(self.h, _fp(ms), _ip(ln)), "kernel_ms")
        return ms, ln

    def get_geometry(self, isrc, irec, maxcent=100000):
        rec = np.zeros(maxcent, GEOREC)
        n = C.c_int()
        self._ck(self.L.kiwi_hip_get_geometry(self.h, isrc, irec, maxcent, C.byref(n), rec.ctypes.data_as(C.c_void_p)),
                 "get_geometry")
        return rec[:n.value].copy()

    def receiver_geometry(self, irec):
        a, b, d = C.c_double(), C.c_double(), C.c_double()
        self._ck(self.L.kiwi_hip_get_receiver_geometry(self.h, irec, C.byref(a), C.byref(b), C.byref(d)),
                 "output_distances")
        return a.value, b.value, d.value

    def device_bytes(self):
        b = C.c_longlong()
        self.L.kiwi_hip_get_device_bytes(self.h, C.byref(b))
        return b.value

    # ------------------------------------------------------------------ seismosizer.py counterparts
    def misfits_for_params(self, sourcetype, params, piece=0):
        """A whole trial list in one call (kiwi_hip_misfits_for_params): the list is evaluated in pieces of `piece` sources
        (0: 128 for the eikonal types, 2048 otherwise), the host discretiser of one piece running while the device
        evaluates another; afterwards the engine holds the head of the list (sources 0 .. piece - 1).  Returns (misfit[N,nmis], norm[N,nmis], global[N], status[N]); piece size does not change a bit."""
        p = np.ascontiguousarray(np.atleast_2d(params), np.float32)
        st = SOURCE_TYPES.get(sourcetype, sourcetype)
        if p.shape[1] != self.L.kiwi_hip_source_nparams(st):
            raise KiwiHipError("set_source_params: wrong number of source parameters")
        if piece <= 0:
            piece = 128 if st in (4, 5) else 2048
        N, nm = p.shape[0], self.nmisfits()
        m = np.zeros((N, nm), np.float32)
        n = np.zeros((N, nm), np.float32)
        g = np.zeros(N, np.float32)
        status = np.zeros(N, np.int32)
        try:
            self._ck(self.L.kiwi_hip_misfits_for_params(self.h, st, N, _fp(p), piece, _fp(m), _fp(n), _fp(g), _ip(status)),
                     "get_misfits")
        except KiwiHipError:
            self.nsrc = 0                  # (a call that fails midway leaves no batch this object may index)
            raise
        self._hold_head_of_list(N, piece, st, status)
        return m, n, g, status

    def _hold_head_of_list(self, N, piece, st, status):
        # pieces are evaluated from the end of the list: the context holds the first piece that uploaded anything; with a
        # multi-device engine that is shard 0's (the first device keeps the head of the list)
        # (kiwi_hip_misfits_for_params: a list of ONE source takes the one-device path; otherwise min(N, devices) shards, shard i
        # = [N i / k, N (i + 1) / k))
        if piece <= 0:
            piece = 128 if st in (4, 5) else 2048
        ndev = self.ndevices()
        k = 1 if (ndev == 1 or N < 2) else min(N, ndev)
        n0 = N // k
        held = 0
        for s0, cnt in _pieces(n0, piece, st):
            if np.any(status[s0:s0 + cnt] == 0):
                held = cnt
                break
        if held:
            self.nsrc = held               # (no piece uploaded anything: the context keeps what it held)

    # ------------------------------------------------------------------ misfit bands (kiwi_bands.hpp)
    def misfit_bands_max(self):
        """The most bands `set_misfit_bands` takes."""
        return int(self.L.kiwi_hip_misfit_bands_max())

    def set_misfit_bands(self, bands):
        """bands: list of (method name, fx, fy) -- a misfit method (l2norm, l1norm, ampspec_l2norm, ampspec_l1norm,
        scalar_product, peak) and the control points of a frequency filter for every receiver, fx None for no filter.
        An empty list removes the bands.  eval / get_misfits are not affected."""
        bands = list(bands)
        meth, npts, xs, ys = [], [], [], []
        for b in bands:
            name, fx, fy = b
            if not isinstance(name, int) and name not in NORMS:
                raise KiwiHipError("set_misfit_bands: nok > unknown norm: %s" % name)
            meth.append(NORMS.get(name, name))
            fx = [] if fx is None else list(np.asarray(fx, np.float32))
            fy = [] if fy is None or not len(fx) else list(np.asarray(fy, np.float32))
            if len(fx) != len(fy):
                raise KiwiHipError("set_misfit_bands: nok > filter abscissae and ordinates differ in length")
            npts.append(len(fx))
            xs += fx
            ys += fy
        meth = np.ascontiguousarray(meth, np.int32)
        npts = np.ascontiguousarray(npts, np.int32)
        xs = np.ascontiguousarray(xs, np.float32)
        ys = np.ascontiguousarray(ys, np.float32)
        self._ck(self.L.kiwi_hip_set_misfit_bands(self.h, len(bands), _ip(meth), _ip(npts), _fp(xs), _fp(ys)), "set_misfit_bands")

    def misfit_bands(self):
        """Number of bands set."""
        n = C.c_int()
        self._ck(self.L.kiwi_hip_get_misfit_bands(self.h, C.byref(n)), "set_misfit_bands")
        return n.value

    def band_misfits(self, isrc0=0, nsrc=None):
        """(misfit[nsrc,nband,nmis], norm[nsrc,nband,nmis], global[nsrc,nband]) of uploaded sources from ONE synthesis: band b
        is what set_misfit_filter(0, ...) + set_misfit_method + eval + get_misfits give with band b's filter and method."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        nb, nm = self.misfit_bands(), self.nmisfits()
        m = np.zeros((nsrc, nb, nm), np.float32)
        n = np.zeros((nsrc, nb, nm), np.float32)
        g = np.zeros((nsrc, nb), np.float32)
        self._ck(self.L.kiwi_hip_band_misfits(self.h, isrc0, nsrc, _fp(m), _fp(n), _fp(g)), "band_misfits")
        return m, n, g

    def band_misfits_for_params(self, sourcetype, params, piece=0):
        """`band_misfits` for a whole trial list, in pieces and over the devices like misfits_for_params.  Returns
        (misfit[N,nband,nmis], norm[N,nband,nmis], global[N,nband], failings); the rows of the failings are zeros."""
        p = np.ascontiguousarray(np.atleast_2d(params), np.float32)
        st = SOURCE_TYPES.get(sourcetype, sourcetype)
        if p.shape[1] != self.L.kiwi_hip_source_nparams(st):
            raise KiwiHipError("set_source_params: wrong number of source parameters")
        N, nb, nm = p.shape[0], self.misfit_bands(), self.nmisfits()
        m = np.zeros((N, nb, nm), np.float32)
        n = np.zeros((N, nb, nm), np.float32)
        g = np.zeros((N, nb), np.float32)
        status = np.zeros(N, np.int32)
        try:
            self._ck(self.L.kiwi_hip_band_misfits_for_params(self.h, st, N, _fp(p), piece, _fp(m), _fp(n), _fp(g), _ip(status)),
                     "band_misfits")
        except KiwiHipError:
            self.nsrc = 0
            raise
        self._hold_head_of_list(N, piece, st, status)
        return m, n, g, [int(i) for i in np.nonzero(status)[0]]

    def band_misfits_ms(self):
        """HIP-event durations [ms] of the last band call: (evaluation, band kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_band_misfits_ms, 3, "band_misfits")

    # ------------------------------------------------------------------ time scan (kiwi_timescan.hpp)
    def time_scan(self, isrc0=0, nsrc=None, k0=0, kstep=1, nk=1):
        """(misfit[nsrc,nk,nmis], norm[nsrc,nmis], global[nsrc,nk], best[nsrc]) of uploaded sources at the origin-time offsets
        (k0 + j kstep) dt, j < nk, from ONE synthesis: the raw synthetic read k samples earlier, everything else as eval +
        get_misfits do it (include/kiwi_hip.h).  best: the offset index of the smallest global misfit, -1 for a failing."""
        nsrc = self.nsrc - isrc0 if nsrc is None else nsrc
        nk_, nm = max(int(nk), 0), self.nmisfits()
        m = np.zeros((nsrc, nk_, nm), np.float32)
        n = np.zeros((nsrc, nm), np.float32)
        g = np.zeros((nsrc, nk_), np.float32)
        b = np.zeros(nsrc, np.int32)
        self._ck(self.L.kiwi_hip_time_scan(self.h, isrc0, nsrc, int(k0), int(kstep), int(nk), _fp(m), _fp(n), _fp(g), _ip(b)), "time_scan")
        return m, n, g, b

    def time_scan_for_params(self, sourcetype, params, k0=0, kstep=1, nk=1, piece=0):
        """`time_scan` for a whole trial list, in pieces and over the devices like misfits_for_params.  Returns
        (misfit[N,nk,nmis], norm[N,nmis], global[N,nk], best[N], failings); the rows of the failings are zeros, their best -1."""
        p = np.ascontiguousarray(np.atleast_2d(params), np.float32)
        st = SOURCE_TYPES.get(sourcetype, sourcetype)
        if p.shape[1] != self.L.kiwi_hip_source_nparams(st):
            raise KiwiHipError("set_source_params: wrong number of source parameters")
        N, nk_, nm = p.shape[0], max(int(nk), 0), self.nmisfits()
        m = np.zeros((N, nk_, nm), np.float32)
        n = np.zeros((N, nm), np.float32)
        g = np.zeros((N, nk_), np.float32)
        b = np.zeros(N, np.int32)
        status = np.zeros(N, np.int32)
        try:
            self._ck(self.L.kiwi_hip_time_scan_for_params(self.h, st, N, _fp(p), piece, int(k0), int(kstep), int(nk), _fp(m), _fp(n),
                                                          _fp(g), _ip(b), _ip(status)), "time_scan")
        except KiwiHipError:
            self.nsrc = 0
            raise
        self._hold_head_of_list(N, piece, st, status)
        return m, n, g, b, [int(i) for i in np.nonzero(status)[0]]

    def time_scan_ms(self):
        """HIP-event durations [ms] of the last scan call: (evaluation, scan kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_time_scan_ms, 3, "time_scan")

    def make_misfits_for_sources(self, sourcetype=None, params=None, piece=0):
        """seismosizer.py:682-722: returns (misfits_by_src[N_s,N_r,N_k], norms_by_src[...], failings) -- float64 arrays,
        receivers in file order, components in string order, disabled receivers as zeros; `failings` lists the indices of
        the trial sources the engine rejected (`SeismosizersReturnedErrors` there, :716-717), whose rows stay zero.
        With `params` the trial list goes through misfits_for_params (discretiser and device overlapped, pieces of
        `piece` sources); without, the sources uploaded before are evaluated."""
        if params is not None:
            m, n, _, status = self.misfits_for_params(sourcetype, params, piece)
            nsrc = len(m)
        else:
            status = self.get_source_status()
            self.eval()
            m, n, _ = self.get_misfits()
            nsrc = self.nsrc
        failings = [int(i) for i in np.nonzero(status)[0]]
        nrec = len(self.components)
        nk = max([len(c) for c in self.components] + [1])
        mis = np.zeros((nsrc, nrec, nk))
        nor = np.zeros((nsrc, nrec, nk))
        j = 0
        for ir, comps in enumerate(self.components):
            if not self.enabled[ir]:
                continue
            k = len(comps)
            mis[:, ir, :k] = m[:, j:j + k]
            nor[:, ir, :k] = n[:, j:j + k]
            j += k
        return mis, nor, failings

    def outer_max_receivers(self):
        """The most receivers `outer_misfits` takes (the weight rows of a draw tile live in LDS)."""
        return int(self.L.kiwi_hip_outer_max_receivers())

    def outer_misfits_slots(self, misfit, norm, slot_receiver, nrec, outer_norm="l2norm", receiver_weights=None, anarchy=False,
                            draw_weights=None, which_draw=None):
        """kiwi_hip_outer_misfits on per-slot arrays: misfit, norm [N_s, nmis] float32 as `get_misfits` / `misfits_for_params`
        return them, `slot_receiver[nmis]` the 0-based receiver of every slot (ascending), `draw_weights[B, nrec]` the weight of
        every receiver in every draw (None: one draw of ones).  Returns (best_value[B] float64, best_index[B] int32,
        global_of_draw[N_s] float64 or None): the lowest global misfit of each draw and its source -- among equal values the
        lowest index; NaN, 0 where every source is excluded -- and the global misfits of all sources under draw `which_draw`."""
        code = _outer_code(outer_norm)
        m = np.ascontiguousarray(misfit, np.float32)
        n = np.ascontiguousarray(norm, np.float32)
        sr = np.ascontiguousarray(slot_receiver, np.int32)
        if m.ndim != 2 or m.shape != n.shape or m.shape[1] != len(sr):
            raise KiwiHipError("outer_misfits: misfit and norm must be [N_s, nmis] with one slot_receiver entry per slot")
        nrec = int(nrec)
        dw = np.ones((1, nrec)) if draw_weights is None else np.ascontiguousarray(draw_weights, np.float64)
        if dw.ndim != 2 or dw.shape[1] != nrec:
            raise KiwiHipError("outer_misfits: draw_weights must be [B, %d]" % nrec)
        w = None
        if receiver_weights is not None:
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(receiver_weights, np.float64), (nrec,)))
        nd = len(dw)
        bv, bi = np.zeros(nd, np.float64), np.zeros(nd, np.int32)
        g = None if which_draw is None else np.zeros(len(m), np.float64)
        self._ck(self.L.kiwi_hip_outer_misfits(self.h, len(m), m.shape[1], nrec, _ip(sr), _fp(m), _fp(n), code, _dp(w),
                                               1 if anarchy else 0, nd, _dp(dw), _dp(bv), _ip(bi),
                                               0 if which_draw is None else int(which_draw), _dp(g)), "outer_misfits")
        return bv, bi, g

    def outer_ms(self):
        """HIP-event durations [ms] of the last outer_misfits: (uploads, kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_outer_ms, 3, "get_outer_ms")

    def outer_misfits(self, misfits_by_src, norms_by_src, outer_norm="l2norm", receiver_weights=None, anarchy=False,
                      draw_weights=None, which_draw=None, ncomponents=None):
        """`make_global_misfits` under B receiver weightings and the best source of each, on the device, from the
        [N_s, N_r, N_k] arrays `make_misfits_for_sources` returns.  The slot map comes from the receivers' components
        (`ncomponents`: slots per receiver, for arrays that are not this engine's own); the values go to the device as
        float32, which is what the engine produced them in.  See `outer_misfits_slots` for the draws and the results."""
        m = np.asarray(misfits_by_src)
        n = np.asarray(norms_by_src)
        if m.ndim != 3 or m.shape != n.shape:
            raise KiwiHipError("outer_misfits: misfits and norms must be [N_s, N_r, N_k]")
        nk = [len(c) for c in getattr(self, "components", [])] if ncomponents is None else [int(k) for k in ncomponents]
        ns, nrec, kmax = m.shape
        if len(nk) != nrec or max(nk + [0]) > kmax:
            raise KiwiHipError("outer_misfits: the arrays do not match the receivers' components")
        slot_receiver = np.repeat(np.arange(nrec, dtype=np.int32), nk)
        if all(k == kmax for k in nk):
            mf, nf = m.reshape(ns, nrec * kmax), n.reshape(ns, nrec * kmax)
        else:
            cols = np.concatenate([ir * kmax + np.arange(k) for ir, k in enumerate(nk)] + [np.zeros(0, np.int64)]).astype(np.int64)
            mf, nf = m.reshape(ns, nrec * kmax)[:, cols], n.reshape(ns, nrec * kmax)[:, cols]
        return self.outer_misfits_slots(mf, nf, slot_receiver, nrec, outer_norm, receiver_weights, anarchy, draw_weights,
                                        which_draw)

    # ------------------------------------------------------------------ what the group families share
    def _read_ms(self, fn, n, what):
        """the n HIP-event durations [ms] a `kiwi_hip_get_*_ms` call answers, as floats"""
        ms = np.zeros(n, np.float32)
        self._ck(fn(self.h, _fp(ms)), what)
        return tuple(float(x) for x in ms)

    def _basis_count(self, K, name, kmax=None):
        K, kmax = int(K), self.linear_fit_max_basis() if kmax is None else kmax
        if not 1 <= K <= kmax:
            raise KiwiHipError(_K_RANGE % (name, K, kmax))
        return K

    def _read_shape(self, fn, lead, count, name):
        """the `count` ints a `_shape` call answers for the leading arguments `lead`, the last of which is K; `name` signs the refusal"""
        v = [np.zeros(1, np.int32) for _ in range(count)]
        if fn(*lead, *[_ip(a) for a in v]):
            raise KiwiHipError(_K_RANGE % (name, lead[-1], self.linear_fit_max_basis()))
        return tuple(int(a[0]) for a in v)

    def _receiver_weights(self, receiver_weights):
        if receiver_weights is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(receiver_weights, np.float64), (len(self.components),)))

    def _nslots(self):
        return sum(len(c) for ir, c in enumerate(self.components) if self.enabled[ir])

    def _candidate_inputs(self, name, outer_norm, K, candidates, receiver_weights, draw_weights=None, krange=None):
        """What a candidate family takes in, checked and as the library wants it: the code of the outer norm, the candidates as
        float64 [ncand, K], the receiver weights as float64 [nrec] or None and, where there are draws, their weights as float64
        [ndraw, nrec].  `name` signs the refusals, `krange` that of K where it is signed otherwise."""
        code = _outer_code(outer_norm)
        K = self._basis_count(K, krange or name)
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(candidates, np.float64)))
        if x.ndim != 2 or x.shape[1] != K:
            raise KiwiHipError("%s: candidates must be [ncand, K = %d]" % (name, K))
        w = self._receiver_weights(receiver_weights)
        if draw_weights is None:
            return code, x, w
        dw = np.ascontiguousarray(np.asarray(draw_weights, np.float64))
        if dw.ndim != 2 or dw.shape[1] != len(self.components):
            raise KiwiHipError("%s: draw_weights must be [ndraw, %d]" % (name, len(self.components)))
        return code, x, w, dw

    def _list_head(self, sourcetype, params, K, piece, name=None):
        """The arguments (sourcetype, ngroup, K, params, piece) a `_params` call takes where the uploaded call takes (isrc0, ngroup,
        K), checked, and the number of rows.  `name` signs the two refusals; None: as set_source_params and linear_fit_params."""
        count, whole = (name, name) if name else ("set_source_params", "linear_fit_params")
        p = np.ascontiguousarray(np.atleast_2d(params), np.float32)
        st = SOURCE_TYPES.get(sourcetype, sourcetype)
        K = int(K)
        if p.shape[1] != self.L.kiwi_hip_source_nparams(st):
            raise KiwiHipError("%s: wrong number of source parameters" % count)
        if K < 1 or p.shape[0] % K or p.shape[0] == 0:
            raise KiwiHipError("%s: %d parameter rows are not whole groups of K = %d" % (whole, p.shape[0], K))
        return (st, p.shape[0] // K, K, _fp(p), int(piece)), len(p)

    def _list_call(self, fn, head, rows, args, what):
        """a `_params` call: afterwards the engine holds the head of the list -- after a call that failed, nothing"""
        try:
            self._ck(fn(self.h, *head, *args), what)
        except KiwiHipError:
            self.nsrc = 0
            raise
        self.nsrc = self._uploaded_sources(rows)

    def _uploaded_sources(self, nlist):
        """how many sources the context holds after a list call of `nlist` rows: its first piece (list order) that uploaded
        anything; a group's status does not say whether ALL of its piece failed to discretise, so the context is asked: the
        longest range of source statuses it answers"""
        buf = np.zeros(max(self.nsrc, nlist, 1), np.int32)
        lo, hi = 0, len(buf)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if self.L.kiwi_hip_get_source_status(self.h, 0, mid, _ip(buf)) == 0:
                lo = mid
            else:
                hi = mid - 1
        return lo

    # ------------------------------------------------------------------ linear fit (kiwi_hip_linear_fit)
    def linear_fit_max_basis(self):
        """The most basis sources per group `linear_fit` takes."""
        return int(self.L.kiwi_hip_linear_fit_max_basis())

    def _linear_fit_arrays(self, ngroup, K, receiver_weights, anarchy, normal, by_receiver):
        """what every `_..._arrays` returns: (the arguments of the call after (isrc0, ngroup, K) or (sourcetype, ngroup, K, params,
        piece), the tuple they fill)"""
        K, ngroup = self._basis_count(K, "linear_fit"), int(ngroup)
        nrec, nn = len(self.components), K * (K + 1) // 2 + K + 1
        w = self._receiver_weights(receiver_weights)
        out = LinearFit(np.zeros((ngroup, K)), np.zeros(ngroup), np.zeros(ngroup, np.int32), np.zeros(ngroup),
                        np.zeros((ngroup, nn)) if normal else None, np.zeros((ngroup, nrec, nn)) if by_receiver else None)
        return (_dp(w), 1 if anarchy else 0, _dp(out.coef), _dp(out.misfit), _ip(out.status), _dp(out.pivot_min), _dp(out.normal),
                _dp(out.by_receiver)), out

    def linear_fit(self, isrc0, ngroup, K, receiver_weights=None, anarchy=False, normal=False, by_receiver=False):
        """Least-squares coefficients of K basis sources per group under l2norm (kiwi_hip_linear_fit): sources
        [isrc0, isrc0 + ngroup K) of the uploaded batch are `ngroup` groups of K consecutive basis sources.  Returns a
        `LinearFit`: coef[ngroup, K], misfit[ngroup] (the global misfit of the fitted combination), status[ngroup] (0 solved,
        1 no solution, 2 a basis source failed to discretise), pivot_min[ngroup] (smallest Cholesky pivot of the unit-diagonal
        normal matrix: judge near-dependence by it), and on request normal[ngroup, NN] (G upper triangle by rows, b, R --
        weighted sums) and by_receiver[ngroup, nrec, NN] (unweighted, zeros for disabled receivers)."""
        args, out = self._linear_fit_arrays(ngroup, K, receiver_weights, anarchy, normal, by_receiver)
        self._ck(self.L.kiwi_hip_linear_fit(self.h, int(isrc0), int(ngroup), int(K), *args), "linear_fit")
        return out

    def linear_fit_params(self, sourcetype, params, K, receiver_weights=None, anarchy=False, normal=False, by_receiver=False, piece=0):
        """`linear_fit` for a parameter list of any length (kiwi_hip_linear_fit_params): params[ngroup * K, nparams], every K
        consecutive rows a group; discretised and uploaded in pieces of `piece` sources (rounded down to a multiple of K;
        0: the default of misfits_for_params), the host discretiser of one piece running while the device works on another.
        Piece size does not change a bit.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._linear_fit_arrays(head[1], K, receiver_weights, anarchy, normal, by_receiver)
        self._list_call(self.L.kiwi_hip_linear_fit_params, head, rows, args, "linear_fit")
        return out

    def linear_fit_ms(self):
        """HIP-event durations [ms] of the last linear fit: (evaluation, fit kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_ms, 3, "get_linear_fit_ms")

    # ------------------------------------------------------------------ linear fit at many origin times (kiwi_hip_linear_fit_time_scan)
    def linear_fit_time_scan_shape(self, K):
        """(offsets per workgroup, window samples per LDS tile) of the Gram-scan kernel for K basis sources."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_time_scan_shape, (int(K),), 2, "linear_fit")

    def _scan_fit_arrays(self, ngroup, K, k0, kstep, nk, receiver_weights, anarchy, normal):
        K, ngroup, nk_ = self._basis_count(K, "linear_fit"), int(ngroup), max(int(nk), 0)
        nn = K * (K + 1) // 2 + K + 1
        w = self._receiver_weights(receiver_weights)
        out = ScanFit(np.zeros((ngroup, nk_, K)), np.zeros((ngroup, nk_)), np.zeros((ngroup, nk_), np.int32), np.zeros((ngroup, nk_)),
                      np.zeros(ngroup, np.int32), np.zeros((ngroup, nk_, nn)) if normal else None)
        return (int(k0), int(kstep), int(nk), _dp(w), 1 if anarchy else 0, _dp(out.coef), _dp(out.misfit), _ip(out.status),
                _dp(out.pivot_min), _ip(out.best), _dp(out.normal)), out

    def linear_fit_time_scan(self, isrc0, ngroup, K, k0=0, kstep=1, nk=1, receiver_weights=None, anarchy=False, normal=False):
        """`linear_fit` at the origin-time offsets (k0 + j kstep) dt, j < nk, from ONE synthesis of the basis sources
        (kiwi_hip_linear_fit_time_scan): the basis synthetics read k samples earlier under the receivers' tapers at their fixed
        places.  Returns a `ScanFit`: coef[ngroup, nk, K], misfit[ngroup, nk], status[ngroup, nk], pivot_min[ngroup, nk],
        best[ngroup] (the offset index of the smallest misfit among the solved offsets, -1 if there is none) and on request
        normal[ngroup, nk, NN].  Offset 0 is `linear_fit` bit for bit."""
        args, out = self._scan_fit_arrays(ngroup, K, k0, kstep, nk, receiver_weights, anarchy, normal)
        self._ck(self.L.kiwi_hip_linear_fit_time_scan(self.h, int(isrc0), int(ngroup), int(K), *args), "linear_fit_time_scan")
        return out

    def linear_fit_time_scan_params(self, sourcetype, params, K, k0=0, kstep=1, nk=1, receiver_weights=None, anarchy=False, normal=False,
                                    piece=0):
        """`linear_fit_time_scan` for a parameter list of any length, cut into pieces and over the devices at group boundaries as
        `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._scan_fit_arrays(head[1], K, k0, kstep, nk, receiver_weights, anarchy, normal)
        self._list_call(self.L.kiwi_hip_linear_fit_time_scan_params, head, rows, args, "linear_fit_time_scan")
        return out

    def linear_fit_time_scan_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_time_scan`: (evaluation, Gram-scan kernel, solve kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_time_scan_ms, 4, "get_linear_fit_time_scan_ms")

    # ------------------------------------------------------------------ candidate coefficient vectors (kiwi_hip_linear_fit_candidates)
    def linear_fit_candidates_shape(self, K):
        """(candidates per workgroup, receivers per LDS stage) of the candidate kernel for K basis sources."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_candidates_shape, (int(K),), 2, "linear_fit")

    def _candidate_arrays(self, ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit, receiver_misfit):
        code, x, w = self._candidate_inputs("linear_fit_candidates", outer_norm, K, candidates, receiver_weights, krange="linear_fit")
        ng, K, nc, nrec = int(ngroup), int(K), len(x), len(self.components)
        out = CandidateScan(np.zeros(ng, np.int32), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, nc)) if misfit else None,
                            np.zeros((ng, nc)) if free_scale else None,
                            np.zeros((ng, nc, nrec), np.float32) if receiver_misfit else None,
                            np.zeros((ng, nrec), np.float32) if receiver_misfit else None, np.zeros((ng, K)), np.zeros(ng))
        return (nc, _dp(x), code, _dp(w), 1 if anarchy else 0, 1 if free_scale else 0, _ip(out.best_index), _dp(out.best_misfit),
                _ip(out.status), _dp(out.misfit), _dp(out.scale), _fp(out.receiver_misfit), _fp(out.receiver_norm), _dp(out.fit_coef),
                _dp(out.fit_misfit)), out

    def linear_fit_candidates(self, isrc0, ngroup, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                              free_scale=False, misfit=True, receiver_misfit=False):
        """The misfits of the coefficient vectors candidates[ncand, K] for every group of `linear_fit`, from the normal
        equations the fit keeps on the device (kiwi_hip_linear_fit_candidates): no synthesis per candidate.  The engine's
        misfit method (the inner norm) must be l2norm; `outer_norm` combines the receivers.  free_scale (l2norm only): a
        candidate is a direction whose best scale is found.  Returns a `CandidateScan`: best_index[ngroup] (-1: none),
        best_misfit[ngroup], status[ngroup] (0 evaluated, 1 no data, 2 a basis source failed to discretise), misfit[ngroup,
        ncand] (misfit=True), scale[ngroup, ncand] (free_scale), receiver_misfit[ngroup, ncand, nrec] and receiver_norm[ngroup,
        nrec] float32 (receiver_misfit=True: what `outer_misfits` takes with one slot per receiver), fit_coef[ngroup, K] and
        fit_misfit[ngroup]: `linear_fit` of the same groups."""
        args, out = self._candidate_arrays(ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit, receiver_misfit)
        self._ck(self.L.kiwi_hip_linear_fit_candidates(self.h, int(isrc0), int(ngroup), int(K), *args), "linear_fit_candidates")
        return out

    def linear_fit_candidates_params(self, sourcetype, params, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                                     free_scale=False, misfit=True, receiver_misfit=False, piece=0):
        """`linear_fit_candidates` for a parameter list of any length (kiwi_hip_linear_fit_candidates_params), cut into pieces
        and over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._candidate_arrays(head[1], K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit, receiver_misfit)
        self._list_call(self.L.kiwi_hip_linear_fit_candidates_params, head, rows, args, "linear_fit_candidates")
        return out

    def linear_fit_candidates_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_candidates`: (evaluation, Gram and solve kernels, candidate kernels,
        downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_candidates_ms, 4, "get_linear_fit_candidates_ms")

    # ------------------------------------------------------------------ candidates with per-receiver shifts (kiwi_hip_linear_fit_candidates_floating)
    def linear_fit_candidates_floating_shape(self, K):
        """(candidates per workgroup, shifts per pass of the cross-correlation kernel, shifts per LDS stage of the candidate
        kernel) for K basis sources."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_candidates_floating_shape, (int(K),), 3, "linear_fit_candidates_floating")

    def _candidate_floating_arrays(self, ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit, cand_shift,
                                   receiver_misfit):
        code, x, w = self._candidate_inputs("linear_fit_candidates_floating", outer_norm, K, candidates, receiver_weights)
        ng, nc, nrec = int(ngroup), len(x), len(self.components)
        out = CandidateFloatingScan(np.zeros(ng, np.int32), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, nrec), np.int32),
                                    np.zeros((ng, nc)) if misfit else None, np.zeros((ng, nc, nrec), np.int16) if cand_shift else None,
                                    np.zeros((ng, nc, nrec), np.float32) if receiver_misfit else None,
                                    np.zeros((ng, nrec), np.float32) if receiver_misfit else None)
        return (nc, _dp(x), code, _dp(w), 1 if anarchy else 0, 1 if free_scale else 0, _ip(out.best_index), _dp(out.best_misfit),
                _ip(out.status), _ip(out.best_shift), _dp(out.misfit), _sp(out.cand_shift), _fp(out.receiver_misfit),
                _fp(out.receiver_norm)), out

    def linear_fit_candidates_floating(self, isrc0, ngroup, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                                       free_scale=False, misfit=True, cand_shift=False, receiver_misfit=False):
        """`linear_fit_candidates` under floating_l2norm (kiwi_hip_linear_fit_candidates_floating): every receiver slides its
        reference by the whole samples of its own range (`set_floating_shiftrange`) and, per candidate, the shift with the
        smallest squared misfit wins.  Nothing is fitted, and free_scale is refused.  Returns a `CandidateFloatingScan`:
        best_index[ngroup] (-1: none), best_misfit[ngroup], status[ngroup] (0 evaluated, 1 no receiver counts, 2 a basis source
        failed to discretise), best_shift[ngroup, nrec] (the winner's shifts in SAMPLES, 0 for receivers that do not count),
        misfit[ngroup, ncand] (misfit=True), cand_shift[ngroup, ncand, nrec] int16 (cand_shift=True; needs misfit),
        receiver_misfit[ngroup, ncand, nrec] and receiver_norm[ngroup, nrec] float32 (receiver_misfit=True: what
        `outer_misfits` takes with one slot per receiver)."""
        args, out = self._candidate_floating_arrays(ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit,
                                                    cand_shift, receiver_misfit)
        self._ck(self.L.kiwi_hip_linear_fit_candidates_floating(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "linear_fit_candidates_floating")
        return out

    def linear_fit_candidates_floating_params(self, sourcetype, params, K, candidates, outer_norm="l1norm", receiver_weights=None,
                                              anarchy=False, free_scale=False, misfit=True, cand_shift=False, receiver_misfit=False,
                                              piece=0):
        """`linear_fit_candidates_floating` for a parameter list of any length (kiwi_hip_linear_fit_candidates_floating_params),
        cut into pieces and over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._candidate_floating_arrays(head[1], K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit,
                                                    cand_shift, receiver_misfit)
        self._list_call(self.L.kiwi_hip_linear_fit_candidates_floating_params, head, rows, args, "linear_fit_candidates_floating")
        return out

    def linear_fit_candidates_floating_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_candidates_floating`: (evaluation, Gram and cross-correlation kernels,
        candidate kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_candidates_floating_ms, 4, "get_linear_fit_candidates_floating_ms")

    # ------------------------------------------------------------------ joint bootstrap of a candidate search with shifts (kiwi_hip_linear_fit_candidates_floating_bootstrap)
    def linear_fit_candidates_floating_bootstrap_shape(self, K):
        """(candidates per workgroup, draws per tile, the most receivers) of the bootstrap kernel under floating_l2norm for K basis
        sources; no device needed."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_candidates_floating_bootstrap_shape, (int(K),), 3,
                                "linear_fit_candidates_floating_bootstrap")

    def _candidate_floating_bootstrap_arrays(self, ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group):
        code, x, w, dw = self._candidate_inputs("linear_fit_candidates_floating_bootstrap", outer_norm, K, candidates, receiver_weights,
                                                draw_weights, krange="linear_fit")
        ng, nd, nrec = int(ngroup), len(dw), len(self.components)
        grp = (ng, nd) if per_group else None
        out = CandidateFloatingBootstrap(np.zeros(nd), np.zeros(nd, np.int32), np.zeros(nd, np.int32), np.zeros((nd, nrec), np.int32),
                                         np.zeros(ng, np.int32), np.zeros(grp) if grp else None, np.zeros(grp, np.int32) if grp else None,
                                         np.zeros(grp + (nrec,), np.int32) if grp else None)
        return (len(x), _dp(x), code, _dp(w), 1 if anarchy else 0, nd, _dp(dw), _dp(out.best_value), _ip(out.best_group),
                _ip(out.best_cand), _ip(out.best_shift), _ip(out.status), _dp(out.group_value), _ip(out.group_cand),
                _ip(out.group_shift)), out

    def linear_fit_candidates_floating_bootstrap(self, isrc0, ngroup, K, candidates, draw_weights, outer_norm="l1norm",
                                                 receiver_weights=None, anarchy=False, per_group=False):
        """The bootstrap over the receivers of a candidate search under floating_l2norm, joint over group and candidate, on the
        device (kiwi_hip_linear_fit_candidates_floating_bootstrap): what `linear_fit_candidates_floating(..., cand_shift=True,
        receiver_misfit=True)` followed by `outer_misfits` with `draw_weights[ndraw, nrec]` answers, bit for bit, without the
        [candidate, receiver] matrices.  Returns a `CandidateFloatingBootstrap`: best_value[ndraw], best_group, best_cand[ndraw]
        (NaN and -1 where every source of a draw is excluded), best_shift[ndraw, nrec] (the winner's shifts in SAMPLES, 0 for
        receivers that do not count), status[ngroup]; per_group=True adds group_value, group_cand[ngroup, ndraw] and
        group_shift[ngroup, ndraw, nrec], the same per group.  A row of ones as draw 0 gives the plain winner."""
        args, out = self._candidate_floating_bootstrap_arrays(ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy,
                                                              per_group)
        self._ck(self.L.kiwi_hip_linear_fit_candidates_floating_bootstrap(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "linear_fit_candidates_floating_bootstrap")
        return out

    def linear_fit_candidates_floating_bootstrap_params(self, sourcetype, params, K, candidates, draw_weights, outer_norm="l1norm",
                                                        receiver_weights=None, anarchy=False, per_group=False, piece=0):
        """`linear_fit_candidates_floating_bootstrap` for a parameter list of any length, cut into pieces and over the devices at
        group boundaries as `linear_fit_params` cuts it; best_group counts the groups of the whole list.  Afterwards the engine
        holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._candidate_floating_bootstrap_arrays(head[1], K, candidates, draw_weights, outer_norm, receiver_weights, anarchy,
                                                              per_group)
        self._list_call(self.L.kiwi_hip_linear_fit_candidates_floating_bootstrap_params, head, rows, args,
                        "linear_fit_candidates_floating_bootstrap")
        return out

    def linear_fit_candidates_floating_bootstrap_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_candidates_floating_bootstrap`: (evaluation, Gram and cross-correlation
        kernels, bootstrap kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms, 4,
                             "get_linear_fit_candidates_floating_bootstrap_ms")

    # ------------------------------------------------------------------ candidates under the amplitude-spectrum norms (kiwi_hip_spectral_candidates)
    def spectral_candidates_shape(self, K, context=True):
        """(candidates per workgroup, bins of spectra per LDS stage, spectra_bins) of `spectral_candidates` for K basis sources;
        spectra_bins is the row length of this engine's `spectra` arrays for the sources it holds -- the longest transform any of
        their slots needs, halved, plus one -- (0 with context=False, which needs no device)."""
        return self._read_shape(self.L.kiwi_hip_spectral_candidates_shape, (self.h if context else None, int(K)), 3, "spectral_candidates")

    def _spectral_candidate_arrays(self, ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit, slot_misfit,
                                   spectra, spectra_bins=None):
        code, x, w = self._candidate_inputs("spectral_candidates", outer_norm, K, candidates, receiver_weights)
        ng, K, nc, nmis = int(ngroup), int(K), len(x), self._nslots()
        nb = (self.spectral_candidates_shape(K)[2] if spectra_bins is None else int(spectra_bins)) if spectra else 0
        out = SpectralCandidateScan(np.zeros(ng, np.int32), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, nc)) if misfit else None,
                                    np.zeros((ng, nc)) if free_scale and misfit else None,
                                    np.zeros((ng, nc, nmis), np.float32) if slot_misfit else None,
                                    np.zeros((ng, nmis), np.float32) if slot_misfit else None,
                                    np.zeros((ng, nmis, nb, K, 2), np.float32) if spectra else None,
                                    np.zeros((ng, nmis, 3), np.int32) if spectra else None,
                                    np.zeros((ng, nmis, nb, 2), np.float32) if spectra else None)
        return (nc, _dp(x), code, _dp(w), 1 if anarchy else 0, 1 if free_scale else 0, _ip(out.best_index), _dp(out.best_misfit),
                _ip(out.status), _dp(out.misfit), _dp(out.scale), _fp(out.slot_misfit), _fp(out.slot_norm), nb, _fp(out.spectra),
                _ip(out.spectra_range), _fp(out.spectra_ref)), out

    def spectral_candidates(self, isrc0, ngroup, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                            free_scale=False, misfit=True, slot_misfit=False, spectra=False, spectra_bins=None):
        """The misfits of given coefficient vectors under ampspec_l2norm / ampspec_l1norm (kiwi_hip_spectral_candidates): sources
        [isrc0, isrc0 + ngroup K) are groups of K basis sources whose complex spectra are combined per candidate; the amplitude of
        the combination is compared with the reference's inside the pass band.  Returns a `SpectralCandidateScan`:
        best_index[ngroup] (-1: none), best_misfit[ngroup], status[ngroup] (0 evaluated, 1 no receiver counts, 2 a basis source
        failed to discretise), misfit[ngroup, ncand] (misfit=True) and scale[ngroup, ncand] (free_scale: ampspec_l2norm with the
        outer l2norm only), slot_misfit[ngroup, ncand, nmis] and slot_norm[ngroup, nmis] float32 (slot_misfit=True: what
        `outer_misfits_slots` takes), spectra[ngroup, nmis, spectra_bins, K, 2], spectra_range[ngroup, nmis, 3] (klo, khi,
        ntrans) and spectra_ref[ngroup, nmis, spectra_bins, 2] (reference amplitude, filter weight) with spectra=True
        (spectra_bins: `spectral_candidates_shape`'s unless given)."""
        args, out = self._spectral_candidate_arrays(ngroup, K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit,
                                                    slot_misfit, spectra, spectra_bins)
        self._ck(self.L.kiwi_hip_spectral_candidates(self.h, int(isrc0), int(ngroup), int(K), *args), "spectral_candidates")
        return out

    def spectral_candidates_params(self, sourcetype, params, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                                   free_scale=False, misfit=True, slot_misfit=False, spectra=False, spectra_bins=None, piece=0):
        """`spectral_candidates` for a parameter list of any length (kiwi_hip_spectral_candidates_params), cut into pieces and
        over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list.  spectra=True without
        spectra_bins: the first group is uploaded to size the rows; a later group that needs longer ones is refused by name."""
        head, rows = self._list_head(sourcetype, params, K, piece, "spectral_candidates")
        if spectra and spectra_bins is None:
            self.set_source_params(sourcetype, np.atleast_2d(params)[:head[2]])
        args, out = self._spectral_candidate_arrays(head[1], K, candidates, outer_norm, receiver_weights, anarchy, free_scale, misfit,
                                                    slot_misfit, spectra, spectra_bins)
        self._list_call(self.L.kiwi_hip_spectral_candidates_params, head, rows, args, "spectral_candidates")
        return out

    def spectral_candidates_ms(self):
        """HIP-event durations [ms] of the last `spectral_candidates`: (evaluation, the spectra kernel alone, candidate kernels,
        downloads); the host's table of kept bins and its upload lie between the first two, in neither."""
        return self._read_ms(self.L.kiwi_hip_get_spectral_candidates_ms, 4, "get_spectral_candidates_ms")

    # ------------------------------------------------------------------ joint bootstrap of a spectral candidate search (kiwi_hip_spectral_candidates_bootstrap)
    def spectral_candidates_bootstrap_shape(self, K):
        """(candidates per workgroup, draws per tile, the most receivers) of the spectral bootstrap kernels for K basis sources; no
        device needed."""
        return self._read_shape(self.L.kiwi_hip_spectral_candidates_bootstrap_shape, (int(K),), 3, "spectral_candidates_bootstrap")

    def _spectral_bootstrap_arrays(self, ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group):
        """the siblings' arrays without the offsets, which this call does not have: best_offset and group_offset of the
        `CandidateBootstrap` are filled afterwards (0 where there is a best, else -1)"""
        args, out = self._candidate_bootstrap_arrays(ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group,
                                                     "spectral_candidates_bootstrap")

        def done():
            out.best_offset[:] = np.where(out.best_cand >= 0, 0, -1)
            if out.group_offset is not None:
                out.group_offset[:] = np.where(out.group_cand >= 0, 0, -1)
            return out
        return args[:9] + args[10:13] + args[14:], done          # (without best_offset and group_offset)

    def spectral_candidates_bootstrap(self, isrc0, ngroup, K, candidates, draw_weights, outer_norm="l1norm", receiver_weights=None,
                                      anarchy=False, per_group=False):
        """The bootstrap over the receivers of a candidate search under ampspec_l2norm / ampspec_l1norm, joint over group and
        candidate, on the device (kiwi_hip_spectral_candidates_bootstrap): what `spectral_candidates(..., slot_misfit=True)`
        followed by `outer_misfits_slots` with `draw_weights[ndraw, nrec]` answers, bit for bit, without the [candidate, slot]
        array leaving the device.  Returns a `CandidateBootstrap`: best_value[ndraw], best_group, best_cand[ndraw] (NaN and -1
        where every source of a draw is excluded; best_offset is 0 or -1: there are no offsets), status[ngroup]; per_group=True
        adds group_value and group_cand[ngroup, ndraw], the same per group.  A row of ones as draw 0 gives the plain winner."""
        args, done = self._spectral_bootstrap_arrays(ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group)
        self._ck(self.L.kiwi_hip_spectral_candidates_bootstrap(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "spectral_candidates_bootstrap")
        return done()

    def spectral_candidates_bootstrap_params(self, sourcetype, params, K, candidates, draw_weights, outer_norm="l1norm",
                                             receiver_weights=None, anarchy=False, per_group=False, piece=0):
        """`spectral_candidates_bootstrap` for a parameter list of any length, cut into pieces and over the devices at group
        boundaries as `linear_fit_params` cuts it; best_group counts the groups of the whole list.  Afterwards the engine holds
        the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece, "spectral_candidates_bootstrap")
        args, done = self._spectral_bootstrap_arrays(head[1], K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group)
        self._list_call(self.L.kiwi_hip_spectral_candidates_bootstrap_params, head, rows, args, "spectral_candidates_bootstrap")
        return done()

    def spectral_candidates_bootstrap_ms(self):
        """HIP-event durations [ms] of the last `spectral_candidates_bootstrap`: (evaluation, the spectra kernel, the slot kernel,
        bootstrap kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_spectral_candidates_bootstrap_ms, 5, "get_spectral_candidates_bootstrap_ms")

    # ------------------------------------------------------------------ candidates under the time-domain l1norm / l2norm (kiwi_hip_waveform_candidates)
    def waveform_candidates_shape(self, K):
        """(candidates per workgroup, samples per LDS stage) of `waveform_candidates` for K basis sources; needs no device."""
        return self._read_shape(self.L.kiwi_hip_waveform_candidates_shape, (int(K),), 2, "waveform_candidates")

    def _waveform_candidate_arrays(self, ngroup, K, candidates, outer_norm, receiver_weights, anarchy, misfit, slot_misfit):
        code, x, w = self._candidate_inputs("waveform_candidates", outer_norm, K, candidates, receiver_weights)
        ng, nc, nmis = int(ngroup), len(x), self._nslots()
        out = WaveformCandidateScan(np.zeros(ng, np.int32), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, nc)) if misfit else None,
                                    np.zeros((ng, nc, nmis), np.float32) if slot_misfit else None,
                                    np.zeros((ng, nmis), np.float32) if slot_misfit else None)
        return (nc, _dp(x), code, _dp(w), 1 if anarchy else 0, _ip(out.best_index), _dp(out.best_misfit), _ip(out.status), _dp(out.misfit),
                _fp(out.slot_misfit), _fp(out.slot_norm)), out

    def waveform_candidates(self, isrc0, ngroup, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False, misfit=True,
                            slot_misfit=False):
        """The misfits of given coefficient vectors under the time-domain l1norm / l2norm (kiwi_hip_waveform_candidates): sources
        [isrc0, isrc0 + ngroup K) are groups of K basis sources whose kept traces are combined per candidate and compared with
        the reference sample by sample.  Returns a `WaveformCandidateScan`: best_index[ngroup] (-1: none), best_misfit[ngroup],
        status[ngroup] (0 evaluated, 1 no receiver counts, 2 a basis source failed to discretise), misfit[ngroup, ncand]
        (misfit=True), slot_misfit[ngroup, ncand, nmis] and slot_norm[ngroup, nmis] float32 (slot_misfit=True: what
        `outer_misfits_slots` takes).  There is no free scale: the moment axis is more candidates."""
        args, out = self._waveform_candidate_arrays(ngroup, K, candidates, outer_norm, receiver_weights, anarchy, misfit, slot_misfit)
        self._ck(self.L.kiwi_hip_waveform_candidates(self.h, int(isrc0), int(ngroup), int(K), *args), "waveform_candidates")
        return out

    def waveform_candidates_params(self, sourcetype, params, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                                   misfit=True, slot_misfit=False, piece=0):
        """`waveform_candidates` for a parameter list of any length (kiwi_hip_waveform_candidates_params), cut into pieces and
        over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece, "waveform_candidates")
        args, out = self._waveform_candidate_arrays(head[1], K, candidates, outer_norm, receiver_weights, anarchy, misfit, slot_misfit)
        self._list_call(self.L.kiwi_hip_waveform_candidates_params, head, rows, args, "waveform_candidates")
        return out

    def waveform_candidates_ms(self):
        """HIP-event durations [ms] of the last `waveform_candidates`: (evaluation, the slot kernel, the fold kernels, downloads);
        the host's tables of a chunk and their upload lie between the first two, in neither."""
        return self._read_ms(self.L.kiwi_hip_get_waveform_candidates_ms, 4, "get_waveform_candidates_ms")

    # ------------------------------------------------------------------ candidates under floating_l1norm / floating_l2norm (kiwi_hip_waveform_candidates_floating)
    def waveform_candidates_floating_shape(self, K):
        """(candidates per workgroup, samples per LDS stage, shifts per pass) of `waveform_candidates_floating` for K basis sources;
        needs no device."""
        return self._read_shape(self.L.kiwi_hip_waveform_candidates_floating_shape, (int(K),), 3, "waveform_candidates_floating")

    def _waveform_candidate_floating_arrays(self, ngroup, K, candidates, outer_norm, receiver_weights, anarchy, misfit, cand_shift,
                                            slot_misfit):
        code, x, w = self._candidate_inputs("waveform_candidates_floating", outer_norm, K, candidates, receiver_weights)
        ng, nc, nrec, nmis = int(ngroup), len(x), len(self.components), self._nslots()
        out = WaveformCandidateFloatingScan(np.zeros(ng, np.int32), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, nrec), np.int32),
                                            np.zeros((ng, nc)) if misfit else None, np.zeros((ng, nc, nrec), np.int16) if cand_shift else None,
                                            np.zeros((ng, nc, nmis), np.float32) if slot_misfit else None,
                                            np.zeros((ng, nmis), np.float32) if slot_misfit else None)
        return (nc, _dp(x), code, _dp(w), 1 if anarchy else 0, _ip(out.best_index), _dp(out.best_misfit), _ip(out.status),
                _ip(out.best_shift), _dp(out.misfit), _sp(out.cand_shift), _fp(out.slot_misfit), _fp(out.slot_norm)), out

    def waveform_candidates_floating(self, isrc0, ngroup, K, candidates, outer_norm="l1norm", receiver_weights=None, anarchy=False,
                                     misfit=True, cand_shift=False, slot_misfit=False):
        """`waveform_candidates` under floating_l1norm / floating_l2norm (kiwi_hip_waveform_candidates_floating): per receiver and
        candidate the reference slides under the fixed taper by the whole-sample shifts of the receiver's range
        (`set_floating_shiftrange`), and the shift with the smallest sum over the receiver's slots wins, as in `eval`.  Returns
        a `WaveformCandidateFloatingScan`: best_index[ngroup] (-1: none), best_misfit[ngroup], status[ngroup] (0 evaluated, 1 no
        receiver counts, 2 a basis source failed to discretise), best_shift[ngroup, nrec] (samples; 0 for a disabled receiver),
        misfit[ngroup, ncand] (misfit=True), cand_shift[ngroup, ncand, nrec] int16 (cand_shift=True, needs misfit),
        slot_misfit[ngroup, ncand, nmis] and slot_norm[ngroup, nmis] float32 (slot_misfit=True: what `outer_misfits_slots`
        takes).  There is no free scale."""
        args, out = self._waveform_candidate_floating_arrays(ngroup, K, candidates, outer_norm, receiver_weights, anarchy, misfit, cand_shift,
                                                             slot_misfit)
        self._ck(self.L.kiwi_hip_waveform_candidates_floating(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "waveform_candidates_floating")
        return out

    def waveform_candidates_floating_params(self, sourcetype, params, K, candidates, outer_norm="l1norm", receiver_weights=None,
                                            anarchy=False, misfit=True, cand_shift=False, slot_misfit=False, piece=0):
        """`waveform_candidates_floating` for a parameter list of any length (kiwi_hip_waveform_candidates_floating_params), cut
        into pieces and over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece, "waveform_candidates_floating")
        args, out = self._waveform_candidate_floating_arrays(head[1], K, candidates, outer_norm, receiver_weights, anarchy, misfit, cand_shift,
                                                             slot_misfit)
        self._list_call(self.L.kiwi_hip_waveform_candidates_floating_params, head, rows, args, "waveform_candidates_floating")
        return out

    def waveform_candidates_floating_ms(self):
        """HIP-event durations [ms] of the last `waveform_candidates_floating`: (evaluation, the floating slot kernel, the fold
        kernels, downloads); the host's tables of a chunk and their upload lie between the first two, in neither."""
        return self._read_ms(self.L.kiwi_hip_get_waveform_candidates_floating_ms, 4, "get_waveform_candidates_floating_ms")

    # ------------------------------------------------------------------ l1norm / l2norm candidates at many origin times (kiwi_hip_waveform_candidates_time_scan)
    def waveform_candidates_time_scan_shape(self, K):
        """(candidates per workgroup, extended samples per LDS stage, offsets per pass) of `waveform_candidates_time_scan` for K
        basis sources; needs no device."""
        return self._read_shape(self.L.kiwi_hip_waveform_candidates_time_scan_shape, (int(K),), 3, "waveform_candidates_time_scan")

    def waveform_candidates_time_scan_rows(self, k0, kstep, nk):
        """The layout of the `rows` array of `waveform_candidates_time_scan` for these offsets: (S = max |k|, floats per basis
        source, row_offset[nmis]); extended sample e of slot m lies at row_offset[m] + S + e."""
        nmis = self._nslots()
        S, stride, ofs = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(max(nmis, 1), np.int32)
        self._ck(self.L.kiwi_hip_waveform_candidates_time_scan_rows(self.h, int(k0), int(kstep), int(nk), _ip(S), _ip(stride), _ip(ofs)),
                 "waveform_candidates_time_scan")
        return int(S[0]), int(stride[0]), ofs[:nmis].copy()

    def _waveform_candidate_time_scan_arrays(self, ngroup, K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy, cand_misfit,
                                             cand_offset, misfit, slot_misfit, rows):
        code, x, w = self._candidate_inputs("waveform_candidates_time_scan", outer_norm, K, candidates, receiver_weights)
        ng, K, nk, nc, nmis = int(ngroup), int(K), int(nk), len(x), self._nslots()
        nj = max(nk, 0)                              # (a bad nk is refused by the library, by name)
        S, row_offset, rows_a = 0, None, None
        if rows:
            S, stride, row_offset = self.waveform_candidates_time_scan_rows(k0, kstep, nk)
            rows_a = np.zeros((ng, K, stride), np.float32)
        out = WaveformCandidateTimeScan(np.zeros(ng, np.int32), np.zeros((ng, nj), np.int32), np.zeros((ng, nj)), np.zeros(ng, np.int32),
                                        np.zeros((ng, nc)) if cand_misfit else None, np.zeros((ng, nc), np.int32) if cand_offset else None,
                                        np.zeros((ng, nj, nc)) if misfit else None,
                                        np.zeros((ng, nj, nc, nmis), np.float32) if slot_misfit else None,
                                        np.zeros((ng, nmis), np.float32) if slot_misfit else None, rows_a, S, row_offset)
        return (int(k0), int(kstep), nk, nc, _dp(x), code, _dp(w), 1 if anarchy else 0, _ip(out.best_offset), _ip(out.best_index),
                _dp(out.best_misfit), _ip(out.status), _dp(out.cand_misfit), _ip(out.cand_offset), _dp(out.misfit), _fp(out.slot_misfit),
                _fp(out.slot_norm), _fp(out.rows)), out

    def waveform_candidates_time_scan(self, isrc0, ngroup, K, k0, kstep, nk, candidates, outer_norm="l1norm", receiver_weights=None,
                                      anarchy=False, cand_misfit=True, cand_offset=True, misfit=False, slot_misfit=False, rows=False):
        """`waveform_candidates` at the nk origin-time offsets k0 + j kstep samples from ONE synthesis of the basis
        (kiwi_hip_waveform_candidates_time_scan): the combined untapered trace of a candidate is read k samples earlier under the
        receiver's fixed taper, against the tapered reference.  Returns a `WaveformCandidateTimeScan`: best_offset[ngroup] (an index j;
        -1: none), best_index[ngroup, nk], best_misfit[ngroup, nk], status[ngroup], cand_misfit and cand_offset[ngroup, ncand] (per
        candidate the first smallest misfit over the offsets and its index), misfit[ngroup, nk, ncand] (misfit=True),
        slot_misfit[ngroup, nk, ncand, nmis] and slot_norm[ngroup, nmis] float32 (slot_misfit=True: with nk x ncand read as sources
        what `outer_misfits_slots` takes), rows[ngroup, K, row_stride] with shift_halo and row_offset (rows=True: the folded, scaled,
        untapered rows of the basis sources, `waveform_candidates_time_scan_rows`).  Offset 0 agrees with `waveform_candidates` to
        rounding, not bit for bit (this call combines, then tapers)."""
        args, out = self._waveform_candidate_time_scan_arrays(ngroup, K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy,
                                                              cand_misfit, cand_offset, misfit, slot_misfit, rows)
        self._ck(self.L.kiwi_hip_waveform_candidates_time_scan(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "waveform_candidates_time_scan")
        return out

    def waveform_candidates_time_scan_params(self, sourcetype, params, K, k0, kstep, nk, candidates, outer_norm="l1norm",
                                             receiver_weights=None, anarchy=False, cand_misfit=True, cand_offset=True, misfit=False,
                                             slot_misfit=False, rows=False, piece=0):
        """`waveform_candidates_time_scan` for a parameter list of any length (kiwi_hip_waveform_candidates_time_scan_params), cut
        into pieces and over devices as `waveform_candidates_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, nrow = self._list_head(sourcetype, params, K, piece, "waveform_candidates_time_scan")
        args, out = self._waveform_candidate_time_scan_arrays(head[1], K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy,
                                                              cand_misfit, cand_offset, misfit, slot_misfit, rows)
        self._list_call(self.L.kiwi_hip_waveform_candidates_time_scan_params, head, nrow, args, "waveform_candidates_time_scan")
        return out

    def waveform_candidates_time_scan_ms(self):
        """HIP-event durations [ms] of the last `waveform_candidates_time_scan`: (evaluation, the rows and scan kernels, the fold
        kernels, downloads); the host's tables of a chunk and their upload lie between the first two, in neither."""
        return self._read_ms(self.L.kiwi_hip_get_waveform_candidates_time_scan_ms, 4, "get_waveform_candidates_time_scan_ms")

    # ------------------------------------------------------------------ joint bootstrap of a waveform candidate search (kiwi_hip_waveform_candidates_bootstrap)
    def waveform_candidates_bootstrap_shape(self, K):
        """(candidates per workgroup, draws per tile, the most receivers) of the waveform bootstrap kernel for K basis sources; no
        device needed."""
        return self._read_shape(self.L.kiwi_hip_waveform_candidates_bootstrap_shape, (int(K),), 3, "waveform_candidates_bootstrap")

    def waveform_candidates_bootstrap(self, isrc0, ngroup, K, candidates, draw_weights, k0=0, kstep=1, nk=1, outer_norm="l1norm",
                                      receiver_weights=None, anarchy=False, per_group=False):
        """The bootstrap over the receivers of a waveform candidate search (l1norm or l2norm inside), joint over group, origin-time
        offset and candidate, on the device (kiwi_hip_waveform_candidates_bootstrap): what
        `waveform_candidates_time_scan(..., slot_misfit=True)` followed by `outer_misfits_slots` with `draw_weights[ndraw, nrec]`
        answers, bit for bit, without the [candidate, slot] array leaving the device.  Returns a `CandidateBootstrap`:
        best_value[ndraw], best_group, best_offset, best_cand[ndraw] (NaN and -1 where every source of a draw is excluded),
        status[ngroup]; per_group=True adds group_value, group_offset and group_cand[ngroup, ndraw], the same per group.  A row of
        ones as draw 0 gives the plain winner."""
        args, out = self._candidate_bootstrap_arrays(ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group,
                                                     "waveform_candidates_bootstrap")
        self._ck(self.L.kiwi_hip_waveform_candidates_bootstrap(self.h, int(isrc0), int(ngroup), int(K), int(k0), int(kstep), int(nk), *args),
                 "waveform_candidates_bootstrap")
        return out

    def waveform_candidates_bootstrap_params(self, sourcetype, params, K, candidates, draw_weights, k0=0, kstep=1, nk=1,
                                             outer_norm="l1norm", receiver_weights=None, anarchy=False, per_group=False, piece=0):
        """`waveform_candidates_bootstrap` for a parameter list of any length, cut into pieces and over the devices at group
        boundaries as `linear_fit_params` cuts it; best_group counts the groups of the whole list.  Afterwards the engine holds
        the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece, "waveform_candidates_bootstrap")
        args, out = self._candidate_bootstrap_arrays(head[1], K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group,
                                                     "waveform_candidates_bootstrap")
        self._list_call(self.L.kiwi_hip_waveform_candidates_bootstrap_params, head, rows, (int(k0), int(kstep), int(nk)) + args,
                        "waveform_candidates_bootstrap")
        return out

    def waveform_candidates_bootstrap_ms(self):
        """HIP-event durations [ms] of the last `waveform_candidates_bootstrap`: (evaluation, the rows and scan kernels, the fold
        kernels, bootstrap kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_waveform_candidates_bootstrap_ms, 5, "get_waveform_candidates_bootstrap_ms")

    # ------------------------------------------------------------------ candidates at many origin times (kiwi_hip_linear_fit_candidates_time_scan)
    def linear_fit_candidates_time_scan_shape(self, K):
        """(candidates per workgroup, receivers per LDS stage) of the candidate-scan kernel for K basis sources."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_candidates_time_scan_shape, (int(K),), 2, "linear_fit")

    def _candidate_scan_arrays(self, ngroup, K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy, free_scale, marginal, misfit,
                               receiver_misfit):
        code, x, w = self._candidate_inputs("linear_fit_candidates_time_scan", outer_norm, K, candidates, receiver_weights,
                                            krange="linear_fit")
        ng, K, nj, nc, nrec = int(ngroup), int(K), max(int(nk), 0), len(x), len(self.components)
        free = bool(free_scale)
        out = CandidateTimeScan(np.zeros(ng, np.int32), np.zeros((ng, nj), np.int32), np.zeros((ng, nj)),
                                np.zeros((ng, nj)) if free else None, np.zeros(ng, np.int32),
                                np.zeros((ng, nc)) if marginal else None, np.zeros((ng, nc), np.int32) if marginal else None,
                                np.zeros((ng, nc)) if marginal and free else None,
                                np.zeros((ng, nj, nc)) if misfit else None, np.zeros((ng, nj, nc)) if misfit and free else None,
                                np.zeros((ng, nj, nc, nrec), np.float32) if receiver_misfit else None,
                                np.zeros((ng, nrec), np.float32) if receiver_misfit else None,
                                np.zeros((ng, nj, K)), np.zeros((ng, nj)), np.zeros((ng, nj), np.int32))
        return (int(k0), int(kstep), int(nk), nc, _dp(x), code, _dp(w), 1 if anarchy else 0, 1 if free_scale else 0, _ip(out.best_offset),
                _ip(out.best_index), _dp(out.best_misfit), _dp(out.best_scale), _ip(out.status), _dp(out.cand_misfit), _ip(out.cand_offset),
                _dp(out.cand_scale), _dp(out.misfit), _dp(out.scale), _fp(out.receiver_misfit), _fp(out.receiver_norm), _dp(out.fit_coef),
                _dp(out.fit_misfit), _ip(out.fit_status)), out

    def linear_fit_candidates_time_scan(self, isrc0, ngroup, K, candidates, k0=0, kstep=1, nk=1, outer_norm="l1norm", receiver_weights=None,
                                        anarchy=False, free_scale=False, marginal=True, misfit=False, receiver_misfit=False):
        """`linear_fit_candidates` at the origin-time offsets (k0 + j kstep) dt, j < nk, from ONE synthesis of the basis sources
        (kiwi_hip_linear_fit_candidates_time_scan): `linear_fit_time_scan`'s sums per offset, `linear_fit_candidates`' evaluation
        on them.  Returns a `CandidateTimeScan`: best_offset[ngroup] (-1: none), best_index[ngroup, nk] (-1: none),
        best_misfit[ngroup, nk], best_scale[ngroup, nk] (free_scale), status[ngroup]; cand_misfit, cand_offset[ngroup, ncand]
        (marginal=True: every candidate's smallest misfit over the offsets and where) and cand_scale (free_scale);
        misfit[ngroup, nk, ncand] (misfit=True) and scale (free_scale); receiver_misfit[ngroup, nk, ncand, nrec] and
        receiver_norm[ngroup, nrec] float32 (receiver_misfit=True); fit_coef[ngroup, nk, K], fit_misfit and fit_status[ngroup, nk]:
        `linear_fit_time_scan` of the same groups.  Arrays not asked for are None."""
        args, out = self._candidate_scan_arrays(ngroup, K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy, free_scale,
                                                marginal, misfit, receiver_misfit)
        self._ck(self.L.kiwi_hip_linear_fit_candidates_time_scan(self.h, int(isrc0), int(ngroup), int(K), *args),
                 "linear_fit_candidates_time_scan")
        return out

    def linear_fit_candidates_time_scan_params(self, sourcetype, params, K, candidates, k0=0, kstep=1, nk=1, outer_norm="l1norm",
                                               receiver_weights=None, anarchy=False, free_scale=False, marginal=True, misfit=False,
                                               receiver_misfit=False, piece=0):
        """`linear_fit_candidates_time_scan` for a parameter list of any length, cut into pieces and over the devices at group
        boundaries as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._candidate_scan_arrays(head[1], K, k0, kstep, nk, candidates, outer_norm, receiver_weights, anarchy, free_scale,
                                                marginal, misfit, receiver_misfit)
        self._list_call(self.L.kiwi_hip_linear_fit_candidates_time_scan_params, head, rows, args, "linear_fit_candidates_time_scan")
        return out

    def linear_fit_candidates_time_scan_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_candidates_time_scan`: (evaluation, Gram-scan kernel, solve kernels,
        candidate-scan kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_candidates_time_scan_ms, 5, "get_linear_fit_candidates_time_scan_ms")

    # ------------------------------------------------------------------ joint bootstrap of a candidate search (kiwi_hip_linear_fit_candidates_bootstrap)
    def linear_fit_candidates_bootstrap_shape(self, K):
        """(candidates per workgroup, draws per tile, the most receivers) of the bootstrap kernel for K basis sources; no device
        needed."""
        return self._read_shape(self.L.kiwi_hip_linear_fit_candidates_bootstrap_shape, (int(K),), 3, "linear_fit")

    def _candidate_bootstrap_arrays(self, ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group,
                                    name="linear_fit_candidates_bootstrap"):
        code, x, w, dw = self._candidate_inputs(name, outer_norm, K, candidates, receiver_weights, draw_weights, krange="linear_fit")
        ng, nd = int(ngroup), len(dw)
        grp = (ng, nd) if per_group else None
        out = CandidateBootstrap(np.zeros(nd), np.zeros(nd, np.int32), np.zeros(nd, np.int32), np.zeros(nd, np.int32), np.zeros(ng, np.int32),
                                 np.zeros(grp) if grp else None, np.zeros(grp, np.int32) if grp else None,
                                 np.zeros(grp, np.int32) if grp else None)
        return (len(x), _dp(x), code, _dp(w), 1 if anarchy else 0, nd, _dp(dw), _dp(out.best_value), _ip(out.best_group),
                _ip(out.best_offset), _ip(out.best_cand), _ip(out.status), _dp(out.group_value), _ip(out.group_offset),
                _ip(out.group_cand)), out

    def linear_fit_candidates_bootstrap(self, isrc0, ngroup, K, candidates, draw_weights, k0=0, kstep=1, nk=1, outer_norm="l1norm",
                                        receiver_weights=None, anarchy=False, per_group=False):
        """The bootstrap over the receivers of a candidate search, joint over group, origin-time offset and candidate, on the
        device (kiwi_hip_linear_fit_candidates_bootstrap): what `linear_fit_candidates_time_scan(..., receiver_misfit=True)`
        followed by `outer_misfits` with `draw_weights[ndraw, nrec]` answers, bit for bit, without the [candidate, receiver]
        matrix.  Returns a `CandidateBootstrap`: best_value[ndraw], best_group, best_offset, best_cand[ndraw] (NaN and -1 where
        every source of a draw is excluded), status[ngroup]; per_group=True adds group_value, group_offset and
        group_cand[ngroup, ndraw], the same per group.  A row of ones as draw 0 gives the plain winner."""
        args, out = self._candidate_bootstrap_arrays(ngroup, K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group)
        self._ck(self.L.kiwi_hip_linear_fit_candidates_bootstrap(self.h, int(isrc0), int(ngroup), int(K), int(k0), int(kstep), int(nk), *args),
                 "linear_fit_candidates_bootstrap")
        return out

    def linear_fit_candidates_bootstrap_params(self, sourcetype, params, K, candidates, draw_weights, k0=0, kstep=1, nk=1,
                                               outer_norm="l1norm", receiver_weights=None, anarchy=False, per_group=False, piece=0):
        """`linear_fit_candidates_bootstrap` for a parameter list of any length, cut into pieces and over the devices at group
        boundaries as `linear_fit_params` cuts it; best_group counts the groups of the whole list.  Afterwards the engine holds
        the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._candidate_bootstrap_arrays(head[1], K, candidates, draw_weights, outer_norm, receiver_weights, anarchy, per_group)
        self._list_call(self.L.kiwi_hip_linear_fit_candidates_bootstrap_params, head, rows, (int(k0), int(kstep), int(nk)) + args,
                        "linear_fit_candidates_bootstrap")
        return out

    def linear_fit_candidates_bootstrap_ms(self):
        """HIP-event durations [ms] of the last `linear_fit_candidates_bootstrap`: (evaluation, Gram-scan kernel, solve kernels,
        bootstrap kernels, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_candidates_bootstrap_ms, 5, "get_linear_fit_candidates_bootstrap_ms")

    # ------------------------------------------------------------------ robust linear fit (kiwi_hip_linear_fit_robust)
    def _robust_fit_arrays(self, ngroup, K, outer_norm, receiver_weights, anarchy, niter, eps):
        code = _outer_code(outer_norm)
        K, ng = self._basis_count(K, "linear_fit"), int(ngroup)
        w = self._receiver_weights(receiver_weights)
        out = RobustFit(np.zeros((ng, K)), np.zeros(ng), np.zeros(ng, np.int32), np.zeros((ng, max(int(niter), 0) + 1, 2)))
        return (code, _dp(w), 1 if anarchy else 0, int(niter), float(eps), _dp(out.coef), _dp(out.misfit), _ip(out.status),
                _dp(out.trace)), out

    def linear_fit_robust(self, isrc0, ngroup, K, outer_norm="l1norm", receiver_weights=None, anarchy=False, niter=8, eps=1e-3):
        """`linear_fit` under an l1 outer norm by iteratively reweighted least squares on the device
        (kiwi_hip_linear_fit_robust); the inner norm is the engine's misfit method: l2norm (the receivers' l2 misfits are
        summed) or l1norm (the samples' absolute residuals are).  `niter` reweighted solves from the l2 solution; `eps`
        (relative) bounds the weights.  outer_norm="l2norm" with the method l2norm forwards to `linear_fit`.  Returns a
        `RobustFit`: coef[ngroup, K], misfit[ngroup] (the global misfit under the two norms), status[ngroup] (0 solved, 1 no
        l2 start, 2 a basis source failed to discretise, 3 a reweighted system broke down: coef and misfit of the iterate
        before), trace[ngroup, niter + 1, 2] ((smoothed objective, misfit) per iterate)."""
        args, out = self._robust_fit_arrays(ngroup, K, outer_norm, receiver_weights, anarchy, niter, eps)
        self._ck(self.L.kiwi_hip_linear_fit_robust(self.h, int(isrc0), int(ngroup), int(K), *args), "linear_fit_robust")
        return out

    def linear_fit_robust_params(self, sourcetype, params, K, outer_norm="l1norm", receiver_weights=None, anarchy=False, niter=8,
                                 eps=1e-3, piece=0):
        """`linear_fit_robust` for a parameter list of any length (kiwi_hip_linear_fit_robust_params), cut into pieces and
        over devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._robust_fit_arrays(head[1], K, outer_norm, receiver_weights, anarchy, niter, eps)
        self._list_call(self.L.kiwi_hip_linear_fit_robust_params, head, rows, args, "linear_fit_robust")
        return out

    def linear_fit_robust_ms(self):
        """HIP-event durations [ms] of the last linear fit of either kind: (evaluation, l2 start, reweighting passes, downloads)."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_robust_ms, 4, "get_linear_fit_robust_ms")

    # ------------------------------------------------------------------ wide linear fit (kiwi_hip_linear_fit_wide)
    def linear_fit_wide_max_basis(self):
        """The most basis sources per group `linear_fit_wide` takes."""
        return int(self.L.kiwi_hip_linear_fit_wide_max_basis())

    def linear_fit_wide_ms(self):
        """HIP-event durations [ms] of the last wide linear fit: (Gram kernels, solve kernel); `linear_fit_ms` has their sum."""
        return self._read_ms(self.L.kiwi_hip_get_linear_fit_wide_ms, 2, "get_linear_fit_wide_ms")

    def _wide_fit_arrays(self, ngroup, K, receiver_weights, anarchy, nonneg, penalty, penalty_relative, normal, by_receiver):
        K, ngroup = self._basis_count(K, "linear_fit", self.linear_fit_wide_max_basis()), int(ngroup)
        nrec, ng, nn = len(self.components), K * (K + 1) // 2, K * (K + 1) // 2 + K + 1
        w = self._receiver_weights(receiver_weights)
        pen = None
        if penalty is not None:
            pen = np.ascontiguousarray(penalty, np.float64)
            if pen.shape == (K, K):
                if not np.array_equal(pen, pen.T):
                    raise KiwiHipError("linear_fit_wide: the penalty matrix is not symmetric")
                pen = np.ascontiguousarray(pen[np.triu_indices(K)])
            if pen.shape != (ng,):
                raise KiwiHipError("linear_fit_wide: the penalty must be [K, K] or the upper triangle by rows [K (K + 1) / 2]")
        out = WideFit(np.zeros((ngroup, K)), np.zeros(ngroup), np.zeros(ngroup, np.int32), np.zeros(ngroup),
                      np.zeros((ngroup, nn)) if normal else None, np.zeros((ngroup, nrec, nn)) if by_receiver else None,
                      np.zeros(ngroup, np.int32), np.zeros(ngroup, np.int32))
        code = nonneg if isinstance(nonneg, (int, np.integer)) and not isinstance(nonneg, bool) else (1 if nonneg else 0)
        return (_dp(w), 1 if anarchy else 0, int(code), _dp(pen), 1 if penalty_relative else 0, _dp(out.coef), _dp(out.misfit),
                _ip(out.status), _dp(out.pivot_min), _ip(out.npositive), _ip(out.nsolves), _dp(out.normal), _dp(out.by_receiver)), out

    def linear_fit_wide(self, isrc0, ngroup, K, receiver_weights=None, anarchy=False, nonneg=False, penalty=None,
                        penalty_relative=False, normal=False, by_receiver=False):
        """`linear_fit` for up to 64 basis sources per group (kiwi_hip_linear_fit_wide), optionally with a quadratic `penalty`
        ([K, K] symmetric, or its upper triangle by rows; added to the folded normal matrix as given, or, `penalty_relative`,
        times the mean of its diagonal) and with non-negative coefficients (`nonneg`: the active-set method of Lawson and
        Hanson, on the device).  Returns a `WideFit`: the fields of `LinearFit` (misfit: the DATA misfit; normal: the sums
        without the penalty; status additionally 4: the cap of 3 K solves was reached) plus npositive[ngroup] (coefficients
        > 0) and nsolves[ngroup] (Cholesky solves made)."""
        args, out = self._wide_fit_arrays(ngroup, K, receiver_weights, anarchy, nonneg, penalty, penalty_relative, normal, by_receiver)
        self._ck(self.L.kiwi_hip_linear_fit_wide(self.h, int(isrc0), int(ngroup), int(K), *args), "linear_fit_wide")
        return out

    def linear_fit_wide_params(self, sourcetype, params, K, receiver_weights=None, anarchy=False, nonneg=False, penalty=None,
                               penalty_relative=False, normal=False, by_receiver=False, piece=0):
        """`linear_fit_wide` for a parameter list of any length (kiwi_hip_linear_fit_wide_params), cut into pieces and over
        devices as `linear_fit_params` cuts it.  Afterwards the engine holds the head of the list."""
        head, rows = self._list_head(sourcetype, params, K, piece)
        args, out = self._wide_fit_arrays(head[1], K, receiver_weights, anarchy, nonneg, penalty, penalty_relative, normal, by_receiver)
        self._list_call(self.L.kiwi_hip_linear_fit_wide_params, head, rows, args, "linear_fit_wide")
        return out

def bootstrap_draw_weights(nrec, ndraw, rng, receiver_mask=None, receiver_weights=None):
    """The resampling counts of `ndraw` bootstrap draws over the enabled receivers, [ndraw, nrec] float64: row d is the
    `bweights` of the d-th successive `make_global_misfits(..., bootstrap=True, rng=rng)` call.  The generator is consumed
    exactly as those calls consume it: one `rng.integers(0, ne, ne)` per draw.  (One `rng.integers(0, ne, (ndraw, ne))`
    yields the same values but can leave the generator's buffered 32-bit half in another state, so whatever the caller drew
    next would differ.)  The device path and the host path so see the same draws from equally seeded generators, and leave
    them alike (tests/test_outer_bootstrap.py)."""
    mask = np.ones(nrec, bool) if receiver_mask is None else np.asarray(receiver_mask, bool)
    if receiver_weights is not None:
        w = np.broadcast_to(np.asarray(receiver_weights, np.float64), (nrec,))
        mask = np.logical_and(mask, w != 0)
    enabled = np.arange(nrec)[mask]
    ne = len(enabled)
    out = np.zeros((ndraw, nrec), np.float64)
    for d in range(ndraw):
        out[d] = np.bincount(enabled[rng.integers(0, ne, ne)], minlength=nrec)
    return out


def make_global_misfits(misfits_by_src, norms_by_src, outer_norm="l2norm", receiver_weights=None, receiver_mask=None,
                        anarchy=False, bootstrap=False, rng=None):
    """seismosizer.py:843-922: per-source global misfit and per source-receiver misfits from [N_s,N_r,N_k]
    arrays, float64.  `anarchy` divides each receiver's weight by its norm (:884-888); `bootstrap` multiplies
    the weights by a resampling count drawn over the enabled receivers (:855-869; sqrt of it for l2, :901-902).
    Differences, deliberate: the reference draws from numpy's global RandomState -- pass `rng` (a
    numpy Generator) for reproducible draws; its anarchy + per-receiver-weights combination under l2norm
    raises a broadcasting error for more than one source (:898), here it works as under l1norm."""
    m = np.asarray(misfits_by_src, np.float64)
    n = np.asarray(norms_by_src, np.float64)
    nrec = m.shape[1]
    w = np.ones(nrec) if receiver_weights is None else np.broadcast_to(np.asarray(receiver_weights, np.float64), (nrec,))
    rweights = np.tile(w, (m.shape[0], 1))
    if bootstrap:
        mask = np.ones(nrec, bool) if receiver_mask is None else np.asarray(receiver_mask, bool)
        if receiver_weights is not None:
            mask = np.logical_and(mask, w != 0)
        enabled = np.arange(nrec)[mask]
        rng = np.random.default_rng() if rng is None else rng
        draw = enabled[rng.integers(0, len(enabled), len(enabled))]
        bweights = np.bincount(draw, minlength=nrec).astype(np.float64)
    if outer_norm == "l1norm":
        m_sr, n_sr = m.sum(2), n.sum(2)
    elif outer_norm == "l2norm":
        m_sr, n_sr = np.sqrt((m ** 2).sum(2)), np.sqrt((n ** 2).sum(2))
    else:
        raise KiwiHipError("unknown norm method: %s" % outer_norm)
    if anarchy:
        rweights = np.maximum(rweights / np.where(n_sr != 0., n_sr, -1.), 0.)
    if bootstrap:
        rweights = rweights * (bweights if outer_norm == "l1norm" else np.sqrt(bweights))
    m_sr = m_sr * rweights
    n_sr = n_sr * rweights
    with np.errstate(divide="ignore", invalid="ignore"):
        if outer_norm == "l1norm":
            ms, ns = m_sr.sum(1), n_sr.sum(1)
            g = np.where(ns > 0, ms / ns, -1.)
        else:
            ms, ns = (m_sr ** 2).sum(1), (n_sr ** 2).sum(1)
            g = np.where(ns > 0, np.sqrt(ms / ns), -1.)
    return np.where(g < 0, np.nan, g), m_sr
