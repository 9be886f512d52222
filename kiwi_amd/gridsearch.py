"""Trial-source grids and the brute-force grid search on top of the batched engine: the Python-3
counterpart of python/tunguska/source.py:119-164 (`Source.grid`) and gridsearch.py:19-23,111-289
(`mimainc_to_gvals`, `MisfitGrid` with bootstrap).  The ordering defined here is the shard ordering of
kiwi_amd/shard.py: the first grid parameter varies slowest."""
import numpy as np

from .engine import SOURCE_TYPES, bootstrap_draw_weights, make_global_misfits
from .lib import KiwiHipError

# wire order of set_source_params (source_bilat.f90:93-106, source_circular.f90:92-102, source_eikonal.f90:97-114,
# source_mt_eikonal.f90:102-124, source_moment_tensor.f90:90-100)
SOURCE_PARAMS = {
    "bilateral": ["time", "north-shift", "east-shift", "depth", "moment", "strike", "dip", "slip-rake", "rupture-rake",
                  "length-a", "length-b", "width", "rupture-velocity", "rise-time"],
    "circular": ["time", "north-shift", "east-shift", "depth", "moment", "strike", "dip", "slip-rake", "radius",
                 "rupture-velocity", "rise-time"],
    "eikonal": ["time", "north-shift", "east-shift", "depth", "moment", "strike", "dip", "slip-rake", "bord-shift-x",
                "bord-shift-y", "bord-radius", "nukl-shift-x", "nukl-shift-y", "rel-rupture-velocity", "rise-time"],
    "mt_eikonal": ["time", "north-shift", "east-shift", "depth", "moment-factor", "strike", "dip", "bord-shift-x",
                   "bord-shift-y", "bord-radius", "nukl-shift-x", "nukl-shift-y", "rel-rupture-velocity", "mxx", "myy",
                   "mzz", "mxy", "mxz", "myz", "rise-time"],
    "moment_tensor": ["time", "north-shift", "east-shift", "depth", "mxx", "myy", "mzz", "mxy", "mxz", "myz", "rise-time"],
    "point_lp": ["time", "north-shift", "east-shift", "depth", "moment", "m_xx", "m_yy", "m_zz", "m_xy", "m_xz", "m_yz",
                 "excitation-time", "main-period"],                                     # source_point_lp.f90:110-122
}


def mimainc_to_gvals(mi, ma, inc):
    """gridsearch.py:19-23: n = round((max-min)/inc)+1 equally spaced values including both ends."""
    vmin, vmax, vinc = float(mi), float(ma), float(inc)
    n = int(round((vmax - vmin) / vinc)) + 1
    if n == 1:
        return np.array([vmin])
    vinc = (vmax - vmin) / (n - 1)
    return np.array([vmin + i * vinc for i in range(n)], np.float64)


def source_grid(sourcetype, base_params, grid_definition, source_constraints=None):
    """source.py:119-164: all combinations of [(parameter, values), ...] applied to the base source, first
    parameter slowest; `source_constraints(dict)` may switch grid nodes off.  Returns params[n, nparams]
    (float32, wire order)."""
    names = SOURCE_PARAMS[sourcetype]
    base = np.asarray(base_params, np.float64)
    if base.shape != (len(names),):
        raise KiwiHipError("%s takes %d parameters" % (sourcetype, len(names)))
    cols = []
    for key, _ in grid_definition:
        if key not in names:
            raise KiwiHipError("unknown parameter '%s' for source type %s" % (key, sourcetype))
        cols.append(names.index(key))
    vals = [np.asarray(v, np.float64).ravel() for _, v in grid_definition]
    if not vals:
        return np.zeros((0, len(names)), np.float32)
    mesh = np.meshgrid(*vals, indexing="ij")                 # first parameter slowest
    n = mesh[0].size
    out = np.tile(base, (n, 1))
    for c, mg in zip(cols, mesh):
        out[:, c] = mg.ravel()
    if source_constraints is not None:
        keep = [bool(source_constraints(dict(zip(names, row)))) for row in out]
        out = out[np.array(keep, bool)]
    return out.astype(np.float32)


def split_time_axis(values, dt):
    """(k0, kstep, nk) when the time axis `values` is evenly spaced by a whole number of samples of `dt` -- (v - v[0]) / dt is an
    integer in fp32 for every value, checked exactly, the integers ascending in equal steps --, so that Engine.time_scan at
    values[0] covers it; None otherwise.  A single value: (0, 1, 1)."""
    v = np.asarray(values, np.float32).ravel()
    if v.size == 0:
        return None
    q = (v - v[0]) / np.float32(dt)                       # fp32 throughout, as the engine takes its times
    k = np.rint(q)
    if not np.all(np.isfinite(q)) or np.any(q != k) or np.any(np.abs(k) > 2 ** 24):
        return None
    k = k.astype(np.int64)
    if v.size == 1:
        return 0, 1, 1
    step = int(k[1] - k[0])
    if step < 1 or np.any(np.diff(k) != step):
        return None
    return 0, step, int(v.size)


class MisfitGridStats:
    """gridsearch.py:45-105 (the numbers, not the plots)."""

    def __init__(self, paramname, best, distribution, tested_values=None):
        self.paramname, self.best, self.tested_values = paramname, best, tested_values
        self.distribution = np.asarray(distribution, np.float64)
        self.mean = float(self.distribution.mean()) if self.distribution.size else float("nan")
        self.std = float(self.distribution.std()) if self.distribution.size else float("nan")

    def converged(self):
        return self.distribution.size > 0 and np.all(self.distribution == self.distribution[0])


class MisfitGrid:
    """Brute force grid search minimizer with builtin bootstrapping (gridsearch.py:111-289)."""

    def __init__(self, sourcetype, base_params, param_ranges=None, param_values=None, source_constraints=None,
                 ref_params=None):
        self.sourcetype = sourcetype
        self.base_params = np.asarray(base_params, np.float32)
        self.ref_params = self.base_params if ref_params is None else np.asarray(ref_params, np.float32)
        if param_values is not None:
            self.param_values = [(p, np.asarray(v, np.float64)) for p, v in param_values]
        else:
            self.param_values = [(p, mimainc_to_gvals(mi, ma, inc)) for p, mi, ma, inc in param_ranges]
        self.sources = source_grid(sourcetype, self.base_params, self.param_values, source_constraints)
        self.sourceparams = [p for p, _ in self.param_values]
        self.misfits_by_src = self.norms_by_src = None
        self.failings = []
        self.best_source = self.misfits_by_s = self.misfits_by_r = self.variability_by_r = None
        self.bootstrap_sources = self.stats = None

    def _compute_time_scan(self, engine, dt):
        """The grid's misfits from one synthesis per node of the grid WITHOUT its time axis, at the axis's first value, and a
        scan of the axis (Engine.time_scan_for_params); the same arrays in the same order as the plain evaluation fills."""
        axes = [i for i, (p, _) in enumerate(self.param_values) if p == "time"]
        if len(axes) != 1:
            raise ValueError("time_scan: the grid needs exactly one `time` axis")
        ax = axes[0]
        split = split_time_axis(self.param_values[ax][1], engine.dt if dt is None else dt)
        if split is None:
            raise ValueError("time_scan: the time axis is not evenly spaced by a whole number of samples")
        k0, kstep, nk = split
        dims = [len(v) for _, v in self.param_values]
        if int(np.prod(dims)) != len(self.sources):
            raise ValueError("time_scan: source constraints have switched grid nodes off; the scan needs the full grid")
        idx = np.arange(len(self.sources)).reshape(dims)
        first = np.take(idx, 0, axis=ax).ravel()                       # nodes at the axis's first value, grid order
        m, n, _, _, failings = engine.time_scan_for_params(self.sourcetype, self.sources[first], k0, kstep, nk)
        nrec = len(engine.components)
        ncomp = max([len(c) for c in engine.components] + [1])
        mis = np.zeros((len(self.sources), nrec, ncomp))
        nor = np.zeros((len(self.sources), nrec, ncomp))
        where = np.moveaxis(idx, ax, -1).reshape(len(first), nk)        # [node without time][offset] -> grid index
        j = 0
        for ir, comps in enumerate(engine.components):
            if not engine.enabled[ir]:
                continue
            k = len(comps)
            mis[where, ir, :k] = m[:, :, j:j + k]
            nor[where, ir, :k] = n[:, None, j:j + k]
            j += k
        self.syntheses_saved = len(self.sources) - len(first)
        self.misfits_by_src, self.norms_by_src = mis, nor
        self.failings = sorted(int(i) for f in failings for i in where[f])

    def compute_mt_time_scan(self, engine, dt=None, evaluate_fitted=True):
        """A free moment tensor at every node of a grid with a `time` axis, from six syntheses per node of the grid WITHOUT that
        axis (`mtfit.fit_moment_tensors_time_scan`, kiwi_hip_linear_fit_time_scan): the linear fit inside the time scan.  The
        grid has exactly one `time` axis that `split_time_axis` accepts (`dt`: the database's sampling interval, default
        engine.dt), no tensor axes, every node switched on, and its source type is `moment_tensor` or `mt_eikonal`; l2norm.
        Fills, in grid order, `fitted_tensors`, `fit_misfits`, `fit_status`, `fit_pivot_min`, the tensor columns of `sources`,
        `ibest`, `best_source`, `misfits_by_s` and `syntheses_saved` (against six syntheses per node of the full grid).  With
        `evaluate_fitted` the fitted sources are then evaluated like any grid, as `compute(linear_mt=True)` does, so that
        `postprocess` works on them."""
        from . import mtfit
        c0 = mtfit.TENSOR_COLUMN.get(SOURCE_TYPES.get(self.sourcetype, self.sourcetype))
        if c0 is None or any(p in mtfit.COMPONENTS for p in self.sourceparams):
            raise KiwiHipError("linear_mt: the source type must be moment_tensor or mt_eikonal and the grid must not run over tensor components")
        axes = [i for i, (p, _) in enumerate(self.param_values) if p == "time"]
        if len(axes) != 1:
            raise ValueError("time_scan: the grid needs exactly one `time` axis")
        ax = axes[0]
        split = split_time_axis(self.param_values[ax][1], engine.dt if dt is None else dt)
        if split is None:
            raise ValueError("time_scan: the time axis is not evenly spaced by a whole number of samples")
        k0, kstep, nk = split
        dims = [len(v) for _, v in self.param_values]
        if int(np.prod(dims)) != len(self.sources):
            raise ValueError("time_scan: source constraints have switched grid nodes off; the scan needs the full grid")
        self.receiver_mask = np.array(engine.enabled, bool)
        self.nreceivers = len(engine.components)
        self.ncomponents = [len(c) for c in engine.components]
        idx = np.arange(len(self.sources)).reshape(dims)
        first = np.take(idx, 0, axis=ax).ravel()                       # nodes at the axis's first value, grid order
        where = np.moveaxis(idx, ax, -1).reshape(len(first), nk)        # [node without time][offset] -> grid index
        tensors, misfit, status, pivot, _ = mtfit.fit_moment_tensors_time_scan(engine, self.sourcetype, self.sources[first], k0, kstep, nk)
        n = len(self.sources)
        self.fitted_tensors, self.fit_misfits = np.full((n, 6), np.nan), np.full(n, np.nan)
        self.fit_status, self.fit_pivot_min = np.zeros(n, np.int32), np.zeros(n)
        self.fitted_tensors[where], self.fit_misfits[where] = tensors, misfit
        self.fit_status[where], self.fit_pivot_min[where] = status, pivot
        solved = self.fit_status == 0
        self.sources[solved, c0:c0 + 6] = self.fitted_tensors[solved].astype(np.float32)
        self.syntheses_saved = 6 * (n - len(first))
        if evaluate_fitted:
            self.misfits_by_src, self.norms_by_src, self.failings = engine.make_misfits_for_sources(self.sourcetype, self.sources)
            self.ref_misfits_by_src, self.ref_norms_by_src, _ = engine.make_misfits_for_sources(self.sourcetype, self.ref_params[None, :])
        self.misfits_by_s = self.fit_misfits
        self.ibest = int(np.nanargmin(self.fit_misfits)) if np.any(np.isfinite(self.fit_misfits)) else 0
        self.best_source = self.sources[self.ibest]

    def compute_dc_time_scan(self, engine, strikes, dips, rakes, moment=None, outer_norm="l1norm", dt=None, cube=False):
        """The best double couple over strikes x dips x rakes at every node of a grid with a `time` axis, from six syntheses per
        node of the grid WITHOUT that axis (`mtfit.scan_double_couples_time_scan`, kiwi_hip_linear_fit_candidates_time_scan).  The
        grid is as `compute_mt_time_scan` asks: exactly one `time` axis that `split_time_axis` accepts, no tensor axes, every node
        switched on, source type `moment_tensor` or `mt_eikonal`; the engine's method is l2norm, `outer_norm` combines the
        receivers; moment=None finds every mechanism's best moment (outer l2norm only).  Fills, in grid order, `dc_sdr` [n, 3],
        `dc_moments`, `dc_misfits`, `dc_index` (the mechanism's row in the grid of mechanisms, -1: none), `dc_status`, the tensor
        columns of `sources` (the best double couple of the node), `ibest`, `best_source`, `misfits_by_s` and `syntheses_saved`
        (against one synthesis per mechanism and node); cube=True also `dc_cube` [nodes without time, ns, nd, nr] and
        `dc_cube_offset`: every mechanism's smallest misfit over the time axis and where."""
        from . import mtfit
        c0 = mtfit.TENSOR_COLUMN.get(SOURCE_TYPES.get(self.sourcetype, self.sourcetype))
        if c0 is None or any(p in mtfit.COMPONENTS for p in self.sourceparams):
            raise KiwiHipError("linear_mt: the source type must be moment_tensor or mt_eikonal and the grid must not run over tensor components")
        axes = [i for i, (p, _) in enumerate(self.param_values) if p == "time"]
        if len(axes) != 1:
            raise ValueError("time_scan: the grid needs exactly one `time` axis")
        ax = axes[0]
        split = split_time_axis(self.param_values[ax][1], engine.dt if dt is None else dt)
        if split is None:
            raise ValueError("time_scan: the time axis is not evenly spaced by a whole number of samples")
        k0, kstep, nk = split
        dims = [len(v) for _, v in self.param_values]
        if int(np.prod(dims)) != len(self.sources):
            raise ValueError("time_scan: source constraints have switched grid nodes off; the scan needs the full grid")
        idx = np.arange(len(self.sources)).reshape(dims)
        first = np.take(idx, 0, axis=ax).ravel()                       # nodes at the axis's first value, grid order
        where = np.moveaxis(idx, ax, -1).reshape(len(first), nk)        # [node without time][offset] -> grid index
        res = mtfit.scan_double_couples_time_scan(engine, self.sourcetype, self.sources[first], strikes, dips, rakes, k0, kstep, nk,
                                                  moment=moment, outer_norm=outer_norm, cube=cube)
        n = len(self.sources)
        self.dc_sdr, self.dc_moments, self.dc_misfits = np.full((n, 3), np.nan), np.full(n, np.nan), np.full(n, np.nan)
        self.dc_index, self.dc_status = np.full(n, -1, np.int32), np.zeros(n, np.int32)
        self.dc_sdr[where] = np.stack([res["strikes"], res["dips_"], res["rakes_"]], 2)
        self.dc_moments[where], self.dc_misfits[where], self.dc_index[where] = res["moments"], res["misfits"], res["indices"]
        self.dc_status[where] = res["status"][:, None]
        if cube:
            self.dc_cube, self.dc_cube_offset = res["cube"], res["cube_offset"]
        has = self.dc_index >= 0
        tensors, _ = mtfit.double_couple_candidates(strikes, dips, rakes)
        self.sources[has, c0:c0 + 6] = (tensors[self.dc_index[has]] * self.dc_moments[has, None]).astype(np.float32)
        nmech = len(tensors)
        self.syntheses_saved = nmech * n - 6 * len(first)
        self.misfits_by_s = self.dc_misfits
        self.ibest = int(np.nanargmin(self.dc_misfits)) if np.any(np.isfinite(self.dc_misfits)) else 0
        self.best_source = self.sources[self.ibest]
        self.dc_scan = res

    def compute(self, engine, dist=None, device=0, linear_mt=False, outer_norm="l2norm", niter=8, eps=1e-3, time_scan=False,
                dt=None):
        """Trace misfits for every grid node (and the reference source), `engine` = kiwi_amd.Engine set up for
        the inversion.  With a torch.distributed group the grid is sharded over the ranks (kiwi_amd/shard.py).
        linear_mt=True (`moment_tensor`, `mt_eikonal`; l2norm): the grid runs over the OTHER parameters and every node gets
        the moment tensor that fits best (kiwi_amd/mtfit.py, six evaluations per node): `fitted_tensors`, `fit_misfits`,
        `fit_status`, `fit_pivot_min` per node, the tensor columns of `sources` replaced by the fitted tensors, `ibest`,
        `best_source` and `misfits_by_s` from the fit.  The fitted sources are then evaluated like any grid, so that
        `postprocess` (bootstrap over the receivers) works on them unchanged.  outer_norm="l1norm" (or an engine whose misfit
        method is l1norm) fits the tensors robustly, `niter` reweighted solves with the relative bound `eps`
        (`mtfit.fit_moment_tensors`); a node whose reweighting broke down (status 3) keeps the tensor it reached.
        time_scan=True: the grid has a `time` axis evenly spaced by whole samples (`split_time_axis`; `dt`: the database's
        sampling interval, default engine.dt); the grid without that axis is synthesised once at the axis's first value and the
        axis is scanned (Engine.time_scan_for_params).  The same arrays in the same order; `syntheses_saved` counts what was
        not synthesised.  ValueError where the axis does not split, and when combined with linear_mt."""
        if time_scan and linear_mt:
            raise ValueError("time_scan cannot be combined with linear_mt")
        if time_scan and dist is not None:
            raise ValueError("time_scan: a sharded scan is the caller's split of the grid without its time axis")
        self.receiver_mask = np.array(engine.enabled, bool)
        self.nreceivers = len(engine.components)
        self.ncomponents = [len(c) for c in engine.components]
        if linear_mt and len(self.sources):
            from . import mtfit
            if dist is not None:
                raise KiwiHipError("linear_mt: a sharded fit is the caller's split of the grid at node boundaries (INTEGRATION.md)")
            c0 = mtfit.TENSOR_COLUMN.get(SOURCE_TYPES[self.sourcetype])
            if c0 is None or any(p in mtfit.COMPONENTS for p in self.sourceparams):
                raise KiwiHipError("linear_mt: the source type must be moment_tensor or mt_eikonal and the grid must not run over tensor components")
            self.fitted_tensors, self.fit_misfits, self.fit_status, self.fit_pivot_min = mtfit.fit_moment_tensors(
                engine, self.sourcetype, self.sources, outer_norm=outer_norm, niter=niter, eps=eps)
            solved = (self.fit_status == 0) | (self.fit_status == 3)
            self.sources[solved, c0:c0 + 6] = self.fitted_tensors[solved].astype(np.float32)
        if time_scan and len(self.sources):
            self._compute_time_scan(engine, dt)
        elif len(self.sources):
            if dist is not None:
                from .shard import sharded_misfits_for_sources
                self.misfits_by_src, self.norms_by_src, self.failings = sharded_misfits_for_sources(
                    engine, self.sourcetype, self.sources, dist, device)
            else:
                self.misfits_by_src, self.norms_by_src, self.failings = engine.make_misfits_for_sources(self.sourcetype,
                                                                                                      self.sources)
        # sources the engine rejected keep zero misfits AND zero norms: their global misfit comes out as NaN and
        # nanargmin passes over them (gridsearch.py:172-178 drops `failings` the same way)
        self.ref_misfits_by_src, self.ref_norms_by_src, _ = engine.make_misfits_for_sources(self.sourcetype,
                                                                                          self.ref_params[None, :])
        self.best_source = None
        if linear_mt and len(self.sources):
            self.misfits_by_s = self.fit_misfits
            self.ibest = int(np.nanargmin(self.fit_misfits)) if np.any(np.isfinite(self.fit_misfits)) else 0
            self.best_source = self.sources[self.ibest]

    def _best_source(self, **cfg):
        g, g_sr = make_global_misfits(self.misfits_by_src, self.norms_by_src, receiver_mask=self.receiver_mask, **cfg)
        ibest = int(np.nanargmin(g)) if np.any(np.isfinite(g)) else 0
        return ibest, g, g_sr

    def _postprocess_device(self, engine, bootstrap_iterations, rng, outer_norm="l2norm", receiver_weights=None, anarchy=False):
        nrec = self.misfits_by_src.shape[1]
        counts = bootstrap_draw_weights(nrec, bootstrap_iterations, rng, self.receiver_mask, receiver_weights)
        draws = np.concatenate([np.ones((1, nrec)), counts], 0)
        _, best, g = engine.outer_misfits(self.misfits_by_src, self.norms_by_src, outer_norm, receiver_weights, anarchy, draws,
                                          which_draw=0, ncomponents=self.ncomponents)
        _, g_sr = make_global_misfits(self.misfits_by_src, self.norms_by_src, outer_norm=outer_norm,
                                      receiver_weights=receiver_weights, receiver_mask=self.receiver_mask, anarchy=anarchy)
        ibest = int(best[0])
        self.ibest, self.best_source, self.misfits_by_s = ibest, self.sources[ibest], g
        self.misfits_by_r, self.variability_by_r = g_sr[ibest], np.std(g_sr, 0)
        self.bootstrap_sources = [self.sources[int(i)] for i in best[1:]]

    def postprocess(self, bootstrap_iterations=1000, rng=None, engine=None, **outer_misfit_config):
        """Global misfits, best source, bootstrap distribution of the best source (gridsearch.py:199-289).
        With `engine` (a kiwi_amd.Engine) the best source and the bootstrap sources come from ONE device call
        (Engine.outer_misfits: draw 0 = every receiver once, draws 1..B = the resampling counts, drawn from `rng` exactly
        as the host path draws them) and `misfits_by_s` from that call's draw 0; `misfits_by_r` and `variability_by_r` stay
        on the host (one pass).  The device's global misfits differ from the host's by a few ulp; without
        `engine` nothing changes."""
        g, g_sr = make_global_misfits(self.ref_misfits_by_src, self.ref_norms_by_src, receiver_mask=self.receiver_mask,
                                      **outer_misfit_config)
        self.ref_misfit, self.ref_misfits_by_r = g[0], g_sr[0]
        if len(self.sources) == 0:
            self.best_source, self.misfits_by_s, self.misfits_by_r, self.variability_by_r = self.base_params, [], [], []
            self.bootstrap_sources, self.stats = [], {}
            return
        rng = np.random.default_rng() if rng is None else rng
        if engine is not None:
            self._postprocess_device(engine, bootstrap_iterations, rng, **outer_misfit_config)
        else:
            ibest, g, g_sr = self._best_source(**outer_misfit_config)
            self.ibest, self.best_source, self.misfits_by_s = ibest, self.sources[ibest], g
            self.misfits_by_r, self.variability_by_r = g_sr[ibest], np.std(g_sr, 0)
            self.bootstrap_sources = [self.sources[self._best_source(bootstrap=True, rng=rng, **outer_misfit_config)[0]]
                                      for _ in range(bootstrap_iterations)]
        names = SOURCE_PARAMS[self.sourcetype]
        self.stats = {}
        for param, gvalues in self.param_values:
            k = names.index(param)
            self.stats[param] = MisfitGridStats(param, float(self.best_source[k]),
                                                [s[k] for s in self.bootstrap_sources], tested_values=gvalues)

    def get_best_misfit(self):
        return self.ref_misfit if len(self.misfits_by_s) == 0 else float(np.nanmin(self.misfits_by_s))


def band_slots_to_receivers(misfit, norm, components, enabled=None):
    """[N_s, N_b, nmis] arrays of Engine.band_misfits -> [N_s, N_b, N_r, N_k] float64 in the layout of
    Engine.make_misfits_for_sources: receivers in file order, components in string order, disabled receivers as zeros."""
    m = np.asarray(misfit, np.float64)
    n = np.asarray(norm, np.float64)
    nrec = len(components)
    enabled = [True] * nrec if enabled is None else list(enabled)
    nk = max([len(c) for c in components] + [1])
    mis = np.zeros(m.shape[:2] + (nrec, nk))
    nor = np.zeros(m.shape[:2] + (nrec, nk))
    j = 0
    for ir, comps in enumerate(components):
        if not enabled[ir]:
            continue
        k = len(comps)
        mis[:, :, ir, :k] = m[:, :, j:j + k]
        nor[:, :, ir, :k] = n[:, :, j:j + k]
        j += k
    return mis, nor


def make_band_global_misfits(misfits_by_src, norms_by_src, band_weights=None, outer_norm="l2norm", receiver_weights=None,
                             anarchy=False):
    """One outer misfit per source from the misfits of several bands (Engine.band_misfits through band_slots_to_receivers):
    [N_s, N_b, N_r, N_k] arrays.  Every (band, component) pair counts as a component of its receiver, its misfit and norm
    factor multiplied by the band's weight (ones by default); the rest is make_global_misfits.  With one band of weight one
    this IS make_global_misfits.  Returns (global[N_s], misfits per source and receiver [N_s, N_r]).  Host numpy."""
    m = np.asarray(misfits_by_src, np.float64)
    n = np.asarray(norms_by_src, np.float64)
    if m.ndim != 4 or m.shape != n.shape:
        raise KiwiHipError("make_band_global_misfits: misfits and norms must be [N_s, N_b, N_r, N_k] arrays of one shape")
    ns, nb, nr, nk = m.shape
    w = np.ones(nb) if band_weights is None else np.asarray(band_weights, np.float64)
    if w.shape != (nb,):
        raise KiwiHipError("make_band_global_misfits: one weight per band")
    fold = lambda a: np.transpose(a * w[None, :, None, None], (0, 2, 1, 3)).reshape(ns, nr, nb * nk)  # noqa: E731
    return make_global_misfits(fold(m), fold(n), outer_norm, receiver_weights, anarchy=anarchy)
