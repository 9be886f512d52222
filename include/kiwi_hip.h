/*
 * kiwi_hip.h -- C-ABI of the MI355X forward-modelling + misfit engine for Kiwi's inner
 * inversion loop (trial source -> synthetic seismograms -> misfits).
 *
 * This is the drop-in boundary: plain C types only, callable from Fortran through
 * iso_c_binding (kiwi_amd/fortran/kiwi_hip_binding.f90), from Python through ctypes
 * (kiwi_amd/engine.py) or from C/C++.  Every function returns 0 on success and a
 * non-zero code on failure; the message is retrieved with kiwi_hip_last_error() and maps
 * onto the reference's recoverable-error convention ("<cmd>: nok >" + message,
 * minimizer.f90:1689-1696).  No function aborts the process.  All arrays are caller-owned,
 * contiguous, and copied before the call returns.  Indices irec/icomp are 1-based like
 * the reference's wire protocol (switch_receiver, minimizer.f90:273-312).
 *
 * The three private engine steps this library replaces are
 *     calculate_seismograms()  minimizer_engine.f90:885-907   (-> make_seismogram, seismogram.f90:36)
 *     scale_seismograms()      minimizer_engine.f90:909-921   (-> receiver.f90:853)
 *     calculate_misfits()      minimizer_engine.f90:924-945   (-> receiver.f90:407, comparator.f90:911,954)
 * batched over many trial sources per call (kiwi_hip_eval); the setters mirror the
 * engine's public state setters, cited one by one below.
 *
 * Sample index convention: all 'first' arguments are indices in the reference's strip
 * index space (t_strip lower bounds, sparse_trace.f90:29-33): a Green's function trace
 * sample j added with shift s lands on seismogram sample j+s (sparse_trace.f90:605), and a
 * reference seismogram read from a file starting at time t0 has first = nint((t0 -
 * reftime)/dt) + 1 (receiver.f90:834-851).
 */
#ifndef KIWI_HIP_H
#define KIWI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kiwi_hip_ctx kiwi_hip_ctx;

/* misfit method ids = comparator.f90:35-42 */
#define KIWI_L2NORM 1
#define KIWI_L1NORM 2
#define KIWI_AMPSPEC_L2NORM 3
#define KIWI_AMPSPEC_L1NORM 4
#define KIWI_SCALAR_PRODUCT 5
#define KIWI_PEAK 6
#define KIWI_FLOATING_L2NORM 7
#define KIWI_FLOATING_L1NORM 8

/* source type ids = parameterized_source.f90:45-50 */
#define KIWI_SRC_BILAT 1
#define KIWI_SRC_CIRCULAR 2
#define KIWI_SRC_POINT_LP 3
#define KIWI_SRC_EIKONAL 4
#define KIWI_SRC_MT_EIKONAL 5
#define KIWI_SRC_MOMENT_TENSOR 6

/* arithmetic contract of the accumulate kernels (kiwi_hip_set_arithmetic).
 * EXACT (default): every fp32 multiply and add of the superposition is rounded on its own, in the reference's order
 *   (gfdb.f90:944-949, sparse_trace.f90:684-703, seismogram.f90:171-250 on an x86-64 host without fused operations):
 *   synthetics and misfits are bit-identical to the CPU restatement of the reference given equal geometry records.
 * FUSED: the same operations in the same order, each multiply contracted with the add that consumes it into one fused
 *   multiply-add (one rounding instead of two; half the vector instructions): tolerance class -- misfits within 1e-6 of the
 *   slot's norm factor, synthetics within 2e-6 of the trace maximum (BASELINE.json north_star: "misfits within 1e-6 relative").
 * Geometry (rows, sample shifts, weights), the comparator's fp64 sums and the host discretisers are the same in both. */
#define KIWI_ARITH_EXACT 0
#define KIWI_ARITH_FUSED 1

/* ---- lifetime: program start / cleanup_minimizer (minimizer_engine.f90:1057-1067) ---- */
int kiwi_hip_init(int device, kiwi_hip_ctx **ctx);
/* SURVEY 8b's `kiwi_hip_init(int ndev_wanted, void** ctx)`: ONE context over ndev_wanted devices of this process
 * (<= 0: every visible device; more than are visible is an error unless KIWI_HIP_MULTI_OVERSUBSCRIBE=1 stacks the contexts
 * on the devices there are -- for tests on a one-GPU box).  The returned context is the first device's and owns the others:
 * every setter called on it is repeated on them (Green's function tensor, receivers, references replicated: SURVEY 8e), and
 * kiwi_hip_misfits_for_params cuts its trial list into contiguous shards in list order (the order of Source.grid,
 * python/tunguska/source.py:119-164), one per device, each evaluated on its device by a thread of its own straight into its slice
 * of the caller's arrays -- no collective.  Everything else (kiwi_hip_eval, getters, kiwi_hip_minimize_lm) works on the first
 * device as with kiwi_hip_init.  Counterpart for the Fortran host of the process pool of python/tunguska/seismosizer.py:785-827;
 * results do not depend on the number of devices (a source's evaluation does not depend on its batch). */
int kiwi_hip_init_multi(int ndev_wanted, kiwi_hip_ctx **ctx);
int kiwi_hip_ndevices(kiwi_hip_ctx *ctx, int *n);
/* KIWI_ARITH_EXACT / KIWI_ARITH_FUSED (above); takes effect at the next kiwi_hip_eval.  The environment variable
 * KIWI_HIP_ARITH=exact|fused sets the initial value of every context (for the unmodified Fortran protocol host). */
int kiwi_hip_set_arithmetic(kiwi_hip_ctx *ctx, int mode);
int kiwi_hip_get_arithmetic(kiwi_hip_ctx *ctx, int *mode);
int kiwi_hip_destroy(kiwi_hip_ctx *ctx);
/* copies the last error message (NUL terminated, truncated to buflen); ctx may be NULL for init errors */
int kiwi_hip_last_error(kiwi_hip_ctx *ctx, char *buf, int buflen);

/* ---- set_database (minimizer_engine.f90:114-139; gfdb.f90:163-264) ----
 * One-time dense upload replacing the lazy chunk cache (gfdb.f90:952-1031).
 * G[((ix*nz+iz)*ng+ig)*L + l], l < nsamp[...] : samples of trace (ix,iz,ig) starting at
 * strip index first[...] (== trace%span(1), sparse_trace.f90:46); interior gaps are zeros;
 * samples at l >= nsamp are ignored (the last valid sample is the repeated end value,
 * sparse_trace.f90:696-703).  nsamp == 0 marks a trace that is not stored (gfdb.f90:1003). */
int kiwi_hip_set_gfdb(kiwi_hip_ctx *ctx, int nx, int nz, int ng, int L,
                      float dt, float dx, float dz, float firstx, float firstz,
                      const float *G, const int *first, const int *nsamp);

/* set_database dbpath nipx nipz (minimizer.f90:91-150 -> gfdb.f90:163-264,1109-1310): the stored database of
 * kiwi_hip_set_gfdb (same arguments), made nipx times denser in distance and nipz times denser in depth by Gulunay's
 * f-k interpolation on the device (nx' = nx*nipx, dx' = dx/nipx, likewise in depth; firstx, firstz unchanged; stored
 * traces stay bit-identical at ix' = ix*nipx, iz' = iz*nipz).  nipx must be a power of two up to 128 and nipz one up
 * to 32 (other values are refused: the reference dies at their first use).  (1,1) is kiwi_hip_set_gfdb. */
int kiwi_hip_set_gfdb_interpolated(kiwi_hip_ctx *ctx, int nipx, int nipz, int nx, int nz, int ng, int L,
                                   float dt, float dx, float dz, float firstx, float firstz,
                                   const float *G, const int *first, const int *nsamp);
/* shape of the installed database: maxlen = longest trace */
int kiwi_hip_get_gfdb_shape(kiwi_hip_ctx *ctx, int *nx, int *nz, int *ng, int *maxlen, float *dx, float *dz);
/* one installed trace, 0-based indices like G's: first sample index, count (0: not stored) and, when out is not NULL,
 * its samples (maxn >= n) */
int kiwi_hip_get_gfdb_trace(kiwi_hip_ctx *ctx, int ix, int iz, int ig, int *first, int *n, float *out, int maxn);

/* set_local_interpolation + set_spacial_undersampling (minimizer_engine.f90:141-163; minimizer.f90:155-207) */
int kiwi_hip_set_interp(kiwi_hip_ctx *ctx, int bilinear, int xundersample, int zundersample);

/* set_effective_dt (minimizer_engine.f90:612-620): shortest duration of interest for the discretisers */
int kiwi_hip_set_effective_dt(kiwi_hip_ctx *ctx, float effective_dt);

/* set_source_location lat lon reftime (minimizer.f90:485-517; degrees, parsed as default real) */
int kiwi_hip_set_source_location(kiwi_hip_ctx *ctx, float lat_deg, float lon_deg, double ref_time);

/* set_receivers (minimizer_engine.f90:165-286): per receiver lat lon [depth] components;
 * components is a string over "acrlduesnw" (receiver.f90:35-56), at most 5, no axis twice */
int kiwi_hip_set_receivers(kiwi_hip_ctx *ctx, int nrec, const double *lat_deg, const double *lon_deg,
                           const float *depth, const char *const *components);
/* switch_receiver (minimizer_engine.f90:288-309) */
int kiwi_hip_switch_receiver(kiwi_hip_ctx *ctx, int irec, int enabled);

/* set_ref_seismograms (minimizer_engine.f90:313-352; receiver.f90:746-851): one trace per receiver component */
int kiwi_hip_set_reference(kiwi_hip_ctx *ctx, int irec, int icomp, int first, int n, const float *data);
/* set_misfit_taper / set_misfit_filter (minimizer_engine.f90:632-698; minimizer.f90:875-1016; receiver.f90:355-389):
 * piecewise linear function control points; npts == 0 removes it; for the filter irec == 0 means every receiver (:646-661) */
int kiwi_hip_set_taper(kiwi_hip_ctx *ctx, int irec, int npts, const float *x, const float *y);
int kiwi_hip_set_filter(kiwi_hip_ctx *ctx, int irec, int npts, const float *x, const float *y);
/* set_misfit_method (minimizer_engine.f90:622-630) */
int kiwi_hip_set_misfit_method(kiwi_hip_ctx *ctx, int method);
/* set_floating_shiftrange ireceiver min-shift max-shift (minimizer_engine.f90:421-451; minimizer.f90:388-419): range in
 * seconds for floating_l1norm / floating_l2norm (receiver.f90:439-510), ireceiver 0 = all; and get_floating_shifts
 * (minimizer_engine.f90:1095-1128): the winning shift in seconds per source and ENABLED receiver, shifts[nsrc][n_enabled] */
int kiwi_hip_set_floating_shiftrange(kiwi_hip_ctx *ctx, int irec, float min_shift, float max_shift);
int kiwi_hip_get_floating_shifts(kiwi_hip_ctx *ctx, int isrc0, int nsrc, float *shifts);
/* shift_ref_seismogram ireceiver shift (minimizer_engine.f90:354-378): move a receiver's reference traces by nint(shift/dt)
 * samples.  autoshift_ref_seismogram ireceiver min-shift max-shift (:380-419; receiver.f90:816-832;
 * comparator.f90:1061-1090): cross-correlate the tapered synthetics of uploaded source `isrc` with the references over
 * the integer shifts of the range, move the references of receiver `irec` (0 = all) to the best shift and return the
 * shifts applied in seconds (shifts[nrec] for irec == 0, else shifts[1]).  Setup-time operations, computed on the host. */
int kiwi_hip_shift_ref_seismogram(kiwi_hip_ctx *ctx, int irec, float shift);
int kiwi_hip_autoshift_ref_seismogram(kiwi_hip_ctx *ctx, int irec, float min_shift, float max_shift, int isrc, float *shifts);
/* set_synthetics_factor (minimizer_engine.f90:700-727; receiver.f90:391-405) */
int kiwi_hip_set_synthetics_factor(kiwi_hip_ctx *ctx, float factor);

/* ---- trial sources ----
 * psm_set + psm_to_tdsm on the host (source_all.f90:216-261,431-465): number of parameters
 * of a source type (<0: unsupported), and one discretisation into a centroid table
 * cent[ncent][10] = north east depth time mxx myy mzz mxy mxz myz (discrete_source.f90:27-30). */
int kiwi_hip_source_nparams(int sourcetype);
int kiwi_hip_discretize(int sourcetype, const float *params, int nparams, float effective_dt,
                        float *cent, int maxcent, int *ncent, float *moment, float *risetime);

/* ---- variable-rupture-speed sources `eikonal` (type 4, 15 params) and `mt_eikonal` (type 5, 20 params)
 * (source_eikonal.f90, source_mt_eikonal.f90).  A crust profile is 31 floats: vp[8] vs[8] rho[8] thickness[7]
 * (t_crust2x2_1d_profile, crust2x2.f90:45-50; layer 8 = below the crust).  The CRUST2.0 tables stay with the
 * caller, which does the two look-ups set_source_location triggers in the reference:
 *   rupture_profile = crust2x2_get_profile(psm%origin)       -- rupture speeds, source_eikonal.f90:472
 *                     (the reference passes the origin in RADIANS there; a drop-in caller does the same)
 *   origin_profile  = crust2x2_get_profile(r2d(psm%origin))  -- crustal thickness, parameterized_source.f90:215
 * set_source_crust and set_source_crustal_thickness_limit (minimizer_engine.f90:479-486) both re-install the
 * default constraints (surface at 1500 m, bottom of the crust; parameterized_source.f90:127-145);
 * set_source_constraints (minimizer_engine.f90:469-477) replaces them: points[n][3], normals[n][3] (ned). */
int kiwi_hip_set_source_crust(kiwi_hip_ctx *ctx, const float *rupture_profile, const float *origin_profile);
int kiwi_hip_set_source_crustal_thickness_limit(kiwi_hip_ctx *ctx, float limit);
int kiwi_hip_get_source_crustal_thickness(kiwi_hip_ctx *ctx, float *thickness);   /* minimizer_engine.f90:488-498 */
int kiwi_hip_set_source_constraints(kiwi_hip_ctx *ctx, int n, const float *points, const float *normals);
/* stateless psm_set + psm_to_tdsm of the two types (needs no GPU); returns 5 for "Empty rupture area"
 * (source_eikonal.f90:284), 6 for a nucleation point outside of the rupture region (:427) */
int kiwi_hip_discretize_eikonal(int sourcetype, const float *params, int nparams, float effective_dt,
                                const float *rupture_profile, int ncon, const float *points, const float *normals,
                                float *cent, int maxcent, int *ncent, float *moment, float *risetime);

/* upload a batch of discretised trial sources: cent_ofs[nsrc+1] row offsets into cent[][10];
 * moment / risetime = psm%moment / psm%risetime per source (parameterized_source.f90:70-71) */
int kiwi_hip_set_sources(kiwi_hip_ctx *ctx, int nsrc, const int *cent_ofs, const float *cent,
                         const float *moment, const float *risetime);
/* the centroid table of uploaded source isrc as the engine holds it (output_source_model writes it to
 * <base>-dsm.table, minimizer_engine.f90:947-977); cent == NULL or maxcent <= 0 only returns the count */
int kiwi_hip_get_source_centroids(kiwi_hip_ctx *ctx, int isrc, int maxcent, int *ncent, float *cent);
/* set_source_params for a whole batch (minimizer_engine.f90:500-523): params[nsrc][nparams] in
 * wire order; discretised on the host with the current effective dt, then uploaded.
 * A trial source the discretiser rejects ("Empty rupture area", source_eikonal.f90:286; nucleation point outside of the
 * rupture region, :428) does not fail the batch: it is recorded (kiwi_hip_get_source_status) and skipped, its misfits,
 * norm factors and global misfit read as zeros -- python/tunguska/seismosizer.py:703-720 (`failings`).  The call
 * returns non-zero only when NO source of the batch could be discretised (a batch of one: the reference's
 * `set_source_params: nok > Empty rupture area`); the statuses stay readable then too. */
int kiwi_hip_set_sources_params(kiwi_hip_ctx *ctx, int sourcetype, int nsrc, const float *params);
/* status[nsrc] of uploaded sources isrc0 ..: 0 discretised, 5 "Empty rupture area", 6 "position of nucleation point is
 * outside of rupture region" (the codes kiwi_hip_discretize_eikonal returns); message text of a code */
int kiwi_hip_get_source_status(kiwi_hip_ctx *ctx, int isrc0, int nsrc, int *status);
int kiwi_hip_source_status_message(int code, char *buf, int buflen);

/* make_misfits_for_sources for a whole trial list in ONE call (python/tunguska/seismosizer.py:682-722), host and device
 * overlapped: the list is cut into pieces of `piece` sources (<= 0: 128 for the eikonal types, 2048 otherwise); while the
 * device evaluates one piece a second host thread discretises the next.  Per piece this IS kiwi_hip_set_sources_params +
 * kiwi_hip_eval + kiwi_hip_get_misfits + kiwi_hip_get_source_status, so misfit[nsrc][nmis], norm[nsrc][nmis], global[nsrc]
 * and status[nsrc] (any may be NULL) are bit for bit what those calls return for any piece size; a piece none of whose
 * sources could be discretised is all failings (zeros), not an error.  Pieces are taken from the end of the list, so the
 * context is left with its HEAD (sources 0 .. piece - 1, evaluated), as after kiwi_hip_set_sources_params + kiwi_hip_eval
 * of those.  (Eikonal types, lists of two pieces or more: the last piece of the list -- the first worked on, whose
 * discretisation nothing hides -- is taken as an eighth, an eighth, a quarter and half of it, and the discretiser runs up to
 * three pieces ahead of the device.)  For the eikonal source types the host discretiser (a fast-marching solve per trial source, eikonal.f90:29-199)
 * costs as much as the device evaluation; overlapped, a sweep runs at the slower of the two instead of their sum. */
int kiwi_hip_misfits_for_params(kiwi_hip_ctx *ctx, int sourcetype, int nsrc, const float *params, int piece,
                                float *misfit, float *norm, float *global, int *status);
/* CPUs the host side may keep busy: allowed hardware threads cut to the cgroup CPU quota (the discretiser's thread count) */
int kiwi_hip_effective_cpus(void);
/* The eikonal discretiser keeps its fast-marching solves (eikonal.f90:29-199) by their complete inputs -- speed grid, grid
 * spacing, start cell (source_mt_eikonal.f90:467-519 builds them in rupture coordinates) -- and returns the stored arrival
 * times when ALL of them recur (hash, then comparison in full: bit-identical centroid tables).  North / east / time shifts
 * and moment-tensor changes of a rupture leave the inputs alone: a location grid at fixed depth costs one solve.  Counters
 * since the library was loaded (either pointer may be NULL); reset != 0 clears them, reset & 2 also drops the stored solves.
 * Process-wide, shared by all contexts.
 * KIWI_HIP_EIK_CACHE=0 in the environment switches the cache off. */
int kiwi_hip_eikonal_cache_stats(long long *hits, long long *misses, int reset);
/* The fast-marching solve on its own (eikonal_solver_fmm, eikonal.f90:29-199; needs no GPU): speed[ny][nx] and times[ny][nx]
 * with x fastest, origin / delta / start as there.  `discard`: nodes of exactly this speed may be left undone once every other
 * node is accepted (what the discretiser passes for the points outside of the rupture; NaN = solve all).  plain != 0 runs the
 * reference's statements one by one, 0 the layout-optimised march the discretiser uses (kiwi_host_fmm.hpp) -- same bits;
 * *fallbacks (may be NULL) = how often, since the library was loaded, the optimised march handed a solve to the plain one. */
int kiwi_hip_fast_marching(const float *speed, int nx, int ny, const float *origin, const float *delta, const float *start,
                           float discard, int plain, float *times, long long *fallbacks);
/* nsolve independent solves in one call; solve k has an nx[k] x ny[k] grid, x fastest, its speeds at speed + ofs[k], its times
 * written to times + ofs[k]; origin, delta, start are [nsolve][2]; discard is [nsolve] (NaN: none).
 * where: 0 = the host's routine (the march of kiwi_hip_fast_marching(plain = 0)) on the discretiser's thread team; needs no GPU
 *            and accepts ctx == NULL;
 *        1 = the device of ctx: one solve per wavefront, each the reference's sequential march (same bits on every node),
 *            on a stream and buffers of the solver's own, cut into several launches where the workspace (16 bytes per node)
 *            would exceed KIWI_HIP_CHUNK_MB.  A solve whose front outgrows the device heap (4096 entries) is solved again by
 *            the host's routine.  Grids with (nx + 2) * (ny + 2) > INT_MAX are refused.
 * *fallbacks (may be NULL): solves of this call handed on -- by the device to the host (where = 1), by the host's optimised
 * march to the plain one (where = 0). */
int kiwi_hip_fast_marching_batch(kiwi_hip_ctx *ctx, int where, int nsolve, const int *nx, const int *ny, const long long *ofs,
                                 const float *speed, const float *origin, const float *delta, const float *start,
                                 const float *discard, float *times, long long *fallbacks);
/* Where the eikonal discretisers (kiwi_hip_set_sources_params, kiwi_hip_misfits_for_params, kiwi_hip_minimize_lm) run the
 * fast-marching solves of a batch: 0 host (default), 1 device -- the solves the cache does not answer go out as one
 * kiwi_hip_fast_marching_batch(where = 1).  Results do not depend on it.  Forwarded to every device of a multi-device context.
 * Initial value: KIWI_HIP_EIK_DEVICE=0|1 in the environment, read at kiwi_hip_init. */
int kiwi_hip_set_eikonal_solver(kiwi_hip_ctx *ctx, int where);
int kiwi_hip_get_eikonal_solver(kiwi_hip_ctx *ctx, int *where);
/* upload, kernel and download milliseconds (HIP events, summed over its launches) of the context's last device batch;
 * any pointer may be NULL; zeros before the first one */
int kiwi_hip_get_eikonal_solver_ms(kiwi_hip_ctx *ctx, double *upload, double *kernel, double *download);
/* of the same batch: kernel launches it took (KIWI_HIP_CHUNK_MB) and the largest heap any of its solves reached (entries; the
 * device heap holds 4096); either pointer may be NULL */
int kiwi_hip_get_eikonal_solver_stats(kiwi_hip_ctx *ctx, int *launches, int *heap_high_water);
/* 1 when the host's optimised march and the device march take an nx x ny grid (its padded size fits an int), else 0 */
int kiwi_hip_fast_marching_grid_ok(long long nx, long long ny);

/* minimize_lm (minimizer_engine.f90:728-874; sminpack/lmdif.f in fp32 with the reference's settings: ftol = xtol =
 * sqrt(spmpar(1)), gtol = 0, maxfev = 500 (n + 1), mode 2 with diag = 1, factor 0.01) over the parameters with
 * mask[i] != 0 (set_source_params_mask), starting at params[nparams].  mins / maxs: limits of the FREE parameters in
 * physical units or both NULL (set_source_subparams_limits, :580-611; :820-842).  Each forward-difference Jacobian is
 * ONE batched evaluation of n sources.  On return params = the source of the LAST forward step -- what the reference
 * leaves in psm and reports through get_source_subparams --, misfit = its global misfit, iterations = forward steps,
 * info as lmdif (8 reported as 4, :796); best (may be NULL) = lmdif's accepted iterate in physical units. */
int kiwi_hip_minimize_lm(kiwi_hip_ctx *ctx, int sourcetype, float *params, const int *mask, const float *mins,
                         const float *maxs, int *info, int *iterations, float *misfit, float *best);

/* The optimiser underneath, usable with any residual function: sminpack/lmdif.f in fp32, the n forward differences of
 * a Jacobian requested as ONE call.  fcn gets k points xs[k][n] (it may modify them in place, as lm_forward_step clamps
 * its argument) and fills fv[k][m]; a negative return aborts and becomes *info.  No device involved. */
typedef int (*kiwi_hip_residual_fn)(void *user, int k, int m, int n, float *xs, float *fv);
int kiwi_hip_lmdif(kiwi_hip_residual_fn fcn, void *user, int m, int n, float *x, float *fvec, float ftol, float xtol,
                   float gtol, int maxfev, float epsfcn, float *diag, int mode, float factor, int *info, int *nfev);

/* ---- the hot path: calculate_seismograms + scale_seismograms + calculate_misfits for
 * sources [isrc0, isrc0+nsrc) of the uploaded batch.  Asynchronous on the context's HIP
 * stream; results stay on the device until fetched. */
int kiwi_hip_eval(kiwi_hip_ctx *ctx, int isrc0, int nsrc);
int kiwi_hip_sync(kiwi_hip_ctx *ctx);

/* get_misfits (minimizer_engine.f90:1130-1172): nmis = sum of components over ENABLED receivers,
 * receiver-major, component-minor */
int kiwi_hip_nmisfits(kiwi_hip_ctx *ctx, int *nmis);
/* misfit[nsrc][nmis], norm[nsrc][nmis] (misfits_norm_factors), global[nsrc] =
 * sqrt(sum m^2)/sqrt(sum n^2) (minimizer_engine.f90:939-942); any pointer may be NULL.  Synchronises. */
int kiwi_hip_get_misfits(kiwi_hip_ctx *ctx, int isrc0, int nsrc, float *misfit, float *norm, float *global);
/* The global misfits of evaluated sources isrc0 .. isrc0 + nsrc - 1 WHERE THEY LIE: a device pointer (fp32, contiguous) on the
 * context's device, valid until the next kiwi_hip_eval / kiwi_hip_set_sources* on the context.  For the multi-GPU exchange
 * (one all-gather of per-source misfit scalars): a collective library takes the shard straight from device memory,
 * no staging through the host.  Synchronises the context's stream (the values are final when the call returns). */
int kiwi_hip_get_global_misfits_device(kiwi_hip_ctx *ctx, int isrc0, int nsrc, const float **device_ptr);

/* output_seismograms (minimizer_engine.f90:980-1010): synthetic of one source of the LAST
 * kiwi_hip_eval range, over the receiver's misfit window.  which: 1 plain (scaled by moment,
 * rise-time folded), 2 tapered.  Returns first sample index and count. */
/* keep the processed synthetics of every evaluated chunk on the device (0 off, 1 plain, 2 tapered) so
 * that kiwi_hip_get_synthetics copies them instead of re-evaluating the source */
int kiwi_hip_set_keep_synthetics(kiwi_hip_ctx *ctx, int which);
int kiwi_hip_get_synthetics(kiwi_hip_ctx *ctx, int isrc, int irec, int icomp, int which,
                            int *first, int *n, float *out, int maxn);
/* the reference probe the same way (output_seismograms ... references plain|tapered|filtered, receiver.f90:618-680):
 * plain = the data as set, tapered / filtered = over the comparator window */
int kiwi_hip_get_reference(kiwi_hip_ctx *ctx, int irec, int icomp, int which, int *first, int *n, float *out, int maxn);

/* ---- measurement / inspection ---- */
/* output_seismogram_spectra (minimizer_engine.f90:1012-1039; probe_get_amp_spectrum, comparator.f90:333-354): amplitude
 * spectrum of the reference (which_probe 0) or of the synthetic of source isrc (1) of one receiver component:
 * |r2c| of the tapered window, n = ntrans / 2 + 1 bins at spacing df, transform length as the spectral comparator sizes
 * the reference / synthetic pair (in the reference it follows the probes' span history); filtered != 0: times the
 * frequency filter where the receiver has one.  Needs references and tapers. */
int kiwi_hip_get_amp_spectrum(kiwi_hip_ctx *ctx, int isrc, int irec, int icomp, int which_probe, int filtered,
                              float *df, int *n, float *out, int maxn);
/* get_principal_axes (minimizer_engine.f90:1248-1258): P and T axis (azimuth, polar angle in degrees, lower hemisphere)
 * of a bilateral source as psm_update_dep_params_bilat derives them (source_bilat.f90:216-239); the reference sets them
 * for no other source type: returns -1 for those.  Host only. */
int kiwi_hip_principal_axes(int sourcetype, const float *params, float *pax, float *tax);
/* output_cross_correlations (minimizer_engine.f90:1283-1306; receiver.f90:597-616; comparator.f90:1061-1090): for one
 * receiver cc[component][shift] = scalar product of the tapered synthetic of source isrc with the reference pulled
 * through its fixed taper, for the integer shifts nint(min/dt) .. nint(max/dt) (first_shift, nshift; nshift = 0 for a
 * disabled receiver).  Set-up-time helper like autoshift: evaluated on the host from one device evaluation. */
int kiwi_hip_get_cross_correlations(kiwi_hip_ctx *ctx, int isrc, int irec, float min_shift, float max_shift,
                                    int *first_shift, int *nshift, float *cc, int maxn);
/* get_peak_amplitudes (minimizer_engine.f90:1174-1212; receiver.f90:544-574; comparator.f90:519-589): per ENABLED
 * receiver the maximum over the misfit window (taper span; without taper the union of the synthetic strips' data spans)
 * of the vector norm of the once (differentiate = 1, velocity) or twice (2, acceleration) differenced synthetics of
 * uploaded source isrc -- vertical + the horizontal pair a/c + r/l or else n/s + e/w, whatever of them the receiver has.
 * get_arias_intensities (:1214-1246; receiver.f90:576-594; comparator.f90:591-625) likewise.  Tapered synthetics where
 * the receiver has a taper; not available while a misfit filter is set.  Without a taper the span is that of THIS
 * source's strips (the reference's strips remember earlier sources).  out[number of enabled receivers]. */
int kiwi_hip_get_peak_amplitudes(kiwi_hip_ctx *ctx, int isrc, int differentiate, float *out);
int kiwi_hip_get_arias_intensities(kiwi_hip_ctx *ctx, int isrc, float *out);

/* HIP-event durations [ms] of the last kiwi_hip_eval on the context stream:
 * ms[0] geometry kernel, ms[1] accumulate kernel(s), ms[2] misfit kernels, ms[3] whole eval;
 * launches[0..2] = number of launches of each in that eval.  Synchronises. */
int kiwi_hip_get_kernel_ms(kiwi_hip_ctx *ctx, float ms[4], int launches[3]);
/* Outer misfit of every trial source under ndraw receiver weightings, and the best source of each (make_global_misfits,
 * seismosizer.py:843-922; the bootstrap over the receivers, gridsearch.py:199-289), on HOST arrays: misfit and norm are the
 * per-slot results [nsrc][nmis] of kiwi_hip_get_misfits / kiwi_hip_misfits_for_params -- of this context, of a gathered
 * sharded run, or anything laid out like them; the context supplies device, stream and chunk bound, nothing of its setup.
 *   slot_receiver[nmis]   receiver (0-based, < nrec) of every slot, ascending: the slots of a receiver are consecutive
 *   outer_norm            1 l1norm, 2 l2norm
 *   receiver_weights      [nrec] or NULL = ones; anarchy != 0 divides each by the receiver's norm (clipped at zero)
 *   draw_weights          [ndraw][nrec]: the weight of receiver r in draw d -- a resampling count under bootstrap, all
 *                         ones for the plain outer misfit
 *   best_value, best_index  [ndraw]: the lowest global misfit of each draw and its source (0-based; among equal values
 *                         the LOWEST index).  A source is excluded from a draw when its weighted norm sum is not
 *                         positive or its misfit is negative or NaN; a draw with every source excluded answers NaN, 0
 *   global_of_draw        [nsrc] or NULL: the global misfit of every source under draw `which_draw`; excluded sources
 *                         read NaN
 * fp64 throughout, every operation rounded on its own in a fixed order (tests/outer_restatement.py restates it): the
 * answer does not depend on chunking (KIWI_HIP_CHUNK_MB) or on how a list is cut into shards.  Under l2norm the squared
 * term is multiplied by the draw weight where the host path multiplies by its root before squaring: a few ulp
 * (INTEGRATION.md).  nrec is bounded by kiwi_hip_outer_max_receivers(); nsrc by INT_MAX. */
int kiwi_hip_outer_misfits(kiwi_hip_ctx *ctx, int nsrc, int nmis, int nrec, const int *slot_receiver, const float *misfit,
                           const float *norm, int outer_norm, const double *receiver_weights, int anarchy, int ndraw,
                           const double *draw_weights, double *best_value, int *best_index, int which_draw,
                           double *global_of_draw);
/* the most receivers kiwi_hip_outer_misfits takes (the weight rows of a draw tile live in LDS) */
int kiwi_hip_outer_max_receivers(void);
/* HIP-event durations [ms] of the last kiwi_hip_outer_misfits: ms[0] uploads, ms[1] kernels, ms[2] downloads */
int kiwi_hip_get_outer_ms(kiwi_hip_ctx *ctx, float ms[3]);
/* Least-squares coefficients of K basis sources per group under the time-domain l2norm, on the device (kiwi_amd/csrc/kiwi_linfit.hpp).
 * Sources [isrc0, isrc0 + ngroup K) of the uploaded batch are ngroup groups of K consecutive basis sources, 1 <= K <=
 * kiwi_hip_linear_fit_max_basis().  With s_i = what the l2norm comparator compares of basis source i (syn_factor x the moment-
 * scaled, rise-time-folded, tapered synthetic; the frequency-filtered trace where the receiver has a misfit filter) and d the
 * reference side of the same comparison, per (group, enabled receiver r), summed over the receiver's slots, in fp64:
 *     G_r[i][j] = dt sum_t s_i[t] s_j[t] (i <= j)     b_r[i] = dt sum_t s_i[t] d[t]     R_r = dt sum_t d[t]^2
 * NN = K (K + 1) / 2 + K + 1 numbers laid out as: G upper triangle by rows, b, R.  The receivers are folded with w_r =
 * receiver_weight[r] (NULL: ones; 0 excludes; disabled receivers never count), divided by sqrt(R_r) if anarchy != 0 (a receiver
 * with R_r = 0 then has weight 0): G = sum w_r^2 G_r, likewise b and R.  G is scaled to unit diagonal and solved by Cholesky:
 *   coef       [ngroup][K]  the minimiser x of | d - sum_i x_i s_i |
 *   misfit     [ngroup]     sqrt(max(R - 2 x.b + x.G.x, 0) / R): the global misfit (l2norm inner and outer norm) of sum_i x_i s_i
 *   status     [ngroup]     0 solved; 1 no solution: a diagonal element that is not positive, a pivot <= K 2^-52, or R not positive;
 *                           2 a basis source of the group failed to discretise (kiwi_hip_get_source_status)
 *   pivot_min  [ngroup] or NULL: the smallest Cholesky pivot of the scaled matrix reached (1 for an orthogonal basis, towards 0
 *                           for a dependent one; rank deficiency shows as a pivot of round-off size, which the breakdown test
 *                           need not catch: judge by this number)
 *   normal     [ngroup][NN] or NULL: the weighted sums G, b, R (unscaled)
 *   normal_by_receiver [ngroup][nrec][NN] or NULL: G_r, b_r, R_r, unweighted; zeros for disabled receivers
 * Groups with status != 0 answer NaN coefficients and misfit; their sums (and, for status 1, the pivot reached) are still returned.
 * Every sum has a fixed order (no atomics; tests/linfit_restatement.py restates it): the answer does not depend on K's
 * neighbours, on chunking (KIWI_HIP_CHUNK_MB), on isrc0 or on how a list is cut into pieces.  The evaluation is kiwi_hip_eval's:
 * misfits, norm factors and global misfits of the basis sources are left as an evaluation with kept synthetics leaves them.
 * Refused (non-zero, kiwi_hip_last_error names the reason): a misfit method other than l2norm, floating shift ranges, an enabled
 * receiver without a misfit taper or without references, K out of range, a range that is not inside the batch. */
int kiwi_hip_linear_fit(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, double *coef,
                        double *misfit, int *status, double *pivot_min, double *normal, double *normal_by_receiver);
/* The same for a parameter list params[ngroup * K][nparams] of any length: discretised and uploaded piece by piece as
 * kiwi_hip_misfits_for_params does (piece: sources per piece, rounded down to a multiple of K; <= 0: that call's default); a
 * context over several devices cuts the GROUP list into one contiguous range per device.  Afterwards the context holds the head
 * of the list. */
int kiwi_hip_linear_fit_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                               const double *receiver_weight, int anarchy, double *coef, double *misfit, int *status,
                               double *pivot_min, double *normal, double *normal_by_receiver);
/* the most basis sources per group (the accumulators of a thread are registers); answers without a device */
int kiwi_hip_linear_fit_max_basis(void);
/* HIP-event durations [ms] of the last linear fit on this context: ms[0] evaluation, ms[1] fit kernels, ms[2] downloads */
int kiwi_hip_get_linear_fit_ms(kiwi_hip_ctx *ctx, float ms[3]);
/* The same coefficients under an l1 OUTER norm -- one noisy receiver must not drag the fit --, by iteratively reweighted least
 * squares on the device (kiwi_amd/csrc/kiwi_linfit_robust.hpp).  The INNER norm is the context's misfit method; outer_norm is 1
 * l1norm or 2 l2norm as for kiwi_hip_outer_misfits.  With x_0 the solution of kiwi_hip_linear_fit (same weights, same anarchy),
 * R_r, b_r, G_r its per-receiver sums, w_r = receiver_weight[r] (NULL: ones; 0 and disabled receivers never count; a receiver whose
 * R_r is not positive is skipped), T_r the samples of receiver r's windows:
 *   l2norm, 2   forwards to kiwi_hip_linear_fit: its coef, misfit and status bit for bit; niter and eps are ignored;
 *               trace[g][0] holds that misfit in both columns, the other entries NaN
 *   l2norm, 1   per iteration m_r = sqrt(max(R_r - 2 x.b_r + x.G_r.x, 0)), n_r = sqrt(R_r), v_r = w_r (anarchy: w_r / n_r),
 *               u_r = v_r / max(m_r, eps n_r); solve sum_r u_r (G_r, b_r).  misfit = sum v_r m_r / sum v_r n_r: make_global_misfits'
 *               l1norm on the l2norm misfits per receiver.  All iterations in one launch on the sums the l2 start left behind
 *   l1norm, 1   per iteration one pass over the kept synthetics: e[t] = d[t] - sum_k x_k s_k[t], a_r = eps sqrt(R_r / (dt T_r)) (eps x
 *               the receiver's reference RMS), om[t] = 1 / max(|e[t]|, a_r); G_r = dt sum om s_i s_j, b_r = dt sum om s_i d,
 *               L_r = dt sum |e|, D_r = dt sum |d|; v_r = w_r (anarchy: w_r / D_r); solve sum_r v_r (G_r, b_r).  misfit =
 *               sum v_r L_r / sum v_r D_r: the global misfit with l1norm inside and outside
 *   l1norm, 2   refused: the square of a sum of absolute values has no quadratic majoriser of this form
 * Each solve is kiwi_hip_linear_fit's (diagonal scaling, Cholesky, pivot test K 2^-52).  niter >= 0 reweighted solves are made;
 * eps > 0 (relative; 1e-3 is a good start) bounds the weights, and the iteration descends on the Huber function with that
 * threshold, which lies within eps / 2 x (threshold sum / norm sum) below the true misfit.
 *   coef    [ngroup][K]  x_niter            misfit  [ngroup]  the true misfit (above) at x_niter
 *   status  [ngroup]     0 solved; 1 no l2 start; 2 a basis source failed to discretise (both answer NaN, as kiwi_hip_linear_fit);
 *                        3 a reweighted system failed the pivot test at iteration i: coef is x_i, misfit its misfit
 *   trace   [ngroup][niter + 1][2] or NULL: (smoothed objective, true misfit) at x_i; NaN rows after a status 3, and for status 1, 2
 * No host round trip between iterations; every sum in a fixed order (tests/linfit_robust_restatement.py): the answer does not
 * depend on chunking, isrc0, piece or the number of devices.  The basis sources' misfits are left as an evaluation under the
 * context's method leaves them.  Refused: what kiwi_hip_linear_fit refuses (with l1norm allowed beside outer_norm 1), niter < 0, eps
 * that is not positive and finite. */
int kiwi_hip_linear_fit_robust(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int outer_norm, const double *receiver_weight,
                               int anarchy, int niter, double eps, double *coef, double *misfit, int *status, double *trace);
/* ... for a parameter list, cut into pieces and over devices as kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_robust_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                      int outer_norm, const double *receiver_weight, int anarchy, int niter, double eps,
                                      double *coef, double *misfit, int *status, double *trace);
/* HIP-event durations [ms] of the last linear fit of either kind: ms[0] evaluation, ms[1] l2 start (Gram and solve kernels),
 * ms[2] reweighting passes, ms[3] downloads */
int kiwi_hip_get_linear_fit_robust_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* kiwi_hip_linear_fit for 1 <= K <= kiwi_hip_linear_fit_wide_max_basis() basis sources per group, with an optional quadratic
 * penalty and optional non-negative coefficients: the multi-time-window slip inversion, where every patch of a fault in every
 * time window is a basis source whose moment must not be negative and neighbouring patches are tied by a smoothing term
 * (kiwi_amd/slipfit.py; kiwi_amd/csrc/kiwi_linfit_wide.hpp).  The same s_i, d, G_r, b_r, R_r, layout (NN = K (K + 1) / 2 + K + 1),
 * fold (receiver_weight, anarchy), scaling to unit diagonal, Cholesky, pivot test K 2^-52, misfit formula and statuses 0, 1, 2;
 * for K <= 8 with nonneg = 0 and no penalty every output equals kiwi_hip_linear_fit's bit for bit.
 *   penalty    [K (K + 1) / 2] or NULL: the upper triangle by rows of a symmetric P.  After the fold G_ij = G_ij + lam P_ij with
 *              lam = 1 (penalty_relative = 0) or lam = (sum_i G_ii) / K, the mean diagonal before the penalty is added
 *              (penalty_relative != 0).  `normal` returns the sums WITHOUT the penalty and `misfit` is the data misfit
 *              sqrt(max(R - 2 x.b + x.G.x, 0) / R) with them; pivot_min, and the diagonal test of status 1, refer to the penalised matrix
 *   nonneg     0: free coefficients.  1: every coefficient >= 0, by the active-set method of Lawson and Hanson on the normal
 *              equations in the scaled variables (A the scaled penalised matrix, c_i = b_i s_i, x = 0, passive set P empty):
 *              (1) w_i = c_i - sum_{j in P} A_ij x_j for i outside P and not barred; the largest (lowest index among equals) joins
 *              P as i*, unless there is none or it is not > 10 K 2^-52 max_i |c_i|: finished.  (2) Solve A_PP z = c_P by the same
 *              Cholesky over P ascending; a failed pivot takes i* out of P and bars it for the rest of the call (a dependent
 *              column), back to (1).  (3) Every z_i > 0: x_P = z, back to (1); otherwise x moves towards z by alpha = min over i in P
 *              with z_i <= 0 of x_i / (x_i - z_i) (lowest index among equals), that index becomes exactly 0, every i with x_i <= 0
 *              leaves P, back to (2).  After 3 K solves: status 4, the current (feasible) x is returned.  Status 1 then only for
 *              a diagonal that is not positive, R not positive, or a scaled b_i or matrix element that is not finite (pivot_min 0);
 *              pivot_min is otherwise the smallest pivot of the last solve that did not break down
 *   status     additionally 4: the cap of 3 K solves was reached (coef and misfit of the feasible iterate)
 *   npositive  [ngroup] or NULL: the coefficients > 0        nsolves  [ngroup] or NULL: Cholesky solves made (1 with nonneg = 0)
 * The whole active-set loop runs on the device without a host round trip; every sum has a fixed order
 * (tests/linfit_wide_restatement.py): the answer does not depend on chunking, isrc0, piece or the number of devices.  Refused:
 * what kiwi_hip_linear_fit refuses, K outside 1 .. 64, nonneg other than 0 or 1, a penalty entry that is not finite.
 * kiwi_hip_get_linear_fit_ms reports the call (ms[1]: Gram and solve kernels). */
int kiwi_hip_linear_fit_wide(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, int nonneg,
                             const double *penalty, int penalty_relative, double *coef, double *misfit, int *status,
                             double *pivot_min, int *npositive, int *nsolves, double *normal, double *normal_by_receiver);
/* ... for a parameter list, cut into pieces and over devices as kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_wide_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                    const double *receiver_weight, int anarchy, int nonneg, const double *penalty,
                                    int penalty_relative, double *coef, double *misfit, int *status, double *pivot_min,
                                    int *npositive, int *nsolves, double *normal, double *normal_by_receiver);
/* HIP-event durations [ms] of the last wide linear fit, which kiwi_hip_get_linear_fit_ms reports as one figure: ms[0] Gram kernels,
 * ms[1] solve kernel (fold, penalty, Cholesky or active-set loop) */
int kiwi_hip_get_linear_fit_wide_ms(kiwi_hip_ctx *ctx, float ms[2]);

/* ---- misfits in several frequency bands and norms from ONE synthesis (kiwi_bands.hpp).  A band is a misfit method (1 to 6: l2norm,
 * l1norm, ampspec_l2norm, ampspec_l1norm, scalar_product, peak) plus an optional frequency filter, the same for every receiver as
 * kiwi_hip_set_filter(ctx, 0, ...) means it; npts[b] == 0: no filter.  x / y: the control points of the bands' filters
 * concatenated band after band.  nband == 0 removes the bands.  Refused: more than kiwi_hip_misfit_bands_max() bands, a floating
 * method, a filter of one control point.  Setting bands changes nothing about kiwi_hip_eval and kiwi_hip_get_misfits. */
int kiwi_hip_misfit_bands_max(void);                       /* 16; answers without a device */
int kiwi_hip_set_misfit_bands(kiwi_hip_ctx *ctx, int nband, const int *method, const int *npts, const float *x, const float *y);
int kiwi_hip_get_misfit_bands(kiwi_hip_ctx *ctx, int *nband);
/* Sources [isrc0, isrc0 + nsrc) of the uploaded batch are synthesised once and compared in every band: misfit and norm
 * [nsrc][nband][nmis], global [nsrc][nband]; any of them may be NULL.  For every band b the three are bit for bit what
 * kiwi_hip_get_misfits returns after kiwi_hip_set_filter(ctx, 0, band b's filter) + kiwi_hip_set_misfit_method(ctx, band b's method)
 * + kiwi_hip_eval with everything else unchanged, whenever the two calls' synthetics are the same bits: always under
 * KIWI_ARITH_EXACT; under KIWI_ARITH_FUSED a different batch shape may choose a different accumulate kernel instantiation, and the
 * tolerance of that contract applies, 1e-6 of max(misfit, norm factor).  One exception under either contract: when no source of
 * the uploaded batch has a rise time, a plain evaluation under an unfiltered time-domain method compares inside the accumulate
 * kernel, with its fp64 partial sums in another fixed order than the band call's; such a band then agrees with it within 1e-6 of
 * max(misfit, norm factor), and bit for bit where KIWI_HIP_FUSE=0 makes the plain evaluation use the order the bands use.  The context's own method and filters are not used for the
 * bands and stay as they are; they are evaluated on the way by the separate comparator kernels, so that kiwi_hip_get_misfits
 * afterwards returns for the range what a plain kiwi_hip_eval leaves (with the same two provisos) -- never band values.  Sources that
 * failed to discretise read as zeros.  Refused, nothing approximated: no bands set; an enabled receiver without a taper or
 * without references; a floating method as the context's own; a range outside the batch; with a band that has a filter or a
 * spectral method: KIWI_HIP_FUSED_FFT=0, or a (source, slot) pair whose transform length lies outside 64 .. 32768 samples (the
 * message names the length). */
int kiwi_hip_band_misfits(kiwi_hip_ctx *ctx, int isrc0, int nsrc, float *misfit, float *norm, float *global);
/* ... for a parameter list of any length: cut into pieces, the host discretiser overlapped and the list sharded over the devices
 * of a kiwi_hip_init_multi context exactly as kiwi_hip_misfits_for_params does; status [nsrc] (or NULL) as there.  The results do
 * not depend on piece, KIWI_HIP_CHUNK_MB, or the number of devices. */
int kiwi_hip_band_misfits_for_params(kiwi_hip_ctx *ctx, int sourcetype, int nsrc, const float *params, int piece,
                                     float *misfit, float *norm, float *global, int *status);
/* HIP-event durations [ms] of the last band call on this context: ms[0] evaluation (geometry, accumulate, the context's own
 * comparator), ms[1] band kernels (with the reference variants made on the way), ms[2] downloads */
int kiwi_hip_get_band_misfits_ms(kiwi_hip_ctx *ctx, float ms[3]);

/* ---- misfits at many origin times from ONE synthesis (kiwi_timescan.hpp).  Offsets are whole samples, k0 + j kstep for
 * j = 0 .. nk - 1.  Definition: for an uploaded source s and an integer offset k the scan's misfit is what the comparator gives when
 * the raw synthetic row of s is read k samples earlier, syn_k[t] = syn_0[t - k] -- the source k dt later -- and everything else is as
 * in a plain evaluation: rise-time fold, moment, synthetics factor, the receiver's taper at its fixed place, the receiver's filter,
 * the context's misfit method, the references and the reference variants (transform lengths) of the plain evaluation.  Offset 0 is
 * the plain evaluation; the norm factors do not depend on the offset.  The scan equals separate evaluations at time + k dt in bits
 * only where every centroid's time / dt is exact in fp32 (and, with a filter or a spectral method, where the moved source asks for the
 * same transform length); otherwise the two differ by the rounding of the fractional shift.  As for the bands, an unfiltered
 * time-domain method of a batch without rise times is compared inside the accumulate kernel by a plain evaluation, in another fixed
 * order of its fp64 partial sums: the scan then agrees with it within 1e-6 of max(misfit, norm factor), and bit for bit under
 * KIWI_HIP_FUSE=0; under KIWI_ARITH_FUSED the same 1e-6 applies throughout.
 * misfit [nsrc][nk][nmis], norm [nsrc][nmis], global [nsrc][nk], best [nsrc]: index j of the smallest global misfit of the source,
 * the lowest among equal values; any of them may be NULL.  Sources that failed to discretise read as zeros, best = -1.  The rows
 * are made max |k| samples wider on either side for the duration of the call only: afterwards the context behaves as if the call
 * had not happened, and kiwi_hip_get_misfits returns for the range what a plain kiwi_hip_eval leaves.  Refused, nothing
 * approximated: a floating method; an enabled receiver without a taper or without references; a range outside the batch; nk < 1,
 * nk > kiwi_hip_time_scan_max_offsets(), kstep < 1, an offset beyond kiwi_hip_time_scan_max_shift(); a row (window + 2 x (fold halo
 * + max |k|)) too long for LDS (the message names the length; INTEGRATION.md, Limits); with a filtered or spectral slot:
 * KIWI_HIP_FUSED_FFT=0, or a transform length outside 64 .. 32768 samples. */
int kiwi_hip_time_scan_max_shift(void);                    /* 1024 samples; answers without a device */
int kiwi_hip_time_scan_max_offsets(void);                  /* 256; answers without a device */
int kiwi_hip_time_scan(kiwi_hip_ctx *ctx, int isrc0, int nsrc, int k0, int kstep, int nk,
                       float *misfit, float *norm, float *global, int *best);
/* ... for a parameter list of any length: pieces, overlapped discretiser and shards of a kiwi_hip_init_multi context exactly as
 * kiwi_hip_misfits_for_params; status [nsrc] (or NULL) as there.  The results do not depend on piece, KIWI_HIP_CHUNK_MB, or the
 * number of devices. */
int kiwi_hip_time_scan_for_params(kiwi_hip_ctx *ctx, int sourcetype, int nsrc, const float *params, int piece, int k0, int kstep, int nk,
                                  float *misfit, float *norm, float *global, int *best, int *status);
/* HIP-event durations [ms] of the last scan call on this context: ms[0] evaluation (geometry, accumulate, the context's own
 * comparator), ms[1] scan kernels, ms[2] downloads */
int kiwi_hip_get_time_scan_ms(kiwi_hip_ctx *ctx, float ms[3]);
/* ---- the linear fit at many origin times from ONE synthesis of the basis (kiwi_amd/csrc/kiwi_linfit_timescan.hpp): the best
 * coefficients of every group at every offset k0 + j kstep, j < nk -- with six elementary tensors per group, a free moment tensor at
 * every (location, origin time) node from six syntheses per location.  Groups are kiwi_hip_linear_fit's: K consecutive basis sources,
 * 1 <= K <= kiwi_hip_linear_fit_max_basis().  Offsets are kiwi_hip_time_scan's, with its limits kiwi_hip_time_scan_max_offsets() and
 * kiwi_hip_time_scan_max_shift().  Definition: for group g and offset k, basis source i has row_i = its folded, moment-scaled,
 * untapered synthetic, and over the receiver's window
 *     s_{i,k}[t] = fp32(syn_factor x fp32(row_i[t - k] x taper[t]))
 * -- the source k dt later, under the receiver's taper at its fixed place --; d[t] is the tapered reference.  G_r(k), b_r(k), R_r
 * (which does not depend on k), the layout NN = K (K + 1) / 2 + K + 1, the fold over the receivers (receiver_weight, anarchy), the
 * scaling, the Cholesky, the pivot test, the misfit formula and the statuses 0 / 1 / 2 are exactly kiwi_hip_linear_fit's.
 *   coef       [ngroup][nk][K]       misfit  [ngroup][nk]       status  [ngroup][nk]
 *   pivot_min  [ngroup][nk] or NULL
 *   best       [ngroup] or NULL: the index j of the smallest misfit[g][j] among the offsets with status 0, the lowest index among
 *                           equal values; -1 when no offset is solved
 *   normal     [ngroup][nk][NN] or NULL: the weighted sums G, b, R (unscaled)
 * A group with a basis source that failed to discretise has status 2 and NaN at every offset, best = -1.
 * Equalities: offset 0 is kiwi_hip_linear_fit bit for bit (same kept sample, same summation order).  Offset k is bit for bit
 * kiwi_hip_linear_fit on a context whose references and tapers are moved by -k samples.  Offset k equals a fit of the sources moved to
 * time + k dt in bits only where every centroid's time / dt is exact in fp32; otherwise the two differ by the rounding of the
 * fractional shift.  (Always under KIWI_ARITH_EXACT; under KIWI_ARITH_FUSED two calls' synthetics may come from different accumulate
 * kernel instantiations, and the answers then agree within that contract's 1e-6 of the traces times the condition number of G.)
 * Every sum has a fixed order: the answer does not depend on nk's split into passes, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or
 * the number of devices.  The rows are made max |k| samples wider for the duration of the call only, as by kiwi_hip_time_scan:
 * afterwards the context behaves as if the call had not happened, and kiwi_hip_get_misfits returns for the basis sources what a
 * plain kiwi_hip_eval leaves.  There is no limit on the window length.
 * Refused, nothing approximated: everything kiwi_hip_linear_fit refuses; everything kiwi_hip_time_scan refuses about nk, kstep and
 * the offsets; an enabled receiver with a misfit filter (the taper sits in front of the filter, so every basis source and offset
 * would need a transform of its own).  There is no robust, wide or per-receiver-shift form and no normal_by_receiver. */
int kiwi_hip_linear_fit_time_scan(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int k0, int kstep, int nk,
                                  const double *receiver_weight, int anarchy, double *coef, double *misfit, int *status,
                                  double *pivot_min, int *best, double *normal);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_time_scan_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                         int k0, int kstep, int nk, const double *receiver_weight, int anarchy, double *coef,
                                         double *misfit, int *status, double *pivot_min, int *best, double *normal);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram-scan kernel, ms[2] solve kernels,
 * ms[3] downloads */
int kiwi_hip_get_linear_fit_time_scan_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the Gram-scan kernel walks its work for K basis sources: *per_pass offsets per workgroup (their accumulators are registers),
 * *tile window samples per LDS tile; answers without a device.  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_linear_fit_time_scan_shape(int K, int *per_pass, int *tile);
/* ---- the misfits of MANY GIVEN coefficient vectors per group from the normal equations kiwi_hip_linear_fit keeps on the device
 * (kiwi_amd/csrc/kiwi_linfit_candidates.hpp): the synthetics are linear in the coefficients, so a whole grid of trial mechanisms
 * at a location -- every double couple over strike x dip x rake as a combination of the six elementary tensors -- costs the six
 * syntheses of the basis and no more.  Groups, K, receiver_weight and anarchy are kiwi_hip_linear_fit's; the context's misfit method
 * (the INNER norm) must be l2norm.  candidates [ncand][K] is shared by all groups.  With G_r, b_r, R_r the sums of receiver r, G, b, R
 * their weighted fold, and for a vector x: x.b = sum_i x_i b_i from zero, (G x)_i = sum_j G_ij x_j from zero, x.G.x = sum_i x_i (G x)_i,
 * all in ascending index order, q(x; G, b, R) = max((R - 2 x.b) + x.G.x, 0):
 *   outer_norm 2 (l2norm)  misfit = sqrt(q(x; G, b, R) / R): kiwi_hip_linear_fit's misfit expression at the given x
 *   outer_norm 1 (l1norm)  receivers r ascending, skipped where w_r == 0 or R_r <= 0: m_r = sqrt(q(x; G_r, b_r, R_r)), n_r = sqrt(R_r),
 *                          v_r = w_r (anarchy: w_r / n_r); misfit = (sum v_r m_r) / (sum v_r n_r): make_global_misfits' l1norm over the
 *                          receivers' l2norm misfits, iterate 0 of kiwi_hip_linear_fit_robust (inner l2norm) at the given x
 *   free_scale 1           (outer_norm 2 only) a candidate is a direction u: a = (u.b) / (u.G.u) on the folded sums, x = a u, the
 *                          misfit as above; NaN for both unless u.G.u > 0.  A negative a is returned as it is (the opposite mechanism)
 *   best_index  [ngroup]   the candidate of the smallest misfit: NaN misfits passed over, the LOWEST index among equal values; -1 if none
 *   best_misfit [ngroup]   its misfit, or NaN
 *   status      [ngroup]   0 evaluated; 1 no data (l2norm: R not positive; l1norm: no receiver counts): NaN, best_index -1;
 *                          2 a basis source of the group failed to discretise: NaN, best_index -1
 *   misfit      [ngroup][ncand] or NULL        scale  [ngroup][ncand] or NULL (free_scale only): a
 *   receiver_misfit  float [ngroup][ncand][nrec] or NULL: m_r;  receiver_norm  float [ngroup][nrec] or NULL: n_r; 0 for receivers that
 *                          are disabled or skipped (and for status 2), NaN m_r for a candidate whose scale is NaN.  With one slot per
 *                          receiver they are what kiwi_hip_outer_misfits takes: the bootstrap over the receivers of a mechanism grid
 *   fit_coef    [ngroup][K] or NULL, fit_misfit [ngroup] or NULL: the free fit of the same groups, kiwi_hip_linear_fit's bits
 * Every sum has a fixed order (tests/linfit_candidates_restatement.py): the answer does not depend on how candidates and receivers
 * are tiled, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.  Afterwards the context is what
 * kiwi_hip_linear_fit leaves.  Refused, nothing approximated: everything kiwi_hip_linear_fit refuses; ncand < 1; a candidate entry
 * that is not finite; outer_norm other than 1, 2; free_scale other than 0, 1; free_scale with outer_norm 1; scale without free_scale.
 * Under the outer l1norm a receiver of several components counts with the l2 misfit of all its components together. */
int kiwi_hip_linear_fit_candidates(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates, int outer_norm,
                                   const double *receiver_weight, int anarchy, int free_scale, int *best_index, double *best_misfit,
                                   int *status, double *misfit, double *scale, float *receiver_misfit, float *receiver_norm,
                                   double *fit_coef, double *fit_misfit);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_candidates_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                          int ncand, const double *candidates, int outer_norm, const double *receiver_weight,
                                          int anarchy, int free_scale, int *best_index, double *best_misfit, int *status,
                                          double *misfit, double *scale, float *receiver_misfit, float *receiver_norm,
                                          double *fit_coef, double *fit_misfit);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram and solve kernels, ms[2] candidate
 * kernels, ms[3] downloads */
int kiwi_hip_get_linear_fit_candidates_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the candidate kernel walks its work: *candidates_per_workgroup (one per lane), *receivers_per_stage rows of sums per LDS
 * stage; answers without a device.  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_linear_fit_candidates_shape(int K, int *candidates_per_workgroup, int *receivers_per_stage);
/* ---- the candidate evaluation at MANY ORIGIN TIMES from one synthesis of the basis
 * (kiwi_amd/csrc/kiwi_linfit_candidates_timescan.hpp): the best double couple, depth and origin time from six syntheses per location.
 * Nothing new is defined.  Groups, K, receiver_weight and anarchy are kiwi_hip_linear_fit's; the offsets k0 + j kstep, j < nk, and
 * their limits are kiwi_hip_time_scan's; the sums of offset j are kiwi_hip_linear_fit_time_scan's (the same Gram-scan kernel, the
 * same solve); the misfit of candidate c at offset j, its free_scale scale and its receiver_misfit are
 * kiwi_hip_linear_fit_candidates' expressions on those sums, operation for operation.  candidates [ncand][K] is shared by all
 * groups and offsets.
 *   best_index  [ngroup][nk], best_misfit [ngroup][nk]   per offset, in the candidate call's total order: NaN passed over, the
 *                          smaller value, the LOWEST candidate index
 *   best_offset [ngroup]   the j of the smallest best_misfit[g][j] among the j with best_index[g][j] >= 0, the lowest j among equal
 *                          values; -1 if there is none
 *   best_scale  [ngroup][nk] or NULL (free_scale only): a = (u.b) / (u.G.u) of the winner on the folded sums of (g, j): the bits
 *                          scale[g][j][best_index[g][j]] has; NaN where there is no winner
 *   status      [ngroup]   0 evaluated; 1 no data; 2 a basis source failed to discretise (NaN, -1 indices, zeros per receiver); it does
 *                          not depend on the offset, because R_r does not
 *   cand_misfit [ngroup][ncand] or NULL: each candidate's smallest misfit over the offsets, j ascending, NaN passed over, the first
 *                          j among equal values -- the mechanism cube with the origin time profiled out --; cand_offset
 *                          [ngroup][ncand] or NULL: that j (NaN and -1 where every offset is NaN); cand_scale [ngroup][ncand] or NULL
 *                          (free_scale only): the scale at that j
 *   misfit, scale  [ngroup][nk][ncand] or NULL;  receiver_misfit  float [ngroup][nk][ncand][nrec] or NULL
 *   receiver_norm  float [ngroup][nrec] or NULL: one row per group; with receiver_misfit read as nk x ncand "sources" they are what
 *                          kiwi_hip_outer_misfits takes: the bootstrap over mechanism and origin time jointly
 *   fit_coef [ngroup][nk][K], fit_misfit [ngroup][nk], fit_status [ngroup][nk], each or NULL: kiwi_hip_linear_fit_time_scan's coef,
 *                          misfit and status
 * Equalities: offset 0 with nk = 1 is kiwi_hip_linear_fit_candidates bit for bit; offset k is bit for bit
 * kiwi_hip_linear_fit_candidates on a context whose references and tapers are moved by -k samples (under KIWI_ARITH_EXACT; under
 * KIWI_ARITH_FUSED as stated for kiwi_hip_linear_fit_time_scan).  The answer does not depend on how candidates and receivers are
 * tiled, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.  Afterwards the context is what
 * kiwi_hip_linear_fit_time_scan leaves.  Refused with a message that starts with "linear_fit_candidates_time_scan:", nothing
 * approximated: everything kiwi_hip_linear_fit_time_scan and kiwi_hip_linear_fit_candidates refuse; best_scale or cand_scale
 * without free_scale; cand_offset without cand_misfit. */
int kiwi_hip_linear_fit_candidates_time_scan(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int k0, int kstep, int nk, int ncand,
                                             const double *candidates, int outer_norm, const double *receiver_weight, int anarchy,
                                             int free_scale, int *best_offset, int *best_index, double *best_misfit, double *best_scale,
                                             int *status, double *cand_misfit, int *cand_offset, double *cand_scale, double *misfit,
                                             double *scale, float *receiver_misfit, float *receiver_norm, double *fit_coef,
                                             double *fit_misfit, int *fit_status);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_candidates_time_scan_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                    int k0, int kstep, int nk, int ncand, const double *candidates, int outer_norm,
                                                    const double *receiver_weight, int anarchy, int free_scale, int *best_offset,
                                                    int *best_index, double *best_misfit, double *best_scale, int *status,
                                                    double *cand_misfit, int *cand_offset, double *cand_scale, double *misfit,
                                                    double *scale, float *receiver_misfit, float *receiver_norm, double *fit_coef,
                                                    double *fit_misfit, int *fit_status);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram-scan kernel, ms[2] solve kernels,
 * ms[3] candidate-scan kernels, ms[4] downloads */
int kiwi_hip_get_linear_fit_candidates_time_scan_ms(kiwi_hip_ctx *ctx, float ms[5]);
/* how the candidate-scan kernel walks its work: *candidates_per_workgroup (one per lane), *receivers_per_stage rows of sums per LDS
 * stage; answers without a device.  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_linear_fit_candidates_time_scan_shape(int K, int *candidates_per_workgroup, int *receivers_per_stage);
/* ---- the JOINT BOOTSTRAP of a candidate search over group (location), origin time and candidate (mechanism) on the device
 * (kiwi_amd/csrc/kiwi_linfit_candidates_bootstrap.hpp): the [candidate][receiver] matrix is never written.  Nothing new is defined.
 * Groups, K (1 .. 8), candidates [ncand][K], receiver_weight and anarchy are kiwi_hip_linear_fit_candidates'; the offsets
 * k0 + j kstep, j < nk, are kiwi_hip_time_scan's (nk = 1 with k0 = 0 is the plain case); draw_weights [ndraw][nrec] and outer_norm
 * are kiwi_hip_outer_misfits'.  The context's method must be l2norm.  There is no free_scale: a scale fitted on all receivers and
 * then held over the draws is not a bootstrap of anything.
 * The equality that defines every output: call kiwi_hip_linear_fit_candidates_time_scan on the same context with the same
 * arguments, free_scale = 0, receiver_misfit and receiver_norm requested; read receiver_misfit [ngroup][nk][ncand][nrec] as
 * nsrc = ngroup nk ncand sources of nmis = nrec slots with slot_receiver = 0 .. nrec - 1, the norm row of group g repeated for each
 * of its sources; call kiwi_hip_outer_misfits with the same outer_norm, receiver_weight, anarchy and draw_weights.  Then
 *   best_value  [ndraw]    is that call's best_value[d], bit for bit
 *   best_group, best_offset, best_cand [ndraw]   are its best_index[d] taken apart as (g nk + j) ncand + c.  A draw with every source
 *                          excluded answers NaN and -1, -1, -1 (kiwi_hip_outer_misfits writes index 0 there: the one deliberate
 *                          difference)
 *   group_value, group_offset, group_cand [ngroup][ndraw], all three or all NULL: the same per group -- kiwi_hip_outer_misfits on
 *                          group g's nk ncand sources alone: the best mechanism and time of every location in every draw, the depth
 *                          profile under resampling
 *   status      [ngroup]   the candidate call's 0 / 1 / 2; groups with status 1 or 2 have zero norms and are excluded from every draw
 * Operation by operation: m_r is the candidate call's receiver misfit (linfit::quad on the row of sums, val = (R - 2 x.b) + x.G.x
 * clamped at 0, the root, ROUNDED TO FLOAT), n_r = (float) sqrt(R_r), both 0 for a receiver that is disabled, has weight 0 or has
 * R_r <= 0; then kiwi_hip_outer_misfits' prepare step with one slot per receiver (under l2norm sqrt(m m), which is m for a float;
 * the receiver weight, under anarchy w / N clipped at zero with N the float n_r widened; a = M rw, b = N rw, both squared under
 * l2norm) and its draw sums ms = ms + a c, ns = ns + b c, receivers ascending from zero, every product and sum rounded on its own;
 * g = ms / ns, the root under l2norm; excluded where ns <= 0, g < 0 or g is NaN.  Order of "best": excluded last, then the value,
 * then the lowest (g, j, c).  This order is total, so nothing depends on tiles, draw passes, chunks (KIWI_HIP_CHUNK_MB), isrc0,
 * piece or the number of devices.
 * A consequence: a draw of all ones is NOT bit for bit kiwi_hip_linear_fit_candidates' misfit under anarchy, because n_r passes
 * through float here, as it does on the host route.  It is bit for bit the host route, and the host route is the contract.  Put a
 * row of ones in as draw 0 to get the plain winner from the same call.
 * Refused with a message that starts with "linear_fit_candidates_bootstrap:", nothing approximated: everything
 * kiwi_hip_linear_fit_candidates_time_scan refuses; ndraw < 1; null draw_weights, best_* or status; a draw_weights or
 * receiver_weight entry that is not finite; more receivers than max_receivers of the shape call (a candidate's misfits of all
 * receivers stay in LDS); only some of the three group_* arrays.  Afterwards the context is what
 * kiwi_hip_linear_fit_candidates_time_scan leaves: the halo put back, the basis sources evaluated plain. */
int kiwi_hip_linear_fit_candidates_bootstrap(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int k0, int kstep, int nk, int ncand,
                                             const double *candidates, int outer_norm, const double *receiver_weight, int anarchy, int ndraw,
                                             const double *draw_weights, double *best_value, int *best_group, int *best_offset,
                                             int *best_cand, int *status, double *group_value, int *group_offset, int *group_cand);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it; the per-draw bests of pieces and devices are combined on the host in the same total order,
 * with the group index of the whole list */
int kiwi_hip_linear_fit_candidates_bootstrap_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                    int k0, int kstep, int nk, int ncand, const double *candidates, int outer_norm,
                                                    const double *receiver_weight, int anarchy, int ndraw, const double *draw_weights,
                                                    double *best_value, int *best_group, int *best_offset, int *best_cand, int *status,
                                                    double *group_value, int *group_offset, int *group_cand);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram-scan kernel, ms[2] solve kernels,
 * ms[3] bootstrap kernels, ms[4] downloads */
int kiwi_hip_get_linear_fit_candidates_bootstrap_ms(kiwi_hip_ctx *ctx, float ms[5]);
/* how the bootstrap kernel walks its work: *candidates_per_workgroup (one per lane), *draws_per_tile weight rows per LDS tile,
 * *max_receivers the most receivers its LDS layout holds (the same for every K); answers without a device.  Non-zero for K outside
 * 1 .. kiwi_hip_linear_fit_max_basis() or a null pointer */
int kiwi_hip_linear_fit_candidates_bootstrap_shape(int K, int *candidates_per_workgroup, int *draws_per_tile, int *max_receivers);
/* ---- the candidate evaluation with PER-RECEIVER TIME SHIFTS (kiwi_amd/csrc/kiwi_linfit_candidates_floating.hpp): the context's
 * misfit method must be floating_l2norm (receiver.f90:439-510): every receiver slides its reference data under the fixed taper by the
 * whole samples of its own range (kiwi_hip_set_floating_shiftrange: fl_lo .. fl_lo + fl_ns - 1), and per candidate the shift with the
 * smallest sum of squared component misfits wins -- the remedy for a velocity model that mis-times single stations, for a whole
 * mechanism grid from the six syntheses of a location.  For a GIVEN x the minimum over the shifts is exact; nothing is fitted.
 * Groups, K, receiver_weight, anarchy and candidates [ncand][K] are kiwi_hip_linear_fit_candidates'.  Per receiver r:
 *   G_r                    kiwi_hip_linear_fit's sums of the tapered kept synthetics (the taper stays with the synthetic: they do not
 *                          depend on the shift)
 *   b_r[q][i], R_r[q]      for shift index q (shift fl_lo + q): dt sum_t s_i[t] a_q[t] and dt sum_t a_q[t]^2 with a_q the reference moved
 *                          by that shift, times the taper (fp32, as the floating evaluation forms it); fp64 sums in the order of G_r's.
 *                          They are the bits kiwi_hip_linear_fit gives on a context whose references were moved by that shift with
 *                          kiwi_hip_shift_ref_seismogram; at shift 0 the bits of the unshifted context
 *   val_q = max((R_r[q] - 2 x.b_r[q]) + x.G_r.x, 0) in kiwi_hip_linear_fit_candidates' order; m_r = sqrt(min_q val_q), the FIRST
 *                          minimum with q ascending; shift_r = fl_lo + argmin; n_r = (sum_q sqrt(R_r[q])) / fl_ns, q ascending: the
 *                          receiver-level form of receiver.f90:501.  A receiver is skipped where w_r == 0 or n_r is not positive
 *   outer_norm 1 (l1norm)  v_r = w_r (anarchy: w_r / n_r); misfit = (sum v_r m_r) / (sum v_r n_r), receivers ascending
 *   outer_norm 2 (l2norm)  misfit = sqrt((sum v_r^2 m_r^2) / (sum v_r^2 n_r^2)), m_r^2 the clamped val; the minimum sits inside the
 *                          sum, so there is no fold-then-evaluate form
 *   best_index, best_misfit [ngroup]   in kiwi_hip_linear_fit_candidates' total order;  status [ngroup]: 0 evaluated; 1 no receiver
 *                          counts: NaN, -1; 2 a basis source of the group failed to discretise: NaN, -1
 *   best_shift  int [ngroup][nrec]     the winner's shifts in samples; 0 for receivers that are disabled or skipped, and without a winner
 *   misfit      [ngroup][ncand] or NULL;  cand_shift  short [ngroup][ncand][nrec] or NULL (needs misfit): every candidate's shifts
 *   receiver_misfit  float [ngroup][ncand][nrec] or NULL: m_r;  receiver_norm  float [ngroup][nrec] or NULL: n_r; zeros as for
 *                          kiwi_hip_linear_fit_candidates.  They are the pair kiwi_hip_outer_misfits takes: the bootstrap over receivers
 * There is no free fit (it is not defined under shifts) and no free_scale.  All ranges (0, 0) and outer_norm 1: bit for bit
 * kiwi_hip_linear_fit_candidates under l2norm.  The answer does not depend on tiling, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the
 * number of devices.  Afterwards the context is what kiwi_hip_eval of the basis sources under floating_l2norm leaves.  Refused with a
 * message that starts with "linear_fit_candidates_floating:", nothing approximated: a method other than floating_l2norm
 * (floating_l1norm is not quadratic in the coefficients); what kiwi_hip_linear_fit refuses otherwise; what
 * kiwi_hip_linear_fit_candidates refuses of ncand, candidates and outer_norm; free_scale other than 0; cand_shift without misfit (or
 * with a range beyond 16 bits).  n_r and the l1norm fold are receiver-level where make_global_misfits works per slot. */
int kiwi_hip_linear_fit_candidates_floating(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates,
                                            int outer_norm, const double *receiver_weight, int anarchy, int free_scale, int *best_index,
                                            double *best_misfit, int *status, int *best_shift, double *misfit, short *cand_shift,
                                            float *receiver_misfit, float *receiver_norm);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_linear_fit_candidates_floating_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                   int ncand, const double *candidates, int outer_norm, const double *receiver_weight,
                                                   int anarchy, int free_scale, int *best_index, double *best_misfit, int *status,
                                                   int *best_shift, double *misfit, short *cand_shift, float *receiver_misfit,
                                                   float *receiver_norm);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram and cross-correlation kernels,
 * ms[2] candidate kernels, ms[3] downloads */
int kiwi_hip_get_linear_fit_candidates_floating_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the kernels walk their work: *candidates_per_workgroup (one per lane), *shifts_per_pass of the cross-correlation kernel (their
 * accumulators are registers), *shifts_per_stage rows of sums per LDS stage of the candidate kernel; answers without a device.
 * Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_linear_fit_candidates_floating_shape(int K, int *candidates_per_workgroup, int *shifts_per_pass, int *shifts_per_stage);
/* ---- the JOINT BOOTSTRAP of a candidate search WITH PER-RECEIVER TIME SHIFTS over group (location) and candidate (mechanism) on the
 * device, with the station delays of every draw's winner (kiwi_amd/csrc/kiwi_linfit_candidates_floating_bootstrap.hpp): neither the
 * [candidate][receiver] misfits nor the [candidate][receiver] shifts are ever written.  Nothing new is defined.  Groups, K, candidates
 * [ncand][K], receiver_weight, anarchy and the floating_l2norm set-up are kiwi_hip_linear_fit_candidates_floating's; draw_weights
 * [ndraw][nrec] and outer_norm are kiwi_hip_outer_misfits'.  There is no origin-time axis and no free_scale.
 * The equality that defines every output: call kiwi_hip_linear_fit_candidates_floating on the same context with the same arguments,
 * misfit, cand_shift, receiver_misfit and receiver_norm requested; read receiver_misfit [ngroup][ncand][nrec] as nsrc = ngroup ncand
 * sources of nmis = nrec slots with slot_receiver = 0 .. nrec - 1, the norm row of group g repeated for each of its sources; call
 * kiwi_hip_outer_misfits with the same outer_norm, receiver_weight, anarchy and draw_weights.  Then
 *   best_value  [ndraw]        is that call's best_value[d], bit for bit
 *   best_group, best_cand [ndraw]   are its best_index[d] taken apart as g ncand + c.  A draw with every source excluded answers NaN,
 *                              -1, -1 and a row of zero shifts (kiwi_hip_outer_misfits writes index 0 there: the one deliberate
 *                              difference)
 *   best_shift  int [ndraw][nrec]   the winner's row cand_shift[best_group][best_cand][.]: the shifts in samples, 0 for a receiver that
 *                              is disabled or skipped.  An int: a shift range beyond 16 bits, which the parent refuses for its
 *                              cand_shift array, is served here
 *   group_value, group_cand [ngroup][ndraw], group_shift int [ngroup][ndraw][nrec], all three or all NULL: the same per group --
 *                              kiwi_hip_outer_misfits on group g's ncand sources alone
 *   status      [ngroup]       the parent call's 0 / 1 / 2; groups with status 1 or 2 have zero norms and never win a draw
 * Operation by operation: m_r = sqrt(min_q val_q) of the parent call ROUNDED TO FLOAT and n_r ROUNDED TO FLOAT, both 0 for a receiver
 * that is skipped; then kiwi_hip_outer_misfits' prepare step with one slot per receiver (under l2norm sqrt(m m), which is m for a
 * float; the receiver weight, under anarchy w / N clipped at zero with N the float n_r widened; a = M rw, b = N rw, both squared under
 * l2norm) and its draw sums ms = ms + a c, ns = ns + b c, receivers ascending from zero, every product and sum rounded on its own;
 * g = ms / ns, the root under l2norm; excluded where ns <= 0, g < 0 or g is NaN.  The shift of a receiver is chosen per (candidate,
 * receiver) before any weight is applied: the draws do not interact with the shift search.  Order of "best": excluded last, then the
 * value, then the lowest (g, c).  This order is total, so nothing depends on tiles, draw passes, chunks (KIWI_HIP_CHUNK_MB), isrc0,
 * piece or the number of devices.  With every range (0, 0) and outer_norm 1: bit for bit kiwi_hip_linear_fit_candidates_bootstrap
 * with nk = 1 at offset 0 on a context under l2norm, and every shift 0.
 * Refused with a message that starts with "linear_fit_candidates_floating_bootstrap:", nothing approximated: everything
 * kiwi_hip_linear_fit_candidates_floating refuses of the set-up, K, ncand, candidates and outer_norm; ndraw < 1; null draw_weights,
 * best_* or status; a draw_weights or receiver_weight entry that is not finite; more receivers than max_receivers of the shape call
 * (a candidate's misfits of all receivers stay in LDS); only some of the three group_* arrays.  Afterwards the context is what
 * kiwi_hip_linear_fit_candidates_floating leaves. */
int kiwi_hip_linear_fit_candidates_floating_bootstrap(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates,
                                                      int outer_norm, const double *receiver_weight, int anarchy, int ndraw,
                                                      const double *draw_weights, double *best_value, int *best_group, int *best_cand,
                                                      int *best_shift, int *status, double *group_value, int *group_cand, int *group_shift);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it; the per-draw bests of pieces and devices are combined on the host in the same total order,
 * with the group index of the whole list, the winner's shift row carried along */
int kiwi_hip_linear_fit_candidates_floating_bootstrap_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params,
                                                             int piece, int ncand, const double *candidates, int outer_norm,
                                                             const double *receiver_weight, int anarchy, int ndraw,
                                                             const double *draw_weights, double *best_value, int *best_group,
                                                             int *best_cand, int *best_shift, int *status, double *group_value,
                                                             int *group_cand, int *group_shift);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] Gram and cross-correlation kernels,
 * ms[2] bootstrap kernels (norms, prepare, candidates, folds, shifts), ms[3] downloads */
int kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the bootstrap kernel walks its work: *candidates_per_workgroup (one per lane), *draws_per_tile weight rows per LDS tile,
 * *max_receivers the most receivers its LDS layout holds (the same for every K); answers without a device.  Non-zero for K outside
 * 1 .. kiwi_hip_linear_fit_max_basis() or a null pointer */
int kiwi_hip_linear_fit_candidates_floating_bootstrap_shape(int K, int *candidates_per_workgroup, int *draws_per_tile, int *max_receivers);
/* The misfits of many GIVEN coefficient vectors per group under the amplitude-spectrum norms (kiwi_spectral_candidates.hpp): the
 * mechanism grid of a location from its six syntheses where the users of the reference search first, ampspec_l2norm (3) or
 * ampspec_l1norm (4) inside a pass band.  The amplitude spectrum is not quadratic in the coefficients, but the complex spectrum is
 * linear in them: X(f) = sum_a x_a S_a(f), S_a the spectra of the K basis sources' tapered traces, so the transforms are paid once
 * per location and a candidate costs K complex multiply-adds and a root per kept bin.  Groups, K, receiver_weight, anarchy and
 * candidates [ncand][K] are kiwi_hip_linear_fit_candidates'; the kernels use (float) x.  Per slot (enabled receiver component):
 *   bins klo .. khi        the smallest range that holds every bin with a non-zero filter weight (0 .. ntrans / 2 without a filter);
 *                          a skipped bin adds exactly nothing (its reference amplitude is |Xref| x 0; a non-zero one is refused)
 *   per bin, ascending     re = xf_0 S_0.re; re = re + xf_a S_a.re, im the same, every product and sum rounded in fp32;
 *                          b = |re + i im| with a correctly rounded root, times the filter weight where the receiver has a filter;
 *                          d = ref_amp - b (synthetics factor as the comparator applies it); one fp64 accumulator: d^2 | |d|
 *   slot misfit            (float) sqrt(df acc) | (float) (df acc), df = 1.f / ((float) ntrans dt); the slot norm factor is the basis
 *                          sources' own (that of the group's first source)
 *   outer fold             make_global_misfits per SLOT with outer_norm 1 (l1norm) or 2 (l2norm), receiver weights and anarchy: the
 *                          expression sequence of kiwi_hip_outer_misfits for one draw of weights 1 -- nothing is receiver-level
 *   free_scale 1           (ampspec_l2norm with outer l2norm only) the candidate is a direction: per slot P = sum a b, Q = sum b b,
 *                          A = sum a a in fp64; s = (sum_r rw_r^2 sum_k df_k P_k) / (sum_r rw_r^2 sum_k df_k Q_k);
 *                          misfit = sqrt(max((A - 2 s P) + s s Q, 0) / D), A the same weighted sum, D the fold's denominator
 *   best_index, best_misfit [ngroup]   NaN passed over, then the value, then the lowest index; -1, NaN if none
 *   status [ngroup]        0 evaluated; 1 no receiver counts; 2 a basis source of the group failed to discretise
 *   misfit, scale          [ngroup][ncand] or NULL (scale needs free_scale)
 *   slot_misfit  float [ngroup][ncand][nmis], slot_norm  float [ngroup][nmis], both or neither: the pair kiwi_hip_outer_misfits takes
 *   spectra      float [ngroup][nmis][spectra_bins][K][2] or NULL: the kept bins of every slot from index 0 (re, im; no filter weight);
 *   spectra_range  int [ngroup][nmis][3]: klo, khi, ntrans;  spectra_ref  float [ngroup][nmis][spectra_bins][2]: reference amplitude
 *                          and filter weight of the kept bins.  spectra_bins from kiwi_hip_spectral_candidates_shape
 * The answer does not depend on tiling, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.  Afterwards the context
 * is what kiwi_hip_eval of the basis sources leaves.  Refused with a message that starts with "spectral_candidates:", nothing
 * approximated: a method other than 3 or 4; an enabled receiver without a misfit taper or without references; K outside 1 .. 8; a
 * range outside the batch; ncand < 1; a candidate that is not finite; a bad outer_norm or free_scale; free_scale outside method 3
 * with outer l2norm, or together with slot_misfit; scale without free_scale; KIWI_HIP_FUSED_FFT=0; a slot whose transform length lies
 * outside 64 .. 32768; basis sources of a group whose transform lengths differ. */
int kiwi_hip_spectral_candidates(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates, int outer_norm,
                                 const double *receiver_weight, int anarchy, int free_scale, int *best_index, double *best_misfit,
                                 int *status, double *misfit, double *scale, float *slot_misfit, float *slot_norm, int spectra_bins,
                                 float *spectra, int *spectra_range, float *spectra_ref);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_spectral_candidates_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece, int ncand,
                                        const double *candidates, int outer_norm, const double *receiver_weight, int anarchy,
                                        int free_scale, int *best_index, double *best_misfit, int *status, double *misfit, double *scale,
                                        float *slot_misfit, float *slot_norm, int spectra_bins, float *spectra, int *spectra_range,
                                        float *spectra_ref);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the spectra kernel alone, ms[2] candidate
 * kernels, ms[3] downloads.  The host's table of kept bins per chunk and its upload lie between ms[0] and ms[1], in neither */
int kiwi_hip_get_spectral_candidates_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the kernels walk their work: *candidates_per_workgroup (one per lane) and *bins_per_stage of spectra per LDS stage of the
 * candidate kernel; ctx may be NULL, the call then answers without a device (*spectra_bins 0).  With a context *spectra_bins is the
 * row length of its spectra arrays (spectra_bins may be NULL).  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_spectral_candidates_shape(kiwi_hip_ctx *ctx, int K, int *candidates_per_workgroup, int *bins_per_stage, int *spectra_bins);
/* The misfits of many GIVEN coefficient vectors per group under the time-domain norms (kiwi_waveform_candidates.hpp): the mechanism
 * grid of a location from its six syntheses under l1norm (2) inside -- the robust norm, which is not quadratic in the coefficients
 * and so has no Gram route -- and, from the residual itself, under l2norm (1).  The waveform is linear in the coefficients:
 * v[t] = sum_a x_a s_a[t], s_a the kept traces of the K basis sources, so a candidate costs K multiply-adds and one |.| per window
 * sample and no synthesis.  Groups, K, receiver_weight, anarchy and candidates [ncand][K] are kiwi_hip_linear_fit_candidates'; the
 * kernels use (float) x.  A misfit filter on a receiver is allowed: the kept rows and the reference side are then the filtered
 * ones, selected as kiwi_hip_linear_fit selects them.  Per slot (enabled receiver component):
 *   per sample, ascending  v = xf_0 s_0[i]; v = v + xf_a s_a[i], every product and sum rounded in fp32; d = ref - v (synthetics
 *                          factor as the comparator applies it); one fp64 accumulator: d^2 | |d|
 *   slot misfit            (float) sqrt(dt acc) | (float) (dt acc); the slot norm factor is that of the group's first source
 *   outer fold             make_global_misfits per SLOT with outer_norm 1 (l1norm) or 2 (l2norm), receiver weights and anarchy: the
 *                          expression sequence of kiwi_hip_outer_misfits for one draw of weights 1
 *   best_index, best_misfit [ngroup]   NaN passed over, then the value, then the lowest index; -1, NaN if none
 *   status [ngroup]        0 evaluated; 1 no receiver counts; 2 a basis source of the group failed to discretise
 *   misfit                 [ngroup][ncand] or NULL
 *   slot_misfit  float [ngroup][ncand][nmis], slot_norm  float [ngroup][nmis], both or neither: the pair kiwi_hip_outer_misfits takes
 * A unit candidate returns its basis source's own slot misfits up to the order of the fp64 sum.  There is no free scale: under
 * l1norm the best scale of a direction has no closed form; the moment axis is more candidates.  The answer does not depend on
 * tiling, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.  Afterwards the context is what kiwi_hip_eval of the
 * basis sources leaves.  Refused with a message that starts with "waveform_candidates:", nothing approximated: a method other than 1
 * or 2 (floating_l2norm goes through kiwi_hip_linear_fit_candidates_floating, the ampspec norms through
 * kiwi_hip_spectral_candidates); an enabled receiver without a misfit taper or without references; K outside 1 .. 8; a range outside
 * the batch; a transform workspace that does not hold one group; ncand < 1; a candidate that is not finite; a bad outer_norm;
 * slot_misfit without slot_norm or the reverse; null mandatory arrays. */
int kiwi_hip_waveform_candidates(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates, int outer_norm,
                                 const double *receiver_weight, int anarchy, int *best_index, double *best_misfit, int *status,
                                 double *misfit, float *slot_misfit, float *slot_norm);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_waveform_candidates_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece, int ncand,
                                        const double *candidates, int outer_norm, const double *receiver_weight, int anarchy,
                                        int *best_index, double *best_misfit, int *status, double *misfit, float *slot_misfit,
                                        float *slot_norm);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the slot kernel, ms[2] the fold kernels,
 * ms[3] downloads.  The host's tables of a chunk and their upload lie between ms[0] and ms[1], in neither */
int kiwi_hip_get_waveform_candidates_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the kernels walk their work: *candidates_per_workgroup (one per lane) and *samples_per_stage of the K rows and the reference
 * side per LDS stage of the slot kernel; answers without a device.  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_waveform_candidates_shape(int K, int *candidates_per_workgroup, int *samples_per_stage);
/* kiwi_hip_waveform_candidates under the floating norms (kiwi_waveform_candidates_floating.hpp): floating_l1norm (8) -- l1 inside
 * against a glitched station AND per-receiver whole-sample shifts against a mis-timed one, at once -- and floating_l2norm (7) in the
 * reference's per-slot form (kiwi_hip_linear_fit_candidates_floating folds that norm per receiver).  Every receiver slides its
 * reference under the fixed taper inside its own range (kiwi_hip_set_floating_shiftrange); the taper stays with the synthetic, so
 * the combined trace v of a candidate is formed once per sample and a further shift costs a subtraction, a |.| and one fp64 add.
 * Groups, K, receiver_weight, anarchy, candidates and the fold are kiwi_hip_waveform_candidates'.  Per receiver and candidate, slots
 * k ascending, shift index q = 0 .. ns - 1 (shift lo + q):
 *   a_q[i]                 the un-tapered reference moved by lo + q, times the taper weight of sample i (one fp32 product)
 *   per sample, ascending  v as in kiwi_hip_waveform_candidates; d = a_q[i] - v (synthetics factor as the comparator applies it); ONE
 *                          fp64 accumulator per (slot, shift): d^2 | |d|
 *   m_kq                   (float) sqrt(dt acc) | (float) (dt acc)
 *   the shift              sum_q = sum_q + (l1 inside ? m_kq : m_kq m_kq) in fp32, k ascending from 0; the FIRST minimum over q wins
 *                          (the receiver's sum decides, not a slot's): exactly how kiwi_hip_eval chooses a source's shifts
 *   slot misfit            m_kq at the winning shift; the slot norm factor is the context's floating one (the mean over the shifts of
 *                          the moved reference's norm)
 *   best_shift             int [ngroup][nrec]: the winner's shifts in samples, 0 for a disabled receiver or where no candidate won
 *   cand_shift             short [ngroup][ncand][nrec] or NULL (needs misfit): every candidate's shifts
 *   best_index, best_misfit, status, misfit, slot_misfit, slot_norm   as in kiwi_hip_waveform_candidates
 * With every range (0, 0) the answers are kiwi_hip_waveform_candidates' under l1norm / l2norm bit for bit.  There is no free scale.
 * The answer does not depend on the pass a shift falls into, tiling, chunking (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of
 * devices.  Afterwards the context is what kiwi_hip_eval of the basis sources leaves.  Refused with a message that starts with
 * "waveform_candidates_floating:", nothing approximated: a method other than 7 or 8 (l1norm and l2norm go through
 * kiwi_hip_waveform_candidates); an enabled receiver without a misfit taper or without references; K outside 1 .. 8; a range outside
 * the batch; ncand < 1; a candidate that is not finite; a bad outer_norm; slot_misfit without slot_norm or the reverse; cand_shift
 * without misfit, or with a shift range beyond 16 bits; null mandatory arrays (best_shift is one). */
int kiwi_hip_waveform_candidates_floating(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates,
                                          int outer_norm, const double *receiver_weight, int anarchy, int *best_index, double *best_misfit,
                                          int *status, int *best_shift, double *misfit, short *cand_shift, float *slot_misfit,
                                          float *slot_norm);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it */
int kiwi_hip_waveform_candidates_floating_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                 int ncand, const double *candidates, int outer_norm, const double *receiver_weight,
                                                 int anarchy, int *best_index, double *best_misfit, int *status, int *best_shift,
                                                 double *misfit, short *cand_shift, float *slot_misfit, float *slot_norm);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the floating slot kernel, ms[2] the fold
 * kernels, ms[3] downloads.  The host's tables of a chunk and their upload lie between ms[0] and ms[1], in neither */
int kiwi_hip_get_waveform_candidates_floating_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the kernel walks its work: *candidates_per_workgroup (one per lane), *samples_per_stage per LDS stage, and *shifts_per_pass
 * whose accumulators a lane holds in registers at once; answers without a device.  Non-zero for K outside
 * 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_waveform_candidates_floating_shape(int K, int *candidates_per_workgroup, int *samples_per_stage, int *shifts_per_pass);
/* kiwi_hip_waveform_candidates at MANY origin times from ONE synthesis of the basis (kiwi_waveform_candidates_timescan.hpp): the best
 * mechanism, depth and origin time under l1norm (2) inside -- the robust norm -- or l2norm (1).  Groups, K (1 .. 8), candidates
 * [ncand][K], receiver_weight, anarchy, outer_norm and the statuses are kiwi_hip_waveform_candidates'; the offsets k_j = k0 + j kstep
 * samples, j < nk, are kiwi_hip_time_scan's, with its limits kiwi_hip_time_scan_max_offsets() and kiwi_hip_time_scan_max_shift().
 * A source moved by k samples has the same synthetic, moved; the receiver's taper and reference stay at their fixed place.  For
 * group g, row_a is the folded, moment-scaled, UNTAPERED synthetic of basis source a over the slot's window widened by S = max |k_j|
 * on either side -- the rows kiwi_hip_linear_fit_time_scan works on --, xf = (float) x.  Per slot (enabled receiver component):
 *   per extended sample e, ONCE per candidate   u[e] = xf_0 row_0[e]; u = u + xf_a row_a[e], a ascending, every product and sum
 *                          rounded in fp32
 *   offset k, window sample i = e + k, i ascending   vt = u[i - k] * taper[i] (one fp32 product); d = ref[i] - vt, ref the tapered
 *                          reference (synthetics factor as the comparator applies it: 1.f ref[i] - syn_factor vt); ONE fp64
 *                          accumulator per offset: d^2 | |d|.  A sample outside the window contributes nothing, also where u is
 *                          not finite
 *   slot misfit            (float) sqrt(dt acc) | (float) (dt acc); the slot norm factors do not depend on k
 *   outer fold             kiwi_hip_waveform_candidates', per (group, offset)
 *   best_index, best_misfit [ngroup][nk]   per offset: NaN passed over, then the value, then the lowest index; -1, NaN if none
 *   best_offset [ngroup]   the index j of the smallest best_misfit in the same order; -1 if none
 *   status [ngroup]        0 evaluated; 1 no receiver counts; 2 a basis source of the group failed to discretise
 *   cand_misfit  double, cand_offset  int [ngroup][ncand] or NULL: per candidate the first smallest misfit over the offsets and its
 *                          index j (NaN, -1 where every offset is NaN); cand_offset needs cand_misfit
 *   misfit                 [ngroup][nk][ncand] or NULL
 *   slot_misfit  float [ngroup][nk][ncand][nmis], slot_norm  float [ngroup][nmis]: with nk x ncand read as sources the pair
 *                          kiwi_hip_outer_misfits takes -- the bootstrap over mechanism and origin time jointly; slot_misfit needs
 *                          slot_norm
 *   rows  float [ngroup][K][row_stride] or NULL: row_a of every basis source, slot m's wlen + 2 S samples from row_offset[m], extended
 *                          sample e at row_offset[m] + S + e (kiwi_hip_waveform_candidates_time_scan_rows); zeros for a group with
 *                          status 2
 * This is the combined source read k samples earlier under the receiver's taper: what kiwi_hip_time_scan would compare for a source
 * with tensor x.  It is NOT kiwi_hip_waveform_candidates bit for bit at offset 0: that call tapers every basis trace before
 * combining (x_a fl(row_a taper)), this one combines first and tapers once, which is what the offsets share; the two agree to
 * rounding.  Two relations are exact: a unit candidate e_a (and K = 1, x = [1]) gives u = row_a, so its slot misfit at offset k is
 * kiwi_hip_time_scan's for basis source a up to the order of the fp64 sum; and the answer does not depend on tiles, passes, chunking
 * (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.  Afterwards the context is what kiwi_hip_eval of the basis sources
 * leaves (offset 0's plain evaluation; the halo is put back).  Refused with a message that starts with
 * "waveform_candidates_time_scan:", nothing approximated: everything kiwi_hip_waveform_candidates refuses; what kiwi_hip_time_scan
 * refuses of the offsets (nk, kstep, the largest shift); an enabled receiver with a misfit filter (the taper sits in front of the
 * filter, so every candidate and offset would need a transform of its own); cand_offset without cand_misfit; slot_misfit without
 * slot_norm or the reverse; null mandatory arrays (best_offset is one). */
int kiwi_hip_waveform_candidates_time_scan(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int k0, int kstep, int nk, int ncand,
                                           const double *candidates, int outer_norm, const double *receiver_weight, int anarchy,
                                           int *best_offset, int *best_index, double *best_misfit, int *status, double *cand_misfit,
                                           int *cand_offset, double *misfit, float *slot_misfit, float *slot_norm, float *rows);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_waveform_candidates_params cuts it */
int kiwi_hip_waveform_candidates_time_scan_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                  int k0, int kstep, int nk, int ncand, const double *candidates, int outer_norm,
                                                  const double *receiver_weight, int anarchy, int *best_offset, int *best_index,
                                                  double *best_misfit, int *status, double *cand_misfit, int *cand_offset, double *misfit,
                                                  float *slot_misfit, float *slot_norm, float *rows);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the rows and scan kernels, ms[2] the fold
 * kernels, ms[3] downloads.  The host's tables of a chunk and their upload lie between ms[0] and ms[1], in neither */
int kiwi_hip_get_waveform_candidates_time_scan_ms(kiwi_hip_ctx *ctx, float ms[4]);
/* how the kernel walks its work: *candidates_per_workgroup (one per lane), *samples_per_stage of extended samples per LDS stage, and
 * *offsets_per_pass whose accumulators a lane holds in registers at once; answers without a device.  Non-zero for K outside
 * 1 .. kiwi_hip_linear_fit_max_basis() */
int kiwi_hip_waveform_candidates_time_scan_shape(int K, int *candidates_per_workgroup, int *samples_per_stage, int *offsets_per_pass);
/* the layout of `rows` for these offsets on this context's receivers: *shift_halo = S, *row_stride floats per basis source, and
 * row_offset [nmis] (or NULL) where each misfit slot's wlen + 2 S samples begin */
int kiwi_hip_waveform_candidates_time_scan_rows(kiwi_hip_ctx *ctx, int k0, int kstep, int nk, int *shift_halo, int *row_stride,
                                                int *row_offset);
/* ---- the JOINT BOOTSTRAP of a WAVEFORM candidate search (l1norm or l2norm inside) over group (location), origin time and candidate
 * (mechanism) on the device (kiwi_amd/csrc/kiwi_waveform_candidates_bootstrap.hpp): the [candidate][slot] array never leaves the
 * device.  Nothing new is defined.  Groups, K (1 .. 8), candidates [ncand][K], receiver_weight, anarchy and the offsets k0 + j kstep,
 * j < nk, are kiwi_hip_waveform_candidates_time_scan's (nk = 1 with k0 = 0 is the plain case: that call's offset 0, which is not
 * kiwi_hip_waveform_candidates bit for bit, see there); draw_weights [ndraw][nrec] and outer_norm are kiwi_hip_outer_misfits'.  The
 * context's method must be l1norm or l2norm.  There is no free scale.
 * The equality that defines every output: call kiwi_hip_waveform_candidates_time_scan on the same context with the same arguments,
 * slot_misfit and slot_norm requested; read slot_misfit [ngroup][nk][ncand][nmis] as nsrc = ngroup nk ncand sources of nmis slots,
 * slot_receiver[m] the receiver of slot m, the norm row of group g repeated for each of its sources; call kiwi_hip_outer_misfits
 * with the same outer_norm, receiver_weight, anarchy and draw_weights.  Then
 *   best_value  [ndraw]    is that call's best_value[d], bit for bit
 *   best_group, best_offset, best_cand [ndraw]   are its best_index[d] taken apart as (g nk + j) ncand + c.  A draw with every source
 *                          excluded answers NaN and -1, -1, -1 (kiwi_hip_outer_misfits writes index 0 there: the one deliberate
 *                          difference)
 *   group_value, group_offset, group_cand [ngroup][ndraw], all three or all NULL: the same per group -- kiwi_hip_outer_misfits on
 *                          group g's nk ncand sources alone
 *   status      [ngroup]   the scan call's 0 / 1 / 2; groups with status 1 or 2 have zero norms and are excluded from every draw
 * Operation by operation (outer_prepare_kernel and outer_draw_kernel of kiwi_outer.hpp): per receiver, its slots ascending,
 * M = M + mv under outer l1norm, M = M + mv mv with the root behind the slots under l2norm, mv the slot misfit as a float, widened;
 * N likewise from the slot norms; rw = w_r, under anarchy q = rw / (N != 0 ? N : -1), rw = q where q > 0 or q is NaN, else 0;
 * a = M rw, b = N rw, both squared under l2norm; ms = ms + a c, ns = ns + b c from zero, receivers ascending, every product and sum
 * rounded on its own; g = ms / ns, the root under l2norm; a source is excluded where ns > 0 fails or g >= 0 fails.  Order of
 * "best": excluded last, then the value, then the lowest (g, j, c).  This order is total, so nothing depends on tiles, draw passes,
 * chunks (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.
 * Refused with a message that starts with "waveform_candidates_bootstrap:", nothing approximated: everything
 * kiwi_hip_waveform_candidates_time_scan refuses, a misfit filter included; ndraw < 1; null draw_weights, best_* or status; a
 * draw_weights or receiver_weight entry that is not finite; more receivers than max_receivers of the shape call (a candidate's
 * column of all receivers stays in LDS); only some of the three group_* arrays.  Afterwards the context is what
 * kiwi_hip_waveform_candidates_time_scan leaves: the halo put back, the basis sources evaluated plain. */
int kiwi_hip_waveform_candidates_bootstrap(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int k0, int kstep, int nk, int ncand,
                                           const double *candidates, int outer_norm, const double *receiver_weight, int anarchy, int ndraw,
                                           const double *draw_weights, double *best_value, int *best_group, int *best_offset,
                                           int *best_cand, int *status, double *group_value, int *group_offset, int *group_cand);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it; the per-draw bests of pieces and devices are combined on the host in the same total order,
 * with the group index of the whole list */
int kiwi_hip_waveform_candidates_bootstrap_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                  int k0, int kstep, int nk, int ncand, const double *candidates, int outer_norm,
                                                  const double *receiver_weight, int anarchy, int ndraw, const double *draw_weights,
                                                  double *best_value, int *best_group, int *best_offset, int *best_cand, int *status,
                                                  double *group_value, int *group_offset, int *group_cand);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the rows and scan kernels, ms[2] the fold
 * kernels, ms[3] bootstrap kernels, ms[4] downloads */
int kiwi_hip_get_waveform_candidates_bootstrap_ms(kiwi_hip_ctx *ctx, float ms[5]);
/* how the bootstrap kernel walks its work: *candidates_per_workgroup (one per lane), *draws_per_tile weight rows per LDS tile,
 * *max_receivers the most receivers its LDS layout holds (the same for every K); answers without a device.  Non-zero for K outside
 * 1 .. kiwi_hip_linear_fit_max_basis() or a null pointer */
int kiwi_hip_waveform_candidates_bootstrap_shape(int K, int *candidates_per_workgroup, int *draws_per_tile, int *max_receivers);
/* ---- the JOINT BOOTSTRAP of a SPECTRAL candidate search (ampspec_l2norm or ampspec_l1norm inside) over group (location) and
 * candidate (mechanism) on the device (kiwi_amd/csrc/kiwi_spectral_candidates_bootstrap.hpp): the [candidate][slot] array never
 * leaves the device.  Nothing new is defined.  Groups, K (1 .. 8), candidates [ncand][K], receiver_weight and anarchy are
 * kiwi_hip_spectral_candidates'; draw_weights [ndraw][nrec] and outer_norm are kiwi_hip_outer_misfits'.  The context's method must be
 * ampspec_l2norm or ampspec_l1norm; a misfit filter on a receiver is allowed, as in kiwi_hip_spectral_candidates.  There is no
 * free scale.
 * The equality that defines every output: call kiwi_hip_spectral_candidates on the same context with the same arguments, free_scale
 * 0, slot_misfit and slot_norm requested; read slot_misfit [ngroup][ncand][nmis] as nsrc = ngroup ncand sources of nmis slots,
 * slot_receiver[m] the receiver of slot m, the norm row of group g repeated for each of its sources; call kiwi_hip_outer_misfits
 * with the same outer_norm, receiver_weight, anarchy and draw_weights.  Then
 *   best_value  [ndraw]    is that call's best_value[d], bit for bit
 *   best_group, best_cand [ndraw]   are its best_index[d] taken apart as g ncand + c.  A draw with every source excluded answers NaN
 *                          and -1, -1 (kiwi_hip_outer_misfits writes index 0 there: the one deliberate difference)
 *   group_value, group_cand [ngroup][ndraw], both or both NULL: the same per group -- kiwi_hip_outer_misfits on group g's ncand
 *                          sources alone
 *   status      [ngroup]   kiwi_hip_spectral_candidates' 0 / 1 / 2; groups with status 1 or 2 are excluded from every draw
 * Operation by operation the slot misfits are kiwi_hip_spectral_candidates' and the fold is kiwi_hip_waveform_candidates_bootstrap's
 * (see there).  Order of "best": excluded last, then the value, then the lowest (g, c).  This order is total, so nothing depends on
 * tiles, draw passes, chunks (KIWI_HIP_CHUNK_MB), isrc0, piece or the number of devices.
 * Refused with a message that starts with "spectral_candidates_bootstrap:", nothing approximated: everything
 * kiwi_hip_spectral_candidates refuses of the set-up; ndraw < 1; null draw_weights, best_* or status; a draw_weights or
 * receiver_weight entry that is not finite; more receivers than max_receivers of the shape call (a candidate's column of all
 * receivers stays in LDS); one of the two group_* arrays without the other.  Afterwards the context is what
 * kiwi_hip_spectral_candidates leaves. */
int kiwi_hip_spectral_candidates_bootstrap(kiwi_hip_ctx *ctx, int isrc0, int ngroup, int K, int ncand, const double *candidates,
                                           int outer_norm, const double *receiver_weight, int anarchy, int ndraw,
                                           const double *draw_weights, double *best_value, int *best_group, int *best_cand, int *status,
                                           double *group_value, int *group_cand);
/* ... for a parameter list params[ngroup * K][nparams] of any length, cut into pieces and over devices at group boundaries as
 * kiwi_hip_linear_fit_params cuts it; the per-draw bests of pieces and devices are combined on the host in the same total order,
 * with the group index of the whole list */
int kiwi_hip_spectral_candidates_bootstrap_params(kiwi_hip_ctx *ctx, int sourcetype, int ngroup, int K, const float *params, int piece,
                                                  int ncand, const double *candidates, int outer_norm, const double *receiver_weight,
                                                  int anarchy, int ndraw, const double *draw_weights, double *best_value,
                                                  int *best_group, int *best_cand, int *status, double *group_value, int *group_cand);
/* HIP-event durations [ms] of the last such call on this context: ms[0] evaluation, ms[1] the spectra kernel, ms[2] the slot kernel,
 * ms[3] bootstrap kernels, ms[4] downloads */
int kiwi_hip_get_spectral_candidates_bootstrap_ms(kiwi_hip_ctx *ctx, float ms[5]);
/* how the kernels walk their work: *candidates_per_workgroup (one per lane, of the slot kernel and of the bootstrap kernel),
 * *draws_per_tile weight rows per LDS tile, *max_receivers the most receivers the bootstrap kernel's LDS layout holds (the same for
 * every K); answers without a device.  Non-zero for K outside 1 .. kiwi_hip_linear_fit_max_basis() or a null pointer */
int kiwi_hip_spectral_candidates_bootstrap_shape(int K, int *candidates_per_workgroup, int *draws_per_tile, int *max_receivers);
/* the most basis sources per group of the wide fit (one lane of a wavefront per row of the solve): 64; answers without a device */
int kiwi_hip_linear_fit_wide_max_basis(void);
/* per (source, receiver, centroid) geometry record of the last eval, 20 floats/ints each
 * (layout in kiwi_amd/csrc/kiwi_kernels.hpp); for parity tests */
int kiwi_hip_get_geometry(kiwi_hip_ctx *ctx, int isrc, int irec, int maxcent, int *ncent, void *records);
/* receiver constants computed at set time: azimuth, back-azimuth [rad], distance [m]
 * (seismogram.f90:99-100), as output_distances prints them (minimizer.f90:1404-1440) */
int kiwi_hip_get_receiver_geometry(kiwi_hip_ctx *ctx, int irec, double *azi, double *bazi, double *dist);
/* device memory currently held [bytes] */
int kiwi_hip_get_device_bytes(kiwi_hip_ctx *ctx, long long *bytes);
/* the extra compiler flags the library was built with (`make EXTRA=...`; empty for the default build): profiles are matched to a
 * build by its kernel sources AND these */
int kiwi_hip_build_flags(char *buf, int buflen);
/* diagnostics: the rate [GB/s, 1e9 bytes] of a pure read of `bytes` bytes of device memory (16 bytes per lane, contiguous
 * slices; choose bytes >> 256 MiB Infinity Cache), `reps` passes timed with HIP events on the context's stream -- the ceiling
 * bench.py holds the accumulate kernels' HBM-regime figure against, measured in the same run */
int kiwi_hip_measure_read_bandwidth(kiwi_hip_ctx *ctx, long long bytes, int reps, double *gbs);

#ifdef __cplusplus
}
#endif
#endif
