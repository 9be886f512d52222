! kiwi_hip_binding.f90 -- iso_c_binding interface to the C-ABI in include/kiwi_hip.h.
!
! This is the Fortran side of the drop-in boundary: a host written in Fortran (the reference's
! minimizer_engine.f90, or this repo's kiwi_amd/fortran/minimizer_hip.f90) `use`s this module and
! replaces its calls to make_seismogram / receiver_scaled_seismograms_to_probes /
! receiver_calculate_misfits by kiwi_hip_* calls (see INTEGRATION.md).  Every function returns
! 0 on success; on failure kiwi_hip_error_message() gives the text for error() (util.f90:133-145).

module kiwi_hip_binding

    use iso_c_binding
    implicit none

    interface

        integer(c_int) function kiwi_hip_init( device, ctx ) bind(C, name='kiwi_hip_init')
            import :: c_int, c_ptr
            integer(c_int), value :: device
            type(c_ptr), intent(out) :: ctx
        end function

        ! one context over ndev_wanted devices of this process (<= 0: all): setters repeated on every device, the trial list of
        ! kiwi_hip_misfits_for_params sharded over them
        integer(c_int) function kiwi_hip_init_multi( ndev_wanted, ctx ) bind(C, name='kiwi_hip_init_multi')
            import :: c_int, c_ptr
            integer(c_int), value :: ndev_wanted
            type(c_ptr), intent(out) :: ctx
        end function

        integer(c_int) function kiwi_hip_ndevices( ctx, n ) bind(C, name='kiwi_hip_ndevices')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: n
        end function

        ! arithmetic contract of the accumulate kernels: 0 exact (default, bit-identical to the reference's rounding), 1 fused
        integer(c_int) function kiwi_hip_set_arithmetic( ctx, mode ) bind(C, name='kiwi_hip_set_arithmetic')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: mode
        end function

        integer(c_int) function kiwi_hip_get_arithmetic( ctx, mode ) bind(C, name='kiwi_hip_get_arithmetic')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: mode
        end function

        integer(c_int) function kiwi_hip_destroy( ctx ) bind(C, name='kiwi_hip_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
        end function

        integer(c_int) function kiwi_hip_last_error( ctx, buf, buflen ) bind(C, name='kiwi_hip_last_error')
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: ctx
            character(kind=c_char), intent(out) :: buf(*)
            integer(c_int), value :: buflen
        end function

        integer(c_int) function kiwi_hip_set_gfdb( ctx, nx, nz, ng, L, dt, dx, dz, firstx, firstz, G, first, nsamp ) &
                bind(C, name='kiwi_hip_set_gfdb')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: nx, nz, ng, L
            real(c_float), value :: dt, dx, dz, firstx, firstz
            real(c_float), intent(in) :: G(*)            ! (L, ng, nz, nx) in Fortran order
            integer(c_int), intent(in) :: first(*), nsamp(*)   ! (ng, nz, nx)
        end function

        integer(c_int) function kiwi_hip_set_gfdb_interpolated( ctx, nipx, nipz, nx, nz, ng, L, dt, dx, dz, firstx, firstz, &
                G, first, nsamp ) bind(C, name='kiwi_hip_set_gfdb_interpolated')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: nipx, nipz, nx, nz, ng, L
            real(c_float), value :: dt, dx, dz, firstx, firstz
            real(c_float), intent(in) :: G(*)            ! the stored database, as kiwi_hip_set_gfdb takes it
            integer(c_int), intent(in) :: first(*), nsamp(*)
        end function

        integer(c_int) function kiwi_hip_get_gfdb_shape( ctx, nx, nz, ng, maxlen, dx, dz ) bind(C, name='kiwi_hip_get_gfdb_shape')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: nx, nz, ng, maxlen
            real(c_float), intent(out) :: dx, dz
        end function

        integer(c_int) function kiwi_hip_get_gfdb_trace( ctx, ix, iz, ig, first, n, out, maxn ) &
                bind(C, name='kiwi_hip_get_gfdb_trace')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: ix, iz, ig, maxn     ! 0-based
            integer(c_int), intent(out) :: first, n
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_set_interp( ctx, bilinear, xus, zus ) bind(C, name='kiwi_hip_set_interp')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: bilinear, xus, zus
        end function

        integer(c_int) function kiwi_hip_set_effective_dt( ctx, edt ) bind(C, name='kiwi_hip_set_effective_dt')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), value :: edt
        end function

        integer(c_int) function kiwi_hip_set_source_location( ctx, lat, lon, reftime ) &
                bind(C, name='kiwi_hip_set_source_location')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            real(c_float), value :: lat, lon              ! degrees, as on the wire (minimizer.f90:511)
            real(c_double), value :: reftime
        end function

        integer(c_int) function kiwi_hip_set_receivers( ctx, nrec, lat, lon, depth, components ) &
                bind(C, name='kiwi_hip_set_receivers')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: nrec
            real(c_double), intent(in) :: lat(*), lon(*)  ! degrees, as in the receivers file
            real(c_float), intent(in) :: depth(*)
            type(c_ptr), intent(in) :: components(*)      ! nrec pointers to NUL-terminated strings
        end function

        integer(c_int) function kiwi_hip_switch_receiver( ctx, irec, enabled ) bind(C, name='kiwi_hip_switch_receiver')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, enabled
        end function

        integer(c_int) function kiwi_hip_set_reference( ctx, irec, icomp, first, n, data ) &
                bind(C, name='kiwi_hip_set_reference')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, icomp, first, n
            real(c_float), intent(in) :: data(*)
        end function

        integer(c_int) function kiwi_hip_set_taper( ctx, irec, npts, x, y ) bind(C, name='kiwi_hip_set_taper')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, npts
            real(c_float), intent(in) :: x(*), y(*)
        end function

        integer(c_int) function kiwi_hip_set_filter( ctx, irec, npts, x, y ) bind(C, name='kiwi_hip_set_filter')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, npts
            real(c_float), intent(in) :: x(*), y(*)
        end function

        integer(c_int) function kiwi_hip_set_misfit_method( ctx, method ) bind(C, name='kiwi_hip_set_misfit_method')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: method
        end function

        integer(c_int) function kiwi_hip_shift_ref_seismogram( ctx, irec, shift ) bind(C, name='kiwi_hip_shift_ref_seismogram')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec
            real(c_float), value :: shift
        end function

        integer(c_int) function kiwi_hip_autoshift_ref_seismogram( ctx, irec, min_shift, max_shift, isrc, shifts ) &
                bind(C, name='kiwi_hip_autoshift_ref_seismogram')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, isrc
            real(c_float), value :: min_shift, max_shift
            real(c_float), intent(out) :: shifts(*)
        end function

        integer(c_int) function kiwi_hip_set_floating_shiftrange( ctx, irec, min_shift, max_shift ) &
                bind(C, name='kiwi_hip_set_floating_shiftrange')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec
            real(c_float), value :: min_shift, max_shift
        end function

        integer(c_int) function kiwi_hip_get_floating_shifts( ctx, isrc0, nsrc, shifts ) &
                bind(C, name='kiwi_hip_get_floating_shifts')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc
            real(c_float), intent(out) :: shifts(*)
        end function

        integer(c_int) function kiwi_hip_set_synthetics_factor( ctx, factor ) &
                bind(C, name='kiwi_hip_set_synthetics_factor')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), value :: factor
        end function

        integer(c_int) function kiwi_hip_source_nparams( sourcetype ) bind(C, name='kiwi_hip_source_nparams')
            import :: c_int
            integer(c_int), value :: sourcetype
        end function

        integer(c_int) function kiwi_hip_discretize( sourcetype, params, nparams, effective_dt, cent, maxcent, &
                                                     ncent, moment, risetime ) bind(C, name='kiwi_hip_discretize')
            import :: c_int, c_float
            integer(c_int), value :: sourcetype, nparams, maxcent
            real(c_float), intent(in) :: params(*)
            real(c_float), value :: effective_dt
            real(c_float), intent(out) :: cent(10,*)
            integer(c_int), intent(out) :: ncent
            real(c_float), intent(out) :: moment, risetime
        end function

        ! crust profiles are 31 reals: vp(8) vs(8) rho(8) thickness(7)  (t_crust2x2_1d_profile, crust2x2.f90:45-50)
        integer(c_int) function kiwi_hip_set_source_crust( ctx, rupture_profile, origin_profile ) &
                bind(C, name='kiwi_hip_set_source_crust')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(in) :: rupture_profile(31), origin_profile(31)
        end function

        integer(c_int) function kiwi_hip_set_source_crustal_thickness_limit( ctx, limit ) &
                bind(C, name='kiwi_hip_set_source_crustal_thickness_limit')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), value :: limit
        end function

        integer(c_int) function kiwi_hip_get_source_crustal_thickness( ctx, thickness ) &
                bind(C, name='kiwi_hip_get_source_crustal_thickness')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: thickness
        end function

        integer(c_int) function kiwi_hip_set_source_constraints( ctx, n, points, normals ) &
                bind(C, name='kiwi_hip_set_source_constraints')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: n
            real(c_float), intent(in) :: points(3,*), normals(3,*)
        end function

        integer(c_int) function kiwi_hip_discretize_eikonal( sourcetype, params, nparams, effective_dt, rupture_profile, &
                                                             ncon, points, normals, cent, maxcent, ncent, moment, &
                                                             risetime ) bind(C, name='kiwi_hip_discretize_eikonal')
            import :: c_int, c_float
            integer(c_int), value :: sourcetype, nparams, ncon, maxcent
            real(c_float), intent(in) :: params(*), rupture_profile(31), points(3,*), normals(3,*)
            real(c_float), value :: effective_dt
            real(c_float), intent(out) :: cent(10,*)
            integer(c_int), intent(out) :: ncent
            real(c_float), intent(out) :: moment, risetime
        end function

        integer(c_int) function kiwi_hip_set_sources( ctx, nsrc, cent_ofs, cent, moment, risetime ) &
                bind(C, name='kiwi_hip_set_sources')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: nsrc
            integer(c_int), intent(in) :: cent_ofs(*)     ! (nsrc+1), 0-based row offsets
            real(c_float), intent(in) :: cent(10,*), moment(*), risetime(*)
        end function

        integer(c_int) function kiwi_hip_set_sources_params( ctx, sourcetype, nsrc, params ) &
                bind(C, name='kiwi_hip_set_sources_params')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, nsrc
            real(c_float), intent(in) :: params(*)        ! (nparams, nsrc)
        end function

        integer(c_int) function kiwi_hip_get_source_status( ctx, isrc0, nsrc, status ) &
                bind(C, name='kiwi_hip_get_source_status')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc          ! isrc0 is 0-based
            integer(c_int), intent(out) :: status(*)      ! 0 ok, 5 empty rupture area, 6 nucleation point outside
        end function

        integer(c_int) function kiwi_hip_source_status_message( code, buf, buflen ) &
                bind(C, name='kiwi_hip_source_status_message')
            import :: c_int, c_char
            integer(c_int), value :: code, buflen
            character(kind=c_char), intent(out) :: buf(*)
        end function

        integer(c_int) function kiwi_hip_misfits_for_params( ctx, sourcetype, nsrc, params, piece, misfit, norm, global, &
                status ) bind(C, name='kiwi_hip_misfits_for_params')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, nsrc, piece   ! piece <= 0: library default
            real(c_float), intent(in) :: params(*)             ! (nparams, nsrc)
            real(c_float), intent(out) :: misfit(*), norm(*)   ! (nmis, nsrc)
            real(c_float), intent(out) :: global(*)            ! (nsrc)
            integer(c_int), intent(out) :: status(*)           ! (nsrc)
        end function

        ! make_global_misfits under ndraw receiver weightings and the best source of each, on host arrays (kiwi_hip.h)
        integer(c_int) function kiwi_hip_outer_misfits( ctx, nsrc, nmis, nrec, slot_receiver, misfit, norm, outer_norm, &
                receiver_weights, anarchy, ndraw, draw_weights, best_value, best_index, which_draw, global_of_draw ) &
                bind(C, name='kiwi_hip_outer_misfits')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: nsrc, nmis, nrec, outer_norm, anarchy, ndraw, which_draw    ! receivers, sources, draws 0-based
            integer(c_int), intent(in) :: slot_receiver(*)
            real(c_float), intent(in) :: misfit(*), norm(*)
            type(c_ptr), value :: receiver_weights        ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(in) :: draw_weights(*)
            real(c_double), intent(out) :: best_value(*)
            integer(c_int), intent(out) :: best_index(*)
            type(c_ptr), value :: global_of_draw          ! c_loc of real(c_double) (nsrc), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_outer_max_receivers() bind(C, name='kiwi_hip_outer_max_receivers')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_get_outer_ms( ctx, ms ) bind(C, name='kiwi_hip_get_outer_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(3)
        end function

        ! least-squares coefficients of K basis sources per group under l2norm, groups of the uploaded batch (kiwi_hip.h)
        integer(c_int) function kiwi_hip_linear_fit( ctx, isrc0, ngroup, k, receiver_weight, anarchy, coef, misfit, status, &
                pivot_min, normal, normal_by_receiver ) bind(C, name='kiwi_hip_linear_fit')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, anarchy      ! isrc0 0-based
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(out) :: coef(*)        ! (k, ngroup)
            real(c_double), intent(out) :: misfit(*)      ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: pivot_min               ! c_loc of real(c_double) (ngroup), or c_null_ptr
            type(c_ptr), value :: normal                  ! c_loc of real(c_double) (nn, ngroup), nn = k (k + 1) / 2 + k + 1, or c_null_ptr
            type(c_ptr), value :: normal_by_receiver      ! c_loc of real(c_double) (nn, nrec, ngroup), or c_null_ptr
        end function

        ! the same for a parameter list of ngroup * k sources, discretised and uploaded piece by piece
        integer(c_int) function kiwi_hip_linear_fit_params( ctx, sourcetype, ngroup, k, params, piece, receiver_weight, anarchy, &
                coef, misfit, status, pivot_min, normal, normal_by_receiver ) bind(C, name='kiwi_hip_linear_fit_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, anarchy
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: coef(*), misfit(*)
            integer(c_int), intent(out) :: status(*)
            type(c_ptr), value :: pivot_min, normal, normal_by_receiver
        end function

        integer(c_int) function kiwi_hip_linear_fit_max_basis() bind(C, name='kiwi_hip_linear_fit_max_basis')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_ms( ctx, ms ) bind(C, name='kiwi_hip_get_linear_fit_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(3)
        end function

        ! the same under an l1 outer norm by iteratively reweighted least squares; the inner norm is the misfit method (kiwi_hip.h)
        integer(c_int) function kiwi_hip_linear_fit_robust( ctx, isrc0, ngroup, k, outer_norm, receiver_weight, anarchy, niter, eps, &
                coef, misfit, status, trace ) bind(C, name='kiwi_hip_linear_fit_robust')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, outer_norm, anarchy, niter      ! isrc0 0-based; outer_norm 1 l1norm, 2 l2norm
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), value :: eps
            real(c_double), intent(out) :: coef(*)        ! (k, ngroup)
            real(c_double), intent(out) :: misfit(*)      ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: trace                   ! c_loc of real(c_double) (2, niter + 1, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_linear_fit_robust_params( ctx, sourcetype, ngroup, k, params, piece, outer_norm, &
                receiver_weight, anarchy, niter, eps, coef, misfit, status, trace ) bind(C, name='kiwi_hip_linear_fit_robust_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, outer_norm, anarchy, niter
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            type(c_ptr), value :: receiver_weight
            real(c_double), value :: eps
            real(c_double), intent(out) :: coef(*), misfit(*)
            integer(c_int), intent(out) :: status(*)
            type(c_ptr), value :: trace
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_robust_ms( ctx, ms ) bind(C, name='kiwi_hip_get_linear_fit_robust_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)
        end function

        ! up to 64 basis sources per group, with a penalty and non-negative coefficients (kiwi_hip.h)
        integer(c_int) function kiwi_hip_linear_fit_wide( ctx, isrc0, ngroup, k, receiver_weight, anarchy, nonneg, penalty, &
                penalty_relative, coef, misfit, status, pivot_min, npositive, nsolves, normal, normal_by_receiver ) &
                bind(C, name='kiwi_hip_linear_fit_wide')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, anarchy, nonneg, penalty_relative      ! isrc0 0-based
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            type(c_ptr), value :: penalty                 ! c_loc of real(c_double) (k (k + 1) / 2), or c_null_ptr
            real(c_double), intent(out) :: coef(*)        ! (k, ngroup)
            real(c_double), intent(out) :: misfit(*)      ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: pivot_min               ! c_loc of real(c_double) (ngroup), or c_null_ptr
            type(c_ptr), value :: npositive, nsolves      ! c_loc of integer(c_int) (ngroup), or c_null_ptr
            type(c_ptr), value :: normal, normal_by_receiver
        end function

        integer(c_int) function kiwi_hip_linear_fit_wide_params( ctx, sourcetype, ngroup, k, params, piece, receiver_weight, anarchy, &
                nonneg, penalty, penalty_relative, coef, misfit, status, pivot_min, npositive, nsolves, normal, &
                normal_by_receiver ) bind(C, name='kiwi_hip_linear_fit_wide_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, anarchy, nonneg, penalty_relative
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            type(c_ptr), value :: receiver_weight, penalty
            real(c_double), intent(out) :: coef(*), misfit(*)
            integer(c_int), intent(out) :: status(*)
            type(c_ptr), value :: pivot_min, npositive, nsolves, normal, normal_by_receiver
        end function

        integer(c_int) function kiwi_hip_linear_fit_wide_max_basis() bind(C, name='kiwi_hip_linear_fit_wide_max_basis')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_wide_ms( ctx, ms ) bind(C, name='kiwi_hip_get_linear_fit_wide_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(2)                 ! Gram kernels, solve kernel
        end function

        ! misfits in several frequency bands and norms from one synthesis (kiwi_hip.h)
        integer(c_int) function kiwi_hip_misfit_bands_max() bind(C, name='kiwi_hip_misfit_bands_max')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_set_misfit_bands( ctx, nband, method, npts, x, y ) bind(C, name='kiwi_hip_set_misfit_bands')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: nband                      ! 0 removes the bands
            integer(c_int), intent(in) :: method(*), npts(*)    ! (nband): method ids 1 to 6; control points of the band's filter, 0 = none
            real(c_float), intent(in) :: x(*), y(*)             ! control points, band after band
        end function

        integer(c_int) function kiwi_hip_get_misfit_bands( ctx, nband ) bind(C, name='kiwi_hip_get_misfit_bands')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: nband
        end function

        integer(c_int) function kiwi_hip_band_misfits( ctx, isrc0, nsrc, misfit, norm, global ) bind(C, name='kiwi_hip_band_misfits')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc                ! isrc0 0-based
            type(c_ptr), value :: misfit, norm                  ! c_loc of real(c_float) (nmis, nband, nsrc), or c_null_ptr
            type(c_ptr), value :: global                        ! c_loc of real(c_float) (nband, nsrc), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_band_misfits_for_params( ctx, sourcetype, nsrc, params, piece, misfit, norm, global, status ) &
                bind(C, name='kiwi_hip_band_misfits_for_params')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, nsrc, piece
            real(c_float), intent(in) :: params(*)              ! (nparams, nsrc)
            type(c_ptr), value :: misfit, norm, global          ! as in kiwi_hip_band_misfits
            type(c_ptr), value :: status                        ! c_loc of integer(c_int) (nsrc), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_get_band_misfits_ms( ctx, ms ) bind(C, name='kiwi_hip_get_band_misfits_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(3)                 ! evaluation, band kernels, downloads
        end function

        ! misfits at many origin times from one synthesis (kiwi_hip.h): offsets k0 + j kstep, j = 0 .. nk - 1, in samples
        integer(c_int) function kiwi_hip_time_scan_max_shift() bind(C, name='kiwi_hip_time_scan_max_shift')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_time_scan_max_offsets() bind(C, name='kiwi_hip_time_scan_max_offsets')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_time_scan( ctx, isrc0, nsrc, k0, kstep, nk, misfit, norm, global, best ) &
                bind(C, name='kiwi_hip_time_scan')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc                ! isrc0 0-based
            integer(c_int), value :: k0, kstep, nk
            type(c_ptr), value :: misfit                        ! c_loc of real(c_float) (nmis, nk, nsrc), or c_null_ptr
            type(c_ptr), value :: norm                          ! c_loc of real(c_float) (nmis, nsrc), or c_null_ptr
            type(c_ptr), value :: global                        ! c_loc of real(c_float) (nk, nsrc), or c_null_ptr
            type(c_ptr), value :: best                          ! c_loc of integer(c_int) (nsrc): 0-based offset index, -1 for a failing; or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_time_scan_for_params( ctx, sourcetype, nsrc, params, piece, k0, kstep, nk, misfit, norm, global, &
                                                               best, status ) bind(C, name='kiwi_hip_time_scan_for_params')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, nsrc, piece
            real(c_float), intent(in) :: params(*)              ! (nparams, nsrc)
            integer(c_int), value :: k0, kstep, nk
            type(c_ptr), value :: misfit, norm, global, best    ! as in kiwi_hip_time_scan
            type(c_ptr), value :: status                        ! c_loc of integer(c_int) (nsrc), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_get_time_scan_ms( ctx, ms ) bind(C, name='kiwi_hip_get_time_scan_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(3)                 ! evaluation, scan kernels, downloads
        end function

        ! the linear fit at many origin times from one synthesis of the basis (kiwi_hip.h): groups as kiwi_hip_linear_fit, offsets as
        ! kiwi_hip_time_scan
        integer(c_int) function kiwi_hip_linear_fit_time_scan( ctx, isrc0, ngroup, k, k0, kstep, nk, receiver_weight, anarchy, coef, &
                misfit, status, pivot_min, best, normal ) bind(C, name='kiwi_hip_linear_fit_time_scan')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, anarchy      ! isrc0 0-based
            integer(c_int), value :: k0, kstep, nk
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(out) :: coef(*)        ! (k, nk, ngroup)
            real(c_double), intent(out) :: misfit(*)      ! (nk, ngroup)
            integer(c_int), intent(out) :: status(*)      ! (nk, ngroup)
            type(c_ptr), value :: pivot_min               ! c_loc of real(c_double) (nk, ngroup), or c_null_ptr
            type(c_ptr), value :: best                    ! c_loc of integer(c_int) (ngroup): 0-based offset index, -1 if none is solved; or c_null_ptr
            type(c_ptr), value :: normal                  ! c_loc of real(c_double) (nn, nk, ngroup), nn = k (k + 1) / 2 + k + 1, or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_linear_fit_time_scan_params( ctx, sourcetype, ngroup, k, params, piece, k0, kstep, nk, &
                receiver_weight, anarchy, coef, misfit, status, pivot_min, best, normal ) &
                bind(C, name='kiwi_hip_linear_fit_time_scan_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, anarchy
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            integer(c_int), value :: k0, kstep, nk
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: coef(*), misfit(*)
            integer(c_int), intent(out) :: status(*)
            type(c_ptr), value :: pivot_min, best, normal ! as in kiwi_hip_linear_fit_time_scan
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_time_scan_ms( ctx, ms ) bind(C, name='kiwi_hip_get_linear_fit_time_scan_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, Gram-scan kernel, solve kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_time_scan_shape( k, per_pass, tile ) bind(C, name='kiwi_hip_linear_fit_time_scan_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: per_pass, tile      ! offsets per workgroup, window samples per LDS tile
        end function

        ! the misfits of many given coefficient vectors per group from the kept normal equations: a mechanism grid from the six
        ! syntheses of the basis (kiwi_hip.h)
        integer(c_int) function kiwi_hip_linear_fit_candidates( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, receiver_weight, &
                anarchy, free_scale, best_index, best_misfit, status, misfit, scale, receiver_misfit, receiver_norm, fit_coef, &
                fit_misfit ) bind(C, name='kiwi_hip_linear_fit_candidates')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy, free_scale      ! isrc0 0-based; outer_norm 1 l1norm, 2 l2norm
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_index(*)  ! (ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: misfit, scale           ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: receiver_misfit         ! c_loc of real(c_float) (nrec, ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: receiver_norm           ! c_loc of real(c_float) (nrec, ngroup), or c_null_ptr
            type(c_ptr), value :: fit_coef, fit_misfit    ! c_loc of real(c_double) (k, ngroup) and (ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_params( ctx, sourcetype, ngroup, k, params, piece, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, free_scale, best_index, best_misfit, status, misfit, scale, receiver_misfit, &
                receiver_norm, fit_coef, fit_misfit ) bind(C, name='kiwi_hip_linear_fit_candidates_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy, free_scale
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_index(*), status(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: misfit, scale, receiver_misfit, receiver_norm, fit_coef, fit_misfit      ! as in kiwi_hip_linear_fit_candidates
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_candidates_ms( ctx, ms ) bind(C, name='kiwi_hip_get_linear_fit_candidates_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, Gram and solve kernels, candidate kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_shape( k, candidates_per_workgroup, receivers_per_stage ) &
                bind(C, name='kiwi_hip_linear_fit_candidates_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, receivers_per_stage
        end function

        ! the candidate evaluation at nk origin-time offsets k0 + j kstep from one synthesis of the basis sources
        integer(c_int) function kiwi_hip_linear_fit_candidates_time_scan( ctx, isrc0, ngroup, k, k0, kstep, nk, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, free_scale, best_offset, best_index, best_misfit, best_scale, status, &
                cand_misfit, cand_offset, cand_scale, misfit, scale, receiver_misfit, receiver_norm, fit_coef, fit_misfit, &
                fit_status ) bind(C, name='kiwi_hip_linear_fit_candidates_time_scan')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, k0, kstep, nk, ncand, outer_norm, anarchy, free_scale
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_offset(*) ! (ngroup): 0-based offset index, -1 if none
            integer(c_int), intent(out) :: best_index(*)  ! (nk, ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (nk, ngroup)
            type(c_ptr), value :: best_scale              ! c_loc of real(c_double) (nk, ngroup), or c_null_ptr; free_scale only
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: cand_misfit, cand_scale ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: cand_offset             ! c_loc of integer(c_int) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: misfit, scale           ! c_loc of real(c_double) (ncand, nk, ngroup), or c_null_ptr
            type(c_ptr), value :: receiver_misfit         ! c_loc of real(c_float) (nrec, ncand, nk, ngroup), or c_null_ptr
            type(c_ptr), value :: receiver_norm           ! c_loc of real(c_float) (nrec, ngroup), or c_null_ptr
            type(c_ptr), value :: fit_coef, fit_misfit    ! c_loc of real(c_double) (k, nk, ngroup) and (nk, ngroup), or c_null_ptr
            type(c_ptr), value :: fit_status              ! c_loc of integer(c_int) (nk, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_time_scan_params( ctx, sourcetype, ngroup, k, params, piece, k0, kstep, &
                nk, ncand, candidates, outer_norm, receiver_weight, anarchy, free_scale, best_offset, best_index, best_misfit, &
                best_scale, status, cand_misfit, cand_offset, cand_scale, misfit, scale, receiver_misfit, receiver_norm, fit_coef, &
                fit_misfit, fit_status ) bind(C, name='kiwi_hip_linear_fit_candidates_time_scan_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, k0, kstep, nk, ncand, outer_norm, anarchy, free_scale
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_offset(*), best_index(*), status(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: best_scale, cand_misfit, cand_offset, cand_scale, misfit, scale, receiver_misfit, receiver_norm, &
                                  fit_coef, fit_misfit, fit_status       ! as in kiwi_hip_linear_fit_candidates_time_scan
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_candidates_time_scan_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_linear_fit_candidates_time_scan_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(5)                 ! evaluation, Gram-scan kernel, solve kernels, candidate-scan kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_time_scan_shape( k, candidates_per_workgroup, receivers_per_stage ) &
                bind(C, name='kiwi_hip_linear_fit_candidates_time_scan_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, receivers_per_stage
        end function

        ! the bootstrap over the receivers of a candidate search, joint over group, origin-time offset and candidate, on the device
        integer(c_int) function kiwi_hip_linear_fit_candidates_bootstrap( ctx, isrc0, ngroup, k, k0, kstep, nk, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_offset, best_cand, status, &
                group_value, group_offset, group_cand ) bind(C, name='kiwi_hip_linear_fit_candidates_bootstrap')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, k0, kstep, nk, ncand, outer_norm, anarchy, ndraw      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(in) :: draw_weights(*) ! (nrec, ndraw)
            real(c_double), intent(out) :: best_value(*)  ! (ndraw); NaN where every source of the draw is excluded
            integer(c_int), intent(out) :: best_group(*), best_offset(*), best_cand(*)    ! (ndraw): 0-based, -1 if none
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: group_value             ! c_loc of real(c_double) (ndraw, ngroup), or c_null_ptr
            type(c_ptr), value :: group_offset, group_cand        ! c_loc of integer(c_int) (ndraw, ngroup); all three or none
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_bootstrap_params( ctx, sourcetype, ngroup, k, params, piece, k0, kstep, &
                nk, ncand, candidates, outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, &
                best_offset, best_cand, status, group_value, group_offset, group_cand ) &
                bind(C, name='kiwi_hip_linear_fit_candidates_bootstrap_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, k0, kstep, nk, ncand, outer_norm, anarchy, ndraw
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*), draw_weights(*)
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: best_value(*)
            integer(c_int), intent(out) :: best_group(*), best_offset(*), best_cand(*), status(*)
            type(c_ptr), value :: group_value, group_offset, group_cand       ! as in kiwi_hip_linear_fit_candidates_bootstrap
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_candidates_bootstrap_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_linear_fit_candidates_bootstrap_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(5)                 ! evaluation, Gram-scan kernel, solve kernels, bootstrap kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_bootstrap_shape( k, candidates_per_workgroup, draws_per_tile, &
                max_receivers ) bind(C, name='kiwi_hip_linear_fit_candidates_bootstrap_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, draws_per_tile, max_receivers
        end function

        ! the bootstrap over the receivers of a WAVEFORM candidate search (l1norm or l2norm inside), joint over group, origin-time
        ! offset and candidate, on the device
        integer(c_int) function kiwi_hip_waveform_candidates_bootstrap( ctx, isrc0, ngroup, k, k0, kstep, nk, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_offset, best_cand, status, &
                group_value, group_offset, group_cand ) bind(C, name='kiwi_hip_waveform_candidates_bootstrap')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, k0, kstep, nk, ncand, outer_norm, anarchy, ndraw      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(in) :: draw_weights(*) ! (nrec, ndraw)
            real(c_double), intent(out) :: best_value(*)  ! (ndraw); NaN where every source of the draw is excluded
            integer(c_int), intent(out) :: best_group(*), best_offset(*), best_cand(*)    ! (ndraw): 0-based, -1 if none
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: group_value             ! c_loc of real(c_double) (ndraw, ngroup), or c_null_ptr
            type(c_ptr), value :: group_offset, group_cand        ! c_loc of integer(c_int) (ndraw, ngroup); all three or none
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_bootstrap_params( ctx, sourcetype, ngroup, k, params, piece, k0, kstep, &
                nk, ncand, candidates, outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, &
                best_offset, best_cand, status, group_value, group_offset, group_cand ) &
                bind(C, name='kiwi_hip_waveform_candidates_bootstrap_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, k0, kstep, nk, ncand, outer_norm, anarchy, ndraw
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*), draw_weights(*)
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: best_value(*)
            integer(c_int), intent(out) :: best_group(*), best_offset(*), best_cand(*), status(*)
            type(c_ptr), value :: group_value, group_offset, group_cand       ! as in kiwi_hip_waveform_candidates_bootstrap
        end function

        integer(c_int) function kiwi_hip_get_waveform_candidates_bootstrap_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_waveform_candidates_bootstrap_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(5)                 ! evaluation, rows + scan kernels, fold kernels, bootstrap kernels, downloads
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_bootstrap_shape( k, candidates_per_workgroup, draws_per_tile, &
                max_receivers ) bind(C, name='kiwi_hip_waveform_candidates_bootstrap_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, draws_per_tile, max_receivers
        end function

        ! the bootstrap over the receivers of a SPECTRAL candidate search (ampspec_l2norm or ampspec_l1norm inside), joint over group
        ! and candidate, on the device
        integer(c_int) function kiwi_hip_spectral_candidates_bootstrap( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, &
                receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_cand, status, group_value, group_cand ) &
                bind(C, name='kiwi_hip_spectral_candidates_bootstrap')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy, ndraw      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(in) :: draw_weights(*) ! (nrec, ndraw)
            real(c_double), intent(out) :: best_value(*)  ! (ndraw); NaN where every source of the draw is excluded
            integer(c_int), intent(out) :: best_group(*), best_cand(*)    ! (ndraw): 0-based, -1 if none
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: group_value             ! c_loc of real(c_double) (ndraw, ngroup), or c_null_ptr
            type(c_ptr), value :: group_cand              ! c_loc of integer(c_int) (ndraw, ngroup); both or none
        end function

        integer(c_int) function kiwi_hip_spectral_candidates_bootstrap_params( ctx, sourcetype, ngroup, k, params, piece, ncand, &
                candidates, outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_cand, status, &
                group_value, group_cand ) bind(C, name='kiwi_hip_spectral_candidates_bootstrap_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy, ndraw
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*), draw_weights(*)
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: best_value(*)
            integer(c_int), intent(out) :: best_group(*), best_cand(*), status(*)
            type(c_ptr), value :: group_value, group_cand         ! as in kiwi_hip_spectral_candidates_bootstrap
        end function

        integer(c_int) function kiwi_hip_get_spectral_candidates_bootstrap_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_spectral_candidates_bootstrap_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(5)                 ! evaluation, spectra kernel, slot kernel, bootstrap kernels, downloads
        end function

        integer(c_int) function kiwi_hip_spectral_candidates_bootstrap_shape( k, candidates_per_workgroup, draws_per_tile, &
                max_receivers ) bind(C, name='kiwi_hip_spectral_candidates_bootstrap_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, draws_per_tile, max_receivers
        end function

        ! the candidate evaluation under floating_l2norm: per receiver and candidate the best whole-sample shift of the reference
        integer(c_int) function kiwi_hip_linear_fit_candidates_floating( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, &
                receiver_weight, anarchy, free_scale, best_index, best_misfit, status, best_shift, misfit, cand_shift, &
                receiver_misfit, receiver_norm ) bind(C, name='kiwi_hip_linear_fit_candidates_floating')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy, free_scale      ! isrc0 0-based; free_scale must be 0
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_index(*)  ! (ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            integer(c_int), intent(out) :: best_shift(*)  ! (nrec, ngroup): the winner's shifts in samples
            type(c_ptr), value :: misfit                  ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: cand_shift              ! c_loc of integer(c_short) (nrec, ncand, ngroup), or c_null_ptr; needs misfit
            type(c_ptr), value :: receiver_misfit         ! c_loc of real(c_float) (nrec, ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: receiver_norm           ! c_loc of real(c_float) (nrec, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_floating_params( ctx, sourcetype, ngroup, k, params, piece, ncand, &
                candidates, outer_norm, receiver_weight, anarchy, free_scale, best_index, best_misfit, status, best_shift, misfit, &
                cand_shift, receiver_misfit, receiver_norm ) bind(C, name='kiwi_hip_linear_fit_candidates_floating_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy, free_scale
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_index(*), status(*), best_shift(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: misfit, cand_shift, receiver_misfit, receiver_norm      ! as in kiwi_hip_linear_fit_candidates_floating
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_candidates_floating_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_linear_fit_candidates_floating_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, Gram and cross-correlation kernels, candidate kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_floating_shape( k, candidates_per_workgroup, shifts_per_pass, &
                shifts_per_stage ) bind(C, name='kiwi_hip_linear_fit_candidates_floating_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, shifts_per_pass, shifts_per_stage
        end function

        ! the bootstrap over the receivers of a candidate search under floating_l2norm, joint over group and candidate, on the device,
        ! with the shifts of every draw's winner
        integer(c_int) function kiwi_hip_linear_fit_candidates_floating_bootstrap( ctx, isrc0, ngroup, k, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_cand, best_shift, status, &
                group_value, group_cand, group_shift ) bind(C, name='kiwi_hip_linear_fit_candidates_floating_bootstrap')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy, ndraw      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            real(c_double), intent(in) :: draw_weights(*) ! (nrec, ndraw)
            real(c_double), intent(out) :: best_value(*)  ! (ndraw); NaN where every source of the draw is excluded
            integer(c_int), intent(out) :: best_group(*), best_cand(*)    ! (ndraw): 0-based, -1 if none
            integer(c_int), intent(out) :: best_shift(*)  ! (nrec, ndraw): the winner's shifts in samples
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: group_value             ! c_loc of real(c_double) (ndraw, ngroup), or c_null_ptr
            type(c_ptr), value :: group_cand              ! c_loc of integer(c_int) (ndraw, ngroup)
            type(c_ptr), value :: group_shift             ! c_loc of integer(c_int) (nrec, ndraw, ngroup); all three or none
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_floating_bootstrap_params( ctx, sourcetype, ngroup, k, params, piece, &
                ncand, candidates, outer_norm, receiver_weight, anarchy, ndraw, draw_weights, best_value, best_group, best_cand, &
                best_shift, status, group_value, group_cand, group_shift ) &
                bind(C, name='kiwi_hip_linear_fit_candidates_floating_bootstrap_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy, ndraw
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*), draw_weights(*)
            type(c_ptr), value :: receiver_weight
            real(c_double), intent(out) :: best_value(*)
            integer(c_int), intent(out) :: best_group(*), best_cand(*), best_shift(*), status(*)
            type(c_ptr), value :: group_value, group_cand, group_shift    ! as in kiwi_hip_linear_fit_candidates_floating_bootstrap
        end function

        integer(c_int) function kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, Gram + xcorr kernels, bootstrap kernels, downloads
        end function

        integer(c_int) function kiwi_hip_linear_fit_candidates_floating_bootstrap_shape( k, candidates_per_workgroup, draws_per_tile, &
                max_receivers ) bind(C, name='kiwi_hip_linear_fit_candidates_floating_bootstrap_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, draws_per_tile, max_receivers
        end function

        ! the candidate evaluation under the amplitude-spectrum norms from the spectra of the basis sources
        integer(c_int) function kiwi_hip_spectral_candidates( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, receiver_weight, &
                anarchy, free_scale, best_index, best_misfit, status, misfit, scale, slot_misfit, slot_norm, spectra_bins, spectra, &
                spectra_range, spectra_ref ) bind(C, name='kiwi_hip_spectral_candidates')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy, free_scale, spectra_bins      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_index(*)  ! (ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: misfit, scale           ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_misfit             ! c_loc of real(c_float) (nmis, ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_norm               ! c_loc of real(c_float) (nmis, ngroup), or c_null_ptr
            type(c_ptr), value :: spectra                 ! c_loc of real(c_float) (2, k, spectra_bins, nmis, ngroup), or c_null_ptr
            type(c_ptr), value :: spectra_range           ! c_loc of integer(c_int) (3, nmis, ngroup), or c_null_ptr
            type(c_ptr), value :: spectra_ref             ! c_loc of real(c_float) (2, spectra_bins, nmis, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_spectral_candidates_params( ctx, sourcetype, ngroup, k, params, piece, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, free_scale, best_index, best_misfit, status, misfit, scale, slot_misfit, &
                slot_norm, spectra_bins, spectra, spectra_range, spectra_ref ) bind(C, name='kiwi_hip_spectral_candidates_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy, free_scale, spectra_bins
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_index(*), status(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: misfit, scale, slot_misfit, slot_norm, spectra, spectra_range, spectra_ref      ! as in kiwi_hip_spectral_candidates
        end function

        integer(c_int) function kiwi_hip_get_spectral_candidates_ms( ctx, ms ) bind(C, name='kiwi_hip_get_spectral_candidates_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, spectra kernel, candidate kernels, downloads
        end function

        integer(c_int) function kiwi_hip_spectral_candidates_shape( ctx, k, candidates_per_workgroup, bins_per_stage, spectra_bins ) &
                bind(C, name='kiwi_hip_spectral_candidates_shape')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx                           ! c_null_ptr: answers without a device
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, bins_per_stage, spectra_bins
        end function

        ! the candidate evaluation under the time-domain l1norm / l2norm from the kept traces of the basis sources
        integer(c_int) function kiwi_hip_waveform_candidates( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, receiver_weight, &
                anarchy, best_index, best_misfit, status, misfit, slot_misfit, slot_norm ) bind(C, name='kiwi_hip_waveform_candidates')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_index(*)  ! (ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: misfit                  ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_misfit             ! c_loc of real(c_float) (nmis, ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_norm               ! c_loc of real(c_float) (nmis, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_params( ctx, sourcetype, ngroup, k, params, piece, ncand, candidates, &
                outer_norm, receiver_weight, anarchy, best_index, best_misfit, status, misfit, slot_misfit, slot_norm ) &
                bind(C, name='kiwi_hip_waveform_candidates_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_index(*), status(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: misfit, slot_misfit, slot_norm      ! as in kiwi_hip_waveform_candidates
        end function

        integer(c_int) function kiwi_hip_get_waveform_candidates_ms( ctx, ms ) bind(C, name='kiwi_hip_get_waveform_candidates_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, slot kernel, fold kernels, downloads
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_shape( k, candidates_per_workgroup, samples_per_stage ) &
                bind(C, name='kiwi_hip_waveform_candidates_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, samples_per_stage
        end function

        ! the candidate evaluation under floating_l1norm / floating_l2norm: kiwi_hip_waveform_candidates with per-receiver shifts
        integer(c_int) function kiwi_hip_waveform_candidates_floating( ctx, isrc0, ngroup, k, ncand, candidates, outer_norm, &
                receiver_weight, anarchy, best_index, best_misfit, status, best_shift, misfit, cand_shift, slot_misfit, slot_norm ) &
                bind(C, name='kiwi_hip_waveform_candidates_floating')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, ncand, outer_norm, anarchy      ! isrc0 0-based
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_index(*)  ! (ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            integer(c_int), intent(out) :: best_shift(*)  ! (nrec, ngroup): the winner's shifts in samples
            type(c_ptr), value :: misfit                  ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: cand_shift              ! c_loc of integer(c_short) (nrec, ncand, ngroup), or c_null_ptr; needs misfit
            type(c_ptr), value :: slot_misfit             ! c_loc of real(c_float) (nmis, ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_norm               ! c_loc of real(c_float) (nmis, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_floating_params( ctx, sourcetype, ngroup, k, params, piece, ncand, &
                candidates, outer_norm, receiver_weight, anarchy, best_index, best_misfit, status, best_shift, misfit, cand_shift, &
                slot_misfit, slot_norm ) bind(C, name='kiwi_hip_waveform_candidates_floating_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, ncand, outer_norm, anarchy
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_index(*), status(*), best_shift(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: misfit, cand_shift, slot_misfit, slot_norm      ! as in kiwi_hip_waveform_candidates_floating
        end function

        integer(c_int) function kiwi_hip_get_waveform_candidates_floating_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_waveform_candidates_floating_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, floating slot kernel, fold kernels, downloads
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_floating_shape( k, candidates_per_workgroup, samples_per_stage, &
                shifts_per_pass ) bind(C, name='kiwi_hip_waveform_candidates_floating_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, samples_per_stage, shifts_per_pass
        end function

        ! the candidate evaluation under l1norm / l2norm at many origin times: kiwi_hip_waveform_candidates x kiwi_hip_time_scan
        integer(c_int) function kiwi_hip_waveform_candidates_time_scan( ctx, isrc0, ngroup, k, k0, kstep, nk, ncand, &
                candidates, outer_norm, receiver_weight, anarchy, best_offset, best_index, best_misfit, status, cand_misfit, &
                cand_offset, misfit, slot_misfit, slot_norm, rows ) bind(C, name='kiwi_hip_waveform_candidates_time_scan')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, ngroup, k, k0, kstep, nk, ncand, outer_norm, anarchy      ! isrc0 0-based; k0 + j kstep
            real(c_double), intent(in) :: candidates(*)   ! (k, ncand)
            type(c_ptr), value :: receiver_weight         ! c_loc of real(c_double) (nrec), or c_null_ptr = ones
            integer(c_int), intent(out) :: best_offset(*) ! (ngroup): 0-based index of the best offset, -1 if none
            integer(c_int), intent(out) :: best_index(*)  ! (nk, ngroup): 0-based candidate, -1 if none
            real(c_double), intent(out) :: best_misfit(*) ! (nk, ngroup)
            integer(c_int), intent(out) :: status(*)      ! (ngroup)
            type(c_ptr), value :: cand_misfit             ! c_loc of real(c_double) (ncand, ngroup), or c_null_ptr
            type(c_ptr), value :: cand_offset             ! c_loc of integer(c_int) (ncand, ngroup), or c_null_ptr; with cand_misfit
            type(c_ptr), value :: misfit                  ! c_loc of real(c_double) (ncand, nk, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_misfit             ! c_loc of real(c_float) (nmis, ncand, nk, ngroup), or c_null_ptr
            type(c_ptr), value :: slot_norm               ! c_loc of real(c_float) (nmis, ngroup), or c_null_ptr
            type(c_ptr), value :: rows                    ! c_loc of real(c_float) (row_stride, k, ngroup), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_time_scan_params( ctx, sourcetype, ngroup, k, params, piece, k0, &
                kstep, nk, ncand, candidates, outer_norm, receiver_weight, anarchy, best_offset, best_index, best_misfit, status, &
                cand_misfit, cand_offset, misfit, slot_misfit, slot_norm, rows ) &
                bind(C, name='kiwi_hip_waveform_candidates_time_scan_params')
            import :: c_int, c_ptr, c_float, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype, ngroup, k, piece, k0, kstep, nk, ncand, outer_norm, anarchy
            real(c_float), intent(in) :: params(*)        ! (nparams, k, ngroup)
            real(c_double), intent(in) :: candidates(*)
            type(c_ptr), value :: receiver_weight
            integer(c_int), intent(out) :: best_offset(*), best_index(*), status(*)
            real(c_double), intent(out) :: best_misfit(*)
            type(c_ptr), value :: cand_misfit, cand_offset, misfit, slot_misfit, slot_norm, rows      ! as in the call above
        end function

        integer(c_int) function kiwi_hip_get_waveform_candidates_time_scan_ms( ctx, ms ) &
                bind(C, name='kiwi_hip_get_waveform_candidates_time_scan_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)                 ! evaluation, rows + scan kernel, fold kernels, downloads
        end function

        integer(c_int) function kiwi_hip_waveform_candidates_time_scan_shape( k, candidates_per_workgroup, samples_per_stage, &
                offsets_per_pass ) bind(C, name='kiwi_hip_waveform_candidates_time_scan_shape')
            import :: c_int
            integer(c_int), value :: k
            integer(c_int), intent(out) :: candidates_per_workgroup, samples_per_stage, offsets_per_pass
        end function

        ! the layout of `rows`: S = max |offset|, floats per basis source, where each misfit slot's wlen + 2 S samples begin
        integer(c_int) function kiwi_hip_waveform_candidates_time_scan_rows( ctx, k0, kstep, nk, shift_halo, row_stride, &
                row_offset ) bind(C, name='kiwi_hip_waveform_candidates_time_scan_rows')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: k0, kstep, nk
            integer(c_int), intent(out) :: shift_halo, row_stride
            type(c_ptr), value :: row_offset              ! c_loc of integer(c_int) (nmis), or c_null_ptr
        end function

        integer(c_int) function kiwi_hip_effective_cpus() bind(C, name='kiwi_hip_effective_cpus')
            import :: c_int
        end function

        integer(c_int) function kiwi_hip_eikonal_cache_stats( hits, misses, reset ) bind(C, name='kiwi_hip_eikonal_cache_stats')
            import :: c_int, c_long_long
            integer(c_long_long), intent(out) :: hits, misses
            integer(c_int), value :: reset
        end function

      ! eikonal_solver_fmm (eikonal.f90:29) on its own: speed, times are (nx,ny) arrays
        integer(c_int) function kiwi_hip_fast_marching( speed, nx, ny, origin, delta, start, discard, plain, times, &
                                                        fallbacks ) bind(C, name='kiwi_hip_fast_marching')
            import :: c_int, c_float, c_long_long
            real(c_float), intent(in) :: speed(*), origin(2), delta(2), start(2)
            integer(c_int), value :: nx, ny, plain
            real(c_float), value :: discard
            real(c_float), intent(out) :: times(*)
            integer(c_long_long), intent(out) :: fallbacks
        end function

      ! nsolve solves in one call: where = 0 the host's routine (ctx may be c_null_ptr), 1 the device of ctx
        integer(c_int) function kiwi_hip_fast_marching_batch( ctx, where, nsolve, nx, ny, ofs, speed, origin, delta, start, &
                                                              discard, times, fallbacks ) &
                                                              bind(C, name='kiwi_hip_fast_marching_batch')
            import :: c_int, c_ptr, c_float, c_long_long
            type(c_ptr), value :: ctx
            integer(c_int), value :: where, nsolve
            integer(c_int), intent(in) :: nx(*), ny(*)
            integer(c_long_long), intent(in) :: ofs(*)            ! 0-based offsets of the solves in speed and times
            real(c_float), intent(in) :: speed(*), origin(2,*), delta(2,*), start(2,*), discard(*)
            real(c_float), intent(out) :: times(*)
            integer(c_long_long), intent(out) :: fallbacks
        end function

      ! where the eikonal discretisers solve: 0 host (default), 1 device (env KIWI_HIP_EIK_DEVICE at kiwi_hip_init)
        integer(c_int) function kiwi_hip_set_eikonal_solver( ctx, where ) bind(C, name='kiwi_hip_set_eikonal_solver')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: where
        end function

        integer(c_int) function kiwi_hip_get_eikonal_solver( ctx, where ) bind(C, name='kiwi_hip_get_eikonal_solver')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: where
        end function

        integer(c_int) function kiwi_hip_get_eikonal_solver_ms( ctx, upload, kernel, download ) &
                                                                bind(C, name='kiwi_hip_get_eikonal_solver_ms')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            real(c_double), intent(out) :: upload, kernel, download
        end function

        integer(c_int) function kiwi_hip_get_eikonal_solver_stats( ctx, launches, heap_high_water ) &
                                                                   bind(C, name='kiwi_hip_get_eikonal_solver_stats')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: launches, heap_high_water
        end function

        integer(c_int) function kiwi_hip_fast_marching_grid_ok( nx, ny ) bind(C, name='kiwi_hip_fast_marching_grid_ok')
            import :: c_int, c_long_long
            integer(c_long_long), value :: nx, ny
        end function

        integer(c_int) function kiwi_hip_eval( ctx, isrc0, nsrc ) bind(C, name='kiwi_hip_eval')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc          ! isrc0 is 0-based
        end function

        integer(c_int) function kiwi_hip_sync( ctx ) bind(C, name='kiwi_hip_sync')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
        end function

        integer(c_int) function kiwi_hip_nmisfits( ctx, nmis ) bind(C, name='kiwi_hip_nmisfits')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), intent(out) :: nmis
        end function

        ! device pointer of the global misfits of a source range (for a device-to-device all-gather)
        integer(c_int) function kiwi_hip_get_global_misfits_device( ctx, isrc0, nsrc, device_ptr ) bind(C, name='kiwi_hip_get_global_misfits_device')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc
            type(c_ptr), intent(out) :: device_ptr
        end function

        integer(c_int) function kiwi_hip_get_misfits( ctx, isrc0, nsrc, misfit, norm, global ) &
                bind(C, name='kiwi_hip_get_misfits')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc0, nsrc
            real(c_float), intent(out) :: misfit(*), norm(*), global(*)   ! (nmis,nsrc), (nmis,nsrc), (nsrc)
        end function

        integer(c_int) function kiwi_hip_set_keep_synthetics( ctx, which ) bind(C, name='kiwi_hip_set_keep_synthetics')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: which
        end function

        integer(c_int) function kiwi_hip_get_synthetics( ctx, isrc, irec, icomp, which, first, n, out, maxn ) &
                bind(C, name='kiwi_hip_get_synthetics')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, irec, icomp, which, maxn
            integer(c_int), intent(out) :: first, n
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_get_kernel_ms( ctx, ms, launches ) bind(C, name='kiwi_hip_get_kernel_ms')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            real(c_float), intent(out) :: ms(4)
            integer(c_int), intent(out) :: launches(3)
        end function

        integer(c_int) function kiwi_hip_get_geometry( ctx, isrc, irec, maxcent, ncent, records ) &
                bind(C, name='kiwi_hip_get_geometry')
            import :: c_int, c_ptr
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, irec, maxcent
            integer(c_int), intent(out) :: ncent
            type(c_ptr), value :: records                    ! maxcent records of 80 bytes (kiwi_kernels.hpp, GeoRec)
        end function

      ! fcn: a bind(C) function  integer(c_int) f( user, k, m, n, xs, fv )  with value arguments user (c_ptr), k, m, n and
      ! arrays xs(n,k), fv(m,k); pass c_funloc(f)
        integer(c_int) function kiwi_hip_lmdif( fcn, user, m, n, x, fvec, ftol, xtol, gtol, maxfev, epsfcn, diag, mode, factor, &
                                                info, nfev ) bind(C, name='kiwi_hip_lmdif')
            import :: c_int, c_ptr, c_funptr, c_float
            type(c_funptr), value :: fcn
            type(c_ptr), value :: user
            integer(c_int), value :: m, n, maxfev, mode
            real(c_float), value :: ftol, xtol, gtol, epsfcn, factor
            real(c_float), intent(inout) :: x(*), fvec(*), diag(*)
            integer(c_int), intent(out) :: info, nfev
        end function

        integer(c_int) function kiwi_hip_get_amp_spectrum( ctx, isrc, irec, icomp, which_probe, filtered, df, n, out, maxn ) &
                bind(C, name='kiwi_hip_get_amp_spectrum')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, irec, icomp, which_probe, filtered, maxn
            real(c_float), intent(out) :: df
            integer(c_int), intent(out) :: n
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_principal_axes( sourcetype, params, pax, tax ) bind(C, name='kiwi_hip_principal_axes')
            import :: c_int, c_float
            integer(c_int), value :: sourcetype
            real(c_float), intent(in) :: params(*)
            real(c_float), intent(out) :: pax(2), tax(2)
        end function

        integer(c_int) function kiwi_hip_get_cross_correlations( ctx, isrc, irec, min_shift, max_shift, first_shift, nshift, &
                                                                  cc, maxn ) bind(C, name='kiwi_hip_get_cross_correlations')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, irec, maxn
            real(c_float), value :: min_shift, max_shift
            integer(c_int), intent(out) :: first_shift, nshift
            real(c_float), intent(out) :: cc(*)
        end function

        integer(c_int) function kiwi_hip_get_peak_amplitudes( ctx, isrc, differentiate, out ) &
                bind(C, name='kiwi_hip_get_peak_amplitudes')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, differentiate
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_get_arias_intensities( ctx, isrc, out ) bind(C, name='kiwi_hip_get_arias_intensities')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_minimize_lm( ctx, sourcetype, params, mask, mins, maxs, info, iterations, misfit, best ) &
                bind(C, name='kiwi_hip_minimize_lm')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: sourcetype
            real(c_float), intent(inout) :: params(*)
            integer(c_int), intent(in) :: mask(*)
            type(c_ptr), value :: mins, maxs                 ! real(c_float) arrays or c_null_ptr
            integer(c_int), intent(out) :: info, iterations
            real(c_float), intent(out) :: misfit
            real(c_float), intent(out) :: best(*)
        end function

        integer(c_int) function kiwi_hip_get_source_centroids( ctx, isrc, maxcent, ncent, cent ) &
                bind(C, name='kiwi_hip_get_source_centroids')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: isrc, maxcent
            integer(c_int), intent(out) :: ncent
            real(c_float), intent(out) :: cent(10,*)
        end function

        integer(c_int) function kiwi_hip_get_device_bytes( ctx, bytes ) bind(C, name='kiwi_hip_get_device_bytes')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: ctx
            integer(c_long_long), intent(out) :: bytes
        end function

        integer(c_int) function kiwi_hip_build_flags( buf, buflen ) bind(C, name='kiwi_hip_build_flags')
            import :: c_int, c_char
            character(kind=c_char), intent(out) :: buf(*)
            integer(c_int), value :: buflen
        end function

      ! diagnostics: GB/s of a pure read of `bytes` bytes of device memory
        integer(c_int) function kiwi_hip_measure_read_bandwidth( ctx, bytes, reps, gbs ) &
                bind(C, name='kiwi_hip_measure_read_bandwidth')
            import :: c_int, c_ptr, c_long_long, c_double
            type(c_ptr), value :: ctx
            integer(c_long_long), value :: bytes
            integer(c_int), value :: reps
            real(c_double), intent(out) :: gbs
        end function

        integer(c_int) function kiwi_hip_get_reference( ctx, irec, icomp, which, first, n, out, maxn ) &
                bind(C, name='kiwi_hip_get_reference')
            import :: c_int, c_ptr, c_float
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec, icomp, which, maxn
            integer(c_int), intent(out) :: first, n
            real(c_float), intent(out) :: out(*)
        end function

        integer(c_int) function kiwi_hip_get_receiver_geometry( ctx, irec, azi, bazi, dist ) &
                bind(C, name='kiwi_hip_get_receiver_geometry')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: ctx
            integer(c_int), value :: irec
            real(c_double), intent(out) :: azi, bazi, dist
        end function

    end interface

  contains

  ! the library's last error as a Fortran string, for error() / "<cmd>: nok >" answers
    function kiwi_hip_error_message( ctx ) result( msg )
        type(c_ptr), intent(in) :: ctx
        character(len=:), allocatable :: msg
        character(kind=c_char) :: buf(1024)
        integer :: i, n, rc
        rc = kiwi_hip_last_error( ctx, buf, 1024_c_int )
        n = 0
        do i = 1, 1024
            if (buf(i) == c_null_char) exit
            n = i
        end do
        allocate( character(len=n) :: msg )
        do i = 1, n
            msg(i:i) = buf(i)
        end do
    end function

end module
