! binding_smoke.f90 -- proves that a Fortran host reaches the C-ABI through iso_c_binding:
! discretises the reference's own unit-test source (test_source_bilat.f90:47-60) through
! kiwi_hip_discretize (host-side, needs no GPU) and prints the result for tests/test_fortran_binding.py.
! With a GPU present it also opens and closes a device context.
program binding_smoke

    use iso_c_binding
    use kiwi_hip_binding
    implicit none

    real(c_float) :: params(14), cent(10,4096), moment, risetime, msum
    integer(c_int) :: ncent, rc, per_pass, tile, per_group, per_stage
    type(c_ptr) :: ctx
    integer :: i

    params = (/ 0., 0., 0., 1000., 1., 90., 45., 90., 0., 2000., 0., 1000., 2000., 1. /)
    if (kiwi_hip_source_nparams( 1_c_int ) /= 14) stop 2
    rc = kiwi_hip_discretize( 1_c_int, params, 14_c_int, 0.5_c_float, cent, 4096_c_int, ncent, moment, risetime )
    if (rc /= 0) stop 3
    msum = 0.
    do i = 1, ncent
        msum = msum + cent(5,i)
    end do
    print '(a,i6,a,f10.6,a,f8.3)', 'ncent ', ncent, ' sum_mxx ', msum, ' moment ', moment

    ! the limits of kiwi_hip_time_scan answer without a device
    if (kiwi_hip_time_scan_max_shift() /= 1024 .or. kiwi_hip_time_scan_max_offsets() /= 256) stop 4

    ! so does the shape of the linear fit's time scan: offsets per pass and samples per tile for six basis sources
    if (kiwi_hip_linear_fit_time_scan_shape( 6_c_int, per_pass, tile ) /= 0) stop 5
    if (per_pass < 1 .or. tile < 256 .or. mod(tile, 256) /= 0) stop 6

    ! and the shape of the candidate kernel: candidates per workgroup and receivers per LDS stage
    if (kiwi_hip_linear_fit_candidates_shape( 6_c_int, per_group, per_stage ) /= 0) stop 7
    if (per_group < 64 .or. per_stage < 1) stop 8

    ! the candidate-scan kernel of the time scan has a shape of its own
    if (kiwi_hip_linear_fit_candidates_time_scan_shape( 6_c_int, per_group, per_stage ) /= 0) stop 9
    if (per_group < 64 .or. per_stage < 1) stop 10

    ! and the kernels of the candidate evaluation with per-receiver shifts: shifts per pass and per LDS stage as well
    if (kiwi_hip_linear_fit_candidates_floating_shape( 6_c_int, per_group, per_pass, per_stage ) /= 0) stop 11
    if (per_group < 64 .or. per_pass < 1 .or. per_stage < 1) stop 12

    ! the candidate kernel of the amplitude-spectrum norms: candidates per workgroup and bins of spectra per LDS stage
    if (kiwi_hip_spectral_candidates_shape( c_null_ptr, 6_c_int, per_group, per_stage, per_pass ) /= 0) stop 13
    if (per_group < 64 .or. per_stage < 1 .or. per_pass /= 0) stop 14

    ! the candidate kernels of the time-domain norms: candidates per workgroup and samples per LDS stage
    if (kiwi_hip_waveform_candidates_shape( 6_c_int, per_group, per_stage ) /= 0) stop 23
    if (per_group < 64 .or. per_stage < 1) stop 24

    ! and of the floating time-domain norms: the shifts a lane holds accumulators for at once as well
    if (kiwi_hip_waveform_candidates_floating_shape( 6_c_int, per_group, per_stage, per_pass ) /= 0) stop 25
    if (per_group < 64 .or. per_stage < 1 .or. per_pass < 1) stop 26

    ! and of their scan over origin times: the offsets a lane holds accumulators for at once
    if (kiwi_hip_waveform_candidates_time_scan_shape( 6_c_int, per_group, per_stage, per_pass ) /= 0) stop 27
    if (per_group < 64 .or. per_stage < 1 .or. per_pass < 8) stop 28

    ! the joint bootstrap of a candidate search: candidates per workgroup, draws per tile, the most receivers its LDS holds
    if (kiwi_hip_linear_fit_candidates_bootstrap_shape( 6_c_int, per_group, per_pass, per_stage ) /= 0) stop 15
    if (per_group < 64 .or. per_pass < 1 .or. per_stage < 64) stop 16

    ! and of a waveform candidate search: a candidate's fp64 column per receiver stays in LDS
    if (kiwi_hip_waveform_candidates_bootstrap_shape( 6_c_int, per_group, per_pass, per_stage ) /= 0) stop 29
    if (per_group < 64 .or. per_pass < 1 .or. per_stage < 64) stop 30

    ! and of a candidate search under the amplitude-spectrum norms: the same bootstrap kernel behind a kernel per slot
    if (kiwi_hip_spectral_candidates_bootstrap_shape( 6_c_int, per_group, per_pass, per_stage ) /= 0) stop 31
    if (per_group < 64 .or. per_pass < 1 .or. per_stage < 64) stop 32

    ! and of a candidate search with per-receiver shifts: a candidate's float column per receiver stays in LDS
    if (kiwi_hip_linear_fit_candidates_floating_bootstrap_shape( 6_c_int, per_group, per_pass, per_stage ) /= 0) stop 33
    if (per_group < 64 .or. per_pass < 1 .or. per_stage < 64) stop 34

    rc = kiwi_hip_init( 0_c_int, ctx )
    if (rc == 0) then
        print '(a)', 'device context ok'
        rc = kiwi_hip_destroy( ctx )
    else
        print '(a,a)', 'no device: ', kiwi_hip_error_message( c_null_ptr )
    end if

end program
