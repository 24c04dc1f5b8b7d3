!=======================================================================
! evpk_mod -- ISO_C_BINDING view of libevpk (include/evpk.h): the C ABI of the
! MI355X EVP solver, as a Fortran host model binds it.
!
! The derived types mirror the C structs field for field (bind(C)); all array
! arguments are passed as c_loc of the caller's own block arrays
! real(dbl_kind) a(nx_block,ny_block,max_blocks) -- the library borrows them
! for the duration of a call only.  Fortran LOGICAL arrays are not interoperable:
! the caller converts tmask/umask/iceumask to integer(c_int32_t) 0/1.
!=======================================================================
      module evpk_mod

      use, intrinsic :: iso_c_binding
      implicit none
      private

      integer (c_int), parameter, public :: &
         EVPK_BND_CYCLIC = 0, EVPK_BND_OPEN = 1, EVPK_BND_CLOSED = 2, EVPK_BND_TRIPOLE = 3
      integer, parameter, public :: EVPK_UNIQUE_ID_BYTES = 128

      type, bind(C), public :: evpk_geom
         integer (c_int32_t) :: nx_global, ny_global
         integer (c_int32_t) :: nx_block, ny_block, nblocks
         integer (c_int32_t) :: ew_boundary, ns_boundary
         type (c_ptr) :: ilo, ihi, jlo, jhi
         type (c_ptr) :: iglob_lo, jglob_lo
         integer (c_int32_t) :: rank, nranks
         integer (c_int32_t) :: device
         type (c_ptr) :: unique_id
         type (c_ptr) :: dxt, dyt, dxhy, dyhx, cxp, cyp, cxm, cym
         type (c_ptr) :: tarear, uarear, tinyarea, tarea, uarea, fcor
         type (c_ptr) :: tmask, umask
         type (c_ptr) :: HTN, HTE            ! optional (c_null_ptr): see include/evpk.h
      end type evpk_geom

      type, bind(C), public :: evpk_params
         real (c_double) :: dt
         integer (c_int32_t) :: ndte
         integer (c_int32_t) :: revised_evp
         real (c_double) :: revp, ecci, denom1, arlx1i, brlx
         real (c_double) :: cosw, sinw
         real (c_double) :: rhow, rhoi, rhos, gravit
         real (c_double) :: a_min, m_min
         integer (c_int32_t) :: tilt_from_slope
         integer (c_int32_t) :: wind_on_ugrid
         integer (c_int32_t) :: kstrength, krdg_partic, krdg_redist, ncat    ! ice_strength on the device (strength = c_null_ptr)
         real (c_double) :: mu_rdg, Cf
         integer (c_int32_t) :: sparse_io = 0     ! 1: sparse transfers in resident-state mode (include/evpk.h)
         integer (c_int32_t) :: reserved_ = 0
      end type evpk_params

      type, bind(C), public :: evpk_step_in
         type (c_ptr) :: aice, vice, vsno, aice_init
         type (c_ptr) :: strairxT, strairyT, strax, stray
         type (c_ptr) :: uocn, vocn, ss_tltx, ss_tlty, Cdn_ocn
         type (c_ptr) :: strength            ! c_null_ptr: the library evaluates ice_strength itself, from ...
         type (c_ptr) :: aicen, vicen, aice0 ! ... the thickness distribution (kstrength = 1)
      end type evpk_step_in

      type, bind(C), public :: evpk_state
         type (c_ptr) :: uvel, vvel
         type (c_ptr) :: stressp(4), stressm(4), stress12(4)
         type (c_ptr) :: iceumask
         type (c_ptr) :: divu, shear, rdg_conv, rdg_shear, prs_sig
         type (c_ptr) :: strintx, strinty, strocnx, strocny, strocnxT, strocnyT
         type (c_ptr) :: strairx, strairy, strtltx, strtlty, fm
         type (c_ptr) :: tmass
         type (c_ptr) :: aiu, umass, uvel_init, vvel_init
         type (c_ptr) :: icetmask
         type (c_ptr) :: strength            ! out: the strength the library computed
      end type evpk_state

      type, bind(C), public :: evpk_stats
         integer (c_int64_t) :: icellt, icellu, ncell_slab
         integer (c_int32_t) :: nstrips, nstrips_total, subcycles_done
         real (c_float) :: loop_ms, kernel_ms
         integer (c_int32_t) :: kernel_launches
         real (c_float) :: kernel2_ms
         integer (c_int32_t) :: kernel2_launches
         integer (c_int32_t) :: strip_rows, strip_rows2, nstrips2
         integer (c_int32_t) :: zone_cols, zone_exchanges
         integer (c_int64_t) :: zone_bytes
         integer (c_int32_t) :: overlap_split, tile_kernel, kernel_timed, kernel2_timed
         real (c_float) :: bound_ms
         integer (c_int32_t) :: bound_updates, compact_metrics, transport, band_row_exchanges
         real (c_float) :: kernel3_ms
         integer (c_int32_t) :: kernel3_launches, kernel3_timed, strip_rows3, nstrips3
         integer (c_int32_t) :: rccl_ranks, device, device_pci
         integer (c_int64_t) :: delivery_checked, delivery_bad
         integer (c_int32_t) :: bound_state_rounds, bound_state_planes
      end type evpk_stats

      ! evpk_eap_state (include/evpk.h): the structure tensor at the four corners, its cell means, the EAP history fields
      type, bind(C) :: evpk_eap_state
         type (c_ptr) :: a11_c(4) = c_null_ptr, a12_c(4) = c_null_ptr
         type (c_ptr) :: a11 = c_null_ptr, a12 = c_null_ptr
         type (c_ptr) :: e11 = c_null_ptr, e12 = c_null_ptr, e22 = c_null_ptr
         type (c_ptr) :: yieldstress11 = c_null_ptr, yieldstress12 = c_null_ptr, yieldstress22 = c_null_ptr
         type (c_ptr) :: s11 = c_null_ptr, s12 = c_null_ptr, s22 = c_null_ptr
      end type evpk_eap_state

      ! evpk_ridge_tracers, evpk_ridge_diag (include/evpk.h): the ice_state tracer indices ridge_shift reads (1-based, 0 = not in
      ! use) and the optional history / flux arrays of ridge_ice (ice_mechred.F90:164-189)
      type, bind(C) :: evpk_ridge_tracers
         integer (c_int32_t) :: nt_qsno = 0, nslyr = 0, nt_alvl = 0, nt_vlvl = 0, nt_apnd = 0, nt_hpnd = 0, nt_fbri = 0
         integer (c_int32_t) :: tr_pond_cesm = 0, tr_pond_lvl = 0, tr_pond_topo = 0
      end type evpk_ridge_tracers
      type, bind(C) :: evpk_ridge_diag
         type (c_ptr) :: dardg1dt = c_null_ptr, dardg2dt = c_null_ptr, dvirdgdt = c_null_ptr, opening = c_null_ptr
         type (c_ptr) :: fpond = c_null_ptr, fresh = c_null_ptr, fhocn = c_null_ptr
         type (c_ptr) :: dardg1ndt = c_null_ptr, dardg2ndt = c_null_ptr, dvirdgndt = c_null_ptr, aparticn = c_null_ptr
         type (c_ptr) :: krdgn = c_null_ptr, araftn = c_null_ptr, vraftn = c_null_ptr, aredistn = c_null_ptr, vredistn = c_null_ptr
      end type evpk_ridge_diag

      ! evpk_itd_tracers, evpk_itd_constants (include/evpk.h): the ice_state tracer indices cleanup_itd / aggregate read (1-based, 0 = not
      ! in use) and the constants of ice_constants / ice_therm_shared that zap_small_areas and zap_snow_temperature read
      type, bind(C) :: evpk_itd_tracers
         integer (c_int32_t) :: nt_Tsfc = 0, nt_qice = 0, nilyr = 0, nt_qsno = 0, nslyr = 0, nt_alvl = 0, nt_apnd = 0, nt_hpnd = 0, nt_fbri = 0
         integer (c_int32_t) :: tr_pond_cesm = 0, tr_pond_lvl = 0, tr_pond_topo = 0, tr_brine = 0
      end type evpk_itd_tracers
      type, bind(C) :: evpk_itd_constants
         real (c_double) :: Tocnfrz, ice_ref_salinity, hs_min, cp_ice, Lfresh, Tmin, puny
      end type evpk_itd_constants

      ! evpk_dyn_args (include/evpk.h): the arguments of evpk_step_dynamics, one struct of borrowed pointers, member for member
      type, bind(C) :: evpk_dyn_args
         integer (c_int32_t) :: advection = 0           ! 0 none, 1 transport_upwind, 2 transport_remap
         integer (c_int32_t) :: ridge = 1
         real (c_double) :: dt
         integer (c_int32_t) :: ndtd = 1
         integer (c_int32_t) :: ncat, ntrcr, ntrcr_dim
         type (c_ptr) :: trcr_depend = c_null_ptr
         type (evpk_itd_tracers) :: t
         integer (c_int32_t) :: nt_vlvl = 0, nt_iage = 0
         type (c_ptr) :: hin_max = c_null_ptr
         type (evpk_itd_constants) :: k
         integer (c_int32_t) :: tr_aero = 0, nbtrcr = 0, heat_capacity = 1
         type (c_ptr) :: tracer_type = c_null_ptr, depend = c_null_ptr, has_dependents = c_null_ptr
         integer (c_int32_t) :: integral_order = 3, l_dp_midpt = 1
         real (c_double) :: rhos_lfresh
         type (c_ptr) :: aice0 = c_null_ptr, aicen = c_null_ptr, vicen = c_null_ptr, vsnon = c_null_ptr, trcrn = c_null_ptr
         type (c_ptr) :: aice = c_null_ptr, vice = c_null_ptr, vsno = c_null_ptr, trcr = c_null_ptr
         type (c_ptr) :: daidtd = c_null_ptr, dvidtd = c_null_ptr, dagedtd = c_null_ptr
         type (c_ptr) :: fpond = c_null_ptr, fresh = c_null_ptr, fsalt = c_null_ptr, fhocn = c_null_ptr, first_ice = c_null_ptr
         type (c_ptr) :: rdg_conv = c_null_ptr, rdg_shear = c_null_ptr
         type (c_ptr) :: diag = c_null_ptr              ! c_loc of an evpk_ridge_diag, or c_null_ptr
      end type evpk_dyn_args

      ! evpk_therm2_args (include/evpk.h): the arguments of evpk_step_therm2 and evpk_new_ice_lateral_melt, member for member
      type, bind(C) :: evpk_therm2_args
         integer (c_int32_t) :: kitd = 1, ktherm = 1, update_ocn_f = 0
         real (c_double) :: dt, yday, hi_min, hfrazilmin, phi_init, dSin0_frazil, cp_ocn
         integer (c_int32_t) :: ncat, ntrcr, ntrcr_dim
         type (c_ptr) :: trcr_depend = c_null_ptr
         type (evpk_itd_tracers) :: t
         integer (c_int32_t) :: nt_sice = 0, nt_iage = 0, nt_FY = 0, nt_vlvl = 0
         type (c_ptr) :: hin_max = c_null_ptr
         type (evpk_itd_constants) :: k
         integer (c_int32_t) :: tr_aero = 0, nbtrcr = 0, heat_capacity = 1, skl_bgc = 0
         type (c_ptr) :: aicen_init = c_null_ptr, vicen_init = c_null_ptr
         type (c_ptr) :: aicen = c_null_ptr, vicen = c_null_ptr, vsnon = c_null_ptr, trcrn = c_null_ptr, aice = c_null_ptr, aice0 = c_null_ptr
         type (c_ptr) :: frain = c_null_ptr, frzmlt = c_null_ptr, Tf = c_null_ptr, sss = c_null_ptr, rside = c_null_ptr, salinz = c_null_ptr
         type (c_ptr) :: frazil = c_null_ptr, frz_onset = c_null_ptr, meltl = c_null_ptr, fpond = c_null_ptr, fresh = c_null_ptr
         type (c_ptr) :: fsalt = c_null_ptr, fhocn = c_null_ptr, first_ice = c_null_ptr
      end type evpk_therm2_args

      ! evpk_thermo_args (include/evpk.h): the arguments of evpk_thermo_vertical, member for member
      type, bind(C) :: evpk_thermo_args
         real (c_double) :: dt, yday
         integer (c_int32_t) :: ktherm = 1, calc_Tsfc = 1, heat_capacity = 1, l_brine = 1, conduct = 0
         real (c_double) :: min_salin
         integer (c_int32_t) :: ncat, ntrcr, ntrcr_dim
         type (evpk_itd_tracers) :: t
         integer (c_int32_t) :: nt_sice = 0
         type (evpk_itd_constants) :: k
         type (c_ptr) :: aicen = c_null_ptr, vicen = c_null_ptr, vsnon = c_null_ptr, trcrn = c_null_ptr
         type (c_ptr) :: flw = c_null_ptr, potT = c_null_ptr, Qa = c_null_ptr, rhoa = c_null_ptr, fsnow = c_null_ptr, fbot = c_null_ptr
         type (c_ptr) :: Tbot = c_null_ptr, sss = c_null_ptr
         type (c_ptr) :: shcoef = c_null_ptr, lhcoef = c_null_ptr
         type (c_ptr) :: fswsfcn = c_null_ptr, fswintn = c_null_ptr, Sswabsn = c_null_ptr, Iswabsn = c_null_ptr
         type (c_ptr) :: fpond = c_null_ptr, mlt_onset = c_null_ptr, frz_onset = c_null_ptr
         type (c_ptr) :: flwoutn = c_null_ptr, evapn = c_null_ptr, freshn = c_null_ptr, fsaltn = c_null_ptr, fhocnn = c_null_ptr
         type (c_ptr) :: fsensn = c_null_ptr, flatn = c_null_ptr, fsurfn = c_null_ptr, fcondtopn = c_null_ptr
         type (c_ptr) :: melttn = c_null_ptr, meltsn = c_null_ptr, meltbn = c_null_ptr, congeln = c_null_ptr, snoicen = c_null_ptr
         type (c_ptr) :: dsnown = c_null_ptr
      end type evpk_thermo_args

      ! evpk_therm1_args (include/evpk.h): the arguments of evpk_step_therm1, member for member.  tv: shcoef, lhcoef, fbot, Tbot may stay
      ! c_null_ptr (given, they receive what the call computed); lmask_n / lmask_s: integer (c_int32_t) block arrays, as evpk_geom's tmask
      type, bind(C) :: evpk_therm1_args
         type (evpk_thermo_args) :: tv
         type (c_ptr) :: aice = c_null_ptr, frzmlt = c_null_ptr, sst = c_null_ptr, Tf = c_null_ptr, strocnxT = c_null_ptr
         type (c_ptr) :: strocnyT = c_null_ptr, uatm = c_null_ptr, vatm = c_null_ptr, wind = c_null_ptr, zlvl = c_null_ptr, frain = c_null_ptr
         type (c_ptr) :: fswthrun = c_null_ptr
         type (c_ptr) :: lmask_n = c_null_ptr, lmask_s = c_null_ptr
         type (c_ptr) :: Cdn_atm = c_null_ptr
         type (c_ptr) :: rside = c_null_ptr, aice_init = c_null_ptr, aicen_init = c_null_ptr, vicen_init = c_null_ptr
         type (c_ptr) :: strairxT = c_null_ptr, strairyT = c_null_ptr, Cdn_atm_ratio = c_null_ptr, fsurf = c_null_ptr, fcondtop = c_null_ptr
         type (c_ptr) :: fsens = c_null_ptr, flat = c_null_ptr, fswabs = c_null_ptr, flwout = c_null_ptr, evap = c_null_ptr, Tref = c_null_ptr
         type (c_ptr) :: Qref = c_null_ptr, Uref = c_null_ptr
         type (c_ptr) :: fresh = c_null_ptr, fsalt = c_null_ptr, fhocn = c_null_ptr, fswthru = c_null_ptr, meltt = c_null_ptr, meltb = c_null_ptr
         type (c_ptr) :: melts = c_null_ptr, congel = c_null_ptr, snoice = c_null_ptr
         type (c_ptr) :: strairxn = c_null_ptr, strairyn = c_null_ptr, Cdn_atm_ratio_n = c_null_ptr, Trefn = c_null_ptr, Qrefn = c_null_ptr
         type (c_ptr) :: Urefn = c_null_ptr
         real (c_double) :: chio = 0.006_c_double, ustar_min = 0.0005_c_double, hi_min = 0.01_c_double, pndaspect = 0.8_c_double
         real (c_double) :: rfracmin = 0.15_c_double, rfracmax = 1.0_c_double
         integer (c_int32_t) :: natmiter = 5, calc_strair = 1, tr_iage = 0, tr_FY = 0, nt_iage = 0, nt_FY = 0
         integer (c_int32_t) :: formdrag = 0, highfreq = 0, atmbndy_constant = 0, fbot_xfer_Cdn_ocn = 0, tr_aero = 0
      end type evpk_therm1_args

      ! evpk_rad_args, evpk_prep_rad_args (include/evpk.h): the arguments of evpk_step_radiation and evpk_prep_radiation, member for
      ! member.  ocn_albedo2D and fswpenln may stay c_null_ptr; of t only nt_Tsfc, nilyr, nslyr are read
      type, bind(C) :: evpk_rad_args
         integer (c_int32_t) :: shortwave_dEdd = 0, calc_Tsfc = 1, heat_capacity = 1, albedo_constant = 0
         integer (c_int32_t) :: ncat, ntrcr, ntrcr_dim
         type (evpk_itd_tracers) :: t
         real (c_double) :: puny
         real (c_double) :: albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, albocn, awtvdr, awtidr, awtvdf, awtidf
         type (c_ptr) :: aicen = c_null_ptr, vicen = c_null_ptr, vsnon = c_null_ptr, trcrn = c_null_ptr
         type (c_ptr) :: swvdr = c_null_ptr, swvdf = c_null_ptr, swidr = c_null_ptr, swidf = c_null_ptr, ocn_albedo2D = c_null_ptr
         type (c_ptr) :: alvdrn = c_null_ptr, alidrn = c_null_ptr, alvdfn = c_null_ptr, alidfn = c_null_ptr, albicen = c_null_ptr
         type (c_ptr) :: albsnon = c_null_ptr, fswsfcn = c_null_ptr, fswintn = c_null_ptr, fswthrun = c_null_ptr
         type (c_ptr) :: Sswabsn = c_null_ptr, Iswabsn = c_null_ptr, fswpenln = c_null_ptr
         type (c_ptr) :: coszen = c_null_ptr, alvdr = c_null_ptr, alidr = c_null_ptr, alvdf = c_null_ptr, alidf = c_null_ptr
         type (c_ptr) :: albice = c_null_ptr, albsno = c_null_ptr, scale_factor = c_null_ptr
      end type evpk_rad_args
      type, bind(C) :: evpk_prep_rad_args
         integer (c_int32_t) :: ncat, nilyr, nslyr
         real (c_double) :: puny
         type (c_ptr) :: aice = c_null_ptr, aicen = c_null_ptr, swvdr = c_null_ptr, swvdf = c_null_ptr, swidr = c_null_ptr, swidf = c_null_ptr
         type (c_ptr) :: alvdr_ai = c_null_ptr, alvdf_ai = c_null_ptr, alidr_ai = c_null_ptr, alidf_ai = c_null_ptr
         type (c_ptr) :: scale_factor = c_null_ptr, fswsfcn = c_null_ptr, fswintn = c_null_ptr, fswthrun = c_null_ptr, fswpenln = c_null_ptr
         type (c_ptr) :: Sswabsn = c_null_ptr, Iswabsn = c_null_ptr
         type (c_ptr) :: fswfac = c_null_ptr
      end type evpk_prep_rad_args

      ! evpk_dedd_args (include/evpk.h): the arguments of evpk_step_radiation_dedd, member for member.  fswpenln may stay c_null_ptr; of t
      ! nt_Tsfc, nt_apnd, nt_hpnd, nilyr, nslyr are read; the scalars default to the namelist defaults of source/ice_init.F90:289-304, :318-321
      type, bind(C) :: evpk_dedd_args
         integer (c_int32_t) :: calc_Tsfc = 1, heat_capacity = 1, tr_pond_cesm = 0, tr_pond_lvl = 0, tr_pond_topo = 0, tr_aero = 0
         integer (c_int32_t) :: ncat, ntrcr, ntrcr_dim
         type (evpk_itd_tracers) :: t
         real (c_double) :: puny
         real (c_double) :: R_ice = 0.0_c_double, R_pnd = 0.0_c_double, R_snw = 1.5_c_double, dT_mlt = 1.5_c_double
         real (c_double) :: rsnw_mlt = 1500.0_c_double, kalg = 0.60_c_double, hs0 = 0.03_c_double, pndaspect = 0.8_c_double
         real (c_double) :: awtvdr = 0.00318_c_double, awtidr = 0.00182_c_double, awtvdf = 0.63282_c_double, awtidf = 0.36218_c_double
         type (c_ptr) :: aicen = c_null_ptr, vicen = c_null_ptr, vsnon = c_null_ptr, trcrn = c_null_ptr
         type (c_ptr) :: swvdr = c_null_ptr, swvdf = c_null_ptr, swidr = c_null_ptr, swidf = c_null_ptr
         type (c_ptr) :: coszen = c_null_ptr
         type (c_ptr) :: alvdrn = c_null_ptr, alidrn = c_null_ptr, alvdfn = c_null_ptr, alidfn = c_null_ptr, albicen = c_null_ptr
         type (c_ptr) :: albsnon = c_null_ptr, fswsfcn = c_null_ptr, fswintn = c_null_ptr, fswthrun = c_null_ptr
         type (c_ptr) :: Sswabsn = c_null_ptr, Iswabsn = c_null_ptr, fswpenln = c_null_ptr
         type (c_ptr) :: alvdr = c_null_ptr, alidr = c_null_ptr, alvdf = c_null_ptr, alidf = c_null_ptr
         type (c_ptr) :: albice = c_null_ptr, albsno = c_null_ptr, scale_factor = c_null_ptr
         type (c_ptr) :: albpndn = c_null_ptr, apeffn = c_null_ptr, snowfracn = c_null_ptr
         type (c_ptr) :: albpnd = c_null_ptr, apeff_ai = c_null_ptr
      end type evpk_dedd_args

      ! evpk_pond_lvl_args (include/evpk.h): what compute_ponds_lvl and the tr_pond_lvl block of run_dEdd hand each other, and the scheme's
      ! namelist, member for member.  Tair is read by evpk_step_therm1_lvl only, fsnow, hs1, dt and linitonly by
      ! evpk_step_radiation_dedd_lvl only; frzpnd: 0 'cesm', 1 'hlid'
      type, bind(C) :: evpk_pond_lvl_args
         type (c_ptr) :: dhsn = c_null_ptr, ffracn = c_null_ptr
         type (c_ptr) :: Tair = c_null_ptr, fsnow = c_null_ptr
         real (c_double) :: dpscale = 1.0_c_double, hs1 = 0.03_c_double, dt = 0.0_c_double
         integer (c_int32_t) :: frzpnd = 0, nt_ipnd = 0, linitonly = 0
      end type evpk_pond_lvl_args

      public :: evpk_get_unique_id, evpk_create, evpk_set_params, evpk_run, &
                evpk_get_stats, evpk_destroy, evpk_last_error, evpk_error_string, &
                evpk_principal_stress, evpk_pin_host, evpk_unpin_host, evpk_host_alloc, evpk_host_free, evpk_host_is_mapped, &
                evpk_upload, evpk_prep, evpk_subcycle, evpk_finish, evpk_download, &
                evpk_connect, evpk_device_check, evpk_restart_write, evpk_restart_read, &
                evpk_halo_update, evpk_halo_update_stress, evpk_transport_upwind_state, &
                evpk_transport_upwind, evpk_remap_init, evpk_transport_remap, evpk_transport_remap_state, &
                EVPK_REMAP_BAD_DEPARTURE, EVPK_REMAP_NEGATIVE_MASS, &
                evpk_eap_state, evpk_eap_init, evpk_eap_upload, evpk_eap_download, &
                evpk_ridge_tracers, evpk_ridge_diag, evpk_ridge_ice, EVPK_RIDGE_STOP, &
                evpk_itd_tracers, evpk_itd_constants, evpk_cleanup_itd, evpk_aggregate, EVPK_ITD_STOP, &
                evpk_dyn_args, evpk_bound_state, evpk_step_dynamics, evpk_linear_itd, EVPK_LITD_STOP, &
                evpk_therm2_args, evpk_new_ice_lateral_melt, evpk_step_therm2, &
                evpk_thermo_args, evpk_thermo_vertical, EVPK_THERMO_STOP, &
                evpk_therm1_args, evpk_step_therm1, &
                evpk_rad_args, evpk_prep_rad_args, evpk_step_radiation, evpk_prep_radiation, &
                evpk_dedd_args, evpk_step_radiation_dedd, &
                evpk_pond_lvl_args, evpk_step_therm1_lvl, evpk_step_radiation_dedd_lvl

      integer (c_int), parameter :: EVPK_REMAP_BAD_DEPARTURE = 11, EVPK_REMAP_NEGATIVE_MASS = 12     ! include/evpk.h
      integer (c_int), parameter :: EVPK_RIDGE_STOP = 13
      integer (c_int), parameter :: EVPK_ITD_STOP = 14
      integer (c_int), parameter :: EVPK_LITD_STOP = 15
      integer (c_int), parameter :: EVPK_THERMO_STOP = 16

      interface
         integer (c_int) function evpk_get_unique_id (id) bind(C, name='evpk_get_unique_id')
            import :: c_int, c_ptr
            type (c_ptr), value :: id
         end function
         integer (c_int) function evpk_create (g, ctx) bind(C, name='evpk_create')
            import :: c_int, c_ptr, evpk_geom
            type (evpk_geom), intent(in) :: g
            type (c_ptr), intent(out) :: ctx
         end function
         integer (c_int) function evpk_set_params (ctx, p) bind(C, name='evpk_set_params')
            import :: c_int, c_ptr, evpk_params
            type (c_ptr), value :: ctx
            type (evpk_params), intent(in) :: p
         end function
         integer (c_int) function evpk_run (ctx, sin, st) bind(C, name='evpk_run')
            import :: c_int, c_ptr, evpk_step_in, evpk_state
            type (c_ptr), value :: ctx
            type (evpk_step_in), intent(in) :: sin
            type (evpk_state), intent(in) :: st
         end function
         ! evpk_run in stages.  st = c_null_ptr in evpk_upload: inputs only, the prognostic state (uvel, vvel, the
         ! twelve stresses, iceumask) stays as the previous call left it on the device
         integer (c_int) function evpk_upload (ctx, sin, st) bind(C, name='evpk_upload')
            import :: c_int, c_ptr, evpk_step_in
            type (c_ptr), value :: ctx
            type (evpk_step_in), intent(in) :: sin
            type (c_ptr), value :: st                      ! c_loc of an evpk_state, or c_null_ptr
         end function
         integer (c_int) function evpk_prep (ctx) bind(C, name='evpk_prep')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx
         end function
         integer (c_int) function evpk_subcycle (ctx, nsub) bind(C, name='evpk_subcycle')
            import :: c_int, c_ptr, c_int32_t
            type (c_ptr), value :: ctx
            integer (c_int32_t), value :: nsub
         end function
         integer (c_int) function evpk_finish (ctx) bind(C, name='evpk_finish')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx
         end function
         integer (c_int) function evpk_download (ctx, st) bind(C, name='evpk_download')
            import :: c_int, c_ptr, evpk_state
            type (c_ptr), value :: ctx
            type (evpk_state), intent(in) :: st
         end function
         integer (c_int) function evpk_get_stats (ctx, s) bind(C, name='evpk_get_stats')
            import :: c_int, c_ptr, evpk_stats
            type (c_ptr), value :: ctx
            type (evpk_stats), intent(out) :: s
         end function
         ! principal_stress (ice_dyn_shared.F90:853) from the device-resident state of the last evp
         integer (c_int) function evpk_principal_stress (ctx, sig1, sig2) bind(C, name='evpk_principal_stress')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx, sig1, sig2
         end function
         ! page-lock a host array kept for the life of the run: moved in place over PCIe instead of staged
         integer (c_int) function evpk_pin_host (ptr, bytes) bind(C, name='evpk_pin_host')
            import :: c_int, c_ptr, c_size_t
            type (c_ptr), value :: ptr
            integer (c_size_t), value :: bytes
         end function
         integer (c_int) function evpk_unpin_host (ptr) bind(C, name='evpk_unpin_host')
            import :: c_int, c_ptr
            type (c_ptr), value :: ptr
         end function
         ! page-locked memory allocated and pinned by the driver (hipHostMalloc): c_f_pointer(out, a, shape) makes it an array
         integer (c_int) function evpk_host_alloc (bytes, out) bind(C, name='evpk_host_alloc')
            import :: c_int, c_ptr, c_size_t
            integer (c_size_t), value :: bytes
            type (c_ptr), intent(out) :: out
         end function
         integer (c_int) function evpk_host_free (ptr) bind(C, name='evpk_host_free')
            import :: c_int, c_ptr
            type (c_ptr), value :: ptr
         end function
         integer (c_int) function evpk_host_is_mapped (ptr, bytes) bind(C, name='evpk_host_is_mapped')
            import :: c_int, c_ptr, c_size_t
            type (c_ptr), value :: ptr
            integer (c_size_t), value :: bytes
         end function
         ! two-phase start (nranks > 1): evpk_create with unique_id = c_null_ptr, agree across ranks, then connect
         integer (c_int) function evpk_connect (ctx, id) bind(C, name='evpk_connect')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx, id
         end function
         integer (c_int) function evpk_device_check (device) bind(C, name='evpk_device_check')
            import :: c_int, c_int32_t
            integer (c_int32_t), value :: device
         end function
         ! the dynamics records of the binary restart (ice_restart_driver.F90:122-176, :295-412) from / into the device state
         integer (c_int) function evpk_restart_write (ctx, path, append, big_endian) bind(C, name='evpk_restart_write')
            import :: c_int, c_ptr, c_char, c_int32_t
            type (c_ptr), value :: ctx
            character (kind=c_char), dimension(*), intent(in) :: path      ! null-terminated
            integer (c_int32_t), value :: append, big_endian
         end function
         integer (c_int) function evpk_restart_read (ctx, path, byte_offset, big_endian) bind(C, name='evpk_restart_read')
            import :: c_int, c_ptr, c_char, c_int32_t, c_int64_t
            type (c_ptr), value :: ctx
            character (kind=c_char), dimension(*), intent(in) :: path
            integer (c_int64_t), value :: byte_offset
            integer (c_int32_t), value :: big_endian
         end function
         ! ice_HaloUpdate / ice_HaloUpdate_stress of a block array on the device (include/evpk.h): a(nx_block,ny_block[,nz],nblocks)
         integer (c_int) function evpk_halo_update (ctx, a, nz, field_loc, field_type, fill) bind(C, name='evpk_halo_update')
            import :: c_int, c_ptr, c_double, c_int32_t
            type (c_ptr), value :: ctx, a
            integer (c_int32_t), value :: nz, field_loc, field_type
            real (c_double), value :: fill
         end function
         integer (c_int) function evpk_halo_update_stress (ctx, a1, a2) bind(C, name='evpk_halo_update_stress')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx, a1, a2
         end function
         ! transport_upwind (ice_transport_driver.F90:634-772) on the resident velocities: works(nx_block,ny_block,narr,nblocks)
         ! as state_to_work fills it, advected in place
         integer (c_int) function evpk_transport_upwind (ctx, dt, narr, works) bind(C, name='evpk_transport_upwind')
            import :: c_int, c_ptr, c_double, c_int32_t
            type (c_ptr), value :: ctx
            real (c_double), value :: dt
            integer (c_int32_t), value :: narr
            type (c_ptr), value :: works
         end function
         ! transport_upwind whole (state_to_work, upwind_field, work_to_state, bound_state; include/evpk.h)
         integer (c_int) function evpk_transport_upwind_state (ctx, dt, ncat, ntrcr, ntrcr_dim, trcr_depend, nt_Tsfc, nt_alvl, nt_apnd, &
               nt_fbri, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, Tocnfrz, aice0, aicen, vicen, vsnon, trcrn) &
               bind(C, name='evpk_transport_upwind_state')
            import :: c_int, c_ptr, c_double, c_int32_t
            type (c_ptr), value :: ctx, trcr_depend, aice0, aicen, vicen, vsnon, trcrn
            real (c_double), value :: dt, Tocnfrz
            integer (c_int32_t), value :: ncat, ntrcr, ntrcr_dim, nt_Tsfc, nt_alvl, nt_apnd, nt_fbri, tr_pond_cesm, tr_pond_lvl, tr_pond_topo
         end function
         ! ridge_ice (ice_mechred.F90:101-746) for every block: the call of step_ridge (ice_step_mod.F90:1285-1305).  rdg_conv,
         ! rdg_shear = c_null_ptr: the planes the last evp / eap left on the device; stop(4): reason, block, i, j
         integer (c_int) function evpk_ridge_ice (ctx, dt, ndtd, ncat, ntrcr, ntrcr_dim, trcr_depend, t, hin_max, rdg_conv, rdg_shear, &
               aice0, aicen, vicen, vsnon, trcrn, diag, stop) bind(C, name='evpk_ridge_ice')
            import :: c_int, c_ptr, c_double, c_int32_t, evpk_ridge_tracers
            type (c_ptr), value :: ctx, trcr_depend, hin_max, rdg_conv, rdg_shear, aice0, aicen, vicen, vsnon, trcrn, diag
            real (c_double), value :: dt
            integer (c_int32_t), value :: ndtd, ncat, ntrcr, ntrcr_dim
            type (evpk_ridge_tracers), intent(in) :: t
            integer (c_int32_t), intent(out) :: stop(4)
         end function
         ! cleanup_itd (ice_itd.F90:1514-1769) for every block: the call of step_ridge (ice_step_mod.F90:1325-1341), dt = dt * ndtd.  fpond,
         ! fresh, fsalt, fhocn, first_ice (integer(c_int32_t), 0 / 1) may be c_null_ptr; stop(4): reason, block, i, j
         integer (c_int) function evpk_cleanup_itd (ctx, dt, ncat, ntrcr, ntrcr_dim, trcr_depend, t, hin_max, k, tr_aero, nbtrcr, &
               heat_capacity, aicen, vicen, vsnon, trcrn, aice0, aice, fpond, fresh, fsalt, fhocn, first_ice, stop) &
               bind(C, name='evpk_cleanup_itd')
            import :: c_int, c_ptr, c_double, c_int32_t, evpk_itd_tracers, evpk_itd_constants
            type (c_ptr), value :: ctx, trcr_depend, hin_max, aicen, vicen, vsnon, trcrn, aice0, aice, fpond, fresh, fsalt, fhocn, first_ice
            real (c_double), value :: dt
            integer (c_int32_t), value :: ncat, ntrcr, ntrcr_dim, tr_aero, nbtrcr, heat_capacity
            type (evpk_itd_tracers), intent(in) :: t
            type (evpk_itd_constants), intent(in) :: k
            integer (c_int32_t), intent(out) :: stop(4)
         end function
         ! linear_itd (ice_therm_itd.F90:69-859) for every block: what step_therm2 does at ice_step_mod.F90:821-871 (kitd = 1).
         ! aicen_init, vicen_init: the state before the vertical thermodynamics; fpond may be c_null_ptr unless tr_pond_topo;
         ! stop(4): reason (2 .. 5 of shift_ice), block, i, j
         integer (c_int) function evpk_linear_itd (ctx, ncat, ntrcr, ntrcr_dim, trcr_depend, t, hin_max, hi_min, k, aicen_init, &
               vicen_init, aicen, vicen, vsnon, trcrn, aice, aice0, fpond, stop) bind(C, name='evpk_linear_itd')
            import :: c_int, c_ptr, c_double, c_int32_t, evpk_itd_tracers, evpk_itd_constants
            type (c_ptr), value :: ctx, trcr_depend, hin_max, aicen_init, vicen_init, aicen, vicen, vsnon, trcrn, aice, aice0, fpond
            real (c_double), value :: hi_min
            integer (c_int32_t), value :: ncat, ntrcr, ntrcr_dim
            type (evpk_itd_tracers), intent(in) :: t
            type (evpk_itd_constants), intent(in) :: k
            integer (c_int32_t), intent(out) :: stop(4)
         end function
         ! bound_state (bound = 1), aggregate (ice_itd.F90:246-458) on every cell and the tendencies of step_dynamics
         ! (ice_step_mod.F90:1152-1189); daidtd, dvidtd, dagedtd may be c_null_ptr
         integer (c_int) function evpk_aggregate (ctx, dt, bound, ncat, ntrcr, ntrcr_dim, trcr_depend, t, nt_iage, Tocnfrz, aicen, vicen, &
               vsnon, trcrn, aice, vice, vsno, aice0, trcr, daidtd, dvidtd, dagedtd) bind(C, name='evpk_aggregate')
            import :: c_int, c_ptr, c_double, c_int32_t, evpk_itd_tracers
            type (c_ptr), value :: ctx, trcr_depend, aicen, vicen, vsnon, trcrn, aice, vice, vsno, aice0, trcr, daidtd, dvidtd, dagedtd
            real (c_double), value :: dt, Tocnfrz
            integer (c_int32_t), value :: bound, ncat, ntrcr, ntrcr_dim, nt_iage
            type (evpk_itd_tracers), intent(in) :: t
         end function
         ! bound_state (ice_state.F90:173-238) alone, one launch between the block arrays; trcrn may be c_null_ptr when ntrcr = 0
         integer (c_int) function evpk_bound_state (ctx, ncat, ntrcr, ntrcr_dim, aicen, vicen, vsnon, trcrn) bind(C, name='evpk_bound_state')
            import :: c_int, c_ptr, c_int32_t
            type (c_ptr), value :: ctx, aicen, vicen, vsnon, trcrn
            integer (c_int32_t), value :: ncat, ntrcr, ntrcr_dim
         end function
         ! everything of step_dynamics behind evp / eap (ice_step_mod.F90:1126-1192) in one call, the arrays staged once;
         ! stop(5): stage (1 transport, 2 ridge, 3 cleanup), reason, block, i, j
         integer (c_int) function evpk_step_dynamics (ctx, a, stop) bind(C, name='evpk_step_dynamics')
            import :: c_int, c_ptr, c_int32_t, evpk_dyn_args
            type (c_ptr), value :: ctx
            type (evpk_dyn_args), intent(in) :: a
            integer (c_int32_t), intent(out) :: stop(5)
         end function
         ! add_new_ice, lateral_melt and (ncat = 1) reduce_area of step_therm2 (ice_step_mod.F90:875-960) in one launch, on the aice / aice0
         ! given: for a host that keeps its own linear_itd
         integer (c_int) function evpk_new_ice_lateral_melt (ctx, a) bind(C, name='evpk_new_ice_lateral_melt')
            import :: c_int, c_ptr, evpk_therm2_args
            type (c_ptr), value :: ctx
            type (evpk_therm2_args), intent(in) :: a
         end function
         ! step_therm2 (ice_step_mod.F90:741-995) in one call, the arrays staged once: the frain line, aggregate_area, linear_itd
         ! (kitd = 1), add_new_ice, lateral_melt, cleanup_itd; stop(5): stage (1 linear_itd, 3 cleanup), reason, block, i, j
         integer (c_int) function evpk_step_therm2 (ctx, a, stop) bind(C, name='evpk_step_therm2')
            import :: c_int, c_ptr, c_int32_t, evpk_therm2_args
            type (c_ptr), value :: ctx
            type (evpk_therm2_args), intent(in) :: a
            integer (c_int32_t), intent(out) :: stop(5)
         end function
         ! thermo_vertical (ice_therm_vertical.F90:79-531, BL99: ktherm = 1, heat_capacity, calc_Tsfc, l_brine) for every category of every
         ! block in one launch: the call of ice_step_mod.F90:513-540; stop(5): reason 1 .. 7, block, category, i, j
         integer (c_int) function evpk_thermo_vertical (ctx, a, stop) bind(C, name='evpk_thermo_vertical')
            import :: c_int, c_ptr, c_int32_t, evpk_thermo_args
            type (c_ptr), value :: ctx
            type (evpk_thermo_args), intent(in) :: a
            integer (c_int32_t), intent(out) :: stop(5)
         end function

         ! step_therm1 (ice_step_mod.F90:154-733) in one call: frzmlt_bottom_lateral, atmo_boundary_layer, increment_age, update_FYarea,
         ! thermo_vertical, compute_ponds_cesm, merge_fluxes; stop(5) as evpk_thermo_vertical (EVPK_THERMO_STOP)
         integer (c_int) function evpk_step_therm1 (ctx, a, stop) bind(C, name='evpk_step_therm1')
            import :: c_int, c_ptr, c_int32_t, evpk_therm1_args
            type (c_ptr), value :: ctx
            type (evpk_therm1_args), intent(in) :: a
            integer (c_int32_t), intent(out) :: stop(5)
         end function
         ! step_radiation (ice_step_mod.F90:1364-1524, shortwave_ccsm3) with the albedo lines of coupling_prep in one launch, and
         ! prep_radiation (:33-145), which an AusCOM host does not call (drivers/auscom/CICE_RunMod.F90:332-338)
         integer (c_int) function evpk_step_radiation (ctx, a) bind(C, name='evpk_step_radiation')
            import :: c_int, c_ptr, evpk_rad_args
            type (c_ptr), value :: ctx
            type (evpk_rad_args), intent(in) :: a
         end function
         integer (c_int) function evpk_prep_radiation (ctx, a) bind(C, name='evpk_prep_radiation')
            import :: c_int, c_ptr, evpk_prep_rad_args
            type (c_ptr), value :: ctx
            type (evpk_prep_rad_args), intent(in) :: a
         end function
         ! step_radiation on its Delta-Eddington branch (ice_step_mod.F90:1408-1451, run_dEdd) with the albedo lines of coupling_prep in
         ! one launch; coszen is in / out: the caller runs compute_coszen first
         integer (c_int) function evpk_step_radiation_dedd (ctx, a) bind(C, name='evpk_step_radiation_dedd')
            import :: c_int, c_ptr, evpk_dedd_args
            type (c_ptr), value :: ctx
            type (evpk_dedd_args), intent(in) :: a
         end function
         ! the two calls above under tr_pond_lvl: compute_ponds_lvl (ice_meltpond_lvl.F90:79-404) in the place of compute_ponds_cesm, and
         ! the level-ice block of run_dEdd (ice_shortwave.F90:1450-1514); dhsn and ffracn of p pass from one to the other
         integer (c_int) function evpk_step_therm1_lvl (ctx, a, p, stop) bind(C, name='evpk_step_therm1_lvl')
            import :: c_int, c_ptr, c_int32_t, evpk_therm1_args, evpk_pond_lvl_args
            type (c_ptr), value :: ctx
            type (evpk_therm1_args), intent(in) :: a
            type (evpk_pond_lvl_args), intent(in) :: p
            integer (c_int32_t), intent(out) :: stop(5)
         end function
         integer (c_int) function evpk_step_radiation_dedd_lvl (ctx, a, p) bind(C, name='evpk_step_radiation_dedd_lvl')
            import :: c_int, c_ptr, evpk_dedd_args, evpk_pond_lvl_args
            type (c_ptr), value :: ctx
            type (evpk_dedd_args), intent(in) :: a
            type (evpk_pond_lvl_args), intent(in) :: p
         end function
         ! horizontal_remap (ice_transport_remap.F90:309-850) on the resident velocities: dxu, dyu, hm once, then
         ! mm(nx_block,ny_block,0:ncat,max_blocks), tm(nx_block,ny_block,ntrace,ncat,max_blocks) advanced in place
         integer (c_int) function evpk_remap_init (ctx, dxu, dyu, hm) bind(C, name='evpk_remap_init')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx, dxu, dyu, hm
         end function
         integer (c_int) function evpk_transport_remap (ctx, dt, ncat, ntrace, mm, tm, tracer_type, depend, has_dependents, &
                                                        integral_order, l_dp_midpt, l_fixed_area) bind(C, name='evpk_transport_remap')
            import :: c_int, c_ptr, c_double, c_int32_t
            type (c_ptr), value :: ctx
            real (c_double), value :: dt
            integer (c_int32_t), value :: ncat, ntrace
            type (c_ptr), value :: mm, tm, tracer_type, depend, has_dependents
            integer (c_int32_t), value :: integral_order, l_dp_midpt, l_fixed_area
         end function
         ! transport_remap with state_to_tracers / tracers_to_state / bound_state on the device too: the state arrays themselves
         integer (c_int) function evpk_transport_remap_state (ctx, dt, ncat, ntrcr, ntrcr_dim, nt_qsno, nslyr, rhos_lfresh, &
               aice0, aicen, vicen, vsnon, trcrn, tracer_type, depend, has_dependents, integral_order, l_dp_midpt) &
               bind(C, name='evpk_transport_remap_state')
            import :: c_int, c_ptr, c_double, c_int32_t
            type (c_ptr), value :: ctx
            real (c_double), value :: dt, rhos_lfresh
            integer (c_int32_t), value :: ncat, ntrcr, ntrcr_dim, nt_qsno, nslyr
            type (c_ptr), value :: aice0, aicen, vicen, vsnon, trcrn, tracer_type, depend, has_dependents
            integer (c_int32_t), value :: integral_order, l_dp_midpt
         end function
         ! EAP (ice_dyn_eap.F90): tables of init_eap once, then the context runs eap(dt); structure tensor up / everything down
         integer (c_int) function evpk_eap_init (ctx, nx_yield, ny_yield, na_yield, s11r, s12r, s22r, s11s, s12s, s22s) &
               bind(C, name='evpk_eap_init')
            import :: c_int, c_ptr, c_int32_t
            type (c_ptr), value :: ctx
            integer (c_int32_t), value :: nx_yield, ny_yield, na_yield
            type (c_ptr), value :: s11r, s12r, s22r, s11s, s12s, s22s
         end function
         integer (c_int) function evpk_eap_upload (ctx, st) bind(C, name='evpk_eap_upload')
            import :: c_int, c_ptr, evpk_eap_state
            type (c_ptr), value :: ctx
            type (evpk_eap_state), intent(in) :: st
         end function
         integer (c_int) function evpk_eap_download (ctx, st) bind(C, name='evpk_eap_download')
            import :: c_int, c_ptr, evpk_eap_state
            type (c_ptr), value :: ctx
            type (evpk_eap_state), intent(in) :: st
         end function
         integer (c_int) function evpk_destroy (ctx) bind(C, name='evpk_destroy')
            import :: c_int, c_ptr
            type (c_ptr), value :: ctx
         end function
         type (c_ptr) function evpk_last_error (ctx) bind(C, name='evpk_last_error')
            import :: c_ptr
            type (c_ptr), value :: ctx
         end function
      end interface

      contains

      ! C string of evpk_last_error -> Fortran string (for abort_ice)
      function evpk_error_string (ctx) result (msg)
         type (c_ptr), intent(in) :: ctx
         character (len=512) :: msg
         type (c_ptr) :: p
         character (kind=c_char), pointer :: s(:)
         integer :: i
         msg = ' '
         p = evpk_last_error (ctx)
         if (.not. c_associated(p)) return
         call c_f_pointer (p, s, [512])
         do i = 1, 512
            if (s(i) == c_null_char) exit
            msg(i:i) = s(i)
         enddo
      end function evpk_error_string

      end module evpk_mod
