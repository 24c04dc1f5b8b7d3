!=======================================================================
! Everything of step_dynamics behind evp / eap on the device, in one library call.
!
! In the reference's step_dynamics (source/ice_step_mod.F90) the lines from the transport call through the tendency loop
! (:1126-1192: transport_upwind | transport_remap, the step_ridge loop, bound_state, aggregate, daidtd / dvidtd / dagedtd)
! become
!     use ice_step_dyn, only: evpk_step_dynamics_core
!     call evpk_step_dynamics_core (dt, ndtd)
! It runs over the reference's own module arrays (ice_state, ice_flux, ice_itd, ice_zbgc_shared) and stages each of them once:
! the four separate entry points would copy the category state up and down once each.  This module only marshals arguments;
! what the call computes is evpk_step_dynamics (include/evpk.h).
!
! ice_transport_driver keeps tracer_type, depend and has_dependents private, so they are rebuilt here from trcr_depend by the
! rule of init_transport (ice_transport_driver.F90:90-118).  integral_order and l_dp_midpt are private there too: optional
! arguments with the reference's values (3, .true.).
!
! More than one task (x-slabs, one GPU each): every task makes this call -- evpk_step_dynamics is collective, bound_state
! exchanges between the slab neighbours and the tripole fold partners; a task without a block column returns at once.  Stops are
! per task, as the reference's l_stop: any non-zero return goes to abort_ice below, which ends the run on every task; the task that
! stopped has still posted its exchanges, so no other task waits for it.  The block number in the message is the task's local one.
!=======================================================================

      module ice_step_dyn

      use ice_kinds_mod
      use, intrinsic :: iso_c_binding
      use evpk_mod

      implicit none
      private
      public :: evpk_step_dynamics_core, evpk_step_radiation_core, evpk_step_radiation_dedd_core
      public :: evpk_step_radiation_dedd_lvl_core, evpk_step_therm1_lvl_core

      ! step_therm1 keeps these five per category only as 2-D locals (ice_step_mod.F90:216-223); the library wants planes per category
      real (kind=dbl_kind), dimension (:,:,:,:), allocatable, save, target :: flwoutn_w, evapn_w, freshn_w, fsaltn_w, fhocnn_w
      integer (c_int32_t), dimension (:,:,:), allocatable, save, target :: lmask_n_w, lmask_s_w

      contains

!=======================================================================

      subroutine evpk_step_dynamics_core (dt, ndtd, integral_order, l_dp_midpt)

      use ice_blocks, only: nx_block, ny_block
      use ice_constants, only: rhos, Lfresh, Tocnfrz, ice_ref_salinity, hs_min, cp_ice, puny
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr, max_blocks
      use ice_dyn_evp, only: evpk_context
      use ice_exit, only: abort_ice
      use ice_fileunits, only: nu_diag
      use ice_flux, only: rdg_conv, rdg_shear, dardg1dt, dardg2dt, dvirdgdt, opening, fpond, fresh, fsalt, fhocn, &
          aparticn, krdgn, aredistn, vredistn, dardg1ndt, dardg2ndt, dvirdgndt, araftn, vraftn, daidtd, dvidtd, dagedtd
      use ice_grid, only: dxu, dyu, hm
      use ice_itd, only: hin_max
      use ice_state, only: aice0, aicen, vicen, vsnon, trcrn, aice, vice, vsno, trcr, ntrcr, trcr_depend, &
          nt_Tsfc, nt_qice, nt_qsno, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_fbri, nt_iage, &
          tr_iage, tr_lvl, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_brine, tr_aero, nbtrcr
      use ice_therm_shared, only: heat_capacity, Tmin
      use ice_transport_driver, only: advection
      use ice_zbgc_shared, only: first_ice

      real (kind=dbl_kind), intent(in) :: dt                 ! time step
      integer (kind=int_kind), intent(in) :: ndtd            ! number of dynamics subcycles
      integer (kind=int_kind), intent(in), optional :: integral_order
      logical (kind=log_kind), intent(in), optional :: l_dp_midpt

      type (evpk_dyn_args) :: a
      type (evpk_ridge_diag), target :: dg
      type (c_ptr) :: ctx
      integer (c_int32_t), dimension (max_ntrcr+2), target :: dep_trcr, ttype, dep, has
      real (c_double), dimension (0:ncat), target :: hin
      integer (c_int32_t), dimension (:,:,:,:), allocatable, target, save :: first_i      ! LOGICAL is not C-interoperable
      integer (c_int32_t) :: stop(5)
      integer (c_int) :: rc
      integer (kind=int_kind) :: nt, k, ntrace
      logical (kind=log_kind), save :: first = .true.
      character (len=16), parameter :: stage(3) = (/ 'transport       ', 'ridge_ice       ', 'cleanup_itd     ' /)

      ctx = evpk_context ()
      if (.not. c_associated(ctx)) call abort_ice('step_dynamics: no velocities on the device: evp has not run yet')

      a%advection = 2
      if (trim(advection) == 'upwind') a%advection = 1
      if (a%advection == 2 .and. first) then
         rc = evpk_remap_init (ctx, loc_r8(dxu), loc_r8(dyu), loc_r8(hm))
         if (rc /= 0) call abort_ice('step_dynamics: evpk_remap_init: '//trim(evpk_error_string(ctx)))
         first = .false.
      endif
      a%ridge = 1
      a%dt = dt
      a%ndtd = int(ndtd, c_int32_t)
      a%ncat = int(ncat, c_int32_t)
      a%ntrcr = int(ntrcr, c_int32_t)
      a%ntrcr_dim = int(max_ntrcr, c_int32_t)
      dep_trcr = 0
      dep_trcr(1:ntrcr) = trcr_depend(1:ntrcr)
      a%trcr_depend = c_loc(dep_trcr)

      ! the tracer indices the stages read, 1-based, 0 = not in use
      a%t%nt_Tsfc = int(nt_Tsfc, c_int32_t)
      a%t%nt_qice = int(nt_qice, c_int32_t);  a%t%nilyr = int(nilyr, c_int32_t)
      a%t%nt_qsno = int(nt_qsno, c_int32_t);  a%t%nslyr = int(nslyr, c_int32_t)
      if (tr_lvl) then
         a%t%nt_alvl = int(nt_alvl, c_int32_t);  a%nt_vlvl = int(nt_vlvl, c_int32_t)
      endif
      if (tr_pond_cesm .or. tr_pond_lvl .or. tr_pond_topo) then
         a%t%nt_apnd = int(nt_apnd, c_int32_t);  a%t%nt_hpnd = int(nt_hpnd, c_int32_t)
      endif
      if (tr_brine) a%t%nt_fbri = int(nt_fbri, c_int32_t)
      if (tr_iage) a%nt_iage = int(nt_iage, c_int32_t)
      a%t%tr_pond_cesm = merge(1_c_int32_t, 0_c_int32_t, tr_pond_cesm)
      a%t%tr_pond_lvl  = merge(1_c_int32_t, 0_c_int32_t, tr_pond_lvl)
      a%t%tr_pond_topo = merge(1_c_int32_t, 0_c_int32_t, tr_pond_topo)
      a%t%tr_brine     = merge(1_c_int32_t, 0_c_int32_t, tr_brine)

      hin(0:ncat) = hin_max(0:ncat)
      a%hin_max = c_loc(hin)
      a%k%Tocnfrz = Tocnfrz;  a%k%ice_ref_salinity = ice_ref_salinity;  a%k%hs_min = hs_min;  a%k%cp_ice = cp_ice
      a%k%Lfresh = Lfresh;  a%k%Tmin = Tmin;  a%k%puny = puny
      ! aerosols, bgc tracers and the zero-layer model are refused by the library, with its message
      a%tr_aero = merge(1_c_int32_t, 0_c_int32_t, tr_aero)
      a%nbtrcr = int(nbtrcr, c_int32_t)
      a%heat_capacity = merge(1_c_int32_t, 0_c_int32_t, heat_capacity)

      ! init_transport's rule (ice_transport_driver.F90:90-118): hice and hsno first, without a parent; a tracer of the area has none
      ! either (type 1), one that hangs on a tracer with a parent of its own is type 3, every other type 2; has_dependents from depend
      ntrace = 2 + ntrcr
      dep = 0;  ttype = 1;  has = 0
      k = 2
      do nt = 1, ntrcr
         dep(k+nt) = int(trcr_depend(nt), c_int32_t)
         ttype(k+nt) = 2
         if (trcr_depend(nt) == 0) then
            ttype(k+nt) = 1
         elseif (trcr_depend(nt) > 2) then
            if (trcr_depend(trcr_depend(nt)-2) > 0) ttype(k+nt) = 3
         endif
      enddo
      do nt = 1, ntrace
         if (dep(nt) > 0) then
            if (dep(nt) > nt) then
               write (nu_diag,*) 'Tracer nt2 =', nt, ' depends on tracer nt1 =', dep(nt)
               call abort_ice ('ice: remap transport: Must have nt2 > nt1')
            endif
            has(dep(nt)) = 1
         endif
      enddo
      a%tracer_type = c_loc(ttype);  a%depend = c_loc(dep);  a%has_dependents = c_loc(has)
      if (present(integral_order)) a%integral_order = int(integral_order, c_int32_t)
      if (present(l_dp_midpt)) a%l_dp_midpt = merge(1_c_int32_t, 0_c_int32_t, l_dp_midpt)
      a%rhos_lfresh = rhos*Lfresh

      ! the module arrays: (nx_block, ny_block, [max_ntrcr,] [ncat,] max_blocks), the first nblocks blocks are used
      a%aice0 = loc_r8(aice0);  a%aicen = loc_r8(aicen);  a%vicen = loc_r8(vicen);  a%vsnon = loc_r8(vsnon);  a%trcrn = loc_r8(trcrn)
      a%aice = loc_r8(aice);  a%vice = loc_r8(vice);  a%vsno = loc_r8(vsno);  a%trcr = loc_r8(trcr)
      a%daidtd = loc_r8(daidtd);  a%dvidtd = loc_r8(dvidtd)
      if (tr_iage) a%dagedtd = loc_r8(dagedtd)
      a%fpond = loc_r8(fpond);  a%fresh = loc_r8(fresh);  a%fsalt = loc_r8(fsalt);  a%fhocn = loc_r8(fhocn)
      a%rdg_conv = loc_r8(rdg_conv);  a%rdg_shear = loc_r8(rdg_shear)
      if (.not. allocated(first_i)) allocate (first_i(nx_block,ny_block,ncat,max_blocks))
      first_i = merge(1_c_int32_t, 0_c_int32_t, first_ice)
      a%first_ice = c_loc(first_i)
      dg%dardg1dt = loc_r8(dardg1dt);  dg%dardg2dt = loc_r8(dardg2dt);  dg%dvirdgdt = loc_r8(dvirdgdt);  dg%opening = loc_r8(opening)
      dg%dardg1ndt = loc_r8(dardg1ndt);  dg%dardg2ndt = loc_r8(dardg2ndt);  dg%dvirdgndt = loc_r8(dvirdgndt)
      dg%aparticn = loc_r8(aparticn);  dg%krdgn = loc_r8(krdgn);  dg%araftn = loc_r8(araftn);  dg%vraftn = loc_r8(vraftn)
      dg%aredistn = loc_r8(aredistn);  dg%vredistn = loc_r8(vredistn)
      a%diag = c_loc(dg)

      rc = evpk_step_dynamics (ctx, a, stop)
      if (rc == EVPK_REMAP_BAD_DEPARTURE) call abort_ice('remap transport: bad departure points')
      if (rc == EVPK_REMAP_NEGATIVE_MASS) call abort_ice('remap transport: negative area')
      if (rc == EVPK_RIDGE_STOP .or. rc == EVPK_ITD_STOP) then
         write (nu_diag,*) 'step_dynamics: ', trim(stage(stop(1))), ' stops: reason, iblk, i, j =', stop(2:5)
         if (rc == EVPK_RIDGE_STOP) call abort_ice ('ice: Ridging error')
         call abort_ice ('ice: ITD cleanup error in step_ridge')
      endif
      if (rc /= 0) call abort_ice('step_dynamics: evpk_step_dynamics: '//trim(evpk_error_string(ctx)))
      first_ice = first_i /= 0

      end subroutine evpk_step_dynamics_core

!=======================================================================

! step_radiation for every block, and the albedo lines of coupling_prep, in one library call.
!
! In the reference's ice_step (drivers/auscom/CICE_RunMod.F90) the loop `call step_radiation (dt, iblk)` and, in coupling_prep, the
! albedo aggregation (:503-548 without the albcnt, albpnd and apeff_ai lines), the four _ai copies (:564-567) and the scale_factor
! line (:582-586) become
!     use ice_step_dyn, only: evpk_step_radiation_core
!     call evpk_step_radiation_core
! over the reference's own module arrays.  alvdr_ai .. alidf_ai are plain copies of the four sums: they are made here on the host.
! This routine only marshals arguments; what the call computes is evpk_step_radiation (include/evpk.h), which refuses
! shortwave = 'dEdd', calc_Tsfc = .false. and the zero-layer model with its message.

      subroutine evpk_step_radiation_core

      use ice_constants, only: puny, albocn, awtvdr, awtidr, awtvdf, awtidf
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr
      use ice_dyn_evp, only: evpk_context
      use ice_exit, only: abort_ice
      use ice_flux, only: swvdr, swvdf, swidr, swidf, coszen, alvdr, alidr, alvdf, alidf, albice, albsno, scale_factor, &
          alvdr_ai, alidr_ai, alvdf_ai, alidf_ai
      use ice_shortwave, only: shortwave, albedo_type, albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, &
          alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, fswsfcn, fswintn, fswthrun, fswpenln, Sswabsn, Iswabsn
#ifdef AusCOM
      use ice_shortwave, only: ocn_albedo2D
#endif
      use ice_state, only: aicen, vicen, vsnon, trcrn, ntrcr, nt_Tsfc
      use ice_therm_shared, only: heat_capacity, calc_Tsfc

      type (evpk_rad_args) :: a
      type (c_ptr) :: ctx
      integer (c_int) :: rc

      ctx = evpk_context ()
      if (.not. c_associated(ctx)) call abort_ice('step_radiation: no context on the device: evp has not run yet')

      a%shortwave_dEdd = merge(1_c_int32_t, 0_c_int32_t, trim(shortwave) == 'dEdd')
      a%calc_Tsfc = merge(1_c_int32_t, 0_c_int32_t, calc_Tsfc)
      a%heat_capacity = merge(1_c_int32_t, 0_c_int32_t, heat_capacity)
      a%albedo_constant = merge(1_c_int32_t, 0_c_int32_t, trim(albedo_type) == 'constant')
      a%ncat = int(ncat, c_int32_t)
      a%ntrcr = int(ntrcr, c_int32_t)
      a%ntrcr_dim = int(max_ntrcr, c_int32_t)
      a%t%nt_Tsfc = int(nt_Tsfc, c_int32_t);  a%t%nilyr = int(nilyr, c_int32_t);  a%t%nslyr = int(nslyr, c_int32_t)
      a%puny = puny
      a%albicev = albicev;  a%albicei = albicei;  a%albsnowv = albsnowv;  a%albsnowi = albsnowi;  a%ahmax = ahmax
      a%snowpatch = snowpatch;  a%albocn = albocn
      a%awtvdr = awtvdr;  a%awtidr = awtidr;  a%awtvdf = awtvdf;  a%awtidf = awtidf

      a%aicen = loc_r8(aicen);  a%vicen = loc_r8(vicen);  a%vsnon = loc_r8(vsnon);  a%trcrn = loc_r8(trcrn)
      a%swvdr = loc_r8(swvdr);  a%swvdf = loc_r8(swvdf);  a%swidr = loc_r8(swidr);  a%swidf = loc_r8(swidf)
#ifdef AusCOM
      a%ocn_albedo2D = loc_r8(ocn_albedo2D)
#endif
      a%alvdrn = loc_r8(alvdrn);  a%alidrn = loc_r8(alidrn);  a%alvdfn = loc_r8(alvdfn);  a%alidfn = loc_r8(alidfn)
      a%albicen = loc_r8(albicen);  a%albsnon = loc_r8(albsnon)
      a%fswsfcn = loc_r8(fswsfcn);  a%fswintn = loc_r8(fswintn);  a%fswthrun = loc_r8(fswthrun)
      a%Sswabsn = loc_r8(Sswabsn);  a%Iswabsn = loc_r8(Iswabsn);  a%fswpenln = loc_r8(fswpenln)
      a%coszen = loc_r8(coszen);  a%alvdr = loc_r8(alvdr);  a%alidr = loc_r8(alidr);  a%alvdf = loc_r8(alvdf);  a%alidf = loc_r8(alidf)
      a%albice = loc_r8(albice);  a%albsno = loc_r8(albsno);  a%scale_factor = loc_r8(scale_factor)

      rc = evpk_step_radiation (ctx, a)
      if (rc /= 0) call abort_ice('step_radiation: evpk_step_radiation: '//trim(evpk_error_string(ctx)))
      alvdr_ai = alvdr;  alidr_ai = alidr;  alvdf_ai = alvdf;  alidf_ai = alidf      ! CICE_RunMod.F90:564-567

      end subroutine evpk_step_radiation_core

!=======================================================================

! step_radiation with shortwave = 'dEdd' for every block, and the albedo lines of coupling_prep, in one library call.
!
! As evpk_step_radiation_core, for a host whose ice_in selects the Delta-Eddington scheme: the loop `call step_radiation (dt, iblk)`
! and, in coupling_prep, the albedo aggregation (:503-548 without the albcnt lines), the four _ai copies (:564-567) and the
! scale_factor line (:582-586) become
!     use ice_step_dyn, only: evpk_step_radiation_dedd_core
!     call evpk_step_radiation_dedd_core
! The cosine of the zenith angle stays on the host: compute_coszen (shr_orb_decl, the libm sin and cos of ice_orbital.F90:130-132) runs
! here over the tmask cells of every block, as run_dEdd does at :1385-1402, and the library stores max(puny, coszen) back on the listed,
! lit cells.  This routine only marshals arguments; what the call computes is evpk_step_radiation_dedd (include/evpk.h), which refuses
! tr_pond_lvl, tr_pond_topo, tr_aero, calc_Tsfc = .false. and the zero-layer model with its message.

      subroutine evpk_step_radiation_dedd_core

      use ice_dyn_evp, only: evpk_context
      use ice_exit, only: abort_ice
      use ice_flux, only: alvdr, alidr, alvdf, alidf, alvdr_ai, alidr_ai, alvdf_ai, alidf_ai

      type (evpk_dedd_args) :: a
      type (c_ptr) :: ctx
      integer (c_int) :: rc

      ctx = evpk_context ()
      if (.not. c_associated(ctx)) call abort_ice('step_radiation: no context on the device: evp has not run yet')
      call dedd_marshal (a)
      rc = evpk_step_radiation_dedd (ctx, a)
      if (rc /= 0) call abort_ice('step_radiation: evpk_step_radiation_dedd: '//trim(evpk_error_string(ctx)))
      alvdr_ai = alvdr;  alidr_ai = alidr;  alvdf_ai = alvdf;  alidf_ai = alidf      ! CICE_RunMod.F90:564-567

      end subroutine evpk_step_radiation_dedd_core

!=======================================================================

! The same under tr_pond_lvl (the scheme the shipped ice_in select beside shortwave = 'dEdd'): the level-ice block of run_dEdd
! (ice_shortwave.F90:1450-1514) on dhsn and ffracn of ice_meltpond_lvl, fsnow of ice_flux, nt_alvl, nt_ipnd, hs1.  initonly is run_dEdd's
! (init_shortwave passes .true.: dhsn then stays as it is).  What the call computes is evpk_step_radiation_dedd_lvl (include/evpk.h).

      subroutine evpk_step_radiation_dedd_lvl_core (initonly)

      use ice_calendar, only: dt
      use ice_dyn_evp, only: evpk_context
      use ice_exit, only: abort_ice
      use ice_flux, only: alvdr, alidr, alvdf, alidf, alvdr_ai, alidr_ai, alvdf_ai, alidf_ai, fsnow
      use ice_meltpond_lvl, only: dhsn, ffracn, hs1
      use ice_state, only: nt_alvl, nt_apnd, nt_hpnd, nt_ipnd

      logical (kind=log_kind), intent(in), optional :: initonly

      type (evpk_dedd_args) :: a
      type (evpk_pond_lvl_args) :: p
      type (c_ptr) :: ctx
      integer (c_int) :: rc

      ctx = evpk_context ()
      if (.not. c_associated(ctx)) call abort_ice('step_radiation: no context on the device: evp has not run yet')
      call dedd_marshal (a)
      a%t%nt_alvl = int(nt_alvl, c_int32_t);  a%t%nt_apnd = int(nt_apnd, c_int32_t);  a%t%nt_hpnd = int(nt_hpnd, c_int32_t)
      p%nt_ipnd = int(nt_ipnd, c_int32_t)
      p%hs1 = hs1;  p%dt = dt
      if (present(initonly)) p%linitonly = merge(1_c_int32_t, 0_c_int32_t, initonly)
      p%dhsn = loc_r8(dhsn);  p%ffracn = loc_r8(ffracn);  p%fsnow = loc_r8(fsnow)
      rc = evpk_step_radiation_dedd_lvl (ctx, a, p)
      if (rc /= 0) call abort_ice('step_radiation: evpk_step_radiation_dedd_lvl: '//trim(evpk_error_string(ctx)))
      alvdr_ai = alvdr;  alidr_ai = alidr;  alvdf_ai = alvdf;  alidf_ai = alidf      ! CICE_RunMod.F90:564-567

      end subroutine evpk_step_radiation_dedd_lvl_core

!=======================================================================

! compute_coszen on the host and the arguments both Delta-Eddington calls share

      subroutine dedd_marshal (a)

      use ice_blocks, only: nx_block, ny_block
      use ice_calendar, only: dt
      use ice_constants, only: puny, awtvdr, awtidr, awtvdf, awtidf
      use ice_domain, only: nblocks
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr
      use ice_flux, only: swvdr, swvdf, swidr, swidf, coszen, alvdr, alidr, alvdf, alidf, albice, albsno, albpnd, apeff_ai, &
          scale_factor
      use ice_grid, only: tmask, tlat, tlon
      use ice_meltpond_cesm, only: hs0
      use ice_meltpond_lvl, only: pndaspect
      use ice_orbital, only: compute_coszen
      use ice_shortwave, only: R_ice, R_pnd, R_snw, dT_mlt, rsnw_mlt, kalg, &
          alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, albpndn, apeffn, snowfracn, fswsfcn, fswintn, fswthrun, fswpenln, &
          Sswabsn, Iswabsn
      use ice_state, only: aicen, vicen, vsnon, trcrn, ntrcr, nt_Tsfc, nt_apnd, nt_hpnd, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero
      use ice_therm_shared, only: heat_capacity, calc_Tsfc

      type (evpk_dedd_args), intent(inout) :: a
      integer (kind=int_kind) :: iblk, i, j, icells
      integer (kind=int_kind), dimension (nx_block*ny_block) :: indxi, indxj

      do iblk = 1, nblocks                                   ! ice_shortwave.F90:1385-1402
         icells = 0
         do j = 1, ny_block
         do i = 1, nx_block
            if (tmask(i,j,iblk)) then
               icells = icells + 1
               indxi(icells) = i
               indxj(icells) = j
            endif
         enddo
         enddo
         call compute_coszen (nx_block, ny_block, icells, indxi, indxj, tlat(:,:,iblk), tlon(:,:,iblk), coszen(:,:,iblk), dt)
      enddo

      a%calc_Tsfc = merge(1_c_int32_t, 0_c_int32_t, calc_Tsfc)
      a%heat_capacity = merge(1_c_int32_t, 0_c_int32_t, heat_capacity)
      a%tr_pond_cesm = merge(1_c_int32_t, 0_c_int32_t, tr_pond_cesm)
      a%tr_pond_lvl = merge(1_c_int32_t, 0_c_int32_t, tr_pond_lvl)
      a%tr_pond_topo = merge(1_c_int32_t, 0_c_int32_t, tr_pond_topo)
      a%tr_aero = merge(1_c_int32_t, 0_c_int32_t, tr_aero)
      a%ncat = int(ncat, c_int32_t)
      a%ntrcr = int(ntrcr, c_int32_t)
      a%ntrcr_dim = int(max_ntrcr, c_int32_t)
      a%t%nt_Tsfc = int(nt_Tsfc, c_int32_t);  a%t%nilyr = int(nilyr, c_int32_t);  a%t%nslyr = int(nslyr, c_int32_t)
      if (tr_pond_cesm) then
         a%t%nt_apnd = int(nt_apnd, c_int32_t);  a%t%nt_hpnd = int(nt_hpnd, c_int32_t)
      endif
      a%puny = puny
      a%R_ice = R_ice;  a%R_pnd = R_pnd;  a%R_snw = R_snw;  a%dT_mlt = dT_mlt;  a%rsnw_mlt = rsnw_mlt;  a%kalg = kalg
      a%hs0 = hs0;  a%pndaspect = pndaspect
      a%awtvdr = awtvdr;  a%awtidr = awtidr;  a%awtvdf = awtvdf;  a%awtidf = awtidf

      a%aicen = loc_r8(aicen);  a%vicen = loc_r8(vicen);  a%vsnon = loc_r8(vsnon);  a%trcrn = loc_r8(trcrn)
      a%swvdr = loc_r8(swvdr);  a%swvdf = loc_r8(swvdf);  a%swidr = loc_r8(swidr);  a%swidf = loc_r8(swidf)
      a%coszen = loc_r8(coszen)
      a%alvdrn = loc_r8(alvdrn);  a%alidrn = loc_r8(alidrn);  a%alvdfn = loc_r8(alvdfn);  a%alidfn = loc_r8(alidfn)
      a%albicen = loc_r8(albicen);  a%albsnon = loc_r8(albsnon)
      a%fswsfcn = loc_r8(fswsfcn);  a%fswintn = loc_r8(fswintn);  a%fswthrun = loc_r8(fswthrun)
      a%Sswabsn = loc_r8(Sswabsn);  a%Iswabsn = loc_r8(Iswabsn);  a%fswpenln = loc_r8(fswpenln)
      a%alvdr = loc_r8(alvdr);  a%alidr = loc_r8(alidr);  a%alvdf = loc_r8(alvdf);  a%alidf = loc_r8(alidf)
      a%albice = loc_r8(albice);  a%albsno = loc_r8(albsno);  a%scale_factor = loc_r8(scale_factor)
      a%albpndn = loc_r8(albpndn);  a%apeffn = loc_r8(apeffn);  a%snowfracn = loc_r8(snowfracn)
      a%albpnd = loc_r8(albpnd);  a%apeff_ai = loc_r8(apeff_ai)

      end subroutine dedd_marshal

!=======================================================================

! step_therm1 under tr_pond_lvl for every block in one library call.
!
! In the reference's ice_step the loop `call step_therm1 (dt, iblk)` becomes
!     use ice_step_dyn, only: evpk_step_therm1_lvl_core
!     call evpk_step_therm1_lvl_core (dt)
! It runs over the reference's own module arrays: the state of ice_state, the forcing and fluxes of ice_flux, the radiation arrays of
! ice_shortwave, Cdn_atm and Cdn_atm_ratio of ice_atmo, and dhsn, ffracn, dpscale, frzpnd, rfracmin, rfracmax, pndaspect of
! ice_meltpond_lvl with Tair and nt_ipnd.  flwoutn, evapn, freshn, fsaltn and fhocnn are 2-D locals of step_therm1; the library wants
! them per category, so this module keeps them.  lmask_n / lmask_s are logical in ice_grid and int32 here.  This routine only marshals
! arguments; what the call computes is evpk_step_therm1_lvl (include/evpk.h), which refuses formdrag, highfreq, atmbndy = 'constant',
! fbot_xfer_type = 'Cdn_ocn', ktherm /= 1, aerosols and the other pond schemes with its message.  The call is not collective.

      subroutine evpk_step_therm1_lvl_core (dt)

      use ice_atmo, only: calc_strair, atmbndy, formdrag, highfreq, natmiter, Cdn_atm, Cdn_atm_ratio
      use ice_blocks, only: nx_block, ny_block
      use ice_calendar, only: yday
      use ice_constants, only: rhos, Lfresh, Tocnfrz, ice_ref_salinity, hs_min, cp_ice, puny
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr, max_blocks
      use ice_dyn_evp, only: evpk_context
      use ice_exit, only: abort_ice
      use ice_fileunits, only: nu_diag
      use ice_flux, only: frzmlt, sst, Tf, strocnxT, strocnyT, rside, meltsn, melttn, meltbn, congeln, snoicen, dsnown, uatm, vatm, &
          wind, rhoa, potT, Qa, zlvl, flatn, fsensn, fsurfn, fcondtopn, flw, fsnow, fpond, sss, mlt_onset, frz_onset, frain, Tair, &
          strairxT, strairyT, fsurf, fcondtop, fsens, flat, fswabs, flwout, evap, Tref, Qref, Uref, fresh, fsalt, fhocn, fswthru, &
          meltt, melts, meltb, congel, snoice
      use ice_grid, only: lmask_n, lmask_s
      use ice_itd, only: hi_min
      use ice_meltpond_lvl, only: ffracn, dhsn, rfracmin, rfracmax, dpscale, pndaspect, frzpnd
      use ice_shortwave, only: fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn
      use ice_state, only: aice, aicen, aice_init, aicen_init, vicen_init, vicen, vsnon, ntrcr, trcrn, nt_Tsfc, nt_qice, nt_qsno, &
          nt_sice, nt_alvl, nt_apnd, nt_hpnd, nt_ipnd, nt_iage, nt_FY, tr_iage, tr_FY, tr_aero, tr_pond_cesm, tr_pond_lvl, tr_pond_topo
      use ice_therm_shared, only: ktherm, calc_Tsfc, heat_capacity, l_brine, conduct, Tmin
      use ice_therm_vertical, only: ustar_min, chio, fbot_xfer_type
      use ice_zbgc_shared, only: min_salin

      real (kind=dbl_kind), intent(in) :: dt                 ! time step

      type (evpk_therm1_args) :: a
      type (evpk_pond_lvl_args) :: p
      type (c_ptr) :: ctx
      integer (c_int) :: rc
      integer (c_int32_t) :: stop(5)

      ctx = evpk_context ()
      if (.not. c_associated(ctx)) call abort_ice('step_therm1: no context on the device: evp has not run yet')

      if (.not. allocated(flwoutn_w)) then
         allocate (flwoutn_w(nx_block,ny_block,ncat,max_blocks), evapn_w(nx_block,ny_block,ncat,max_blocks), &
                   freshn_w(nx_block,ny_block,ncat,max_blocks), fsaltn_w(nx_block,ny_block,ncat,max_blocks), &
                   fhocnn_w(nx_block,ny_block,ncat,max_blocks), lmask_n_w(nx_block,ny_block,max_blocks), &
                   lmask_s_w(nx_block,ny_block,max_blocks))
         lmask_n_w = merge(1_c_int32_t, 0_c_int32_t, lmask_n)
         lmask_s_w = merge(1_c_int32_t, 0_c_int32_t, lmask_s)
      endif

      a%tv%dt = dt;  a%tv%yday = yday
      a%tv%ktherm = int(ktherm, c_int32_t)
      a%tv%calc_Tsfc = merge(1_c_int32_t, 0_c_int32_t, calc_Tsfc)
      a%tv%heat_capacity = merge(1_c_int32_t, 0_c_int32_t, heat_capacity)
      a%tv%l_brine = merge(1_c_int32_t, 0_c_int32_t, l_brine)
      a%tv%conduct = merge(1_c_int32_t, 0_c_int32_t, trim(conduct) == 'bubbly')
      a%tv%min_salin = min_salin
      a%tv%ncat = int(ncat, c_int32_t);  a%tv%ntrcr = int(ntrcr, c_int32_t);  a%tv%ntrcr_dim = int(max_ntrcr, c_int32_t)
      a%tv%t%nt_Tsfc = int(nt_Tsfc, c_int32_t);  a%tv%t%nt_qice = int(nt_qice, c_int32_t);  a%tv%t%nilyr = int(nilyr, c_int32_t)
      a%tv%t%nt_qsno = int(nt_qsno, c_int32_t);  a%tv%t%nslyr = int(nslyr, c_int32_t)
      a%tv%t%nt_alvl = int(nt_alvl, c_int32_t);  a%tv%t%nt_apnd = int(nt_apnd, c_int32_t);  a%tv%t%nt_hpnd = int(nt_hpnd, c_int32_t)
      a%tv%t%tr_pond_cesm = merge(1_c_int32_t, 0_c_int32_t, tr_pond_cesm)
      a%tv%t%tr_pond_lvl = merge(1_c_int32_t, 0_c_int32_t, tr_pond_lvl)
      a%tv%t%tr_pond_topo = merge(1_c_int32_t, 0_c_int32_t, tr_pond_topo)
      a%tv%nt_sice = int(nt_sice, c_int32_t)
      a%tv%k%Tocnfrz = Tocnfrz;  a%tv%k%ice_ref_salinity = ice_ref_salinity;  a%tv%k%hs_min = hs_min;  a%tv%k%cp_ice = cp_ice
      a%tv%k%Lfresh = Lfresh;  a%tv%k%Tmin = Tmin;  a%tv%k%puny = puny
      a%tv%aicen = loc_r8(aicen);  a%tv%vicen = loc_r8(vicen);  a%tv%vsnon = loc_r8(vsnon);  a%tv%trcrn = loc_r8(trcrn)
      a%tv%flw = loc_r8(flw);  a%tv%potT = loc_r8(potT);  a%tv%Qa = loc_r8(Qa);  a%tv%rhoa = loc_r8(rhoa);  a%tv%fsnow = loc_r8(fsnow)
      a%tv%sss = loc_r8(sss)
      a%tv%fswsfcn = loc_r8(fswsfcn);  a%tv%fswintn = loc_r8(fswintn);  a%tv%Sswabsn = loc_r8(Sswabsn);  a%tv%Iswabsn = loc_r8(Iswabsn)
      a%tv%fpond = loc_r8(fpond);  a%tv%mlt_onset = loc_r8(mlt_onset);  a%tv%frz_onset = loc_r8(frz_onset)
      a%tv%flwoutn = c_loc(flwoutn_w);  a%tv%evapn = c_loc(evapn_w);  a%tv%freshn = c_loc(freshn_w);  a%tv%fsaltn = c_loc(fsaltn_w)
      a%tv%fhocnn = c_loc(fhocnn_w)
      a%tv%fsensn = loc_r8(fsensn);  a%tv%flatn = loc_r8(flatn);  a%tv%fsurfn = loc_r8(fsurfn);  a%tv%fcondtopn = loc_r8(fcondtopn)
      a%tv%melttn = loc_r8(melttn);  a%tv%meltsn = loc_r8(meltsn);  a%tv%meltbn = loc_r8(meltbn);  a%tv%congeln = loc_r8(congeln)
      a%tv%snoicen = loc_r8(snoicen);  a%tv%dsnown = loc_r8(dsnown)

      a%aice = loc_r8(aice);  a%frzmlt = loc_r8(frzmlt);  a%sst = loc_r8(sst);  a%Tf = loc_r8(Tf)
      a%strocnxT = loc_r8(strocnxT);  a%strocnyT = loc_r8(strocnyT);  a%uatm = loc_r8(uatm);  a%vatm = loc_r8(vatm)
      a%wind = loc_r8(wind);  a%zlvl = loc_r8(zlvl);  a%frain = loc_r8(frain)
      a%fswthrun = loc_r8(fswthrun)
      a%lmask_n = c_loc(lmask_n_w);  a%lmask_s = c_loc(lmask_s_w)
      a%Cdn_atm = loc_r8(Cdn_atm)
      a%rside = loc_r8(rside);  a%aice_init = loc_r8(aice_init);  a%aicen_init = loc_r8(aicen_init);  a%vicen_init = loc_r8(vicen_init)
      a%strairxT = loc_r8(strairxT);  a%strairyT = loc_r8(strairyT);  a%Cdn_atm_ratio = loc_r8(Cdn_atm_ratio)
      a%fsurf = loc_r8(fsurf);  a%fcondtop = loc_r8(fcondtop);  a%fsens = loc_r8(fsens);  a%flat = loc_r8(flat)
      a%fswabs = loc_r8(fswabs);  a%flwout = loc_r8(flwout);  a%evap = loc_r8(evap)
      a%Tref = loc_r8(Tref);  a%Qref = loc_r8(Qref);  a%Uref = loc_r8(Uref)
      a%fresh = loc_r8(fresh);  a%fsalt = loc_r8(fsalt);  a%fhocn = loc_r8(fhocn);  a%fswthru = loc_r8(fswthru)
      a%meltt = loc_r8(meltt);  a%meltb = loc_r8(meltb);  a%melts = loc_r8(melts);  a%congel = loc_r8(congel);  a%snoice = loc_r8(snoice)
      a%chio = chio;  a%ustar_min = ustar_min;  a%hi_min = hi_min;  a%pndaspect = pndaspect
      a%rfracmin = rfracmin;  a%rfracmax = rfracmax
      a%natmiter = int(natmiter, c_int32_t)
      a%calc_strair = merge(1_c_int32_t, 0_c_int32_t, calc_strair)
      a%tr_iage = merge(1_c_int32_t, 0_c_int32_t, tr_iage);  a%tr_FY = merge(1_c_int32_t, 0_c_int32_t, tr_FY)
      a%nt_iage = int(nt_iage, c_int32_t);  a%nt_FY = int(nt_FY, c_int32_t)
      a%formdrag = merge(1_c_int32_t, 0_c_int32_t, formdrag);  a%highfreq = merge(1_c_int32_t, 0_c_int32_t, highfreq)
      a%atmbndy_constant = merge(1_c_int32_t, 0_c_int32_t, trim(atmbndy) == 'constant')
      a%fbot_xfer_Cdn_ocn = merge(1_c_int32_t, 0_c_int32_t, trim(fbot_xfer_type) == 'Cdn_ocn')
      a%tr_aero = merge(1_c_int32_t, 0_c_int32_t, tr_aero)

      p%dhsn = loc_r8(dhsn);  p%ffracn = loc_r8(ffracn);  p%Tair = loc_r8(Tair)
      p%dpscale = dpscale
      p%frzpnd = merge(1_c_int32_t, 0_c_int32_t, trim(frzpnd) == 'hlid')
      p%nt_ipnd = int(nt_ipnd, c_int32_t)

      rc = evpk_step_therm1_lvl (ctx, a, p, stop)
      if (rc == EVPK_THERMO_STOP) then
         write (nu_diag,*) 'evpk_step_therm1_lvl: vertical thermo error, reason', stop(1), ' local block', stop(2), &
                           ' category', stop(3), ' i, j =', stop(4), stop(5)
         call abort_ice ('ice: Vertical thermo error')
      endif
      if (rc /= 0) call abort_ice('step_therm1: evpk_step_therm1_lvl: '//trim(evpk_error_string(ctx)))

      end subroutine evpk_step_therm1_lvl_core

!=======================================================================

! The reference declares its module arrays without TARGET, so C_LOC cannot be applied to them directly; passed to an
! assumed-size TARGET dummy (sequence association: a contiguous whole array is passed by address, no copy) their address can be
! taken.  The arrays live as long as the run.

      type (c_ptr) function loc_r8 (a)
      real (kind=dbl_kind), dimension (*), intent(in), target :: a
      loc_r8 = c_loc(a)
      end function loc_r8

      end module ice_step_dyn
