!=======================================================================
! ref_therm2 -- test infrastructure (ours, not reference code): a driver for the reference's own linear_itd, add_new_ice, lateral_melt
! (ice_therm_itd, compiled unmodified and whole by oracle/ref/Makefile (target therm2), with fit_line, update_vertical_tracers and the mushy liquidus
! of ice_therm_mushy) and aggregate_area, reduce_area, cleanup_itd (ice_itd).  It is written from the interfaces of those routines and
! from their calls in step_therm2 (ice_step_mod.F90:792-993): the domain is set up as in ref_itd.F90 (init_domain_blocks,
! init_domain_distribution), and per case the tracer indices / flags of ice_state (nt_sice, nt_FY and tr_FY among them), hin_max, hi_min
! and kitd of ice_itd, ktherm and heat_capacity of ice_therm_shared, Tocnfrz, skl_bgc = .false., nbtrcr = 0, tr_aero = .false. and
! istep1 are set from the input.  hin_max is set again from the input before EVERY case: linear_itd overwrites hin_max(ncat) in the
! module (ice_therm_itd.F90:208), and what it leaves there is written out with the case.
!
! A mode word selects what runs, block by block (every stage of a block before the next block, as the reference's block loop does):
!   1 (L)  aggregate_area, the list of physical cells with aice > puny, linear_itd if the list is not empty -- the call
!          evpk_linear_itd makes; the frain line is NOT applied.  One dump.
!   2 (T)  step_therm2 in its order: the frain line on every cell of the block, aggregate_area, [kitd == 1: the aice > puny list and
!          linear_itd if it is not empty]; the tmask list and add_new_ice; lateral_melt and, if ncat == 1, reduce_area; cleanup_itd.
!          Four dumps: after linear_itd, after add_new_ice, after lateral_melt / reduce_area, after cleanup_itd, with
!          l_stop / istop / jstop per block and stage.  A block that stops runs none of its later stages (the reference aborts);
!          the other blocks run on, so that the lowest stopping block can be read off.
! That call order is this driver's and stays formally unpinned, as evp()'s does: step_therm2 itself `use`s ice_flux and ice_grid.
! faero_ocn is a zero array of max_aero planes, flux_bio and ocean_bio have extent 0 (nbtrcr = 0); add_new_ice_bgc is never reached
! (tr_brine must be 0 in mode 2; in mode 1 linear_itd reads tr_brine only inside its compile-time disabled conservation check).
! pop_icediag (cpl_parameters): add_new_ice imports it under AusCOM (ice_therm_itd.F90:1270) and never reads it, nor does any other
! routine driven here, so it keeps the default of drivers/auscom/cpl_parameters.F90 (.false.); the header records it.
! l_conservation_check is the module's compile-time .false. (ice_therm_itd.F90:37).
! tests/golden/make_ref_therm2.py turns the dumps into the fixtures tests/golden/ref_litd_*.npz and ref_therm2_*.npz.
!
! Input (stream, native-endian; int32 / real64; logicals as int32 0/1): KMTG, ULATG (nx_global, ny_global), then any number of cases,
! ended by 0:
!   mode | ntrcr | nt_Tsfc nt_qice nt_qsno nt_sice nt_alvl nt_vlvl nt_apnd nt_hpnd nt_fbri nt_iage nt_FY tr_pond_cesm tr_pond_lvl
!   tr_pond_topo tr_brine | kitd ktherm update_ocn_f | dt Tocnfrz hi_min yday phi_init dSin0_frazil | hin_max(0:ncat)
!   | trcr_depend(ntrcr) | tmask (nx,ny,nblocks) | aicen_init vicen_init aicen vicen vsnon (nx,ny,ncat,max_blocks)
!   | trcrn (nx,ny,max_ntrcr,ncat,max_blocks)
!   | aice0 aice frazil frz_onset meltl fpond fresh fsalt fhocn frain frzmlt Tf sss rside (nx,ny,max_blocks each)
!   | salinz (nx,ny,nilyr+1,max_blocks) | first_ice (nx,ny,ncat,max_blocks)
! Output: nx_block ny_block ncat max_ntrcr max_blocks nblocks nilyr pop_icediag | per block ilo ihi jlo jhi
!   | rhoi rhos rhow Lfresh cp_ice cp_ocn ice_ref_salinity puny hfrazilmin hs_min (the reference's compile-time constants), then per case
!   nstage (1 or 4) | l_stop istop jstop per block and stage (3, nblocks, nstage) | hin_max(ncat) as the case leaves it
!   | per stage: aicen vicen vsnon trcrn | aice0 aice frazil frz_onset meltl fpond fresh fsalt fhocn | first_ice
! The reference's own nu_diag text goes to <out>.diag.
! Usage:  ref_therm2 <in.bin> <out.bin>   with the namelist file cice_in.nml (domain_nml) in the working directory.
!=======================================================================
program ref_therm2

   use ice_kinds_mod
   use ice_communicate, only: init_communicate
   use ice_fileunits, only: init_fileunits, nu_diag
   use ice_domain_size, only: nx_global, ny_global, max_blocks, ncat, max_ntrcr, nilyr, max_aero
   use ice_blocks, only: block, get_block, nx_block, ny_block
   use ice_domain, only: init_domain_blocks, init_domain_distribution, nblocks, blocks_ice
   use ice_calendar, only: istep1
   use ice_constants, only: Tocnfrz, rhoi, rhos, rhow, Lfresh, cp_ice, cp_ocn, ice_ref_salinity, puny, hs_min
   use ice_therm_shared, only: heat_capacity, ktherm, hfrazilmin
   use ice_itd, only: hin_max, hi_min, kitd, cleanup_itd, aggregate_area, reduce_area
   use ice_therm_itd, only: linear_itd, add_new_ice, lateral_melt
   use ice_zbgc_shared, only: skl_bgc
   use cpl_parameters, only: pop_icediag
   use ice_state, only: ntrcr, nbtrcr, nt_Tsfc, nt_qice, nt_qsno, nt_sice, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_ipnd, nt_aero, nt_fbri, &
                        nt_iage, nt_FY, tr_iage, tr_FY, tr_lvl, tr_pond, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero, tr_brine

   implicit none

   integer, parameter :: uin = 201, uout = 202, udiag = 203, nw = 14, nwo = 9
   character (len=512) :: fin, fout
   integer (int_kind) :: mode, iblk, i, j, s, ilo, ihi, jlo, jhi, istop, jstop, idx(15), sw(3), nstage, icells
   real (dbl_kind) :: dt, yday, phi_init, dSin0_frazil, sc(6)
   logical (log_kind) :: l_stop, update_ocn_f, stopped
   type (block) :: b
   real (dbl_kind), allocatable :: kmtg(:,:), ulatg(:,:), hin(:)
   integer (int_kind), allocatable :: tm(:,:,:), dep(:), fi(:,:,:,:), st(:,:,:), indxi(:), indxj(:), sfi(:,:,:,:,:)
   logical (log_kind), allocatable :: lm(:,:,:), first_ice(:,:,:,:)
   real (dbl_kind), allocatable :: aicen_init(:,:,:,:), vicen_init(:,:,:,:), aicen(:,:,:,:), vicen(:,:,:,:), vsnon(:,:,:,:), &
                                   trcrn(:,:,:,:,:), w(:,:,:,:), salinz(:,:,:,:), faero(:,:,:), fbio(:,:,:), obio(:,:,:), &
                                   sa(:,:,:,:,:,:), str(:,:,:,:,:,:), s2(:,:,:,:,:)

   call get_command_argument(1, fin)
   call get_command_argument(2, fout)
   open (uin,  file=trim(fin),  access='stream', form='unformatted', status='old')
   open (uout, file=trim(fout), access='stream', form='unformatted', status='replace')

   call init_communicate
   call init_fileunits
   open (udiag, file=trim(fout)//'.diag', form='formatted', status='replace')
   nu_diag = udiag

   call init_domain_blocks
   allocate (kmtg(nx_global,ny_global), ulatg(nx_global,ny_global))
   read (uin) kmtg
   read (uin) ulatg
   call init_domain_distribution(kmtg, ulatg)

   write (uout) nx_block, ny_block, ncat, max_ntrcr, max_blocks, nblocks, nilyr, merge(1, 0, pop_icediag)
   do iblk = 1, nblocks
      b = get_block(blocks_ice(iblk), iblk)
      write (uout) b%ilo, b%ihi, b%jlo, b%jhi
   enddo
   write (uout) rhoi, rhos, rhow, Lfresh, cp_ice, cp_ocn, ice_ref_salinity, puny, hfrazilmin, hs_min

   allocate (tm(nx_block,ny_block,nblocks), lm(nx_block,ny_block,nblocks), fi(nx_block,ny_block,ncat,max_blocks), &
             first_ice(nx_block,ny_block,ncat,max_blocks), st(3,nblocks,4), hin(0:ncat), indxi(nx_block*ny_block), &
             indxj(nx_block*ny_block), aicen_init(nx_block,ny_block,ncat,max_blocks), vicen_init(nx_block,ny_block,ncat,max_blocks), &
             aicen(nx_block,ny_block,ncat,max_blocks), vicen(nx_block,ny_block,ncat,max_blocks), &
             vsnon(nx_block,ny_block,ncat,max_blocks), trcrn(nx_block,ny_block,max_ntrcr,ncat,max_blocks), &
             w(nx_block,ny_block,max_blocks,nw), salinz(nx_block,ny_block,nilyr+1,max_blocks), faero(nx_block,ny_block,max_aero), &
             fbio(nx_block,ny_block,0), obio(nx_block,ny_block,0), sa(nx_block,ny_block,ncat,max_blocks,3,4), &
             str(nx_block,ny_block,max_ntrcr,ncat,max_blocks,4), s2(nx_block,ny_block,max_blocks,nwo,4), &
             sfi(nx_block,ny_block,ncat,max_blocks,4))

   heat_capacity = .true.
   skl_bgc = .false.
   istep1 = 0
   nbtrcr = 0
   tr_aero = .false.
   do
      read (uin) mode
      if (mode == 0) exit
      read (uin) ntrcr
      read (uin) idx
      nt_Tsfc = idx(1); nt_qice = idx(2); nt_qsno = idx(3); nt_sice = idx(4); nt_alvl = idx(5); nt_vlvl = idx(6); nt_apnd = idx(7)
      nt_hpnd = idx(8); nt_fbri = idx(9); nt_iage = idx(10); nt_FY = idx(11)
      tr_pond_cesm = idx(12) /= 0; tr_pond_lvl = idx(13) /= 0; tr_pond_topo = idx(14) /= 0; tr_brine = idx(15) /= 0
      tr_pond = tr_pond_cesm .or. tr_pond_lvl .or. tr_pond_topo
      tr_lvl = nt_alvl > 0
      tr_iage = nt_iage > 0
      tr_FY = nt_FY > 0
      nt_ipnd = 0; nt_aero = 0                                            ! not read by these routines with these flags
      if (mode == 2 .and. (tr_brine .or. nt_sice <= 0)) stop 'ref_therm2: mode 2 needs nt_sice and tr_brine = 0'
      read (uin) sw
      kitd = sw(1); ktherm = sw(2); update_ocn_f = sw(3) /= 0
      read (uin) sc
      dt = sc(1); Tocnfrz = sc(2); hi_min = sc(3); yday = sc(4); phi_init = sc(5); dSin0_frazil = sc(6)
      read (uin) hin
      hin_max(0:ncat) = hin(0:ncat)
      allocate (dep(ntrcr))
      read (uin) dep
      read (uin) tm
      lm = tm /= 0
      read (uin) aicen_init, vicen_init, aicen, vicen, vsnon
      read (uin) trcrn
      read (uin) w            ! 1 aice0 2 aice 3 frazil 4 frz_onset 5 meltl 6 fpond 7 fresh 8 fsalt 9 fhocn 10 frain 11 frzmlt 12 Tf 13 sss 14 rside
      read (uin) salinz
      read (uin) fi
      first_ice = fi /= 0
      faero = 0.0_dbl_kind
      st = 0
      nstage = merge(1, 4, mode == 1)
      write (nu_diag,*) 'CASE', mode

      do iblk = 1, nblocks
         b = get_block(blocks_ice(iblk), iblk)
         ilo = b%ilo; ihi = b%ihi; jlo = b%jlo; jhi = b%jhi
         write (nu_diag,*) 'BLOCK', iblk
         stopped = .false.

         ! ---- stage 1: [the frain line,] aggregate_area, linear_itd (ice_step_mod.F90:804-871)
         if (mode == 2) then
            do j = 1, ny_block
            do i = 1, nx_block
               w(i,j,iblk,7) = w(i,j,iblk,7) + w(i,j,iblk,10)*w(i,j,iblk,2)
            enddo
            enddo
         endif
         call aggregate_area (nx_block, ny_block, aicen(:,:,:,iblk), w(:,:,iblk,2), w(:,:,iblk,1))
         if (mode == 1 .or. kitd == 1) then
            icells = 0
            do j = jlo, jhi
            do i = ilo, ihi
               if (w(i,j,iblk,2) > puny) then
                  icells = icells + 1
                  indxi(icells) = i
                  indxj(icells) = j
               endif
            enddo
            enddo
            if (icells > 0) then
               call linear_itd (nx_block, ny_block, icells, indxi, indxj, ntrcr, dep, aicen_init(:,:,:,iblk), vicen_init(:,:,:,iblk), &
                                aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), w(:,:,iblk,2), &
                                w(:,:,iblk,1), w(:,:,iblk,6), l_stop, istop, jstop)
               st(1,iblk,1) = merge(1, 0, l_stop); st(2,iblk,1) = istop; st(3,iblk,1) = jstop
               stopped = l_stop
            endif
         endif
         call snap (1)
         if (mode == 1) cycle

         ! ---- stage 2: the tmask list and add_new_ice (:879-914)
         if (.not. stopped) then
            icells = 0
            do j = jlo, jhi
            do i = ilo, ihi
               if (lm(i,j,iblk)) then
                  icells = icells + 1
                  indxi(icells) = i
                  indxj(icells) = j
               endif
            enddo
            enddo
            call add_new_ice (nx_block, ny_block, ntrcr, icells, indxi, indxj, dt, aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), &
                              vicen(:,:,:,iblk), w(:,:,iblk,1), w(:,:,iblk,2), w(:,:,iblk,11), w(:,:,iblk,3), w(:,:,iblk,4), yday, &
                              update_ocn_f, w(:,:,iblk,7), w(:,:,iblk,8), w(:,:,iblk,12), w(:,:,iblk,13), salinz(:,:,:,iblk), phi_init, &
                              dSin0_frazil, nbtrcr, fbio, obio, l_stop, istop, jstop)
            st(1,iblk,2) = merge(1, 0, l_stop); st(2,iblk,2) = istop; st(3,iblk,2) = jstop
            stopped = l_stop
         endif
         call snap (2)

         ! ---- stage 3: lateral_melt, reduce_area (:931-960)
         if (.not. stopped) then
            call lateral_melt (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, w(:,:,iblk,6), w(:,:,iblk,7), w(:,:,iblk,8), w(:,:,iblk,9), &
                               faero, w(:,:,iblk,14), w(:,:,iblk,5), aicen(:,:,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), &
                               trcrn(:,:,:,:,iblk))
            if (ncat == 1) call reduce_area (nx_block, ny_block, ilo, ihi, jlo, jhi, lm(:,:,iblk), aicen(:,:,1,iblk), vicen(:,:,1,iblk), &
                                             aicen_init(:,:,1,iblk), vicen_init(:,:,1,iblk))
         endif
         call snap (3)

         ! ---- stage 4: cleanup_itd (:967-982)
         if (.not. stopped) then
            call cleanup_itd (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, ntrcr, aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), &
                              vicen(:,:,:,iblk), vsnon(:,:,:,iblk), w(:,:,iblk,1), w(:,:,iblk,2), dep, w(:,:,iblk,6), w(:,:,iblk,7), &
                              w(:,:,iblk,8), w(:,:,iblk,9), tr_aero=tr_aero, tr_pond_topo=tr_pond_topo, heat_capacity=heat_capacity, &
                              nbtrcr=nbtrcr, first_ice=first_ice(:,:,:,iblk), l_stop=l_stop, istop=istop, jstop=jstop)
            st(1,iblk,4) = merge(1, 0, l_stop); st(2,iblk,4) = istop; st(3,iblk,4) = jstop
         endif
         call snap (4)
      enddo

      write (uout) nstage
      write (uout) st(:,:,1:nstage)
      write (uout) hin_max(ncat)
      do s = 1, nstage
         write (uout) sa(:,:,:,:,1,s), sa(:,:,:,:,2,s), sa(:,:,:,:,3,s)
         write (uout) str(:,:,:,:,:,s)
         write (uout) s2(:,:,:,:,s)
         write (uout) sfi(:,:,:,:,s)
      enddo
      deallocate (dep)
   enddo

   close (uin)
   close (uout)
   close (udiag)

contains

   subroutine snap (s)                  ! the state of block iblk as stage s leaves it (the other blocks' planes: as read)
      integer (int_kind), intent(in) :: s
      if (iblk == 1) then
         sa(:,:,:,:,1,s) = aicen; sa(:,:,:,:,2,s) = vicen; sa(:,:,:,:,3,s) = vsnon
         str(:,:,:,:,:,s) = trcrn
         s2(:,:,:,:,s) = w(:,:,:,1:nwo)
         sfi(:,:,:,:,s) = merge(1, 0, first_ice)
      endif
      sa(:,:,:,iblk,1,s) = aicen(:,:,:,iblk); sa(:,:,:,iblk,2,s) = vicen(:,:,:,iblk); sa(:,:,:,iblk,3,s) = vsnon(:,:,:,iblk)
      str(:,:,:,:,iblk,s) = trcrn(:,:,:,:,iblk)
      s2(:,:,iblk,:,s) = w(:,:,iblk,1:nwo)
      sfi(:,:,:,iblk,s) = merge(1, 0, first_ice(:,:,:,iblk))
   end subroutine snap

end program ref_therm2
