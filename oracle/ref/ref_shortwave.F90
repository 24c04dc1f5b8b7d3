!=======================================================================
! ref_shortwave -- test infrastructure (ours, not reference code): a driver for the reference's own shortwave_ccsm3 (with compute_albedos,
! constant_albedos, absorbed_solar), run_dEdd (with compute_coszen of ice_orbital, shortwave_dEdd_set_snow / _set_pond, shortwave_dEdd,
! compute_dEdd, solution_dEdd) and compute_ponds_lvl (with brine_permeability), compiled by oracle/ref/Makefile (target shortwave) from a
! guarded slice of ice_shortwave and of ice_meltpond_lvl and from ice_orbital / shr_orb_mod whole.  It is written from the interfaces of those
! routines and from their calls in step_radiation (ice_step_mod.F90:1364-1524) and step_therm1 (:623-642): the domain is set up as in
! ref_therm2.F90, and per case the module variables the routines read are set from the input -- the namelist scalars of ice_shortwave
! (which the slice's private -> public rewrite makes reachable with ocn_albedo2D and exp_min), hs0, hp1, hs1, pndaspect of the pond modules,
! ntrcr, the nt_* indices and tr_pond_* of ice_state, yday, sec, dt of ice_calendar, heat_capacity, ktherm and l_brine of ice_therm_shared.
!
! A mode word selects what runs, block by block:
!   1 (C)  step_radiation on its calc_Tsfc / not-dEdd branch: the zeroing of :1408-1423, then shortwave_ccsm3
!   2 (D)  init_orbit (once), the zeroing, compute_coszen on the tmask list by itself (cz0: the cosine run_dEdd starts from, before
!          shortwave_dEdd raises it to puny on the lit cells it lists), then run_dEdd, with initonly absent, .false. or .true.
!   3 (P)  compute_ponds_lvl per category as step_therm1 calls it, with rfrac = rfracmin + (rfracmax - rfracmin) aicen of :624
!   4 (O)  init_orbit and shr_orb_decl alone: the declination of (yday, sec), from which the generator places its cells
! Behind modes 1 and 2 the driver RESTATES the albedo lines of coupling_prep (drivers/auscom/CICE_RunMod.F90:503-548, :582-586) on the
! category arrays the reference wrote: that aggregation, the call order and the zeroing are this driver's and stay formally unpinned.
! Arrays the reference does not zero before it writes them (albicen, albsnon, albpndn, apeffn, snowfracn, coszen) start from -9.
!
! Input (stream, native-endian; int32 / real64): KMTG, ULATG (nx_global, ny_global), then any number of cases, ended by 0:
!   mode | [4: yday, sec and no more]
!   ntrcr | nt_Tsfc nt_qice nt_sice nt_alvl nt_apnd nt_hpnd nt_ipnd tr_pond_cesm tr_pond_lvl tr_pond_topo
!   | tmask (nx,ny,nblocks) | aicen vicen vsnon (nx,ny,ncat,max_blocks) | trcrn (nx,ny,max_ntrcr,ncat,max_blocks)
!   1: swvdr swvdf swidr swidf ocn_albedo2D (nx,ny,max_blocks each) | albedo_type (0 default, 1 constant)
!      | albicev albicei albsnowv albsnowi ahmax snowpatch dalb_mlt awtvdr awtidr awtvdf awtidf (variables of the AusCOM ice_constants)
!   2: swvdr swvdf swidr swidf tlat tlon fsnow (nx,ny,max_blocks each) | dhsn ffracn (nx,ny,ncat,max_blocks) | sec initonly (-1 absent, 0, 1)
!      | R_ice R_pnd R_snw dT_mlt rsnw_mlt kalg hs0 hp1 hs1 pndaspect dt yday awtvdr awtidr awtvdf awtidf
!   3: frain Tair (nx,ny,max_blocks) | melttn meltsn fsurfn dhsn (nx,ny,ncat,max_blocks) | frzpnd (0 cesm, 1 hlid)
!      | dt hi_min dpscale pndaspect rfracmin rfracmax
! Output: nx_block ny_block ncat max_ntrcr max_blocks nblocks nilyr nslyr | per block ilo ihi jlo jhi
!   | rhos rhoi rhow rhofresh puny hs_min Timelt kappav hi_ssl hs_ssl hpmin hp0 gravit viscosity_dyn Lfresh
!     cp_ice cp_ocn depressT kice Tffresh (the reference's compile-time constants), then per case
!   1: the nine category arrays alvdrn alidrn alvdfn alidfn albicen albsnon fswsfcn fswintn fswthrun | Sswabsn Iswabsn fswpenln | coszen
!      alvdr alidr alvdf alidf albice albsno scale_factor
!   2: exp_min delta | cz0 coszen | alvdrn alidrn alvdfn alidfn albicen albsnon fswsfcn fswintn fswthrun albpndn apeffn snowfracn dhsn
!      | Sswabsn Iswabsn fswpenln | alvdr alidr alvdf alidf albice albsno albpnd apeff_ai scale_factor
!   3: trcrn | ffracn
!   4: delta eccf
! Usage:  ref_shortwave <in.bin> <out.bin>   with the namelist file cice_in.nml (domain_nml) in the working directory.
!=======================================================================
program ref_shortwave

   use ice_kinds_mod
   use ice_communicate, only: init_communicate
   use ice_fileunits, only: init_fileunits, nu_diag
   use ice_domain_size, only: nx_global, ny_global, max_blocks, ncat, max_ntrcr, nilyr, nslyr
   use ice_blocks, only: block, get_block, nx_block, ny_block
   use ice_domain, only: init_domain_blocks, init_domain_distribution, nblocks, blocks_ice
   use ice_calendar, only: yday, sec, dt_cal => dt
   use ice_constants
   use ice_therm_shared, only: heat_capacity, ktherm, l_brine
   use ice_diagnostics, only: print_points
   use ice_state, only: ntrcr, nt_Tsfc, nt_qice, nt_sice, nt_alvl, nt_apnd, nt_hpnd, nt_ipnd, nt_aero, tr_aero, tr_pond, tr_pond_cesm, &
                        tr_pond_lvl, tr_pond_topo
   use ice_meltpond_cesm, only: hs0
   use ice_meltpond_topo, only: hp1
   use ice_meltpond_lvl, only: hs1, pndaspect_m => pndaspect, compute_ponds_lvl
   use ice_orbital, only: init_orbit, compute_coszen, eccen, mvelpp, lambm0, obliqr
   use shr_orb_mod, only: shr_orb_decl
   use ice_shortwave, only: shortwave_ccsm3, run_dEdd, albedo_type, albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, dalb_mlt, &
                            R_ice, R_pnd, R_snw, dT_mlt, rsnw_mlt, kalg, hi_ssl, hs_ssl, hpmin, hp0, exp_min, ocn_albedo2D

   implicit none

   integer, parameter :: uin = 201, uout = 202, udiag = 203
   character (len=512) :: fin, fout
   character (len=char_len) :: frzpnd
   integer (int_kind) :: mode, iblk, i, j, n, ilo, ihi, jlo, jhi, idx(10), sw(2), icells, isec, atype
   real (dbl_kind) :: sc(16), delta, eccf, yd, dt, hi_min, dpscale, pndaspect, rfracmin, rfracmax
   logical (log_kind) :: orbit
   type (block) :: b
   real (dbl_kind), allocatable :: kmtg(:,:), ulatg(:,:)
   integer (int_kind), allocatable :: tm(:,:,:), indxi(:), indxj(:)
   logical (log_kind), allocatable :: lm(:,:,:)
   real (dbl_kind), allocatable :: aicen(:,:,:,:), vicen(:,:,:,:), vsnon(:,:,:,:), trcrn(:,:,:,:,:), f(:,:,:,:), c(:,:,:,:,:), &
                                   Ssw(:,:,:,:,:), Isw(:,:,:,:,:), pen(:,:,:,:,:), cz(:,:,:), cz0(:,:,:), agg(:,:,:,:), &
                                   dhsn(:,:,:,:), ffracn(:,:,:,:), flx(:,:,:,:,:), rfrac(:,:)

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

   write (uout) nx_block, ny_block, ncat, max_ntrcr, max_blocks, nblocks, nilyr, nslyr
   do iblk = 1, nblocks
      b = get_block(blocks_ice(iblk), iblk)
      write (uout) b%ilo, b%ihi, b%jlo, b%jhi
   enddo
   write (uout) rhos, rhoi, rhow, rhofresh, puny, hs_min, Timelt, kappav, hi_ssl, hs_ssl, hpmin, hp0, &
                gravit, viscosity_dyn, Lfresh, cp_ice, cp_ocn, depressT, kice, Tffresh

   allocate (tm(nx_block,ny_block,nblocks), lm(nx_block,ny_block,nblocks), indxi(nx_block*ny_block), indxj(nx_block*ny_block), &
             aicen(nx_block,ny_block,ncat,max_blocks), vicen(nx_block,ny_block,ncat,max_blocks), vsnon(nx_block,ny_block,ncat,max_blocks), &
             trcrn(nx_block,ny_block,max_ntrcr,ncat,max_blocks), f(nx_block,ny_block,max_blocks,7), c(nx_block,ny_block,ncat,max_blocks,12), &
             Ssw(nx_block,ny_block,nslyr,ncat,max_blocks), Isw(nx_block,ny_block,nilyr,ncat,max_blocks), &
             pen(nx_block,ny_block,nilyr+1,ncat,max_blocks), cz(nx_block,ny_block,max_blocks), cz0(nx_block,ny_block,max_blocks), &
             agg(nx_block,ny_block,max_blocks,9), dhsn(nx_block,ny_block,ncat,max_blocks), ffracn(nx_block,ny_block,ncat,max_blocks), &
             flx(nx_block,ny_block,ncat,max_blocks,3), rfrac(nx_block,ny_block))

   heat_capacity = .true.
   ktherm = 1
   l_brine = .true.                 ! (init_thermo_vertical's, under heat_capacity with saltmax > min_salin: ice_therm_vertical.F90)
   print_points = .false.
   tr_aero = .false.
   nt_aero = 0
   orbit = .false.
   do
      read (uin) mode
      if (mode == 0) exit
      if (mode == 4) then
         read (uin) yd
         read (uin) isec
         if (.not. orbit) call init_orbit
         orbit = .true.
         call shr_orb_decl (yd + isec/secday, eccen, mvelpp, lambm0, obliqr, delta, eccf)
         write (uout) delta, eccf
         cycle
      endif
      read (uin) ntrcr
      read (uin) idx
      nt_Tsfc = idx(1); nt_qice = idx(2); nt_sice = idx(3); nt_alvl = idx(4); nt_apnd = idx(5); nt_hpnd = idx(6); nt_ipnd = idx(7)
      tr_pond_cesm = idx(8) /= 0; tr_pond_lvl = idx(9) /= 0; tr_pond_topo = idx(10) /= 0
      tr_pond = tr_pond_cesm .or. tr_pond_lvl .or. tr_pond_topo
      if (tr_pond_topo) stop 'ref_shortwave: tr_pond_topo is not driven'
      read (uin) tm
      lm = tm /= 0
      read (uin) aicen, vicen, vsnon
      read (uin) trcrn
      write (nu_diag,*) 'CASE', mode

      if (mode == 1 .or. mode == 2) then
         ! what step_radiation zeroes (ice_step_mod.F90:1408-1423): c 1-4 the albedos, 7-9 fswsfcn fswintn fswthrun; the rest starts from -9
         c = -9.0_dbl_kind
         c(:,:,:,:,1:4) = c0; c(:,:,:,:,7:9) = c0
         pen = c0; Isw = c0; Ssw = c0
         cz = -9.0_dbl_kind; cz0 = -9.0_dbl_kind
      endif

      if (mode == 1) then
         read (uin) f(:,:,:,1:5)
         ocn_albedo2D = f(:,:,:,5)
         read (uin) atype
         albedo_type = 'default'
         if (atype == 1) albedo_type = 'constant'
         read (uin) sc(1:11)
         albicev = sc(1); albicei = sc(2); albsnowv = sc(3); albsnowi = sc(4); ahmax = sc(5); snowpatch = sc(6); dalb_mlt = sc(7)
         awtvdr = sc(8); awtidr = sc(9); awtvdf = sc(10); awtidf = sc(11)
         do iblk = 1, nblocks
            b = get_block(blocks_ice(iblk), iblk)
            call shortwave_ccsm3 (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, aicen(:,:,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), &
                                  trcrn(:,:,nt_Tsfc,:,iblk), f(:,:,iblk,1), f(:,:,iblk,2), f(:,:,iblk,3), f(:,:,iblk,4), &
                                  c(:,:,:,iblk,1), c(:,:,:,iblk,2), c(:,:,:,iblk,3), c(:,:,:,iblk,4), c(:,:,:,iblk,7), c(:,:,:,iblk,8), &
                                  c(:,:,:,iblk,9), pen(:,:,:,:,iblk), Isw(:,:,:,:,iblk), Ssw(:,:,:,:,iblk), c(:,:,:,iblk,5), &
                                  c(:,:,:,iblk,6), cz(:,:,iblk), ocn_albedo2D(:,:,iblk))
            call aggregate (.false.)
         enddo
         write (uout) c(:,:,:,:,1:9)
         write (uout) Ssw, Isw, pen
         write (uout) cz
         write (uout) agg(:,:,:,1:6), agg(:,:,:,9)

      elseif (mode == 2) then
         read (uin) f
         read (uin) dhsn, ffracn
         read (uin) sw
         read (uin) sc
         sec = sw(1)
         R_ice = sc(1); R_pnd = sc(2); R_snw = sc(3); dT_mlt = sc(4); rsnw_mlt = sc(5); kalg = sc(6); hs0 = sc(7); hp1 = sc(8); hs1 = sc(9)
         pndaspect_m = sc(10); dt_cal = sc(11); yday = sc(12)
         awtvdr = sc(13); awtidr = sc(14); awtvdf = sc(15); awtidf = sc(16)
         if (.not. orbit) call init_orbit
         orbit = .true.
         call shr_orb_decl (yday + sec/secday, eccen, mvelpp, lambm0, obliqr, delta, eccf)
         do iblk = 1, nblocks
            b = get_block(blocks_ice(iblk), iblk)
            icells = 0
            do j = 1, ny_block
            do i = 1, nx_block
               if (lm(i,j,iblk)) then
                  icells = icells + 1
                  indxi(icells) = i
                  indxj(icells) = j
               endif
            enddo
            enddo
            call compute_coszen (nx_block, ny_block, icells, indxi, indxj, f(:,:,iblk,5), f(:,:,iblk,6), cz0(:,:,iblk), dt_cal)
            if (sw(2) < 0) then
               call run_dEdd (b%ilo, b%ihi, b%jlo, b%jhi, aicen(:,:,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), trcrn(:,:,:,:,iblk), &
                              f(:,:,iblk,5), f(:,:,iblk,6), lm(:,:,iblk), f(:,:,iblk,1), f(:,:,iblk,2), f(:,:,iblk,3), f(:,:,iblk,4), &
                              cz(:,:,iblk), f(:,:,iblk,7), c(:,:,:,iblk,1), c(:,:,:,iblk,3), c(:,:,:,iblk,2), c(:,:,:,iblk,4), &
                              c(:,:,:,iblk,7), c(:,:,:,iblk,8), c(:,:,:,iblk,9), pen(:,:,:,:,iblk), Ssw(:,:,:,:,iblk), Isw(:,:,:,:,iblk), &
                              c(:,:,:,iblk,5), c(:,:,:,iblk,6), c(:,:,:,iblk,10), c(:,:,:,iblk,11), c(:,:,:,iblk,12), dhsn(:,:,:,iblk), &
                              ffracn(:,:,:,iblk))
            else
               call run_dEdd (b%ilo, b%ihi, b%jlo, b%jhi, aicen(:,:,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), trcrn(:,:,:,:,iblk), &
                              f(:,:,iblk,5), f(:,:,iblk,6), lm(:,:,iblk), f(:,:,iblk,1), f(:,:,iblk,2), f(:,:,iblk,3), f(:,:,iblk,4), &
                              cz(:,:,iblk), f(:,:,iblk,7), c(:,:,:,iblk,1), c(:,:,:,iblk,3), c(:,:,:,iblk,2), c(:,:,:,iblk,4), &
                              c(:,:,:,iblk,7), c(:,:,:,iblk,8), c(:,:,:,iblk,9), pen(:,:,:,:,iblk), Ssw(:,:,:,:,iblk), Isw(:,:,:,:,iblk), &
                              c(:,:,:,iblk,5), c(:,:,:,iblk,6), c(:,:,:,iblk,10), c(:,:,:,iblk,11), c(:,:,:,iblk,12), dhsn(:,:,:,iblk), &
                              ffracn(:,:,:,iblk), initonly = sw(2) /= 0)
            endif
            call aggregate (.true.)
         enddo
         write (uout) exp_min, delta
         write (uout) cz0, cz
         write (uout) c
         write (uout) dhsn
         write (uout) Ssw, Isw, pen
         write (uout) agg

      elseif (mode == 3) then
         read (uin) f(:,:,:,1:2)
         read (uin) flx
         read (uin) dhsn
         read (uin) atype
         frzpnd = 'cesm'
         if (atype == 1) frzpnd = 'hlid'
         read (uin) sc(1:6)
         dt = sc(1); hi_min = sc(2); dpscale = sc(3); pndaspect = sc(4); rfracmin = sc(5); rfracmax = sc(6)
         ffracn = -9.0_dbl_kind
         do iblk = 1, nblocks
            b = get_block(blocks_ice(iblk), iblk)
            ilo = b%ilo; ihi = b%ihi; jlo = b%jlo; jhi = b%jhi
            do n = 1, ncat
               rfrac(:,:) = rfracmin + (rfracmax-rfracmin) * aicen(:,:,n,iblk)
               call compute_ponds_lvl (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, hi_min, dpscale, frzpnd, pndaspect, rfrac, &
                                       flx(:,:,n,iblk,1), flx(:,:,n,iblk,2), f(:,:,iblk,1), f(:,:,iblk,2), flx(:,:,n,iblk,3), &
                                       dhsn(:,:,n,iblk), ffracn(:,:,n,iblk), aicen(:,:,n,iblk), vicen(:,:,n,iblk), vsnon(:,:,n,iblk), &
                                       trcrn(:,:,nt_qice:nt_qice+nilyr-1,n,iblk), trcrn(:,:,nt_sice:nt_sice+nilyr-1,n,iblk), &
                                       trcrn(:,:,nt_Tsfc,n,iblk), trcrn(:,:,nt_alvl,n,iblk), trcrn(:,:,nt_apnd,n,iblk), &
                                       trcrn(:,:,nt_hpnd,n,iblk), trcrn(:,:,nt_ipnd,n,iblk))
            enddo
         enddo
         write (uout) trcrn
         write (uout) ffracn
      else
         stop 'ref_shortwave: unknown mode'
      endif
   enddo

   close (uin)
   close (uout)
   close (udiag)

contains

   ! the albedo lines of coupling_prep on block iblk, restated: agg 1 alvdr 2 alidr 3 alvdf 4 alidf 5 albice 6 albsno 7 albpnd 8 apeff_ai
   ! 9 scale_factor
   subroutine aggregate (ponds)
      logical (log_kind), intent(in) :: ponds
      agg(:,:,iblk,:) = c0
      do n = 1, ncat
      do j = 1, ny_block
      do i = 1, nx_block
         agg(i,j,iblk,3) = agg(i,j,iblk,3) + c(i,j,n,iblk,3)*aicen(i,j,n,iblk)
         agg(i,j,iblk,4) = agg(i,j,iblk,4) + c(i,j,n,iblk,4)*aicen(i,j,n,iblk)
         agg(i,j,iblk,1) = agg(i,j,iblk,1) + c(i,j,n,iblk,1)*aicen(i,j,n,iblk)
         agg(i,j,iblk,2) = agg(i,j,iblk,2) + c(i,j,n,iblk,2)*aicen(i,j,n,iblk)
         if (cz(i,j,iblk) > puny) then
            agg(i,j,iblk,5) = agg(i,j,iblk,5) + c(i,j,n,iblk,5)*aicen(i,j,n,iblk)
            agg(i,j,iblk,6) = agg(i,j,iblk,6) + c(i,j,n,iblk,6)*aicen(i,j,n,iblk)
            if (ponds) agg(i,j,iblk,7) = agg(i,j,iblk,7) + c(i,j,n,iblk,10)*aicen(i,j,n,iblk)
         endif
         if (ponds) agg(i,j,iblk,8) = agg(i,j,iblk,8) + c(i,j,n,iblk,11)*aicen(i,j,n,iblk)
      enddo
      enddo
      enddo
      do j = 1, ny_block
      do i = 1, nx_block
         agg(i,j,iblk,9) = f(i,j,iblk,1)*(c1 - agg(i,j,iblk,1)) + f(i,j,iblk,2)*(c1 - agg(i,j,iblk,3)) &
                         + f(i,j,iblk,3)*(c1 - agg(i,j,iblk,2)) + f(i,j,iblk,4)*(c1 - agg(i,j,iblk,4))
      enddo
      enddo
   end subroutine aggregate

end program ref_shortwave
