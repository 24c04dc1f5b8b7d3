!=======================================================================
! ref_itd -- test infrastructure (ours, not reference code): a driver for the reference's own cleanup_itd, aggregate (ice_itd) and
! bound_state (ice_state), compiled unmodified by oracle/ref/Makefile (target itd).  It is written from the interfaces of those routines and from
! their calls in step_ridge (ice_step_mod.F90:1325-1341) and step_dynamics (:1152-1189): the domain is set up as in ref_harness.F90
! (init_domain_blocks, init_domain_distribution -> halo_info), the tracer indices / flags of ice_state, hin_max of ice_itd,
! heat_capacity of ice_therm_shared and Tocnfrz are set from the input, cleanup_itd is called block by block with the block's
! ilo .. jhi, and -- unless a block stopped -- bound_state, then per block aggregate and the three tendency lines follow in
! step_dynamics' order (that call order is this driver's and stays formally unpinned, as evp()'s does).
! tests/golden/make_ref_itd.py turns its dumps into the fixtures tests/golden/ref_itd_*.npz.
!
! Input (stream, native-endian; int32 / real64; logicals as int32 0/1): KMTG, ULATG (nx_global, ny_global), then any number of cases,
! ended by 0:
!   1 | ntrcr | nt_Tsfc nt_qice nt_qsno nt_alvl nt_vlvl nt_apnd nt_hpnd nt_fbri nt_iage tr_pond_cesm tr_pond_lvl tr_pond_topo tr_brine
!   | dt (= dt * ndtd of step_ridge; the tendencies divide by it too)  Tocnfrz | hin_max(0:ncat) | trcr_depend(ntrcr)
!   | tmask(nx,ny,nblocks) | aicen vicen vsnon (nx,ny,ncat,max_blocks) | trcrn (nx,ny,max_ntrcr,ncat,max_blocks)
!   | aice0 aice fpond fresh fsalt fhocn daidtd dvidtd dagedtd (nx,ny,max_blocks each) | first_ice (nx,ny,ncat,max_blocks)
! Output: nx_block ny_block ncat max_ntrcr max_blocks nblocks | per block ilo ihi jlo jhi |, then per case
!   l_stop istop jstop per block (3, nblocks)
!   | after cleanup_itd: aicen vicen vsnon trcrn aice0 aice fpond fresh fsalt fhocn first_ice
!   | chain (1 if it ran) | after the chain: aicen vicen vsnon trcrn aice vice vsno aice0 trcr (nx,ny,max_ntrcr,max_blocks) daidtd dvidtd dagedtd
! The reference's own nu_diag text goes to <out>.diag.
! Usage:  ref_itd <in.bin> <out.bin>   with the namelist file cice_in.nml (domain_nml) in the working directory.
!=======================================================================
program ref_itd

   use ice_kinds_mod
   use ice_communicate, only: init_communicate
   use ice_fileunits, only: init_fileunits, nu_diag
   use ice_domain_size, only: nx_global, ny_global, max_blocks, ncat, max_ntrcr
   use ice_blocks, only: block, get_block, nx_block, ny_block
   use ice_domain, only: init_domain_blocks, init_domain_distribution, nblocks, blocks_ice
   use ice_calendar, only: istep1
   use ice_constants, only: Tocnfrz
   use ice_therm_shared, only: heat_capacity
   use ice_itd, only: hin_max, cleanup_itd, aggregate
   use ice_state, only: bound_state, ntrcr, nbtrcr, nt_Tsfc, nt_qice, nt_qsno, nt_sice, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_ipnd, &
                        nt_aero, nt_fbri, nt_iage, tr_iage, tr_lvl, tr_pond, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero, tr_brine

   implicit none

   integer, parameter :: uin = 201, uout = 202, udiag = 203
   character (len=512) :: fin, fout
   integer (int_kind) :: more, iblk, i, j, ilo, ihi, jlo, jhi, istop, jstop, idx(13), chain
   real (dbl_kind) :: dt
   logical (log_kind) :: l_stop
   type (block) :: b
   real (dbl_kind), allocatable :: kmtg(:,:), ulatg(:,:)
   integer (int_kind), allocatable :: tm(:,:,:), dep(:), fi(:,:,:,:), st(:,:)
   logical (log_kind), allocatable :: lm(:,:,:), first_ice(:,:,:,:)
   real (dbl_kind), allocatable :: aicen(:,:,:,:), vicen(:,:,:,:), vsnon(:,:,:,:), trcrn(:,:,:,:,:), w(:,:,:,:), vice(:,:,:), &
                                   vsno(:,:,:), trcr(:,:,:,:)

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

   write (uout) nx_block, ny_block, ncat, max_ntrcr, max_blocks, nblocks
   do iblk = 1, nblocks
      b = get_block(blocks_ice(iblk), iblk)
      write (uout) b%ilo, b%ihi, b%jlo, b%jhi
   enddo

   allocate (tm(nx_block,ny_block,nblocks), lm(nx_block,ny_block,nblocks), fi(nx_block,ny_block,ncat,max_blocks), &
             first_ice(nx_block,ny_block,ncat,max_blocks), st(3,nblocks), &
             aicen(nx_block,ny_block,ncat,max_blocks), vicen(nx_block,ny_block,ncat,max_blocks), &
             vsnon(nx_block,ny_block,ncat,max_blocks), trcrn(nx_block,ny_block,max_ntrcr,ncat,max_blocks), &
             w(nx_block,ny_block,max_blocks,9), vice(nx_block,ny_block,max_blocks), vsno(nx_block,ny_block,max_blocks), &
             trcr(nx_block,ny_block,max_ntrcr,max_blocks))

   heat_capacity = .true.
   istep1 = 0
   nbtrcr = 0
   do
      read (uin) more
      if (more == 0) exit
      read (uin) ntrcr
      read (uin) idx
      nt_Tsfc = idx(1); nt_qice = idx(2); nt_qsno = idx(3); nt_alvl = idx(4); nt_vlvl = idx(5); nt_apnd = idx(6); nt_hpnd = idx(7)
      nt_fbri = idx(8); nt_iage = idx(9)
      tr_pond_cesm = idx(10) /= 0; tr_pond_lvl = idx(11) /= 0; tr_pond_topo = idx(12) /= 0; tr_brine = idx(13) /= 0
      tr_pond = tr_pond_cesm .or. tr_pond_lvl .or. tr_pond_topo
      tr_lvl = nt_alvl > 0
      tr_iage = nt_iage > 0
      tr_aero = .false.
      nt_sice = 0; nt_ipnd = 0; nt_aero = 0                                ! not read by these routines with these flags
      read (uin) dt, Tocnfrz
      read (uin) hin_max
      allocate (dep(ntrcr))
      read (uin) dep
      read (uin) tm
      lm = tm /= 0
      read (uin) aicen, vicen, vsnon
      read (uin) trcrn
      read (uin) w                  ! 1 aice0, 2 aice, 3 fpond, 4 fresh, 5 fsalt, 6 fhocn, 7 daidtd, 8 dvidtd, 9 dagedtd
      read (uin) fi
      first_ice = fi /= 0
      vice = 0.0_dbl_kind; vsno = 0.0_dbl_kind; trcr = 0.0_dbl_kind
      write (nu_diag,*) 'CASE'

      chain = 1
      do iblk = 1, nblocks                        ! step_ridge (ice_step_mod.F90:1325-1341)
         b = get_block(blocks_ice(iblk), iblk)
         ilo = b%ilo; ihi = b%ihi; jlo = b%jlo; jhi = b%jhi
         write (nu_diag,*) 'BLOCK', iblk
         call cleanup_itd (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, ntrcr, aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), &
                           vicen(:,:,:,iblk), vsnon(:,:,:,iblk), w(:,:,iblk,1), w(:,:,iblk,2), dep, w(:,:,iblk,3), w(:,:,iblk,4), &
                           w(:,:,iblk,5), w(:,:,iblk,6), tr_aero=tr_aero, tr_pond_topo=tr_pond_topo, heat_capacity=heat_capacity, &
                           nbtrcr=nbtrcr, first_ice=first_ice(:,:,:,iblk), l_stop=l_stop, istop=istop, jstop=jstop)
         st(1,iblk) = merge(1, 0, l_stop); st(2,iblk) = istop; st(3,iblk) = jstop
         if (l_stop) chain = 0
      enddo
      write (uout) st
      write (uout) aicen, vicen, vsnon
      write (uout) trcrn
      write (uout) w(:,:,:,1:6)
      fi = merge(1, 0, first_ice)
      write (uout) fi
      write (uout) chain

      if (chain == 1) then                        ! step_dynamics (:1152-1189)
         call bound_state (aicen, trcrn, vicen, vsnon)
         do iblk = 1, nblocks
            call aggregate (nx_block, ny_block, aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), &
                            w(:,:,iblk,2), trcr(:,:,1:ntrcr,iblk), vice(:,:,iblk), vsno(:,:,iblk), w(:,:,iblk,1), lm(:,:,iblk), &
                            ntrcr, dep)
            b = get_block(blocks_ice(iblk), iblk)
            do j = b%jlo, b%jhi
            do i = b%ilo, b%ihi
               w(i,j,iblk,8) = (vice(i,j,iblk) - w(i,j,iblk,8)) / dt
               w(i,j,iblk,7) = (w(i,j,iblk,2) - w(i,j,iblk,7)) / dt
               if (tr_iage) w(i,j,iblk,9) = (trcr(i,j,nt_iage,iblk) - w(i,j,iblk,9)) / dt
            enddo
            enddo
         enddo
         write (uout) aicen, vicen, vsnon
         write (uout) trcrn
         write (uout) w(:,:,:,2), vice, vsno, w(:,:,:,1)
         write (uout) trcr
         write (uout) w(:,:,:,7:9)
      endif
      deallocate (dep)
   enddo

   close (uin)
   close (uout)
   close (udiag)

end program ref_itd
