!=======================================================================
! ref_ridge -- test infrastructure (ours, not reference code): a driver for the reference's own ridge_ice (ice_mechred), compiled
! unmodified by oracle/ref/Makefile (target ridge).  It is written from ridge_ice's interface and step_ridge's call (ice_step_mod.F90:1272-1305): it
! sets the namelist switches of ice_mechred, hin_max of ice_itd and the tracer indices / flags of ice_state that ridge_shift and
! compute_tracers read, builds step_ridge's cell list (physical cells with tmask) and calls ridge_ice block by block with every
! optional argument.  tests/golden/make_ref_ridge.py turns its dumps into the fixtures tests/golden/ref_ridge_*.npz.
!
! Input (stream, native-endian; int32 / real64; logicals as int32 0/1), any number of cases, ended by ncase = 0:
!   1 (a case follows) | nblocks ntrcr krdg_partic krdg_redist ndtd | dt mu_rdg | hin_max(0:ncat) | trcr_depend(ntrcr)
!   | nt_qsno nt_alvl nt_vlvl nt_apnd nt_hpnd nt_fbri tr_pond_cesm tr_pond_lvl tr_pond_topo
!   per block: ilo ihi jlo jhi | tmask | rdg_conv rdg_shear aice0 | aicen vicen vsnon | trcrn(nx,ny,ntrcr,ncat)
!              | d2(:,:,1:7) = dardg1dt dardg2dt dvirdgdt opening fpond fresh fhocn
!              | d3(:,:,:,1:9) = dardg1ndt dardg2ndt dvirdgndt aparticn krdgn araftn vraftn aredistn vredistn
! Output per block: l_stop istop jstop icells | aice0 | aicen vicen vsnon | trcrn | d2 | d3
! The reference's own nu_diag text goes to <out>.diag, with a line 'BLOCK n' of ours before each call ("Repeat ridging" is counted
! per block from it).
! Usage:  ref_ridge <in.bin> <out.bin>
!=======================================================================
program ref_ridge

   use ice_kinds_mod
   use ice_fileunits, only: nu_diag
   use ice_domain_size, only: ncat, max_aero
   use ice_blocks, only: nx_block, ny_block
   use ice_itd, only: hin_max
   use ice_mechred, only: ridge_ice, krdg_partic, krdg_redist, mu_rdg
   use ice_state, only: nt_Tsfc, nt_qice, nt_qsno, nt_sice, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_ipnd, nt_aero, nt_fbri, &
                        tr_lvl, tr_pond, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero, tr_brine

   implicit none

   integer, parameter :: uin = 201, uout = 202, udiag = 203
   character (len=512) :: fin, fout
   integer (int_kind) :: more, nblocks, ntrcr, ndtd, ilo, ihi, jlo, jhi, n, i, j, icells, istop, jstop, ic, il, it
   integer (int_kind) :: idx(9)
   real (dbl_kind) :: dt
   logical (log_kind) :: l_stop
   integer (int_kind), allocatable :: tm(:,:), indxi(:), indxj(:), dep(:)
   real (dbl_kind), allocatable :: p(:,:,:), a(:,:,:), v(:,:,:), s(:,:,:), t(:,:,:,:), d2(:,:,:), d3(:,:,:,:), faero(:,:,:)

   call get_command_argument(1, fin)
   call get_command_argument(2, fout)
   open (uin,  file=trim(fin),  access='stream', form='unformatted', status='old')
   open (uout, file=trim(fout), access='stream', form='unformatted', status='replace')
   open (udiag, file=trim(fout)//'.diag', form='formatted', status='replace')
   nu_diag = udiag

   allocate (tm(nx_block,ny_block), indxi(nx_block*ny_block), indxj(nx_block*ny_block), p(nx_block,ny_block,3), &
             a(nx_block,ny_block,ncat), v(nx_block,ny_block,ncat), s(nx_block,ny_block,ncat), d2(nx_block,ny_block,7), &
             d3(nx_block,ny_block,ncat,9), faero(nx_block,ny_block,max_aero))
   write (uout) nx_block, ny_block, ncat

   do
      read (uin) more
      if (more == 0) exit
      read (uin) nblocks, ntrcr, ic, il, ndtd
      krdg_partic = ic
      krdg_redist = il
      read (uin) dt, mu_rdg
      read (uin) hin_max
      allocate (dep(ntrcr), t(nx_block,ny_block,ntrcr,ncat))
      read (uin) dep
      read (uin) idx
      nt_Tsfc = 0; nt_qice = 0; nt_sice = 0; nt_ipnd = 0; nt_aero = 0       ! not read by ridge_ice with these flags
      nt_qsno = idx(1); nt_alvl = idx(2); nt_vlvl = idx(3); nt_apnd = idx(4); nt_hpnd = idx(5); nt_fbri = idx(6)
      tr_pond_cesm = idx(7) /= 0; tr_pond_lvl = idx(8) /= 0; tr_pond_topo = idx(9) /= 0
      tr_pond = tr_pond_cesm .or. tr_pond_lvl .or. tr_pond_topo
      tr_lvl = nt_alvl > 0
      tr_brine = nt_fbri > 0
      tr_aero = .false.
      write (nu_diag,*) 'CASE'
      do n = 1, nblocks
         read (uin) ilo, ihi, jlo, jhi
         read (uin) tm
         read (uin) p
         read (uin) a, v, s
         read (uin) t
         read (uin) d2
         read (uin) d3
         icells = 0                              ! step_ridge's list (ice_step_mod.F90:1272-1281)
         do j = jlo, jhi
         do i = ilo, ihi
            if (tm(i,j) /= 0) then
               icells = icells + 1
               indxi(icells) = i
               indxj(icells) = j
            endif
         enddo
         enddo
         l_stop = .false.; istop = 0; jstop = 0
         faero = 0.0_dbl_kind
         write (nu_diag,*) 'BLOCK', n
         if (icells > 0) then
            call ridge_ice (nx_block, ny_block, dt, ndtd, ntrcr, icells, indxi, indxj, p(:,:,1), p(:,:,2), a, t, v, s, p(:,:,3), &
                            dep, l_stop, istop, jstop, d2(:,:,1), d2(:,:,2), d2(:,:,3), d2(:,:,4), d2(:,:,5), d2(:,:,6), d2(:,:,7), &
                            faero, d3(:,:,:,4), d3(:,:,:,5), d3(:,:,:,8), d3(:,:,:,9), d3(:,:,:,1), d3(:,:,:,2), d3(:,:,:,3), &
                            d3(:,:,:,6), d3(:,:,:,7))
         endif
         write (uout) merge(1, 0, l_stop), istop, jstop, icells
         write (uout) p(:,:,3)
         write (uout) a, v, s
         write (uout) t
         write (uout) d2
         write (uout) d3
      enddo
      deallocate (dep, t)
   enddo

   close (uin)
   close (uout)
   close (udiag)

end program ref_ridge
