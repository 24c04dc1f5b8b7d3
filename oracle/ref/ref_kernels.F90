!=======================================================================
! ref_kernels -- test infrastructure (ours, not reference code): a second driver beside ref_harness.F90, for the routines of
! the SLICE module that oracle/ref/Makefile (target `kernels`) cuts out of the reference's ice_dyn_shared / ice_dyn_evp at
! build time: evp_prep1, evp_prep2, stress, stepu, evp_finish, principal_stress.  It is written from those routines'
! interfaces; it holds no body text of evp().  tests/golden/make_ref_kernels.py turns its dumps into the fixtures
! tests/golden/ref_dyn_*.npz.
!
! Records (int32 tag first; arrays are (nx_block, ny_block) planes, native-endian real64 / int32, logicals as int32 0/1):
!   10  the module scalars set_evp_parameters would set (it reaches ice_grid and is not in the slice) + use_ocnslope
!   11..16  ONE call of evp_prep1 / evp_prep2 / stress / stepu / evp_finish / principal_stress on one block
!   20  the CHAIN on the whole grid, in evp()'s call order, with the reference's own ice_HaloUpdate / ice_HaloUpdate_stress
!       between the calls: evp_prep1 -> icetmask halo -> evp_prep2 -> strength, velocity halo -> ndte x (stress -> stepu ->
!       velocity halo) -> stress fold on tripole grids -> evp_finish.  The T<->U averages (to_ugrid, t2ugrid_vector,
!       u2tgrid_vector) live in ice_grid and cannot be built here: aiu, umass and the U-grid wind stress are INPUTS of the
!       record, and strocnxT / strocnyT leave as evp_finish wrote them (on U points).
! Usage:  ref_kernels <in.bin> <out.bin>   with cice_in.nml (domain_nml) in the working directory.
!=======================================================================
program ref_kernels

   use ice_kinds_mod
   use ice_communicate, only: init_communicate
   use ice_fileunits, only: init_fileunits, nu_diag, ice_stdout
   use ice_domain_size, only: nx_global, ny_global, max_blocks
   use ice_blocks, only: block, get_block, nx_block, ny_block
   use ice_domain, only: init_domain_blocks, init_domain_distribution, nblocks, blocks_ice, halo_info
   use ice_boundary, only: ice_HaloUpdate, ice_HaloUpdate_stress
   use ice_constants, only: field_loc_center, field_loc_NEcorner, field_type_scalar, field_type_vector, dragio, rhow, c0
   use cpl_parameters, only: use_ocnslope
   use ice_dyn_shared          ! the slice: everything is public there

   implicit none

   integer, parameter :: uin = 201, uout = 202, NP = 64
   character (len=512) :: fin, fout
   integer (int_kind) :: op, ilo, ihi, jlo, jhi, ksub, icellt, icellu, irev, islope, nb, n, k, tripole, nsub
   real (dbl_kind) :: dt
   real (dbl_kind), allocatable :: kmtg(:,:), ulatg(:,:)
   real (dbl_kind), allocatable :: p(:,:,:), str(:,:,:)             ! p(:,:,1:NP): the planes of a single-routine record
   integer (int_kind), allocatable :: ip(:,:,:), ix(:,:)
   logical (log_kind), allocatable :: lp(:,:,:)
   ! chain
   real (dbl_kind), allocatable :: c(:,:,:,:), fld2(:,:,:,:), strtmp(:,:,:)
   integer (int_kind), allocatable :: ci(:,:,:,:), cx(:,:,:), cnt(:,:)
   logical (log_kind), allocatable :: cl(:,:,:,:)
   type (block) :: b

   call get_command_argument(1, fin)
   call get_command_argument(2, fout)
   open (uin,  file=trim(fin),  access='stream', form='unformatted', status='old')
   open (uout, file=trim(fout), access='stream', form='unformatted', status='replace')

   call init_communicate
   call init_fileunits
   nu_diag = ice_stdout
   call init_domain_blocks
   allocate (kmtg(nx_global,ny_global), ulatg(nx_global,ny_global))
   read (uin) kmtg
   read (uin) ulatg
   call init_domain_distribution(kmtg, ulatg)
   write (uout) nx_global, ny_global, nx_block, ny_block, max_blocks, nblocks
   do n = 1, nblocks
      b = get_block(blocks_ice(n), n)
      write (uout) b%ilo, b%ihi, b%jlo, b%jhi
   enddo

   allocate (p(nx_block,ny_block,NP), ip(nx_block,ny_block,4), lp(nx_block,ny_block,4), ix(nx_block*ny_block,4), &
             str(nx_block,ny_block,8))

   do
      read (uin) op
      select case (op)
      case (0)
         exit

      case (10)         ! module scalars
         read (uin) ndte, irev, islope
         read (uin) revp, ecci, dtei, dte2T, denom1, arlx1i, brlx, cosw, sinw, dragio
         revised_evp = irev /= 0
         use_ocnslope = islope /= 0
         dragw = dragio * rhow

      case (11)         ! evp_prep1: aice vice vsno strairxT strairyT | tmask  ->  strairx strairy tmass | icetmask
         read (uin) ilo, ihi, jlo, jhi
         read (uin) p(:,:,1:5)
         read (uin) ip(:,:,1)
         lp(:,:,1) = ip(:,:,1) /= 0
         call evp_prep1 (nx_block, ny_block, ilo, ihi, jlo, jhi, p(:,:,1), p(:,:,2), p(:,:,3), lp(:,:,1), &
                         p(:,:,4), p(:,:,5), p(:,:,6), p(:,:,7), p(:,:,8), ip(:,:,2))
         write (uout) p(:,:,6:8)
         write (uout) ip(:,:,2)

      case (12)         ! evp_prep2
         ! in : 1 aiu 2 umass 3 fcor 4 uocn 5 vocn 6 strairx 7 strairy 8 ss_tltx 9 ss_tlty 10 fm 11 strtltx 12 strtlty
         !      13 strocnx 14 strocny 15 strintx 16 strinty 17-28 stressp_1..4 stressm_1..4 stress12_1..4 29 uvel 30 vvel
         !      31 uvel_init 32 vvel_init (intent(out), written on physical cells only: their ghost cells keep the input)
         !      | umask icetmask iceumask
         ! out: 10-32 again, 33 umassdti 34 waterx 35 watery 36 forcex 37 forcey | iceumask, the counts, the four lists
         read (uin) ilo, ihi, jlo, jhi
         read (uin) dt
         read (uin) p(:,:,1:32)
         read (uin) ip(:,:,1:3)
         lp(:,:,1) = ip(:,:,1) /= 0
         lp(:,:,3) = ip(:,:,3) /= 0
         ix = 0
         call evp_prep2 (nx_block, ny_block, ilo, ihi, jlo, jhi, icellt, icellu, ix(:,1), ix(:,2), ix(:,3), ix(:,4), &
                         p(:,:,1), p(:,:,2), p(:,:,33), p(:,:,3), lp(:,:,1), p(:,:,4), p(:,:,5), p(:,:,6), p(:,:,7), &
                         p(:,:,8), p(:,:,9), ip(:,:,2), lp(:,:,3), p(:,:,10), dt, p(:,:,11), p(:,:,12), p(:,:,13), p(:,:,14), &
                         p(:,:,15), p(:,:,16), p(:,:,34), p(:,:,35), p(:,:,36), p(:,:,37), &
                         p(:,:,17), p(:,:,18), p(:,:,19), p(:,:,20), p(:,:,21), p(:,:,22), p(:,:,23), p(:,:,24), &
                         p(:,:,25), p(:,:,26), p(:,:,27), p(:,:,28), p(:,:,31), p(:,:,32), p(:,:,29), p(:,:,30))
         ip(:,:,3) = merge(1, 0, lp(:,:,3))
         write (uout) p(:,:,10:37)
         write (uout) ip(:,:,3)
         write (uout) icellt, icellu
         write (uout) ix

      case (13)         ! stress
         ! in : 1 uvel 2 vvel 3 dxt 4 dyt 5 dxhy 6 dyhx 7 cxp 8 cyp 9 cxm 10 cym 11 tarear 12 tinyarea 13 strength
         !      14-25 the stresses 26 shear 27 divu 28 prs_sig 29 rdg_conv 30 rdg_shear;  out: 14-30, str(:,:,1:8)
         read (uin) ksub, icellt
         read (uin) ix(:,1:2)
         read (uin) p(:,:,1:30)
         call stress (nx_block, ny_block, ksub, icellt, ix(:,1), ix(:,2), p(:,:,1), p(:,:,2), p(:,:,3), p(:,:,4), p(:,:,5), &
                      p(:,:,6), p(:,:,7), p(:,:,8), p(:,:,9), p(:,:,10), p(:,:,11), p(:,:,12), p(:,:,13), &
                      p(:,:,14), p(:,:,15), p(:,:,16), p(:,:,17), p(:,:,18), p(:,:,19), p(:,:,20), p(:,:,21), &
                      p(:,:,22), p(:,:,23), p(:,:,24), p(:,:,25), p(:,:,26), p(:,:,27), p(:,:,28), p(:,:,29), p(:,:,30), str)
         write (uout) p(:,:,14:30)
         write (uout) str

      case (14)         ! stepu
         ! in : 1 Cw 2 aiu 3 uocn 4 vocn 5 waterx 6 watery 7 forcex 8 forcey 9 umassdti 10 fm 11 uarear 12 strocnx
         !      13 strocny 14 strintx 15 strinty 16 uvel_init 17 vvel_init 18 uvel 19 vvel, str;  out: 12-15, 18-19
         read (uin) icellu
         read (uin) ix(:,1:2)
         read (uin) p(:,:,1:19)
         read (uin) str
         call stepu (nx_block, ny_block, icellu, p(:,:,1), ix(:,1), ix(:,2), p(:,:,2), str, p(:,:,3), p(:,:,4), p(:,:,5), &
                     p(:,:,6), p(:,:,7), p(:,:,8), p(:,:,9), p(:,:,10), p(:,:,11), p(:,:,12), p(:,:,13), p(:,:,14), &
                     p(:,:,15), p(:,:,16), p(:,:,17), p(:,:,18), p(:,:,19))
         write (uout) p(:,:,12:15)
         write (uout) p(:,:,18:19)

      case (15)         ! evp_finish
         ! in : 1 Cw 2 uvel 3 vvel 4 uocn 5 vocn 6 aiu 7 fm 8 strintx 9 strinty 10 strairx 11 strairy 12 strocnx 13 strocny
         !      14 strocnxT 15 strocnyT;  out: 12-15
         read (uin) icellu
         read (uin) ix(:,1:2)
         read (uin) p(:,:,1:15)
         call evp_finish (nx_block, ny_block, icellu, p(:,:,1), ix(:,1), ix(:,2), p(:,:,2), p(:,:,3), p(:,:,4), p(:,:,5), &
                          p(:,:,6), p(:,:,7), p(:,:,8), p(:,:,9), p(:,:,10), p(:,:,11), p(:,:,12), p(:,:,13), p(:,:,14), p(:,:,15))
         write (uout) p(:,:,12:15)

      case (16)         ! principal_stress: stressp_1 stressm_1 stress12_1 prs_sig -> sig1 sig2
         read (uin) p(:,:,1:4)
         call principal_stress (nx_block, ny_block, p(:,:,1), p(:,:,2), p(:,:,3), p(:,:,4), p(:,:,5), p(:,:,6))
         write (uout) p(:,:,5:6)

      case (20)         ! the chain, whole grid.  Planes of c(:,:,k,iblk):
         ! in : 1 aice 2 vice 3 vsno 4 strairxT 5 strairyT 6 aiu 7 umass 8 strairx(U) 9 strairy(U) 10 fcor 11 uocn 12 vocn
         !      13 ss_tltx 14 ss_tlty 15 Cw 16 strength 17 dxt 18 dyt 19 dxhy 20 dyhx 21 cxp 22 cyp 23 cxm 24 cym 25 tarear
         !      26 tinyarea 27 uarear 28 fm 29 strtltx 30 strtlty 31 strocnx 32 strocny 33 strintx 34 strinty
         !      35-46 the stresses 47 uvel 48 vvel | tmask umask iceumask
         ! work / out: 49 tmass 50 strairx(T, as evp_prep1 left it) 51 strairy 52 umassdti 53 waterx 54 watery 55 forcex
         !      56 forcey 57 uvel_init 58 vvel_init 59 shear 60 divu 61 prs_sig 62 rdg_conv 63 rdg_shear 64 strocnxT 65 strocnyT
         !      66 sig1 67 sig2 | icetmask
         nb = nblocks
         read (uin) dt, nsub, tripole
         allocate (c(nx_block,ny_block,67,nb), ci(nx_block,ny_block,4,nb), cl(nx_block,ny_block,3,nb), cx(nx_block*ny_block,4,nb), &
                   cnt(2,nb), fld2(nx_block,ny_block,2,nb), strtmp(nx_block,ny_block,8))
         c = c0; cx = 0
         do n = 1, nb
            read (uin) c(:,:,1:48,n)
            read (uin) ci(:,:,1:3,n)
         enddo
         cl = ci(:,:,1:3,:) /= 0
         do n = 1, nb
            b = get_block(blocks_ice(n), n)
            call evp_prep1 (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, c(:,:,1,n), c(:,:,2,n), c(:,:,3,n), cl(:,:,1,n), &
                            c(:,:,4,n), c(:,:,5,n), c(:,:,50,n), c(:,:,51,n), c(:,:,49,n), ci(:,:,4,n))
         enddo
         call halo_i4 (ci, 4)
         do n = 1, nb
            b = get_block(blocks_ice(n), n)
            call evp_prep2 (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, cnt(1,n), cnt(2,n), cx(:,1,n), cx(:,2,n), cx(:,3,n), &
                            cx(:,4,n), c(:,:,6,n), c(:,:,7,n), c(:,:,52,n), c(:,:,10,n), cl(:,:,2,n), c(:,:,11,n), c(:,:,12,n), &
                            c(:,:,8,n), c(:,:,9,n), c(:,:,13,n), c(:,:,14,n), ci(:,:,4,n), cl(:,:,3,n), c(:,:,28,n), dt, &
                            c(:,:,29,n), c(:,:,30,n), c(:,:,31,n), c(:,:,32,n), c(:,:,33,n), c(:,:,34,n), c(:,:,53,n), c(:,:,54,n), &
                            c(:,:,55,n), c(:,:,56,n), c(:,:,35,n), c(:,:,36,n), c(:,:,37,n), c(:,:,38,n), c(:,:,39,n), c(:,:,40,n), &
                            c(:,:,41,n), c(:,:,42,n), c(:,:,43,n), c(:,:,44,n), c(:,:,45,n), c(:,:,46,n), c(:,:,57,n), c(:,:,58,n), &
                            c(:,:,47,n), c(:,:,48,n))
         enddo
         call halo_r8 (c, 16, field_loc_center, field_type_scalar)
         call halo_uv
         do ksub = 1, nsub
            do n = 1, nb
               call stress (nx_block, ny_block, ksub, cnt(1,n), cx(:,1,n), cx(:,2,n), c(:,:,47,n), c(:,:,48,n), c(:,:,17,n), &
                            c(:,:,18,n), c(:,:,19,n), c(:,:,20,n), c(:,:,21,n), c(:,:,22,n), c(:,:,23,n), c(:,:,24,n), c(:,:,25,n), &
                            c(:,:,26,n), c(:,:,16,n), c(:,:,35,n), c(:,:,36,n), c(:,:,37,n), c(:,:,38,n), c(:,:,39,n), c(:,:,40,n), &
                            c(:,:,41,n), c(:,:,42,n), c(:,:,43,n), c(:,:,44,n), c(:,:,45,n), c(:,:,46,n), c(:,:,59,n), c(:,:,60,n), &
                            c(:,:,61,n), c(:,:,62,n), c(:,:,63,n), strtmp)
               call stepu (nx_block, ny_block, cnt(2,n), c(:,:,15,n), cx(:,3,n), cx(:,4,n), c(:,:,6,n), strtmp, c(:,:,11,n), &
                           c(:,:,12,n), c(:,:,53,n), c(:,:,54,n), c(:,:,55,n), c(:,:,56,n), c(:,:,52,n), c(:,:,28,n), c(:,:,27,n), &
                           c(:,:,31,n), c(:,:,32,n), c(:,:,33,n), c(:,:,34,n), c(:,:,57,n), c(:,:,58,n), c(:,:,47,n), c(:,:,48,n))
            enddo
            call halo_uv
         enddo
         if (tripole /= 0) then
            do k = 35, 43, 4          ! stressp, stressm, stress12: (1,3) (3,1) (2,4) (4,2)
               call fold (k, k + 2); call fold (k + 2, k); call fold (k + 1, k + 3); call fold (k + 3, k + 1)
            enddo
         endif
         do n = 1, nb
            call evp_finish (nx_block, ny_block, cnt(2,n), c(:,:,15,n), cx(:,3,n), cx(:,4,n), c(:,:,47,n), c(:,:,48,n), c(:,:,11,n), &
                             c(:,:,12,n), c(:,:,6,n), c(:,:,28,n), c(:,:,33,n), c(:,:,34,n), c(:,:,8,n), c(:,:,9,n), c(:,:,31,n), &
                             c(:,:,32,n), c(:,:,64,n), c(:,:,65,n))
            call principal_stress (nx_block, ny_block, c(:,:,35,n), c(:,:,39,n), c(:,:,43,n), c(:,:,61,n), c(:,:,66,n), c(:,:,67,n))
         enddo
         ci(:,:,3,:) = merge(1, 0, cl(:,:,3,:))
         do n = 1, nb
            write (uout) c(:,:,28:67,n)
            write (uout) ci(:,:,3:4,n)
            write (uout) cnt(:,n)
         enddo
         deallocate (c, ci, cl, cx, cnt, fld2, strtmp)

      case default
         write (*,*) 'ref_kernels: unknown op ', op
         stop 2
      end select
   enddo

   close (uin)
   close (uout)

contains

   subroutine halo_r8 (a, k, loc, ftype)
      real (dbl_kind), intent(inout) :: a(:,:,:,:)
      integer (int_kind), intent(in) :: k, loc, ftype
      real (dbl_kind), allocatable :: w(:,:,:)
      allocate (w(nx_block,ny_block,nblocks))
      w = a(:,:,k,:)
      call ice_HaloUpdate (w, halo_info, loc, ftype)
      a(:,:,k,:) = w
   end subroutine halo_r8

   subroutine halo_i4 (a, k)
      integer (int_kind), intent(inout) :: a(:,:,:,:)
      integer (int_kind), intent(in) :: k
      integer (int_kind), allocatable :: w(:,:,:)
      allocate (w(nx_block,ny_block,nblocks))
      w = a(:,:,k,:)
      call ice_HaloUpdate (w, halo_info, field_loc_center, field_type_scalar)
      a(:,:,k,:) = w
   end subroutine halo_i4

   subroutine halo_uv       ! both velocity components in one 3-D update, as the reference's fld2
      fld2(:,:,1,:) = c(:,:,47,:)
      fld2(:,:,2,:) = c(:,:,48,:)
      call ice_HaloUpdate (fld2, halo_info, field_loc_NEcorner, field_type_vector)
      c(:,:,47,:) = fld2(:,:,1,:)
      c(:,:,48,:) = fld2(:,:,2,:)
   end subroutine halo_uv

   subroutine fold (k1, k2)
      integer (int_kind), intent(in) :: k1, k2
      real (dbl_kind), allocatable :: w1(:,:,:), w2(:,:,:)
      allocate (w1(nx_block,ny_block,nblocks), w2(nx_block,ny_block,nblocks))
      w1 = c(:,:,k1,:); w2 = c(:,:,k2,:)
      call ice_HaloUpdate_stress (w1, w2, halo_info, field_loc_center, field_type_scalar)
      c(:,:,k1,:) = w1
   end subroutine fold

end program ref_kernels
