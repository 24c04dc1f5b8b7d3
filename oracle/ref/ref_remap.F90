!=======================================================================
! ref_remap -- test infrastructure (ours, not reference code): a third driver, for the routines of the SLICE module that
! oracle/ref/Makefile (target `kernels`) cuts out of the reference's ice_transport_remap at build time: make_masks,
! construct_fields, limited_gradient, departure_points, locate_triangles, triangle_coordinates, transport_integrals,
! update_fields.  It is written from those routines' interfaces and from the call order of horizontal_remap, which itself
! cannot be built (it reaches ice_grid): that order therefore stays pinned by the restatement alone.
! tests/golden/make_ref_remap.py turns its dumps into the fixtures tests/golden/ref_remap_*.npz.
!
! Records (int32 tag first; arrays native-endian real64 / int32 in Fortran order, logicals as int32 0/1):
!   30  every routine ALONE on one block, each fed what the routine before it returned (no halo update in between: the ghost
!       cells are as the routines leave them):  make_masks; limited_gradient on planes of its own; construct_fields for open
!       water (no tracers) and per category; departure_points; then for edge = east, north: locate_triangles,
!       triangle_coordinates, transport_integrals per category; update_fields per category with its stop flag.
!   31  the CHAIN on the whole grid in horizontal_remap's order, nghost = 1, maskhalo_remap = .false., l_fixed_area = .false.:
!       block loop 1 -> the reference's own ice_HaloUpdate of dpx / dpy (NE corner, vector), mc (centre, scalar), mx / my
!       (centre, vector), tc (scalar), tx / ty (vector) -> block loop 2.  Leaves mm, tm and, per block and edge, the compressed
!       triangle lists with iflux, jflux, triarea and the vertices (for the coverage count); or the stop case: 1 bad departure points,
!       2 negative mass, with block, category and istop / jstop.
! Usage:  ref_remap <in.bin> <out.bin>   with cice_in.nml (domain_nml) in the working directory.
!=======================================================================
program ref_remap

   use ice_kinds_mod
   use ice_communicate, only: init_communicate
   use ice_fileunits, only: init_fileunits, nu_diag, ice_stdout
   use ice_domain_size, only: nx_global, ny_global, max_blocks, ncat
   use ice_blocks, only: block, get_block, nx_block, ny_block, nghost
   use ice_domain, only: init_domain_blocks, init_domain_distribution, nblocks, blocks_ice, halo_info
   use ice_boundary, only: ice_HaloUpdate
   use ice_constants, only: field_loc_center, field_loc_NEcorner, field_type_scalar, field_type_vector, c0, c1, c12
   use ice_transport_remap     ! the slice: everything is public there

   implicit none

   integer, parameter :: uin = 201, uout = 202
   character (len=512) :: fin, fout
   character (len=char_len) :: edge
   integer (int_kind) :: op, ilo, ihi, jlo, jhi, nt, iorder, imid, n, ie, nb, ib, rc, sblk, scat, istop, jstop, nn
   real (dbl_kind) :: dt
   logical (log_kind) :: l_stop, midpt
   real (dbl_kind), allocatable :: kmtg(:,:), ulatg(:,:)
   integer (int_kind), allocatable :: ttype(:), dep(:), ihas(:)
   logical (log_kind), allocatable :: has(:)
   ! one block
   real (dbl_kind), allocatable :: mm(:,:,:), tm(:,:,:,:), g(:,:,:), mmask(:,:,:), tmask(:,:,:,:), mc(:,:,:), mx(:,:,:), my(:,:,:), &
                                   tc(:,:,:,:), tx(:,:,:,:), ty(:,:,:,:), dpx(:,:), dpy(:,:), xp(:,:,:,:), yp(:,:,:,:), triarea(:,:,:), &
                                   edgearea(:,:), mflx(:,:,:,:), mtflx(:,:,:,:,:), av(:,:,:), gx(:,:), gy(:,:)
   integer (int_kind), allocatable :: icnc(:), indxinc(:,:), indxjnc(:,:), icng(:), indxing(:,:), indxjng(:,:), iflux(:,:,:), jflux(:,:,:), &
                                      stops(:,:)
   ! chain
   real (dbl_kind), allocatable :: cm(:,:,:,:), ct(:,:,:,:,:), cg(:,:,:,:), cdpx(:,:,:), cdpy(:,:,:), cmc(:,:,:,:), cmx(:,:,:,:), cmy(:,:,:,:), &
                                   ctc(:,:,:,:,:), ctx(:,:,:,:,:), cty(:,:,:,:,:), ctri(:,:,:,:,:), cxy(:,:,:,:,:,:,:)
   integer (int_kind), allocatable :: cicng(:,:,:), cindx(:,:,:,:,:), cflux(:,:,:,:,:,:)
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
   write (uout) nx_global, ny_global, nx_block, ny_block, max_blocks, nblocks, ncat
   do n = 1, nblocks
      b = get_block(blocks_ice(n), n)
      write (uout) b%ilo, b%ihi, b%jlo, b%jhi
   enddo

   nn = nx_block*ny_block
   allocate (av(nx_block,ny_block,4), mmask(nx_block,ny_block,0:ncat), mc(nx_block,ny_block,0:ncat), mx(nx_block,ny_block,0:ncat), &
             my(nx_block,ny_block,0:ncat), dpx(nx_block,ny_block), dpy(nx_block,ny_block), xp(nx_block,ny_block,0:nvert,ngroups), &
             yp(nx_block,ny_block,0:nvert,ngroups), triarea(nx_block,ny_block,ngroups), edgearea(nx_block,ny_block), &
             mflx(nx_block,ny_block,0:ncat,2), gx(nx_block,ny_block), gy(nx_block,ny_block), icnc(0:ncat), indxinc(nn,0:ncat), &
             indxjnc(nn,0:ncat), icng(ngroups), indxing(nn,ngroups), indxjng(nn,ngroups), iflux(nx_block,ny_block,ngroups), &
             jflux(nx_block,ny_block,ngroups), stops(3,0:ncat), mm(nx_block,ny_block,0:ncat))
   av(:,:,1:2) = c0           ! xav, yav, xxav, yyav as init_remap sets them (it reaches ice_grid and is not in the slice)
   av(:,:,3:4) = c1/c12

   do
      read (uin) op
      if (op == 0) exit
      if (op /= 30 .and. op /= 31) then
         write (*,*) 'ref_remap: unknown op ', op
         stop 2
      endif
      if (op == 30) read (uin) ilo, ihi, jlo, jhi
      read (uin) nt, iorder, imid
      read (uin) dt
      midpt = imid /= 0
      allocate (ttype(nt), dep(nt), ihas(nt), has(nt))
      read (uin) ttype, dep, ihas
      has = ihas /= 0
      allocate (tm(nx_block,ny_block,nt,ncat), tmask(nx_block,ny_block,nt,ncat), tc(nx_block,ny_block,nt,ncat), tx(nx_block,ny_block,nt,ncat), &
                ty(nx_block,ny_block,nt,ncat), mtflx(nx_block,ny_block,nt,ncat,2))

      if (op == 30) then
         ! g: 1 hm 2 uvel 3 vvel 4 dxu 5 dyu 6 HTN 7 HTE 8 tarear 9 phi 10 cnx 11 cny
         allocate (g(nx_block,ny_block,11))
         read (uin) mm
         read (uin) tm
         read (uin) g
         call make_masks (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, nt, has, icnc, indxinc, indxjnc, mm, mmask, tm, tmask)
         write (uout) icnc
         write (uout) indxinc, indxjnc
         write (uout) mmask
         write (uout) tmask
         call limited_gradient (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, g(:,:,9), mmask(:,:,1), g(:,:,10), g(:,:,11), gx, gy)
         write (uout) gx, gy
         call construct_fields (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, nt, ttype, dep, has, icnc(0), indxinc(:,0), indxjnc(:,0), &
                                g(:,:,1), av(:,:,1), av(:,:,2), av(:,:,3), av(:,:,4), mm(:,:,0), mc(:,:,0), mx(:,:,0), my(:,:,0), mmask(:,:,0))
         do n = 1, ncat
            call construct_fields (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, nt, ttype, dep, has, icnc(n), indxinc(:,n), indxjnc(:,n), &
                                   g(:,:,1), av(:,:,1), av(:,:,2), av(:,:,3), av(:,:,4), mm(:,:,n), mc(:,:,n), mx(:,:,n), my(:,:,n), &
                                   mmask(:,:,n), tm(:,:,:,n), tc(:,:,:,n), tx(:,:,:,n), ty(:,:,:,n), tmask(:,:,:,n))
         enddo
         write (uout) mc, mx, my
         write (uout) tc, tx, ty
         l_stop = .false.; istop = 0; jstop = 0
         call departure_points (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, dt, g(:,:,2), g(:,:,3), g(:,:,4), g(:,:,5), g(:,:,6), &
                                g(:,:,7), dpx, dpy, midpt, l_stop, istop, jstop)
         write (uout) merge(1, 0, l_stop), istop, jstop
         write (uout) dpx, dpy
         if (.not. l_stop) then
            do ie = 1, 2
               edge = 'east'
               if (ie == 2) edge = 'north'
               edgearea = c0; indxing = 0; indxjng = 0
               call locate_triangles (nx_block, ny_block, ilo, ihi, jlo, jhi, nghost, edge, icng, indxing, indxjng, dpx, dpy, g(:,:,4), &
                                      g(:,:,5), xp, yp, iflux, jflux, triarea, .false., edgearea)
               write (uout) icng
               write (uout) indxing, indxjng
               write (uout) xp, yp
               write (uout) iflux, jflux
               write (uout) triarea, edgearea
               call triangle_coordinates (nx_block, ny_block, iorder, icng, indxing, indxjng, xp, yp)
               write (uout) xp, yp
               call transport_integrals (nx_block, ny_block, nt, icng, indxing, indxjng, ttype, dep, iorder, triarea, iflux, jflux, xp, yp, &
                                         mc(:,:,0), mx(:,:,0), my(:,:,0), mflx(:,:,0,ie))
               do n = 1, ncat
                  call transport_integrals (nx_block, ny_block, nt, icng, indxing, indxjng, ttype, dep, iorder, triarea, iflux, jflux, xp, yp, &
                                            mc(:,:,n), mx(:,:,n), my(:,:,n), mflx(:,:,n,ie), tc(:,:,:,n), tx(:,:,:,n), ty(:,:,:,n), &
                                            mtflx(:,:,:,n,ie))
               enddo
               write (uout) mflx(:,:,:,ie)
               write (uout) mtflx(:,:,:,:,ie)
            enddo
            stops = 0
            l_stop = .false.; istop = 0; jstop = 0
            call update_fields (nx_block, ny_block, ilo, ihi, jlo, jhi, nt, ttype, dep, g(:,:,8), l_stop, istop, jstop, mflx(:,:,0,1), &
                                mflx(:,:,0,2), mm(:,:,0))
            stops(:,0) = (/ merge(1, 0, l_stop), istop, jstop /)
            do n = 1, ncat
               l_stop = .false.; istop = 0; jstop = 0
               call update_fields (nx_block, ny_block, ilo, ihi, jlo, jhi, nt, ttype, dep, g(:,:,8), l_stop, istop, jstop, mflx(:,:,n,1), &
                                   mflx(:,:,n,2), mm(:,:,n), mtflx(:,:,:,n,1), mtflx(:,:,:,n,2), tm(:,:,:,n))
               stops(:,n) = (/ merge(1, 0, l_stop), istop, jstop /)
            enddo
            write (uout) stops
            write (uout) mm
            write (uout) tm
         endif
         deallocate (g)

      else        ! 31: the chain.  cg: 1 hm 2 uvel 3 vvel 4 dxu 5 dyu 6 HTN 7 HTE 8 tarear
         nb = nblocks
         allocate (cm(nx_block,ny_block,0:ncat,nb), ct(nx_block,ny_block,nt,ncat,nb), cg(nx_block,ny_block,8,nb), cdpx(nx_block,ny_block,nb), &
                   cdpy(nx_block,ny_block,nb), cmc(nx_block,ny_block,0:ncat,nb), cmx(nx_block,ny_block,0:ncat,nb), cmy(nx_block,ny_block,0:ncat,nb), &
                   ctc(nx_block,ny_block,nt,ncat,nb), ctx(nx_block,ny_block,nt,ncat,nb), cty(nx_block,ny_block,nt,ncat,nb), &
                   ctri(nx_block,ny_block,ngroups,2,nb), cicng(ngroups,2,nb), cindx(nn,ngroups,2,2,nb), cflux(nx_block,ny_block,ngroups,2,2,nb), &
                   cxy(nx_block,ny_block,0:nvert,ngroups,2,2,nb))
         do ib = 1, nb
            read (uin) cm(:,:,:,ib)
            read (uin) ct(:,:,:,:,ib)
            read (uin) cg(:,:,:,ib)
         enddo
         rc = 0; sblk = 0; scat = -1; istop = 0; jstop = 0
         do ib = 1, nb
            b = get_block(blocks_ice(ib), ib)
            call make_masks (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nghost, nt, has, icnc, indxinc, indxjnc, cm(:,:,:,ib), mmask, &
                             ct(:,:,:,:,ib), tmask)
            call construct_fields (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nghost, nt, ttype, dep, has, icnc(0), indxinc(:,0), &
                                   indxjnc(:,0), cg(:,:,1,ib), av(:,:,1), av(:,:,2), av(:,:,3), av(:,:,4), cm(:,:,0,ib), cmc(:,:,0,ib), &
                                   cmx(:,:,0,ib), cmy(:,:,0,ib), mmask(:,:,0))
            do n = 1, ncat
               call construct_fields (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nghost, nt, ttype, dep, has, icnc(n), indxinc(:,n), &
                                      indxjnc(:,n), cg(:,:,1,ib), av(:,:,1), av(:,:,2), av(:,:,3), av(:,:,4), cm(:,:,n,ib), cmc(:,:,n,ib), &
                                      cmx(:,:,n,ib), cmy(:,:,n,ib), mmask(:,:,n), ct(:,:,:,n,ib), ctc(:,:,:,n,ib), ctx(:,:,:,n,ib), &
                                      cty(:,:,:,n,ib), tmask(:,:,:,n))
            enddo
            l_stop = .false.; istop = 0; jstop = 0
            call departure_points (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nghost, dt, cg(:,:,2,ib), cg(:,:,3,ib), cg(:,:,4,ib), &
                                   cg(:,:,5,ib), cg(:,:,6,ib), cg(:,:,7,ib), cdpx(:,:,ib), cdpy(:,:,ib), midpt, l_stop, istop, jstop)
            if (l_stop) then
               rc = 1; sblk = ib
               exit
            endif
         enddo
         if (rc == 0) then
            call ice_HaloUpdate (cdpx, halo_info, field_loc_NEcorner, field_type_vector)
            call ice_HaloUpdate (cdpy, halo_info, field_loc_NEcorner, field_type_vector)
            call ice_HaloUpdate (cmc, halo_info, field_loc_center, field_type_scalar)
            call ice_HaloUpdate (cmx, halo_info, field_loc_center, field_type_vector)
            call ice_HaloUpdate (cmy, halo_info, field_loc_center, field_type_vector)
            if (nt > 0) then
               call ice_HaloUpdate (ctc, halo_info, field_loc_center, field_type_scalar)
               call ice_HaloUpdate (ctx, halo_info, field_loc_center, field_type_vector)
               call ice_HaloUpdate (cty, halo_info, field_loc_center, field_type_vector)
            endif
            blocks2: do ib = 1, nb
               b = get_block(blocks_ice(ib), ib)
               do ie = 1, 2
                  edge = 'east'
                  if (ie == 2) edge = 'north'
                  edgearea = c0; indxing = 0; indxjng = 0
                  call locate_triangles (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nghost, edge, icng, indxing, indxjng, cdpx(:,:,ib), &
                                         cdpy(:,:,ib), cg(:,:,4,ib), cg(:,:,5,ib), xp, yp, iflux, jflux, triarea, .false., edgearea)
                  cicng(:,ie,ib) = icng; cindx(:,:,1,ie,ib) = indxing; cindx(:,:,2,ie,ib) = indxjng
                  cflux(:,:,:,1,ie,ib) = iflux; cflux(:,:,:,2,ie,ib) = jflux; ctri(:,:,:,ie,ib) = triarea
                  cxy(:,:,:,:,1,ie,ib) = xp; cxy(:,:,:,:,2,ie,ib) = yp
                  call triangle_coordinates (nx_block, ny_block, iorder, icng, indxing, indxjng, xp, yp)
                  call transport_integrals (nx_block, ny_block, nt, icng, indxing, indxjng, ttype, dep, iorder, triarea, iflux, jflux, xp, yp, &
                                            cmc(:,:,0,ib), cmx(:,:,0,ib), cmy(:,:,0,ib), mflx(:,:,0,ie))
                  do n = 1, ncat
                     call transport_integrals (nx_block, ny_block, nt, icng, indxing, indxjng, ttype, dep, iorder, triarea, iflux, jflux, xp, &
                                               yp, cmc(:,:,n,ib), cmx(:,:,n,ib), cmy(:,:,n,ib), mflx(:,:,n,ie), ctc(:,:,:,n,ib), &
                                               ctx(:,:,:,n,ib), cty(:,:,:,n,ib), mtflx(:,:,:,n,ie))
                  enddo
               enddo
               l_stop = .false.; istop = 0; jstop = 0
               call update_fields (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nt, ttype, dep, cg(:,:,8,ib), l_stop, istop, jstop, &
                                   mflx(:,:,0,1), mflx(:,:,0,2), cm(:,:,0,ib))
               if (l_stop) then
                  rc = 2; sblk = ib; scat = 0
                  exit blocks2
               endif
               do n = 1, ncat
                  call update_fields (nx_block, ny_block, b%ilo, b%ihi, b%jlo, b%jhi, nt, ttype, dep, cg(:,:,8,ib), l_stop, istop, jstop, &
                                      mflx(:,:,n,1), mflx(:,:,n,2), cm(:,:,n,ib), mtflx(:,:,:,n,1), mtflx(:,:,:,n,2), ct(:,:,:,n,ib))
                  if (l_stop) then
                     rc = 2; sblk = ib; scat = n
                     exit blocks2
                  endif
               enddo
            enddo blocks2
         endif
         write (uout) rc, sblk, scat, istop, jstop
         if (rc == 0) then
            do ib = 1, nb
               write (uout) cm(:,:,:,ib)
               write (uout) ct(:,:,:,:,ib)
               write (uout) cicng(:,:,ib)
               write (uout) cindx(:,:,:,:,ib)
               write (uout) cflux(:,:,:,:,:,ib)
               write (uout) ctri(:,:,:,:,ib)
               write (uout) cxy(:,:,:,:,:,:,ib)
            enddo
         endif
         deallocate (cm, ct, cg, cdpx, cdpy, cmc, cmx, cmy, ctc, ctx, cty, ctri, cicng, cindx, cflux, cxy)
      endif
      deallocate (ttype, dep, ihas, has, tm, tmask, tc, tx, ty, mtflx)
   enddo

   close (uin)
   close (uout)

end program ref_remap
