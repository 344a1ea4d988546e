!  contribs_fields_driver -- per-feature contributions from the 27 MAPL fields through
!  OHXBoosterPredictContribsFields, into the layout a GridComp export would hand over: one
!  real(c_float), target :: c(im,jm,km,F+1) array, feature f at c_loc(c(1,1,1,f)), the bias last.
!  Links against libohxgb.so only.
!
!  usage: contribs_fields_driver <state.bin> <model file> <out.bin> <k1> <k2> <approximate 0|1> [ntree_limit]
!
!  state.bin: as oh_mock_driver reads it (tests/helpers.py write_state_file); PL (field 2) in Pa, -999.0 missing.
!  out.bin: int32 rc; real32 c(im,jm,km,28), zero outside levels k1..k2.
program contribs_fields_driver
   use, intrinsic :: iso_c_binding
   use ohx_bindings
   implicit none

   integer, parameter :: NF = 27
   real(c_float), parameter :: XX_MISS = -999.0
   logical, parameter :: two_d(NF) = [ .true., .false., .false., .false., .false., .false., .false., .false., .false., &
                                       .false., .false., .false., .false., .false., .false., .false., .false., .false., &
                                       .false., .false., .false., .true., .true., .false., .false., .false., .true. ]
   character(len=1024) :: state_file, model_file, out_file, arg
   integer(c_int32_t) :: im, jm, km, dyn
   real(c_float) :: tropp_min, ohscale
   real(c_float), allocatable, target :: pl(:,:,:), tropp(:,:), f2(:,:,:), f3(:,:,:,:)
   real(c_float), allocatable, target :: c(:,:,:,:)
   type(c_ptr) :: fields(NF), outs(NF + 1), booster
   integer(c_int32_t) :: is2d(NF)
   integer :: f, n2, n3, u, k1, k2, approximate, ntree_limit
   integer(c_int) :: rc, rc2

   if (command_argument_count() < 6) then
      print *, 'usage: contribs_fields_driver <state.bin> <model> <out.bin> <k1> <k2> <approximate> [ntree_limit]'
      stop 2
   end if
   call get_command_argument(1, state_file)
   call get_command_argument(2, model_file)
   call get_command_argument(3, out_file)
   call get_command_argument(4, arg)
   read(arg, *) k1
   call get_command_argument(5, arg)
   read(arg, *) k2
   call get_command_argument(6, arg)
   read(arg, *) approximate
   ntree_limit = 0
   if (command_argument_count() >= 7) then
      call get_command_argument(7, arg)
      read(arg, *) ntree_limit
   end if

   open(newunit=u, file=trim(state_file), access='stream', form='unformatted', status='old', action='read')
   read(u) im, jm, km, dyn, tropp_min, ohscale
   allocate(pl(im,jm,km), tropp(im,jm))
   read(u) pl
   read(u) tropp
   allocate(f2(im,jm,count(two_d)), f3(im,jm,km,NF - count(two_d)))
   n2 = 0
   n3 = 0
   do f = 1, NF
      if (two_d(f)) then
         n2 = n2 + 1
         read(u) f2(:,:,n2)
         fields(f) = c_loc(f2(1,1,n2))
         is2d(f) = 1
      else
         n3 = n3 + 1
         read(u) f3(:,:,:,n3)
         fields(f) = c_loc(f3(1,1,1,n3))
         is2d(f) = 0
      end if
   end do
   close(u)

   allocate(c(im,jm,km,NF + 1))
   c = 0.0
   do f = 1, NF + 1
      outs(f) = c_loc(c(1,1,1,f))
   end do

   rc = XGBoosterCreate(c_null_ptr, 0_c_int64_t, booster)
   if (rc == 0) rc = XGBoosterLoadModel(booster, ohx_c_string(model_file))
   if (rc == 0) rc = OHXBoosterPredictContribsFields(booster, fields, is2d, int(NF, c_int), 1_c_int, int(im, c_int), &
                                                     int(jm, c_int), int(km, c_int), int(k1, c_int), int(k2, c_int), &
                                                     XX_MISS, int(approximate, c_int), int(ntree_limit, c_int), outs)
   if (rc /= 0) print *, 'contribs_fields_driver: ', ohx_last_error()
   rc2 = XGBoosterFree(booster)

   open(newunit=u, file=trim(out_file), access='stream', form='unformatted', status='replace', action='write')
   write(u) int(rc, c_int32_t)
   write(u) c
   close(u)
   if (rc /= 0) stop 1
end program contribs_fields_driver
