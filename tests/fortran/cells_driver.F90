!  cells_driver -- the tropospheric cells of one column of a 4 x 3 x 6 block, selected on the GPU through
!  OHXSelectCells (a = PL 3-D, b = TROPP 2-D) and gathered through OHXGatherCells, from Fortran.
!  Links against libohxgb.so only.
!
!  usage: cells_driver <i> <j>
!
!  The fields are small integers, exact in real32, that tests/test_gpu_cells.py builds again in numpy:
!     LAT(i,j)   = 10 i + j                     2-D
!     PL(i,j,k)  = 1000 k k + 37 i + 11 j       3-D, Pa: the field divided by 100
!     T(i,j,k)   = 200 + i + 2 j + 3 k          3-D
!     ALB(i,j)   = i j / 8                      2-D
!     TROPP(i,j) = 9000 + 500 i + 100 j         2-D, Pa
!  Output: "count <n>", then per selected cell "<cell index> <bits of the row's four floats as int32>".
program cells_driver
   use, intrinsic :: iso_c_binding
   use ohx_bindings
   implicit none

   integer, parameter :: IM = 4, JM = 3, KM = 6, NF = 4
   real(c_float), target :: lat(IM,JM), pl(IM,JM,KM), t(IM,JM,KM), alb(IM,JM), tropp(IM,JM)
   real(c_float) :: rows(NF,KM)
   type(c_ptr) :: fields(NF)
   integer(c_int32_t) :: is2d(NF)
   integer(c_int64_t) :: cells(KM), count
   character(len=64) :: arg
   integer :: i, j, k, ic, jc, n, f
   integer(c_int) :: rc

   if (command_argument_count() < 2) then
      print *, 'usage: cells_driver <i> <j>'
      stop 2
   end if
   call get_command_argument(1, arg)
   read(arg, *) ic
   call get_command_argument(2, arg)
   read(arg, *) jc

   do j = 1, JM
      do i = 1, IM
         lat(i,j) = real(10 * i + j, c_float)
         alb(i,j) = real(i * j, c_float) / 8.0_c_float
         tropp(i,j) = real(9000 + 500 * i + 100 * j, c_float)
         do k = 1, KM
            pl(i,j,k) = real(1000 * k * k + 37 * i + 11 * j, c_float)
            t(i,j,k) = real(200 + i + 2 * j + 3 * k, c_float)
         end do
      end do
   end do
   fields = [ c_loc(lat), c_loc(pl), c_loc(t), c_loc(alb) ]
   is2d = [ 1, 0, 0, 1 ]

   count = 0
   rows = 0.0
   rc = OHXSelectCells(int(IM, c_int), int(JM, c_int), int(KM, c_int), int(ic, c_int), int(ic, c_int), &
                       int(jc, c_int), int(jc, c_int), 1_c_int, int(KM, c_int), c_loc(pl), 0_c_int, c_loc(tropp), &
                       1_c_int, 0.0_c_float, cells, int(KM, c_int64_t), count)
   if (rc == 0) rc = OHXGatherCells(fields, is2d, int(NF, c_int), 1_c_int, int(IM, c_int), int(JM, c_int), &
                                    int(KM, c_int), cells, count, rows)
   if (rc /= 0) then
      print *, 'cells_driver: ', ohx_last_error()
      stop 1
   end if
   print '(a,i0)', 'count ', count
   do n = 1, int(count)
      print '(i0,4(1x,i0))', cells(n), (transfer(rows(f,n), 0_c_int32_t), f = 1, NF)
   end do
end program cells_driver
