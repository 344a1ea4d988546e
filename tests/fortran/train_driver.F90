!  train_driver -- every training and explaining entry point of ohx_bindings called from Fortran, one family a run:
!  quantile cuts, leaf refit, visit counts and covers, the twelve boosting calls, contributions and interactions.
!  Links against libohxgb.so and libamdhip64 only.  tests/test_gpu_fortran_training.py writes the inputs, starts one
!  process a family and compares what comes back with the numpy restatements of the header, bit for bit.
!
!  usage: train_driver <family> <dir>        family: cuts | refit | visits | boost | explain
!
!  Read from <dir> (the arrays raw little-endian float32, rows as x(ncol, nrow): the C row-major matrix):
!     args.txt                    one scalar a line, in the order of read_args below; floats as their bits (an int32)
!     x.f32  y.f32  w.f32         the training rows, labels and weights
!     ex.f32 ey.f32 ew.f32        the held-out rows, labels and weights
!     base.json                   the model every booster is loaded from (explain: explain.json)
!  Written to <dir>:
!     <family>.txt                "<key> <n>" followed by n lines of one integer each: integers as they are, every
!                                 float as its bits (transfer to int32; the RMSE doubles to int64)
!     <name>.json                 XGBoosterSaveModel after the calls that change the forest
!  The first non-zero rc prints ohx_last_error() and stops with status 1; nothing is started after it.  The one rc that
!  must NOT be zero is OHXQuantileCuts with a cap of 0, which the header refuses with *needed set.
!
!  Device addresses come from the four HIP calls bound privately below; the stream is c_null_ptr everywhere.
program train_driver
   use, intrinsic :: iso_c_binding
   use ohx_bindings
   implicit none

   interface
      function hipMalloc(ptr, nbytes) bind(C, name="hipMalloc") result(rc)
         import :: c_int, c_ptr, c_size_t
         type(c_ptr), intent(out)  :: ptr
         integer(c_size_t), value  :: nbytes
         integer(c_int)            :: rc
      end function
      function hipMemcpy(dst, src, nbytes, kind) bind(C, name="hipMemcpy") result(rc)
         import :: c_int, c_ptr, c_size_t
         type(c_ptr), value        :: dst, src
         integer(c_size_t), value  :: nbytes
         integer(c_int), value     :: kind
         integer(c_int)            :: rc
      end function
      function hipFree(ptr) bind(C, name="hipFree") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ptr
         integer(c_int)     :: rc
      end function
      function hipDeviceSynchronize() bind(C, name="hipDeviceSynchronize") result(rc)
         import :: c_int
         integer(c_int) :: rc
      end function
   end interface
   integer(c_int), parameter :: HOST_TO_DEVICE = 1        ! hipMemcpyHostToDevice

   character(len=1024) :: family, dir
   integer :: ou
   ! args.txt
   integer(c_int64_t) :: nrow, ncol, nheld, min_child_rows, seed, grid_row0
   integer(c_int) :: max_bins, rounds, max_depth, deep_depth, patience, unvisited, grid_im, grid_jm
   real(c_float) :: missing, eta, lambda, gamma, min_child_weight, subsample, colsample, prior_weight
   ! the arrays, their copies in HBM, and the four matrices
   real(c_float), allocatable, target :: x(:,:), y(:), w(:), ex(:,:), ey(:), ew(:)
   type(c_ptr) :: d_x, d_y, d_w, d_ex, d_ey, d_ew
   type(c_ptr) :: hmat, dmat, ehmat, edmat
   ! cuts
   integer(c_int64_t), allocatable :: cut_ptr(:)
   real(c_float), allocatable :: cut_values(:)
   integer(c_int64_t) :: ncut
   ! boost: the booster of the call at hand and every output of the twelve calls
   type(c_ptr) :: b
   integer(c_int64_t), target :: nodes
   real(c_double), allocatable, target :: train(:), eval(:)
   integer(c_int) :: run, best

   if (command_argument_count() < 2) then
      print *, 'usage: train_driver <family> <dir>'
      stop 2
   end if
   call get_command_argument(1, family)
   call get_command_argument(2, dir)
   call read_args()
   allocate(x(ncol, nrow), y(nrow), w(nrow), ex(ncol, nheld), ey(nheld), ew(nheld))
   call read_f32('x.f32', x, nrow * ncol)
   call read_f32('y.f32', y, nrow)
   call read_f32('w.f32', w, nrow)
   call read_f32('ex.f32', ex, nheld * ncol)
   call read_f32('ey.f32', ey, nheld)
   call read_f32('ew.f32', ew, nheld)
   open(newunit=ou, file=trim(dir)//'/'//trim(family)//'.txt', status='replace', action='write')

   ! the matrices: one the library copies from the host, one over rows this program put in HBM
   d_x = to_device(c_loc(x), nrow * ncol)
   d_y = to_device(c_loc(y), nrow)
   d_w = to_device(c_loc(w), nrow)
   d_ex = to_device(c_loc(ex), nheld * ncol)
   d_ey = to_device(c_loc(ey), nheld)
   d_ew = to_device(c_loc(ew), nheld)
   call hip(hipDeviceSynchronize(), 'hipDeviceSynchronize')
   call need(XGDMatrixCreateFromMat(x, nrow, ncol, missing, hmat), 'XGDMatrixCreateFromMat')
   call need(XGDMatrixCreateFromMat(ex, nheld, ncol, missing, ehmat), 'XGDMatrixCreateFromMat (held out)')
   call need(OHXDMatrixCreateFromDevice(d_x, nrow, ncol, missing, dmat), 'OHXDMatrixCreateFromDevice')
   call need(OHXDMatrixCreateFromDevice(d_ex, nheld, ncol, missing, edmat), 'OHXDMatrixCreateFromDevice (held out)')

   select case (trim(family))
   case ('cuts')
      call run_cuts()
   case ('refit')
      call run_refit()
   case ('visits')
      call run_visits()
   case ('boost')
      call run_boost()
   case ('explain')
      call run_explain()
   case default
      print *, 'train_driver: no family ', trim(family)
      stop 2
   end select

   call need(XGDMatrixFree(hmat), 'XGDMatrixFree')
   call need(XGDMatrixFree(ehmat), 'XGDMatrixFree')
   call need(XGDMatrixFree(dmat), 'XGDMatrixFree')
   call need(XGDMatrixFree(edmat), 'XGDMatrixFree')
   call hip(hipFree(d_x), 'hipFree')
   call hip(hipFree(d_y), 'hipFree')
   call hip(hipFree(d_w), 'hipFree')
   call hip(hipFree(d_ex), 'hipFree')
   call hip(hipFree(d_ey), 'hipFree')
   call hip(hipFree(d_ew), 'hipFree')
   call put1('done', 1_c_int64_t)
   close(ou)

contains

   ! ---- plumbing ----

   subroutine need(rc, what)
      integer(c_int), intent(in) :: rc
      character(len=*), intent(in) :: what
      if (rc /= 0) then
         print '(a,a,a,i0,a,a)', 'train_driver: ', what, ' returned ', rc, ': ', ohx_last_error()
         stop 1
      end if
   end subroutine

   subroutine hip(rc, what)
      integer(c_int), intent(in) :: rc
      character(len=*), intent(in) :: what
      if (rc /= 0) then
         print '(a,a,a,i0)', 'train_driver: ', what, ' returned ', rc
         stop 1
      end if
   end subroutine

   function bits_to_float(b) result(v)
      integer(c_int32_t), intent(in) :: b
      real(c_float) :: v
      v = transfer(b, 0.0_c_float)
   end function

   subroutine read_args()
      integer :: u
      integer(c_int32_t) :: b(8)
      open(newunit=u, file=trim(dir)//'/args.txt', status='old', action='read')
      read(u, *) nrow
      read(u, *) ncol
      read(u, *) nheld
      read(u, *) b(1)
      read(u, *) max_bins
      read(u, *) rounds
      read(u, *) max_depth
      read(u, *) deep_depth
      read(u, *) b(2)
      read(u, *) b(3)
      read(u, *) b(4)
      read(u, *) min_child_rows
      read(u, *) b(5)
      read(u, *) b(6)
      read(u, *) b(7)
      read(u, *) seed
      read(u, *) patience
      read(u, *) unvisited
      read(u, *) b(8)
      read(u, *) grid_im
      read(u, *) grid_jm
      read(u, *) grid_row0
      close(u)
      missing = bits_to_float(b(1))
      eta = bits_to_float(b(2))
      lambda = bits_to_float(b(3))
      gamma = bits_to_float(b(4))
      min_child_weight = bits_to_float(b(5))
      subsample = bits_to_float(b(6))
      colsample = bits_to_float(b(7))
      prior_weight = bits_to_float(b(8))
   end subroutine

   subroutine read_f32(name, a, n)
      character(len=*), intent(in) :: name
      integer(c_int64_t), intent(in) :: n
      real(c_float), intent(out) :: a(n)
      integer :: u
      open(newunit=u, file=trim(dir)//'/'//name, access='stream', form='unformatted', status='old', action='read')
      read(u) a
      close(u)
   end subroutine

   function to_device(src, n) result(d)
      type(c_ptr), intent(in) :: src
      integer(c_int64_t), intent(in) :: n
      type(c_ptr) :: d
      call hip(hipMalloc(d, int(4 * n, c_size_t)), 'hipMalloc')
      call hip(hipMemcpy(d, src, int(4 * n, c_size_t), HOST_TO_DEVICE), 'hipMemcpy')
   end function

   function load(name) result(b)
      character(len=*), intent(in) :: name
      type(c_ptr) :: b
      call need(XGBoosterCreate(c_null_ptr, 0_c_int64_t, b), 'XGBoosterCreate')
      call need(XGBoosterLoadModel(b, ohx_c_string(trim(dir)//'/'//name//'.json')), 'XGBoosterLoadModel')
   end function

   subroutine save_and_free(b, name)
      type(c_ptr), intent(in) :: b
      character(len=*), intent(in) :: name
      call need(XGBoosterSaveModel(b, ohx_c_string(trim(dir)//'/'//name//'.json')), 'XGBoosterSaveModel')
      call need(XGBoosterFree(b), 'XGBoosterFree')
   end subroutine

   subroutine put(key, v)
      character(len=*), intent(in) :: key
      integer(c_int64_t), intent(in) :: v(:)
      integer :: i
      write(ou, '(a,1x,i0)') key, size(v)
      do i = 1, size(v)
         write(ou, '(i0)') v(i)
      end do
   end subroutine

   subroutine put1(key, v)
      character(len=*), intent(in) :: key
      integer(c_int64_t), intent(in) :: v
      call put(key, [v])
   end subroutine

   subroutine put_floats(key, v)
      character(len=*), intent(in) :: key
      real(c_float), intent(in) :: v(:)
      integer :: i
      write(ou, '(a,1x,i0)') key, size(v)
      do i = 1, size(v)
         write(ou, '(i0)') transfer(v(i), 0_c_int32_t)
      end do
   end subroutine

   subroutine put_doubles(key, v)
      character(len=*), intent(in) :: key
      real(c_double), intent(in) :: v(:)
      integer :: i
      write(ou, '(a,1x,i0)') key, size(v)
      do i = 1, size(v)
         write(ou, '(i0)') transfer(v(i), 0_c_int64_t)
      end do
   end subroutine

   ! ---- cuts: OHXQuantileCuts, OHXDMatrixQuantileCuts ----

   !  OHXQuantileCuts the way a caller sizes its array: a cap of 0 first, to read `needed`, then with room
   subroutine host_cuts(report)
      logical, intent(in) :: report
      real(c_float) :: nothing(1)
      integer(c_int64_t) :: needed
      integer(c_int) :: rc
      allocate(cut_ptr(ncol + 1))
      needed = -1
      rc = OHXQuantileCuts(x, nrow, ncol, missing, max_bins, cut_ptr, nothing, 0_c_int64_t, needed)
      if (rc == 0 .or. needed < 1) then
         print '(a,i0,a,i0)', 'train_driver: OHXQuantileCuts with cap 0 returned ', rc, ' and needed = ', needed
         stop 1
      end if
      ncut = needed
      allocate(cut_values(ncut))
      needed = -1
      call need(OHXQuantileCuts(x, nrow, ncol, missing, max_bins, cut_ptr, cut_values, ncut, needed), 'OHXQuantileCuts')
      if (report) then
         call put1('sizing_rc', int(rc, c_int64_t))
         call put1('sizing_needed', ncut)
         call put1('host_needed', needed)
         call put('host_ptr', cut_ptr)
         call put_floats('host_values', cut_values)
      end if
   end subroutine

   subroutine matrix_cuts(key, m, row_step)
      character(len=*), intent(in) :: key
      type(c_ptr), intent(in) :: m
      integer(c_int64_t), intent(in) :: row_step
      integer(c_int64_t) :: ptr(ncol + 1), needed, cap
      real(c_float), allocatable :: values(:)
      cap = ncol * 254
      allocate(values(cap))
      needed = -1
      call need(OHXDMatrixQuantileCuts(m, row_step, max_bins, ptr, values, cap, needed, c_null_ptr), &
                'OHXDMatrixQuantileCuts '//key)
      call put1(key//'_needed', needed)
      call put(key//'_ptr', ptr)
      call put_floats(key//'_values', values(1:needed))
   end subroutine

   subroutine run_cuts()
      call host_cuts(.true.)
      call matrix_cuts('hostmat_step1', hmat, 1_c_int64_t)
      call matrix_cuts('hostmat_step3', hmat, 3_c_int64_t)
      call matrix_cuts('devmat_step1', dmat, 1_c_int64_t)
      call matrix_cuts('devmat_step3', dmat, 3_c_int64_t)
   end subroutine

   ! ---- refit: OHXBoosterRefitLeaves, OHXBoosterRefitLeavesDevice ----

   subroutine run_refit()
      type(c_ptr) :: b, dest
      integer(c_int64_t), target :: leaves
      integer :: form, how
      character(len=32) :: name
      do form = 1, 2
         do how = 1, 2
            b = load('base')
            leaves = -1
            dest = c_null_ptr
            if (how == 1) dest = c_loc(leaves)
            name = 'refit_'//trim(merge('host  ', 'device', form == 1))//'_'//trim(merge('loc ', 'null', how == 1))
            if (form == 1) then
               call need(OHXBoosterRefitLeaves(b, hmat, y, nrow, eta, lambda, unvisited, dest), 'OHXBoosterRefitLeaves')
            else
               call need(OHXBoosterRefitLeavesDevice(b, dmat, d_y, nrow, eta, lambda, unvisited, dest, c_null_ptr), &
                         'OHXBoosterRefitLeavesDevice')
            end if
            call put1(trim(name)//'_leaves', leaves)
            call save_and_free(b, trim(name))
         end do
      end do
   end subroutine

   ! ---- visits: the five visit-count and cover calls ----

   subroutine put_counts(b, key)
      type(c_ptr), intent(in) :: b
      character(len=*), intent(in) :: key
      integer(c_int64_t) :: ntree, rows_seen
      type(c_ptr) :: p_offsets, p_counts
      integer(c_int64_t), pointer :: offsets(:), counts(:)
      ntree = -1
      rows_seen = -1
      call need(OHXBoosterGetVisitCounts(b, c_null_ptr, ntree, p_offsets, p_counts, rows_seen), 'OHXBoosterGetVisitCounts')
      call c_f_pointer(p_offsets, offsets, [int(ntree + 1)])
      call c_f_pointer(p_counts, counts, [int(offsets(ntree + 1))])
      call put1(key//'_ntree', ntree)
      call put1(key//'_rows_seen', rows_seen)
      call put(key//'_offsets', offsets)
      call put(key//'_counts', counts)
   end subroutine

   subroutine run_visits()
      type(c_ptr) :: b
      b = load('base')
      call need(OHXBoosterCountVisits(b, hmat), 'OHXBoosterCountVisits')
      call put_counts(b, 'after_host')
      call need(OHXBoosterCountVisitsDevice(b, dmat, c_null_ptr), 'OHXBoosterCountVisitsDevice')
      call put_counts(b, 'after_device')                       ! counts accumulate: twice the rows
      call need(OHXBoosterResetVisitCounts(b), 'OHXBoosterResetVisitCounts')
      call put_counts(b, 'after_reset')
      call need(OHXBoosterCountVisitsDevice(b, edmat, c_null_ptr), 'OHXBoosterCountVisitsDevice (held out)')
      call put_counts(b, 'held_out')
      call need(OHXBoosterRefreshCover(b, c_null_ptr, prior_weight), 'OHXBoosterRefreshCover')
      call save_and_free(b, 'visits_refreshed')
   end subroutine

   ! ---- boost: the twelve OHXBoosterBoostTrees* entry points ----

   !  a freshly loaded booster, and every output set to what no call returns
   function fresh() result(h)
      type(c_ptr) :: h
      h = load('base')
      nodes = -1
      run = -1
      best = -1
      train = -1.0_c_double
      eval = -1.0_c_double
   end function

   subroutine report(name, with_eval)
      character(len=*), intent(in) :: name
      logical, intent(in) :: with_eval
      call put1(name//'_nodes_added', nodes)
      if (with_eval) then
         call put1(name//'_rounds_run', int(run, c_int64_t))
         call put1(name//'_best_round', int(best, c_int64_t))
         call put_doubles(name//'_train_rmse', train)
         call put_doubles(name//'_eval_rmse', eval)
      end if
      call save_and_free(b, 'boost_'//name)
   end subroutine

   subroutine run_boost()
      allocate(train(rounds + 1), eval(rounds + 1))
      call host_cuts(.false.)

      b = fresh()
      call need(OHXBoosterBoostTrees(b, hmat, y, nrow, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, &
                                     min_child_rows, c_loc(nodes)), 'OHXBoosterBoostTrees')
      call report('Plain', .false.)
      b = fresh()
      call need(OHXBoosterBoostTreesDevice(b, dmat, d_y, nrow, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, &
                                           min_child_rows, c_loc(nodes), c_null_ptr), 'OHXBoosterBoostTreesDevice')
      call report('PlainDevice', .false.)

      b = fresh()
      call need(OHXBoosterBoostTreesEval(b, hmat, y, nrow, ehmat, c_loc(ey), nheld, cut_ptr, cut_values, rounds, &
                                         max_depth, eta, lambda, gamma, min_child_rows, patience, c_loc(train), &
                                         c_loc(eval), run, best, c_loc(nodes)), 'OHXBoosterBoostTreesEval')
      call report('Eval', .true.)
      b = fresh()
      call need(OHXBoosterBoostTreesEvalDevice(b, dmat, d_y, nrow, edmat, d_ey, nheld, cut_ptr, cut_values, rounds, &
                                               max_depth, eta, lambda, gamma, min_child_rows, patience, c_loc(train), &
                                               c_loc(eval), run, best, c_loc(nodes), c_null_ptr), &
                'OHXBoosterBoostTreesEvalDevice')
      call report('EvalDevice', .true.)

      b = fresh()
      call need(OHXBoosterBoostTreesWeighted(b, hmat, y, c_loc(w), nrow, ehmat, c_loc(ey), c_loc(ew), nheld, cut_ptr, &
                                             cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
                                             patience, c_loc(train), c_loc(eval), run, best, c_loc(nodes)), &
                'OHXBoosterBoostTreesWeighted')
      call report('Weighted', .true.)
      b = fresh()
      call need(OHXBoosterBoostTreesWeightedDevice(b, dmat, d_y, d_w, nrow, edmat, d_ey, d_ew, nheld, cut_ptr, &
                                                   cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
                                                   patience, c_loc(train), c_loc(eval), run, best, c_loc(nodes), &
                                                   c_null_ptr), 'OHXBoosterBoostTreesWeightedDevice')
      call report('WeightedDevice', .true.)

      b = fresh()
      call need(OHXBoosterBoostTreesSampled(b, hmat, y, c_loc(w), nrow, ehmat, c_loc(ey), c_loc(ew), nheld, cut_ptr, &
                                            cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
                                            subsample, colsample, seed, patience, c_loc(train), c_loc(eval), run, best, &
                                            c_loc(nodes)), 'OHXBoosterBoostTreesSampled')
      call report('Sampled', .true.)
      b = fresh()
      call need(OHXBoosterBoostTreesSampledDevice(b, dmat, d_y, d_w, nrow, edmat, d_ey, d_ew, nheld, cut_ptr, &
                                                  cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
                                                  subsample, colsample, seed, patience, c_loc(train), c_loc(eval), run, &
                                                  best, c_loc(nodes), c_null_ptr), 'OHXBoosterBoostTreesSampledDevice')
      call report('SampledDevice', .true.)

      b = fresh()
      call need(OHXBoosterBoostTreesDeep(b, hmat, y, c_loc(w), nrow, ehmat, c_loc(ey), c_loc(ew), nheld, cut_ptr, &
                                         cut_values, rounds, deep_depth, eta, lambda, gamma, min_child_weight, &
                                         patience, c_loc(train), c_loc(eval), run, best, c_loc(nodes)), &
                'OHXBoosterBoostTreesDeep')
      call report('Deep', .true.)
      b = fresh()
      call need(OHXBoosterBoostTreesDeepDevice(b, dmat, d_y, d_w, nrow, edmat, d_ey, d_ew, nheld, cut_ptr, &
                                               cut_values, rounds, deep_depth, eta, lambda, gamma, min_child_weight, &
                                               patience, c_loc(train), c_loc(eval), run, best, c_loc(nodes), &
                                               c_null_ptr), 'OHXBoosterBoostTreesDeepDevice')
      call report('DeepDevice', .true.)

      b = fresh()
      call need(OHXBoosterBoostTreesDeepSampled(b, hmat, y, c_loc(w), nrow, ehmat, c_loc(ey), c_loc(ew), nheld, cut_ptr, &
                                                cut_values, rounds, deep_depth, eta, lambda, gamma, min_child_weight, &
                                                subsample, colsample, seed, patience, c_loc(train), c_loc(eval), run, &
                                                best, c_loc(nodes)), 'OHXBoosterBoostTreesDeepSampled')
      call report('DeepSampled', .true.)
      b = fresh()
      call need(OHXBoosterBoostTreesDeepSampledDevice(b, dmat, d_y, d_w, nrow, edmat, d_ey, d_ew, nheld, cut_ptr, &
                                                      cut_values, rounds, deep_depth, eta, lambda, gamma, &
                                                      min_child_weight, subsample, colsample, seed, patience, &
                                                      c_loc(train), c_loc(eval), run, best, c_loc(nodes), c_null_ptr), &
                'OHXBoosterBoostTreesDeepSampledDevice')
      call report('DeepSampledDevice', .true.)
   end subroutine

   ! ---- explain: contributions, interactions, OHXDMatrixSetGrid, OHXBoosterGetNumCategoricalSplits ----

   subroutine run_explain()
      type(c_ptr) :: b, p
      integer(c_int64_t) :: n, ncat
      real(c_float), pointer :: phi(:,:), inter(:,:,:), margin(:)
      real(c_float), allocatable :: before(:)
      integer :: nf, i
      logical :: same
      b = load('explain')
      nf = int(ncol) + 1
      n = -1
      call need(OHXBoosterPredictContribs(b, ehmat, 0_c_int, 0_c_int, n, p), 'OHXBoosterPredictContribs')
      call put1('contribs_len', n)
      call c_f_pointer(p, phi, [nf, int(nheld)])
      call put_floats('contribs', reshape(phi, [nf * int(nheld)]))
      n = -1
      call need(OHXBoosterPredictInteractions(b, edmat, 0_c_int, 0_c_int, n, p), 'OHXBoosterPredictInteractions')
      call put1('interactions_len', n)
      call c_f_pointer(p, inter, [nf, nf, int(nheld)])
      call put_floats('interactions', reshape(inter, [nf * nf * int(nheld)]))
      ! a grid hint changes no byte of a predict
      n = -1
      call need(XGBoosterPredict(b, ehmat, 1_c_int, 0_c_int, 0_c_int, n, p), 'XGBoosterPredict')
      call c_f_pointer(p, margin, [int(n)])
      allocate(before(n))
      before = margin
      call need(OHXDMatrixSetGrid(ehmat, grid_im, grid_jm, grid_row0), 'OHXDMatrixSetGrid')
      n = -1
      call need(XGBoosterPredict(b, ehmat, 1_c_int, 0_c_int, 0_c_int, n, p), 'XGBoosterPredict after OHXDMatrixSetGrid')
      call c_f_pointer(p, margin, [int(n)])
      same = n == size(before)
      if (same) then
         do i = 1, int(n)
            same = same .and. transfer(margin(i), 0_c_int32_t) == transfer(before(i), 0_c_int32_t)
         end do
      end if
      call put1('predict_len', n)
      call put1('predict_same_after_set_grid', int(merge(1, 0, same), c_int64_t))
      call put_floats('predict', margin)
      ncat = -1
      call need(OHXBoosterGetNumCategoricalSplits(b, ncat), 'OHXBoosterGetNumCategoricalSplits')
      call put1('categorical_splits', ncat)
      call need(XGBoosterFree(b), 'XGBoosterFree')
   end subroutine

end program train_driver
