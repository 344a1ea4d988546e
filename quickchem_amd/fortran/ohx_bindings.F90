!  ohx_bindings -- ISO_C_BINDING view of libohxgb.so (include/ohxgb.h).
!
!  This is the thin shim BASELINE.json's north star asks for: Fortran host code
!  reaches the HIP kernels through plain C symbols, no CUDA-compat layer.  The
!  first group are the XGBoost C-API symbols that QuickChem's own
!  Shared/xgb_fortran_api.F90 binds (that module links against libohxgb.so
!  unchanged -- see INTEGRATION.md); they are declared again here, under their C
!  names, so that this tree builds without the reference.  The second group is
!  the additive fused entry point.
module ohx_bindings
   use, intrinsic :: iso_c_binding
   implicit none
   private

   public :: XGDMatrixCreateFromMat, XGDMatrixFree, XGDMatrixNumRow, XGDMatrixNumCol
   public :: XGBoosterCreate, XGBoosterFree, XGBoosterLoadModel, XGBoosterSaveModel
   public :: XGBoosterPredict, XGBoosterSetParam, OHXBoosterPredictFields, OHXDMatrixSetGrid, OHXBoosterPredictContribs
   public :: OHXBoosterPredictInteractions, OHXBoosterPredictContribsFields, OHXBoosterPredictContribsFieldsDevice
   public :: OHXCommGetUniqueId, OHXCommInitRank, OHXCommFree, OHXCommInfo, OHXShardRows, OHXAllGatherOH, OHX_UNIQUE_ID_BYTES
   public :: OHXBoosterGetNumCategoricalSplits
   public :: OHXSelectCells, OHXSelectCellsDevice, OHXGatherCells, OHXGatherCellsDevice
   public :: OHXScatterCells, OHXScatterCellsDevice
   public :: OHXDMatrixCreateFromDevice
   public :: OHXBoosterCountVisits, OHXBoosterCountVisitsDevice, OHXBoosterGetVisitCounts, OHXBoosterResetVisitCounts
   public :: OHXBoosterRefreshCover, OHXBoosterRefitLeaves, OHXBoosterRefitLeavesDevice
   public :: OHXBoosterBoostTrees, OHXBoosterBoostTreesDevice, OHXBoosterBoostTreesEval, OHXBoosterBoostTreesEvalDevice
   public :: OHXBoosterBoostTreesWeighted, OHXBoosterBoostTreesWeightedDevice
   public :: OHXBoosterBoostTreesSampled, OHXBoosterBoostTreesSampledDevice
   public :: OHXBoosterBoostTreesDeep, OHXBoosterBoostTreesDeepDevice
   public :: OHXBoosterBoostTreesDeepSampled, OHXBoosterBoostTreesDeepSampledDevice
   public :: OHXQuantileCuts, OHXDMatrixQuantileCuts
   public :: ohx_last_error, ohx_c_string

   integer, parameter :: OHX_UNIQUE_ID_BYTES = 128

   interface
      ! ---- symbols bound by the reference (Shared/xgb_fortran_api.F90:19-119) ----
      function XGDMatrixCreateFromMat(data, nrow, ncol, missing, out) bind(C, name="XGDMatrixCreateFromMat") result(rc)
         import :: c_int, c_float, c_int64_t, c_ptr
         real(c_float), intent(in)      :: data(*)
         integer(c_int64_t), value      :: nrow, ncol
         real(c_float), value           :: missing
         type(c_ptr), intent(out)       :: out
         integer(c_int)                 :: rc
      end function

      function XGDMatrixFree(handle) bind(C, name="XGDMatrixFree") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int)     :: rc
      end function

      function XGDMatrixNumRow(handle, out) bind(C, name="XGDMatrixNumRow") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value              :: handle
         integer(c_int64_t), intent(out) :: out
         integer(c_int)                  :: rc
      end function

      function XGDMatrixNumCol(handle, out) bind(C, name="XGDMatrixNumCol") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value              :: handle
         integer(c_int64_t), intent(out) :: out
         integer(c_int)                  :: rc
      end function

      ! dmats: the reference hands over ONE handle by value with len = 0
      ! (OH_GridCompMod.F90:255-256); the library never reads it then.
      function XGBoosterCreate(dmats, len, out) bind(C, name="XGBoosterCreate") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value        :: dmats
         integer(c_int64_t), value :: len
         type(c_ptr), intent(out)  :: out
         integer(c_int)            :: rc
      end function

      function XGBoosterFree(handle) bind(C, name="XGBoosterFree") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int)     :: rc
      end function

      function XGBoosterLoadModel(handle, fname) bind(C, name="XGBoosterLoadModel") result(rc)
         import :: c_int, c_ptr, c_char
         type(c_ptr), value                 :: handle
         character(kind=c_char), intent(in) :: fname(*)
         integer(c_int)                     :: rc
      end function

      function XGBoosterSaveModel(handle, fname) bind(C, name="XGBoosterSaveModel") result(rc)
         import :: c_int, c_ptr, c_char
         type(c_ptr), value                 :: handle
         character(kind=c_char), intent(in) :: fname(*)
         integer(c_int)                     :: rc
      end function

      function XGBoosterPredict(handle, dmat, option_mask, ntree_limit, training, length, prediction) &
            bind(C, name="XGBoosterPredict") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value              :: handle, dmat
         integer(c_int), value           :: option_mask, ntree_limit, training
         integer(c_int64_t), intent(out) :: length
         type(c_ptr), intent(out)        :: prediction
         integer(c_int)                  :: rc
      end function

      ! ---- beyond the reference's bindings ----
      function XGBoosterSetParam(handle, name, val) bind(C, name="XGBoosterSetParam") result(rc)
         import :: c_int, c_ptr, c_char
         type(c_ptr), value                 :: handle
         character(kind=c_char), intent(in) :: name(*), val(*)
         integer(c_int)                     :: rc
      end function

      function XGBGetLastError_c() bind(C, name="XGBGetLastError") result(msg)
         import :: c_ptr
         type(c_ptr) :: msg
      end function

      ! The whole RUN section of predict_OH_with_XGB in one kernel (ohxgb.h).
      function OHXBoosterPredictFields(handle, fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, &
                                       apply_pow10, ohscale, oh_ml, margin) &
            bind(C, name="OHXBoosterPredictFields") result(rc)
         import :: c_int, c_ptr, c_float, c_int32_t
         type(c_ptr), value             :: handle
         type(c_ptr), intent(in)        :: fields(*)
         integer(c_int32_t), intent(in) :: is2d(*)
         integer(c_int), value          :: nfield, pl_feature, im, jm, km, k1, k2
         real(c_float), value           :: missing
         integer(c_int), value          :: apply_pow10
         real(c_float), value           :: ohscale
         type(c_ptr), value             :: oh_ml, margin
         integer(c_int)                 :: rc
      end function

      ! Per-feature contributions (ohxgb.h part 2): approximate = 0 exact TreeSHAP, 1 xgboost's approximate
      ! attribution.  out_result points at nrow * (F + 1) floats owned by the booster (row-major: in Fortran a
      ! (F + 1, nrow) array through c_f_pointer), column F + 1 the bias; valid until the next contribs call.
      function OHXBoosterPredictContribs(handle, dmat, approximate, ntree_limit, out_len, out_result) &
            bind(C, name="OHXBoosterPredictContribs") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value         :: handle, dmat
         integer(c_int), value      :: approximate, ntree_limit
         integer(c_int64_t)         :: out_len
         type(c_ptr)                :: out_result
         integer(c_int)             :: rc
      end function

      ! SHAP interaction values (ohxgb.h part 2): out_result points at nrow * (F + 1)**2 floats owned by the booster
      ! (row-major [row][i][k]: in Fortran an (F + 1, F + 1, nrow) array through c_f_pointer, index F + 1 the bias);
      ! valid until the next interactions call.
      function OHXBoosterPredictInteractions(handle, dmat, approximate, ntree_limit, out_len, out_result) &
            bind(C, name="OHXBoosterPredictInteractions") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value         :: handle, dmat
         integer(c_int), value      :: approximate, ntree_limit
         integer(c_int64_t)         :: out_len
         type(c_ptr)                :: out_result
         integer(c_int)             :: rc
      end function

      ! Per-feature contributions from the fields (ohxgb.h part 2): fields / is2d / ... as OHXBoosterPredictFields;
      ! out(f) = c_loc of an (im,jm,km) real(c_float) array for f = 1 .. F + 1 (F + 1 the bias), or c_null_ptr for one
      ! not wanted.  Levels k1..k2 are written.  Declarations only: nothing the oracle drivers link calls these.
      function OHXBoosterPredictContribsFields(handle, fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, &
                                               approximate, ntree_limit, out) &
            bind(C, name="OHXBoosterPredictContribsFields") result(rc)
         import :: c_int, c_ptr, c_float, c_int32_t
         type(c_ptr), value             :: handle
         type(c_ptr), intent(in)        :: fields(*)
         integer(c_int32_t), intent(in) :: is2d(*)
         integer(c_int), value          :: nfield, pl_feature, im, jm, km, k1, k2
         real(c_float), value           :: missing
         integer(c_int), value          :: approximate, ntree_limit
         type(c_ptr), intent(in)        :: out(*)
         integer(c_int)                 :: rc
      end function

      ! The same on device addresses, enqueued on `stream` (a hipStream_t; c_null_ptr = the default stream).
      function OHXBoosterPredictContribsFieldsDevice(handle, d_fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, &
                                                     missing, approximate, ntree_limit, d_out, stream) &
            bind(C, name="OHXBoosterPredictContribsFieldsDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int32_t
         type(c_ptr), value             :: handle
         type(c_ptr), intent(in)        :: d_fields(*)
         integer(c_int32_t), intent(in) :: is2d(*)
         integer(c_int), value          :: nfield, pl_feature, im, jm, km, k1, k2
         real(c_float), value           :: missing
         integer(c_int), value          :: approximate, ntree_limit
         type(c_ptr), intent(in)        :: d_out(*)
         type(c_ptr), value             :: stream
         integer(c_int)                 :: rc
      end function

      ! Selected gridcells (ohxgb.h part 2): a cell index is c = (i-1) + im*((j-1) + jm*(k-1)), integer(c_int64_t).
      ! Declarations only, as above.  a, b: c_loc of an (im,jm,km) array, or of an (im,jm) one with a_is2d / b_is2d
      ! /= 0; c_null_ptr for none (b: the scalar b0; a: every cell of the box).  cells holds cap entries.
      function OHXSelectCells(im, jm, km, i1, i2, j1, j2, k1, k2, a, a_is2d, b, b_is2d, b0, cells, cap, count) &
            bind(C, name="OHXSelectCells") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         integer(c_int), value          :: im, jm, km, i1, i2, j1, j2, k1, k2
         type(c_ptr), value             :: a, b
         integer(c_int), value          :: a_is2d, b_is2d
         real(c_float), value           :: b0
         integer(c_int64_t)             :: cells(*)
         integer(c_int64_t), value      :: cap
         integer(c_int64_t), intent(out) :: count
         integer(c_int)                 :: rc
      end function

      ! The same on device addresses: d_cells, d_count (one int64) and d_status (one int32 of bits, or c_null_ptr) are
      ! device pointers; enqueued on `stream`.
      function OHXSelectCellsDevice(im, jm, km, i1, i2, j1, j2, k1, k2, d_a, a_is2d, d_b, b_is2d, b0, d_cells, cap, &
                                    d_count, d_status, stream) bind(C, name="OHXSelectCellsDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         integer(c_int), value          :: im, jm, km, i1, i2, j1, j2, k1, k2
         type(c_ptr), value             :: d_a, d_b
         integer(c_int), value          :: a_is2d, b_is2d
         real(c_float), value           :: b0
         type(c_ptr), value             :: d_cells
         integer(c_int64_t), value      :: cap
         type(c_ptr), value             :: d_count, d_status, stream
         integer(c_int)                 :: rc
      end function

      ! rows(nfield, ncell): column n is the row of cell cells(n); fields / is2d / pl_feature as OHXBoosterPredictFields.
      function OHXGatherCells(fields, is2d, nfield, pl_feature, im, jm, km, cells, ncell, rows) &
            bind(C, name="OHXGatherCells") result(rc)
         import :: c_int, c_ptr, c_float, c_int32_t, c_int64_t
         type(c_ptr), intent(in)        :: fields(*)
         integer(c_int32_t), intent(in) :: is2d(*)
         integer(c_int), value          :: nfield, pl_feature, im, jm, km
         integer(c_int64_t), intent(in) :: cells(*)
         integer(c_int64_t), value      :: ncell
         real(c_float)                  :: rows(*)
         integer(c_int)                 :: rc
      end function

      function OHXGatherCellsDevice(d_fields, is2d, nfield, pl_feature, im, jm, km, d_cells, ncell, d_rows, d_status, &
                                    stream) bind(C, name="OHXGatherCellsDevice") result(rc)
         import :: c_int, c_ptr, c_int32_t, c_int64_t
         type(c_ptr), intent(in)        :: d_fields(*)
         integer(c_int32_t), intent(in) :: is2d(*)
         integer(c_int), value          :: nfield, pl_feature, im, jm, km
         type(c_ptr), value             :: d_cells
         integer(c_int64_t), value      :: ncell
         type(c_ptr), value             :: d_rows, d_status, stream
         integer(c_int)                 :: rc
      end function

      ! out3d(cells(n)) = values(col + 1, n) for values(stride, ncell); cells strictly ascending.
      function OHXScatterCells(values, stride, col, cells, ncell, out3d, im, jm, km) &
            bind(C, name="OHXScatterCells") result(rc)
         import :: c_int, c_float, c_int64_t
         real(c_float), intent(in)      :: values(*)
         integer(c_int64_t), value      :: stride, col
         integer(c_int64_t), intent(in) :: cells(*)
         integer(c_int64_t), value      :: ncell
         real(c_float)                  :: out3d(*)
         integer(c_int), value          :: im, jm, km
         integer(c_int)                 :: rc
      end function

      function OHXScatterCellsDevice(d_values, stride, col, d_cells, ncell, d_out3d, im, jm, km, d_status, stream) &
            bind(C, name="OHXScatterCellsDevice") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value             :: d_values
         integer(c_int64_t), value      :: stride, col
         type(c_ptr), value             :: d_cells
         integer(c_int64_t), value      :: ncell
         type(c_ptr), value             :: d_out3d
         integer(c_int), value          :: im, jm, km
         type(c_ptr), value             :: d_status, stream
         integer(c_int)                 :: rc
      end function

      ! A DMatrix over rows that already lie in HBM (ohxgb.h part 2): d_data is the DEVICE address of nrow x ncol
      ! real(c_float), row-major (in Fortran a (ncol, nrow) array); the matrix borrows it until XGDMatrixFree.
      function OHXDMatrixCreateFromDevice(d_data, nrow, ncol, missing, out) &
            bind(C, name="OHXDMatrixCreateFromDevice") result(rc)
         import :: c_int, c_float, c_int64_t, c_ptr
         type(c_ptr), value             :: d_data
         integer(c_int64_t), value      :: nrow, ncol
         real(c_float), value           :: missing
         type(c_ptr), intent(out)       :: out
         integer(c_int)                 :: rc
      end function

      ! Optional hint: the DMatrix rows are rows row0.. of the (im,jm,*) gather (ohxgb.h); speed only.
      function OHXDMatrixSetGrid(handle, im, jm, row0) bind(C, name="OHXDMatrixSetGrid") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value        :: handle
         integer(c_int), value     :: im, jm
         integer(c_int64_t), value :: row0
         integer(c_int)            :: rc
      end function

      ! Nodes of the loaded model with a categorical split (ohxgb.h); 0 for a booster without one.  A booster that has
      ! some predicts through XGBoosterPredict only: the fields, contributions and Run1 forms refuse it.
      function OHXBoosterGetNumCategoricalSplits(handle, out) bind(C, name="OHXBoosterGetNumCategoricalSplits") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value              :: handle
         integer(c_int64_t), intent(out) :: out
         integer(c_int)                  :: rc
      end function

      !  Node visit counts and the covers refreshed from them (include/ohxgb.h; docs/16_visit_counts.md).
      !  Called by tests/fortran/train_driver.F90; nothing the oracle-linked drivers link calls them.
      function OHXBoosterCountVisits(handle, dmat) bind(C, name="OHXBoosterCountVisits") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle, dmat
         integer(c_int)     :: rc
      end function

      function OHXBoosterCountVisitsDevice(handle, dmat, stream) bind(C, name="OHXBoosterCountVisitsDevice") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle, dmat, stream
         integer(c_int)     :: rc
      end function

      !  tree_offsets: c_ptr to ntree + 1 integer(c_int64_t); counts: c_ptr to tree_offsets(ntree + 1) integer(c_int64_t)
      function OHXBoosterGetVisitCounts(handle, stream, ntree, tree_offsets, counts, rows_seen) &
            bind(C, name="OHXBoosterGetVisitCounts") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value              :: handle, stream
         integer(c_int64_t), intent(out) :: ntree, rows_seen
         type(c_ptr), intent(out)        :: tree_offsets, counts
         integer(c_int)                  :: rc
      end function

      function OHXBoosterResetVisitCounts(handle) bind(C, name="OHXBoosterResetVisitCounts") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int)     :: rc
      end function

      function OHXBoosterRefreshCover(handle, stream, prior_weight) bind(C, name="OHXBoosterRefreshCover") result(rc)
         import :: c_int, c_ptr, c_float
         type(c_ptr), value   :: handle, stream
         real(c_float), value :: prior_weight
         integer(c_int)       :: rc
      end function

      !  Leaf refit (include/ohxgb.h; docs/17_leaf_refit.md).  Called by tests/fortran/train_driver.F90; nothing the
      !  oracle-linked drivers link calls them.  labels: nlabel real(c_float) on the host; d_labels: their DEVICE address (c_ptr).
      !  leaves_refit: c_loc of an integer(c_int64_t), or c_null_ptr - the header allows NULL
      function OHXBoosterRefitLeaves(handle, dmat, labels, nlabel, eta, lambda, unvisited, leaves_refit) &
            bind(C, name="OHXBoosterRefitLeaves") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel
         real(c_float), value            :: eta, lambda
         integer(c_int), value           :: unvisited
         type(c_ptr), value              :: leaves_refit
         integer(c_int)                  :: rc
      end function

      function OHXBoosterRefitLeavesDevice(handle, dmat, d_labels, nlabel, eta, lambda, unvisited, leaves_refit, stream) &
            bind(C, name="OHXBoosterRefitLeavesDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, stream
         integer(c_int64_t), value       :: nlabel
         real(c_float), value            :: eta, lambda
         integer(c_int), value           :: unvisited
         type(c_ptr), value              :: leaves_refit
         integer(c_int)                  :: rc
      end function

      !  Called by tests/fortran/train_driver.F90.
      !  Boosting new trees (include/ohxgb.h; docs/18_boost_trees.md).  labels: nlabel
      !  real(c_float) on the host; d_labels: their DEVICE address (c_ptr); cut_ptr / cut_values: HOST arrays in both
      !  forms.  nodes_added: c_loc of an integer(c_int64_t), or c_null_ptr
      function OHXBoosterBoostTrees(handle, dmat, labels, nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, &
            gamma, min_child_rows, nodes_added) bind(C, name="OHXBoosterBoostTrees") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth
         real(c_float), value            :: eta, lambda, gamma
         integer(c_int64_t), value       :: min_child_rows
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesDevice(handle, dmat, d_labels, nlabel, cut_ptr, cut_values, rounds, max_depth, eta, &
            lambda, gamma, min_child_rows, nodes_added, stream) bind(C, name="OHXBoosterBoostTreesDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, stream
         integer(c_int64_t), value       :: nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth
         real(c_float), value            :: eta, lambda, gamma
         integer(c_int64_t), value       :: min_child_rows
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  Called by tests/fortran/train_driver.F90.
      !  Boosting with a held-out set (include/ohxgb.h; docs/20_boost_eval.md).  eval_dmat: a
      !  second DMatrix or c_null_ptr; eval_labels: c_loc of eval_nlabel real(c_float) on the host (d_eval_labels: their
      !  DEVICE address), or c_null_ptr without a held-out set.  train_rmse / eval_rmse: c_loc of rounds + 1
      !  real(c_double), or c_null_ptr; rounds_run / best_round: integer(c_int) out; nodes_added as above
      function OHXBoosterBoostTreesEval(handle, dmat, labels, nlabel, eval_dmat, eval_labels, eval_nlabel, cut_ptr, &
            cut_values, rounds, max_depth, eta, lambda, gamma, min_child_rows, patience, train_rmse, eval_rmse, &
            rounds_run, best_round, nodes_added) bind(C, name="OHXBoosterBoostTreesEval") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, eval_dmat, eval_labels
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma
         integer(c_int64_t), value       :: min_child_rows
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesEvalDevice(handle, dmat, d_labels, nlabel, eval_dmat, d_eval_labels, eval_nlabel, &
            cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_rows, patience, train_rmse, &
            eval_rmse, rounds_run, best_round, nodes_added, stream) &
            bind(C, name="OHXBoosterBoostTreesEvalDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, eval_dmat, d_eval_labels, stream
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma
         integer(c_int64_t), value       :: min_child_rows
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  Called by tests/fortran/train_driver.F90.
      !  Boosting with row weights (include/ohxgb.h; docs/21_row_weights.md).  weights /
      !  eval_weights: c_loc of nlabel / eval_nlabel real(c_float) on the host (d_weights / d_eval_weights: their DEVICE
      !  addresses), or c_null_ptr for weights of 1.  min_child_weight stands where min_child_rows stood.  The rest as above
      function OHXBoosterBoostTreesWeighted(handle, dmat, labels, weights, nlabel, eval_dmat, eval_labels, eval_weights, &
            eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, patience, &
            train_rmse, eval_rmse, rounds_run, best_round, nodes_added) &
            bind(C, name="OHXBoosterBoostTreesWeighted") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, weights, eval_dmat, eval_labels, eval_weights
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesWeightedDevice(handle, dmat, d_labels, d_weights, nlabel, eval_dmat, d_eval_labels, &
            d_eval_weights, eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
            patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added, stream) &
            bind(C, name="OHXBoosterBoostTreesWeightedDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, d_weights, eval_dmat, d_eval_labels, d_eval_weights, stream
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  Called by tests/fortran/train_driver.F90.
      !  Boosting with row and column subsampling (include/ohxgb.h; docs/22_sampling.md).  The
      !  weighted call with subsample, colsample_bytree (both in (0, 1]) and seed (the 64 bits of a uint64) before patience
      function OHXBoosterBoostTreesSampled(handle, dmat, labels, weights, nlabel, eval_dmat, eval_labels, eval_weights, &
            eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, subsample, &
            colsample_bytree, seed, patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added) &
            bind(C, name="OHXBoosterBoostTreesSampled") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, weights, eval_dmat, eval_labels, eval_weights
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight, subsample, colsample_bytree
         integer(c_int64_t), value       :: seed
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesSampledDevice(handle, dmat, d_labels, d_weights, nlabel, eval_dmat, d_eval_labels, &
            d_eval_weights, eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
            subsample, colsample_bytree, seed, patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added, &
            stream) bind(C, name="OHXBoosterBoostTreesSampledDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, d_weights, eval_dmat, d_eval_labels, d_eval_weights, stream
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight, subsample, colsample_bytree
         integer(c_int64_t), value       :: seed
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  Called by tests/fortran/train_driver.F90.
      !  Trees deeper than eight levels (include/ohxgb.h; docs/23_deep_trees.md).  The weighted
      !  call's argument lists with max_depth in 1..18; with max_depth > 8 the call waits once a level from level 7 on
      function OHXBoosterBoostTreesDeep(handle, dmat, labels, weights, nlabel, eval_dmat, eval_labels, eval_weights, &
            eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, patience, &
            train_rmse, eval_rmse, rounds_run, best_round, nodes_added) &
            bind(C, name="OHXBoosterBoostTreesDeep") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, weights, eval_dmat, eval_labels, eval_weights
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesDeepDevice(handle, dmat, d_labels, d_weights, nlabel, eval_dmat, d_eval_labels, &
            d_eval_weights, eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
            patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added, stream) &
            bind(C, name="OHXBoosterBoostTreesDeepDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, d_weights, eval_dmat, d_eval_labels, d_eval_weights, stream
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  Row and column subsampling for trees deeper than eight levels (include/ohxgb.h; docs/24_deep_sampled.md).
      !  Called by tests/fortran/train_driver.F90.
      !  The sampled call's argument lists with max_depth in 1..18; with max_depth > 8 the call
      !  waits once a level from level 7 on
      function OHXBoosterBoostTreesDeepSampled(handle, dmat, labels, weights, nlabel, eval_dmat, eval_labels, eval_weights, &
            eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, subsample, &
            colsample_bytree, seed, patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added) &
            bind(C, name="OHXBoosterBoostTreesDeepSampled") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, weights, eval_dmat, eval_labels, eval_weights
         real(c_float), intent(in)       :: labels(*)
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight, subsample, colsample_bytree
         integer(c_int64_t), value       :: seed
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      function OHXBoosterBoostTreesDeepSampledDevice(handle, dmat, d_labels, d_weights, nlabel, eval_dmat, d_eval_labels, &
            d_eval_weights, eval_nlabel, cut_ptr, cut_values, rounds, max_depth, eta, lambda, gamma, min_child_weight, &
            subsample, colsample_bytree, seed, patience, train_rmse, eval_rmse, rounds_run, best_round, nodes_added, &
            stream) bind(C, name="OHXBoosterBoostTreesDeepSampledDevice") result(rc)
         import :: c_int, c_ptr, c_float, c_int64_t
         type(c_ptr), value              :: handle, dmat, d_labels, d_weights, eval_dmat, d_eval_labels, d_eval_weights, stream
         integer(c_int64_t), value       :: nlabel, eval_nlabel
         integer(c_int64_t), intent(in)  :: cut_ptr(*)
         real(c_float), intent(in)       :: cut_values(*)
         integer(c_int), value           :: rounds, max_depth, patience
         real(c_float), value            :: eta, lambda, gamma, min_child_weight, subsample, colsample_bytree
         integer(c_int64_t), value       :: seed
         type(c_ptr), value              :: train_rmse, eval_rmse
         integer(c_int), intent(out)     :: rounds_run, best_round
         type(c_ptr), value              :: nodes_added
         integer(c_int)                  :: rc
      end function

      !  data: a row-major host sample (nrow x ncol); cut_ptr: ncol + 1 entries out; needed: the cut values in all
      function OHXQuantileCuts(data, nrow, ncol, missing, max_bins, cut_ptr, cut_values, cap, needed) &
            bind(C, name="OHXQuantileCuts") result(rc)
         import :: c_int, c_float, c_int64_t
         real(c_float), intent(in)       :: data(*)
         integer(c_int64_t), value       :: nrow, ncol
         real(c_float), value            :: missing
         integer(c_int), value           :: max_bins
         integer(c_int64_t), intent(out) :: cut_ptr(*)
         real(c_float), intent(out)      :: cut_values(*)
         integer(c_int64_t), value       :: cap
         integer(c_int64_t), intent(out) :: needed
         integer(c_int)                  :: rc
      end function

      !  the same cuts from rows 0, row_step, 2 * row_step, ... of a DMatrix in HBM; cut_ptr (the matrix's ncol + 1
      !  entries), cut_values and needed are host arrays; stream: a hipStream_t the rows are ready on (c_null_ptr = default)
      function OHXDMatrixQuantileCuts(dmat, row_step, max_bins, cut_ptr, cut_values, cap, needed, stream) &
            bind(C, name="OHXDMatrixQuantileCuts") result(rc)
         import :: c_int, c_float, c_int64_t, c_ptr
         type(c_ptr), value              :: dmat
         integer(c_int64_t), value       :: row_step
         integer(c_int), value           :: max_bins
         integer(c_int64_t), intent(out) :: cut_ptr(*)
         real(c_float), intent(out)      :: cut_values(*)
         integer(c_int64_t), value       :: cap
         integer(c_int64_t), intent(out) :: needed
         type(c_ptr), value              :: stream
         integer(c_int)                  :: rc
      end function

      ! ---- part 4 of ohxgb.h: the OH field reassembled on every GPU of a node, for a host that has MPI but no
      !      torch.distributed.  Rank 0 gets the id, MPI_Bcast carries its OHX_UNIQUE_ID_BYTES bytes, every rank
      !      (hipSetDevice done) inits; d_shard / d_full are DEVICE addresses, stream a hipStream_t (c_null_ptr = default)
      function OHXCommGetUniqueId(id) bind(C, name="OHXCommGetUniqueId") result(rc)
         import :: c_int, c_char
         character(kind=c_char), intent(out) :: id(*)
         integer(c_int)                      :: rc
      end function

      function OHXCommInitRank(id, nranks, rank, comm) bind(C, name="OHXCommInitRank") result(rc)
         import :: c_int, c_char, c_ptr
         character(kind=c_char), intent(in) :: id(*)
         integer(c_int), value              :: nranks, rank
         type(c_ptr), intent(out)           :: comm
         integer(c_int)                     :: rc
      end function

      function OHXCommFree(comm) bind(C, name="OHXCommFree") result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: comm
         integer(c_int)     :: rc
      end function

      function OHXCommInfo(rccl_version) bind(C, name="OHXCommInfo") result(rc)
         import :: c_int
         integer(c_int), intent(out) :: rccl_version
         integer(c_int)              :: rc
      end function

      function OHXShardRows(nrows_total, nranks, rank, row0, nrows) bind(C, name="OHXShardRows") result(rc)
         import :: c_int, c_int64_t
         integer(c_int64_t), value       :: nrows_total
         integer(c_int), value           :: nranks, rank
         integer(c_int64_t), intent(out) :: row0, nrows
         integer(c_int)                  :: rc
      end function

      function OHXAllGatherOH(comm, d_shard, nrows_local, nrows_total, d_full, stream) &
            bind(C, name="OHXAllGatherOH") result(rc)
         import :: c_int, c_ptr, c_int64_t
         type(c_ptr), value        :: comm, d_shard, d_full, stream
         integer(c_int64_t), value :: nrows_local, nrows_total
         integer(c_int)            :: rc
      end function

      function c_strlen(s) bind(C, name="strlen") result(n)
         import :: c_ptr, c_size_t
         type(c_ptr), value :: s
         integer(c_size_t)  :: n
      end function
   end interface

contains

   !  NUL-terminated copy of a trimmed Fortran string
   function ohx_c_string(s) result(cs)
      character(len=*), intent(in) :: s
      character(kind=c_char, len=:), allocatable :: cs
      cs = trim(s)//c_null_char
   end function

   !  The library's per-thread error text (the reference never asks for it; it only
   !  asserts rc == 0, OH_GridCompMod.F90:252-265,353-378).
   function ohx_last_error() result(msg)
      character(len=:), allocatable :: msg
      type(c_ptr) :: p
      character(kind=c_char), pointer :: chars(:)
      integer :: n, i
      p = XGBGetLastError_c()
      if (.not. c_associated(p)) then
         msg = ''
         return
      end if
      n = int(c_strlen(p))
      call c_f_pointer(p, chars, [n])
      allocate(character(len=n) :: msg)
      do i = 1, n
         msg(i:i) = chars(i)
      end do
   end function

end module ohx_bindings
