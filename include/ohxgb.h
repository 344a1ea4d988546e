/*
 * ohxgb.h — C ABI of libohxgb.so, the MI355X (gfx950) OH-chemistry predictor.
 *
 * Drop-in boundary: GEOS-ESM/QuickChem reaches XGBoost through the Fortran
 * module xgb_fortran_api, which binds eleven XGBoost C-API symbols with
 * ISO_C_BINDING.  libohxgb.so exports those same symbols, with the C signatures
 * the bindings imply, so QuickChem links against it instead of libxgboost 1.6.0
 * (reference Shared/CMakeLists.txt:8-12) without touching a line of Fortran.
 * Each declaration below cites the reference binding it replaces
 * (paths relative to the QuickChem tree).
 *
 * Everything computes on the GPU.  There is no CPU fallback: a compute call
 * made where no HIP device is usable returns -1 and XGBGetLastError() says so.
 *
 * Conventions (xgboost 1.6.0 c_api.h): every function returns 0 on success and
 * -1 on failure; the message is then available, per thread, from
 * XGBGetLastError().  Handles are opaque pointers created by the library and
 * released by the matching *Free call.
 */
#ifndef OHXGB_H_
#define OHXGB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* DMatrixHandle;
typedef void* BoosterHandle;
typedef uint64_t bst_ulong;

/* ------------------------------------------------------------------------
 * Part 1 — the XGBoost C-API subset QuickChem binds
 * ------------------------------------------------------------------------ */

/* Last error message of the calling thread.  Not bound by the reference (it
 * only asserts rc == 0, OH_GridComp/OH_GridCompMod.F90:252-265,353-378). */
const char* XGBGetLastError(void);

/* Shared/xgb_fortran_api.F90:86-94, called at OH_GridCompMod.F90:251 (1x27
 * dummy) and :347 (the N x 27 batch).  `data` is row-major [nrow][ncol]
 * (Fortran xx_carr(27,N)); it is copied to HBM before the call returns, the
 * caller may free it at once.  Entries equal to `missing`, or NaN, are missing
 * values.  As in xgboost 1.6.0, +-inf in the data is an error unless `missing`
 * is itself infinite. */
int XGDMatrixCreateFromMat(const float* data, bst_ulong nrow, bst_ulong ncol, float missing, DMatrixHandle* out);

/* Shared/xgb_fortran_api.F90:45-48, called at OH_GridCompMod.F90:264,377. */
int XGDMatrixFree(DMatrixHandle handle);

/* Shared/xgb_fortran_api.F90:98-103 and :107-112 (bound, unused by OH). */
int XGDMatrixNumRow(DMatrixHandle handle, bst_ulong* out);
int XGDMatrixNumCol(DMatrixHandle handle, bst_ulong* out);

/* Shared/xgb_fortran_api.F90:35-40 and :53-58 (bound, unused by OH).
 * SaveBinary writes this library's own dense container ("OHXDMAT1");
 * CreateFromFile reads that container, or CSV text when the name ends in
 * ".csv" or carries "?format=csv" (all columns are features). */
int XGDMatrixSaveBinary(DMatrixHandle handle, const char* fname, int silent);
int XGDMatrixCreateFromFile(const char* fname, int silent, DMatrixHandle* out);

/* Shared/xgb_fortran_api.F90:76-82, called at OH_GridCompMod.F90:256.  The
 * reference passes ONE handle by value with len == 0 ("setting this to 27
 * results in a Seg Fault", :255): `dmats` is never dereferenced when len == 0,
 * and cached matrices are not needed for prediction in any case. */
int XGBoosterCreate(const DMatrixHandle dmats[], bst_ulong len, BoosterHandle* out);

/* Shared/xgb_fortran_api.F90:116-119 (the reference leaves it commented out,
 * OH_GridCompMod.F90:389-392). */
int XGBoosterFree(BoosterHandle handle);

/* Shared/xgb_fortran_api.F90:19-23, called at OH_GridCompMod.F90:261.  Format
 * by extension as in xgboost 1.6.0: ".json" JSON, ".ubj" UBJSON (draft 12),
 * anything else the legacy binary format of the production ".model"/".bin"
 * files (OH_GridComp/OH_instance_OH.rc:17-20). */
int XGBoosterLoadModel(BoosterHandle handle, const char* fname);

/* Shared/xgb_fortran_api.F90:27-31 (bound, unused by OH). */
int XGBoosterSaveModel(BoosterHandle handle, const char* fname);

/* Same loader from memory (xgboost c_api.h; not bound by the reference). */
int XGBoosterLoadModelFromBuffer(BoosterHandle handle, const void* buf, bst_ulong len);

/* Shared/xgb_fortran_api.F90:62-72, called at OH_GridCompMod.F90:356 with
 * option_mask = 0, ntree_limit = 0, training = 0 (:231-235).
 *   option_mask: 0 normal, 1 output margin, 16 leaf indices; others refused.
 *   ntree_limit: 0 = all trees.
 * *out_result points at a host buffer owned by the booster, valid until the
 * next predict on that booster or XGBoosterFree (the reference never frees
 * it, :362,381).  *out_len = nrow (asserted at :359).
 *
 * Boosters with several output groups (G = max(num_class, num_target) >= 2:
 * multi:softprob, multi:softmax, 1.6.0's multi-target regression;
 * OHXBoosterGetNumGroups), as xgboost 1.6.0 lays them out, row-major:
 *   option_mask 1                         [nrow][G] margins
 *   option_mask 0, identity objective     [nrow][G] margins
 *   option_mask 0, multi:softprob         [nrow][G] softmax of the row's margins
 *   option_mask 0, multi:softmax          [nrow]    index of the row's first maximal margin, as float
 *   option_mask 0, any other objective    refused, as for one group
 *   option_mask 16                        [nrow][L] leaf ids, trees in FILE order
 * Group g's margin is the base margin plus the leaves of the trees with
 * tree_info == g, added in file order; a group without trees has the base
 * margin.  ntree_limit = k > 0 means the first k rounds: file trees
 * [0, L = min(T, k * G)) (1.6.0's GetIterationFromTreeLimit, num_parallel_tree
 * 1; unpinned against libxgboost, as everything here).  *out_len = nrow * G
 * (nrow for multi:softmax, nrow * L for leaf ids).  Fortran callers: size the
 * c_f_pointer of out_result by out_len, not by the number of rows.
 * OHXBoosterPredictDevice writes the same into d_out (sized accordingly) and
 * is not capturable for such a booster: -1 inside a stream capture, nothing
 * enqueued.  The fields forms, OHXBoosterPredictContribsFields[Device] and
 * OHXBoosterRun1[Device] are single-output and refuse such a booster.
 *
 * Categorical splits (xgboost 1.6.0's JSON / UBJSON: split_type, categories, categories_nodes,
 * categories_segments, categories_sizes; docs/14_categorical.md).  A node with split_type 1 on feature f holds a set S
 * of categories, non-negative integers of at most OHX_MAX_CATEGORY.  With M = max(S) and
 * Size = 32 * ceil((M + 1) / 32) - the bit capacity of 1.6.0's per-node bit field - a row with v = x[f] goes, the
 * tests made in this order:
 *   v missing (NaN, equal to the matrix's `missing`, a column the matrix lacks)   the default child, as at a
 *                                                                                numeric split: tested FIRST
 *   v < 0 or v >= Size (compared as floats)                                       left if default_left, else right
 *   else, c = (int)v (truncation: 2.7 is category 2, -0.0 is 0), c in S           RIGHT
 *   else                                                                          left
 * Size is checked before the cast, so no float outside int range is cast.  Numeric nodes, the leaf sum (base plus
 * the leaves in tree order, float32, per row), ntree_limit, the base margin and the +-inf rule of both matrix forms
 * are unchanged.  This restates common::Decision / GetNextNode<has_missing, has_categorical> of xgboost 1.6.0 and is,
 * as everything here, unpinned against a real libxgboost.
 * Such a booster (one output group only: several are refused at load) predicts through XGBoosterPredict and
 * OHXBoosterPredictDevice with option_mask 0 (identity objectives), 1 and 16, by kernels of its own (node format 3 of
 * OHXBoosterGetInfo); "ohx_kernel" and the other launch knobs are accepted and do not select a kernel for it (a grid said
 * with OHXDMatrixSetGrid and "ohx_brick" shape the tile kernel's waves as they do for every booster).  Bit
 * for bit the same whatever the batch, the form or the kernel.  OHXBoosterPredictDevice is not capturable for it
 * (-1 inside a stream capture, nothing enqueued).  XGBoosterSaveModel writes it as JSON or UBJSON; the legacy binary
 * format is refused, as by 1.6.0.  Refused at the top of the call, with a message that says "categorical":
 * OHXBoosterPredictFields[Device], OHXBoosterPredictContribs[Device], OHXBoosterPredictContribsFields[Device],
 * OHXBoosterPredictInteractions[Device], OHXBoosterRun1[Device]. */
#define OHX_MAX_CATEGORY 16777215 /* 2**24 - 1: larger integers are not exact in float32 */
int XGBoosterPredict(BoosterHandle handle, DMatrixHandle dmat, int option_mask, unsigned ntree_limit, int training,
                     bst_ulong* out_len, const float** out_result);

/* xgboost c_api.h; not bound by the reference.  Understood names:
 *   "ohx_kernel"      auto | ring | super1 | super2 | super3 | super4 | packed1 | packed2 |
 *                     packed4 | wide : node format and trees in flight per lane.  ring: super-nodes, the records
 *                     of a walk's first four steps resident in LDS, 16 wavefronts per block walking the same four
 *                     trees at a time (the big batches of a 27-feature booster; everything else of such a booster
 *                     goes the super2 way).  auto = ring for 27-feature boosters of 5 or more steps per tree
 *                     (where it is faster: 20 % at the OH booster's 9 steps), else super2
 *   "ohx_ring_rounds" ring kernels: tiles per wavefront and launch (default 64; 0 = one launch);
 *                     at most 16 for rows not known to lie on a grid, 4 for rows in no order (clustering pass)
 *   "ohx_reserve_cus" ring kernels (rows): compute units left free, 0..128 (default 0).  A ring block owns its CU for the
 *                     length of a launch; a collective enqueued beside the predict (OHXAllGatherOH, torch.distributed)
 *                     otherwise only gets on the chip at a launch boundary
 *   "ohx_run1_pieces" experiment knob of OHXBoosterRun1[Device]: n > 1 walks n ranges of j one after the other, with the
 *                     feature engineering of the next and the post-processing of the last on a second stream beside
 *                     the walk; 0 and 1 = one piece (default: measured, pieces are slower - profiles/r05_sweeps.txt)
 *   "ohx_copy_engine" kernel (default) | dma | auto, process-wide (the handle may be NULL): how REGISTERED host arrays
 *                     cross PCIe.  kernel = a list of arrays per launch of a copy kernel (the GPU reads / writes the
 *                     caller's memory itself; the one list that crosses under the walk by DMA); dma = every array by
 *                     hipMemcpyAsync (the DMA engines: a fixed price per array, no wave on any CU); auto = the host form
 *                     of OHXBoosterRun1 times its own first ticks both ways (two of warm-up, then eight of each) and keeps
 *                     the faster, trying again every 512 ticks.  Measured at 1, 2, 3 and 6 ranks on a card
 *                     (profiles/r06_ranks_per_gpu_block_48x24_engines.json): the kernels win at every count (a rank's tick
 *                     0.29 against 0.61 ms alone, 1.35 against 3.13 ms at six), auto says so every time, and its trial
 *                     costs the tail - hence not the default.  The same bits either way.
 *   "ohx_register_host"  0 | 1, process-wide (the handle may be NULL): the host arrays handed to OHXBoosterRun1,
 *                     OHXOHPostProcess and OHXBoosterPredictFields are registered with the GPU driver the first time
 *                     they are seen and moved by DMA - a rank-sized block's forty arrays by ONE copy launch - from
 *                     then on (a 48 x 24 x 72 block's Run1 tick: 0.98 -> 0.52 ms; six ranks sharing the GPU: 3.3 ->
 *                     0.7 ms).  A CONTRACT: every array passed while this is on must stay allocated until
 *                     OHXUnregisterHost(array), OHXReleaseScratch() or the end of the process (MAPL's state arrays
 *                     do); an array that is freed while registered is reached through a registration the library
 *                     cannot check - ROCm's follows the process's page tables, so the next copy faults rather than
 *                     reads stale pages, but it fails.  Nothing is unregistered under a copy in flight (the device
 *                     is synchronised first).  Default 0 (the OH shell turns it on: register_host_arrays, default T)
 *   "ohx_copy_blocks" process-wide: blocks per launch of the kernel that moves registered host arrays (default 64; 0 = a
 *                     block per KiB).  Small on purpose: a chip full of wavefronts waiting on PCIe moves a rank's arrays
 *                     slower and keeps every other stream's kernels from starting meanwhile.
 *                     Launches that WRITE the caller's arrays (a tick's results, at its end) use 512 blocks
 *                     (OHX_COPY_BACK_BLOCKS in the environment, read once; 0 = as "ohx_copy_blocks")
 *   "ohx_tree_tops"   auto | on | off : super-nodes: fetch a tree's first records with one coalesced load per
 *                     wavefront (auto = forests of 7 or more steps per tree, where it is faster)
 *   "ohx_cluster"     auto | on | off : group rows of no known order by the decisions they take at the top of
 *                     the first trees before walking them ("ohx_cluster_trees", "ohx_cluster_steps",
 *                     "ohx_cluster_zorder" shape the key)
 *   "ohx_tree_split"  auto | off | 2..10 : a batch that leaves half of the chip's wave slots empty has its trees cut
 *                     into runs walked by different wavefronts, the leaves summed in tree order by a second launch
 *                     (a predict on 10 000 .. 300 000 rows takes a third of the time; margins unchanged, bit for bit)
 *   "ohx_defer_missing"  auto | on | off : rows that hold missing values are predicted by a second, small launch
 *                     instead of putting their whole wavefront on the missing-aware walk (auto = batches of 262 144
 *                     rows and more)
 *   "ohx_launches_per_residency"  tiles per wave per launch (default 2; 0 = one launch)
 *   "ohx_brick" = "a,b,c", "ohx_brick_k_fastest", "ohx_prefetch", "ohx_coop_rows", "ohx_xcd_remap", "ohx_lds_pad", "ohx_overlap_group"
 *                     launch-shape knobs behind profiles/ *_sweeps.txt; the defaults are the measured best
 *   "ohx_top_levels", "ohx_line_slots", "ohx_min_chunk"  placement of the packed format
 *   "ohx_super_pack"  0..3 : which super-node groups of a tree share a 128-byte line below the records of a walk's first
 *                     four steps (0 = breadth first, 1 = trees on 128-byte bases, 2 = + sibling pairs in one line, 3 = +
 *                     families in two lines; docs/03_hbm_layout.md); the margins are the same bits whatever the value
 *   "ohx_contribs_split"  auto | off : OHXBoosterPredictContribs[Device]: a batch that leaves most of the chip's wave
 *                     slots empty has its trees split over waves and the per-tree contributions summed in tree order by a
 *                     second launch (auto), or one wave per 64 rows walks every tree (off); the same bits either way;
 *                     the same for OHXBoosterPredictInteractions[Device] (there a wave per 64 rows and feature)
 *   "ohx_cat_kernel"  auto | direct : boosters with categorical splits: direct = margins by the kernel without LDS
 *                     too (auto: the tile kernel where a block's tiles fit a CU's LDS, up to 160 features)
 *   "ohx_device"      HIP device ordinal for this booster
 *   "ohx_objective"   squarederror (default) | pseudohuber | quantile : the loss the OHXBoosterBoostTrees* calls fit, as the
 *                     (gradient, hessian) pair of a row (defined bit for bit with OHXBoosterBoostTreesWeighted below;
 *                     docs/26_objectives.md).  Any other value returns -1 and the message names "ohx_objective".  Kept on
 *                     the handle, written into no model file; the forest's own objective name is not changed.  The name
 *                     "objective" without the prefix is an xgboost parameter and is ignored.  With pseudohuber the calls
 *                     that keep row counts, not hessian sums - OHXBoosterBoostTrees[Device], OHXBoosterBoostTreesEval[Device]
 *                     - and OHXBoosterRefitLeaves[Device] return -1 before anything is enqueued; the message names
 *                     OHXBoosterBoostTreesWeighted.  With quantile (the pinball loss at "ohx_quantile_alpha", with leaves that
 *                     are weighted quantiles of residuals; docs/32_quantile_objective.md) the same calls are refused the same
 *                     way, and so are OHXBoosterBoostTreesDeep[Device] and ...DeepSampled[Device] at any depth and every
 *                     setting that replaces the split kernels - ohx_reg_alpha or ohx_max_delta_step not 0, a non-zero
 *                     ohx_monotone_constraints entry, ohx_colsample_bylevel or ohx_colsample_bynode below 1; each message
 *                     names what to call or unset.  It acts on OHXBoosterBoostTreesWeighted[Device] and ...Sampled[Device]
 *   "ohx_huber_slope" the slope delta of pseudohuber: a decimal number, finite, 2^-10 <= delta <= 256 (default 1).
 *                     Anything else returns -1 and the message names "ohx_huber_slope"
 *   "ohx_quantile_alpha" alpha of the quantile objective and of the quantile metric: a decimal number, finite,
 *                     2^-10 <= alpha <= 1 - 2^-10 (default 0.5), parsed as "ohx_huber_slope" is.  Anything else ("", "0",
 *                     "1", "nan", "1x", "0.5 ", "-0.1") returns -1 and the message names "ohx_quantile_alpha".  Kept on the
 *                     handle, written into no model file
 *   "ohx_grow_pairs"  auto (default) | on : for tests and measurement.  on = squared error goes through the pair kernels
 *                     too (a pass that writes every row's pair once a round, and histogram kernels that read it); auto =
 *                     only an objective that needs them does.  The same bits either way.  With none of the three set
 *                     every boost call runs the kernels it ran before they existed
 *   "ohx_reg_alpha"   the L1 threshold alpha on a node's gradient sum: a decimal number, finite, >= 0 (default 0)
 *   "ohx_max_delta_step" the bound m on |base_weight|: a decimal number, finite, >= 0 (default 0 = off).  Both enter the
 *                     gain and the leaf of OHXBoosterBoostTreesWeighted, ...Sampled, ...Deep and ...DeepSampled as defined
 *                     with the Weighted call below (docs/27_regularisation_and_metrics.md).  Anything else ("", "1x",
 *                     "1 ", nan, inf, a negative number) returns -1 and the message names the parameter
 *   "ohx_eval_metric" rmse (default) | mae | pseudohuber | quantile : what train_rmse[] and eval_rmse[] of those four calls hold and
 *                     what their stop rule compares (defined with the Weighted call below; delta is "ohx_huber_slope"
 *                     and alpha "ohx_quantile_alpha" whatever the objective).  Any other value returns -1 and the message names "ohx_eval_metric".
 *                     All three are kept on the handle and written into no model file; the names without the prefix are
 *                     xgboost's and stay ignored.  While ohx_reg_alpha or ohx_max_delta_step is not 0 or the metric is
 *                     not rmse, OHXBoosterBoostTrees[Device] and OHXBoosterBoostTreesEval[Device] (row counts and
 *                     two-word sums) return -1 before anything is enqueued, and while ohx_reg_alpha or
 *                     ohx_max_delta_step is not 0 so does OHXBoosterRefitLeaves[Device] (it would refit unregularised
 *                     leaves); the message names OHXBoosterBoostTreesWeighted.  With all three at their defaults every
 *                     boost call runs the kernels it ran before they existed
 *   "ohx_monotone_constraints" the monotone constraints of boosting: `(` entries `)` with the entries separated by `,`,
 *                     each -1, 0, 1 or +1; spaces and tabs between tokens are ignored, so Python's str((1, 0, -1)) is
 *                     valid; () is the default, none.  Entry f is c_f, the constraint on feature f of the booster: +1 =
 *                     a new tree must not fall as x_f rises, -1 = must not rise, 0 = free; fewer entries than
 *                     num_feature means 0 for the rest.  At most 128 entries.  Anything else ("", no parentheses, 2, 1.0,
 *                     a trailing comma, 129 entries) returns -1 and the message names "ohx_monotone_constraints".  A
 *                     list whose entries are all 0 is the default: such a call launches nothing new and produces the
 *                     default's bytes.  Kept on the handle and written into no model file; the name without the prefix
 *                     is xgboost's and stays ignored.  It acts on OHXBoosterBoostTreesWeighted, ...Sampled, ...Deep and
 *                     ...DeepSampled as defined with the Weighted call below (docs/28_monotone_constraints.md).  More
 *                     entries than num_feature make each of those calls return -1 before anything is enqueued, and the
 *                     message names the parameter.  While some c_f != 0, OHXBoosterBoostTrees[Device] and
 *                     OHXBoosterBoostTreesEval[Device] (row counts; their split kernels keep no intervals) and
 *                     OHXBoosterRefitLeaves[Device] (a refit would undo the intervals) return -1 before anything is
 *                     enqueued; the message names OHXBoosterBoostTreesWeighted.  In every refusal the forest and the
 *                     outputs are untouched
 *   "ohx_colsample_bylevel", "ohx_colsample_bynode" boosting: the fraction of a tree's features that a level of the tree
 *                     sees, and the fraction of a level's features that one node may split on.  Each is a decimal float,
 *                     finite, with 0 < v <= 1; the default is 1.  Anything else ("", not a number, 0, a negative, > 1,
 *                     nan, inf) returns -1 and the message names the parameter.  Both are kept on the handle and written
 *                     into no model file; the names without the prefix are xgboost's and stay ignored.  They act on
 *                     OHXBoosterBoostTreesSampled[Device] and OHXBoosterBoostTreesDeepSampled[Device], the calls that
 *                     carry a seed, as defined with the Sampled call below (docs/29_colsample_level_node.md).  While
 *                     either is not 1, OHXBoosterBoostTrees[Device], ...Eval[Device], ...Weighted[Device] and
 *                     ...Deep[Device] return -1 before anything is enqueued; the message names
 *                     OHXBoosterBoostTreesSampled, and the forest and every output are untouched.
 *                     OHXBoosterRefitLeaves chooses no split and is unaffected
 *   "ohx_interaction_constraints" the interaction constraints of boosting: which features may act together in one
 *                     tree.  The value is a list of groups, `[` groups `]` with the groups separated by `,`; each group
 *                     is `[` ids `]` with the ids separated by `,`; each id is a decimal integer without sign.  Spaces
 *                     and tabs between tokens are ignored, so Python's str([[0, 2], [1, 3, 4]]) is valid; [] is the
 *                     default, none.  At most 64 groups; every group is non-empty and its ids are distinct; every id is
 *                     below 128; a feature may appear in several groups.  Anything else ("", [[]], [0, 1], [[0, 0]],
 *                     [[1.0]], [[-1]], a trailing comma, 65 groups, an id of 128) returns -1, the message names
 *                     "ohx_interaction_constraints", and the handle keeps its previous value.  Kept on the handle and
 *                     written into no model file; the name without the prefix is xgboost's and stays ignored.  It acts
 *                     on OHXBoosterBoostTreesWeighted, ...Sampled, ...Deep and ...DeepSampled as defined with the
 *                     Weighted call below (docs/35_interaction_constraints.md).  An id >= num_feature makes every boost
 *                     call return -1 before anything is enqueued.  The constraints are inactive when the list is empty
 *                     or when some group holds every feature 0 .. num_feature - 1: such a call launches nothing new and
 *                     produces the default's bytes.  While they are active, OHXBoosterBoostTrees[Device] and
 *                     OHXBoosterBoostTreesEval[Device] (row counts; their split kernels keep no feature sets; the
 *                     message names OHXBoosterBoostTreesWeighted), ohx_objective=quantile, and ohx_colsample_bylevel or
 *                     ohx_colsample_bynode where they take a feature away (n_lvl != n_sel or n_node != n_lvl) return -1
 *                     before anything is enqueued; every message names the parameter, and the forest and every output
 *                     are untouched.  OHXBoosterRefitLeaves chooses no split and is unaffected
 * None of them changes a prediction.
 * xgboost's own parameter names ("nthread", "predictor", ...) are accepted and
 * ignored. */
int XGBoosterSetParam(BoosterHandle handle, const char* name, const char* value);

/* ------------------------------------------------------------------------
 * Part 2 — device-resident and fused entry points (additive)
 * ------------------------------------------------------------------------ */

/* HIP device count, or -1 with an error message when HIP is unusable. */
int OHXDeviceCount(int* out);

/* As XGDMatrixCreateFromMat, but `d_data` already lives in HBM.  The matrix
 * BORROWS the pointer (no copy); it must stay valid until XGDMatrixFree.
 * The inf check of the host path is folded into the predict kernels instead:
 * a predict on data holding +-inf fails (OHXBoosterCheck reports it).
 * Ordering: the library reads the rows on streams of its own.  The host-form
 * calls on such a matrix (XGBoosterPredict, XGDMatrixSaveBinary) first wait for
 * everything enqueued so far on the legacy default stream, hence on every
 * blocking stream; rows filled on a NON-blocking stream of the caller's must
 * be synchronised by the caller, or the *Device forms used, which take the
 * producing stream as an argument. */
int OHXDMatrixCreateFromDevice(const float* d_data, bst_ulong nrow, bst_ulong ncol, float missing, DMatrixHandle* out);

/* Optional hint, any DMatrix: its rows are rows row0, row0+1, ... of the gather
 * m = (i-1) + im*((j-1) + jm*(k-k1)) that predict_OH_with_XGB builds
 * (OH_GridCompMod.F90:309-345); row0 > 0 for a rank's contiguous shard.  Predictions do not
 * change.  The kernels then give each wavefront a brick of 4x4x4 (or 8x4x2, 8x8x1) neighbouring
 * gridcells instead of 64 consecutive rows, which measures 1.19x faster on C360 L72 because
 * neighbours in all three directions walk the same tree nodes.  im = jm = 0 says "no grid": 64 consecutive
 * rows per wavefront, and the library does not look for a level size either. */
int OHXDMatrixSetGrid(DMatrixHandle handle, int im, int jm, bst_ulong row0);

/* What the library knows about the rows of a DMatrix (any pointer may be NULL).  Without a hint the
 * library looks for the level size by itself, ONCE per matrix, at the first predict on it: the reference's
 * gather stacks levels and its first column, LAT, is a 2-D field (OH_GridCompMod.F90:313), so that column
 * repeats bit for bit with period im*jm.  A period found that way is reported as im = level size, jm = 1,
 * inferred = 1 and is worth as much as the full hint to within 1 % (runs of 8 cells x 8 levels per
 * wavefront).  For a matrix the library copied itself (XGDMatrixCreateFromMat) this call looks if nobody
 * has yet; for a matrix over device memory it reports what is known so far. */
int OHXDMatrixGetGrid(DMatrixHandle handle, int* im, int* jm, bst_ulong* row0, int* inferred);

/* The same search on demand.  Waits for `stream` (the rows must be there), then looks; *found (may be
 * NULL) says whether a level size was found.  Replaces any earlier hint.  A device-resident caller that
 * wants OHXBoosterPredictDevice never to wait calls this (or OHXDMatrixSetGrid) beforehand: the first
 * predict on a matrix nobody has described waits for its stream once to look.  For matrices the library copied
 * itself (XGDMatrixCreateFromMat) that is once per SHAPE: what the first predict finds is remembered by (rows,
 * columns) for the life of the process, so a host that creates and frees its matrix every tick, as the reference
 * does (OH_GridCompMod.F90:347,377), pays the search and the wait at the first tick only.  This call and
 * OHXDMatrixGetGrid always look. */
int OHXDMatrixInferGrid(DMatrixHandle handle, void* stream, int* found);

/* Predict straight into device memory: d_out[nrow] margins (or [nrow][ntree]
 * leaf ids with option_mask 16).  `stream` is a hipStream_t (NULL = default
 * stream); the call only enqueues work (but see OHXDMatrixInferGrid for the first
 * predict on an undescribed matrix).  OHXBoosterCheck surfaces errors the
 * kernels raised (inf in the input; without it a device form's caller never
 * learns of them).  A booster keeps single scratch buffers
 * (error flags, Run1 intermediates, staging): calls on ONE booster must not run
 * concurrently on two streams or threads; different boosters are independent.
 * hipGraphs: this call and OHXBoosterPredictFieldsDevice may be made on a stream
 * that is being captured - what they enqueue is launches, memsets and copies on
 * `stream` - once ONE plain call of the same shape has been made on the booster
 * and the matrix (it allocates the booster's buffers, uploads the model and looks
 * at the matrix).  A capture that would have to allocate or to wait returns -1
 * with a message that says so and enqueues nothing.  While capturing the library
 * leaves out what its host side does beside the launches to adapt the NEXT call
 * (the read-back of how many rows went to the second launch): a replay walks the
 * way the last plain call decided, and is bit-identical to a plain call on the
 * same contents (tests/test_gpu_graph.py).  OHXBoosterRun1Device is not
 * capturable: it waits for its slab count. */
int OHXBoosterPredictDevice(BoosterHandle handle, DMatrixHandle dmat, int option_mask, unsigned ntree_limit,
                            float* d_out, void* stream);
int OHXBoosterCheck(BoosterHandle handle, void* stream);

/* Per-feature contributions of each row, as xgboost 1.6.0's XGBoosterPredict with pred_contribs (approximate = 0:
 * exact TreeSHAP, option_mask 4 there) or approx_contribs (approximate = 1, option_mask 8 there).  A separate entry
 * point: XGBoosterPredict's option_mask is unchanged (and already departs from 1.6.0's bits: 16 = leaf indices here).
 * Output: nrow x (F + 1) float32, row-major, F = the booster's num_feature; column F is the bias.  *out_len =
 * nrow * (F + 1); *out_result is a host buffer owned by the booster, valid until its next contribs call or
 * XGBoosterFree.  Both matrix forms; missing values as in the predict paths (NaN, the matrix's `missing`, columns
 * the matrix does not have).  ntree_limit: 0 = all trees, else the first ntree_limit.
 * Semantics, f = the margin XGBoosterPredict(option_mask = 1) returns; for each tree t of the range:
 *   mean(n)  = the leaf value at a leaf, (mean(l) * cover(l) + mean(r) * cover(r)) / cover(n) at a split, in float in
 *              this order (1.6.0 FillNodeMeanValues); cover = the node's sum_hess.
 *   bias     = sum over trees of mean_t(root) in tree order from 0, then + the margin's base.
 *   exact    = path-dependent TreeSHAP (Lundberg et al. 2020, Algorithm 2): at a split on feature j the row goes left
 *              if x_j < cond, a missing value takes the default child; zero fraction cover(child) / cover(parent),
 *              one fraction 1 if the row takes that child else 0; a feature that occurs again on a path has its
 *              fractions multiplied into one element; phi_j goes to column j.
 *   approximate = 1.6.0's CalculateContributionsApprox: along the row's path, mean(next) - mean(current) to the
 *              split feature's slot, leaf - mean(last) to the last split's slot.
 *   Each tree's contributions are accumulated on their own and added into the row's totals in tree order (1.6.0's
 *   this_tree_contribs -> p_contribs).  Local accuracy: sum_j out[r][j] == f[r] up to rounding.  A row's bits do not
 *   depend on the batch it is in, and the host and device forms agree bit for bit.  As everywhere in this library,
 *   parity with libxgboost itself is not pinned (exact mode evaluates the same recurrences per leaf path in float32,
 *   so its rounding differs from 1.6.0's recursive walk).
 * Refused (-1, nothing enqueued): no model; an objective whose margin base is unknown (as option_mask 1); more
 * columns than features; a split whose cover is not finite and > 0 (the model has no cover statistics - 1.6.0 would
 * quietly produce NaN; a LEAF of cover 0 is accepted: its zero fraction is 0, and both modes give the Shapley value /
 * the Saabas walk, as 1.6.0's algorithm does); a root-to-leaf path over more than 32 distinct features, or more than 128 features; d_out
 * NULL; and, for the device form, a stream that is being captured: contributions are not capturable.
 * Tables (node means, a path table per leaf - docs/12_contributions.md for their size) are built at the first call
 * on a loaded model and kept until the model is replaced or XGBoosterFree; OHXReleaseScratch leaves them alone.
 * Contributions use buffers of their own, never one of the predict, fields or Run1 paths.  The device form only
 * enqueues on `stream`.  +-inf in the rows is reported by the host form only: there, as in predict, +-inf in ANY of a
 * row's columns is an error unless `missing` is itself infinite, in both modes (not only in the columns the row's
 * paths split on). */
/* Several output groups (G >= 2, XGBoosterPredict): [nrow][G][F+1], each group's block computed over the group's
 * trees (ntree_limit as in XGBoosterPredict), its bias the base margin plus the group's trees' root means in file
 * order; *out_len = nrow * G * (F+1), and the device form's d_out holds as many floats. */
int OHXBoosterPredictContribs(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                              bst_ulong* out_len, const float** out_result);
int OHXBoosterPredictContribsDevice(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                                    float* d_out, void* stream);

/* SHAP interaction values of each row, as xgboost 1.6.0's XGBoosterPredict with pred_interactions
 * (PredictInteractionContributions).  Output: nrow x (F + 1) x (F + 1) float32, row-major [row][i][k], F the
 * booster's num_feature, index F the bias.  *out_len = nrow * (F + 1)^2; *out_result is a host buffer owned by the
 * booster, valid until its next interactions call or XGBoosterFree.  Missing values, ntree_limit, the margin base and
 * the matrix forms as in OHXBoosterPredictContribs.  With phi = what OHXBoosterPredictContribs returns for the same
 * row, trees and `approximate` (bit for bit: the same launch fills it):
 *   exact (approximate = 0), i != k, both < F:  Phi_ik = (phi_k | i on - phi_k | i off) / 2, 1.6.0's conditioning
 *              inside path-dependent TreeSHAP: on a path that holds feature i (its element c, occurrences merged as in
 *              contributions) "on" multiplies the path's weight by c's one fraction, "off" by its zero fraction, and c
 *              leaves the permutation; phi_k is taken over the other elements.  Per path:
 *              1/2 (o_c - z_c) (o_k - z_k) leaf W(path without c, k), W the unwound path sum.  Paths without i add
 *              nothing to row i.  Each tree's row is accumulated on its own and added in tree order from 0.
 *   diagonal   Phi_ii = phi_i - sum_{k != i} Phi_ik in 1.6.0's float order: from 0, for k = 0 .. F add phi_i at
 *              k == i and subtract Phi_ik otherwise.
 *   bias       row F and column F are 0 except Phi_FF = phi_F (conditioning on index F matches no split).
 *   approximate = 1: 1.6.0's approximate walk ignores the condition, so every off-diagonal is 0 and the diagonal is
 *              OHXBoosterPredictContribs(approximate = 1)'s vector, bit for bit.
 *   A feature no tree of the range splits on has an all-zero row and column.  Mathematically Phi is symmetric, row i
 *   sums to phi_i and the matrix to the margin of XGBoosterPredict(option_mask = 1), up to rounding.  A row's bits do
 *   not depend on the batch, on "ohx_contribs_split", or on the form.  No float atomics.  Parity with libxgboost itself
 *   is not pinned (the recurrences run per leaf path in float32, and 1.6.0 stores (on - off) / 2 from double).
 * Refused (-1, nothing enqueued): everything OHXBoosterPredictContribs refuses (no model, unknown margin base, more
 * columns than features, a split without cover, a path over 32 distinct features, more than 128 features, d_out or
 * an output argument NULL, a stream being captured); +-inf in any column of a row in the host form unless `missing`
 * is itself infinite; an output that cannot be allocated.  The tables are the contributions' (built once, at the
 * first exact call of either entry point) plus, for exact mode, an index of the paths that hold each feature (one
 * 4-byte entry per path element; docs/12_contributions.md section 12.6).  The buffers are the booster's contributions
 * state's but none a contribs call uses, and never one of the predict, fields or Run1 paths; dropped with the model
 * and at XGBoosterFree, rebuilt after an "ohx_device" move.  Exact mode costs about (path length) times what exact
 * contributions cost per row: it is for subsets of rows.  The device form only enqueues on `stream`. */
/* Several output groups: [nrow][G][F+1][F+1], each group's block as OHXBoosterPredictContribs's. */
int OHXBoosterPredictInteractions(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                                  bst_ulong* out_len, const float** out_result);
int OHXBoosterPredictInteractionsDevice(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                                        float* d_out, void* stream);

/* Per-feature contributions from the MAPL fields, one 3-D array per feature: OHXBoosterPredictContribs without the
 * row matrix.  Inputs as OHXBoosterPredictFields, gather included: fields[f] is (im,jm,km) Fortran order, or (im,jm)
 * when is2d[f] != 0 (broadcast over the levels); field pl_feature is divided by 100 as a float32 division (-1: none);
 * a value equal to `missing`, or NaN, is missing; features at or past nfield (nfield <= num_feature) are missing.
 * Gridcell m = i + im*(j + jm*(k-k1)) for k = k1..k2 (1-based, inclusive).
 * Output: out[0..F], F the booster's num_feature; out[f] an (im,jm,km) Fortran-order array, out[F] the bias.  For
 * k1 <= k <= k2, out[f](i,j,k) is, bit for bit, what OHXBoosterPredictContribs returns at [m][f] (same `approximate`
 * and ntree_limit) for the row the fields kernels walk for gridcell m.  Levels outside k1..k2 are left untouched.  A
 * NULL out[f] is not computed into anything nor copied back; all NULL is refused.  k2 == k1 - 1 does nothing and
 * succeeds.  A gridcell's bits depend on neither the launch shape ("ohx_contribs_split" applies), the form, nor the
 * slab it is in.
 * Host form: host pointers; the slab (3-D fields: levels k1..k2 only) and the requested outputs are staged in buffers
 * of the booster's contributions state (never one of the predict, fields or Run1 paths; dropped with the model and at
 * XGBoosterFree, rebuilt after an "ohx_device" move), and the call returns when every requested out[f] is written.
 * +-inf in a gathered value of the slab (after the PL division) is an error unless `missing` is itself infinite, in
 * both modes.  Device form: device pointers, work enqueued on `stream`; +-inf is not checked (as in
 * OHXBoosterPredictContribsDevice); not capturable.
 * Refused (-1, nothing enqueued): what OHXBoosterPredictContribs refuses (no model, unknown margin base, a split
 * without cover, a path over 32 distinct features in exact mode, approximate not 0 or 1); what the fields forms
 * refuse, with their messages (nfield over num_feature or 32, a booster over 32 features, im, jm or km not positive, a
 * bad k range, NULL fields, is2d, out or field); every out[f] NULL; for the device form, a stream being captured. */
int OHXBoosterPredictContribsFields(BoosterHandle handle, const float* const fields[], const int32_t is2d[],
                                    int nfield, int pl_feature, int im, int jm, int km, int k1, int k2,
                                    float missing, int approximate, unsigned ntree_limit, float* const out[]);
int OHXBoosterPredictContribsFieldsDevice(BoosterHandle handle, const float* const d_fields[], const int32_t is2d[],
                                          int nfield, int pl_feature, int im, int jm, int km, int k1, int k2,
                                          float missing, int approximate, unsigned ntree_limit,
                                          float* const d_out[], void* stream);

/* Selected gridcells: choose cells of an (im,jm,km) block on the device, gather their rows from the fields into a
 * device row matrix for the rows forms (OHXDMatrixCreateFromDevice, then OHXBoosterPredictDevice, ...ContribsDevice,
 * ...InteractionsDevice: the expensive answers, for a column or a few thousand cells), scatter per-cell results back
 * into (im,jm,km) arrays.  None of the six calls takes a booster (docs/15_selected_cells.md).
 * A cell index is c = (i-1) + im*((j-1) + jm*(k-1)) for 1-based i, j, k: an int64 in [0, im*jm*km), the offset of the
 * cell in any (im,jm,km) Fortran-order array, whatever the slab.
 * Host forms take host pointers, stage through buffers of their own call (never a booster's; of 3-D arrays only the
 * levels that are needed cross PCIe) and return when the outputs are complete.  Device forms take device pointers,
 * only enqueue on `stream` (NULL = the default stream) and never wait; the first selection or scatter on a stream
 * allocates a 32 KiB table for that stream (so: one plain call before capturing).
 * d_status (device forms, may be NULL) is a word the kernels OR bits into and never clear:
 *   OHX_CELLS_OUT_OF_RANGE      a cell index outside [0, im*jm*km).  It is never dereferenced: the gather writes NaN
 *                               into every column of that row, the scatter skips the entry.
 *   OHX_CELLS_NOT_ASCENDING     the scatter's cells are not strictly ascending
 *   OHX_CELLS_OVER_CAP          the selection found more cells than cap
 * The host forms do all of the above and then return -1 with a message that names the first bad position.
 *
 * OHXSelectCells: the cells of the box i1..i2, j1..j2, k1..k2 (1-based, inclusive; i2 == i1 - 1 and the like: an empty
 * box, nothing selected, success) with a(i,j[,k]) > b(i,j[,k]), compared as float32, in strictly ascending order;
 * *count = how many.  a_is2d / b_is2d != 0: an (im,jm) array, the same for every level.  b == NULL: the scalar b0.
 * a == NULL: every cell of the box (b, b0 unused).  NaN on either side selects nothing.  So: a box or a column (a
 * NULL), a mask (a = mask, b0 = 0), the troposphere of OH Run1 (a = PL_MOD, b = TROPP 2-D).  When more than cap cells
 * are selected the first cap are written, the full count is reported and OHX_CELLS_OVER_CAP raised.  The order comes
 * from a scan of per-block counts, never from an atomic counter: the same array every run.  The device form writes
 * *d_count (an int64 on the device).
 *
 * OHXGatherCells: rows[ncell][nfield] float32, row-major; row n holds, for cell cells[n], what the fields forms put
 * in their tile for that gridcell before missing is canonicalised: fields[f] at the cell - at its (i,j) when is2d[f]
 * - and field pl_feature divided by 100 as a float32 division (-1: none).  Values equal to a missing marker stay as
 * they are: the DMatrix made over `rows` says what is missing, and features past nfield are columns it does not have.
 * Any order and duplicates are allowed in cells; ncell == 0 does nothing.  Refused: nfield < 1 or > 32, im, jm or km
 * not positive, NULL arrays (the fields forms' messages).
 *
 * OHXScatterCells: out3d[cells[n]] = values[n * stride + col]; every other cell is left untouched.  cells must be
 * strictly ascending.  An entry that is not above EVERY entry in front of it (so: one that is <= its predecessor) is
 * skipped and OHX_CELLS_NOT_ASCENDING raised, hence no cell is written twice and the result does not depend on
 * scheduling, whatever the list holds.  One call per output column. */
#define OHX_CELLS_OUT_OF_RANGE 1u
#define OHX_CELLS_NOT_ASCENDING 2u
#define OHX_CELLS_OVER_CAP 4u
int OHXSelectCells(int im, int jm, int km, int i1, int i2, int j1, int j2, int k1, int k2, const float* a, int a_is2d,
                   const float* b, int b_is2d, float b0, int64_t* cells, int64_t cap, int64_t* count);
int OHXSelectCellsDevice(int im, int jm, int km, int i1, int i2, int j1, int j2, int k1, int k2, const float* d_a,
                         int a_is2d, const float* d_b, int b_is2d, float b0, int64_t* d_cells, int64_t cap,
                         int64_t* d_count, uint32_t* d_status, void* stream);
int OHXGatherCells(const float* const fields[], const int32_t is2d[], int nfield, int pl_feature, int im, int jm, int km,
                   const int64_t* cells, int64_t ncell, float* rows);
int OHXGatherCellsDevice(const float* const d_fields[], const int32_t is2d[], int nfield, int pl_feature, int im, int jm,
                         int km, const int64_t* d_cells, int64_t ncell, float* d_rows, uint32_t* d_status, void* stream);
int OHXScatterCells(const float* values, int64_t stride, int64_t col, const int64_t* cells, int64_t ncell, float* out3d,
                    int im, int jm, int km);
int OHXScatterCellsDevice(const float* d_values, int64_t stride, int64_t col, const int64_t* d_cells, int64_t ncell,
                          float* d_out3d, int im, int jm, int km, uint32_t* d_status, void* stream);

/* Node visit counts, and the covers refreshed from them (docs/16_visit_counts.md).  Every contribution the library
 * computes is weighted by sum_hess, the cover the training run left in the model file: it answers "relative to the
 * training set".  These calls count how many rows of the CALLER's data pass every node, and make those counts the
 * covers, so that contributions answer "relative to this data" - xgboost's process_type = update, updater = refresh,
 * refresh_leaf = 0 on data whose hessian is 1 a row (reg:squarederror); parity with libxgboost is not pinned.
 * Counting.  OHXBoosterCountVisits walks every row of the matrix down EVERY tree exactly as a margin predict does (a
 * value that is NaN or equal to the matrix's `missing` takes the default child; a column the matrix lacks is missing;
 * x < cond goes left; +-inf is compared as the float it is - XGDMatrixCreateFromMat has already refused it for host
 * data, and the count calls raise no flag) and adds one to the counter of the leaf it reaches.  Both matrix forms.
 * Counts ACCUMULATE over calls until OHXBoosterResetVisitCounts, a model load or XGBoosterFree; an "ohx_device" move
 * resets them too.  The host form returns when the rows are added; the device form only enqueues on `stream` and is
 * not capturable.  Counts are integers (64-bit counters, integer atomics only, no float atomics): they do not depend
 * on the batch split, the launch shape, OHXDMatrixSetGrid, a knob, or the form.  Knobs, for tests and measurements:
 * "ohx_visits_kernel" = auto | global | lds (global: one 64-bit global add per distinct leaf and wave; lds: a tree
 * whose leaf histogram fits keeps it in LDS and flushes it once per block; auto = global, the faster of the two on the
 * C360 L72 batch, docs/16_visit_counts.md 16.4), "ohx_visits_lds_leaves" = n (with lds: a tree of more than n leaves
 * is counted the global way; auto or 0 = what fits a CU).
 * Reading.  OHXBoosterGetVisitCounts waits for `stream`, copies the leaf counters back and sums them up each tree on
 * the host.  *ntree = the trees; tree_offsets has *ntree + 1 entries; counts[tree_offsets[t] + n] is the number of
 * counted rows that passed node n of file tree t, in the file's node numbering; *rows_seen = the rows counted.  A
 * tree's root equals *rows_seen, a split equals the sum of its two children, unreachable and deleted slots are 0.  The
 * buffers are the booster's and stay valid until the next visits call on it.  Before any count: all zeros.
 * Refresh.  OHXBoosterRefreshCover waits for `stream` and stores, for every node reachable from a root,
 *   sum_hess := (float)count + prior_weight * sum_hess_old
 * in float32, the product rounded and then the sum (no fused multiply-add).  prior_weight = 0 is xgboost's refresh on
 * hessian-1 data; prior_weight > 0 blends the training cover in, so that subtrees no counted row reached keep a
 * positive cover.  All or nothing.  Refused with the forest untouched: nothing counted yet; prior_weight negative or
 * not finite; any SPLIT whose new cover would not be finite and > 0 (the message names the first such tree and node and
 * says how many of the splits there are; a LEAF of cover 0 stays legal, as in OHXBoosterPredictContribs).  On success
 * the contributions state is dropped exactly as a model load drops it (its tables are rebuilt at the next call), the
 * counters are kept, XGBoosterSaveModel writes the new sum_hess in all three formats, unreachable nodes keep their old
 * value, and every prediction is unchanged bit for bit: no walk reads cover.
 * Refused at the top of every one of the five calls: no model; a booster with categorical splits; several output
 * groups; NULL output arguments; and, for the count calls, more columns than features, no usable HIP device, and (the
 * device form) a stream that is being captured.  The visit state - the walk's own node format, the counters, the
 * result buffers - is built at first use and never shares a buffer with the predict, fields, Run1 or contributions
 * paths (a graph captured earlier still replays); dropped when a model is loaded and at XGBoosterFree;
 * OHXReleaseScratch leaves it alone.  Calls on ONE booster must not run concurrently (OHXBoosterPredictDevice). */
int OHXBoosterCountVisits(BoosterHandle handle, DMatrixHandle dmat);
int OHXBoosterCountVisitsDevice(BoosterHandle handle, DMatrixHandle dmat, void* stream);
int OHXBoosterGetVisitCounts(BoosterHandle handle, void* stream, bst_ulong* ntree, const bst_ulong** tree_offsets,
                             const uint64_t** counts, uint64_t* rows_seen);
int OHXBoosterResetVisitCounts(BoosterHandle handle);
int OHXBoosterRefreshCover(BoosterHandle handle, void* stream, float prior_weight);

/* Leaf refit (docs/17_leaf_refit.md): every tree keeps its structure and every leaf value is estimated again from the
 * CALLER's rows and labels - the other half of xgboost's process_type = update, updater = refresh: refresh_leaf = 1,
 * for reg:squarederror (gradient pred - label, hessian 1 a row).  The semantics restate xgboost 1.6.0 (TreeRefresher in
 * updater_refresh.cc, CalcWeight in param.h); parity with libxgboost is not pinned.
 * With T trees in file order, `base` the margin every prediction starts from and y the labels, for t = 0 .. T-1:
 *  1. pred_t[r] = base + new_leaf_0(r) + ... + new_leaf_{t-1}(r), float32, added in tree order per row: the sum a
 *     margin predict of the refit model makes.
 *  2. Row r reaches leaf l_t(r) of tree t exactly as a margin predict does - the walk of OHXBoosterCountVisits: NaN, the
 *     matrix's `missing` or a column the matrix lacks takes the default child; x < cond goes left; +-inf is compared as
 *     the float it is.  The walk does not read leaf values.
 *  3. g = pred_t[r] - y[r], one float32 subtraction; q = (int64) rint(g * 2^24): the product is exact in float32, the
 *     rounding is to nearest even.
 *  4. G_l = the sum of q over the leaf's rows, an int64; H_l = the number of those rows.  Integer adds only (no float
 *     atomics): the sums depend on neither the order of the rows, the launch shape, the form, nor
 *     OHXDMatrixSetGrid.
 *  5. w = (float)( -((double)G_l * 2^-24) / ((double)H_l + (double)lambda) ).
 *  6. new_leaf = w * eta, one float32 multiply (no fused multiply-add).  This is CalcWeight with reg_alpha = 0,
 *     max_delta_step = 0 and min_child_weight <= 1, times learning_rate.  The leaf's base_weight becomes w.
 *  7. A leaf no row reaches (H_l == 0): unvisited = 0 keeps its value and base_weight - a stated departure from
 *     xgboost: no row says anything about such a leaf; unvisited = 1 stores +0.0f in both, as xgboost does.
 * *leaves_refit (may be NULL) receives the number of leaves with H_l > 0 over all trees.
 * All or nothing: the forest is replaced only after every tree is done and the device's error word has been read back
 * clean.  Refused, with the forest untouched: no model; categorical splits; several output groups; an objective that
 * is not identity / squared error; NULL labels; eta not finite; lambda not finite or negative; unvisited not 0 or 1;
 * nlabel != the matrix's rows, or no rows; more than 2^31 rows; more columns than features; a stream that is being
 * captured (nothing is enqueued); no usable HIP device (no CPU fallback); a leaf-id buffer that cannot be allocated
 * (the message says how many bytes T * nrow * 4 is); and any row at any tree whose g is not finite or has
 * |g| >= 256 - the kernels raise a flag and the message says "label" (|q| < 2^32 and at most 2^31 rows is what keeps G
 * inside an int64).
 * On success leaf value and base_weight are replaced and every other array of the forest is untouched - sum_hess
 * included, which remains OHXBoosterRefreshCover's job.  Everything built from leaf values is dropped as a model load
 * drops it: the flattened device forests and the contributions state; a graph captured earlier is as stale as after
 * XGBoosterLoadModel.  The visit state holds no leaf value and is kept with its counters.  XGBoosterSaveModel writes
 * the new leaves in all three formats.
 * Both forms wait.  The host form stages the labels and returns when the forest is replaced.  The device form takes
 * d_labels in HBM (nlabel floats, ready on `stream`), enqueues on `stream` and waits for it once at the end, to read the
 * leaves and the error word back - as OHXBoosterRefreshCover waits.  The refit state (the walk's node format, T x nrow
 * leaf ids, the running prediction, the sums, the leaf tables, the staged labels) is the booster's own and never a
 * buffer of the predict, fields, Run1, contributions or visit paths; dropped when a model is loaded, by an
 * "ohx_device" move and at XGBoosterFree.  Calls on ONE booster must not run concurrently. */
int OHXBoosterRefitLeaves(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel, float eta,
                          float lambda, int unvisited, bst_ulong* leaves_refit);
int OHXBoosterRefitLeavesDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                                float eta, float lambda, int unvisited, bst_ulong* leaves_refit, void* stream);

/* Boosting new trees (docs/18_boost_trees.md): `rounds` depth-limited regression trees are fitted, one after another, to
 * the squared-error gradient of the CALLER's rows and labels with a histogram method on the GPU, and appended to the
 * forest - what a user with labels does after OHXBoosterRefitLeaves has taken the frozen structure as far as it goes.
 * Parity with libxgboost's hist updater is NOT claimed: the formulas restate xgboost 1.6.0's CalcGain and CalcWeight
 * (param.h) with reg_alpha = 0 and max_delta_step = 0; the candidate set and the tie rules are this library's own and
 * are stated here.  Every bit of the result is defined by integer sums and by double arithmetic in a stated order.
 * Cuts.  Feature f has ncut_f = cut_ptr[f+1] - cut_ptr[f] cut values c_0 < c_1 < ..., 0 <= ncut_f <= 254, finite and
 * strictly ascending; cut_ptr has F + 1 entries (F = the booster's num_feature, 1 <= F <= 128) and starts at 0.  A
 * row's bin for f is b = #{j : c_j <= x}, compared as float32: +inf gives ncut_f, -inf gives 0; NaN, the matrix's
 * `missing` or a column the matrix lacks gives the missing bin, 255.  Hence x < c_j exactly when b <= j: the float walk
 * of every predict path partitions rows exactly as the bins do.
 * OHXQuantileCuts (host only: no device, no booster) makes cuts from a row-major host sample [nrow][ncol] and max_bins
 * in 2..255.  Per column: (1) the values that are not missing (NaN or == missing) and are finite, sorted ascending,
 * s_0..s_{n-1}, with distinct values u_0 < ... < u_{m-1}; (2) m <= 1: no cuts; (3) m <= max_bins: the cuts are
 * u_1..u_{m-1}; (4) otherwise the candidates s[floor(j * n / max_bins)] for j = 1..max_bins-1, deduplicated, with any
 * equal to u_0 dropped.  (5) It writes cut_ptr (ncol + 1 entries), *needed = the number of cut values, and the values
 * into cut_values; if more than `cap` are needed it refuses (rc -1) with *needed still set.
 * Per new tree t, with pred the float32 margin of the forest so far - initially, bit for bit, what
 * XGBoosterPredict(option_mask = 1) returns:
 *  1. g = pred - y; q = (int64) rint(g * 2^24): both exactly as steps 3-4 of the refit above, with the same refusal for
 *     a gradient that is not finite or has |g| >= 256.  At most 2^31 rows.
 *  2. Nodes are numbered in allocation order: the root is 0; levels d = 0 .. max_depth-1 are processed in turn; within
 *     a level the open nodes are taken in ascending id; a node that splits gets the next two ids, left = n,
 *     right = n + 1.
 *  3. Histograms.  For an open node p, feature f and bin b, Ghist[p][f][b] is the int64 sum of q over the node's rows in
 *     that bin and Hhist[p][f][b] the count of those rows, the missing bin included.  Integer adds only (no float
 *     atomics): the sums depend on neither the order of the rows, the launch shape, the form, nor OHXDMatrixSetGrid.
 *  4. Split choice.  Candidates are (f, j, dl) with j < ncut_f and dl in {0, 1}.
 *     GL = sum_{b<=j} Ghist[b] + (dl ? Ghist[missing] : 0), HL likewise, GR = Gp - GL, HR = Hp - HL, in integers.  A
 *     candidate is valid when HL >= min_child_rows and HR >= min_child_rows (min_child_rows >= 1).  In double, with
 *     Gd = (double)G * 2^-24: gain(G, H) = (Gd * Gd) / ((double)H + (double)lambda) and
 *     loss_chg = (gain(L) + gain(R)) - gain(P); no fused multiply-add.  The best candidate is the largest loss_chg,
 *     compared as doubles; exact ties go to the lexicographically smallest (f, j, dl) - so the default is right whenever
 *     the node holds no missing value of f.  The node splits when a valid candidate exists and best > (double)gamma
 *     (gamma >= 0).
 *  5. Node records.  A split stores feature = f, value = c_j, default_left = dl, loss_chg = (float)best.  Every node
 *     stores sum_hess = (float)Hp and base_weight = w = (float)( -((double)Gp * 2^-24) / ((double)Hp + (double)lambda) ),
 *     the refit's step 5.  A leaf stores value = w * eta (one float32 multiply), loss_chg = 0, feature = 0 and
 *     default_left = 0.  parent holds the file's left-child bit (bit 31; the root is -1); leaf_child_cnt is 0, deleted is
 *     0, and there are no categorical arrays.  A node with Hp < 2 * min_child_rows, or one at max_depth, is a leaf
 *     without evaluation.
 *  6. pred += leaf(row), one float32 add per row.  tree_info gets 0.
 * *nodes_added (may be NULL) receives the total number of nodes over the new trees.
 * All or nothing: the forest is extended only after every round is done and the device's error word has been read back
 * clean.  On success everything built from the forest is dropped as a model load drops it: the flattened device
 * forests, the contributions state, the refit state, and the visit state WITH its counters (the leaf numbering has
 * changed); a graph captured earlier is stale.  XGBoosterSaveModel writes the longer forest in all three formats, and
 * contributions work at once: the new trees carry covers.
 * Refused, with the forest untouched: no model (a loaded model with 0 trees is accepted); categorical splits; several
 * output groups; an objective that is not identity / squared error; NULL labels or cuts; no feature, or more than 128
 * features; rounds < 1; max_depth outside 1..8; eta not finite; lambda or gamma not finite or negative;
 * min_child_rows < 1; cuts that are not finite or not strictly ascending, or more than 254 for a feature; nlabel != the
 * matrix's rows, or no rows; more than 2^31 rows; more columns than features; a stream that is being captured (nothing
 * is enqueued); no usable HIP device (no CPU fallback); a buffer that cannot be allocated (the message says the
 * bytes); and a gradient out of range at any round (the message says "label").
 * Both forms wait once, at the end.  The host form stages the labels; the device form takes d_labels in HBM (nlabel
 * floats, ready on `stream`) and enqueues on `stream`.  The cut arrays are HOST pointers in both forms.  The grow state
 * (bin planes of F * nrow bytes, row positions, the running margin, the level's histograms, the node records, the
 * staged labels and cuts) is the booster's own and never a buffer of another path; dropped when a model is loaded, by
 * an "ohx_device" move and at XGBoosterFree.  Calls on ONE booster must not run concurrently. */
int OHXBoosterBoostTrees(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel,
                         const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                         float lambda, float gamma, bst_ulong min_child_rows, bst_ulong* nodes_added);
int OHXBoosterBoostTreesDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                               const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                               float lambda, float gamma, bst_ulong min_child_rows, bst_ulong* nodes_added, void* stream);
/* Boosting with a held-out set (docs/20_boost_eval.md): the call above, with the RMSE of the training rows and of a
 * second, held-out matrix after every round, and early stopping on the held-out error - without leaving the GPU between
 * rounds.  Tree t (1-based) is exactly the tree OHXBoosterBoostTrees grows at round t from the same arguments: the
 * held-out rows never influence a tree.
 * The metric.  For a set of n rows with running float32 margin pred_t after t new trees (t = 0 is the forest as
 * loaded; the held-out rows' initial margin is, bit for bit, what XGBoosterPredict(option_mask = 1) returns for them,
 * and every new tree adds its leaf with one float32 add, a row stepping left exactly when x < c_j, NaN, the held-out
 * matrix's own `missing` or a column it lacks taking the default): g = pred_t[r] - y[r], one float32 subtraction;
 * q = (int64) rint(g * 2^24), exactly as step 1 above; S_t = sum_r q_r^2 is an exact integer.  |g| < 256 gives
 * |q| <= 2^32 - 256, so q^2 < 2^64 fits a uint64; the device keeps S_t as two uint64 accumulators, one summing the high
 * 32 bits of each q^2 and one the low 32 bits, and with at most 2^31 rows neither can overflow.  Integer adds only: the
 * sums depend on neither the order of the rows, the launch shape, the form, nor OHXDMatrixSetGrid.
 * train_rmse[t] and eval_rmse[t] are written for t = 0 .. *rounds_run (room for rounds + 1 doubles each; either may
 * be NULL; later entries are untouched): sqrt( (double)S_t * 2^-48 / (double)n ), where (double)S_t is the exact
 * integer rounded to nearest even, as an unsigned __int128 conversion rounds it, the scaling is exact, and the division
 * and the square root are IEEE double.
 * The stop rule is decided on the exact integers, never on the doubles.  best starts at 0; after tree t is grown,
 * best = t if S_eval[t] < S_eval[best] - strictly: a tie is not an improvement.  If patience >= 1 and
 * t - best >= patience the call stops and *rounds_run = t; otherwise *rounds_run = rounds.  *best_round = best.
 * What is kept.  patience == 0: all `rounds` trees are appended; the forest, and XGBoosterSaveModel's bytes in all three
 * formats, equal what OHXBoosterBoostTrees leaves.  patience >= 1: trees 1 .. best are appended and the later ones are
 * discarded - a stated departure from xgboost, which keeps them and records best_iteration.  best == 0 is a success
 * that appends nothing: the forest and everything built from it stay as they were.  *nodes_added (may be NULL) counts
 * the kept trees' nodes.
 * The held-out matrix.  eval_dmat == NULL means no held-out set: eval_labels must be NULL, eval_nlabel 0 and patience
 * 0; only train_rmse is written and *best_round = *rounds_run.  Otherwise it is a matrix of either form, possibly the
 * same handle as dmat, with its own `missing`, 1 to 2^31 rows, at most the booster's number of features (the columns it
 * lacks fall in the missing bin), on the training matrix's device; eval_nlabel equals its row count.
 * Refused, with the forest and every output untouched: everything OHXBoosterBoostTrees refuses, in the same order and
 * with the same guarantees; in addition patience < 0; patience >= 1 without a held-out matrix; eval labels without a
 * held-out matrix, or NULL with one; NULL rounds_run or best_round; a held-out handle that is stale; a held-out matrix
 * with no rows, more than 2^31 rows, more columns than features, another device, or eval_nlabel != its rows.  Nothing
 * is enqueued before the last argument check.  The range refusal covers every margin that is summed: a training
 * residual that is not finite or has |g| >= 256 at t = 0 .. rounds_run (the message says "label"; the plain call never
 * looks at the margin after its last tree, this one does), and a held-out one likewise (the message says
 * "eval label"), also in a round whose tree would have been discarded.
 * patience == 0 waits once, at the end: sums, records and the error word come back together.  patience >= 1 waits once
 * a round for that round's held-out sums and the error word (a few tens of bytes), and enqueues nothing more once the
 * rule says stop.  The device form takes d_labels and d_eval_labels in HBM, ready on `stream`.  Not capturable.  The
 * held-out bin planes and margin, the staged eval labels and the sums are part of the grow state.  Everything else is
 * as for OHXBoosterBoostTrees: all or nothing, what a success drops, no concurrent calls on ONE booster. */
int OHXBoosterBoostTreesEval(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel,
                             DMatrixHandle eval_dmat, const float* eval_labels, bst_ulong eval_nlabel,
                             const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                             float lambda, float gamma, bst_ulong min_child_rows, int patience, double* train_rmse,
                             double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added);
int OHXBoosterBoostTreesEvalDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                                   DMatrixHandle eval_dmat, const float* d_eval_labels, bst_ulong eval_nlabel,
                                   const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                                   float lambda, float gamma, bst_ulong min_child_rows, int patience, double* train_rmse,
                                   double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                   void* stream);
/* Boosting with row weights (docs/21_row_weights.md): OHXBoosterBoostTreesEval with a weight per training row and per
 * held-out row - a fit and an error weighted by air mass or cell area, or a fit that ignores some rows (weight 0)
 * without a second matrix.  weights holds nlabel floats and eval_weights eval_nlabel floats; either may be NULL, and
 * NULL means every weight is 1.0f.  Steps that are not restated here are those of OHXBoosterBoostTrees (the cuts, the
 * bins, steps 2 and 6) and of OHXBoosterBoostTreesEval (the margins, the stop rule, what is kept, the held-out matrix).
 * Weights and per-row quantities.  w is finite with 0 <= w < 256.  hq = (uint64) rint(w * 2^24), which is < 2^32: the
 * row's hessian in the gradient's fixed point.  g = pred - y as in step 1; the refusal for g not finite or |g| >= 256
 * looks at g before the weight, so a zero-weight row with a NaN label is still refused with "label".  gw = g * w is one
 * float32 multiply, not fused; |gw| >= 256 is refused, and the message says "label".  q = (int64) rint(gw * 2^24):
 * |q| < 2^32 and at most 2^31 rows keep G inside an int64, exactly as in step 1.
 * Histograms.  Ghist[p][f][b] is the int64 sum of q and Hhist[p][f][b] the uint64 sum of hq over the node's rows in the
 * bin; a sum of hq is < 2^63.  Integer adds only (no float atomics, no compare-and-swap): the sums depend on neither
 * the order of the rows, the launch shape, the form, nor OHXDMatrixSetGrid.
 * Gain, leaf and node records.  Hd = (double)H * 2^-24, the conversion rounded to nearest even and the scaling exact.
 * gain(G, H) = (Gd * Gd) / (Hd + (double)lambda) and loss_chg = (gain(L) + gain(R)) - gain(P) as in step 4;
 * base_weight = (float)( -Gd / (Hd + (double)lambda) ); sum_hess = (float)Hd; the leaf value is base_weight * eta, one
 * float32 multiply.
 * Valid candidates.  A candidate is valid when HL > 0 and HR > 0 as integers (so that lambda = 0 never divides by
 * zero) and HLd >= (double)min_child_weight and HRd >= (double)min_child_weight; min_child_weight is finite and >= 0
 * and takes the place of min_child_rows.  A node with Hd < 2 * min_child_weight (in double), or one at max_depth, is a
 * leaf without evaluation.  The total order of the candidates, the tie rule, the node numbering and the record format
 * are unchanged.
 * The metric.  e = (int64) rint(g * 2^24) is the unweighted residual of OHXBoosterBoostTreesEval (its q).
 * S_t = sum_r hq_r * e_r^2 is an exact integer < 2^127 and W = sum_r hq_r; W does not change between rounds.
 * train_rmse[t] and eval_rmse[t] are sqrt( ((double)S_t * 2^-72) / ((double)W * 2^-24) ): both conversions are from
 * unsigned __int128, rounded to nearest even; the scalings are exact; the division and the square root are IEEE double.
 * On the device, with e^2 = a * 2^32 + b (a, b < 2^32) and m = 0xFFFFFFFF, a set keeps three uint64 accumulators a
 * round: P2 += (hq * a) >> 32; P1 += ((hq * a) & m) + ((hq * b) >> 32); P0 += (hq * b) & m; so that
 * S = P2 * 2^64 + P1 * 2^32 + P0.  hq, a, b < 2^32, so neither product overflows a uint64; a row adds less than 2^32 to
 * P2, to P0 and to W and at most 2^33 - 2 to P1, so at 2^31 rows P2, P0 and W stay below 2^63 and P1 at or below
 * 2^64 - 2^32: none of the accumulators can overflow.  The stop rule compares the exact S_eval[t], strictly, as for
 * OHXBoosterBoostTreesEval.
 * Consequences.  With all weights 1.0f (or NULL) and min_child_weight = (float)min_child_rows, the forest,
 * XGBoosterSaveModel's bytes in all three formats and both RMSE arrays equal those of OHXBoosterBoostTreesEval (hq is
 * 2^24, so Hd is the row count and S / W is sum q^2 / n).  A weight-0 row influences no tree and no sum.  A weight of 2
 * or 4 equals that many copies of the row in every sum of the metric, and in every histogram wherever g * 2^24 is a
 * whole number (|g| >= 0.5, or pred and y on the 2^-24 grid): rint(w * x) = w * rint(x) needs that, and a smaller g with
 * bits below 2^-24 may differ from its copies by one unit of q.
 * Refused, with the forest and every output untouched: everything OHXBoosterBoostTreesEval refuses, in the same order
 * (min_child_weight not finite or negative stands where min_child_rows < 1 stood); eval_weights given without a
 * held-out matrix; a weight that is not finite, is negative or is >= 256 (the message says "weight" for the training
 * set and "eval weight" for the held-out set); a training set whose W is 0, or a held-out set whose W is 0.
 * The objective ("ohx_objective", "ohx_huber_slope" of XGBoosterSetParam).  What is stated above is squarederror.  In
 * general a training row r has, at the start of every round, a pair (q, hq) made as follows; every operation is float32
 * and rounds once, nothing is fused into a multiply-add, the division and the square root are IEEE:
 *   z  = pred - y                      refused ("label") if not finite or |z| >= 256 - before the weight, as above
 *   w  = weight (NULL: 1.0f)           refused ("weight") if not finite, < 0 or >= 256
 *   squarederror:  g = z; h = 1.0f
 *   pseudohuber:   d2 = delta * delta; z2 = z * z; s = sqrtf(1.0f + z2 / d2); g = z / s; c = d2 + z2; h = d2 / (c * s)
 *   gw = g * w   refused ("label") if |gw| >= 256;   hw = h * w
 *   q  = (int64) rint(gw * 2^24);      hq = (uint64) rint(hw * 2^24)     (h <= 1, so hq < 2^32)
 * This restates PseudoHuberRegression::GetGradient of xgboost 1.6.0; parity with libxgboost is not pinned, the text above
 * is the definition.  With delta >= 2^-10 and |z| < 256 nothing overflows (z2 / d2 < 2^36).  The pair does not depend on
 * whether float32 denormals are flushed to zero: 1 + z2 / d2 and d2 + z2 absorb a denormal z2, and a denormal g gives
 * q = 0 either way.  A row that is out of the bag of a sampled call has the pair (0, 0); its label and its weight are
 * checked all the same.  Everything downstream is the text above with this q and hq: the histograms, the candidates and
 * their order, min_child_weight on Hd, sum_hess = (float)Hd, base_weight and the leaf.  The metric is unchanged - the RMSE
 * of the margin against the labels, weighted by rint(w * 2^24), whose W is constant over the rounds - and so are the stop
 * rule, what is kept, all or nothing, the forms and "not capturable".  With pseudohuber a round whose root has H == 0
 * (every in-bag hq rounds to 0: a leaf would divide by lambda alone) is refused, the message says "hessian", and the
 * forest and every output are untouched, as for "bag".  The same holds for OHXBoosterBoostTreesSampled, ...Deep and
 * ...DeepSampled.
 * The quantile objective ("ohx_objective" = quantile, alpha = "ohx_quantile_alpha" as a float32).
 *   alpha_q = (uint32) rint(alpha * 2^24), so 2^14 <= alpha_q <= 2^24 - 2^14; everything below is defined on alpha_q.
 * Pair: z, w and their refusals as above;
 *   quantile:      g = (z >= 0) ? 1.0f - alpha : -alpha; h = 1.0f
 * in float32; gw, hw, q and hq as above, so hq = rint(w * 2^24) and a leaf's H is the weight it holds.  A row out of the
 * bag, or one that raised a flag, has the pair (0, 0) as above.  Structure: the tree is grown from these pairs exactly as
 * above - histograms, candidates, their order, lambda, gamma, min_child_weight, the bag and colsample_bytree.  Leaf: after
 * the last level every leaf node p of the new tree is set as follows.  The rows that count are those with pos == p and
 * hq_i > 0 (in the bag, unflagged and of non-zero weight).  For each, r_i = y_i - pred_i in float32 with pred as at the
 * start of the round (this is -z bit for bit), and k_i = key(bits(r_i)), where key maps a float's bits to an unsigned
 * integer in the order of the floats: -0.0f counts as +0.0f, u = bits; key = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000).
 *   W_p = sum hq_i;   C_p(k) = sum of hq_i over k_i <= k
 *   k*  = the smallest key with alpha_q * W_p <= 2^24 * C_p(k*)      exact integers (unsigned __int128; both sides < 2^88)
 *   q_p = the float whose key is k*;   value = q_p * eta  (one float32 multiply)
 * The leaf is the lower weighted alpha-quantile of the leaf's residuals, with no interpolation; it depends on neither the
 * order of the rows nor the launch shape.  base_weight, sum_hess, G and H of the record stay as the split left them (the
 * Newton values, as xgboost's adaptive leaf leaves them).  A leaf with W_p == 0 keeps its record; only a weightless root
 * of the Weighted call is one.  The held-out walk, the assembled tree, the saved model, pred and both metric arrays carry
 * the quantile leaves.  This is xgboost's adaptive leaf (reg:quantileerror since 2.0) without its interpolation; parity
 * with libxgboost is not pinned, the text above is the definition.  Refused under the quantile objective, before anything
 * is enqueued and with the forest and every output untouched: the calls named with "ohx_objective" above.
 * Regularisation ("ohx_reg_alpha" = alpha, "ohx_max_delta_step" = m of XGBoosterSetParam).  What is stated above is
 * alpha = 0 and m = 0.  In general, with Gd = (double)G * 2^-24, Hd = (double)H * 2^-24, D = Hd + (double)lambda and alpha
 * and m widened to double; every operation is a double operation and rounds once, nothing is fused:
 *   T  = Gd >  alpha ? Gd - alpha : (Gd < -alpha ? Gd + alpha : +0.0)          ThresholdL1 of xgboost 1.6.0 param.h
 *   w  = (-T) / D;   if (m > 0 && fabs(w) > m) w = copysign(m, w)
 *   gain(G, H) = m == 0 ?  (T * T) / D
 *                        : -((2.0 * Gd) * w + (D * w) * w) - (2.0 * alpha) * fabs(w)
 *   base_weight = (float)w;   leaf = base_weight * eta  (one float32 multiply)
 *   loss_chg = (gain(L) + gain(R)) - gain(P)      as above
 * With alpha = 0 and m = 0 these are, bit for bit, the gain and the leaf above, a base_weight of -0.0f at G == 0
 * included.  Where |Gd| <= alpha, T is +0.0 and base_weight is -0.0f.  The second gain form is twice the reduction of the
 * regularised objective at the clipped w; mathematically it is the first form wherever nothing is clipped.  It departs
 * from CalcGain of xgboost 1.6.0 in this: CalcGain also takes the first form whenever max_delta_step == 0, but with a
 * step it returns -(2 G w + D w^2) + alpha |w| on the clipped w, returns 0 below min_child_weight, and works on its own
 * floating-point sums; here the L1 term enters the clipped form as -2 alpha |w|, so that the form is the regularised
 * objective's own reduction and agrees with the first wherever nothing is clipped, min_child_weight stays a rule on
 * which splits are admitted, and everything is double.  Parity with libxgboost is not pinned; the
 * text above is the definition.  Unchanged: the candidates and their total order, the ties, which splits are admitted and
 * which nodes are evaluated, min_child_weight on Hd, sum_hess, the node numbering, the record format and the refusals of
 * a root with H == 0 ("bag", "hessian").  A loss_chg may now be negative where a child is clipped; such a candidate loses
 * to gamma >= 0 as any other.
 * Monotone constraints ("ohx_monotone_constraints": c_f of feature f).  What is stated above is every c_f = 0.  With any
 * c_f != 0 ("active"), and Gd, Hd, D, alpha and m as under Regularisation - every operation is a double operation and
 * rounds once, nothing is fused - every node p carries an interval (lo_p, hi_p) of doubles, the root's (-inf, +inf), and
 *   w(G, H; lo, hi) = the w above (L1 threshold, then the step clip), then clamped:  w < lo ? lo : (w > hi ? hi : w)
 *   gain_w(G, H, w) = -((2.0 * Gd) * w + (D * w) * w) - (2.0 * alpha) * fabs(w)
 * gain_w is the second gain form above at a weight that is given; with active constraints it is used for every node of
 * the tree, whatever m is.  For candidate (f, j, dl) of node p, wL = w(GL, HL; lo_p, hi_p) and wR likewise.  It is
 * admitted when the rule above admits it and c_f == 0, or c_f > 0 && wL <= wR, or c_f < 0 && wL >= wR, and
 *   loss_chg = (gain_w(L, wL) + gain_w(R, wR)) - gain_w(P, w(Gp, Hp; lo_p, hi_p))
 * When p splits on f, mid = (wL + wR) * 0.5; with c_f > 0 the left child gets (lo_p, mid) and the right (mid, hi_p), with
 * c_f < 0 the left gets (mid, hi_p) and the right (lo_p, mid), and with c_f == 0 both inherit (lo_p, hi_p).  wL and wR lie
 * in the children's own intervals, so a child's weight is the same under its parent's interval and under its own.
 *   base_weight = (float) w(G, H; lo, hi) with the node's own interval;   leaf = base_weight * eta  (one float32 multiply)
 * Unchanged: the candidates and their total order (f, j, dl) with the original f under a feature list, and the ties; which
 * splits the rule above admits and which nodes are evaluated, min_child_weight on Hd, and sum_hess; the node numbering,
 * the record format and the refusals of a root with H == 0; the bag, the metrics, the stop rule, all or nothing, both forms
 * and "not capturable".  A negative loss_chg loses to gamma >= 0 as above.  The consequence: for eta > 0 a new tree is
 * non-decreasing (c_f = 1) or non-increasing (c_f = -1) in x_f over non-missing values, with every other feature fixed;
 * a row whose x_f is missing goes where default_left sends it and is outside the claim.  Parity with libxgboost is not
 * pinned; the text above is the definition.  The same holds for OHXBoosterBoostTreesSampled, ...Deep and ...DeepSampled.
 * Interaction constraints ("ohx_interaction_constraints": a list of groups of feature ids).  What is stated above is no
 * group.  The constraints are active unless the list is empty or some group holds every feature 0 .. F - 1, F the
 * booster's num_feature.  While they are active every node carries two 128-bit sets of the booster's feature ids:
 *   P(root) = {}            A(root) = every feature 0 .. F - 1
 *   p splits on f, children c:   P(c) = P(p) + {f}
 *                                A(c) = P(c) + the union of every group g with P(c) a subset of g
 *   candidates of node p:  the (f, j, dl) the call has without the constraints, with f additionally in A(p)
 * Under a tree's feature list the candidates are the list's intersection with A(p).  Everything else is unchanged: the
 * bag and the integer histograms; the total order (f, j, dl) with the original f, and the ties; which splits are
 * admitted, which nodes are evaluated, and min_child_weight; the gain form of whichever of the objective, the
 * regularisation and the monotone constraints is active; the node's sums, sum_hess and base_weight; the node numbering
 * and the records; the refusals of a root with H == 0; the metrics, the stop rule and all or nothing; both forms, and
 * "not capturable".  A node with no candidate in A(p) is a leaf.  A feature in no group, once split on, admits only the
 * path's own features below it.  Parity with libxgboost is not pinned; the text above is the definition.
 *   C1.  With inactive constraints the forest, XGBoosterSaveModel's bytes in all three formats and both metric arrays
 *     equal those of the same call with the parameter never set, and nothing of the kernels of interaction constraints is
 *     launched, set or loaded.
 *   C2.  In every new tree, every split node p has its feature in A(p), with A derived from the features on p's path by
 *     the text above.  In particular the features on any root-to-leaf path lie together in one group, or are a single
 *     feature.
 *   C3.  With every feature in a group of its own, every tree splits on one feature only.
 *   C4.  The result depends on neither the row order, the launch shape, the batch size of the deep levels, the form nor
 *     the stream.
 * They compose with squared error and pseudo-Huber, ohx_reg_alpha, ohx_max_delta_step, ohx_monotone_constraints, all
 * metrics, weights, a held-out set and patience, and with any subsample and colsample_bytree.  Refused while active, at
 * the top and with nothing enqueued: ohx_colsample_bylevel or ohx_colsample_bynode taking a feature away,
 * ohx_objective=quantile, and the two calls that keep row counts.  The sets of the tree at hand, 32 bytes a node of the
 * call's node stride, and the groups are part of the grow state; where they cannot be allocated the call returns -1 and
 * the message names the bytes.  The same holds for OHXBoosterBoostTreesSampled, ...Deep and ...DeepSampled.
 * The metric ("ohx_eval_metric").  What is stated above is rmse.  For one row z = pred - y in float32 (refused as above if
 * not finite or |z| >= 256), hq = rint(w * 2^24), delta = "ohx_huber_slope" whatever the objective, and
 *   rmse         sq = e * e,  e = (int64) rint(z * 2^24)
 *   mae          sq = |e|
 *   pseudohuber  d2 = delta * delta; z2 = z * z; s = sqrtf(1.0f + z2 / d2); mf = z2 / (1.0f + s);   float32, IEEE, not fused
 *                sq = (uint64) rint(mf * 2^24)
 *   quantile     sq = |e| * (z < 0 ? alpha_q : 2^24 - alpha_q),  alpha_q of "ohx_quantile_alpha" as above;  sq < 2^56
 * mf is delta^2 (s - 1) written without a cancellation at small z; mf <= delta |z| < 2^16, so sq < 2^40, and a denormal z2
 * or mf gives sq = 0 whether or not denormals are flushed.  S = sum hq * sq is exact and W is as above.  train_rmse[t] and
 * eval_rmse[t] - the arrays keep their names - then hold, for mae and pseudohuber, ((double)S_t * 2^-48) / ((double)W *
 * 2^-24), both conversions from unsigned __int128 and no square root: the weighted mean absolute error, and the weighted
 * mean of delta^2 (sqrt(1 + z^2 / delta^2) - 1).  For quantile they hold ((double)S_t * 2^-72) / ((double)W * 2^-24), the
 * weighted mean pinball loss at alpha, likewise without a square root.  The stop rule compares the exact S_eval[t] of the metric, strictly, as
 * above.  The same holds for OHXBoosterBoostTreesSampled, ...Deep and ...DeepSampled.
 * Everything else is OHXBoosterBoostTreesEval's: all or nothing; what a success drops; patience == 0 waits once, at the
 * end, and patience >= 1 waits once a round; eval_dmat == NULL works as there, and eval_weights must then be NULL.  Not
 * capturable.  The host form stages the weights with the labels; the device form takes d_weights and d_eval_weights in
 * HBM (or NULL), ready on `stream`.  The staged weights and the wider sums are part of the grow state.  Calls on ONE
 * booster must not run concurrently. */
int OHXBoosterBoostTreesWeighted(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                 bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                 const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                 const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                 float min_child_weight, int patience, double* train_rmse, double* eval_rmse,
                                 int* rounds_run, int* best_round, bst_ulong* nodes_added);
int OHXBoosterBoostTreesWeightedDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                       const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                       const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                       const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                       float eta, float lambda, float gamma, float min_child_weight, int patience,
                                       double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                       bst_ulong* nodes_added, void* stream);
/* Boosting with row and column subsampling (docs/22_sampling.md): OHXBoosterBoostTreesWeighted with three more
 * arguments before patience - subsample, the fraction of the rows a tree is fitted to; colsample_bytree, the fraction of
 * the features it may split on; and the seed of the draws.  Every tree of a call draws a fresh bag of rows and a fresh
 * set of features, on the GPU, inside the one call.  Everything not restated here is OHXBoosterBoostTreesWeighted's:
 * weights (NULL means 1.0f), min_child_weight, the metric, the stop rule, what is kept, all or nothing, what a success
 * drops, the two forms, not capturable.
 * The mix function.  All arithmetic is uint64 and wraps:
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * Tree keys.  gamma64 = 0x9E3779B97F4A7C15.  Tree t = 1..rounds of the call has index i = T0 + t - 1, where T0 is the
 * number of trees the forest holds when the call starts.  K_row(i) = mix(seed + gamma64 * (2i + 1)) and
 * K_col(i) = mix(seed + gamma64 * (2i + 2)).
 * Rows.  k_s = (uint32) rint((double)subsample * 2^24).  Row r is the 0-based row of the training matrix; it is in the
 * bag of tree i exactly when (mix(K_row(i) + r) >> 40) < k_s.  k_s == 2^24 (subsample 1.0f) puts every row in and
 * draws nothing.
 * Columns.  F is the booster's num_feature and n_sel = max(1, (int) floor((double)colsample_bytree * F)).  Feature f
 * has key c_f = mix(K_col(i) + f); the selected set is the n_sel features smallest by (c_f, f), kept in ascending f.
 * n_sel == F selects all and draws nothing.
 * The tree.  Tree t is the tree OHXBoosterBoostTreesWeighted grows at that round from the same running margin with two
 * changes: every out-of-bag row has weight 0, and every unselected feature has an empty cut list.  So out-of-bag rows
 * add nothing to any histogram; node sums, sum_hess, base_weight and min_child_weight are over the bag; the candidates,
 * their total order (f, j, dl) with the original f, ties, node numbering and records are unchanged.
 * Everything else sees every row at its full weight: pred += leaf(row) for every row, in or out of the bag;
 * train_rmse, eval_rmse, W, the stop rule and the range and weight refusals cover all rows, and a NaN label on an
 * out-of-bag row is still refused with "label".
 * The result depends on the order of the rows only through r in the draw.  Launch shape, form, stream and
 * OHXDMatrixSetGrid change nothing.  Integer adds only.
 * Consequence.  With subsample = colsample_bytree = 1.0f and any seed, the forest, XGBoosterSaveModel's bytes in all
 * three formats and both RMSE arrays equal those of OHXBoosterBoostTreesWeighted.
 * Column sampling by level and by node ("ohx_colsample_bylevel", "ohx_colsample_bynode"; docs/29_colsample_level_node.md).
 * What is stated above is both at 1.  The nesting tree -> level -> node and the max(1, floor(...)) at each stage are
 * ColumnSampler's of xgboost 1.6.0; the draws are this library's own.  mix, gamma64, K_col(i) and i = T0 + t - 1 are those
 * above, and S_tree is the tree's n_sel selected features, drawn exactly as above.
 *   Level.  d is the depth of the nodes being split, the root's being 0.
 *     n_lvl = max(1, (int) floor((double)colsample_bylevel * n_sel)).  K_lvl(i, d) = mix(K_col(i) + gamma64 * (d + 1)).
 *     Feature f of S_tree has key mix(K_lvl(i, d) + f); S_lvl(d) is the n_lvl features of S_tree smallest by (key, f), kept
 *     in ascending f.  n_lvl == n_sel draws nothing: S_lvl(d) = S_tree.
 *   Node.  p is the node's id in the tree in allocation order, the root being 0.
 *     n_node = max(1, (int) floor((double)colsample_bynode * n_lvl)).  K_node(i, p) = mix(K_col(i) + gamma64 * (32 + p)).
 *     Feature f of S_lvl(d) has key mix(K_node(i, p) + f); S_node(p) is the n_node features of S_lvl(d) smallest by
 *     (key, f).  n_node == n_lvl draws nothing: S_node(p) = S_lvl(d).  d + 1 <= 18 < 32, so level keys and node keys
 *     never share an input.
 *   The tree.  The candidates of node p are the (f, j, dl) with f in S_node(p).  Everything else is as stated above, word
 *     for word: the bag; the integer histograms; the total order (f, j, dl) with the original f, and the ties; which
 *     splits are admitted and which nodes are evaluated; the node's sums, sum_hess and base_weight; the gain form of
 *     whichever of the objective, the regularisation and the monotone constraints is active; the node numbering and the
 *     records; the refusal of a root with H == 0; the margins and the metrics over every row; the stop rule, all or
 *     nothing, both forms, not capturable.
 *   The result depends on the seed, the tree index, the level, the node id and the feature; not on the launch shape, the
 *   batch size of the deep levels, the form, the stream or OHXDMatrixSetGrid.  The two fractions compose with both
 *   objectives, ohx_reg_alpha, ohx_max_delta_step, ohx_monotone_constraints, all three metrics, weights, a held-out set
 *   and patience, and with any subsample and colsample_bytree, 1.0 included.
 *   C1.  With n_lvl == n_sel and n_node == n_lvl the call takes the path it takes without the two parameters, whatever
 *     their values or the seed - in particular with both at 1: the forest, XGBoosterSaveModel's bytes in all three
 *     formats and both metric arrays equal those of the same call at the defaults, and nothing of the kernels of column
 *     sampling by level and node is launched, set or loaded.
 *   C2.  Every split node p of a new tree has its feature in S_node(p); all split nodes of one level have their features
 *     in that level's S_lvl(d).  With n_lvl == 1 every split of a level is on the same feature.
 *   C3.  OHXBoosterBoostTreesDeepSampled at max_depth <= 8 equals OHXBoosterBoostTreesSampled with the same parameters,
 *     in bytes and arrays.
 *   The level lists of every round, rounds x max_depth x n_lvl bytes, are part of the grow state, made before anything
 *   is enqueued; where they cannot be allocated the call returns -1 and the message names the bytes.
 * Refused, with the forest and every output untouched: everything OHXBoosterBoostTreesWeighted refuses, in the same
 * order; after min_child_weight and before the cuts, subsample not finite, <= 0, > 1, or with k_s == 0, then
 * colsample_bytree not finite, <= 0, or > 1; and, on the device, a round whose bag holds no weight (root H == 0), also
 * a round whose tree would have been discarded (the message says "bag").  The bag's bit plane and the selected features
 * of every round are part of the grow state.  Calls on ONE booster must not run concurrently. */
int OHXBoosterBoostTreesSampled(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                float min_child_weight, float subsample, float colsample_bytree, uint64_t seed, int patience,
                                double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                bst_ulong* nodes_added);
int OHXBoosterBoostTreesSampledDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                      const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                      const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                      const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                      float eta, float lambda, float gamma, float min_child_weight, float subsample,
                                      float colsample_bytree, uint64_t seed, int patience, double* train_rmse,
                                      double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                      void* stream);
/* Trees deeper than eight levels (docs/23_deep_trees.md): OHXBoosterBoostTreesWeighted with max_depth in 1..18.  The
 * argument lists are those of the Weighted call and of its Device form.  Everything is OHXBoosterBoostTreesWeighted's,
 * word for word: the cuts and the bins; hq, q, the integer histograms, the candidates, their total order and the ties;
 * node numbering in allocation order, level by level, in ascending id, and the records; min_child_weight, the metric,
 * the stop rule, what is kept, all or nothing, what a success drops, the two forms, not capturable.  One thing changes:
 * max_depth is in 1..18.  Eighteen is the depth the walk kernels, the path tables and the file formats are exercised
 * at; nothing deeper has run.
 * The size of a tree.  A split needs HL > 0 and HR > 0, so every leaf holds a row: a tree has at most
 * min(2^(max_depth + 1) - 1, 2 * nrow - 1) nodes.  The node table of the call holds min(2^(max_depth + 1), 2 * nrow)
 * records a round; the histograms of the levels from 8 on are kept in HBM for a batch of node slots at a time, so the
 * scratch does not grow with the depth.  The sums are integers: which kernel makes them, and in how many batches,
 * cannot change a bit.
 * Consequences.  With max_depth <= 8 the forest, XGBoosterSaveModel's bytes in all three formats and both RMSE arrays
 * equal those of OHXBoosterBoostTreesWeighted (the call takes that path as it is).  With unit weights and
 * min_child_weight = (float)min_child_rows they equal those of OHXBoosterBoostTreesEval, at any max_depth both accept.
 * Waiting.  With max_depth <= 8 the call waits as the Weighted call does.  With max_depth > 8 it also waits, in every
 * tree, once per level from level 7 on for the 16-byte level word (the ids of the open nodes): the host enqueues exactly
 * the batches the next level needs and ends the tree at the first level without an open node, so a request for depth 18
 * on rows that stop splitting at level 12 enqueues no empty level.  Levels below 7 read nothing back.  The device form
 * therefore waits for `stream` inside the call.
 * Row and column subsampling are not offered at these depths: there is no Deep form of the Sampled call.
 * (OHXBoosterBoostTreesDeepSampled, below, has since become that form; this call still takes neither fraction.)
 * Refused, with the forest and every output untouched: everything OHXBoosterBoostTreesWeighted refuses, in the same
 * order, the max_depth message reading "max_depth must be in 1..18"; a node table or a scratch buffer that cannot be
 * allocated is refused with its bytes.  The uint32 row positions and the held-out walk's node table are part of the
 * grow state.  Calls on ONE booster must not run concurrently. */
int OHXBoosterBoostTreesDeep(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                             bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels, const float* eval_weights,
                             bst_ulong eval_nlabel, const bst_ulong* cut_ptr, const float* cut_values, int rounds,
                             int max_depth, float eta, float lambda, float gamma, float min_child_weight, int patience,
                             double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                             bst_ulong* nodes_added);
int OHXBoosterBoostTreesDeepDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, const float* d_weights,
                                   bst_ulong nlabel, DMatrixHandle eval_dmat, const float* d_eval_labels,
                                   const float* d_eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                   const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                   float min_child_weight, int patience, double* train_rmse, double* eval_rmse,
                                   int* rounds_run, int* best_round, bst_ulong* nodes_added, void* stream);
/* Row and column subsampling for trees deeper than eight levels (docs/24_deep_sampled.md): OHXBoosterBoostTreesSampled
 * with max_depth in 1..18.  The argument lists are those of the Sampled call and of its Device form, argument for
 * argument.  The call is OHXBoosterBoostTreesSampled, word for word: the mix function, the tree keys with T0, the bag,
 * n_sel and the selection by (c_f, f); the tree is the Weighted call's where every out-of-bag row has weight 0 and every
 * unselected feature has an empty cut list; everything else sees every row at its full weight - pred += leaf(row) for
 * every row, train_rmse, eval_rmse, W, the stop rule, the range and weight refusals, a NaN label on an out-of-bag row
 * refused with "label", and the round whose bag holds no weight refused with "bag".  One thing changes: max_depth is in
 * 1..18.
 * The size of a tree and the waiting are OHXBoosterBoostTreesDeep's: at most min(2^(max_depth + 1) - 1, 2 * nrow - 1)
 * nodes, a node table of min(2^(max_depth + 1), 2 * nrow) records a round, and with max_depth > 8 one wait per level
 * from level 7 on for the 16-byte level word, in every tree; the host enqueues no empty level.  From level 8 on a row
 * outside the bag makes no add and an unselected feature none for any row: the histograms of a batch of node slots are
 * compact, n_sel columns a slot, and the scratch is min(batch, open nodes) * n_sel * 256 * 16 bytes.
 * Integer adds only.  The result depends on the order of the rows only through r in the draw.  Launch shape, batch
 * size, form, stream and OHXDMatrixSetGrid change nothing.
 * Consequences.  With max_depth <= 8 the forest, XGBoosterSaveModel's bytes in all three formats and both RMSE arrays
 * equal those of OHXBoosterBoostTreesSampled (the call takes that path as it is).  With subsample = colsample_bytree =
 * 1.0f and any seed they equal those of OHXBoosterBoostTreesDeep, at any max_depth (nothing is drawn, allocated or
 * enqueued for the sampling).
 * Refused, with the forest and every output untouched: everything OHXBoosterBoostTreesSampled refuses, in the same
 * order - the fractions after min_child_weight and before the cuts - the max_depth message reading "max_depth must be
 * in 1..18"; every buffer that cannot be allocated is refused with its bytes.  Not capturable.  The bag's bit plane, the
 * selected features of every round, the uint32 row positions and the held-out walk's node table are part of the grow
 * state.  Calls on ONE booster must not run concurrently. */
int OHXBoosterBoostTreesDeepSampled(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                    bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                    const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                    const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                    float min_child_weight, float subsample, float colsample_bytree, uint64_t seed,
                                    int patience, double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                    bst_ulong* nodes_added);
int OHXBoosterBoostTreesDeepSampledDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                          const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                          const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                          const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                          float eta, float lambda, float gamma, float min_child_weight, float subsample,
                                          float colsample_bytree, uint64_t seed, int patience, double* train_rmse,
                                          double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                          void* stream);
int OHXQuantileCuts(const float* data, bst_ulong nrow, bst_ulong ncol, float missing, int max_bins, bst_ulong* cut_ptr,
                    float* cut_values, bst_ulong cap, bst_ulong* needed);
/* OHXDMatrixQuantileCuts (docs/19_device_cuts.md) makes the same cuts from a DMatrix's rows where they lie, in HBM: no
 * booster, either matrix form (XGDMatrixCreateFromMat or OHXDMatrixCreateFromDevice).  The result is what
 * OHXQuantileCuts returns for the row-major sample made of rows 0, row_step, 2 * row_step, ... (< nrow) of the matrix,
 * the matrix's own `missing`, and the same max_bins and cap: steps (1)-(5) above apply word for word, including the
 * `cap` refusal with *needed still set.  One stated difference: a cut equal to zero is always +0.0f (the host form's
 * sort leaves the sign of a zero unspecified; x < -0.0f and x < +0.0f are the same predicate, so no bin changes).
 * No sort is made: an exact radix select over an order-preserving integer key finds every distinct value or order
 * statistic from integer histograms in three passes over the sampled rows.  Integer adds only (no float atomics, no
 * compare-and-swap loops): the result depends on neither the order of the sampled rows, the launch shape,
 * OHXDMatrixSetGrid, nor the matrix form.
 * cut_ptr (ncol + 1 entries, ncol the MATRIX's columns), cut_values and needed are HOST pointers.  A matrix of fewer
 * columns than the booster has features yields ncol + 1 pointers; the caller repeats the last one for the columns the
 * matrix lacks.  nrow == 0 succeeds with every pointer 0 and launches nothing.
 * `stream` is the stream the rows are ready on: the call enqueues there and waits once, at the end.  It is not
 * capturable.  Its scratch (ncol x 4096 and ncol x 255 x 1024 counters of 4 bytes, and a record per column) is the
 * call's own: allocated on the matrix's device, freed before it returns, never a booster's buffer.
 * Refused (rc -1, nothing enqueued, outputs other than *needed untouched): an invalid handle; NULL cut_ptr or needed;
 * NULL cut_values with cap != 0; max_bins outside 2..255; row_step < 1; more than 2^31 rows; a stream that is being
 * captured; no usable HIP device (no CPU fallback); a buffer that cannot be allocated (the message says the bytes). */
int OHXDMatrixQuantileCuts(DMatrixHandle dmat, bst_ulong row_step, int max_bins, bst_ulong* cut_ptr, float* cut_values,
                           bst_ulong cap, bst_ulong* needed, void* stream);

/* The whole of predict_OH_with_XGB's RUN section in one kernel
 * (OH_GridCompMod.F90:303-383): gathers the 27 MAPL fields in place (field f is
 * (im,jm,km) Fortran order, or (im,jm) when is2d[f] != 0; feature order of
 * :313-339), divides field `pl_feature` by 100 (Pa -> hPa, :314; pass -1 for
 * none), predicts rows m = i + im*(j + jm*(k-k1)) for k = k1..k2 (1-based,
 * inclusive, the slab of :300-301), and stores
 *   oh_ml(i,j,k) = 10**pred * ohscale      (:369 and :1569)
 * leaving the other levels of oh_ml untouched.  apply_pow10 = 0 stores the raw
 * margin times ohscale instead.  margin (optional, may be NULL) receives the raw
 * xx_pred(m).  Host-pointer form: stages through HBM and returns when oh_ml is
 * complete.  Device form: all pointers are device pointers, work is enqueued. */
int OHXBoosterPredictFields(BoosterHandle handle, const float* const fields[], const int32_t is2d[], int nfield,
                            int pl_feature, int im, int jm, int km, int k1, int k2, float missing, int apply_pow10,
                            float ohscale, float* oh_ml, float* margin);
int OHXBoosterPredictFieldsDevice(BoosterHandle handle, const float* const d_fields[], const int32_t is2d[],
                                  int nfield, int pl_feature, int im, int jm, int km, int k1, int k2, float missing,
                                  int apply_pow10, float ohscale, float* d_oh_ml, float* d_margin, void* stream);

/* ------------------------------------------------------------------------
 * Part 3 — the steps either side of the predict call (additive)
 * ------------------------------------------------------------------------
 * OHXBoosterRun1 does the arithmetic of OH Run1 from the imports to the INTERNAL
 * field OH (OH_GridComp/OH_GridCompMod.F90:1240-1257, 1444-1478, 1488, 1557-1595)
 * in HBM, so the engineered features never round-trip to the host:
 *   PL_MOD = (PLE_MOD(k-1)+PLE_MOD(k))*0.5, TV_MOD, NDWET_MOD            (:1247-1257)
 *   stratO3 = GMITO3 - GMITTO3                                           (:1446)
 *   gridBoxThickness = ZLE(k-1)-ZLE(k); aod = thickness * (BC+OC+BR+DU+SU+SS+NI)   (:1451-1458)
 *   tauclwDN/taucliDN/aodDN(k) = SUM(x(k:km)), taucliUP/tauclwUP/aodUP(k) = SUM(x(1:k)),
 *       each sum accumulated from zero in ascending level order          (:1468-1478)
 *   PL_BST = (PLE_BST(k-1)+PLE_BST(k))*0.5                               (:1488)
 *   the k-slab, predict_OH_with_XGB, OH_ML *= OHscale                    (:1559-1569)
 *   OH = PL_MOD > TROPP ? OH_ML : default_OH ; OH = (OH*NDWET_MOD)*1.0e-6   (:1579-1595)
 * What stays with the caller: the choice of import per OH_data_source.  LAT in degrees and the
 * local-noon SZA are 2-D inputs of the struct; OHXSolarGeometry below computes them the reference's
 * way for a caller who wants that on the GPU too.
 * All arrays are Fortran order: 3-D (im,jm,km), edge fields (im,jm,0:km), 2-D
 * (im,jm).  MAPL's constants are passed in, not restated.  Host form stages
 * through HBM and returns when the outputs are complete; device form takes device
 * pointers and enqueues (it waits once, for the slab count, which runs on the
 * library's second stream beside the feature kernels).
 * Host form: the arrays cross PCIe in the order the tick needs them - PLE and TROPP of
 * the model (the slab count), the feature engineering's inputs, then what only the walk
 * reads (of the sixteen 3-D fields among those, the slab's levels only), last and under
 * the walk what the mask and the unit conversion read.  The same array may be passed
 * for several members (ONLINE_INST: T is t_mod and t_bst): it crosses once.  With
 * "ohx_register_host" every list is one launch of a small copy kernel.
 * Streams: the library owns two per device for the life of the process - one for kernels, one
 * for copies - and nothing of it runs on the null stream; every stream a process has used
 * is a hardware queue, and a GPU that several ranks share time-slices queues once they
 * outnumber its slots.  Experiment knobs in the environment, read
 * once: OHX_RUN1_STREAMS=1 (copies on the kernels' stream), OHX_RUN1_GATE=1 (a kernel
 * is launched when this thread has seen its inputs arrive, not enqueued behind a wait for
 * them), OHX_RUN1_SLAB_IN_PLACE=1 (the slab count reads the caller's registered PLE and
 * TROPP over PCIe); both measured worth nothing, both off. */
typedef struct OHXRun1Args {
  int32_t im, jm, km;
  int32_t dynamic_k_range;           /* .NOT. compute_once_per_day (:1561) */
  float tropp_min;                   /* Pa, 4000.0 (:1563) */
  float ohscale;                     /* :1569 */
  float missing;                     /* -999.0 (:213) */
  float avogad, runiv, epsilon;      /* MAPL_AVOGAD, MAPL_RUNIV, MAPL_EPSILON */
  /* the model's own state: slab, tropopause mask, number density */
  const float *ple_mod, *t_mod, *q_mod, *tropp_mod;
  /* inputs to the engineered features */
  const float *ple_bst, *zle_bst, *tauclw, *taucli;
  const float *scacoef[7];           /* BC OC BR DU SU SS NI at the chosen wavelength */
  const float *gmito3, *gmitto3;
  /* features used as they are (order of :313-339 where not engineered) */
  const float *lat_deg, *t_bst, *no2, *o3, *ch4, *co, *isop, *acet, *c2h6, *c3h8, *prpe, *alk4, *mp, *h2o2;
  const float *cloud, *qv, *albuv, *ch2o, *sza;
  const float *default_oh;           /* import oh_OH, mol/mol (:1548) */
  /* outputs */
  float *oh;                         /* INTERNAL OH, molec/cm3 */
  float *oh_boost;                   /* export OH_boost = OH_ML*OHscale (may be NULL) */
  float *ndwet;                      /* DIAG_NDWET (may be NULL) */
  int32_t *k1, *k2;                  /* HOST pointers, 1-based slab (may be NULL) */
  /* optional dumps of the engineered features - the reference's DIAG_* exports, its only in-model
   * debugging hook (:1607-1640, OH_StateSpecs.rc:41-73); each may be NULL.  (im,jm,km), strato3 (im,jm):
   * PL_BST (Pa), tauclwDN, taucliDN, taucliUP, tauclwUP, aodUP, aodDN, the layer aod, stratO3 */
  float *diag_pl_bst, *diag_tauclwdn, *diag_tauclidn, *diag_taucliup, *diag_tauclwup;
  float *diag_aodup, *diag_aoddn, *diag_aod, *diag_strato3;
} OHXRun1Args;

/* Levels: 1 <= km <= 640 (the column sums hold one column of km levels per lane in a CU's 160 KiB of LDS); more is
 * refused before anything is staged or enqueued, with an error that names the limit.  GEOS's L72, L91, L132, L137
 * and L181 are all within it. */
int OHXBoosterRun1(BoosterHandle handle, const OHXRun1Args* args);
int OHXBoosterRun1Device(BoosterHandle handle, const OHXRun1Args* args, void* stream);

/* The tail of OH Run1 alone, for a tick that does not call Boost (compute_once_per_day and nhms > 0,
 * OH_GridCompMod.F90:1189-1193): with oh_ml = the OH_ML*OHscale kept from the last Boost,
 *   PL_MOD, TV_MOD, NDWET_MOD as above (:1247-1257);
 *   OH = PL_MOD > TROPP ? oh_ml : default_OH ; OH = (OH*NDWET_MOD)*1.0e-6      (:1579-1595)
 * ndwet may be NULL.  Host form stages through HBM; device form takes device pointers and enqueues. */
int OHXOHPostProcess(int im, int jm, int km, float avogad, float runiv, float epsilon, const float* ple_mod,
                     const float* t_mod, const float* q_mod, const float* tropp_mod, const float* default_oh,
                     const float* oh_ml, float* oh, float* ndwet);
int OHXOHPostProcessDevice(int im, int jm, int km, float avogad, float runiv, float epsilon, const float* d_ple_mod,
                           const float* d_t_mod, const float* d_q_mod, const float* d_tropp_mod,
                           const float* d_default_oh, const float* d_oh_ml, float* d_oh, float* d_ndwet, void* stream);

/* The solar geometry of OH Run1.  OHXJulianDay: JulianDay(nymd) with the reference's leap_year
 * (OH_GridCompMod.F90:1905-1970; host integer arithmetic).  OHXSolarGeometry: latarr =
 * LATS*MAPL_RADIANS_TO_DEGREES (:1444) and sza_noon = computeSolarZenithAngle_LocalNoon(jday, LATS,
 * LONS) (:401-466, 1481-1482) for (im,jm) arrays in radians; either output may be NULL.  float32 in
 * the reference's order of evaluation; sin/asin/cos/acos are the device library's, so the result
 * agrees with a host run to a few ulp of cos(zenith) - which acos turns into up to ~0.05 degree
 * where the sun is overhead.  SZA feeds tree splits: a caller that needs OH bit-identical to a CPU
 * run passes its own sza to OHXBoosterRun1 instead. */
int OHXJulianDay(int nymd, int* jday);
int OHXSolarGeometry(int jday, const float* lats, const float* lons, int im, int jm, float degrees_to_radians,
                     float radians_to_degrees, float* lat_deg, float* sza_noon);
int OHXSolarGeometryDevice(int jday, const float* d_lats, const float* d_lons, int im, int jm, float degrees_to_radians,
                           float radians_to_degrees, float* d_lat_deg, float* d_sza_noon, void* stream);

/* Model facts for roofline accounting: info[0] trees, [1] nodes in the model,
 * [2] node slots in HBM, [3] bytes of the node array the selected kernel reads,
 * [4] max depth, [5] features, [6] node format in use (0 wide, 1 packed, 2 super-nodes, 3 the 16-byte nodes of a
 * booster with categorical splits: then [3] counts the nodes and the words of the sets kept beside them),
 * [7] vector-memory instructions one wavefront issues to walk the whole forest once (super-nodes). */
int OHXBoosterGetInfo(BoosterHandle handle, bst_ulong info[8]);
/* Output groups of the loaded model: xgboost 1.6.0's num_output_group, max(num_class, num_target, 1).  1 for the OH
 * booster; G >= 2 changes the shapes XGBoosterPredict, OHXBoosterPredictContribs and OHXBoosterPredictInteractions
 * return (their comments).  -1 when the booster holds no model. */
int OHXBoosterGetNumGroups(BoosterHandle handle, bst_ulong* out);
/* Nodes of the loaded model with a categorical split (split_type 1) over all trees.  0 for every booster without
 * one: such a booster is flattened, launched and predicted exactly as before.  -1 when the booster holds no model. */
int OHXBoosterGetNumCategoricalSplits(BoosterHandle handle, bst_ulong* out);
/* Name of the GPU kernel XGBoosterPredict / OHXBoosterPredictDevice launch for rows of `ncol` columns with the
 * booster's current parameters, as a profiler prints it (without namespaces and arguments), e.g.
 * "predict_rows_tile_kernel<2,2,true,true>".  *out stays valid until the next call on this handle. */
int OHXBoosterKernelSymbol(BoosterHandle handle, bst_ulong ncol, const char** out);
/* Every GPU kernel a margin predict on THIS matrix launches with the booster's current parameters, in launch order,
 * joined by " + " - the size of the batch decides (a small one has its trees split over waves and a second launch that
 * sums the leaves in tree order; a big one of the OH booster goes through the ring kernel and the launches behind it).
 * Decided by the code that launches (kernels.hip plan_rows).  Not listed: the clustering pass in front of rows that
 * are in no known order, the level-size search of a matrix nobody described.  *out as above. */
int OHXBoosterKernelSymbolRows(BoosterHandle handle, DMatrixHandle dmat, const char** out);
/* How often a block of the ring kernels (the default for the OH booster's big batches) gave up waiting for another
 * since the booster's forest went to the GPU.  Never seen in 6 700 whole-batch calls (tools/ring_soak.py), and not an
 * error: every ring launch train is followed, on the same stream, by a launch of the tile kernel that only runs when a
 * block gave up and then predicts the train's rows again - same bits, the host is not involved, so the device forms
 * (OHXBoosterPredictDevice, ...FieldsDevice, Run1Device) are covered without OHXBoosterCheck.  The first sighting is
 * said on stderr by the next call that reads the flags back.  Waits for `stream`.  (The reference asserts rc == 0 on
 * XGBoosterPredict, OH_GridComp/OH_GridCompMod.F90:356-358: a time-out must not end a model run.) */
int OHXBoosterRingReruns(BoosterHandle handle, void* stream, bst_ulong* out);
/* What "ohx_copy_engine" = auto (when asked for) has decided for OHXBoosterRun1's host form on this booster: *choice = -1 while it is
 * still trying (or when auto is not in charge: the engine was set, or the arrays are not registered), 0 = copy kernels,
 * 1 = DMA; *trials = how many trials have ended, *picked_dma = how many of them picked DMA.  Any of the three may be NULL. */
int OHXBoosterCopyEngineChoice(BoosterHandle handle, int* choice, unsigned* trials, unsigned* picked_dma);

/* ------------------------------------------------------------------------
 * Part 4 — reassembling the OH field across the GPUs of a node (additive)
 * ------------------------------------------------------------------------
 * Inside GEOS nothing is exchanged: every rank keeps the block it predicted
 * (OH_GridCompMod.F90:1199-1202, 1565).  For a caller that wants the whole field on every GPU
 * (BASELINE.json configs #4/#5) the gridcell rows are cut into contiguous shards, rank r of N holding
 * OHXShardRows' rows, and ONE collective - an RCCL all-gather over xGMI - puts every shard at its rows of
 * d_full on every rank.  Set-up as RCCL's own: rank 0 calls OHXCommGetUniqueId, the host distributes the
 * OHX_UNIQUE_ID_BYTES bytes by whatever it has (MPI_Bcast in a GEOS-like host), every rank - its HIP device
 * already current - calls OHXCommInitRank.  OHXAllGatherOH only enqueues on `stream`; d_shard may be
 * d_full + row0 (in place).  Equal shards are one ncclAllGather; ragged ones - and equal ones when the
 * environment said OHX_ALLGATHER=pairs at OHXCommInitRank (read once, there; every rank must be started with the
 * same setting) - the direct exchange of SURVEY.md §8e: one group of ncclSend / ncclRecv
 * between all pairs of ranks, every shard travelling its own xGMI link.  The communicator belongs to the HIP
 * device that was current at OHXCommInitRank: a call with another device current is refused.
 * librccl.so is loaded at the first of these calls, not linked (nor is its header needed to build). */
typedef void* OHXCommHandle;
#define OHX_UNIQUE_ID_BYTES 128
int OHXCommGetUniqueId(void* id);
int OHXCommInitRank(const void* id, int nranks, int rank, OHXCommHandle* out);
int OHXCommFree(OHXCommHandle comm);
/* RCCL's version code (ncclGetVersion), for a benchmark's record */
int OHXCommInfo(int* rccl_version);
/* rows [*row0, *row0 + *nrows) of rank `rank`: contiguous, sizes differing by at most one row */
int OHXShardRows(bst_ulong nrows_total, int nranks, int rank, bst_ulong* row0, bst_ulong* nrows);
int OHXAllGatherOH(OHXCommHandle comm, const float* d_shard, bst_ulong nrows_local, bst_ulong nrows_total,
                   float* d_full, void* stream);

/* An array that was handed over while "ohx_register_host" was on is about to be freed or reallocated: its registration
 * goes (after the device has been synchronised).  An array the library never registered is not an error. */
int OHXUnregisterHost(const void* array);

/* Returns the device buffers the library keeps between calls to the driver: freed DMatrix storage parked
 * for the next XGDMatrixCreateFromMat (the reference creates and frees its matrix on every OH tick,
 * OH_GridCompMod.F90:347,377; at most two buffers are kept; OHX_DMATRIX_POOL=0 in the environment keeps
 * none), and drops every host registration ("ohx_register_host").  Live handles are not touched. */
int OHXReleaseScratch(void);

#ifdef __cplusplus
}
#endif
#endif /* OHXGB_H_ */
