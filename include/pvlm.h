/*
 * pvlm.h — C ABI of the MI355X-native association + residual/Jacobian engine (libpvlm.so).
 *
 * This is the drop-in boundary for ONE hot path of 3dv-casia/PanoVLM: the ICP-style inner loop
 * (LiDAR<->LiDAR / camera<->LiDAR correspondence search + residual/Jacobian evaluation).  Every
 * entry point names the reference interface it replaces (paths relative to the PanoVLM tree).
 * Plain pointers and sizes only; no exceptions cross the boundary; every function returns a
 * pvlm_status (0 = OK, negative = error, message via pvlm_last_error).
 *
 * Threading: one pvlm_ctx per GPU; a ctx is NOT thread-safe, different ctxs are independent.  A call may use a few short-lived host
 * threads of its own for host-side passes over its inputs (pvlm_scan_upload_batch: bounding boxes and the staging copy of a large batch);
 * they are joined before the call returns.
 * Memory: buffers passed in are caller-owned and only read during the call unless stated.
 * Host pointers unless a parameter is prefixed d_ (device pointer, same GPU as the ctx).
 */
#ifndef PVLM_H_
#define PVLM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pvlm_ctx pvlm_ctx;
typedef struct pvlm_resset pvlm_resset;   /* a device-resident set of residual blocks of one functor */
typedef struct pvlm_neq pvlm_neq;         /* block-sparse normal equations (per-pose 6x6 blocks)     */
typedef struct pvlm_scan pvlm_scan;       /* device-resident feature clouds of one LiDAR scan        */

typedef enum {
  PVLM_OK = 0,
  PVLM_ERR_ARG = -1,      /* bad argument (NULL, negative size, unknown enum)             */
  PVLM_ERR_HIP = -2,      /* HIP runtime error (no device, launch failure, ...)           */
  PVLM_ERR_NOMEM = -3,    /* host or device allocation failed                             */
  PVLM_ERR_STATE = -4,    /* call order violated (e.g. evaluate before pvlm_set_poses)    */
  PVLM_ERR_CAPACITY = -5, /* caller-provided output buffer too small                      */
  PVLM_ERR_REFUSED = -6   /* the input is valid for the reference but outside what this entry point handles (pvlm_ring_extract_batch: a non-finite
                             coordinate, more undecided segmentation edges than its tables hold): the caller takes its own path for it; nothing else failed */
} pvlm_status;

/* Residual functors — base/CostFunction.h.  All are 1 residual x 4 parameter blocks of 3
 * (angleAxis_rw, t_rw, angleAxis_nw, t_nw), i.e. AutoDiffCostFunction<F,1,3,3,3,3>. */
typedef enum {
  PVLM_POINT2PLANE_METER = 0,   /* base/CostFunction.h:567-619 ; row = [P_n(3) plane(4)]            stride 7  */
  PVLM_POINT2PLANE_ANGLE = 1,   /* base/CostFunction.h:630-729 ; row = [P_n(3) plane(4)]            stride 7  */
  PVLM_POINT2LINE_METER = 2,    /* base/CostFunction.h:769-829 ; row = [P_n(3) A(3) B(3)]           stride 9  */
  PVLM_POINT2LINE_ANGLE = 3,    /* base/CostFunction.h:836-934 ; row = [P_n(3) A(3) B(3)]           stride 9  */
  PVLM_PLANE2PLANE_GLOBAL = 4,  /* base/CostFunction.h:350-425 ; row = [plane_ref(3) a(3) b(3) w]   stride 10 */
  PVLM_PLANE_IOU = 5            /* base/CostFunction.h:433-507 ; row = [plane(4) mid_n(3) mid_r(3) angle w] stride 12 */
} pvlm_functor;

#define PVLM_FLAG_NORMALIZE_DISTANCE 1u /* `normalize_distance` of the *_Angle functors (Config.h:117) */

typedef enum {
  PVLM_LOSS_NONE = 0,  /* loss_function == nullptr (util/Optimization.cpp:304,417)         */
  PVLM_LOSS_HUBER = 1  /* ceres::HuberLoss(a)       (util/Optimization.cpp:513-517)        */
} pvlm_loss;

/* ---- context ------------------------------------------------------------------------------ */
pvlm_status pvlm_create(int device, pvlm_ctx** ctx);
pvlm_status pvlm_destroy(pvlm_ctx* ctx);
const char* pvlm_last_error(const pvlm_ctx* ctx);   /* valid until the next call on ctx */
const char* pvlm_version(void);
/* Launch on an externally owned hipStream_t (e.g. the caller's framework stream).  The handle is
 * used as given: NULL is HIP's default (null) stream, which is what a framework hands out for its
 * default stream.  pvlm_use_own_stream returns to the context's private non-blocking stream (the
 * state after pvlm_create).  Kernels of one ctx are always issued on exactly one stream. */
pvlm_status pvlm_set_stream(pvlm_ctx* ctx, void* hip_stream);
pvlm_status pvlm_use_own_stream(pvlm_ctx* ctx);
pvlm_status pvlm_synchronize(pvlm_ctx* ctx);
/* HIP-event timing on the ctx stream (bench.py measures kernel time with these). */
pvlm_status pvlm_timer_start(pvlm_ctx* ctx);
pvlm_status pvlm_timer_stop(pvlm_ctx* ctx, float* elapsed_ms);   /* records, synchronises, returns ms */
pvlm_status pvlm_device_info(pvlm_ctx* ctx, int* cu_count, int64_t* hbm_bytes, char* name, int name_cap);
/* Device memory.  Every device buffer of a context comes from a caching sub-allocator owned by the context (hipMalloc
 * maps pages at 40-70 ms per GB on MI355X; the reference's own loop re-associates every outer iteration,
 * lidar_mapping/LidarOdometry.cpp:38-110, so scratch and outputs of similar size are needed again and again).
 * pvlm_reserve makes sure ONE free range of `bytes` exists (a production host reserves its working set once, next to
 * uploading the scans); pvlm_trim synchronises and returns every unused slab to the driver; pvlm_mem_info reports bytes
 * held from the driver, bytes handed out, the high-water mark and the number of hipMalloc calls so far (a steady state
 * adds none).  Any pointer may be NULL.  PVLM_NO_POOL=1 in the environment bypasses the pool (debugging). */
pvlm_status pvlm_reserve(pvlm_ctx* ctx, int64_t bytes);
/* The pinned staging window of pvlm_scan_upload[_batch] (64 MB by default, PVLM_UPLOAD_STAGE_MB) is allocated by the first upload that needs it:
 * hipHostMalloc + first touch of 64 MB cost 25 ms.  A host that knows it will upload reserves the window at start-up.  The same call allocates the
 * 32 MB pinned arena every other small host <-> device copy of the context goes through (8 ms inside whichever call needs it first otherwise).      */
pvlm_status pvlm_reserve_staging(pvlm_ctx* ctx, int64_t bytes);
/* Loads the code objects of the library's kernels now (one empty launch per translation unit + a synchronisation).  HIP loads a code object at the first launch of
 * one of its kernels — 5-20 ms each, ~60 ms for all of them — which otherwise lands inside the first call that needs it (the first EstimatePose of a process).  Like
 * pvlm_reserve / pvlm_reserve_staging: once per context, after pvlm_create; never needed for correctness. */
pvlm_status pvlm_preload(pvlm_ctx* ctx);
pvlm_status pvlm_trim(pvlm_ctx* ctx);
pvlm_status pvlm_mem_info(const pvlm_ctx* ctx, int64_t* reserved, int64_t* in_use, int64_t* peak, int64_t* device_allocs);
/* HIP graph of a step: the calls issued between _begin and _end on this context (pvlm_set_poses_dev,
 * pvlm_neq_accumulate_dev / pvlm_eval_pair_blocks_dev / pvlm_eval_dev, pvlm_allreduce_sum_f64 — the `_dev` forms, which
 * neither allocate nor synchronise once they have run once with the same objects) are captured instead of executed;
 * pvlm_graph_launch replays them as one submission on the context's stream with the CURRENT contents of the device
 * buffers they were given (pose arrays, packed buffer).  One LM step is five small kernels around the fused one: replayed
 * as a graph they cost one launch.  A call that would have to allocate or synchronise inside a capture fails with
 * PVLM_ERR_STATE (run the step once eagerly first).  Needs a real stream (the context's own, or one given to
 * pvlm_set_stream), not the legacy NULL stream. */
typedef struct pvlm_graph pvlm_graph;
pvlm_status pvlm_graph_begin(pvlm_ctx* ctx);
pvlm_status pvlm_graph_end(pvlm_ctx* ctx, pvlm_graph** out);
pvlm_status pvlm_graph_launch(pvlm_ctx* ctx, pvlm_graph* graph);
pvlm_status pvlm_graph_destroy(pvlm_ctx* ctx, pvlm_graph* graph);
/* Per-kernel timing of the dominant kernels: when enabled, every launch of the fused
 * residual/Jacobian kernel (which=0), the materialise kernel (which=1) and the k-NN + plane-fit
 * association kernel (which=2) and of the batched camera-LiDAR vote kernel (which=3) is bracketed by HIP events on the ctx stream.  pvlm_profile_read
 * synchronises and returns the accumulated milliseconds and launch count since the last
 * pvlm_profile_enable(ctx, 1). */
pvlm_status pvlm_profile_enable(pvlm_ctx* ctx, int on);
pvlm_status pvlm_profile_read(pvlm_ctx* ctx, int which, double* total_ms, int64_t* launches);

/* ---- parameter blocks ---------------------------------------------------------------------- *
 * The pose table the residual blocks index: angleAxis_lw_list / t_lw_list of
 * lidar_mapping/LidarOdometry.cpp:23-33 (and angleAxis_cw_list / t_cw_list of
 * joint_optimization/CameraLidarOptimizer.cpp:387-548 appended behind them).  n x 3 each. */
pvlm_status pvlm_set_poses(pvlm_ctx* ctx, int n, const double* angle_axis, const double* translation);
pvlm_status pvlm_set_poses_dev(pvlm_ctx* ctx, int n, const double* d_angle_axis, const double* d_translation);

/* ---- residual sets ---------------------------------------------------------------------------- *
 * Replaces the per-correspondence `X::Create(...)` + `problem.AddResidualBlock(cost, loss, aa_r,
 * t_r, aa_n, t_n)` loops of util/Optimization.cpp:538-557 (point-to-plane), :410-434
 * (line-to-line), :583-602 (camera-LiDAR).  Residual blocks are grouped in `n_pairs` segments;
 * segment p = rows [pair_offsets[p], pair_offsets[p+1]) all share the parameter blocks
 * (pair_ref[p], pair_nei[p]) — exactly the (i, n_idx) loop nest of the reference.  `rows` is
 * n x stride doubles with the per-functor row layout given at pvlm_functor.  `weight` is the
 * scalar weight of kinds 0..3 (ignored by the *_Angle functors, as in the reference). */
pvlm_status pvlm_resset_upload(pvlm_ctx* ctx, pvlm_functor kind, unsigned flags, double weight, int64_t n,
                               int n_pairs, const int64_t* pair_offsets, const int* pair_ref, const int* pair_nei,
                               const double* rows, int stride, pvlm_resset** out);
pvlm_status pvlm_resset_destroy(pvlm_ctx* ctx, pvlm_resset* rs);
pvlm_status pvlm_resset_info(const pvlm_resset* rs, int64_t* n, int* n_pairs, int* kind, unsigned* flags);
/* Point-to-plane sets: consecutive rows whose plane is bit-identical share one entry of a plane table that the fused evaluation
 * (pvlm_eval_pair_blocks*, pvlm_neq_accumulate*) then reads instead of the four plane columns.  *in_use: 1 when the set was given the table
 * (by its mean run length, or PVLM_PLANE_RUNS=0/1); *runs: the runs counted (0 when the set was never counted).  Results do not depend on it. */
pvlm_status pvlm_resset_plane_runs(const pvlm_resset* rs, int* in_use, int64_t* runs);
/* Point-to-plane sets made by pvlm_assoc_point2plane that took the plane-run table in the block form, with at most 65 536 queries per neighbour scan: the
 * fused evaluation reads a row's point (columns 0..2) from ONE table per distinct neighbour scan of the call, through the row's 16-bit query number, and
 * visits its work list in an order that brings the readers of a table slice together (PVLM_POINT_TABLE=0/1, PVLM_DISPATCH_ORDER=0/1).  The tables are a snapshot
 * owned by the set.  *in_use: 1 when the set has the form; *tables: its tables; *positions: the grid of the fused kernel (work-list entries + padding;
 * the number of work-list entries when the order is the identity).  Results do not depend on any of it. */
pvlm_status pvlm_resset_point_table(const pvlm_resset* rs, int* in_use, int* tables, int* positions);
/* Debug read of that form, shaped like pvlm_assoc_point2plane_debug: per residual block in compact order the stored query number (qnum, n entries) and the
 * entry of its neighbour's table under that number (points, n x 3 doubles).  Either may be NULL.  PVLM_ERR_STATE when the set does not have the form. */
pvlm_status pvlm_resset_point_table_debug(pvlm_ctx* ctx, const pvlm_resset* rs, uint16_t* qnum, double* points);
/* Copies the segment table / rows back (rows in the upload layout); any pointer may be NULL. */
pvlm_status pvlm_resset_download(pvlm_ctx* ctx, const pvlm_resset* rs, int64_t* pair_offsets, int* pair_ref,
                                 int* pair_nei, double* rows);
/* Replaces the pose ids of the set's segments (pair_ref / pair_nei, n_pairs each).  A set produced by the association carries the ids
 * of the scans it was built from (lidars[i].id, util/Optimization.cpp:527-528); a problem that mixes such sets with uploaded ones
 * (camera poses + LiDAR poses, joint_optimization/CameraLidarOptimizer.cpp:394-417) renumbers them once into ONE pose table, so that a
 * single pvlm_set_poses and a single packed buffer serve every set.  Queued on the context stream; no synchronisation. */
pvlm_status pvlm_resset_set_pose_ids(pvlm_ctx* ctx, pvlm_resset* rs, const int* pair_ref, const int* pair_nei);

/* ceres::CostFunction::Evaluate for every block of the set at the poses of pvlm_set_poses:
 * residuals[n] and jacobians[n x 12] = [d/daa_r | d/dt_r | d/daa_n | d/dt_n] (row-major per block,
 * the layout AutoDiffCostFunction<F,1,3,3,3,3> hands to Ceres).  jacobians may be NULL (cost-only
 * evaluation).  Values are the RAW residuals (no loss applied), as Evaluate returns them. */
pvlm_status pvlm_eval(pvlm_ctx* ctx, const pvlm_resset* rs, double* residuals, double* jacobians);
/* Same, outputs left in device memory (async on the ctx stream; no host copies). */
pvlm_status pvlm_eval_dev(pvlm_ctx* ctx, const pvlm_resset* rs, double* d_residuals, double* d_jacobians);

/* ---- host-visible evaluation: the Ceres-feeding boundary ------------------------------------------------------- *
 * ceres::CostFunction::Evaluate reads host memory, so the last hop of this mode is a PCIe link (30 GB/s measured on the
 * MI355X box, against 5 TB/s for the kernel): the API is built around that hop.
 *   pvlm_host_alloc / _free     page-locked host memory (the copies run at link rate and asynchronously only into it;
 *                               pageable destinations work but serialise).
 *   pvlm_eval_host_async        residuals[n] and jacobians[n x 12] (NULL = cost only) as pvlm_eval, delivered
 *                               asynchronously on the context's stream: 104 B per block.
 *   pvlm_eval_wrench_host_async the same information in 56 B per block: wrench_rows[n x 7] = [r | c(3) | g(3)] plus the
 *                               per-pair tables pair_tables[n_pairs x PVLM_PAIR_TABLE] = [R_rn(9) | t_rn(3) | t_rw(3) |
 *                               J_l(aa_r)(9) | M_n(9)], from which the host forms the row on demand (36 multiply-adds):
 *                                 d r/d aa_r = c^T J_l      d r/d t_r = g^T      d r/d aa_n = c^T M_n      d r/d t_n = -g^T R_rn
 *                               (row-major 3x3 blocks; integration/pvlm_ceres.hpp does it inside Evaluate).
 *   pvlm_eval_force_host_async  kinds 0..3 (the point functors), 32 B per block: force_rows[n x 4] = [r | g(3)].  The moment is
 *                               c = (R_rn P_n + t_rn - t_rw) x g with P_n = the first three entries of the block's row (the host holds them:
 *                               pvlm_resset_download) and R_rn, t_rn, t_rw from the pair table — 15 more multiply-adds in Evaluate for
 *                               43 % fewer bytes over the link, which is the roof of this mode.
 * All three go through a bounded device staging buffer (PVLM_STAGE_ROWS rows, 32 M by default) slice by slice; the results
 * are complete after pvlm_synchronize.  Residuals are RAW (no loss), in the compact order of pvlm_resset_download. */
#define PVLM_PAIR_TABLE 33
pvlm_status pvlm_host_alloc(pvlm_ctx* ctx, int64_t bytes, void** out);
pvlm_status pvlm_host_free(pvlm_ctx* ctx, void* p);
pvlm_status pvlm_eval_host_async(pvlm_ctx* ctx, const pvlm_resset* rs, double* residuals, double* jacobians_or_null);
pvlm_status pvlm_eval_wrench_host_async(pvlm_ctx* ctx, const pvlm_resset* rs, double* wrench_rows, double* pair_tables);
pvlm_status pvlm_eval_force_host_async(pvlm_ctx* ctx, const pvlm_resset* rs, double* force_rows, double* pair_tables);

/* Fused evaluation: residual + Jacobian in registers, loss-corrected (Ceres corrector for
 * rho'' <= 0: scale r and J by sqrt(rho')) and contracted into per-pair normal-equation blocks
 *   out[p] = [ H_rr(36) | H_rn(36) | H_nn(36) | g_r(6) | g_n(6) | cost(1) ]   (121 doubles, row-major)
 * with H = J^T J, g = J^T r, cost = sum 1/2 rho(r^2) over the segment.  Deterministic. */
#define PVLM_PAIR_BLOCK 121
pvlm_status pvlm_eval_pair_blocks(pvlm_ctx* ctx, const pvlm_resset* rs, pvlm_loss loss, double loss_a, double* out);
pvlm_status pvlm_eval_pair_blocks_dev(pvlm_ctx* ctx, const pvlm_resset* rs, pvlm_loss loss, double loss_a, double* d_out);

/* ---- block-sparse normal equations ------------------------------------------------------------ *
 * The Gauss-Newton system the outer trust-region solver needs (what Ceres assembles internally
 * from the blocks of ceres::Problem; LidarOdometry.cpp:36-80).  Packed layout (doubles):
 *   [ Hdiag n_poses x 36 | Hoff n_upairs x 36 | g n_poses x 6 | cost 1 ]
 * Hoff[u] is the 6x6 block d2/dx_i dx_j for the unordered pose pair (upair_i[u] < upair_j[u]).
 * One RCCL all-reduce(sum) of this buffer per LM iteration is the only multi-GPU exchange. */
pvlm_status pvlm_neq_create(pvlm_ctx* ctx, int n_poses, int n_upairs, const int* upair_i, const int* upair_j,
                            pvlm_neq** out);
pvlm_status pvlm_neq_destroy(pvlm_ctx* ctx, pvlm_neq* neq);
int64_t pvlm_neq_size(const pvlm_neq* neq); /* number of doubles in the packed buffer */
/* packed (+)= contribution of one residual set.  d_packed is a device buffer of pvlm_neq_size()
 * doubles (e.g. the tensor handed to the all-reduce); zero_first!=0 clears it before adding. */
pvlm_status pvlm_neq_accumulate_dev(pvlm_ctx* ctx, pvlm_neq* neq, const pvlm_resset* rs, pvlm_loss loss,
                                    double loss_a, int zero_first, double* d_packed);
pvlm_status pvlm_neq_accumulate(pvlm_ctx* ctx, pvlm_neq* neq, const pvlm_resset* rs, pvlm_loss loss, double loss_a,
                                int zero_first, double* packed_host_inout);
/* The same contribution, queued: the set is linearised into the structure's OWN device buffer (kept with the handle) and its copy
 * into `packed` (host, pvlm_neq_size() doubles) is queued behind it — nothing is allocated after the first call and nothing
 * waits.  An LM driver calls it once per residual set of its problem (pvlm_set_poses in that set's pose numbering first) and then
 * pvlm_synchronize ONCE: every `packed` is complete when that returns.  One submission and one synchronisation per
 * linearisation, whatever the number of residual sets (lidar_mapping/LidarOdometry.cpp:36-80 evaluates point-to-plane and
 * line-to-line blocks in the same ceres::Solve). */
pvlm_status pvlm_neq_accumulate_async(pvlm_ctx* ctx, pvlm_neq* neq, const pvlm_resset* rs, pvlm_loss loss, double loss_a, double* packed);
/* A whole problem in ONE packed buffer: the n residual sets are linearised one after the other and SUMMED on the device into the
 * buffer of neq[0] (all n structures must have been created with the same n_poses and pair list, and the sets must share one pose
 * numbering — pvlm_resset_set_pose_ids below); one copy into `packed` (host, pvlm_neq_size(neq[0]) doubles) is queued behind them and
 * is complete after the next pvlm_synchronize.  Nothing is allocated after the first call, nothing waits. */
pvlm_status pvlm_neq_accumulate_sets(pvlm_ctx* ctx, int n, pvlm_neq* const* neq, const pvlm_resset* const* rs, const pvlm_loss* loss,
                                     const double* loss_a, double* packed);

/* ---- panoramic reprojection blocks with point elimination ---------------------------------------- *
 * PanoramaReprojResidual_1Angle (base/CostFunction.h:218-247): r = w * angle(R(aa_cw) X + t_cw, bearing),
 * three parameter blocks (aa_cw, t_cw, point_3d), added per track observation by AddCameraResidual
 * (util/Optimization.cpp:172-222) inside CameraLidarOptimizer::Optimize (CameraLidarOptimizer.cpp:431-432),
 * solved upstream by Ceres *_SCHUR (util/Optimization.cpp:608-634).  Here the 3-D points live on the GPU
 * and are eliminated there: the host only sees the reduced 6x6 camera blocks.
 *   observations are grouped by point: point p owns [point_offsets[p], point_offsets[p+1]);
 *   cam_ids index the pose table of pvlm_set_poses (angleAxis_cw, t_cw);
 *   bearings: n_obs x 3, any norm (normalised like the functor's constructor); points: n_points x 3.
 * Packed output of pvlm_ba_reduce (pvlm_ba_packed_size doubles), F = n_cams, U = n_upairs (co-visible pairs,
 * ui < uj, from pvlm_ba_structure):
 *   [ S_diag F x 36 | S_off U x 36 (rows ui, cols uj) | g F x 6 | cost | U_diag F x 6 | g_cam F x 6 | gmax_points ]
 * S, g = Schur complement of the point blocks damped as the LM driver damps every column:
 *   V* = V + diag(clamp(V_kk s_k^2, min_diag, max_diag) / (radius s_k^2)),  s_k = 1/(1+sqrt(V_kk)) at the
 *   first call (init_scale = 1; Ceres' Jacobi scaling), cameras are left undamped/unscaled for the caller;
 * U_diag / g_cam = diagonal and gradient of the camera blocks BEFORE elimination (for the caller's scaling,
 * damping and gradient test);
 * gmax_points = max |gradient| over the point blocks; cost = sum rho(r^2)/2.
 * pvlm_ba_step back-substitutes the points for the camera steps dcam (F x 6, zeros for constant blocks; it needs a
 * pvlm_ba_reduce at the current poses: no pvlm_set_poses since, or one that set the same values from host memory again, so that a
 * caller with several sets can reload each set's poses before its step) into the candidate points and returns out3 = [model cost decrease of these blocks, |dX|^2, |X|^2];
 * pvlm_ba_cost evaluates the cost at the current (candidate = 0) or candidate points with the poses of the
 * last pvlm_set_poses; pvlm_ba_accept makes the candidate current.  pvlm_ba_eval materialises r and the
 * 1x9 Jacobian rows [d/daa_cw | d/dt_cw | d/dX] (Ceres-feeding / parity mode).  pvlm_ba_set_constant marks
 * points (mask[p] != 0) as constant parameter blocks (Problem::SetParameterBlockConstant, the
 * refine_structure = false case of CameraLidarOptimizer.cpp:462-466): they are neither eliminated nor moved;
 * mask = NULL frees all. */
typedef struct pvlm_baset pvlm_baset;
pvlm_status pvlm_ba_create(pvlm_ctx* ctx, int n_points, int64_t n_obs, const int64_t* point_offsets, const int* cam_ids,
                           const double* bearings, const double* points, double weight, pvlm_baset** out);
pvlm_status pvlm_ba_destroy(pvlm_ctx* ctx, pvlm_baset* set);
pvlm_status pvlm_ba_structure(const pvlm_baset* set, int* n_points, int64_t* n_obs, int* n_cams, int* n_upairs, int* ui, int* uj);
int64_t pvlm_ba_packed_size(const pvlm_baset* set);
pvlm_status pvlm_ba_get_points(pvlm_ctx* ctx, const pvlm_baset* set, int candidate, double* points);
pvlm_status pvlm_ba_set_points(pvlm_ctx* ctx, pvlm_baset* set, const double* points);
pvlm_status pvlm_ba_set_constant(pvlm_ctx* ctx, pvlm_baset* set, const unsigned char* mask_or_null);
pvlm_status pvlm_ba_eval(pvlm_ctx* ctx, const pvlm_baset* set, double* r, double* J_or_null);
pvlm_status pvlm_ba_reduce(pvlm_ctx* ctx, pvlm_baset* set, pvlm_loss loss, double loss_a, int init_scale, double radius,
                           double min_diag, double max_diag, double* packed);
pvlm_status pvlm_ba_step(pvlm_ctx* ctx, pvlm_baset* set, pvlm_loss loss, double loss_a, const double* dcam, double* out3);
pvlm_status pvlm_ba_cost(pvlm_ctx* ctx, const pvlm_baset* set, pvlm_loss loss, double loss_a, int candidate, double* cost);
pvlm_status pvlm_ba_accept(pvlm_ctx* ctx, pvlm_baset* set);

/* ---- K31: the two-row reprojection kinds (SfMGlobalBA / MVS::RefineCameraPose) ----------------------------------- *
 * AddCameraResidual (util/Optimization.cpp:172-222) adds, per (track, observation) of a frame with a valid pose:
 *   PVLM_BA_ANGLE1  PanoramaReprojResidual_1Angle (base/CostFunction.h:218-247): obs = n_obs x 3 bearings, exactly
 *                   pvlm_ba_create; pvlm_ba_create(...) == pvlm_ba_create_kind(PVLM_BA_ANGLE1, 0, 0, ...).
 *   PVLM_BA_ANGLE2  PanoramaReprojResidual_2Angle (:178-214): obs = n_obs x 2 sphere angles (lon, lat) as
 *                   eq.ImageToSphere(kp.pt) gives them (float template, Equirectangular.h:99-105, widened to double); the
 *                   constructor's "x += 2 pi if x < 0" is applied here, in double.
 *                   r = w (lon' - x, lat - y), lon' = atan2(p0, p2) + (2 pi if < 0), lat = -asin(p1 / |p|).
 *   PVLM_BA_PIXEL   PanoramaReprojResidual_Pixel (:249-288): obs = n_obs x 2 keypoint pixels kp.pt (float widened to
 *                   double, no rounding); rows, cols > 0 = image size.
 *                   r = w (cols (0.5 + lon / 2pi) - x, rows (0.5 - lat / pi) - y).
 * p = R(aa_cw) X + t_cw with the exact atan2 / asin (not FastAtan2).  Parity traps kept from upstream, not fixed:
 *   - no seam wrap: the pixel residual jumps by cols across lon = +-pi, the 2Angle one by 2 pi across lon = 0;
 *   - the loss acts on the block's squared norm s = r0^2 + r1^2 (Huber's outer region scales r and J by sqrt(rho'),
 *     no rank-one term), as for the one-row kind;
 *   - at the poles (p0 = p2 = 0) upstream's Jets give inf / NaN derivatives; here both rows' derivatives are 0.
 * The Jacobian is closed form (dlon/dp = (p2, 0, -p0) / (p0^2 + p2^2), dlat/dp = -(e1 - p1 p / |p|^2) / sqrt(p0^2 + p2^2)).
 * Every other entry point takes a set of any kind with the same meaning and the same packed layout; for a two-row set
 * pvlm_ba_eval writes n_obs x 2 residuals (row 0 then row 1 of each observation) and n_obs x 2 x 9 Jacobian rows.
 * The reduce of every kind is the gather form: no atomics, the same bits on every run. */
typedef enum { PVLM_BA_ANGLE1 = 0, PVLM_BA_ANGLE2 = 1, PVLM_BA_PIXEL = 2 } pvlm_ba_kind;
pvlm_status pvlm_ba_create_kind(pvlm_ctx* ctx, pvlm_ba_kind kind, int rows, int cols, int n_points, int64_t n_obs, const int64_t* point_offsets,
                                const int* cam_ids, const double* obs, const double* points, double weight, pvlm_baset** out);
/* kind, image size and residual rows per observation (1 or 2) of a set; null outputs are skipped */
pvlm_status pvlm_ba_info(const pvlm_baset* set, pvlm_ba_kind* kind, int* rows, int* cols, int* rows_per_obs);

/* ---- K31: track filters after a global BA (SfM::GlobalBundleAdjustment, sfm/SfM.cpp:1362-1383) ------------------- *
 * One thread per track, all-of over its observations; keep[t] = 1 when the track survives.  The caller compacts.
 *   track t owns the observations [point_offsets[t], point_offsets[t+1]); frame_ids[i] indexes T_cw (n_frames x 12, row-major
 *   3 x 4 [R | t]); keypoints_f32: n_obs x 2 keypoint pixels (cv::Point2f); points: n_points x 3 (double).
 *   T_cw = GetPose().inverse() for valid frames, all zero for invalid ones (upstream does not skip them).  The host mirror
 *   inverts rigidly (R^T, -R^T t), as elsewhere; upstream's general Eigen 4x4 inverse differs by about 1e-16.
 *   p = ((T0 X0 + T1 X1) + T2 X2) + T3 per row, in double.
 * PVLM_FILTER_PIXEL  FilterTracksPixelResidual (sfm/Structure.cpp:121-156): threshold < 0 keeps everything.  Rejects when
 *   (kp.x - u)^2 + (kp.y - v)^2 > threshold^2 in double, (u, v) = the double eq.CamToImage with FastAtan2
 *   (USE_FAST_ATAN2).  An invalid frame projects (0, 0, 0) to the image centre, so its observation can reject.
 * PVLM_FILTER_ANGLE  FilterTracksAngleResidual (:158-193): rejects when (p . ray) / |p| / |ray| < cos(threshold pi / 180)
 *   (the cosine is taken on the host).  ray = eq.ImageToCam(kp.pt), which binds to the cv::Point2i overload: the keypoint
 *   is rounded half-to-even and un-projected in float with r = 1.  |ray| = cv::norm(Point3f) is taken as
 *   sqrt((double)x*x + (double)y*y + (double)z*z), recalled from OpenCV, not pinned.  An invalid frame gives a NaN cosine:
 *   its observations never reject.
 * Threshold tests in double without FMA contraction: the same decisions as a non-FMA x86-64 build. */
typedef enum { PVLM_FILTER_PIXEL = 0, PVLM_FILTER_ANGLE = 1 } pvlm_filter_mode;
pvlm_status pvlm_filter_tracks(pvlm_ctx* ctx, pvlm_filter_mode mode, int rows, int cols, int n_points, const int64_t* point_offsets, const int* frame_ids,
                               const float* keypoints_f32, const double* points, int n_frames, const double* T_cw_3x4, double threshold,
                               unsigned char* keep);

/* ---- K32: structure from tracks (TriangulateTracks / FilterTracksToFar, sfm/Structure.cpp:8-119) ---- *
 * One lane per track; the caller compacts, as with pvlm_filter_tracks.  Same input convention: track t owns the observations
 * [track_offsets[t], track_offsets[t+1]) in their order, frame_ids[i] indexes the frame tables, T_cw = n_frames x 12 row-major [R | t].
 * pvlm_triangulate_tracks: TriangulateNView (sfm/Triangulate.cpp:198-226) per track.  Exactly one of keypoints_f32 (n_obs x 2 pixels;
 *   the bearing is eq.ImageToCam(kp.pt) through the cv::Point2i overload, taken on the device as in PVLM_FILTER_ANGLE; rows, cols > 0)
 *   and bearings_f32 (n_obs x 3, bearings of any origin, e.g. sfm/SfM.cpp:1503) is non-null; anything else is PVLM_ERR_ARG.
 *   frame_valid: n_frames bytes or NULL (every frame valid).  Two observations: Triangulate2View (the midpoint in camera 1, moved to the
 *   world), more: TriangulateNViewAlgebraic (the eigenvector of the smallest eigenvalue of AtA, hnormalized), fewer: +inf.  All in double,
 *   without FMA contraction; nothing is special-cased, IEEE runs its course on degenerate input.
 *   status[t]: 0 = triangulated; 1 = dropped by upstream's rule "any coordinate is +-inf" (:56-57), the point is written as computed;
 *              2 = an observation lies in a frame with frame_valid == 0, the point is NaN.
 * Traps and divergences, next to K31's:
 *   - a NaN point is NOT dropped (status 0): isinf(NaN) is false upstream, e.g. two parallel rays from one centre.  Kept.
 *   - status 2 is the one deliberate divergence: upstream inverts the singular pose of an invalid frame with Eigen's general inverse and
 *     hands the result to the eigen-solver; what comes out depends on those two routines on inf / NaN input and cannot be pinned here.
 *   - the N-view eigenvector comes from a cyclic Jacobi, upstream's from Eigen's tridiagonal QL: parity to rounding, not in bits.
 *   - the output order of the host mirror's TriangulateTracks is ascending track id, what one thread gives upstream; upstream's own
 *     order is whatever its OpenMP critical section gives.
 * pvlm_filter_tracks_far: FilterTracksToFar.  points: n_tracks x 3; t_wc: n_frames x 3 camera centres.  Per track, over its distinct
 *   frames with a valid pose in ascending id: baseline = the largest centre distance (FurthestPoints, base/Geometry.hpp:594-617; 0 with
 *   fewer than two centres), average = the mean of |centre - point| (NaN without centres).  keep[t] = 0 when
 *   threshold * baseline < average; NaN compares false, so such a track is kept. */
pvlm_status pvlm_triangulate_tracks(pvlm_ctx* ctx, int rows, int cols, int n_tracks, const int64_t* track_offsets, const int* frame_ids,
                                    const float* keypoints_f32 /* n_obs x 2, or NULL */, const float* bearings_f32 /* n_obs x 3, or NULL */,
                                    int n_frames, const double* T_cw_3x4, const unsigned char* frame_valid, double* points /* n_tracks x 3 */,
                                    unsigned char* status /* n_tracks */);
pvlm_status pvlm_filter_tracks_far(pvlm_ctx* ctx, int n_tracks, const int64_t* track_offsets, const int* frame_ids, const double* points, int n_frames,
                                   const double* t_wc /* n_frames x 3 */, const unsigned char* frame_valid, double threshold, unsigned char* keep);

/* ---- K33: brute-force 2-NN SIFT matching (MatchSIFT util/SIFT.cpp:130-162, SfM::MatchImagePairs sfm/SfM.cpp:229-295) ---- *
 * The definition (csrc/pvlm_match_core.h): descriptors are rows of 128 float; d2(a, b) = the fmaf chain c = fmaf(a[k] - b[k], a[k] - b[k], c) over
 * k = 0..127 from c = 0; distance = sqrtf(d2); the two nearest train rows by (d2, index), an exact tie to the lower index; ratio test
 * distance0 < ratio * distance1 in float, strictly; matches in query order.  [recalled] the summation order of cv::cuda's brute-force matcher is
 * not pinned; the FLANN branch of MatchSIFT is approximate and not mirrored.
 * Deliberate divergence: a train side with exactly ONE row gives no matches (upstream reads raw_matches[i][1] out of bounds there); a side
 * with no rows gives none either, as upstream.
 * pvlm_descset_create: the descriptors of n frames (rows[f] x 128 floats, row-major, descs[f] may be NULL when rows[f] == 0) copied to the device,
 *   where they stay (what upstream's d_descriptors[i].upload does, sfm/SfM.cpp:237-243).  width must be 128 (PVLM_ERR_ARG otherwise); a non-finite
 *   value anywhere is PVLM_ERR_ARG, found by a device-side check.  The set belongs to the context it was created with: another one is PVLM_ERR_ARG.
 * pvlm_match_knn2: the raw knnMatch(d[src], d[tgt], 2) of every pair: per query of pair p, in pair order, then query order, the two train indices
 *   (-1 where absent) and the two distances (+inf where absent); idx and dist hold 2 x sum(rows[src[p]]) entries.
 * pvlm_match_pairs: the loop body of SfM::MatchImagePairs for every pair: MatchSIFT, then the pair filter (:266-275): the pair is dropped with
 *   fewer than matches_threshold matches; of the others the matches with (double)distance < 0.8 * (double)dmax stay (dmax the pair's largest
 *   distance); dropped again with fewer than matches_threshold left.  matches_threshold < 0 is PVLM_ERR_ARG (upstream's first comparison converts
 *   it to size_t and drops every pair).  keep[p] = 1 for a surviving pair; its records are out[match_offsets[p] .. match_offsets[p + 1]), in query
 *   order; pairs come out in the order of the input list (upstream: the order of an OpenMP critical section).  *needed = match_offsets[n_pairs];
 *   when it exceeds capacity the call returns PVLM_ERR_CAPACITY with keep, match_offsets and *needed set and no record past capacity written.
 * flags: PVLM_FLAG_MATCH_EXACT evaluates the definition for every (query, train row) on the vector ALU.  Without it every query is screened on the
 *   fp32 matrix core (s = |a|^2 + |b|^2 - 2 a.b, the 4 smallest), the 4 candidates are evaluated with the definition and accepted only when a
 *   worst-case rounding bound certifies that no other row can enter or tie the top two; every other query is evaluated exactly.  The results are
 *   bit-identical in both modes; stats->fallback_queries counts the exactly evaluated ones. */
#define PVLM_FLAG_MATCH_EXACT 0x400u
typedef struct pvlm_descset pvlm_descset;
typedef struct pvlm_match { int query, train; float distance; } pvlm_match;
typedef struct pvlm_match_stats { long long queries, fallback_queries; int batches; } pvlm_match_stats;
pvlm_status pvlm_descset_create(pvlm_ctx* ctx, int n_frames, const int* rows, int width, const float* const* descs, pvlm_descset** out);
void pvlm_descset_destroy(pvlm_ctx* ctx, pvlm_descset* set);
pvlm_status pvlm_match_knn2(pvlm_ctx* ctx, const pvlm_descset* set, int n_pairs, const int* src, const int* tgt, unsigned flags, int* idx, float* dist,
                            pvlm_match_stats* stats_or_null);
pvlm_status pvlm_match_pairs(pvlm_ctx* ctx, const pvlm_descset* set, int n_pairs, const int* src, const int* tgt, float ratio, int matches_threshold,
                             unsigned flags, unsigned char* keep /* n_pairs */, long long* match_offsets /* n_pairs + 1 */, pvlm_match* out, long long capacity,
                             long long* needed, pvlm_match_stats* stats_or_null);

/* ---- K34: relative poses from the matches (SfM::FilterImagePairs sfm/SfM.cpp:298-480, base/EssentialMatrix.cpp, base/ACRansac_NFA.cpp) ---- *
 * The definition (csrc/pvlm_essential_core.h): per pair n_runs (upstream: 40) independent runs of FindEssentialACRANSAC (base/EssentialMatrix.cpp:180-288, ac_ransac_mode
 * = true as upstream forces it, so there is no `precision`) with up to max_iterations (upstream: 300) hypotheses; ComputeEssential (:10-40) with both of Eigen's
 * decompositions restated as a cyclic Jacobi in fp64 of fixed rotation order (parity with Eigen by tolerance); the residual Square(asin(p2 . (E p1).normalized())) and
 * ACRansac_NFA::ComputeNFA (base/ACRansac_NFA.cpp:103-137, the non-quantified branch, max_threshold = inf) with asin and log10 evaluated without libm, identically on the
 * host and on the device; DecomposeEssential (:151-178) and SfM::CheckRT (sfm/SfM.cpp:1478-1547) on the run's inliers with the 3-degree tests as comparisons of the
 * cosine against a threshold derived from the host's acos; the selection inside a run (:361-380) and over the runs (:413-416).  As upstream, hypothesis k of a run is
 * fitted to all 8 (k + 1) points sampled so far (min_point_set1/2 are never cleared, :194).
 * Deliberate divergences: the sampling is a Philox-4x32-10 stream keyed by (seed, src frame, tgt frame, run) (upstream: std::random_device per draw; nothing to be equal
 * to), so the result of a pair does not depend on the other pairs of the call; a pair with fewer than 9 matches is dropped (upstream returns zero below 8 and reads out
 * of bounds at exactly 8); among runs with equal CheckRT counts the lowest run index wins (upstream: an unstable sort); parallax is not produced (its reader is
 * commented out upstream, :369-373); PVLM_FLAG_ESSENTIAL_FRESH_SAMPLE fits every hypothesis to its own 8 points only (the textbook 8-point hypothesis).
 * Inputs: bearings[f] = rows[f] x 3 floats, eq.ImageToCam of the frame's keypoints (sfm/SfM.cpp:311-319; pvlm_image_to_cam_f32); the matches of pair p are
 * matches[match_offsets[p] .. match_offsets[p + 1]), query a keypoint of src[p], train one of tgt[p]: what pvlm_match_pairs writes.  A frame or keypoint index out of
 * range, n_runs < 1, max_iterations outside [1, 2^24], more than 2^29 matches in one pair are PVLM_ERR_ARG.
 * pvlm_essential_acransac: the raw result of every run: E (row-major, chain c = p * n_runs + run; all zero = no model), the run's minNFA (+inf for a dropped pair), and
 *   the run's inlier set (indices into the pair's matches, in the order of the sorted residuals, as upstream leaves inlier_idx) at inliers[inlier_offsets[c] ..).
 * pvlm_filter_image_pairs: the loop body of FilterImagePairs up to, and not including, RefineRelativePose: keep[p], R_21 (row-major), t_21 of the winning run, its
 *   CheckRT inliers (indices into the pair's matches, ascending) at inlier_idx[inlier_offsets[p] ..) and their triangulated points (camera 1's frame).
 * Both: *needed = the records in all; when it exceeds capacity the call returns PVLM_ERR_CAPACITY with everything but the records set and no record past capacity
 * written.  stats: chains run, hypotheses evaluated, chains that ran in LDS and chains (pairs above 1024 matches) that sorted through global scratch.
 * A call works through its pair list in batches of up to 2^15 chains; the environment variable PVLM_ESSENTIAL_BATCH_PAIRS (read at every call) lowers the number of
 * pairs per batch.  It changes no result; the tests use it to run several batches on a small list. */
#define PVLM_FLAG_ESSENTIAL_FRESH_SAMPLE 0x800u
typedef struct pvlm_essential_params { int n_runs /* 40 */, max_iterations /* 300 */, triangulation_num_threshold; unsigned long long seed; } pvlm_essential_params;
typedef struct pvlm_essential_stats { long long chains, hypotheses, lds_chains, fallback_chains; } pvlm_essential_stats;
pvlm_status pvlm_essential_acransac(pvlm_ctx* ctx, int n_frames, const float* const* bearings /* 3 floats per keypoint */, const int* rows, int n_pairs, const int* src,
                                    const int* tgt, const long long* match_offsets /* n_pairs + 1 */, const pvlm_match* matches, const pvlm_essential_params* params,
                                    unsigned flags, double* E /* n_pairs * n_runs * 9 */, double* nfa /* n_pairs * n_runs */,
                                    long long* inlier_offsets /* n_pairs * n_runs + 1 */, int* inliers, long long capacity, long long* needed,
                                    pvlm_essential_stats* stats_or_null);
pvlm_status pvlm_filter_image_pairs(pvlm_ctx* ctx, int n_frames, const float* const* bearings, const int* rows, int n_pairs, const int* src, const int* tgt,
                                    const long long* match_offsets, const pvlm_match* matches, const pvlm_essential_params* params, unsigned flags,
                                    unsigned char* keep /* n_pairs */, double* R_21 /* n_pairs * 9 */, double* t_21 /* n_pairs * 3 */,
                                    long long* inlier_offsets /* n_pairs + 1 */, int* inlier_idx, double* triangulated /* 3 per inlier */, long long capacity,
                                    long long* needed, pvlm_essential_stats* stats_or_null);

/* ---- K35: VLAD image retrieval (sfm/VLAD.cpp: Kmeans :46-95, ComputeVLADEmbedding :97-154, FindNeighbors :156-183; SfM::InitImagePairs sfm/SfM.cpp:49-168) ---- *
 * The definition (csrc/pvlm_vlad_core.h).  Nearest centre: of the alive centres the one with the smallest (d2, centre index), d2 the fmaf chain of K33, an exact tie
 * to the lower index.  k-means: assign[i] = 0 at the start (part of upstream's "changed" test); the initial centres are copies of the training rows init_rows names
 * (indices into the concatenation of the train frames' rows, in list order; duplicates are allowed); a pass assigns every row, sets `changed` where that differs from
 * assign[i], and recomputes every alive centre; passes repeat while changed and fewer than max_iterations have run; max_iterations == 0 returns the initial rows.
 * Embedding: per row the residual against its nearest alive centre in float, type 2 divides it by its fp64 norm; block[c] += residual in float, rows ascending; per
 * block type 0 sign sqrtf(|v|), type 1 v / norm(block), type 2 sign root5(|v|) (a fifth root by IEEE + * / only: within one float ulp of (float)pow((double)x, 0.2),
 * see the header); then the whole vector is divided by its fp64 norm.  Neighbours: sim(i, j) the fp64 chain of the exact products, k ascending; row i lists the first
 * min(neighbor_size, n) frames in ascending (-sim, index), the frame itself included wherever it lands.
 * [recalled] upstream leaves every summation to OpenCV (cv::BFMatcher, cv::norm, the dot and += of cv::Mat); those orders are not pinned.  The header fixes its own.
 * Deliberate divergences: the mean of a centre is (float)(S / (double)count) with S an fp64 sum in a fixed order (members ascending, runs of 256, run sums ascending;
 * upstream: float Mat arithmetic); a centre without members is DEAD (alive[c] = 0, its row zeros, never a candidate again, its VLAD block zero; upstream: a NaN row
 * that no comparison ever selects, the same outcome); a row equal to its centre contributes nothing to a type 2 vector (upstream: 0/0 turns the whole vector NaN); a
 * zero block stays zero under type 1, a zero vector (a frame without descriptors) stays zero (upstream: NaN).
 * pvlm_vlad_kmeans: codebook (book_size x 128), alive (book_size), optionally assign (one per training row).  stats: queries and fallback_queries summed over the
 *   passes, iterations = passes run, dead_centres, batches = row batches per pass.
 * pvlm_vlad_embed: one vector per frame of the set, kept on the device in a pvlm_vladset (pvlm_vladset_read copies them out).  alive_or_null: NULL = every centre.
 * pvlm_vlad_neighbors: n_frames x min(neighbor_size, n_frames) indices; sim_or_null: the n_frames x n_frames similarities, copied out only on request.
 * PVLM_ERR_ARG: book_size < 1 or above 4096, more centres than training rows, an init_rows entry or a frame index out of range, max_iterations < 0, a value that
 * is not finite in an alive row of the codebook, normalization outside 0..2, neighbor_size < 1, a set or vladset used with another context.
 * flags: PVLM_FLAG_MATCH_EXACT as in K33 (the assignment is K33's search with the packed alive centres as the train side); bit-identical results in both modes.
 * The rows are worked through in batches of whole frames of up to 2^18 rows; the environment variable PVLM_VLAD_BATCH_ROWS (read at every call) lowers that.  It
 * changes no result; the tests use it to cross batch boundaries on small inputs. */
typedef struct pvlm_vladset pvlm_vladset;
typedef struct pvlm_vlad_stats { long long queries, fallback_queries; int iterations, dead_centres, batches; } pvlm_vlad_stats;
pvlm_status pvlm_vlad_kmeans(pvlm_ctx* ctx, const pvlm_descset* set, int n_train, const int* train_frames, int book_size, int max_iterations,
                             const long long* init_rows /* book_size */, unsigned flags, float* codebook /* book_size x 128 */, unsigned char* alive /* book_size */,
                             int* assign_or_null /* one per training row */, pvlm_vlad_stats* stats_or_null);
pvlm_status pvlm_vlad_embed(pvlm_ctx* ctx, const pvlm_descset* set, int book_size, const float* codebook, const unsigned char* alive_or_null,
                            int normalization /* 0, 1, 2 as VLAD.h */, unsigned flags, pvlm_vladset** out, pvlm_vlad_stats* stats_or_null);
pvlm_status pvlm_vladset_read(pvlm_ctx* ctx, const pvlm_vladset* set, float* out /* n_frames x 128 book_size */);
pvlm_status pvlm_vlad_neighbors(pvlm_ctx* ctx, const pvlm_vladset* set, int neighbor_size, int* neighbors /* n_frames x min(neighbor_size, n_frames) */,
                                double* sim_or_null /* n_frames x n_frames */);
void pvlm_vladset_destroy(pvlm_ctx* ctx, pvlm_vladset* set);

/* ---- K36: refinement of the relative poses (SfM::RefineRelativePose sfm/SfM.cpp:482-485, SfMLocalBA util/Optimization.cpp:84-170) ---- *
 * The definition (csrc/pvlm_relpose_core.h): per pair a two-view bundle adjustment.  Camera 1 is the identity and constant; camera 2's (angle-axis, t) starts from
 * R_21, t_21; the pair's triangulated points are free and start where they are; every inlier contributes two blocks, on the keypoint matches[inlier].query of frame
 * src[p] and on the keypoint .train of frame tgt[p], each with its own frame's img_rows / img_cols.  kind: PVLM_BA_PIXEL = PanoramaReprojResidual_Pixel with
 * HuberLoss(4.0) (what upstream calls), PVLM_BA_ANGLE2 = PanoramaReprojResidual_2Angle on eq.ImageToSphere of the keypoint with HuberLoss(4 pi / 180); the loss acts
 * on the block's squared norm; no seam wrap of the residual, zero derivatives at the poles (as K31).  The trust-region policy is the one of the host mirror's
 * ceres_like::Solve with the defaults of Solver::Options and at most max_num_iterations (upstream: 50) iterations; the points are eliminated per point, the reduced
 * system is one 6 x 6.  Every sum over the points has one order, a function of the pair's inlier count alone (a fixed partition over 64 lanes and a fixed tree), so
 * the result of a pair depends neither on the other pairs of the call nor on the batch it falls into, and is bit-reproducible from run to run.
 * Write-back (util/Optimization.cpp:158-168): R_21 from the angle-axis, scale = |t|, t_21 = t / scale, triangulated[i] /= scale, ok[p] = isfinite(final cost).
 * Deliberate divergences: a pair without inliers comes back unchanged with ok = 1, zero steps and termination 6 (upstream: an empty Ceres problem); a pair whose
 * scale is zero or not finite comes back with its input pose and points and ok = 0 (upstream: a division by zero); the rotation goes through the host mirror's own
 * matrix / angle-axis pair, as K31 does.
 * Inputs: exactly what pvlm_filter_image_pairs writes (match_offsets / matches as it reads them; inlier_offsets, inlier_idx, R_21, t_21, triangulated as it writes
 * them) plus the frames' keypoints in pixels (2 floats per keypoint, rows_kp[f] of them) and image sizes.  R_21, t_21, triangulated are read and replaced.
 * summaries: initial and final cost, ACCEPTED and rejected steps (Ceres' own summary counts iteration 0 as a successful step: its number is successful_steps + 1),
 * termination: 0 max_num_iterations reached, 1 function tolerance, 2 gradient tolerance, 3 parameter tolerance, 4 trust region collapsed, 5 initial cost not
 * finite, 6 no inliers.
 * PVLM_ERR_ARG, with no output touched: a frame, match or keypoint index out of range, an inlier index past the pair's matches, a pose, point or keypoint that is
 * not finite, max_num_iterations < 0, PVLM_BA_ANGLE1 (not implemented for this entry).
 * A call works through its pair list in batches of up to 2^14 pairs or 2^21 inliers; the environment variable PVLM_RELPOSE_BATCH_PAIRS (read at every call) lowers
 * the number of pairs per batch.  It changes no result; the tests use it to run several batches on a small list.
 * pvlm_relpose_workgroup_size: the lanes of the workgroup that refines one pair (the partition of the sums; the tests place their sizes around it). */
typedef struct pvlm_relpose_params { pvlm_ba_kind kind; int max_num_iterations /* 50 */; } pvlm_relpose_params;
typedef struct pvlm_relpose_summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; } pvlm_relpose_summary;
pvlm_status pvlm_refine_relative_poses(pvlm_ctx* ctx, int n_frames, const float* const* keypoints /* 2 floats per keypoint, pixels */, const int* rows_kp,
                                       const int* img_rows, const int* img_cols, int n_pairs, const int* src, const int* tgt,
                                       const long long* match_offsets /* n_pairs + 1 */, const pvlm_match* matches, const long long* inlier_offsets /* n_pairs + 1 */,
                                       const int* inlier_idx, double* R_21 /* in/out, n_pairs * 9 */, double* t_21 /* in/out, n_pairs * 3 */,
                                       double* triangulated /* in/out, 3 per inlier */, const pvlm_relpose_params* params, unsigned char* ok /* n_pairs */,
                                       pvlm_relpose_summary* summaries_or_null);
int pvlm_relpose_workgroup_size(void);

/* ---- K42: translation averaging (SfM::EstimateGlobalTranslation sfm/SfM.cpp:1047; TranslationAveragingDLT / L2 / SoftL1 sfm/TranslationAveraging.cpp:31-204) ---- *
 * The definition (csrc/pvlm_transavg_core.h).  Unknowns: the translation t_cw of every camera (origin_idx constant and zero) and one private scale per pair.
 * Pair p: r = t[second] - R_21 t[first] - s_p d_p, d_p = t_21 / |t_21| (base/CostFunction.h:51-83), under SoftLOneLoss(loss_a) on |r|^2 (no loss when loss_a < 0,
 * :184-185); per scale one ScaleFactor block (CostFunction.h:119-144): scales[p] != 1 (as written, :101) gives the bounds upper_scale_ratio * s0 and
 * lower_scale_ratio * s0 and the parameter bounds [0.5 s0, 3 s0]; otherwise ScaleFactor(2, 1) and no parameter bounds.  R_21 is row-major.
 * Per LM iteration the scales are eliminated (a 1 x 1 pivot per pair), the reduced 3 x 3 camera blocks are gathered per camera over a CSR of its incident pairs
 * and the camera system goes through the solver behind pvlm_spd_solve_blocks; the scale steps are back-substituted, the candidate scales CLAMPED onto their
 * parameter bounds and the step quality taken against the model at the clamped step.  The trust-region policy is ceres_like::Solve's (Solver::Options' defaults).
 * Every sum has one order (per camera: its pairs in list order over pvlm_transavg_group_size() lanes and a fixed butterfly; the scalars: a fixed tree over the
 * pairs), so a call is bit-reproducible from run to run — for a pair list that names no camera pair more than twice (the solver adds repeated blocks atomically).
 * Write-back (:160-166): summary->final_cost; weight[i] = (|t2 - R_21 t1 - scales[i] t_21| + 1e-2)^-0.5, t_21 not normalised, as line 165 is written.
 * Deliberate divergences: the functor's `weight` member is never applied upstream and is not applied here (weight is only written); R_21 is used directly instead
 * of through an angle-axis vector (as K36); Ceres' own treatment of parameter bounds (projection plus a line search) is replaced by the clamp without a line search;
 * no pairs: nothing is changed, termination 6; the three 3 F vectors of an iteration (gather, right-hand side, camera step) pass through the host, the per-pair
 * state stays on the device.
 * pvlm_transavg_dlt: the least-squares solution of the stacked t_j - R_ji t_i = t_ji by its normal equations with camera 0 fixed at zero (upstream: SparseQR on a
 * system that is rank-deficient by the gauge t_i = R_i c, so it returns SOME basic solution; every caller runs SetToOrigin afterwards, which cancels the gauge).
 * info: 0, or k > 0 when the system is not positive definite (a pair graph that is not connected); the output is then untouched.
 * summary: initial and final cost, accepted and rejected steps, termination on K36's numbering (6: no pairs).
 * PVLM_ERR_ARG, with no output touched: a NULL, a camera index out of range, first == second, an input that is not finite, t_21 of zero length, origin_idx out of
 * range, translations[origin_idx] not zero (upstream asserts), max_num_iterations < 0.
 * pvlm_transavg_group_size: the lanes that share one camera's gather (the tests place the degrees of a hub camera around it).  The environment variable
 * PVLM_TRANSAVG_MAX_BLOCKS (read at every call) lowers the grid of the per-pair kernels; it changes no result, the tests use it to make them stride.  With
 * PVLM_TRANSAVG_PROFILE set, pvlm_transavg_solve prints one line on stderr: the wall clock of the call split into kernels, camera solves and host. */
typedef struct pvlm_transavg_params { double loss_a /* 0.01 */, upper_scale_ratio, lower_scale_ratio; int max_num_iterations /* 50 */; } pvlm_transavg_params;
typedef struct pvlm_transavg_summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; } pvlm_transavg_summary;
pvlm_status pvlm_transavg_dlt(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21 /* n_pairs * 9 */,
                              const double* t_21 /* n_pairs * 3 */, double* translations_out /* n_cameras * 3 */, int* info);
pvlm_status pvlm_transavg_solve(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, const double* t_21,
                                double* scales /* in/out, n_pairs */, int origin_idx, double* translations /* in/out, 3 per camera */,
                                double* weight /* in/out, n_pairs */, const pvlm_transavg_params* params, pvlm_transavg_summary* summary);
int pvlm_transavg_group_size(void);

/* ---- K44: BATA translation averaging (BATA / LUDRevised / IRLS sfm/BATA.cpp:36-237; the wrapper TranslationAveragingBATA sfm/TranslationAveraging.cpp:483-525) ---- *
 * The definition (csrc/pvlm_bata_core.h).  P pairs (first, second) with unit directions dir and positive start scales; the camera ids must lie in [0, n_cameras).
 * As upstream (:197, :207) the cameras are F = max_id - min_id + 1 with the ids shifted by min_id: F * 3 numbers are written to centres (and lud_centres), the
 * rest of an n_cameras * 3 buffer is left alone.  The pair's difference is d_k = t[first] - t[second]; camera 0 is the gauge and comes back as zero.
 * LUD stage (init_iteration times): weights w_k = 1, then (|r_k|^2 + delta)^-1/2 (the double square root of :75 / :118 as written); min sum w_k |d_k - s_k dir_k|^2
 * subject to sum_k dir_k . d_k = P and sum t = 0; s_k = d_k . dir_k / |dir_k|^2, r_k = d_k - s_k dir_k.  The start: scales0 * P / sum(scales0).
 * IRLS stage (outer_iteration - 1 outers of inner_iteration inners): per outer e_k = |d_k / S_k - dir_k|, Wvec = 1 below robust_threshold, thr / e above, 0 at
 * equality or NaN (:144-146); per inner S_k = |d_k|^2 / (d_k . dir_k), +inf where negative (:156, the row drops out), the Laplacian weight Wvec_k / S_k^2, the
 * right-hand side +-(Wvec_k / S_k) dir_k, camera 0 fixed.  outer_iteration = 1 returns the LUD centres.  scales_out: the S of the last pass.
 * Deliberate divergences.  Upstream factorises the indefinite (3 F + 4) KKT matrix of the LUD stage with SparseLU; here it is two positive definite solves of the
 * grounded weighted Laplacian, x1 = L^-1 (2 A^T B), x2 = L^-1 c with c = At0^T vec(dir), t = x1 - lambda x2, lambda = (c^T x1 - P) / (c^T x2): exact, because c and
 * A^T B are orthogonal to the translations, so the multiplier of sum t = 0 is zero, and upstream moves camera 0 to the origin anyway (:121-123) — the method
 * diverges, not the result.  The system is L (x) I3 and goes through the solver behind pvlm_spd_solve_blocks, re-assembled for every right-hand side.  Upstream's
 * SparseQR on A^T A (:161) is a Cholesky: a system that is not positive definite (a pair graph that is not connected, a camera whose pairs have all dropped) gives
 * info > 0 where upstream returns some basic solution; a scale or solution that is not finite (0 / 0: two cameras on one point) gives info = -1 where upstream
 * carries the NaN on.  Svec.txt, LUD.txt and LUD.pcd are not written.  Which pairs are unscaled (:192-193) and what they draw (:64) is the caller's business.
 * info: 0; k > 0 not positive definite; -1 not finite; -2 no pairs.  Unless info is 0 no output is touched.
 * Every sum has one order (per camera: its pairs in list order over pvlm_bata_group_size() lanes and a fixed butterfly; the scalars: a fixed tree over the pairs),
 * so a call is bit-reproducible from run to run — for a pair list that names no camera pair more than twice (the solver adds repeated blocks atomically).
 * PVLM_ERR_ARG, with no output touched: a NULL (the two optional outputs apart), a camera index out of range, first == second, an input that is not finite, a
 * direction not of unit length within 1e-9, a scale <= 0, init_iteration < 1, inner_iteration < 1, outer_iteration < 1, n_cameras < 2.
 * The environment variable PVLM_BATA_MAX_BLOCKS (read at every call) lowers the grid of the kernels; it changes no result, the tests use it to make them stride.
 * With PVLM_BATA_PROFILE set, a call prints one line on stderr: its wall clock split into kernels, camera solves and host. */
typedef struct pvlm_bata_params { double delta /* 1e-6 */; int init_iteration /* 10 */, inner_iteration /* 10 */, outer_iteration /* 10 */; double robust_threshold /* 0.1 */; } pvlm_bata_params;
pvlm_status pvlm_transavg_bata(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir /* n_pairs * 3, unit */,
                               const double* scales0 /* n_pairs, all > 0 */, const pvlm_bata_params* params, double* centres /* out, F * 3, camera 0 = 0 */,
                               double* lud_centres_or_null, double* scales_out_or_null, int* info);
int pvlm_bata_group_size(void);

/* ---- K40: rotation averaging (SfM::EstimateGlobalRotation sfm/SfM.cpp:811-905; RotationAveragingRefineL1 / RotationAveragingL2 sfm/RotationAveraging.cpp:317-582) ---- *
 * The definition (csrc/pvlm_rotavg_core.h).  F cameras, P pairs (first, second, R_21 row-major), rotations R_cw row-major, 9 per camera.
 * pvlm_rotavg_l1 is RotationAveragingRefineL1 with weight function 1 (:428-582): rotations[start_idx] is the identity and stays it.  Pair error
 * e_p = log(R_2w^T R_21 R_1w) (:476-478).  L1 stage (:460-503): per outer iteration the errors b, then the ADMM of least absolute deviations (rho = 1, alpha = 1,
 * absolute tolerance 1e-4, relative tolerance 1e-2, at most 1000 iterations, stopped by the two-norm tests of the method; not converged is not an error, as upstream
 * ignores Solve's return value); curr_e = |x|, break before the update when last_e < curr_e, R <- R exp(x_r), continue while ++iter < 32 && curr_e > 1e-5 &&
 * (last_e - curr_e) / curr_e > 1e-2.  IRLS stage (:505-580): errors = A x_prev - b, weights = |errors|^-1.5 per row and component, A^T W A x = A^T W b, the same
 * update, curr_e = |x_prev - x|, the same loop condition.  summary: the L1 outer iterations, the ADMM iterations of all of them, the IRLS iterations and info:
 * 0, or k > 0 when an IRLS system was not finite or not positive definite (a pair error of zero gives an infinite weight); the rotations are then those of the last
 * completed iteration (upstream returns false, :553-557).
 * pvlm_rotavg_l2 is RotationAveragingL2 (:317-374): one angle-axis vector per camera, none fixed, r_p = log(R_2w R_1w^T R_21^T) (PairWiseRotationResidual,
 * base/CostFunction.h:17-47) under SoftLOneLoss(loss_a) on |r|^2 (no loss when loss_a < 0), LM with ceres_like::Solve's policy and Solver::Options' defaults, the
 * Jacobi scaling and LM diagonal of K42.  summary: K42's fields and termination numbering (6: no pairs).  The result is unusable only if it is not finite (the
 * rotations are then left as they came).
 * Deliberate divergences.  Upstream carries every pair twice, (i, j, R_21) and (j, i, R_21^T), in the order of a std::map; the mirrored half of every ADMM vector is
 * the negative of the first half, so P rows are carried with the factors 2 and sqrt(2) that follow (A^T A = 2 L (x) I_3, L the Laplacian of the pair graph without
 * start_idx); x, y and z decouple in the L1 stage: (2 L)^-1 is formed ONCE per call as a dense matrix of order F - 1 (pvlm_spd_solve with the identity as right-hand
 * sides) and the x-update of every ADMM iteration is a dense product with three columns, where upstream factorises once and substitutes; the IRLS systems go through
 * the solver behind pvlm_spd_solve_blocks (upstream: SimplicialLDLT); analytic 3 x 3 Jacobians replace the autodiff; R_21 is used directly instead of through an
 * angle-axis vector (as K36 and K42); rotations_after_L1.txt is not written.
 * Every sum has one order (per camera: its pairs in list order over pvlm_rotavg_group_size() lanes and a fixed butterfly; the scalars: a fixed tree over pairs or
 * cameras; the dense product: a row over 64 lanes, lane l the columns l, l + 64, ..., and a fixed butterfly), so a call is bit-reproducible from run to run.
 * PVLM_ERR_ARG, with no output touched: a NULL, a camera index out of range, first == second, the same camera pair named twice in either orientation (upstream's
 * map would collapse it), an input that is not finite, start_idx out of range, rotations[start_idx] not the identity on entry to _l1, a pair graph that is not
 * connected, n_cameras < 1, max_num_iterations < 0.
 * The environment variable PVLM_ROTAVG_MAX_BLOCKS (read at every call) lowers the grids of the kernels; it changes no result, the tests use it to make them stride.
 * With PVLM_ROTAVG_PROFILE set, each call prints one line on stderr: its wall clock split into kernels, solves, the forming of (2 L)^-1 and host. */
typedef struct pvlm_rotavg_l1_summary { int l1_iterations, admm_iterations, irls_iterations, info; } pvlm_rotavg_l1_summary;
typedef struct pvlm_rotavg_l2_params { double loss_a /* 0.07 */; int max_num_iterations /* 50 */; } pvlm_rotavg_l2_params;
typedef struct pvlm_rotavg_l2_summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; } pvlm_rotavg_l2_summary;
pvlm_status pvlm_rotavg_l1(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21 /* n_pairs * 9 */, int start_idx,
                           double* rotations /* in/out, 9 per camera */, pvlm_rotavg_l1_summary* summary);
pvlm_status pvlm_rotavg_l2(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21, double* rotations /* in/out */,
                           const pvlm_rotavg_l2_params* params, pvlm_rotavg_l2_summary* summary);
int pvlm_rotavg_group_size(void);

/* ---- K45: the least-square start of the L2 rotation-averaging method (RotationAveragingLeastSquare sfm/RotationAveraging.cpp:185-275) ---- *
 * The definition (csrc/pvlm_rotstart_core.h).  F cameras, P pairs (first, second, R_21 row-major, either orientation).  M = A^T A of the equations
 * R_2w - R_21 R_1w = 0 has one 3 x 3 block per pair; wanted is the invariant subspace of its three smallest eigenvalues, then per camera the polar factor of its
 * 3 x 3 block, the sign rule det < 0 -> -rot and the product with rot_0^T (camera 0 ends as the identity up to rounding).
 * STATED DIVERGENCE: upstream takes a dense SelfAdjointEigenSolver of the 3 F x 3 F matrix (72 F^2 bytes, 27 F^3 operations); here it is shift-and-invert subspace
 * iteration of width 3 with Rayleigh-Ritz on the block-sparse matrix: sigma = shift_rel * d_max (d_max: the largest camera degree), per iteration three solves with
 * M + sigma I through the solver behind pvlm_spd_solve_blocks, the Cholesky of the 3 x 3 Gram matrix, the 3 x 3 eigen-decomposition of Q^T M Q, until
 * max_k |M x_k - theta_k x_k| <= tol * d_max.  The result depends only on the subspace (the core header says why), so the method differs and the result does not.
 * rotations: on entry the start (9 per camera; the host mirror passes RotationAveragingSpanningTree's result, but any 3 F x 3 matrix of full rank serves), on
 * exit R_cw.  summary: iterations, solves (three per iteration), info, the last residual over d_max, the three Ritz values.  info: 0; k > 0: M + sigma I is not
 * positive definite (an R_21 far from a rotation); -1: something was not finite; -2: max_iterations reached; -3: a camera's block or a Gram matrix (the start's
 * among them) is singular.  Unless info is 0, rotations is left as it came.
 * Every sum has one order (per camera: its pairs in list order over pvlm_rotavg_group_size() lanes and a fixed butterfly; the scalars: a fixed tree over the
 * cameras), so a call is bit-reproducible from run to run.
 * PVLM_ERR_ARG, with no output touched: a NULL, a camera index out of range, first == second, the same camera pair named twice in either orientation, an input that
 * is not finite, a pair graph that is not connected (a null space of six dimensions has no answer), n_cameras < 2 or n_pairs < 1 (upstream returns false),
 * shift_rel <= 0, tol <= 0, max_iterations < 1.
 * PVLM_ROTAVG_MAX_BLOCKS and PVLM_ROTAVG_PROFILE act as for K40. */
typedef struct pvlm_rotavg_lsq_params { double shift_rel /* 1e-9 */, tol /* 1e-12 */; int max_iterations /* 100 */; } pvlm_rotavg_lsq_params;
typedef struct pvlm_rotavg_lsq_summary { int iterations, solves, info; double residual /* last, / d_max */, theta[3]; } pvlm_rotavg_lsq_summary;
pvlm_status pvlm_rotavg_least_square(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21 /* n_pairs * 9 */,
                                     double* rotations /* in: the start, out: R_cw; 9 per camera */, const pvlm_rotavg_lsq_params* params,
                                     pvlm_rotavg_lsq_summary* summary);

/* ---- K46: translation averaging on world-frame directions (TranslationAveragingL2Chordal sfm/TranslationAveraging.cpp:206-274; one solve of
 *      TranslationAveragingLUD's loop :553-626; ChrodalResidual, LUDResidual, ScaleFactor base/CostFunction.h:89-173) ---- *
 * The definition (csrc/pvlm_transdir_core.h).  Unknowns: the CENTRE c of every camera (upstream's t_wc; origin_idx constant and zero); dir[p] is the measured
 * direction of pair p, a unit vector in the world frame (upstream: R_w2 t_21 normalised).  Both run K42's LM on the pair-graph layer (gather, fixed tree, camera
 * system through the solver behind pvlm_spd_solve_blocks) with ceres_like::Solve's policy.
 * pvlm_transavg_chordal: u = c[first] - c[second], r = u / |u| - dir (weight 1) under HuberLoss(loss_a) on |r|^2; max_num_iterations 300, function_tolerance 1e-7,
 * parameter_tolerance 1e-8 upstream (:254-257).  There is no scale and nothing is eliminated.  THE COST IS INVARIANT UNDER c -> lambda c: the overall scale is a gauge
 * that the LM damping alone holds, so the result keeps roughly the scale of its start; compare results after a scale fit.  Two cameras on one point make the cost
 * not finite: at the start that is termination 5 with centres untouched, at a candidate a rejected step.
 * pvlm_transavg_lud: one private scale per pair, e = c[first] - c[second] - s_p dir_p, ONE residual w_p |e|^(1/2), no loss; weight[p] = w_p is READ and applied
 * (the LUD functor reads its weight, unlike K42's).  Scale block by the incoming scale s0: s0 != 1 (as written, :563) gives ScaleFactor(upper_scale_ratio s0,
 * lower_scale_ratio s0) and the parameter bounds [0.5 s0, 3 s0]; otherwise ScaleFactor(2, 1) and a parameter LOWER bound of 1 only (:576-578; K42's unscaled pairs
 * have none).  Per LM iteration the scales are eliminated (a 1 x 1 pivot), the camera system solved, the scale steps back-substituted, the candidate scales CLAMPED
 * onto their parameter bounds and the step quality taken against the model at the clamped step — K42's stand-in for Ceres' projection plus line search, the same
 * divergence.  Write-back (:615-626): weight[p] = (|e_p| + 1e-2)^-1/2, *sum_e = sum |e_p| over the fixed tree, both on dir_p (upstream normalises R_w2 t_21 in the
 * functor and rotates the normalised t_21 in the weight: rounding apart, the same vector).
 * Further divergence: where |e| == 0 at a linearisation point the pair contributes a zero row; upstream's Jet gives a non-finite derivative there and Ceres fails.
 * summary: K42's fields and termination numbering (6: no pairs, nothing touched; 5: initial cost not finite, nothing but the summary touched).
 * Every sum has one order (per camera: its pairs in list order over pvlm_transdir_group_size() lanes and a fixed butterfly; the scalars: a fixed tree), so a call is
 * bit-reproducible from run to run — for a pair list that names no camera pair more than twice (the solver adds repeated blocks atomically).
 * PVLM_ERR_ARG, with no output touched: a NULL, a camera index out of range, first == second, an input that is not finite, a direction not of unit length within
 * 1e-9, for _lud a weight <= 0, origin_idx out of range, centres[origin_idx] not zero, max_num_iterations < 0.
 * The environment variable PVLM_TRANSDIR_MAX_BLOCKS (read at every call) lowers the grids of the kernels; it changes no result, the tests use it to make them stride.
 * With PVLM_TRANSDIR_PROFILE set, a call prints one line on stderr: its wall clock split into kernels, camera solves and host. */
typedef struct pvlm_transdir_chordal_params { double loss_a /* 0.5 */; int max_num_iterations /* 300 */; } pvlm_transdir_chordal_params;
typedef struct pvlm_transdir_lud_params { double upper_scale_ratio, lower_scale_ratio; int max_num_iterations /* 50 */; } pvlm_transdir_lud_params;
typedef struct pvlm_transdir_summary { double initial_cost, final_cost; int successful_steps, unsuccessful_steps, termination; } pvlm_transdir_summary;
pvlm_status pvlm_transavg_chordal(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir /* n_pairs * 3, unit */,
                                  int origin_idx, double* centres /* in/out, 3 per camera */, const pvlm_transdir_chordal_params* params,
                                  pvlm_transdir_summary* summary);
pvlm_status pvlm_transavg_lud(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* dir /* n_pairs * 3, unit */,
                              double* scales /* in/out, n_pairs */, double* weight /* in: w_p, out: the next weights; n_pairs */, int origin_idx,
                              double* centres /* in/out, 3 per camera */, const pvlm_transdir_lud_params* params, double* sum_e, pvlm_transdir_summary* summary);
int pvlm_transdir_group_size(void);

/* ---- K47: TranslationAveragingL1, the triplet minimax programme (sfm/TranslationAveraging.cpp:277-417) ---- *
 * The definition (csrc/pvlm_translp_core.h).  Unknowns: t_cw of every camera, one lambda per TRIPLET, one gamma.  triplet_pairs names, per triplet (i < j < k), the
 * indices of its pairs (i,j), (j,k), (i,k) in the pair list (upstream: PoseGraph::FindTriplet over the pairs).  For each of the three pairs and each component c the
 * rows  e_c - gamma <= 0  and  e_c + gamma >= 0  with e = t[second] - R_21 t[first] - lambda_T t_21: 18 rows per triplet (:328-380).  Bounds: the origin's
 * translation fixed at zero, gamma >= 0 (implied by the row pairs), lambda_T >= lo_T = 0.9 x the mean of |t_21| over the triplet's pairs, t_21 NOT normalised
 * (:381-385; the `first = 1` of :319 is overwritten).  Cost: gamma.  With the bound row -lambda_T <= -lo_T a triplet has 19 rows; `duals`, when given, receives the
 * multiplier z >= 0 of every row, 19 per triplet: row 6 q + 2 c of pair slot q is e_c - gamma <= 0, row 6 q + 2 c + 1 is -e_c - gamma <= 0, row 18 the bound.
 * DELIBERATE DIVERGENCES from upstream:
 *   The method is a primal-dual interior-point iteration (Mehrotra's predictor and corrector on the normal equations, each lambda eliminated by a 1 x 1 pivot, the
 *   gamma column taken as a 1 x 1 border, three camera solves per iteration through the solver behind pvlm_spd_solve_blocks), not Clp's simplex.
 *   The optimum of this programme is a FACE, not a point.  Upstream returns whichever vertex Clp's pivoting reaches; this returns a point near the face's analytic
 *   centre.  At gamma equal to 1e-11, a simplex vertex and an interior-point solution were seen 0.65 to 1.4 m apart on scenes 5 m across, and a rounding-sized
 *   (1e-13 relative) disturbance of the solves moves the interior-point translations by up to 2e-4 m while gamma moves by 1e-13.  So gamma, feasibility and the dual
 *   certificate are the contract; the translation values are not.
 *   Gauge: cameras joined by a triplet form components.  origin_idx pins its own component; every other component has its lowest-numbered camera pinned at zero
 *   (that component's translation is free in upstream's programme too: no optimum changes).  A camera in no triplet stays zero; what Clp leaves in a free column that
 *   no row touches has not been verified.  Both are counted (n_components, n_loose).
 *   The start is t = 0, whatever `translations` holds on entry.
 * Start: lambda = lo + 1, gamma = max |e| + 1, s = h - G x, z = 1 / rows.  Step: 0.99 of the way to the boundary, capped at 1.  Stop when s^T z <= gap_tol
 * max(1, |gamma|), |G x + s - h|_inf <= feas_tol and |c + G^T z|_inf <= feas_tol, or after max_iterations.  The camera systems are Jacobi-scaled with 1e-12 added to
 * the scaled diagonal; a factorisation that fails multiplies that by 100 and is retried, at most three times in a call (bumps).
 * summary: gamma, dual_objective (sum lo_T z_bound: by weak duality a lower bound of the optimum when dual_residual is zero), gap (s^T z), primal_residual,
 * dual_residual, iterations, bumps, n_components, n_loose, termination: 0 converged, 1 iteration limit, 2 factorisation lost after the bumps, 3 not finite, 6 no
 * triplets (nothing touched).  Unless termination is 0 or 1, no output but the summary is touched.
 * Every sum has one order (per camera and per pair: its (triplet, slot) entries in triplet order over pvlm_translp_group_size() lanes and a fixed butterfly; the
 * scalars: a fixed tree), so a call is bit-reproducible from run to run.
 * PVLM_ERR_ARG, with no output touched: a NULL (duals apart), an index out of range, first >= second, a repeated pair, a triplet whose three pairs do not form
 * (i,j), (j,k), (i,k) with i < j < k, an input that is not finite, translations[origin_idx] not zero, max_iterations < 1, a tolerance <= 0.
 * The environment variable PVLM_TRANSLP_MAX_BLOCKS (read at every call) lowers the grids of the kernels; it changes no result, the tests use it to make them stride.
 * With PVLM_TRANSLP_PROFILE set, a call prints one line on stderr: its wall clock split into kernels, camera solves and host. */
typedef struct pvlm_translp_params { int max_iterations /* 60 */; double gap_tol /* 1e-9 */, feas_tol /* 1e-9 */; } pvlm_translp_params;
typedef struct pvlm_translp_summary { double gamma, dual_objective, gap, primal_residual, dual_residual; int iterations, bumps, n_components, n_loose, termination; } pvlm_translp_summary;
pvlm_status pvlm_transavg_l1(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21 /* n_pairs * 9, row-major */,
                             const double* t_21 /* n_pairs * 3 */, int n_triplets, const int* triplet_pairs /* n_triplets * 3: indices of (i,j), (j,k), (i,k) */,
                             int origin_idx, double* translations /* in/out, 3 per camera */, double* duals /* out, optional: 19 per triplet */,
                             const pvlm_translp_params* params, pvlm_translp_summary* summary);
int pvlm_translp_group_size(void);

/* ---- K48: the triplets of the pair graph (PoseGraph::FindTriplet, sfm/PoseGraph.cpp:195-226) and SfM::FilterByTriplet's test (sfm/SfM.cpp:705-778) ---- *
 * The definition (csrc/pvlm_triplet_core.h).  n_pairs pairs (first, second) with first < second < n_cameras, no pair named twice, in any list order.  The rank of a
 * pair is its position in ascending order of first * n_cameras + second.  The triplets are all (i, j, k), i < j < k, whose three pairs are in the list, in
 * lexicographic order: under these conditions exactly the order of upstream's walk over its std::set of edges.
 * pvlm_triplets_find: `triplets` receives i, j, k per triplet and `triplet_pairs` the caller's list indices of (i,j), (j,k), (i,k) — the layout pvlm_transavg_l1
 *   takes; either may be NULL (not wanted).  *needed = the number of triplets, always set (64-bit: an exhaustive graph of 454 cameras has 15.5 M).  When an output is
 *   wanted and *needed exceeds capacity (in triplets) the call returns PVLM_ERR_CAPACITY with *needed and pair_counts set and no triplet at or past capacity written
 *   (the convention of pvlm_match_pairs); with neither output wanted capacity is not looked at.  pair_counts, when given, receives per pair of the caller's list the
 *   number of triplets whose smallest pair (i, j) it is; their sum is *needed and, taken in rank order, their running sum is a triplet's position.
 * pvlm_triplets_filter: the loop measure of a triplet is upstream's as written, c = trace((R_31^T R_32) R_21) / 3 clamped by min(1.0, max(c, -1.0)); a triplet is
 *   kept when acos(c) * 180 / M_PI < angle_threshold_deg, and keep[p] = 1 when pair p lies in at least one kept triplet, else 0.  The device decides clamp(c) > cut with
 *   cut = cos(angle_threshold_deg * pi / 180) wherever |clamp(c) - cut| > 1e-12; the triplets inside that band (n_uncertain of them) are decided on the host by the
 *   literal acos chain, so keep is the literal test's result.  A c that is not finite goes where the written clamp sends it (NaN to 1.0: kept, as upstream keeps it);
 *   R_21 is therefore not required to be finite.  A threshold <= 0 keeps nothing, one above 180 everything.
 * PVLM_ERR_ARG, with no output touched: a NULL (the outputs marked optional apart; with n_pairs == 0 only needed / stats are required), a negative size or capacity, a
 * camera index out of range, first >= second, a pair named twice, a threshold that is not finite.  n_pairs == 0 is PVLM_OK with zero triplets.
 * Rank and rows are made on the host in the call's set-up (one sort of n_pairs keys).  The environment variable PVLM_TRIPLET_MAX_BLOCKS (read at every call) lowers
 * the grids of the kernels and PVLM_TRIPLET_UNCERTAIN_CAP the first capacity of the uncertain list (4096; an overflow runs the pass once more with the reported
 * count); neither changes a result, the tests use them.  With PVLM_TRIPLET_PROFILE set, a call prints one line on stderr: its wall clock split into rank / rows,
 * upload, count, scan, emit and copy-out (find) or filter pass and copy-out (filter), each stage then ending in a wait.  Synchronous; PVLM_ERR_STATE inside a capture. */
typedef struct pvlm_triplet_stats { long long n_triplets, n_kept_triplets, n_uncertain, n_kept_pairs; } pvlm_triplet_stats;
pvlm_status pvlm_triplets_find(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, int* triplets /* 3 per triplet, NULL: not wanted */,
                               int* triplet_pairs /* 3 per triplet, NULL: not wanted */, long long capacity, long long* needed,
                               long long* pair_counts /* n_pairs, optional: triplets whose smallest pair this is */);
pvlm_status pvlm_triplets_filter(pvlm_ctx* ctx, int n_cameras, int n_pairs, const int* first, const int* second, const double* R_21 /* n_pairs * 9, row-major */,
                                 double angle_threshold_deg, unsigned char* keep /* n_pairs */, pvlm_triplet_stats* stats);
int pvlm_triplet_group_size(void);

/* ---- K49: MVS::SelectNeighborSFM (mvs/MVS.cpp:248-332): the neighbour views of every reference view from the tracks the views share ---- *
 * The definition (csrc/pvlm_neighbor_sfm_core.h).  F views with poses T_wc (3 x 4, row-major, the camera centre in the fourth column), T tracks in CSR form
 * (track_offsets[T + 1] from 0, view_ids ascending inside a track — a view may occur twice —, points 3 per track).  For every track in order and every i < j of its
 * views, in double: V = X - C, depth = |V|, angle = VectorAngle3D(V1, V2) * 180 / M_PI, a = min(powf(float(angle / 10.0), 1.5f), 1.f) (a float), s12 = f(depth1 /
 * depth2), s21 = f(depth2 / depth1) with f(s) = 1.6 * 1.6 / s / s above 1.6, 1 from 1 on, s * s below; score(id1, id2) += s12 * a and score(id2, id1) += s21 * a into
 * a FLOAT matrix, every += being float(double(cell) + product), the additions of a cell in track order.  Per row the columns with score > 0 are walked by
 * std::greater<pair<float, size_t>> (score descending, equal scores by column DESCENDING) until neighbor_size are accepted; a candidate is accepted when
 * ||t_nr|| > sq_distance_threshold, T_nr = T_wn^-1 T_wr.  Upstream compares the norm, not its square, with the squared threshold (:322): kept literally.  T_nr is
 * the rigid inverse in double, stored as float (as SelectNeighborKNN of the host mirror).  A view may be its own neighbour when a track names it twice, as upstream.
 * Outputs: n_neighbors[F]; ids / scores [F * neighbor_size], R_nr [.. * 9, row-major], t_nr [.. * 3]; the slots a row does not fill hold id -1 and zeros.
 * The score matrix stays on the device.  The device's acos / powf need not equal the host library's to the bit; a score differs from the literal host loop's by at
 * most (n + 2) * 2^-23 * score, n the cell's contribution count.  A row in which two candidates adjacent in the walk (the first one behind the walk included) are
 * closer than the sum of their bounds, or a tested ||t_nr|| lies within 1e-12 (relative) of the threshold, is recomputed on the host by the literal loop for that row:
 * stats->n_uncertain counts them.  n_candidates: cells with score > 0; n_contributions: additions (two per (i, j)); n_repeat_tracks: tracks naming a view twice.
 * Deliberate divergence: a track naming a view >= F or one with pose_valid == 0 is refused (upstream would read a sentinel pose and produce NaNs).
 * PVLM_ERR_ARG, with no output touched: a NULL, a negative size, offsets that do not start at 0 or ascend, views of a track that do not ascend, such a track, a NaN
 * threshold.  PVLM_NEIGHBOR_TILE (read at every call) lowers the column tile of the accumulation (pvlm_neighbor_sfm_tile_cols()); it changes no result, the tests use
 * it.  With PVLM_NEIGHBOR_PROFILE set a call prints its wall clock split into index, upload, accumulation, selection, copy-out and host rows on stderr, each stage
 * then ending in a wait.  Synchronous; PVLM_ERR_STATE inside a capture.
 * pvlm_mvs_neighbor_sfm_score_row: one row of the device's score matrix (and the contribution counts, optional) for the tests. */
typedef struct pvlm_neighbor_sfm_stats { long long n_candidates, n_contributions, n_repeat_tracks, n_uncertain; } pvlm_neighbor_sfm_stats;
pvlm_status pvlm_mvs_select_neighbors_sfm(pvlm_ctx* ctx, int n_views, const double* T_wc_3x4, const unsigned char* pose_valid, int n_tracks, const int64_t* track_offsets,
                                          const int* view_ids, const double* points /* n_tracks x 3 */, int neighbor_size, double sq_distance_threshold,
                                          int* n_neighbors /* n_views */, int* ids, float* R_nr, float* t_nr, float* scores, pvlm_neighbor_sfm_stats* stats);
pvlm_status pvlm_mvs_neighbor_sfm_score_row(pvlm_ctx* ctx, int n_views, const double* T_wc_3x4, const unsigned char* pose_valid, int n_tracks, const int64_t* track_offsets,
                                            const int* view_ids, const double* points, int row, float* scores /* n_views */, int* counts /* n_views, optional */);
int pvlm_neighbor_sfm_tile_cols(void);

/* ---- dense SPD solve for an LM driver (not hot path) ------------------------------------------------------------ *
 * Blocked fp64 Cholesky + triangular solves on the GPU (hand-written: 32-wide block columns, 64 x 64 register-tiled
 * trailing updates).  Solves A X = B for a symmetric positive definite n x n matrix (dense, host, full symmetric storage)
 * and B = n x nrhs (column-major, host, overwritten by X).  *info = 0 on success, k > 0 when the leading minor of order k
 * is not positive definite (X is then undefined).  Upstream this step is inside ceres::Solve (SPARSE_SCHUR,
 * util/Optimization.cpp:608-666); the host mirror's stand-in LM driver uses it once the reduced pose system is too large
 * for a host factorisation (a Room-sized joint problem has 5442 unknowns). */
pvlm_status pvlm_spd_solve(pvlm_ctx* ctx, int n, int nrhs, const double* A, double* B, int* info);
/* Block-sparse input: M = D (sum of the 6x6 blocks) D + diag(diag_add), D = diag(scale), assembled on the device, then
 * M x = rhs solved in place (rhs host, n doubles).  blocks: n_blocks x 36 row-major; row_idx / col_idx: n_blocks x 6
 * scalar indices of the block's rows / columns (-1 = constant parameter, dropped).  mirror[b] != 0 (block between two
 * different poses) also adds the transposed block to the other triangle; a block of a pose with itself is given in full
 * with mirror = 0.  Repeated blocks add up.  A block between two DIFFERENT poses must be given with mirror != 0 (or in both
 * triangles): from 1500 unknowns on the unknowns are reordered before the factorisation, which reads one triangle of the
 * REORDERED matrix — a block given in one triangle only may land in the other one.  *info = 0 on success; k > 0 = the leading
 * minor of order k of the matrix AS FACTORISED (reordered when pvlm_spd_last_plan reports a tile-sparse plan) is not positive
 * definite: take it as "not positive definite", not as the index of an unknown. */
pvlm_status pvlm_spd_solve_blocks(pvlm_ctx* ctx, int n, int n_blocks, const int* row_idx, const int* col_idx, const int* mirror, const double* blocks,
                                  const double* scale, const double* diag_add, double* rhs, int* info);
/* Makes the plan of a structure AHEAD of the solve that needs it: the host half (ordering, symbolic factorisation, schedule lists: ~10 ms for a Floor-sized
 * pose graph) starts on a thread of its own and the call returns at once; the lists are copied.  The next pvlm_spd_solve_blocks whose n / row_idx / col_idx /
 * mirror are EXACTLY these takes the plan (waiting for the thread if it is still at work); with any other structure the prefetch is dropped and the plan is made
 * inside the solve as without this call — a hint, never a change of result.  The host mirror's LM driver calls it on entry to a Solve, so that the plan is made
 * beside the upload of the residual sets and the first linearisation (upstream: inside ceres::Solve's preprocessing, util/Optimization.cpp:638-666).
 * pvlm_spd_plan_prefetch_hits: how many solves of this context took a prefetched plan. */
pvlm_status pvlm_spd_plan_prefetch(pvlm_ctx* ctx, int n, int n_blocks, const int* row_idx, const int* col_idx, const int* mirror);
pvlm_status pvlm_spd_plan_prefetch_hits(const pvlm_ctx* ctx, long long* hits);
/* How the last pvlm_spd_solve_blocks structure of this context is factorised: *tile_sparse = 1 when the dense kernels skip the
 * structurally zero 64-row tiles (ordering of the pose graph by minimum degree + elimination-tree postorder; the reference selects
 * SPARSE_SCHUR for 50 < lidars <= 2000, util/Optimization.cpp:641-658), *update_fraction = its tile updates / those of the dense
 * factorisation.  Systems under 1500 unknowns, or whose fraction exceeds 0.6, keep the natural order and the dense kernels. */
pvlm_status pvlm_spd_plan_info(const pvlm_ctx* ctx, int* tile_sparse, double* update_fraction);
/* The schedule of that factorisation.  From 1500 unknowns on the pose graph is ordered by NESTED DISSECTION (recursive bisection by breadth-first level sets; the
 * halves first, the separator last; every group aligned to a 64-row tile by identity rows) and the block columns are factorised LEVEL by level: the columns of a level
 * do not depend on each other — one launch factorises them all, one launch applies their trailing updates (a workgroup per target tile, sources added in list order:
 * bit-reproducible), the triangular solves run level by level too.  *levels = dependent steps (0: the column-by-column factorisation is in use — small systems,
 * PVLM_SPD_LEVELS=0, or a graph whose schedule is not shorter than two thirds of its block columns), *block_columns = block columns of the (padded) system,
 * *padded_rows = its rows.  The reference leaves this to Ceres' SPARSE_SCHUR (util/Optimization.cpp:638-666).  Any pointer may be NULL. */
pvlm_status pvlm_spd_plan_schedule(const pvlm_ctx* ctx, int* levels, int* block_columns, int* padded_rows);
/* The dense TAIL of that schedule.  The last group of the dissection (the top separator) is dense once everything below it is eliminated and every one of its block
 * columns is a level of its own; from eight such columns on they are factorised by ONE launch instead (a tile Cholesky in 64 x 64 tiles whose workgroups hand the
 * finished tiles to each other inside the launch; forward substitution inside it, backward substitution in a second launch).  *tail_block_columns = the block columns
 * done that way (0: none — PVLM_SPD_TAIL=0, no level schedule, or a short separator), *launched_levels = the levels that still run launch by launch.  With the
 * one-launch form of the whole factorisation (pvlm_spd_one_launch, the default) EVERY block column is done inside one launch: *tail_block_columns = all of them,
 * *launched_levels = 0.  Bit-reproducible like the levels; last-bit differences against PVLM_SPD_TAIL=0 (another order of the same sums).  Any pointer may be NULL. */
pvlm_status pvlm_spd_plan_tail(const pvlm_ctx* ctx, int* tail_block_columns, int* launched_levels);
/* ONE LAUNCH for the whole tile-sparse factorisation (the default with a level schedule): every 64 x 64 tile of the factor is a task (its sources = the earlier tile
 * columns that hold both tiles; the sources of a tile that exist two levels ahead of it are split off into chunk tasks that subtract them from the tile in memory as
 * soon as they exist), tasks are ordered by dependency depth, workgroups take them by a ticket and hand finished tiles to each other inside the launch (payload stored
 * write-through, one flag per task); the forward substitution rides along and the backward substitution is a second launch over the tile columns.  Floor system: 278
 * dependent launches -> 2, 6.9 -> 3.2 ms per solve.  pvlm_spd_plan_tail then reports every block column as done inside one launch (launched_levels 0).
 * The workgroups of such a launch WAIT for each other, which presumes that the launch gets the GPU's workgroup slots: processes that share one GPU should switch it off
 * (enable = 0: level launches + the dense tail; enable < 0: no change, query only).  A solve whose launch does not get through within 2 s is redone with the level
 * launches by itself, the context keeps them from then on, and *fallbacks (may be NULL) counts such solves.  Both forms are bit-reproducible; they differ from each
 * other in the last bits (another order of the same sums) — ranks that must agree bit for bit use the same form.
 * Test hook: enable = 2 + k makes task k of the one launch withhold its tile (what a launch that does not get through looks like): the next solve runs into the limit
 * and exercises the recovery; tests/test_linalg_gpu.py. */
pvlm_status pvlm_spd_one_launch(pvlm_ctx* ctx, int enable, long long* fallbacks);

/* ---- multi-GPU exchange (RCCL over xGMI) -------------------------------------------------------- *
 * The reference is single-process (OpenMP only); sharding scan pairs across GPUs introduces exactly one
 * exchange: all-reduce(sum) of the packed normal-equation buffer per LM iteration.
 * One process per GPU.  Rank 0 obtains a 128-byte id (pvlm_comm_unique_id), the host's launcher carries
 * it to the other ranks, every rank calls pvlm_comm_create (collective).  The all-reduce is enqueued on
 * the ctx stream, in place, on a device buffer of `count` doubles (e.g. the d_packed of
 * pvlm_neq_accumulate_dev).  RCCL is loaded lazily on the first pvlm_comm_* call. */
typedef struct pvlm_comm pvlm_comm;
pvlm_status pvlm_comm_unique_id(pvlm_ctx* ctx, unsigned char id_out[128]);
pvlm_status pvlm_comm_create(pvlm_ctx* ctx, int world_size, int rank, const unsigned char id[128], pvlm_comm** out);
pvlm_status pvlm_comm_destroy(pvlm_ctx* ctx, pvlm_comm* comm);
pvlm_status pvlm_allreduce_sum_f64(pvlm_ctx* ctx, pvlm_comm* comm, double* d_buf, int64_t count);
/* Same on a HOST buffer (staged through the context's device buffer, synchronous): for hosts whose LM driver keeps the
 * summed system in host memory, like the mirrored one (panovlm_amd/host: Exchange / MakeRcclExchange). */
pvlm_status pvlm_allreduce_sum_f64_host(pvlm_ctx* ctx, pvlm_comm* comm, double* buf, int64_t count);

/* ---- scans and LiDAR<->LiDAR association -------------------------------------------------------- *
 * Input contract = the public members of sensors/Velodyne.h:80-91 during association: feature
 * clouds in the WORLD frame as float32 (the float buffers pcl::transformPointCloud left behind,
 * sensors/Velodyne.cpp:1773-1808), class tag = PointXYZI::intensity, pose (R_wl, t_wl) double. */
typedef struct {
  int id;                     /* Velodyne::id — index into the pose table                         */
  const double* R_wl;         /* 9, row-major                                                     */
  const double* t_wl;         /* 3                                                                */
  int n_surf_flat;            const float* surf_flat_xyz;      const float* surf_flat_tag;       /* queries  (xyz interleaved) */
  int n_surf_less_flat;       const float* surf_less_flat_xyz; const float* surf_less_flat_tag;  /* targets                     */
  int n_corner;               const float* corner_xyz;         /* cornerLessSharp                 */
  const int* p2s_offsets;     const int* p2s_ids;              /* point_to_segment as CSR (n_corner+1) */
  int n_segments;             const int* segment_size;         /* edge_segmented[s].size()        */
  const double* segment_coeffs; /* 6 per segment, LiDAR-local (point, unit direction)             */
  const double* end_points;     /* 2x3 per segment, LiDAR-local                                   */
  const float* seg_points_xyz;  /* optional: the points of edge_segmented[0], [1], ... one after the other (sum of
                                   segment_size x 3 floats, WORLD frame like the clouds) — needed by pvlm_line2line_residuals */
  int point_stride_floats;      /* distance in floats between consecutive points of surf_flat_xyz / surf_less_flat_xyz / corner_xyz AND between
                                   consecutive entries of the two tag arrays.  0 (or 3 for the xyz arrays): packed, as documented above.  4: the arrays point
                                   INTO pcl::PointXYZI-style records {x, y, z, intensity} (xyz = &cloud[0].x, tag = &cloud[0].intensity): the upload gathers them
                                   itself and the caller flattens nothing.  seg_points_xyz is always packed.                                                  */
} pvlm_scan_desc;

pvlm_status pvlm_scan_upload(pvlm_ctx* ctx, const pvlm_scan_desc* desc, pvlm_scan** out);
/* The same for `n_scans` scans at once (descs[k] -> out[k]; all or nothing): one staging copy, one device allocation
 * shared by the batch (released when the last of its scans is destroyed) and one set of grid-build launches — what the
 * loop over lidars of AddLidarPointToPlaneResidual / AddLidarLineToLineResidual2 (util/Optimization.cpp:521, :345) needs
 * at every outer iteration of LidarOdometry::EstimatePose, when all 454 re-posed Room scans change at once
 * (lidar_mapping/LidarOdometry.cpp:150-170).  pvlm_scan_upload is the n_scans = 1 case. */
pvlm_status pvlm_scan_upload_batch(pvlm_ctx* ctx, int n_scans, const pvlm_scan_desc* descs, pvlm_scan** out);
pvlm_status pvlm_scan_destroy(pvlm_ctx* ctx, pvlm_scan* scan);

/* Velodyne::Transform2LidarWorld / Velodyne::Transform2Local (sensors/Velodyne.cpp:1773-1808, :1810-1848) on the RESIDENT clouds of n_scans
 * scans, as LidarOdometry::RefinePose calls them around every solve (lidar_mapping/LidarOdometry.cpp:17-21, :100-110): scan k's float clouds
 * (surfFlat, surfLessFlat, cornerLessSharp and the segments' points) are replaced IN PLACE by T_k applied the way
 * pcl::transformPointCloud(cloud, cloud, Eigen::Matrix4d) applies it — per coordinate float(((m0 x + m1 y) + m2 z) + m3), the float point promoted
 * to double — so the device's clouds equal the host's after any number of World <-> Local round trips, bit for bit, and nothing is uploaded again.
 * T_rowmajor12: n_scans x 12 doubles, the upper 3 x 4 of T_k row-major ([R | t]; T_wl = [R_wl | t_wl] for Transform2LidarWorld,
 * [R_wl^T | -R_wl^T t_wl] for Transform2Local).  rebuild_grids != 0: the voxel grids of the transformed clouds are rebuilt — bounding boxes
 * reduced on the device, the same plan and tables an upload of the same floats gets; rebuild_grids == 0 leaves them stale (a scan on its way
 * to the local frame is not searched): pvlm_knn / pvlm_assoc_point2plane on such a scan return PVLM_ERR_STATE until a call with
 * rebuild_grids != 0.  The pose of a scan (R_wl, t_wl of its descriptor) is NOT touched: pvlm_scan_set_pose.  A scan may be listed once.
 * On an error after the launch (a coordinate left the float range: PVLM_ERR_ARG) the clouds stay transformed and the grids stale: destroy
 * the scans. */
pvlm_status pvlm_scan_transform_batch(pvlm_ctx* ctx, int n_scans, pvlm_scan* const* scans, const double* T_rowmajor12, int rebuild_grids);
/* Velodyne::SetRotation / SetTranslation (sensors/Velodyne.h:213-233) for a resident scan: replaces the pose the association and the line
 * kernels read (R_wl 9 row-major, t_wl 3).  Host-side state only; the clouds are not moved. */
pvlm_status pvlm_scan_set_pose(pvlm_ctx* ctx, pvlm_scan* scan, const double* R_wl, const double* t_wl);
/* Tests / visualisation: the resident arrays of one cloud of a scan.  which: 0 surfFlat, 1 surfLessFlat, 2 cornerLessSharp, 3 the segments'
 * points.  pvlm_scan_cloud_info: the cloud's size and (clouds 1, 2) the parameters of its voxel grid; pvlm_scan_cloud_fetch: xyz (n x 3), and of
 * the grid cell_count / cell_start (table_size ints each), keys (table_size 64-bit words; hashed tables only) and the cell-sorted points
 * (n x 4 floats: x, y, z, original index as int bits; the order INSIDE a cell is not deterministic).  NULL = skip. */
typedef struct pvlm_grid_info {
  int n;                       /* points                                                                   */
  int has_grid, stale;         /* clouds 1, 2 with n > 0; stale: transformed without rebuild              */
  int dense, nx, ny, nz, xf;   /* dense table: (iz ny + iy) nx + ix, cells xf times finer along x          */
  int table_size;              /* dense: cells + 1; hashed: slots (power of two)                           */
  float cell, origin[3];
} pvlm_grid_info;
pvlm_status pvlm_scan_cloud_info(const pvlm_scan* scan, int which, pvlm_grid_info* info);
pvlm_status pvlm_scan_cloud_fetch(pvlm_ctx* ctx, const pvlm_scan* scan, int which, float* xyz, int* cell_count, int* cell_start,
                                  unsigned long long* keys, float* sorted_xyzi);

/* Exact k-nearest-neighbour search of `queries` (nq x 3 float, world frame) in the scan's
 * surfLessFlat cloud (which=0) or cornerLessSharp cloud (which=1): what
 * pcl::KdTreeFLANN<PointXYZI>::nearestKSearch returns at LidarFeatureAssociate.cpp:575 / :496 —
 * float32 squared distances accumulated as ((dx*dx)+dy*dy)+dz*dz, ascending, ties by index.
 * Neighbours farther than `max_dist` are not searched: rows with fewer than k neighbours within
 * max_dist get idx = -1 / sqd = +inf in the missing slots.  k <= 16. */
pvlm_status pvlm_knn(pvlm_ctx* ctx, const pvlm_scan* scan, int which, const float* queries, int nq, int k,
                     float max_dist, int32_t* idx, float* sqd);

/* The searches of FindNeighbors (lidar_mapping/LidarFeatureAssociate.cpp:19-111) for ALL scans at once.  Upstream builds a pcl::KdTreeFLANN over the scan centres
 * (float32 PointXYZI) and asks, per scan, for nearestKSearch(neighbor_size) and radiusSearch(20 m) — both return ascending L2_Simple distances, ties in index order.
 * Here: row i of the result = the positions j of all centres ordered by the 64-bit key (bits of the float32 squared distance ((dx*dx)+dy*dy)+dz*dz from centre i)
 * << 32 | j, ascending — the first k entries of a row are the k nearest (the scan itself first), the entries whose distance lies below a squared radius are the radius
 * search (the caller recomputes the distance of an entry it looks at: three multiply-adds).  One workgroup per row (distances + a bitonic sort in LDS).
 * xyz: n x 3 floats (host); order: n x n positions (uint16, host, the caller's).  n <= 4096 (PVLM_ERR_CAPACITY beyond: the caller keeps its own search).  The set
 * logic of FindNeighbors (loop closures, temporal neighbours) stays with the caller: it walks sorted rows. */
pvlm_status pvlm_centre_orders(pvlm_ctx* ctx, int n, const float* xyz, uint16_t* order);

/* AssociatePoint2Plane(ref, nei, plane_tolerance, dist_threshold) of
 * lidar_mapping/LidarFeatureAssociate.cpp:550-630 for a BATCH of ordered scan pairs
 * (ref[p], nei[p]); the result is the residual set util/Optimization.cpp:506-562
 * (AddLidarPointToPlaneResidual) would have added for those pairs, in the same order:
 * segment p holds the accepted correspondences of pair p in query order.
 * kind = PVLM_POINT2PLANE_ANGLE or _METER (config.angle_residual), flags/weight as for upload. */
pvlm_status pvlm_assoc_point2plane(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei,
                                   double plane_tolerance, float dist_threshold, pvlm_functor kind, unsigned flags,
                                   double weight, pvlm_resset** out);
/* The plane of a correspondence (lidar_mapping/LidarFeatureAssociate.cpp:592-602: FormPlane, base/Geometry.hpp:345-373 — Eigen's column-pivoted
 * Householder QR of the 10 x 3 system A n = -1) is computed in one of two ways:
 *   default                      normal equations + an a-posteriori bound on the distance to the QR's solution (csrc/pvlm_assoc_core.h:
 *                                form_plane_fast).  The reference's accept / reject decision is taken from it only when it holds for every solution
 *                                inside the bound; otherwise — the largest point distance within ~1e-6 of plane_tolerance, an ill-conditioned
 *                                neighbourhood — the QR runs for that query.  Same correspondences, same order; the stored plane is within 5e-7
 *                                relative of the QR's by construction (1e-11 typically; the bar of the path is 1e-6).
 *   PVLM_FLAG_ASSOC_EXACT_FIT    the QR for every query, operation by operation, unfused: records bit-identical to an x86-64 build of the
 *                                reference (what the parity tests pin).  About 1.6 x the time of the plane-fit kernel.
 * pvlm_assoc_point2plane_stats: how many queries of the set took the QR because the fast fit refused (0 in exact mode). */
#define PVLM_FLAG_ASSOC_EXACT_FIT 0x200u
pvlm_status pvlm_assoc_point2plane_stats(const pvlm_resset* rs, int64_t* exact_fits);
/* The same + how the call was run: its batches (column blocks) and how many of them ran the exact plane-fit kernel.  In the default mode the first batch is a
 * probe of about a million queries (PVLM_ASSOC_PROBE_ROWS): when the fast fit refuses more than 2 % of its queries — neighbourhoods the normal equations cannot
 * handle, e.g. raw scans as targets — the other batches run the QR kernel directly, which is then the faster one.  Decided from the data alone. */
pvlm_status pvlm_assoc_point2plane_stats2(const pvlm_resset* rs, int64_t* exact_fits, int* batches, int* exact_kernel_batches);
/* Optional debug readback of the last pvlm_assoc_point2plane call: query index and the 10
 * neighbour indices of every accepted correspondence (n x 1, n x 10). */
pvlm_status pvlm_assoc_point2plane_debug(pvlm_ctx* ctx, const pvlm_resset* rs, int32_t* query_idx, int32_t* nn_idx);

/* Vote matrix of AssociateLine2Line (lidar_mapping/LidarFeatureAssociate.cpp:457-473):
 * votes[nei_seg][ref_seg] = number of nei cornerLessSharp points of that nei segment whose
 * PointToLineDistance3D to the ref segment's world line is <= dist_threshold.
 * votes is n_nei_segments x n_ref_segments, row-major, int32. */
pvlm_status pvlm_line2line_votes(pvlm_ctx* ctx, const pvlm_scan* ref, const pvlm_scan* nei, float dist_threshold,
                                 int32_t* votes);

/* Batched form — every (ref, nei) pair of an outer iteration in ONE launch and one copy back (the reference
 * calls AssociateLine2Line twice per pair per outer iteration: LidarLineMatch.cpp:68, util/Optimization.cpp:379).
 * The vote block of pair p starts at votes + vote_offsets[p] (n_nei_segments(p) x n_ref_segments(p), row-major);
 * vote_offsets (n_pairs + 1) is an output.  votes == NULL only fills vote_offsets (sizing call);
 * PVLM_ERR_CAPACITY if capacity (int32 elements) < vote_offsets[n_pairs]. */
pvlm_status pvlm_line2line_votes_batch(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei,
                                       float dist_threshold, int64_t* vote_offsets, int32_t* votes, int64_t capacity);

/* The batched votes reduced on the device to what FindAssociations (LidarFeatureAssociate.cpp:126-133) reads first: per neighbour segment (row of the
 * pair's n_nei_segments x n_ref_segments block) the reference segment with the most votes — the first of equals — and that count.  Rows of pair p:
 * [row_offsets[p], row_offsets[p + 1]) (a pair whose reference scan has no segment has none); n_pairs + 1 offsets.  best_col / best_count null =
 * sizing call; PVLM_ERR_CAPACITY if capacity (entries) < row_offsets[n_pairs]. */
pvlm_status pvlm_line2line_best_batch(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, float dist_threshold,
                                      int64_t* row_offsets, int32_t* best_col, int32_t* best_count, int64_t capacity);

/* Residual blocks of the line-to-line term, built on the device (the body of the innermost loops of
 * AddLidarLineToLineResidual2, util/Optimization.cpp:404-434): match m says that segment match_nei_seg[m] of scan
 * nei[match_pair[m]] was associated with segment match_ref_seg[m] of scan ref[match_pair[m]] (AssociateLine2Line +
 * the line-track filter, decided by the caller).  Every point of the neighbour segment becomes one Point2Line block
 *   [ World2Local_nei(point) | ref_local_point + 0.1 dir | ref_local_point - 0.1 dir ]      (Optimization.cpp:410-434)
 * on the parameter blocks (ref, nei), in match order and, inside a match, in the order of edge_segmented[seg] — the
 * order the reference's AddResidualBlock calls have.  Matches must be sorted by pair; consecutive matches of one pair form
 * one segment of the result.  kind = PVLM_POINT2LINE_ANGLE / _METER.  Both scans must have been uploaded with
 * seg_points_xyz.  Upstream this loop costs one heap-allocated AutoDiffCostFunction per POINT (600 k per outer iteration
 * at Room scale); here the rows never exist on the host. */
pvlm_status pvlm_line2line_residuals(pvlm_ctx* ctx, int n_pairs, pvlm_scan* const* ref, pvlm_scan* const* nei, int n_matches,
                                     const int* match_pair, const int* match_nei_seg, const int* match_ref_seg, pvlm_functor kind,
                                     unsigned flags, double weight, pvlm_resset** out);

/* ---- equirectangular camera model + camera<->LiDAR voting --------------------------------------- */
/* Equirectangular::CamToImage<T> (sensors/Equirectangular.h:173-182, FastAtan2 variant) for n
 * points; cam n x 3, pixels n x 2.  _f32 mirrors the cv::Point3f overloads, _f64 the Eigen ones. */
pvlm_status pvlm_cam_to_image_f32(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* cam, float* pixels);
pvlm_status pvlm_cam_to_image_f64(pvlm_ctx* ctx, int rows, int cols, int64_t n, const double* cam, double* pixels);
/* Equirectangular::ImageToCam<T> (sensors/Equirectangular.h:149-170). */
pvlm_status pvlm_image_to_cam_f32(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* pixels, float r, float* cam);
pvlm_status pvlm_image_to_cam_f64(pvlm_ctx* ctx, int rows, int cols, int64_t n, const double* pixels, double r, double* cam);

/* Same maps on device-resident buffers (async on the ctx stream, no copies) — whole-panorama use. */
pvlm_status pvlm_cam_to_image_f32_dev(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* d_cam, float* d_pixels);
pvlm_status pvlm_image_to_cam_f32_dev(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* d_pixels, float r, float* d_cam);

/* ProjectLidar2PanoramaDepth (util/Visualization.h:407-441; the LiDAR-seeded depth prior of mvs/MVS.cpp:510-514):
 * transforms the cloud (n x 3 float, LiDAR frame) by T_cl like pcl::transformPointCloud, projects with
 * Equirectangular::CamToImage<float> and paints depth * 256 (uint16) over the window
 * [floor(px) - size/2, ceil(px) + size/2]^2; points whose window leaves the image are skipped; where windows
 * overlap the LAST point of the cloud wins, as in the reference's sequential loop.  depth: rows x cols uint16. */
pvlm_status pvlm_project_lidar_depth(pvlm_ctx* ctx, int rows, int cols, int64_t n, const float* xyz, const double* T_cl_rowmajor16,
                                     unsigned size, uint16_t* depth);

/* ---- K37: LiDAR depth completion ---------------------------------------------------------------------------------------------------------
 * DepthCompletion (util/DepthCompletion.cpp:154-316) for a batch of n_images equal-sized images (rows x cols, one after the other): the chain of masked dilations,
 * close, medians, column scans, hole fills and the bilateral filter that csrc/pvlm_depthfill_core.h states stage by stage, with the OpenCV semantics it rests on and
 * the deliberate divergence of the bilateral filter.  Exactly one input: sparse_u16 (depth * 256, upstream's CV_16U image; value / 256 is exact) or sparse_f32
 * (metres; a value with a sign bit or a non-finite value is PVLM_ERR_ARG).  At least one output: dense_f32 (DepthCompletion's result) and / or dense_u16
 * (rint(result * 256), half to even, saturated: what ComputeDepthImage stores).  max_depth must be finite and > 0.  The images are worked through in bounded
 * batches of whole images; PVLM_DEPTHFILL_BATCH_IMAGES (read at every call) lowers the limit and changes no result.  Synchronous; PVLM_ERR_STATE inside a capture. */
typedef struct pvlm_depthfill_stats {
  long long images;        /* images completed */
  long long batches;       /* device batches they were worked through in */
  long long valid_in;      /* pixels with s0 > 0.1 (a depth in (0.1, max_depth]) over all inputs */
  long long valid_out;     /* pixels > 0.1 over all results */
  double splat_ms;         /* HIP-event time of the batches' splats, the clearing of their 64-bit images and the upload of the points included (pvlm_compute_depth_images; else 0) */
  double fill_ms;          /* HIP-event time of the batches' three completion kernels */
} pvlm_depthfill_stats;
pvlm_status pvlm_depth_completion(pvlm_ctx* ctx, int rows, int cols, int n_images, const uint16_t* sparse_u16_or_null, const float* sparse_f32_or_null, float max_depth,
                                  float* dense_f32_or_null, uint16_t* dense_u16_or_null, pvlm_depthfill_stats* stats_or_null);
/* The loop body of SfM::ComputeDepthImage (sfm/SfM.cpp:170-226) for all scans in one call: ProjectLidar2PanoramaDepth(cloud, rows, cols, T_cl, size) (the splat of
 * pvlm_project_lidar_depth), DepthCompletion(depth, max_depth), x 256, uint16; nothing returns to the host in between.  rows x cols is the size of the depth
 * image (upstream passes (image rows + 1) / 2 and (image cols + 1) / 2 and size 4).  Scan s is the points first_point[s] .. first_point[s + 1] of xyz (3 floats each,
 * LiDAR frame; first_point ascending from 0, PVLM_ERR_ARG otherwise); T_cl (16 doubles, row-major) is the one calibration of all scans.  depth_u16: n_scans
 * images.  A scan without points gives an all-zero image.  No visualisation, no file export. */
pvlm_status pvlm_compute_depth_images(pvlm_ctx* ctx, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl_rowmajor16,
                                      unsigned size, float max_depth, uint16_t* depth_u16, pvlm_depthfill_stats* stats_or_null);

/* pvlm_depthset: the uint16 depth maps of a set of frames, resident on the device (upstream: frames[i].depth_map).  A frame without a map is "empty"
 * (depth_map.empty()); frames may differ in size.  The memory comes from the context's pool: pvlm_mem_info counts it as in use and pvlm_trim leaves it alone, as
 * for a pvlm_descset.  A set may be used only with the context that made it (PVLM_ERR_ARG otherwise).
 * pvlm_depthset_compute: pvlm_compute_depth_images with the same arguments, checks and batches (PVLM_DEPTHFILL_BATCH_IMAGES included), the n_scans maps left in ONE
 * device allocation of a new set; nothing returns to the host but the two counters of the statistics.
 * pvlm_depthset_create: a set of n_frames empty frames.  pvlm_depthset_upload: frame `frame` becomes the rows x cols map depth_u16 (its own allocation; a map
 * uploaded there before is released).  pvlm_depthset_info: the size of a frame's map, 0 x 0 for an empty frame.  pvlm_depthset_read: one map to the host
 * (rows x cols of pvlm_depthset_info; an empty frame is PVLM_ERR_ARG).  Synchronous; PVLM_ERR_STATE inside a capture. */
typedef struct pvlm_depthset pvlm_depthset;
pvlm_status pvlm_depthset_compute(pvlm_ctx* ctx, int rows, int cols, int n_scans, const long long* first_point, const float* xyz, const double* T_cl_rowmajor16,
                                  unsigned size, float max_depth, pvlm_depthset** out, pvlm_depthfill_stats* stats_or_null);
pvlm_status pvlm_depthset_create(pvlm_ctx* ctx, int n_frames, pvlm_depthset** out);
pvlm_status pvlm_depthset_upload(pvlm_ctx* ctx, pvlm_depthset* set, int frame, int rows, int cols, const uint16_t* depth_u16);
pvlm_status pvlm_depthset_info(const pvlm_depthset* set, int frame, int* rows, int* cols);
pvlm_status pvlm_depthset_read(pvlm_ctx* ctx, const pvlm_depthset* set, int frame, uint16_t* depth_u16_out);
void pvlm_depthset_destroy(pvlm_ctx* ctx, pvlm_depthset* set);

/* ---- K39: the translation scale of every pair from the resident depth maps ---------------------------------------------------------------------
 * SfM::SetTranslationScaleDepthMap(eq, pair) (sfm/SfM.cpp:487-603) for n_pairs pairs in one call, as csrc/pvlm_scale_core.h states it: bit for bit what the host
 * step computes (fp64, no contraction, the mean added in list order).  eq_rows x eq_cols: the one Equirectangular of all frames; frame_rows[f]: the image rows of
 * frame f (the half-size test d1.rows == (rows + 1) / 2); pair p is (src[p], tgt[p]) with the points point_offsets[p] .. point_offsets[p + 1] of triangulated (3
 * doubles each, in the first camera's frame), R_21 (9, row-major) and t_21 (3).  A scaled pair: ok = 1, t_21 and its points multiplied by the scale,
 * points_with_depth, upper_scale and lower_scale set (0, 0 for the median fall-back).  An unscaled pair (an empty map, or fewer than 10 scales): ok = 0, t_21, the
 * points, upper_scale and lower_scale untouched, points_with_depth = 0 when both maps were there and untouched otherwise.  A pair's result does not depend on the
 * other pairs, the batch or the run.  PVLM_ERR_ARG with no output touched: a frame index outside the set, offsets that do not ascend from 0, a pose or point that is
 * not finite, eq_rows or eq_cols <= 0.  The list is worked through in batches bounded in pairs and points; PVLM_SCALE_BATCH_PAIRS (read at every call) lowers the
 * pair limit and changes no result.  Synchronous; PVLM_ERR_STATE inside a capture. */
typedef struct pvlm_scale_stats {
  long long pairs_mean;      /* pairs scaled by the mean of the kept scales */
  long long pairs_median;    /* pairs scaled by the median fall-back */
  long long pairs_unscaled;  /* pairs left as they were */
  long long points_tested;   /* points of the pairs whose two maps were there */
  long long points_scaled;   /* points that gave a consistent scale pair */
  long long batches;
} pvlm_scale_stats;
pvlm_status pvlm_set_translation_scales(pvlm_ctx* ctx, const pvlm_depthset* set, int eq_rows, int eq_cols, const int* frame_rows /* n_frames of the set */, int n_pairs,
                                        const int* src, const int* tgt, const long long* point_offsets /* n_pairs + 1 */, const double* R_21, double* t_21 /* in/out */,
                                        double* triangulated /* in/out */, unsigned char* ok, int* points_with_depth /* in/out */, double* upper_scale /* in/out */,
                                        double* lower_scale /* in/out */, pvlm_scale_stats* stats_or_null);
int pvlm_scale_workgroup_size(void);

/* ---- K41: SIFT keypoints and (Root)SIFT descriptors (util/SIFT.cpp:10-128 behind Frame::ExtractKeyPoints / ComputeDescriptor, sensors/Frame.cpp:110-121) ----
 * The definition (csrc/pvlm_sift_core.h) is this library's own statement of cv::xfeatures2d::SIFT as upstream calls it; there is no OpenCV build to pin it against.
 * [recalled] create(nfeatures): 3 layers per octave, contrast threshold 0.04, edge threshold 10, sigma 1.6, first octave -1; the float build (sift_wt = float,
 *   fixed-point scale 1).  [recalled] cvRound is round-half-to-even; that is every "rint" below.
 * Base image: grey -> float; doubled by bilinear interpolation at (d + 0.5) / 2 - 0.5 with a replicated border (weights exactly 0.25 / 0.75); blurred with
 *   sigma sqrt(max(1.6^2 - 1^2, 0.01)) [recalled].  Octaves: round(log2(min(base w, base h)) - 2) + 1 [recalled], evaluated in integers.
 * Layers: layer i >= 1 is layer i - 1 blurred with sqrt((1.6 k^i)^2 - (1.6 k^(i-1))^2), k = 2^(1/3); 6 Gaussian and 5 difference layers per octave; the next
 *   octave is layer 3 at every second pixel (2y, 2x) ([recalled] upstream: resize INTER_NEAREST to (w / 2, h / 2), the same pixels for even sizes).
 * Blur: separable, rows then columns; taps = floor(8 sigma + 1.5) | 1 [recalled]; coefficients exp(-x^2 / 2 sigma^2) normalised in double on the host and rounded
 *   to float once; reflect-101 folded as often as needed; s = s + c[k] * tap for k ascending from s = 0, multiply and add unfused.
 * Extrema: strictly inside a 5-pixel border, |v| > floor(0.5 * 0.04 / 3 * 255) = 1, >= all 26 neighbours (v > 0) or <= all 26 (v < 0) [recalled].
 * Refinement [recalled adjustLocalExtrema]: at most 5 Newton steps of the 3-D quadratic fit with derivative scales 1/255 * (0.5, 1, 0.25); the 3 x 3 system by
 *   cofactors in float; an offset component of 0.5 or more moves by rint(offset); leaving layers 1..3 or the border, 5 moves, a zero determinant or an offset of
 *   1e6 or more rejects; contrast |D + 0.5 g.x| / 255-scaled * 3 >= 0.04; edge tr^2 * 10 < 11^2 det, det > 0.  Record: x = (c + xc) 2^o, y = (r + xr) 2^o,
 *   size = 1.6 * 2^((layer + xi) / 3) * 2^o * 2, response = |contrast|, octave word = o + (layer << 8) + (rint((xi + 0.5) * 255) << 16).
 * Orientation [recalled calcOrientationHist]: 36 bins, radius rint(3 * 1.5 * scale), weight exp(-(i^2 + j^2) / (2 (1.5 scale)^2)), pixels with a missing neighbour
 *   skipped, [1 4 6 4 1] / 16 smoothing, every local peak >= 0.8 of the maximum with parabolic interpolation, angle = 360 - 10 * bin (360 -> 0).
 * Selection, in this order: duplicates (equal x, y, size, angle; the first in order stays), retainBest(nfeatures) (everything with response >= the nfeatures-th
 *   largest: ties keep more than n), coordinates and size * 0.5 and the octave byte - 1 (first octave -1), then the mask: dropped where
 *   mask(rint y, rint x) == 0, the indices clamped into the image.
 * Descriptor [recalled calcSIFTDescriptor]: on the keypoint's own Gaussian layer, 4 x 4 x 8 bins, histogram width 3 * size / 2, radius
 *   rint(width * sqrt 2 * 5 / 2) capped at the layer's diagonal, weight exp(-(r^2 + c^2) / 8) in bin units, trilinear; clamp at 0.2 of the norm, * 512 / norm,
 *   rint saturated to 0..255, stored as float.  RootSIFT (PVLM_FLAG_SIFT_ROOT, util/SIFT.cpp:10-21): per row v / L1, square root, * 512.
 * Deliberate divergences:
 *   - exp, atan2, sin / cos, 2^x and sqrt are this library's deterministic ones (K37's exp_neg, a polynomial atan2, Taylor sin / cos, IEEE sqrt), not OpenCV's
 *     hal::fastAtan2 / exp32f tables; histogram sums have one fixed order (sample j of a window belongs to lane j % 64, lanes added in ascending order).
 *   - keypoints come out in one defined order: octave, layer, row, column of the detection, then ascending histogram bin; the selection is a stable filter of
 *     that order (upstream: TLS-parallel row strips and nth_element).
 *   - an all-zero row under RootSIFT stays zero (upstream divides by 0); an image with a side below 8 pixels is PVLM_ERR_ARG; the pyramid is built once for
 *     detect and compute (upstream builds it twice with identical values).
 *   - the refinement rejects an offset component of 1e6 or more in magnitude (or a NaN) where upstream rejects above INT_MAX / 3: the bound within which the
 *     half-to-even rounding used here is exact; either is far outside any offset that could move to a pixel of the image.
 *   - the next octave takes the pixels (2y, 2x) of layer 3; for odd sizes upstream's INTER_NEAREST resize picks other columns.
 * pvlm_sift_extract: n_images grey images of rows x cols (uint8, row-major), an optional mask of the same size, nfeatures > 0.  Image i's keypoints are
 *   keypoints[kp_offsets[i] .. kp_offsets[i + 1]) and their descriptors the same rows of `descriptors` (128 floats each): Frame's layout, what pvlm_descset_create
 *   takes.  *needed = kp_offsets[n_images]; when it exceeds capacity the call returns PVLM_ERR_CAPACITY with kp_offsets and *needed set and nothing past
 *   capacity written.  A call that fails for capacity has done all the work but the descriptors: size the first call by n_images * nfeatures plus some room
 *   for ties at the nfeatures-th response and repeat only on PVLM_ERR_CAPACITY (pvlm::ReadImages and the Python binding do).  descriptors == NULL asks for the
 *   keypoints alone: the descriptor kernel is not run.  One image is in flight at a time; its layers come from the context's pool.  The selection runs on the host between the orientation and
 *   the descriptor kernels.  A result does not depend on the other images of the batch.  Synchronous; PVLM_ERR_STATE inside a capture.
 * pvlm_sift_pyramid_debug: one image; the 6 Gaussian and 5 difference layers of `octave` (octave_rows x octave_cols floats each; either may be NULL), that
 *   octave's refined candidates and the whole image's keypoints before the selection, both with the capacity protocol above. */
#define PVLM_FLAG_SIFT_ROOT 0x1000u
typedef struct pvlm_sift_keypoint { float x, y, size, angle, response; int octave; } pvlm_sift_keypoint;
typedef struct pvlm_sift_candidate {
  int octave, layer, r, c;          /* the refined position in its octave's pixels */
  float x, y, size, response;       /* before the first octave's 0.5 */
  int word, det_layer, det_r, det_c; /* the octave word; where the extremum was detected */
} pvlm_sift_candidate;
typedef struct pvlm_sift_stats {
  long long images, octaves;
  long long candidates;            /* refined extrema */
  long long keypoints_detected;    /* with their orientations, before the selection */
  long long keypoints;             /* returned */
  double part_ms[6];               /* device time by HIP events: (a) doubling + first blur, (b) layer blurs + differences, (c) decimation, (d) extrema +
                                      refinement, (e) orientation, (f) descriptors */
} pvlm_sift_stats;
pvlm_status pvlm_sift_extract(pvlm_ctx* ctx, int n_images, int rows, int cols, const unsigned char* const* images, const unsigned char* mask_or_null, int nfeatures,
                              unsigned flags, long long* kp_offsets /* n_images + 1 */, pvlm_sift_keypoint* keypoints, float* descriptors /* 128 per keypoint */,
                              long long capacity, long long* needed, pvlm_sift_stats* stats_or_null);
pvlm_status pvlm_sift_pyramid_debug(pvlm_ctx* ctx, int rows, int cols, const unsigned char* image, int octave, int* n_octaves, int* octave_rows, int* octave_cols,
                                    float* gauss_or_null /* 6 layers */, float* dog_or_null /* 5 layers */, pvlm_sift_candidate* candidates, long long candidate_capacity,
                                    long long* candidates_needed, pvlm_sift_keypoint* keypoints, long long keypoint_capacity, long long* keypoints_needed);

/* MVS::InitDepthNormal (mvs/MVS.cpp:496-584; config 5 "LiDAR-seeded depth priors"): the depth image of
 * pvlm_project_lidar_depth (uint16, depth * 256; size 2 upstream, :512) seeds the depth map, every pixel without a LiDAR depth
 * gets a uniform random depth in [min_depth, max_depth], keep_lidar_constant != 0 marks the seeded pixels in depth_constant
 * (config.keep_lidar_constant, :561-565), `mask` (float, 1 = keep) zeroes excluded pixels (:571), and every kept pixel gets a
 * random unit normal facing the camera (GenerateRandomNormal :1404-1431).  lidar_depth == NULL is the use_lidar = false branch
 * (:566-569), mask == NULL keeps everything.  Random draws: upstream uses one cv::RNG seeded with time(NULL); here draw k of
 * pixel e is a hash of (seed, e, k), as in pvlm_mvs_propagate — the same arguments give the same maps.
 * depth: rows x cols, normal: rows x cols x 3 (outputs); depth_constant: rows x cols uint8, written only with a LiDAR image. */
pvlm_status pvlm_mvs_init_depth_normal(pvlm_ctx* ctx, int rows, int cols, const uint16_t* lidar_depth_or_null, const float* mask_or_null, float min_depth,
                                       float max_depth, int keep_lidar_constant, unsigned long long seed, float* depth, float* normal,
                                       unsigned char* depth_constant_or_null);
/* MVS::RemoveSmallSegments (mvs/MVS.cpp:1504-1577, called at the end of a view's estimation, :102 / :138): 4-connected regions of
 * similar depth (relative difference < depth_diff_threshold, config 0.01) grown from seeds in column-major order; regions with fewer
 * than min_segment pixels (config/Room.txt:92: 100) lose depth (0), normal (0) and confidence (-1) — pixels without depth are
 * regions of size one and are reset as well.  In place on HOST arrays, executed on the host: the growth rule divides by the depth
 * of the pixel a neighbour is reached from, so the result depends on the sequential seed order (see csrc/pvlm_mvs.hip). */
pvlm_status pvlm_mvs_remove_small_segments(pvlm_ctx* ctx, int rows, int cols, float depth_diff_threshold, int min_segment, float* depth, float* normal,
                                           float* conf, int64_t* removed_or_null);

/* Photometric scoring pass of the panoramic PatchMatch MVS: MVS::InitPatchMap + MVS::InitConfMap(use_geometry = false)
 * (mvs/MVS.cpp:586-680) with the photometric term of ScorePixel (:774-923): for every pixel with depth > 0 the
 * bilaterally weighted NCC of its (2 half_window + 1)^2 / step^2 window against each neighbour panorama through the
 * plane-induced homography R_nr + t_nr n^T / d, averaged over the two best neighbours; conf = -1 (and depth / normal
 * zeroed) where the reference patch is invalid, the plane faces away (d > 0) or no neighbour sees the window.
 * ref_gray / nei_gray[b]: rows x cols uint8; R_nr: n x 9 row-major, t_nr: n x 3 (reference -> neighbour camera);
 * depth (rows x cols), normal (rows x cols x 3, camera frame), conf (rows x cols): float32, in-out. n_neighbors <= 16.
 * nei_depth != NULL = InitConfMap(use_geometry = true): nei_depth[b] is neighbour b's photometric depth map
 * (Frame::depth_filter) and every neighbour score gets the geometric-consistency adjustment of ScorePixel :857-893
 * (forward / backward projection through that depth map, 0.2 x min(angle in degrees, 2) penalty). */
pvlm_status pvlm_mvs_init_conf_map(pvlm_ctx* ctx, int rows, int cols, int half_window, int step, const unsigned char* ref_gray, int n_neighbors,
                                   const unsigned char* const* nei_gray, const float* R_nr, const float* t_nr, float* depth, float* normal,
                                   float* conf, const float* const* nei_depth_or_null);

/* PatchMatch sweep: MVS::EstimateDepthMapSingle(ref, Propagate::CHECKER_BOARD, max_iter, conf_threshold, use_geometry)
 * (mvs/MVS.cpp:682-720) = max_iter x PropagateCheckerBoard (:1098-1129; per pixel ProcessPixel :721-772: the four direct
 * neighbours' hypotheses interpolated to the pixel and re-scored with the smoothness term, then PerturbDepthNormal3
 * :1254-1320: up to 6 random + 6 refining perturbations), then hypotheses with conf < conf_threshold are dropped
 * (depth 0, conf -1, normal 0; depth_constant pixels are kept).  depth / normal / conf are IN-OUT and must hold an
 * initialised state (InitDepthNormal + pvlm_mvs_init_conf_map).  nei_depth != NULL = use_geometry; depth_constant may
 * be NULL; min_depth / max_depth = config.min_depth / max_depth.
 * RANDOM DRAWS: upstream all OpenMP threads pull from one cv::RNG seeded with time(NULL) (mvs/MVS.cpp:30), a data race
 * that makes every run different; here draw k of pixel e in colour pass p is a hash of (seed, p, e, k) — the same
 * arguments give the same maps. */
pvlm_status pvlm_mvs_propagate(pvlm_ctx* ctx, int rows, int cols, int half_window, int step, const unsigned char* ref_gray, int n_neighbors,
                               const unsigned char* const* nei_gray, const float* R_nr, const float* t_nr, float* depth, float* normal, float* conf,
                               const float* const* nei_depth_or_null, const unsigned char* depth_constant_or_null, float min_depth, float max_depth,
                               unsigned long long seed, int max_iter, float conf_threshold);
/* The same with Propagate::SEQUENTIAL — the strategy config/Room.txt:90 and config/Floor.txt:88 select (propagate_strategy = 2):
 * MVS::PropagateSequential (mvs/MVS.cpp:1057-1097) walks the image in raster order on even iterations (a pixel takes the
 * hypotheses of its LEFT and UPPER neighbour, which the walk has just updated) and backwards on odd ones (right, lower); pixels
 * with patch.sq0 <= 0 are skipped.  Here every anti-diagonal col + row = d is one launch, ascending (descending) d: a pixel
 * reads only its four direct neighbours, so the pixels of a diagonal are independent and each sees exactly what the raster walk
 * shows it — same maps as the sequential loop, bit for bit.  Draw k of pixel e in iteration i = hash(seed, i, e, k). */
pvlm_status pvlm_mvs_propagate_sequential(pvlm_ctx* ctx, int rows, int cols, int half_window, int step, const unsigned char* ref_gray, int n_neighbors,
                                          const unsigned char* const* nei_gray, const float* R_nr, const float* t_nr, float* depth, float* normal,
                                          float* conf, const float* const* nei_depth_or_null, const unsigned char* depth_constant_or_null,
                                          float min_depth, float max_depth, unsigned long long seed, int max_iter, float conf_threshold);

/* Depth-map fusion filter: MVS::FilterDepthImage (mvs/MVS.cpp:1735-1790) with ProjectDepthConfToRef (:2011-2070, depth):
 * every neighbour depth map is forward-projected into the reference view (4-pixel splat, nearest range wins); a reference
 * depth survives when >= 2 neighbours agree within 0.8 x threshold at the pixel and >= 5 (neighbour, 4-neighbourhood)
 * samples agree within 1.2 x threshold (or depth_constant marks it).  depth_filter / conf_filter (rows x cols float)
 * are outputs, 0 where rejected; conf / conf_filter and depth_constant may be NULL. */
pvlm_status pvlm_mvs_filter_depth(pvlm_ctx* ctx, int rows, int cols, int n_neighbors, const float* const* nei_depth, const float* R_nr, const float* t_nr,
                                  const float* depth, const float* conf_or_null, const unsigned char* depth_constant_or_null,
                                  float depth_diff_threshold, float* depth_filter, float* conf_filter_or_null);

/* The fusion filter the reference's MVS pipeline actually runs (mvs/MVS.cpp:194): MVS::FilterDepthImageRefine
 * (mvs/MVS.cpp:1794-1890) with ProjectDepthConfToRef projecting depth and confidence (:2011-2070).  A reference depth is
 * replaced by the confidence-weighted average of itself and the neighbour ranges that agree within 1.2 x threshold when
 * >= 2 neighbours agree, the agreeing confidence exceeds the disagreeing one (occlusions / free-space violations) and
 * the average lies in [min_depth, max_depth] (config.min_depth / max_depth, base/Config.h:65-66); conf_filter = positive -
 * negative confidence.  depth_constant pixels that fail keep their depth with confidence 1.  nei_conf[b] = neighbour
 * b's conf_map after ConvertNCC2Conf (:2343); conf (the reference frame's conf_map) is IN-OUT: zeroed where depth <= 0,
 * as upstream.  depth_filter / conf_filter: rows x cols float outputs, 0 where rejected. */
pvlm_status pvlm_mvs_filter_depth_refine(pvlm_ctx* ctx, int rows, int cols, int n_neighbors, const float* const* nei_depth,
                                         const float* const* nei_conf, const float* R_nr, const float* t_nr, const float* depth, float* conf,
                                         const unsigned char* depth_constant_or_null, float depth_diff_threshold, float min_depth, float max_depth,
                                         float* depth_filter, float* conf_filter);

/* Depth map -> coloured world points: MVS::DepthImageToCloud (mvs/MVS.cpp:2073-2107; filter_sky = 1, normal_out = NULL) and
 * MVS::DepthNormalToCloud (:2109-2142; filter_sky = 0, normal_out != NULL), the per-frame bodies of MVS::MergeDepthImages
 * (:2144-2166; what MVS::FuseDepthMaps :224-227 saves as MVS-merge.pcd) and of the per-frame .pcd export.  A pixel with
 * 0 < depth < 0.8 max_depth becomes TranslatePoint<float, double>(ImageToCam(col, row) * depth, T_wc) (base/Geometry.hpp:545-551)
 * with its colour — unless filter_sky and BGR2HSV (util/Visualization.cpp:57-77) puts the colour in the reference's "sky blue"
 * box (H 100..124, S 43..200, V 150..255) — and, with normal_out, the normal R_wc n.  Points come out in raster order, as
 * the reference's loops push them.  bgr: rows x cols x 3 (cv::Vec3b order); T_wc: the frame pose, 3 x 4 or 4 x 4 row-major
 * (12 doubles read); xyz / normal_out: capacity rows x cols x 3 float, rgb: rows x cols x 3 bytes (r, g, b); *n_points = points written.
 * pvlm_mvs_views_depth_to_cloud (declared below) reads depth (or depth_filter) and normal of a resident view instead. */
pvlm_status pvlm_mvs_depth_to_cloud(pvlm_ctx* ctx, int rows, int cols, const float* depth, const unsigned char* bgr, const float* normal_or_null,
                                    const double* T_wc, float max_depth, int filter_sky, float* xyz, unsigned char* rgb, float* normal_out_or_null,
                                    long long* n_points);

/* Resident view set: the maps of n_views equally sized views (grey image, depth, normal, conf, depth_filter, conf_filter —
 * the cv::Mat members of sensors/Frame.h the MVS touches) stay in HBM across the calls, so that a view's scoring pass,
 * sweeps and fusion filter — and its use as somebody's neighbour — cost no PCIe traffic.  Same kernels and results as
 * the per-call entry points above.  `nei` holds view indices (each != ref); R_nr / t_nr as above.
 *   pvlm_mvs_views_estimate      max_iter < 0: MVS::InitConfMap(ref, ., use_geometry); max_iter >= 0: MVS::EstimateDepthMapSingle
 *                                (checkerboard; pvlm_mvs_views_estimate_sequential: the sequential sweep).  use_geometry reads the neighbours' depth_filter (the photometric depth the reference
 *                                keeps there, mvs/MVS.cpp:470-473): pvlm_mvs_views_snapshot_depth copies depth -> depth_filter of a view.
 *   pvlm_mvs_views_filter_refine MVS::FilterDepthImageRefine(ref): writes depth_filter / conf_filter of ref, zeroes its conf where depth <= 0.
 * estimate / filter_refine / snapshot_depth are asynchronous on the context's stream; upload / download synchronise.
 * NULL pointers in upload / download skip that map. */
typedef struct pvlm_mvs_views pvlm_mvs_views;
pvlm_status pvlm_mvs_views_create(pvlm_ctx* ctx, int rows, int cols, int n_views, pvlm_mvs_views** out);
pvlm_status pvlm_mvs_views_destroy(pvlm_ctx* ctx, pvlm_mvs_views* views);
pvlm_status pvlm_mvs_views_depth_to_cloud(pvlm_ctx* ctx, pvlm_mvs_views* views, int view, int use_filtered_depth, const unsigned char* bgr, const double* T_wc,
                                          float max_depth, int filter_sky, float* xyz, unsigned char* rgb, float* normal_out_or_null, long long* n_points);
pvlm_status pvlm_mvs_views_upload(pvlm_ctx* ctx, pvlm_mvs_views* views, int view, const unsigned char* gray_or_null, const float* depth_or_null,
                                  const float* normal_or_null, const float* conf_or_null);
pvlm_status pvlm_mvs_views_download(pvlm_ctx* ctx, pvlm_mvs_views* views, int view, float* depth_or_null, float* normal_or_null, float* conf_or_null,
                                    float* depth_filter_or_null, float* conf_filter_or_null);
pvlm_status pvlm_mvs_views_snapshot_depth(pvlm_ctx* ctx, pvlm_mvs_views* views, int view);
pvlm_status pvlm_mvs_views_estimate(pvlm_ctx* ctx, pvlm_mvs_views* views, int ref, int n_neighbors, const int* nei, const float* R_nr, const float* t_nr,
                                    int half_window, int step, int use_geometry, const unsigned char* depth_constant_or_null, float min_depth,
                                    float max_depth, unsigned long long seed, int max_iter, float conf_threshold);
/* EstimateDepthMapSingle with Propagate::SEQUENTIAL on a resident view (see pvlm_mvs_propagate_sequential); max_iter >= 0 */
pvlm_status pvlm_mvs_views_estimate_sequential(pvlm_ctx* ctx, pvlm_mvs_views* views, int ref, int n_neighbors, const int* nei, const float* R_nr,
                                               const float* t_nr, int half_window, int step, int use_geometry, const unsigned char* depth_constant_or_null,
                                               float min_depth, float max_depth, unsigned long long seed, int max_iter, float conf_threshold);
/* The same for n_jobs DISTINCT reference views in one go (one launch per anti-diagonal covers all of them): a single view's
 * diagonal is too short to fill the GPU, and upstream runs this strategy with one image per thread for the same reason
 * (mvs/MVS.cpp:87-93).  Job j: reference refs[j], its nei_counts[j] neighbours follow those of job j - 1 in nei / R_nr / t_nr,
 * random stream seeds[j]; depth_constant: NULL or n_jobs pointers (NULL entries allowed).  Results = n_jobs calls of
 * pvlm_mvs_views_estimate_sequential, bit for bit.  Synchronises before returning. */
pvlm_status pvlm_mvs_views_estimate_sequential_batch(pvlm_ctx* ctx, pvlm_mvs_views* views, int n_jobs, const int* refs, const int* nei_counts, const int* nei,
                                                     const float* R_nr, const float* t_nr, int half_window, int step, int use_geometry,
                                                     const unsigned char* const* depth_constant_or_null, float min_depth, float max_depth,
                                                     const unsigned long long* seeds, int max_iter, float conf_threshold);
pvlm_status pvlm_mvs_views_filter_refine(pvlm_ctx* ctx, pvlm_mvs_views* views, int ref, int n_neighbors, const int* nei, const float* R_nr, const float* t_nr,
                                         const unsigned char* depth_constant_or_null, float depth_diff_threshold, float min_depth, float max_depth);

/* Hot loop #3 of CameraLidarLineAssociate::AssociateByAngle
 * (joint_optimization/CameraLidarLineAssociate.cpp:394-426): for every image line (x1,y1,x2,y2
 * pixels, n_lines x 4 float) and every LiDAR corner point (LiDAR-local float xyz, transformed by
 * T_cl as pcl::transformPointCloud does) apply the 15 m range test and the two 3-degree angle tests
 * and count votes per LiDAR segment.  votes is n_lines x n_segments int32. */
pvlm_status pvlm_cam_lidar_votes(pvlm_ctx* ctx, int rows, int cols, const float* lines, int n_lines,
                                 const pvlm_scan* lidar_local, const double* T_cl_rowmajor16, int32_t* votes);

/* Batched form — every (frame, LiDAR) pair of AssociateLineMulti (CameraLidarOptimizer.cpp:345-377, an omp loop
 * over frames upstream) in one launch: pair p uses the image lines [line_offsets[p], line_offsets[p+1]) of
 * `lines`, the scan lidar_local[p] and T_cl + 16 p; its votes (n_lines(p) x n_segments(p)) start at
 * votes + vote_offsets[p].  Sizing / capacity rules as for pvlm_line2line_votes_batch. */
pvlm_status pvlm_cam_lidar_votes_batch(pvlm_ctx* ctx, int n_pairs, int rows, int cols, const int64_t* line_offsets,
                                       const float* lines, pvlm_scan* const* lidar_local, const double* T_cl_rowmajor16,
                                       int64_t* vote_offsets, int32_t* votes, int64_t capacity);

/* The same launch with the votes returned SPARSE: a few per cent of the counters are non-zero (43 MB of dense blocks for the 1 362 pairs of a Room
 * sequence).  vote_offsets as above (the dense layout the indices refer to); nz_index[k] = dense position of the k-th non-zero counter (ascending:
 * pair by pair, line by line, segment by segment), nz_count[k] = its value; *n_nz = how many there are.  capacity = room in nz_index / nz_count:
 * PVLM_ERR_CAPACITY when it is too small (*n_nz is set: call again). */
pvlm_status pvlm_cam_lidar_votes_batch_sparse(pvlm_ctx* ctx, int n_pairs, int rows, int cols, const int64_t* line_offsets, const float* lines,
                                              pvlm_scan* const* lidar_local, const double* T_cl_rowmajor16, int64_t* vote_offsets, int64_t* nz_index,
                                              int32_t* nz_count, int64_t capacity, int64_t* n_nz);

/* ---- LiDAR feature extraction, range-image stages ------------------------------------------------------- *
 * The per-point / per-ring stages in front of the association, for a BATCH of raw scans in one go (the reference runs them scan by
 * scan under `omp parallel for`, lidar_mapping/LidarOdometry.cpp:131-147):
 *   Velodyne::ReOrderVLP      sensors/Velodyne.cpp:371-526    firing order -> ring order; range image; (ring, column) of every point
 *   Velodyne::Segmentation    sensors/Velodyne.cpp:1438-1586  range-image labelling; points of small components dropped (segment != 0)
 *   adaptive-window curvature sensors/Velodyne.cpp:623-657    the first loop of Velodyne::ExtractFeatures (method ADAPTIVE)
 * What they produce — cloud_scan, point_idx_to_image, image_to_point_idx, range_image, scanStartInd / scanEndInd, cloudCurvature,
 * left_neighbor / right_neighbor, cloudDistance (sensors/Velodyne.h:97-120 and the locals of ExtractFeatures) — is what the
 * sort-dependent picks (ExtractEdgeFeatures2 :883-1000, ExtractPlaneFeatures2 :1098-1189) read.
 * xyzi: the scan as LoadLidar left it (sensors/Velodyne.cpp:92-145; camera-style axes, float x y z intensity), point i at
 * xyzi + i * stride_floats (pcl::PointXYZI: stride 8; packed: 4).  Non-finite coordinates are an error (LoadLidar removed them).
 * Decisions that go through the float libm of the reference's host (atan / atan2 with `using namespace std`) are certified on
 * the device in fp64 interval form; the few points / edges that cannot be certified are decided by the libm of THIS host
 * inside the call (resolved_points / resolved_edges count them; replayed = 1 when a scan's +z crossing needed every point). */
typedef struct pvlm_ring_batch pvlm_ring_batch;
typedef struct pvlm_raw_scan {
  const float* xyzi;
  int n;
  int stride_floats;
} pvlm_raw_scan;
typedef struct pvlm_ring_result {
  int n_raw;                        /* points handed in                                                                          */
  int n_reordered;                  /* cloud_scan.size() after ReOrderVLP                                                        */
  int n_kept;                       /* cloud_scan.size() after Segmentation (== n_reordered when segment == 0)                   */
  int resolved_points, resolved_edges, replayed;
  const int* ring_count_reordered;  /* 64 entries: points per ring after ReOrderVLP                                              */
  const int* ring_count;            /* 64 entries: points per ring of the kept cloud: scanStartInd[r] = sum_{q<r} + 5,
                                       scanEndInd[r] = sum_{q<=r} - 6 (:520-522, :1575-1580)                                      */
  /* the kept cloud, n_kept entries each, valid until pvlm_ring_batch_destroy (pinned host memory owned by the batch):           */
  const int* source;                /* index of the point in the raw scan: cloud_scan[i] = (raw xyz, intensity = ring)           */
  const int* ring_col;              /* point_idx_to_image[i] as (ring << 16) | column                                            */
  const float* curvature;           /* cloudCurvature[i]; -1 where upstream leaves it unset                                      */
  const int* half_window;           /* left_neighbor[i] = i - half_window[i], right_neighbor[i] = i + half_window[i]; -1 = unset  */
  const float* range;               /* cloudDistance[i] = range_image(point_idx_to_image[i])  (:566-569)                         */
  const int* sorted;                /* cloudSortInd: the six sectors of every ring (:707-723) ordered by curvature as ExtractEdgeFeatures2
                                       :896 / ExtractPlaneFeatures2 :1110 sort them; index order outside the sectors                */
  const unsigned char* sector_host; /* n_rings x 6: 1 = the sector holds equal curvatures (or a NaN, or > 2048 points): std::sort's
                                       order of equal keys is the library's, `sorted` is the index order there and the caller sorts */
  /* pvlm_ring_extract_batch_picks only (picks == 1): the picks of ExtractEdgeFeatures2 (:883-1000) / ExtractPlaneFeatures2 (:1098-1189) and the
   * voxel grid of the less-flat points, ring by ring.  A scan with any ring_host[r] != 0 (incidence angle within libm distance of the threshold,
   * a sector left to the host, a ring beyond the kernel's bounds) is to be picked by the caller from the arrays above.                          */
  int picks;
  float max_curvature, intersect_angle_threshold;   /* what the picks were made with                                                */
  const unsigned char* state;       /* PointClassification bits of every kept point after both pick passes                         */
  const int* corner;                /* n_rings x 181: count, then the edge picks in pick order: point | 0x80000000 when sharp       */
  const int* flat;                  /* n_rings x 25: count, then the plane picks (surfFlat) in pick order                           */
  const int* voxel_span;            /* n_rings x 2: first, count of the ring's surfLessFlat centroids in `voxels`                  */
  const float* voxels;              /* x, y, z, class (1 = POINT_NORMAL) per centroid, ascending voxel order inside a ring          */
  const unsigned char* ring_host;   /* n_rings flags                                                                               */
} pvlm_ring_result;
pvlm_status pvlm_ring_extract_batch(pvlm_ctx* ctx, int n_scans, const pvlm_raw_scan* scans, int n_rings, int horizon_scans, int segment,
                                    pvlm_ring_batch** out);
/* The same, plus K24: the feature picks and the voxel grid (max_curvature, intersect_angle_threshold: the arguments of Velodyne::ExtractFeatures).  With the picks made
 * on the device the five per-point arrays curvature / half_window / range / sorted / sector_host (16 of the 27 B per point of the download) are delivered only for the
 * scans that have a ring left to the host (ring_host != 0) — they are NULL for the others — unless bit 1 of `segment` is set (segment = 2 | run_segmentation: always). */
pvlm_status pvlm_ring_extract_batch_picks(pvlm_ctx* ctx, int n_scans, const pvlm_raw_scan* scans, int n_rings, int horizon_scans, int segment,
                                          float max_curvature, float intersect_angle_threshold, pvlm_ring_batch** out);
pvlm_status pvlm_ring_batch_scan(const pvlm_ring_batch* batch, int scan, pvlm_ring_result* result);
/* The device-resident arrays of one scan (tests, visualisation).  state 0: after ReOrderVLP, 1: after Segmentation.  cloud_xyzi: n x 4
 * (intensity = ring), ring_col_pairs: n x 2, range_image / image_to_point: n_rings x horizon_scans (0 / -1 = empty).  NULL = skip. */
pvlm_status pvlm_ring_batch_fetch(pvlm_ctx* ctx, const pvlm_ring_batch* batch, int scan, int state, float* cloud_xyzi, int* ring_col_pairs,
                                  float* range_image, int* image_to_point);
/* HIP-event milliseconds of the last run: [0] upload  [1] K16 ring/azimuth + host libm  [2] K17 columns (+ replays)  [3] K18 scatter
 * [4] K19 edges + host libm  [5] K20 components  [6] K21 compaction + K22 curvature  [7] download. */
pvlm_status pvlm_ring_batch_timing(const pvlm_ring_batch* batch, double* ms8);
pvlm_status pvlm_ring_batch_destroy(pvlm_ctx* ctx, pvlm_ring_batch* batch);
/* Tests: the device's restatement of std::sort (csrc/pvlm_stdsort.h, sort_wave) on caller-given keys, n <= 4096: order[k] = index of the k-th element
 * as std::sort of the indices 0 .. n-1 by `keys[a] < keys[b]` leaves them — equal keys in libstdc++'s order.                                      */
pvlm_status pvlm_ring_debug_sort(pvlm_ctx* ctx, const unsigned* keys, int n, int* order);

/* ---- growth of the line segments of a batch of scans (N3, K27) -----------------------------------------------------------------------------
 * The growth phase of ExtractLineFeatures / ExpandLine (sensors/LidarLineExtraction.cpp:296-389, :10-70; called by Velodyne::EdgeToLine,
 * sensors/Velodyne.cpp:1269-1324) for every scan of a batch.  The segment grown from edge point i with its neighbours (a, b), 1 <= a < b <= 4 among its four nearest
 * edge points, never looks at what other segments took — only upstream's walk over the start points does (a point an earlier segment took is skipped) — so the
 * device grows the tasks of the next start points side by side and replays the walk over them (csrc/pvlm_linegrow.hip).  clouds[s]: the edge points of scan s
 * (cornerLessSharp before the filter), n <= 65535, stride_floats >= 3 floats between points (pcl::PointXYZI: 4).
 * pvlm_line_grow_scan: the segments upstream's walk keeps for one scan, in its order (start point ascending, then the combinations (1,2) (1,3) (1,4) (2,3) (2,4)
 * (3,4)): seg_task[q] = 6 i + combination, members[seg_offset[q] .. seg_offset[q + 1]) = ascending point ids of segment q (>= 5), coeffs[6 q ..] =
 * FormLine(members, 1.0) (zeros when that fit refuses: kept, as upstream keeps it).  status != 0: a segment of this scan outgrew the kernel's lists (2: more than 64
 * members, or more than 8192 edge points) or met a turn angle the host's acos has to decide (3) — the scan is to be grown by the caller.  PVLM_ERR_REFUSED: the
 * batch's segment pool was exhausted (nothing is returned; grow on the host).  The result lives in host memory until pvlm_line_grow_destroy. */
typedef struct pvlm_edge_cloud { const float* xyz; int n; int stride_floats; } pvlm_edge_cloud;
typedef struct pvlm_line_grow pvlm_line_grow;
typedef struct pvlm_line_grow_result {
  int status, n_points, n_segments;
  const int* seg_task;
  const int* seg_offset;            /* n_segments + 1 entries, offsets into `members` */
  const int* members;
  const double* coeffs;
  double kernel_ms;                 /* HIP-event time of the batch's two kernels */
  long long tasks_run;              /* (start point, neighbour pair) tasks the batch grew, the speculative ones included */
} pvlm_line_grow_result;
pvlm_status pvlm_line_grow_batch(pvlm_ctx* ctx, int n_scans, const pvlm_edge_cloud* clouds, pvlm_line_grow** out);
/* The same in two halves: _begin copies the clouds, queues the batch on a stream of its own (ordered behind what the context's stream holds at that moment) and returns
 * without waiting — the caller's next calls on this context (the range-image stages of the next device batch, say) run beside it; _finish waits and brings the
 * segments down.  One batch in flight per context (PVLM_ERR_STATE otherwise); pvlm_line_grow_scan serves finished batches only. */
pvlm_status pvlm_line_grow_begin(pvlm_ctx* ctx, int n_scans, const pvlm_edge_cloud* clouds, pvlm_line_grow** out);
pvlm_status pvlm_line_grow_finish(pvlm_ctx* ctx, pvlm_line_grow* grow);
pvlm_status pvlm_line_grow_scan(const pvlm_line_grow* grow, int scan, pvlm_line_grow_result* result);
pvlm_status pvlm_line_grow_destroy(pvlm_ctx* ctx, pvlm_line_grow* grow);

/* ---- motion compensation of the sweeps (N5) ---------------------------------------------------------------------------------------------
 * Velodyne::UndistortCloud(R_we, t_we) (sensors/Velodyne.cpp:1642-1674) for every scan of LidarOdometry::UndistortLidars
 * (lidar_mapping/LidarOdometry.cpp:189-263) in one call: point i of n moves by the share i / n of the motion from the sweep's start pose (R_wl, t_wl)
 * to its end pose (R_we, t_we) — rotation by Identity.slerp(i / n, q_se), translation (i / n) t_se.  xyzi: n points of stride_floats >= 4 floats
 * (x, y, z first; pcl::PointXYZI: 8), updated in place; rotations row-major 3x3, world <- sensor.  The caller picks the end pose (next scan's pose
 * through SlerpPose, ...) and clears the feature clouds as upstream does.                                                                    */
typedef struct pvlm_undistort_scan {
  float* xyzi;
  int n;
  int stride_floats;
  const double* R_wl; const double* t_wl;
  const double* R_we; const double* t_we;
} pvlm_undistort_scan;
pvlm_status pvlm_undistort_batch(pvlm_ctx* ctx, int n_scans, const pvlm_undistort_scan* scans);

/* ---- the fused LiDAR map (K29) -----------------------------------------------------------------------------------------------------------
 * The body of LidarOdometry::FuseLidar (lidar_mapping/LidarOdometry.cpp:323-348; CameraLidarOptimizer::FuseLidar has the same) for the scans the caller
 * selected: a point is kept unless range > max_range^2 or range < min_range^2, range = (double)((x*x + y*z) + z*z) in float (upstream's y*z kept;
 * NaN ranges are kept), and moved to the world frame, float(((m00 x + m01 y) + m02 z) + m03) in double per coordinate; intensity unchanged.
 * The result is the kept points in scan order, then point order, as 4 floats (x, y, z, intensity) each.  The selection of the scans (stride, valid
 * flags, reloads) is the caller's (host mirror: LidarOdometry::FuseLidar).
 * pvlm_fuse_scan: n points; x, y, z at xyz[i * stride_floats + 0..2], intensity at intensity[i * stride_floats] (pcl::PointXYZI: stride 8, intensity =
 * xyz + 4; a packed x y z i record: stride 4, intensity = xyz + 3); T_wl: 16 doubles, row-major world <- sensor (the last row is not read). */
typedef struct pvlm_fuse_scan {
  const float* xyz;
  const float* intensity;
  int n;
  int stride_floats;
  const double* T_wl;
} pvlm_fuse_scan;
/* Host clouds in, the caller's host buffer out (capacity points of 4 floats).  *n_out = points kept; per_scan_or_null[s] = those of scan s.  A capacity below
 * *n_out returns PVLM_ERR_ARG with *n_out (and the per-scan counts) set; points past capacity are not written.  Works through a bounded pinned window in pieces of
 * whole scans (the upload of one piece beside the kernels and the download of the one before); synchronous; PVLM_ERR_STATE inside a graph capture. */
pvlm_status pvlm_fuse_scans(pvlm_ctx* ctx, int n_scans, const pvlm_fuse_scan* scans, double min_range, double max_range, float* out_xyzi, long long capacity,
                            long long* n_out, long long* per_scan_or_null);
/* The same on device clouds: the descriptor array and the poses are host memory, xyz / intensity, d_out, d_n_out and d_per_scan_or_null (n_scans counts) device
 * memory; d_out must be 16-byte aligned (the points are written as float4; PVLM_ERR_ARG otherwise).  Queued on the context's stream without a host synchronisation: *d_n_out is the full kept count even when it exceeds capacity (points past capacity are
 * not written).  PVLM_ERR_STATE inside a graph capture. */
pvlm_status pvlm_fuse_scans_dev(pvlm_ctx* ctx, int n_scans, const pvlm_fuse_scan* device_clouds, double min_range, double max_range, float* d_out,
                                long long capacity, long long* d_n_out, long long* d_per_scan_or_null);

/* ---- the coloured LiDAR map (K30) --------------------------------------------------------------------------------------------------------
 * The colour stage of Texture::ColorizeLidarPointCloud (mvs/Texture.cpp:14-80) for the (scan, frame) pairs the caller selected (both poses valid): a point of the
 * scan (cloud_scan, LiDAR frame) is kept when distance = (double)((x*x + y*y) + z*z) in float is neither < min_dist^2 nor > max_dist^2 (NaN passes), its camera
 * point p = (T_cl (x, y, z, 1)).hnormalized() in double ((m0 x + m1 y) + m2 z) + m3 per row) projects through the double Equirectangular::CamToImage to
 * (round(u), round(v)) inside the image (std::round, then x86-64's conversion: NaN never lands on a pixel), and the pixel's OpenCV 8-bit HSV is not sky
 * (h 100..124, s 43..200, v 150..255).  The record is (x, y, z of the LiDAR-frame point, colour word): 4 x 4 bytes, the fourth the bits of
 * b | g << 8 | r << 16 | 255 << 24 (pcl::PointXYZRGB's rgb and the PCD data record).  Kept points in pair order, then point order.
 * pvlm_colorize_pair: n points, x y z at xyz[i * stride_floats + 0..2] (pcl::PointXYZI: stride 8); T_cl: 12 doubles, rows 0..2 of the rigid camera <- LiDAR
 * transform T_wc^-1 T_wl (its last row is taken as 0 0 0 1); bgr: rows x cols BGR8 pixels, row r at bgr + r * row_bytes (row_bytes >= 3 cols,
 * rows * row_bytes < 2^31). */
typedef struct pvlm_colorize_pair {
  const float* xyz;
  int n;
  int stride_floats;
  const double* T_cl;
  const unsigned char* bgr;
  int rows;
  int cols;
  long long row_bytes;
} pvlm_colorize_pair;
/* Host clouds and images in, the caller's host buffer out (capacity records).  *n_out = points kept; per_pair_or_null[s] = those of pair s.  A capacity below
 * *n_out returns PVLM_ERR_ARG with *n_out (and the per-pair counts) set; records past capacity are not written.  The images stay on the host: pieces of whole pairs
 * go through a bounded pinned window (clouds up, the pixel of every point projected on the device and brought down, the pixels' BGR gathered by host threads
 * and sent up, the HSV test and the compaction on the device); the next piece's upload and projection overlap this one's gather.  Synchronous;
 * PVLM_ERR_STATE inside a graph capture. */
pvlm_status pvlm_colorize_scans(pvlm_ctx* ctx, int n_pairs, const pvlm_colorize_pair* pairs, double min_dist, double max_dist, float* out_records,
                                long long capacity, long long* n_out, long long* per_pair_or_null);
/* The same on device clouds and images: the descriptor array and T_cl are host memory, xyz, bgr, d_out, d_n_out and d_per_pair_or_null (n_pairs counts) device
 * memory; d_out must be 16-byte aligned (PVLM_ERR_ARG otherwise).  Queued on the context's stream without a host synchronisation: *d_n_out is the full kept count
 * even when it exceeds capacity (records past capacity are not written).  PVLM_ERR_STATE inside a graph capture. */
pvlm_status pvlm_colorize_scans_dev(pvlm_ctx* ctx, int n_pairs, const pvlm_colorize_pair* device_pairs, double min_dist, double max_dist, float* d_out,
                                    long long capacity, long long* d_n_out, long long* d_per_pair_or_null);
/* Tests: the device's OpenCV 8-bit BGR -> HSV (hrange 180) of n host pixels, bgr and hsv_out n x 3 bytes. */
pvlm_status pvlm_colorize_debug_hsv(pvlm_ctx* ctx, long long n, const unsigned char* bgr, unsigned char* hsv_out);

#ifdef __cplusplus
}
#endif
#endif /* PVLM_H_ */
