/*
 * include/lmono_hip.h -- C ABI of the MI355X-native lmono per-scan hot path.
 *
 * The reference (bobocode/lmono, ROS-1 C++) has no FFI / plugin registry; its seams are ROS topics,
 * the Estimator call surface and the Ceres cost-function ABI.  Each entry point below
 * names the reference interface it stands in for.  All functions return 0 on success or a negative
 * LMONO_E* code, never throw, and are re-entrant per context.  Pointers suffixed _d are device (HBM)
 * pointers, _h host pointers.  No torch / HIP types appear in signatures (streams travel as void*).
 */
#ifndef LMONO_HIP_H
#define LMONO_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMONO_OK            0
#define LMONO_EINVAL       -1   /* bad argument                                            */
#define LMONO_ENODEV       -2   /* no usable gfx950 device / HIP runtime error              */
#define LMONO_ENOMEM       -3   /* device allocation failed                                 */
#define LMONO_ECAPACITY    -4   /* batch exceeds the capacity it was created with           */
#define LMONO_ESCAN        -5   /* a scan violated a kernel limit (see lmono_batch_status)  */

#define LMONO_MAX_RINGS     64
#define LMONO_RING_CAP      4096  /* max points of one ring after filtering                 */
#define LMONO_MAX_SHARP     (64 * 6 * 2)
#define LMONO_MAX_LESS_SHARP (64 * 6 * 20)
#define LMONO_MAX_FLAT      (64 * 6 * 4)

typedef struct lmono_ctx lmono_ctx;
typedef struct lmono_scan_batch lmono_scan_batch;

/* ---- context ---------------------------------------------------------------------------- */
lmono_ctx  *lmono_create(int device);           /* NULL when HIP / the device is unavailable */
void        lmono_destroy(lmono_ctx *);
const char *lmono_last_error(const lmono_ctx *);
int         lmono_set_stream(lmono_ctx *, void *hip_stream); /* hipStream_t; NULL = default  */
/* Run this context on a non-blocking stream the library creates (and destroys with the context).  No reference counterpart: the
 * reference runs marginalisation inline (Estimator.cc:1280-1470); the host mirror uses a second context on its own stream so that it
 * overlaps the next frame's solve.  A context is used by one host thread at a time; two contexts on two threads do not serialise
 * (the host-array entry points carve their scratch from a per-context arena and copy on the context stream only). */
int         lmono_use_own_stream(lmono_ctx *);
int         lmono_synchronize(lmono_ctx *);
/* Tuning / test switches of a context (no reference counterpart).  LMONO_OPT_CORR_TILE selects the laserOdometry correspondence
 * search: 3 (default) = flattened candidate sweeps over the (azimuth bin, scan line) index (k_corr_flat; needs no hash grid);
 * 0 = 32 lanes per feature point on a 1 m hash grid (k_correspond + k_grid_build: the round-1 search, compiled into the diagnostic
 * build liblmono_hip_diag.so only, where the two are checked against each other -- tests/diag_search_modes.py).  The product library
 * refuses every value but 3.  (Rounds 2-3 carried four more formulations -- LDS sector tiles, thread per feature, a sector-staged
 * flat search, one persistent workgroup per chain; all measured slower, profiles/r2/NOTES.md, profiles/r3/NOTES.md sections 2-3 --
 * they were removed in round 4 and live in the history at commit d914e8c.)                                                        */
#define LMONO_OPT_CORR_TILE 0
/* test hook: n > 0 makes the default search (mode 3) hand every n-th feature point to its fall-back kernel (k_correspond_list), which
 * then runs without hash grids; results must not change.  0 = off.                                                              */
#define LMONO_OPT_DEFER_EVERY 1
/* chain groups of lmono_odom_batch[_d]: G = 1 .. 8 groups of chains advance on G HIP streams side by side (results unchanged).
 * Default 4 (one per hardware queue); at most 3 for a context on a caller-created stream (the runtime keeps one queue for the null
 * stream); reduced until every group holds at least 32 chains, so a 1-chain call is ungrouped.                                */
#define LMONO_OPT_ODOM_STREAMS 2
/* lead-in of lmono_odom_batch[_d]'s chains: >= 0 = only the last N lead-in scan pairs of a chain use all feature points, the earlier
 * ones a quarter of them (a lead-in pair only produces the next pair's warm start); -1 (default) = every pair uses all of them.
 * An accuracy / speed knob like n_chains and lead: n_chains = 1 is unaffected.                                                  */
#define LMONO_OPT_LEAD_FULL 3
/* boundary validation of lmono_odom_batch[_d]'s chained schedule (n_chains > 1), in units of 1e-9: after the chains have run, the warm
 * start every chain used for its first owned scan pair (its own lead-in's estimate) is compared on the device with the increment the
 * strictly sequential schedule warm-starts from (the predecessor chain's last one): residual = max(|dq_i|, 0.1 |dt_i| / m).  Chains
 * above the tolerance are re-started from the sequential warm start and re-run until their increments agree with the stored ones
 * within it (everything behind stands), in rounds until no boundary is flagged; lmono_odom_boundary_report tells what happened.
 * Default 1000 (1e-6: 2e-6 rad, 1e-5 m); 0 = no validation (and no synchronisation inside lmono_odom_batch_d).                    */
#define LMONO_OPT_BOUNDARY_TOL 4
/* workgroups per window of lmono_ba_solve (the K = 1 / 2 / 4 / 8 workgroups of a window share its linearisations and candidate costs; the sums are formed
 * per 16-observation segment and added in segment order, so the result is the same bit for bit whatever K is): 0 (default) = as many as keep the
 * batch within half the device's compute units (hipDeviceProp_t::multiProcessorCount; on 256 CUs: 8 for up to 16 windows, 4 for up to 32, 2 for up to 64, else 1; at most 4
 * when the windows average fewer than 64 segments); 1, 2, 4, 8 = that many.  A cluster whose workgroups do not all become resident gives up (bounded polls) and
 * lmono_ba_batch_read solves the batch again with one workgroup per window: same bytes.  Takes effect at the next
 * lmono_ba_batch_create / _update of the context (the scratch is sized then).  (Slot 5 was round 3's LMONO_OPT_ODOM_PERSIST, removed in round 4.)   */
#define LMONO_OPT_BA_CLUSTER 5
/* lead-in seeding of lmono_odom_batch[_d]'s chains (slot 6: round 3's LMONO_OPT_CORR_SECT, removed since): 0 = every lead-in starts from the identity and
 * keeps its own estimates (the reference's initial para_q / para_t); 1 = after the first step of the pass the state of every chain that is still in its
 * lead-in becomes the component-wise median of the first results of chains c - 1, c, c + 1 (a constant-velocity prior across 1.8 s that rejects a first
 * pair gone wrong in clutter).  An accuracy / speed knob like lead: results are validated at the chain boundaries either way; n_chains = 1 is unaffected. */
#define LMONO_OPT_LEAD_SEED 6
#define LMONO_OPT_COUNT     7
int         lmono_set_option(lmono_ctx *, int key, int value);
int         lmono_get_option(lmono_ctx *, int key, int *value);     /* the configured value (option values may be negative) */
const char *lmono_version(void);

/* ---- LiDAR front end: A-LOAM scanRegistration::laserCloudHandler ------------------------ *
 * Reference interface: ROS node "ascanRegistration" subscribing /velodyne_points and
 * publishing /laser_cloud_{sharp,less_sharp,flat,less_flat} (source absent from the reference tree:
 * /root/reference/.gitmodules:1-3, README.md:54-60; behavioural spec SURVEY.md Appendix A.1).
 * A batch holds the device-resident working set of n independent scans.                      */
lmono_scan_batch *lmono_batch_create(lmono_ctx *, int n_scans_cap, int64_t total_points_cap);
void              lmono_batch_destroy(lmono_scan_batch *);

/* xyzi_d: [total][4] float32 (KITTI .bin layout) already resident in HBM; offsets_h: [n_scans+1]
 * point offsets of each scan.  n_lines in {16,32,64}; min_range = A-LOAM `minimum_range`.    */
int lmono_scanreg_batch(lmono_ctx *, lmono_scan_batch *, const float *xyzi_d, const int64_t *offsets_h,
                        int n_scans, int n_lines, float min_range);
/* Same with the scans in HOST memory (what the reference's node callback receives in a sensor_msgs/PointCloud2, or a
 * KITTI .bin file read from disk): the points are staged into a batch-owned HBM buffer on the context stream first.
 * This is the PCIe-inclusive entry; the resident-in-HBM one above is what bench.py times.                       */
int lmono_scanreg_batch_h(lmono_ctx *, lmono_scan_batch *, const float *xyzi_h, const int64_t *offsets_h,
                          int n_scans, int n_lines, float min_range);

/* Streamed input (PCIe-inclusive operation): lmono_batch_stage_h enqueues the H2D copy of a working set's points into the batch's own
 * staging buffer on the library's copy stream and returns at once (xyzi_h should be pinned: lmono_host_alloc, or hipHostRegister'ed by the
 * caller); lmono_scanreg_batch_staged makes the compute stream wait for that copy ON THE DEVICE and registers the staged scans.  With two
 * batches the copy of working set i + 1 runs under the compute of working set i; a batch's staging buffer is not overwritten before its
 * front end has read it.  No reference counterpart (the reference receives one message at a time in host memory).                    */
void *lmono_host_alloc(lmono_ctx *, size_t bytes);
void  lmono_host_free(lmono_ctx *, void *);
int lmono_batch_stage_h(lmono_ctx *, lmono_scan_batch *, const float *xyzi_h, int64_t total_points);
int lmono_scanreg_batch_staged(lmono_ctx *, lmono_scan_batch *, const int64_t *offsets_h, int n_scans, int n_lines, float min_range);

/* counts_h: [n_scans][6] = n_cloud, n_sharp, n_less_sharp, n_flat, n_less_flat, status.
 * status bits: 1 a ring holds more than LMONO_RING_CAP points (scan contributes no features); 2 a "last" cloud did not fit
 * its hash grid (too many points, a table page without a free slot, or a cell beyond +-1024 m: that table is empty, the
 * next scan finds no correspondences in it); 4 scan-line ids too disordered for the windowed walk and 16 a 1 m cell with
 * more than 32767 points (both: the generic, slower search path is used, results unchanged); 8 walk truncated.       */
int lmono_batch_counts(lmono_ctx *, lmono_scan_batch *, int32_t *counts_h);
/* which: 0 ring-sorted cloud, 1 sharp, 2 less_sharp, 3 flat, 4 less_flat.  out_h: [cap][4] float32.
 * Returns the number of points copied (>= 0) or a negative error.                               */
int lmono_batch_get_cloud(lmono_ctx *, lmono_scan_batch *, int scan, int which, float *out_h, int cap);
/* curvature (float32) and label (int32: 2 sharp, 1 less sharp, -1 flat, 0 other) of the sorted cloud.  The registration keeps no
 * curvature array (k_select computes what it needs per sector): with curv_h set, this call computes the scan's curvature on the
 * context stream into a buffer of its own and changes nothing that a later registration or odometry call reads. */
int lmono_batch_get_curvature(lmono_ctx *, lmono_scan_batch *, int scan, float *curv_h, int32_t *label_h, int cap);

/* ---- LiDAR odometry: A-LOAM laserOdometry main loop + lidarFactor.hpp + ceres::Solve ------- *
 * Reference interface: ROS node "alaserOdometry" (feature clouds in, /laser_odom_to_init out; spec
 * SURVEY.md Appendix A.2/A.3).  Runs scan-to-scan odometry over the scans of a registered batch.
 * The sequence is cut into n_chains contiguous ranges processed concurrently; a range starting at
 * scan s > 0 starts `lead` scans early from an identity warm start and discards its lead-in
 * (n_chains = 1, lead = 0 = the strictly sequential reference behaviour).
 * incr_h / poses_h (either may be NULL): [n_scans][7] = q(x,y,z,w), t of T(k-1 -> k) and of the
 * accumulated pose t_w += q_w * t, q_w = q_w * q.                                              */
int lmono_odom_batch(lmono_ctx *, lmono_scan_batch *, int n_chains, int lead, double *incr_h, double *poses_h);
/* Same, results stay on the device: incr_d, poses_d [n_scans][7] float64 (may be NULL).       */
int lmono_odom_batch_d(lmono_ctx *, lmono_scan_batch *, int n_chains, int lead, double *incr_d, double *poses_d);

/* What the boundary validation of the last lmono_odom_batch[_d] / lmono_odom_shard_* call on this batch did (LMONO_OPT_BOUNDARY_TOL).
 * resid_h [n_chains] (may be NULL): residual of every chain's warm start at the first check (entry 0: 0, or the shard's external
 * boundary); rerun_h [n_chains] (may be NULL): scan pairs re-run per chain.  No reference counterpart (the reference is sequential). */
typedef struct {
    int n_chains;
    int flagged;        /* boundaries above the tolerance, summed over the rounds                                   */
    int chains_rerun;   /* distinct chains re-started                                                              */
    int pairs_rerun;    /* scan pairs re-run by them                                                               */
    int rounds;         /* check + repair rounds (a repair that reaches its chain's end can flag the next boundary) */
    int unresolved;     /* boundaries still above the tolerance behind the last repair round (counted by one more check when the
                         * round cap n_chains + 1 ends the loop; 0 otherwise)                                       */
    double tol, max_resid, repair_ms;
} lmono_boundary_report;
int lmono_odom_boundary_report(lmono_ctx *, lmono_scan_batch *, lmono_boundary_report *rep, double *resid_h, int32_t *rerun_h, int cap);

/* Scan-range sharding over the GPUs of a node: the batch holds scans [first_owned - lead', n) of a longer sequence, the
 * first `first_owned` of them are the previous rank's (chain 0's lead-in; their increments are not produced).  lmono_odom_shard_d runs
 * the chains over the owned scans; after ONE all-gather of every rank's last increment (incr_d[n - 1]), lmono_odom_shard_validate
 * checks chain 0's warm start against the previous rank's last increment prev_incr_h[7] exactly like an inner boundary and repairs;
 * *changed_last = 1 when this rank's own last increment changed (the next rank must validate again).  incr_d [n][7] as above.
 * lmono_odom_shard_main_d is lmono_odom_shard_d WITHOUT the validation of the boundaries inside the rank: the caller exchanges the last
 * increments right after the main pass and lmono_odom_shard_validate then validates every boundary of the rank -- the external one too --
 * in one set of repair rounds (prev_incr_h = NULL on the rank that owns the sequence's first scan: inner boundaries only).               */
int lmono_odom_shard_d(lmono_ctx *, lmono_scan_batch *, int n_chains, int lead, int first_owned, double *incr_d);
int lmono_odom_shard_main_d(lmono_ctx *, lmono_scan_batch *, int n_chains, int lead, int first_owned, double *incr_d);
int lmono_odom_shard_validate(lmono_ctx *, lmono_scan_batch *, const double *prev_incr_h, double *incr_d, int *changed_last);

/* Online form: ONE scan per call, as the reference's nodes run (ROS callbacks laserCloudHandler -> laserOdometry at sensor rate; lmono
 * consumes the result per frame: mono_lidar_mapping/src/image_process/MeasurementManager.cc:17-24, config/kitti_config_00.yaml:7-8).
 * A stream keeps the previous scan's feature clouds and search index on the device ("last") and A-LOAM's para_q / para_t between calls
 * (SURVEY.md A.2): lmono_odom_step registers the new scan (scanRegistration), runs the scan pair (2 x [correspondences -> <= 4 LM
 * iterations]) warm-started from the previous increment and returns q_last_curr / t_last_curr and the accumulated q_w_curr / t_w_curr
 * -- the same numbers lmono_odom_batch(n_chains 1, lead 0) gives for the same scans, bit for bit.  xyzi: [n_points][4] float32, host
 * (on_device 0) or HBM (1).  use_warm_start != 0: q_last_curr / t_last_curr are read as the pair's warm start instead of the stream's
 * own.  info [8] (may be NULL): n_cloud, n_sharp, n_less_sharp, n_flat, n_less_flat, status, LM iterations (outer 0 << 8 | outer 1),
 * residual blocks of the last solve.  history >= 1 slots of scans are kept (the slots are reused cyclically).  Synchronous.         */
typedef struct lmono_odom_stream lmono_odom_stream;
lmono_odom_stream *lmono_odom_stream_create(lmono_ctx *, int max_points_per_scan, int n_lines, float min_range, int history);
void lmono_odom_stream_destroy(lmono_odom_stream *);
int lmono_odom_step(lmono_ctx *, lmono_odom_stream *, const float *xyzi, int n_points, int on_device, int use_warm_start,
                    double *q_last_curr, double *t_last_curr, double *q_w_curr, double *t_w_curr, int32_t *info);
/* the batch / scan index holding the stream's newest scan: for lmono_batch_get_cloud and lmono_mapper_process (laserMapping behind it) */
int lmono_odom_stream_scan(lmono_odom_stream *, lmono_scan_batch **batch, int *scan);

/* Debug/parity view of one odometry step: correspondences of outer iteration `outer` (0/1) for the scan
 * pair (scan-1, scan) evaluated at pose q,t: corr_h [n_sharp + n_flat][4] = (a, b, c, kind).       */
int lmono_odom_correspond(lmono_ctx *, lmono_scan_batch *, int scan, const double q[4], const double t[3],
                          int32_t *corr_h, int cap);

/* ---- lmono BA factors: batched ceres::CostFunction::Evaluate -------------------------------------------- *
 * Reference interfaces (paths under /root/reference/mono_lidar_mapping), one residual block per index:
 *   kind 0 LASER   LASERFactor ctor + Evaluate            include/factor/LaserFactor.h:29-100
 *          params[14] = pose_i, pose_j (x y z qx qy qz qw); consts[24] = L0_Ri, L0_Rj (3x3 row-major), L0_Pi, L0_Pj;
 *          info[36] = LASERFactor::sqrt_info (Estimator.cc:95); r[6]; J[84] = J_i[6x7], J_j[6x7]
 *   kind 1 MONO    MonoProjectionFactor::Evaluate          src/factor/MonoProjectionFactor.cc:40-174
 *          params[22] = ex, pose_i, pose_j, inv_depth; consts[4] = pt_i.xy, pt_j.xy (normalised image points);
 *          info[4] = MonoProjectionFactor::sqrt_info (Estimator.cc:94); r[2]; J[44] = J_ex, J_i, J_j [2x7 each], J_depth[2]
 *   kind 2 PRIOR   PriorFactor ctor + Evaluate             include/factor/PriorFactor.h:29-69
 *          params[7] = ex; consts[16] = 4x4 transform row-major; info[2] = PRIOR_T, PRIOR_R; r[6]; J[42]
 *   kind 3 REPROJ  ReprojectionFactor ctor + Evaluate      include/factor/ReprojectionFactor.h:16-78
 *          params[1] = inv_depth; consts[44] = pt_i.xy, pt_j.xy, Ri, Pi, Rj, Pj, EX(4x4); info[1] = FACTOR_WEIGHT; r[2]; J[2]
 * Jacobians follow the Ceres layout (row-major, global block size, 7th pose column zero) and reproduce the reference's
 * formulae literally, including their known non-analytic blocks.  J may be NULL (residuals only).   */
#define LMONO_FACTOR_LASER  0
#define LMONO_FACTOR_MONO   1
#define LMONO_FACTOR_PRIOR  2
#define LMONO_FACTOR_REPROJ 3
int lmono_factor_eval(lmono_ctx *, int kind, int count, const double *params_h, const double *consts_h,
                      const double *info_h, double *r_h, double *J_h);
int lmono_factor_eval_d(lmono_ctx *, int kind, int count, const double *params_d, const double *consts_d,
                        const double *info_d, double *r_d, double *J_d);
/* The same with ceres::CostFunction::Evaluate's per-block contract (LaserFactor.h:45, MonoProjectionFactor.cc:40: any jacobians[k]
 * may be NULL): block_mask [count] holds one byte per residual block, bit k set = the Jacobian of parameter block k is wanted
 * (LASER: pose_i, pose_j; MONO: ex, pose_i, pose_j, inv_depth; PRIOR: ex; REPROJ: inv_depth).  Blocks whose bit is clear are left
 * untouched in J; a zero byte is `jacobians == NULL` for that residual block.  block_mask NULL = every block.                     */
int lmono_factor_eval_blocks(lmono_ctx *, int kind, int count, const double *params_h, const double *consts_h,
                             const double *info_h, double *r_h, double *J_h, const unsigned char *block_mask_h);
int lmono_factor_eval_blocks_d(lmono_ctx *, int kind, int count, const double *params_d, const double *consts_d,
                               const double *info_d, double *r_d, double *J_d, const unsigned char *block_mask_d);

/* ---- lmono sliding-window BA: Estimator::optimization()'s solve, batched over independent windows ------------ *
 * Reference interface: Estimator::optimization() -> ceres::Solve(DENSE_SCHUR, DOGLEG, max_num_iterations = NUM_ITERATIONS)
 * (mono_lidar_mapping/src/image_process/Estimator.cc:1124-1305) over para_pose[11][7], para_ex[1][7],
 * para_depth_inv[F][1] (Estimator.h:255-257) with PriorFactor / LASERFactor / MonoProjectionFactor+CauchyLoss(1).
 * A window depends on its predecessor, so a batch holds windows of independent sequences.  All arrays are host
 * pointers; lmono_ba_batch_create copies them into HBM once, lmono_ba_solve runs one workgroup per window.
 * Supported maximum: LMONO_BA_MAX_FEATURES = 1664 inverse-depth blocks per window (the reference sizes para_depth_inv[10000],
 * Estimator.h:256; its tracker caps a frame at MAX_CNT = 150 tracks, FeatureTracker.cc:21, so the 11 frames of a window can hold at
 * most 1650 tracks, of which the ones tracked >= TRACK_CNT frames enter a solve -- 100-300 on the S2 streams, SURVEY.md section 8:
 * the bound is above anything the reference's own front end can produce).  Up to 448 features the per-feature vectors of the dogleg step
 * (scale, D, gs, gn, va, vb, H_ff, g_f: 8 doubles per feature) live in LDS beside the 72 x 72 reduced system; a batch with a larger
 * window runs a second instantiation of the kernels that keeps them in an L2 scratch (same arithmetic in the same order, slower per
 * iteration).  A window above the bound is refused with LMONO_ECAPACITY by lmono_ba_batch_create / _update (and by the per-track
 * calls: lmono_triangulate, lmono_depth_refine, lmono_outlier_scores, lmono_shift_depth*) -- nothing is truncated.               */
#define LMONO_BA_MAX_FEATURES 1664
typedef struct lmono_ba_batch lmono_ba_batch;
typedef struct {
    int n_windows;
    const int *feat_off;        /* [n_windows+1] features (inverse-depth blocks) of each window                     */
    const int *obs_off;         /* [n_windows+1] MonoProjectionFactor blocks of each window                         */
    const int *flags;           /* [n_windows][4] n_poses (= frame_count+1 <= 11), use_prior, ex_constant, use_mono   */
    const double *poses;        /* [n_windows][11][7] para_pose, x y z qx qy qz qw                                  */
    const double *ex;           /* [n_windows][7] para_ex                                                           */
    const double *inv_depth;    /* [feat_off[n]] para_depth_inv                                                     */
    const int *obs_feat;        /* [obs_off[n]] window-local feature index; blocks grouped by feature, ascending     */
    const int *obs_i, *obs_j;   /* anchor frame (start_frame) and observing frame of each block                     */
    const double *obs_pts;      /* [obs_off[n]][4] pt_i.xy, pt_j.xy (normalised image coordinates)                 */
    const double *laser_consts; /* [n_windows][10][24] L0_Ri, L0_Rj, L0_Pi, L0_Pj of consecutive frames             */
    const double *prior_T;      /* [n_windows][16] prior_trans = TLC[0] at solve time (Estimator.cc:1155-1160)       */
    const double *laser_info;   /* [36] LASERFactor::sqrt_info; mono_info [4] MonoProjectionFactor::sqrt_info;      */
    const double *mono_info;
    const double *prior_w;      /* [2] PRIOR_T, PRIOR_R                                                             */
} lmono_ba_desc;
lmono_ba_batch *lmono_ba_batch_create(lmono_ctx *, const lmono_ba_desc *);
void            lmono_ba_batch_destroy(lmono_ba_batch *);
/* load another problem into an existing batch, reusing its device arrays (Estimator::optimization() of the next frame: the
 * reference rebuilds its ceres::Problem per call, Estimator.cc:1017; here the frame loop allocates nothing in steady state)  */
int             lmono_ba_batch_update(lmono_ctx *, lmono_ba_batch *, const lmono_ba_desc *);
int lmono_ba_solve(lmono_ctx *, lmono_ba_batch *, int max_iterations);   /* asynchronous on the context stream    */
int lmono_ba_batch_reset(lmono_ctx *, lmono_ba_batch *);                 /* restore the state given at creation   */
/* poses_h [n][11][7], ex_h [n][7], inv_depth_h [F total], summary_h [n][6] = initial_cost, final_cost, iterations,
 * termination (0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE), successful steps, unsuccessful steps; any may be NULL */
int lmono_ba_batch_read(lmono_ctx *, lmono_ba_batch *, double *poses_h, double *ex_h, double *inv_depth_h, double *summary_h);
/* Diagnostic (no reference counterpart): a -DLMONO_BOUNDS build of the library checks every global access of k_ba_solve against the batch's allocation
 * and records the first one outside it instead of faulting: out4 = hits, source line of the first, its byte offset, its block.  The product build
 * answers LMONO_EINVAL.  tests/test_bounds_gpu.py builds the checked library into a scratch directory and runs the BA tests' problems through it.       */
int lmono_debug_bounds(lmono_ctx *, unsigned long long *out4);

/* ---- per-feature numerics of FeatureManager / Estimator (batched over windows; host arrays) ---------------- *
 * lmono_triangulate: FeatureManager::triangulate (src/image_process/FeatureManager.cc:75-255): linear multi-view
 *   triangulation of every track with estimated_depth <= 0 and >= track_cnt observations, then (refine_max_iter >= 0)
 *   the joint 1-D Ceres refinement with ReprojectionFactor + CauchyLoss(1) and setDepth()'s solve_flag (1 ok, 2 failed).
 *   Rs_h [n][11][9], Ps_h [n][11][3] (row-major), tlc_h [n][16]; track f of a window starts at start_frame[f] and owns the
 *   normalised points pts[obs_off[f] .. obs_off[f+1]) (first one = anchor); depth_h in/out.
 * lmono_outlier_scores: Estimator::outliersRejection's statistic FACTOR_WEIGHT * mean reprojection error
 *   (src/image_process/Estimator.cc:104-190); -1 for tracks shorter than track_cnt.
 * lmono_shift_depth: FeatureManager::removeBackShiftDepth as called by Estimator::slideWindowOld
 *   (FeatureManager.cc:540-590, Estimator.cc:744-763) for the tracks anchored at the dropped frame.
 * Malformed descriptors are refused on the host, before anything is uploaded or launched, with LMONO_EINVAL, a message in
 * lmono_last_error and the output arrays untouched (the kernels index Rs / Ps / pts by these arrays without a check of their own):
 *   - feat_off[0] != 0, or feat_off / obs_off not ascending (equal neighbours -- an empty window, a track without
 *     observations -- are fine), or obs_off[0] < 0;
 *   - start_frame[f] < 0, or start_frame[f] + nobs_f > 11 for a track with nobs_f > 0 observations (a window has 11 frames);
 *   - track_cnt < 1;
 *   - lmono_triangulate only: window_size outside 0..10, refine_max_iter > LMONO_FEAT_MAX_REFINE_ITER (the reference runs 50;
 *     refine_max_iter < 0 means "linear step only": solve_flag_h is then not written);
 *   - lmono_shift_depth: n < 0;  lmono_shift_depth_batch: track_off_h[0] != 0 or track_off_h not ascending.
 * Degenerate numerics are NOT refused, they are the reference's: lmono_outlier_scores of a track with a single observation (possible
 * only under track_cnt = 1) has no reprojection to average and returns the 0 / 0 of its mean, NaN; a depth <= 0 or a reprojected
 * z of 0 gives the score the division gives (finite, inf or NaN); lmono_shift_depth* returns -1 for every shifted z <= 0.    */
#define LMONO_FEAT_MAX_REFINE_ITER 1000
int lmono_triangulate(lmono_ctx *, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                      const int *start_frame_h, const int *obs_off_h, const double *pts_h, double *depth_h, int *solve_flag_h,
                      int track_cnt, int window_size, double factor_weight, int refine_max_iter);
int lmono_outlier_scores(lmono_ctx *, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                         const int *start_frame_h, const int *obs_off_h, const double *pts_h, const double *depth_h,
                         int track_cnt, double factor_weight, double *score_h);
int lmono_shift_depth(lmono_ctx *, const double *back_R0, const double *back_P0, const double *R1, const double *P1, const double *tlc,
                      int n, const double *pt_i_h, const double *depth_h, double *depth_out_h);
/* The same for n_windows independent Estimators in one call (EstimatorBatch: N sequences stepped in lock-step, SURVEY.md 8e "parallel only across
 * independent sequences"): frames_h [n_windows][40] = back_R0 (9), back_P0 (3), R1 (9), P1 (3), TLC (16, row-major 4 x 4) of each window;
 * track_off_h [n_windows + 1] offsets of the windows' tracks in pt_i_h / depth_h / depth_out_h.  A window's results are the single call's, bit for bit. */
int lmono_shift_depth_batch(lmono_ctx *, int n_windows, const double *frames_h, const int *track_off_h,
                            const double *pt_i_h, const double *depth_h, double *depth_out_h);

/* ---- marginalisation prior: Estimator::margin(), MARGIN_OLD branch first ------------------------------------ *
 * Reference interfaces: Estimator::margin (src/image_process/Estimator.cc:1307-1405), MarginalizationInfo::
 * {preMarginalize, marginalize} and Marginalization::Evaluate (src/factor/MarginalizationFactor.cc:109-131, :176-272,
 * :309-373).  Factors: LASERFactor(pose0, pose1) and one MonoProjectionFactor + CauchyLoss(1) per observation of the
 * tracks anchored at frame 0 (observations grouped by track; obs_j in 1..10; obs_pts = pt_i.xy, pt_j.xy -- the
 * reference passes the never-initialised right_pt here).  Kept blocks, in this order: ex, pose1 .. pose10 (n = 66).
 * lin_J_h [n_windows][66*66] = linearized_jacobians, lin_r_h [n_windows][66] = linearized_residuals (defined up to an
 * orthogonal row transform: compare J^T J and J^T r); status_h bit 0: H_mm needed the eps = 1e-8 cut; bit 1: the QL iteration of the eigen-decomposition hit its 60-sweep cap on an eigenvalue (never seen).
 * Refused with LMONO_EINVAL before any launch: offsets that do not start at 0 or descend, a null inv_depth / obs_feat / obs_j / obs_pts array
 * while the counts say it is not empty, observations not grouped by track, obs_j outside 1..10, the same frame twice in one track.
 * lmono_marg_evaluate: residual = r0 + J dx with x0_h / x_h [n_windows][11][7] (ex, pose1..pose10).               */
int lmono_marginalize(lmono_ctx *, int n_windows, const int *feat_off_h, const int *obs_off_h, const double *poses_h, const double *ex_h,
                      const double *inv_depth_h, const int *obs_feat_h, const int *obs_j_h, const double *obs_pts_h,
                      const double *laser01_h, const double *laser_info_h, const double *mono_info_h,
                      double *lin_J_h, double *lin_r_h, int *status_h);
int lmono_marg_evaluate(lmono_ctx *, int n_windows, const double *lin_J_h, const double *lin_r_h, const double *x0_h, const double *x_h,
                        double *residual_h);
/* The MARGIN_SECOND_NEW branch of Estimator::margin() (Estimator.cc:1406-1470): the only factor is the previous prior itself
 * (`Marginalization(last_marginalization_info)`, MarginalizationFactor.cc:300-373) over its n_blocks parameter blocks (7 doubles
 * each, 6 local; <= 11), evaluated at the current values x_h [n_windows][n_blocks][7] (linearisation point x0_h), and the block
 * drop_block (the one aliasing para_pose[WINDOW_SIZE - 1]) is eliminated: H = J^T J, b = J^T r, eigen pseudo-inverse of the 6x6
 * H_mm with the eps = 1e-8 cut, Schur complement, second eigen-decomposition.  lin_J_h [n_windows][n0*n0], lin_r_h [n_windows][n0],
 * n0 = 6 n_blocks; outputs over the kept blocks in their old order: lin_J_out_h [n_windows][n*n], lin_r_out_h [n_windows][n],
 * n = n0 - 6; the new linearisation point is x_h without the dropped block.  status_h bit 0: H_mm needed the eps cut.          */
int lmono_marg_second_new(lmono_ctx *, int n_windows, int n_blocks, int drop_block, const double *lin_J_h, const double *lin_r_h,
                          const double *x0_h, const double *x_h, double *lin_J_out_h, double *lin_r_out_h, int *status_h);

/* ---- laserMapping, optimisation step -------------------------------------------------------------------
 * Replaces the `for iterCount < 2 { 5-NN in the corner / surf map kd-trees; PCA line test -> LidarEdgeFactor; 5-point
 * plane fit -> LidarPlaneNormFactor; ceres::Solve }` block of A-LOAM laserMapping.cpp process() (source absent from the
 * reference tree; behavioural spec SURVEY.md Appendix A.4), batched over n_streams independent sequences.
 * *_map_h: the map clouds of each stream's 5 x 5 x 3 cube neighbourhood, *_stack_h: its voxel-filtered scan clouds
 * ([total][4] float32 x y z intensity, host memory; *_off: [n_streams + 1] point offsets).  pose_qt: [n_streams][7]
 * q_w_curr (x y z w), t_w_curr -- initial guess in, refined pose out.  stats (optional): [n_streams][8] = edge blocks of
 * the two outer iterations, plane blocks of the two, LM iterations of the two, then the device time of the whole batch in
 * microseconds: grid build, optimisation (2 x [correspond + solve]).  nn_out (optional):
 * [total stack points][5] neighbour indices of the last outer iteration (corner points first; -1 = no residual block).
 * The cube-map bookkeeping and the voxel filters of process() are not behind this ABI yet.                            */
int lmono_map_refine(lmono_ctx *, int n_streams,
                     const float *corner_map_h, const int64_t *corner_map_off, const float *surf_map_h, const int64_t *surf_map_off,
                     const float *corner_stack_h, const int64_t *corner_stack_off, const float *surf_stack_h, const int64_t *surf_stack_off,
                     double *pose_qt, int32_t *stats, int32_t *nn_out);

/* pcl::VoxelGrid (cubic leaf, every field averaged) on n_clouds independent clouds in one call: laserMapping's
 * downSizeFilterCorner / downSizeFilterSurf on the scan clouds and on the cubes of the neighbourhood (A-LOAM
 * laserMapping.cpp process()).  xyzi_h: [total][4] float32, off: [n_clouds + 1], leaf_h:
 * [n_clouds] leaf size in metres (<= 65536 points per cloud).  out_h: capacity total points; out_off: [n_clouds + 1]
 * offsets of the filtered clouds (centroids in ascending cell index, the points of a cell summed in index order).  */
int lmono_voxel_filter(lmono_ctx *, int n_clouds, const float *xyzi_h, const int64_t *off, const float *leaf_h,
                       float *out_h, int64_t *out_off);

/* laserMapping with a device-resident map: the 21 x 21 x 11 array of 50 m cubes of laserMapping.cpp (laserCloudCornerArray /
 * laserCloudSurfArray) lives in HBM, the library keeps only (offset, count) per cube on the host.  One call = one
 * process() of the node for scan `scan` of a registered batch (its less-sharp / less-flat clouds are read in place):
 * transformAssociateToMap, cube shifts, VoxelGrid of the scan clouds (mapping_line_resolution / _plane_resolution),
 * the optimisation block, transformUpdate, insertion of the scan into the cubes and re-filtering of the 5 x 5 x 3
 * neighbourhood.  q_wodom / t_wodom: laserOdometry's pose of the scan; q_w_curr / t_w_curr: aft_mapped_to_init.
 * stats (optional, [8]): edge blocks of the two outer iterations, plane blocks, LM iterations, then two sizes (for traffic
 * accounting): map points of the 5 x 5 x 3 neighbourhood handed to the optimisation, points of the cubes a map update rebuilt.
 * lmono_mapper_process keeps the (offset, count) table of the cubes ON THE DEVICE and plans the map update there: the call enqueues
 * the whole frame, waits once for the refined pose and returns; the scan joins the map behind the return (stream order: the next
 * call, lmono_mapper_cube and lmono_mapper_reset see the finished map).  Consequences for the caller: stats[7] is the PREVIOUS
 * frame's update, and an update the device had to refuse (LMONO_ECAPACITY: more than 65536 points in a cube, workspace or arena
 * exhausted) is reported by the following calls on the mapper until lmono_mapper_reset -- that update did not touch the map.
 * lmono_mapper_process_batch keeps the table on the host (one planning pass for all streams, two waits per frame); a mapper may be
 * used through both, the table is converted on entry.
 * A-LOAM laserMapping.cpp process(), source absent from the reference tree.          */
typedef struct lmono_mapper lmono_mapper;
lmono_mapper *lmono_mapper_create(lmono_ctx *, float line_res, float plane_res);      /* HDL-64 launch file: 0.4, 0.8 */
void          lmono_mapper_destroy(lmono_mapper *);
int           lmono_mapper_reset(lmono_ctx *, lmono_mapper *);                        /* empty map, identity correction */
int lmono_mapper_process(lmono_ctx *, lmono_mapper *, lmono_scan_batch *, int scan, const double q_wodom[4], const double t_wodom[3],
                         double q_w_curr[4], double t_w_curr[3], int32_t *stats);
/* n independent streams advanced by one frame each, every phase one launch for all of them: mappers[n] (distinct),
 * batches[n], scans[n], q_wodom [n][4], t_wodom [n][3] -> q_w_curr [n][4], t_w_curr [n][3], stats [n][8] (optional) */
int lmono_mapper_process_batch(lmono_ctx *, int n, lmono_mapper *const *mappers, lmono_scan_batch *const *batches, const int *scans,
                               const double *q_wodom, const double *t_wodom, double *q_w_curr, double *t_w_curr, int32_t *stats);
/* cube (i, j, k) of the corner (which = 0) / surf (1) array: returns its size; copies the points when out_h != NULL */
int lmono_mapper_cube(lmono_ctx *, lmono_mapper *, int which, int i, int j, int k, float *out_h, int cap);

/* ---- colour projection of the map builder ------------------------------------------------------------
 * Replaces MapBuilder::associateToMap + MapBuilder::depthFill (mono_lidar_mapping/src/map_builder/Map_Builder.cc:213-403)
 * and the accumulation of MapBuilder::processMapping (:8-90): a LiDAR scan is moved into the camera frame (the
 * pcl::transformPointCloud of map_build_node.cc:216-225, passed as `transform`), projected with camodocal's pinhole model
 * (camera_models/src/camera_models/PinholeCamera.cc:450-545), splatted into an 8-bit depth image (100 - z), hole-filled
 * (dilate / close / dilate 7 + fill / median 5 / bilateral or Gaussian), and every pixel with 0 < depth < 70 m is lifted
 * back to a coloured 3-D point, in row-major pixel order, in the camera frame (topic rgb_points) and in the world frame
 * (q_wc, t_wc = the Q, T arguments of associateToMap), the latter appended to the device-resident rgb_map.
 * The display products (HSV overlay :244, JET heat map :255) are not produced.                                          */
typedef struct {
    int width, height;                       /* image size (config image_width / image_height)                         */
    double fx, fy, cx, cy, k1, k2, p1, p2;   /* PINHOLE projection_parameters / distortion_parameters of the cam yaml   */
    int kernel_size;                         /* kernel_size (odd, <= 11)                                                */
    int kernel_type;                         /* kernel_type: 0 "FULL" (rect), 1 "CROSS", 2 anything else (ellipse)       */
    int blur_type;                           /* blur_type: 0 "bilateral", 1 anything else (Gaussian)                     */
} lmono_camera;
typedef struct { float x, y, z; uint32_t bgra; } lmono_point_rgb;   /* pcl::PointXYZRGB payload: b | g << 8 | r << 16 | 255 << 24 */
typedef struct lmono_map_builder lmono_map_builder;
/* max_cloud_points: largest scan of the host-buffer entry; map_capacity_points: capacity of rgb_map (>= width * height) */
lmono_map_builder *lmono_map_builder_create(lmono_ctx *, const lmono_camera *, int max_cloud_points, int64_t map_capacity_points);
void               lmono_map_builder_destroy(lmono_map_builder *);
/* One associateToMap: xyzi_h [n_points][4] float32 scan (LiDAR frame), transform: row-major 4 x 4 LiDAR -> camera,
 * bgr_h: [height][width][3] uint8 (cv::Mat BGR8), q_wc (x y z w) / t_wc: camera pose.  n_out: size of the coloured cloud. */
int lmono_associate_to_map(lmono_ctx *, lmono_map_builder *, const float *xyzi_h, int n_points, const double transform[16],
                           const uint8_t *bgr_h, const double q_wc[4], const double t_wc[3], int *n_out);
/* n_streams independent map builders advanced by one frame each, scans and images already resident in HBM (xyzi_d[s],
 * bgr_d[s] device pointers; transforms [n][16], q_wc [n][4], t_wc [n][3], n_out [n] host arrays); four launches in all. */
int lmono_associate_to_map_batch(lmono_ctx *, int n_streams, lmono_map_builder *const *mbs, const float *const *xyzi_d, const int *n_points,
                                 const double *transforms, const uint8_t *const *bgr_d, const double *q_wc, const double *t_wc, int *n_out);
int lmono_map_builder_depth(lmono_ctx *, lmono_map_builder *, uint8_t *depth_h);       /* filled depth map of the last frame */
/* coloured cloud of the last frame: which = 0 camera frame, 1 world frame; returns its size (copies when out_h != NULL)  */
int lmono_map_builder_cloud(lmono_ctx *, lmono_map_builder *, int which, lmono_point_rgb *out_h, int cap);
int64_t lmono_map_builder_map(lmono_ctx *, lmono_map_builder *, lmono_point_rgb *out_h, int64_t cap);   /* rgb_map; returns its size */
int lmono_map_builder_clear(lmono_ctx *, lmono_map_builder *);                         /* rgb_map->clear()                    */

/* ---- voxel-grid global colour map -------------------------------------------------------------------------
 * The pcl::VoxelGrid<pcl::PointXYZRGB> at a 0.1 m leaf that MapBuilder::processMapping carries commented out
 * (mono_lidar_mapping/src/map_builder/Map_Builder.cc:82-98): the filter the reference left commented out; a definition of this
 * project (16-bit fixed-point in-cell offsets summed as integers, 64-bit cell keys with no bounding box, output in ascending key order:
 * z-major, then y, then x).  A device-resident hash table bounded by the number of occupied voxels; its content is the same bytes
 * for every insertion order, split and batch.  Points with a non-finite coordinate or a cell index outside -2^20 .. 2^20 - 1 are
 * rejected and counted.
 * leaf finite and > 0, 1 <= max_voxels <= 2^30 (else NULL + lmono_last_error).  stats (optional) [4] per map: points inserted, points
 * rejected, voxels new in this call, voxels in the map afterwards.  An insert that needs more than max_voxels voxels returns
 * LMONO_ECAPACITY and leaves nothing of that call in the map; from then on the map is full: every insert returns LMONO_ECAPACITY
 * until lmono_voxel_map_clear (size / read / cells keep working), an insert of n == 0 points included: the full map wins.  At most
 * 2^30 points per call; on a map that is not full n == 0 is a successful no-op with no launch.  A map keeps this fixed size unless it
 * is told to grow (lmono_voxel_map_set_growth) or is rebuilt (lmono_voxel_map_reserve, which also makes a full map usable again without
 * losing its content); both are below. */
typedef struct lmono_voxel_map lmono_voxel_map;
lmono_voxel_map *lmono_voxel_map_create(lmono_ctx *, float leaf, int64_t max_voxels);
void             lmono_voxel_map_destroy(lmono_voxel_map *);
int              lmono_voxel_map_clear(lmono_ctx *, lmono_voxel_map *);
int              lmono_voxel_map_insert(lmono_ctx *, lmono_voxel_map *, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats);
int              lmono_voxel_map_insert_d(lmono_ctx *, lmono_voxel_map *, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats);
/* n distinct maps each take the world-frame cloud of the last frame of one of n distinct builders, straight from the builder's
 * device memory; two launches in all.  LMONO_EINVAL when a builder's last world cloud is no longer in rgb_map (as
 * lmono_map_builder_cloud(which = 1)); a builder with an empty last frame contributes nothing.  A stream that does not fit is refused
 * as above (LMONO_ECAPACITY); the other streams of the call are inserted.  If one of the maps is full already, the whole call is refused
 * with LMONO_ECAPACITY before any launch and no stream is inserted. */
int              lmono_voxel_map_insert_frames(lmono_ctx *, int n, lmono_voxel_map *const *maps, lmono_map_builder *const *mbs, int64_t *stats);
int64_t          lmono_voxel_map_size(lmono_ctx *, lmono_voxel_map *);
/* one point per voxel in ascending key order; returns the voxel count (copies when out_h != NULL) */
int64_t          lmono_voxel_map_read(lmono_ctx *, lmono_voxel_map *, lmono_point_rgb *out_h, int64_t cap);
/* diagnostic view: keys ascending, counts, sums [n][6] (offsets x y z in 2^-16 leaf, colour r g b); any output may be NULL.  counts are
 * reported modulo 2^32 (the table's are 64-bit): composed counts above that are out of this view's scope */
int64_t          lmono_voxel_map_cells(lmono_ctx *, lmono_voxel_map *, uint64_t *keys_h, uint32_t *counts_h, uint64_t *sums_h, int64_t cap);
int              lmono_voxel_map_tile(void);   /* points a workgroup of the insert sums on chip (tests place point counts around it) */
/* Compose: fold n_src voxel maps, each moved by a rigid transform (row-major 3 x 4 doubles, applied as given), into
 * dst.  Every occupied source voxel goes where its output point (what read returns) lands after the transform, with its count as weight,
 * count * offset as offset sums and its own colour sums; all integers, so dst holds the same bytes for every order and split of the
 * sources, and is an ordinary voxel map afterwards (it takes inserts and can be a source).  Sources are not modified; their leaves and
 * dst's may differ.  stats (optional) [6]: source voxels moved, source voxels rejected (moved point non-finite or outside the cell range),
 * points moved (sum of counts), points rejected, voxels new in dst, voxels in dst afterwards.  LMONO_EINVAL before any launch: a NULL or
 * foreign handle, dst among srcs, a source named twice, a non-finite transform entry, n_src < 0 (or > 65535, or more than 2^30 source
 * voxels).  A call that needs more than max_voxels voxels returns LMONO_ECAPACITY, leaves nothing of ANY source in dst (one destination:
 * all or nothing) and dst full until cleared, exactly as an insert; stats are then 0 0 0 0 0 and the size before the call.  n_src == 0
 * or only empty sources: a successful no-op with no launch, unless dst is full (LMONO_ECAPACITY: the full map wins). */
int              lmono_voxel_map_compose(lmono_ctx *, lmono_voxel_map *dst, int n_src, lmono_voxel_map *const *srcs,
                                         const double *transforms /* [n_src][12] */, int64_t *stats /* optional [6] */);
/* A live map changes size.  reserve rebuilds map s of n distinct maps for max_voxels[s] voxels -- more, fewer or as many
 * as it has room for now, max(size, 1) <= max_voxels[s] <= 2^30 -- with its content unchanged, byte for byte: all new tables are
 * allocated first, then one clear launch and one launch that moves the occupied records serve all n maps (an empty map needs no move),
 * and the old tables are released only when every new one has been checked; ends synchronised.  While it runs the old and the new tables
 * exist side by side: that sum is the call's high-water mark.  A map that was full is no longer: what refused calls left behind is
 * dropped, so exactly max_voxels[s] voxels fit again; reserve with the current max_voxels is the way on after a refused insert without
 * clear.  LMONO_EINVAL before any launch or allocation, no map changed: n <= 0, a NULL or foreign handle, a map named twice, a value
 * below the map's size (or 1) or above 2^30.  LMONO_ENOMEM when a new table cannot be allocated, LMONO_ENODEV when a rebuilt table does
 * not hold exactly the map's voxels (table inconsistent): no map changed either.
 * set_growth: limit_voxels == 0 (the default) keeps the size fixed; otherwise max_voxels <= limit_voxels <= 2^30 (else LMONO_EINVAL),
 * and insert, insert_d, insert_frames, insert_filtered and compose (its dst) grow the map instead of refusing: the maps of the refused
 * streams are rebuilt for min(limit, 2 * max_voxels) as by reserve and the call is repeated for those streams only, until each fits or
 * stands at its limit.  The content and the stats are those of a fixed map that was large enough, and the capacity afterwards is the
 * smallest of max_voxels, min(limit, 2 max_voxels), min(limit, 4 max_voxels), ... that holds the voxels.  A stream that does not fit at
 * the limit is refused as above (LMONO_ECAPACITY, nothing inserted, map full at the limit); if a new table cannot be allocated the call
 * returns LMONO_ENOMEM with that map full, and a later reserve repairs it.  The limit bounds this automatic growth only: reserve may go
 * above it, and the map then never grows by itself.
 * capacity: out = max_voxels, slots of the table (64 B each), growth limit (0: fixed), tables replaced so far (by reserve or growth). */
int              lmono_voxel_map_reserve(lmono_ctx *, int n, lmono_voxel_map *const *maps, const int64_t *max_voxels);
int              lmono_voxel_map_set_growth(lmono_ctx *, lmono_voxel_map *, int64_t limit_voxels);
int              lmono_voxel_map_capacity(lmono_ctx *, lmono_voxel_map *, int64_t out[4]);

/* ---- statistical outlier removal in front of the voxel map ---------------------------------------------------
 * The pcl::StatisticalOutlierRemoval<pcl::PointXYZRGB> with setMeanK(100) / setStddevMulThresh(1.0) that MapBuilder::processMapping
 * carries commented out in front of its voxel grid (mono_lidar_mapping/src/map_builder/Map_Builder.cc:24-29), as a device-resident
 * filter between the map builder and the voxel map.  A definition of this project (lmono_amd/csrc/sor.hpp): the score of a point is
 * the sum of the distances to its mean_k nearest neighbours in units of 2^-16 m, an exact integer; a point with fewer than mean_k
 * neighbours within rho = (max_rings - 0.25) cell is isolated and removed without entering the statistics (PCL would look as far as
 * it must); a scored point is kept iff score <= mean + stddev_mul * sample standard deviation of the scores.  Points the voxel map
 * would reject at leaf = cell (non-finite, cell index outside -2^20 .. 2^20 - 1) are rejected: counted, never neighbours, never kept.
 * The result is a pure function of the set of input points; the output is the kept points in input order, payload untouched.
 * create: 1 <= max_points <= 2^28, 1 <= mean_k <= 128, stddev_mul finite, cell finite and > 0, 1 <= max_rings <= 64 and
 * (max_rings - 0.25) cell <= 256 (else NULL + lmono_last_error).  stats (optional) [8] per stream: points in, rejected, isolated,
 * scored (M), kept, A = sum of scores, Bhi, Blo = high and low 32-bit halves of the squared scores, summed.  n > max_points returns
 * LMONO_ECAPACITY before any launch; n == 0 is a successful empty result with no launch.  Every call replaces the filter's last result. */
typedef struct lmono_sor lmono_sor;
lmono_sor *lmono_sor_create(lmono_ctx *, int64_t max_points, int mean_k, double stddev_mul, float cell, int max_rings);
void       lmono_sor_destroy(lmono_sor *);
int        lmono_sor_filter(lmono_ctx *, lmono_sor *, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats);
int        lmono_sor_filter_d(lmono_ctx *, lmono_sor *, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats);
/* n distinct filters each take the world-frame cloud of the last frame of one of n distinct builders, straight from the builder's
 * device memory; one launch per phase for all streams.  LMONO_EINVAL when a builder's last world cloud is no longer in rgb_map; a
 * builder with an empty last frame gives an empty result.  A stream's bytes do not depend on the batch it travels in. */
int        lmono_sor_filter_frames(lmono_ctx *, int n, lmono_sor *const *sors, lmono_map_builder *const *mbs, int64_t *stats);
/* the kept points of the last call in input order; returns their count (copies when out_h != NULL) */
int64_t    lmono_sor_cloud(lmono_ctx *, lmono_sor *, lmono_point_rgb *out_h, int64_t cap);
/* diagnostic view of the last call, per input point: keep flag and score (0xffffffff = isolated or rejected); returns the point count */
int64_t    lmono_sor_scores(lmono_ctx *, lmono_sor *, uint8_t *keep_h, uint32_t *v_h, int64_t cap);
int        lmono_sor_threshold(lmono_ctx *, lmono_sor *, double out[3]);            /* mean, sqrt(var), thr in v units */
/* measurement view of the last call: out[0] rings scanned, summed over the valid points; out[1] points scored by the radix select */
int        lmono_sor_diag(lmono_ctx *, lmono_sor *, int64_t out[2]);
/* n distinct maps each fold in the last output of one of n distinct filters, from device memory: the two insert launches and the
 * capacity rules of lmono_voxel_map_insert_frames, unchanged (stats [4] per map as there). */
int        lmono_voxel_map_insert_filtered(lmono_ctx *, int n, lmono_voxel_map *const *maps, lmono_sor *const *sors, int64_t *stats);

/* ---- map builder: point-to-point ICP against a target cloud ------------------------------------------------
 * The pcl::IterativeClosestPoint with setMaxCorrespondenceDistance(0.5) / setMaximumIterations(50) / setTransformationEpsilon(1e-8) /
 * setEuclideanFitnessEpsilon(1) that MapBuilder::processMapping carries commented out between its outlier removal and its voxel grid
 * (mono_lidar_mapping/src/map_builder/Map_Builder.cc:31-59), as a device-resident stage between the outlier filter and the voxel map.
 * A definition of this project (lmono_amd/csrc/icp.hpp): every source point is paired with its nearest target point (ties by x, y, z)
 * if that lies within max_corr; the pairs enter a closed-form rigid fit (Horn) through exact integer sums in 2^-16 m fixed point about
 * the middle of the target's bounding box, so the result is a pure function of the SET of target points and of the source points: the
 * same bytes for every point order, grid tuning (cell, max_rings), batch and launch schedule.  Parity with PCL is unpinned.
 * eps: the run ends with status 0 when both the squared change of the translation and of the rotation matrix fall below it;
 * mse_eps (0: off): status 2 when the mean squared distance changes by less between two iterations; status 1: max_iter reached;
 * status 3: fewer than 3 pairs (the state is kept).  cell and max_rings tune the search grid and need (max_rings - 0.25) cell >= max_corr.
 * stats [8] per stream: source points, source points not usable (non-finite or 2048 m or more from the origin on an axis), target
 * points, target points rejected, iterations run, status, pairs and E = sum of squared distances in units of 2^-24 m^2 of the last
 * iteration.  n > max returns LMONO_ECAPACITY before any launch; n == 0 is a successful empty result with no launch; an align before
 * any set_target returns LMONO_EINVAL.  Every align replaces the aligner's last result. */
typedef struct lmono_icp lmono_icp;
lmono_icp *lmono_icp_create(lmono_ctx *, int64_t max_source_points, int64_t max_target_points, float max_corr, int max_iter, double eps, double mse_eps,
                            float cell, int max_rings);
void       lmono_icp_destroy(lmono_icp *);
/* the default cell for max_corr at max_rings = 2: the smallest float32 h >= max_corr / 1.75f with (2 - 0.25) h >= max_corr in float32 */
float      lmono_icp_default_cell(float max_corr);
/* the initial guess, row-major 3 x 4 (NULL: identity), applied to every source point before the first iteration and composed into the result */
int        lmono_icp_set_guess(lmono_ctx *, lmono_icp *, const double g[12]);
/* pairs of step and solve launches between two reads of the streams' done words (default 2); the result does not depend on it */
int        lmono_icp_set_poll_interval(lmono_ctx *, lmono_icp *, int pairs);
/* the target: built once, it serves every align until the next set_target*.  _map: one point per occupied voxel, what lmono_voxel_map_read
 * gives, without a host copy (frame-to-map).  _aligned: the aligned cloud of the last align (frame-to-frame, the reference's "last cloud"). */
int        lmono_icp_set_target(lmono_ctx *, lmono_icp *, const lmono_point_rgb *pts_h, int64_t n);
int        lmono_icp_set_target_d(lmono_ctx *, lmono_icp *, const lmono_point_rgb *pts_d, int64_t n);
int        lmono_icp_set_target_map(lmono_ctx *, lmono_icp *, lmono_voxel_map *);
int        lmono_icp_set_target_aligned(lmono_ctx *, lmono_icp *);
int        lmono_icp_align(lmono_ctx *, lmono_icp *, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats);
int        lmono_icp_align_d(lmono_ctx *, lmono_icp *, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats);
/* n distinct aligners each take the world-frame cloud of the last frame of one of n distinct builders, or the last output of one of n
 * distinct outlier filters, straight from device memory; one launch per phase for all streams.  A stream's bytes do not depend on the
 * batch it travels in. */
int        lmono_icp_align_frames(lmono_ctx *, int n, lmono_icp *const *icps, lmono_map_builder *const *mbs, int64_t *stats);
int        lmono_icp_align_filtered(lmono_ctx *, int n, lmono_icp *const *icps, lmono_sor *const *sors, int64_t *stats);
/* the last align: its transform (row-major 3 x 4, what lmono_voxel_map_compose takes: guess included), every input point in input order
 * moved by it (payload untouched), (pairs, E) of every iteration that ran, and the last iteration's squared distance per source point
 * (+inf: unmatched).  cloud, history and distances return the count (and copy when the pointer is not NULL). */
int        lmono_icp_transform(lmono_ctx *, lmono_icp *, double out[12]);
int64_t    lmono_icp_cloud(lmono_ctx *, lmono_icp *, lmono_point_rgb *out_h, int64_t cap);
int64_t    lmono_icp_history(lmono_ctx *, lmono_icp *, int64_t *n_e_h, int64_t cap);
int64_t    lmono_icp_distances(lmono_ctx *, lmono_icp *, float *d2_h, int64_t cap);
/* n distinct maps each fold in the aligned cloud of one of n distinct aligners, from device memory: the two insert launches and the
 * capacity rules of lmono_voxel_map_insert_frames, unchanged (stats [4] per map as there). */
int        lmono_voxel_map_insert_aligned(lmono_ctx *, int n, lmono_voxel_map *const *maps, lmono_icp *const *icps, int64_t *stats);

/* ---- map builder: surface normals and curvature of a cloud -------------------------------------------------
 * The pcl::NormalEstimation with setRadiusSearch(0.05) on both clouds that opens MapBuilder::alignmentToMap, the coarse map-to-map
 * alignment the reference carries commented out (mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210); every later stage of that
 * function (SIFT keypoints, FPFH, the sample-consensus initial alignment) consumes these normals; of those the FPFH descriptors are
 * provided (lmono_fpfh_*, below) and the sample-consensus initial alignment (lmono_sacia_*, below), the SIFT keypoints are not yet.
 * A definition of this project (lmono_amd/csrc/normals.hpp): the neighbours of a point are all valid points, itself and duplicates
 * included, within radius of it (d2 <= radius^2 in float32); their offsets from the point in 2^-16 m fixed point about the middle of
 * the cloud's bounding box give exact integer sums; the scatter matrix of those sums is diagonalised in fp64 (cyclic Jacobi, 8 sweeps);
 * the normal is the unit eigenvector of the smallest eigenvalue, curvature = that eigenvalue over the trace (0 for a zero trace).  The
 * normal faces the viewpoint; without one, or exactly edge-on, its component of largest magnitude is positive.  A record is a pure
 * function of the SET of points and of the point: the same bytes for every point order, grid tuning (cell, max_rings) and batch.
 * Parity with PCL is unpinned.  Limits: max_points <= 2^26, 0 < radius <= 4, min_neighbours >= 3, (max_rings - 0.25) cell >= radius.
 * A point that is non-finite or 2048 m or more from the origin on an axis is rejected: never a neighbour, count 0.  A rejected point
 * and a point with fewer than min_neighbours neighbours get four NaNs (0x7fc00000).
 * stats [8] per stream: points in, rejected, with a normal, without (too few neighbours), sum of the neighbour counts, largest
 * neighbour count, 0, 0.  n > max_points returns LMONO_ECAPACITY before any launch; n == 0 is a successful empty result with no
 * launch.  Every compute replaces the handle's last result. */
typedef struct lmono_normals lmono_normals;
typedef struct { float nx, ny, nz, curvature; } lmono_normal;
lmono_normals *lmono_normals_create(lmono_ctx *, int64_t max_points, float radius, int min_neighbours, float cell, int max_rings);
void       lmono_normals_destroy(lmono_normals *);
/* the default cell for radius at max_rings = 2: the smallest float32 h >= radius / 1.75f with (2 - 0.25) h >= radius in float32 */
float      lmono_normals_default_cell(float radius);
/* viewpoint: three finite floats or NULL */
int        lmono_normals_compute(lmono_ctx *, lmono_normals *, const lmono_point_rgb *pts_h, int64_t n, const float *viewpoint, int64_t *stats);
int        lmono_normals_compute_d(lmono_ctx *, lmono_normals *, const lmono_point_rgb *pts_d, int64_t n, const float *viewpoint, int64_t *stats);
/* n distinct handles each take the world-frame cloud of the last frame of one of n distinct builders straight from device memory; one
 * launch per phase for all streams (viewpoints: [n][3] or NULL).  A stream's bytes do not depend on the batch it travels in. */
int        lmono_normals_compute_frames(lmono_ctx *, int n, lmono_normals *const *normals, lmono_map_builder *const *mbs, const float *viewpoints, int64_t *stats);
/* one point per occupied voxel, what lmono_voxel_map_read gives, without a host copy and in the order the device found them:
 * lmono_normals_cloud tells which point each record belongs to */
int        lmono_normals_compute_map(lmono_ctx *, lmono_normals *, lmono_voxel_map *, const float *viewpoint, int64_t *stats);
/* the last result in input order: records and neighbour counts (either pointer may be NULL), and the points they belong to.  Both
 * return the count (and copy when a pointer is not NULL). */
int64_t    lmono_normals_read(lmono_ctx *, lmono_normals *, lmono_normal *out_h, uint32_t *count_h, int64_t cap);
int64_t    lmono_normals_cloud(lmono_ctx *, lmono_normals *, lmono_point_rgb *out_h, int64_t cap);

/* ---- map builder: FPFH descriptors at keypoints ----------------------------------------------------------------
 * The pcl::FPFHEstimation with setSearchSurface and setRadiusSearch(0.05) of MapBuilder::alignmentToMap
 * (mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210, commented out in the reference).  The surface is the cloud of a normals
 * handle after a compute, read in device memory with its records; the keypoints are m <= max_keypoints finite positions on the host,
 * not necessarily points of the cloud (the reference's SIFT keypoint detector is not provided: one point per voxel of a map at a
 * coarse leaf serves).  A definition of this project (lmono_amd/csrc/fpfh.hpp): PCL's pair features in fp64 without transcendentals,
 * three 11-bin histograms per surface point within radius of a keypoint (integer counts), and per keypoint their sum under the
 * integer weight (uint64)(2^40 / (max(d2, 2^-20) * pairs)) in exact hi / lo words, each sub-histogram scaled to sum to 100 and
 * written as 33 floats (FPFHSignature33's layout).  A surface point at the keypoint counts with the largest weight (PCL skips it).
 * A descriptor is a pure function of the SET of surface points with normals and of the keypoint: the same bytes for every point
 * order, grid tuning (cell, max_rings) and batch.  Parity with PCL is unpinned.  Limits: max_points <= 2^26, max_keypoints <= 4096,
 * 0 < radius <= 4, (max_rings - 0.25) cell >= radius; the radius is independent of the normals'.
 * Per keypoint: the descriptor, the number of contributing surface points, and a flag (0: none contributed, the descriptor is 33 zeros).
 * stats [8] per stream: keypoints in, with a descriptor, without, surface points with an SPFH, sum of their pair counts, largest
 * pair count, sum of the keypoints' contributing points, largest.  A normals handle without a result (or with an empty one) and a
 * non-finite keypoint return LMONO_EINVAL, m > max_keypoints or a cloud above max_points LMONO_ECAPACITY, all before any launch;
 * m == 0 is a successful empty result.  Every compute replaces the handle's last result. */
typedef struct lmono_fpfh lmono_fpfh;
lmono_fpfh *lmono_fpfh_create(lmono_ctx *, int64_t max_points, int64_t max_keypoints, float radius, float cell, int max_rings);
void       lmono_fpfh_destroy(lmono_fpfh *);
/* the default cell for radius at max_rings = 2: lmono_normals_default_cell's rule */
float      lmono_fpfh_default_cell(float radius);
/* keypoints_h: [m][3] float */
int        lmono_fpfh_compute(lmono_ctx *, lmono_fpfh *, lmono_normals *, const float *keypoints_h, int64_t m, int64_t *stats);
/* n distinct handles, each over one normals handle (which may repeat) and its own keypoints; one launch per phase for all streams.
 * A stream's bytes do not depend on the batch it travels in. */
int        lmono_fpfh_compute_batch(lmono_ctx *, int n, lmono_fpfh *const *fpfhs, lmono_normals *const *normals, const float *const *keypoints_h, const int64_t *ms, int64_t *stats);
/* the last result in keypoint order: descriptors [m][33], contributing points [m], flags [m] (any pointer may be NULL), and the
 * keypoints themselves.  Both return the count (and copy when a pointer is not NULL). */
int64_t    lmono_fpfh_read(lmono_ctx *, lmono_fpfh *, float *desc_h, uint32_t *count_h, uint32_t *flag_h, int64_t cap);
int64_t    lmono_fpfh_keypoints(lmono_ctx *, lmono_fpfh *, float *out_h, int64_t cap);

/* ---- map builder: sample-consensus initial alignment on FPFH descriptors ------------------------------------
 * Replaces the pcl::SampleConsensusInitialAlignment of MapBuilder::alignmentToMap (computeInitialAlignment: setMinSampleDistance(0.5),
 * setMaxCorrespondenceDistance(1.0), setMaximumIterations(30); mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210, commented out in
 * the reference), a definition of this project (lmono_amd/csrc/sacia.hpp): per source keypoint the k_corr target keypoints of nearest
 * descriptor, exactly, ties to the lowest index; hypothesis h draws three source keypoints at least min_sample_dist apart and one candidate
 * of each from the PnP RANSAC's counter-based generator, fits them with the closed form of lmono_icp_*, and is scored by the integer sum of
 * the squared distances to the nearest target keypoint, truncated at max_corr^2; the least (error, h) wins.  Keypoints without a descriptor
 * take no part; fewer than 3 with one on either side, a handle without a result and a keypoint 2048 m or more from the first one of its
 * side return LMONO_EINVAL.  0 <= min_sample_dist <= 4096, 0 < max_corr <= 16, k_corr in 1 .. 32, n_hyp in 1 .. 65536; launch_hyps: the
 * hypotheses of one launch (0: all), which changes no result.  stats [8]: ok (0: every hypothesis was void, the handle then shows no
 * transform), the winning h (-1), its error word, its inliers, void hypotheses, usable source keypoints, usable target keypoints, n_hyp. */
typedef struct lmono_sacia lmono_sacia;
lmono_sacia *lmono_sacia_create(lmono_ctx *, float min_sample_dist, float max_corr, int k_corr, int n_hyp, uint32_t seed, int launch_hyps);
void       lmono_sacia_destroy(lmono_sacia *);
int        lmono_sacia_align(lmono_ctx *, lmono_sacia *, lmono_fpfh *src, lmono_fpfh *tgt, int64_t *stats);
/* the last align: its transform, row-major 3 x 4, what lmono_icp_set_guess takes (LMONO_EINVAL without one), and per hypothesis the
 * error word (all ones: void) and the inliers; errors returns the count (and copies when a pointer is not NULL). */
int        lmono_sacia_transform(lmono_ctx *, lmono_sacia *, double out[12]);
int64_t    lmono_sacia_errors(lmono_ctx *, lmono_sacia *, uint64_t *err_h, uint32_t *inl_h, int64_t cap);

/* ---- image feature tracker ---------------------------------------------------------------------------------
 * Replaces FeatureTracker::trackImage of the mono path, use_rejectF = 0 or 1 (lmono_tracker_set_reject_f) (mono_lidar_mapping/src/image_process/
 * FeatureTracker.cc:189-433): BGR2GRAY (:193), forward / backward pyramidal LK with the 0.5 px round-trip and inBorder tests
 * (:213-249), track_cnt++ (:251), setMask (:55-84, ties in track count kept in current order), goodFeaturesToTrack under the
 * mask (:281-297), undistortedPts through the PINHOLE liftProjective (:172-187) and ptsVelocity (:94-133).  The pyramid of a
 * frame and its Scharr planes stay on the device and become the previous pyramid of the next frame.  The camera is the
 * lmono_camera of the map builder (its kernel_* / blur_type fields are not read).  Not provided: rejectWithF (:435-503; a
 * non-zero flags argument is refused), the right-image branch (:305-347), drawTrack.                                        */
#define LMONO_TRACK_MAX_POINTS 512   /* largest max_cnt                                       */
#define LMONO_TRACK_GREY8      0     /* image: [height][width] uint8                          */
#define LMONO_TRACK_BGR8       1     /* image: [height][width][3] uint8 (cv::Mat BGR8)        */
#define LMONO_TRACK_REJECT_F   1     /* flags bit: refused -- use lmono_tracker_set_reject_f  */
/* one feature of the frame (:372-397): id, normalised x y (z = 1), pixel u v, velocity of the normalised point, track count;
 * id / x_n / y_n / u / v / vx / vy are FeatureManager::Image's (feature_id, xyz_uv_velocity) with camera_id 0 */
typedef struct { int32_t id; float x_n, y_n, u, v, vx, vy; int32_t track_cnt; } lmono_track_record;
typedef struct lmono_tracker lmono_tracker;
/* max_cnt: MAX_CNT (1..512); min_dist: MIN_DIST in pixels (1..128); flags: 0.  NULL (see lmono_last_error) for an image side
 * of 21 pixels or less (the LK window), limits exceeded or LMONO_TRACK_REJECT_F. */
lmono_tracker *lmono_tracker_create(lmono_ctx *, const lmono_camera *, int max_cnt, int min_dist, int flags);
void           lmono_tracker_destroy(lmono_tracker *);
int            lmono_tracker_reset(lmono_ctx *, lmono_tracker *);                       /* forget points, ids and the last frame */
/* One trackImage on a host image.  records_out: [cap >= max_cnt] (may be NULL); *n_out: features of the frame. */
int lmono_tracker_track(lmono_ctx *, lmono_tracker *, double time, const uint8_t *image_h, int format, lmono_track_record *records_out, int cap, int *n_out);
/* n_streams independent trackers (distinct) advanced by one frame each, images already resident in HBM (image_d[s] device
 * pointers; times, caps, n_out host arrays [n]; records_out [n] host pointers); every phase is one launch for all streams. */
int lmono_tracker_track_batch(lmono_ctx *, int n_streams, lmono_tracker *const *trackers, const double *times, const uint8_t *const *image_d, int format,
                              lmono_track_record *const *records_out, const int *caps, int *n_out);
/* diagnostics: level `level` of the last frame's pyramid and its Scharr planes (any output may be NULL); returns the number of
 * levels (cv::buildOpticalFlowPyramid keeps a level while both sides exceed 21) */
int lmono_tracker_pyramid(lmono_ctx *, lmono_tracker *, int level, uint8_t *image_h, int16_t *dx_h, int16_t *dy_h, int *width, int *height);
/* min-eigenvalue corner response [height][width] fp32 of the last frame that had room for new corners */
int lmono_tracker_response(lmono_ctx *, lmono_tracker *, float *response_h);
/* the two cv::calcOpticalFlowPyrLK calls of :218 / :223 between the last two frames on n <= 512 given points: pts_h [n][2] ->
 * fwd_h [n][2], rev_h [n][2], status_h [n][2] (forward, backward; backward is 0 where forward failed).  Leaves the tracks alone. */
int lmono_tracker_lk(lmono_ctx *, lmono_tracker *, int n, const float *pts_h, float *fwd_h, float *rev_h, uint8_t *status_h);
/* rejectWithF (:259-262, :435-503): after the forward-backward test, n_hyp 8-point hypotheses from a
 * counter-based sample stream keyed by (seed, frames since the last reset, hypothesis, draw) are scored in fp64 against
 * f_threshold (F_THRESHOLD, gate 1); F is refitted over the winner's inliers, and an inlier whose symmetric distance
 * r^2 / (|l|^2 + |l'|^2) exceeds f_dis (F_DIS, :467-499) is dropped too (gate 2).  Our own definition: parity with OpenCV's
 * RANSAC is unpinned.  Fewer than 8 survivors: the step does not run; no valid hypothesis or fewer than 8 inliers: all dropped. */
typedef struct { double f_threshold, f_dis, focal_length; int32_t n_hyp; uint32_t seed; } lmono_reject_f;   /* focal_length 0 -> 460, n_hyp 0 -> 256 */
int lmono_tracker_set_reject_f(lmono_ctx *, lmono_tracker *, const lmono_reject_f *);   /* NULL: off; takes effect with the next frame */
/* last frame: stats[4] = valid hypotheses, best hypothesis, gate-1 inliers, kept after gate 2 (all -1: step did not run); F [9] row-major */
int lmono_tracker_reject_stats(lmono_ctx *, lmono_tracker *, int32_t *stats, double *F);
/* diagnostic, like lmono_tracker_lk: the step on n (8..512) given pixel pairs with the tracker's camera and parameters; leaves the tracks alone */
int lmono_tracker_reject_f(lmono_ctx *, lmono_tracker *, int n, const float *prev_px_h, const float *cur_px_h, uint32_t frame_key,
                           uint8_t *status_h, int32_t *stats, double *F);

/* ---- keyframe descriptors ------------------------------------------------------------------------------------
 * Replaces the per-keyframe image work of the loop detector, KeyFrame (mono_lidar_mapping/src/loop_detection/KeyFrame.cc):
 * computeBRIEFPoint (:184-210: cv::FAST(image, kp, 20, true), a BRIEF descriptor per corner, liftProjective), computeWindowBRIEFPoint
 * (:172-182: a descriptor per window point point_2d_uv), DVision's BRIEF::compute (src/loop_detection/DVision/BRIEF.cpp:39-106:
 * 9 x 9 Gaussian blur with sigma 2, 256 pixel-pair tests), searchByBRIEFDes / searchInAera (:217-267: exhaustive Hamming search from
 * 128 with a strict <, matched below 80) and the count that findConnection compares with MIN_BRIEF_LOOP_NUM (:455-462, :557).
 * FAST-9/16 with 3 x 3 strict non-maximum suppression and the integer blur ([7 17 32 46 52 46 32 17 7] / 256 per axis, REFLECT_101,
 * one rounding) are definitions of this project, written out in DESIGN.md 6f: parity with cv::FAST and cv::GaussianBlur is unpinned.
 * BRIEF and the search follow the reference's source statement by statement.  The test pattern is an argument (the reference reads
 * brief_pattern.yml from BRIEF_PATTERN_FILE at run time).  Keypoints are in row-major order (y, then x).
 * PnPRANSAC and the rest of findConnection (:296-351, :551-688) are lmono_keyframes_verify below.
 * db.query / db.add and LoopDetector::detectLoop are lmono_keyframes_query / _detect_loop further below.  Not provided: the USE_ORB
 * branch, the thumbnail, distributionValidation (dead code), every DEBUG_IMAGE product.                                              */
typedef struct { int8_t x1[256], y1[256], x2[256], y2[256]; } lmono_brief_pattern;   /* every offset in -63..63 */
typedef struct lmono_keyframes lmono_keyframes;
/* A device-resident store of up to max_keyframes (<= 65535) keyframes of up to max_keypoints (<= 65535) FAST corners each: per keyframe
 * its keypoints, normalised keypoints, descriptors (8 uint32: bit i is bit i & 31 of word i >> 5), window points and window descriptors.
 * fast_threshold: 0 means 20 (:187).  The camera is the lmono_camera of the map builder (PINHOLE; kernel_* / blur_type are not read).
 * NULL (see lmono_last_error) for an image side outside 16..8192, limits exceeded or a pattern offset outside -63..63. */
lmono_keyframes *lmono_keyframes_create(lmono_ctx *, const lmono_camera *, const lmono_brief_pattern *, int max_keyframes, int max_keypoints, int fast_threshold);
void             lmono_keyframes_destroy(lmono_keyframes *);
int              lmono_keyframes_clear(lmono_ctx *, lmono_keyframes *);                    /* forget every keyframe */
int              lmono_keyframes_size(lmono_ctx *, lmono_keyframes *);                     /* stored keyframes (or an error < 0) */
/* The first KeyFrame constructor (:14-93) on a host image (format: LMONO_TRACK_GREY8 / LMONO_TRACK_BGR8): window_uv_h [n_window <= 512][2]
 * are point_2d_uv.  *index_out: the new keyframe's index; *n_keypoints_out: FAST corners found (also when refused).  LMONO_ECAPACITY,
 * with the store unchanged and nothing truncated, when the image has more corners than max_keypoints or the store is full. */
int lmono_keyframes_add(lmono_ctx *, lmono_keyframes *, const uint8_t *image_h, int format, int n_window, const float *window_uv_h, int *index_out, int *n_keypoints_out);
/* n independent stores (distinct) advanced by one keyframe each, images already resident in HBM (image_d[s] device pointers; n_window,
 * index_out, n_keypoints_out host arrays [n]; window_uv_h [n] host pointers); every phase is one launch for all streams and the call has
 * one read-back.  When any stream is refused (LMONO_ECAPACITY) no store is changed. */
int lmono_keyframes_add_batch(lmono_ctx *, int n, lmono_keyframes *const *stores, const uint8_t *const *image_d, int format, const int *n_window,
                              const float *const *window_uv_h, int *index_out, int *n_keypoints_out);
/* The second KeyFrame constructor (:96-133): a keyframe from saved keypoints [n][2], normalised keypoints [n][2] and descriptors [n][8],
 * without an image; optionally with window points and their descriptors (n_window may be 0). */
int lmono_keyframes_load(lmono_ctx *, lmono_keyframes *, int n_keypoints, const float *keypoints_h, const float *norm_h, const uint32_t *descriptors_h,
                         int n_window, const float *window_uv_h, const uint32_t *window_descriptors_h, int *index_out);
/* searchByBRIEFDes (:248-267) of keyframe `cur`'s window descriptors against n_old stored keyframes in one launch.  Outputs (any may be
 * NULL) are [n_old][n_window of cur]: status (1: matched), index of the nearest old keypoint (-1: no distance below 128), its distance
 * (128 then), the matched old pixel and old normalised point ((0, 0) when unmatched, as the reference pushes); counts_h [n_old]: matched
 * points per old keyframe, the number findConnection compares with MIN_BRIEF_LOOP_NUM (:557).  Equal distances: the lowest index wins. */
int lmono_keyframes_match(lmono_ctx *, lmono_keyframes *, int cur, int n_old, const int32_t *old_indices, uint8_t *status_h, int32_t *index_h, int32_t *dist_h,
                          float *old_uv_h, float *old_norm_h, int32_t *counts_h);
/* diagnostics: the blurred image and the FAST score image (A - 1 at a corner, else 0), [height][width] uint8, of the last image added
 * (refused ones included); either may be NULL */
int lmono_keyframes_images(lmono_ctx *, lmono_keyframes *, uint8_t *blur_h, uint8_t *score_h);
/* a stored keyframe: counts and (any may be NULL) keypoints [n][2], normalised keypoints [n][2], descriptors [n][8], window points
 * [m][2], window descriptors [m][8]; call once with NULL arrays for the counts */
int lmono_keyframes_get(lmono_ctx *, lmono_keyframes *, int index, int *n_keypoints, float *keypoints_h, float *norm_h, uint32_t *descriptors_h,
                        int *n_window, float *window_uv_h, uint32_t *window_descriptors_h);

/* ---- loop verification -------------------------------------------------------------------------------------------
 * KeyFrame::PnPRANSAC (KeyFrame.cc:296-351) and the gates of findConnection (:551-688).  The PnP step is a RANSAC of this project's
 * own definition, written out in DESIGN.md 6g: exactly n_hyp hypotheses of 4 pairs each from the counter-based sample stream of the
 * tracker's rejection keyed by (seed, a caller-given key, hypothesis, draw), every one 12 damped Gauss-Newton steps from the guess in
 * fp64 (K = I), scored against `threshold` on the normalised plane; the winner (most inliers, then the lowest hypothesis) is refitted
 * over its inliers.  Parity with cv::solvePnPRansac is unpinned.  Fewer than 4 pairs: the step does not run (stats all -1); no valid
 * hypothesis or fewer than 4 inliers: status all 0 and the pose is the guess unchanged.  Poses are t (x y z), q (x y z w).            */
typedef struct {
    double threshold;                 /* 0 -> 10.0 / 460.0 (:328)                                    */
    int32_t n_hyp;                    /* 0 -> 256, at most 1024                                      */
    uint32_t seed;
    int32_t min_brief_loop_num;       /* MIN_BRIEF_LOOP_NUM, 0 -> 25                                 */
    int32_t min_pnp_loop_num;         /* MIN_PNP_LOOP_NUM, 0 -> 5                                    */
    double angle_threshold;           /* ANGLE_THRESHOLD (degrees), 0 -> 30                          */
    double trans_threshold;           /* TRANS_THRESHOLD (m), 0 -> 20                                */
} lmono_pnp_params;
/* The PnP step alone on n (1..65535) independent problems in one launch (params may be NULL: the defaults; the gates are not read).
 * counts_h [n] pairs per problem (0..512; more: LMONO_ECAPACITY); points_3d_h [sum][3] and points_2d_h [sum][2] (normalised image
 * points) concatenated in problem order; guess_tq_h [n][7] camera-from-world; keys_h [n] the sample stream's key of each problem.
 * Outputs: status_h [sum] (1: inlier of the winner), pose_tq_h [n][7] (optional), stats_h [n][4] (optional) = valid hypotheses, best
 * hypothesis, the winner's inliers, refit steps run (all -1: the step did not run).  A problem's bytes do not depend on its batch. */
int lmono_pnp_ransac(lmono_ctx *, const lmono_pnp_params *, int n, const int32_t *counts_h, const float *points_3d_h, const float *points_2d_h,
                     const double *guess_tq_h, const uint32_t *keys_h, uint8_t *status_h, double *pose_tq_h, int32_t *stats_h);
/* findConnection of keyframe `cur` against n_old stored keyframes: lmono_keyframes_match, the matched pairs compacted on the device,
 * the PnP step over every candidate in one launch (key: cur << 16 | old index -- a store holds at most 65535 keyframes, so no two pairs
 * of one store share a key; a candidate whose match count is at or below
 * min_brief_loop_num skips it, :557), one read-back, then on the host :341-350, :570-588 and :636-682.
 * point_3d_h [n_window of cur][3]: point_3d of the current keyframe's window points (world frame); vio_tq [7]: origin_vio_T / _R;
 * ex_tq [7]: tlc, qlc (camera in body); old_tq_h [n_old][7]: T_w_i, R_w_i of the old keyframes, or NULL (then channel_h must be NULL).
 * Outputs (any may be NULL), per candidate: brief_counts_h [n_old]; pnp_inliers_h [n_old] (0 when the step did not run or failed);
 * status_h [n_old][n_window] after both reductions; pnp_tq_old_h [n_old][7] PnP_T_old, PnP_R_old; loop_info_h [n_old][8] in the
 * layout lmono_pose_graph_create reads; has_loop_h [n_old]: count > min_brief_loop_num && inliers > min_pnp_loop_num &&
 * |relative_euler| < angle_threshold && |relative_t| < trans_threshold; channel_h [n_old][15]: old_T, old_Q (w x y z), correct_T,
 * correct_Q (w x y z), cur; relative_euler_h [n_old][3] (degrees); pose_tq_h [n_old][7] and stats_h [n_old][4] as in lmono_pnp_ransac.
 * Where the step did not run or failed, the pose is the guess of :308-312 and everything derived from a pose is derived from it. */
int lmono_keyframes_verify(lmono_ctx *, lmono_keyframes *, int cur, int n_old, const int32_t *old_indices, const float *point_3d_h, const double *vio_tq,
                           const double *ex_tq, const double *old_tq_h, const lmono_pnp_params *, int32_t *brief_counts_h, int32_t *pnp_inliers_h,
                           uint8_t *status_h, double *pnp_tq_old_h, double *loop_info_h, uint8_t *has_loop_h, double *channel_h, double *relative_euler_h,
                           double *pose_tq_h, int32_t *stats_h);

/* ---- loop detection ----------------------------------------------------------------------------------------------
 * LoopDetector::detectLoop (mono_lidar_mapping/src/loop_detection/LoopDetector.cc:167-260): the BRIEF vocabulary tree, the BoW vector of
 * a keyframe, db.query and the score rules, for TF_IDF weighting and L1_NORM scoring (the pair the reference's vocabulary uses; any
 * other is refused).  The stored keyframes are the database: entry e is keyframe e of the store, and a query of keyframe `cur` sees the
 * entries before it, as the reference queries before it adds.  Every sum is sequential fp64 in the order DESIGN.md 6h writes out, and
 * equal scores order by entry id.  Parity with a compiled DBoW2 is unpinned.  Not provided: the direct index, delete_entry, the other
 * scoring and weighting types. */
typedef struct lmono_brief_vocabulary lmono_brief_vocabulary;
/* BriefVocabulary::loadBin (VocabularyBinary.hpp; TemplatedVocabulary.h:1500-1560) from the file's records: k, L, scoringType (0: L1_NORM),
 * weightingType (0: TF_IDF); n_nodes records node_id / parent_id / weight / descriptors [n_nodes][8] (uint32: bit i is bit i & 31 of word
 * i >> 5, the bytes of the file's 4 x uint64); n_words records word_node_id / word_id.  Node 0 is the root and has no record; the children
 * of a node are the records that name it as parent, in file order.  NULL with the reason in lmono_last_error, before anything is uploaded,
 * for: k outside 2..64, L outside 1..10, other types, n_nodes outside 1..16777215, node ids that are not exactly 1..n_nodes, a parent
 * outside 0..n_nodes or equal to its node, a negative or non-finite weight, more than k children, a node unreachable from the root or
 * deeper than L, words that are not a bijection between 0..n_words-1 and the leaves. */
lmono_brief_vocabulary *lmono_brief_vocabulary_create(lmono_ctx *, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id,
                                                      const double *weight, const uint32_t *descriptors, int n_words, const int32_t *word_node_id, const int32_t *word_id);
/* the handle goes; a store the vocabulary is attached to keeps the device tree alive */
void lmono_brief_vocabulary_destroy(lmono_brief_vocabulary *);
/* TemplatedVocabulary::transform(feature, word_id, weight) (:1217-1258) of n descriptors [n][8]: from the root to the child at the
 * smallest Hamming distance (the first of equal children) until a leaf -> word_h [n], weight_h [n] (either may be NULL) */
int lmono_brief_vocabulary_transform(lmono_ctx *, lmono_brief_vocabulary *, int n, const uint32_t *desc_h, int32_t *word_h, double *weight_h);
/* db.setVocabulary (LoopDetector.cc:29): attach a vocabulary to a store (NULL detaches and frees the store's BoW arrays).  One vocabulary
 * serves any number of stores.  LMONO_ECAPACITY for a store created with max_keypoints > 16384.  BoW vectors are built lazily, by the
 * three calls below, for every stored keyframe that has none yet; lmono_keyframes_clear and this call forget them. */
int lmono_keyframes_set_vocabulary(lmono_ctx *, lmono_keyframes *, lmono_brief_vocabulary *);
/* the BoW vector of stored keyframe `index` (TemplatedVocabulary.h:1065-1121, BowVector.cpp:34-84): words of weight > 0 in ascending id,
 * value = the weight added once per occurrence, divided by the L1 norm -> *n_out entries in word_h / value_h (room for the keyframe's
 * corner count; either may be NULL) */
int lmono_keyframes_bow(lmono_ctx *, lmono_keyframes *, int index, int *n_out, int32_t *word_h, double *value_h);
/* db.query(brief_descriptors of cur, ret, max_results, max_id) (TemplatedDatabase.h:656-723): entry e < cur is admitted iff e < max_id ||
 * max_id == -1 || e == cur - 1; admitted entries that share a word with cur, ordered by Score descending (ties: the lower id), cut to
 * max_results (1..16) -> *n_out, id_h, score_h (room for max_results).  A pure function of the store's contents below cur. */
int lmono_keyframes_query(lmono_ctx *, lmono_keyframes *, int cur, int max_results, int max_id, int *n_out, int32_t *id_h, double *score_h);
/* LoopDetector::detectLoop (:181-259, without DEBUG_IMAGE): ret = query(cur, 4, cur - loop_search_gap) -> *n_out, id_h [4], score_h [4];
 * *loop_index_out: -1 when cur - loop_search_gap < 0, else the rule of :200-259 with its constants 0.05 and 0.015 (-1: no loop).
 * LMONO_EINVAL before any launch: no vocabulary attached, cur not a stored keyframe. */
int lmono_keyframes_detect_loop(lmono_ctx *, lmono_keyframes *, int cur, int loop_search_gap, int *loop_index_out, int *n_out, int32_t *id_h, double *score_h);
/* ... of keyframe cur [s] of n distinct stores that share one vocabulary: every phase is one launch over all streams, one read-back;
 * loop_index_out [n], n_out [n], id_h [n][4], score_h [n][4].  A stream's bytes do not depend on the batch it travels in. */
int lmono_keyframes_detect_loop_batch(lmono_ctx *, int n, lmono_keyframes *const *stores, const int *cur, int loop_search_gap, int *loop_index_out, int *n_out,
                                      int32_t *id_h, double *score_h);

/* ---- loop-closure pose graph -- NEW FEATURE, no counterpart in the reference --------------------------
 * The reference detects loops and publishes loop_info = relative_t, relative_q (w x y z), relative_yaw
 * (mono_lidar_mapping/src/loop_detection/KeyFrame.cc:570-633) and re-anchors the window rigidly (Estimator.cc:309-365); it never
 * optimises a graph and only carries the unused 4-DoF helpers of include/loop_detection/Loop_Detector.h:99-168.  This entry is
 * the 4-DoF (yaw, x, y, z; degrees) keyframe graph those helpers belong to: odometry edges to the four previous keyframes,
 * one Huber(0.1) edge per loop (yaw residual / 10), keyframe 0 fixed, Ceres-style Levenberg-Marquardt with a block-banded
 * Cholesky in reverse Cuthill-McKee order.
 * poses_tq_h: [n][7] keyframe poses t (x y z), q (x y z w); loops_h: [n_loops][2] (old keyframe, current keyframe);
 * loop_info_h: [n_loops][8] in the layout above.
 * Multi-GPU: every rank creates the same graph; per round each rank calls lmono_pose_graph_linearise(rank, world) -- the
 * normal equations of the edges it owns --, the fp64 buffer lmono_pose_graph_reduce_buffer (reduce_count doubles) is summed
 * over ranks with one all-reduce (RCCL), and lmono_pose_graph_step takes the identical trust-region step on every rank.   */
typedef struct lmono_pose_graph lmono_pose_graph;
lmono_pose_graph *lmono_pose_graph_create(lmono_ctx *, int n, const double *poses_tq_h, int n_loops, const int32_t *loops_h, const double *loop_info_h);
void              lmono_pose_graph_destroy(lmono_pose_graph *);
int   lmono_pose_graph_reset(lmono_ctx *, lmono_pose_graph *);                    /* back to the odometry poses, same graph */
int   lmono_pose_graph_info(lmono_pose_graph *, int64_t *reduce_count, int *bandwidth_blocks, int *n_edges);
/* pos_out [n]: the elimination position of every keyframe (reverse Cuthill-McKee); H, g and cost of the reduce buffer are
 * stored in that order: H [n][bandwidth + 1][16] (block (p, p - d), row-major, lower band) | g [4 n] | cost [n] */
int   lmono_pose_graph_order(lmono_pose_graph *, int32_t *pos_out);
void *lmono_pose_graph_reduce_buffer(lmono_pose_graph *);                         /* device pointer, reduce_count doubles */
/* use a caller-owned device buffer of reduce_count doubles instead (e.g. the storage of the tensor handed to the all-reduce) */
int   lmono_pose_graph_set_reduce_buffer(lmono_pose_graph *, void *buffer_d);
int   lmono_pose_graph_linearise(lmono_ctx *, lmono_pose_graph *, int rank, int world);
int   lmono_pose_graph_step(lmono_ctx *, lmono_pose_graph *, int max_iter, int *done);   /* done (optional) synchronises   */
int   lmono_pose_graph_optimize(lmono_ctx *, lmono_pose_graph *, int max_iter);          /* one GPU: the loop of the two   */
/* poses_tq_h: [n][7] optimised keyframes; stats (optional, [6]): LM iterations, initial cost, final cost, half bandwidth
 * (blocks), accepted steps, rejected steps */
int   lmono_pose_graph_result(lmono_ctx *, lmono_pose_graph *, double *poses_tq_h, double *stats);

/* ---- camera-LiDAR rotation calibration, ESTIMATE_LASER == 2 ---------------------------------------------------------
 * Estimator.cc:403-430 and src/initial/AxxbSolver.cc.  Per stream and frame: (1) the essential matrix of the frame's pairs of normalised
 * points, the Hartley-normalised 8-point fit over all of them (pairs with a non-finite coordinate are dropped; fewer than 9 left: the
 * identity); (2) R1 = U W V^T, R2 = U W^T V^T, t = +-u3; (3) the cheirality vote of testTriangulation over (R1, t), (R1, -t), (R2, t),
 * (R2, -t), R1 on a strict majority, the winner transposed; (4) one step of CalibrationExRotation on a running 4 x 4 sum of the
 * Huber-weighted blocks L(q_cam) - R(q_lidar): rlc = the transposed rotation of the smallest eigenvector, sv = the square roots of the
 * eigenvalues, descending, ok = frame_count >= count && sv[2] > 0.25.  All fp64, one written order; parity with OpenCV and Eigen is unpinned.
 * Quaternions are x y z w.  pairs [sum m][4] = prev x, prev y, cur x, cur y, concatenated in call order; m [n] in 0..512.
 * stats [n][6] = pairs used, the four front counts, the winner (0: R1, 1: R2, -1: the identity by rule).  Refused before any launch, with
 * no state changed: m > 512 (LMONO_ECAPACITY); a negative m, a stream index out of range or named twice in one call, count < 1, a
 * non-finite quaternion (LMONO_EINVAL).  Outputs may be NULL.  A stream's bytes do not depend on the batch it travels in. */
typedef struct lmono_excalib lmono_excalib;
int  lmono_excalib_create(lmono_ctx *, int n_streams, lmono_excalib **out);
void lmono_excalib_destroy(lmono_excalib *);
int  lmono_excalib_reset(lmono_excalib *, int stream);          /* stream -1: all.  frame_count 0, a zero sum, rlc = I */
/* stages 1-3 alone, stateless: R_out [n][9] = the camera's rotation increment R_{c,k-1}^T R_{c,k} */
int  lmono_relative_rotation(lmono_ctx *, int n, const int32_t *m, const double *pairs, double *R_out, int32_t *stats);
/* stage 4 alone on given rotation pairs: q_cam [n][4], q_lidar [n][4] -> rlc [n][9], sv [n][4], huber [n], ok [n] */
int  lmono_excalib_push(lmono_excalib *, int n, const int32_t *streams, const double *q_cam, const double *q_lidar, int count, double *rlc, double *sv,
                        double *huber, int32_t *ok);
/* stages 1-4 of n distinct streams in one launch: q_cam is Quaterniond(R_cam) */
int  lmono_excalib_step(lmono_excalib *, int n, const int32_t *streams, const int32_t *m, const double *pairs, const double *q_lidar, int count,
                        double *R_cam, int32_t *stats, double *rlc, double *sv, double *huber, int32_t *ok);
int  lmono_excalib_state(lmono_excalib *, int stream, int *frame_count, double *M, double *rlc);   /* M [16], rlc [9] */

/* ---- pose composition (laserOdometry: t_w_curr += q_w_curr * t_last_curr; q_w_curr *= q_last_curr) ------- *
 * lmono_pose_prefix_d: poses_d[k - first] = incr[first] (+) ... (+) incr[k] for k in [first, n) (incr[0] is the
 * identity: first = 0 gives poses relative to scan 0, first > 0 poses relative to scan first-1).  lmono_pose_rebase_d: poses[k] <- bases[0] (+) ... (+) bases[n_bases-1] (+) poses[k]; with scans
 * sharded over GPUs, bases are the cumulative transforms of the lower ranks (one RCCL all-gather of 56 B/rank). */
int lmono_pose_prefix_d(lmono_ctx *, const double *incr_d, int first, int n, double *poses_d);
int lmono_pose_rebase_d(lmono_ctx *, const double *bases_d, int n_bases, double *poses_d, int n);

/* Device-time accounting with hipEvents recorded on the context stream around every kernel group of every
 * lmono_scanreg_batch / lmono_odom_batch call since the last reset.  ms_out[0..8] = summed milliseconds of:
 * [0] front end total, [1] odometry total, [2] k_ring_sort, [3] k_curvature (an empty slot: k_select computes the curvature), [4] k_select, [5] k_voxel,
 * [6] k_compact_index (compaction + line index), [7] k_grid_build, [8] k_line_index (the full-width launch),
 * [9] all k_correspond launches, [10] all k_lm_solve launches, [11] number of k_correspond (= k_lm_solve)
 * launches.  Both calls synchronise the stream.                                                            */
int lmono_timing_reset(lmono_ctx *);
int lmono_timing_read(lmono_ctx *, double *ms_out, int cap, int *n_scanreg_calls, int *n_odom_calls);

#ifdef __cplusplus
}
#endif
#endif
