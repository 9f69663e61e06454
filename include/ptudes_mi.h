/*
 * ptudes_mi.h -- C-ABI of libptudes_mi.so: the MI355X-native lidar-odometry core.
 *
 * Drop-in boundary for ONE hot path of bexcite/ptudes-lab: the `ptudes ekf-bench ouster` loop
 * (reference src/ptudes/cli/ekf_bench.py:493-563) = KISS-ICP scan-to-local-map registration
 * (reference src/ptudes/kiss.py:54-131, arithmetic in the third-party kiss-icp 0.2.10) + the ptudes
 * error-state EKF (reference src/ptudes/ins/es_ekf.py:191-329).
 *
 * The reference has NO C/FFI boundary of its own: the path sits behind two Python classes
 * (KissICPWrapper, ESEKF) and below them kiss-icp's private pybind11 module.  The entry points here
 * are what a ctypes/pybind11 binding for those classes binds; each one names the reference
 * interface it replaces.  INTEGRATION.md shows the Python-side stubs.
 *
 * Conventions (same as the reference): poses are 4x4 row-major doubles, T_world<-body, body = IMU
 * frame; quaternions xyzw; ICP tangent order (translation, rotation); the EKF attitude error is a
 * right perturbation.  Every function returns 0 on success, < 0 on error (ptl_last_error() gives the
 * text, thread-local).  A handle is not thread-safe; distinct handles are independent.  Each handle
 * owns one HIP stream on cfg.device_id.  Caller owns all buffers passed in; the library copies.
 * All numerics run on the GPU (hand-written HIP kernels, gfx950); there is no CPU fallback.
 */
#ifndef PTUDES_MI_H
#define PTUDES_MI_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTL_OK 0
#define PTL_ERR_ARG -1
#define PTL_ERR_HIP -2      /* HIP runtime error / no device */
#define PTL_ERR_CAPACITY -3 /* a device-side capacity (map pool / hash table / scan size) was exceeded */
#define PTL_ERR_STATE -4

#define PTL_F32 0
#define PTL_F64 1

/* ---- ABI guard.  Every configuration struct starts with {struct_size, abi_version}: the CALLER writes sizeof(its own struct) and the
 * PTL_ABI_VERSION it was compiled / written against (PTL_CFG_INIT does both) BEFORE handing the struct to the library, and
 * ptl_*_default_cfg / ptl_*_create refuse a struct whose size or version is not the library's with PTL_ERR_ARG and both numbers in
 * ptl_last_error() - without writing a byte.  A binding in another language (ctypes, cgo, JNI) that was written against an older header
 * therefore fails at its first call instead of being overrun by the library's memset or read past its end (a field appended to
 * ptl_icp_cfg did exactly that to round 5's documented stub).  ptl_abi_version() / ptl_sizeof_cfg() let such a binding assert its
 * layout at load time (INTEGRATION.md section 2 does).  Bump PTL_ABI_VERSION with every change of a struct or a prototype; a new entry point
 * changes neither, so it does not bump the version. */
#define PTL_ABI_VERSION 6
#define PTL_CFG_ICP 0
#define PTL_CFG_EKF 1
#define PTL_CFG_SEQ 2
#define PTL_CFG_ICP_STATS 3
#define PTL_CFG_PKT_FORMAT 4
#define PTL_CFG_MAP_SCORE 5
#define PTL_CFG_INIT(cfg_ptr) do { memset((cfg_ptr), 0, sizeof *(cfg_ptr)); (cfg_ptr)->struct_size = (uint32_t)sizeof *(cfg_ptr); (cfg_ptr)->abi_version = PTL_ABI_VERSION; } while (0)
int ptl_abi_version(void);
/* the library's sizeof for PTL_CFG_ICP / _EKF / _SEQ / _ICP_STATS (the three configuration structs and the per-scan counter row),
 * PTL_CFG_PKT_FORMAT (ptl_pkt_format) and PTL_CFG_MAP_SCORE (ptl_map_score_cfg); -1 for an unknown id */
int64_t ptl_sizeof_cfg(int which);

const char *ptl_last_error(void);
/* 1 when a HIP device is usable (the only backend); never falls back to a CPU path */
int ptl_backend(void);
int ptl_device_count(void);
int ptl_device_sync(int device_id); /* hipDeviceSynchronize on that device */
/* Page-lock (hipHostRegister) / release a HOST buffer the caller will upload sweeps from - a recording read into memory, a capture ring:
 * the uploads (ptl_*_upload_scan / _range, synchronous copies) then go by DMA straight from it instead of through the runtime's staging
 * buffer (12.6 -> 2x GB/s on the measurement box, tools/stream_feed.py).  Optional; any buffer may be passed to the uploads unpinned. */
int ptl_host_pin(int device_id, void *host_ptr, uint64_t bytes);
int ptl_host_unpin(void *host_ptr);

/* ------------------------------------------------------------------------------------------------
 * ICP handle == reference KissICPWrapper (src/ptudes/kiss.py:18-166) + the kiss_icp.KissICP it owns
 * ---------------------------------------------------------------------------------------------- */
typedef struct ptl_icp ptl_icp;

typedef struct {
    uint32_t struct_size;         /* sizeof(ptl_icp_cfg) as the CALLER knows it - set before ptl_icp_default_cfg (PTL_CFG_INIT) */
    uint32_t abi_version;         /* PTL_ABI_VERSION as the caller knows it */
    /* algorithm parameters: reference kiss.py:40-43 + kiss-icp 0.2.10 config defaults */
    double max_range;             /* kiss.py:25, ekf_bench.py:360-363 */
    double min_range;             /* kiss.py:24,43 */
    double voxel_size;            /* max_range / 100 */
    int32_t max_points_per_voxel; /* 20 */
    double initial_threshold;     /* 2.0 */
    double min_motion_th;         /* 0.1 */
    int32_t deskew;               /* 1 (kiss.py:41) */
    int32_t max_iterations;       /* 500 */
    double convergence;           /* 1e-4 */
    /* device / capacity parameters (no reference counterpart) */
    int32_t device_id;
    int32_t scan_cols;            /* W: when t01 == NULL, point i gets t = (i % W) * (1/W) (kiss.py:34-35) */
    int64_t max_points_per_scan;  /* upper bound of n per register_frame */
    int64_t map_block_capacity;   /* voxel blocks in the local-map pool */
    int64_t map_table_capacity;   /* hash slots (power of two) */
    int32_t gn_workgroups;        /* workgroups of the persistent Gauss-Newton kernel */
    int32_t rebuild_every;        /* rebuild the map hash table every this many scans (drops tombstones) */
    int32_t gn_threads;           /* threads per workgroup of that kernel (multiple of 64, 256..1024) */
    int32_t gn_lanes_per_point;   /* 32: latency form (one point per 32 lanes, one sequence over the whole chip);
                                   * 8: throughput form (lane-per-point answer cache, 8 lanes per searched point, moment
                                   * accumulation; gn_threads <= 512) - what the batched runner uses per sequence, and the
                                   * faster form for dense scans (tens of thousands of source points) */
    int64_t map_small_blocks;     /* 0 (default): every voxel owns a full block of max_points_per_voxel points.  > 0: that many SMALL blocks
                                   * (one 128-byte line, 5 points) beside the map_block_capacity full ones - a voxel starts small and moves to a
                                   * full block when a batch takes it past 5 points.  For sparse maps (BASELINE config 5, 0.1 m voxels: 3.6
                                   * points per voxel): the pool shrinks to a third and a sparse voxel is one line.  Free-running batches only. */
} ptl_icp_cfg;

/* per-scan counters; identical meaning to oracle/oracle.h orc_icp_stats (SURVEY.md 8(d) byte model) */
typedef struct {
    double sigma;        /* kiss.py:99 */
    double err_dt;       /* kiss.py:118 (KissICPWrapper._err_dt) */
    double err_drot;     /* kiss.py:119-120 (KissICPWrapper._err_drot) */
    int32_t iterations;
    int32_t n_corr_last;
    int64_t n_in;
    int64_t n_valid;     /* N_v */
    int64_t n_down;      /* N_d */
    int64_t n_src;       /* N_s */
    int64_t sum_cand;    /* sum_i C_i */
    int64_t map_voxels;  /* M_v */
    int64_t map_points;
} ptl_icp_stats;

/* fills every field with the reference defaults for (max_range, min_range) (kiss.py:21-43); cfg->struct_size / abi_version must
 * already hold the caller's values (PTL_CFG_INIT) - a mismatch is refused with PTL_ERR_ARG and nothing is written */
int ptl_icp_default_cfg(ptl_icp_cfg *cfg, double max_range, double min_range);
/* KissICPWrapper.__init__ (kiss.py:21-52) */
int ptl_icp_create(const ptl_icp_cfg *cfg, ptl_icp **out);
int ptl_icp_destroy(ptl_icp *h);

/* KissICPWrapper.register_frame / _kiss_register_frame (kiss.py:54-131).
 * xyz: n x 3 (dtype PTL_F32 / PTL_F64), host memory; points with |p| outside (min_range, max_range)
 * are dropped, so RANGE==0 returns may be passed as (0,0,0) instead of being masked (kiss.py:59-60).
 * t01: n per-point normalised times (kiss.py:61) or NULL => column-implicit (cfg.scan_cols).
 * guess: 4x4 initial guess (ekf_bench.py:533-548) or NULL => constant-velocity prediction (kiss.py:102-105).
 * out_pose: poses[-1] after the call (kiss.py:74).  stats may be NULL. */
int ptl_icp_register_frame(ptl_icp *h, const void *xyz, int dtype, int64_t n, const double *t01,
                           double scan_ts, const double *guess, double out_pose[16], ptl_icp_stats *stats);
/* KissICPWrapper.poses / .pose (kiss.py:142-153): copies up to max poses (16 doubles each) */
/* Per-call registrations (ptl_icp_register_frame / _range) normally return after the scan's MAP UPDATE, because the statistics
 * row carries the map size.  on != 0: return as soon as the registration itself (the Gauss-Newton kernel) is done - what the
 * reference's register_frame returns is the pose (kiss.py:74) - while the map update runs beside the caller's next steps and the
 * next call's upload and K0-K4; stats->map_voxels / map_points are then -1 (ptl_icp_map_size gives them on demand) and an error
 * flag raised by that update is reported by the next call. */
int ptl_icp_set_lazy_map_stats(ptl_icp *h, int32_t on);
int ptl_icp_num_poses(ptl_icp *h, int64_t *n);
int ptl_icp_get_poses(ptl_icp *h, double *out, int64_t max_poses, int64_t *n_written);
/* kiss_icp.KissICP.get_prediction_model, used at ekf_bench.py:545 */
int ptl_icp_get_prediction(ptl_icp *h, double out[16]);
/* KissICPWrapper.local_map_points (kiss.py:159-161) */
int ptl_icp_map_size(ptl_icp *h, int64_t *voxels, int64_t *points);
int ptl_icp_map_points(ptl_icp *h, double *xyz_out, int64_t max_points, int64_t *n_written);
/* intermediates of the last register_frame, what _kiss_register_frame returns (kiss.py:131): frame_downsample, source */
int ptl_icp_last_frame_down(ptl_icp *h, double *xyz_out, int64_t max_points, int64_t *n_written);
int ptl_icp_last_source(ptl_icp *h, double *xyz_out, int64_t max_points, int64_t *n_written);

/* KissICPWrapper.deskew (kiss.py:76-78): motion-compensate `xyz` (n x 3 f64) with the last two poses; fewer than two
 * poses => returned unchanged */
int ptl_icp_deskew(ptl_icp *h, const double *xyz, const double *t01, int64_t n, double *out);

/* Stage-level entry points (teacher-forced parity checks of single kernels; kiss-icp 0.2.10 units):
 * VoxelHashMap::AddPoints + RemovePointsFarFromLocation on world-frame points */
int ptl_icp_map_add(ptl_icp *h, const double *xyz_world, int64_t n, const double origin[3], int prune);
/* GetCorrespondences + BuildLinearSystem for already-transformed source points: 21 JTJ upper + 6 JTr */
int ptl_icp_linear_system(ptl_icp *h, const double *src_world, int64_t n, double max_dist, double kernel,
                          double sums[27], int64_t *n_corr, int64_t *n_cand);
/* RegisterFrame: full Gauss-Newton loop of `frame` (sensor frame) against the current map */
int ptl_icp_align(ptl_icp *h, const double *frame, int64_t n, const double guess[16], double max_dist,
                  double kernel, double out_pose[16], int32_t *iterations);

/* ------------------------------------------------------------------------------------------------
 * Range-image input == ouster client.XYZLut as the reference uses it (kiss.py:28-29, 59-60) + reduce_active_beams
 * (utils.py:328-341).  SURVEY.md 8(f) rank 1: a sweep enters as a 512 KB u32 range image instead of 3 MB of xyz.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ptl_lut ptl_lut;
/* beam angles in degrees (H each), beam-origin offset in mm, lidar_to_sensor 4x4 with mm translation (SensorInfo
 * fields of the same names); extrinsic16_m (nullable): 4x4 with metre translation, applied on top
 * (use_extrinsics=True, ekf_bench.py:440-452) */
int ptl_lut_create(int device_id, int32_t H, int32_t W, const double *beam_altitude_deg, const double *beam_azimuth_deg,
                   double lidar_origin_to_beam_origin_mm, const double *lidar_to_sensor16_mm,
                   const double *extrinsic16_m, ptl_lut **out);
int ptl_lut_destroy(ptl_lut *l);
/* XYZLut.__call__: range image (H*W u32, mm, 0 = no return) -> H*W x 3 f64 metres */
int ptl_lut_apply(ptl_lut *l, const uint32_t *range_mm, double *xyz_out);
/* StreamStatsTracker.trackScan (reference ins/data.py:284-308): over the non-zero ranges of the rows
 * np.linspace(0, H, beams_num, endpoint=False, dtype=int) (all rows when beams_num <= 0), scaled by range_to_m
 * (0.001; 0.008 for the RNG15 profile, :242-252): out5 = {count, mean, population variance, min, max} */
int ptl_range_stats(int device_id, const uint32_t *range, int32_t H, int32_t W, int32_t beams_num, double range_to_m,
                    double out5[5]);
/* Posed scans for the map fly-by.
 * ouster.sdk.pose_util.TrajectoryEvaluator.poses_at as the reference uses it (utils.py:368 time_bounds 1.5,
 * cli/ekf_bench.py:489 time_bounds 1.0; third-party): pose at each of n timestamps on the SE(3) geodesic between the
 * bracketing knots (ts strictly increasing, poses 4x4 row-major); the first / last segment is extended by bound_before /
 * bound_after seconds; timestamps further out get the identity and are counted in n_outside (the reference skips them). */
int ptl_traj_poses_at(int device_id, const double *knot_ts, const double *knot_poses16, int64_t n_knots, double bound_before,
                      double bound_after, const double *ts, int64_t n, double *poses16_out, int64_t *n_outside);
/* ouster client.dewarp(XYZLut(scan), column_poses = scan.pose) (reference fly.py:75-86 through ScansAccumulator): world
 * xyz (H*W x 3 f64) of a range image whose W columns carry their own pose (W x 16).  As upstream, pixels without a
 * return land on their column's sensor origin; n_valid (nullable) counts the pixels with a return. */
int ptl_lut_dewarp(ptl_lut *l, const uint32_t *range_mm, const double *col_poses16, double *xyz_out, int64_t *n_valid);
/* rows kept active by reduce_active_beams(ls, beams_num); beams_num <= 0 = all rows.  Applies to range-image input. */
int ptl_icp_set_active_beams(ptl_icp *h, int32_t H, int32_t beams_num);
/* register_frame on a raw range image; per-pixel times are column-implicit (kiss.py:34-35) */
int ptl_icp_register_range(ptl_icp *h, ptl_lut *lut, const uint32_t *range_mm, double scan_ts, const double *guess,
                           double out_pose[16], ptl_icp_stats *stats);

/* profiling: HIP-event time of the dominant kernel (the persistent Gauss-Newton loop) since last reset; enable = n > 1
 * times every n-th launch only (the two event records cost ~18 us per scan) */
int ptl_icp_profile(ptl_icp *h, int enable, double *gn_ms_total, int64_t *gn_launches, int reset);
/* diagnostic: accumulated clock ticks of workgroup 0 per phase of that kernel (nn, wg-reduce+publish, barrier,
 * grid-reduce, solve) and out[5] = iterations, since the handle was created / reset */
int ptl_icp_gn_phases(ptl_icp *h, int64_t out[8]);
/* diagnostic: ticks each Gauss-Newton workgroup spent in the search phase since creation; out holds 2 * gn_workgroups
 * values (until the last / the first wavefront finished) */
int ptl_icp_gn_wg_clocks(ptl_icp *h, int64_t *out, int32_t max_wgs);
/* diagnostic: what the handle's last ptl_icp_linear_system left on the device: [0..27) the sums, [27] the pair count, [28] the
 * candidate count, the rest 0 (all 0 after a cold start).  The diagnostic builds' values are read with ptl_icp_diag. */
int ptl_icp_debug_sums(ptl_icp *h, double out[32]);
/* diagnostic builds (csrc/diag.h: make PHASES=1, IT0=1, STAGES=1, EXTRA=-DMAP_DIAG; ptl_build_info [13]): every value they collect has a
 * named 64-bit slot.  ptl_diag_slots() of them, slot i named ptl_diag_slot_name(i) (a static string; null outside the range);
 * ptl_icp_diag copies them all (max_slots >= ptl_diag_slots()), cumulative since the handle's cold start, all 0 in the product build.
 * With ptl_batch_icp / ptl_seq_icp it reads a member of a runner between its launches. */
int ptl_diag_slots(void);
const char *ptl_diag_slot_name(int slot);
int ptl_icp_diag(ptl_icp *h, int64_t *out, int32_t max_slots);
/* test hook: workgroup `wg` of the following Gauss-Newton launches returns at once (-1 = back to normal, also clears the
 * time-out flag): the others must run into the exchange time-out, abort together and report it - not hang */
int ptl_icp_debug_stall_workgroup(ptl_icp *h, int32_t wg);
/* test hook: at most `free_blocks` free voxel blocks left in the pool (< 0: unchanged), `table_used` map-table entries declared
 * taken (< 0: unchanged): the following map updates raise the pool / table capacity flags (PTL_ERR_CAPACITY at the next wait) */
int ptl_icp_debug_limit_capacity(ptl_icp *h, int32_t free_blocks, int64_t table_used);
/* test hook: a read-only dump of the handle's map table.  Waits for the handle's map stream and main stream, then copies to the host
 * (every array nullable): `entries` - the table's slots, 16 bytes each: u64 key (all ones = empty, all ones - 1 = tombstone; else the
 * voxel's three indices + 2^20 in 21 bits each, x highest), i32 block id | stored count << 24 (-1 = none), i32 list head; `bhdr` - the block
 * directory, 4 i32 per block: stored count, table slot, batch points pending, pad; `bfirst` - 3 doubles per block, the voxel's first point.
 * info: [0] table entries created since the last rebuild (tombstones included), [1] live voxels, [2] the device error flags (returned,
 * not raised), [3] slots - 1 of the map table, [4] / [5] of the pass-1 / pass-2 per-scan voxel tables, [6] blocks in the directory,
 * [7] small blocks among them.  max_slots / max_blocks below [3] + 1 / [6]: PTL_ERR_CAPACITY.  No kernel runs and nothing on the device
 * changes.  With ptl_batch_icp / ptl_seq_icp it serves the members of a runner between its launches. */
int ptl_icp_debug_table(ptl_icp *h, void *entries, int64_t max_slots, int32_t *bhdr, double *bfirst, int64_t max_blocks, int64_t info[8]);
/* test hook: set the 22-bit launch epoch of the Gauss-Newton exchange (exercises its wrap-around) */
int ptl_icp_debug_set_epoch(ptl_icp *h, uint32_t epoch);

/* ------------------------------------------------------------------------------------------------
 * EKF handle == reference ESEKF (src/ptudes/ins/es_ekf.py:57-365)
 * ---------------------------------------------------------------------------------------------- */
typedef struct ptl_ekf ptl_ekf;

typedef struct {
    uint32_t struct_size; /* sizeof(ptl_ekf_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double init_grav[3]; /* es_ekf.py:75 */
    double init_bacc[3]; /* es_ekf.py:76 */
    double init_bgyr[3]; /* es_ekf.py:77 */
    int32_t device_id;
} ptl_ekf_cfg;

int ptl_ekf_default_cfg(ptl_ekf_cfg *cfg);
int ptl_ekf_create(const ptl_ekf_cfg *cfg, ptl_ekf **out);        /* ESEKF.__init__  (:73-179) */
int ptl_ekf_destroy(ptl_ekf *h);
/* processImu (:191-237) and processPose (:259-329) only queue their launch (the payload travels in the kernel
 * arguments): they return before the step has run; ptl_ekf_get_state / pose_mat / ts wait for it */
int ptl_ekf_process_imu(ptl_ekf *h, const double lacc[3], const double avel[3], double ts);
/* batch form: imu is n x 7 rows (ts, lacc[3], avel[3]); one launch for the whole batch */
int ptl_ekf_process_imu_batch(ptl_ekf *h, const double *imu, int64_t n);
int ptl_ekf_process_pose(ptl_ekf *h, const double pose[16], const double *meas_cov36);
/* nav[19] = pos(3) quat_xyzw(4) vel(3) bias_gyr(3) bias_acc(3) grav(3) (ESEKF.nav, :181-184); cov 18x18 (._cov) */
int ptl_ekf_get_state(ptl_ekf *h, double nav[19], double cov[324]);
int ptl_ekf_pose_mat(ptl_ekf *h, double T[16]); /* NavState.pose_mat (ins/data.py:70-74) */
int ptl_ekf_ts(ptl_ekf *h, double *ts);         /* ESEKF.ts (:186-189) */

/* Fixed-interval Rauch-Tung-Striebel smoother over the filter's own history (no reference counterpart: the reference's filter is causal).
 * While the log is on, every pose update appends one entry (8 KB, fp64) to a device log: the filter's time, the state and covariance
 * before the update (x_{k|k-1}, P_{k|k-1}), the product Phi of the IMU transitions Fx since the previous update, and the state and
 * covariance after it (x_{k|k}, P_{k|k}).  The filter's arithmetic does not change: its outputs are bit-identical with the log on or off.
 * The backward pass (one workgroup per filter) gives, per logged update in update order, the smoothed 4x4 pose (the res_poses form), its
 * timestamp, optionally the smoothed nav[19] (ptl_ekf_get_state's layout) and P^s (18x18); every output but poses16 may be NULL.
 * A full log stops writing and the smoothing call returns PTL_ERR_CAPACITY; smoothing without a log returns PTL_ERR_STATE, and so does a
 * P_{k+1|k} that is not positive definite (ptl_last_error() names the entry).  A failed call leaves the handle usable.
 * ptl_ekf_log_enable: a fresh, empty log for `capacity` updates (0 = off, frees it). */
int ptl_ekf_log_enable(ptl_ekf *h, int64_t capacity);
/* copies up to max_rows rows; *n_rows (nullable) = rows copied */
int ptl_ekf_smooth(ptl_ekf *h, double *poses16, double *ts, double *nav19, double *cov324, int64_t max_rows, int64_t *n_rows);
/* The raw log: up to max_entries entries of PTL_SMOOTHER_LOG_STRIDE doubles each (layout below; the rest of an entry is padding);
 * *n_entries = entries logged (nullable); *overflow (nullable) = 1 once an update found the log full */
#define PTL_SMOOTHER_LOG_STRIDE 1024
#define PTL_SMOOTHER_LOG_TS 0          /* the filter's time at the update (= res_t) */
#define PTL_SMOOTHER_LOG_NAV_PRED 1    /* nav[19] before the update, x_{k|k-1} */
#define PTL_SMOOTHER_LOG_P_PRED 20     /* 18x18 before the update, P_{k|k-1} */
#define PTL_SMOOTHER_LOG_PHI 344       /* 18x18 product of the IMU transitions Fx since the previous logged update, Phi_{k-1->k} */
#define PTL_SMOOTHER_LOG_NAV_POST 668  /* nav[19] after the update, x_{k|k} */
#define PTL_SMOOTHER_LOG_P_POST 687    /* 18x18 after the update, P_{k|k} */
int ptl_ekf_smoother_log(ptl_ekf *h, double *entries, int64_t max_entries, int64_t *n_entries, int32_t *overflow);

/* ------------------------------------------------------------------------------------------------
 * Whole-sequence runner == the reference's driver loop (cli/ekf_bench.py:493-563) on a pre-uploaded
 * sequence: all scans + IMU samples resident in HBM, no host round trip per scan.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ptl_seq ptl_seq;

typedef struct {
    uint32_t struct_size; /* sizeof(ptl_seq_cfg) as the caller knows it (PTL_CFG_INIT); icp and ekf carry their own */
    uint32_t abi_version;
    ptl_icp_cfg icp;
    ptl_ekf_cfg ekf;
    int64_t n_scans;
    int64_t points_per_scan;    /* H * W, every scan has exactly this many (invalid returns = (0,0,0)) */
    int64_t n_imu;
    int32_t use_imu_prediction; /* ekf_bench.py:533-535 */
    int32_t with_ekf;           /* 0 => ICP only (BASELINE config 2) */
    int32_t range_input;        /* batches: 1 => every sweep arrives as a raw range image (ptl_batch_set_lut + ptl_batch_upload_range) and is KEPT as
                                 * one: 4 resident bytes per pixel instead of the 12 of a float32 xyz sweep - 240 sequences x 1 000 sweeps of 128x1024 are
                                 * 126 GB instead of 377 GB (the reference walks a recording of any length, data.py:31-77).  ptl_batch_upload_scan is then
                                 * refused.  0 (default): 12-byte slots, either form may be uploaded.  Ignored by ptl_seq_create. */
    int32_t resident_scans;     /* batches, free-running driver: 0 (default) = every sweep of the run resident (n_scans slots per sequence).  R >= 2 = a RING of
                                 * R sweep slots per sequence - a recording of any length at the full batch width (the reference walks a file scan by scan,
                                 * data.py:31-77, cli/ekf_bench.py:493-563): sweeps are uploaded in order, sweep k takes slot k % R once scan k - R is known
                                 * to be complete (ptl_batch_wait), and uploads of later sweeps may run while a launch works on earlier ones - between
                                 * ptl_batch_enqueue and ptl_batch_wait, or from another host thread (the only calls of a handle that may overlap).
                                 * ptl_batch_enqueue refuses scans whose sweeps are not there.  Ignored by ptl_seq_create. */
} ptl_seq_cfg;

int ptl_seq_create(const ptl_seq_cfg *cfg, ptl_seq **out);
int ptl_seq_destroy(ptl_seq *s);
/* host -> HBM: scan k (points_per_scan x 3 float32, row-major beam-outer) */
int ptl_seq_upload_scan(ptl_seq *s, int64_t k, const float *xyz);
/* the same sweep as a raw range image (points_per_scan u32, mm, 0 = no return): 1/3 of the bytes; the LUT (and
 * optionally reduce_active_beams) must be set with ptl_seq_set_lut before the run */
int ptl_seq_upload_range(ptl_seq *s, int64_t k, const uint32_t *range_mm);
int ptl_seq_set_lut(ptl_seq *s, ptl_lut *lut, int32_t active_beams);
/* imu: n_imu x 7 (ts, lacc, avel); imu_end[k] = number of IMU samples that precede scan k in the event stream */
int ptl_seq_upload_imu(ptl_seq *s, const double *imu, const int64_t *imu_end);
/* cold-start the filters/map and run scans [0, n) (n <= n_scans); returns after the stream has drained */
int ptl_seq_run(ptl_seq *s, int64_t n);
/* continue with the next n scans from where the last run / advance stopped (state kept) */
int ptl_seq_advance(ptl_seq *s, int64_t n);
/* the same split in two: enqueue the next n scans on the handle's stream without waiting, then wait + check
 * device error flags (lets several sequences on one GPU overlap on their own streams) */
int ptl_seq_enqueue(ptl_seq *s, int64_t n);
int ptl_seq_wait(ptl_seq *s);
/* res_poses (n x 16), res_t (n), kiss_poses (n x 16), stats (n): any may be NULL; n_out = scans processed
 * (scans with no IMU since the previous one are skipped when with_ekf, ekf_bench.py:512-518) */
int ptl_seq_results(ptl_seq *s, double *res_poses, double *res_t, double *kiss_poses, ptl_icp_stats *stats,
                    int64_t max_n, int64_t *n_out);
/* device pointer + row count of the (T x 8) NC-GT rows [t, x,y,z, qx,qy,qz,qw] of the last run, for the
 * RCCL trajectory gather (no host copy) */
int ptl_seq_traj_device(ptl_seq *s, void **dev_ptr, int64_t *rows);
/* device-to-device copy of those rows into a caller-owned DEVICE buffer (e.g. a torch tensor's data_ptr) */
int ptl_seq_copy_traj(ptl_seq *s, void *dst_device, int64_t max_rows, int64_t *rows);
int ptl_seq_icp(ptl_seq *s, ptl_icp **icp);
/* The smoother (see ptl_ekf_log_enable) for the sequence's filter: capacity n_scans, refused (PTL_ERR_STATE) when with_ekf == 0.  A cold
 * start (ptl_seq_run) empties the log, ptl_seq_advance / _enqueue continue it.  The rows of ptl_seq_smooth (n_scans capacity in every
 * buffer) align one for one with the rows of ptl_seq_results: a scan skipped for want of IMU samples has no update and no entry. */
int ptl_seq_smoother_enable(ptl_seq *s, int32_t on);
int ptl_seq_smooth(ptl_seq *s, double *poses16, double *ts, double *nav19, double *cov324, int64_t *n_rows);
int ptl_seq_smoother_log(ptl_seq *s, double *entries, int64_t max_entries, int64_t *n_entries, int32_t *overflow);
int ptl_seq_profile(ptl_seq *s, int enable, double *gn_ms_total, int64_t *gn_launches, int reset);

/* One scan of the reference's loop body (cli/ekf_bench.py:493-563) for the per-call handles in ONE host round trip: the n_imu IMU samples
 * that precede the scan (rows [ts, lacc(3), avel(3)]: ESEKF.processImu each, es_ekf.py:191-237), the registration (kiss.py:83-131) with
 * the filter's pose as its guess (use_imu_prediction, ekf_bench.py:533-535), else `guess` (nullable: the constant-velocity model),
 * ESEKF.processPose with the new pose (es_ekf.py:259-329).  kiss_pose = the registration's pose, ekf_pose / ekf_ts = the filter's pose
 * after the update and its timestamp (what the loop appends, ekf_bench.py:561-563); any output may be NULL.  Same kernels and order as
 * the separate calls - same bits - with the hand-overs done on the device (the host waits once instead of three times). */
int ptl_icp_ekf_step(ptl_icp *icp, ptl_ekf *ekf, const double *imu_rows, int64_t n_imu, const void *xyz, int dtype, int64_t n,
                     const double *t01, const double *guess, int32_t use_imu_prediction, double kiss_pose[16],
                     double ekf_pose[16], double *ekf_ts, ptl_icp_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Batched runner: up to 256 independent sequences on ONE GPU.  The sequences s = x (mod 8) live on XCD x (their maps,
 * probe rows and exchange stay in its L2); the workgroups with blockIdx & 7 == x form 1 / 2 / 4 teams of gn_workgroups /
 * 8, / 16, / 32 workgroups (<= 8 / <= 16 / <= 64 sequences), 8 teams for up to 128 sequences, 16 beyond
 * (ptl_batch_set_team_workgroups overrides).  Two drivers, see ptl_batch_set_driver: the free-running
 * kernel (default) and lockstep (one launch per stage for all sequences, <= 32 sequences).  Each sequence's results are
 * bit-identical to running it alone with a team's workgroups and the same gn_lanes_per_point.  cfg describes every sequence (same n_scans / points_per_scan / n_imu; gn_workgroups = 8 x
 * workgroups per XCD); with_ekf requires >= 1 IMU sample between consecutive scans.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ptl_batch ptl_batch;
int ptl_batch_create(const ptl_seq_cfg *cfg, int32_t n_sequences, ptl_batch **out);
int ptl_batch_destroy(ptl_batch *b);
int ptl_batch_upload_scan(ptl_batch *b, int32_t seq, int64_t k, const float *xyz);
int ptl_batch_set_lut(ptl_batch *b, ptl_lut *lut, int32_t active_beams);
int ptl_batch_upload_range(ptl_batch *b, int32_t seq, int64_t k, const uint32_t *range_mm);
int ptl_batch_upload_imu(ptl_batch *b, int32_t seq, const double *imu, const int64_t *imu_end);
int ptl_batch_run(ptl_batch *b, int64_t n);     /* cold start + scans [0, n), waits */
int ptl_batch_enqueue(ptl_batch *b, int64_t n); /* next n scans, does not wait */
int ptl_batch_wait(ptl_batch *b);
int ptl_batch_results(ptl_batch *b, int32_t seq, double *res_poses, double *res_t, double *kiss_poses,
                      ptl_icp_stats *stats, int64_t max_n, int64_t *n_out);
int ptl_batch_copy_traj(ptl_batch *b, int32_t seq, void *dst_device, int64_t max_rows, int64_t *rows);
/* The smoother (see ptl_ekf_log_enable, ptl_seq_smoother_enable) for every sequence of the batch, either driver, resident or sweep ring.
 * ptl_batch_run / _reset empty the logs, ptl_batch_enqueue continues them.  ptl_batch_smooth: one launch smooths every sequence and waits;
 * ptl_batch_smoothed then copies sequence seq's rows (n_scans capacity in every buffer; PTL_ERR_STATE when nothing was smoothed since the
 * last run / enqueue). */
int ptl_batch_smoother_enable(ptl_batch *b, int32_t on);
int ptl_batch_smooth(ptl_batch *b);
int ptl_batch_smoothed(ptl_batch *b, int32_t seq, double *poses16, double *ts, double *nav19, double *cov324, int64_t *n_rows);
int ptl_batch_smoother_log(ptl_batch *b, int32_t seq, double *entries, int64_t max_entries, int64_t *n_entries, int32_t *overflow);
int ptl_batch_gn_phases(ptl_batch *b, int64_t out[8]); /* like ptl_icp_gn_phases, for the shared launch */
int ptl_batch_icp(ptl_batch *b, int32_t seq, ptl_icp **icp); /* the ICP handle of one sequence (diagnostics, map export) */
int ptl_batch_profile(ptl_batch *b, int enable, double *gn_ms_total, int64_t *gn_launches, int reset);
/* Which driver advances the batch (choose before the first scan of a run):
 *   free_running != 0 (the default when gn_lanes_per_point = 8): one persistent launch (kx_seq_run) carries up to
 *     scans_per_launch scans (0 = keep, default 256) of EVERY sequence; the workgroups of a sequence walk its whole
 *     per-scan pipeline - reference cli/ekf_bench.py:493-563 - at their own pace, so a sequence whose Gauss-Newton loop
 *     converges early starts its next scan instead of waiting for the slowest one.  ptl_batch_profile then times these
 *     launches.  Needs gn_lanes_per_point = 8 and a grid whose workgroups can all be resident (checked here, or at the
 *     first enqueue when the driver is the default); scans_per_launch <= 4096.
 *   free_running == 0: lockstep, one launch per stage for all sequences; a step lasts as long as its slowest sequence.
 * Same results either way (bit-identical). */
int ptl_batch_set_driver(ptl_batch *b, int32_t free_running, int64_t scans_per_launch);
/* back to the cold start (empty maps, fresh filters, scan 0 next) without running anything - what ptl_batch_run does first;
 * after it the driver and the team size may be chosen again for the same handle and the same uploaded sweeps */
int ptl_batch_reset(ptl_batch *b);
/* phase clocks of sequence s in the free-running kernel, 100 MHz wall-clock ticks summed since the cold start:
 * workgroup 0's K0-K4 | its wait before the Gauss-Newton loop | the loop | its wait after it | its map update;
 * out[5] the filter workgroup's step; out[6] scans */
int ptl_batch_seq_clocks(ptl_batch *b, int32_t seq, int64_t out[8]);
/* Team size of the free-running kernel: `team_workgroups` workgroups (1 .. min(64, gn_workgroups / 8); 0 = the default for
 * the number of sequences) walk one scan of one sequence together; an XCD's gn_workgroups / 8 / team_workgroups teams serve
 * its sequences scan by scan.  Smaller teams spread the per-iteration fixed costs of the Gauss-Newton loop (workgroup
 * reduction, exchange, 6x6 solve) over more points each and want more sequences in flight; the results of a sequence
 * are those of a run alone with `team_workgroups` workgroups.  Before the first scan of a run. */
int ptl_batch_set_team_workgroups(ptl_batch *b, int32_t team_workgroups);
int ptl_batch_team_workgroups(ptl_batch *b, int32_t *team_workgroups, int32_t *teams /* nullable: teams that can get work */);
/* Executed-work counters of sequence `seq`, cumulative since the cold start - what the kernels requested from memory, as
 * opposed to the brute-force counts of ptl_icp_stats: [0] full 27-voxel searches (points the answer cache did not
 * settle), [1] probe rows rebuilt (27 hash probes each), [2] stored map points read by the searches, [3] Gauss-Newton
 * iterations, [4] / [5] voxel claims of down-sampling pass 1 / 2, [6] source point-iterations, [7] scans, [8] point-iterations settled as
 * "nothing in reach" (the point's last search found its 27 voxels empty and it has not left its voxel: neither a row evaluation nor a
 * search - exact, the map does not change inside a registration), [9] frame_downsample points the map update dropped where it found
 * their voxel already holding max_points_per_voxel points (no list push, no world-frame copy, nothing for the later phases to walk),
 * [10..15] reserved (0). */
int ptl_batch_exec_counters(ptl_batch *b, int32_t seq, uint64_t out[16]);
/* Where the scans of sequence `seq` ran in the free-running kernel, cumulative since the cold start: out[0] scans run by a
 * team of another XCD than the sequence's home XCD (seq & 7) - a team whose own XCD had nothing for it; out[1] scans that
 * ran on another XCD than the sequence's previous scan (the cross-XCD hand-overs: the previous scan's data sits in another
 * L2); out[2] XCC id of the last scan + 1; out[3] reserved. */
int ptl_batch_sched_counters(ptl_batch *b, int32_t seq, uint64_t out[4]);
/* Sticky status word of the free-running driver (cleared by ptl_batch_run / ptl_batch_reset): why teams left a launch
 * other than "all scans done" - 1 a teammate never reached the head-of-launch barrier, 2 ... the job barrier, 4 a team
 * found no work for its whole idle budget while sequences were pending, 8 a team gave up on a sequence (see that
 * sequence's error flags), 16 a sequence did not reach the last scan of a launch (it gets the time-out flag).
 * ptl_batch_wait returns PTL_ERR_CAPACITY for a flagged sequence and PTL_ERR_STATE for a status without one (bit 4 alone -
 * a team that only idled past its budget while every sequence reached its last scan - is reported here, not as an error):
 * no exit of the persistent kernel is silent. */
int ptl_batch_status(ptl_batch *b, uint32_t *status);
/* test hook: workgroup `block` of the free-running grid returns right before the job barrier of its `round`-th job of every
 * launch from now on (0 = the first); block < 0 switches it off */
int ptl_batch_debug_stall_block(ptl_batch *b, int32_t block, int32_t round);
/* test hook: points per thread and pass of the free-running kernel's map update (reference kiss.py:129) - 0 = only ask, else the
 * build's default (8) or its second instance (4); *points_out = the value in effect.  Results must not depend on it. */
int ptl_batch_debug_set_map_points_per_thread(ptl_batch *b, int32_t points, int32_t *points_out);
/* Environment: PTL_TEAM_SYNC=agent when the batch is created keeps the agent-scope release (L2 write-back) at every team
 * barrier of the free-running kernel instead of the XCD-local shortcut (same results; a diagnostic switch).
 * PTL_SCHED_MARGIN=n (default 1): a team takes the least-advanced free sequence of ANOTHER XCD as soon as it is n scans behind its own
 * XCD's least-advanced one (all sequences of the device stay within a scan of each other); -1 = only when its own XCD has nothing left.
 *
 * Memory: one sequence of a batch holds 480 B per point of points_per_scan of work buffers (probe and answer rows, ...:
 * 63 MB at 128x1024), its two per-scan voxel tables (64 and 16 slots of 16 B per point: 134 + 34 MB - sparse on purpose,
 * a taken line costs a claim a dependent read), map_table_capacity x 16 B (256 MB at the default 2^24 slots: sparse for
 * the same reason, see ptl_icp_default_cfg), map_block_capacity x (block size + 44) B (512-B blocks of points at 20 points per
 * voxel, 40 B of block directory - header and first point - and 4 B of free stack each: 278 MB at the default 512 k blocks),
 * map_small_blocks x (128 + 48) B when the second block class is on, and its resident sweeps (n_scans x points_per_scan x 12 B):
 * ~790 MB + sweeps at the defaults.  ptl_batch_create checks the sum against
 * hipMemGetInfo and fails with PTL_ERR_CAPACITY and the numbers when it does not fit. */

/* Compile-time constants of the loaded build that a caller's byte model depends on (bench.py EXEC_COST): [0] candidates
 * per answer row, [1] doubles per answer row, [2] source positions a workgroup keeps in LDS, [3] / [4] points per thread
 * and pass of K1 + map update / K2-K4 in the free-running kernel, [5] threads per workgroup of the 8-lane kernels,
 * [6] lanes per point of the full search, [7] nearest other boxes in its first round, [8] voxels per survivor round,
 * [9] chunks phase A requests ahead, [10] 1000 x the pruning margin, [11] / [12] bytes per map-table / voxel-table
 * entry, [13] the diagnostic flavours compiled in, a bit each: 1 PHASES, 2 IT0, 4 STAGES, 8 MAP_DIAG (0 = the product build), [14] reserved (0; rounds 5's movement-budget experiment is gone from the sources),
 * [15] candidates that ptl_icp_pose_hits stages and processes at a time. */
int ptl_build_info(int32_t out[16]);
/* identity of what THIS library was built from: sha256 over the kernel sources, the Makefile and the experiment flags (12 hex digits,
 * csrc/Makefile CODE_ID).  bench.py records it in its line and tools/pmc_summary.py in every counter summary: a counter pass speaks
 * for the build it ran on, whatever the source tree looks like by then. */
const char *ptl_code_id(void);

/* ---- multi-GPU: the final trajectory gather.  The reference has no distributed layer; the path shards
 * across independent sequences only (one rank per GPU, no data-path collective) and its ONE collective is the all-gather of every
 * rank's NC-GT rows [t, x, y, z, qx, qy, qz, qw] (reference utils.py:191-252 writes such rows) after the run: ncclAllGather straight
 * from librccl (opened on first use; PTL_RCCL_PATH overrides the search), RCCL over xGMI on the node.
 * The library does no bootstrap: ONE rank calls ptl_comm_unique_id, the caller carries the PTL_COMM_ID_BYTES bytes to the other ranks
 * (environment, file, gloo / MPI / TCP - its business), EVERY rank then calls ptl_comm_create (collective: returns when all have). */
#define PTL_COMM_ID_BYTES 128
typedef struct ptl_comm ptl_comm;
int ptl_comm_unique_id(uint8_t id[PTL_COMM_ID_BYTES]);
int ptl_comm_create(const uint8_t id[PTL_COMM_ID_BYTES], int32_t world, int32_t rank, int32_t device_id, ptl_comm **out);
int ptl_comm_destroy(ptl_comm *c);
/* Every rank: d_rows = S x T x 8 doubles in DEVICE memory (sequence-major, rows beyond a sequence's count are padding),
 * counts = S valid row counts (host); S and T equal on every rank.  On return, on every rank, rows_out [world][S][T][8] and
 * counts_out [world][S] (host) hold everybody's. */
int ptl_gather_trajectories(ptl_comm *c, const double *d_rows, int64_t S, int64_t T, const int64_t *counts,
                            double *rows_out, int64_t *counts_out);
/* ... the rows a batch's filter kernel wrote on device (what ptl_batch_copy_traj copies), T = the batch's n_scans:
 * rows_out [world][n_sequences][n_scans][8], counts_out [world][n_sequences] */
int ptl_batch_gather_trajectories(ptl_batch *b, ptl_comm *c, double *rows_out, int64_t *counts_out);

/* ------------------------------------------------------------------------------------------------
 * IMU deskew (no reference counterpart: kiss-icp deskews with its constant-velocity model).  Optional, for the
 * filter-coupled paths: the fused per-call step, ptl_seq_* and ptl_batch_* under both drivers.  Off: nothing changes, bit for bit.
 *
 * Knots.  The filter records (ts, pos[3], q xyzw[4]) of its nominal pose (world <- body, ptl_ekf_pose_mat's convention): knot 0 is the
 * state right after the most recent pose update (before any update: after the filter's first IMU sample), then one knot per IMU sample
 * consumed after it, taken after that sample's mechanisation; a sample whose ts does not exceed the previous knot's adds none.  Every pose
 * update restarts the list.  A knot that does not fit raises the overflow flag (sticky until a cold start): the run then returns
 * PTL_ERR_CAPACITY, and the scans that follow are not deskewed.
 * Sweep times.  Per scan, absolute (t0, t1) on the IMU clock; column j (t01 = j / W) is at t_j = t0 + (j / W)(t1 - t0).
 * Reference instant.  t_ref = the last knot's time = the filter's time at this scan's update (= res_t): column j is moved by
 * M_j = T(t_ref)^-1 T(t_j), so the registered pose, the IMU-prediction guess and the filter update refer to one instant (the constant-
 * velocity mode refers to mid-sweep).
 * Interpolation.  T(t) = P_i Exp(a Log(P_i^-1 P_i+1)), a = (t - kt_i) / (kt_i+1 - kt_i), i the largest index with kt_i <= t clamped to
 * [0, n - 2] (ptl_traj_poses_at's form); outside the knots the end segment's twist extrapolates, by at most the largest knot interval.
 * Fallback.  Fewer than 2 knots, an overflowed list, or a column beyond that bound: no deskew for the scan (mode 0, like kiss-icp's first
 * two scans).  ptl_*_deskew_modes give the mode per scan: 0 none, 1 constant velocity, 2 IMU.
 * Refused (PTL_ERR_ARG / PTL_ERR_STATE, the handle stays usable): the mode without a filter (with_ekf = 0) or with deskew off, explicit
 * per-point t01, a run without sweep times, a knot capacity below what the IMU samples between two scans need, and (ptl_seq) a scan
 * without a new IMU sample (the driver loop would skip it).  Enable at a cold start: a reset keeps the mode, the knot list starts empty. */
#define PTL_KNOT_STRIDE 8   /* doubles per knot: */
#define PTL_KNOT_TS 0       /* the filter's time */
#define PTL_KNOT_POS 1      /* pos[3], world */
#define PTL_KNOT_Q 4        /* q xyzw[4], world <- body */
#define PTL_DESKEW_NONE 0
#define PTL_DESKEW_CV 1
#define PTL_DESKEW_IMU 2
/* capacity >= 2: a fresh, empty knot list (0 = off, frees it); the raw list, up to max_knots knots (n_knots: its length) */
int ptl_ekf_knots_enable(ptl_ekf *h, int64_t capacity);
int ptl_ekf_knots(ptl_ekf *h, double *knots, int64_t max_knots, int64_t *n_knots, int32_t *overflow);
/* ptl_icp_ekf_step with the scan's table from the filter's knots (the filter needs ptl_ekf_knots_enable with capacity >= n_imu + 1):
 * sweep times t0 <= t1 instead of t01; the prologue waits for the predicts instead of running beside them.  The handle's other entry
 * points keep the constant-velocity deskew. */
int ptl_icp_ekf_step_imu_deskew(ptl_icp *icp, ptl_ekf *ekf, const double *imu_rows, int64_t n_imu, const void *xyz, int dtype, int64_t n,
                                double t0, double t1, const double *guess, int32_t use_imu_prediction, double kiss_pose[16],
                                double ekf_pose[16], double *ekf_ts, ptl_icp_stats *stats);
/* mode per registered scan of a per-call handle (n: scans written); the current column table, 12 x W doubles entry-major (R row-major 9,
 * t 3; entry q of column j at [q W + j]), for tests */
int ptl_icp_deskew_modes(ptl_icp *h, int32_t *modes, int64_t max_n, int64_t *n);
int ptl_icp_column_table(ptl_icp *h, double *out);
/* the sequence runner: on / off (knot_capacity for the filter's list), sweep times (n_scans x 2), modes of the scans run, raw knots */
int ptl_seq_imu_deskew_enable(ptl_seq *s, int32_t on, int64_t knot_capacity);
int ptl_seq_upload_sweep_times(ptl_seq *s, const double *t0t1);
int ptl_seq_deskew_modes(ptl_seq *s, int32_t *modes, int64_t max_n, int64_t *n);
int ptl_seq_knots(ptl_seq *s, double *knots, int64_t max_knots, int64_t *n_knots, int32_t *overflow);
/* ... every sequence of a batch (sweep times stay resident for all n_scans, also with the sweep ring: 16 B per scan) */
int ptl_batch_imu_deskew_enable(ptl_batch *b, int32_t on, int64_t knot_capacity);
int ptl_batch_upload_sweep_times(ptl_batch *b, int32_t seq, const double *t0t1);
int ptl_batch_deskew_modes(ptl_batch *b, int32_t seq, int32_t *modes, int64_t max_n, int64_t *n);
int ptl_batch_knots(ptl_batch *b, int32_t seq, double *knots, int64_t max_knots, int64_t *n_knots, int32_t *overflow);

/* ------------------------------------------------------------------------------------------------
 * Posed scans into the world map (reference cli/flyby.py:71-131, utils.py:344-392, fly.py:75-111).  Every lidar column gets
 * its pose on a time-stamped trajectory, the sweep is de-warped with them and its returns are added to the voxel map of a ptl_icp used as a
 * map container (like ptl_icp_map_add) - on the device, in scan order: the result equals ptl_traj_poses_at -> ptl_lut_dewarp -> the rows
 * with a return -> ptl_icp_map_add bit for bit (one definition of the arithmetic, csrc/fly_kernels.h), without the two trips through the host.
 * A scan with ANY column outside [first knot - bound_before, last knot + bound_after] is skipped as a whole (reference utils.py:379-384).
 * Work buffers are the map handle's (nothing is allocated per scan, a runner is only read); map, trajectory, LUT and runner on one device
 * (else PTL_ERR_ARG); W = the map handle's scan_cols and H W <= its max_points_per_scan (else PTL_ERR_CAPACITY); pool / table exhaustion
 * is reported as ptl_icp_map_add reports it.  Per scan 8 bytes (count, flag) come back beside that error word; a multi-scan build
 * reads its two totals once, at its end. */
typedef struct ptl_traj ptl_traj; /* a time-stamped trajectory resident on a device */
/* validation as ptl_traj_poses_at (>= 2 knots, strictly increasing: PTL_ERR_ARG naming the knot), BEFORE any HIP call */
int ptl_traj_create(int device_id, const double *knot_ts, const double *knot_poses16, int64_t n_knots, double bound_before,
                    double bound_after, ptl_traj **out);
int ptl_traj_destroy(ptl_traj *t);
/* one posed scan: a range image with its LUT, or H x W f32 xyz in the sensor frame with (0,0,0) = no return; col_ts: W seconds.
 * *n_valid = returns added (nullable), *skipped = 1 when a column lay outside the bounds and nothing was added (nullable) */
int ptl_icp_map_add_posed_range(ptl_icp *map, ptl_traj *t, ptl_lut *lut, const uint32_t *range_mm, const double *col_ts,
                                int64_t *n_valid, int32_t *skipped);
int ptl_icp_map_add_posed_xyz(ptl_icp *map, ptl_traj *t, const float *xyz, int32_t H, int32_t W, const double *col_ts,
                              int64_t *n_valid, int32_t *skipped);
/* the RESIDENT sweeps [first, last] of a runner, no sweep crosses the bus: column j of sweep k fires at
 * t0t1[2k] + (j / W)(t0t1[2k+1] - t0t1[2k]) (the IMU deskew's convention above); t0t1: n_scans x 2, host.  Waits for the runner's own
 * streams first and never writes to the runner (its later scans are bit-identical).  PTL_ERR_STATE: range images without a LUT, a batch
 * with a sweep ring (resident_scans: its sweeps are gone).  One sequence per call (a map handle is 0.5 GB at the defaults). */
int ptl_seq_map_build(ptl_seq *s, ptl_icp *map, ptl_traj *t, const double *t0t1, int64_t first, int64_t last, int64_t *n_valid,
                      int64_t *n_skipped);
int ptl_batch_map_build(ptl_batch *b, int32_t seq, ptl_icp *map, ptl_traj *t, const double *t0t1, int64_t first, int64_t last,
                        int64_t *n_valid, int64_t *n_skipped);

/* ------------------------------------------------------------------------------------------------
 * Ouster lidar packets decoded on the device (what ouster-sdk's PacketFormat / ScanBatcher / LidarScan do for the
 * reference's feed, data.py:31-77 - third party, restated from the published packet layouts).  The host decides which packets form a
 * sweep (2 bytes read per packet, `sweep_of_packet`); the device turns the column-major payloads into the staggered range image
 * u32[H][W] in mm (column = measurement_id), the column timestamps u64[W] in ns, the column status words u16[W] (LEGACY: the low half
 * of its 32-bit status) and one summary record per sweep.  A column counts only with status bit 0 set and measurement_id < W; what no
 * counted column supplies is 0; of two counted columns of a sweep with one measurement_id the later in arrival order wins (the owner is
 * resolved before anything is written); otherwise the result does not depend on the order of the packets.
 * ---------------------------------------------------------------------------------------------- */
#define PTL_PKT_LEGACY 0                        /* 16-B column header, 12-B pixels (range: 20 bits), 32-bit status behind the pixels */
#define PTL_PKT_RNG19_RFL8_SIG16_NIR16 1        /* 32-B packet header and footer, 12-B column header, 12-B pixels (range: 19 bits) */
#define PTL_PKT_RNG15_RFL8_NIR8 2               /* ... 4-B pixels, range: 15 bits in units of 8 mm */
#define PTL_PKT_RNG19_RFL8_SIG16_NIR16_DUAL 3   /* ... 16-B pixels, the FIRST return's range: 19 bits */
typedef struct {
    uint32_t struct_size;  /* sizeof(ptl_pkt_format) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    int32_t profile;             /* PTL_PKT_* */
    int32_t pixels_per_column;   /* H */
    int32_t columns_per_frame;   /* W */
    int32_t columns_per_packet;  /* C, <= 64 */
} ptl_pkt_format;
typedef struct {
    uint32_t frame_id;         /* of the sweep's first packet in arrival order (0: the sweep got no packet) */
    uint32_t valid_columns;    /* image columns supplied by a counted packet column */
    uint32_t first_valid_id;   /* lowest / highest measurement_id among them (0 when there is none) ... */
    uint32_t last_valid_id;
    uint64_t first_valid_ts;   /* ... and their timestamps, ns; last_valid_ts is ouster client.last_valid_column_ts */
    uint64_t last_valid_ts;
    uint32_t nonzero_ranges;   /* pixels of the image with a return */
    uint32_t ignored_columns;  /* packet columns with status bit 0 set and measurement_id >= W */
} ptl_pkt_summary;
/* bytes of one lidar packet of that format (24896 / 24832 / 8448 / 33024 for H = 128, C = 16), < 0 on a refused format (struct_size /
 * abi_version mismatch, unknown profile, H, W or C < 1, C > 64, a packet above 60 KB) */
int64_t ptl_pkt_packet_bytes(const ptl_pkt_format *fmt);
typedef struct ptl_pktdec ptl_pktdec;
/* a decoder for up to max_packets packets and max_sweeps sweeps per call: owns its stream and its device staging */
int ptl_pktdec_create(const ptl_pkt_format *fmt, int32_t device_id, int64_t max_packets, int32_t max_sweeps, ptl_pktdec **out);
int ptl_pktdec_destroy(ptl_pktdec *d);
/* packets: n packets in HOST memory (pageable, or page-locked with ptl_host_pin), packet i at packets + i * stride_bytes; the buffer and the
 * stride are 4-byte aligned, stride_bytes >= the packet size.  sweep_of_packet[i] in [0, n_sweeps) or < 0 = not part of any sweep.
 * Outputs (host, any may be NULL): range_out n_sweeps x H x W, col_ts_out n_sweeps x W, col_status_out n_sweeps x W, summary_out
 * n_sweeps.  Arguments are checked before any HIP call. */
int ptl_pktdec_decode(ptl_pktdec *d, const void *packets, int64_t stride_bytes, int64_t n, const int32_t *sweep_of_packet, int32_t n_sweeps,
                      uint32_t *range_out, uint64_t *col_ts_out, uint16_t *col_status_out, ptl_pkt_summary *summary_out);
/* The channel fields of a pixel beside its range.  A field is `bytes` (1, 2 or 4) at byte `offset` from the start of the pixel,
 * offset % bytes == 0 and offset + bytes <= the profile's pixel size (12 / 12 / 4 / 16 bytes); its value is (little-endian word & mask) << shift
 * for shift >= 0 and >> -shift otherwise (|shift| <= 31), as u32; mask == 0 means all bits.  The descriptor is DATA: ptl_pkt_field_default fills
 * it from this table (restated from Ouster's published pixel layouts and UNPINNED - no copy of them was at hand; a wrong row is a one-line fix
 * there, or a descriptor of the caller's own, not a kernel change):
 *   profile                       RANGE                 REFLECTIVITY  SIGNAL    NEAR_IR        second return
 *   LEGACY                        u32 @0 & 0x000fffff   u16 @4        u16 @6    u16 @8         none
 *   RNG19_RFL8_SIG16_NIR16        u32 @0 & 0x0007ffff   u8 @4         u16 @6    u16 @8         none
 *   RNG15_RFL8_NIR8               u16 @0 & 0x7fff << 3  u8 @2         none      u8 @3 << 4     none
 *   RNG19_RFL8_SIG16_NIR16_DUAL   u32 @0 & 0x0007ffff   u8 @3         u16 @8    u16 @12        RANGE2 u32 @4 & 0x0007ffff, REFLECTIVITY2 u8 @7, SIGNAL2 u16 @10
 * A field image is u32[H][W], staggered like the range image: image column `id` is written by the packet column that supplies the range image's
 * (the last counted one in arrival order) and by nobody else; a column that no counted packet column supplies is 0; a field is written whether
 * or not the pixel's range is 0.  RANGE through this path equals range_out bit for bit. */
#define PTL_PKT_FIELD_RANGE 0
#define PTL_PKT_FIELD_REFLECTIVITY 1
#define PTL_PKT_FIELD_SIGNAL 2
#define PTL_PKT_FIELD_NEAR_IR 3
#define PTL_PKT_FIELD_RANGE2 4
#define PTL_PKT_FIELD_REFLECTIVITY2 5
#define PTL_PKT_FIELD_SIGNAL2 6
#define PTL_PKT_MAX_FIELDS 4 /* fields per ptl_pktdec_decode_fields call */
typedef struct {
    uint32_t struct_size;  /* sizeof(ptl_pkt_field) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    int32_t offset;        /* bytes from the start of the pixel */
    int32_t bytes;         /* 1, 2 or 4 */
    uint32_t mask;         /* 0: all bits */
    int32_t shift;         /* > 0 left, < 0 right */
} ptl_pkt_field;
/* the library's sizeof(ptl_pkt_field) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_pkt_sizeof_field(void);
/* the table's descriptor of PTL_PKT_FIELD_* in fmt's profile; out->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a
 * mismatch is refused with PTL_ERR_ARG and nothing is written.  PTL_ERR_ARG naming profile and field where the profile has no such field. */
int ptl_pkt_field_default(const ptl_pkt_format *fmt, int32_t field_id, ptl_pkt_field *out);
/* ptl_pktdec_decode and, from the same staged packets (they cross the bus once; the three passes run as they are, ONE added launch reads the
 * staged packets again), n_fields (1 .. PTL_PKT_MAX_FIELDS) field images: field_out[f] (host, n_sweeps x H x W u32, none NULL) gets fields[f].
 * The other outputs as ptl_pktdec_decode's (any may be NULL).  Checked before any HIP call and refused with the numbers (PTL_ERR_ARG): n_fields
 * outside 1 .. 4, a descriptor of another size or version, bytes not 1, 2 or 4, a negative or misaligned offset, offset + bytes past the
 * pixel, |shift| > 31 - and everything ptl_pktdec_decode checks.  The field staging is the decoder's, made by the first call that needs it. */
int ptl_pktdec_decode_fields(ptl_pktdec *d, const void *packets, int64_t stride_bytes, int64_t n, const int32_t *sweep_of_packet, int32_t n_sweeps,
                             const ptl_pkt_field *fields, int32_t n_fields, uint32_t *const *field_out, uint32_t *range_out,
                             uint64_t *col_ts_out, uint16_t *col_status_out, ptl_pkt_summary *summary_out);
/* profiling: HIP-event time of the device work of the decoder's calls (the initialisation and the three passes, not the copies) since the last
 * reset, and the number of calls timed; like ptl_icp_profile */
int ptl_pktdec_profile(ptl_pktdec *d, int enable, double *ms_total, int64_t *calls, int reset);
/* Sweep k of a runner that takes range images, decoded from its n packets (tightly packed: stride = the packet size) straight into the
 * sweep's slot: afterwards the slot holds byte for byte what ptl_*_upload_range of the decoded image leaves, and the host never built the
 * image.  Preconditions and sweep-ring order errors of ptl_*_upload_range; the decoder's H W must be the runner's points_per_scan and both
 * live on one device (else PTL_ERR_ARG).  summary (1 record) and col_ts (W) are nullable. */
int ptl_seq_upload_packets(ptl_seq *s, ptl_pktdec *dec, int64_t k, const void *packets, int64_t n, ptl_pkt_summary *summary, uint64_t *col_ts);
int ptl_batch_upload_packets(ptl_batch *b, int32_t seq, ptl_pktdec *dec, int64_t k, const void *packets, int64_t n, ptl_pkt_summary *summary,
                             uint64_t *col_ts);

/* ------------------------------------------------------------------------------------------------
 * Sharpness of a voxel map without ground truth (no reference counterpart).  The score is of the map AS STORED: a voxel
 * keeps its first max_points_per_voxel points, and only those are scored and counted as neighbours.
 * Per stored point q:
 *   membership  a stored point p (q included) is a neighbour iff (dx dx + dy dy) + dz dz <= radius radius, d = p - q, evaluated in that order
 *               without contraction: an integer fact, the same everywhere;
 *   covariance  n = number of neighbours, m = mean of the offsets d, Sigma = (1/n) sum d d^T - m m^T in fp64 (offsets from q: every term is
 *               at most radius^2 in magnitude);
 *   eigenvalues lambda0 <= lambda1 <= lambda2 of Sigma by cyclic Jacobi with a fixed number of sweeps (no closed trigonometric form: it loses
 *               its digits at the planar neighbourhoods that matter here), each clipped below at 0;
 *   outputs     plane_var = lambda0 (a crisp wall: about the sensor noise; a doubled wall: about (half the gap)^2);
 *               entropy = 0.5 (3 ln(2 pi e) + sum_i ln(lambda_i + sigma_floor^2)), the differential entropy of the neighbourhood Gaussian -
 *               the floor keeps a perfectly planar neighbourhood finite;
 *   sparse      n < min_neighbours: counted, not scored; its per-point outputs are n and two NaNs.
 * Parameters: 0 < radius <= the map's voxel size (with the truncating voxel index every point within radius of a point of voxel k lies in
 * voxels k - 1 .. k + 1 on each axis: the 27-voxel search is then complete; otherwise PTL_ERR_ARG with both numbers), min_neighbours >= 1 (it
 * counts the point itself), sigma_floor > 0.  The defaults (radius = voxel size, 5, voxel size / 100) are defaults a caller may change and the
 * result echoes - not tuned values.
 * Counts are exact.  The means are reduced on the device by a fixed tree over the per-point values in pool order: two builds of the same map
 * may hand out block ids differently, so their means are equal only up to summation order (their per-point values are equal bit for bit). */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_map_score_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double radius;
    int32_t min_neighbours;
    double sigma_floor;
} ptl_map_score_cfg;
typedef struct {
    int64_t n_points, n_scored, n_sparse;   /* stored points = scored + sparse */
    double mean_plane_var, mean_entropy;    /* over the scored points; 0 when there is none */
    double mean_neighbours;                 /* mean n over ALL stored points (0 for an empty map) */
    double radius;                          /* the parameters as used */
    int32_t min_neighbours;
    double sigma_floor;
    double device_ms;                       /* HIP-event time of the call's device work on the handle's own stream (0 for an empty map): the one
                                             * field that is not a function of the map - only the library can bracket that stream, cf. ptl_icp_profile */
} ptl_map_score_result;
/* the defaults for a map of that voxel size; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is
 * refused with PTL_ERR_ARG and nothing is written */
int ptl_map_score_default_cfg(ptl_map_score_cfg *cfg, double voxel_size);
/* Scores the map of `map` (cfg nullable: the defaults).  Waits for the handle's map update first, never writes to the map, keeps nothing in the
 * handle: its work buffers live for the call.  xyz_out (3 per point), n_out, plane_var_out, entropy_out: all four or none; when given they
 * receive every stored point with its values in one common order (pool order, unspecified) and *n_written (nullable) their number;
 * max_points below the map's point count: PTL_ERR_CAPACITY naming the count, nothing written.  A handle whose max_points_per_voxel needs more
 * than 64 KB of staging (27 P 24 bytes: P > 98): PTL_ERR_CAPACITY - a guard that no handle reaches today, since ptl_icp_create refuses more
 * than 32 points per voxel.  PTL_ERR_STATE when the map table does not lead every voxel back to its block (nothing is scored then).  Arguments are checked before any HIP call; an empty map gives the all-zero
 * summary (with the parameters). */
int ptl_icp_map_score(ptl_icp *map, const ptl_map_score_cfg *cfg, ptl_map_score_result *out, double *xyz_out, int32_t *n_out,
                      double *plane_var_out, double *entropy_out, int64_t max_points, int64_t *n_written);

/* ------------------------------------------------------------------------------------------------
 * Frames of the fly-by drawn on the device (the picture the reference's viewer shows, src/ptudes/fly.py and cli/flyby.py
 * through ouster-sdk's PointViz - third party; the drawing here is this library's own).  Every stored point of a map, and optionally an
 * overlay cloud the renderer owns, is projected through a pinhole camera and depth-tested into a frame; the map stays in HBM.
 * Frame buffer: per pixel a 64-bit key = (bits of float32(view depth) << 32) | rgba, an empty pixel is all ones, a pixel's final key is the
 * minimum over the splats that cover it - a function of the SET of points, not of their order.  Two points at the same float32 depth in a
 * pixel resolve to the smaller rgba word.  rgba words are the bytes R, G, B, A in memory order (R the lowest byte of the word).
 * Per point p (world) and camera: (xc, yc, zc) = view p with view a row-major 3 x 4 (world -> camera, +z forward, +x right, +y down),
 * each row evaluated as ((v0 x + v1 y) + v2 z) + v3; rejected when !(zc > near_m) or zc >= far_m, before any division;
 * u = fx (xc / zc) + cx, v = fy (yc / zc) + cy; pixel (floor(u), floor(v)); the footprint is point_px x point_px pixels (1 .. 5) whose top-left is
 * (floor(u) - (point_px - 1) / 2, floor(v) - (point_px - 1) / 2) (integer division), clipped pixel by pixel to the image.  A map point's colour is
 * palette[clamp(floor((z - z_lo) * (256 / (z_hi - z_lo))), 0, 255)], z its world height; an overlay point's colour is taken as given.
 * With edl_strength > 0 the resolved colour is shaded by eye-dome lighting from the depths d of the four neighbours at edl_radius_px (left, right,
 * up, down; those inside the image and not empty): s = exp(-edl_strength max(0, mean(log2 d - log2 d_nb))), channel c -> floor(c s + 0.5), alpha kept.
 * All arithmetic is fp64 without contraction; csrc/render_kernels.h spells out the order. */
typedef struct ptl_render ptl_render;
#define PTL_RENDER_MAX_KEY_BYTES (1ll << 30) /* bound of width * height * max_frames_per_call * 8, the key buffer of one launch */
typedef struct {
    uint32_t struct_size;        /* sizeof(ptl_render_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    int32_t width, height;       /* pixels, 1 .. 16384 each */
    int32_t point_px;            /* footprint of a map point, 1 .. 5 (default 2) */
    int32_t max_frames_per_call; /* frames per launch (default 16) */
    double z_lo, z_hi;           /* world heights of palette entries 0 and 255 (default -2, 10); z_hi > z_lo */
    uint32_t background_rgba;    /* default 0xFF000000: opaque black */
    double edl_strength;         /* 0 (default) = off */
    int32_t edl_radius_px;       /* >= 1 (default 1) */
} ptl_render_cfg;
/* a plain array element, not a versioned struct */
typedef struct {
    double view[12];
    double fx, fy, cx, cy, near_m, far_m;
} ptl_render_cam;
/* the library's sizeof(ptl_render_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_render_sizeof_cfg(void);
/* the defaults above for a width x height frame; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is
 * refused with PTL_ERR_ARG and nothing is written */
int ptl_render_default_cfg(ptl_render_cfg *cfg, int32_t width, int32_t height);
/* refused with the offending numbers, before any HIP call: width / height outside 1 .. 16384, point_px outside 1 .. 5, max_frames_per_call < 1,
 * z_hi <= z_lo, edl_strength < 0 or not finite, edl_radius_px < 1, a key buffer above PTL_RENDER_MAX_KEY_BYTES.  The renderer owns a stream,
 * the key buffer and the output staging of one launch, the palette and the overlay. */
int ptl_render_create(const ptl_render_cfg *cfg, int32_t device_id, ptl_render **out);
int ptl_render_destroy(ptl_render *r);
/* 256 rgba words.  The default: entry i = {R = i, G = 255 - |2 i - 255|, B = 255 - i, A = 255} - blue at z_lo over green to red at z_hi */
int ptl_render_set_palette(ptl_render *r, const uint32_t rgba[256]);
/* the world heights of palette entries 0 and 255 for the frames that follow (cfg.z_lo, cfg.z_hi); z_hi <= z_lo: PTL_ERR_ARG with both numbers */
int ptl_render_set_z_range(ptl_render *r, double z_lo, double z_hi);
/* the overlay cloud (e.g. the trajectory's positions): n points xyz (n x 3 f64, world) with their colours, drawn point_px wide (1 .. 5) into
 * every frame after the map under the same depth test; n = 0 clears it (xyz / rgba may then be NULL) */
int ptl_render_set_overlay(ptl_render *r, const double *xyz, const uint32_t *rgba, int64_t n, int32_t point_px);
/* A colour of its own for every stored point of ONE map handle: n little-endian rgba words in pool order (block id, then slot:
 * the order of ptl_paint_read's, ptl_carve_read's and ptl_icp_map_score's per-point outputs).  n must equal the map's stored point count, else
 * PTL_ERR_ARG with both numbers; rgba == NULL or n == 0 clears the colours (map may then be NULL).  The renderer keeps the words, its own
 * per-block prefix of that map and the count; the map handle must outlive them or they must be cleared first.  Frames of THAT handle with an
 * unchanged point count then take a point's colour from its word instead of the height palette - projection, footprint, depth key, the
 * minimum, the overlay and eye-dome lighting are unchanged; the same handle with a changed count gives PTL_ERR_STATE from ptl_render_frames;
 * any other handle draws palette frames as before. */
int ptl_render_set_point_colors(ptl_render *r, ptl_icp *map, const uint32_t *rgba, int64_t n);
/* n_frames frames of `map` (nullable: the overlay only) through cams[n_frames], in launches of max_frames_per_call frames.  Like
 * ptl_icp_map_score it waits for the handle's map update, only reads the map and keeps nothing in the map handle.  Outputs (host): rgba_out
 * n_frames x height x width words; depth_out (nullable) as many float32, +inf = empty; keys_out (nullable) as many raw 64-bit keys;
 * in_view_out (nullable) n_frames counts of the points (map and overlay) that passed the depth test with at least one pixel of their footprint
 * in the image; device_ms (nullable) the HIP-event time of the launches' device work.  Checked before any HIP call, refused with the numbers:
 * n_frames < 0, a camera with near_m <= 0 or far_m <= near_m or a non-finite entry, renderer and map on different devices.  An empty map
 * gives background frames and zero counts. */
int ptl_render_frames(ptl_render *r, ptl_icp *map, const ptl_render_cam *cams, int64_t n_frames, uint32_t *rgba_out, float *depth_out,
                      uint64_t *keys_out, int64_t *in_view_out, double *device_ms);
/* measurement hook (tools/render_cost.py): on == 0 drops the plain load in front of the 64-bit atomicMin - the same frames, every covered
 * pixel then costs an atomic */
int ptl_render_debug_set_early_reject(ptl_render *r, int32_t on);

/* ------------------------------------------------------------------------------------------------
 * Distance of query points to the stored points of a map (no reference counterpart): the cloud-to-cloud nearest-neighbour
 * distance with the voxel map as the search structure.  Distances are to the map AS STORED: a voxel keeps its first max_points_per_voxel points.
 * Per query q: d2(q) = min over all stored points p of `ref` of (dx dx + dy dy) + dz dz, d = p - q, fp64 in that order without contraction;
 * q is matched iff d2 <= max_dist max_dist (the product made once, as a double); its per-point output is d2 when matched and +inf when not.
 * A query with a non-finite coordinate is counted in n_invalid and gets NaN; a query whose voxel index lies outside the key range is unmatched.
 * n_within[k] counts the queries with d2 <= thresholds[k] thresholds[k].  A minimum does not depend on the order of its terms: d2, the match and
 * every count are exact functions of the set of stored points and the query.  sum_dist (of sqrt(d2)), sum_dist2 (of d2) and max_dist2_seen run
 * over the matched queries; the sums are reduced on the device by a fixed tree in query order (array queries: per staged chunk, the chunk
 * sums added on the host in chunk order), so they depend on the order of the queries only up to summation order.
 * Parameters: 0 < max_dist <= ref's voxel size (the 27-voxel search is complete then, cf. the map score's radius), 1 .. 8 thresholds, ascending
 * (equal neighbours allowed), each in (0, max_dist].  The defaults (max_dist = voxel size, one threshold = max_dist) are a caller's choice echoed
 * back, not tuned values. */
#define PTL_MAP_CMP_MAX_THRESHOLDS 8
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_map_cmp_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double max_dist;
    int32_t n_thresholds;
    double thresholds[PTL_MAP_CMP_MAX_THRESHOLDS];
} ptl_map_cmp_cfg;
typedef struct {
    int64_t n_query, n_invalid, n_matched;          /* unmatched = n_query - n_invalid - n_matched */
    int64_t n_within[PTL_MAP_CMP_MAX_THRESHOLDS];   /* entries from n_thresholds on are 0 */
    double sum_dist, sum_dist2, max_dist2_seen;     /* over the matched queries; 0 when there is none */
    double max_dist;                                /* the parameters as used */
    int32_t n_thresholds;
    double thresholds[PTL_MAP_CMP_MAX_THRESHOLDS];
    double device_ms;                               /* HIP-event time of the call's device work on ref's stream (0 without queries), cf. ptl_map_score_result */
} ptl_map_cmp_result;
/* the library's sizeof(ptl_map_cmp_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_map_cmp_sizeof_cfg(void);
/* the defaults for a reference map of that voxel size; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch
 * is refused with PTL_ERR_ARG and nothing is written */
int ptl_map_cmp_default_cfg(ptl_map_cmp_cfg *cfg, double voxel_size);
/* n queries xyz (n x 3 f64, host) against the map of `ref` (cfg nullable: the defaults).  The queries are staged and processed in chunks of a
 * fixed size inside the call: no device buffer grows with n.  dist2_out (nullable): n doubles, the per-point outputs in query order.  Waits
 * for the handle's map update first, only reads the map and keeps nothing in the handle.  Checked before any HIP call, refused with the numbers
 * (PTL_ERR_ARG): null ref / result, xyz null with n > 0, n < 0, max_dist <= 0, not finite or above ref's voxel size, n_thresholds outside 1 .. 8,
 * a threshold <= 0, above max_dist or below its predecessor.  PTL_ERR_STATE when the table leads to a block that does not hold the probed
 * voxel.  An empty reference leaves every finite query unmatched; n = 0 gives the zero summary (with the parameters). */
int ptl_icp_map_distance(ptl_icp *ref, const ptl_map_cmp_cfg *cfg, const double *xyz, int64_t n, ptl_map_cmp_result *result, double *dist2_out);
/* The same with the stored points of `src` as the queries, walked on the device in pool order (block id, then slot): nothing but the summary
 * crosses the bus.  xyz_out (3 per point) and dist2_out: both or neither; when given they receive every stored point of src with its output in
 * that order and *n_written (nullable) their number; max_points below src's point count: PTL_ERR_CAPACITY naming the count, nothing written.
 * ref and src must live on one device (else PTL_ERR_ARG with both ids); src == ref is allowed (every d2 is then 0).  Waits for both handles'
 * map updates, only reads both maps. */
int ptl_icp_map_compare(ptl_icp *ref, ptl_icp *src, const ptl_map_cmp_cfg *cfg, ptl_map_cmp_result *result, double *xyz_out, double *dist2_out,
                        int64_t max_points, int64_t *n_written);

/* ------------------------------------------------------------------------------------------------
 * Free space carved: the moving-object points of a world map (no reference counterpart).  A second pass over the sweeps that
 * built a map, posed by the same trajectory: for every STORED map point it counts the rays that went through the point and the rays that ended
 * at it.  All outputs are integers; sums of integers have no order, so every count is an exact function of the map's stored points and the set
 * of rays - the lane mapping, the launch geometry and the order of the sweeps do not change it.  All arithmetic fp64 in the written order,
 * without contraction.
 * Parameters: radius > 0; margin >= 0; 0 < step <= the map's voxel size vs; min_range >= 0; max_range > min_range, max_range / step <= 65536.
 * The defaults (radius = vs / 10, margin = vs, step = vs / 2, min_range = 0, max_range = 120 vs) are a caller's choice that the result echoes
 * back, not tuned values.
 * Ray: a pixel with a return.  Its end w is the world point the posed-scan pass gives it (ptl_icp_map_add_posed_*), its origin o the
 * translation of its own column's pose; d = w - o, len2 = (dx dx + dy dy) + dz dz, len = sqrt(len2).  The ray is used iff
 * min_range <= len <= max_range, otherwise it is counted in n_rays_out_of_range; a pixel without a return is counted in n_no_return.  A sweep
 * with any column outside the trajectory's bounds is skipped as a whole and counted (n_scans_skipped), as ptl_icp_map_add_posed_* skips it.
 * March: the samples are k = 0, 1, ... while t_k = ((double)k + 0.5) step < len: a_k = t_k / len, s_k[c] = o[c] + a_k d[c]; the last sample is
 * w itself, not o + 1 d.  A sample's voxel is the map's own truncating index (int)(coordinate / vs) per axis; a sample outside the key range
 * (2^20 voxels either side) is passed over; consecutive samples with one key visit the voxel once.  Every coordinate of s_k is monotone in k and
 * so is the index: a ray cannot return to a voxel it has left.
 * Vote: for every point p stored in a visited voxel, e = p - o: c = e x d with six separately rounded products (cx = ey dz - ez dy, ...); p is
 * near the ray iff (cx cx + cy cy) + cz cz <= (radius radius) len2 (the left factor made once per call, the product once per ray);
 * t_p = ((ex dx + ey dy) + ez dz) / len.  A near point with t_p < min_range gets nothing; with t_p <= len - margin through += 1; otherwise with
 * t_p <= len + margin support += 1; beyond that nothing.
 * ONLY the visited voxels are looked at: a point within `radius` of a ray whose centre line misses the point's voxel is NOT counted.  This is
 * part of the definition; the rays of a sweep are dense against `radius`.  Which points count as moving is the caller's policy on the two
 * counts (the Python layer's CarveVotes.dynamic), not the library's. */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_carve_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double radius, margin, step, min_range, max_range;
} ptl_carve_cfg;
typedef struct {
    int64_t n_points;                                  /* stored points of the map (the length of the per-point arrays) */
    int64_t n_scans, n_scans_skipped;                  /* sweeps carved / skipped as outside the trajectory's bounds */
    int64_t n_rays, n_rays_out_of_range, n_no_return;  /* pixels of the carved sweeps: used rays, returns outside [min_range, max_range], no return */
    int64_t n_voxel_visits;                            /* visited voxels that the map holds, over all rays */
    int64_t n_points_through, n_points_supported;      /* points with a non-zero count */
    int64_t sum_through, sum_support;
    double radius, margin, step, min_range, max_range; /* the parameters as used */
    double device_ms;                                  /* HIP-event time of the handle's device work so far: prefixes, sweeps, the read's reduction */
} ptl_carve_result;
typedef struct ptl_carve ptl_carve; /* the votes for one map: its own stream, column table, sweep staging and vote arrays */
/* the library's sizeof(ptl_carve_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_carve_sizeof_cfg(void);
/* the defaults for a map of that voxel size; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is
 * refused with PTL_ERR_ARG and nothing is written */
int ptl_carve_default_cfg(ptl_carve_cfg *cfg, double voxel_size);
/* cfg nullable: the defaults of the map's voxel size.  Waits for the map's update, snapshots its point count and the per-block prefixes of the
 * pool order (block id, then slot: the order of ptl_icp_map_score's and ptl_icp_map_compare's per-point outputs) and clears the votes.  The map
 * handle must outlive the carve handle and is only ever read.  Checked before any HIP call, refused with the numbers (PTL_ERR_ARG): null map /
 * out, a cfg of another size or version, each parameter bound above. */
int ptl_carve_create(ptl_icp *map, const ptl_carve_cfg *cfg, ptl_carve **out);
int ptl_carve_destroy(ptl_carve *c);
/* one posed sweep, with the arguments of ptl_icp_map_add_posed_range / _xyz: *n_valid = the sweep's used rays (nullable), *skipped = 1 when a
 * column lay outside the bounds and nothing was counted but the sweep (nullable).  Trajectory, LUT and map on one device (else PTL_ERR_ARG with
 * the ids); W = the map handle's scan_cols and H W <= its max_points_per_scan (else PTL_ERR_CAPACITY with the numbers) - all before any HIP call.
 * Every add and read compares the map's point count with the snapshot: a map updated since ptl_carve_create gives PTL_ERR_STATE.
 * PTL_ERR_STATE as well when the map's table leads a probe to a block that does not hold the probed voxel. */
int ptl_carve_add_posed_range(ptl_carve *c, ptl_traj *t, ptl_lut *lut, const uint32_t *range_mm, const double *col_ts, int64_t *n_valid,
                              int32_t *skipped);
int ptl_carve_add_posed_xyz(ptl_carve *c, ptl_traj *t, const float *xyz, int32_t H, int32_t W, const double *col_ts, int64_t *n_valid,
                            int32_t *skipped);
/* the RESIDENT sweeps [first, last] of a runner, no sweep crosses the bus; arguments, column times and state errors as ptl_seq_map_build /
 * ptl_batch_map_build.  *n_valid = used rays, *n_skipped = sweeps skipped (both nullable) */
int ptl_carve_add_seq(ptl_carve *c, ptl_seq *s, ptl_traj *t, const double *t0t1, int64_t first, int64_t last, int64_t *n_valid,
                      int64_t *n_skipped);
int ptl_carve_add_batch(ptl_carve *c, ptl_batch *b, int32_t seq, ptl_traj *t, const double *t0t1, int64_t first, int64_t last,
                        int64_t *n_valid, int64_t *n_skipped);
/* the summary so far, and (all three arrays given, or none) every stored point (3 doubles) with its two counts in pool order; *n_written
 * (nullable) their number.  max_points below the map's point count: PTL_ERR_CAPACITY naming the count, nothing written.  The votes stay: sweeps
 * may be added and read again. */
int ptl_carve_read(ptl_carve *c, ptl_carve_result *result, double *xyz_out, uint32_t *through_out, uint32_t *support_out, int64_t max_points,
                   int64_t *n_written);

/* ------------------------------------------------------------------------------------------------
 * A sweep's fit to a map at each of K candidate poses (no reference counterpart): the search half of finding the sensor in a
 * saved map - ptl_icp_align is the refinement half.  K poses x n points are evaluated resident; K x n_thresholds integers come back.
 * Per candidate k (row-major 4 x 4 fp64; the top three rows are used as given, nothing is re-orthonormalised) and query point q_i (sensor frame):
 * wx = ((r00 qx + r01 qy) + r02 qz) + tx, wy and wz likewise, fp64 in that order without contraction; d2(w) is ptl_icp_map_distance's - the
 * minimum over all stored points of (dx dx + dy dy) + dz dz with the same neighbourhood and key-range rule; hits[k][j] = the number of i with
 * d2 <= thresholds[j] thresholds[j] (the products made once, as doubles).  A query point with a non-finite coordinate is never a hit and is
 * counted once in n_invalid_points; a candidate with a non-finite entry in its top three rows takes no probe, gets hits = -1 at every threshold
 * and is counted in n_invalid_poses; a transformed point that is not finite or lies outside the key range is not a hit.  Counts of integers have
 * no order: every output is an exact function of the set of stored points, the query set and the pose.
 * best_hits[j] / best_pose[j]: the largest hits[.][j] over the valid candidates and the SMALLEST candidate index that attains it; without a valid
 * candidate (n_poses = 0 included) best_pose[j] = -1 and best_hits[j] = 0, as for j >= n_thresholds.
 * Parameters: 0 < max_dist <= the map's voxel size, 1 .. 4 thresholds, ascending (equal neighbours allowed), each in (0, max_dist].  The defaults
 * (max_dist = voxel size, one threshold = max_dist) are a caller's choice echoed back, not tuned values. */
#define PTL_POSE_SEARCH_MAX_THRESHOLDS 4
#define PTL_POSE_SEARCH_MAX_POINTS (1 << 20)
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_pose_search_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double max_dist;
    int32_t n_thresholds;
    double thresholds[PTL_POSE_SEARCH_MAX_THRESHOLDS];
} ptl_pose_search_cfg;
typedef struct {
    int64_t n_points, n_invalid_points;                   /* query points, and those with a non-finite coordinate */
    int64_t n_poses, n_invalid_poses;                     /* candidates, and those with a non-finite entry in the top three rows */
    int64_t best_pose[PTL_POSE_SEARCH_MAX_THRESHOLDS];    /* per threshold: the smallest index with the most hits, -1 = no valid candidate */
    int64_t best_hits[PTL_POSE_SEARCH_MAX_THRESHOLDS];
    double max_dist;                                      /* the parameters as used */
    int32_t n_thresholds;
    double thresholds[PTL_POSE_SEARCH_MAX_THRESHOLDS];
    double device_ms;                                     /* HIP-event time of the call's device work on the map's stream, staging copies included */
} ptl_pose_search_result;
/* the library's sizeof(ptl_pose_search_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_pose_search_sizeof_cfg(void);
/* the defaults for a map of that voxel size; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is
 * refused with PTL_ERR_ARG and nothing is written */
int ptl_pose_search_default_cfg(ptl_pose_search_cfg *cfg, double voxel_size);
/* n query points xyz (n x 3 f64, host, sensor frame) at n_poses candidates poses16 (n_poses x 16 f64, host) against the map of `map` (cfg
 * nullable: the defaults).  hits_out (nullable): n_poses x n_thresholds counts, candidate-major.  The query points are resident for the call;
 * the candidates are staged and processed in chunks of a fixed size (ptl_build_info [15]): no device buffer grows with n_poses.  Waits for the
 * handle's map update first, only reads the map and keeps nothing in the handle.  Checked before any HIP call, refused with the numbers
 * (PTL_ERR_ARG): null map / result, xyz null with n > 0, n < 0, poses16 null with n_poses > 0, n_poses < 0, max_dist <= 0, not finite or above the
 * map's voxel size, n_thresholds outside 1 .. 4, a threshold <= 0, above max_dist or below its predecessor; n > 2^20: PTL_ERR_CAPACITY.
 * PTL_ERR_STATE when the table leads to a block that does not hold the probed voxel.  An empty map gives zeros for every valid candidate;
 * n = 0 as well. */
int ptl_icp_pose_hits(ptl_icp *map, const ptl_pose_search_cfg *cfg, const double *xyz, int64_t n, const double *poses16, int64_t n_poses,
                      ptl_pose_search_result *result, int32_t *hits_out);

/* ------------------------------------------------------------------------------------------------
 * The world map painted: a lidar channel field per STORED map point.  A second pass over the sweeps that built a map, posed by
 * the same trajectory, each with a field image u32[H][W] of the same pixels (reflectivity, signal, near-infrared, the range itself): every
 * stored point gets the sum of the field values of the rays that ended AT it and their number.  All outputs are integers; sums of integers have
 * no order, so every output is an exact function of the stored points and the set of (ray, value) pairs - the lane mapping, the launch
 * geometry and the order of the sweeps do not change it.
 * Ray: a pixel with a return.  Its end w is the world point the posed-scan pass gives it (ptl_icp_map_add_posed_*; the same device functions,
 * so the same bits).  A pixel without a return is counted in n_no_return and adds nothing, whatever its field value.  A sweep with any column
 * outside the trajectory's bounds is skipped as a whole and counted (n_scans_skipped), as ptl_icp_map_add_posed_* skips it.
 * Per ray: its voxel is the map's own truncating index (int)(coordinate / vs) per axis; a w outside the key range (2^20 voxels either side, or
 * not finite) makes the ray unmatched.  The voxel is looked up; for every stored point p of that voxel with p.x == w.x && p.y == w.y &&
 * p.z == w.z (comparison of doubles): sum[p] += field[pixel] (u64), count[p] += 1 (u32).  A ray that matched at least one point counts in
 * n_rays_matched; any other ray - into a full voxel, into an absent voxel, out of the key range - in n_rays_unmatched.
 * Consequence: a map built from sweeps S on trajectory T and painted with S on T has count >= 1 at EVERY stored point (a voxel's first
 * max_points_per_voxel points are among those rays), and n_rays_unmatched is exactly the number of returns the build did not store.
 * The mean of a point is the caller's sum / count (the Python layer's PaintValues.mean), as is any colour made of it. */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_paint_result) as the caller knows it (PTL_CFG_INIT): ptl_paint_read refuses another size or version */
    uint32_t abi_version;
    int64_t n_points;                                      /* stored points of the map (the length of the per-point arrays) */
    int64_t n_points_painted;                              /* points with count > 0 */
    int64_t n_scans, n_scans_skipped;                      /* sweeps painted / skipped as outside the trajectory's bounds */
    int64_t n_rays_matched, n_rays_unmatched, n_no_return; /* pixels of the painted sweeps */
    int64_t sum_count;                                     /* the sum of count over the stored points */
    double device_ms;                                      /* HIP-event time of the handle's device work so far: prefixes, sweeps, the read's reduction */
} ptl_paint_result;
typedef struct ptl_paint ptl_paint; /* the sums for one map: its own stream, column table, sweep and field staging, sum and count arrays */
/* the library's sizeof(ptl_paint_result) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_paint_sizeof_result(void);
/* Waits for the map's update, snapshots its point count and the per-block prefixes of the pool order (block id, then slot: the order of
 * ptl_carve_read's, ptl_icp_map_score's and ptl_icp_map_compare's per-point outputs) and clears sum and count.  The map handle must outlive
 * the paint handle and is only ever read.  Null map / out: PTL_ERR_ARG before any HIP call. */
int ptl_paint_create(ptl_icp *map, ptl_paint **out);
int ptl_paint_destroy(ptl_paint *p);
/* one posed sweep, with the arguments of ptl_icp_map_add_posed_range / _xyz, and its field image (H x W u32, row-major, the pixels of the
 * sweep): *n_matched = the sweep's matched rays (nullable), *skipped = 1 when a column lay outside the bounds and nothing was counted but the
 * sweep (nullable).  Trajectory, LUT and map on one device (else PTL_ERR_ARG with the ids); W = the map handle's scan_cols and H W <= its
 * max_points_per_scan (else PTL_ERR_CAPACITY with the numbers) - all before any HIP call.  Every add and read compares the map's point count with
 * the snapshot: a map updated since ptl_paint_create gives PTL_ERR_STATE.  PTL_ERR_STATE as well when the map's table leads a probe to a block
 * outside the pool or to one whose first point is not in the probed voxel. */
int ptl_paint_add_posed_range(ptl_paint *p, ptl_traj *t, ptl_lut *lut, const uint32_t *range_mm, const uint32_t *field, const double *col_ts,
                              int64_t *n_matched, int32_t *skipped);
int ptl_paint_add_posed_xyz(ptl_paint *p, ptl_traj *t, const float *xyz, const uint32_t *field, int32_t H, int32_t W, const double *col_ts,
                            int64_t *n_matched, int32_t *skipped);
/* the summary so far, and (all three arrays given, or none) every stored point (3 doubles) with its sum and count in pool order; *n_written
 * (nullable) their number.  result->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is refused with
 * PTL_ERR_ARG and nothing is written.  max_points below the map's point count: PTL_ERR_CAPACITY naming the count, nothing written.  The values
 * stay: sweeps may be added and read again. */
int ptl_paint_read(ptl_paint *p, ptl_paint_result *result, double *xyz_out, uint64_t *sum_out, uint32_t *count_out, int64_t max_points,
                   int64_t *n_written);

/* ------------------------------------------------------------------------------------------------
 * The occupancy grid of a run: free, occupied and unknown cells of a top-down 2-D grid (no reference counterpart).  A pass over
 * the sweeps of a run, posed by its trajectory: for every CELL it counts the rays that crossed the cell on their way (free) and the rays that
 * ended in it (hit).  No map handle is involved.  All outputs are integers; sums of integers have no order, so free and hit are an exact
 * function of the SET of rays and the parameters - the lane mapping, the launch geometry and the order of the sweeps do not change them.  All
 * arithmetic fp64 in the written order, without contraction.
 * Parameters: cell > 0; x0, y0 the world coordinates of the corner of cell (0, 0); nx, ny >= 1 with nx ny <= 2^26; z_lo <= z_hi, the height
 * band RELATIVE TO THE RAY'S OWN ORIGIN; margin >= 0; 0 < step <= cell; min_range >= 0; max_range > min_range, max_range / step <= 65536.
 * ptl_grid_default_cfg fills step = cell / 2, margin = cell, min_range = 0, max_range = 600 cell, band [-0.5, +0.5] m; the bounds (x0, y0, nx,
 * ny) and the staging sizes have no default.  The defaults are a caller's choice that the result echoes back, NOT tuned values: nobody has run
 * this on a real recording.
 * Ray: ptl_carve's ray.  A pixel with a return; its end w is the world point the posed-scan pass gives it (ptl_icp_map_add_posed_*), its origin
 * o the translation of its own column's pose; d = w - o, len2 = (dx dx + dy dy) + dz dz, len = sqrt(len2).  The ray is used iff
 * min_range <= len <= max_range, otherwise it is counted in n_rays_out_of_range; a pixel without a return is counted in n_no_return.  A sweep
 * with any column outside the trajectory's bounds is skipped as a whole and counted (n_scans_skipped).
 * Samples: k = 0, 1, ... while t_k = ((double)k + 0.5) step < len: a_k = t_k / len, s_k[c] = o[c] + a_k d[c].  A sample is a FREE sample iff
 * also t_k <= len - margin.
 * Cell of a point p: fx = (p.x - x0) / cell, fy = (p.y - y0) / cell; p is in the grid iff fx >= 0 && fx < (double)nx && fy >= 0 &&
 * fy < (double)ny, compared in fp64 before any integer conversion (a NaN fails it); then ix = (int)fx, iy = (int)fy.  p is in the band iff
 * z_lo <= p.z - o.z && p.z - o.z <= z_hi.
 * Runs: consecutive free samples with the same cell state - "outside the grid" or the pair (ix, iy) - form a run (run-based, like the carve's
 * "consecutive samples with one key visit the voxel once"; nothing rests on monotonicity).
 * Votes of one used ray: if w is in the grid and in the band, hit[cell(w)] += 1.  Every run whose cell is in the grid and which has at least one
 * sample in the band gives free[cell] += 1 - except the LAST run when its cell equals cell(w) and the ray scored a hit there.  A ray adds at
 * most 1 to any counter of a cell per run.
 * The counters are u32.  The handle keeps the number of used rays so far; an add that could carry it past 2^32 - 1 (every pixel of the add
 * taken as a used ray) is refused before any HIP call with PTL_ERR_CAPACITY and the numbers: no counter can wrap.
 * Which cells count as occupied is the caller's policy on the two counts (the Python layer's GridCounts.classify), not the library's. */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_grid_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double cell, x0, y0;
    double z_lo, z_hi, margin, step, min_range, max_range;
    int64_t max_pixels_per_scan; /* sizes the handle's sweep staging for the per-call adds: scan_cols .. 2^24 */
    int32_t nx, ny;
    int32_t scan_cols;           /* W of every sweep: sizes the handle's column table */
} ptl_grid_cfg;
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_grid_result) as the caller knows it (PTL_CFG_INIT): ptl_grid_read refuses another size or version */
    uint32_t abi_version;
    int64_t n_scans, n_scans_skipped;                  /* sweeps used / skipped as outside the trajectory's bounds */
    int64_t n_rays, n_rays_out_of_range, n_no_return;  /* pixels of the used sweeps: used rays, returns outside [min_range, max_range], no return */
    int64_t n_runs_voted;                              /* free votes over all rays (= sum_free) */
    int64_t n_ends_outside;                            /* used rays whose end lies outside the grid */
    int64_t n_cells_free, n_cells_hit;                 /* cells with a non-zero count */
    int64_t sum_free, sum_hit;
    int32_t box_ix0, box_iy0, box_ix1, box_iy1;        /* the touched box: min and max ix, iy (inclusive) over the cells with any count; an empty
                                                          box is (0, 0, -1, -1) */
    double cell, x0, y0, z_lo, z_hi, margin, step, min_range, max_range; /* the parameters as used */
    int32_t nx, ny;
    double device_ms;                                  /* HIP-event time of the handle's device work so far: sweeps, the reads' reductions */
} ptl_grid_result;
typedef struct ptl_grid ptl_grid; /* the counts of one grid: its own stream, column table, sweep staging, count arrays and counters */
/* the library's sizeof(ptl_grid_cfg) / sizeof(ptl_grid_result) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_grid_sizeof_cfg(void);
int64_t ptl_grid_sizeof_result(void);
/* the defaults above for that cell size, everything else zero; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a
 * mismatch is refused with PTL_ERR_ARG and nothing is written */
int ptl_grid_default_cfg(ptl_grid_cfg *cfg, double cell);
/* a grid of nx x ny cells on that device, all counts zero.  Checked before any HIP call, refused with the numbers (PTL_ERR_ARG): null cfg / out,
 * a cfg of another size or version, each parameter bound above, scan_cols < 1, max_pixels_per_scan outside scan_cols .. 2^24. */
int ptl_grid_create(int32_t device_id, const ptl_grid_cfg *cfg, ptl_grid **out);
int ptl_grid_destroy(ptl_grid *g);
/* one posed sweep, with the arguments of ptl_carve_add_posed_range / _xyz: *n_valid = the sweep's used rays (nullable), *skipped = 1 when a
 * column lay outside the bounds and nothing was counted but the sweep (nullable).  Trajectory, LUT and grid on one device (else PTL_ERR_ARG with
 * the ids); W = the handle's scan_cols and H W <= its max_pixels_per_scan, used rays so far + H W <= 2^32 - 1 (else PTL_ERR_CAPACITY with the
 * numbers) - all before any HIP call. */
int ptl_grid_add_posed_range(ptl_grid *g, ptl_traj *t, ptl_lut *lut, const uint32_t *range_mm, const double *col_ts, int64_t *n_valid,
                             int32_t *skipped);
int ptl_grid_add_posed_xyz(ptl_grid *g, ptl_traj *t, const float *xyz, int32_t H, int32_t W, const double *col_ts, int64_t *n_valid,
                           int32_t *skipped);
/* the RESIDENT sweeps [first, last] of a runner, no sweep crosses the bus; arguments, column times and state errors as ptl_carve_add_seq /
 * ptl_carve_add_batch.  *n_valid = used rays, *n_skipped = sweeps skipped (both nullable) */
int ptl_grid_add_seq(ptl_grid *g, ptl_seq *s, ptl_traj *t, const double *t0t1, int64_t first, int64_t last, int64_t *n_valid,
                     int64_t *n_skipped);
int ptl_grid_add_batch(ptl_grid *g, ptl_batch *b, int32_t seq, ptl_traj *t, const double *t0t1, int64_t first, int64_t last,
                       int64_t *n_valid, int64_t *n_skipped);
/* the summary so far, and (both arrays given, or neither) the counts of the rectangle of w x h cells at (ix0, iy0), row-major [h][w] with ix
 * contiguous.  result->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is refused with PTL_ERR_ARG and
 * nothing is written.  With the arrays, a rectangle that is empty or not inside the grid is PTL_ERR_ARG with the numbers; without them the
 * rectangle is not looked at.  The counts stay: sweeps may be added and read again. */
int ptl_grid_read(ptl_grid *g, ptl_grid_result *result, int32_t ix0, int32_t iy0, int32_t w, int32_t h, uint32_t *free_out, uint32_t *hit_out);
/* all counts and counters back to zero (the used rays too); the parameters stay */
int ptl_grid_clear(ptl_grid *g);

/* ------------------------------------------------------------------------------------------------
 * A sweep's rays cast through a saved map: per pixel the first stored point along the pixel's ray (no reference counterpart).
 * It answers what a posed sweep sees that the map does not and what the map holds that the sweep no longer sees, and - cast on a constant
 * range image - gives the virtual sweep that the map predicts at a pose.  The map is only read.  Every output is plainly stored per pixel; a
 * minimum with a total tie order has no order of evaluation, so status, t_hit, len and index are an exact function of the map's stored points
 * and the ray - the lane mapping and the launch geometry do not change them.  All arithmetic fp64 in the written order, without contraction.
 * Parameters: radius > 0; 0 < step <= the map's voxel size vs; min_range >= 0; max_range > min_range, max_range / step <= 65536.  The
 * defaults (radius = vs / 5, step = vs / 2, min_range = 0, max_range = 120 vs) are a caller's choice that the result echoes back, NOT tuned
 * values: nobody has run this on a real recording.  The map keeps a bounded number of points per voxel, so a thin ray can pass a wall's voxel
 * without meeting a point: radius is the caller's lever on the share of rays that hit.
 * Ray: ptl_carve's ray.  A pixel with a return; its end w is the world point the posed-scan pass gives it (ptl_icp_map_add_posed_*), its origin
 * o the translation of its own column's pose; d = w - o, len2 = (dx dx + dy dy) + dz dz, len = sqrt(len2).  status 0: no return.  status 3
 * (degenerate, counted): a return with len2 == 0 or a non-finite coordinate of w.  Every other return is cast, whatever its length: the
 * measured length is reported and never used to stop the march.  A sweep with any column outside the trajectory's bounds is skipped as a whole
 * and reported (result->skipped), as ptl_icp_map_add_posed_* skips it: every pixel then has status 0, t_hit = len = -1, index = -1.
 * March: the samples are k = 0, 1, ... while t_k = ((double)k + 0.5) step < max_range: a_k = t_k / len, s_k[c] = o[c] + a_k d[c]; there is no
 * end sample.  A sample's voxel is the map's own truncating index (int)(coordinate / vs) per axis; a sample outside the key range (2^20 voxels
 * either side) is passed over; consecutive samples with one key visit the voxel once.
 * Hit: for a point p stored in a visited voxel, e = p - o: c = e x d with six separately rounded products (cx = ey dz - ez dy, ...); p is near
 * iff (cx cx + cy cy) + cz cz <= (radius radius) len2 (the left factor made once per call, the product once per ray);
 * t_p = ((ex dx + ey dy) + ez dz) / len; p qualifies iff it is near and min_range <= t_p <= max_range.  The FIRST visited voxel, in march
 * order, that holds a qualifying point decides: the hit is that voxel's qualifying point with the smallest t_p; ties go to the lexicographically
 * smaller (x, y, z), then to the smaller pool index.  A voxel without a qualifying point is left for good, and a qualifying point with a smaller
 * t_p in a LATER voxel does not change the answer.  status 1: hit.  status 2: marched to max_range without one.
 * ONLY the voxels on the centre line are looked at.  Both rules are part of the definition, as in ptl_carve, and both are what allows a ray to
 * stop at its first hit.
 * Outputs per pixel, row-major [H][W]: status (u8); t_hit (fp64, -1 unless a hit); len (fp64, -1 unless a return; for a degenerate return the
 * value as computed, which may be 0, inf or NaN); index (i32: the hit point's index in POOL ORDER - block id, then slot: the order of
 * ptl_cast_points and of ptl_icp_map_score's, ptl_icp_map_compare's, ptl_carve_read's and ptl_paint_read's per-point outputs; -1 unless a hit).
 * What has changed is the caller's policy on len against t_hit (the Python layer's CastSweep.changes), not the library's.
 * Launch constants (ptl_build_info has no free slot): 256 threads per workgroup, a half-wave of 32 lanes per ray, at most 16384 workgroups. */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_cast_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double radius, step, min_range, max_range;
} ptl_cast_cfg;
typedef struct {
    int64_t n_pixels;                                  /* H W of the sweep */
    int64_t n_no_return, n_degenerate, n_hit, n_miss;  /* pixels per status 0, 3, 1, 2; all zero but n_pixels when the sweep was skipped */
    int64_t n_voxel_visits;                            /* visited voxels that the map holds, over all rays, up to and including each ray's deciding one */
    int32_t skipped;                                   /* 1: a column lay outside the trajectory's bounds, nothing was cast */
    int32_t reserved;
    double radius, step, min_range, max_range;         /* the parameters as used */
    double device_ms;                                  /* HIP-event time of this call's device work: upload, column table, the cast */
} ptl_cast_result;
typedef struct ptl_cast ptl_cast; /* casts through one map: its own stream, column table, sweep staging, prefixes and per-pixel output buffers */
/* the library's sizeof(ptl_cast_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_cast_sizeof_cfg(void);
/* the defaults for a map of that voxel size; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is
 * refused with PTL_ERR_ARG and nothing is written */
int ptl_cast_default_cfg(ptl_cast_cfg *cfg, double voxel_size);
/* cfg nullable: the defaults of the map's voxel size.  Waits for the map's update, snapshots its point count and the per-block prefixes of the
 * pool order.  The map handle must outlive the cast handle and is only ever read.  Checked before any HIP call, refused with the numbers
 * (PTL_ERR_ARG): null map / out, a cfg of another size or version, each parameter bound above. */
int ptl_cast_create(ptl_icp *map, const ptl_cast_cfg *cfg, ptl_cast **out);
int ptl_cast_destroy(ptl_cast *c);
/* one posed sweep, with the arguments of ptl_carve_add_posed_range / _xyz.  result and every output array are nullable; an array that is given
 * holds H W elements.  Trajectory, LUT and map on one device (else PTL_ERR_ARG with the ids); W = the map handle's scan_cols and
 * H W <= its max_points_per_scan (else PTL_ERR_CAPACITY with the numbers) - all before any HIP call.  Every call compares the map's point
 * count with the snapshot: a map updated since ptl_cast_create gives PTL_ERR_STATE.  PTL_ERR_STATE as well when the map's table leads a probe
 * to a block that does not hold the probed voxel.  Nothing is kept between calls: two calls with the same arguments give the same bytes. */
int ptl_cast_posed_range(ptl_cast *c, ptl_traj *t, ptl_lut *lut, const uint32_t *range_mm, const double *col_ts, ptl_cast_result *result,
                         uint8_t *status_out, double *t_out, double *len_out, int32_t *index_out);
int ptl_cast_posed_xyz(ptl_cast *c, ptl_traj *t, const float *xyz, int32_t H, int32_t W, const double *col_ts, ptl_cast_result *result,
                       uint8_t *status_out, double *t_out, double *len_out, int32_t *index_out);
/* the stored points (3 doubles each) in pool order, so that an index can be resolved; *n_written (nullable) their number.  max_points below
 * the map's point count: PTL_ERR_CAPACITY naming the count, nothing written. */
int ptl_cast_points(ptl_cast *c, double *xyz_out, int64_t max_points, int64_t *n_written);

/* ------------------------------------------------------------------------------------------------
 * Revisited places: polar height descriptors of sweeps, matched on the device at every heading (the Scan Context idea of Kim &
 * Kim, IROS 2018, in an integer form; no reference counterpart).  A descriptor is a polar grid of n_ring x n_sector cells around the sensor
 * holding the greatest height level per cell; a turn about z is a cyclic shift of the sector axis.  The handle is a database of descriptors
 * and compares a query with EVERY stored descriptor at EVERY shift: no ring-key pre-filter, no tree.  Past the binning comparisons everything
 * is an integer; a maximum has no order of evaluation, so a descriptor is an exact function of the SET of points and the tables, and a match
 * an exact function of the stored bytes - neither depends on the order of the points, the lane mapping or the launch geometry.
 * Parameters: n_ring R in 1 .. 64; n_sector S in 4 .. 64; 0 < min_radius < max_radius / R; z_step > 0; z_min finite; capacity (entries) in
 * 1 .. 2^20; max_points_per_scan in 1 .. 2^24.  ptl_place_default_cfg gives R = 20, S = 60, min_radius 1, max_radius 80, z_min -2,
 * z_step 0.0625, capacity 4096, max_points_per_scan 2^20: a caller's choice that nothing here has tuned - nobody has run this on a real
 * recording.
 * Tables, made once on the host at create and uploaded (ptl_place_tables returns them; they are part of the input to the definition):
 * ring_edge2[0] = min_radius min_radius, ring_edge2[i] = e e with e = max_radius (double)i / (double)R (i = 1 .. R);
 * sector_dir[2 j], [2 j + 1] = cos t_j, sin t_j with t_j = 2 pi (double)j / (double)S.
 * Descriptor of a sweep.  All arithmetic fp64 in the written order, without contraction; float32 input is converted first.  A point p is the
 * LUT's sensor-frame point of a pixel as ptl_lut_apply gives it, or a row of an xyz array.
 *   return   a range of 0, or an xyz row of (0, 0, 0), is no return (n_no_return); a non-finite coordinate drops the point (n_non_finite).
 *   level    rot9 (nullable, row-major, every entry finite): p' = (r0 x + r1 y) + r2 z per row.  Null and the identity give the same bytes.
 *   ring     rho2 = x x + y y; the ring is the largest i with ring_edge2[i] <= rho2; a point is kept iff ring_edge2[0] <= rho2 &&
 *            rho2 < ring_edge2[R] (a NaN fails it), else it is dropped (n_out_of_radius).  No square root.
 *   sector   c_j = ex_j y - ey_j x (two rounded products, one subtraction); the sector is the smallest j with c_j >= 0 &&
 *            c_((j + 1) mod S) < 0; no such j drops the point (n_no_sector).  No arctangent.
 *   level    h = (z - z_min) / z_step; a point is kept iff h >= 0 (a NaN fails it), else dropped (n_below); h >= 254.0 gives 255, compared
 *            in fp64 before any integer conversion; otherwise the level is 1 + (int)h.
 *   cell     the MAXIMUM level of its points, 0 if it has none.
 * Layout: sector-major u8, desc[j][r], column stride Rpad = R rounded up to 4, pad bytes 0; an entry is S Rpad bytes with a ptl_place_info.
 * Distance: dist(q, c, s) = sum over j < S, r < R of |q[(j + s) mod S][r] - c[j][r]| (u32, at most 64 64 255).  The best shift of a pair is
 * the s with the smallest dist, ties to the smaller s.  Convention: a query whose points are the entry's points turned by +s 2 pi / S about z
 * has best shift s and dist 0 up to binning; the rigid guess that takes query coordinates into the entry's frame is Rz(-2 pi s / S).
 * Launch constants (ptl_build_info has no free slot): 256 threads per workgroup; the match gives a lane to each shift, a wavefront to four
 * entries at a time. */
typedef struct {
    uint32_t struct_size;    /* sizeof(ptl_place_cfg) as the caller knows it (PTL_CFG_INIT) */
    uint32_t abi_version;
    double min_radius, max_radius, z_min, z_step;
    int64_t max_points_per_scan; /* sizes the handle's sweep staging */
    int32_t n_ring, n_sector;
    int32_t capacity;            /* entries */
    int32_t reserved;
} ptl_place_cfg;
typedef struct {
    int64_t n_points;                                                /* pixels / rows of the sweep */
    int64_t n_no_return, n_non_finite, n_out_of_radius, n_no_sector, n_below; /* dropped, in that order of the tests */
    int64_t n_used;                                                  /* points that reached a cell */
    int64_t n_cells, sum_levels;                                     /* non-zero cells and the sum of their levels */
} ptl_place_info;
typedef struct {
    int64_t best_query;      /* ptl_place_match: the query as given; ptl_place_match_all: the query of the best pair, -1 when none */
    int64_t best_entry;      /* the entry with the smallest dist, ties to the smaller index (match_all: then to the smaller query); -1 when none */
    int64_t n_compared;      /* (query, entry) pairs compared */
    uint32_t best_dist;
    int32_t best_shift;
    double device_ms;        /* HIP-event time of this call's device work */
} ptl_place_result;
typedef struct ptl_place ptl_place; /* a database of descriptors: its own stream, tables, sweep staging, the entries, their infos, a query slot */
/* the library's sizeof(ptl_place_cfg) (ptl_sizeof_cfg keeps its six ids) */
int64_t ptl_place_sizeof_cfg(void);
/* the defaults above; cfg->struct_size / abi_version must hold the caller's values (PTL_CFG_INIT) - a mismatch is refused with PTL_ERR_ARG and
 * nothing is written */
int ptl_place_default_cfg(ptl_place_cfg *cfg);
/* an empty database on that device.  Checked before any HIP call, refused with the numbers (PTL_ERR_ARG): null cfg / out, a cfg of another
 * size or version, each parameter bound above. */
int ptl_place_create(int32_t device_id, const ptl_place_cfg *cfg, ptl_place **out);
int ptl_place_destroy(ptl_place *p);
/* no entries, a zero query slot; parameters and tables stay */
int ptl_place_clear(ptl_place *p);
/* the number of entries */
int ptl_place_size(ptl_place *p, int64_t *n_entries);
/* the tables as uploaded: ring_edge2[R + 1], sector_dir[2 S] (both nullable) */
int ptl_place_tables(ptl_place *p, double *ring_edge2, double *sector_dir);
/* HIP-event time of the describe calls so far and their number (both nullable); reset != 0 zeroes both afterwards */
int ptl_place_profile(ptl_place *p, double *describe_ms, int64_t *n_describes, int32_t reset);
/* the descriptor of one sweep.  It always lands in the handle's QUERY SLOT; with keep = 1 it is also appended and *index is the entry count
 * before, with keep = 0 *index = -1 (index, info nullable).  A full database with keep = 1: PTL_ERR_CAPACITY with the numbers, nothing is
 * appended, the query slot and *info are still written.  Refused before any HIP call with the numbers: a LUT on another device or with more
 * than max_points_per_scan pixels, n outside 0 .. max_points_per_scan (PTL_ERR_CAPACITY above it), a dtype that is neither PTL_F32 nor
 * PTL_F64, a non-finite entry of rot9. */
int ptl_place_describe_range(ptl_place *p, ptl_lut *lut, const uint32_t *range_mm, const double *rot9, int32_t keep, int64_t *index,
                             ptl_place_info *info);
int ptl_place_describe_xyz(ptl_place *p, const void *xyz, int dtype, int64_t n, const double *rot9, int32_t keep, int64_t *index,
                           ptl_place_info *info);
/* query (an entry index, or -1 for the query slot) against every entry c in [first, last]: dist_out[c - first], shift_out[c - first] its best
 * shift and distance (both nullable), *result (nullable) the best entry.  last < first is an empty range and PTL_OK (best_entry = -1);
 * otherwise 0 <= first <= last < entries, else PTL_ERR_ARG with the numbers. */
int ptl_place_match(ptl_place *p, int64_t query, int64_t first, int64_t last, uint32_t *dist_out, int32_t *shift_out, ptl_place_result *result);
/* the loop-closure batch form: for every entry i in [q_first, q_last] the best (dist, j) over the entries j <= i - min_gap with its shift, ties
 * to the smaller j, then to the smaller shift; entry_out[i - q_first] = -1 (dist 0, shift 0) when no j qualifies.  Three integers per query
 * cross the bus (every array nullable).  min_gap >= 0; q_last < q_first is an empty range and PTL_OK. */
int ptl_place_match_all(ptl_place *p, int64_t q_first, int64_t q_last, int64_t min_gap, int32_t *entry_out, uint32_t *dist_out,
                        int32_t *shift_out, ptl_place_result *result);
/* entries [first, last]: desc_out (S Rpad bytes each) and info_out (both nullable); last < first reads nothing */
int ptl_place_read(ptl_place *p, int64_t first, int64_t last, uint8_t *desc_out, ptl_place_info *info_out);
/* appends n stored descriptors with their infos (a database saved and restored).  Refused before any HIP call: a non-zero pad byte
 * (PTL_ERR_ARG naming entry, sector and byte), entries + n above the capacity (PTL_ERR_CAPACITY with the numbers); nothing is appended then. */
int ptl_place_load(ptl_place *p, int64_t n, const uint8_t *desc, const ptl_place_info *info);

#ifdef __cplusplus
}
#endif
#endif
