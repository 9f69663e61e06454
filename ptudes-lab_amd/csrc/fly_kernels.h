// fly_kernels.h -- posed scans into the world map (the map fly-by's compute half).
//
// The ONE definition of the posed-scan arithmetic: the geodesic pose of a time-stamped trajectory (d_traj_pose_at), the sensor-frame
// point of a range-image pixel (d_lut_pixel) and the pose product of a pixel with its column's transform (d_pose_pixel).  The per-call
// stage kernels of ptudes_mi.hip (k_traj_poses_at, k_dewarp) and the fused passes below call the same functions, so the three-call
// path (poses_at -> dewarp -> map_add through the host) and the fused one give the same bits.
//
// Fused passes, per scan, all on the MAP handle's stream and buffers (coltab, bcnt1, d_in, FlyWs):
//   k_fly_coltab  one thread per column: binary search over the resident knots, SE(3) geodesic, 12 doubles into the entry-major
//                 [12][W] table (coltab's layout: consecutive pixels read consecutive words); one workgroup, so the per-scan
//                 "outside" flag is a workgroup vote written once, with no atomics and nothing to clear between scans
//   k_fly_count   returns per 256-pixel block (the prefix of the next pass)
//   k_fly_emit    pixel -> world point with its column's entry, compacted IN SCAN ORDER (a voxel keeps its first points in scan
//                 order) into the handle's point buffer; leaves the device count the map insert passes take as n_ptr
// then k_map_insert_a / b / c of icp_kernels.h, as ptl_icp_map_add runs them.  A scan with any column outside the bounds adds nothing.
#pragma once
#include "icp_kernels.h"

// Poses along a time-stamped trajectory == ouster.sdk.pose_util.TrajectoryEvaluator as the reference uses it
// (utils.py:344-392 pose_scans_from_nc_gt, time_bounds = 1.5; cli/ekf_bench.py:489, :537 --use-gt-guess, time_bounds = 1.0;
// third-party, [UPSTREAM-KNOWLEDGE]): between the knots (t_i, P_i) that bracket t the pose is the SE(3) geodesic
//   P(t) = P_i Exp(alpha Log(P_i^-1 P_i+1)),  alpha = (t - t_i) / (t_i+1 - t_i);
// up to `before` / `after` seconds outside the knots the first / last segment is extended (alpha < 0 / > 1); further out
// there is no pose (false; the reference skips such scans, utils.py:382-384).  Binary search for the segment.
__device__ __forceinline__ bool d_traj_pose_at(const double* kt, const double* kp, int n, double before, double after, double t, Rt* out) {
    if (!(t >= kt[0] - before) || !(t <= kt[n - 1] + after)) return false;
    int lo = 0, hi = n - 1;  // largest i with kt[i] <= t, clamped to a valid segment start
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kt[mid] <= t) lo = mid; else hi = mid;
    }
    const int i = lo < n - 1 ? lo : n - 2;
    const double alpha = (t - kt[i]) / (kt[i + 1] - kt[i]);
    const Rt P0 = rt_from16(kp + 16 * (size_t)i), P1 = rt_from16(kp + 16 * (size_t)(i + 1));
    double xi[6];
    se3_log(rt_mul(rt_inv(P0), P1), xi);
    for (int k = 0; k < 6; ++k) xi[k] *= alpha;
    *out = rt_mul(P0, se3_exp(xi));
    return true;
}
// XYZLut of pixel i: range (mm) x direction + offset, metres; no return (range 0) -> (0, 0, 0)
__device__ __forceinline__ void d_lut_pixel(unsigned rg, const double* dir, const double* off, size_t i, double p[3]) {
    const double r = (double)rg;
    for (int k = 0; k < 3; ++k) p[k] = rg ? r * dir[3 * i + k] + off[3 * i + k] : 0.0;
}
// ouster client.dewarp of one pixel: R p + t with its column's transform M (R row-major 9, t 3), in this order of operations
__device__ __forceinline__ void d_pose_pixel(const double M[12], const double p[3], double w[3]) {
    for (int k = 0; k < 3; ++k) w[k] = ((M[3 * k] * p[0] + M[3 * k + 1] * p[1]) + M[3 * k + 2] * p[2]) + M[9 + k];
}

// what the fused passes leave on the device, one per map handle
struct FlyWs {
    int n;                 // returns of the last scan in the handle's point buffer (0 when it was skipped): n_ptr of the map insert
    int outside;           // the last scan had a column outside the trajectory's bounds
    long long n_valid;     // returns added / scans skipped since the caller cleared them (a multi-scan build reads them once, at its end)
    long long n_skipped;
};

// column j of the sweep fires at col_ts[j], or (col_ts null) at t0 + (j / W)(t1 - t0) - the IMU deskew's convention
__global__ __launch_bounds__(256) void k_fly_coltab(const double* kt, const double* kp, int n, double before, double after,
                                                    const double* col_ts, double t0, double t1, int W, double* coltab, FlyWs* ws) {
    bool out_any = false;
    for (int j = (int)threadIdx.x; j < W; j += 256) {
        const double t = col_ts ? col_ts[j] : t0 + ((double)j / (double)W) * (t1 - t0);
        Rt P;
        if (!d_traj_pose_at(kt, kp, n, before, after, t, &P)) { out_any = true; P = rt_identity(); }
        double* o = coltab + (size_t)j;  // entry q of column j at [q W + j]
        for (int q = 0; q < 9; ++q) o[(size_t)q * W] = P.R[q];
        for (int q = 0; q < 3; ++q) o[(size_t)(9 + q) * W] = P.t[q];
    }
    const int any = __syncthreads_or(out_any ? 1 : 0);
    if (threadIdx.x == 0) ws->outside = any;
}

// the raw sweep in HBM: a u32 range image with its LUT (RANGE = true), or f32 xyz in the sensor frame with (0, 0, 0) = no return
template <bool RANGE>
__device__ __forceinline__ bool d_fly_pixel(const void* raw, const double* dir, const double* off, int i, double p[3]) {
    if (RANGE) {
        const unsigned rg = ((const unsigned*)raw)[i];
        d_lut_pixel(rg, dir, off, (size_t)i, p);
        return rg != 0u;
    }
    const float* x = (const float*)raw + 3 * (size_t)i;
    const float a = x[0], b = x[1], c = x[2];
    p[0] = (double)a; p[1] = (double)b; p[2] = (double)c;
    return a != 0.0f || b != 0.0f || c != 0.0f;
}
template <bool RANGE>
__global__ __launch_bounds__(256) void k_fly_count(const void* raw, int n, int* bcnt, const FlyWs* ws) {
    if (ws->outside) return;  // (the whole scan is skipped: the next pass does not read the counts)
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    bool v = false;
    if (i < n) {
        if (RANGE) v = ((const unsigned*)raw)[i] != 0u;
        else { const float* x = (const float*)raw + 3 * (size_t)i; v = x[0] != 0.0f || x[1] != 0.0f || x[2] != 0.0f; }
    }
    const int nv = __syncthreads_count(v ? 1 : 0);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = nv;
}
template <bool RANGE>
__global__ __launch_bounds__(256) void k_fly_emit(const void* raw, const double* dir, const double* off, int n, int W, const double* coltab,
                                                  const int* bcnt, double* out, FlyWs* ws) {
    const int b = (int)blockIdx.x, last = (int)gridDim.x - 1;
    if (ws->outside) {
        if (b == last && threadIdx.x == 0) { ws->n = 0; ws->n_skipped += 1; }
        return;
    }
    const int off_part = block_offset_part(bcnt, b);
    const int i = b * 256 + (int)threadIdx.x;
    bool v[1] = {false};
    double w[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        double p[3], M[12];
        v[0] = d_fly_pixel<RANGE>(raw, dir, off, i, p);
        const double* m = coltab + (size_t)(i % W);
        for (int q = 0; q < 12; ++q) M[q] = m[(size_t)q * W];
        d_pose_pixel(M, p, w);
    }
    int rk[1], total;
    block_rank_u<1>(v, rk, total);
    const int o0 = block_offset(off_part);
    if (v[0]) {
        const size_t o = (size_t)(o0 + rk[0]) * 3;
        out[o] = w[0]; out[o + 1] = w[1]; out[o + 2] = w[2];
    }
    if (b == last && threadIdx.x == 0) { ws->n = o0 + total; ws->n_valid += o0 + total; }
}
