// pose_kernels.h -- how well a sweep fits a voxel map at each of K candidate poses (include/ptudes_mi.h ptl_icp_pose_hits):
// the search half of "where in a saved map is the sensor now?".  The refinement half is ptl_icp_align, used as it is.
//
// A map has voxel size vs; n query points q_i (sensor frame, fp64); K candidates, row-major 4 x 4 fp64 of which the top three rows are used as
// given (nothing is re-orthonormalised); max_dist (0 < max_dist <= vs) and 1 .. 4 thresholds, ascending, each in (0, max_dist]; their squares
// are made once on the host, as doubles.  For candidate k and point i, fp64 in exactly this order, no contraction (-ffp-contract=off):
//   w         wx = ((r00 qx + r01 qy) + r02 qz) + tx, wy and wz likewise with rows 1 and 2;
//   d2(w)     what ptl_icp_map_distance defines (compare_kernels.h): the minimum over ALL stored points of (dx dx + dy dy) + dz dz, with the same
//             score_need widening at voxel faces and the same key-range rule - cmp_query itself is called, not restated;
//   hits      [k][j] = the number of i with d2 <= thr_j thr_j;
//   invalid   a query point with a non-finite coordinate is never a hit (its w is not finite either: cmp_query's NaN compares false) and is
//             counted once, not per candidate, in n_invalid_points; a candidate with a non-finite entry in its top three rows takes no probe,
//             gets hits = -1 at every threshold and is counted in n_invalid_poses; a finite pose may still carry a finite point to a w that
//             is not finite or lies outside the key range: no hit;
//   best      per threshold the largest hits[.][j] over the valid candidates and the SMALLEST candidate index that attains it; no valid candidate
//             (K = 0 included): index -1, hits 0.
// Counts of integers have no order: every output is an exact function of the SET of stored points, the query set and the pose - not of the
// pool order, the lane mapping or the launch geometry.
//
// Mapping: a workgroup takes a candidate (grid-stride over the staged chunk), so the pose is uniform over the wavefront and sits in scalar
// registers.  Within the workgroup a half-wave takes a query point, lane v of the half neighbour voxel v - cmp_query's mapping, the 27 probes of
// a point side by side.  The query points are re-read per candidate from one resident buffer (24 B a point against 27 scattered lines: no LDS
// staging).  A wavefront's hits come from a ballot over its two half leaders and stay in a register; lane 0 of each wavefront puts them into
// LDS, thread j adds the four wavefronts' in wavefront order and writes hits[k][j] with a plain store: no atomics on the result, nothing to zero.
// Every loop is bounded by n, the chunk or the voxel count, and no workgroup waits for another.
//
//   k_pose_hits      the pass above over one staged chunk of candidates
//   k_pose_invalid   one workgroup: the query points with a non-finite coordinate (integers, a fixed tree)
//   k_pose_best      one workgroup: the chunk's best candidate per threshold folded into the call's running best; the chunks come in ascending
//                    order on one stream and a later chunk wins only with MORE hits, so the smallest index stays
// A found voxel that does not hold the probed key is counted in `bad` by cmp_query: the call then fails with PTL_ERR_STATE.
// The pass only reads the map.
#pragma once
#include "compare_kernels.h"

#define POSE_THREADS 256
#define POSE_WAVES (POSE_THREADS / 64)
#define POSE_CHUNK 4096        // candidates staged and processed at a time (ptl_build_info [15])
#define POSE_MAX_THR 4
#define POSE_MAX_POINTS (1 << 20)
#define POSE_MAX_BLOCKS 1024   // workgroups of a k_pose_hits launch: a full chunk gives each four candidates (4 096 wavefronts: all resident)

struct PoseArgs {
    CmpArgs cmp;           // max_dist, max2, thr2[0 .. n_thr), n_thr, bad (cmp_query's half; d2 / xyz_out stay null)
    const double* xyz;     // [n][3] query points, sensor frame
    int n;
    const double* poses;   // [n_poses][16] the staged chunk
    int n_poses;
    int* hits;             // [n_poses][n_thr]
};

__global__ __launch_bounds__(POSE_THREADS) void k_pose_hits(Ctx c, PoseArgs a) {
    __shared__ int sh[POSE_WAVES][POSE_MAX_THR];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, hl = lane & 31, wave = tid >> 6;
    const int n_thr = a.cmp.n_thr;
    for (int k = blockIdx.x; k < a.n_poses; k += gridDim.x) {  // (uniform over the workgroup)
        const double* T = a.poses + 16 * (size_t)k;
        double m[12];
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 12; ++e) { m[e] = T[e]; ok = ok && (m[e] - m[e] == 0.0); }
        if (!ok) {  // (uniform: every thread read the same twelve words)
            if (tid < n_thr) a.hits[(size_t)k * n_thr + tid] = -1;
            continue;
        }
        int cnt[POSE_MAX_THR] = {0, 0, 0, 0};
        for (int base = 2 * wave; base < a.n; base += 2 * POSE_WAVES) {  // (uniform over the wavefront)
            const int q = base + half;
            const bool act = q < a.n;
            double qx = 0.0, qy = 0.0, qz = 0.0;
            if (act) { qx = a.xyz[3 * (size_t)q]; qy = a.xyz[3 * (size_t)q + 1]; qz = a.xyz[3 * (size_t)q + 2]; }
            const double wx = ((m[0] * qx + m[1] * qy) + m[2] * qz) + m[3];
            const double wy = ((m[4] * qx + m[5] * qy) + m[6] * qz) + m[7];
            const double wz = ((m[8] * qx + m[9] * qy) + m[10] * qz) + m[11];
            const double r = cmp_query(c, a.cmp, act, wx, wy, wz, hl);
            const bool lead = act && hl == 0;
#pragma unroll
            for (int j = 0; j < POSE_MAX_THR; ++j)
                if (j < n_thr) cnt[j] += __popcll(__ballot(lead && r <= a.cmp.thr2[j]));  // (NaN and +inf compare false)
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < POSE_MAX_THR; ++j) sh[wave][j] = cnt[j];
        }
        __syncthreads();
        if (tid < n_thr) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < POSE_WAVES; ++w) s += sh[w][tid];
            a.hits[(size_t)k * n_thr + tid] = s;
        }
        __syncthreads();  // (the next candidate's counts go into the same words)
    }
}

// out[0] = query points with a non-finite coordinate.  One workgroup; integers, a fixed tree.
__global__ __launch_bounds__(1024) void k_pose_invalid(const double* xyz, int n, int* out) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x;
    int acc = 0;
    for (int i = tid; i < n; i += 1024) {
        const double x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        acc += ((x - x == 0.0) && (y - y == 0.0) && (z - z == 0.0)) ? 0 : 1;
    }
    sh[tid] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[0] = sh[0];
}

// A candidate's rank at one threshold: hits in the high word, the index counted down in the low word - the larger key has more hits or, at
// equal hits, the smaller index.  -1 = no valid candidate.
__device__ __forceinline__ long long pose_key(int hits, long long index) { return ((long long)hits << 32) | (0x7fffffffll - index); }

// best[j] (j < n_thr) and invalid[0] hold the call's running values; `first` = this is the call's first chunk (nothing is read then, so nothing
// has to be zeroed).  index0 = the call's index of the chunk's first candidate (the host keeps every index below 2^31).
__global__ __launch_bounds__(1024) void k_pose_best(const int* hits, int n_poses, int n_thr, int index0, int first, long long* best, int* invalid) {
    __shared__ long long sh[1024];
    const int tid = threadIdx.x;
    for (int j = 0; j <= n_thr; ++j) {  // (j == n_thr: the invalid candidates' count, in the same words)
        long long acc = j < n_thr ? -1ll : 0ll;
        for (int k = tid; k < n_poses; k += 1024) {
            const int h = hits[(size_t)k * n_thr + (j < n_thr ? j : 0)];
            if (j == n_thr) acc += h < 0 ? 1 : 0;
            else if (h >= 0) { const long long key = pose_key(h, (long long)index0 + k); acc = key > acc ? key : acc; }
        }
        __syncthreads();  // (the previous quantity's readers are done)
        sh[tid] = acc;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if (tid < o) sh[tid] = j == n_thr ? sh[tid] + sh[tid + o] : (sh[tid + o] > sh[tid] ? sh[tid + o] : sh[tid]);
            __syncthreads();
        }
        if (tid == 0) {
            if (j == n_thr) invalid[0] = (first ? 0 : invalid[0]) + (int)sh[0];
            else best[j] = (first || sh[0] > best[j]) ? sh[0] : best[j];
        }
    }
}
