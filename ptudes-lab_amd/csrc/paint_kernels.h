// paint_kernels.h -- the world map painted: a lidar channel field summed per STORED point (include/ptudes_mi.h ptl_paint_*).
// A second pass over the sweeps that built a map, posed by the same trajectory, each with a field image u32[H][W] (reflectivity, signal,
// near-infrared, the range itself).  Every output is an integer and sums of integers have no order: each sum and count is an exact function of
// the map's stored points and the SET of (ray, value) pairs - not of the lane mapping, the launch geometry or the order of the sweeps.
//
//   ray      a pixel with a return; its end w = d_pose_pixel(column entry, d_fly_pixel(pixel)) of fly_kernels.h - the functions the map build
//            (k_fly_emit) and the carve call, called here and not restated, so w carries the bits the build stored.  A pixel without a return
//            is counted in n_no_return and adds nothing, whatever its field value.  A sweep with any column outside the trajectory's bounds
//            is skipped as a whole and counted (k_fly_coltab's flag, the rule of ptl_icp_map_add_posed_*).
//   voxel    vox_key(w, vs), the map's own truncating index, behind the carve's range guard (|coordinate / vs| < 1.1e6 before the integer
//            conversion; NaN fails it).  A w outside the key range makes the ray unmatched.
//   paint    map_find looks the voxel up; for every stored point p of that voxel with p.x == w.x && p.y == w.y && p.z == w.z (comparison of
//            doubles): sum[p] += field[pixel] (u64), count[p] += 1 (u32).  A ray that matched at least one point counts in n_rays_matched, any
//            other ray - into a full voxel, into an absent voxel, out of the key range - in n_rays_unmatched.
// A map built from sweeps S on trajectory T and painted with S on T therefore has count >= 1 at every stored point (a voxel's first P points are
// among those rays), and n_rays_unmatched is the number of returns the build did not store.
//
// Lane mapping: one lane per pixel.  The raw sweep, the field image and the column table are read coalesced (consecutive lanes, consecutive
// words); the 64 rays of a wavefront probe the table independently, one map_find each - a ray has ONE voxel, so there is no chain of dependent
// lookups to spread over lanes as the carve's march has.  The point loop is bounded by the voxel's count (score_blk_count, at most the block's
// capacity), the probe by the table's size (map_find).  The adds are plain atomicAdd on u64 / u32 whose results are unused.
//
//   k_paint_rays     one launch per sweep behind k_fly_coltab (fly_kernels.h, as it is)
//   k_paint_reduce   the summary of the count array (integers, one workgroup)
// The per-block prefix of the pool order is k_score_count / k_score_scan (score_kernels.h) expanded by k_carve_blkoff, and the stored points
// come out through k_carve_export (carve_kernels.h) - all four as they are: the walk's per-block count and the prefix's per-block count are ONE
// function, score_blk_count.  A found block outside the pool, or one whose first point does not carry the probed key, is counted in `bad`: the
// call then fails with PTL_ERR_STATE.  Nothing here writes the map, its tables or the map handle's work buffers.
#pragma once
#include "icp_kernels.h"
#include "fly_kernels.h"
#include "score_kernels.h"
#include "carve_kernels.h"

#define PAINT_THREADS 256
#define PAINT_MAX_BLOCKS 16384  // workgroups of a k_paint_rays launch (grid-stride beyond)
// slots of the 64-bit counters
#define PAINT_N_MATCHED 0
#define PAINT_N_UNMATCHED 1
#define PAINT_N_NORET 2
#define PAINT_N_SCANS 3
#define PAINT_N_SKIPPED 4
#define PAINT_COUNTERS 8

struct PaintArgs {
    const int* blk_off;          // [pool_cap] exclusive prefix of the stored points per block id
    unsigned long long* sum;     // [n_alloc], pool order
    unsigned* count;             // [n_alloc]
    int n_alloc;
    unsigned long long* counts;  // [PAINT_COUNTERS]
    int* bad;
};

// the stored points of voxel `want` that ARE w get the value; returns 1 when at least one did
__device__ __forceinline__ int paint_voxel(const Ctx& c, const PaintArgs& a, unsigned long long want, const double w[3], unsigned value) {
    const int pb = map_find(c, want);
    if (pb < 0) return 0;
    const int b = pb & BLK_ID_MASK;
    if (b >= c.pool_cap) { atomicAdd(a.bad, 1); return 0; }
    const int cnt = score_blk_count(c, b);
    if (cnt == 0) return 0;
    const double* X = blk_x(c, b);
    const int out0 = a.blk_off[b];
    int hit = 0;
    for (int j = 0; j < cnt; ++j) {
        if (!(X[3 * j] == w[0] && X[3 * j + 1] == w[1] && X[3 * j + 2] == w[2])) continue;
        const int oi = out0 + j;
        if (oi < 0 || oi >= a.n_alloc) continue;  // (cannot happen behind the create call's check of the directory's total)
        atomicAdd(&a.sum[oi], (unsigned long long)value);
        atomicAdd(&a.count[oi], 1u);
        hit = 1;
    }
    unsigned long long have; int hx, hy, hz;
    vox_key(v3(X[0], X[1], X[2]), c.vs, have, hx, hy, hz);
    if (have != want) atomicAdd(a.bad, 1);
    return hit;
}

// one launch per sweep, behind k_fly_coltab on the same stream; raw as d_fly_pixel reads it, field the u32 image of the same pixels
template <bool RANGE>
__global__ __launch_bounds__(PAINT_THREADS) void k_paint_rays(const void* raw, const double* dir, const double* off, const unsigned* field, int n,
                                                              int W, const double* coltab, const FlyWs* ws, Ctx c, PaintArgs a) {
    if (ws->outside) {  // (the whole sweep is skipped)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[PAINT_N_SKIPPED], 1ull);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[PAINT_N_SCANS], 1ull);
    const int lane = threadIdx.x & 63;
    const double inv = 1.0 / c.vs;
    int n_match = 0, n_unmatch = 0, n_noret = 0;
    for (long long base = (long long)blockIdx.x * PAINT_THREADS; base < n; base += (long long)gridDim.x * PAINT_THREADS) {  // (uniform over the workgroup)
        const long long q = base + threadIdx.x;
        const bool act = q < n;
        bool ret = false;
        unsigned value = 0u;
        double w[3] = {0.0, 0.0, 0.0};
        if (act) {
            double p[3], M[12];
            ret = d_fly_pixel<RANGE>(raw, dir, off, (int)q, p);
            value = field[q];
            const double* m = coltab + (size_t)(q % W);
            for (int e = 0; e < 12; ++e) M[e] = m[(size_t)e * W];
            d_pose_pixel(M, p, w);
        }
        // (a coordinate beyond the key range never reaches the integer conversion: 2^20 voxels either side, 1.1e6 is past them; NaN fails too)
        const bool go = ret && fabs(w[0] * inv) < 1.1e6 && fabs(w[1] * inv) < 1.1e6 && fabs(w[2] * inv) < 1.1e6;
        unsigned long long key; int kx, ky, kz;
        const bool has = vox_key(go ? v3(w[0], w[1], w[2]) : v3(0.0, 0.0, 0.0), c.vs, key, kx, ky, kz) && go;
        const int hit = has ? paint_voxel(c, a, key, w, value) : 0;
        if (act) {
            if (!ret) n_noret += 1;
            else if (hit) n_match += 1;
            else n_unmatch += 1;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        n_match += __shfl_xor(n_match, s); n_unmatch += __shfl_xor(n_unmatch, s); n_noret += __shfl_xor(n_noret, s);
    }
    if (lane == 0) {
        if (n_match) atomicAdd(&a.counts[PAINT_N_MATCHED], (unsigned long long)n_match);
        if (n_unmatch) atomicAdd(&a.counts[PAINT_N_UNMATCHED], (unsigned long long)n_unmatch);
        if (n_noret) atomicAdd(&a.counts[PAINT_N_NORET], (unsigned long long)n_noret);
    }
}

// out[0] = points with count > 0, out[1] = sum of count.  One workgroup.
__global__ __launch_bounds__(1024) void k_paint_reduce(const unsigned* count, int n, unsigned long long* out) {
    __shared__ unsigned long long sh[2][1024];
    const int tid = threadIdx.x;
    unsigned long long np = 0, sc = 0;
    for (int i = tid; i < n; i += 1024) {
        const unsigned k = count[i];
        np += k ? 1 : 0; sc += k;
    }
    sh[0][tid] = np; sh[1][tid] = sc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; }
        __syncthreads();
    }
    if (tid < 2) out[tid] = sh[tid][0];
}
