// carve_kernels.h -- free-space carving: which stored points of a world map did later rays pass through (include/ptudes_mi.h ptl_carve_*,
// DESIGN.md 3.24).  A second pass over the sweeps that built a map, posed by the same trajectory; per stored point it counts the rays that went
// THROUGH the point and the rays that ended AT it (support).  Every output is an integer and sums of integers have no order: each count is an
// exact function of the map's stored points and the SET of rays - not of the lane mapping, the launch geometry or the order of the sweeps.
//
// Parameters: radius > 0, margin >= 0, 0 < step <= voxel size vs, min_range >= 0, max_range > min_range with max_range / step <= 65536.
// All arithmetic fp64 in the written order, no contraction (-ffp-contract=off).
//
//   ray      a pixel with a return; its end w = d_pose_pixel(column entry, d_fly_pixel(pixel)) of fly_kernels.h, its origin o the translation of
//            its own column's pose (entries 9 .. 11 of the column table); d = w - o, len2 = (dx dx + dy dy) + dz dz, len = sqrt(len2).  Used iff
//            min_range <= len <= max_range, else counted in n_rays_out_of_range; a pixel without a return is counted in n_no_return.  A sweep
//            with any column outside the trajectory's bounds is skipped as a whole and counted (k_fly_coltab's flag, the rule of
//            ptl_icp_map_add_posed_*).
//   march    samples k = 0, 1, ... while t_k = ((double)k + 0.5) step < len: a_k = t_k / len, s_k[c] = o[c] + a_k d[c]; the last sample is w
//            itself (not o + 1 d).  A sample's voxel is vox_key(s, vs), the map's own truncating index; a sample outside the key range is
//            passed over; consecutive samples with one key visit the voxel once.  Every coordinate of s_k is monotone in k and so is the index:
//            a ray cannot return to a voxel it has left.
//   vote     for every point p stored in a visited voxel, e = p - o: c = e x d with six separately rounded products (cx = ey dz - ez dy, ...);
//            p is near the ray iff (cx cx + cy cy) + cz cz <= (radius radius) len2 (the left factor made once per call, the product once per
//            ray); t_p = ((ex dx + ey dy) + ez dz) / len.  A near point with t_p < min_range gets nothing; with t_p <= len - margin
//            through += 1; otherwise with t_p <= len + margin support += 1; beyond that nothing.
// ONLY the visited voxels are looked at: a point within `radius` of a ray whose centre line misses the point's voxel is not counted.  That is
// part of the definition (the rays of a sweep are dense against `radius`), not an approximation of another one.
//
// Lane mapping: a half-wave (32 lanes) per ray, its samples side by side as compare_kernels.h maps a query's 27 voxels.  Lane l takes sample
// base + l and makes its key; it learns from its neighbour (__shfl_up; the first lane from the previous round's last key) whether the voxel is
// new; only then does it run map_find, take score_blk_count and blk_x, walk the points and issue integer atomicAdds whose results are unused.
// Rounds of 32 until the ray is done.  A ray's probes are in flight together instead of a chain of dependent lookups in one lane (DESIGN.md
// 3.9: a dependent random line costs microseconds at load).  CARVE_LANES=1 (make EXTRA=-DCARVE_LANES=1) builds the same definition with one
// lane per ray, for the measurement of tools/map_carve_cost.py.
//
//   k_carve_blkoff   the chunk prefix of k_score_count / k_score_scan (score_kernels.h, as they are) expanded to a per-block exclusive prefix:
//                    the votes live in two u32 arrays in POOL ORDER (block id, then slot), the order of the map score's per-point outputs
//   k_carve_rays     one launch per sweep behind k_fly_coltab (fly_kernels.h, as it is)
//   k_carve_export   the stored points in pool order;  k_carve_reduce   the summary of the two vote arrays (integers, one workgroup)
// A found block outside the pool, or one whose first point does not carry the probed key, is counted in `bad`: the call then fails with
// PTL_ERR_STATE.  Nothing here writes the map, its tables or the map handle's work buffers.
#pragma once
#include "icp_kernels.h"
#include "fly_kernels.h"
#include "score_kernels.h"

#ifndef CARVE_LANES
#define CARVE_LANES 32        // lanes per ray: 32 (a half-wave, the product) or 1 (the measurement's comparison build)
#endif
#define CARVE_THREADS 256
#define CARVE_MAX_BLOCKS 16384  // workgroups of a k_carve_rays launch (grid-stride beyond)
#define CARVE_MAX_SAMPLES 65536 // max_range / step
// slots of the 64-bit counters
#define CARVE_N_RAYS 0
#define CARVE_N_OOR 1
#define CARVE_N_NORET 2
#define CARVE_N_VISITS 3
#define CARVE_N_SCANS 4
#define CARVE_N_SKIPPED 5
#define CARVE_COUNTERS 8

struct CarveArgs {
    double r2;                   // radius * radius (host)
    double margin, step, min_range, max_range;
    const int* blk_off;          // [pool_cap] exclusive prefix of the stored points per block id
    unsigned* through;           // [n_alloc]
    unsigned* support;           // [n_alloc]
    int n_alloc;
    unsigned long long* counts;  // [CARVE_COUNTERS]
    int* bad;
};

// one wavefront per chunk of SCORE_CHUNK block ids
__global__ __launch_bounds__(256) void k_carve_blkoff(Ctx c, const int* chunk_off, int* blk_off) {
    const int b = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int mine = b < c.pool_cap ? score_blk_count(c, b) : 0;
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (b < c.pool_cap) blk_off[b] = incl - mine + chunk_off[b / SCORE_CHUNK];
}

// the votes of one ray for the stored points of voxel `want`; returns 1 when the map holds the voxel
__device__ __forceinline__ int carve_voxel(const Ctx& c, const CarveArgs& a, unsigned long long want, const double o[3], const double d[3],
                                           double len, double rr, double t_thr, double t_sup) {
    const int pb = map_find(c, want);
    if (pb < 0) return 0;
    const int b = pb & BLK_ID_MASK;
    if (b >= c.pool_cap) { atomicAdd(a.bad, 1); return 0; }
    const int cnt = score_blk_count(c, b);
    if (cnt == 0) return 0;
    const double* X = blk_x(c, b);
    const int out0 = a.blk_off[b];
    for (int j = 0; j < cnt; ++j) {
        const double ex = X[3 * j] - o[0], ey = X[3 * j + 1] - o[1], ez = X[3 * j + 2] - o[2];
        const double cx = ey * d[2] - ez * d[1], cy = ez * d[0] - ex * d[2], cz = ex * d[1] - ey * d[0];
        if (!((cx * cx + cy * cy) + cz * cz <= rr)) continue;
        const double tp = ((ex * d[0] + ey * d[1]) + ez * d[2]) / len;
        const int oi = out0 + j;
        if (oi < 0 || oi >= a.n_alloc) continue;  // (cannot happen behind the create call's check of the directory's total)
        if (tp < a.min_range) continue;
        if (tp <= t_thr) atomicAdd(&a.through[oi], 1u);
        else if (tp <= t_sup) atomicAdd(&a.support[oi], 1u);
    }
    unsigned long long have; int hx, hy, hz;
    vox_key(v3(X[0], X[1], X[2]), c.vs, have, hx, hy, hz);
    if (have != want) atomicAdd(a.bad, 1);
    return 1;
}

// the march of one ray by the L lanes that share it (hl = lane among them); `use` is the same in all of them.  L == 32: every lane of the
// WAVEFRONT gets here and stays until both halves are done (the shuffles stay within a half, the loop's exit is a vote over the wavefront).
template <int L>
__device__ __forceinline__ int carve_ray(const Ctx& c, const CarveArgs& a, bool use, const double o[3], const double d[3], const double w[3],
                                         double len, double len2, int hl) {
    const double rr = a.r2 * len2, t_thr = len - a.margin, t_sup = len + a.margin;
    const double inv = 1.0 / c.vs;
    int visits = 0;
    bool prev_has = false;
    unsigned long long prev_key = 0ull;
    for (int base = 0; base <= CARVE_MAX_SAMPLES + 2 * L; base += L) {
        const int k = base + hl;
        const double tk = ((double)k + 0.5) * a.step;
        const bool in_k = use && tk < len;
        const bool last = use && !in_k && (k == 0 || ((double)(k - 1) + 0.5) * a.step < len);  // the sample behind the march: w itself
        double sx = w[0], sy = w[1], sz = w[2];
        if (in_k) {
            const double ak = tk / len;
            sx = o[0] + ak * d[0]; sy = o[1] + ak * d[1]; sz = o[2] + ak * d[2];
        }
        // (a coordinate beyond the key range never reaches the integer conversion: 2^20 voxels either side, 1.1e6 is past them; NaN fails too)
        const bool go = (in_k || last) && fabs(sx * inv) < 1.1e6 && fabs(sy * inv) < 1.1e6 && fabs(sz * inv) < 1.1e6;
        unsigned long long key; int kx, ky, kz;
        const bool has = vox_key(go ? v3(sx, sy, sz) : v3(0.0, 0.0, 0.0), c.vs, key, kx, ky, kz) && go;
        unsigned long long nkey = prev_key;
        bool nhas = prev_has;
        if constexpr (L > 1) {
            const unsigned long long uk = __shfl_up(key, 1, L);
            const int uh = __shfl_up(has ? 1 : 0, 1, L);
            if (hl > 0) { nkey = uk; nhas = uh != 0; }
        }
        if (has && !(nhas && nkey == key)) visits += carve_voxel(c, a, key, o, d, len, rr, t_thr, t_sup);
        if constexpr (L > 1) {
            prev_key = __shfl(key, L - 1, L);
            prev_has = __shfl(has ? 1 : 0, L - 1, L) != 0;
            const bool more = __shfl(in_k ? 1 : 0, L - 1, L) != 0;  // the half's last lane is still inside the ray: another round
            if (!__any(more)) break;
        } else {
            prev_key = key; prev_has = has;
            if (!in_k) break;
        }
    }
    return visits;
}

// one launch per sweep, behind k_fly_coltab on the same stream; raw as d_fly_pixel reads it
template <bool RANGE>
__global__ __launch_bounds__(CARVE_THREADS) void k_carve_rays(const void* raw, const double* dir, const double* off, int n, int W,
                                                              const double* coltab, const FlyWs* ws, Ctx c, CarveArgs a) {
    if (ws->outside) {  // (the whole sweep is skipped)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[CARVE_N_SKIPPED], 1ull);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[CARVE_N_SCANS], 1ull);
    constexpr int L = CARVE_LANES, PER_WAVE = 64 / L;
    const int lane = threadIdx.x & 63, sub = lane / L, hl = lane % L;
    const int wave = blockIdx.x * (CARVE_THREADS / 64) + (threadIdx.x >> 6), waves = gridDim.x * (CARVE_THREADS / 64);
    int n_rays = 0, n_oor = 0, n_noret = 0, n_visits = 0;
    for (long long base = (long long)PER_WAVE * wave; base < n; base += (long long)PER_WAVE * waves) {  // (uniform over the wavefront)
        const long long q = base + sub;
        const bool act = q < n;
        bool use = false;
        double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, len = 0.0, len2 = 0.0;
        if (act) {
            double p[3], M[12];
            const bool ret = d_fly_pixel<RANGE>(raw, dir, off, (int)q, p);
            const double* m = coltab + (size_t)(q % W);
            for (int e = 0; e < 12; ++e) M[e] = m[(size_t)e * W];
            d_pose_pixel(M, p, w);
            for (int e = 0; e < 3; ++e) { o[e] = M[9 + e]; d[e] = w[e] - o[e]; }
            len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            len = sqrt(len2);
            use = ret && len >= a.min_range && len <= a.max_range;
            if (hl == 0) {
                if (!ret) n_noret += 1;
                else if (!use) n_oor += 1;
                else n_rays += 1;
            }
        }
        n_visits += carve_ray<L>(c, a, use, o, d, w, len, len2, hl);
    }
    for (int s = 32; s > 0; s >>= 1) {
        n_rays += __shfl_xor(n_rays, s); n_oor += __shfl_xor(n_oor, s); n_noret += __shfl_xor(n_noret, s); n_visits += __shfl_xor(n_visits, s);
    }
    if (lane == 0) {
        if (n_rays) atomicAdd(&a.counts[CARVE_N_RAYS], (unsigned long long)n_rays);
        if (n_oor) atomicAdd(&a.counts[CARVE_N_OOR], (unsigned long long)n_oor);
        if (n_noret) atomicAdd(&a.counts[CARVE_N_NORET], (unsigned long long)n_noret);
        if (n_visits) atomicAdd(&a.counts[CARVE_N_VISITS], (unsigned long long)n_visits);
    }
}

// the stored points in pool order (the order of the vote arrays), one thread per block id
__global__ __launch_bounds__(256) void k_carve_export(Ctx c, const int* blk_off, int n_alloc, double* xyz) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= c.pool_cap) return;
    const int cnt = score_blk_count(c, b);
    if (cnt == 0) return;
    const double* X = blk_x(c, b);
    const int out0 = blk_off[b];
    for (int j = 0; j < cnt; ++j) {
        const int oi = out0 + j;
        if (oi < 0 || oi >= n_alloc) continue;
        xyz[3 * (size_t)oi] = X[3 * j]; xyz[3 * (size_t)oi + 1] = X[3 * j + 1]; xyz[3 * (size_t)oi + 2] = X[3 * j + 2];
    }
}

// out[0] = points with through > 0, out[1] = points with support > 0, out[2] = sum of through, out[3] = sum of support.  One workgroup.
__global__ __launch_bounds__(1024) void k_carve_reduce(const unsigned* through, const unsigned* support, int n, unsigned long long* out) {
    __shared__ unsigned long long sh[4][1024];
    const int tid = threadIdx.x;
    unsigned long long nt = 0, ns = 0, st = 0, ss = 0;
    for (int i = tid; i < n; i += 1024) {
        const unsigned t = through[i], s = support[i];
        nt += t ? 1 : 0; ns += s ? 1 : 0; st += t; ss += s;
    }
    sh[0][tid] = nt; sh[1][tid] = ns; sh[2][tid] = st; sh[3][tid] = ss;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; sh[2][tid] += sh[2][tid + o]; sh[3][tid] += sh[3][tid + o]; }
        __syncthreads();
    }
    if (tid < 4) out[tid] = sh[tid][0];
}
