// cast_kernels.h -- a sweep's rays cast through a saved map: per pixel the first stored point along the pixel's ray (include/ptudes_mi.h
// ptl_cast_*).  Read-only: nothing here writes the map, its tables or the map handle's work buffers.  Every output is plainly
// stored by the one lane that owns the pixel - no atomics on them, nothing to clear - and a minimum with a total tie order has no order of
// evaluation: status, t_hit, len and index are an exact function of the map's stored points and the ray, not of the lane mapping or the launch
// geometry.
//
// Parameters: radius > 0, 0 < step <= voxel size vs, min_range >= 0, max_range > min_range with max_range / step <= 65536.
// All arithmetic fp64 in the written order, no contraction (-ffp-contract=off).
//
//   ray      a pixel with a return; its end w = d_pose_pixel(column entry, d_fly_pixel(pixel)) of fly_kernels.h, its origin o the translation of
//            its own column's pose (entries 9 .. 11 of the column table): the carve's ray.  d = w - o, len2 = (dx dx + dy dy) + dz dz,
//            len = sqrt(len2).  status 0: no return.  status 3 (degenerate): a return with len2 == 0 or a non-finite coordinate of w.  Every
//            other return is cast whatever its length: len is reported, it never stops the march.  A sweep with any column outside the
//            trajectory's bounds is skipped as a whole (k_fly_coltab's flag): every pixel gets status 0, t_hit = len = -1, index = -1.
//   march    samples k = 0, 1, ... while t_k = ((double)k + 0.5) step < max_range: a_k = t_k / len, s_k[c] = o[c] + a_k d[c]; no end sample.
//            A sample's voxel is vox_key(s, vs), the map's own truncating index; a sample outside the key range is passed over; consecutive
//            samples with one key visit the voxel once.
//   hit      for a point p stored in a visited voxel, e = p - o: c = e x d with six separately rounded products (cx = ey dz - ez dy, ...); p is
//            near iff (cx cx + cy cy) + cz cz <= (radius radius) len2 (the left factor made once per call, the product once per ray);
//            t_p = ((ex dx + ey dy) + ez dz) / len; p qualifies iff it is near and min_range <= t_p <= max_range.  The FIRST visited voxel, in
//            march order, that holds a qualifying point decides: the hit is that voxel's qualifying point with the smallest t_p, ties to the
//            lexicographically smaller (x, y, z), then to the smaller pool index.  A voxel without a qualifying point is left for good; a
//            qualifying point with a smaller t_p in a LATER voxel does not change the answer.  status 1: hit.  status 2: marched to max_range
//            without one.
// ONLY the voxels on the centre line are looked at.  Both rules are part of the definition (as carve_kernels.h's), and both are what allows
// the early exit.
//
// Lane mapping, the carve's: a half-wave (32 lanes) per ray.  Lane l takes sample base + l and makes its key; it learns from its neighbour
// (__shfl_up; the first lane from the previous round's last key) whether the voxel is new; only then does it run map_find, take
// score_blk_count and blk_x, walk the points and keep its best (t_p, x, y, z, index).  A ballot finds the half's lowest lane with a qualifying
// point: its best is the ray's, and the ray stops after that round; otherwise the next 32 samples follow.  n_voxel_visits counts the visited
// voxels that the map holds up to and including the deciding one (the lanes behind it in the deciding round do not count): exact as well.
// Every loop is bounded by max_range / step or the voxel's point count; no workgroup waits for another.
//
//   k_cast_rays      one launch per sweep behind k_fly_coltab (fly_kernels.h, as it is); the pool-order prefix is k_score_count / k_score_scan
//                    (score_kernels.h) and k_carve_blkoff, the stored points in pool order k_carve_export (carve_kernels.h), all as they are
// A found block outside the pool, or one whose first point does not carry the probed key, is counted in `bad`: the call then fails with
// PTL_ERR_STATE.
#pragma once
#include "icp_kernels.h"
#include "fly_kernels.h"
#include "score_kernels.h"
#include "carve_kernels.h"

#define CAST_THREADS 256
#define CAST_MAX_BLOCKS 16384  // workgroups of a k_cast_rays launch (grid-stride beyond)
#define CAST_MAX_SAMPLES 65536 // max_range / step
// pixel status
#define CAST_ST_NONE 0
#define CAST_ST_HIT 1
#define CAST_ST_MISS 2
#define CAST_ST_DEGENERATE 3
// slots of the 64-bit counters
#define CAST_N_NORET 0
#define CAST_N_DEGEN 1
#define CAST_N_HIT 2
#define CAST_N_MISS 3
#define CAST_N_VISITS 4
#define CAST_N_SKIPPED 5
#define CAST_COUNTERS 8

struct CastArgs {
    double r2;                   // radius * radius (host)
    double step, min_range, max_range;
    const int* blk_off;          // [pool_cap] exclusive prefix of the stored points per block id
    int n_alloc;
    unsigned char* status;       // [n] per pixel
    double* t_hit;               // [n]
    double* len;                 // [n]
    int* index;                  // [n]
    unsigned long long* counts;  // [CAST_COUNTERS]
    int* bad;
};

// the best qualifying point of voxel `want` for one ray: q = 1 when there is one, then (bt, bi) = its t_p and pool index.  Returns 1 when the
// map holds the voxel
__device__ __forceinline__ int cast_voxel(const Ctx& c, const CastArgs& a, unsigned long long want, const double o[3], const double d[3],
                                          double len, double rr, int& q, double& bt, int& bi) {
    const int pb = map_find(c, want);
    if (pb < 0) return 0;
    const int b = pb & BLK_ID_MASK;
    if (b >= c.pool_cap) { atomicAdd(a.bad, 1); return 0; }
    const int cnt = score_blk_count(c, b);
    if (cnt == 0) return 0;
    const double* X = blk_x(c, b);
    const int out0 = a.blk_off[b];
    double bx = 0.0, by = 0.0, bz = 0.0;
    for (int j = 0; j < cnt; ++j) {
        const double px = X[3 * j], py = X[3 * j + 1], pz = X[3 * j + 2];
        const double ex = px - o[0], ey = py - o[1], ez = pz - o[2];
        const double cx = ey * d[2] - ez * d[1], cy = ez * d[0] - ex * d[2], cz = ex * d[1] - ey * d[0];
        if (!((cx * cx + cy * cy) + cz * cz <= rr)) continue;
        const double tp = ((ex * d[0] + ey * d[1]) + ez * d[2]) / len;
        if (!(tp >= a.min_range && tp <= a.max_range)) continue;
        const int oi = out0 + j;
        if (oi < 0 || oi >= a.n_alloc) continue;  // (cannot happen behind the create call's check of the directory's total)
        // (j ascends and so does the pool index: only a strictly smaller (t_p, x, y, z) takes over)
        const bool less = !q || tp < bt || (tp == bt && (px < bx || (px == bx && (py < by || (py == by && pz < bz)))));
        if (less) { q = 1; bt = tp; bi = oi; bx = px; by = py; bz = pz; }
    }
    unsigned long long have; int hx, hy, hz;
    vox_key(v3(X[0], X[1], X[2]), c.vs, have, hx, hy, hz);
    if (have != want) atomicAdd(a.bad, 1);
    return 1;
}

// the march of one ray by the 32 lanes of its half-wave (hl = lane among them, sub = the half); `use` is the same in all of them.  Every lane
// of the WAVEFRONT gets here and stays until both halves are done (the shuffles stay within a half, the loop's exit is a vote over the
// wavefront).  Returns 1 on a hit, then (r_t, r_i); `visits` as the header defines it.  In the deciding round the lanes behind the winning
// one have probed and walked their voxels before the ballot says so: their results and visits are masked, the work is spent (part of why the
// early exit buys little).
__device__ __forceinline__ int cast_ray(const Ctx& c, const CastArgs& a, bool use, const double o[3], const double d[3], double len, double len2,
                                        int hl, int sub, double& r_t, int& r_i, int& visits) {
    const double rr = a.r2 * len2;
    const double inv = 1.0 / c.vs;
    bool done = !use, prev_has = false;
    unsigned long long prev_key = 0ull;
    int found = 0;
    visits = 0;
    for (int base = 0; base < CAST_MAX_SAMPLES + 32; base += 32) {
        const int k = base + hl;
        const double tk = ((double)k + 0.5) * a.step;
        const bool in_k = !done && tk < a.max_range;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (in_k) {
            const double ak = tk / len;
            sx = o[0] + ak * d[0]; sy = o[1] + ak * d[1]; sz = o[2] + ak * d[2];
        }
        // (a coordinate beyond the key range never reaches the integer conversion: 2^20 voxels either side, 1.1e6 is past them; NaN fails too)
        const bool go = in_k && fabs(sx * inv) < 1.1e6 && fabs(sy * inv) < 1.1e6 && fabs(sz * inv) < 1.1e6;
        unsigned long long key; int kx, ky, kz;
        const bool has = vox_key(go ? v3(sx, sy, sz) : v3(0.0, 0.0, 0.0), c.vs, key, kx, ky, kz) && go;
        unsigned long long nkey = prev_key;
        bool nhas = prev_has;
        const unsigned long long uk = __shfl_up(key, 1, 32);
        const int uh = __shfl_up(has ? 1 : 0, 1, 32);
        if (hl > 0) { nkey = uk; nhas = uh != 0; }
        int q = 0, vis = 0, bi = -1;
        double bt = -1.0;
        if (has && !(nhas && nkey == key)) vis = cast_voxel(c, a, key, o, d, len, rr, q, bt, bi);
        const unsigned hq = (unsigned)(__ballot(q) >> (32 * sub)), hv = (unsigned)(__ballot(vis) >> (32 * sub));
        const int win = hq ? __ffs(hq) - 1 : 31;  // the half's lowest lane with a qualifying point: the earliest voxel of the round
        const double wt = __shfl(bt, win, 32);
        const int wi = __shfl(bi, win, 32);
        visits += __popc(hv & ((2u << win) - 1u));  // (win == 31: every lane of the half)
        if (hq && !done) { found = 1; r_t = wt; r_i = wi; done = true; }
        prev_key = __shfl(key, 31, 32);
        prev_has = __shfl(has ? 1 : 0, 31, 32) != 0;
        const bool more = !done && __shfl(in_k ? 1 : 0, 31, 32) != 0;  // the half's last lane is still inside max_range: another round
        if (!__any(more)) break;
    }
    return found;
}

// one launch per sweep, behind k_fly_coltab on the same stream; raw as d_fly_pixel reads it
template <bool RANGE>
__global__ __launch_bounds__(CAST_THREADS) void k_cast_rays(const void* raw, const double* dir, const double* off, int n, int W,
                                                            const double* coltab, const FlyWs* ws, Ctx c, CastArgs a) {
    if (ws->outside) {  // (the whole sweep is skipped: every pixel says so)
        for (long long i = (long long)blockIdx.x * CAST_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CAST_THREADS) {
            a.status[i] = CAST_ST_NONE; a.t_hit[i] = -1.0; a.len[i] = -1.0; a.index[i] = -1;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[CAST_N_SKIPPED], 1ull);
        return;
    }
    constexpr int PER_WAVE = 2;
    const int lane = threadIdx.x & 63, sub = lane >> 5, hl = lane & 31;
    const int wave = blockIdx.x * (CAST_THREADS / 64) + (threadIdx.x >> 6), waves = gridDim.x * (CAST_THREADS / 64);
    unsigned long long n_noret = 0, n_degen = 0, n_hit = 0, n_miss = 0, n_visits = 0;
    for (long long base = (long long)PER_WAVE * wave; base < n; base += (long long)PER_WAVE * waves) {  // (uniform over the wavefront)
        const long long q = base + sub;
        const bool act = q < n;
        bool use = false, ret = false;
        double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, len = 0.0, len2 = 0.0;
        if (act) {
            double p[3], M[12];
            ret = d_fly_pixel<RANGE>(raw, dir, off, (int)q, p);
            const double* m = coltab + (size_t)(q % W);
            for (int e = 0; e < 12; ++e) M[e] = m[(size_t)e * W];
            d_pose_pixel(M, p, w);
            for (int e = 0; e < 3; ++e) { o[e] = M[9 + e]; d[e] = w[e] - o[e]; }
            len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            len = sqrt(len2);
            const bool finite = fabs(w[0]) <= 1.7976931348623157e308 && fabs(w[1]) <= 1.7976931348623157e308 && fabs(w[2]) <= 1.7976931348623157e308;
            use = ret && finite && len2 != 0.0;
        }
        double r_t = -1.0;
        int r_i = -1, visits = 0;
        const int found = cast_ray(c, a, use, o, d, len, len2, hl, sub, r_t, r_i, visits);
        if (act && hl == 0) {
            const int st = !ret ? CAST_ST_NONE : (!use ? CAST_ST_DEGENERATE : (found ? CAST_ST_HIT : CAST_ST_MISS));
            a.status[q] = (unsigned char)st;
            a.t_hit[q] = found ? r_t : -1.0;
            a.len[q] = ret ? len : -1.0;
            a.index[q] = found ? r_i : -1;
            n_noret += st == CAST_ST_NONE; n_degen += st == CAST_ST_DEGENERATE; n_hit += st == CAST_ST_HIT; n_miss += st == CAST_ST_MISS;
            n_visits += (unsigned long long)visits;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        n_noret += __shfl_xor(n_noret, s); n_degen += __shfl_xor(n_degen, s); n_hit += __shfl_xor(n_hit, s); n_miss += __shfl_xor(n_miss, s);
        n_visits += __shfl_xor(n_visits, s);
    }
    if (lane == 0) {
        if (n_noret) atomicAdd(&a.counts[CAST_N_NORET], n_noret);
        if (n_degen) atomicAdd(&a.counts[CAST_N_DEGEN], n_degen);
        if (n_hit) atomicAdd(&a.counts[CAST_N_HIT], n_hit);
        if (n_miss) atomicAdd(&a.counts[CAST_N_MISS], n_miss);
        if (n_visits) atomicAdd(&a.counts[CAST_N_VISITS], n_visits);
    }
}
