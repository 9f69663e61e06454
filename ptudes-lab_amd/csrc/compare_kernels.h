// compare_kernels.h -- distance of query points to the stored points of a voxel map (include/ptudes_mi.h ptl_icp_map_distance /
// ptl_icp_map_compare): the cloud-to-cloud nearest-neighbour distance, with the map as the search structure.
//
// A reference map R has voxel size vs and P points per voxel; parameters max_dist (0 < max_dist <= vs) and 1 .. 8 thresholds, ascending,
// each in (0, max_dist].  For every query point q:
//   d2(q)     the minimum over ALL stored points p of R of (dx dx + dy dy) + dz dz, d = p - q, fp64 in exactly this order, no contraction
//             (-ffp-contract=off);
//   matched   d2(q) <= max_dist max_dist (the product is made once on the host, as a double); the per-point output is d2 itself for a
//             matched point and +inf otherwise;
//   invalid   a query with a non-finite coordinate: counted as n_invalid, its output is NaN;
//   range     a query whose voxel index lies outside the key range (KEY_OFF) is unmatched and takes no table probe;
//   n_within  [k] counts the queries with d2 <= thr_k thr_k (the squares are made on the host as well).
// A minimum does not depend on the order of its terms: d2, the match and every count are exact functions of the SET of stored points and the
// query - not of the pool order, a block id, the launch geometry or the lane mapping.
//
// max_dist <= vs: with the truncating voxel index (vox_key) index 0 spans (-vs, vs) and every other index one vs, so a stored point within
// max_dist of a query of voxel k lies in voxels k - 1 .. k + 1 on each axis - in exact arithmetic.  The rounded expression admits a pair whose
// exact distance exceeds max_dist by less than one rounding; at max_dist = vs such a pair can sit two voxels apart, and a query that close to
// a face probes one voxel further on that axis (score_need of score_kernels.h, the same situation).  A stored point outside the probed voxels is
// farther than max_dist under the rounded expression too, so leaving it out changes no output: every output above max_dist^2 is +inf.
//
// Lane mapping: a half-wave (32 lanes) per query.  Lane v of the half takes neighbour voxel v (27 of them, (i, j, k) ascending; up to 125 with
// the rare extra voxels, in rounds of 32): map_find, the voxel's stored count from the directory with the clamp of score_blk_count, its points
// straight from the pool, its own running minimum; a __shfl_xor minimum tree over the half gives the result and lane 0 of the half writes it.
// The 27 probes of a query are therefore in flight side by side instead of a chain of 27 dependent lookups in one lane (a
// dependent random line costs microseconds at load).
//
//   k_cmp_points<CmpArraySrc>  queries from an n x 3 fp64 array (a staged chunk of the host's); a wavefront takes two consecutive queries
//   k_cmp_points<CmpPoolSrc>   queries are the stored points of a second map, in pool order (block id, then slot): a wavefront takes 64 consecutive
//                              block ids, reads their counts (coalesced), and walks their points two at a time; the output index comes from the
//                              chunk prefix of k_score_count / k_score_scan (score_kernels.h), used as they are
//   k_cmp_reduce               one workgroup: thread t adds entries t, t + 1024, ... in that order, then a fixed tree in LDS - no float atomics
// A found voxel whose first stored point does not carry the probed key, or whose block id lies outside the pool, is counted in `bad` (an integer
// atomic): the call then fails with PTL_ERR_STATE instead of reporting distances to an inconsistent table.
// The pass only reads both maps.
#pragma once
#include "icp_kernels.h"
#include "score_kernels.h"

#define CMP_THREADS 256
#define CMP_CHUNK (1 << 17)   // queries of the array source staged and processed at a time
#define CMP_MAX_THR 8
#define CMP_MAX_BLOCKS 16384  // workgroups of a k_cmp_points launch (grid-stride beyond)
#define CMP_SUMS 16           // doubles of a reduced summary (k_cmp_reduce)

struct CmpArgs {
    double max_dist, max2;       // max2 = max_dist * max_dist (host)
    double thr2[CMP_MAX_THR];    // thr_k * thr_k (host)
    int n_thr;
    int n_alloc;                 // entries of d2 (and of xyz_out)
    double* d2;                  // [n_alloc]
    double* xyz_out;             // [n_alloc][3] or null (pool source)
    int* bad;
};

struct CmpArraySrc {
    const double* xyz;  // [n][3]
    int n;
};
struct CmpPoolSrc {
    Ctx c;                 // the map whose stored points are the queries
    const int* chunk_off;  // exclusive prefix of its points per chunk of SCORE_CHUNK block ids (k_score_scan)
    int n_chunks;
};

// d2 of one query against the stored points of c, for the 32 lanes of a half together (hl = lane within the half); every lane of the WAVEFRONT
// gets here (the voxel index votes across it, the minimum tree shuffles within the half), `act` says whether this half holds a query.
// Returns in every lane of the half: d2 when matched, +inf when not, NaN for a non-finite query.
__device__ __forceinline__ double cmp_query(const Ctx& c, const CmpArgs& a, bool act, double qx, double qy, double qz, int hl) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const bool finite = (qx - qx == 0.0) && (qy - qy == 0.0) && (qz - qz == 0.0);
    // (a coordinate beyond the key range never reaches the integer conversion: 2^20 voxels either side, 1.1e6 is past them)
    const double inv = 1.0 / c.vs;
    const bool near_enough = finite && fabs(qx * inv) < 1.1e6 && fabs(qy * inv) < 1.1e6 && fabs(qz * inv) < 1.1e6;
    const bool go = act && near_enough;
    unsigned long long key; int kx, ky, kz;
    const bool in_keys = vox_key(go ? v3(qx, qy, qz) : v3(0.0, 0.0, 0.0), c.vs, key, kx, ky, kz);
    double best = inf;
    if (go && in_keys) {
        const int nx = score_need(qx, kx, c.vs, a.max_dist), ny = score_need(qy, ky, c.vs, a.max_dist), nz = score_need(qz, kz, c.vs, a.max_dist);
        const int x0 = -1 - ((nx >> 1) & 1), y0 = -1 - ((ny >> 1) & 1), z0 = -1 - ((nz >> 1) & 1);
        const int cx = 3 + (nx & 1) + ((nx >> 1) & 1), cy = 3 + (ny & 1) + ((ny >> 1) & 1), cz = 3 + (nz & 1) + ((nz >> 1) & 1);
        const int n_vox = cx * cy * cz;  // 27, rarely up to 125
        for (int v = hl; v < n_vox; v += 32) {
            const int vx = kx + x0 + v / (cy * cz), vy = ky + y0 + (v / cz) % cy, vz = kz + z0 + v % cz;
            if ((((unsigned)(vx + KEY_OFF) | (unsigned)(vy + KEY_OFF) | (unsigned)(vz + KEY_OFF)) >> 21) != 0u) continue;
            const unsigned long long want = pack_key(vx, vy, vz);
            const int pb = map_find(c, want);
            if (pb < 0) continue;
            const int b = pb & BLK_ID_MASK;
            if (b >= c.pool_cap) { atomicAdd(a.bad, 1); continue; }
            const int cnt = score_blk_count(c, b);
            if (cnt == 0) continue;
            const double* X = blk_x(c, b);
            for (int j = 0; j < cnt; ++j) {
                const double dx = X[3 * j] - qx, dy = X[3 * j + 1] - qy, dz = X[3 * j + 2] - qz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                best = d2 < best ? d2 : best;
            }
            unsigned long long have; int hx, hy, hz;
            vox_key(v3(X[0], X[1], X[2]), c.vs, have, hx, hy, hz);
            if (have != want) atomicAdd(a.bad, 1);
        }
    }
    for (int o = 16; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    return !finite ? nan : (best <= a.max2 ? best : inf);
}

__device__ __forceinline__ void cmp_walk(const CmpArraySrc& s, const Ctx& c, const CmpArgs& a) {
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const int wave = blockIdx.x * (CMP_THREADS / 64) + (threadIdx.x >> 6), waves = gridDim.x * (CMP_THREADS / 64);
    for (long long base = 2ll * wave; base < s.n; base += 2ll * waves) {  // (uniform over the wavefront)
        const long long q = base + half;
        const bool act = q < s.n;
        double qx = 0.0, qy = 0.0, qz = 0.0;
        if (act) { qx = s.xyz[3 * q]; qy = s.xyz[3 * q + 1]; qz = s.xyz[3 * q + 2]; }
        const double r = cmp_query(c, a, act, qx, qy, qz, hl);
        if (act && hl == 0 && q < a.n_alloc) a.d2[q] = r;
    }
}

__device__ __forceinline__ void cmp_walk(const CmpPoolSrc& s, const Ctx& c, const CmpArgs& a) {
    const Ctx& m = s.c;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const int wave = blockIdx.x * (CMP_THREADS / 64) + (threadIdx.x >> 6), waves = gridDim.x * (CMP_THREADS / 64);
    for (int ch = wave; ch < s.n_chunks; ch += waves) {  // (uniform over the wavefront)
        const int b0 = ch * SCORE_CHUNK;
        const int mine = b0 + lane < m.pool_cap ? score_blk_count(m, b0 + lane) : 0;
        int incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const int excl = incl - mine + s.chunk_off[ch];
        if (__ballot(mine > 0) == 0ull) continue;
        for (int bi = 0; bi < SCORE_CHUNK; ++bi) {
            const int cnt = __shfl(mine, bi);
            if (cnt == 0) continue;  // (uniform)
            const int out0 = __shfl(excl, bi);
            const double* X = blk_x(m, b0 + bi);
            for (int p0 = 0; p0 < cnt; p0 += 2) {
                const int pt = p0 + half;
                const bool act = pt < cnt;
                double qx = 0.0, qy = 0.0, qz = 0.0;
                if (act) { qx = X[3 * pt]; qy = X[3 * pt + 1]; qz = X[3 * pt + 2]; }
                const double r = cmp_query(c, a, act, qx, qy, qz, hl);
                const int o = out0 + pt;
                if (act && hl == 0 && o < a.n_alloc) {
                    a.d2[o] = r;
                    if (a.xyz_out) { a.xyz_out[3 * (size_t)o] = qx; a.xyz_out[3 * (size_t)o + 1] = qy; a.xyz_out[3 * (size_t)o + 2] = qz; }
                }
            }
        }
    }
}

// c: the reference map; s: where the queries come from
template <class SRC>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_points(SRC s, Ctx c, CmpArgs a) {
    cmp_walk(s, c, a);
}

// out[0] = invalid queries, out[1] = matched, out[2] = sum of sqrt(d2), out[3] = sum of d2, out[4] = largest d2 (the last three over the matched
// queries), out[5 + k] = queries with d2 <= thr2[k].  The counts are exact: integers below 2^53.  One workgroup; thread t takes entries t,
// t + 1024, ... in that order, then a fixed tree.
__global__ __launch_bounds__(1024) void k_cmp_reduce(const double* d2, int n, CmpArgs a, double* out) {
    __shared__ double sh[1024];
    const int tid = threadIdx.x;
    double acc[5 + CMP_MAX_THR];
#pragma unroll
    for (int k = 0; k < 5 + CMP_MAX_THR; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const double v = d2[i];
        if (v != v) { acc[0] += 1.0; continue; }
        if (!(v <= a.max2)) continue;
        acc[1] += 1.0; acc[2] += sqrt(v); acc[3] += v; acc[4] = v > acc[4] ? v : acc[4];
#pragma unroll
        for (int k = 0; k < CMP_MAX_THR; ++k)
            if (k < a.n_thr && v <= a.thr2[k]) acc[5 + k] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 5 + CMP_MAX_THR; ++k) {
        __syncthreads();  // (the previous quantity's readers are done)
        sh[tid] = acc[k];
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if (tid < o) sh[tid] = k == 4 ? (sh[tid + o] > sh[tid] ? sh[tid + o] : sh[tid]) : sh[tid] + sh[tid + o];
            __syncthreads();
        }
        if (tid == 0) out[k] = sh[0];
    }
}
