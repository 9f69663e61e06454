// score_kernels.h -- sharpness of a voxel map without ground truth (include/ptudes_mi.h ptl_icp_map_score).
//
// Per stored map point q: its neighbours are the stored points p (q included) with (dx dx + dy dy) + dz dz <= radius^2, d = p - q; n of
// them; m = mean of the offsets d; Sigma = (1/n) sum d d^T - m m^T (fp64; offsets from q keep every term <= radius^2); lambda0 <= lambda1 <=
// lambda2 its eigenvalues by cyclic Jacobi with a fixed number of sweeps, clipped below at 0; plane_var = lambda0, entropy = 0.5 (3 ln(2 pi e) +
// sum ln(lambda_i + sigma_floor^2)).  n < min_neighbours: sparse, counted, plane_var = entropy = NaN.
//
// radius <= voxel size: with the truncating voxel index (voxel_index) index 0 spans (-vs, vs), every other index one vs; a point within
// radius of a point of voxel k lies in voxels k - 1 .. k + 1 on each axis, so the 27 probed voxels hold every neighbour - in exact
// arithmetic.  The rounded membership expression admits a pair whose exact distance exceeds the radius by less than one rounding; at radius =
// vs such a pair can sit two voxels apart, and a voxel that holds a point that close to a face probes one voxel further on that axis
// (score_need).
//
// The pass only reads the map.  Four launches on the handle's stream:
//   k_score_count   stored points per chunk of 64 consecutive block ids (one wavefront per chunk, coalesced directory reads)
//   k_score_scan    exclusive prefix of the chunk counts, one workgroup: the output order is the pool order (block id, then slot)
//   k_score_points  one wavefront per workgroup walks chunks; per occupied block (= voxel): key from its first point (vox_key), lanes 0 .. 26
//                   probe the 27 neighbour voxels in (i, j, k) ascending order (map_find / pack_key), their stored points are staged ONCE into
//                   LDS in that order (27 P 24 bytes, dynamic), then lane l and lane l + 32 share point l of the voxel: the first takes the even,
//                   the second the odd staged candidates, each sequentially, and the two partial sums are added once (a + b = b + a: both lanes
//                   hold the same bits).  In the candidate loop the 32 lanes of a half read ONE LDS address (a broadcast, no bank conflict).
//   k_score_reduce  one workgroup: every thread adds its strided share of the per-point values in index order, then a fixed tree in LDS
// A point's result is a function of the stored points of its 27 voxels and their slot order only: no float atomics, nothing depends on a block
// id or on scheduling.  The means depend on the order of the per-point arrays, i.e. on how the build handed out block ids.
#pragma once
#include "icp_kernels.h"

#define SCORE_CHUNK 64        // block ids per chunk = lanes of a wavefront
#define SCORE_SWEEPS 8        // cyclic Jacobi sweeps over the three off-diagonal entries (3 x 3 symmetric: converged to rounding after 4 - 5)
#define SCORE_LDS_LIMIT 64000 // bytes of staging a workgroup may ask for (64 KB; the rest of its 64 KiB stays free for the static words): 27 P 24, P <= 98

struct ScoreArgs {
    double radius;
    double r2;          // radius * radius
    double floor2;      // sigma_floor * sigma_floor
    int min_nb;
    int n_chunks;
    int n_alloc;        // entries of the per-point arrays
    int stage_pts;      // staged points that fit the dynamic LDS (27 P)
    const int* chunk_off;
    double* xyz;        // [n_alloc][3] or null
    int* nb;            // [n_alloc]
    double* pv;         // [n_alloc]
    double* ent;        // [n_alloc]
    int* bad;           // voxels whose own key does not lead back to their block (an inconsistent table): the call fails with PTL_ERR_STATE
};

// Stored points of block b: the directory's count, as the export (k_map_export) reads it.  After the wait for the map stream a per-call map's
// count never exceeds the block's capacity (an insert stores below blk_cap only, and the pass that closes an update writes the clipped count), so
// the clamp changes nothing there; it is the bound the staging relies on.  Should a header ever exceed it, the total differs from the map
// state's and the call returns PTL_ERR_STATE instead of reading past a block.
template <class CT>
__device__ __forceinline__ int score_blk_count(const CT& c, int b) {
    const int cnt = blk_hdr(c, b)[0];
    const int cap = blk_cap(c, b);
    return cnt <= 0 ? 0 : (cnt < cap ? cnt : cap);
}

__global__ __launch_bounds__(256) void k_score_count(Ctx c, int* chunk_cnt) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    int cnt = b < c.pool_cap ? score_blk_count(c, b) : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && b < c.pool_cap) chunk_cnt[b / SCORE_CHUNK] = cnt;
}

// exclusive prefix over n chunk counts, one workgroup of 1024: off[i] = sum of cnt[0 .. i), off[n] = the total
__global__ __launch_bounds__(1024) void k_score_scan(const int* cnt, int n, int* off) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    sh[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    int run = sh[tid] - s;  // exclusive
    for (int i = lo; i < hi; ++i) { off[i] = run; run += cnt[i]; }
    if (tid == 1023) off[n] = sh[1023];
}

// Which voxels beyond the 27 can hold a neighbour of a point with coordinate q in voxel k of one axis: bit 0 = two voxels up, bit 1 = two
// voxels down.  In exact arithmetic none can (the radius argument above); but membership is the ROUNDED expression, and fl(p - q) can come
// out as radius when the exact difference exceeds it by less than one rounding - with radius = vs, q a hair below a voxel face and p on the
// next face but one (0.5 - 1 ulp and 1.0 at vs = 0.5: voxels 0 and 2).  hi2 / lo2: the far face of the adjacent voxel under the truncating
// index (index 0 spans (-vs, vs)).  The margin is generous: a bit set in vain costs probes, never a neighbour.
__device__ __forceinline__ int score_need(double q, int k, double vs, double r) {
    const double hi2 = (k + 1 >= 0 ? (double)(k + 2) : (double)(k + 1)) * vs, lo2 = (k - 1 <= 0 ? (double)(k - 2) : (double)(k - 1)) * vs;
    const double m = 1.0e-14 * ((fabs(q) + fabs(hi2)) + (fabs(lo2) + r));
    return ((hi2 - q) <= r + m ? 1 : 0) | ((q - lo2) <= r + m ? 2 : 0);
}

// eigenvalues of the symmetric 3 x 3 matrix {a00 a01 a02; . a11 a12; . . a22}, ascending, clipped below at 0: cyclic Jacobi, fixed sweeps
__device__ __forceinline__ void score_jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = cs * arp - sn * arq, rq = sn * arp + cs * arq;
    arp = rp; arq = rq;
}
__device__ __forceinline__ void score_eig3(double a00, double a01, double a02, double a11, double a12, double a22, double lam[3]) {
    for (int sweep = 0; sweep < SCORE_SWEEPS; ++sweep) {
        score_jacobi_rot(a00, a11, a01, a02, a12);  // (p, q) = (0, 1), r = 2
        score_jacobi_rot(a00, a22, a02, a01, a12);  // (0, 2), r = 1
        score_jacobi_rot(a11, a22, a12, a01, a02);  // (1, 2), r = 0
    }
    double l0 = a00, l1 = a11, l2 = a22, t;
    if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
    if (l1 > l2) { t = l1; l1 = l2; l2 = t; }
    if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
    lam[0] = l0 > 0.0 ? l0 : 0.0; lam[1] = l1 > 0.0 ? l1 : 0.0; lam[2] = l2 > 0.0 ? l2 : 0.0;
}

__global__ __launch_bounds__(64) void k_score_points(Ctx c, ScoreArgs a) {
    extern __shared__ double stage[];  // [stage_pts][3]: the stored points of the 27 voxels, (i, j, k) ascending, slot order
    __shared__ int s_cnt[SCORE_CHUNK], s_off[SCORE_CHUNK];
    __shared__ int v_blk[27], v_cnt[27], v_off[28];
    const int lane = threadIdx.x;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int ch = blockIdx.x; ch < a.n_chunks; ch += gridDim.x) {
        const int b0 = ch * SCORE_CHUNK;
        __syncthreads();  // (the previous chunk's readers of s_cnt / s_off are done)
        s_cnt[lane] = b0 + lane < c.pool_cap ? score_blk_count(c, b0 + lane) : 0;
        __syncthreads();
        if (lane == 0) {
            int run = a.chunk_off[ch];
            for (int i = 0; i < SCORE_CHUNK; ++i) { s_off[i] = run; run += s_cnt[i]; }
        }
        __syncthreads();
        for (int bi = 0; bi < SCORE_CHUNK; ++bi) {
            const int cnt = s_cnt[bi];
            if (cnt == 0) continue;  // (uniform: every lane reads the same word)
            const int b = b0 + bi, out0 = s_off[bi];
            const double* X = blk_x(c, b);
            unsigned long long key; int kx, ky, kz;
            vox_key(v3(X[0], X[1], X[2]), c.vs, key, kx, ky, kz);
            __syncthreads();  // (the previous voxel's readers of the stage and of v_* are done)
            if (lane < 27) {
                const int vx = kx + lane / 9 - 1, vy = ky + (lane / 3) % 3 - 1, vz = kz + lane % 3 - 1;
                const bool in_range = ((unsigned)(vx + KEY_OFF) | (unsigned)(vy + KEY_OFF) | (unsigned)(vz + KEY_OFF)) < (1u << 21);
                const int pb = in_range ? map_find(c, pack_key(vx, vy, vz)) : -1;
                const int nb_blk = pb < 0 ? -1 : (pb & BLK_ID_MASK);
                v_blk[lane] = nb_blk;
                v_cnt[lane] = nb_blk < 0 || nb_blk >= c.pool_cap ? 0 : score_blk_count(c, nb_blk);
            }
            __syncthreads();
            if (lane == 0) {
                int run = 0;
                for (int v = 0; v < 27; ++v) {
                    v_off[v] = run;
                    run += v_cnt[v];
                    if (run > a.stage_pts) { v_cnt[v] -= run - a.stage_pts; run = a.stage_pts; }  // (cannot happen: every count <= P)
                }
                v_off[27] = run;
            }
            __syncthreads();
            for (int v = 0; v < 27; ++v) {
                const int vc = v_cnt[v];
                if (vc == 0) continue;
                const double* Y = blk_x(c, v_blk[v]);
                double* dst = stage + 3 * (size_t)v_off[v];
                for (int l = lane; l < 3 * vc; l += 64) dst[l] = Y[l];
            }
            __syncthreads();
            if (v_blk[13] != b) {  // (uniform) never on a consistent map: reported, and the points leave as unscored instead of staying unwritten
                if (lane == 0) atomicAdd(a.bad, 1);
                for (int pt = lane; pt < cnt; pt += 64) {
                    const int o = out0 + pt;
                    if (o >= a.n_alloc) continue;
                    a.nb[o] = 0; a.pv[o] = nan; a.ent[o] = nan;
                    if (a.xyz) { a.xyz[3 * (size_t)o] = X[3 * pt]; a.xyz[3 * (size_t)o + 1] = X[3 * pt + 1]; a.xyz[3 * (size_t)o + 2] = X[3 * pt + 2]; }
                }
                continue;
            }
            const int total = v_off[27], half = lane >> 5;
            const int own = v_off[13];  // the voxel itself is the 14th of the 27
            // voxels two steps away on an axis where a point of this voxel sits within rounding of the far face of the adjacent voxel (score_need)
            int need = 0;
            for (int pt = lane; pt < cnt; pt += 64)
                need |= score_need(stage[3 * (own + pt)], kx, c.vs, a.radius) | score_need(stage[3 * (own + pt) + 1], ky, c.vs, a.radius) << 2 |
                        score_need(stage[3 * (own + pt) + 2], kz, c.vs, a.radius) << 4;
            for (int o = 32; o > 0; o >>= 1) need |= __shfl_xor(need, o);
            for (int base = 0; base < cnt; base += 32) {
                const int pt = base + (lane & 31);
                const bool act = pt < cnt;
                double qx = 0.0, qy = 0.0, qz = 0.0;
                if (act) { qx = stage[3 * (own + pt)]; qy = stage[3 * (own + pt) + 1]; qz = stage[3 * (own + pt) + 2]; }
                int n = 0;
                double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
                for (int j = half; j < total; j += 2) {
                    const double dx = stage[3 * j] - qx, dy = stage[3 * j + 1] - qy, dz = stage[3 * j + 2] - qz;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= a.r2) {
                        n += 1;
                        sx += dx; sy += dy; sz += dz;
                        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
                    }
                }
                n += __shfl_xor(n, 32);
                sx += __shfl_xor(sx, 32); sy += __shfl_xor(sy, 32); sz += __shfl_xor(sz, 32);
                sxx += __shfl_xor(sxx, 32); sxy += __shfl_xor(sxy, 32); sxz += __shfl_xor(sxz, 32);
                syy += __shfl_xor(syy, 32); syz += __shfl_xor(syz, 32); szz += __shfl_xor(szz, 32);
                if (need) {
                    // rare: the voxels beyond the 27, (i, j, k) ascending, straight from the pool, every lane for its own point; both lanes of a
                    // point add the same terms to the same totals
                    for (int ex = -1 - ((need >> 1) & 1); ex <= 1 + (need & 1); ++ex)
                        for (int ey = -1 - ((need >> 3) & 1); ey <= 1 + ((need >> 2) & 1); ++ey)
                            for (int ez = -1 - ((need >> 5) & 1); ez <= 1 + ((need >> 4) & 1); ++ez) {
                                if (ex >= -1 && ex <= 1 && ey >= -1 && ey <= 1 && ez >= -1 && ez <= 1) continue;
                                const int vx = kx + ex, vy = ky + ey, vz = kz + ez;
                                if ((((unsigned)(vx + KEY_OFF) | (unsigned)(vy + KEY_OFF) | (unsigned)(vz + KEY_OFF)) >> 21) != 0u) continue;
                                const int pb = map_find(c, pack_key(vx, vy, vz));
                                const int eb = pb < 0 ? -1 : (pb & BLK_ID_MASK);
                                const int ec = eb < 0 || eb >= c.pool_cap ? 0 : score_blk_count(c, eb);
                                const double* Y = ec > 0 ? blk_x(c, eb) : nullptr;
                                for (int j = 0; j < ec; ++j) {
                                    const double dx = Y[3 * j] - qx, dy = Y[3 * j + 1] - qy, dz = Y[3 * j + 2] - qz;
                                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                                    if (d2 <= a.r2) {
                                        n += 1;
                                        sx += dx; sy += dy; sz += dz;
                                        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
                                    }
                                }
                            }
                }
                if (!act || half != 0) continue;
                const int o = out0 + pt;
                if (o >= a.n_alloc) continue;
                double pvar = nan, entropy = nan;
                if (n >= a.min_nb && n > 0) {
                    const double inv = 1.0 / (double)n;
                    const double mx = sx * inv, my = sy * inv, mz = sz * inv;
                    double lam[3];
                    score_eig3(sxx * inv - mx * mx, sxy * inv - mx * my, sxz * inv - mx * mz, syy * inv - my * my, syz * inv - my * mz,
                               szz * inv - mz * mz, lam);
                    pvar = lam[0];
                    entropy = 0.5 * (3.0 * 2.8378770664093453 + ((log(lam[0] + a.floor2) + log(lam[1] + a.floor2)) + log(lam[2] + a.floor2)));
                }
                a.nb[o] = n; a.pv[o] = pvar; a.ent[o] = entropy;
                if (a.xyz) { a.xyz[3 * (size_t)o] = qx; a.xyz[3 * (size_t)o + 1] = qy; a.xyz[3 * (size_t)o + 2] = qz; }
            }
        }
    }
}

// out[0] = scored points, out[1] = sum of their plane_var, out[2] = sum of their entropy, out[3] = sum of n over ALL points (exact: integers
// below 2^53).  One workgroup; thread t adds entries t, t + 1024, ... in that order, then a fixed tree.
__global__ __launch_bounds__(1024) void k_score_reduce(const int* nb, const double* pv, const double* ent, int n, int min_nb, double* out) {
    __shared__ double sh[4][1024];
    const int tid = threadIdx.x;
    double cnt = 0.0, spv = 0.0, sent = 0.0, snb = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const int k = nb[i];
        snb += (double)k;
        if (k >= min_nb) { cnt += 1.0; spv += pv[i]; sent += ent[i]; }
    }
    sh[0][tid] = cnt; sh[1][tid] = spv; sh[2][tid] = sent; sh[3][tid] = snb;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; sh[2][tid] += sh[2][tid + o]; sh[3][tid] += sh[3][tid + o]; }
        __syncthreads();
    }
    if (tid < 4) out[tid] = sh[tid][0];
}
