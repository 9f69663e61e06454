// place_kernels.h -- revisited places: polar height descriptors of sweeps and their comparison at every heading (include/ptudes_mi.h
// ptl_place_*).  The definition - tables, binning, level, layout, distance, tie rules - is in the header and is not restated
// here.  Past the binning comparisons everything is an integer: a descriptor is a maximum per cell and a match a sum of absolute differences
// of bytes, so neither depends on the lane mapping or the launch geometry.  All fp64 arithmetic in the written order (-ffp-contract=off).
//
//   k_place_bin    grid stride over the points of one sweep.  A workgroup keeps the S Rpad cells as u32 in LDS (at most 16 KB) together with
//                  both tables, fills them with an LDS atomic maximum and flushes its NON-ZERO cells to the global u32 grid with an atomic
//                  maximum whose result is unused.  The sector is found by walking j = 0 .. S - 1 over the table as the definition words it
//                  (the first j with c_j >= 0 && c_(j+1) < 0): 3 fp64 operations per step, 64 steps at most, and no shortcut to prove.
//                  The six counters are summed over the wavefront before one atomic each.
//   k_place_pack   one workgroup: the u32 grid to the u8 query slot (pad bytes are cells nobody writes: 0), n_cells and sum_levels with the
//                  counters into the slot's info.
//   k_place_match  one query against the entries [first, last].  The query lies DOUBLED along the sector axis in LDS, its column stride
//                  RDP = Rpad / 4 | 1 dwords: lane s (its shift) reads dword (s + j) RDP + w for the entry's dword j Rpad / 4 + w, so a shift
//                  is an offset of whole columns and - RDP odd - the 32 lanes of an LDS access hit 32 banks (5 dwords at R = 20).  The entry's
//                  dwords are uniform over the wavefront; a wavefront takes PLACE_TILE entries at a time, so that one LDS read feeds
//                  PLACE_TILE v_sad_u8.  The minimum over lanes is taken on the packed key dist << 6 | shift (dist < 2^20), the best entry on
//                  dist << 26 | entry << 6 | shift with one 64-bit atomic minimum per wavefront.
//   k_place_match_all  a wavefront per QUERY i, the four queries of a workgroup doubled in LDS side by side; every wavefront walks the entries
//                  j <= i - min_gap in the same tiles, so the four queries of a workgroup read the same entry dwords one after the other and
//                  three of the four reads are cache hits.  The running minimum is the 64-bit key above, kept in a register: no atomics.
// Lanes at and above S compute shift 0 again and are masked out of the minimum.  Every loop is bounded by a count; no workgroup waits for
// another.  Results are written with ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLACE_THREADS 256
#define PLACE_MAX_BLOCKS 1024
#define PLACE_TILE 4            // entries per wavefront and pass of the match
#define PLACE_MAX_RING 64
#define PLACE_MAX_SECTOR 64
// slots of the 64-bit counters of a describe
#define PLACE_N_NORET 0
#define PLACE_N_NONFINITE 1
#define PLACE_N_RADIUS 2
#define PLACE_N_NOSECTOR 3
#define PLACE_N_BELOW 4
#define PLACE_N_USED 5
#define PLACE_COUNTERS 8
#define PLACE_KEY_NONE 0xffffffffffffffffull

// what the device writes beside a descriptor: ptl_place_info's layout (checked on the host against the header's struct)
struct PlaceInfoDev {
    long long n_points, n_no_return, n_non_finite, n_out_of_radius, n_no_sector, n_below, n_used, n_cells, sum_levels;
};

struct PlaceArgs {
    int R, S, Rpad;
    double z_min, z_step;
    const double* ring_edge2;   // [R + 1]
    const double* sector_dir;   // [2 S]
    double rot[9];
    int has_rot;
    unsigned* grid;             // [S Rpad] u32 cells
    unsigned long long* counts; // [PLACE_COUNTERS]
};

// MODE 0: u32 ranges through the LUT; 1: f32 xyz; 2: f64 xyz
template <int MODE>
__global__ __launch_bounds__(PLACE_THREADS) void k_place_bin(const void* raw, const double* dir, const double* off, long long n, PlaceArgs a) {
    __shared__ unsigned cells[PLACE_MAX_SECTOR * PLACE_MAX_RING];
    __shared__ double edge2[PLACE_MAX_RING + 1];
    __shared__ double sdir[2 * PLACE_MAX_SECTOR];
    const int n_cells = a.S * a.Rpad;
    for (int i = threadIdx.x; i < n_cells; i += PLACE_THREADS) cells[i] = 0u;
    for (int i = threadIdx.x; i <= a.R; i += PLACE_THREADS) edge2[i] = a.ring_edge2[i];
    for (int i = threadIdx.x; i < 2 * a.S; i += PLACE_THREADS) sdir[i] = a.sector_dir[i];
    __syncthreads();
    int n_noret = 0, n_nonfinite = 0, n_radius = 0, n_nosector = 0, n_below = 0, n_used = 0;
    for (long long q = (long long)blockIdx.x * PLACE_THREADS + threadIdx.x; q < n; q += (long long)gridDim.x * PLACE_THREADS) {
        double x, y, z;
        bool ret;
        if constexpr (MODE == 0) {
            const unsigned rg = ((const unsigned*)raw)[q];
            const double r = (double)rg;
            ret = rg != 0u;
            x = r * dir[3 * q] + off[3 * q]; y = r * dir[3 * q + 1] + off[3 * q + 1]; z = r * dir[3 * q + 2] + off[3 * q + 2];
        } else if constexpr (MODE == 1) {
            const float* p = (const float*)raw + 3 * q;
            x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
            ret = !(x == 0.0 && y == 0.0 && z == 0.0);
        } else {
            const double* p = (const double*)raw + 3 * q;
            x = p[0]; y = p[1]; z = p[2];
            ret = !(x == 0.0 && y == 0.0 && z == 0.0);
        }
        if (!ret) { n_noret += 1; continue; }
        if (!(fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308 && fabs(z) <= 1.7976931348623157e308)) { n_nonfinite += 1; continue; }
        if (a.has_rot) {
            const double lx = (a.rot[0] * x + a.rot[1] * y) + a.rot[2] * z;
            const double ly = (a.rot[3] * x + a.rot[4] * y) + a.rot[5] * z;
            const double lz = (a.rot[6] * x + a.rot[7] * y) + a.rot[8] * z;
            x = lx; y = ly; z = lz;
        }
        const double rho2 = x * x + y * y;
        if (!(edge2[0] <= rho2 && rho2 < edge2[a.R])) { n_radius += 1; continue; }
        int ring = 0;
        for (int i = 1; i < a.R; ++i) ring = edge2[i] <= rho2 ? i : ring;
        int sector = -1;
        double c = sdir[0] * y - sdir[1] * x;
        for (int j = 0; j < a.S; ++j) {
            const int jn = j + 1 < a.S ? j + 1 : 0;
            const double cn = sdir[2 * jn] * y - sdir[2 * jn + 1] * x;
            if (sector < 0 && c >= 0.0 && cn < 0.0) sector = j;
            c = cn;
        }
        if (sector < 0) { n_nosector += 1; continue; }
        const double h = (z - a.z_min) / a.z_step;
        if (!(h >= 0.0)) { n_below += 1; continue; }
        const unsigned level = h >= 254.0 ? 255u : 1u + (unsigned)(int)h;
        n_used += 1;
        atomicMax(&cells[sector * a.Rpad + ring], level);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_cells; i += PLACE_THREADS) {
        const unsigned v = cells[i];
        if (v) atomicMax(&a.grid[i], v);
    }
    for (int s = 32; s > 0; s >>= 1) {
        n_noret += __shfl_xor(n_noret, s); n_nonfinite += __shfl_xor(n_nonfinite, s); n_radius += __shfl_xor(n_radius, s);
        n_nosector += __shfl_xor(n_nosector, s); n_below += __shfl_xor(n_below, s); n_used += __shfl_xor(n_used, s);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_noret) atomicAdd(&a.counts[PLACE_N_NORET], (unsigned long long)n_noret);
        if (n_nonfinite) atomicAdd(&a.counts[PLACE_N_NONFINITE], (unsigned long long)n_nonfinite);
        if (n_radius) atomicAdd(&a.counts[PLACE_N_RADIUS], (unsigned long long)n_radius);
        if (n_nosector) atomicAdd(&a.counts[PLACE_N_NOSECTOR], (unsigned long long)n_nosector);
        if (n_below) atomicAdd(&a.counts[PLACE_N_BELOW], (unsigned long long)n_below);
        if (n_used) atomicAdd(&a.counts[PLACE_N_USED], (unsigned long long)n_used);
    }
}

// one workgroup; desc: the query slot's S Rpad bytes, info: its info
__global__ __launch_bounds__(PLACE_THREADS) void k_place_pack(const unsigned* grid, const unsigned long long* counts, int n_cells, long long n_points,
                                                              unsigned char* desc, PlaceInfoDev* info) {
    __shared__ unsigned long long part[2 * (PLACE_THREADS / 64)];
    unsigned long long nz = 0, sum = 0;
    for (int i = threadIdx.x; i < n_cells; i += PLACE_THREADS) {
        const unsigned v = grid[i];
        desc[i] = (unsigned char)v;
        nz += v ? 1 : 0; sum += v;
    }
    for (int s = 32; s > 0; s >>= 1) { nz += __shfl_xor(nz, s); sum += __shfl_xor(sum, s); }
    if ((threadIdx.x & 63) == 0) { part[2 * (threadIdx.x >> 6)] = nz; part[2 * (threadIdx.x >> 6) + 1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        nz = 0; sum = 0;
        for (int w = 0; w < PLACE_THREADS / 64; ++w) { nz += part[2 * w]; sum += part[2 * w + 1]; }
        info->n_points = n_points;
        info->n_no_return = (long long)counts[PLACE_N_NORET]; info->n_non_finite = (long long)counts[PLACE_N_NONFINITE];
        info->n_out_of_radius = (long long)counts[PLACE_N_RADIUS]; info->n_no_sector = (long long)counts[PLACE_N_NOSECTOR];
        info->n_below = (long long)counts[PLACE_N_BELOW]; info->n_used = (long long)counts[PLACE_N_USED];
        info->n_cells = (long long)nz; info->sum_levels = (long long)sum;
    }
}

// a query of S columns of RD dwords, doubled along the sector axis into LDS with the column stride RDP
__device__ __forceinline__ void place_stage_query(unsigned* qq, const unsigned* q, int S, int RD, int RDP, int tid, int threads) {
    for (int i = tid; i < 2 * S * RD; i += threads) {
        const int col = i / RD, w = i - col * RD;
        qq[col * RDP + w] = q[(col < S ? col : col - S) * RD + w];
    }
}

// the packed keys dist << 6 | shift of PLACE_TILE entries against the staged query, the minimum over the wavefront's lanes in every lane;
// e[t]: the entries' dwords, uniform over the wavefront
template <int RDC>
__device__ __forceinline__ void place_tile_keys(const unsigned* qq, const unsigned* (&e)[PLACE_TILE], int S, int RD_, int lane,
                                                unsigned (&key)[PLACE_TILE]) {
    const int RD = RDC ? RDC : RD_, RDP = RD | 1;
    const int sl = lane < S ? lane : 0;
    unsigned acc[PLACE_TILE];
    for (int t = 0; t < PLACE_TILE; ++t) acc[t] = 0u;
    const unsigned* ql = qq + sl * RDP;
    for (int j = 0; j < S; ++j) {
#pragma unroll
        for (int w = 0; w < RD; ++w) {
            const unsigned qd = ql[j * RDP + w];
#pragma unroll
            for (int t = 0; t < PLACE_TILE; ++t) acc[t] = __builtin_amdgcn_sad_u8(qd, e[t][j * RD + w], acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < PLACE_TILE; ++t) {
        unsigned k = lane < S ? (acc[t] << 6 | (unsigned)lane) : 0xffffffffu;
        for (int s = 32; s > 0; s >>= 1) { const unsigned o = __shfl_xor(k, s); k = o < k ? o : k; }
        key[t] = k;
    }
}

// RDC: Rpad / 4 as a compile-time constant (5: the default R = 20, whose inner loop unrolls), or 0 for any other, read from RD.
// desc: the entries' dwords, ED = S RD each; q: the query's dwords.  dist / shift: [last - first + 1]; best: one 64-bit key, preset to
// PLACE_KEY_NONE.  Dynamic LDS: 2 S RDP dwords
template <int RDC>
__global__ __launch_bounds__(PLACE_THREADS) void k_place_match(const unsigned* __restrict__ desc, const unsigned* __restrict__ q, int S, int RD,
                                                               int first, int last, unsigned* __restrict__ dist, int* __restrict__ shift,
                                                               unsigned long long* best) {
    extern __shared__ __attribute__((aligned(16))) unsigned place_lds[];
    const int RDP = RD | 1, ED = S * RD;
    place_stage_query(place_lds, q, S, RD, RDP, threadIdx.x, PLACE_THREADS);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (PLACE_THREADS / 64) + (threadIdx.x >> 6)), waves = gridDim.x * (PLACE_THREADS / 64);
    unsigned long long mine = PLACE_KEY_NONE;
    for (long long c0 = (long long)first + (long long)PLACE_TILE * wave; c0 <= last; c0 += (long long)PLACE_TILE * waves) {
        const unsigned* e[PLACE_TILE];
        for (int t = 0; t < PLACE_TILE; ++t) { const long long c = c0 + t <= last ? c0 + t : last; e[t] = desc + (size_t)c * ED; }
        unsigned key[PLACE_TILE];
        place_tile_keys<RDC>(place_lds, e, S, RD, lane, key);
        for (int t = 0; t < PLACE_TILE; ++t) {
            const long long c = c0 + t;
            if (c > last) break;
            if (lane == 0) { dist[c - first] = key[t] >> 6; shift[c - first] = (int)(key[t] & 63u); }
            const unsigned long long k = (unsigned long long)(key[t] >> 6) << 26 | (unsigned long long)c << 6 | (key[t] & 63u);
            mine = k < mine ? k : mine;
        }
    }
    if (lane == 0 && mine != PLACE_KEY_NONE) atomicMin(best, mine);
}

// queries [q_first, q_last], a wavefront each; entry / dist / shift: [q_last - q_first + 1].  Dynamic LDS: 4 x 2 S RDP dwords
template <int RDC>
__global__ __launch_bounds__(PLACE_THREADS) void k_place_match_all(const unsigned* __restrict__ desc, int S, int RD, int q_first, int q_last,
                                                                   int min_gap, int* __restrict__ entry, unsigned* __restrict__ dist,
                                                                   int* __restrict__ shift, unsigned long long* best) {
    extern __shared__ __attribute__((aligned(16))) unsigned place_lds[];
    const int RDP = RD | 1, ED = S * RD;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long i = (long long)q_first + (long long)blockIdx.x * (PLACE_THREADS / 64) + w;  // this wavefront's query
    unsigned* qq = place_lds + (size_t)w * 2 * S * RDP;
    place_stage_query(qq, desc + (size_t)(i <= q_last ? i : q_last) * ED, S, RD, RDP, lane, 64);
    __syncthreads();
    if (i > q_last) return;
    const long long j_last = i - min_gap;
    unsigned long long mine = PLACE_KEY_NONE;
    for (long long c0 = 0; c0 <= j_last; c0 += PLACE_TILE) {
        const unsigned* e[PLACE_TILE];
        for (int t = 0; t < PLACE_TILE; ++t) { const long long c = c0 + t <= j_last ? c0 + t : j_last; e[t] = desc + (size_t)c * ED; }
        unsigned key[PLACE_TILE];
        place_tile_keys<RDC>(qq, e, S, RD, lane, key);
        for (int t = 0; t < PLACE_TILE; ++t) {
            const long long c = c0 + t;
            if (c > j_last) break;
            const unsigned long long k = (unsigned long long)(key[t] >> 6) << 26 | (unsigned long long)c << 6 | (key[t] & 63u);
            mine = k < mine ? k : mine;
        }
    }
    if (lane == 0) {
        const bool any = mine != PLACE_KEY_NONE;
        entry[i - q_first] = any ? (int)((mine >> 6) & 0xfffffu) : -1;
        dist[i - q_first] = any ? (unsigned)(mine >> 26) : 0u;
        shift[i - q_first] = any ? (int)(mine & 63u) : 0;
        // the best pair of the call: dist, then the entry, then the query (the host takes the pair's shift from shift[])
        if (any) atomicMin(best, (mine >> 6) << 20 | (unsigned long long)(i - q_first));
    }
}
