// grid_kernels.h -- the occupancy grid of a run: free, occupied and unknown cells of a top-down 2-D grid (include/ptudes_mi.h ptl_grid_*,
// DESIGN.md 3.29).  A pass over the sweeps of a run, posed by its trajectory; per CELL it counts the rays that crossed the cell on their way
// (free) and the rays that ended in it (hit).  It needs no map: the evidence is the rays themselves.  Every output is an integer and sums of
// integers have no order: free and hit are an exact function of the SET of rays and the parameters - not of the lane mapping, the launch
// geometry or the order of the sweeps.
//
// Parameters: cell > 0; x0, y0 the world coordinates of the corner of cell (0, 0); nx, ny >= 1 with nx ny <= 2^26; z_lo <= z_hi, the height
// band RELATIVE TO THE RAY'S OWN ORIGIN; margin >= 0; 0 < step <= cell; min_range >= 0, max_range > min_range with max_range / step <= 65536.
// The defaults (step = cell / 2, margin = cell, min_range = 0, max_range = 600 cell, band [-0.5, +0.5] m; the bounds have none) are a caller's
// choice that the result echoes back, not tuned values: nobody has run this on a real recording.
// All arithmetic fp64 in the written order, no contraction (-ffp-contract=off).
//
//   ray      carve's ray (carve_kernels.h), called and not restated: a pixel with a return; its end w = d_pose_pixel(column entry,
//            d_fly_pixel(pixel)) of fly_kernels.h, its origin o the translation of its own column's pose (entries 9 .. 11 of the column
//            table); d = w - o, len2 = (dx dx + dy dy) + dz dz, len = sqrt(len2).  Used iff min_range <= len <= max_range, else counted in
//            n_rays_out_of_range; a pixel without a return is counted in n_no_return.  A sweep with any column outside the trajectory's bounds
//            is skipped as a whole and counted (k_fly_coltab's flag, as it is).
//   samples  k = 0, 1, ... while t_k = ((double)k + 0.5) step < len: a_k = t_k / len, s_k[c] = o[c] + a_k d[c].  A sample is a FREE sample iff
//            also t_k <= len - margin (t_k grows with k: the free samples are the first ones).
//   cell     of a point p: fx = (p.x - x0) / cell, fy = (p.y - y0) / cell; p is in the grid iff fx >= 0 && fx < (double)nx && fy >= 0 &&
//            fy < (double)ny, compared in fp64 BEFORE any integer conversion (a NaN fails it); then ix = (int)fx, iy = (int)fy.  p is in the
//            band iff z_lo <= p.z - o.z && p.z - o.z <= z_hi.
//   runs     consecutive free samples with the same cell state - "outside the grid" or the pair (ix, iy) - form a run.  The rule is run-based,
//            as carve's "consecutive samples with one key visit the voxel once"; it does not rest on monotonicity.
//   votes    of one used ray: if w is in the grid and in the band, hit[cell(w)] += 1.  Every run whose cell is in the grid and which has at
//            least one sample in the band gives free[cell] += 1 - except the LAST run when its cell equals cell(w) and the ray scored a hit
//            there.  A ray adds at most 1 to any counter of a cell per run.
// The counters are u32: the host refuses an add that could carry the number of used rays past 2^32 - 1, so none can wrap.  Which cells count
// as occupied is host policy (the Python layer's GridCounts.classify), not the library's.
//
// Lane mapping: ONE LANE PER RAY, the mapping DESIGN.md 3.24 measured 3.4 times ahead of a half-wave per ray: a ray march is bound by
// instruction issue.  Pixel q goes to lane q of consecutive wavefronts: a wavefront holds 64 neighbouring COLUMNS of one beam, whose azimuths
// differ - not 64 beams of one azimuth, which would all vote for the same cells.  The lane walks its samples, keeps the current run's cell and
// its "any sample in band" flag, and votes on a change of cell; after the loop it settles the last run against the end's cell and votes the
// hit.  Every loop is bounded by the sample limit or the pixel count; no workgroup waits for another.
// The vote: the wavefront MERGES equal cells across its lanes before the atomic (GRID_MERGE=1, the default): a ballot of the voting lanes, the
// first of them broadcasts its cell, the lanes with that cell drop out and their leader issues ONE atomicAdd(&free[iy nx + ix], count) whose
// result is unused (a no-return global atomic); rounds until no voter is left, at most 64.  The sample loop is then uniform over the
// wavefront (it ends when no lane has a free sample left).  make EXTRA=-DGRID_MERGE=0 builds the plain form of the same definition - every
// lane its own atomicAdd(.., 1u) - for the measurement of tools/occupancy_grid_cost.py: on the MI355X the plain form took 2.6 times as long,
// because half of all votes of a sweep go to the 1 % of cells next to the sensor, which every ray crosses.
//
//   k_grid_rays     one launch per sweep behind k_fly_coltab (fly_kernels.h, as it is); at most GRID_MAX_BLOCKS workgroups, grid stride beyond
//   k_grid_reduce   the summary of the two count arrays inside ptl_grid_read: cells with free > 0, cells with hit > 0, both sums, the touched
//                   bounding box (integers only)
// Nothing here reads or writes a map.
#pragma once
#include "icp_kernels.h"
#include "fly_kernels.h"

#ifndef GRID_MERGE
#define GRID_MERGE 1          // 1: a wavefront merges equal cells before the atomic (the product); 0: every lane issues its own atomic
#endif
#define GRID_THREADS 256
#define GRID_MAX_BLOCKS 1024   // workgroups of a k_grid_rays launch (grid stride beyond): 262 144 lanes, which a test's sweep passes
#define GRID_MAX_SAMPLES 65536 // max_range / step
#define GRID_MAX_CELLS (1 << 26)
// slots of the 64-bit counters
#define GRID_N_RAYS 0
#define GRID_N_OOR 1
#define GRID_N_NORET 2
#define GRID_N_RUNS 3
#define GRID_N_ENDS_OUT 4
#define GRID_N_SCANS 5
#define GRID_N_SKIPPED 6
#define GRID_COUNTERS 8
// k_grid_reduce: four 64-bit sums behind the counters, and the box (ix0, iy0, ix1, iy1) as four ints the host presets to (max, max, -1, -1)
#define GRID_SUMS 4

struct GridArgs {
    double cell, x0, y0, z_lo, z_hi, margin, step, min_range, max_range;
    int nx, ny;
    unsigned* free;              // [ny][nx]
    unsigned* hit;               // [ny][nx]
    unsigned long long* counts;  // [GRID_COUNTERS]
};

// the cell of a point: its index iy nx + ix, or -1 outside the grid
__device__ __forceinline__ int grid_cell(const GridArgs& a, double px, double py) {
    const double fx = (px - a.x0) / a.cell, fy = (py - a.y0) / a.cell;
    if (!(fx >= 0.0 && fx < (double)a.nx && fy >= 0.0 && fy < (double)a.ny)) return -1;
    return (int)fy * a.nx + (int)fx;
}

// one vote per lane with `vote`; MERGE: every lane of the wavefront gets here, the lanes with one cell send one add of their number
template <bool MERGE>
__device__ __forceinline__ void grid_vote(unsigned* arr, bool vote, int idx) {
    if constexpr (MERGE) {
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(vote ? 1 : 0);
        for (int round = 0; round < 64 && todo; ++round) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int want = __shfl(idx, leader);
            const unsigned long long same = __ballot((vote && idx == want) ? 1 : 0);
            if (lane == leader) atomicAdd(&arr[want], (unsigned)__popcll(same));
            todo &= ~same;
        }
    } else {
        if (vote) atomicAdd(&arr[idx], 1u);
    }
}

// one launch per sweep, behind k_fly_coltab on the same stream; raw as d_fly_pixel reads it
template <bool RANGE>
__global__ __launch_bounds__(GRID_THREADS) void k_grid_rays(const void* raw, const double* dir, const double* off, int n, int W,
                                                            const double* coltab, const FlyWs* ws, GridArgs a) {
    if (ws->outside) {  // (the whole sweep is skipped)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[GRID_N_SKIPPED], 1ull);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counts[GRID_N_SCANS], 1ull);
    constexpr bool MERGE = GRID_MERGE != 0;
    const int lane = threadIdx.x & 63;
    const long long lanes = (long long)gridDim.x * GRID_THREADS;
    int n_rays = 0, n_oor = 0, n_noret = 0, n_ends_out = 0;
    long long n_runs = 0;
    // (base is uniform over the wavefront: with MERGE every lane stays in the loops until the wavefront is done)
    for (long long base = (long long)blockIdx.x * GRID_THREADS + (threadIdx.x & ~63); base < n; base += lanes) {
        const long long q = base + lane;
        bool use = false;
        double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, len = 0.0;
        if (q < n) {
            double p[3], M[12];
            const bool ret = d_fly_pixel<RANGE>(raw, dir, off, (int)q, p);
            const double* m = coltab + (size_t)(q % W);
            for (int e = 0; e < 12; ++e) M[e] = m[(size_t)e * W];
            d_pose_pixel(M, p, w);
            for (int e = 0; e < 3; ++e) { o[e] = M[9 + e]; d[e] = w[e] - o[e]; }
            const double len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            len = sqrt(len2);
            use = ret && len >= a.min_range && len <= a.max_range;
            if (!ret) n_noret += 1;
            else if (!use) n_oor += 1;
            else n_rays += 1;
        }
        const double t_free = len - a.margin;
        bool have = false, cur_band = false;
        int cur = -1;  // the current run's cell, -1 = outside the grid
        for (int k = 0; k <= GRID_MAX_SAMPLES; ++k) {
            const double tk = ((double)k + 0.5) * a.step;
            const bool in_k = use && tk < len && tk <= t_free;
            if (MERGE ? !__any(in_k ? 1 : 0) : !in_k) break;
            bool flush = false;
            int fidx = 0;
            if (in_k) {
                const double ak = tk / len;
                const double sx = o[0] + ak * d[0], sy = o[1] + ak * d[1], sz = o[2] + ak * d[2];
                const int idx = grid_cell(a, sx, sy);
                const double dz = sz - o[2];
                const bool band = a.z_lo <= dz && dz <= a.z_hi;
                if (!(have && idx == cur)) {
                    flush = have && cur >= 0 && cur_band;
                    fidx = cur;
                    cur = idx; cur_band = false; have = true;
                }
                cur_band = cur_band || band;
            }
            n_runs += flush ? 1 : 0;
            grid_vote<MERGE>(a.free, flush, fidx);
        }
        // the end, and the last run against it
        const int widx = use ? grid_cell(a, w[0], w[1]) : -1;
        const double wz = w[2] - o[2];
        const bool hit = use && widx >= 0 && a.z_lo <= wz && wz <= a.z_hi;
        const bool last = use && have && cur >= 0 && cur_band && !(hit && cur == widx);
        n_ends_out += (use && widx < 0) ? 1 : 0;
        n_runs += last ? 1 : 0;
        grid_vote<MERGE>(a.free, last, cur);
        grid_vote<MERGE>(a.hit, hit, widx);
    }
    for (int s = 32; s > 0; s >>= 1) {
        n_rays += __shfl_xor(n_rays, s); n_oor += __shfl_xor(n_oor, s); n_noret += __shfl_xor(n_noret, s); n_ends_out += __shfl_xor(n_ends_out, s);
        n_runs += __shfl_xor(n_runs, s);
    }
    if (lane == 0) {
        if (n_rays) atomicAdd(&a.counts[GRID_N_RAYS], (unsigned long long)n_rays);
        if (n_oor) atomicAdd(&a.counts[GRID_N_OOR], (unsigned long long)n_oor);
        if (n_noret) atomicAdd(&a.counts[GRID_N_NORET], (unsigned long long)n_noret);
        if (n_ends_out) atomicAdd(&a.counts[GRID_N_ENDS_OUT], (unsigned long long)n_ends_out);
        if (n_runs) atomicAdd(&a.counts[GRID_N_RUNS], (unsigned long long)n_runs);
    }
}

// sums[0] = cells with free > 0, sums[1] = cells with hit > 0, sums[2] = sum of free, sums[3] = sum of hit; box = (min ix, min iy, max ix,
// max iy) over the cells with any count, preset by the host to (INT_MAX, INT_MAX, -1, -1): an empty box stays that way.  Integers only.
__global__ __launch_bounds__(256) void k_grid_reduce(const unsigned* free, const unsigned* hit, int nx, int n_cells, unsigned long long* sums,
                                                     int* box) {
    unsigned long long nf = 0, nh = 0, sf = 0, sh = 0;
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_cells; i += (long long)gridDim.x * 256) {
        const unsigned f = free[i], h = hit[i];
        nf += f ? 1 : 0; nh += h ? 1 : 0; sf += f; sh += h;
        if (f | h) {
            const int ix = (int)(i % nx), iy = (int)(i / nx);
            x0 = ix < x0 ? ix : x0; y0 = iy < y0 ? iy : y0; x1 = ix > x1 ? ix : x1; y1 = iy > y1 ? iy : y1;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        nf += __shfl_xor(nf, s); nh += __shfl_xor(nh, s); sf += __shfl_xor(sf, s); sh += __shfl_xor(sh, s);
        const int ax = __shfl_xor(x0, s), ay = __shfl_xor(y0, s), bx = __shfl_xor(x1, s), by = __shfl_xor(y1, s);
        x0 = ax < x0 ? ax : x0; y0 = ay < y0 ? ay : y0; x1 = bx > x1 ? bx : x1; y1 = by > y1 ? by : y1;
    }
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        atomicAdd(&sums[0], nf); atomicAdd(&sums[1], nh); atomicAdd(&sums[2], sf); atomicAdd(&sums[3], sh);
        atomicMin(&box[0], x0); atomicMin(&box[1], y0); atomicMax(&box[2], x1); atomicMax(&box[3], y1);
    }
}
