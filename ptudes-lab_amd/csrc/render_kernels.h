// render_kernels.h -- frames of the fly-by drawn on the device: point splats with a depth test (include/ptudes_mi.h ptl_render_frames).
//
// Frame buffer.  Per frame width * height 64-bit keys, key = (bits of float32(view depth) << 32) | rgba, an empty pixel is all ones.  The view
// depth is positive, so the unsigned order of the float's bits is the depth order, and a pixel's final key is the MINIMUM over all splats
// that cover it: a function of the set of drawn points only - not of the pool order, a block id, the launch geometry or scheduling.  Two
// points at the same float32 depth in one pixel resolve to the smaller rgba word (the low half of the key decides the minimum); rgba is the
// little-endian word of the bytes R, G, B, A (R is the lowest byte).
//
// Per point (x, y, z) and camera {view[12] row-major 3 x 4, fx, fy, cx, cy, near, far}, all in fp64, no contraction (-ffp-contract=off), in this order:
//   xc = ((v0 x + v1 y) + v2 z) + v3,  yc = ((v4 x + v5 y) + v6 z) + v7,  zc = ((v8 x + v9 y) + v10 z) + v11
//   rejected when !(zc > near) or zc >= far                              (before any division)
//   u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy
//   column = floor(u), row = floor(v)                                    (floor, not truncation: u = -0.5 is column -1)
//   rejected when floor(u) is outside [-8, width + 8) or floor(v) outside [-8, height + 8), NaN included  (no footprint of <= 5 pixels reaches
//   the image from there; the test is on the doubles, so a quotient beyond the integers never becomes a pixel index)
//   footprint: point_px x point_px pixels (1 .. 5), top-left (column - (point_px - 1) / 2, row - (point_px - 1) / 2) with integer division,
//   clipped pixel by pixel to the image
//   colour of a map point: palette[clamp(floor((z - z_lo) zscale), 0, 255)], zscale = 256 / (z_hi - z_lo) computed once on the host, z the WORLD
//   height of the point (NaN gives entry 0); an overlay point carries its own rgba
//   depth half of the key: the bits of (float) zc (round to nearest even)
//   per covered pixel: a plain load of the current key, and only when the new key is smaller a 64-bit atomicMin.  Keys only ever decrease
//   during a frame, so a stale load can only cause an atomic that changes nothing, never skip one that would.
//   A point that passed the depth test and has at least one pixel of its footprint inside the image counts as "in view"; the counts are kept per
//   lane and added with one atomic per wavefront and frame.
//
// k_render_splat<MapSrc>      walks the map's pool the way the export does: a wavefront takes 64 consecutive block ids, reads their stored counts from
//                             the directory (coalesced), then its lanes take the chunk's point slots (block, slot) in order - consecutive lanes read
//                             consecutive 24-byte points of one block.  Grid: (point chunks, frames of the batch), grid-stride over the chunks, the
//                             block count capped.
// k_render_splat<OverlaySrc>  the same body over a renderer-owned array of (xyz fp64, rgba); its point size is the overlay's.
// k_render_resolve            one thread per pixel and frame: empty -> background, else the key's colour; with edl_strength > 0 eye-dome lighting from
//                             the depth halves d of the four neighbours at edl_radius_px, in the order left, right, up, down, those in the image and not
//                             empty: m = (sum of (log2(d) - log2(d_nb))) / their number (0 when there is none),
//                             s = exp(-edl_strength max(0, m)), each colour channel c becomes floor(c s + 0.5), alpha is kept.  Writes RGBA8 and, when
//                             asked, the float32 depth (+inf for an empty pixel).
// Clearing the keys is a memset with 0xFF on the renderer's stream.
#pragma once
#include "icp_kernels.h"
#include "score_kernels.h"  // score_blk_count: the per-block count of the ColorSrc walk and of its prefix

#define RENDER_THREADS 256
#define RENDER_MAX_BLOCKS 2048   // workgroups per frame of a splat launch
#define RENDER_MAX_PX 5
#define RENDER_EMPTY 0xFFFFFFFFFFFFFFFFull

struct RenderCam {  // == ptl_render_cam
    double v[12];
    double fx, fy, cx, cy, near_m, far_m;
};

struct RenderArgs {
    int width, height;
    int point_px;              // of map points
    double z_lo, zscale;       // colour of a map point
    const RenderCam* cams;     // [frames of the batch]
    const unsigned* palette;   // [256]
    unsigned long long* keys;  // [frames][height][width]
    unsigned long long* in_view;  // [frames]
};

struct MapSrc {
    Ctx c;
};
struct OverlaySrc {
    const double* xyz;     // [n][3]
    const unsigned* rgba;  // [n]
    int n;
    int point_px;
};

// one point into one frame; true when it is in view.  EARLY: the plain load in front of the atomic.
template <bool EARLY>
__device__ __forceinline__ bool render_point(const RenderArgs& a, const RenderCam& cam, unsigned long long* keys, double x, double y, double z,
                                             unsigned rgba, int px) {
    const double xc = ((cam.v[0] * x + cam.v[1] * y) + cam.v[2] * z) + cam.v[3];
    const double yc = ((cam.v[4] * x + cam.v[5] * y) + cam.v[6] * z) + cam.v[7];
    const double zc = ((cam.v[8] * x + cam.v[9] * y) + cam.v[10] * z) + cam.v[11];
    if (!(zc > cam.near_m) || zc >= cam.far_m) return false;
    const double u = cam.fx * (xc / zc) + cam.cx, v = cam.fy * (yc / zc) + cam.cy;
    const double fu = floor(u), fv = floor(v);
    if (!(fu >= -8.0 && fu < (double)(a.width + 8)) || !(fv >= -8.0 && fv < (double)(a.height + 8))) return false;
    const int half = (px - 1) / 2;
    const int x0 = (int)fu - half, y0 = (int)fv - half;
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)zc) << 32) | (unsigned long long)rgba;
    bool any = false;
    for (int dy = 0; dy < px; ++dy) {
        const int yy = y0 + dy;
        if ((unsigned)yy >= (unsigned)a.height) continue;
        for (int dx = 0; dx < px; ++dx) {
            const int xx = x0 + dx;
            if ((unsigned)xx >= (unsigned)a.width) continue;
            any = true;
            unsigned long long* p = keys + (size_t)yy * (size_t)a.width + (size_t)xx;
            if (!EARLY || *p > key) atomicMin(p, key);
        }
    }
    return any;
}

__device__ __forceinline__ unsigned render_palette_index(double z, double z_lo, double zscale) {
    const double t = floor((z - z_lo) * zscale);
    return t >= 255.0 ? 255u : (t > 0.0 ? (unsigned)(int)t : 0u);
}

// the in-view counts of a wavefront's lanes -> one atomic (every lane of the wavefront gets here)
__device__ __forceinline__ void render_count(unsigned long long* dst, int mine) {
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine > 0) atomicAdd(dst, (unsigned long long)mine);
}

template <bool EARLY>
__device__ __forceinline__ void render_walk(const MapSrc& s, const RenderArgs& a, const RenderCam& cam, unsigned long long* keys, int& mine) {
    const Ctx& c = s.c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = RENDER_THREADS / 64;
    const int n_chunks = (c.pool_cap + 63) / 64;
    const int S = c.n_small > 0 && c.P < SMALL_CAP ? SMALL_CAP : c.P;  // point slots per block of the walk
    for (int ch = blockIdx.x * waves + wave; ch < n_chunks; ch += gridDim.x * waves) {
        const int b = ch * 64 + lane;
        int cnt = 0;
        if (b < c.pool_cap) {
            const int h = blk_hdr(c, b)[0], cap = blk_cap(c, b);
            cnt = h <= 0 ? 0 : (h < cap ? h : cap);
        }
        if (__ballot(cnt > 0) == 0ull) continue;  // (uniform)
        for (int it = 0; it < S; ++it) {
            const int i = it * 64 + lane, bi = i / S, j = i - bi * S;
            const int cb = __shfl(cnt, bi);
            if (j >= cb) continue;
            const double* X = blk_x(c, ch * 64 + bi) + 3 * j;
            const double x = X[0], y = X[1], z = X[2];
            mine += render_point<EARLY>(a, cam, keys, x, y, z, a.palette[render_palette_index(z, a.z_lo, a.zscale)], a.point_px) ? 1 : 0;
        }
    }
}

template <bool EARLY>
__device__ __forceinline__ void render_walk(const OverlaySrc& s, const RenderArgs& a, const RenderCam& cam, unsigned long long* keys, int& mine) {
    for (int i = blockIdx.x * RENDER_THREADS + threadIdx.x; i < s.n; i += gridDim.x * RENDER_THREADS)
        mine += render_point<EARLY>(a, cam, keys, s.xyz[3 * (size_t)i], s.xyz[3 * (size_t)i + 1], s.xyz[3 * (size_t)i + 2], s.rgba[i], s.point_px) ? 1 : 0;
}

// k_render_splat<ColorSrc>: the walk of MapSrc over the same pool with a colour word PER STORED POINT in pool order (block id, then slot:
// ptl_render_set_point_colors) in place of the height palette; projection, footprint, depth key and the minimum are
// render_point's, unchanged.  rgba[blk_off[b] + j] is point j of block b; blk_off is the exclusive prefix of score_blk_count over the block ids
// (k_score_count / k_score_scan / k_carve_blkoff), and the walk's per-block count here is score_blk_count too: ONE function on both sides.
struct ColorSrc {
    Ctx c;
    const int* blk_off;    // [pool_cap]
    const unsigned* rgba;  // [n], pool order
    int n;
};
template <bool EARLY>
__device__ __forceinline__ void render_walk(const ColorSrc& s, const RenderArgs& a, const RenderCam& cam, unsigned long long* keys, int& mine) {
    const Ctx& c = s.c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = RENDER_THREADS / 64;
    const int n_chunks = (c.pool_cap + 63) / 64;
    const int S = c.n_small > 0 && c.P < SMALL_CAP ? SMALL_CAP : c.P;  // point slots per block of the walk
    for (int ch = blockIdx.x * waves + wave; ch < n_chunks; ch += gridDim.x * waves) {
        const int b = ch * 64 + lane;
        const int cnt = b < c.pool_cap ? score_blk_count(c, b) : 0;
        const int off = cnt > 0 ? s.blk_off[b] : 0;
        if (__ballot(cnt > 0) == 0ull) continue;  // (uniform)
        for (int it = 0; it < S; ++it) {
            const int i = it * 64 + lane, bi = i / S, j = i - bi * S;
            const int cb = __shfl(cnt, bi), ob = __shfl(off, bi);
            if (j >= cb) continue;
            const int oi = ob + j;
            if (oi < 0 || oi >= s.n) continue;  // (cannot happen behind the set call's check of the directory's total)
            const double* X = blk_x(c, ch * 64 + bi) + 3 * j;
            mine += render_point<EARLY>(a, cam, keys, X[0], X[1], X[2], s.rgba[oi], a.point_px) ? 1 : 0;
        }
    }
}

template <class SRC, bool EARLY>
__global__ __launch_bounds__(RENDER_THREADS) void k_render_splat(SRC s, RenderArgs a) {
    const int f = blockIdx.y;
    const RenderCam cam = a.cams[f];
    unsigned long long* keys = a.keys + (size_t)f * (size_t)a.width * (size_t)a.height;
    int mine = 0;
    render_walk<EARLY>(s, a, cam, keys, mine);
    render_count(a.in_view + f, mine);
}

struct ResolveArgs {
    int width, height, n_frames;
    unsigned background;
    double edl_strength;
    int edl_radius;
    const unsigned long long* keys;
    unsigned* rgba;   // [frames][height][width]
    float* depth;     // the same, or null
};

__device__ __forceinline__ void render_edl_term(const unsigned long long* K, int w, int h, int x, int y, double l2d, double& sum, int& n) {
    if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return;
    const unsigned long long k = K[(size_t)y * (size_t)w + (size_t)x];
    if (k == RENDER_EMPTY) return;
    sum += l2d - log2((double)__uint_as_float((unsigned)(k >> 32)));
    n += 1;
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_resolve(ResolveArgs a) {
    const size_t per = (size_t)a.width * (size_t)a.height;
    const size_t i = (size_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (i >= per * (size_t)a.n_frames) return;
    const size_t f = i / per, pix = i - f * per;
    const int y = (int)(pix / (size_t)a.width), x = (int)(pix - (size_t)y * (size_t)a.width);
    const unsigned long long* K = a.keys + f * per;
    const unsigned long long k = K[pix];
    if (k == RENDER_EMPTY) {
        a.rgba[i] = a.background;
        if (a.depth) a.depth[i] = __uint_as_float(0x7F800000u);
        return;
    }
    unsigned rgba = (unsigned)k;
    const float d = __uint_as_float((unsigned)(k >> 32));
    if (a.edl_strength > 0.0) {
        const double l2d = log2((double)d);
        double sum = 0.0;
        int n = 0;
        render_edl_term(K, a.width, a.height, x - a.edl_radius, y, l2d, sum, n);
        render_edl_term(K, a.width, a.height, x + a.edl_radius, y, l2d, sum, n);
        render_edl_term(K, a.width, a.height, x, y - a.edl_radius, l2d, sum, n);
        render_edl_term(K, a.width, a.height, x, y + a.edl_radius, l2d, sum, n);
        const double m = n > 0 ? sum / (double)n : 0.0;
        const double s = exp(-a.edl_strength * (m > 0.0 ? m : 0.0));
        unsigned out = rgba & 0xFF000000u;
        for (int ch = 0; ch < 3; ++ch) {
            const double cc = floor((double)((rgba >> (8 * ch)) & 0xFFu) * s + 0.5);
            out |= ((unsigned)(int)cc & 0xFFu) << (8 * ch);
        }
        rgba = out;
    }
    a.rgba[i] = rgba;
    if (a.depth) a.depth[i] = d;
}
