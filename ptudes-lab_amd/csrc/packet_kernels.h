// packet_kernels.h -- Ouster lidar UDP payloads -> staggered range image + column headers, on the device.
//
// A packet is column-major (C columns of [header | H pixels | trailer]); the image is row-major (u32[H][W], column = measurement_id), so
// the work is a transpose.  Three passes behind one initialisation (k_pkt_init: no owners, no first packets, zero counters), one launch each
// for ALL packets / sweeps of a call:
//   k_pkt_owner   one thread per packet column: which packet column supplies image column (sweep, measurement_id)?  The LAST counted one
//                 in arrival order - an integer atomicMax over (packet index * C + column), so the answer does not depend on scheduling.
//   k_pkt_decode  one workgroup per packet: the packet goes to LDS once with 16-byte loads; thread (h, c), c fastest, reads pixel h of
//                 column c from LDS and writes image row h at that column's measurement_id - C consecutive u32 per row (64 B at C = 16)
//                 while the ids of a packet are consecutive, as the sensor sends them.  Only the owner of an image column writes it.
//   k_pkt_finish  one workgroup per (sweep, row): zeroes what no counted column supplied; row 0 also writes the sweep's summary.
// Every output word is written exactly once per call, by a writer chosen before anything is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PKT_THREADS 256
#define PKT_MAX_COLS 64         // columns per packet the decode kernel keeps owners for
#define PKT_MAX_BYTES 61440     // a packet is staged whole in LDS
#define PKT_NO_PACKET 0x7fffffff  // first_pkt of a sweep without a packet

// byte layout of one lidar profile for (H, C); every offset is a multiple of 4 (2 for the 16-bit fields)
struct PktLayout {
    int H, W, C;
    int pkt_hdr;        // bytes before column 0
    int col_stride;     // column header + H pixels + column trailer
    int col_hdr;        // bytes before pixel 0 of a column
    int pix;            // bytes per pixel; the range field is its first dword (u16 in the 4-byte pixel)
    unsigned mask;      // range bits
    int shift;          // value << shift = mm
    int status_off;     // in the column; bit 0 = valid
    int frame_off;      // u16, in the packet
    int bytes;          // whole packet
    int stride;         // device stride of the staged packets, a multiple of 16
};

struct PktSummary {     // == ptl_pkt_summary (include/ptudes_mi.h)
    uint32_t frame_id, valid_columns, first_valid_id, last_valid_id;
    uint64_t first_valid_ts, last_valid_ts;
    uint32_t nonzero_ranges, ignored_columns;
};

struct PktOut {
    unsigned* img;              // sweep s: img + s * img_stride, [H][W]
    size_t img_stride;          // in u32
    unsigned long long* ts;     // [sweeps][W]
    unsigned short* status;     // [sweeps][W]
    int* owner;                 // [sweeps][W]: packet * C + column of the counted column that supplies it, -1 none
    int* first_pkt;             // [sweeps]: lowest packet index of the sweep (its frame id is the sweep's)
    PktSummary* sum;            // [sweeps]
};

__device__ __forceinline__ unsigned pkt_u16(const unsigned* dw, int byte_off) { return (dw[byte_off >> 2] >> ((byte_off & 2) * 8)) & 0xffffu; }

__global__ __launch_bounds__(PKT_THREADS) void k_pkt_init(int n_sweeps, int W, PktOut o) {
    const int i = blockIdx.x * PKT_THREADS + threadIdx.x;
    if (i < n_sweeps * W) o.owner[i] = -1;
    if (i < n_sweeps) {
        o.first_pkt[i] = PKT_NO_PACKET;
        o.sum[i] = PktSummary{};
    }
}

// sop == nullptr: every packet belongs to sweep 0
__global__ __launch_bounds__(PKT_THREADS) void k_pkt_owner(PktLayout L, const unsigned char* pkts, const int* sop, int n, PktOut o) {
    const int i = blockIdx.x * PKT_THREADS + threadIdx.x;
    if (i >= n * L.C) return;
    const int p = i / L.C, c = i - p * L.C;
    const int s = sop ? sop[p] : 0;
    if (s < 0) return;
    const unsigned* col = (const unsigned*)(pkts + (size_t)p * L.stride + L.pkt_hdr + (size_t)c * L.col_stride);
    const unsigned id = pkt_u16(col, 8), st = pkt_u16(col, L.status_off);
    if (c == 0) atomicMin(&o.first_pkt[s], p);
    if (!(st & 1u)) return;
    if (id >= (unsigned)L.W) { atomicAdd(&o.sum[s].ignored_columns, 1u); return; }
    atomicMax(&o.owner[(size_t)s * L.W + id], i);
}

__global__ __launch_bounds__(PKT_THREADS) void k_pkt_decode(PktLayout L, const unsigned char* pkts, const int* sop, PktOut o) {
    extern __shared__ uint4 pkt_lds4[];
    __shared__ int s_id[PKT_MAX_COLS];
    __shared__ unsigned s_nz;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int s = sop ? sop[p] : 0;
    if (s < 0) return;  // (uniform: the whole workgroup leaves)
    const uint4* src = (const uint4*)(pkts + (size_t)p * L.stride);
    for (int i = tid; i < (L.stride >> 4); i += PKT_THREADS) pkt_lds4[i] = src[i];
    if (tid == 0) s_nz = 0;
    __syncthreads();
    const unsigned* dw = (const unsigned*)pkt_lds4;
    if (tid < L.C) {
        const unsigned* col = dw + ((L.pkt_hdr + tid * L.col_stride) >> 2);
        const unsigned id = pkt_u16(col, 8), st = pkt_u16(col, L.status_off);
        int mine = -1;
        if ((st & 1u) && id < (unsigned)L.W && o.owner[(size_t)s * L.W + id] == p * L.C + tid) {
            mine = (int)id;
            // (the column stride is 12 + 12 H or 20 + 12 H: a timestamp is 4-byte aligned only, two dwords)
            o.ts[(size_t)s * L.W + id] = (unsigned long long)col[0] | ((unsigned long long)col[1] << 32);
            o.status[(size_t)s * L.W + id] = (unsigned short)st;
        }
        s_id[tid] = mine;
    }
    __syncthreads();
    unsigned* img = o.img + (size_t)s * o.img_stride;
    const int HC = L.H * L.C;
    for (int base = 0; base < HC; base += PKT_THREADS) {  // (uniform trip count: the ballot below sees every lane)
        const int idx = base + tid;
        unsigned r = 0;
        if (idx < HC) {
            const int h = idx / L.C, c = idx - h * L.C, id = s_id[c];
            if (id >= 0) {
                r = (dw[(L.pkt_hdr + c * L.col_stride + L.col_hdr + h * L.pix) >> 2] & L.mask) << L.shift;
                img[(size_t)h * L.W + id] = r;
            }
        }
        const unsigned long long b = __ballot(r != 0);
        if ((tid & 63) == 0 && b) atomicAdd(&s_nz, (unsigned)__popcll(b));
    }
    __syncthreads();
    if (tid == 0 && s_nz) atomicAdd(&o.sum[s].nonzero_ranges, s_nz);
}

// grid (sweeps, H)
__global__ __launch_bounds__(PKT_THREADS) void k_pkt_finish(PktLayout L, const unsigned char* pkts, PktOut o) {
    __shared__ unsigned s_cnt, s_first, s_last;
    const int s = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int* own = o.owner + (size_t)s * L.W;
    unsigned* row = o.img + (size_t)s * o.img_stride + (size_t)h * L.W;
    for (int w = tid; w < L.W; w += PKT_THREADS)
        if (own[w] < 0) row[w] = 0;
    if (h != 0) return;
    if (tid == 0) { s_cnt = 0; s_first = 0xffffffffu; s_last = 0; }
    __syncthreads();
    for (int w = tid; w < L.W; w += PKT_THREADS) {
        if (own[w] < 0) {
            o.ts[(size_t)s * L.W + w] = 0;
            o.status[(size_t)s * L.W + w] = 0;
        } else {
            atomicAdd(&s_cnt, 1u);
            atomicMin(&s_first, (unsigned)w);
            atomicMax(&s_last, (unsigned)w);
        }
    }
    __syncthreads();
    if (tid == 0) {
        PktSummary* m = &o.sum[s];  // (nonzero_ranges / ignored_columns: summed by the two passes before)
        const int fp = o.first_pkt[s];
        m->frame_id = fp == PKT_NO_PACKET ? 0u : pkt_u16((const unsigned*)(pkts + (size_t)fp * L.stride), L.frame_off);
        m->valid_columns = s_cnt;
        m->first_valid_id = s_cnt ? s_first : 0u;
        m->last_valid_id = s_cnt ? s_last : 0u;
        m->first_valid_ts = s_cnt ? o.ts[(size_t)s * L.W + s_first] : 0ull;
        m->last_valid_ts = s_cnt ? o.ts[(size_t)s * L.W + s_last] : 0ull;
    }
}
