// packet_field_kernels.h -- the channel fields of Ouster lidar pixels -> staggered field images, on the device (include/ptudes_mi.h
// ptl_pktdec_decode_fields).  packet_kernels.h keeps one field of a pixel, the range; reflectivity, signal and near-infrared
// sit in the same pixel words.  This pass runs BEHIND the three passes of packet_kernels.h (as they are) on the same staged packets and the
// same owners, so the packets cross the bus once and a field image has the range image's columns.
//
// A field of a pixel (ptl_pkt_field): `bytes` (1, 2 or 4) at byte `offset` from the start of the pixel, offset % bytes == 0 and
// offset + bytes <= the pixel size; value = (little-endian word & mask) << shift for shift >= 0, >> -shift otherwise, as u32; mask == 0 means
// all bits.  Which field sits where in which profile is DATA handed in by the caller (ptl_pkt_field_default holds the table), not code.
//
// Decode rule: field image u32[H][W], staggered like the range image.  Image column `id` is written by the owner k_pkt_owner chose (the last
// counted packet column in arrival order) and by nobody else; a column with no owner is 0; a field is written whether or not the pixel's
// range is 0.
//
//   k_pkt_fields   ONE launch for all requested fields (1 .. PKT_MAX_FIELDS).  Workgroups [0, n): one per packet, the packet staged whole in
//                  LDS with 16-byte loads as k_pkt_decode stages it; thread (h, c), c fastest, reads the ALIGNED dword that holds the field
//                  of pixel h of column c - a pixel starts on a dword and offset % bytes == 0, so a byte or halfword never straddles two
//                  dwords - and shifts the field down: no unaligned or sub-dword LDS load.  The pixel's dwords are read once per field, C
//                  consecutive u32 of an image row are written together (64 B at C = 16), per field.  Workgroups [n, n + sweeps H): one per
//                  (sweep, row), zero what no counted column supplies - the owners are final before this launch, so the two kinds of
//                  workgroup write disjoint words and every output word is written exactly once.
#pragma once
#include "packet_kernels.h"

#define PKT_MAX_FIELDS 4

struct PktFields {
    int n;                          // 1 .. PKT_MAX_FIELDS
    int off[PKT_MAX_FIELDS];        // bytes from the start of the pixel
    int bytes[PKT_MAX_FIELDS];      // 1, 2, 4
    unsigned mask[PKT_MAX_FIELDS];  // applied to the field's word; never 0 here (the host turns 0 into all ones)
    int shift[PKT_MAX_FIELDS];      // > 0 left, < 0 right, |shift| <= 31
    unsigned* img[PKT_MAX_FIELDS];  // field f, sweep s: img[f] + s * img_stride, [H][W]
    size_t img_stride;              // in u32
};

// the field at byte `off` (a multiple of `bytes`) behind the dword-aligned byte `pix` of the staged packet
__device__ __forceinline__ unsigned pkt_field_value(const unsigned* dw, int pix, int off, int bytes, unsigned mask, int shift) {
    const int at = pix + off;
    unsigned v = dw[at >> 2] >> ((at & 3) * 8);
    if (bytes == 1) v &= 0xffu;
    else if (bytes == 2) v &= 0xffffu;
    v &= mask;
    return shift >= 0 ? v << shift : v >> -shift;
}

__global__ __launch_bounds__(PKT_THREADS) void k_pkt_fields(PktLayout L, const unsigned char* pkts, const int* sop, int n_pkts, PktOut o, PktFields F) {
    extern __shared__ uint4 pktf_lds4[];
    __shared__ int s_id[PKT_MAX_COLS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_pkts) {  // (uniform) the rows' share: what no counted column supplies is 0
        const int r = (int)blockIdx.x - n_pkts, s = r / L.H, h = r - s * L.H;
        const int* own = o.owner + (size_t)s * L.W;
        for (int w = tid; w < L.W; w += PKT_THREADS)
            if (own[w] < 0)
                for (int f = 0; f < F.n; ++f) F.img[f][(size_t)s * F.img_stride + (size_t)h * L.W + w] = 0;
        return;
    }
    const int p = blockIdx.x;
    const int s = sop ? sop[p] : 0;
    if (s < 0) return;  // (uniform: the whole workgroup leaves)
    const uint4* src = (const uint4*)(pkts + (size_t)p * L.stride);
    for (int i = tid; i < (L.stride >> 4); i += PKT_THREADS) pktf_lds4[i] = src[i];
    __syncthreads();
    const unsigned* dw = (const unsigned*)pktf_lds4;
    if (tid < L.C) {
        const unsigned* col = dw + ((L.pkt_hdr + tid * L.col_stride) >> 2);
        const unsigned id = pkt_u16(col, 8), st = pkt_u16(col, L.status_off);
        s_id[tid] = ((st & 1u) && id < (unsigned)L.W && o.owner[(size_t)s * L.W + id] == p * L.C + tid) ? (int)id : -1;
    }
    __syncthreads();
    const int HC = L.H * L.C;
    for (int idx = tid; idx < HC; idx += PKT_THREADS) {
        const int h = idx / L.C, c = idx - h * L.C, id = s_id[c];
        if (id < 0) continue;
        const int pix = L.pkt_hdr + c * L.col_stride + L.col_hdr + h * L.pix;
        for (int f = 0; f < F.n; ++f)
            F.img[f][(size_t)s * F.img_stride + (size_t)h * L.W + id] = pkt_field_value(dw, pix, F.off[f], F.bytes[f], F.mask[f], F.shift[f]);
    }
}
