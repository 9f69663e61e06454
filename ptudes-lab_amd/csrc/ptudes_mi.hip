// ptudes_mi.hip -- C-ABI (include/ptudes_mi.h) + host orchestration of the HIP kernels.
//
// One HIP stream per handle; all arithmetic runs in the kernels of icp_kernels.h / ekf_kernels.h.
// The host only sizes buffers, enqueues launches and copies results: there is no CPU compute path.
#include "../../include/ptudes_mi.h"
#include "ekf_kernels.h"
#include "icp_kernels.h"
#include "seq_kernel.h"
#include "fly_kernels.h"
#include "packet_kernels.h"
#include "packet_field_kernels.h"
#include "score_kernels.h"
#include "render_kernels.h"
#include "compare_kernels.h"
#include "carve_kernels.h"
#include "cast_kernels.h"
#include "grid_kernels.h"
#include "paint_kernels.h"
#include "place_kernels.h"
#include "pose_kernels.h"
#include "hip_own.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

static thread_local char g_err[512] = "";
static int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
// (a failed runtime call also leaves its code in the runtime's sticky "last error": it is cleared here, or a LATER, unrelated
// HIPCHK(hipGetLastError()) - behind a kernel launch of another handle - would report this call's failure as its own)
#define HIPCHK(x)                                                                                    \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) { (void)hipGetLastError(); return set_err(PTL_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } \
    } while (0)

extern "C" const char* ptl_last_error(void) { return g_err; }
extern "C" int ptl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int ptl_backend(void) { return ptl_device_count() > 0 ? 1 : 0; }
extern "C" int ptl_host_pin(int device_id, void* host_ptr, uint64_t bytes) {
    if (!host_ptr || bytes == 0) return set_err(PTL_ERR_ARG, "null argument");
    if (ptl_device_count() <= device_id || device_id < 0) return set_err(PTL_ERR_HIP, "no HIP device %d", device_id);
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipHostRegister(host_ptr, (size_t)bytes, hipHostRegisterDefault));
    return PTL_OK;
}
extern "C" int ptl_host_unpin(void* host_ptr) {
    if (!host_ptr) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipHostUnregister(host_ptr));
    return PTL_OK;
}

// ---- ABI guard (include/ptudes_mi.h): a configuration struct says how big its writer thinks it is and which ABI it was written against
extern "C" int ptl_abi_version(void) { return PTL_ABI_VERSION; }
extern "C" int64_t ptl_sizeof_cfg(int which) {
    switch (which) {
        case PTL_CFG_ICP: return (int64_t)sizeof(ptl_icp_cfg);
        case PTL_CFG_EKF: return (int64_t)sizeof(ptl_ekf_cfg);
        case PTL_CFG_SEQ: return (int64_t)sizeof(ptl_seq_cfg);
        case PTL_CFG_ICP_STATS: return (int64_t)sizeof(ptl_icp_stats);
        case PTL_CFG_PKT_FORMAT: return (int64_t)sizeof(ptl_pkt_format);
        case PTL_CFG_MAP_SCORE: return (int64_t)sizeof(ptl_map_score_cfg);
    }
    return -1;
}
// (the two leading words are read only: on a mismatch nothing of the caller's memory is written)
static int abi_check(const char* what, uint32_t size_caller, uint32_t abi_caller, size_t size_lib) {
    if (size_caller == (uint32_t)size_lib && abi_caller == (uint32_t)PTL_ABI_VERSION) return PTL_OK;
    return set_err(PTL_ERR_ARG, "%s: the caller's struct_size = %u, abi_version = %u; this library's sizeof(%s) = %zu, PTL_ABI_VERSION = %d "
                   "- set both before the call (PTL_CFG_INIT) and rebuild / rewrite the binding against this library's include/ptudes_mi.h",
                   what, size_caller, abi_caller, what, size_lib, PTL_ABI_VERSION);
}
#define ABI_CHECK(what, p) do { int rc_ = abi_check(#what, (p)->struct_size, (p)->abi_version, sizeof(what)); if (rc_) return rc_; } while (0)

// ================================================================================================ ICP
// (every handle: streams first, events next, the memory's owner last - they are destroyed in the reverse order)
struct ptl_icp {
    ptl_icp_cfg cfg;
    Stream stream;       // its own, or borrowed from the runner it is a member of
    Stream map_stream;   // the map update's (below)
    Ctx c = {};          // kernel context (device pointers)
    int64_t n_max = 0;
    int nblk_scan = 0;
    void* d_in = nullptr;       // staging for host-provided scans (n_max * 3 * 8 bytes)
    double* d_t01 = nullptr;
    double* d_ext = nullptr;    // staging for a host-provided guess
    int* d_counter = nullptr;
    int64_t traj_cap = 0;
    int64_t scans_done = 0;
    unsigned char* d_row_mask = nullptr;  // active-beam mask for range-image input, or null
    int64_t last_n = 0;          // points of the previous scan
    bool lazy_map_stats = false; // per-call API: do not wait for the scan's map update before returning (ptl_icp_set_lazy_map_stats)
    // profiling of the dominant kernel
    int prof_every = 1;  // time every n-th GN launch (two event records cost ~18 us of command-processor time per scan)
    GnTimer prof;
    // set by the sequence runner around a scan: the GN kernel waits for `gn_wait` (the EKF stream produced the guess)
    hipEvent_t gn_wait = nullptr, gn_done = nullptr;  // ... and `gn_done` is recorded right after it (a second event: two streams waiting on one measured slower); both borrowed
    Event ev_step_guess, ev_step_gn;  // ptl_icp_ekf_step's own pair (created on first use)
    // ev_gn is recorded right after each GN launch: the map update (and the sequence runner's EKF step) start from it.
    // frame_down is double-buffered so that K3 of scan k+1 does not overwrite what K7 of scan k still reads.
    // the map update (K7-K10, rebuild) runs on `map_stream`: it needs the GN result (ev_gn) and must be complete before
    // the next GN launch (ev_map); beside it, on `stream`, run K0-K4 of the next scan
    Event ev_map;
    bool ev_map_valid = false;
    Event ev_gn;
    bool ev_gn_valid = false;
    int* n_src_hint = nullptr;  // pinned host copy of the last scan's N_s, written by an asynchronous copy on the map stream
    double* fd_buf[2] = {nullptr, nullptr};
    // IMU deskew: the prologue waits for `pro_wait` (the filter's predicts through the sweep's samples); the per-call step's sweep times and
    // recorded modes, one entry per scan (dk_cap entries, grown with the scans)
    hipEvent_t pro_wait = nullptr;   // (borrowed)
    double* dk_t0t1 = nullptr;
    int* dk_modes = nullptr;
    int64_t dk_cap = 0;
    bool dk_wired = false;           // the device state holds the IMU deskew's wiring: the prologue runs its IMU instance
    std::vector<signed char> dk_rec; // per registered scan (icp_enqueue_scan): its deskew mode, or -1 = IMU-wired (the device recorded it)
    FlyWs* d_fly = nullptr;          // posed scans into the map (fly_kernels.h): count, flag and totals, allocated by the first such call
    DevOwner mem;                    // every device buffer above and in `c`, and the pinned word
};

extern "C" int ptl_icp_default_cfg(ptl_icp_cfg* cfg, double max_range, double min_range) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_icp_cfg, cfg);
    PTL_CFG_INIT(cfg);
    cfg->max_range = max_range;
    cfg->min_range = min_range;
    cfg->voxel_size = max_range / 100.0;  // kiss-icp load_config
    cfg->max_points_per_voxel = 20;
    cfg->initial_threshold = 2.0;
    cfg->min_motion_th = 0.1;
    cfg->deskew = 1;
    cfg->max_iterations = 500;
    cfg->convergence = 1e-4;
    cfg->device_id = 0;
    cfg->scan_cols = 1024;
    cfg->max_points_per_scan = 131072;
    cfg->map_block_capacity = 1 << 19;
    // The table is sparse on purpose: a 2 x 2 x 2 brick of voxels is one 128-byte line, and two bricks that hash to the same line push each other's
    // entries into dependent probe rounds (probe-row rebuilds, map insert).  ~30 k occupied bricks in 2 M lines hardly ever meet; in the 262 k lines of
    // round 3's 2^21 slots they did: Gauss-Newton 2 357 -> 2 196 us per scan, + 7 % scans/s (profiles/r04_y_map_table_and_rebuild.txt).  256 MB per
    // sequence - what 288 GB per GPU are for.  The rebuild (tombstones dropped, table cleared by the team) is correspondingly rarer.
    cfg->map_table_capacity = 1 << 24;
    cfg->gn_workgroups = 256;
    cfg->rebuild_every = 128;
    cfg->gn_threads = 1024;
    cfg->gn_lanes_per_point = 32;
    cfg->map_small_blocks = 0;
    return PTL_OK;
}

// the whole of every destroy function: the handle's device first, then its members in their order
template <class H>
static int handle_destroy(H* h, int device_id) {
    (void)hipSetDevice(device_id);
    delete h;
    return PTL_OK;
}
#define ERR_FLAGS_FMT "device capacity/error flags 0x%x (1 key range, 2 block pool, 4 map table, 8 vds table, 16 gn barrier timeout)"

// ---- the kernel instance for a run-time configuration: f gets the template arguments as std::integral_constant values
// points per voxel: 20 (the default, unrolled) or 0 (any)
template <class F>
static void pick_p(int P, F&& f) {
    if (P == 20) f(std::integral_constant<int, 20>{}); else f(std::integral_constant<int, 0>{});
}
// workgroups per team: one of GC..., else 0 (any)
template <int... GC, class F>
static void pick_team(int g, F&& f) {
    if (!((g == GC ? (f(std::integral_constant<int, GC>{}), true) : false) || ...)) f(std::integral_constant<int, 0>{});
}
// A persistent kernel's workgroups wait for each other, so ALL of them have to be resident at once: what the runtime reports for this
// kernel on this device (partitioned GPU, fewer CUs, larger workgroups) instead of finding out through a poll time-out
template <class K>
static hipError_t resident_capacity(K kernel, int threads, int device_id, int* per_cu, int* cus) {
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kernel, threads, 0);
    return e != hipSuccess ? e : hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device_id);
}

__global__ void k_fill_free_stack(int* fs, int n, int base) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) fs[i] = base + n - 1 - i;  // pops hand out low block ids first
}
__global__ void k_state_init(DevState* st, int n_full, int n_small) {
    if (threadIdx.x || blockIdx.x) return;
    const double *dk_knots = st->dk_knots, *dk_t0t1 = st->dk_t0t1;  // the IMU deskew's wiring survives a cold start
    const long long* dk_nknots = st->dk_nknots;
    const int* dk_kovf = st->dk_kovf;
    int* dk_modes = st->dk_modes;
    const int dk_n = st->dk_n;
    memset(st, 0, sizeof(DevState));
    st->dk_knots = dk_knots; st->dk_t0t1 = dk_t0t1; st->dk_nknots = dk_nknots; st->dk_kovf = dk_kovf; st->dk_modes = dk_modes; st->dk_n = dk_n;
    Rt I = rt_identity();
    rt_to16(I, st->pose_first); rt_to16(I, st->pose_prev); rt_to16(I, st->pose_last);
    rt_to16(I, st->model_dev); rt_to16(I, st->guess); rt_to16(I, st->new_pose); rt_to16(I, st->T_icp);
    st->free_top = n_full;
    st->free_top_s = n_small;
    st->pool_hw = n_small;  // (an id bound: the full blocks' ids start behind the small ones)
    st->stats_pending = -1;
    st->dbg_dead_wg = -1;
}

// slots of a per-scan voxel table (power of two): make EXTRA="-DVDS1_SLOTS_PER_POINT=n -DVDS2_SLOTS_PER_POINT=m" for A/B runs
#ifndef VDS1_SLOTS_PER_POINT
#define VDS1_SLOTS_PER_POINT 64
#endif
#ifndef VDS2_SLOTS_PER_POINT
#define VDS2_SLOTS_PER_POINT 16
#endif
static size_t vds_table_slots(size_t per_point, size_t n) {
    size_t vcap = 1024;
    while (vcap < per_point * n) vcap <<= 1;
    return vcap;
}
static int icp_reset_device(ptl_icp* h) {
    Ctx& c = h->c;
    const DevOwner& m = h->mem;  // (each buffer whole: its size is what icp_alloc asked for)
    HIPCHK(hipMemsetAsync(c.vtab1, 0xFF, m.bytes_of(c.vtab1), h->stream));  // (key = EMPTY, index = none)
    HIPCHK(hipMemsetAsync(c.vtab2, 0xFF, m.bytes_of(c.vtab2), h->stream));
    HIPCHK(hipMemsetAsync(c.tab, 0xFF, m.bytes_of(c.tab), h->stream));
    HIPCHK(hipMemsetAsync(c.blocks, 0, m.bytes_of(c.blocks), h->stream));
    HIPCHK(hipMemsetAsync(c.bhdr, 0, m.bytes_of(c.bhdr), h->stream));
    HIPCHK(hipMemsetAsync(c.bfirst, 0, m.bytes_of(c.bfirst), h->stream));
    HIPCHK(hipMemsetAsync(c.bcnt1, 0, m.bytes_of(c.bcnt1), h->stream));  // look-back words of the compactions: tag 0 = never published
    HIPCHK(hipMemsetAsync(c.bcnt2, 0, m.bytes_of(c.bcnt2), h->stream));
    HIPCHK(hipMemsetAsync(c.gn_rows_ll, 0, m.bytes_of(c.gn_rows_ll), h->stream));  // the launch epoch restarts with the state
    HIPCHK(hipMemsetAsync(c.gn_xsum_ll, 0, m.bytes_of(c.gn_xsum_ll), h->stream));
    HIPCHK(hipMemsetAsync(c.wg_clk + 2 * c.G, 0, DIAG_SLOTS * sizeof *c.wg_clk, h->stream));  // (the per-workgroup clocks in front count since creation)
    k_fill_free_stack<<<(c.pool_cap - c.n_small + 255) / 256, 256, 0, h->stream>>>(c.free_stack, c.pool_cap - c.n_small, c.n_small);
    if (c.n_small > 0) k_fill_free_stack<<<(c.n_small + 255) / 256, 256, 0, h->stream>>>(c.free_stack_s, c.n_small, 0);
    k_state_init<<<1, 64, 0, h->stream>>>(c.st, c.pool_cap - c.n_small, c.n_small);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->map_stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // the other streams must not start on half-reset tables
    h->ev_gn_valid = false; h->ev_map_valid = false;
    h->scans_done = 0;
    h->last_n = 0;
    h->dk_rec.clear();
    return PTL_OK;
}

// the sizes of a registration handle's buffers, from its configuration (host only: nothing is allocated)
static void icp_settle(ptl_icp* h, const ptl_icp_cfg* cfg) {
    h->cfg = *cfg;
    Ctx& c = h->c;
    const int64_t n = cfg->max_points_per_scan;
    h->n_max = n;
    c.max_range = cfg->max_range; c.min_range = cfg->min_range; c.vs = cfg->voxel_size;
    c.vds1 = cfg->voxel_size * 0.5;  // KissICP.voxelize
    c.vds2 = cfg->voxel_size * 1.5;
    c.init_thr = cfg->initial_threshold; c.min_motion = cfg->min_motion_th; c.conv = cfg->convergence;
    c.P = cfg->max_points_per_voxel; c.deskew = cfg->deskew; c.max_iter = cfg->max_iterations;
    c.W = cfg->scan_cols > 0 ? cfg->scan_cols : 1;
    c.n_max = (int)n;
    // per-scan voxel tables.  A table line holds a 2x2x2 brick of voxels (brick_slot), so what counts is how many LINES are taken:
    // a voxel of a brick that lands on a taken line walks on through dependent reads, and one such voxel among the 512 claims of a
    // wavefront's round costs the wavefront another round trip.  The lines a scan touches do not depend on the table's size, the
    // slots are released by the compaction that follows (no clear per scan): size costs footprint only.  Pass 1 (~46 k voxels of
    // ~120 k points): 64 slots per point (K0-K4 516 -> 485 us per scan against 8; 32: 493); pass 2 (~14 k voxels): 16.
    c.vmask = (unsigned)(vds_table_slots(VDS1_SLOTS_PER_POINT, n) - 1);
    c.vmask2 = (unsigned)(vds_table_slots(VDS2_SLOTS_PER_POINT, n) - 1);
    c.tmask = (unsigned)(cfg->map_table_capacity - 1);
    c.bstride = (int)(((size_t)c.P * 24 + 127) / 128 * 128);  // points only: the per-voxel header lives in the block directory (bhdr / bfirst)
    c.n_small = (int)cfg->map_small_blocks;
    c.pool_cap = (int)(cfg->map_block_capacity + cfg->map_small_blocks);  // block ids: the small blocks first, then map_block_capacity full ones
    c.G = cfg->gn_workgroups;
    c.overlap_pre = 1;
    h->nblk_scan = (int)((n + 255) / 256);
}
// trajectory / statistics rows a handle starts with: 4096, doubled (as icp_grow_traj would) until a batch member's whole run fits
static int64_t icp_traj_rows(int64_t n_scans, bool batch_member) {
    int64_t cap = 4096;
    while (batch_member && cap < n_scans) cap *= 2;
    return cap;
}
// EVERY device buffer a settled registration handle is created with, once: `m` allocates them (h->mem) or only counts their bytes
// (ptl_batch_create's capacity check).  Per point of max_points_per_scan the work buffers (deskewed points, slots, frame_down x 2,
// source x 2, world frame_down, list links, probe rows, answer rows, the per-call input), the two per-scan voxel tables, the map table,
// the block pool with its directory and free stacks, the exchange rows, the state, `traj_rows` result rows
static void icp_alloc(DevOwner& m, ptl_icp* h, int64_t traj_rows) {
    Ctx& c = h->c;
    const size_t n = (size_t)h->n_max, n_small = (size_t)(c.n_small > 0 ? c.n_small : 1);
    m.add(&c.pts, 3 * n);
    m.add(&c.slot1, n); m.add(&c.slot2, n);
    m.add(&c.vtab1, (size_t)c.vmask + 1); m.add(&c.vtab2, (size_t)c.vmask2 + 1);
    m.add(&c.bcnt1, (size_t)h->nblk_scan); m.add(&c.bcnt2, (size_t)h->nblk_scan);
    m.add(&h->fd_buf[0], 3 * n); m.add(&c.src0, 3 * n);
    c.fd = h->fd_buf[0];
    m.add(&h->fd_buf[1], 3 * n);
    m.add(&c.src_cur, 3 * n); m.add(&c.fdw, 3 * n);
    m.add(&c.coltab, (size_t)c.W * 12);
    m.add(&c.pslot, n); m.add(&c.nxt, n);
    m.add(&c.prank, n); m.add(&c.plen, n);
    m.add(&c.tab, (size_t)c.tmask + 1);
    m.add(&c.blocks, (size_t)c.n_small * SMALL_BYTES + (size_t)(c.pool_cap - c.n_small) * c.bstride);
    c.big_base = (unsigned char*)((uintptr_t)c.blocks + (uintptr_t)c.n_small * SMALL_BYTES - (uintptr_t)c.n_small * (uintptr_t)c.bstride);
    m.add(&c.bhdr, (size_t)c.pool_cap * 4); m.add(&c.bfirst, (size_t)c.pool_cap * 3);
    m.add(&c.free_stack, (size_t)(c.pool_cap - c.n_small));
    m.add(&c.free_stack_s, n_small); m.add(&c.mig_list, n_small);
    m.add(&c.pc_key, n); m.add(&c.pc_pb, 32 * n); m.add(&c.pc_ans, GN8_ANS_ROW * n);
    m.add_pinned(&h->n_src_hint, 1);
    m.add(&c.gn_rows_ll, (size_t)2 * c.G * 64);
    m.add(&c.gn_xsum_ll, (size_t)2 * 8 * 8 * 64);
    m.add(&c.wg_clk, (size_t)c.G * 2 + DIAG_SLOTS);  // the per-workgroup clocks, then the named slots of the diagnostic builds (diag.h)
    m.add(&c.st, 1);
    h->traj_cap = traj_rows;
    c.traj_cap = (int)traj_rows;
    m.add(&c.traj, (size_t)traj_rows * 16);
    m.add(&c.sstats, (size_t)traj_rows);
    m.add((unsigned char**)&h->d_in, n * 3 * 8);
    m.add(&h->d_t01, n);
    m.add(&h->d_ext, 16);
    m.add(&h->d_counter, 4);
}
// traj_rows: the trajectory / statistics rows to start with (icp_traj_rows)
static int icp_create_impl(const ptl_icp_cfg* cfg, hipStream_t shared_stream, ptl_icp** out, bool batch_member = false, int64_t traj_rows = 4096) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "null argument");
    ABI_CHECK(ptl_icp_cfg, cfg);
    // the search maps one lane of a 32-lane group to one stored point of a voxel: more than 32 per voxel would be stored and never examined
    if (cfg->max_points_per_voxel < 1 || cfg->max_points_per_voxel > 32) return set_err(PTL_ERR_ARG, "max_points_per_voxel must be in [1, 32]");
    if (cfg->map_block_capacity < 1 || cfg->map_small_blocks < 0 || cfg->map_block_capacity + cfg->map_small_blocks >= (1 << 24) - 1)
        return set_err(PTL_ERR_ARG, "map_block_capacity + map_small_blocks must be below 2^24 - 1");
    if (cfg->map_small_blocks > 0 && !batch_member)
        return set_err(PTL_ERR_ARG, "map_small_blocks (two block classes) is served by the free-running batch driver only: a voxel's move to a full block is part of its map update");
    if (cfg->map_small_blocks > 0 && cfg->max_points_per_voxel < SMALL_CAP) return set_err(PTL_ERR_ARG, "map_small_blocks needs max_points_per_voxel >= %d", SMALL_CAP);
    if (cfg->map_table_capacity & (cfg->map_table_capacity - 1)) return set_err(PTL_ERR_ARG, "map_table_capacity must be a power of two");
    if (cfg->max_points_per_scan < 1 || cfg->gn_workgroups < 1 || cfg->gn_workgroups > 512) return set_err(PTL_ERR_ARG, "bad capacity (gn_workgroups must be in [1, 512])");
    if (cfg->max_iterations < 1 || cfg->max_iterations > 1000) return set_err(PTL_ERR_ARG, "max_iterations must be in [1, 1000]");
    if (cfg->gn_threads < 256 || cfg->gn_threads > GN_MAX_THREADS || (cfg->gn_threads & 63)) return set_err(PTL_ERR_ARG, "gn_threads must be a multiple of 64 in [256, GN_MAX_THREADS]");
    if (cfg->gn_lanes_per_point != 32 && cfg->gn_lanes_per_point != 8) return set_err(PTL_ERR_ARG, "gn_lanes_per_point must be 32 or 8");
    if (cfg->gn_lanes_per_point == 8 && cfg->gn_threads > GN8_MAX_THREADS) return set_err(PTL_ERR_ARG, "gn_lanes_per_point = 8 runs at most %d threads per workgroup", GN8_MAX_THREADS);
    if (ptl_device_count() <= cfg->device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", cfg->device_id);
    HIPCHK(hipSetDevice(cfg->device_id));
    {
        int per_cu = 0, cus = 0;
        hipError_t e = hipSuccess;
        pick_p(cfg->max_points_per_voxel, [&](auto pc) {  // (of the 8-lane kernel, the instance with the largest footprint)
            e = cfg->gn_lanes_per_point == 8 ? resident_capacity(k_gn_loop8<pc(), 0>, cfg->gn_threads, cfg->device_id, &per_cu, &cus)
                                             : resident_capacity(k_gn_loop<pc(), true>, cfg->gn_threads, cfg->device_id, &per_cu, &cus);
        });
        if (e != hipSuccess) return set_err(PTL_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));
        if ((int64_t)per_cu * cus < cfg->gn_workgroups)
            return set_err(PTL_ERR_STATE, "gn_workgroups = %d x %d threads cannot be co-resident on device %d (%d CUs x %d workgroups per CU): "
                           "lower gn_workgroups", cfg->gn_workgroups, cfg->gn_threads, cfg->device_id, cus, per_cu);
    }
    std::unique_ptr<ptl_icp> owner(new ptl_icp());  // (an error return below deletes the handle, and with it what it holds by then)
    ptl_icp* h = owner.get();
    icp_settle(h, cfg);
    if (shared_stream) h->stream.borrow(shared_stream);
    else if (h->stream.create() != hipSuccess) return set_err(PTL_ERR_HIP, "hipStreamCreate failed");
    Ctx& c = h->c;
    DevOwner& m = h->mem;
    icp_alloc(m, h, traj_rows);
    bool ok = m.err == hipSuccess && h->map_stream.create() == hipSuccess && h->ev_map.create() == hipSuccess && h->ev_gn.create() == hipSuccess;
    if (ok) *h->n_src_hint = 0;
    ok = ok && hipMemset(c.gn_rows_ll, 0, m.bytes_of(c.gn_rows_ll)) == hipSuccess && hipMemset(c.gn_xsum_ll, 0, m.bytes_of(c.gn_xsum_ll)) == hipSuccess &&
         hipMemset(c.wg_clk, 0, m.bytes_of(c.wg_clk)) == hipSuccess && hipMemset(c.st, 0, sizeof(DevState)) == hipSuccess;  // (IMU deskew off: k_state_init keeps its wiring)
    if (!ok) return set_err(PTL_ERR_HIP, "device allocation failed: %s", hipGetErrorString(m.err != hipSuccess ? m.err : hipGetLastError()));
    int rc = icp_reset_device(h);
    if (rc != PTL_OK) return rc;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return set_err(PTL_ERR_HIP, "init sync failed");
    *out = owner.release();
    return PTL_OK;
}
extern "C" int ptl_icp_create(const ptl_icp_cfg* cfg, ptl_icp** out) { return icp_create_impl(cfg, nullptr, out); }
extern "C" int ptl_icp_destroy(ptl_icp* h) { return h ? handle_destroy(h, h->cfg.device_id) : PTL_OK; }

static int icp_grow_traj(ptl_icp* h) {
    // doubles the trajectory / stats buffers (host-side decision: scans_done is known on the host)
    Ctx& c = h->c;
    const int64_t ncap = h->traj_cap * 2;
    double* nt = nullptr;
    ScanStats* ns = nullptr;
    DevOwner tmp;  // (the new rows are the handle's once the old ones are out of use)
    HIPCHK(tmp.alloc(&nt, (size_t)ncap * 16));
    HIPCHK(tmp.alloc(&ns, (size_t)ncap));
    HIPCHK(hipMemcpyAsync(nt, c.traj, (size_t)h->traj_cap * 16 * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(ns, c.sstats, (size_t)h->traj_cap * sizeof(ScanStats), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->map_stream));
    HIPCHK(hipDeviceSynchronize());  // (a sequence runner's EKF stream may still read the old trajectory rows)
    h->mem.replace(&c.traj, tmp, nt);
    h->mem.replace(&c.sstats, tmp, ns);
    h->traj_cap = ncap; c.traj_cap = (int)ncap;
    return PTL_OK;
}

static int map_rebuild(ptl_icp* h, hipStream_t s) {
    Ctx& c = h->c;
    HIPCHK(hipMemsetAsync(c.tab, 0xFF, ((size_t)c.tmask + 1) * sizeof(TabEnt), s));
    HIPCHK(hipMemsetAsync(&c.st->tab_used, 0, sizeof(unsigned), s));
    k_map_rebuild<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c);
    return PTL_OK;
}

// Enqueue one whole scan on the handle's stream (no host synchronisation):
// in_f32 / in_f64 / t01 / ext_guess are DEVICE pointers (one of in_* non-null).
struct ptl_lut {
    int device_id = 0, H = 0, W = 0;
    double *dir = nullptr, *off = nullptr;
    DevOwner mem;
};
static int icp_enqueue_scan(ptl_icp* h, const float* in_f32, const double* in_f64, const double* t01, int64_t n,
                            const double* ext_guess, const unsigned* in_range = nullptr, const ptl_lut* lut = nullptr) {
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "scan has %lld points, capacity %lld", (long long)n, (long long)h->n_max);
    if (h->scans_done >= h->traj_cap) { int rc = icp_grow_traj(h); if (rc) return rc; }
    Ctx c = h->c;
    c.in_f32 = in_f32; c.in_f64 = in_f64; c.t01 = t01; c.n_in = (int)n; c.ext_guess = ext_guess;
    c.in_range = in_range;
    if (in_range) {
        if (!lut || (int64_t)lut->H * lut->W != n || lut->W != c.W) return set_err(PTL_ERR_ARG, "range image needs a LUT of the same H x W (W = cfg.scan_cols)");
        c.lut_dir = lut->dir; c.lut_off = lut->off;
        c.row_mask = h->d_row_mask;
    }
    const int nb = (int)((n + 255) / 256) > 0 ? (int)((n + 255) / 256) : 1;
    hipStream_t s = h->stream;
    const int nb1 = (int)(((n > h->last_n ? n : h->last_n) + 255) / 256) > 0 ? (int)(((n > h->last_n ? n : h->last_n) + 255) / 256) : 1;
    // frame_down of this scan goes to the buffer the previous scan's map update is not reading
    c.fd = h->fd_buf[h->scans_done & 1];
    h->c.fd = c.fd;
    // K0-K4 on the main stream, right behind the previous GN kernel (no hand-over: a stream that has to wait for another
    // pays ~20 us of wake-up latency); beside them run the previous scan's map update (map stream) and, in the sequence
    // runner, the EKF step (its own stream) - both are done before this chain is, so the waits below do not block
    if (h->pro_wait) HIPCHK(hipStreamWaitEvent(s, h->pro_wait, 0));  // IMU deskew: the table needs the sweep's knots
    if (h->dk_wired) k_scan_prologue_imu<<<1, 1024, 0, s>>>(c);
    else k_scan_prologue<<<1, 1024, 0, s>>>(c);
    h->dk_rec.push_back(h->dk_wired ? (signed char)-1 : (signed char)((c.deskew && h->scans_done >= 2) ? DK_MODE_CV : DK_MODE_NONE));
    k_deskew_vds1<<<nb1, 256, 0, s>>>(c);
    k_count_w1<<<nb, 256, 0, s>>>(c);
    k_compact_fd<<<nb, 256, 0, s>>>(c);
    k_vds2_fd<<<nb, 256, 0, s>>>(c);  // (over the compact frame_downsample: blocks beyond N_d find nothing to do)
    k_count_w2<<<nb, 256, 0, s>>>(c);
    k_compact_src<<<nb, 256, 0, s>>>(c);
    if (h->ev_map_valid) HIPCHK(hipStreamWaitEvent(s, h->ev_map, 0));
    if (h->gn_wait) HIPCHK(hipStreamWaitEvent(s, h->gn_wait, 0));
    HIPCHK(h->prof.begin(s, (h->scans_done % h->prof_every) == 0));
    // ends with the post-ICP bookkeeping (kiss.py:116-128).  Dense scans (more source points than 32-lane groups) run the
    // variant that keeps probe results in memory; the previous scan's N_s, copied back without a wait, is the hint
    const bool dense = *h->n_src_hint > (int64_t)c.G * (h->cfg.gn_threads / 32);
    pick_p(c.P, [&](auto pc) {
        if (h->cfg.gn_lanes_per_point == 8) pick_team<32, 16, 8>(c.G, [&](auto gc) { k_gn_loop8<pc(), gc()><<<c.G, h->cfg.gn_threads, 0, s>>>(c, 0); });
        else if (dense) k_gn_loop<pc(), true><<<c.G, h->cfg.gn_threads, 0, s>>>(c, 0);
        else k_gn_loop<pc(), false><<<c.G, h->cfg.gn_threads, 0, s>>>(c, 0);
    });
    HIPCHK(h->prof.end(s));
    HIPCHK(hipEventRecord(h->ev_gn, s));
    h->ev_gn_valid = true;
    if (h->gn_done) HIPCHK(hipEventRecord(h->gn_done, s));
    // local_map.update(frame_downsample, new_pose)  (kiss.py:129), on the map stream
    hipStream_t sm = h->map_stream;
    HIPCHK(hipStreamWaitEvent(sm, h->ev_gn, 0));
    k_map_insert_a<<<nb, 256, 0, sm>>>(c, c.fd, &c.st->n_down_ins, 0, 1);
    k_map_insert_b<<<nb, 256, 0, sm>>>(c, &c.st->n_down_ins, 0);
    k_map_insert_c<<<nb, 256, 0, sm>>>(c, &c.st->n_down_ins, 0);
    k_map_prune<<<(c.pool_cap + 255) / 256, 256, 0, sm>>>(c, nullptr, 1);
    h->last_n = n;
    h->scans_done++;
    if (h->cfg.rebuild_every > 0 && (h->scans_done % h->cfg.rebuild_every) == 0) { int rc = map_rebuild(h, sm); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(h->n_src_hint, &c.st->n_src_last, sizeof(int), hipMemcpyDeviceToHost, sm));  // hint for the next launches
    HIPCHK(hipEventRecord(h->ev_map, sm));
    h->ev_map_valid = true;
    HIPCHK(hipGetLastError());
    return PTL_OK;
}

// Every entry point that touches the map, the device state or the handle's staging buffers (d_in, d_ext, fdw) on h->stream goes through
// this first: with lazy_map_stats a registration returns while its scan's map update (K7-K10, the rebuild) still runs on map_stream, and
// the sequence runner leaves one in flight too - work enqueued on h->stream must be ordered behind it (map_add / align /
// linear_system used to start beside it: two inserts on one table and pool, or a search over a half-inserted batch).
static int icp_join_map(ptl_icp* h) {
    if (h->ev_map_valid) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_map, 0));
    return PTL_OK;
}
static int icp_check_flags(ptl_icp* h) {
    int flags = 0;
    HIPCHK(hipStreamSynchronize(h->map_stream));  // the last scan's map update
    k_finish_scan<<<1, 64, 0, h->stream>>>(h->c);  // closes the last scan's bookkeeping (no-op when none is pending)
    HIPCHK(hipMemcpyAsync(&flags, &h->c.st->err_flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->prof.collect();
    if (flags) return set_err(PTL_ERR_CAPACITY, ERR_FLAGS_FMT, flags);
    return PTL_OK;
}

__global__ void k_finish_pose(Ctx c) {  // KissICP.poses.append of the scan just registered, WITHOUT the map statistics (its map update may still be running)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    finish_pending(c, c.st);
}
static void stats_out(const ScanStats& s, ptl_icp_stats* o);
// what follows the enqueue of a per-call registration: close the scan, bring pose and statistics row back, check the error flags.
// Default: after the scan's map update (map size is part of the row).  lazy_map_stats: as soon as the Gauss-Newton kernel is done -
// the map update (K7-K10, ~80 us) then runs beside the caller's next steps and the next call's upload and K0-K4; the row's map_voxels /
// map_points are -1 (ptl_icp_map_size gives them on demand) and an error flag raised by that update is reported by the next call.
static int icp_percall_finish(ptl_icp* h, double out_pose[16], ptl_icp_stats* stats) {
    const bool lazy = h->lazy_map_stats;
    if (!lazy && h->ev_map_valid) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_map, 0));  // map size is part of the row
    if (lazy) k_finish_pose<<<1, 64, 0, h->stream>>>(h->c);
    else k_finish_scan<<<1, 64, 0, h->stream>>>(h->c);  // close the scan before its stats row is read back
    const int64_t k = h->scans_done - 1;
    double pose[16];
    ScanStats ss;
    int flags = 0;
    HIPCHK(hipMemcpyAsync(pose, h->c.traj + 16 * k, sizeof pose, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&ss, h->c.sstats + k, sizeof ss, hipMemcpyDeviceToHost, h->stream));
    int rc = PTL_OK;
    if (lazy) {
        HIPCHK(hipMemcpyAsync(&flags, &h->c.st->err_flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->prof.collect();
        if (flags) rc = set_err(PTL_ERR_CAPACITY, ERR_FLAGS_FMT, flags);
        ss.map_voxels = -1; ss.map_points = -1;
    } else {
        rc = icp_check_flags(h);
    }
    if (rc) return rc;
    if (out_pose) memcpy(out_pose, pose, sizeof pose);
    if (stats) stats_out(ss, stats);
    return PTL_OK;
}
extern "C" int ptl_icp_set_lazy_map_stats(ptl_icp* h, int32_t on) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    h->lazy_map_stats = on != 0;
    return PTL_OK;
}
static void stats_out(const ScanStats& s, ptl_icp_stats* o) {
    o->sigma = s.sigma; o->err_dt = s.err_dt; o->err_drot = s.err_drot;
    o->iterations = s.iterations; o->n_corr_last = s.n_corr_last; o->n_in = s.n_in; o->n_valid = s.n_valid;
    o->n_down = s.n_down; o->n_src = s.n_src; o->sum_cand = s.sum_cand; o->map_voxels = s.map_voxels;
    o->map_points = s.map_points;
}

extern "C" int ptl_icp_register_frame(ptl_icp* h, const void* xyz, int dtype, int64_t n, const double* t01,
                                      double scan_ts, const double* guess, double out_pose[16], ptl_icp_stats* stats) {
    (void)scan_ts;
    if (!h || (!xyz && n > 0) || n < 0) return set_err(PTL_ERR_ARG, "bad argument");
    if (dtype != PTL_F32 && dtype != PTL_F64) return set_err(PTL_ERR_ARG, "dtype must be PTL_F32 or PTL_F64");
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "scan has %lld points, capacity %lld", (long long)n, (long long)h->n_max);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    const size_t esz = dtype == PTL_F32 ? 4 : 8;
    if (n) HIPCHK(hipMemcpyAsync(h->d_in, xyz, (size_t)n * 3 * esz, hipMemcpyHostToDevice, h->stream));
    if (t01 && n) HIPCHK(hipMemcpyAsync(h->d_t01, t01, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    if (guess) HIPCHK(hipMemcpyAsync(h->d_ext, guess, 16 * 8, hipMemcpyHostToDevice, h->stream));
    int rc = icp_enqueue_scan(h, dtype == PTL_F32 ? (const float*)h->d_in : nullptr,
                              dtype == PTL_F64 ? (const double*)h->d_in : nullptr, t01 ? h->d_t01 : nullptr, n,
                              guess ? h->d_ext : nullptr);
    if (rc) return rc;
    return icp_percall_finish(h, out_pose, stats);
}

extern "C" int ptl_icp_num_poses(ptl_icp* h, int64_t* n) {
    if (!h || !n) return set_err(PTL_ERR_ARG, "null argument");
    *n = h->scans_done;
    return PTL_OK;
}
extern "C" int ptl_icp_get_poses(ptl_icp* h, double* out, int64_t max_poses, int64_t* n_written) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    const int64_t n = h->scans_done < max_poses ? h->scans_done : max_poses;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    if (n > 0) HIPCHK(hipMemcpyAsync(out, h->c.traj, (size_t)n * 16 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_written) *n_written = n;
    return PTL_OK;
}
__global__ void k_prediction(const DevState* st, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    Rt p = (st->n_poses >= 2) ? rt_mul(rt_inv(rt_from16(st->pose_prev)), rt_from16(st->pose_last)) : rt_identity();
    rt_to16(p, out);
}
extern "C" int ptl_icp_get_prediction(ptl_icp* h, double out[16]) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int rcj = icp_join_map(h); if (rcj) return rcj; }
    k_prediction<<<1, 64, 0, h->stream>>>(h->c.st, h->d_ext);
    HIPCHK(hipMemcpyAsync(out, h->d_ext, 16 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
extern "C" int ptl_icp_map_size(ptl_icp* h, int64_t* voxels, int64_t* points) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    DevState st;
    HIPCHK(hipStreamSynchronize(h->map_stream));  // (a map update may still be under way: lazy_map_stats, the sequence runner)
    HIPCHK(hipMemcpyAsync(&st, h->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (voxels) *voxels = st.n_live;
    if (points) *points = st.map_points;
    return PTL_OK;
}
extern "C" int ptl_icp_map_points(ptl_icp* h, double* xyz_out, int64_t max_points, int64_t* n_written) {
    if (!h || !xyz_out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    double* d_out = nullptr;
    HIPCHK(hipStreamSynchronize(h->map_stream));  // (a map update may still be under way)
    DevOwner tmp;
    HIPCHK(tmp.alloc(&d_out, (size_t)(max_points > 0 ? max_points : 1) * 3));
    HIPCHK(hipMemsetAsync(h->d_counter, 0, sizeof(int), h->stream));
    k_map_export<<<(h->c.pool_cap + 255) / 256, 256, 0, h->stream>>>(h->c, d_out, h->d_counter, (int)max_points);
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, h->d_counter, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t n = cnt < max_points ? cnt : max_points;
    if (n > 0) HIPCHK(hipMemcpy(xyz_out, d_out, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
    if (n_written) *n_written = n;
    return PTL_OK;
}
static int copy_cloud(ptl_icp* h, const double* d_src, const int* d_n, double* out, int64_t max_points, int64_t* n_written) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, d_n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t m = n < max_points ? n : max_points;
    if (m > 0) HIPCHK(hipMemcpy(out, d_src, (size_t)m * 3 * 8, hipMemcpyDeviceToHost));
    if (n_written) *n_written = m;
    return PTL_OK;
}
extern "C" int ptl_icp_last_frame_down(ptl_icp* h, double* out, int64_t max_points, int64_t* n_written) {
    return copy_cloud(h, h ? h->c.fd : nullptr, h ? &h->c.st->n_down_ins : nullptr, out, max_points, n_written);
}
extern "C" int ptl_icp_last_source(ptl_icp* h, double* out, int64_t max_points, int64_t* n_written) {
    return copy_cloud(h, h ? h->c.src0 : nullptr, h ? &h->c.st->n_src_last : nullptr, out, max_points, n_written);
}

extern "C" int ptl_icp_deskew(ptl_icp* h, const double* xyz, const double* t01, int64_t n, double* out) {
    if (!h || (!xyz && n > 0) || (!t01 && n > 0) || !out || n < 0) return set_err(PTL_ERR_ARG, "bad argument");
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "too many points");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    if (n == 0) return PTL_OK;
    { int rcj = icp_join_map(h); if (rcj) return rcj; }  // (the result is staged in fdw, which insert b of a running map update still reads)
    k_finish_scan<<<1, 64, 0, h->stream>>>(h->c);
    HIPCHK(hipMemcpyAsync(h->d_in, xyz, (size_t)n * 24, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_t01, t01, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    k_deskew_only<<<(int)((n + 255) / 256), 256, 0, h->stream>>>(h->c, (const double*)h->d_in, h->d_t01, (int)n, h->c.fdw);
    HIPCHK(hipMemcpyAsync(out, h->c.fdw, (size_t)n * 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
extern "C" int ptl_icp_map_add(ptl_icp* h, const double* xyz_world, int64_t n, const double origin[3], int prune) {
    if (!h || (!xyz_world && n > 0)) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    Ctx& c = h->c;
    hipStream_t s = h->stream;
    { int rcj = icp_join_map(h); if (rcj) return rcj; }
    for (int64_t off = 0; off < n; off += h->n_max) {  // batches keep scan order: earlier batch = earlier points
        const int m = (int)((n - off) < h->n_max ? (n - off) : h->n_max);
        HIPCHK(hipMemcpyAsync(h->d_in, xyz_world + 3 * off, (size_t)m * 24, hipMemcpyHostToDevice, s));
        const int nb = (m + 255) / 256;
        k_map_insert_a<<<nb, 256, 0, s>>>(c, (const double*)h->d_in, nullptr, m, 0);
        k_map_insert_b<<<nb, 256, 0, s>>>(c, nullptr, m);
        k_map_insert_c<<<nb, 256, 0, s>>>(c, nullptr, m);
    }
    if (prune && origin) {
        HIPCHK(hipMemcpyAsync(h->d_ext, origin, 24, hipMemcpyHostToDevice, s));
        k_map_prune<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, h->d_ext, 0);
    }
    return icp_check_flags(h);
}

__global__ void k_set_gn(Ctx c, int n_src, double max_dist, double kernel, const double* guess) {
    DevState* st = c.st;
    if (threadIdx.x == 0) {
        st->n_src = n_src; st->gn_max_dist = max_dist; st->gn_kernel = kernel;
        st->gn_epoch = (st->gn_epoch + 1u) & 0x3FFFFFu;
        st->gn_abort = 0;
        if (guess) for (int i = 0; i < 16; ++i) st->guess[i] = guess[i];
        __threadfence_block();
    }
    __syncthreads();
    gn_ll_clear_on_wrap(c);
}
extern "C" int ptl_icp_linear_system(ptl_icp* h, const double* src_world, int64_t n, double max_dist, double kernel,
                                     double sums[27], int64_t* n_corr, int64_t* n_cand) {
    if (!h || !src_world || !sums) return set_err(PTL_ERR_ARG, "null argument");
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "too many points");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    Ctx& c = h->c;
    { int rcj = icp_join_map(h); if (rcj) return rcj; }
    HIPCHK(hipMemcpyAsync(c.src_cur, src_world, (size_t)n * 24, hipMemcpyHostToDevice, h->stream));
    k_set_gn<<<1, 64, 0, h->stream>>>(c, (int)n, max_dist, kernel, nullptr);
    pick_p(c.P, [&](auto pc) { k_gn_loop<pc(), false><<<c.G, h->cfg.gn_threads, 0, h->stream>>>(c, 1); });
    double out[32];
    HIPCHK(hipMemcpyAsync(out, (char*)c.st + offsetof(DevState, lin_sums), sizeof out, hipMemcpyDeviceToHost, h->stream));
    int rc = icp_check_flags(h);
    if (rc) return rc;
    memcpy(sums, out, 27 * 8);
    if (n_corr) *n_corr = (int64_t)out[27];
    if (n_cand) *n_cand = (int64_t)out[28];
    return PTL_OK;
}
extern "C" int ptl_icp_align(ptl_icp* h, const double* frame, int64_t n, const double guess[16], double max_dist,
                             double kernel, double out_pose[16], int32_t* iterations) {
    if (!h || !frame || !guess || !out_pose) return set_err(PTL_ERR_ARG, "null argument");
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "too many points");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    Ctx& c = h->c;
    { int rcj = icp_join_map(h); if (rcj) return rcj; }
    HIPCHK(hipMemcpyAsync(c.src0, frame, (size_t)n * 24, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ext, guess, 128, hipMemcpyHostToDevice, h->stream));
    k_set_gn<<<1, 64, 0, h->stream>>>(c, (int)n, max_dist, kernel, h->d_ext);
    pick_p(c.P, [&](auto pc) { k_gn_loop<pc(), false><<<c.G, h->cfg.gn_threads, 0, h->stream>>>(c, 2); });  // new_pose = T_icp * guess, trajectory untouched
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    int rc = icp_check_flags(h);
    if (rc) return rc;
    memcpy(out_pose, st.new_pose, 128);
    if (iterations) *iterations = st.gn_iters;
    return PTL_OK;
}

// test hook: set the launch epoch of the Gauss-Newton exchange (its 22-bit wrap-around is otherwise 4 million scans away)
__global__ void k_set_epoch(DevState* st, unsigned v) { if (threadIdx.x == 0 && blockIdx.x == 0) st->gn_epoch = v & 0x3FFFFFu; }
extern "C" int ptl_icp_debug_set_epoch(ptl_icp* h, uint32_t epoch) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    int rc = icp_check_flags(h);
    if (rc) return rc;
    k_set_epoch<<<1, 64, 0, h->stream>>>(h->c.st, epoch);
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

// test hook: workgroup `wg` of the following Gauss-Newton launches returns at once (-1: back to normal).  The others run into
// the exchange time-out, raise the abort word and leave; the call that synchronises next reports the error flag.
__global__ void k_set_dead_wg(DevState* st, int wg) { if (threadIdx.x == 0 && blockIdx.x == 0) { st->dbg_dead_wg = wg; st->err_flags &= ~ERR_GN_TIMEOUT; } }
extern "C" int ptl_icp_debug_stall_workgroup(ptl_icp* h, int32_t wg) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->map_stream));
    k_set_dead_wg<<<1, 64, 0, h->stream>>>(h->c.st, wg);
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

// test hook: leave the handle's block pool with at most `free_blocks` free blocks (< 0: unchanged) and / or declare `table_used`
// entries of its map table taken (< 0: unchanged) - the next map updates then run into ERR_POOL / ERR_TABLE, which the call
// that synchronises next reports as PTL_ERR_CAPACITY
__global__ void k_limit_capacity(DevState* st, int free_blocks, long long table_used) {
    if (threadIdx.x || blockIdx.x) return;
    if (free_blocks >= 0 && st->free_top > free_blocks) st->free_top = free_blocks;
    if (table_used >= 0) st->tab_used = (unsigned)table_used;
}
extern "C" int ptl_icp_debug_limit_capacity(ptl_icp* h, int32_t free_blocks, int64_t table_used) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->map_stream));
    k_limit_capacity<<<1, 64, 0, h->stream>>>(h->c.st, free_blocks, (long long)table_used);
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

// test hook: the handle's map table, block directory and table counters as they are, copied to the host.  Waits for the map stream and the
// main stream, launches no kernel, writes nothing on the device and reports no error flag as an error (it returns the word)
extern "C" int ptl_icp_debug_table(ptl_icp* h, void* entries, int64_t max_slots, int32_t* bhdr, double* bfirst, int64_t max_blocks, int64_t info[8]) {
    if (!h || !info) return set_err(PTL_ERR_ARG, "null argument");
    const Ctx& c = h->c;
    const int64_t slots = (int64_t)c.tmask + 1;
    if ((entries && max_slots < slots) || ((bhdr || bfirst) && max_blocks < c.pool_cap))
        return set_err(PTL_ERR_CAPACITY, "the table has %lld slots and the directory %d blocks", (long long)slots, c.pool_cap);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->map_stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    DevState st;
    HIPCHK(hipMemcpy(&st, c.st, sizeof st, hipMemcpyDeviceToHost));
    if (entries) HIPCHK(hipMemcpy(entries, c.tab, (size_t)slots * sizeof(TabEnt), hipMemcpyDeviceToHost));
    if (bhdr) HIPCHK(hipMemcpy(bhdr, c.bhdr, (size_t)c.pool_cap * 4 * sizeof(int), hipMemcpyDeviceToHost));
    if (bfirst) HIPCHK(hipMemcpy(bfirst, c.bfirst, (size_t)c.pool_cap * 3 * sizeof(double), hipMemcpyDeviceToHost));
    info[0] = (int64_t)st.tab_used; info[1] = st.n_live; info[2] = st.err_flags; info[3] = (int64_t)c.tmask;
    info[4] = (int64_t)c.vmask; info[5] = (int64_t)c.vmask2; info[6] = c.pool_cap; info[7] = c.n_small;
    return PTL_OK;
}

// diagnostic: ticks every GN workgroup spent in the search phase since creation: out[0..G) until its last wavefront
// finished, out[G..2G) its first wavefront
extern "C" int ptl_icp_gn_wg_clocks(ptl_icp* h, int64_t* out, int32_t max_wgs) {
    if (!h || !out || max_wgs < h->c.G) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(out, h->c.wg_clk, (size_t)h->c.G * 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

// diagnostic: what the handle's last ptl_icp_linear_system left on the device: the 27 sums, the pair count, the candidate count (nothing else
// is kept there: the diagnostic builds' values are read with ptl_icp_diag)
extern "C" int ptl_icp_debug_sums(ptl_icp* h, double out[32]) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(out, (char*)h->c.st + offsetof(DevState, lin_sums), 256, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
// diagnostic: the named slots of diag.h (all 0 in the product build), cumulative since the handle's cold start
extern "C" int ptl_diag_slots(void) { return DIAG_SLOTS; }
extern "C" const char* ptl_diag_slot_name(int slot) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (const DiagSlotName& e : DIAG_SLOT_NAMES)
            for (int k = 0; k < e.words; ++k) v.push_back(e.words == 1 ? std::string(e.base) : std::string(e.base) + "_" + std::to_string(k));
        return v;
    }();
    return slot >= 0 && slot < (int)names.size() ? names[slot].c_str() : nullptr;
}
extern "C" int ptl_icp_diag(ptl_icp* h, int64_t* out, int32_t max_slots) {
    if (!h || !out || max_slots < DIAG_SLOTS) return set_err(PTL_ERR_ARG, "bad argument (ptl_diag_slots() words are written)");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(out, h->c.wg_clk + 2 * h->c.G, DIAG_SLOTS * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
// diagnostic: accumulated per-phase clock ticks of workgroup 0 in the GN loop since the handle was reset
// out[0..4] = nn, wg-reduce+publish, barrier, grid-reduce, solve; out[5] = iterations
extern "C" int ptl_icp_gn_phases(ptl_icp* h, int64_t out[8]) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(out, (char*)h->c.st + offsetof(DevState, gn_phase_clk), 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

extern "C" int ptl_icp_profile(ptl_icp* h, int enable, double* gn_ms_total, int64_t* gn_launches, int reset) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->prof.report(enable, gn_ms_total, gn_launches, reset);
    h->prof_every = enable > 1 ? enable : 1;
    return PTL_OK;
}

// ------------------------------------------------------------------------------------------------ range-image input
extern "C" int ptl_lut_create(int device_id, int32_t H, int32_t W, const double* beam_altitude_deg,
                              const double* beam_azimuth_deg, double lidar_origin_to_beam_origin_mm,
                              const double* lidar_to_sensor16_mm, const double* extrinsic16_m, ptl_lut** out) {
    if (!beam_altitude_deg || !beam_azimuth_deg || !lidar_to_sensor16_mm || !out || H < 1 || W < 1) return set_err(PTL_ERR_ARG, "bad argument");
    if (ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    // total transform in millimetres: extrinsic (metres -> mm) * lidar_to_sensor
    double T[16];
    memcpy(T, lidar_to_sensor16_mm, sizeof T);
    if (extrinsic16_m) {
        double E[16], R[16];
        memcpy(E, extrinsic16_m, sizeof E);
        E[3] *= 1e3; E[7] *= 1e3; E[11] *= 1e3;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += E[4 * i + k] * T[4 * k + j];
                R[4 * i + j] = s;
            }
        memcpy(T, R, sizeof T);
    }
    std::unique_ptr<ptl_lut> l(new ptl_lut());  // (an error return below deletes it, and with it what it has allocated)
    l->device_id = device_id; l->H = H; l->W = W;
    double* d_tmp = nullptr;
    DevOwner tmp;
    const size_t n = (size_t)H * W;
    l->mem.add(&l->dir, 3 * n); l->mem.add(&l->off, 3 * n); tmp.add(&d_tmp, (size_t)2 * H + 16);
    if (l->mem.err != hipSuccess || tmp.err != hipSuccess) return set_err(PTL_ERR_HIP, "LUT allocation failed");
    HIPCHK(hipMemcpy(d_tmp, beam_altitude_deg, (size_t)H * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tmp + H, beam_azimuth_deg, (size_t)H * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tmp + 2 * H, T, sizeof T, hipMemcpyHostToDevice));
    k_build_lut<<<(int)((n + 255) / 256), 256>>>(H, W, d_tmp, d_tmp + H, lidar_origin_to_beam_origin_mm, d_tmp + 2 * H, l->dir, l->off);
    HIPCHK(hipDeviceSynchronize());
    *out = l.release();
    return PTL_OK;
}
extern "C" int ptl_lut_destroy(ptl_lut* l) { return l ? handle_destroy(l, l->device_id) : PTL_OK; }
// XYZLut.__call__: range image -> (H*W, 3) f64 xyz in metres (RANGE == 0 -> (0,0,0))
__global__ __launch_bounds__(256) void k_lut_apply(int n, const unsigned* range, const double* dir, const double* off, double* xyz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned rg = range[i];
    const double r = (double)rg;
    for (int k = 0; k < 3; ++k) xyz[3 * (size_t)i + k] = rg ? r * dir[3 * (size_t)i + k] + off[3 * (size_t)i + k] : 0.0;
}
extern "C" int ptl_lut_apply(ptl_lut* l, const uint32_t* range_mm, double* xyz_out) {
    if (!l || !range_mm || !xyz_out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(l->device_id));
    const size_t n = (size_t)l->H * l->W;
    unsigned* d_r = nullptr;
    double* d_x = nullptr;
    DevOwner tmp;
    HIPCHK(tmp.alloc(&d_r, n));
    HIPCHK(tmp.alloc(&d_x, 3 * n));
    HIPCHK(hipMemcpy(d_r, range_mm, n * 4, hipMemcpyHostToDevice));
    k_lut_apply<<<(int)((n + 255) / 256), 256>>>((int)n, d_r, l->dir, l->off, d_x);
    HIPCHK(hipMemcpy(xyz_out, d_x, n * 24, hipMemcpyDeviceToHost));
    return PTL_OK;
}
// rows np.linspace(0, H, beams_num, endpoint=False, dtype=int), that is (int)(i * (H / beams_num)), marked 1 among H
static std::vector<unsigned char> beam_mask(int H, int beams_num) {
    std::vector<unsigned char> m((size_t)H, 0);
    const double step = (double)H / (double)beams_num;
    for (int i = 0; i < beams_num; ++i) {
        const int r = (int)((double)i * step);
        if (r >= 0 && r < H) m[(size_t)r] = 1;
    }
    return m;
}
// StreamStatsTracker.trackScan's reduction (reference ins/data.py:284-308) on a range image given by the host
extern "C" int ptl_range_stats(int device_id, const uint32_t* range, int32_t H, int32_t W, int32_t beams_num,
                               double range_to_m, double out5[5]) {
    if (!range || !out5 || H < 1 || W < 1) return set_err(PTL_ERR_ARG, "bad argument");
    if (ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    const size_t n = (size_t)H * W;
    unsigned* d_r = nullptr;
    unsigned char* d_m = nullptr;
    double* d_o = nullptr;
    DevOwner tmp;
    HIPCHK(tmp.alloc(&d_r, n));
    HIPCHK(tmp.alloc(&d_o, 5));
    HIPCHK(hipMemcpy(d_r, range, n * 4, hipMemcpyHostToDevice));
    if (beams_num > 0) {  // (:288-293)
        HIPCHK(tmp.alloc(&d_m, (size_t)H));
        HIPCHK(hipMemcpy(d_m, beam_mask(H, beams_num).data(), (size_t)H, hipMemcpyHostToDevice));
    }
    k_range_stats<<<1, 1024>>>(d_r, H, W, d_m, range_to_m, d_o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out5, d_o, 40, hipMemcpyDeviceToHost));
    return PTL_OK;
}
// reduce_active_beams (reference utils.py:328-341): rows np.linspace(0, H, beams, endpoint=False, dtype=int) stay
// active, every other row's RANGE is treated as 0.  beams_num <= 0 re-enables all rows.
extern "C" int ptl_icp_set_active_beams(ptl_icp* h, int32_t H, int32_t beams_num) {
    if (!h || H < 1) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mem.release(&h->d_row_mask);
    if (beams_num <= 0) return PTL_OK;
    HIPCHK(h->mem.alloc(&h->d_row_mask, (size_t)H));
    HIPCHK(hipMemcpy(h->d_row_mask, beam_mask(H, beams_num).data(), (size_t)H, hipMemcpyHostToDevice));
    return PTL_OK;
}
// KissICPWrapper.register_frame on a raw range image (reference kiss.py:54-74): XYZLut + RANGE != 0 mask + pipeline
extern "C" int ptl_icp_register_range(ptl_icp* h, ptl_lut* lut, const uint32_t* range_mm, double scan_ts,
                                      const double* guess, double out_pose[16], ptl_icp_stats* stats) {
    (void)scan_ts;
    if (!h || !lut || !range_mm) return set_err(PTL_ERR_ARG, "null argument");
    const int64_t n = (int64_t)lut->H * lut->W;
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "scan has %lld points, capacity %lld", (long long)n, (long long)h->n_max);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(h->d_in, range_mm, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (guess) HIPCHK(hipMemcpyAsync(h->d_ext, guess, 16 * 8, hipMemcpyHostToDevice, h->stream));
    int rc = icp_enqueue_scan(h, nullptr, nullptr, nullptr, n, guess ? h->d_ext : nullptr, (const unsigned*)h->d_in, lut);
    if (rc) return rc;
    return icp_percall_finish(h, out_pose, stats);
}

// ------------------------------------------------------------------------------------------------ posed scans (flyby)
// Poses along a time-stamped trajectory (fly_kernels.h d_traj_pose_at); a timestamp outside the bounds gets the identity and is counted.
// One thread per timestamp.
__global__ __launch_bounds__(256) void k_traj_poses_at(const double* kt, const double* kp, int n, double before, double after,
                                                       const double* ts, int m, double* out, int* n_outside) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    Rt P;
    if (!d_traj_pose_at(kt, kp, n, before, after, ts[j], &P)) {
        atomicAdd(n_outside, 1);
        for (int k = 0; k < 16; ++k) out[16 * (size_t)j + k] = (k % 5 == 0) ? 1.0 : 0.0;
        return;
    }
    rt_to16(P, out + 16 * (size_t)j);
}
extern "C" int ptl_traj_poses_at(int device_id, const double* knot_ts, const double* knot_poses16, int64_t n_knots,
                                 double bound_before, double bound_after, const double* ts, int64_t n, double* poses16_out,
                                 int64_t* n_outside) {
    if (!knot_ts || !knot_poses16 || !ts || !poses16_out || n_knots < 2 || n < 0) return set_err(PTL_ERR_ARG, "bad argument (a trajectory needs >= 2 knots)");
    for (int64_t i = 1; i < n_knots; ++i)
        if (!(knot_ts[i] > knot_ts[i - 1])) return set_err(PTL_ERR_ARG, "knot timestamps must increase strictly (knot %lld)", (long long)i);
    if (ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    if (n_outside) *n_outside = 0;
    if (n == 0) return PTL_OK;
    double *d_kt = nullptr, *d_kp = nullptr, *d_ts = nullptr, *d_out = nullptr;
    int* d_cnt = nullptr;
    DevOwner tmp;
    tmp.add(&d_kt, (size_t)n_knots); tmp.add(&d_kp, (size_t)n_knots * 16);
    tmp.add(&d_ts, (size_t)n); tmp.add(&d_out, (size_t)n * 16); tmp.add(&d_cnt, 1);
    HIPCHK(tmp.err);
    HIPCHK(hipMemcpy(d_kt, knot_ts, (size_t)n_knots * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_kp, knot_poses16, (size_t)n_knots * 128, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ts, ts, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_cnt, 0, sizeof(int)));
    int outside = 0;
    k_traj_poses_at<<<(int)((n + 255) / 256), 256>>>(d_kt, d_kp, (int)n_knots, bound_before, bound_after, d_ts, (int)n, d_out, d_cnt);
    HIPCHK(hipMemcpy(poses16_out, d_out, (size_t)n * 128, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&outside, d_cnt, sizeof(int), hipMemcpyDeviceToHost));
    if (n_outside) *n_outside = outside;
    return PTL_OK;
}
// ouster client.dewarp(XYZLut(scan), column_poses = scan.pose) (what ScansAccumulator does with a posed scan, reference
// fly.py:75-86): pixel (u, v) -> R_v (range dir + off) + t_v with the pose of ITS column.  As upstream, pixels without a
// return (range 0 -> xyz 0) land on their column's sensor origin; n_valid counts the others.  The arithmetic: fly_kernels.h.
__global__ __launch_bounds__(256) void k_dewarp(int H, int W, const unsigned* range, const double* dir, const double* off,
                                                const double* col_poses, double* xyz, int* n_valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (i < H * W) {
        const unsigned rg = range[i];
        const Rt P = rt_from16(col_poses + 16 * (size_t)(i % W));
        double p[3], M[12], w[3];
        for (int k = 0; k < 9; ++k) M[k] = P.R[k];
        for (int k = 0; k < 3; ++k) M[9 + k] = P.t[k];
        d_lut_pixel(rg, dir, off, (size_t)i, p);
        d_pose_pixel(M, p, w);
        for (int k = 0; k < 3; ++k) xyz[3 * (size_t)i + k] = w[k];
        valid = rg != 0;
    }
    const int nv = __syncthreads_count(valid ? 1 : 0);
    if (threadIdx.x == 0 && nv) atomicAdd(n_valid, nv);
}
extern "C" int ptl_lut_dewarp(ptl_lut* l, const uint32_t* range_mm, const double* col_poses16, double* xyz_out, int64_t* n_valid) {
    if (!l || !range_mm || !col_poses16 || !xyz_out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(l->device_id));
    const size_t n = (size_t)l->H * l->W;
    unsigned* d_r = nullptr;
    double *d_x = nullptr, *d_p = nullptr;
    int* d_c = nullptr;
    DevOwner tmp;
    tmp.add(&d_r, n); tmp.add(&d_x, 3 * n); tmp.add(&d_p, (size_t)l->W * 16); tmp.add(&d_c, 1);
    HIPCHK(tmp.err);
    HIPCHK(hipMemcpy(d_r, range_mm, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_p, col_poses16, (size_t)l->W * 128, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_c, 0, sizeof(int)));
    int cnt = 0;
    k_dewarp<<<(int)((n + 255) / 256), 256>>>(l->H, l->W, d_r, l->dir, l->off, d_p, d_x, d_c);
    HIPCHK(hipMemcpy(xyz_out, d_x, n * 24, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&cnt, d_c, sizeof(int), hipMemcpyDeviceToHost));
    if (n_valid) *n_valid = cnt;
    return PTL_OK;
}

// ================================================================================================ EKF
struct ptl_ekf {
    ptl_ekf_cfg cfg;
    Stream stream;  // its own, or borrowed from the runner it is a member of
    EkfState* st = nullptr;
    double* d_buf = nullptr;  // staging: imu rows / pose / cov
    int64_t buf_rows = 1024;
    // fixed-interval smoother (ptl_ekf_log_enable): the history log in HBM, the backward pass's outputs, its job and status words
    double* d_log = nullptr;
    int64_t log_cap = 0;
    double* d_sm = nullptr;  // [cap][16] poses | [cap] t | [cap][19] nav | [cap][324] P^s
    EkfSmoothJob job = {};
    EkfSmoothJob* d_job = nullptr;
    long long* d_info = nullptr;
    // IMU deskew knot list (ptl_ekf_knots_enable)
    double* d_knots = nullptr;
    int64_t knot_cap = 0;
    DevOwner mem;
};

extern "C" int ptl_ekf_default_cfg(ptl_ekf_cfg* cfg) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_ekf_cfg, cfg);
    PTL_CFG_INIT(cfg);
    cfg->init_grav[2] = -9.782940329221166;  // GRAV * DOWN (es_ekf.py:75, ins/data.py:10)
    return PTL_OK;
}
static int ekf_reset(ptl_ekf* h) {
    HIPCHK(hipMemcpyAsync(h->d_buf, h->cfg.init_grav, 24, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_buf + 3, h->cfg.init_bacc, 24, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_buf + 6, h->cfg.init_bgyr, 24, hipMemcpyHostToDevice, h->stream));
    k_ekf_init<<<1, 64, 0, h->stream>>>(h->st, h->d_buf, h->d_buf + 3, h->d_buf + 6);
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// the device buffers a filter is created with: `m` allocates them (h->mem) or only counts their bytes
static void ekf_alloc(DevOwner& m, ptl_ekf* h) {
    m.add(&h->st, 1);
    m.add(&h->d_buf, (size_t)h->buf_rows * 7 + 64);
}
static int ekf_create_impl(const ptl_ekf_cfg* cfg, hipStream_t shared, ptl_ekf** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "null argument");
    ABI_CHECK(ptl_ekf_cfg, cfg);
    if (ptl_device_count() <= cfg->device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", cfg->device_id);
    HIPCHK(hipSetDevice(cfg->device_id));
    std::unique_ptr<ptl_ekf> owner(new ptl_ekf());
    ptl_ekf* h = owner.get();
    h->cfg = *cfg;
    if (shared) h->stream.borrow(shared);
    else if (h->stream.create() != hipSuccess) return set_err(PTL_ERR_HIP, "stream");
    ekf_alloc(h->mem, h);
    int rc = h->mem.err == hipSuccess ? PTL_OK : set_err(PTL_ERR_HIP, "device allocation failed");
    if (rc == PTL_OK && hipMemsetAsync(h->st, 0, sizeof(EkfState), h->stream) != hipSuccess) rc = set_err(PTL_ERR_HIP, "memset");  // smoother log off
    if (rc == PTL_OK) rc = ekf_reset(h);
    if (rc == PTL_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = set_err(PTL_ERR_HIP, "sync");
    if (rc) return rc;
    *out = owner.release();
    return PTL_OK;
}
extern "C" int ptl_ekf_create(const ptl_ekf_cfg* cfg, ptl_ekf** out) { return ekf_create_impl(cfg, nullptr, out); }
extern "C" int ptl_ekf_destroy(ptl_ekf* h) { return h ? handle_destroy(h, h->cfg.device_id) : PTL_OK; }
// n IMU rows -> the filter's predicts, staged through d_buf buf_rows at a time with a wait for the buffer's reuse; wait_last = false leaves
// the last buf_rows or fewer in flight for the caller's own wait
static int ekf_stage_imu(ptl_ekf* h, const double* imu, int64_t n, bool wait_last) {
    for (int64_t off = 0; off < n; off += h->buf_rows) {
        const int m = (int)((n - off) < h->buf_rows ? (n - off) : h->buf_rows);
        HIPCHK(hipMemcpyAsync(h->d_buf, imu + 7 * off, (size_t)m * 56, hipMemcpyHostToDevice, h->stream));
        k_ekf_step<<<1, EKF_THREADS, 0, h->stream>>>(h->st, h->d_buf, 0, m, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
        if (wait_last || off + m < n) HIPCHK(hipStreamSynchronize(h->stream));
    }
    return PTL_OK;
}
extern "C" int ptl_ekf_process_imu_batch(ptl_ekf* h, const double* imu, int64_t n) {
    if (!h || (!imu && n > 0)) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    const int rc = ekf_stage_imu(h, imu, n, true);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
extern "C" int ptl_ekf_process_imu(ptl_ekf* h, const double lacc[3], const double avel[3], double ts) {
    if (!h || !lacc || !avel) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    const EkfRow7 row = {{ts, lacc[0], lacc[1], lacc[2], avel[0], avel[1], avel[2]}};
    k_ekf_imu_value<<<1, 384, 0, h->stream>>>(h->st, row);  // asynchronous: the getters synchronise
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
extern "C" int ptl_ekf_process_pose(ptl_ekf* h, const double pose[16], const double* meas_cov36) {
    if (!h || !pose) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    EkfPoseArg a;
    memcpy(a.pose, pose, sizeof a.pose);
    a.has_cov = meas_cov36 ? 1 : 0;
    if (meas_cov36) memcpy(a.cov, meas_cov36, sizeof a.cov); else memset(a.cov, 0, sizeof a.cov);
    k_ekf_pose_value<<<1, 384, 0, h->stream>>>(h->st, a);  // asynchronous: the getters synchronise
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
extern "C" int ptl_ekf_get_state(ptl_ekf* h, double nav[19], double cov[324]) {
    if (!h) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    EkfState st;
    HIPCHK(hipMemcpyAsync(&st, h->st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nav) {
        memcpy(nav, st.nav.pos, 24); memcpy(nav + 3, st.nav.q, 32); memcpy(nav + 7, st.nav.vel, 24);
        memcpy(nav + 10, st.nav.bg, 24); memcpy(nav + 13, st.nav.ba, 24); memcpy(nav + 16, st.nav.grav, 24);
    }
    if (cov) memcpy(cov, st.P, sizeof st.P);
    return PTL_OK;
}
extern "C" int ptl_ekf_pose_mat(ptl_ekf* h, double T[16]) {
    if (!h || !T) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(T, (char*)h->st + offsetof(EkfState, pose), 128, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
extern "C" int ptl_ekf_ts(ptl_ekf* h, double* ts) {
    if (!h || !ts) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipMemcpyAsync(ts, (char*)h->st + (offsetof(EkfState, nav) + offsetof(EkfNav, cur_ts)), 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}

// ---- fixed-interval RTS smoother (ekf_kernels.h: the log inside d_ekf_step, k_ekf_smooth)
__global__ void k_ekf_log_set(EkfState* e, double* log, long long cap) {
    const int t = threadIdx.x;
    for (int i = t; i < EKF_N * EKF_N; i += blockDim.x) e->Phi[i] = (i % (EKF_N + 1) == 0) ? 1.0 : 0.0;
    if (t == 0) { e->log = log; e->log_cap = cap; e->log_count = 0; e->log_overflow = 0; }
}
static void ekf_log_free(ptl_ekf* h) {
    h->mem.release(&h->d_log); h->mem.release(&h->d_sm); h->mem.release(&h->d_job); h->mem.release(&h->d_info);
    h->log_cap = 0;
}
// capacity > 0: a fresh, empty log of that many updates (the old one, if any, is dropped); 0: off.  The caller's other streams must be idle.
static int ekf_log_set(ptl_ekf* h, int64_t cap) {
    HIPCHK(hipStreamSynchronize(h->stream));
    k_ekf_log_set<<<1, 64, 0, h->stream>>>(h->st, nullptr, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    ekf_log_free(h);
    if (cap <= 0) return PTL_OK;
    const size_t c = (size_t)cap;
    if (h->mem.alloc(&h->d_log, c * EKF_LOG_STRIDE) != hipSuccess || h->mem.alloc(&h->d_sm, c * 360) != hipSuccess ||
        h->mem.alloc(&h->d_job, 1) != hipSuccess || h->mem.alloc(&h->d_info, 2) != hipSuccess) {
        ekf_log_free(h);
        return set_err(PTL_ERR_HIP, "smoother log allocation failed (%lld entries, %.1f MB)", (long long)cap, cap * (EKF_LOG_STRIDE + 360) * 8 / 1e6);
    }
    h->log_cap = cap;
    h->job.e = h->st;
    h->job.pose = h->d_sm; h->job.t = h->d_sm + 16 * c; h->job.nav = h->d_sm + 17 * c; h->job.cov = h->d_sm + 36 * c;
    h->job.info = h->d_info;
    HIPCHK(hipMemcpyAsync(h->d_job, &h->job, sizeof h->job, hipMemcpyHostToDevice, h->stream));
    k_ekf_log_set<<<1, 64, 0, h->stream>>>(h->st, h->d_log, (long long)cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
// the status words of k_ekf_smooth -> return code
static int smooth_status(const ptl_ekf* h, const long long info[2], const char* who, int seq) {
    if (info[0] == 0) return PTL_OK;
    if (info[0] == -1) return set_err(PTL_ERR_CAPACITY, "%s: sequence %d: the smoother log overflowed (capacity %lld updates); a cold start or a new log empties it", who, seq, (long long)h->log_cap);
    if (info[0] == -2) return set_err(PTL_ERR_STATE, "%s: sequence %d: no smoother log", who, seq);
    return set_err(PTL_ERR_STATE, "%s: sequence %d: P_pred of log entry %lld is not positive definite (Cholesky failed): smoothed rows not valid", who, seq, info[0] - 1);
}
// rows [0, n) of the last backward pass of h -> host (poses16 required, the others nullable)
static int smooth_copy_out(const ptl_ekf* h, int64_t n, double* poses16, double* ts, double* nav19, double* cov324) {
    if (n <= 0) return PTL_OK;
    const size_t c = (size_t)h->log_cap;
    HIPCHK(hipMemcpy(poses16, h->d_sm, (size_t)n * 128, hipMemcpyDeviceToHost));
    if (ts) HIPCHK(hipMemcpy(ts, h->d_sm + 16 * c, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (nav19) HIPCHK(hipMemcpy(nav19, h->d_sm + 17 * c, (size_t)n * 19 * 8, hipMemcpyDeviceToHost));
    if (cov324) HIPCHK(hipMemcpy(cov324, h->d_sm + 36 * c, (size_t)n * 324 * 8, hipMemcpyDeviceToHost));
    return PTL_OK;
}
static int ekf_smooth_impl(ptl_ekf* h, const char* who, double* poses16, double* ts, double* nav19, double* cov324, int64_t max_rows, int64_t* n_rows) {
    if (!h->d_log) return set_err(PTL_ERR_STATE, "%s: the smoother log is not enabled", who);
    k_ekf_smooth<<<1, EKF_SMOOTH_THREADS, 0, h->stream>>>(h->d_job);
    HIPCHK(hipGetLastError());
    long long info[2];
    HIPCHK(hipMemcpyAsync(info, h->d_info, sizeof info, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int rc = smooth_status(h, info, who, 0);
    if (rc) return rc;
    const int64_t n = info[1] < max_rows ? info[1] : max_rows;
    rc = smooth_copy_out(h, n, poses16, ts, nav19, cov324);
    if (rc) return rc;
    if (n_rows) *n_rows = n;
    return PTL_OK;
}
static int ekf_log_read(ptl_ekf* h, double* entries, int64_t max_entries, int64_t* n_entries, int32_t* overflow) {
    if (!h->d_log) return set_err(PTL_ERR_STATE, "the smoother log is not enabled");
    long long cnt = 0;
    int ovf = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(&cnt, (char*)h->st + offsetof(EkfState, log_count), sizeof cnt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ovf, (char*)h->st + offsetof(EkfState, log_overflow), sizeof ovf, hipMemcpyDeviceToHost));
    const int64_t n = cnt < max_entries ? cnt : max_entries;
    if (entries && n > 0) HIPCHK(hipMemcpy(entries, h->d_log, (size_t)n * EKF_LOG_STRIDE * 8, hipMemcpyDeviceToHost));
    if (n_entries) *n_entries = cnt;
    if (overflow) *overflow = ovf;
    return PTL_OK;
}
static_assert(EKF_LOG_STRIDE == PTL_SMOOTHER_LOG_STRIDE && EKF_LOG_TS == PTL_SMOOTHER_LOG_TS && EKF_LOG_NAV_PRED == PTL_SMOOTHER_LOG_NAV_PRED &&
              EKF_LOG_P_PRED == PTL_SMOOTHER_LOG_P_PRED && EKF_LOG_PHI == PTL_SMOOTHER_LOG_PHI && EKF_LOG_NAV_POST == PTL_SMOOTHER_LOG_NAV_POST &&
              EKF_LOG_P_POST == PTL_SMOOTHER_LOG_P_POST, "log layout of include/ptudes_mi.h");
extern "C" int ptl_ekf_smoother_log(ptl_ekf* h, double* entries, int64_t max_entries, int64_t* n_entries, int32_t* overflow) {
    if (!h || max_entries < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    return ekf_log_read(h, entries, max_entries, n_entries, overflow);
}
extern "C" int ptl_ekf_log_enable(ptl_ekf* h, int64_t capacity) {
    if (!h || capacity < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    return ekf_log_set(h, capacity);
}
extern "C" int ptl_ekf_smooth(ptl_ekf* h, double* poses16, double* ts, double* nav19, double* cov324, int64_t max_rows, int64_t* n_rows) {
    if (!h || !poses16 || max_rows < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    return ekf_smooth_impl(h, "ptl_ekf_smooth", poses16, ts, nav19, cov324, max_rows, n_rows);
}

// ---- IMU deskew: the filter's knot list (ekf_kernels.h d_ekf_step) and the registration's wiring to it (d_imu_coltab)
static_assert(EKF_KNOT_STRIDE == PTL_KNOT_STRIDE, "knot layout of include/ptudes_mi.h");
__global__ void k_ekf_knots_set(EkfState* e, double* kn, long long cap) {
    if (threadIdx.x || blockIdx.x) return;
    e->knots = kn; e->knot_cap = cap; e->knot_count = 0; e->knot_overflow = 0;
}
// capacity >= 2: a fresh, empty knot list (the old one is dropped); 0: off.  The caller's other streams must be idle.
static int ekf_knots_set(ptl_ekf* h, int64_t cap) {
    HIPCHK(hipStreamSynchronize(h->stream));
    k_ekf_knots_set<<<1, 64, 0, h->stream>>>(h->st, nullptr, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mem.release(&h->d_knots);
    h->knot_cap = 0;
    if (cap <= 0) return PTL_OK;
    if (h->mem.alloc(&h->d_knots, (size_t)cap * EKF_KNOT_STRIDE) != hipSuccess) return set_err(PTL_ERR_HIP, "knot list allocation failed (%lld knots)", (long long)cap);
    h->knot_cap = cap;
    k_ekf_knots_set<<<1, 64, 0, h->stream>>>(h->st, h->d_knots, (long long)cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
static int ekf_knots_read(ptl_ekf* h, double* knots, int64_t max_knots, int64_t* n_knots, int32_t* overflow) {
    if (!h->d_knots) return set_err(PTL_ERR_STATE, "the knot list is not enabled");
    long long cnt = 0;
    int ovf = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(&cnt, (char*)h->st + offsetof(EkfState, knot_count), sizeof cnt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ovf, (char*)h->st + offsetof(EkfState, knot_overflow), sizeof ovf, hipMemcpyDeviceToHost));
    const int64_t n = cnt < max_knots ? cnt : max_knots;
    if (knots && n > 0) HIPCHK(hipMemcpy(knots, h->d_knots, (size_t)n * EKF_KNOT_STRIDE * 8, hipMemcpyDeviceToHost));
    if (n_knots) *n_knots = cnt;
    if (overflow) *overflow = ovf;
    return PTL_OK;
}
static int ekf_knot_overflow(ptl_ekf* h, int* ovf) {
    HIPCHK(hipMemcpyAsync(ovf, (char*)h->st + offsetof(EkfState, knot_overflow), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTL_OK;
}
extern "C" int ptl_ekf_knots_enable(ptl_ekf* h, int64_t capacity) {
    if (!h || capacity < 0 || capacity == 1) return set_err(PTL_ERR_ARG, "bad argument (capacity: 0 = off, else >= 2 knots)");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    return ekf_knots_set(h, capacity);
}
extern "C" int ptl_ekf_knots(ptl_ekf* h, double* knots, int64_t max_knots, int64_t* n_knots, int32_t* overflow) {
    if (!h || max_knots < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    return ekf_knots_read(h, knots, max_knots, n_knots, overflow);
}
struct DkWire { const double* knots; const long long* nknots; const int* kovf; const double* t0t1; int* modes; int n; };
__global__ void k_dk_set(DevState* st, DkWire w) {
    if (threadIdx.x || blockIdx.x) return;
    st->dk_knots = w.knots; st->dk_nknots = w.nknots; st->dk_kovf = w.kovf; st->dk_t0t1 = w.t0t1; st->dk_modes = w.modes; st->dk_n = w.n;
}
__global__ void k_dk_times(double* t0t1, double t0, double t1) {
    if (threadIdx.x || blockIdx.x) return;
    t0t1[0] = t0; t0t1[1] = t1;
}
// the registration `h` deskews from filter `e`'s knots with the sweep times / mode record t0t1 / modes (n scans); e == nullptr: off
static int dk_wire(ptl_icp* h, ptl_ekf* e, const double* t0t1, int* modes, int64_t n) {
    DkWire w;
    memset(&w, 0, sizeof w);
    if (e) {
        w.knots = e->d_knots;
        w.nknots = (const long long*)((char*)e->st + offsetof(EkfState, knot_count));
        w.kovf = (const int*)((char*)e->st + offsetof(EkfState, knot_overflow));
        w.t0t1 = t0t1; w.modes = modes; w.n = (int)n;
    }
    k_dk_set<<<1, 64, 0, h->stream>>>(h->c.st, w);
    HIPCHK(hipGetLastError());
    h->dk_wired = e != nullptr;
    return PTL_OK;
}
// knots a filter needs when it consumes imu_end[0] samples before scan 0 and imu_end[k] - imu_end[k - 1] after the update of scan k - 1
static int64_t dk_knots_needed(const std::vector<int64_t>& imu_end) {
    int64_t need = imu_end.empty() ? 0 : imu_end[0];
    for (size_t k = 1; k < imu_end.size(); ++k) need = std::max(need, 1 + imu_end[k] - imu_end[k - 1]);
    return need;
}
extern "C" int ptl_icp_deskew_modes(ptl_icp* h, int32_t* modes, int64_t max_n, int64_t* n) {
    if (!h || !modes || max_n < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    int64_t m = h->scans_done < max_n ? h->scans_done : max_n;
    if (m > (int64_t)h->dk_rec.size()) m = (int64_t)h->dk_rec.size();
    int64_t dev = 0;  // scans up to the last IMU-wired one: their modes come from the device record (which holds dk_cap >= those)
    for (int64_t k = 0; k < m; ++k) if (h->dk_rec[(size_t)k] < 0) dev = k + 1;
    if (dev > h->dk_cap) return set_err(PTL_ERR_STATE, "ptl_icp_deskew_modes: no device record for scan %lld", (long long)dev - 1);
    if (dev > 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(modes, h->dk_modes, (size_t)dev * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (int64_t k = 0; k < m; ++k) if (h->dk_rec[(size_t)k] >= 0) modes[k] = h->dk_rec[(size_t)k];
    if (n) *n = m;
    return PTL_OK;
}
extern "C" int ptl_icp_column_table(ptl_icp* h, double* out) {
    if (!h || !out) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->c.coltab, (size_t)h->c.W * 12 * 8, hipMemcpyDeviceToHost));
    return PTL_OK;
}

// ================================================================================================ one scan of the driver loop, per-call handles
// The reference's loop body (cli/ekf_bench.py:493-563) for host-fed data in ONE host round trip: the IMU samples that precede the scan
// (processImu each), the registration with the filter's pose as its guess (--use-imu-prediction) or the caller's / the constant-velocity
// one, processPose with the new pose.  Object by object (ESEKF.processImu x n, ekf.nav.pose_mat(), register_frame, processPose, nav again)
// that is n + 2 launches and THREE synchronising read-backs per scan; here the filter's launches go to its own stream, the Gauss-Newton
// kernel waits for the predicts on the device and reads the guess there, the update waits for the Gauss-Newton kernel on the device and
// reads the pose there, and the host waits once.  Same kernels, same order of operations per handle: same bits.
// imu_deskew: the column table of this scan comes from the filter's knots (sweep times t0, t1); its prologue waits for the predicts.
static int icp_ekf_step_impl(ptl_icp* h, ptl_ekf* e, const double* imu_rows, int64_t n_imu, const void* xyz, int dtype, int64_t n,
                             const double* t01, const double* guess, int32_t use_imu_prediction, double kiss_pose[16],
                             double ekf_pose[16], double* ekf_ts, ptl_icp_stats* stats, bool imu_deskew, double t0, double t1) {
    if (!h || !e || (!imu_rows && n_imu > 0) || (!xyz && n > 0) || n < 0 || n_imu < 0) return set_err(PTL_ERR_ARG, "bad argument");
    if (dtype != PTL_F32 && dtype != PTL_F64) return set_err(PTL_ERR_ARG, "dtype must be PTL_F32 or PTL_F64");
    if (n > h->n_max) return set_err(PTL_ERR_CAPACITY, "scan has %lld points, capacity %lld", (long long)n, (long long)h->n_max);
    if (h->cfg.device_id != e->cfg.device_id) return set_err(PTL_ERR_ARG, "registration on device %d, filter on device %d", h->cfg.device_id, e->cfg.device_id);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    if (imu_deskew) {
        if (!h->cfg.deskew) return set_err(PTL_ERR_STATE, "IMU deskew: deskew is off in the registration's configuration");
        if (!e->d_knots) return set_err(PTL_ERR_STATE, "IMU deskew: the filter keeps no knot list (ptl_ekf_knots_enable)");
        if (n_imu + 1 > e->knot_cap) return set_err(PTL_ERR_ARG, "IMU deskew: %lld IMU samples need %lld knots, the filter's list holds %lld", (long long)n_imu, (long long)n_imu + 1, (long long)e->knot_cap);
        if (!(t1 >= t0)) return set_err(PTL_ERR_ARG, "IMU deskew: sweep times must satisfy t0 <= t1");
        if (h->scans_done >= h->dk_cap) {  // the per-scan sweep times and modes grow with the scans
            const int64_t cap = h->dk_cap > 0 ? 2 * h->dk_cap : h->traj_cap;
            double* nt = nullptr;
            int* nm = nullptr;
            DevOwner tmp;
            HIPCHK(tmp.alloc(&nt, (size_t)cap * 2));
            HIPCHK(tmp.alloc(&nm, (size_t)cap));
            HIPCHK(hipMemset(nm, 0, (size_t)cap * sizeof(int)));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (h->dk_modes) HIPCHK(hipMemcpy(nm, h->dk_modes, (size_t)h->dk_cap * sizeof(int), hipMemcpyDeviceToDevice));
            h->mem.replace(&h->dk_t0t1, tmp, nt);
            h->mem.replace(&h->dk_modes, tmp, nm);
            h->dk_cap = cap;
        }
    }
    if (!h->ev_step_guess) {
        HIPCHK(h->ev_step_guess.create());
        HIPCHK(h->ev_step_gn.create());
    }
    hipStream_t es = e->stream;
    // processImu x n_imu (ptl_ekf_process_imu_batch's kernel).  Any count is served, like the call-by-call loop (a long IMU-only prefix,
    // dropped lidar frames, a 1 kHz IMU): what does not fit the staging buffer goes first, buf_rows samples at a time with a wait for
    // the buffer's reuse; the last buf_rows or fewer ride on this step's single wait.
    int rc = ekf_stage_imu(e, imu_rows, n_imu, false);
    if (rc) return rc;
    const size_t esz = dtype == PTL_F32 ? 4 : 8;
    if (n) HIPCHK(hipMemcpyAsync(h->d_in, xyz, (size_t)n * 3 * esz, hipMemcpyHostToDevice, h->stream));
    if (t01 && n) HIPCHK(hipMemcpyAsync(h->d_t01, t01, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    const double* guess_ptr = nullptr;
    if (use_imu_prediction || imu_deskew) HIPCHK(hipEventRecord(h->ev_step_guess, es));  // the predicts are through
    if (use_imu_prediction) {  // ekf.nav.pose_mat() as the guess, read on the device once the predicts are through
        h->gn_wait = h->ev_step_guess;
        guess_ptr = (const double*)((char*)e->st + offsetof(EkfState, pose));
    } else if (guess) {
        HIPCHK(hipMemcpyAsync(h->d_ext, guess, 16 * 8, hipMemcpyHostToDevice, h->stream));
        guess_ptr = h->d_ext;
    }
    if (imu_deskew) {  // this scan's sweep times, the wiring to the filter's knots, and the prologue behind the predicts
        k_dk_times<<<1, 64, 0, h->stream>>>(h->dk_t0t1 + 2 * h->scans_done, t0, t1);
        rc = dk_wire(h, e, h->dk_t0t1, h->dk_modes, h->dk_cap);
        if (rc) return rc;
        h->pro_wait = h->ev_step_guess;
    }
    h->gn_done = h->ev_step_gn;
    rc = icp_enqueue_scan(h, dtype == PTL_F32 ? (const float*)h->d_in : nullptr, dtype == PTL_F64 ? (const double*)h->d_in : nullptr,
                          t01 ? h->d_t01 : nullptr, n, guess_ptr);
    h->gn_wait = nullptr; h->gn_done = nullptr; h->pro_wait = nullptr;
    if (imu_deskew) {  // the handle's other entry points keep the constant-velocity deskew
        const int rc2 = dk_wire(h, nullptr, nullptr, nullptr, 0);
        if (!rc) rc = rc2;
    }
    if (rc) return rc;
    // processPose(kiss pose): behind the Gauss-Newton kernel, on the filter's stream; its outputs (pose after the update, timestamp) land
    // in the tail of the filter's staging buffer
    double* d_out = e->d_buf + (size_t)e->buf_rows * 7;
    HIPCHK(hipStreamWaitEvent(es, h->ev_step_gn, 0));
    k_ekf_step<<<1, EKF_THREADS, 0, es>>>(e->st, e->d_buf, 0, 0, h->c.traj + 16 * (h->scans_done - 1), nullptr, d_out, d_out + 16, nullptr, 1);
    double out[17];
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, es));
    rc = icp_percall_finish(h, kiss_pose, stats);  // (synchronises the registration's stream: pose, statistics row, error flags)
    HIPCHK(hipStreamSynchronize(es));
    if (rc) return rc;
    if (imu_deskew) {
        int ovf = 0;
        rc = ekf_knot_overflow(e, &ovf);
        if (rc) return rc;
        if (ovf) return set_err(PTL_ERR_CAPACITY, "IMU deskew: the filter's knot list overflowed (capacity %lld)", (long long)e->knot_cap);
    }
    if (ekf_pose) memcpy(ekf_pose, out, 128);
    if (ekf_ts) *ekf_ts = out[16];
    return PTL_OK;
}
extern "C" int ptl_icp_ekf_step(ptl_icp* h, ptl_ekf* e, const double* imu_rows, int64_t n_imu, const void* xyz, int dtype, int64_t n,
                                const double* t01, const double* guess, int32_t use_imu_prediction, double kiss_pose[16],
                                double ekf_pose[16], double* ekf_ts, ptl_icp_stats* stats) {
    return icp_ekf_step_impl(h, e, imu_rows, n_imu, xyz, dtype, n, t01, guess, use_imu_prediction, kiss_pose, ekf_pose, ekf_ts, stats, false, 0.0, 0.0);
}
extern "C" int ptl_icp_ekf_step_imu_deskew(ptl_icp* h, ptl_ekf* e, const double* imu_rows, int64_t n_imu, const void* xyz, int dtype, int64_t n,
                                           double t0, double t1, const double* guess, int32_t use_imu_prediction, double kiss_pose[16],
                                           double ekf_pose[16], double* ekf_ts, ptl_icp_stats* stats) {
    return icp_ekf_step_impl(h, e, imu_rows, n_imu, xyz, dtype, n, nullptr, guess, use_imu_prediction, kiss_pose, ekf_pose, ekf_ts, stats, true, t0, t1);
}

// ================================================================================================ one sequence of a runner
// What the sequence runner keeps once and the batched runner once per sequence: the registration and the filter, the sweep slots, the IMU
// rows and their split over the scans, the result rows, and the IMU deskew's sweep times and mode record.  The streams, events and the
// driver's position stay with the runner: the helpers below enqueue nothing on a stream of their own and leave synchronising to the caller.
struct SeqLane {
    ptl_icp* icp = nullptr;
    ptl_ekf* ekf = nullptr;
    float* d_scans = nullptr;       // sweep slots
    double* d_imu = nullptr;        // [n_imu][7]
    std::vector<int64_t> imu_end;   // [n_scans] IMU samples before scan k
    int* d_imu_end = nullptr;       // [n_scans] the same on the device (batched runner: its kernels read it)
    int64_t imu_pos = 0;            // IMU samples the filter has been given
    double* d_res_poses = nullptr;  // [n_scans][16]
    double* d_res_t = nullptr;      // [n_scans]
    double* d_rows = nullptr;       // [n_scans][8]
    // IMU deskew: sweep times and modes of all n_scans (also with the sweep ring), and whether the times came since it was enabled
    double* d_dk_t0t1 = nullptr;    // [n_scans][2]
    int* d_dk_modes = nullptr;      // [n_scans]
    bool dk_times = false;
    DevOwner mem;  // the lane's own buffers
    ~SeqLane() { delete icp; delete ekf; }  // (the runner has set the device; its streams, which the two borrow, outlive the lane)
};

// what ptl_seq_create and ptl_batch_create check and settle alike: `out` = *cfg with room for a whole sweep in the registration and the
// filter on the registration's device
static int seq_cfg_settle(const ptl_seq_cfg* cfg, ptl_seq_cfg* out) {
    ABI_CHECK(ptl_seq_cfg, cfg);
    ABI_CHECK(ptl_icp_cfg, &cfg->icp);
    ABI_CHECK(ptl_ekf_cfg, &cfg->ekf);
    if (cfg->n_scans < 1 || cfg->points_per_scan < 1) return set_err(PTL_ERR_ARG, "empty sequence");
    if (ptl_device_count() <= cfg->icp.device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", cfg->icp.device_id);
    HIPCHK(hipSetDevice(cfg->icp.device_id));
    *out = *cfg;
    if (out->icp.max_points_per_scan < cfg->points_per_scan) out->icp.max_points_per_scan = cfg->points_per_scan;
    out->ekf.device_id = cfg->icp.device_id;
    return PTL_OK;
}
// a lane's own device buffers for a settled configuration (`slots` sweep slots of `slot_bytes` each, the IMU rows, the result rows; a batch
// member: the IMU split on the device): `m` allocates them (l.mem) or only counts their bytes
static void lane_alloc(DevOwner& m, SeqLane& l, const ptl_seq_cfg& cfg, size_t slot_bytes, size_t slots, bool batch) {
    const size_t n = (size_t)cfg.n_scans, nim = cfg.n_imu > 0 ? (size_t)cfg.n_imu : 1;
    m.add((unsigned char**)&l.d_scans, slots * slot_bytes);
    m.add(&l.d_imu, nim * 7);
    m.add(&l.d_res_poses, n * 16); m.add(&l.d_res_t, n); m.add(&l.d_rows, n * 8);
    if (batch) m.add(&l.d_imu_end, n);
}
// device bytes one member of a batch asks for - its registration (*icp_bytes), its filter and the lane's own buffers: the three allocation
// functions over an owner that only counts, on handles that are settled and never created
static size_t lane_footprint_bytes(const ptl_seq_cfg& cfg, size_t slot_bytes, size_t slots, size_t* icp_bytes) {
    DevOwner count(true);
    ptl_icp icp;
    ptl_ekf ekf;
    SeqLane l;
    icp_settle(&icp, &cfg.icp);
    icp_alloc(count, &icp, icp_traj_rows(cfg.n_scans, true));
    *icp_bytes = count.requested();
    ekf_alloc(count, &ekf);
    lane_alloc(count, l, cfg, slot_bytes, slots, true);
    return count.requested();
}
// the registration (on `stream`), the filter (on `ekf_stream`), `slots` sweep slots of `slot_bytes` each, the IMU rows and the result rows of
// a settled configuration.  batch: a member of a batch (icp_create_impl's batch_member, the whole trajectory up front, the IMU split on the device)
static int lane_create(SeqLane& l, const ptl_seq_cfg& cfg, hipStream_t stream, hipStream_t ekf_stream, size_t slot_bytes, size_t slots, bool batch,
                       const char* who) {
    int rc = icp_create_impl(&cfg.icp, stream, &l.icp, batch, icp_traj_rows(cfg.n_scans, batch));
    if (rc == PTL_OK) rc = ekf_create_impl(&cfg.ekf, ekf_stream, &l.ekf);
    if (rc) return rc;
    lane_alloc(l.mem, l, cfg, slot_bytes, slots, batch);
    if (l.mem.err != hipSuccess || (batch && hipMemset(l.d_imu_end, 0, l.mem.bytes_of(l.d_imu_end)) != hipSuccess))
        return set_err(PTL_ERR_HIP, "%s: allocation failed (%.1f MB of sweeps per sequence)", who, slots * slot_bytes / 1e6);
    l.imu_end.assign((size_t)cfg.n_scans, 0);
    return PTL_OK;
}
// the IMU rows and their split over the scans.  one_per_scan: at least one sample between consecutive scans - lockstep batching cannot
// skip a scan of one sequence only (ekf_bench.py:512-518)
static int lane_upload_imu(SeqLane& l, const ptl_seq_cfg& cfg, const double* imu, const int64_t* imu_end, bool one_per_scan) {
    if (cfg.n_imu > 0) HIPCHK(hipMemcpy(l.d_imu, imu, (size_t)cfg.n_imu * 56, hipMemcpyHostToDevice));
    for (int64_t k = 0; k < cfg.n_scans; ++k) {
        if (imu_end[k] < 0 || imu_end[k] > cfg.n_imu || (k && imu_end[k] < imu_end[k - 1])) return set_err(PTL_ERR_ARG, "imu_end must be non-decreasing within [0, n_imu]");
        if (one_per_scan && k && imu_end[k] == imu_end[k - 1]) return set_err(PTL_ERR_ARG, "batched runs need at least one IMU sample between consecutive scans (scan %lld)", (long long)k);
        l.imu_end[(size_t)k] = imu_end[k];
    }
    if (!l.d_imu_end) return PTL_OK;
    const std::vector<int> e32(l.imu_end.begin(), l.imu_end.end());
    HIPCHK(hipMemcpy(l.d_imu_end, e32.data(), e32.size() * sizeof(int), hipMemcpyHostToDevice));
    return PTL_OK;
}
// the first min(n_out, max_n) rows of the lane's results -> host; the caller has synchronised its streams
static int lane_results(const SeqLane& l, bool with_ekf, int64_t n_out, double* res_poses, double* res_t, double* kiss_poses, ptl_icp_stats* stats,
                        int64_t max_n, int64_t* n_written) {
    const int64_t n = n_out < max_n ? n_out : max_n;
    if (n > 0) {
        if (res_poses && with_ekf) HIPCHK(hipMemcpy(res_poses, l.d_res_poses, (size_t)n * 128, hipMemcpyDeviceToHost));
        if (res_t && with_ekf) HIPCHK(hipMemcpy(res_t, l.d_res_t, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (kiss_poses) HIPCHK(hipMemcpy(kiss_poses, l.icp->c.traj, (size_t)n * 128, hipMemcpyDeviceToHost));
        if (stats) {
            std::vector<ScanStats> tmp((size_t)n);
            HIPCHK(hipMemcpy(tmp.data(), l.icp->c.sstats, (size_t)n * sizeof(ScanStats), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n; ++i) stats_out(tmp[(size_t)i], &stats[i]);
        }
    }
    if (n_written) *n_written = n;
    return PTL_OK;
}
// the first min(n_out, max_rows) trajectory rows -> device memory, on `stream` (the caller has synchronised its other streams)
static int lane_copy_traj(const SeqLane& l, const ptl_seq_cfg& cfg, int64_t n_out, hipStream_t stream, void* dst_device, int64_t max_rows, int64_t* rows) {
    if (!cfg.with_ekf) return set_err(PTL_ERR_STATE, "trajectory rows need with_ekf");
    const int64_t n = n_out < max_rows ? n_out : max_rows;
    if (n > 0) HIPCHK(hipMemcpyAsync(dst_device, l.d_rows, (size_t)n * 64, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (rows) *rows = n;
    return PTL_OK;
}
// the filter's smoother log and knot list (the caller has synchronised its streams)
static int lane_smoother_log(const SeqLane& l, const ptl_seq_cfg& cfg, const char* who, double* entries, int64_t max_entries, int64_t* n_entries, int32_t* overflow) {
    if (!cfg.with_ekf) return set_err(PTL_ERR_STATE, "%s: an ICP-only run has no filter log", who);
    return ekf_log_read(l.ekf, entries, max_entries, n_entries, overflow);
}
static int lane_knots(const SeqLane& l, const ptl_seq_cfg& cfg, const char* who, double* knots, int64_t max_knots, int64_t* n_knots, int32_t* overflow) {
    if (!cfg.with_ekf) return set_err(PTL_ERR_STATE, "%s: an ICP-only run has no filter", who);
    return ekf_knots_read(l.ekf, knots, max_knots, n_knots, overflow);
}

// ---- IMU deskew of a lane
// knots the filter needs for the lane's IMU split, against `cap`
static int lane_dk_knots_check(const SeqLane& l, int64_t cap, const char* who, int seq) {
    const int64_t need = dk_knots_needed(l.imu_end);
    if (need > cap) return set_err(PTL_ERR_ARG, "%s: IMU deskew: sequence %d: the IMU samples between two scans need %lld knots, capacity %lld", who, seq, (long long)need, (long long)cap);
    return PTL_OK;
}
// ptl_*_imu_deskew_enable's arguments against the configuration and the IMU split of each of the n lanes
static int dk_enable_check(const ptl_seq_cfg& cfg, const SeqLane* lanes, int n, int32_t on, int64_t knot_capacity, const char* who) {
    if (!cfg.with_ekf) return set_err(PTL_ERR_STATE, "%s: an ICP-only run (with_ekf = 0) has no filter to deskew with", who);
    if (!on) return PTL_OK;
    if (!cfg.icp.deskew) return set_err(PTL_ERR_STATE, "%s: deskew is off in the configuration", who);
    if (knot_capacity < 2) return set_err(PTL_ERR_ARG, "%s: knot_capacity must be >= 2", who);
    for (int s = 0; s < n; ++s) {
        const int rc = lane_dk_knots_check(lanes[s], knot_capacity, who, s);
        if (rc) return rc;
    }
    return PTL_OK;
}
// knot_capacity > 0: a fresh knot list, an empty mode record and the registration wired to both (the sweep times follow); 0: off, the
// constant-velocity deskew.  The caller's streams are idle.
static int lane_dk_set(SeqLane& l, int64_t n_scans, int64_t knot_capacity) {
    const size_t n = (size_t)n_scans;
    l.dk_times = false;
    int rc = dk_wire(l.icp, nullptr, nullptr, nullptr, 0);
    if (rc == PTL_OK) rc = ekf_knots_set(l.ekf, 0);
    if (rc || knot_capacity <= 0) return rc;
    if ((!l.d_dk_t0t1 && l.mem.alloc(&l.d_dk_t0t1, 2 * n) != hipSuccess) || (!l.d_dk_modes && l.mem.alloc(&l.d_dk_modes, n) != hipSuccess))
        return set_err(PTL_ERR_HIP, "IMU deskew: allocation failed");
    HIPCHK(hipMemset(l.d_dk_modes, 0, n * sizeof(int)));
    rc = ekf_knots_set(l.ekf, knot_capacity);
    return rc ? rc : dk_wire(l.icp, l.ekf, l.d_dk_t0t1, l.d_dk_modes, (int64_t)n);
}
// before an enqueue: sweep times there, knots enough
static int lane_dk_ready(const SeqLane& l, const char* who, int seq) {
    if (!l.dk_times) return set_err(PTL_ERR_STATE, "%s: IMU deskew: sequence %d has no sweep times (upload_sweep_times)", who, seq);
    return lane_dk_knots_check(l, l.ekf->knot_cap, who, seq);
}
// after a wait: a truncated knot list is an error, not a quiet fallback
static int lane_dk_overflow(const SeqLane& l, const char* who, int seq) {
    int ovf = 0;
    const int rc = ekf_knot_overflow(l.ekf, &ovf);
    if (rc) return rc;
    if (ovf) return set_err(PTL_ERR_CAPACITY, "%s: IMU deskew: sequence %d: the filter's knot list overflowed (capacity %lld)", who, seq, (long long)l.ekf->knot_cap);
    return PTL_OK;
}
// (t0, t1) of every scan, t1 >= t0 (the caller has synchronised its streams)
static int lane_upload_sweep_times(SeqLane& l, int64_t n_scans, const double* t0t1, const char* who) {
    for (int64_t k = 0; k < n_scans; ++k)
        if (!(t0t1[2 * k + 1] >= t0t1[2 * k])) return set_err(PTL_ERR_ARG, "%s: scan %lld has t1 < t0", who, (long long)k);
    HIPCHK(hipMemcpy(l.d_dk_t0t1, t0t1, (size_t)n_scans * 16, hipMemcpyHostToDevice));
    l.dk_times = true;
    return PTL_OK;
}
// modes of the first min(n_out, max_n) scans: the device record with IMU deskew on, else the constant-velocity deskew's (none for the first
// two scans); the caller has synchronised its streams
static int lane_deskew_modes(const SeqLane& l, const ptl_seq_cfg& cfg, bool dk_on, int64_t n_out, int32_t* modes, int64_t max_n, int64_t* n) {
    const int64_t m = n_out < max_n ? n_out : max_n;
    if (!dk_on) {
        for (int64_t k = 0; k < m; ++k) modes[k] = (cfg.icp.deskew && k >= 2) ? DK_MODE_CV : DK_MODE_NONE;
    } else if (m > 0) {
        HIPCHK(hipMemcpy(modes, l.d_dk_modes, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    }
    if (n) *n = m;
    return PTL_OK;
}

// ================================================================================================ sequence runner
struct ptl_seq {
    ptl_seq_cfg cfg;
    Stream stream;
    // The EKF launches run on their own stream: the update with scan k's pose and the IMU predicts up to scan k+1
    // overlap scan k's map update and scan k+1's deskew / downsampling; only the GN kernel waits for the EKF
    // (its guess), and the EKF waits for the GN kernel (the pose measurement).
    Stream ekf_stream;
    Event ev_guess, ev_gn;
    Event ev_pro;  // IMU deskew: the event the prologue waits for
    SeqLane lane;  // sweep slots: [n_scans][pps][3] f32
    std::vector<int64_t> scan_of_out;  // scan index of each processed output
    int64_t n_out = 0;
    int64_t next_scan = 0, imus_per_scan = 0;  // driver-loop position (ekf_bench.py:491-518)
    ptl_lut* lut = nullptr;          // non-null => sweeps were uploaded as u32 range images
    std::vector<unsigned char> is_range;
    bool dk_on = false;  // IMU deskew (ptl_seq_imu_deskew_enable)
};

extern "C" int ptl_seq_destroy(ptl_seq* s) { return s ? handle_destroy(s, s->cfg.icp.device_id) : PTL_OK; }
extern "C" int ptl_seq_create(const ptl_seq_cfg* cfg, ptl_seq** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "null argument");
    ptl_seq_cfg c;
    int rc = seq_cfg_settle(cfg, &c);
    if (rc) return rc;
    std::unique_ptr<ptl_seq> owner(new ptl_seq());
    ptl_seq* s = owner.get();
    s->cfg = c;
    if (s->stream.create() != hipSuccess || s->ekf_stream.create() != hipSuccess || s->ev_guess.create() != hipSuccess || s->ev_gn.create() != hipSuccess)
        return set_err(PTL_ERR_HIP, "stream / event creation failed");
    rc = lane_create(s->lane, c, s->stream, s->ekf_stream, (size_t)c.points_per_scan * 12, (size_t)c.n_scans, false, "ptl_seq_create");
    if (rc) return rc;
    s->is_range.assign((size_t)c.n_scans, 0);
    *out = owner.release();
    return PTL_OK;
}
extern "C" int ptl_seq_upload_scan(ptl_seq* s, int64_t k, const float* xyz) {
    if (!s || !xyz || k < 0 || k >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    const size_t bytes = (size_t)s->cfg.points_per_scan * 12;
    HIPCHK(hipMemcpy((char*)s->lane.d_scans + (size_t)k * bytes, xyz, bytes, hipMemcpyHostToDevice));
    return PTL_OK;
}
// sweep k as a raw range image (H*W u32 mm); needs ptl_seq_set_lut before running
extern "C" int ptl_seq_upload_range(ptl_seq* s, int64_t k, const uint32_t* range_mm) {
    if (!s || !range_mm || k < 0 || k >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    const size_t slot = (size_t)s->cfg.points_per_scan * 12;
    HIPCHK(hipMemcpy((char*)s->lane.d_scans + (size_t)k * slot, range_mm, (size_t)s->cfg.points_per_scan * 4, hipMemcpyHostToDevice));
    s->is_range[(size_t)k] = 1;
    return PTL_OK;
}
extern "C" int ptl_seq_set_lut(ptl_seq* s, ptl_lut* lut, int32_t active_beams) {
    if (!s || !lut) return set_err(PTL_ERR_ARG, "null argument");
    if ((int64_t)lut->H * lut->W != s->cfg.points_per_scan) return set_err(PTL_ERR_ARG, "LUT size does not match points_per_scan");
    s->lut = lut;
    return ptl_icp_set_active_beams(s->lane.icp, lut->H, active_beams);
}
extern "C" int ptl_seq_upload_imu(ptl_seq* s, const double* imu, const int64_t* imu_end) {
    if (!s || !imu_end || (!imu && s->cfg.n_imu > 0)) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    return lane_upload_imu(s->lane, s->cfg, imu, imu_end, false);
}
static int seq_reset(ptl_seq* s) {
    int rc = icp_reset_device(s->lane.icp);
    if (rc) return rc;
    rc = ekf_reset(s->lane.ekf);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s->ekf_stream));  // EKF launches may go to either stream afterwards
    s->scan_of_out.clear();
    s->n_out = 0;
    s->next_scan = 0;
    s->lane.imu_pos = 0;
    s->imus_per_scan = 1;  // ekf_bench.py:491
    return PTL_OK;
}
// The reference's driver loop (cli/ekf_bench.py:493-563) enqueued for the next n scans: IMU samples up to
// the scan -> EKF predict; scan -> guess (EKF nav pose when use_imu_prediction) -> ICP -> EKF update.
// Nothing here waits for the device.
extern "C" int ptl_seq_enqueue(ptl_seq* s, int64_t n) {
    if (!s || n < 0 || s->next_scan + n > s->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    SeqLane& l = s->lane;
    const bool with_ekf = s->cfg.with_ekf != 0;
    const double* guess_ptr = (with_ekf && s->cfg.use_imu_prediction) ? (const double*)((char*)l.ekf->st + offsetof(EkfState, pose)) : nullptr;
    const size_t pps = (size_t)s->cfg.points_per_scan;
    const int64_t end = s->next_scan + n;
    hipStream_t es = s->ekf_stream;  // used when the EKF does not feed the registration (no IMU prediction)
    if (s->dk_on) {  // IMU deskew: sweep times, knots enough, and no scan the driver loop would skip (scan k's table is at index k)
        const int rc = lane_dk_ready(l, "ptl_seq_enqueue", 0);
        if (rc) return rc;
        if (s->next_scan == 0 && end > 0 && l.imu_end[0] == 0) return set_err(PTL_ERR_ARG, "IMU deskew: scan 0 has no IMU sample before it");
        for (int64_t k = s->next_scan > 0 ? s->next_scan : 1; k < end; ++k)
            if (l.imu_end[(size_t)k] == l.imu_end[(size_t)k - 1]) return set_err(PTL_ERR_ARG, "IMU deskew: scan %lld has no IMU sample after scan %lld", (long long)k, (long long)k - 1);
    }
    for (int64_t k = s->next_scan; k < end; ++k) {
        // IMU samples that precede scan k and were not consumed yet (only before the very first scan of a run,
        // or when the previous scan was skipped: otherwise the previous scan's EKF launch already ran them)
        const int64_t e = with_ekf ? l.imu_end[(size_t)k] : l.imu_pos;
        if (e > l.imu_pos) {
            k_ekf_step<<<1, EKF_THREADS, 0, es>>>(l.ekf->st, l.d_imu, (int)l.imu_pos, (int)e, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
            s->imus_per_scan += e - l.imu_pos;
            l.imu_pos = e;
        }
        s->next_scan = k + 1;
        if (with_ekf && !s->imus_per_scan) continue;  // ekf_bench.py:512-518
        s->imus_per_scan = 0;
        const int64_t o = s->n_out;
        const int64_t e2 = (k + 1 < s->cfg.n_scans) ? l.imu_end[(size_t)k + 1] : l.imu_pos;
        if (with_ekf && guess_ptr) {
            // the EKF step (update with scan k-1's pose, IMU predicts up to scan k) runs on its own stream beside K0-K4 and
            // the map update; the GN launch of scan k waits for its pose - by then (K0-K4 take longer) it is there
            HIPCHK(hipEventRecord(s->ev_guess, es));
            l.icp->gn_wait = s->ev_guess;
        }
        if (with_ekf) l.icp->gn_done = s->ev_gn;
        if (s->dk_on) {  // the prologue (the column table) waits for the predicts through the sweep's samples: no overlap with them
            HIPCHK(hipEventRecord(s->ev_pro, es));
            l.icp->pro_wait = s->ev_pro;
        }
        int rc;
        if (s->is_range[(size_t)k]) {
            if (!s->lut) rc = set_err(PTL_ERR_STATE, "scan %lld is a range image but no LUT was set", (long long)k);
            else rc = icp_enqueue_scan(l.icp, nullptr, nullptr, nullptr, (int64_t)pps, guess_ptr,
                                       (const unsigned*)(l.d_scans + (size_t)k * pps * 3), s->lut);
        } else {
            rc = icp_enqueue_scan(l.icp, l.d_scans + (size_t)k * pps * 3, nullptr, nullptr, (int64_t)pps, guess_ptr);
        }
        l.icp->gn_wait = nullptr; l.icp->gn_done = nullptr; l.icp->pro_wait = nullptr;
        if (rc) return rc;
        const double* kiss_pose = l.icp->c.traj + 16 * (l.icp->scans_done - 1);
        if (with_ekf) {
            HIPCHK(hipStreamWaitEvent(es, s->ev_gn, 0));  // recorded right after the GN launch
            k_ekf_step<<<1, EKF_THREADS, 0, es>>>(l.ekf->st, l.d_imu, (int)l.imu_pos, (int)e2, kiss_pose, nullptr,
                                                 l.d_res_poses + 16 * o, l.d_res_t + o, l.d_rows + 8 * o, 1);
        }
        if (with_ekf) {
            s->imus_per_scan += e2 - l.imu_pos;
            l.imu_pos = e2;
        }
        s->scan_of_out.push_back(k);
        s->n_out++;
    }
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
extern "C" int ptl_seq_wait(ptl_seq* s) {
    if (!s) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    int rc = icp_check_flags(s->lane.icp);
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    if (rc == PTL_OK && s->dk_on) rc = lane_dk_overflow(s->lane, "ptl_seq_wait", 0);
    return rc;
}
extern "C" int ptl_seq_run(ptl_seq* s, int64_t n) {
    if (!s || n < 0 || n > s->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    int rc = seq_reset(s);
    if (rc) return rc;
    rc = ptl_seq_enqueue(s, n);
    if (rc) return rc;
    return ptl_seq_wait(s);
}
extern "C" int ptl_seq_advance(ptl_seq* s, int64_t n) {
    int rc = ptl_seq_enqueue(s, n);
    if (rc) return rc;
    return ptl_seq_wait(s);
}
extern "C" int ptl_seq_smoother_enable(ptl_seq* s, int32_t on) {
    if (!s) return set_err(PTL_ERR_ARG, "null argument");
    if (!s->cfg.with_ekf) return set_err(PTL_ERR_STATE, "ptl_seq_smoother_enable: an ICP-only sequence (with_ekf = 0) has no filter to smooth");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return ekf_log_set(s->lane.ekf, on ? s->cfg.n_scans : 0);
}
extern "C" int ptl_seq_smooth(ptl_seq* s, double* poses16, double* ts, double* nav19, double* cov324, int64_t* n_rows) {
    if (!s || !poses16) return set_err(PTL_ERR_ARG, "null argument");
    if (!s->cfg.with_ekf) return set_err(PTL_ERR_STATE, "ptl_seq_smooth: an ICP-only sequence has no filter to smooth");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return ekf_smooth_impl(s->lane.ekf, "ptl_seq_smooth", poses16, ts, nav19, cov324, s->cfg.n_scans, n_rows);
}
extern "C" int ptl_seq_smoother_log(ptl_seq* s, double* entries, int64_t max_entries, int64_t* n_entries, int32_t* overflow) {
    if (!s || max_entries < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return lane_smoother_log(s->lane, s->cfg, "ptl_seq_smoother_log", entries, max_entries, n_entries, overflow);
}
// IMU deskew for the sequence's scans
extern "C" int ptl_seq_imu_deskew_enable(ptl_seq* s, int32_t on, int64_t knot_capacity) {
    if (!s) return set_err(PTL_ERR_ARG, "null argument");
    int rc = dk_enable_check(s->cfg, &s->lane, 1, on, knot_capacity, "ptl_seq_imu_deskew_enable");
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(s->lane.icp->map_stream));
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    s->dk_on = false;
    if (on && !s->ev_pro) HIPCHK(s->ev_pro.create());
    rc = lane_dk_set(s->lane, s->cfg.n_scans, on ? knot_capacity : 0);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->dk_on = on && rc == PTL_OK;
    return rc;
}
extern "C" int ptl_seq_upload_sweep_times(ptl_seq* s, const double* t0t1) {
    if (!s || !t0t1) return set_err(PTL_ERR_ARG, "null argument");
    if (!s->dk_on) return set_err(PTL_ERR_STATE, "ptl_seq_upload_sweep_times: IMU deskew is not enabled");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return lane_upload_sweep_times(s->lane, s->cfg.n_scans, t0t1, "ptl_seq_upload_sweep_times");
}
extern "C" int ptl_seq_deskew_modes(ptl_seq* s, int32_t* modes, int64_t max_n, int64_t* n) {
    if (!s || !modes || max_n < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return lane_deskew_modes(s->lane, s->cfg, s->dk_on, s->n_out, modes, max_n, n);
}
extern "C" int ptl_seq_knots(ptl_seq* s, double* knots, int64_t max_knots, int64_t* n_knots, int32_t* overflow) {
    if (!s || max_knots < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    return lane_knots(s->lane, s->cfg, "ptl_seq_knots", knots, max_knots, n_knots, overflow);
}
extern "C" int ptl_seq_copy_traj(ptl_seq* s, void* dst_device, int64_t max_rows, int64_t* rows) {
    if (!s || !dst_device) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    return lane_copy_traj(s->lane, s->cfg, s->n_out, s->stream, dst_device, max_rows, rows);
}
extern "C" int ptl_device_sync(int device_id) {
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipDeviceSynchronize());
    return PTL_OK;
}
extern "C" int ptl_seq_results(ptl_seq* s, double* res_poses, double* res_t, double* kiss_poses, ptl_icp_stats* stats,
                               int64_t max_n, int64_t* n_out) {
    if (!s) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    return lane_results(s->lane, s->cfg.with_ekf != 0, s->n_out, res_poses, res_t, kiss_poses, stats, max_n, n_out);
}
extern "C" int ptl_seq_traj_device(ptl_seq* s, void** dev_ptr, int64_t* rows) {
    if (!s || !dev_ptr || !rows) return set_err(PTL_ERR_ARG, "null argument");
    *dev_ptr = s->lane.d_rows;
    *rows = s->n_out;
    return PTL_OK;
}
extern "C" int ptl_seq_icp(ptl_seq* s, ptl_icp** icp) {
    if (!s || !icp) return set_err(PTL_ERR_ARG, "null argument");
    *icp = s->lane.icp;
    return PTL_OK;
}
extern "C" int ptl_seq_profile(ptl_seq* s, int enable, double* gn_ms_total, int64_t* gn_launches, int reset) {
    if (!s) return set_err(PTL_ERR_ARG, "null argument");
    return ptl_icp_profile(s->lane.icp, enable, gn_ms_total, gn_launches, reset);
}

// ================================================================================================ batched runner
// S independent sequences on ONE GPU.  Two drivers over the same stage bodies:
//   free-running (default with gn_lanes_per_point = 8): one persistent launch (kx_seq_run, seq_kernel.h) carries up to
//     scans_per_launch scans of every sequence; each sequence's workgroups walk its pipeline at their own pace;
//   lockstep: every stage is one launch for all S scans (blockIdx.y = sequence), the S Gauss-Newton loops share one
//     persistent launch, and a step lasts as long as its slowest sequence.
struct ptl_batch {
    ptl_seq_cfg cfg;
    int S = 0;
    Stream stream;
    // the map update and the filter step of scan k run on `side` beside K0-K4 of scan k + 1 (both need only the GN result);
    // the GN launch of scan k + 1 waits for them
    Stream side;
    Event ev_gn, ev_side;
    bool ev_side_valid = false;
    // IMU deskew (ptl_batch_imu_deskew_enable): on for every sequence (their sweep times and modes: the lanes); the lockstep driver's prologue
    // waits for `ev_filter`, recorded behind the filter step
    bool dk_on = false;
    Event ev_filter;
    bool ev_filter_valid = false;
    GnTimer prof;                // the dominant kernel's launches
    DevOwner mem;                // the batch's own buffers and the pinned flag words
    SeqLane lane[GN_MAX_SEQ];    // sweep slots: [ring][pps][3] f32, or [ring][pps] u32 with range_input (declared behind what must outlive the lanes)
    unsigned* d_bar = nullptr;   // [SEQ_MAX_TEAMS][64] barrier counters and job words of the free-running kernel's teams
    SeqSched* d_sched = nullptr; // [8] its per-XCD scan schedulers
    int *d_flags = nullptr, *h_flags = nullptr;  // [GN_MAX_SEQ + 1] error flags of every sequence + the status word, gathered by k_finish_all (h_flags: pinned)
    unsigned* d_status = nullptr;  // one sticky word: why teams of the free-running kernel left a launch early (SEQ_EXIT_*), cleared by a reset
    int force_agent = 0;         // PTL_TEAM_SYNC=agent in the environment when the batch was created: no XCD-local barrier shortcut
    int balance_margin = 1;      // PTL_SCHED_MARGIN (default 1; -1 = a team looks abroad only when its own XCD has nothing for it): seq_kernel.h SeqRun
    int dbg_dead_block = -1, dbg_dead_round = -1;  // test hook: ptl_batch_debug_stall_block
    int um_alt = 0;              // test hook: ptl_batch_debug_set_map_points_per_thread
    bool free_running = false;
    int team_wgs = 0;            // workgroups per team of the free-running kernel (0 = by the number of sequences, batch_gseq)
    bool seq_run_checked = false;
    int64_t scans_per_launch = 256;
    unsigned char is_range = 0;
    ptl_lut* lut = nullptr;
    SeqCtx* d_ctx = nullptr;
    int64_t next_scan = 0, n_out = 0;
    // Sweep ring (ptl_seq_cfg.resident_scans, round 6): the batch keeps `ring` sweep slots per sequence (ring == n_scans: every sweep resident, as
    // before); scan k lives in slot k % ring.  ring_lap = the lap d_ctx's scan_base is set for (a launch never crosses a lap: enqueue splits there).
    // up_hi[s] = sweeps of sequence s uploaded so far (in order); done_scans = scans whose launches are known complete (ptl_batch_wait).  Both are
    // atomics: uploads may run on another host thread while ptl_batch_wait blocks.
    int64_t ring = 0, ring_lap = 0;
    std::atomic<int64_t> up_hi[GN_MAX_SEQ] = {};
    std::atomic<int64_t> done_scans{0};
    bool ctx_dirty = true;
    // fixed-interval smoother (ptl_batch_smoother_enable): one k_ekf_smooth job per sequence, their status words side by side
    EkfSmoothJob* d_sm_jobs = nullptr;
    long long* d_sm_info = nullptr;
    std::vector<long long> h_sm_info;
    bool sm_done = false;  // the last ptl_batch_smooth succeeded and nothing ran since
};

// launch geometry: workgroups per team.  Lockstep (kx_assign): one team per sequence, 1 / 2 / 4 per XCD.  Free-running: 1 / 2 / 4
// teams per XCD for up to 8 / 16 / 64 sequences as before (a team of 8 workgroups of 512 threads at the default 256 workgroups),
// 8 teams up to 128 sequences, 16 beyond; ptl_batch_set_team_workgroups overrides.  Smaller teams pay the per-iteration
// fixed costs (workgroup reduction, exchange, solve) over more points each and need more sequences to stay busy.
static int batch_gseq(const ptl_batch* b) {
    if (b->free_running && b->team_wgs > 0) return b->team_wgs;
    const int J = b->cfg.icp.gn_workgroups / 8;
    if (!b->free_running || b->S <= 64) return J / (b->S <= 8 ? 1 : b->S <= 16 ? 2 : 4);
    const int g = J / (b->S <= 128 ? 8 : 16);
    return g < 1 ? 1 : g;
}
// every workgroup of the persistent launch has to be resident (they wait for each other); a team needs a workgroup
// beside the filter's
static int batch_check_seq_run(ptl_batch* b) {
    const ptl_icp_cfg& ic = b->cfg.icp;
    if (ic.gn_lanes_per_point != 8) return set_err(PTL_ERR_ARG, "free-running batches use the 8-lane Gauss-Newton kernel (gn_lanes_per_point = 8)");
    const int gseq = batch_gseq(b), J = ic.gn_workgroups / 8;
    if (gseq < 1 || gseq > J || gseq > 64) return set_err(PTL_ERR_ARG, "a team needs 1 .. min(64, gn_workgroups / 8 = %d) workgroups, not %d", J, gseq);
    if (b->S > 8 * SEQ_SLOTS) return set_err(PTL_ERR_ARG, "at most %d sequences", 8 * SEQ_SLOTS);
    // the look-back words of the one-pass compactions tell a stale count from this scan's by a 16-bit tag (scan % 65535 + 1, lookback_tag):
    // a run must not come back to a tag it has used
    if (b->cfg.n_scans >= 65535) return set_err(PTL_ERR_ARG, "free-running batches run at most 65534 scans per sequence (look-back tags of the compaction passes)");
    if (b->cfg.with_ekf && ic.gn_threads < 384) return set_err(PTL_ERR_ARG, "free-running batches with a filter need gn_threads >= 384 (the filter step maps one thread to each of the 324 covariance cells)");
    int per_cu = 0, cus = 0;
    hipError_t e = hipSuccess;
    pick_p(ic.max_points_per_voxel, [&](auto pc) {
        pick_team<32, 16, 8, 4, 2, 1>(gseq, [&](auto gc) { e = resident_capacity(kx_seq_run<pc(), gc()>, ic.gn_threads, ic.device_id, &per_cu, &cus); });
    });
    if (e != hipSuccess) return set_err(PTL_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));
    if ((int64_t)per_cu * cus < ic.gn_workgroups)
        return set_err(PTL_ERR_STATE, "free-running batch: %d workgroups x %d threads cannot be co-resident on device %d (%d CUs x %d per CU): lower gn_workgroups",
                       ic.gn_workgroups, ic.gn_threads, ic.device_id, cus, per_cu);
    return PTL_OK;
}
extern "C" int ptl_batch_destroy(ptl_batch* b) { return b ? handle_destroy(b, b->cfg.icp.device_id) : PTL_OK; }
extern "C" int ptl_batch_create(const ptl_seq_cfg* cfg, int32_t n_sequences, ptl_batch** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "null argument");
    if (n_sequences < 1 || n_sequences > GN_MAX_SEQ) return set_err(PTL_ERR_ARG, "n_sequences must be in [1, %d]", GN_MAX_SEQ);
    ptl_seq_cfg c;
    int rc = seq_cfg_settle(cfg, &c);
    if (rc) return rc;
    if ((c.icp.gn_workgroups & 31) || c.icp.gn_workgroups > 512) return set_err(PTL_ERR_ARG, "batched runs need gn_workgroups = a multiple of 32 (8 XCDs x up to 4 sequences each), at most 512");
    if (c.resident_scans < 0 || c.resident_scans == 1) return set_err(PTL_ERR_ARG, "resident_scans must be 0 (every sweep resident) or >= 2 sweep slots per sequence");
    const int64_t ring = (c.resident_scans > 0 && c.resident_scans < c.n_scans) ? c.resident_scans : c.n_scans;
    const size_t slot = (size_t)c.points_per_scan * (c.range_input ? 4 : 12);  // resident bytes of a sweep
    {   // the whole batch has to fit the device: say so here, with numbers, instead of failing part-way through the allocations
        // (what a member's allocation functions ask for, plus slack for the granularity of the runtime's own allocations)
        size_t icp_bytes = 0;
        const size_t per_seq = lane_footprint_bytes(c, slot, (size_t)ring, &icp_bytes) + (1u << 20) + (64u << 10);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && per_seq * (size_t)n_sequences > free_b)
            return set_err(PTL_ERR_CAPACITY, "batch of %d sequences needs %.1f GB of device memory (%.0f MB per sequence: %.0f MB of work buffers, map table "
                           "and block pool, %.0f MB of sweeps), %.1f GB are free of %.1f GB: fewer sequences, fewer resident sweeps or a smaller map_block_capacity",
                           n_sequences, per_seq * (double)n_sequences / 1e9, per_seq / 1e6, icp_bytes / 1e6,
                           (double)ring * slot / 1e6, free_b / 1e9, total_b / 1e9);
    }
    const bool free_running = c.icp.gn_lanes_per_point == 8;
    if (!free_running && c.icp.map_small_blocks > 0) return set_err(PTL_ERR_ARG, "map_small_blocks (two block classes) needs the free-running driver (gn_lanes_per_point = 8)");
    if (ring < c.n_scans && !free_running) return set_err(PTL_ERR_ARG, "resident_scans (the sweep ring) is served by the free-running driver (gn_lanes_per_point = 8)");
    std::unique_ptr<ptl_batch> owner(new ptl_batch());
    ptl_batch* b = owner.get();
    b->cfg = c;
    b->S = n_sequences;
    b->free_running = free_running;
    b->ring = ring;
    {   // PTL_TEAM_SYNC=agent: the teams of the free-running kernel keep the agent-scope release at every barrier (seq_kernel.h team_sync)
        const char* e = getenv("PTL_TEAM_SYNC");
        b->force_agent = (e && strcmp(e, "agent") == 0) ? 1 : 0;
        const char* m = getenv("PTL_SCHED_MARGIN");
        b->balance_margin = (m && *m) ? atoi(m) : 1;
        if (b->balance_margin < -1 || b->balance_margin > 4096) b->balance_margin = 1;
    }
    if (b->stream.create() != hipSuccess || b->side.create() != hipSuccess || b->ev_gn.create() != hipSuccess || b->ev_side.create() != hipSuccess)
        return set_err(PTL_ERR_HIP, "stream / event creation failed");
    for (int s = 0; s < b->S && rc == PTL_OK; ++s) rc = lane_create(b->lane[s], c, b->stream, b->stream, slot, (size_t)ring, true, "ptl_batch_create");
    if (rc == PTL_OK) {
        DevOwner& m = b->mem;
        m.add(&b->d_ctx, (size_t)GN_MAX_SEQ); m.add(&b->d_bar, (size_t)SEQ_MAX_TEAMS * 64); m.add(&b->d_sched, (size_t)8);
        m.add(&b->d_status, (size_t)16);
        m.add(&b->d_flags, (size_t)GN_MAX_SEQ + 1); m.add_pinned(&b->h_flags, (size_t)GN_MAX_SEQ + 1);
        if (m.err != hipSuccess || hipMemset(b->d_status, 0, m.bytes_of(b->d_status)) != hipSuccess) rc = set_err(PTL_ERR_HIP, "batch allocation failed");
    }
    // (the free-running driver's own limits - co-residency of the persistent grid, team size - are checked when that driver is
    // chosen or first used: a batch that is switched to lockstep right after creation must not be refused on them)
    if (rc) return rc;
    *out = owner.release();
    return PTL_OK;
}
// Sweep ring (resident_scans < n_scans): sweeps arrive in order, and sweep k may take its slot (k % ring) only when the scan that used the slot
// before - k - ring - is known to be complete (ptl_batch_wait has returned for it).  Uploads of later sweeps may run while a launch works on
// earlier ones - from the thread that enqueued it, between ptl_batch_enqueue and ptl_batch_wait, or from another host thread.
static int batch_ring_slot_free(ptl_batch* b, int32_t s, int64_t k) {
    if (b->ring >= b->cfg.n_scans) return PTL_OK;
    const int64_t hi = b->up_hi[s], done = b->done_scans;
    if (k != hi) return set_err(PTL_ERR_STATE, "sweep ring (resident_scans = %lld): sweeps are uploaded in order - sequence %d expects sweep %lld, got %lld",
                                (long long)b->ring, s, (long long)hi, (long long)k);
    if (k >= done + b->ring) return set_err(PTL_ERR_STATE, "sweep ring (resident_scans = %lld): slot of sweep %lld still holds sweep %lld, which is not known to be done "
                                            "(%lld scans complete): ptl_batch_wait first", (long long)b->ring, (long long)k, (long long)(k - b->ring), (long long)done);
    return PTL_OK;
}
extern "C" int ptl_batch_upload_scan(ptl_batch* b, int32_t s, int64_t k, const float* xyz) {
    if (!b || !xyz || s < 0 || s >= b->S || k < 0 || k >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    if (b->is_range || b->cfg.range_input) return set_err(PTL_ERR_STATE, "this batch holds range images");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    int rc = batch_ring_slot_free(b, s, k);
    if (rc) return rc;
    const size_t bytes = (size_t)b->cfg.points_per_scan * 12;
    HIPCHK(hipMemcpy((char*)b->lane[s].d_scans + (size_t)(k % b->ring) * bytes, xyz, bytes, hipMemcpyHostToDevice));
    if (b->ring < b->cfg.n_scans) b->up_hi[s] = k + 1;
    return PTL_OK;
}
extern "C" int ptl_batch_upload_range(ptl_batch* b, int32_t s, int64_t k, const uint32_t* range_mm) {
    if (!b || !range_mm || s < 0 || s >= b->S || k < 0 || k >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    if (!b->lut) return set_err(PTL_ERR_STATE, "set the LUT first (ptl_batch_set_lut)");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    int rc = batch_ring_slot_free(b, s, k);
    if (rc) return rc;
    const size_t slot = (size_t)b->cfg.points_per_scan * (b->cfg.range_input ? 4 : 12);
    HIPCHK(hipMemcpy((char*)b->lane[s].d_scans + (size_t)(k % b->ring) * slot, range_mm, (size_t)b->cfg.points_per_scan * 4, hipMemcpyHostToDevice));
    if (b->ring < b->cfg.n_scans) b->up_hi[s] = k + 1;
    return PTL_OK;
}
extern "C" int ptl_batch_set_lut(ptl_batch* b, ptl_lut* lut, int32_t active_beams) {
    if (!b || !lut) return set_err(PTL_ERR_ARG, "null argument");
    if ((int64_t)lut->H * lut->W != b->cfg.points_per_scan || lut->W != b->cfg.icp.scan_cols) return set_err(PTL_ERR_ARG, "LUT size does not match the batch");
    b->lut = lut;
    b->is_range = 1;
    b->ctx_dirty = true;
    for (int s = 0; s < b->S; ++s) { int rc = ptl_icp_set_active_beams(b->lane[s].icp, lut->H, active_beams); if (rc) return rc; }
    return PTL_OK;
}
extern "C" int ptl_batch_upload_imu(ptl_batch* b, int32_t s, const double* imu, const int64_t* imu_end) {
    if (!b || !imu_end || s < 0 || s >= b->S || (!imu && b->cfg.n_imu > 0)) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    return lane_upload_imu(b->lane[s], b->cfg, imu, imu_end, b->cfg.with_ekf != 0);
}
static int batch_push_ctx(ptl_batch* b) {
    std::vector<SeqCtx> hv((size_t)GN_MAX_SEQ);
    SeqCtx* h = hv.data();
    memset(h, 0, sizeof(SeqCtx) * GN_MAX_SEQ);
    const bool with_ekf = b->cfg.with_ekf != 0;
    for (int s = 0; s < b->S; ++s) {
        Ctx c = b->lane[s].icp->c;
        c.in_f32 = nullptr; c.in_f64 = nullptr; c.in_range = nullptr; c.t01 = nullptr;
        c.n_in = (int)b->cfg.points_per_scan;
        c.overlap_pre = 1;  // the prologue of scan k + 1 runs beside the map update of scan k (side stream)
        c.ext_guess = (with_ekf && b->cfg.use_imu_prediction) ? (const double*)((char*)b->lane[s].ekf->st + offsetof(EkfState, pose)) : nullptr;
        if (b->is_range) { c.lut_dir = b->lut->dir; c.lut_off = b->lut->off; c.row_mask = b->lane[s].icp->d_row_mask; }
        h[s].c = c;
        h[s].scan_stride_floats = (long long)b->cfg.points_per_scan * (b->cfg.range_input ? 1 : 3);
        // (sweep ring: scan k of lap L = k / ring sits in slot k - L ring; the kernel addresses scan_base + k stride, so the base moves back a ring per lap)
        h[s].scan_base = b->lane[s].d_scans - (long long)b->ring_lap * (long long)b->ring * h[s].scan_stride_floats;
        h[s].input_is_range = b->is_range;
        h[s].n_scans = (int)b->cfg.n_scans;
        h[s].fd_buf[0] = b->lane[s].icp->fd_buf[0]; h[s].fd_buf[1] = b->lane[s].icp->fd_buf[1];
        h[s].ekf = b->lane[s].ekf->st; h[s].imu = b->lane[s].d_imu; h[s].imu_end = b->lane[s].d_imu_end;
        h[s].res_poses = b->lane[s].d_res_poses; h[s].res_t = b->lane[s].d_res_t; h[s].rows = b->lane[s].d_rows;
    }
    HIPCHK(hipMemcpyAsync(b->d_ctx, h, sizeof(SeqCtx) * GN_MAX_SEQ, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->ctx_dirty = false;
    return PTL_OK;
}
static int batch_reset(ptl_batch* b) {
    for (int s = 0; s < b->S; ++s) {
        int rc = icp_reset_device(b->lane[s].icp);
        if (rc) return rc;
        rc = ekf_reset(b->lane[s].ekf);
        if (rc) return rc;
        b->lane[s].imu_pos = 0;
    }
    b->next_scan = 0;
    b->n_out = 0;
    b->done_scans = 0;
    b->sm_done = false;
    if (b->ring_lap != 0) { b->ring_lap = 0; b->ctx_dirty = true; }
    if (b->ring < b->cfg.n_scans)  // a ring that has been lapped no longer holds the run's first sweeps: they are uploaded again; else what is there stays
        for (int s = 0; s < b->S; ++s) if (b->up_hi[s] > b->ring) b->up_hi[s] = 0;
    HIPCHK(hipMemsetAsync(b->d_status, 0, sizeof(unsigned), b->stream));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->ev_side_valid = false;
    b->ev_filter_valid = false;
    return PTL_OK;
}
// IMU deskew: sweep times of every sequence, knots enough for the IMU samples between two scans
static int batch_dk_check(ptl_batch* b) {
    for (int s = 0; b->dk_on && s < b->S; ++s) {
        const int rc = lane_dk_ready(b->lane[s], "ptl_batch_enqueue", s);
        if (rc) return rc;
    }
    return PTL_OK;
}
__global__ void k_ring_rebase(SeqCtx* a, int S, long long delta_floats) {
    const int s = (int)threadIdx.x;
    if (s < S) a[s].scan_base += delta_floats;
}
// The filter's argument block for the `ns` sequences from `l` on: each filter's IMU rows from where it stands (imu_pos) up to the samples
// before scan `stop_scan` (< 0: none), and where it stands moves there.  out_row >= 0: the step starts with the update by the registration's
// pose of that output row and writes that row of the results.  Returns whether any sequence has samples to run.
static bool ekf_args_fill(EkfBatchArgs& ea, SeqLane* l, int ns, int64_t stop_scan, int64_t out_row = -1) {
    memset(&ea, 0, sizeof ea);
    bool any = false;
    for (int q = 0; q < ns; ++q, ++l) {
        const int64_t i1 = stop_scan >= 0 ? l->imu_end[(size_t)stop_scan] : l->imu_pos;
        ea.e[q] = l->ekf->st; ea.imu[q] = l->d_imu;
        ea.i0[q] = (int)l->imu_pos; ea.i1[q] = (int)i1;
        any = any || i1 > l->imu_pos;
        if (out_row >= 0) {
            ea.pose[q] = l->icp->c.traj + 16 * out_row;
            ea.out_pose[q] = l->d_res_poses + 16 * out_row; ea.out_t[q] = l->d_res_t + out_row; ea.out_row8[q] = l->d_rows + 8 * out_row;
        }
        if (out_row >= 0 || i1 > l->imu_pos) l->imu_pos = i1;
    }
    ea.update_first = out_row >= 0 ? 1 : 0;
    return any;
}
// free-running driver: the scans [next_scan, next_scan + n) of every sequence in launches of up to scans_per_launch scans
static int batch_enqueue_free(ptl_batch* b, int64_t n) {
    const bool with_ekf = b->cfg.with_ekf != 0;
    const int S = b->S;
    const ptl_icp_cfg& ic = b->cfg.icp;
    hipStream_t st = b->stream;
    const int64_t end = b->next_scan + n;
    if (!b->seq_run_checked) { int rc = batch_check_seq_run(b); if (rc) return rc; b->seq_run_checked = true; }
    if (b->ring < b->cfg.n_scans)
        for (int s = 0; s < S; ++s)
            if (b->up_hi[s] < end) return set_err(PTL_ERR_STATE, "sweep ring: sequence %d has sweeps [0, %lld) uploaded, the launch needs [%lld, %lld)", s, (long long)b->up_hi[s].load(),
                                                  (long long)b->next_scan, (long long)end);
    while (b->next_scan < end) {
        const int64_t k0 = b->next_scan;
        int64_t k1 = (end - k0 > b->scans_per_launch) ? k0 + b->scans_per_launch : end;
        if (b->ring < b->cfg.n_scans) {  // a launch stays inside one lap of the ring (its sweeps are contiguous there)
            const int64_t lap = k0 / b->ring, lap_end = (lap + 1) * b->ring;
            if (k1 > lap_end) k1 = lap_end;
            if (lap != b->ring_lap) {
                k_ring_rebase<<<1, GN_MAX_SEQ, 0, st>>>(b->d_ctx, S, -(long long)(lap - b->ring_lap) * (long long)b->ring * (long long)b->cfg.points_per_scan * (b->cfg.range_input ? 1 : 3));
                b->ring_lap = lap;
            }
        }
        if (with_ekf) {  // IMU samples before the first scan of the launch that the filter has not seen (a run's first scan)
            for (int s0 = 0; s0 < S; s0 += EKF_MAX_SEQ) {  // (the argument block holds EKF_MAX_SEQ sequences)
                EkfBatchArgs ea;
                const int ns = S - s0 < EKF_MAX_SEQ ? S - s0 : EKF_MAX_SEQ;
                if (ekf_args_fill(ea, b->lane + s0, ns, k0)) kb_ekf_step<<<ns, 384, 0, st>>>(ea);
            }
        }
        HIPCHK(hipMemsetAsync(b->d_bar, 0, (size_t)SEQ_MAX_TEAMS * 64 * sizeof(unsigned), st));
        k_sched_init<<<1, 8 * SEQ_SLOTS, 0, st>>>(b->d_sched, S, (int)k0, (int)k1);
        HIPCHK(b->prof.begin(st));
        SeqRun r;
        r.S = S; r.k0 = (int)k0; r.k1 = (int)k1; r.with_ekf = with_ekf ? 1 : 0; r.rebuild_every = ic.rebuild_every;
        const int gseq = batch_gseq(b);
        r.G = gseq;
        r.um_alt = b->um_alt;
        r.balance_margin = b->balance_margin;
        r.force_agent = b->force_agent; r.dbg_dead_block = b->dbg_dead_block; r.dbg_dead_round = b->dbg_dead_round;
        pick_p(ic.max_points_per_voxel, [&](auto pc) {
            pick_team<32, 16, 8, 4, 2, 1>(gseq, [&](auto gc) { kx_seq_run<pc(), gc()><<<ic.gn_workgroups, ic.gn_threads, 0, st>>>(b->d_ctx, r, b->d_sched, b->d_bar, b->d_status); });
        });
        HIPCHK(b->prof.end(st));
        // did every sequence reach scan k1?  (a team may have left the launch while holding one: no exit is silent)
        k_sched_check<<<1, 8 * SEQ_SLOTS, 0, st>>>(b->d_ctx, b->d_sched, S, (int)k1, b->d_status);
        for (int s = 0; s < S; ++s) {
            if (with_ekf) b->lane[s].imu_pos = (k1 < b->cfg.n_scans) ? b->lane[s].imu_end[(size_t)k1] : b->lane[s].imu_end[(size_t)k1 - 1];
            b->lane[s].icp->scans_done += (k1 - k0);
            b->lane[s].icp->last_n = b->cfg.points_per_scan;
        }
        b->n_out += k1 - k0;
        b->next_scan = k1;
    }
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// back to the cold start (empty maps, fresh filters, scan 0 next) without running anything: what ptl_batch_run does first; after it the
// driver and the team size may be chosen again
extern "C" int ptl_batch_reset(ptl_batch* b) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    return batch_reset(b);
}
extern "C" int ptl_batch_set_driver(ptl_batch* b, int32_t free_running, int64_t scans_per_launch) {
    if (!b || scans_per_launch < 0) return set_err(PTL_ERR_ARG, "bad argument");
    if (b->next_scan != 0) return set_err(PTL_ERR_STATE, "choose the driver before the first scan of a run");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    if (scans_per_launch > 4096) return set_err(PTL_ERR_ARG, "scans_per_launch: at most 4096 (every wait inside the persistent kernel has a poll budget worth seconds, and a launch must stay well below it)");
    if (scans_per_launch > 0) b->scans_per_launch = scans_per_launch;
    if (!free_running && b->cfg.icp.map_small_blocks > 0) return set_err(PTL_ERR_ARG, "map_small_blocks (two block classes) needs the free-running driver");
    if (!free_running && b->ring < b->cfg.n_scans) return set_err(PTL_ERR_ARG, "resident_scans (the sweep ring) needs the free-running driver");
    const bool was = b->free_running;
    b->free_running = free_running != 0;
    b->seq_run_checked = false;
    if (free_running) { int rc = batch_check_seq_run(b); if (rc) { b->free_running = was; return rc; } b->seq_run_checked = true; }
    return PTL_OK;
}
// workgroups per team of the free-running kernel (0 = the default for the number of sequences, batch_gseq); before the first scan of a run
extern "C" int ptl_batch_set_team_workgroups(ptl_batch* b, int32_t team_workgroups) {
    if (!b || team_workgroups < 0) return set_err(PTL_ERR_ARG, "bad argument");
    if (b->next_scan != 0) return set_err(PTL_ERR_STATE, "choose the team size before the first scan of a run");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    const int was = b->team_wgs;
    b->team_wgs = team_workgroups;
    b->seq_run_checked = false;
    if (b->free_running) { int rc = batch_check_seq_run(b); if (rc) { b->team_wgs = was; return rc; } b->seq_run_checked = true; }
    return PTL_OK;
}
extern "C" int ptl_batch_team_workgroups(ptl_batch* b, int32_t* team_workgroups, int32_t* teams) {
    if (!b || !team_workgroups) return set_err(PTL_ERR_ARG, "null argument");
    const int g = batch_gseq(b);
    *team_workgroups = g;
    if (teams) {  // teams that can get work: per XCD min(workgroups / team size, its sequences)
        int n = 0;
        for (int x = 0; x < 8 && x < b->S; ++x) { const int per = (b->cfg.icp.gn_workgroups / 8) / (g > 0 ? g : 1), ns = (b->S - x + 7) / 8; n += per < ns ? per : ns; }
        *teams = n;
    }
    return PTL_OK;
}
extern "C" int ptl_batch_enqueue(ptl_batch* b, int64_t n) {
    if (!b || n < 0 || b->next_scan + n > b->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    b->sm_done = false;
    if (b->ctx_dirty) { int rc = batch_push_ctx(b); if (rc) return rc; }
    { int rc = batch_dk_check(b); if (rc) return rc; }
    if (b->free_running) return batch_enqueue_free(b, n);
    if (b->S > 32) return set_err(PTL_ERR_ARG, "the lockstep driver serves up to 32 sequences (four per XCD); %d need the free-running one", b->S);
    if (b->cfg.icp.map_small_blocks > 0) return set_err(PTL_ERR_ARG, "map_small_blocks (two block classes) needs the free-running driver");
    const bool with_ekf = b->cfg.with_ekf != 0;
    const int S = b->S;
    const int64_t pps = b->cfg.points_per_scan;
    const int nb = (int)((pps + 255) / 256);
    const ptl_icp_cfg& ic = b->cfg.icp;
    hipStream_t st = b->stream;
    const int64_t end = b->next_scan + n;
    for (int64_t k = b->next_scan; k < end; ++k) {
        if (with_ekf) {  // IMU samples before the first scan of a run (later ones ride on the previous scan's EKF launch)
            EkfBatchArgs ea;
            if (ekf_args_fill(ea, b->lane, S, k)) {
                if (b->ev_side_valid) HIPCHK(hipStreamWaitEvent(st, b->ev_side, 0));
                kb_ekf_step<<<S, 384, 0, st>>>(ea);
            }
        }
        const int ki = (int)k;
        if (b->dk_on && b->ev_filter_valid) HIPCHK(hipStreamWaitEvent(st, b->ev_filter, 0));  // IMU deskew: the table needs the sweep's knots
        if (b->dk_on) kb_scan_prologue_imu<<<dim3(1, S), 1024, 0, st>>>(b->d_ctx, ki);
        else kb_scan_prologue<<<dim3(1, S), 1024, 0, st>>>(b->d_ctx, ki);
        kb_deskew_vds1<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        kb_count_w1<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        kb_compact_fd<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        kb_vds2_fd<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        kb_count_w2<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        kb_compact_src<<<dim3(nb, S), 256, 0, st>>>(b->d_ctx, ki);
        if (b->ev_side_valid) HIPCHK(hipStreamWaitEvent(st, b->ev_side, 0));  // the previous scan's map update and filter step
        HIPCHK(b->prof.begin(st));
        // one sequence per XCD: workgroups with blockIdx & 7 == s run sequence s's loop with gn_workgroups / 8 workgroups
        pick_p(ic.max_points_per_voxel, [&](auto pc) {
            const int gseq = (ic.gn_workgroups / 8) / (S <= 8 ? 1 : S <= 16 ? 2 : 4);  // workgroups per sequence
            if (ic.gn_lanes_per_point == 8) pick_team<32, 16, 8, 4, 2, 1>(gseq, [&](auto gc) { kx_gn_loop8<pc(), gc()><<<ic.gn_workgroups, ic.gn_threads, 0, st>>>(b->d_ctx, S, ki); });
            else kx_gn_loop<pc()><<<ic.gn_workgroups, ic.gn_threads, 0, st>>>(b->d_ctx, S, ki);
        });
        HIPCHK(b->prof.end(st));
        HIPCHK(hipEventRecord(b->ev_gn, st));
        hipStream_t sd = b->side;
        HIPCHK(hipStreamWaitEvent(sd, b->ev_gn, 0));
        const int64_t o = b->n_out;
        if (with_ekf) {  // first: its pose is the next scan's guess
            EkfBatchArgs ea;
            ekf_args_fill(ea, b->lane, S, (k + 1 < b->cfg.n_scans) ? k + 1 : -1, o);
            kb_ekf_step<<<S, 384, 0, sd>>>(ea);
            if (b->dk_on) { HIPCHK(hipEventRecord(b->ev_filter, sd)); b->ev_filter_valid = true; }
        }
        kb_map_insert_a<<<dim3(nb, S), 256, 0, sd>>>(b->d_ctx, ki);
        kb_map_insert_b<<<dim3(nb, S), 256, 0, sd>>>(b->d_ctx, ki);
        kb_map_insert_c<<<dim3(nb, S), 256, 0, sd>>>(b->d_ctx, ki);
        kb_map_prune<<<dim3((unsigned)((ic.map_block_capacity + 255) / 256), S), 256, 0, sd>>>(b->d_ctx, ki);
        for (int s = 0; s < S; ++s) { b->lane[s].icp->scans_done++; b->lane[s].icp->last_n = pps; }
        b->n_out++;
        b->next_scan = k + 1;
        if (ic.rebuild_every > 0 && (b->n_out % ic.rebuild_every) == 0) {
            for (int s = 0; s < S; ++s) {
                HIPCHK(hipMemsetAsync(b->lane[s].icp->c.tab, 0xFF, ((size_t)b->lane[s].icp->c.tmask + 1) * sizeof(TabEnt), sd));
                HIPCHK(hipMemsetAsync(&b->lane[s].icp->c.st->tab_used, 0, sizeof(unsigned), sd));
            }
            kb_map_rebuild<<<dim3((unsigned)((ic.map_block_capacity + 255) / 256), S), 256, 0, sd>>>(b->d_ctx, ki);
        }
        HIPCHK(hipEventRecord(b->ev_side, sd));
        b->ev_side_valid = true;
    }
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// closes the last scan of EVERY sequence (what k_finish_scan does for one) and collects the error flags and the batch's status word in one
// array: one launch and one copy per wait instead of S launches and S + 1 copies (240 + 241 of them sat inside the bench's timed region:
// 3 % of a 20-step run)
__global__ void k_finish_all(const SeqCtx* a, int S, const unsigned* status, int* out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) out[GN_MAX_SEQ] = (int)*status;
    if (s >= S) return;
    const Ctx& c = a[s].c;
    finish_pending(c, c.st);
    flush_map_stats(c, c.st);
    out[s] = c.st->err_flags;
}
extern "C" int ptl_batch_wait(ptl_batch* b) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    if (b->ctx_dirty) { int rc = batch_push_ctx(b); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(b->side));
    k_finish_all<<<(b->S + 63) / 64, 64, 0, b->stream>>>(b->d_ctx, b->S, b->d_status, b->d_flags);
    HIPCHK(hipMemcpyAsync(b->h_flags, b->d_flags, (size_t)(GN_MAX_SEQ + 1) * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->done_scans = b->next_scan;  // (every launch enqueued so far is through: their sweep slots may be overwritten)
    const int* flags = b->h_flags;
    const unsigned status = (unsigned)b->h_flags[GN_MAX_SEQ];
    b->prof.collect();
    for (int s = 0; s < b->S; ++s)
        if (flags[s]) return set_err(PTL_ERR_CAPACITY, "sequence %d: " ERR_FLAGS_FMT "; batch status 0x%x", s, flags[s], status);
    // no sequence carries an error, but a team of the free-running kernel left a launch early (a workgroup that never reached a
    // barrier; teams that never got work): the scans are complete, the launch was not healthy - said, not swallowed
    // (a team that only ran out of its idle budget while the last sequences were in other teams' hands - bit 4 alone, every sequence at its last
    // scan - did no harm: the bit stays readable through ptl_batch_status, the wait does not fail on it)
    if (status & ~SEQ_EXIT_IDLE) return set_err(PTL_ERR_STATE, "free-running launch: teams left early, status 0x%x (1 head-of-launch barrier, 2 job barrier, 4 idle, 8 gave up on a sequence, 16 scans incomplete)", status);
    for (int s = 0; b->dk_on && s < b->S; ++s) {
        const int rc = lane_dk_overflow(b->lane[s], "ptl_batch_wait", s);
        if (rc) return rc;
    }
    return PTL_OK;
}
extern "C" int ptl_batch_status(ptl_batch* b, uint32_t* status) {
    if (!b || !status) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(status, b->d_status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PTL_OK;
}
// test hook: workgroup `block` of the free-running grid returns right before the job barrier of its `round`-th job (0 = the first
// of every launch from now on); block < 0 = none
extern "C" int ptl_batch_debug_stall_block(ptl_batch* b, int32_t block, int32_t round) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    b->dbg_dead_block = block; b->dbg_dead_round = block < 0 ? -1 : round;
    return PTL_OK;
}
// test hook: points per thread and pass of the free-running kernel's map update - the build's default (SEQ_UM, 8) or its second instance
// (SEQ_UM_ALT, 4); anything else is refused.  The result must not depend on it (tests/test_gpu_batch.py).  points_out: the value in effect.
extern "C" int ptl_batch_debug_set_map_points_per_thread(ptl_batch* b, int32_t points, int32_t* points_out) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    if (points != 0 && points != SEQ_UM && points != SEQ_UM_ALT) return set_err(PTL_ERR_ARG, "this build carries the map update at %d and %d points per thread", SEQ_UM, SEQ_UM_ALT);
    if (points != 0) b->um_alt = (points == SEQ_UM_ALT && SEQ_UM_ALT != SEQ_UM) ? 1 : 0;
    if (points_out) *points_out = b->um_alt ? SEQ_UM_ALT : SEQ_UM;
    return PTL_OK;
}
// where the scans of sequence s ran (free-running kernel), cumulative since the cold start: out[0] scans run by a team of another XCD than
// the sequence's home XCD (s & 7), out[1] scans that ran on another XCD than the sequence's previous scan, out[2] XCC id of the last scan + 1
extern "C" int ptl_batch_sched_counters(ptl_batch* b, int32_t s, uint64_t out[4]) {
    if (!b || !out || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(out, (char*)b->lane[s].icp->c.st + offsetof(DevState, sched_cnt), 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PTL_OK;
}
// compile-time constants of this build that callers' byte models depend on (bench.py EXEC_COST):
//   [0] GN8_KCAND  [1] doubles per answer row  [2] GN8_LDS_PTS  [3] SEQ_U  [4] SEQ_U2  [5] GN8_MAX_THREADS  [6] GN8_LPB  [7] GN8_SPEC
//   [8] GN8_SURV  [9] GN8_PREFETCH  [10] 1000 x GN8_KEEP  [11] bytes per map table entry  [12] bytes per VDS entry
//   [13] diagnostic flavours compiled in (diag.h): 1 PHASES | 2 IT0 | 4 STAGES | 8 MAP_DIAG, 0 = the product build
//   [15] POSE_CHUNK (pose_kernels.h)
#ifndef PTL_CODE_ID
#define PTL_CODE_ID "unknown"
#endif
extern "C" const char* ptl_code_id(void) { return PTL_CODE_ID; }
extern "C" int ptl_build_info(int32_t out[16]) {
    if (!out) return set_err(PTL_ERR_ARG, "null argument");
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = GN8_KCAND; out[1] = GN8_ANS_ROW; out[2] = GN8_LDS_PTS; out[3] = SEQ_U; out[4] = SEQ_U2; out[5] = GN8_MAX_THREADS;
    out[6] = GN8_LPB; out[7] = GN8_SPEC; out[8] = GN8_SURV; out[9] = GN8_PREFETCH; out[10] = (int32_t)(1000.0 * GN8_KEEP + 0.5);
    out[11] = (int32_t)sizeof(TabEnt); out[12] = (int32_t)sizeof(VdsEnt); out[13] = diag::flavours; out[14] = 0; out[15] = POSE_CHUNK;
    return PTL_OK;
}
extern "C" int ptl_batch_run(ptl_batch* b, int64_t n) {
    if (!b || n < 0 || n > b->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    int rc = batch_reset(b);
    if (rc) return rc;
    rc = ptl_batch_enqueue(b, n);
    if (rc) return rc;
    return ptl_batch_wait(b);
}
extern "C" int ptl_batch_results(ptl_batch* b, int32_t s, double* res_poses, double* res_t, double* kiss_poses,
                                 ptl_icp_stats* stats, int64_t max_n, int64_t* n_out) {
    if (!b || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    return lane_results(b->lane[s], b->cfg.with_ekf != 0, b->n_out, res_poses, res_t, kiss_poses, stats, max_n, n_out);
}
extern "C" int ptl_batch_smoother_enable(ptl_batch* b, int32_t on) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    if (!b->cfg.with_ekf) return set_err(PTL_ERR_STATE, "ptl_batch_smoother_enable: ICP-only sequences (with_ekf = 0) have no filter to smooth");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->sm_done = false;
    b->mem.release(&b->d_sm_jobs);
    b->mem.release(&b->d_sm_info);
    for (int s = 0; s < b->S; ++s) {
        int rc = ekf_log_set(b->lane[s].ekf, on ? b->cfg.n_scans : 0);
        if (rc) {
            for (int q = 0; q < s; ++q) (void)ekf_log_set(b->lane[q].ekf, 0);
            return rc;
        }
    }
    if (!on) return PTL_OK;
    if (b->mem.alloc(&b->d_sm_jobs, (size_t)b->S) != hipSuccess || b->mem.alloc(&b->d_sm_info, (size_t)b->S * 2) != hipSuccess) {
        for (int q = 0; q < b->S; ++q) (void)ekf_log_set(b->lane[q].ekf, 0);
        return set_err(PTL_ERR_HIP, "smoother job allocation failed");
    }
    std::vector<EkfSmoothJob> jobs((size_t)b->S);
    for (int s = 0; s < b->S; ++s) {
        jobs[(size_t)s] = b->lane[s].ekf->job;
        jobs[(size_t)s].info = b->d_sm_info + 2 * s;  // every status word in one copy
    }
    b->h_sm_info.assign((size_t)b->S * 2, 0);
    HIPCHK(hipMemcpy(b->d_sm_jobs, jobs.data(), jobs.size() * sizeof(EkfSmoothJob), hipMemcpyHostToDevice));
    return PTL_OK;
}
extern "C" int ptl_batch_smooth(ptl_batch* b) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    if (!b->d_sm_jobs) return set_err(PTL_ERR_STATE, "ptl_batch_smooth: the smoother is not enabled (ptl_batch_smoother_enable)");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    b->sm_done = false;
    HIPCHK(hipStreamSynchronize(b->side));
    k_ekf_smooth<<<b->S, EKF_SMOOTH_THREADS, 0, b->stream>>>(b->d_sm_jobs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_sm_info.data(), b->d_sm_info, (size_t)b->S * 2 * sizeof(long long), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int s = 0; s < b->S; ++s) {
        const int rc = smooth_status(b->lane[s].ekf, &b->h_sm_info[2 * (size_t)s], "ptl_batch_smooth", s);
        if (rc) return rc;
    }
    b->sm_done = true;
    return PTL_OK;
}
extern "C" int ptl_batch_smoothed(ptl_batch* b, int32_t seq, double* poses16, double* ts, double* nav19, double* cov324, int64_t* n_rows) {
    if (!b || !poses16 || seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    if (!b->sm_done) return set_err(PTL_ERR_STATE, "ptl_batch_smoothed: no backward pass since the last run (ptl_batch_smooth)");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    const int64_t n = b->h_sm_info[2 * (size_t)seq + 1];
    int rc = smooth_copy_out(b->lane[seq].ekf, n, poses16, ts, nav19, cov324);
    if (rc) return rc;
    if (n_rows) *n_rows = n;
    return PTL_OK;
}
extern "C" int ptl_batch_smoother_log(ptl_batch* b, int32_t seq, double* entries, int64_t max_entries, int64_t* n_entries, int32_t* overflow) {
    if (!b || seq < 0 || seq >= b->S || max_entries < 0) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    return lane_smoother_log(b->lane[seq], b->cfg, "ptl_batch_smoother_log", entries, max_entries, n_entries, overflow);
}
// IMU deskew for every sequence of the batch, either driver, resident or sweep ring
extern "C" int ptl_batch_imu_deskew_enable(ptl_batch* b, int32_t on, int64_t knot_capacity) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    int rc = dk_enable_check(b->cfg, b->lane, b->S, on, knot_capacity, "ptl_batch_imu_deskew_enable");
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->dk_on = false;
    b->ev_filter_valid = false;
    if (on && !b->ev_filter) HIPCHK(b->ev_filter.create());
    for (int s = 0; s < b->S; ++s) {  // every sequence off first: a failure leaves none half on
        rc = lane_dk_set(b->lane[s], b->cfg.n_scans, 0);
        if (rc) return rc;
    }
    for (int s = 0; on && s < b->S && rc == PTL_OK; ++s) rc = lane_dk_set(b->lane[s], b->cfg.n_scans, knot_capacity);
    HIPCHK(hipStreamSynchronize(b->stream));
    b->dk_on = on && rc == PTL_OK;
    return rc;
}
extern "C" int ptl_batch_upload_sweep_times(ptl_batch* b, int32_t seq, const double* t0t1) {
    if (!b || !t0t1 || seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    if (!b->dk_on) return set_err(PTL_ERR_STATE, "ptl_batch_upload_sweep_times: IMU deskew is not enabled");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    return lane_upload_sweep_times(b->lane[seq], b->cfg.n_scans, t0t1, "ptl_batch_upload_sweep_times");
}
extern "C" int ptl_batch_deskew_modes(ptl_batch* b, int32_t seq, int32_t* modes, int64_t max_n, int64_t* n) {
    if (!b || !modes || max_n < 0 || seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    return lane_deskew_modes(b->lane[seq], b->cfg, b->dk_on, b->n_out, modes, max_n, n);
}
extern "C" int ptl_batch_knots(ptl_batch* b, int32_t seq, double* knots, int64_t max_knots, int64_t* n_knots, int32_t* overflow) {
    if (!b || max_knots < 0 || seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    return lane_knots(b->lane[seq], b->cfg, "ptl_batch_knots", knots, max_knots, n_knots, overflow);
}
extern "C" int ptl_batch_copy_traj(ptl_batch* b, int32_t s, void* dst_device, int64_t max_rows, int64_t* rows) {
    if (!b || !dst_device || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    return lane_copy_traj(b->lane[s], b->cfg, b->n_out, b->stream, dst_device, max_rows, rows);
}
extern "C" int ptl_batch_icp(ptl_batch* b, int32_t s, ptl_icp** icp) {
    if (!b || !icp || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    *icp = b->lane[s].icp;
    return PTL_OK;
}
extern "C" int ptl_batch_seq_clocks(ptl_batch* b, int32_t s, int64_t out[8]) {
    if (!b || !out || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->stream));
    long long h[8];
    HIPCHK(hipMemcpy(h, (char*)b->lane[s].icp->c.st + offsetof(DevState, seq_clk), sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out[i] = h[i];
    return PTL_OK;
}
// executed-work counters of sequence s (DevState::exec_cnt), cumulative since the cold start
extern "C" int ptl_batch_exec_counters(ptl_batch* b, int32_t s, uint64_t out[16]) {
    if (!b || !out || s < 0 || s >= b->S) return set_err(PTL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    memset(out, 0, 16 * sizeof(uint64_t));
    HIPCHK(hipMemcpy(out, (char*)b->lane[s].icp->c.st + offsetof(DevState, exec_cnt), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + 8, (char*)b->lane[s].icp->c.st + offsetof(DevState, empty_cnt), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));  // [8] empty_cnt, [9] full_cnt
    return PTL_OK;
}
extern "C" int ptl_batch_gn_phases(ptl_batch* b, int64_t out[8]) {
    if (!b || !out) return set_err(PTL_ERR_ARG, "null argument");
    return ptl_icp_gn_phases(b->lane[0].icp, out);
}
extern "C" int ptl_batch_profile(ptl_batch* b, int enable, double* gn_ms_total, int64_t* gn_launches, int reset) {
    if (!b) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->prof.report(enable, gn_ms_total, gn_launches, reset);
    return PTL_OK;
}

// ================================================================================================ multi-GPU: the trajectory gather (RCCL)
// The path shards across sequences only; its one collective is the all-gather of every rank's (S, T, 8) NC-GT rows
// [t, x, y, z, qx, qy, qz, qw] after the run (ptl_gather_trajectories) - ncclAllGather straight from librccl, over
// xGMI on the node.  The library does NO bootstrap: rank 0 makes the 128-byte ncclUniqueId (ptl_comm_unique_id), the caller carries the
// bytes to the other ranks however it likes (environment, a file, a gloo / MPI / TCP broadcast), every rank calls ptl_comm_create.
// librccl is opened on first use (dlopen): a process that never gathers needs no RCCL, and a process that has torch loaded gets the
// librccl that is already mapped.
#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
extern char g_rccl_why[320];
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    char why[256] = "";
};
RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    // RCCL has to sit on the SAME HIP runtime as this library: a process may hold two ROCm stacks (torch bundles its own libamdhip64 /
    // librccl with the same sonames; whichever HIP runtime was mapped first serves everybody).  So the first choice is the librccl that
    // lives beside the HIP runtime this library is actually bound to; a bare soname comes last (it would return whatever is already mapped).
    const char* override_path = getenv("PTL_RCCL_PATH");
    char beside[2][600] = {"", ""};
    {
        Dl_info info;
        if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
            const char* slash = strrchr(info.dli_fname, '/');
            if (slash) {
                const int dir = (int)(slash - info.dli_fname);
                snprintf(beside[0], sizeof beside[0], "%.*s/librccl.so.1", dir, info.dli_fname);
                snprintf(beside[1], sizeof beside[1], "%.*s/librccl.so", dir, info.dli_fname);
            }
        }
    }
    const char* names[] = {override_path, beside[0], beside[1], "librccl.so.1", "librccl.so"};
    for (const char* n : names) {
        if (!n || !*n) continue;
        if (override_path && *override_path && n != override_path) break;  // PTL_RCCL_PATH is exclusive: that library or none
        api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
        snprintf(api.why, sizeof api.why, "%s", dlerror());
    }
    if (!api.lib) { snprintf(g_rccl_why, sizeof g_rccl_why, "librccl could not be opened (%s); PTL_RCCL_PATH overrides the search", api.why); return nullptr; }
#define RSYM(f) api.f = (decltype(api.f))dlsym(api.lib, "nccl" #f)
    RSYM(GetUniqueId); RSYM(CommInitRank); RSYM(AllGather); RSYM(CommDestroy); RSYM(CommAbort); RSYM(GetErrorString);
#undef RSYM
    if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy || !api.GetErrorString) {
        snprintf(g_rccl_why, sizeof g_rccl_why, "the librccl that was opened lacks a needed symbol");
        dlclose(api.lib);
        api.lib = nullptr;
        return nullptr;
    }
    return &api;
}
char g_rccl_why[320] = "";
const char* rccl_why() { return g_rccl_why; }
}  // namespace
#define RCCLCHK(api, x)                                                                                          \
    do {                                                                                                         \
        ncclResult_t r_ = (x);                                                                                   \
        if (r_ != ncclSuccess) return set_err(PTL_ERR_HIP, "%s: %s (%s:%d)", #x, (api)->GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

struct ptl_comm {
    ncclComm_t comm = nullptr;
    int world = 0, rank = 0, device_id = 0;
    Stream stream;
    // staging of the gather, kept between calls (grow-only): send [per_rank], recv [world x per_rank] on the device, the host mirror of recv
    double *d_send = nullptr, *d_recv = nullptr;
    size_t cap_send = 0, cap_recv = 0;
    std::vector<double> host;
    bool broken = false;  // a local failure aborted the communicator (ncclCommAbort): the peers' collective fails instead of hanging, every later call is refused
    DevOwner mem;
};
extern "C" int ptl_comm_unique_id(uint8_t id[PTL_COMM_ID_BYTES]) {
    if (!id) return set_err(PTL_ERR_ARG, "null argument");
    static_assert(PTL_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the ABI's id size is RCCL's");
    RcclApi* api = rccl_api();
    if (!api) return set_err(PTL_ERR_STATE, "%s", rccl_why());
    ncclUniqueId u;
    RCCLCHK(api, api->GetUniqueId(&u));
    memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return PTL_OK;
}
extern "C" int ptl_comm_create(const uint8_t id[PTL_COMM_ID_BYTES], int32_t world, int32_t rank, int32_t device_id, ptl_comm** out) {
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return set_err(PTL_ERR_ARG, "bad argument");
    if (ptl_device_count() <= device_id || device_id < 0) return set_err(PTL_ERR_HIP, "no HIP device %d", device_id);
    RcclApi* api = rccl_api();
    if (!api) return set_err(PTL_ERR_STATE, "%s", rccl_why());
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_comm> owner(new ptl_comm());
    ptl_comm* c = owner.get();
    c->world = world; c->rank = rank; c->device_id = device_id;
    if (c->stream.create() != hipSuccess) return set_err(PTL_ERR_HIP, "stream creation failed");
    ncclUniqueId u;
    memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = api->CommInitRank(&c->comm, world, u, rank);  // (collective: returns when every rank has called it)
    if (r != ncclSuccess) return set_err(PTL_ERR_HIP, "ncclCommInitRank(world %d, rank %d, device %d): %s", world, rank, device_id, api->GetErrorString(r));
    *out = owner.release();
    return PTL_OK;
}
extern "C" int ptl_comm_destroy(ptl_comm* c) {
    if (!c) return PTL_OK;
    RcclApi* api = rccl_api();
    (void)hipSetDevice(c->device_id);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (api && c->comm && !c->broken) (void)api->CommDestroy(c->comm);
    delete c;
    return PTL_OK;
}
// every rank: S sequences x T rows x 8 doubles on the DEVICE (padded with anything) and S row counts on the host; same S and T on every rank.
// rows_out [world][S][T][8] and counts_out [world][S] on the host, filled on every rank.  One ncclAllGather: the counts ride behind the rows
// in the same send buffer (as doubles - exact for any count below 2^53).
// A failure on THIS rank between communicator creation and the collective must not leave the peers waiting in ncclAllGather for ever
// (they sit in hipStreamSynchronize without a time-out): the communicator is aborted, which fails their collective.
static int comm_fail(ptl_comm* c, RcclApi* api, int rc) {
    if (api && api->CommAbort && c->comm && !c->broken) (void)api->CommAbort(c->comm);
    c->broken = true;
    return rc;
}
extern "C" int ptl_gather_trajectories(ptl_comm* c, const double* d_rows, int64_t S, int64_t T, const int64_t* counts,
                                       double* rows_out, int64_t* counts_out) {
    // arguments first: nothing is allocated, staged or sent for a call that is wrong in itself (the peers of a rank that returns HERE
    // are the caller's to tell - every rank validates the same S and T, and a bad count aborts the communicator below)
    if (!c || !d_rows || !counts || !rows_out || !counts_out || S < 1 || T < 1) return set_err(PTL_ERR_ARG, "bad argument");
    if (c->broken) return set_err(PTL_ERR_STATE, "the communicator was aborted after an earlier failure on this rank: create a new one");
    RcclApi* api = rccl_api();
    if (!api) return set_err(PTL_ERR_STATE, "%s", rccl_why());
    for (int64_t s = 0; s < S; ++s)
        if (counts[s] < 0 || counts[s] > T) return comm_fail(c, api, set_err(PTL_ERR_ARG, "count of sequence %lld outside [0, T]", (long long)s));
    HIPCHK(hipSetDevice(c->device_id));
    const size_t per_rank = (size_t)S * (size_t)T * 8 + (size_t)S, all = per_rank * (size_t)c->world;
    if (c->cap_send < per_rank) {
        c->mem.release(&c->d_send);
        c->cap_send = 0;
        if (c->mem.alloc(&c->d_send, per_rank) != hipSuccess) return comm_fail(c, api, set_err(PTL_ERR_HIP, "gather buffer allocation failed (%.1f MB)", per_rank * 8 / 1e6));
        c->cap_send = per_rank;
    }
    if (c->cap_recv < all) {
        c->mem.release(&c->d_recv);
        c->cap_recv = 0;
        if (c->mem.alloc(&c->d_recv, all) != hipSuccess) return comm_fail(c, api, set_err(PTL_ERR_HIP, "gather buffer allocation failed (%.1f MB)", all * 8 / 1e6));
        c->cap_recv = all;
    }
    if (c->host.size() < all + (size_t)S) c->host.resize(all + (size_t)S);
    double* cnt = c->host.data() + all;  // (the counts as doubles, staged behind the mirror: exact below 2^53)
    for (int64_t s = 0; s < S; ++s) cnt[s] = (double)counts[s];
    if (hipMemcpyAsync(c->d_send, d_rows, (size_t)S * T * 64, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->d_send + (size_t)S * T * 8, cnt, (size_t)S * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return comm_fail(c, api, set_err(PTL_ERR_HIP, "gather staging failed: %s", hipGetErrorString(hipGetLastError())));
    ncclResult_t r = api->AllGather(c->d_send, c->d_recv, per_rank, ncclDouble, c->comm, c->stream);
    if (r != ncclSuccess) return comm_fail(c, api, set_err(PTL_ERR_HIP, "ncclAllGather: %s", api->GetErrorString(r)));
    if (hipMemcpyAsync(c->host.data(), c->d_recv, all * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return comm_fail(c, api, set_err(PTL_ERR_HIP, "gather read-back failed: %s", hipGetErrorString(hipGetLastError())));
    for (int rk = 0; rk < c->world; ++rk) {
        const double* p = c->host.data() + per_rank * (size_t)rk;
        memcpy(rows_out + (size_t)rk * S * T * 8, p, (size_t)S * T * 64);
        for (int64_t s = 0; s < S; ++s) counts_out[(size_t)rk * S + s] = (int64_t)p[(size_t)S * T * 8 + s];
    }
    return PTL_OK;
}
// ICP-only batches have no filter and so no NC-GT rows of its making: the registration's own poses (KissICP.poses, reference kiss.py:130,
// what `ekf-bench ouster` writes when no filter corrects them) as rows [scan index, x, y, z, qx, qy, qz, qw]
__global__ void k_kiss_rows(const double* traj16, int n, double* rows8) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const double* T = traj16 + 16 * (size_t)k;
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    double q[4];
    R_to_quat(R, q);
    double* o = rows8 + 8 * (size_t)k;
    o[0] = (double)k; o[1] = T[3]; o[2] = T[7]; o[3] = T[11];
    o[4] = q[0]; o[5] = q[1]; o[6] = q[2]; o[7] = q[3];
}
// ... of a batch: the rows its filter kernel wrote for every sequence (ptl_batch_copy_traj's source), T = the batch's n_scans
extern "C" int ptl_batch_gather_trajectories(ptl_batch* b, ptl_comm* c, double* rows_out, int64_t* counts_out) {
    if (!b || !c || !rows_out || !counts_out) return set_err(PTL_ERR_ARG, "null argument");
    if (c->device_id != b->cfg.icp.device_id) return set_err(PTL_ERR_ARG, "communicator on device %d, batch on device %d", c->device_id, b->cfg.icp.device_id);
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->side));
    HIPCHK(hipStreamSynchronize(b->stream));
    const int64_t S = b->S, T = b->cfg.n_scans;
    double* d_rows = nullptr;
    DevOwner tmp;
    HIPCHK(tmp.alloc(&d_rows, (size_t)S * T * 8));
    std::vector<int64_t> counts((size_t)S, b->n_out < T ? b->n_out : T);
    hipError_t e = hipMemsetAsync(d_rows, 0, (size_t)S * T * 64, b->stream);
    for (int64_t s = 0; s < S && e == hipSuccess; ++s) {
        const int64_t n = counts[(size_t)s];
        if (n <= 0) continue;
        if (b->cfg.with_ekf) e = hipMemcpyAsync(d_rows + (size_t)s * T * 8, b->lane[s].d_rows, (size_t)n * 64, hipMemcpyDeviceToDevice, b->stream);
        else { k_kiss_rows<<<(int)((n + 63) / 64), 64, 0, b->stream>>>(b->lane[s].icp->c.traj, (int)n, d_rows + (size_t)s * T * 8); e = hipGetLastError(); }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return set_err(PTL_ERR_HIP, "row staging failed: %s", hipGetErrorString(e));
    return ptl_gather_trajectories(c, d_rows, S, T, counts.data(), rows_out, counts_out);
}

// ================================================================================================ posed scans into the map
// The world map of a run, built on the device: a trajectory resident as knots, sweeps taken from where they already are (the caller's
// host buffer once, or a runner's resident slots), every pass on the MAP handle's stream and in the map handle's buffers (fly_kernels.h).
struct ptl_traj {
    int device_id = 0;  // (first member: the one-device rule is tested by changing it)
    int n = 0;
    double *d_kt = nullptr, *d_kp = nullptr;
    double before = 0, after = 0;
    DevOwner mem;
};
extern "C" int ptl_traj_create(int device_id, const double* knot_ts, const double* knot_poses16, int64_t n_knots, double bound_before,
                               double bound_after, ptl_traj** out) {
    if (!knot_ts || !knot_poses16 || !out) return set_err(PTL_ERR_ARG, "null argument");
    if (n_knots < 2) return set_err(PTL_ERR_ARG, "a trajectory needs >= 2 knots (%lld given: knot %lld is missing)", (long long)n_knots, (long long)(n_knots < 0 ? 0 : n_knots));
    if (n_knots > (1 << 30)) return set_err(PTL_ERR_ARG, "too many knots");
    for (int64_t i = 1; i < n_knots; ++i)
        if (!(knot_ts[i] > knot_ts[i - 1])) return set_err(PTL_ERR_ARG, "knot timestamps must increase strictly (knot %lld)", (long long)i);
    if (device_id < 0 || ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_traj> t(new ptl_traj());
    t->device_id = device_id; t->n = (int)n_knots; t->before = bound_before; t->after = bound_after;
    t->mem.add(&t->d_kt, (size_t)n_knots); t->mem.add(&t->d_kp, (size_t)n_knots * 16);
    hipError_t e = t->mem.err;
    if (e == hipSuccess) e = hipMemcpy(t->d_kt, knot_ts, (size_t)n_knots * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_kp, knot_poses16, (size_t)n_knots * 128, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipGetLastError(); return set_err(PTL_ERR_HIP, "ptl_traj_create: %s", hipGetErrorString(e)); }
    *out = t.release();
    return PTL_OK;
}
extern "C" int ptl_traj_destroy(ptl_traj* t) { return t ? handle_destroy(t, t->device_id) : PTL_OK; }
// what every posed-scan entry point checks (before any HIP call) and sets up: one device, the map handle's geometry, its FlyWs, and its
// stream ordered behind a map update that may still run
static int fly_prepare(ptl_icp* h, const ptl_traj* t, const ptl_lut* lut, int64_t H, int64_t W, const char* who) {
    if (t->device_id != h->cfg.device_id) return set_err(PTL_ERR_ARG, "%s: trajectory on device %d, map on device %d", who, t->device_id, h->cfg.device_id);
    if (lut && lut->device_id != h->cfg.device_id) return set_err(PTL_ERR_ARG, "%s: LUT on device %d, map on device %d", who, lut->device_id, h->cfg.device_id);
    if (H < 1 || W < 1) return set_err(PTL_ERR_ARG, "%s: empty scan", who);
    if (W != h->c.W) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld columns, the map handle's scan_cols is %d", who, (long long)W, h->c.W);
    if (H * W > h->n_max) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld pixels, the map handle's max_points_per_scan is %lld", who, (long long)(H * W), (long long)h->n_max);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    if (!h->d_fly) {
        HIPCHK(h->mem.alloc(&h->d_fly, 1));
        HIPCHK(hipMemsetAsync(h->d_fly, 0, sizeof(FlyWs), h->stream));
    }
    return icp_join_map(h);
}
// one posed scan enqueued on the map handle's stream; raw (device): the sweep; d_col_ts (device, W) or the sweep's (t0, t1)
static int fly_enqueue(ptl_icp* h, const ptl_traj* t, const void* raw, bool is_range, const ptl_lut* lut, int H, int W, const double* d_col_ts,
                       double t0, double t1) {
    const Ctx& c = h->c;
    hipStream_t s = h->stream;
    const int n = H * W, nb = (n + 255) / 256;
    FlyWs* ws = h->d_fly;
    double* pts = (double*)h->d_in;
    k_fly_coltab<<<1, 256, 0, s>>>(t->d_kt, t->d_kp, t->n, t->before, t->after, d_col_ts, t0, t1, W, c.coltab, ws);
    if (is_range) {
        k_fly_count<true><<<nb, 256, 0, s>>>(raw, n, c.bcnt1, ws);
        k_fly_emit<true><<<nb, 256, 0, s>>>(raw, lut->dir, lut->off, n, W, c.coltab, c.bcnt1, pts, ws);
    } else {
        k_fly_count<false><<<nb, 256, 0, s>>>(raw, n, c.bcnt1, ws);
        k_fly_emit<false><<<nb, 256, 0, s>>>(raw, nullptr, nullptr, n, W, c.coltab, c.bcnt1, pts, ws);
    }
    k_map_insert_a<<<nb, 256, 0, s>>>(c, pts, &ws->n, 0, 0);  // as ptl_icp_map_add, with the device count
    k_map_insert_b<<<nb, 256, 0, s>>>(c, &ws->n, 0);
    k_map_insert_c<<<nb, 256, 0, s>>>(c, &ws->n, 0);
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// per-call form: the raw sweep and its column times go up once (staged in the handle's deskew buffers, idle in a map container), the
// count and the flag come back (8 bytes, beside the error word ptl_icp_map_add reads too)
static int fly_add_percall(ptl_icp* h, ptl_traj* t, ptl_lut* lut, const void* raw_host, size_t raw_bytes, bool is_range, int64_t H, int64_t W,
                           const double* col_ts, int64_t* n_valid, int32_t* skipped, const char* who) {
    int rc = fly_prepare(h, t, lut, H, W, who);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->c.pts, raw_host, raw_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_t01, col_ts, (size_t)W * 8, hipMemcpyHostToDevice, h->stream));
    rc = fly_enqueue(h, t, h->c.pts, is_range, lut, (int)H, (int)W, h->d_t01, 0.0, 0.0);
    if (rc) return rc;
    int nf[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(nf, h->d_fly, sizeof nf, hipMemcpyDeviceToHost, h->stream));
    rc = icp_check_flags(h);  // (waits for the stream)
    if (rc) return rc;
    if (n_valid) *n_valid = nf[0];
    if (skipped) *skipped = nf[1] ? 1 : 0;
    return PTL_OK;
}
extern "C" int ptl_icp_map_add_posed_range(ptl_icp* map, ptl_traj* t, ptl_lut* lut, const uint32_t* range_mm, const double* col_ts,
                                           int64_t* n_valid, int32_t* skipped) {
    if (!map || !t || !lut || !range_mm || !col_ts) return set_err(PTL_ERR_ARG, "null argument");
    return fly_add_percall(map, t, lut, range_mm, (size_t)lut->H * lut->W * 4, true, lut->H, lut->W, col_ts, n_valid, skipped, "ptl_icp_map_add_posed_range");
}
extern "C" int ptl_icp_map_add_posed_xyz(ptl_icp* map, ptl_traj* t, const float* xyz, int32_t H, int32_t W, const double* col_ts,
                                         int64_t* n_valid, int32_t* skipped) {
    if (!map || !t || !xyz || !col_ts) return set_err(PTL_ERR_ARG, "null argument");
    return fly_add_percall(map, t, nullptr, xyz, (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * 12, false, H, W, col_ts, n_valid, skipped, "ptl_icp_map_add_posed_xyz");
}
// resident form: sweeps [first, last] of a lane, `slot` bytes apart; nothing but the two totals crosses the bus, once, at the end.
// The caller has checked the runner's side and waited for its streams; the lane is only read.
static int fly_build(ptl_icp* map, ptl_traj* t, const SeqLane& l, size_t slot, const unsigned char* is_range_k, bool all_range, const ptl_lut* lut,
                     int64_t pps, const double* t0t1, int64_t first, int64_t last, int64_t* n_valid, int64_t* n_skipped, const char* who) {
    if (map == l.icp) return set_err(PTL_ERR_ARG, "%s: the map handle is the runner's own registration handle", who);
    const int64_t W = map->c.W;
    if (pps % W) return set_err(PTL_ERR_CAPACITY, "%s: %lld points per sweep are no multiple of the map handle's scan_cols = %lld", who, (long long)pps, (long long)W);
    if (l.icp->c.W != W) return set_err(PTL_ERR_CAPACITY, "%s: the runner's scan_cols is %d, the map handle's %lld", who, l.icp->c.W, (long long)W);
    int rc = fly_prepare(map, t, lut, pps / W, W, who);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(&map->d_fly->n_valid, 0, 2 * sizeof(long long), map->stream));
    for (int64_t k = first; k <= last; ++k) {
        const bool rg = all_range || (is_range_k && is_range_k[(size_t)k]);
        rc = fly_enqueue(map, t, (const char*)l.d_scans + (size_t)k * slot, rg, lut, (int)(pps / W), (int)W, nullptr, t0t1[2 * k], t0t1[2 * k + 1]);
        if (rc) return rc;
    }
    long long tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(tot, &map->d_fly->n_valid, sizeof tot, hipMemcpyDeviceToHost, map->stream));
    rc = icp_check_flags(map);
    if (rc) return rc;
    if (n_valid) *n_valid = tot[0];
    if (n_skipped) *n_skipped = tot[1];
    return PTL_OK;
}
extern "C" int ptl_seq_map_build(ptl_seq* s, ptl_icp* map, ptl_traj* t, const double* t0t1, int64_t first, int64_t last, int64_t* n_valid,
                                 int64_t* n_skipped) {
    if (!s || !map || !t || !t0t1) return set_err(PTL_ERR_ARG, "null argument");
    if (first < 0 || last < first || last >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_seq_map_build: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)s->cfg.n_scans);
    if (s->cfg.icp.device_id != map->cfg.device_id) return set_err(PTL_ERR_ARG, "ptl_seq_map_build: runner on device %d, map on device %d", s->cfg.icp.device_id, map->cfg.device_id);
    bool any_range = false;
    for (int64_t k = first; k <= last; ++k) any_range = any_range || s->is_range[(size_t)k];
    if (any_range && !s->lut) return set_err(PTL_ERR_STATE, "ptl_seq_map_build: the sweeps are range images but no LUT was set (ptl_seq_set_lut)");
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(s->stream));  // the runner's own work first; its sweeps are then only read
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    return fly_build(map, t, s->lane, (size_t)s->cfg.points_per_scan * 12, s->is_range.data(), false, any_range ? s->lut : nullptr, s->cfg.points_per_scan,
                     t0t1, first, last, n_valid, n_skipped, "ptl_seq_map_build");
}
extern "C" int ptl_batch_map_build(ptl_batch* b, int32_t seq, ptl_icp* map, ptl_traj* t, const double* t0t1, int64_t first, int64_t last,
                                   int64_t* n_valid, int64_t* n_skipped) {
    if (!b || !map || !t || !t0t1) return set_err(PTL_ERR_ARG, "null argument");
    if (seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "ptl_batch_map_build: sequence %d of %d", seq, b->S);
    if (first < 0 || last < first || last >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_batch_map_build: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)b->cfg.n_scans);
    if (b->cfg.icp.device_id != map->cfg.device_id) return set_err(PTL_ERR_ARG, "ptl_batch_map_build: batch on device %d, map on device %d", b->cfg.icp.device_id, map->cfg.device_id);
    if (b->ring < b->cfg.n_scans) return set_err(PTL_ERR_STATE, "ptl_batch_map_build: the batch keeps a ring of %lld sweep slots (resident_scans): earlier sweeps are gone", (long long)b->ring);
    if (b->cfg.range_input && !b->lut) return set_err(PTL_ERR_STATE, "ptl_batch_map_build: a range-input batch needs its LUT (ptl_batch_set_lut)");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    HIPCHK(hipStreamSynchronize(b->stream));  // the batch's own work first; its sweeps are then only read
    HIPCHK(hipStreamSynchronize(b->side));
    const size_t slot = (size_t)b->cfg.points_per_scan * (b->cfg.range_input ? 4 : 12);
    return fly_build(map, t, b->lane[seq], slot, nullptr, b->is_range != 0, b->is_range ? b->lut : nullptr, b->cfg.points_per_scan, t0t1, first, last,
                     n_valid, n_skipped, "ptl_batch_map_build");
}

// ================================================================================================ map score
// The definition is in include/ptudes_mi.h, the kernels in score_kernels.h.  Everything is checked on the host before the first HIP call; the
// work buffers (chunk counts and offsets, the per-point values) are sized from the map's point count and live for the call.
static void map_score_defaults(ptl_map_score_cfg* cfg, double voxel_size) {
    PTL_CFG_INIT(cfg);
    cfg->radius = voxel_size;
    cfg->min_neighbours = 5;
    cfg->sigma_floor = voxel_size / 100.0;
}
extern "C" int ptl_map_score_default_cfg(ptl_map_score_cfg* cfg, double voxel_size) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_map_score_cfg, cfg);
    if (!(voxel_size > 0.0)) return set_err(PTL_ERR_ARG, "voxel_size must be positive (got %g)", voxel_size);
    map_score_defaults(cfg, voxel_size);
    return PTL_OK;
}
extern "C" int ptl_icp_map_score(ptl_icp* map, const ptl_map_score_cfg* cfg, ptl_map_score_result* out, double* xyz_out, int32_t* n_out,
                                 double* plane_var_out, double* entropy_out, int64_t max_points, int64_t* n_written) {
    if (!map || !out) return set_err(PTL_ERR_ARG, "null argument");
    ptl_map_score_cfg use;
    if (cfg) { ABI_CHECK(ptl_map_score_cfg, cfg); use = *cfg; } else map_score_defaults(&use, map->cfg.voxel_size);
    const int given = (xyz_out != nullptr) + (n_out != nullptr) + (plane_var_out != nullptr) + (entropy_out != nullptr);
    if (given != 0 && given != 4) return set_err(PTL_ERR_ARG, "the four per-point arrays (xyz, n, plane_var, entropy) are given together or not at all");
    if (given && max_points < 0) return set_err(PTL_ERR_ARG, "max_points must not be negative");
    const double vs = map->cfg.voxel_size;
    if (!(use.radius > 0.0) || !(use.radius <= vs))
        return set_err(PTL_ERR_ARG, "radius = %g: the 27-voxel search needs 0 < radius <= the map's voxel size = %g", use.radius, vs);
    if (use.min_neighbours < 1) return set_err(PTL_ERR_ARG, "min_neighbours = %d: must be >= 1 (it counts the point itself)", use.min_neighbours);
    if (!(use.sigma_floor > 0.0) || !(use.sigma_floor < 1.0e150)) return set_err(PTL_ERR_ARG, "sigma_floor = %g: must be positive and finite", use.sigma_floor);
    const int P = map->cfg.max_points_per_voxel;
    if (P < 1) return set_err(PTL_ERR_ARG, "max_points_per_voxel = %d", P);
    const size_t stage_bytes = (size_t)27 * (size_t)P * 24;
    if (stage_bytes > SCORE_LDS_LIMIT)
        return set_err(PTL_ERR_CAPACITY, "max_points_per_voxel = %d needs %zu bytes of staging (27 voxels x P points x 24 bytes); the limit is %d bytes: P <= %d",
                       P, stage_bytes, SCORE_LDS_LIMIT, SCORE_LDS_LIMIT / (27 * 24));
    HIPCHK(hipSetDevice(map->cfg.device_id));
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, map->stream));
    HIPCHK(hipStreamSynchronize(map->stream));
    const int64_t n = st.map_points;
    if (n < 0 || n > (int64_t)0x7fffffff) return set_err(PTL_ERR_STATE, "the map reports %lld points", (long long)n);
    if (given && max_points < n)
        return set_err(PTL_ERR_CAPACITY, "the map holds %lld points, max_points = %lld", (long long)n, (long long)max_points);
    memset(out, 0, sizeof *out);
    out->radius = use.radius; out->min_neighbours = use.min_neighbours; out->sigma_floor = use.sigma_floor;
    if (n_written) *n_written = 0;
    if (n == 0) return PTL_OK;
    const Ctx& c = map->c;
    const int n_chunks = (c.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr, *d_nb = nullptr;
    double *d_pv = nullptr, *d_ent = nullptr, *d_xyz = nullptr, *d_sum = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1);
    tmp.add(&d_nb, (size_t)n); tmp.add(&d_pv, (size_t)n); tmp.add(&d_ent, (size_t)n);
    if (given) tmp.add(&d_xyz, (size_t)n * 3);
    int* d_bad = nullptr;
    tmp.add(&d_sum, 4); tmp.add(&d_bad, 1);
    HIPCHK(tmp.err);
    Event e0, e1;
    HIPCHK(e0.create(hipEventDefault)); HIPCHK(e1.create(hipEventDefault));
    hipStream_t s = map->stream;
    ScoreArgs a = {};
    a.radius = use.radius; a.r2 = use.radius * use.radius; a.floor2 = use.sigma_floor * use.sigma_floor; a.min_nb = use.min_neighbours;
    a.n_chunks = n_chunks; a.n_alloc = (int)n; a.stage_pts = 27 * P;
    a.chunk_off = d_off; a.xyz = d_xyz; a.nb = d_nb; a.pv = d_pv; a.ent = d_ent; a.bad = d_bad;
    HIPCHK(hipEventRecord(e0, s));  // (all of the call's device work lies between the two events; every per-point slot is written by k_score_points)
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    k_score_count<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    k_score_points<<<n_chunks < 8192 ? n_chunks : 8192, 64, stage_bytes, s>>>(c, a);
    k_score_reduce<<<1, 1024, 0, s>>>(d_nb, d_pv, d_ent, (int)n, use.min_neighbours, d_sum);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipGetLastError());
    int total = 0, bad = 0;
    double sums[4];
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sums, d_sum, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return set_err(PTL_ERR_STATE, "the map table does not lead back to %d of the map's voxels: nothing was scored", bad);
    if (total != (int)n) return set_err(PTL_ERR_STATE, "the block directory holds %d points, the map state %lld", total, (long long)n);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    out->n_points = n;
    out->n_scored = (int64_t)sums[0];
    out->n_sparse = n - out->n_scored;
    out->mean_plane_var = out->n_scored ? sums[1] / sums[0] : 0.0;
    out->mean_entropy = out->n_scored ? sums[2] / sums[0] : 0.0;
    out->mean_neighbours = sums[3] / (double)n;
    out->device_ms = ms;
    if (given) {
        HIPCHK(hipMemcpy(xyz_out, d_xyz, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(n_out, d_nb, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(plane_var_out, d_pv, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(entropy_out, d_ent, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (n_written) *n_written = n;
    }
    return PTL_OK;
}

// ================================================================================================ map distance
// The definition is in include/ptudes_mi.h, the kernels in compare_kernels.h.  Everything is checked on the host before the first HIP call; the
// work buffers (one staged chunk of queries or the chunk prefix of the source map, the per-query values, the summaries) live for the call.
static void map_cmp_defaults(ptl_map_cmp_cfg* cfg, double voxel_size) {
    PTL_CFG_INIT(cfg);
    cfg->max_dist = voxel_size;
    cfg->n_thresholds = 1;
    cfg->thresholds[0] = voxel_size;
}
extern "C" int64_t ptl_map_cmp_sizeof_cfg(void) { return (int64_t)sizeof(ptl_map_cmp_cfg); }
extern "C" int ptl_map_cmp_default_cfg(ptl_map_cmp_cfg* cfg, double voxel_size) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_map_cmp_cfg, cfg);
    if (!(voxel_size > 0.0) || !(voxel_size < 1.0e150)) return set_err(PTL_ERR_ARG, "voxel_size must be positive and finite (got %g)", voxel_size);
    map_cmp_defaults(cfg, voxel_size);
    return PTL_OK;
}
static_assert(PTL_MAP_CMP_MAX_THRESHOLDS == CMP_MAX_THR, "the header's threshold count is the kernels'");
// the configuration as used (cfg nullable: the defaults of ref's voxel size), checked; fills the kernel arguments' parameter half and the result's echo
static int map_cmp_setup(const char* who, ptl_icp* ref, const ptl_map_cmp_cfg* cfg, ptl_map_cmp_result* result, CmpArgs* a) {
    ptl_map_cmp_cfg use;
    if (cfg) { ABI_CHECK(ptl_map_cmp_cfg, cfg); use = *cfg; } else map_cmp_defaults(&use, ref->cfg.voxel_size);
    const double vs = ref->cfg.voxel_size;
    if (!(use.max_dist > 0.0) || !(use.max_dist <= vs))
        return set_err(PTL_ERR_ARG, "%s: max_dist = %g: the 27-voxel search needs 0 < max_dist <= the reference map's voxel size = %g", who, use.max_dist, vs);
    if (use.n_thresholds < 1 || use.n_thresholds > CMP_MAX_THR)
        return set_err(PTL_ERR_ARG, "%s: n_thresholds = %d: must be in [1, %d]", who, use.n_thresholds, CMP_MAX_THR);
    for (int k = 0; k < use.n_thresholds; ++k) {
        const double t = use.thresholds[k];
        if (!(t > 0.0) || !(t <= use.max_dist))
            return set_err(PTL_ERR_ARG, "%s: threshold %d = %g: must be in (0, max_dist = %g]", who, k, t, use.max_dist);
        if (k > 0 && t < use.thresholds[k - 1])
            return set_err(PTL_ERR_ARG, "%s: threshold %d = %g is below threshold %d = %g: ascending order", who, k, t, k - 1, use.thresholds[k - 1]);
    }
    memset(result, 0, sizeof *result);
    memset(a, 0, sizeof *a);
    result->max_dist = a->max_dist = use.max_dist;
    a->max2 = use.max_dist * use.max_dist;
    result->n_thresholds = a->n_thr = use.n_thresholds;
    for (int k = 0; k < use.n_thresholds; ++k) { result->thresholds[k] = use.thresholds[k]; a->thr2[k] = use.thresholds[k] * use.thresholds[k]; }
    return PTL_OK;
}
// one reduced summary (k_cmp_reduce) into the result; the sums in the order the summaries are handed in
static void map_cmp_add(ptl_map_cmp_result* r, const double* sums) {
    r->n_invalid += (int64_t)sums[0];
    r->n_matched += (int64_t)sums[1];
    r->sum_dist += sums[2];
    r->sum_dist2 += sums[3];
    if (sums[4] > r->max_dist2_seen) r->max_dist2_seen = sums[4];
    for (int k = 0; k < r->n_thresholds; ++k) r->n_within[k] += (int64_t)sums[5 + k];
}
extern "C" int ptl_icp_map_distance(ptl_icp* ref, const ptl_map_cmp_cfg* cfg, const double* xyz, int64_t n, ptl_map_cmp_result* result, double* dist2_out) {
    if (!ref || !result) return set_err(PTL_ERR_ARG, "ptl_icp_map_distance: null argument");
    if (n < 0) return set_err(PTL_ERR_ARG, "ptl_icp_map_distance: n = %lld: must not be negative", (long long)n);
    if (n > 0 && !xyz) return set_err(PTL_ERR_ARG, "ptl_icp_map_distance: %lld queries without xyz", (long long)n);
    CmpArgs a;
    { int rc = map_cmp_setup("ptl_icp_map_distance", ref, cfg, result, &a); if (rc) return rc; }
    result->n_query = n;
    if (n == 0) return PTL_OK;
    HIPCHK(hipSetDevice(ref->cfg.device_id));
    HIPCHK(hipStreamSynchronize(ref->map_stream));  // (a map update may still be under way)
    const int64_t n_chunks = (n + CMP_CHUNK - 1) / CMP_CHUNK;
    const int cap = (int)(n < CMP_CHUNK ? n : CMP_CHUNK);
    DevOwner tmp;
    double *d_xyz = nullptr, *d_d2 = nullptr, *d_sum = nullptr;
    int* d_bad = nullptr;
    tmp.add(&d_xyz, (size_t)cap * 3); tmp.add(&d_d2, (size_t)cap); tmp.add(&d_sum, (size_t)n_chunks * CMP_SUMS); tmp.add(&d_bad, 1);
    HIPCHK(tmp.err);
    Event e0, e1;
    HIPCHK(e0.create(hipEventDefault)); HIPCHK(e1.create(hipEventDefault));
    hipStream_t s = ref->stream;
    a.d2 = d_d2; a.bad = d_bad; a.n_alloc = cap;
    HIPCHK(hipEventRecord(e0, s));
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    for (int64_t ch = 0; ch < n_chunks; ++ch) {  // (one staging buffer: the stream's order keeps a chunk's kernels ahead of the next chunk's copy)
        const int64_t off = ch * (int64_t)CMP_CHUNK;
        const int m = (int)(n - off < CMP_CHUNK ? n - off : CMP_CHUNK);
        HIPCHK(hipMemcpyAsync(d_xyz, xyz + 3 * off, (size_t)m * 24, hipMemcpyHostToDevice, s));
        CmpArraySrc src = {d_xyz, m};
        const int wg = (m + 2 * (CMP_THREADS / 64) - 1) / (2 * (CMP_THREADS / 64));
        k_cmp_points<CmpArraySrc><<<wg < CMP_MAX_BLOCKS ? wg : CMP_MAX_BLOCKS, CMP_THREADS, 0, s>>>(src, ref->c, a);
        k_cmp_reduce<<<1, 1024, 0, s>>>(d_d2, m, a, d_sum + ch * CMP_SUMS);
        if (dist2_out) HIPCHK(hipMemcpyAsync(dist2_out + off, d_d2, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipGetLastError());
    int bad = 0;
    std::vector<double> sums((size_t)n_chunks * CMP_SUMS);
    HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sums.data(), d_sum, sums.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return set_err(PTL_ERR_STATE, "ptl_icp_map_distance: the reference map's table led %d probes to a block that does not hold the probed voxel", bad);
    for (int64_t ch = 0; ch < n_chunks; ++ch) map_cmp_add(result, sums.data() + ch * CMP_SUMS);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    result->device_ms = ms;
    return PTL_OK;
}
extern "C" int ptl_icp_map_compare(ptl_icp* ref, ptl_icp* src, const ptl_map_cmp_cfg* cfg, ptl_map_cmp_result* result, double* xyz_out, double* dist2_out,
                                   int64_t max_points, int64_t* n_written) {
    if (!ref || !src || !result) return set_err(PTL_ERR_ARG, "ptl_icp_map_compare: null argument");
    if ((xyz_out != nullptr) != (dist2_out != nullptr)) return set_err(PTL_ERR_ARG, "ptl_icp_map_compare: xyz_out and dist2_out are given together or not at all");
    const bool given = xyz_out != nullptr;
    if (given && max_points < 0) return set_err(PTL_ERR_ARG, "ptl_icp_map_compare: max_points = %lld: must not be negative", (long long)max_points);
    if (ref->cfg.device_id != src->cfg.device_id)
        return set_err(PTL_ERR_ARG, "ptl_icp_map_compare: reference map on device %d, source map on device %d", ref->cfg.device_id, src->cfg.device_id);
    CmpArgs a;
    ptl_map_cmp_result r0;  // (the caller's is written once nothing can be refused for an argument any more)
    { int rc = map_cmp_setup("ptl_icp_map_compare", ref, cfg, &r0, &a); if (rc) return rc; }
    HIPCHK(hipSetDevice(ref->cfg.device_id));
    HIPCHK(hipStreamSynchronize(ref->map_stream));  // (a map update may still be under way, in either handle)
    HIPCHK(hipStreamSynchronize(src->map_stream));
    HIPCHK(hipStreamSynchronize(src->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, src->c.st, sizeof st, hipMemcpyDeviceToHost, ref->stream));
    HIPCHK(hipStreamSynchronize(ref->stream));
    const int64_t n = st.map_points;
    if (n < 0 || n > (int64_t)0x7fffffff) return set_err(PTL_ERR_STATE, "ptl_icp_map_compare: the source map reports %lld points", (long long)n);
    if (given && max_points < n)
        return set_err(PTL_ERR_CAPACITY, "ptl_icp_map_compare: the source map holds %lld points, max_points = %lld", (long long)n, (long long)max_points);
    *result = r0;
    if (n_written) *n_written = 0;
    result->n_query = n;
    if (n == 0) return PTL_OK;
    const Ctx& m = src->c;
    const int n_chunks = (m.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr, *d_bad = nullptr;
    double *d_d2 = nullptr, *d_xyz = nullptr, *d_sum = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1); tmp.add(&d_d2, (size_t)n);
    if (given) tmp.add(&d_xyz, (size_t)n * 3);
    tmp.add(&d_sum, CMP_SUMS); tmp.add(&d_bad, 1);
    HIPCHK(tmp.err);
    Event e0, e1;
    HIPCHK(e0.create(hipEventDefault)); HIPCHK(e1.create(hipEventDefault));
    hipStream_t s = ref->stream;
    a.d2 = d_d2; a.xyz_out = d_xyz; a.bad = d_bad; a.n_alloc = (int)n;
    CmpPoolSrc ps = {m, d_off, n_chunks};
    HIPCHK(hipEventRecord(e0, s));  // (every per-point slot is written by k_cmp_points when the directory's total is the map state's - checked below)
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    k_score_count<<<(m.pool_cap + 255) / 256, 256, 0, s>>>(m, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    const int wg = (n_chunks + CMP_THREADS / 64 - 1) / (CMP_THREADS / 64);
    k_cmp_points<CmpPoolSrc><<<wg < CMP_MAX_BLOCKS ? wg : CMP_MAX_BLOCKS, CMP_THREADS, 0, s>>>(ps, ref->c, a);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipGetLastError());
    int total = 0, bad = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return set_err(PTL_ERR_STATE, "ptl_icp_map_compare: the reference map's table led %d probes to a block that does not hold the probed voxel", bad);
    if (total != (int)n) return set_err(PTL_ERR_STATE, "ptl_icp_map_compare: the source map's block directory holds %d points, its map state %lld", total, (long long)n);
    Event e2, e3;
    HIPCHK(e2.create(hipEventDefault)); HIPCHK(e3.create(hipEventDefault));
    double sums[CMP_SUMS];
    HIPCHK(hipEventRecord(e2, s));  // (the reduction reads all n slots: only behind the check that all of them were written)
    k_cmp_reduce<<<1, 1024, 0, s>>>(d_d2, (int)n, a, d_sum);
    HIPCHK(hipEventRecord(e3, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, d_sum, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    map_cmp_add(result, sums);
    float ms = 0, ms2 = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    HIPCHK(hipEventElapsedTime(&ms2, e2, e3));
    result->device_ms = (double)ms + (double)ms2;
    if (given) {
        HIPCHK(hipMemcpy(xyz_out, d_xyz, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist2_out, d_d2, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (n_written) *n_written = n;
    }
    return PTL_OK;
}

// ================================================================================================ pose search
// The definition is in include/ptudes_mi.h, the kernels in pose_kernels.h.  Everything is checked on the host before the first HIP call; the
// work buffers (the query points, one staged chunk of candidates and its counts, the running best) live for the call.
static void pose_search_defaults(ptl_pose_search_cfg* cfg, double voxel_size) {
    PTL_CFG_INIT(cfg);
    cfg->max_dist = voxel_size;
    cfg->n_thresholds = 1;
    cfg->thresholds[0] = voxel_size;
}
extern "C" int64_t ptl_pose_search_sizeof_cfg(void) { return (int64_t)sizeof(ptl_pose_search_cfg); }
extern "C" int ptl_pose_search_default_cfg(ptl_pose_search_cfg* cfg, double voxel_size) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_pose_search_cfg, cfg);
    if (!(voxel_size > 0.0) || !(voxel_size < 1.0e150)) return set_err(PTL_ERR_ARG, "voxel_size must be positive and finite (got %g)", voxel_size);
    pose_search_defaults(cfg, voxel_size);
    return PTL_OK;
}
static_assert(PTL_POSE_SEARCH_MAX_THRESHOLDS == POSE_MAX_THR && POSE_MAX_THR <= CMP_MAX_THR, "the header's threshold count is the kernels'");
static_assert(PTL_POSE_SEARCH_MAX_POINTS == POSE_MAX_POINTS, "the header's point limit is the kernels'");
extern "C" int ptl_icp_pose_hits(ptl_icp* map, const ptl_pose_search_cfg* cfg, const double* xyz, int64_t n, const double* poses16, int64_t n_poses,
                                 ptl_pose_search_result* result, int32_t* hits_out) {
    const char* who = "ptl_icp_pose_hits";
    if (!map || !result) return set_err(PTL_ERR_ARG, "%s: null argument", who);
    if (n < 0) return set_err(PTL_ERR_ARG, "%s: n = %lld: must not be negative", who, (long long)n);
    if (n > 0 && !xyz) return set_err(PTL_ERR_ARG, "%s: %lld query points without xyz", who, (long long)n);
    if (n_poses < 0) return set_err(PTL_ERR_ARG, "%s: n_poses = %lld: must not be negative", who, (long long)n_poses);
    if (n_poses > 0 && !poses16) return set_err(PTL_ERR_ARG, "%s: %lld candidates without poses16", who, (long long)n_poses);
    ptl_pose_search_cfg use;
    if (cfg) { ABI_CHECK(ptl_pose_search_cfg, cfg); use = *cfg; } else pose_search_defaults(&use, map->cfg.voxel_size);
    const double vs = map->cfg.voxel_size;
    if (!(use.max_dist > 0.0) || !(use.max_dist <= vs))
        return set_err(PTL_ERR_ARG, "%s: max_dist = %g: the 27-voxel search needs 0 < max_dist <= the map's voxel size = %g", who, use.max_dist, vs);
    if (use.n_thresholds < 1 || use.n_thresholds > POSE_MAX_THR)
        return set_err(PTL_ERR_ARG, "%s: n_thresholds = %d: must be in [1, %d]", who, use.n_thresholds, POSE_MAX_THR);
    for (int k = 0; k < use.n_thresholds; ++k) {
        const double t = use.thresholds[k];
        if (!(t > 0.0) || !(t <= use.max_dist))
            return set_err(PTL_ERR_ARG, "%s: threshold %d = %g: must be in (0, max_dist = %g]", who, k, t, use.max_dist);
        if (k > 0 && t < use.thresholds[k - 1])
            return set_err(PTL_ERR_ARG, "%s: threshold %d = %g is below threshold %d = %g: ascending order", who, k, t, k - 1, use.thresholds[k - 1]);
    }
    if (n > (int64_t)POSE_MAX_POINTS)
        return set_err(PTL_ERR_CAPACITY, "%s: n = %lld query points, at most %d are held resident for a call", who, (long long)n, POSE_MAX_POINTS);
    if (n_poses > (int64_t)0x7fffffff - POSE_CHUNK)  // (k_pose_best ranks a candidate by a 31-bit index)
        return set_err(PTL_ERR_CAPACITY, "%s: n_poses = %lld, at most %lld candidates a call", who, (long long)n_poses, (long long)0x7fffffff - POSE_CHUNK);
    const int T = use.n_thresholds;
    PoseArgs a;
    memset(&a, 0, sizeof a);
    memset(result, 0, sizeof *result);
    result->max_dist = a.cmp.max_dist = use.max_dist;
    a.cmp.max2 = use.max_dist * use.max_dist;
    result->n_thresholds = a.cmp.n_thr = T;
    for (int k = 0; k < T; ++k) { result->thresholds[k] = use.thresholds[k]; a.cmp.thr2[k] = use.thresholds[k] * use.thresholds[k]; }
    for (int k = 0; k < POSE_MAX_THR; ++k) result->best_pose[k] = -1;
    result->n_points = n;
    result->n_poses = n_poses;
    if (n == 0 && n_poses == 0) return PTL_OK;
    HIPCHK(hipSetDevice(map->cfg.device_id));
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    const int cap = (int)(n_poses < POSE_CHUNK ? n_poses : POSE_CHUNK);
    DevOwner tmp;
    double *d_xyz = nullptr, *d_poses = nullptr;
    int *d_hits = nullptr, *d_cnt = nullptr;
    long long* d_best = nullptr;
    tmp.add(&d_xyz, (size_t)(n > 0 ? n : 1) * 3); tmp.add(&d_poses, (size_t)(cap > 0 ? cap : 1) * 16);
    tmp.add(&d_hits, (size_t)(cap > 0 ? cap : 1) * POSE_MAX_THR); tmp.add(&d_best, POSE_MAX_THR);
    tmp.add(&d_cnt, 3);  // [0] inconsistent probes (cmp_query's `bad`), [1] invalid query points, [2] invalid candidates
    HIPCHK(tmp.err);
    Event e0, e1;
    HIPCHK(e0.create(hipEventDefault)); HIPCHK(e1.create(hipEventDefault));
    hipStream_t s = map->stream;
    a.cmp.bad = d_cnt; a.xyz = d_xyz; a.n = (int)n; a.poses = d_poses; a.hits = d_hits;
    HIPCHK(hipEventRecord(e0, s));
    HIPCHK(hipMemsetAsync(d_cnt, 0, 3 * sizeof(int), s));
    if (n > 0) HIPCHK(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 24, hipMemcpyHostToDevice, s));
    k_pose_invalid<<<1, 1024, 0, s>>>(d_xyz, (int)n, d_cnt + 1);
    // (one staging buffer: the stream's order keeps a chunk's kernels and its copy back ahead of the next chunk's copy in)
    for (int64_t off = 0; off < n_poses; off += POSE_CHUNK) {
        const int m = (int)(n_poses - off < POSE_CHUNK ? n_poses - off : POSE_CHUNK);
        HIPCHK(hipMemcpyAsync(d_poses, poses16 + 16 * off, (size_t)m * 128, hipMemcpyHostToDevice, s));
        a.n_poses = m;
        k_pose_hits<<<m < POSE_MAX_BLOCKS ? m : POSE_MAX_BLOCKS, POSE_THREADS, 0, s>>>(map->c, a);
        k_pose_best<<<1, 1024, 0, s>>>(d_hits, m, T, (int)off, off == 0 ? 1 : 0, d_best, d_cnt + 2);
        if (hits_out) HIPCHK(hipMemcpyAsync(hits_out + off * T, d_hits, (size_t)m * T * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipGetLastError());
    int cnt[3] = {0, 0, 0};
    long long best[POSE_MAX_THR] = {-1, -1, -1, -1};
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
    if (n_poses > 0) HIPCHK(hipMemcpyAsync(best, d_best, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cnt[0]) return set_err(PTL_ERR_STATE, "%s: the map's table led %d probes to a block that does not hold the probed voxel", who, cnt[0]);
    result->n_invalid_points = cnt[1];
    result->n_invalid_poses = cnt[2];
    for (int k = 0; k < T; ++k)
        if (best[k] >= 0) { result->best_hits[k] = best[k] >> 32; result->best_pose[k] = 0x7fffffffll - (best[k] & 0xffffffffll); }
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    result->device_ms = ms;
    return PTL_OK;
}

// ================================================================================================ free space carved
// The definition is in include/ptudes_mi.h, the kernels in carve_kernels.h.  Everything is checked on the host before the first HIP call.  The
// carve handle owns what its passes need - stream, column table, sweep staging, prefixes, vote arrays, counters - and only reads the map handle.
struct ptl_carve {
    int device_id = 0;  // (first member, as in ptl_traj)
    ptl_icp* map = nullptr;
    ptl_carve_cfg cfg;
    int64_t n_points = 0;  // the map's point count at create: every add and read compares
    int n_alloc = 1;
    double device_ms = 0;
    Stream stream;
    Event e0, e1;
    double* coltab = nullptr;   // [12][W]
    double* d_ts = nullptr;     // [W]
    void* d_raw = nullptr;      // one sweep of the caller's: n_max pixels of f32 xyz or u32 ranges
    FlyWs* d_fly = nullptr;     // k_fly_coltab's flag
    int* d_blk_off = nullptr;   // [pool_cap]
    unsigned *d_through = nullptr, *d_support = nullptr;  // [n_alloc], pool order
    double* d_xyz = nullptr;    // [n_alloc][3], made by the first read that asks for it
    unsigned long long* d_counts = nullptr;  // [CARVE_COUNTERS] + 4 of the read's reduction
    int* d_bad = nullptr;
    unsigned long long counts[CARVE_COUNTERS] = {};  // the host's copy after the last add
    DevOwner mem;
};
static void carve_defaults(ptl_carve_cfg* cfg, double vs) {
    PTL_CFG_INIT(cfg);
    cfg->radius = vs / 10.0; cfg->margin = vs; cfg->step = vs / 2.0; cfg->min_range = 0.0; cfg->max_range = 120.0 * vs;
}
extern "C" int64_t ptl_carve_sizeof_cfg(void) { return (int64_t)sizeof(ptl_carve_cfg); }
extern "C" int ptl_carve_default_cfg(ptl_carve_cfg* cfg, double voxel_size) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_carve_cfg, cfg);
    if (!(voxel_size > 0.0) || !(voxel_size < 1.0e150)) return set_err(PTL_ERR_ARG, "voxel_size must be positive and finite (got %g)", voxel_size);
    carve_defaults(cfg, voxel_size);
    return PTL_OK;
}
// the event pair around a piece of the handle's device work, added to its device_ms (the stream has been waited for)
static int carve_clock(ptl_carve* h) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    h->device_ms += ms;
    return PTL_OK;
}
// the map as it is now: its update waited for, its point count against the snapshot
static int carve_map_unchanged(ptl_carve* h, const char* who) {
    ptl_icp* m = h->map;
    HIPCHK(hipSetDevice(h->device_id));
    HIPCHK(hipStreamSynchronize(m->map_stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, m->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((int64_t)st.map_points != h->n_points)
        return set_err(PTL_ERR_STATE, "%s: the map holds %lld points, it held %lld at ptl_carve_create: a map updated since then needs a new carve handle", who,
                       (long long)st.map_points, (long long)h->n_points);
    return PTL_OK;
}
extern "C" int ptl_carve_create(ptl_icp* map, const ptl_carve_cfg* cfg, ptl_carve** out) {
    if (!map || !out) return set_err(PTL_ERR_ARG, "ptl_carve_create: null argument");
    ptl_carve_cfg use;
    if (cfg) { ABI_CHECK(ptl_carve_cfg, cfg); use = *cfg; } else carve_defaults(&use, map->cfg.voxel_size);
    const double vs = map->cfg.voxel_size;
    if (!(use.radius > 0.0) || !(use.radius < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_carve_create: radius = %g: must be positive and finite", use.radius);
    if (!(use.margin >= 0.0) || !(use.margin < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_carve_create: margin = %g: must be >= 0 and finite", use.margin);
    if (!(use.step > 0.0) || !(use.step <= vs))
        return set_err(PTL_ERR_ARG, "ptl_carve_create: step = %g: the march needs 0 < step <= the map's voxel size = %g", use.step, vs);
    if (!(use.min_range >= 0.0)) return set_err(PTL_ERR_ARG, "ptl_carve_create: min_range = %g: must be >= 0", use.min_range);
    if (!(use.max_range > use.min_range)) return set_err(PTL_ERR_ARG, "ptl_carve_create: max_range = %g: must be above min_range = %g", use.max_range, use.min_range);
    if (!(use.max_range / use.step <= (double)CARVE_MAX_SAMPLES))
        return set_err(PTL_ERR_ARG, "ptl_carve_create: max_range / step = %g / %g = %g samples per ray: the limit is %d", use.max_range, use.step,
                       use.max_range / use.step, CARVE_MAX_SAMPLES);
    HIPCHK(hipSetDevice(map->cfg.device_id));
    std::unique_ptr<ptl_carve> h(new ptl_carve());
    h->device_id = map->cfg.device_id; h->map = map; h->cfg = use;
    HIPCHK(h->stream.create());
    HIPCHK(h->e0.create(hipEventDefault)); HIPCHK(h->e1.create(hipEventDefault));
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    HIPCHK(hipStreamSynchronize(map->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t n = st.map_points;
    if (n < 0 || n > (int64_t)0x7fffffff) return set_err(PTL_ERR_STATE, "ptl_carve_create: the map reports %lld points", (long long)n);
    h->n_points = n; h->n_alloc = n > 0 ? (int)n : 1;
    const Ctx& c = map->c;
    const int n_chunks = (c.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    const size_t px = (size_t)map->n_max;
    h->mem.add(&h->coltab, (size_t)12 * c.W); h->mem.add(&h->d_ts, (size_t)c.W);
    { unsigned char* raw = nullptr; h->mem.add(&raw, px * 12); h->d_raw = raw; }
    h->mem.add(&h->d_fly, 1); h->mem.add(&h->d_blk_off, (size_t)c.pool_cap);
    h->mem.add(&h->d_through, (size_t)h->n_alloc); h->mem.add(&h->d_support, (size_t)h->n_alloc);
    h->mem.add(&h->d_counts, (size_t)CARVE_COUNTERS + 4); h->mem.add(&h->d_bad, 1);
    HIPCHK(h->mem.err);
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1);
    HIPCHK(tmp.err);
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->e0, s));
    HIPCHK(hipMemsetAsync(h->d_fly, 0, sizeof(FlyWs), s));
    HIPCHK(hipMemsetAsync(h->d_through, 0, (size_t)h->n_alloc * 4, s));
    HIPCHK(hipMemsetAsync(h->d_support, 0, (size_t)h->n_alloc * 4, s));
    HIPCHK(hipMemsetAsync(h->d_counts, 0, ((size_t)CARVE_COUNTERS + 4) * 8, s));
    HIPCHK(hipMemsetAsync(h->d_bad, 0, sizeof(int), s));
    k_score_count<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    k_carve_blkoff<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_off, h->d_blk_off);
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total != (int)n) return set_err(PTL_ERR_STATE, "ptl_carve_create: the block directory holds %d points, the map state %lld", total, (long long)n);
    { int rc = carve_clock(h.get()); if (rc) return rc; }
    *out = h.release();
    return PTL_OK;
}
extern "C" int ptl_carve_destroy(ptl_carve* c) { return c ? handle_destroy(c, c->device_id) : PTL_OK; }
// what every add checks before any HIP call
static int carve_check(ptl_carve* h, const ptl_traj* t, const ptl_lut* lut, int64_t H, int64_t W, const char* who) {
    const ptl_icp* m = h->map;
    if (t->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: trajectory on device %d, map on device %d", who, t->device_id, h->device_id);
    if (lut && lut->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: LUT on device %d, map on device %d", who, lut->device_id, h->device_id);
    if (H < 1 || W < 1) return set_err(PTL_ERR_ARG, "%s: empty scan (%lld x %lld)", who, (long long)H, (long long)W);
    if (W != m->c.W) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld columns, the map handle's scan_cols is %d", who, (long long)W, m->c.W);
    if (H * W > m->n_max) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld pixels, the map handle's max_points_per_scan is %lld", who, (long long)(H * W), (long long)m->n_max);
    return PTL_OK;
}
// one sweep enqueued on the carve handle's stream; raw (device): the sweep; d_col_ts (device, W) or the sweep's (t0, t1)
static int carve_enqueue(ptl_carve* h, const ptl_traj* t, const void* raw, bool is_range, const ptl_lut* lut, int H, int W, const double* d_col_ts,
                         double t0, double t1) {
    const Ctx& c = h->map->c;
    hipStream_t s = h->stream;
    const int n = H * W;
    CarveArgs a = {};
    a.r2 = h->cfg.radius * h->cfg.radius; a.margin = h->cfg.margin; a.step = h->cfg.step; a.min_range = h->cfg.min_range; a.max_range = h->cfg.max_range;
    a.blk_off = h->d_blk_off; a.through = h->d_through; a.support = h->d_support; a.n_alloc = h->n_alloc; a.counts = h->d_counts; a.bad = h->d_bad;
    const int per_wg = (CARVE_THREADS / 64) * (64 / CARVE_LANES);
    const int wg = (n + per_wg - 1) / per_wg, grid = wg < CARVE_MAX_BLOCKS ? wg : CARVE_MAX_BLOCKS;
    k_fly_coltab<<<1, 256, 0, s>>>(t->d_kt, t->d_kp, t->n, t->before, t->after, d_col_ts, t0, t1, W, h->coltab, h->d_fly);
    if (is_range) k_carve_rays<true><<<grid, CARVE_THREADS, 0, s>>>(raw, lut->dir, lut->off, n, W, h->coltab, h->d_fly, c, a);
    else k_carve_rays<false><<<grid, CARVE_THREADS, 0, s>>>(raw, nullptr, nullptr, n, W, h->coltab, h->d_fly, c, a);
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// closes an add: the counters and the table's verdict come back, the host's copy of the counters moves on; the deltas are the call's
static int carve_finish(ptl_carve* h, int64_t* n_valid, int64_t* n_skipped, const char* who) {
    unsigned long long now[CARVE_COUNTERS];
    int bad = 0;
    HIPCHK(hipEventRecord(h->e1, h->stream));
    HIPCHK(hipMemcpyAsync(now, h->d_counts, sizeof now, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    { int rc = carve_clock(h); if (rc) return rc; }
    if (n_valid) *n_valid = (int64_t)(now[CARVE_N_RAYS] - h->counts[CARVE_N_RAYS]);
    if (n_skipped) *n_skipped = (int64_t)(now[CARVE_N_SKIPPED] - h->counts[CARVE_N_SKIPPED]);
    memcpy(h->counts, now, sizeof now);
    if (bad) return set_err(PTL_ERR_STATE, "%s: the map's table led %d probes to a block that does not hold the probed voxel", who, bad);
    return PTL_OK;
}
static int carve_add_percall(ptl_carve* h, ptl_traj* t, ptl_lut* lut, const void* raw_host, size_t raw_bytes, bool is_range, int64_t H, int64_t W,
                             const double* col_ts, int64_t* n_valid, int32_t* skipped, const char* who) {
    int rc = carve_check(h, t, lut, H, W, who);
    if (rc) return rc;
    rc = carve_map_unchanged(h, who);
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->e0, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_raw, raw_host, raw_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ts, col_ts, (size_t)W * 8, hipMemcpyHostToDevice, h->stream));
    rc = carve_enqueue(h, t, h->d_raw, is_range, lut, (int)H, (int)W, h->d_ts, 0.0, 0.0);
    if (rc) return rc;
    int64_t sk = 0;
    rc = carve_finish(h, n_valid, &sk, who);
    if (skipped) *skipped = sk ? 1 : 0;
    return rc;
}
extern "C" int ptl_carve_add_posed_range(ptl_carve* c, ptl_traj* t, ptl_lut* lut, const uint32_t* range_mm, const double* col_ts, int64_t* n_valid,
                                         int32_t* skipped) {
    if (!c || !t || !lut || !range_mm || !col_ts) return set_err(PTL_ERR_ARG, "ptl_carve_add_posed_range: null argument");
    return carve_add_percall(c, t, lut, range_mm, (size_t)lut->H * lut->W * 4, true, lut->H, lut->W, col_ts, n_valid, skipped, "ptl_carve_add_posed_range");
}
extern "C" int ptl_carve_add_posed_xyz(ptl_carve* c, ptl_traj* t, const float* xyz, int32_t H, int32_t W, const double* col_ts, int64_t* n_valid,
                                       int32_t* skipped) {
    if (!c || !t || !xyz || !col_ts) return set_err(PTL_ERR_ARG, "ptl_carve_add_posed_xyz: null argument");
    return carve_add_percall(c, t, nullptr, xyz, (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * 12, false, H, W, col_ts, n_valid, skipped, "ptl_carve_add_posed_xyz");
}
// resident form, as fly_build: sweeps [first, last] of a lane, `slot` bytes apart.  The caller has checked the runner's side and waited for its
// streams; the lane is only read.
static int carve_build(ptl_carve* h, ptl_traj* t, const SeqLane& l, size_t slot, const unsigned char* is_range_k, bool all_range, const ptl_lut* lut,
                       int64_t pps, const double* t0t1, int64_t first, int64_t last, int64_t* n_valid, int64_t* n_skipped, const char* who) {
    const int64_t W = h->map->c.W;
    if (pps % W) return set_err(PTL_ERR_CAPACITY, "%s: %lld points per sweep are no multiple of the map handle's scan_cols = %lld", who, (long long)pps, (long long)W);
    if (l.icp->c.W != W) return set_err(PTL_ERR_CAPACITY, "%s: the runner's scan_cols is %d, the map handle's %lld", who, l.icp->c.W, (long long)W);
    int rc = carve_check(h, t, lut, pps / W, W, who);
    if (rc) return rc;
    rc = carve_map_unchanged(h, who);
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->e0, h->stream));
    for (int64_t k = first; k <= last; ++k) {
        const bool rg = all_range || (is_range_k && is_range_k[(size_t)k]);
        rc = carve_enqueue(h, t, (const char*)l.d_scans + (size_t)k * slot, rg, lut, (int)(pps / W), (int)W, nullptr, t0t1[2 * k], t0t1[2 * k + 1]);
        if (rc) return rc;
    }
    return carve_finish(h, n_valid, n_skipped, who);
}
extern "C" int ptl_carve_add_seq(ptl_carve* c, ptl_seq* s, ptl_traj* t, const double* t0t1, int64_t first, int64_t last, int64_t* n_valid,
                                 int64_t* n_skipped) {
    if (!c || !s || !t || !t0t1) return set_err(PTL_ERR_ARG, "ptl_carve_add_seq: null argument");
    if (first < 0 || last < first || last >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_carve_add_seq: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)s->cfg.n_scans);
    if (s->cfg.icp.device_id != c->device_id) return set_err(PTL_ERR_ARG, "ptl_carve_add_seq: runner on device %d, map on device %d", s->cfg.icp.device_id, c->device_id);
    bool any_range = false;
    for (int64_t k = first; k <= last; ++k) any_range = any_range || s->is_range[(size_t)k];
    if (any_range && !s->lut) return set_err(PTL_ERR_STATE, "ptl_carve_add_seq: the sweeps are range images but no LUT was set (ptl_seq_set_lut)");
    HIPCHK(hipSetDevice(c->device_id));
    HIPCHK(hipStreamSynchronize(s->stream));  // the runner's own work first; its sweeps are then only read
    HIPCHK(hipStreamSynchronize(s->ekf_stream));
    return carve_build(c, t, s->lane, (size_t)s->cfg.points_per_scan * 12, s->is_range.data(), false, any_range ? s->lut : nullptr, s->cfg.points_per_scan,
                       t0t1, first, last, n_valid, n_skipped, "ptl_carve_add_seq");
}
extern "C" int ptl_carve_add_batch(ptl_carve* c, ptl_batch* b, int32_t seq, ptl_traj* t, const double* t0t1, int64_t first, int64_t last,
                                   int64_t* n_valid, int64_t* n_skipped) {
    if (!c || !b || !t || !t0t1) return set_err(PTL_ERR_ARG, "ptl_carve_add_batch: null argument");
    if (seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "ptl_carve_add_batch: sequence %d of %d", seq, b->S);
    if (first < 0 || last < first || last >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_carve_add_batch: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)b->cfg.n_scans);
    if (b->cfg.icp.device_id != c->device_id) return set_err(PTL_ERR_ARG, "ptl_carve_add_batch: batch on device %d, map on device %d", b->cfg.icp.device_id, c->device_id);
    if (b->ring < b->cfg.n_scans) return set_err(PTL_ERR_STATE, "ptl_carve_add_batch: the batch keeps a ring of %lld sweep slots (resident_scans): earlier sweeps are gone", (long long)b->ring);
    if (b->cfg.range_input && !b->lut) return set_err(PTL_ERR_STATE, "ptl_carve_add_batch: a range-input batch needs its LUT (ptl_batch_set_lut)");
    HIPCHK(hipSetDevice(c->device_id));
    HIPCHK(hipStreamSynchronize(b->stream));  // the batch's own work first; its sweeps are then only read
    HIPCHK(hipStreamSynchronize(b->side));
    const size_t slot = (size_t)b->cfg.points_per_scan * (b->cfg.range_input ? 4 : 12);
    return carve_build(c, t, b->lane[seq], slot, nullptr, b->is_range != 0, b->is_range ? b->lut : nullptr, b->cfg.points_per_scan, t0t1, first, last,
                       n_valid, n_skipped, "ptl_carve_add_batch");
}
extern "C" int ptl_carve_read(ptl_carve* h, ptl_carve_result* result, double* xyz_out, uint32_t* through_out, uint32_t* support_out, int64_t max_points,
                              int64_t* n_written) {
    if (!h || !result) return set_err(PTL_ERR_ARG, "ptl_carve_read: null argument");
    const int given = (xyz_out != nullptr) + (through_out != nullptr) + (support_out != nullptr);
    if (given != 0 && given != 3) return set_err(PTL_ERR_ARG, "ptl_carve_read: the three per-point arrays (xyz, through, support) are given together or not at all (%d given)", given);
    if (given && max_points < 0) return set_err(PTL_ERR_ARG, "ptl_carve_read: max_points = %lld: must not be negative", (long long)max_points);
    const int64_t n = h->n_points;
    if (given && max_points < n) return set_err(PTL_ERR_CAPACITY, "ptl_carve_read: the map holds %lld points, max_points = %lld", (long long)n, (long long)max_points);
    { int rc = carve_map_unchanged(h, "ptl_carve_read"); if (rc) return rc; }
    if (n_written) *n_written = 0;
    hipStream_t s = h->stream;
    if (given && n > 0 && !h->d_xyz) HIPCHK(h->mem.alloc(&h->d_xyz, (size_t)n * 3));
    unsigned long long sums[4] = {0, 0, 0, 0};
    HIPCHK(hipEventRecord(h->e0, s));
    k_carve_reduce<<<1, 1024, 0, s>>>(h->d_through, h->d_support, (int)n, h->d_counts + CARVE_COUNTERS);
    if (given && n > 0) k_carve_export<<<(h->map->c.pool_cap + 255) / 256, 256, 0, s>>>(h->map->c, h->d_blk_off, h->n_alloc, h->d_xyz);
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, h->d_counts + CARVE_COUNTERS, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    { int rc = carve_clock(h); if (rc) return rc; }
    memset(result, 0, sizeof *result);
    result->n_points = n;
    result->n_scans = (int64_t)h->counts[CARVE_N_SCANS]; result->n_scans_skipped = (int64_t)h->counts[CARVE_N_SKIPPED];
    result->n_rays = (int64_t)h->counts[CARVE_N_RAYS]; result->n_rays_out_of_range = (int64_t)h->counts[CARVE_N_OOR];
    result->n_no_return = (int64_t)h->counts[CARVE_N_NORET]; result->n_voxel_visits = (int64_t)h->counts[CARVE_N_VISITS];
    result->n_points_through = (int64_t)sums[0]; result->n_points_supported = (int64_t)sums[1];
    result->sum_through = (int64_t)sums[2]; result->sum_support = (int64_t)sums[3];
    result->radius = h->cfg.radius; result->margin = h->cfg.margin; result->step = h->cfg.step;
    result->min_range = h->cfg.min_range; result->max_range = h->cfg.max_range;
    result->device_ms = h->device_ms;
    if (given && n > 0) {
        HIPCHK(hipMemcpy(xyz_out, h->d_xyz, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(through_out, h->d_through, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(support_out, h->d_support, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (given && n_written) *n_written = n;
    return PTL_OK;
}

// ================================================================================================ rays cast through a map
// The definition is in include/ptudes_mi.h, the kernel in cast_kernels.h.  Everything is checked on the host before the first HIP call.  The
// cast handle owns what its pass needs - stream, column table, sweep staging, prefixes, per-pixel outputs, counters - and only reads the map
// handle.  Nothing is kept between calls but the prefixes.
struct ptl_cast {
    int device_id = 0;  // (first member, as in ptl_traj)
    ptl_icp* map = nullptr;
    ptl_cast_cfg cfg;
    int64_t n_points = 0;  // the map's point count at create: every call compares
    int n_alloc = 1;
    Stream stream;
    Event e0, e1;
    double* coltab = nullptr;   // [12][W]
    double* d_ts = nullptr;     // [W]
    void* d_raw = nullptr;      // one sweep of the caller's: n_max pixels of f32 xyz or u32 ranges
    FlyWs* d_fly = nullptr;     // k_fly_coltab's flag
    int* d_blk_off = nullptr;   // [pool_cap]
    unsigned char* d_status = nullptr;  // [n_max] per pixel, as are the next three
    double *d_t = nullptr, *d_len = nullptr;
    int* d_index = nullptr;
    double* d_xyz = nullptr;    // [n_alloc][3], made by the first ptl_cast_points
    unsigned long long* d_counts = nullptr;  // [CAST_COUNTERS]
    int* d_bad = nullptr;
    DevOwner mem;
};
static void cast_defaults(ptl_cast_cfg* cfg, double vs) {
    PTL_CFG_INIT(cfg);
    cfg->radius = vs / 5.0; cfg->step = vs / 2.0; cfg->min_range = 0.0; cfg->max_range = 120.0 * vs;
}
extern "C" int64_t ptl_cast_sizeof_cfg(void) { return (int64_t)sizeof(ptl_cast_cfg); }
extern "C" int ptl_cast_default_cfg(ptl_cast_cfg* cfg, double voxel_size) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_cast_cfg, cfg);
    if (!(voxel_size > 0.0) || !(voxel_size < 1.0e150)) return set_err(PTL_ERR_ARG, "voxel_size must be positive and finite (got %g)", voxel_size);
    cast_defaults(cfg, voxel_size);
    return PTL_OK;
}
// the map as it is now: its update waited for, its point count against the snapshot
static int cast_map_unchanged(ptl_cast* h, const char* who) {
    ptl_icp* m = h->map;
    HIPCHK(hipSetDevice(h->device_id));
    HIPCHK(hipStreamSynchronize(m->map_stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, m->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((int64_t)st.map_points != h->n_points)
        return set_err(PTL_ERR_STATE, "%s: the map holds %lld points, it held %lld at ptl_cast_create: a map updated since then needs a new cast handle", who,
                       (long long)st.map_points, (long long)h->n_points);
    return PTL_OK;
}
extern "C" int ptl_cast_create(ptl_icp* map, const ptl_cast_cfg* cfg, ptl_cast** out) {
    if (!map || !out) return set_err(PTL_ERR_ARG, "ptl_cast_create: null argument");
    ptl_cast_cfg use;
    if (cfg) { ABI_CHECK(ptl_cast_cfg, cfg); use = *cfg; } else cast_defaults(&use, map->cfg.voxel_size);
    const double vs = map->cfg.voxel_size;
    if (!(use.radius > 0.0) || !(use.radius < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_cast_create: radius = %g: must be positive and finite", use.radius);
    if (!(use.step > 0.0) || !(use.step <= vs))
        return set_err(PTL_ERR_ARG, "ptl_cast_create: step = %g: the march needs 0 < step <= the map's voxel size = %g", use.step, vs);
    if (!(use.min_range >= 0.0)) return set_err(PTL_ERR_ARG, "ptl_cast_create: min_range = %g: must be >= 0", use.min_range);
    if (!(use.max_range > use.min_range)) return set_err(PTL_ERR_ARG, "ptl_cast_create: max_range = %g: must be above min_range = %g", use.max_range, use.min_range);
    if (!(use.max_range / use.step <= (double)CAST_MAX_SAMPLES))
        return set_err(PTL_ERR_ARG, "ptl_cast_create: max_range / step = %g / %g = %g samples per ray: the limit is %d", use.max_range, use.step,
                       use.max_range / use.step, CAST_MAX_SAMPLES);
    HIPCHK(hipSetDevice(map->cfg.device_id));
    std::unique_ptr<ptl_cast> h(new ptl_cast());
    h->device_id = map->cfg.device_id; h->map = map; h->cfg = use;
    HIPCHK(h->stream.create());
    HIPCHK(h->e0.create(hipEventDefault)); HIPCHK(h->e1.create(hipEventDefault));
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    HIPCHK(hipStreamSynchronize(map->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t n = st.map_points;
    if (n < 0 || n > (int64_t)0x7fffffff) return set_err(PTL_ERR_STATE, "ptl_cast_create: the map reports %lld points", (long long)n);
    h->n_points = n; h->n_alloc = n > 0 ? (int)n : 1;
    const Ctx& c = map->c;
    const int n_chunks = (c.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    const size_t px = (size_t)map->n_max;
    h->mem.add(&h->coltab, (size_t)12 * c.W); h->mem.add(&h->d_ts, (size_t)c.W);
    { unsigned char* raw = nullptr; h->mem.add(&raw, px * 12); h->d_raw = raw; }
    h->mem.add(&h->d_fly, 1); h->mem.add(&h->d_blk_off, (size_t)c.pool_cap);
    h->mem.add(&h->d_status, px); h->mem.add(&h->d_t, px); h->mem.add(&h->d_len, px); h->mem.add(&h->d_index, px);
    h->mem.add(&h->d_counts, (size_t)CAST_COUNTERS); h->mem.add(&h->d_bad, 1);
    HIPCHK(h->mem.err);
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1);
    HIPCHK(tmp.err);
    hipStream_t s = h->stream;
    HIPCHK(hipMemsetAsync(h->d_fly, 0, sizeof(FlyWs), s));
    HIPCHK(hipMemsetAsync(h->d_bad, 0, sizeof(int), s));
    k_score_count<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    k_carve_blkoff<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_off, h->d_blk_off);
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total != (int)n) return set_err(PTL_ERR_STATE, "ptl_cast_create: the block directory holds %d points, the map state %lld", total, (long long)n);
    *out = h.release();
    return PTL_OK;
}
extern "C" int ptl_cast_destroy(ptl_cast* c) { return c ? handle_destroy(c, c->device_id) : PTL_OK; }
// what every call checks before any HIP call
static int cast_check(ptl_cast* h, const ptl_traj* t, const ptl_lut* lut, int64_t H, int64_t W, const char* who) {
    const ptl_icp* m = h->map;
    if (t->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: trajectory on device %d, map on device %d", who, t->device_id, h->device_id);
    if (lut && lut->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: LUT on device %d, map on device %d", who, lut->device_id, h->device_id);
    if (H < 1 || W < 1) return set_err(PTL_ERR_ARG, "%s: empty scan (%lld x %lld)", who, (long long)H, (long long)W);
    if (W != m->c.W) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld columns, the map handle's scan_cols is %d", who, (long long)W, m->c.W);
    if (H * W > m->n_max) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld pixels, the map handle's max_points_per_scan is %lld", who, (long long)(H * W), (long long)m->n_max);
    return PTL_OK;
}
static int cast_percall(ptl_cast* h, ptl_traj* t, ptl_lut* lut, const void* raw_host, size_t raw_bytes, bool is_range, int64_t H, int64_t W,
                        const double* col_ts, ptl_cast_result* result, uint8_t* status_out, double* t_out, double* len_out, int32_t* index_out,
                        const char* who) {
    int rc = cast_check(h, t, lut, H, W, who);
    if (rc) return rc;
    rc = cast_map_unchanged(h, who);
    if (rc) return rc;
    const Ctx& c = h->map->c;
    hipStream_t s = h->stream;
    const int n = (int)(H * W);
    CastArgs a = {};
    a.r2 = h->cfg.radius * h->cfg.radius; a.step = h->cfg.step; a.min_range = h->cfg.min_range; a.max_range = h->cfg.max_range;
    a.blk_off = h->d_blk_off; a.n_alloc = h->n_alloc; a.status = h->d_status; a.t_hit = h->d_t; a.len = h->d_len; a.index = h->d_index;
    a.counts = h->d_counts; a.bad = h->d_bad;
    const int per_wg = (CAST_THREADS / 64) * 2;
    const int wg = (n + per_wg - 1) / per_wg, grid = wg < CAST_MAX_BLOCKS ? wg : CAST_MAX_BLOCKS;
    HIPCHK(hipEventRecord(h->e0, s));
    HIPCHK(hipMemcpyAsync(h->d_raw, raw_host, raw_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_ts, col_ts, (size_t)W * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->d_counts, 0, (size_t)CAST_COUNTERS * 8, s));
    HIPCHK(hipMemsetAsync(h->d_bad, 0, sizeof(int), s));
    k_fly_coltab<<<1, 256, 0, s>>>(t->d_kt, t->d_kp, t->n, t->before, t->after, h->d_ts, 0.0, 0.0, (int)W, h->coltab, h->d_fly);
    if (is_range) k_cast_rays<true><<<grid, CAST_THREADS, 0, s>>>(h->d_raw, lut->dir, lut->off, n, (int)W, h->coltab, h->d_fly, c, a);
    else k_cast_rays<false><<<grid, CAST_THREADS, 0, s>>>(h->d_raw, nullptr, nullptr, n, (int)W, h->coltab, h->d_fly, c, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->e1, s));
    unsigned long long now[CAST_COUNTERS];
    int bad = 0;
    HIPCHK(hipMemcpyAsync(now, h->d_counts, sizeof now, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return set_err(PTL_ERR_STATE, "%s: the map's table led %d probes to a block that does not hold the probed voxel", who, bad);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    if (status_out) HIPCHK(hipMemcpy(status_out, h->d_status, (size_t)n, hipMemcpyDeviceToHost));
    if (t_out) HIPCHK(hipMemcpy(t_out, h->d_t, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (len_out) HIPCHK(hipMemcpy(len_out, h->d_len, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (index_out) HIPCHK(hipMemcpy(index_out, h->d_index, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (result) {
        memset(result, 0, sizeof *result);
        result->n_pixels = n;
        result->n_no_return = (int64_t)now[CAST_N_NORET]; result->n_degenerate = (int64_t)now[CAST_N_DEGEN];
        result->n_hit = (int64_t)now[CAST_N_HIT]; result->n_miss = (int64_t)now[CAST_N_MISS];
        result->n_voxel_visits = (int64_t)now[CAST_N_VISITS];
        result->skipped = now[CAST_N_SKIPPED] ? 1 : 0;
        result->radius = h->cfg.radius; result->step = h->cfg.step; result->min_range = h->cfg.min_range; result->max_range = h->cfg.max_range;
        result->device_ms = ms;
    }
    return PTL_OK;
}
extern "C" int ptl_cast_posed_range(ptl_cast* c, ptl_traj* t, ptl_lut* lut, const uint32_t* range_mm, const double* col_ts, ptl_cast_result* result,
                                    uint8_t* status_out, double* t_out, double* len_out, int32_t* index_out) {
    if (!c || !t || !lut || !range_mm || !col_ts) return set_err(PTL_ERR_ARG, "ptl_cast_posed_range: null argument");
    return cast_percall(c, t, lut, range_mm, (size_t)lut->H * lut->W * 4, true, lut->H, lut->W, col_ts, result, status_out, t_out, len_out, index_out,
                        "ptl_cast_posed_range");
}
extern "C" int ptl_cast_posed_xyz(ptl_cast* c, ptl_traj* t, const float* xyz, int32_t H, int32_t W, const double* col_ts, ptl_cast_result* result,
                                  uint8_t* status_out, double* t_out, double* len_out, int32_t* index_out) {
    if (!c || !t || !xyz || !col_ts) return set_err(PTL_ERR_ARG, "ptl_cast_posed_xyz: null argument");
    return cast_percall(c, t, nullptr, xyz, (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * 12, false, H, W, col_ts, result, status_out, t_out, len_out,
                        index_out, "ptl_cast_posed_xyz");
}
extern "C" int ptl_cast_points(ptl_cast* h, double* xyz_out, int64_t max_points, int64_t* n_written) {
    if (!h || !xyz_out) return set_err(PTL_ERR_ARG, "ptl_cast_points: null argument");
    if (max_points < 0) return set_err(PTL_ERR_ARG, "ptl_cast_points: max_points = %lld: must not be negative", (long long)max_points);
    const int64_t n = h->n_points;
    if (max_points < n) return set_err(PTL_ERR_CAPACITY, "ptl_cast_points: the map holds %lld points, max_points = %lld", (long long)n, (long long)max_points);
    { int rc = cast_map_unchanged(h, "ptl_cast_points"); if (rc) return rc; }
    if (n_written) *n_written = 0;
    if (n > 0) {
        hipStream_t s = h->stream;
        if (!h->d_xyz) HIPCHK(h->mem.alloc(&h->d_xyz, (size_t)n * 3));
        k_carve_export<<<(h->map->c.pool_cap + 255) / 256, 256, 0, s>>>(h->map->c, h->d_blk_off, h->n_alloc, h->d_xyz);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(xyz_out, h->d_xyz, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
    }
    if (n_written) *n_written = n;
    return PTL_OK;
}

// ================================================================================================ the map painted
// The definition is in include/ptudes_mi.h, the kernels in paint_kernels.h.  Everything is checked on the host before the first HIP call.  The
// paint handle owns what its passes need - stream, column table, sweep and field staging, prefixes, sum and count arrays, counters - and only
// reads the map handle.
struct ptl_paint {
    int device_id = 0;  // (first member, as in ptl_traj)
    ptl_icp* map = nullptr;
    int64_t n_points = 0;  // the map's point count at create: every add and read compares
    int n_alloc = 1;
    double device_ms = 0;
    Stream stream;
    Event e0, e1;
    double* coltab = nullptr;   // [12][W]
    double* d_ts = nullptr;     // [W]
    void* d_raw = nullptr;      // one sweep of the caller's: n_max pixels of f32 xyz or u32 ranges
    unsigned* d_field = nullptr;  // [n_max] the sweep's field image
    FlyWs* d_fly = nullptr;     // k_fly_coltab's flag
    int* d_blk_off = nullptr;   // [pool_cap]
    unsigned long long* d_sum = nullptr;  // [n_alloc], pool order
    unsigned* d_count = nullptr;          // [n_alloc]
    double* d_xyz = nullptr;    // [n_alloc][3], made by the first read that asks for it
    unsigned long long* d_counts = nullptr;  // [PAINT_COUNTERS] + 2 of the read's reduction
    int* d_bad = nullptr;
    unsigned long long counts[PAINT_COUNTERS] = {};  // the host's copy after the last add
    DevOwner mem;
};
extern "C" int64_t ptl_paint_sizeof_result(void) { return (int64_t)sizeof(ptl_paint_result); }
// the event pair around a piece of the handle's device work, added to its device_ms (the stream has been waited for)
static int paint_clock(ptl_paint* h) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    h->device_ms += ms;
    return PTL_OK;
}
// the map as it is now: its update waited for, its point count against the snapshot
static int paint_map_unchanged(ptl_paint* h, const char* who) {
    ptl_icp* m = h->map;
    HIPCHK(hipSetDevice(h->device_id));
    HIPCHK(hipStreamSynchronize(m->map_stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, m->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((int64_t)st.map_points != h->n_points)
        return set_err(PTL_ERR_STATE, "%s: the map holds %lld points, it held %lld at ptl_paint_create: a map updated since then needs a new paint handle", who,
                       (long long)st.map_points, (long long)h->n_points);
    return PTL_OK;
}
extern "C" int ptl_paint_create(ptl_icp* map, ptl_paint** out) {
    if (!map || !out) return set_err(PTL_ERR_ARG, "ptl_paint_create: null argument");
    HIPCHK(hipSetDevice(map->cfg.device_id));
    std::unique_ptr<ptl_paint> h(new ptl_paint());
    h->device_id = map->cfg.device_id; h->map = map;
    HIPCHK(h->stream.create());
    HIPCHK(h->e0.create(hipEventDefault)); HIPCHK(h->e1.create(hipEventDefault));
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    HIPCHK(hipStreamSynchronize(map->stream));
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t n = st.map_points;
    if (n < 0 || n > (int64_t)0x7fffffff) return set_err(PTL_ERR_STATE, "ptl_paint_create: the map reports %lld points", (long long)n);
    h->n_points = n; h->n_alloc = n > 0 ? (int)n : 1;
    const Ctx& c = map->c;
    const int n_chunks = (c.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    const size_t px = (size_t)map->n_max;
    h->mem.add(&h->coltab, (size_t)12 * c.W); h->mem.add(&h->d_ts, (size_t)c.W);
    { unsigned char* raw = nullptr; h->mem.add(&raw, px * 12); h->d_raw = raw; }
    h->mem.add(&h->d_field, px);
    h->mem.add(&h->d_fly, 1); h->mem.add(&h->d_blk_off, (size_t)c.pool_cap);
    h->mem.add(&h->d_sum, (size_t)h->n_alloc); h->mem.add(&h->d_count, (size_t)h->n_alloc);
    h->mem.add(&h->d_counts, (size_t)PAINT_COUNTERS + 2); h->mem.add(&h->d_bad, 1);
    HIPCHK(h->mem.err);
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1);
    HIPCHK(tmp.err);
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->e0, s));
    HIPCHK(hipMemsetAsync(h->d_fly, 0, sizeof(FlyWs), s));
    HIPCHK(hipMemsetAsync(h->d_sum, 0, (size_t)h->n_alloc * 8, s));
    HIPCHK(hipMemsetAsync(h->d_count, 0, (size_t)h->n_alloc * 4, s));
    HIPCHK(hipMemsetAsync(h->d_counts, 0, ((size_t)PAINT_COUNTERS + 2) * 8, s));
    HIPCHK(hipMemsetAsync(h->d_bad, 0, sizeof(int), s));
    k_score_count<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    k_carve_blkoff<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_off, h->d_blk_off);
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total != (int)n) return set_err(PTL_ERR_STATE, "ptl_paint_create: the block directory holds %d points, the map state %lld", total, (long long)n);
    { int rc = paint_clock(h.get()); if (rc) return rc; }
    *out = h.release();
    return PTL_OK;
}
extern "C" int ptl_paint_destroy(ptl_paint* p) { return p ? handle_destroy(p, p->device_id) : PTL_OK; }
// one sweep: checked before any HIP call, staged (sweep, field, column times), enqueued behind k_fly_coltab, the counters and the table's
// verdict read back; the deltas of the counters are the call's
static int paint_add_percall(ptl_paint* h, ptl_traj* t, ptl_lut* lut, const void* raw_host, size_t raw_bytes, bool is_range, const uint32_t* field,
                             int64_t H, int64_t W, const double* col_ts, int64_t* n_matched, int32_t* skipped, const char* who) {
    const ptl_icp* m = h->map;
    if (t->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: trajectory on device %d, map on device %d", who, t->device_id, h->device_id);
    if (lut && lut->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: LUT on device %d, map on device %d", who, lut->device_id, h->device_id);
    if (H < 1 || W < 1) return set_err(PTL_ERR_ARG, "%s: empty scan (%lld x %lld)", who, (long long)H, (long long)W);
    if (W != m->c.W) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld columns, the map handle's scan_cols is %d", who, (long long)W, m->c.W);
    if (H * W > m->n_max) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld pixels, the map handle's max_points_per_scan is %lld", who, (long long)(H * W), (long long)m->n_max);
    int rc = paint_map_unchanged(h, who);
    if (rc) return rc;
    const Ctx& c = m->c;
    hipStream_t s = h->stream;
    const int n = (int)(H * W);
    HIPCHK(hipEventRecord(h->e0, s));
    HIPCHK(hipMemcpyAsync(h->d_raw, raw_host, raw_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_field, field, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_ts, col_ts, (size_t)W * 8, hipMemcpyHostToDevice, s));
    PaintArgs a = {};
    a.blk_off = h->d_blk_off; a.sum = h->d_sum; a.count = h->d_count; a.n_alloc = h->n_alloc; a.counts = h->d_counts; a.bad = h->d_bad;
    const int wg = (n + PAINT_THREADS - 1) / PAINT_THREADS, grid = wg < PAINT_MAX_BLOCKS ? wg : PAINT_MAX_BLOCKS;
    k_fly_coltab<<<1, 256, 0, s>>>(t->d_kt, t->d_kp, t->n, t->before, t->after, h->d_ts, 0.0, 0.0, (int)W, h->coltab, h->d_fly);
    if (is_range) k_paint_rays<true><<<grid, PAINT_THREADS, 0, s>>>(h->d_raw, lut->dir, lut->off, h->d_field, n, (int)W, h->coltab, h->d_fly, c, a);
    else k_paint_rays<false><<<grid, PAINT_THREADS, 0, s>>>(h->d_raw, nullptr, nullptr, h->d_field, n, (int)W, h->coltab, h->d_fly, c, a);
    HIPCHK(hipGetLastError());
    unsigned long long now[PAINT_COUNTERS];
    int bad = 0;
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipMemcpyAsync(now, h->d_counts, sizeof now, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    rc = paint_clock(h);
    if (rc) return rc;
    if (n_matched) *n_matched = (int64_t)(now[PAINT_N_MATCHED] - h->counts[PAINT_N_MATCHED]);
    if (skipped) *skipped = now[PAINT_N_SKIPPED] != h->counts[PAINT_N_SKIPPED] ? 1 : 0;
    memcpy(h->counts, now, sizeof now);
    if (bad) return set_err(PTL_ERR_STATE, "%s: the map's table led %d probes to a block that does not hold the probed voxel", who, bad);
    return PTL_OK;
}
extern "C" int ptl_paint_add_posed_range(ptl_paint* p, ptl_traj* t, ptl_lut* lut, const uint32_t* range_mm, const uint32_t* field, const double* col_ts,
                                         int64_t* n_matched, int32_t* skipped) {
    if (!p || !t || !lut || !range_mm || !field || !col_ts) return set_err(PTL_ERR_ARG, "ptl_paint_add_posed_range: null argument");
    return paint_add_percall(p, t, lut, range_mm, (size_t)lut->H * lut->W * 4, true, field, lut->H, lut->W, col_ts, n_matched, skipped, "ptl_paint_add_posed_range");
}
extern "C" int ptl_paint_add_posed_xyz(ptl_paint* p, ptl_traj* t, const float* xyz, const uint32_t* field, int32_t H, int32_t W, const double* col_ts,
                                       int64_t* n_matched, int32_t* skipped) {
    if (!p || !t || !xyz || !field || !col_ts) return set_err(PTL_ERR_ARG, "ptl_paint_add_posed_xyz: null argument");
    return paint_add_percall(p, t, nullptr, xyz, (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * 12, false, field, H, W, col_ts, n_matched, skipped, "ptl_paint_add_posed_xyz");
}
extern "C" int ptl_paint_read(ptl_paint* h, ptl_paint_result* result, double* xyz_out, uint64_t* sum_out, uint32_t* count_out, int64_t max_points,
                              int64_t* n_written) {
    if (!h || !result) return set_err(PTL_ERR_ARG, "ptl_paint_read: null argument");
    ABI_CHECK(ptl_paint_result, result);
    const int given = (xyz_out != nullptr) + (sum_out != nullptr) + (count_out != nullptr);
    if (given != 0 && given != 3) return set_err(PTL_ERR_ARG, "ptl_paint_read: the three per-point arrays (xyz, sum, count) are given together or not at all (%d given)", given);
    if (given && max_points < 0) return set_err(PTL_ERR_ARG, "ptl_paint_read: max_points = %lld: must not be negative", (long long)max_points);
    const int64_t n = h->n_points;
    if (given && max_points < n) return set_err(PTL_ERR_CAPACITY, "ptl_paint_read: the map holds %lld points, max_points = %lld", (long long)n, (long long)max_points);
    { int rc = paint_map_unchanged(h, "ptl_paint_read"); if (rc) return rc; }
    if (n_written) *n_written = 0;
    hipStream_t s = h->stream;
    if (given && n > 0 && !h->d_xyz) HIPCHK(h->mem.alloc(&h->d_xyz, (size_t)n * 3));
    unsigned long long sums[2] = {0, 0};
    HIPCHK(hipEventRecord(h->e0, s));
    k_paint_reduce<<<1, 1024, 0, s>>>(h->d_count, (int)n, h->d_counts + PAINT_COUNTERS);
    if (given && n > 0) k_carve_export<<<(h->map->c.pool_cap + 255) / 256, 256, 0, s>>>(h->map->c, h->d_blk_off, h->n_alloc, h->d_xyz);
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, h->d_counts + PAINT_COUNTERS, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    { int rc = paint_clock(h); if (rc) return rc; }
    const uint32_t size = result->struct_size, abi = result->abi_version;
    memset(result, 0, sizeof *result);
    result->struct_size = size; result->abi_version = abi;
    result->n_points = n; result->n_points_painted = (int64_t)sums[0];
    result->n_scans = (int64_t)h->counts[PAINT_N_SCANS]; result->n_scans_skipped = (int64_t)h->counts[PAINT_N_SKIPPED];
    result->n_rays_matched = (int64_t)h->counts[PAINT_N_MATCHED]; result->n_rays_unmatched = (int64_t)h->counts[PAINT_N_UNMATCHED];
    result->n_no_return = (int64_t)h->counts[PAINT_N_NORET];
    result->sum_count = (int64_t)sums[1];
    result->device_ms = h->device_ms;
    if (given && n > 0) {
        HIPCHK(hipMemcpy(xyz_out, h->d_xyz, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sum_out, h->d_sum, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(count_out, h->d_count, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (given && n_written) *n_written = n;
    return PTL_OK;
}

// ================================================================================================ revisited places
// The definition is in include/ptudes_mi.h, the kernels in place_kernels.h.  Everything is checked on the host before the first HIP call.  The
// handle owns its stream, events, both tables, one sweep's staging, the u32 cell grid of a describe, the entries with their infos (the query
// slot is entry number `capacity`) and the outputs of a match.
struct ptl_place {
    int device_id = 0;             // (first member, as in ptl_traj)
    int64_t n_entries = 0;
    ptl_place_cfg cfg;
    int Rpad = 0, RD = 0;          // column stride in bytes and in dwords
    size_t entry_bytes = 0;
    double describe_ms = 0;
    int64_t n_describes = 0;
    std::vector<double> ring_edge2, sector_dir;
    Stream stream;
    Event e0, e1;
    double* d_tab = nullptr;       // ring_edge2[R + 1], sector_dir[2 S]
    void* d_raw = nullptr;         // one sweep of the caller's: max_points_per_scan rows of f64 xyz at most
    unsigned* d_grid = nullptr;    // [S Rpad]
    unsigned long long* d_counts = nullptr;  // [PLACE_COUNTERS], then the best key of a match
    unsigned char* d_desc = nullptr;         // [capacity + 1] entries
    PlaceInfoDev* d_info = nullptr;          // [capacity + 1]
    unsigned* d_dist = nullptr;    // [capacity] each: the outputs of a match
    int *d_shift = nullptr, *d_entry = nullptr;
    DevOwner mem;
};
static_assert(sizeof(PlaceInfoDev) == sizeof(ptl_place_info), "the device's info record is ptl_place_info");
#define PLACE_MAX_CAPACITY ((int64_t)1 << 20)
#define PLACE_MAX_POINTS ((int64_t)1 << 24)
extern "C" int64_t ptl_place_sizeof_cfg(void) { return (int64_t)sizeof(ptl_place_cfg); }
extern "C" int ptl_place_default_cfg(ptl_place_cfg* cfg) {
    if (!cfg) return set_err(PTL_ERR_ARG, "ptl_place_default_cfg: cfg is null");
    ABI_CHECK(ptl_place_cfg, cfg);
    PTL_CFG_INIT(cfg);
    cfg->n_ring = 20; cfg->n_sector = 60; cfg->min_radius = 1.0; cfg->max_radius = 80.0; cfg->z_min = -2.0; cfg->z_step = 0.0625;
    cfg->capacity = 4096; cfg->max_points_per_scan = (int64_t)1 << 20;
    return PTL_OK;
}
static int place_clock(ptl_place* h, double* ms_out) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    *ms_out = ms;
    return PTL_OK;
}
static int place_zero(ptl_place* h) {
    const size_t slot = (size_t)h->cfg.capacity;
    HIPCHK(hipMemsetAsync(h->d_desc + slot * h->entry_bytes, 0, h->entry_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->d_info + slot, 0, sizeof(PlaceInfoDev), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->n_entries = 0;
    return PTL_OK;
}
extern "C" int ptl_place_create(int32_t device_id, const ptl_place_cfg* cfg, ptl_place** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "ptl_place_create: null argument");
    ABI_CHECK(ptl_place_cfg, cfg);
    const ptl_place_cfg& u = *cfg;
    if (u.n_ring < 1 || u.n_ring > PLACE_MAX_RING) return set_err(PTL_ERR_ARG, "ptl_place_create: n_ring = %d: must be in 1 .. %d", u.n_ring, PLACE_MAX_RING);
    if (u.n_sector < 4 || u.n_sector > PLACE_MAX_SECTOR) return set_err(PTL_ERR_ARG, "ptl_place_create: n_sector = %d: must be in 4 .. %d", u.n_sector, PLACE_MAX_SECTOR);
    if (!(u.max_radius < 1.0e150) || !(u.min_radius > 0.0) || !(u.min_radius < u.max_radius / (double)u.n_ring))
        return set_err(PTL_ERR_ARG, "ptl_place_create: min_radius = %g, max_radius = %g, n_ring = %d: need 0 < min_radius < max_radius / n_ring = %g, finite",
                       u.min_radius, u.max_radius, u.n_ring, u.max_radius / (double)u.n_ring);
    if (!(u.z_step > 0.0) || !(u.z_step < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_place_create: z_step = %g: must be positive and finite", u.z_step);
    if (!(fabs(u.z_min) < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_place_create: z_min = %g: must be finite", u.z_min);
    if (u.capacity < 1 || (int64_t)u.capacity > PLACE_MAX_CAPACITY)
        return set_err(PTL_ERR_ARG, "ptl_place_create: capacity = %d entries: must be in 1 .. %lld", u.capacity, (long long)PLACE_MAX_CAPACITY);
    if (u.max_points_per_scan < 1 || u.max_points_per_scan > PLACE_MAX_POINTS)
        return set_err(PTL_ERR_ARG, "ptl_place_create: max_points_per_scan = %lld: must be in 1 .. %lld", (long long)u.max_points_per_scan, (long long)PLACE_MAX_POINTS);
    if (device_id < 0) return set_err(PTL_ERR_ARG, "ptl_place_create: device_id = %d: must not be negative", device_id);
    if (ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_place> h(new ptl_place());
    const int R = u.n_ring, S = u.n_sector;
    h->device_id = device_id; h->cfg = u; h->Rpad = (R + 3) / 4 * 4; h->RD = h->Rpad / 4; h->entry_bytes = (size_t)S * h->Rpad;
    h->ring_edge2.resize((size_t)R + 1); h->sector_dir.resize((size_t)2 * S);
    h->ring_edge2[0] = u.min_radius * u.min_radius;
    for (int i = 1; i <= R; ++i) { const double e = u.max_radius * (double)i / (double)R; h->ring_edge2[(size_t)i] = e * e; }
    for (int j = 0; j < S; ++j) {
        const double t = 2.0 * 3.14159265358979323846 * (double)j / (double)S;
        h->sector_dir[(size_t)2 * j] = cos(t); h->sector_dir[(size_t)2 * j + 1] = sin(t);
    }
    HIPCHK(h->stream.create());
    HIPCHK(h->e0.create(hipEventDefault)); HIPCHK(h->e1.create(hipEventDefault));
    const size_t slots = (size_t)u.capacity + 1;
    h->mem.add(&h->d_tab, (size_t)R + 1 + 2 * (size_t)S);
    { unsigned char* raw = nullptr; h->mem.add(&raw, (size_t)u.max_points_per_scan * 24); h->d_raw = raw; }
    h->mem.add(&h->d_grid, h->entry_bytes); h->mem.add(&h->d_counts, (size_t)PLACE_COUNTERS + 1);
    h->mem.add(&h->d_desc, slots * h->entry_bytes); h->mem.add(&h->d_info, slots);
    h->mem.add(&h->d_dist, (size_t)u.capacity); h->mem.add(&h->d_shift, (size_t)u.capacity); h->mem.add(&h->d_entry, (size_t)u.capacity);
    HIPCHK(h->mem.err);
    HIPCHK(hipMemcpyAsync(h->d_tab, h->ring_edge2.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tab + R + 1, h->sector_dir.data(), (size_t)2 * S * 8, hipMemcpyHostToDevice, h->stream));
    { int rc = place_zero(h.get()); if (rc) return rc; }
    *out = h.release();
    return PTL_OK;
}
extern "C" int ptl_place_destroy(ptl_place* p) { return p ? handle_destroy(p, p->device_id) : PTL_OK; }
extern "C" int ptl_place_clear(ptl_place* p) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_clear: null argument");
    HIPCHK(hipSetDevice(p->device_id));
    return place_zero(p);
}
extern "C" int ptl_place_size(ptl_place* p, int64_t* n_entries) {
    if (!p || !n_entries) return set_err(PTL_ERR_ARG, "ptl_place_size: null argument");
    *n_entries = p->n_entries;
    return PTL_OK;
}
extern "C" int ptl_place_tables(ptl_place* p, double* ring_edge2, double* sector_dir) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_tables: null argument");
    if (ring_edge2) memcpy(ring_edge2, p->ring_edge2.data(), p->ring_edge2.size() * 8);
    if (sector_dir) memcpy(sector_dir, p->sector_dir.data(), p->sector_dir.size() * 8);
    return PTL_OK;
}
extern "C" int ptl_place_profile(ptl_place* p, double* describe_ms, int64_t* n_describes, int32_t reset) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_profile: null argument");
    if (describe_ms) *describe_ms = p->describe_ms;
    if (n_describes) *n_describes = p->n_describes;
    if (reset) { p->describe_ms = 0; p->n_describes = 0; }
    return PTL_OK;
}
// one sweep into the query slot, and behind the last entry when kept; mode as k_place_bin's; the arguments have been checked
static int place_describe(ptl_place* h, const void* raw_host, size_t raw_bytes, int mode, const ptl_lut* lut, int64_t n, const double* rot9,
                          int32_t keep, int64_t* index, ptl_place_info* info, const char* who) {
    if (rot9)
        for (int e = 0; e < 9; ++e)
            if (!(fabs(rot9[e]) < 1.0e150)) return set_err(PTL_ERR_ARG, "%s: rot9[%d] = %g: every entry must be finite", who, e, rot9[e]);
    const ptl_place_cfg& u = h->cfg;
    HIPCHK(hipSetDevice(h->device_id));
    hipStream_t s = h->stream;
    PlaceArgs a = {};
    a.R = u.n_ring; a.S = u.n_sector; a.Rpad = h->Rpad; a.z_min = u.z_min; a.z_step = u.z_step;
    a.ring_edge2 = h->d_tab; a.sector_dir = h->d_tab + u.n_ring + 1;
    a.has_rot = rot9 ? 1 : 0;
    for (int e = 0; e < 9; ++e) a.rot[e] = rot9 ? rot9[e] : 0.0;
    a.grid = h->d_grid; a.counts = h->d_counts;
    const size_t slot = (size_t)u.capacity;
    const int64_t wg = (n + PLACE_THREADS - 1) / PLACE_THREADS;
    const int blocks = (int)(wg < 1 ? 1 : wg < PLACE_MAX_BLOCKS ? wg : PLACE_MAX_BLOCKS);
    HIPCHK(hipEventRecord(h->e0, s));
    if (raw_bytes) HIPCHK(hipMemcpyAsync(h->d_raw, raw_host, raw_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->d_grid, 0, h->entry_bytes * 4, s));
    HIPCHK(hipMemsetAsync(h->d_counts, 0, (size_t)PLACE_COUNTERS * 8, s));
    if (mode == 0) k_place_bin<0><<<blocks, PLACE_THREADS, 0, s>>>(h->d_raw, lut->dir, lut->off, (long long)n, a);
    else if (mode == 1) k_place_bin<1><<<blocks, PLACE_THREADS, 0, s>>>(h->d_raw, nullptr, nullptr, (long long)n, a);
    else k_place_bin<2><<<blocks, PLACE_THREADS, 0, s>>>(h->d_raw, nullptr, nullptr, (long long)n, a);
    k_place_pack<<<1, PLACE_THREADS, 0, s>>>(h->d_grid, h->d_counts, (int)h->entry_bytes, (long long)n, h->d_desc + slot * h->entry_bytes, h->d_info + slot);
    HIPCHK(hipGetLastError());
    const bool full = keep && h->n_entries >= (int64_t)u.capacity;
    if (keep && !full) {
        const size_t at = (size_t)h->n_entries;
        HIPCHK(hipMemcpyAsync(h->d_desc + at * h->entry_bytes, h->d_desc + slot * h->entry_bytes, h->entry_bytes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(h->d_info + at, h->d_info + slot, sizeof(PlaceInfoDev), hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipEventRecord(h->e1, s));
    ptl_place_info got;
    HIPCHK(hipMemcpyAsync(&got, h->d_info + slot, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double ms = 0;
    { int rc = place_clock(h, &ms); if (rc) return rc; }
    h->describe_ms += ms; h->n_describes += 1;
    if (info) *info = got;
    if (index) *index = -1;
    if (full)
        return set_err(PTL_ERR_CAPACITY, "%s: the database holds %lld entries, its capacity is %d: nothing was appended (the query slot holds the descriptor)",
                       who, (long long)h->n_entries, u.capacity);
    if (keep) { if (index) *index = h->n_entries; h->n_entries += 1; }
    return PTL_OK;
}
extern "C" int ptl_place_describe_range(ptl_place* p, ptl_lut* lut, const uint32_t* range_mm, const double* rot9, int32_t keep, int64_t* index,
                                        ptl_place_info* info) {
    if (!p || !lut || !range_mm) return set_err(PTL_ERR_ARG, "ptl_place_describe_range: null argument");
    if (lut->device_id != p->device_id) return set_err(PTL_ERR_ARG, "ptl_place_describe_range: LUT on device %d, places on device %d", lut->device_id, p->device_id);
    const int64_t n = (int64_t)lut->H * lut->W;
    if (n > p->cfg.max_points_per_scan)
        return set_err(PTL_ERR_CAPACITY, "ptl_place_describe_range: the sweep has %lld pixels, the handle's max_points_per_scan is %lld", (long long)n,
                       (long long)p->cfg.max_points_per_scan);
    return place_describe(p, range_mm, (size_t)n * 4, 0, lut, n, rot9, keep, index, info, "ptl_place_describe_range");
}
extern "C" int ptl_place_describe_xyz(ptl_place* p, const void* xyz, int dtype, int64_t n, const double* rot9, int32_t keep, int64_t* index,
                                      ptl_place_info* info) {
    if (!p || (!xyz && n > 0)) return set_err(PTL_ERR_ARG, "ptl_place_describe_xyz: null argument");
    if (dtype != PTL_F32 && dtype != PTL_F64) return set_err(PTL_ERR_ARG, "ptl_place_describe_xyz: dtype = %d: PTL_F32 (%d) or PTL_F64 (%d)", dtype, PTL_F32, PTL_F64);
    if (n < 0) return set_err(PTL_ERR_ARG, "ptl_place_describe_xyz: n = %lld: must not be negative", (long long)n);
    if (n > p->cfg.max_points_per_scan)
        return set_err(PTL_ERR_CAPACITY, "ptl_place_describe_xyz: the sweep has %lld points, the handle's max_points_per_scan is %lld", (long long)n,
                       (long long)p->cfg.max_points_per_scan);
    return place_describe(p, xyz, (size_t)n * (dtype == PTL_F32 ? 12 : 24), dtype == PTL_F32 ? 1 : 2, nullptr, n, rot9, keep, index, info,
                          "ptl_place_describe_xyz");
}
// RD = 5 (R = 17 .. 20, the default's) has its own instance of the match kernels, every other RD the general one
extern "C" int ptl_place_match(ptl_place* p, int64_t query, int64_t first, int64_t last, uint32_t* dist_out, int32_t* shift_out, ptl_place_result* result) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_match: null argument");
    if (query < -1 || query >= p->n_entries) return set_err(PTL_ERR_ARG, "ptl_place_match: query = %lld: -1 (the query slot) or an entry below %lld", (long long)query, (long long)p->n_entries);
    const bool empty = last < first;
    if (!empty && (first < 0 || last >= p->n_entries))
        return set_err(PTL_ERR_ARG, "ptl_place_match: entries [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)p->n_entries);
    ptl_place_result res = {};
    res.best_query = query; res.best_entry = -1;
    if (!empty) {
        HIPCHK(hipSetDevice(p->device_id));
        hipStream_t s = p->stream;
        const int S = p->cfg.n_sector, RD = p->RD;
        const int64_t n = last - first + 1, tiles = (n + PLACE_TILE - 1) / PLACE_TILE, wg = (tiles + PLACE_THREADS / 64 - 1) / (PLACE_THREADS / 64);
        const int blocks = (int)(wg < PLACE_MAX_BLOCKS ? wg : PLACE_MAX_BLOCKS);
        const size_t lds = (size_t)2 * S * (RD | 1) * 4;
        const unsigned* desc = (const unsigned*)p->d_desc;
        const unsigned* q = (const unsigned*)(p->d_desc + (size_t)(query < 0 ? (int64_t)p->cfg.capacity : query) * p->entry_bytes);
        unsigned long long* d_best = p->d_counts + PLACE_COUNTERS;
        unsigned long long best = PLACE_KEY_NONE;
        HIPCHK(hipEventRecord(p->e0, s));
        HIPCHK(hipMemsetAsync(d_best, 0xff, 8, s));
        if (RD == 5) k_place_match<5><<<blocks, PLACE_THREADS, lds, s>>>(desc, q, S, RD, (int)first, (int)last, p->d_dist, p->d_shift, d_best);
        else k_place_match<0><<<blocks, PLACE_THREADS, lds, s>>>(desc, q, S, RD, (int)first, (int)last, p->d_dist, p->d_shift, d_best);
        HIPCHK(hipEventRecord(p->e1, s));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, s));
        if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, p->d_dist, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (shift_out) HIPCHK(hipMemcpyAsync(shift_out, p->d_shift, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        { int rc = place_clock(p, &res.device_ms); if (rc) return rc; }
        res.n_compared = n;
        res.best_dist = (uint32_t)(best >> 26); res.best_entry = (int64_t)((best >> 6) & 0xfffffu); res.best_shift = (int32_t)(best & 63u);
    }
    if (result) *result = res;
    return PTL_OK;
}
extern "C" int ptl_place_match_all(ptl_place* p, int64_t q_first, int64_t q_last, int64_t min_gap, int32_t* entry_out, uint32_t* dist_out,
                                   int32_t* shift_out, ptl_place_result* result) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_match_all: null argument");
    if (min_gap < 0) return set_err(PTL_ERR_ARG, "ptl_place_match_all: min_gap = %lld: must not be negative", (long long)min_gap);
    const bool empty = q_last < q_first;
    if (!empty && (q_first < 0 || q_last >= p->n_entries))
        return set_err(PTL_ERR_ARG, "ptl_place_match_all: queries [%lld, %lld] of %lld entries", (long long)q_first, (long long)q_last, (long long)p->n_entries);
    ptl_place_result res = {};
    res.best_query = -1; res.best_entry = -1;
    if (!empty) {
        HIPCHK(hipSetDevice(p->device_id));
        hipStream_t s = p->stream;
        const int S = p->cfg.n_sector, RD = p->RD;
        const int64_t n = q_last - q_first + 1;
        const int gap = (int)(min_gap < PLACE_MAX_CAPACITY ? min_gap : PLACE_MAX_CAPACITY);  // (beyond the capacity no entry qualifies either)
        const int blocks = (int)((n + PLACE_THREADS / 64 - 1) / (PLACE_THREADS / 64));
        const size_t lds = (size_t)(PLACE_THREADS / 64) * 2 * S * (RD | 1) * 4;
        const unsigned* desc = (const unsigned*)p->d_desc;
        unsigned long long* d_best = p->d_counts + PLACE_COUNTERS;
        unsigned long long best = PLACE_KEY_NONE;
        HIPCHK(hipEventRecord(p->e0, s));
        HIPCHK(hipMemsetAsync(d_best, 0xff, 8, s));
        if (RD == 5) k_place_match_all<5><<<blocks, PLACE_THREADS, lds, s>>>(desc, S, RD, (int)q_first, (int)q_last, gap, p->d_entry, p->d_dist, p->d_shift, d_best);
        else k_place_match_all<0><<<blocks, PLACE_THREADS, lds, s>>>(desc, S, RD, (int)q_first, (int)q_last, gap, p->d_entry, p->d_dist, p->d_shift, d_best);
        HIPCHK(hipEventRecord(p->e1, s));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, s));
        if (entry_out) HIPCHK(hipMemcpyAsync(entry_out, p->d_entry, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, p->d_dist, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (shift_out) HIPCHK(hipMemcpyAsync(shift_out, p->d_shift, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        { int rc = place_clock(p, &res.device_ms); if (rc) return rc; }
        for (int64_t i = q_first; i <= q_last; ++i) res.n_compared += i - min_gap >= 0 ? i - min_gap + 1 : 0;
        if (best != PLACE_KEY_NONE) {
            const int64_t qi = (int64_t)(best & 0xfffffu);
            int32_t sh = 0;
            HIPCHK(hipMemcpy(&sh, p->d_shift + qi, 4, hipMemcpyDeviceToHost));
            res.best_query = q_first + qi; res.best_entry = (int64_t)((best >> 20) & 0xfffffu); res.best_dist = (uint32_t)(best >> 40); res.best_shift = sh;
        }
    }
    if (result) *result = res;
    return PTL_OK;
}
extern "C" int ptl_place_read(ptl_place* p, int64_t first, int64_t last, uint8_t* desc_out, ptl_place_info* info_out) {
    if (!p) return set_err(PTL_ERR_ARG, "ptl_place_read: null argument");
    if (last < first) return PTL_OK;
    if (first < 0 || last >= p->n_entries) return set_err(PTL_ERR_ARG, "ptl_place_read: entries [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)p->n_entries);
    HIPCHK(hipSetDevice(p->device_id));
    const size_t n = (size_t)(last - first + 1);
    if (desc_out) HIPCHK(hipMemcpy(desc_out, p->d_desc + (size_t)first * p->entry_bytes, n * p->entry_bytes, hipMemcpyDeviceToHost));
    if (info_out) HIPCHK(hipMemcpy(info_out, p->d_info + first, n * sizeof(ptl_place_info), hipMemcpyDeviceToHost));
    return PTL_OK;
}
extern "C" int ptl_place_load(ptl_place* p, int64_t n, const uint8_t* desc, const ptl_place_info* info) {
    if (!p || n < 0 || (n > 0 && (!desc || !info))) return set_err(PTL_ERR_ARG, "ptl_place_load: null argument or n = %lld below zero", (long long)n);
    if (p->n_entries + n > (int64_t)p->cfg.capacity)
        return set_err(PTL_ERR_CAPACITY, "ptl_place_load: %lld entries + %lld to load are above the capacity of %d: nothing was appended", (long long)p->n_entries,
                       (long long)n, p->cfg.capacity);
    const int R = p->cfg.n_ring, S = p->cfg.n_sector;
    for (int64_t k = 0; k < n && R < p->Rpad; ++k)
        for (int j = 0; j < S; ++j)
            for (int r = R; r < p->Rpad; ++r)
                if (desc[(size_t)k * p->entry_bytes + (size_t)j * p->Rpad + r])
                    return set_err(PTL_ERR_ARG, "ptl_place_load: entry %lld, sector %d, byte %d = %u: a pad byte (ring >= %d) must be 0; nothing was appended",
                                   (long long)k, j, r, (unsigned)desc[(size_t)k * p->entry_bytes + (size_t)j * p->Rpad + r], R);
    if (n == 0) return PTL_OK;
    HIPCHK(hipSetDevice(p->device_id));
    HIPCHK(hipMemcpy(p->d_desc + (size_t)p->n_entries * p->entry_bytes, desc, (size_t)n * p->entry_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_info + p->n_entries, info, (size_t)n * sizeof(ptl_place_info), hipMemcpyHostToDevice));
    p->n_entries += n;
    return PTL_OK;
}

// ================================================================================================ occupancy grid
// The definition is in include/ptudes_mi.h, the kernels in grid_kernels.h.  Everything is checked on the host before the first HIP call.  The
// grid handle owns what its passes need - stream, events, column table, sweep staging, both count arrays, counters - and knows no map.
struct ptl_grid {
    int device_id = 0;             // (first member, as in ptl_traj)
    uint64_t n_rays_used = 0;      // used rays so far, the host's copy after the last add (second member: a test reaches it as it reaches device_id)
    ptl_grid_cfg cfg;
    int64_t n_cells = 0;
    double device_ms = 0;
    Stream stream;
    Event e0, e1;
    double* coltab = nullptr;      // [12][W]
    double* d_ts = nullptr;        // [W]
    void* d_raw = nullptr;         // one sweep of the caller's: max_pixels_per_scan pixels of f32 xyz or u32 ranges
    FlyWs* d_fly = nullptr;        // k_fly_coltab's flag
    unsigned *d_free = nullptr, *d_hit = nullptr;  // [ny][nx]
    unsigned long long* d_counts = nullptr;        // [GRID_COUNTERS] + GRID_SUMS of the read's reduction
    int* d_box = nullptr;          // [4] of the read's reduction
    unsigned long long counts[GRID_COUNTERS] = {};  // the host's copy after the last add
    DevOwner mem;
};
#define GRID_MAX_RAYS 0xffffffffull
#define GRID_MAX_PIXELS ((int64_t)1 << 24)
extern "C" int64_t ptl_grid_sizeof_cfg(void) { return (int64_t)sizeof(ptl_grid_cfg); }
extern "C" int64_t ptl_grid_sizeof_result(void) { return (int64_t)sizeof(ptl_grid_result); }
extern "C" int ptl_grid_default_cfg(ptl_grid_cfg* cfg, double cell) {
    if (!cfg) return set_err(PTL_ERR_ARG, "ptl_grid_default_cfg: cfg is null");
    ABI_CHECK(ptl_grid_cfg, cfg);
    if (!(cell > 0.0) || !(cell < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_grid_default_cfg: cell must be positive and finite (got %g)", cell);
    PTL_CFG_INIT(cfg);
    cfg->cell = cell; cfg->step = cell / 2.0; cfg->margin = cell; cfg->min_range = 0.0; cfg->max_range = 600.0 * cell;
    cfg->z_lo = -0.5; cfg->z_hi = 0.5;
    return PTL_OK;
}
static int grid_clock(ptl_grid* h) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    h->device_ms += ms;
    return PTL_OK;
}
static int grid_zero(ptl_grid* h) {
    hipStream_t s = h->stream;
    HIPCHK(hipMemsetAsync(h->d_fly, 0, sizeof(FlyWs), s));
    HIPCHK(hipMemsetAsync(h->d_free, 0, (size_t)h->n_cells * 4, s));
    HIPCHK(hipMemsetAsync(h->d_hit, 0, (size_t)h->n_cells * 4, s));
    HIPCHK(hipMemsetAsync(h->d_counts, 0, ((size_t)GRID_COUNTERS + GRID_SUMS) * 8, s));
    HIPCHK(hipStreamSynchronize(s));
    memset(h->counts, 0, sizeof h->counts);
    h->n_rays_used = 0;
    return PTL_OK;
}
extern "C" int ptl_grid_create(int32_t device_id, const ptl_grid_cfg* cfg, ptl_grid** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "ptl_grid_create: null argument");
    ABI_CHECK(ptl_grid_cfg, cfg);
    const ptl_grid_cfg& u = *cfg;
    if (!(u.cell > 0.0) || !(u.cell < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_grid_create: cell = %g: must be positive and finite", u.cell);
    if (!(fabs(u.x0) < 1.0e150) || !(fabs(u.y0) < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_grid_create: origin (x0, y0) = (%g, %g): must be finite", u.x0, u.y0);
    if (u.nx < 1 || u.ny < 1) return set_err(PTL_ERR_ARG, "ptl_grid_create: nx x ny = %d x %d: both must be >= 1", u.nx, u.ny);
    if ((int64_t)u.nx * u.ny > (int64_t)GRID_MAX_CELLS)
        return set_err(PTL_ERR_ARG, "ptl_grid_create: nx x ny = %d x %d = %lld cells: the limit is %d (2^26)", u.nx, u.ny, (long long)((int64_t)u.nx * u.ny), GRID_MAX_CELLS);
    if (!(u.z_lo <= u.z_hi)) return set_err(PTL_ERR_ARG, "ptl_grid_create: band [z_lo, z_hi] = [%g, %g]: z_lo must not be above z_hi", u.z_lo, u.z_hi);
    if (!(u.margin >= 0.0) || !(u.margin < 1.0e150)) return set_err(PTL_ERR_ARG, "ptl_grid_create: margin = %g: must be >= 0 and finite", u.margin);
    if (!(u.step > 0.0) || !(u.step <= u.cell)) return set_err(PTL_ERR_ARG, "ptl_grid_create: step = %g: the march needs 0 < step <= cell = %g", u.step, u.cell);
    if (!(u.min_range >= 0.0)) return set_err(PTL_ERR_ARG, "ptl_grid_create: min_range = %g: must be >= 0", u.min_range);
    if (!(u.max_range > u.min_range)) return set_err(PTL_ERR_ARG, "ptl_grid_create: max_range = %g: must be above min_range = %g", u.max_range, u.min_range);
    if (!(u.max_range / u.step <= (double)GRID_MAX_SAMPLES))
        return set_err(PTL_ERR_ARG, "ptl_grid_create: max_range / step = %g / %g = %g samples per ray: the limit is %d", u.max_range, u.step,
                       u.max_range / u.step, GRID_MAX_SAMPLES);
    if (u.scan_cols < 1) return set_err(PTL_ERR_ARG, "ptl_grid_create: scan_cols = %d: must be >= 1", u.scan_cols);
    if (u.max_pixels_per_scan < u.scan_cols || u.max_pixels_per_scan > GRID_MAX_PIXELS)
        return set_err(PTL_ERR_ARG, "ptl_grid_create: max_pixels_per_scan = %lld: must be in scan_cols = %d .. %lld", (long long)u.max_pixels_per_scan, u.scan_cols,
                       (long long)GRID_MAX_PIXELS);
    if (device_id < 0) return set_err(PTL_ERR_ARG, "ptl_grid_create: device_id = %d: must not be negative", device_id);
    if (ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_grid> h(new ptl_grid());
    h->device_id = device_id; h->cfg = u; h->n_cells = (int64_t)u.nx * u.ny;
    HIPCHK(h->stream.create());
    HIPCHK(h->e0.create(hipEventDefault)); HIPCHK(h->e1.create(hipEventDefault));
    h->mem.add(&h->coltab, (size_t)12 * u.scan_cols); h->mem.add(&h->d_ts, (size_t)u.scan_cols);
    { unsigned char* raw = nullptr; h->mem.add(&raw, (size_t)u.max_pixels_per_scan * 12); h->d_raw = raw; }
    h->mem.add(&h->d_fly, 1);
    h->mem.add(&h->d_free, (size_t)h->n_cells); h->mem.add(&h->d_hit, (size_t)h->n_cells);
    h->mem.add(&h->d_counts, (size_t)GRID_COUNTERS + GRID_SUMS); h->mem.add(&h->d_box, 4);
    HIPCHK(h->mem.err);
    { int rc = grid_zero(h.get()); if (rc) return rc; }
    *out = h.release();
    return PTL_OK;
}
extern "C" int ptl_grid_destroy(ptl_grid* g) { return g ? handle_destroy(g, g->device_id) : PTL_OK; }
extern "C" int ptl_grid_clear(ptl_grid* g) {
    if (!g) return set_err(PTL_ERR_ARG, "ptl_grid_clear: null argument");
    HIPCHK(hipSetDevice(g->device_id));
    return grid_zero(g);
}
// what every add checks before any HIP call; pixels = every pixel the add could turn into a used ray
static int grid_check(ptl_grid* h, const ptl_traj* t, const ptl_lut* lut, int64_t H, int64_t W, int64_t sweeps, bool staged, const char* who) {
    if (t->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: trajectory on device %d, grid on device %d", who, t->device_id, h->device_id);
    if (lut && lut->device_id != h->device_id) return set_err(PTL_ERR_ARG, "%s: LUT on device %d, grid on device %d", who, lut->device_id, h->device_id);
    if (H < 1 || W < 1) return set_err(PTL_ERR_ARG, "%s: empty scan (%lld x %lld)", who, (long long)H, (long long)W);
    if (W != h->cfg.scan_cols) return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld columns, the grid handle's scan_cols is %d", who, (long long)W, h->cfg.scan_cols);
    if (H * W > (staged ? h->cfg.max_pixels_per_scan : (int64_t)0x7fffffff))
        return set_err(PTL_ERR_CAPACITY, "%s: the scan has %lld pixels, the grid handle's max_pixels_per_scan is %lld", who, (long long)(H * W),
                       (long long)h->cfg.max_pixels_per_scan);
    const uint64_t pixels = (uint64_t)(H * W) * (uint64_t)sweeps;
    if (h->n_rays_used + pixels > GRID_MAX_RAYS)
        return set_err(PTL_ERR_CAPACITY, "%s: %llu used rays so far + %llu pixels could pass %llu (2^32 - 1), the range of the u32 counts: read the grid and "
                       "ptl_grid_clear it, or use another handle", who, (unsigned long long)h->n_rays_used, (unsigned long long)pixels, (unsigned long long)GRID_MAX_RAYS);
    return PTL_OK;
}
// one sweep enqueued on the grid handle's stream; raw (device): the sweep; d_col_ts (device, W) or the sweep's (t0, t1)
static int grid_enqueue(ptl_grid* h, const ptl_traj* t, const void* raw, bool is_range, const ptl_lut* lut, int H, int W, const double* d_col_ts,
                        double t0, double t1) {
    hipStream_t s = h->stream;
    const int n = H * W;
    const ptl_grid_cfg& u = h->cfg;
    GridArgs a = {};
    a.cell = u.cell; a.x0 = u.x0; a.y0 = u.y0; a.z_lo = u.z_lo; a.z_hi = u.z_hi; a.margin = u.margin; a.step = u.step;
    a.min_range = u.min_range; a.max_range = u.max_range; a.nx = u.nx; a.ny = u.ny;
    a.free = h->d_free; a.hit = h->d_hit; a.counts = h->d_counts;
    const int wg = (n + GRID_THREADS - 1) / GRID_THREADS, grid = wg < GRID_MAX_BLOCKS ? wg : GRID_MAX_BLOCKS;
    k_fly_coltab<<<1, 256, 0, s>>>(t->d_kt, t->d_kp, t->n, t->before, t->after, d_col_ts, t0, t1, W, h->coltab, h->d_fly);
    if (is_range) k_grid_rays<true><<<grid, GRID_THREADS, 0, s>>>(raw, lut->dir, lut->off, n, W, h->coltab, h->d_fly, a);
    else k_grid_rays<false><<<grid, GRID_THREADS, 0, s>>>(raw, nullptr, nullptr, n, W, h->coltab, h->d_fly, a);
    HIPCHK(hipGetLastError());
    return PTL_OK;
}
// closes an add: the counters come back, the host's copy moves on; the deltas are the call's
static int grid_finish(ptl_grid* h, int64_t* n_valid, int64_t* n_skipped) {
    unsigned long long now[GRID_COUNTERS];
    HIPCHK(hipEventRecord(h->e1, h->stream));
    HIPCHK(hipMemcpyAsync(now, h->d_counts, sizeof now, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    { int rc = grid_clock(h); if (rc) return rc; }
    if (n_valid) *n_valid = (int64_t)(now[GRID_N_RAYS] - h->counts[GRID_N_RAYS]);
    if (n_skipped) *n_skipped = (int64_t)(now[GRID_N_SKIPPED] - h->counts[GRID_N_SKIPPED]);
    memcpy(h->counts, now, sizeof now);
    h->n_rays_used = now[GRID_N_RAYS];
    return PTL_OK;
}
static int grid_add_percall(ptl_grid* h, ptl_traj* t, ptl_lut* lut, const void* raw_host, size_t raw_bytes, bool is_range, int64_t H, int64_t W,
                            const double* col_ts, int64_t* n_valid, int32_t* skipped, const char* who) {
    int rc = grid_check(h, t, lut, H, W, 1, true, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device_id));
    HIPCHK(hipEventRecord(h->e0, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_raw, raw_host, raw_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ts, col_ts, (size_t)W * 8, hipMemcpyHostToDevice, h->stream));
    rc = grid_enqueue(h, t, h->d_raw, is_range, lut, (int)H, (int)W, h->d_ts, 0.0, 0.0);
    if (rc) return rc;
    int64_t sk = 0;
    rc = grid_finish(h, n_valid, &sk);
    if (skipped) *skipped = sk ? 1 : 0;
    return rc;
}
extern "C" int ptl_grid_add_posed_range(ptl_grid* g, ptl_traj* t, ptl_lut* lut, const uint32_t* range_mm, const double* col_ts, int64_t* n_valid,
                                        int32_t* skipped) {
    if (!g || !t || !lut || !range_mm || !col_ts) return set_err(PTL_ERR_ARG, "ptl_grid_add_posed_range: null argument");
    return grid_add_percall(g, t, lut, range_mm, (size_t)lut->H * lut->W * 4, true, lut->H, lut->W, col_ts, n_valid, skipped, "ptl_grid_add_posed_range");
}
extern "C" int ptl_grid_add_posed_xyz(ptl_grid* g, ptl_traj* t, const float* xyz, int32_t H, int32_t W, const double* col_ts, int64_t* n_valid,
                                      int32_t* skipped) {
    if (!g || !t || !xyz || !col_ts) return set_err(PTL_ERR_ARG, "ptl_grid_add_posed_xyz: null argument");
    return grid_add_percall(g, t, nullptr, xyz, (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * 12, false, H, W, col_ts, n_valid, skipped, "ptl_grid_add_posed_xyz");
}
// resident form, as carve_build: sweeps [first, last] of a lane, `slot` bytes apart.  The caller has checked the runner's side; the lane is
// only read.  `wait_a`, `wait_b`: the runner's streams, waited for after the checks and before the first launch
static int grid_build(ptl_grid* h, ptl_traj* t, const SeqLane& l, size_t slot, const unsigned char* is_range_k, bool all_range, const ptl_lut* lut,
                      int64_t pps, const double* t0t1, int64_t first, int64_t last, hipStream_t wait_a, hipStream_t wait_b, int64_t* n_valid,
                      int64_t* n_skipped, const char* who) {
    const int64_t W = h->cfg.scan_cols;
    if (pps % W) return set_err(PTL_ERR_CAPACITY, "%s: %lld points per sweep are no multiple of the grid handle's scan_cols = %lld", who, (long long)pps, (long long)W);
    if (l.icp->c.W != W) return set_err(PTL_ERR_CAPACITY, "%s: the runner's scan_cols is %d, the grid handle's %lld", who, l.icp->c.W, (long long)W);
    int rc = grid_check(h, t, lut, pps / W, W, last - first + 1, false, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device_id));
    HIPCHK(hipStreamSynchronize(wait_a));  // the runner's own work first; its sweeps are then only read
    HIPCHK(hipStreamSynchronize(wait_b));
    HIPCHK(hipEventRecord(h->e0, h->stream));
    for (int64_t k = first; k <= last; ++k) {
        const bool rg = all_range || (is_range_k && is_range_k[(size_t)k]);
        rc = grid_enqueue(h, t, (const char*)l.d_scans + (size_t)k * slot, rg, lut, (int)(pps / W), (int)W, nullptr, t0t1[2 * k], t0t1[2 * k + 1]);
        if (rc) return rc;
    }
    return grid_finish(h, n_valid, n_skipped);
}
extern "C" int ptl_grid_add_seq(ptl_grid* g, ptl_seq* s, ptl_traj* t, const double* t0t1, int64_t first, int64_t last, int64_t* n_valid,
                                int64_t* n_skipped) {
    if (!g || !s || !t || !t0t1) return set_err(PTL_ERR_ARG, "ptl_grid_add_seq: null argument");
    if (first < 0 || last < first || last >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_grid_add_seq: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)s->cfg.n_scans);
    if (s->cfg.icp.device_id != g->device_id) return set_err(PTL_ERR_ARG, "ptl_grid_add_seq: runner on device %d, grid on device %d", s->cfg.icp.device_id, g->device_id);
    bool any_range = false;
    for (int64_t k = first; k <= last; ++k) any_range = any_range || s->is_range[(size_t)k];
    if (any_range && !s->lut) return set_err(PTL_ERR_STATE, "ptl_grid_add_seq: the sweeps are range images but no LUT was set (ptl_seq_set_lut)");
    return grid_build(g, t, s->lane, (size_t)s->cfg.points_per_scan * 12, s->is_range.data(), false, any_range ? s->lut : nullptr, s->cfg.points_per_scan,
                      t0t1, first, last, s->stream, s->ekf_stream, n_valid, n_skipped, "ptl_grid_add_seq");
}
extern "C" int ptl_grid_add_batch(ptl_grid* g, ptl_batch* b, int32_t seq, ptl_traj* t, const double* t0t1, int64_t first, int64_t last,
                                  int64_t* n_valid, int64_t* n_skipped) {
    if (!g || !b || !t || !t0t1) return set_err(PTL_ERR_ARG, "ptl_grid_add_batch: null argument");
    if (seq < 0 || seq >= b->S) return set_err(PTL_ERR_ARG, "ptl_grid_add_batch: sequence %d of %d", seq, b->S);
    if (first < 0 || last < first || last >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "ptl_grid_add_batch: sweeps [%lld, %lld] of %lld", (long long)first, (long long)last, (long long)b->cfg.n_scans);
    if (b->cfg.icp.device_id != g->device_id) return set_err(PTL_ERR_ARG, "ptl_grid_add_batch: batch on device %d, grid on device %d", b->cfg.icp.device_id, g->device_id);
    if (b->ring < b->cfg.n_scans) return set_err(PTL_ERR_STATE, "ptl_grid_add_batch: the batch keeps a ring of %lld sweep slots (resident_scans): earlier sweeps are gone", (long long)b->ring);
    if (b->cfg.range_input && !b->lut) return set_err(PTL_ERR_STATE, "ptl_grid_add_batch: a range-input batch needs its LUT (ptl_batch_set_lut)");
    const size_t slot = (size_t)b->cfg.points_per_scan * (b->cfg.range_input ? 4 : 12);
    return grid_build(g, t, b->lane[seq], slot, nullptr, b->is_range != 0, b->is_range ? b->lut : nullptr, b->cfg.points_per_scan, t0t1, first, last,
                      b->stream, b->side, n_valid, n_skipped, "ptl_grid_add_batch");
}
extern "C" int ptl_grid_read(ptl_grid* h, ptl_grid_result* result, int32_t ix0, int32_t iy0, int32_t w, int32_t hh, uint32_t* free_out, uint32_t* hit_out) {
    if (!h || !result) return set_err(PTL_ERR_ARG, "ptl_grid_read: null argument");
    ABI_CHECK(ptl_grid_result, result);
    const int given = (free_out != nullptr) + (hit_out != nullptr);
    if (given == 1) return set_err(PTL_ERR_ARG, "ptl_grid_read: the two arrays (free, hit) are given together or not at all (1 given)");
    const ptl_grid_cfg& u = h->cfg;
    if (given && (w < 1 || hh < 1 || ix0 < 0 || iy0 < 0 || (int64_t)ix0 + w > u.nx || (int64_t)iy0 + hh > u.ny))
        return set_err(PTL_ERR_ARG, "ptl_grid_read: the rectangle of %d x %d cells at (%d, %d) is empty or not inside the grid of %d x %d", w, hh, ix0, iy0, u.nx, u.ny);
    HIPCHK(hipSetDevice(h->device_id));
    hipStream_t s = h->stream;
    unsigned long long sums[GRID_SUMS] = {0, 0, 0, 0};
    int box[4] = {0x7fffffff, 0x7fffffff, -1, -1};
    const int64_t wg = (h->n_cells + 255) / 256;
    HIPCHK(hipEventRecord(h->e0, s));
    HIPCHK(hipMemsetAsync(h->d_counts + GRID_COUNTERS, 0, (size_t)GRID_SUMS * 8, s));
    HIPCHK(hipMemcpyAsync(h->d_box, box, sizeof box, hipMemcpyHostToDevice, s));
    k_grid_reduce<<<(int)(wg < 1024 ? wg : 1024), 256, 0, s>>>(h->d_free, h->d_hit, u.nx, (int)h->n_cells, h->d_counts + GRID_COUNTERS, h->d_box);
    HIPCHK(hipEventRecord(h->e1, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, h->d_counts + GRID_COUNTERS, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(box, h->d_box, sizeof box, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    { int rc = grid_clock(h); if (rc) return rc; }
    const uint32_t size = result->struct_size, abi = result->abi_version;
    memset(result, 0, sizeof *result);
    result->struct_size = size; result->abi_version = abi;
    result->n_scans = (int64_t)h->counts[GRID_N_SCANS]; result->n_scans_skipped = (int64_t)h->counts[GRID_N_SKIPPED];
    result->n_rays = (int64_t)h->counts[GRID_N_RAYS]; result->n_rays_out_of_range = (int64_t)h->counts[GRID_N_OOR];
    result->n_no_return = (int64_t)h->counts[GRID_N_NORET]; result->n_runs_voted = (int64_t)h->counts[GRID_N_RUNS];
    result->n_ends_outside = (int64_t)h->counts[GRID_N_ENDS_OUT];
    result->n_cells_free = (int64_t)sums[0]; result->n_cells_hit = (int64_t)sums[1];
    result->sum_free = (int64_t)sums[2]; result->sum_hit = (int64_t)sums[3];
    const bool empty = box[2] < 0;
    result->box_ix0 = empty ? 0 : box[0]; result->box_iy0 = empty ? 0 : box[1]; result->box_ix1 = box[2]; result->box_iy1 = box[3];
    result->cell = u.cell; result->x0 = u.x0; result->y0 = u.y0; result->z_lo = u.z_lo; result->z_hi = u.z_hi; result->margin = u.margin;
    result->step = u.step; result->min_range = u.min_range; result->max_range = u.max_range; result->nx = u.nx; result->ny = u.ny;
    result->device_ms = h->device_ms;
    if (given) {
        const size_t at = (size_t)iy0 * u.nx + ix0;
        HIPCHK(hipMemcpy2D(free_out, (size_t)w * 4, h->d_free + at, (size_t)u.nx * 4, (size_t)w * 4, (size_t)hh, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy2D(hit_out, (size_t)w * 4, h->d_hit + at, (size_t)u.nx * 4, (size_t)w * 4, (size_t)hh, hipMemcpyDeviceToHost));
    }
    return PTL_OK;
}

// ================================================================================================ fly-by frames
// The definition is in include/ptudes_mi.h, the kernels in render_kernels.h.  Everything is checked on the host before the first HIP call.  The
// renderer owns what one launch needs: the keys and the resolved outputs of max_frames_per_call frames, their cameras and counters.
static_assert(sizeof(RenderCam) == sizeof(ptl_render_cam), "the device's camera is the header's");
struct ptl_render {
    ptl_render_cfg cfg;
    int device_id = 0;
    bool early_reject = true;
    Stream stream;
    unsigned* d_palette = nullptr;            // [256]
    RenderCam* d_cams = nullptr;              // [max_frames_per_call]
    unsigned long long* d_keys = nullptr;     // [max_frames_per_call][height][width]
    unsigned* d_rgba = nullptr;               // the same
    float* d_depth = nullptr;                 // the same
    unsigned long long* d_in_view = nullptr;  // [max_frames_per_call]
    double* d_ov_xyz = nullptr;               // the overlay: [ov_n][3]
    unsigned* d_ov_rgba = nullptr;            // [ov_n]
    int64_t ov_n = 0;
    int ov_px = 1;
    ptl_icp* col_map = nullptr;               // the map handle whose stored points carry colours of their own (ptl_render_set_point_colors)
    int64_t col_n = 0;                        // its point count when they were set
    unsigned* d_col_rgba = nullptr;           // [col_n], pool order
    int* d_col_off = nullptr;                 // [pool_cap of col_map] exclusive prefix of the stored points per block id
    DevOwner mem;
};
static void render_defaults(ptl_render_cfg* cfg, int32_t width, int32_t height) {
    PTL_CFG_INIT(cfg);
    cfg->width = width; cfg->height = height;
    cfg->point_px = 2;
    cfg->max_frames_per_call = 16;
    cfg->z_lo = -2.0; cfg->z_hi = 10.0;
    cfg->background_rgba = 0xFF000000u;
    cfg->edl_strength = 0.0;
    cfg->edl_radius_px = 1;
}
static int render_check_cfg(const ptl_render_cfg* c) {
    if (c->width < 1 || c->width > 16384 || c->height < 1 || c->height > 16384)
        return set_err(PTL_ERR_ARG, "frame of %d x %d pixels: width and height must be in [1, 16384]", c->width, c->height);
    if (c->point_px < 1 || c->point_px > RENDER_MAX_PX) return set_err(PTL_ERR_ARG, "point_px = %d: must be in [1, %d]", c->point_px, RENDER_MAX_PX);
    if (c->max_frames_per_call < 1) return set_err(PTL_ERR_ARG, "max_frames_per_call = %d: must be >= 1", c->max_frames_per_call);
    if (!(c->z_hi > c->z_lo) || !(c->z_hi - c->z_lo < 1.0e300))
        return set_err(PTL_ERR_ARG, "z_lo = %g, z_hi = %g: the palette needs finite z_hi > z_lo", c->z_lo, c->z_hi);
    if (!(c->edl_strength >= 0.0) || !(c->edl_strength < 1.0e300)) return set_err(PTL_ERR_ARG, "edl_strength = %g: must be >= 0 and finite", c->edl_strength);
    if (c->edl_radius_px < 1) return set_err(PTL_ERR_ARG, "edl_radius_px = %d: must be >= 1", c->edl_radius_px);
    const long long key_bytes = (long long)c->width * c->height * 8 * (long long)c->max_frames_per_call;
    if (key_bytes > PTL_RENDER_MAX_KEY_BYTES)
        return set_err(PTL_ERR_ARG, "%d frames of %d x %d pixels per launch need a key buffer of %lld bytes; the bound is %lld",
                       c->max_frames_per_call, c->width, c->height, key_bytes, (long long)PTL_RENDER_MAX_KEY_BYTES);
    return PTL_OK;
}
extern "C" int64_t ptl_render_sizeof_cfg(void) { return (int64_t)sizeof(ptl_render_cfg); }
extern "C" int ptl_render_default_cfg(ptl_render_cfg* cfg, int32_t width, int32_t height) {
    if (!cfg) return set_err(PTL_ERR_ARG, "cfg is null");
    ABI_CHECK(ptl_render_cfg, cfg);
    if (width < 1 || width > 16384 || height < 1 || height > 16384)
        return set_err(PTL_ERR_ARG, "frame of %d x %d pixels: width and height must be in [1, 16384]", width, height);
    render_defaults(cfg, width, height);
    return PTL_OK;
}
extern "C" int ptl_render_destroy(ptl_render* r) { return r ? handle_destroy(r, r->device_id) : PTL_OK; }
extern "C" int ptl_render_create(const ptl_render_cfg* cfg, int32_t device_id, ptl_render** out) {
    if (!cfg || !out) return set_err(PTL_ERR_ARG, "null argument");
    ABI_CHECK(ptl_render_cfg, cfg);
    int rc = render_check_cfg(cfg);
    if (rc) return rc;
    if (device_id < 0 || ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_render> r(new ptl_render());
    r->cfg = *cfg; r->device_id = device_id;
    if (r->stream.create() != hipSuccess) return set_err(PTL_ERR_HIP, "stream creation failed");
    DevOwner& m = r->mem;
    const size_t F = (size_t)cfg->max_frames_per_call, px = (size_t)cfg->width * (size_t)cfg->height;
    m.add(&r->d_palette, 256); m.add(&r->d_cams, F); m.add(&r->d_keys, F * px); m.add(&r->d_rgba, F * px); m.add(&r->d_depth, F * px);
    m.add(&r->d_in_view, F);
    if (m.err != hipSuccess) return set_err(PTL_ERR_HIP, "ptl_render_create: %s (%zu bytes)", hipGetErrorString(m.err), m.requested());
    uint32_t ramp[256];
    for (int i = 0; i < 256; ++i) {
        const int tri = 2 * i - 255;
        ramp[i] = (uint32_t)i | (uint32_t)(255 - (tri < 0 ? -tri : tri)) << 8 | (uint32_t)(255 - i) << 16 | 0xFF000000u;
    }
    HIPCHK(hipMemcpy(r->d_palette, ramp, sizeof ramp, hipMemcpyHostToDevice));
    *out = r.release();
    return PTL_OK;
}
extern "C" int ptl_render_set_palette(ptl_render* r, const uint32_t rgba[256]) {
    if (!r || !rgba) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(r->device_id));
    HIPCHK(hipStreamSynchronize(r->stream));
    HIPCHK(hipMemcpy(r->d_palette, rgba, 256 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return PTL_OK;
}
extern "C" int ptl_render_set_z_range(ptl_render* r, double z_lo, double z_hi) {
    if (!(z_hi > z_lo) || !(z_hi - z_lo < 1.0e300)) return set_err(PTL_ERR_ARG, "z_lo = %g, z_hi = %g: the palette needs finite z_hi > z_lo", z_lo, z_hi);
    if (!r) return set_err(PTL_ERR_ARG, "null argument");
    r->cfg.z_lo = z_lo; r->cfg.z_hi = z_hi;
    return PTL_OK;
}
extern "C" int ptl_render_set_overlay(ptl_render* r, const double* xyz, const uint32_t* rgba, int64_t n, int32_t point_px) {
    if (n < 0 || n > 0x7fffffffLL) return set_err(PTL_ERR_ARG, "ptl_render_set_overlay: n = %lld (0 .. 2^31 - 1)", (long long)n);
    if (n > 0 && (point_px < 1 || point_px > RENDER_MAX_PX)) return set_err(PTL_ERR_ARG, "ptl_render_set_overlay: point_px = %d: must be in [1, %d]", point_px, RENDER_MAX_PX);
    if (!r || (n > 0 && (!xyz || !rgba))) return set_err(PTL_ERR_ARG, "ptl_render_set_overlay: null argument");
    HIPCHK(hipSetDevice(r->device_id));
    HIPCHK(hipStreamSynchronize(r->stream));
    r->mem.release(&r->d_ov_xyz);
    r->mem.release(&r->d_ov_rgba);
    r->ov_n = 0;
    if (n == 0) return PTL_OK;
    HIPCHK(r->mem.alloc(&r->d_ov_xyz, (size_t)n * 3));
    HIPCHK(r->mem.alloc(&r->d_ov_rgba, (size_t)n));
    HIPCHK(hipMemcpy(r->d_ov_xyz, xyz, (size_t)n * 24, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(r->d_ov_rgba, rgba, (size_t)n * 4, hipMemcpyHostToDevice));
    r->ov_n = n; r->ov_px = point_px;
    return PTL_OK;
}
// colours per stored point of one map handle: the words, the renderer's own per-block prefix of that map, and the count
extern "C" int ptl_render_set_point_colors(ptl_render* r, ptl_icp* map, const uint32_t* rgba, int64_t n) {
    if (!r) return set_err(PTL_ERR_ARG, "ptl_render_set_point_colors: null renderer");
    if (n < 0 || n > 0x7fffffffLL) return set_err(PTL_ERR_ARG, "ptl_render_set_point_colors: n = %lld (0 .. 2^31 - 1)", (long long)n);
    const bool clear = !rgba || n == 0;
    if (!clear && !map) return set_err(PTL_ERR_ARG, "ptl_render_set_point_colors: %lld colours without a map", (long long)n);
    if (!clear && map->cfg.device_id != r->device_id)
        return set_err(PTL_ERR_ARG, "ptl_render_set_point_colors: renderer on device %d, map on device %d", r->device_id, map->cfg.device_id);
    HIPCHK(hipSetDevice(r->device_id));
    HIPCHK(hipStreamSynchronize(r->stream));
    r->mem.release(&r->d_col_rgba);
    r->mem.release(&r->d_col_off);
    r->col_map = nullptr; r->col_n = 0;
    if (clear) return PTL_OK;
    HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, map->stream));
    HIPCHK(hipStreamSynchronize(map->stream));
    if ((int64_t)st.map_points != n)
        return set_err(PTL_ERR_ARG, "ptl_render_set_point_colors: %lld colours for a map of %lld stored points: one word per stored point, in pool order",
                       (long long)n, (long long)st.map_points);
    const Ctx& c = map->c;
    const int n_chunks = (c.pool_cap + SCORE_CHUNK - 1) / SCORE_CHUNK;
    HIPCHK(r->mem.alloc(&r->d_col_rgba, (size_t)n));
    HIPCHK(r->mem.alloc(&r->d_col_off, (size_t)c.pool_cap));
    DevOwner tmp;
    int *d_cnt = nullptr, *d_off = nullptr;
    tmp.add(&d_cnt, (size_t)n_chunks); tmp.add(&d_off, (size_t)n_chunks + 1);
    HIPCHK(tmp.err);
    const hipStream_t s = r->stream;
    k_score_count<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_cnt);
    k_score_scan<<<1, 1024, 0, s>>>(d_cnt, n_chunks, d_off);
    k_carve_blkoff<<<(c.pool_cap + 255) / 256, 256, 0, s>>>(c, d_off, r->d_col_off);
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + n_chunks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(r->d_col_rgba, rgba, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total != (int)n) {
        r->mem.release(&r->d_col_rgba);
        r->mem.release(&r->d_col_off);
        return set_err(PTL_ERR_STATE, "ptl_render_set_point_colors: the block directory holds %d points, the map state %lld", total, (long long)n);
    }
    r->col_map = map; r->col_n = n;
    return PTL_OK;
}
extern "C" int ptl_render_debug_set_early_reject(ptl_render* r, int32_t on) {
    if (!r) return set_err(PTL_ERR_ARG, "null argument");
    r->early_reject = on != 0;
    return PTL_OK;
}
extern "C" int ptl_render_frames(ptl_render* r, ptl_icp* map, const ptl_render_cam* cams, int64_t n_frames, uint32_t* rgba_out, float* depth_out,
                                 uint64_t* keys_out, int64_t* in_view_out, double* device_ms) {
    // (the values first: they are refused with their numbers whatever else is wrong with the call)
    if (n_frames < 0) return set_err(PTL_ERR_ARG, "ptl_render_frames: n_frames = %lld: must not be negative", (long long)n_frames);
    if (n_frames > 0 && !cams) return set_err(PTL_ERR_ARG, "ptl_render_frames: %lld frames without cameras", (long long)n_frames);
    for (int64_t f = 0; f < n_frames; ++f) {
        const ptl_render_cam& c = cams[f];
        if (!(c.near_m > 0.0) || !(c.far_m > c.near_m))
            return set_err(PTL_ERR_ARG, "ptl_render_frames: camera %lld: near_m = %g, far_m = %g (need 0 < near_m < far_m)", (long long)f, c.near_m, c.far_m);
        double s = 0.0;
        for (int k = 0; k < 12; ++k) s += c.view[k] * 0.0;
        s += (c.fx + c.fy + c.cx + c.cy) * 0.0;
        if (!(s == 0.0)) return set_err(PTL_ERR_ARG, "ptl_render_frames: camera %lld has a non-finite entry", (long long)f);
    }
    if (!r) return set_err(PTL_ERR_ARG, "ptl_render_frames: null renderer");
    if (n_frames > 0 && !rgba_out) return set_err(PTL_ERR_ARG, "ptl_render_frames: null rgba_out");
    if (map && map->cfg.device_id != r->device_id)
        return set_err(PTL_ERR_ARG, "ptl_render_frames: renderer on device %d, map on device %d", r->device_id, map->cfg.device_id);
    if (device_ms) *device_ms = 0.0;
    if (n_frames == 0) return PTL_OK;
    HIPCHK(hipSetDevice(r->device_id));
    bool draw_map = false;
    if (map) {
        HIPCHK(hipStreamSynchronize(map->map_stream));  // (a map update may still be under way)
        DevState st;
        HIPCHK(hipMemcpyAsync(&st, map->c.st, sizeof st, hipMemcpyDeviceToHost, map->stream));
        HIPCHK(hipStreamSynchronize(map->stream));
        draw_map = st.map_points > 0;
        if (map == r->col_map && (int64_t)st.map_points != r->col_n)
            return set_err(PTL_ERR_STATE, "ptl_render_frames: the map holds %lld points, it held %lld when its point colours were set "
                           "(ptl_render_set_point_colors): set them again for the map as it is, or clear them", (long long)st.map_points, (long long)r->col_n);
    }
    const bool own_colors = map && map == r->col_map;
    const ptl_render_cfg& cfg = r->cfg;
    const hipStream_t s = r->stream;
    const size_t px = (size_t)cfg.width * (size_t)cfg.height;
    Event e0, e1;
    HIPCHK(e0.create(hipEventDefault)); HIPCHK(e1.create(hipEventDefault));
    RenderArgs a = {};
    a.width = cfg.width; a.height = cfg.height; a.point_px = cfg.point_px;
    a.z_lo = cfg.z_lo; a.zscale = 256.0 / (cfg.z_hi - cfg.z_lo);
    a.cams = r->d_cams; a.palette = r->d_palette; a.keys = r->d_keys; a.in_view = r->d_in_view;
    double ms_total = 0.0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += cfg.max_frames_per_call) {
        const int nf = (int)std::min<int64_t>(cfg.max_frames_per_call, n_frames - f0);
        HIPCHK(hipMemcpyAsync(r->d_cams, cams + f0, (size_t)nf * sizeof(RenderCam), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(e0, s));
        HIPCHK(hipMemsetAsync(r->d_keys, 0xFF, (size_t)nf * px * 8, s));  // (k_render_clear: every key all ones)
        HIPCHK(hipMemsetAsync(r->d_in_view, 0, (size_t)nf * 8, s));
        if (draw_map && own_colors) {
            ColorSrc src = {map->c, r->d_col_off, r->d_col_rgba, (int)r->col_n};
            const int n_chunks = (map->c.pool_cap + 63) / 64, want = (n_chunks + RENDER_THREADS / 64 - 1) / (RENDER_THREADS / 64);
            const dim3 grid((unsigned)std::max(1, std::min(want, RENDER_MAX_BLOCKS)), (unsigned)nf);
            if (r->early_reject) k_render_splat<ColorSrc, true><<<grid, RENDER_THREADS, 0, s>>>(src, a);
            else k_render_splat<ColorSrc, false><<<grid, RENDER_THREADS, 0, s>>>(src, a);
        } else if (draw_map) {
            MapSrc src = {map->c};
            const int n_chunks = (map->c.pool_cap + 63) / 64, want = (n_chunks + RENDER_THREADS / 64 - 1) / (RENDER_THREADS / 64);
            const dim3 grid((unsigned)std::max(1, std::min(want, RENDER_MAX_BLOCKS)), (unsigned)nf);
            if (r->early_reject) k_render_splat<MapSrc, true><<<grid, RENDER_THREADS, 0, s>>>(src, a);
            else k_render_splat<MapSrc, false><<<grid, RENDER_THREADS, 0, s>>>(src, a);
        }
        if (r->ov_n > 0) {
            OverlaySrc src = {r->d_ov_xyz, r->d_ov_rgba, (int)r->ov_n, r->ov_px};
            const int want = (int)((r->ov_n + RENDER_THREADS - 1) / RENDER_THREADS);
            const dim3 grid((unsigned)std::min(want, RENDER_MAX_BLOCKS), (unsigned)nf);
            if (r->early_reject) k_render_splat<OverlaySrc, true><<<grid, RENDER_THREADS, 0, s>>>(src, a);
            else k_render_splat<OverlaySrc, false><<<grid, RENDER_THREADS, 0, s>>>(src, a);
        }
        ResolveArgs ra = {};
        ra.width = cfg.width; ra.height = cfg.height; ra.n_frames = nf; ra.background = cfg.background_rgba;
        ra.edl_strength = cfg.edl_strength; ra.edl_radius = cfg.edl_radius_px;
        ra.keys = r->d_keys; ra.rgba = r->d_rgba; ra.depth = depth_out ? r->d_depth : nullptr;
        k_render_resolve<<<(unsigned)(((size_t)nf * px + RENDER_THREADS - 1) / RENDER_THREADS), RENDER_THREADS, 0, s>>>(ra);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rgba_out + (size_t)f0 * px, r->d_rgba, (size_t)nf * px * 4, hipMemcpyDeviceToHost, s));
        if (depth_out) HIPCHK(hipMemcpyAsync(depth_out + (size_t)f0 * px, r->d_depth, (size_t)nf * px * 4, hipMemcpyDeviceToHost, s));
        if (keys_out) HIPCHK(hipMemcpyAsync(keys_out + (size_t)f0 * px, r->d_keys, (size_t)nf * px * 8, hipMemcpyDeviceToHost, s));
        if (in_view_out) HIPCHK(hipMemcpyAsync(in_view_out + f0, r->d_in_view, (size_t)nf * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        ms_total += ms;
    }
    if (device_ms) *device_ms = ms_total;
    return PTL_OK;
}

// ================================================================================================ lidar packets
// The byte layout of a profile (the table of DESIGN.md 3.16) and the decoder handle: packets are staged once at a 16-byte stride, the
// three passes of packet_kernels.h run on the decoder's stream, and the image goes either to the decoder's own staging (ptl_pktdec_decode)
// or straight into a runner's sweep slot (ptl_*_upload_packets).
static_assert(sizeof(PktSummary) == sizeof(ptl_pkt_summary), "the device's summary record is the header's");
static int pkt_layout(const ptl_pkt_format* f, PktLayout* out) {
    if (!f) return set_err(PTL_ERR_ARG, "null packet format");
    ABI_CHECK(ptl_pkt_format, f);
    PktLayout L = {};
    L.H = f->pixels_per_column; L.W = f->columns_per_frame; L.C = f->columns_per_packet;
    if (L.H < 1 || L.W < 1 || L.C < 1 || L.C > PKT_MAX_COLS || L.H > 4096 || L.W > (1 << 16))
        return set_err(PTL_ERR_ARG, "packet format: H = %d, W = %d, C = %d (need H in [1, 4096], W in [1, 65536], C in [1, %d])", L.H, L.W, L.C, PKT_MAX_COLS);
    int trailer = 0, footer = 32;
    L.pkt_hdr = 32; L.col_hdr = 12; L.pix = 12; L.mask = 0x0007ffffu; L.shift = 0; L.status_off = 10; L.frame_off = 2;
    switch (f->profile) {
        case PTL_PKT_LEGACY:
            L.pkt_hdr = 0; footer = 0; L.col_hdr = 16; trailer = 4; L.mask = 0x000fffffu; L.status_off = 16 + 12 * L.H; L.frame_off = 10;
            break;
        case PTL_PKT_RNG19_RFL8_SIG16_NIR16: break;
        case PTL_PKT_RNG15_RFL8_NIR8: L.pix = 4; L.mask = 0x7fffu; L.shift = 3; break;
        case PTL_PKT_RNG19_RFL8_SIG16_NIR16_DUAL: L.pix = 16; break;
        default: return set_err(PTL_ERR_ARG, "unknown lidar packet profile %d (PTL_PKT_*)", f->profile);
    }
    L.col_stride = L.col_hdr + L.H * L.pix + trailer;
    const int64_t bytes = (int64_t)L.pkt_hdr + (int64_t)L.C * L.col_stride + footer;
    if (bytes > PKT_MAX_BYTES) return set_err(PTL_ERR_ARG, "a packet of %lld bytes is above the %d the decoder stages", (long long)bytes, PKT_MAX_BYTES);
    L.bytes = (int)bytes;
    L.stride = (L.bytes + 15) & ~15;
    *out = L;
    return PTL_OK;
}
extern "C" int64_t ptl_pkt_packet_bytes(const ptl_pkt_format* fmt) {
    PktLayout L;
    const int rc = pkt_layout(fmt, &L);
    return rc ? rc : L.bytes;
}

struct ptl_pktdec {
    int device_id = 0;
    PktLayout L = {};
    int64_t max_packets = 0;
    int max_sweeps = 0;
    Stream stream;
    GnTimer prof;                     // ptl_pktdec_profile: the device time of a call's four launches
    unsigned char* d_pkts = nullptr;  // [max_packets] at L.stride
    int* d_sop = nullptr;             // [max_packets]
    PktOut o = {};                    // owner, first packet, timestamps, status, summaries: [max_sweeps]; o.img: the decoder's own images
    unsigned* d_img = nullptr;        // [max_sweeps][H][W]
    unsigned* d_fimg = nullptr;       // [PKT_MAX_FIELDS][max_sweeps][H][W] field images, made by the first ptl_pktdec_decode_fields
    DevOwner mem;
};
extern "C" int ptl_pktdec_destroy(ptl_pktdec* d) { return d ? handle_destroy(d, d->device_id) : PTL_OK; }
extern "C" int ptl_pktdec_create(const ptl_pkt_format* fmt, int32_t device_id, int64_t max_packets, int32_t max_sweeps, ptl_pktdec** out) {
    if (!fmt || !out) return set_err(PTL_ERR_ARG, "null argument");
    PktLayout L;
    int rc = pkt_layout(fmt, &L);
    if (rc) return rc;
    if (max_packets < 1 || max_packets > (1 << 20) || max_sweeps < 1 || max_sweeps > (1 << 16) || max_packets * L.C > 0x7fffffffLL ||
        (int64_t)max_sweeps * L.W > 0x7fffffffLL)
        return set_err(PTL_ERR_ARG, "ptl_pktdec_create: max_packets = %lld (1 .. 2^20), max_sweeps = %d (1 .. 2^16)", (long long)max_packets, max_sweeps);
    if (device_id < 0 || ptl_device_count() <= device_id) return set_err(PTL_ERR_HIP, "no HIP device %d (the HIP backend is the only backend)", device_id);
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ptl_pktdec> d(new ptl_pktdec());
    d->device_id = device_id; d->L = L; d->max_packets = max_packets; d->max_sweeps = max_sweeps;
    if (d->stream.create() != hipSuccess) return set_err(PTL_ERR_HIP, "stream creation failed");
    DevOwner& m = d->mem;
    const size_t S = (size_t)max_sweeps, W = (size_t)L.W;
    m.add(&d->d_pkts, (size_t)max_packets * L.stride); m.add(&d->d_sop, (size_t)max_packets);
    m.add(&d->d_img, S * L.H * W); m.add(&d->o.ts, S * W); m.add(&d->o.status, S * W); m.add(&d->o.owner, S * W);
    m.add(&d->o.first_pkt, S); m.add(&d->o.sum, S);
    if (m.err != hipSuccess) return set_err(PTL_ERR_HIP, "ptl_pktdec_create: %s (%zu bytes)", hipGetErrorString(m.err), m.requested());
    d->o.img = d->d_img;
    d->o.img_stride = (size_t)L.H * W;
    *out = d.release();
    return PTL_OK;
}
// what both forms check before any HIP call
static int pktdec_check(const ptl_pktdec* d, const void* packets, int64_t stride, int64_t n, const int32_t* sop, int32_t n_sweeps, const char* who) {
    if (!d || !packets) return set_err(PTL_ERR_ARG, "%s: null argument", who);
    if (((uintptr_t)packets & 3) || (stride & 3)) return set_err(PTL_ERR_ARG, "%s: the packet buffer and its stride must be 4-byte aligned", who);
    if (stride < d->L.bytes) return set_err(PTL_ERR_ARG, "%s: stride of %lld bytes, a packet has %d", who, (long long)stride, d->L.bytes);
    if (n < 0 || n > d->max_packets) return set_err(PTL_ERR_ARG, "%s: %lld packets, the decoder was created for %lld", who, (long long)n, (long long)d->max_packets);
    if (n_sweeps < 1 || n_sweeps > d->max_sweeps) return set_err(PTL_ERR_ARG, "%s: %d sweeps, the decoder was created for %d", who, n_sweeps, d->max_sweeps);
    if (sop)
        for (int64_t i = 0; i < n; ++i)
            if (sop[i] >= n_sweeps) return set_err(PTL_ERR_ARG, "%s: packet %lld names sweep %d of %d", who, (long long)i, sop[i], n_sweeps);
    return PTL_OK;
}
// the three passes for n staged packets into `o` (its img: the decoder's staging or a runner's slot); nothing here waits
static int pktdec_run(ptl_pktdec* d, const void* packets, int64_t stride, int64_t n, const int32_t* sop, int32_t n_sweeps, const PktOut& o) {
    const PktLayout& L = d->L;
    const hipStream_t st = d->stream;
    if (n > 0) {
        if (stride == L.stride) HIPCHK(hipMemcpyAsync(d->d_pkts, packets, (size_t)n * L.stride, hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemcpy2DAsync(d->d_pkts, (size_t)L.stride, packets, (size_t)stride, (size_t)L.bytes, (size_t)n, hipMemcpyHostToDevice, st));
        if (sop) HIPCHK(hipMemcpyAsync(d->d_sop, sop, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIPCHK(d->prof.begin(st));
    hipLaunchKernelGGL(k_pkt_init, dim3((unsigned)((n_sweeps * L.W + PKT_THREADS - 1) / PKT_THREADS)), dim3(PKT_THREADS), 0, st, (int)n_sweeps, L.W, o);
    const int* dsop = sop ? d->d_sop : nullptr;
    if (n > 0) {
        const int cols = (int)(n * L.C);
        hipLaunchKernelGGL(k_pkt_owner, dim3((unsigned)((cols + PKT_THREADS - 1) / PKT_THREADS)), dim3(PKT_THREADS), 0, st, L, d->d_pkts, dsop, (int)n, o);
        hipLaunchKernelGGL(k_pkt_decode, dim3((unsigned)n), dim3(PKT_THREADS), (size_t)L.stride, st, L, d->d_pkts, dsop, o);
    }
    hipLaunchKernelGGL(k_pkt_finish, dim3((unsigned)n_sweeps, (unsigned)L.H), dim3(PKT_THREADS), 0, st, L, d->d_pkts, o);
    HIPCHK(hipGetLastError());
    HIPCHK(d->prof.end(st));
    return PTL_OK;
}
extern "C" int ptl_pktdec_profile(ptl_pktdec* d, int enable, double* ms_total, int64_t* calls, int reset) {
    if (!d) return set_err(PTL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(d->device_id));
    HIPCHK(hipStreamSynchronize(d->stream));
    d->prof.report(enable, ms_total, calls, reset);
    return PTL_OK;
}
extern "C" int ptl_pktdec_decode(ptl_pktdec* d, const void* packets, int64_t stride_bytes, int64_t n, const int32_t* sweep_of_packet, int32_t n_sweeps,
                                 uint32_t* range_out, uint64_t* col_ts_out, uint16_t* col_status_out, ptl_pkt_summary* summary_out) {
    if (!sweep_of_packet) return set_err(PTL_ERR_ARG, "ptl_pktdec_decode: null argument");
    int rc = pktdec_check(d, packets, stride_bytes, n, sweep_of_packet, n_sweeps, "ptl_pktdec_decode");
    if (rc) return rc;
    HIPCHK(hipSetDevice(d->device_id));
    rc = pktdec_run(d, packets, stride_bytes, n, sweep_of_packet, n_sweeps, d->o);
    if (rc) return rc;
    const size_t S = (size_t)n_sweeps, W = (size_t)d->L.W;
    const hipStream_t st = d->stream;
    if (range_out) HIPCHK(hipMemcpyAsync(range_out, d->d_img, S * d->L.H * W * 4, hipMemcpyDeviceToHost, st));
    if (col_ts_out) HIPCHK(hipMemcpyAsync(col_ts_out, d->o.ts, S * W * 8, hipMemcpyDeviceToHost, st));
    if (col_status_out) HIPCHK(hipMemcpyAsync(col_status_out, d->o.status, S * W * 2, hipMemcpyDeviceToHost, st));
    if (summary_out) HIPCHK(hipMemcpyAsync(summary_out, d->o.sum, S * sizeof(PktSummary), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PTL_OK;
}
// ---- the channel fields of a pixel: the table of include/ptudes_mi.h as data, and one launch of packet_field_kernels.h behind
// the three passes
static_assert(PKT_MAX_FIELDS == PTL_PKT_MAX_FIELDS, "the kernel's field slots are the header's");
extern "C" int64_t ptl_pkt_sizeof_field(void) { return (int64_t)sizeof(ptl_pkt_field); }
static const char* const PKT_PROFILE_NAME[4] = {"LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"};
static const char* const PKT_FIELD_NAME[7] = {"RANGE", "REFLECTIVITY", "SIGNAL", "NEAR_IR", "RANGE2", "REFLECTIVITY2", "SIGNAL2"};
struct PktFieldRow { int offset, bytes; unsigned mask; int shift; };  // bytes == 0: the profile has no such field
static const PktFieldRow PKT_FIELD_TABLE[4][7] = {
    /* LEGACY */                      {{0, 4, 0x000fffffu, 0}, {4, 2, 0, 0}, {6, 2, 0, 0}, {8, 2, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},
    /* RNG19_RFL8_SIG16_NIR16 */      {{0, 4, 0x0007ffffu, 0}, {4, 1, 0, 0}, {6, 2, 0, 0}, {8, 2, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},
    /* RNG15_RFL8_NIR8 */             {{0, 2, 0x7fffu, 3}, {2, 1, 0, 0}, {0, 0, 0, 0}, {3, 1, 0, 4}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},
    /* RNG19_RFL8_SIG16_NIR16_DUAL */ {{0, 4, 0x0007ffffu, 0}, {3, 1, 0, 0}, {8, 2, 0, 0}, {12, 2, 0, 0}, {4, 4, 0x0007ffffu, 0}, {7, 1, 0, 0}, {10, 2, 0, 0}},
};
extern "C" int ptl_pkt_field_default(const ptl_pkt_format* fmt, int32_t field_id, ptl_pkt_field* out) {
    if (!fmt || !out) return set_err(PTL_ERR_ARG, "ptl_pkt_field_default: null argument");
    ABI_CHECK(ptl_pkt_format, fmt);
    ABI_CHECK(ptl_pkt_field, out);
    if (fmt->profile < 0 || fmt->profile > 3) return set_err(PTL_ERR_ARG, "ptl_pkt_field_default: unknown lidar packet profile %d (PTL_PKT_*)", fmt->profile);
    if (field_id < 0 || field_id > 6) return set_err(PTL_ERR_ARG, "ptl_pkt_field_default: unknown field %d (PTL_PKT_FIELD_*: 0 .. 6)", field_id);
    const PktFieldRow& r = PKT_FIELD_TABLE[fmt->profile][field_id];
    if (r.bytes == 0)
        return set_err(PTL_ERR_ARG, "ptl_pkt_field_default: profile %s (%d) has no field %s (%d)", PKT_PROFILE_NAME[fmt->profile], fmt->profile,
                       PKT_FIELD_NAME[field_id], field_id);
    out->offset = r.offset; out->bytes = r.bytes; out->mask = r.mask; out->shift = r.shift;
    return PTL_OK;
}
extern "C" int ptl_pktdec_decode_fields(ptl_pktdec* d, const void* packets, int64_t stride_bytes, int64_t n, const int32_t* sweep_of_packet, int32_t n_sweeps,
                                        const ptl_pkt_field* fields, int32_t n_fields, uint32_t* const* field_out, uint32_t* range_out,
                                        uint64_t* col_ts_out, uint16_t* col_status_out, ptl_pkt_summary* summary_out) {
    const char* who = "ptl_pktdec_decode_fields";
    if (!sweep_of_packet || !fields || !field_out) return set_err(PTL_ERR_ARG, "%s: null argument", who);
    int rc = pktdec_check(d, packets, stride_bytes, n, sweep_of_packet, n_sweeps, who);
    if (rc) return rc;
    if (n_fields < 1 || n_fields > PKT_MAX_FIELDS) return set_err(PTL_ERR_ARG, "%s: n_fields = %d: 1 .. %d fields per call", who, n_fields, PKT_MAX_FIELDS);
    const PktLayout& L = d->L;
    PktFields F = {};
    F.n = n_fields;
    for (int f = 0; f < n_fields; ++f) {
        const ptl_pkt_field& q = fields[f];
        ABI_CHECK(ptl_pkt_field, &q);
        if (!field_out[f]) return set_err(PTL_ERR_ARG, "%s: field_out[%d] is null", who, f);
        if (q.bytes != 1 && q.bytes != 2 && q.bytes != 4) return set_err(PTL_ERR_ARG, "%s: field %d: bytes = %d: a field has 1, 2 or 4 bytes", who, f, q.bytes);
        if (q.offset < 0 || q.offset % q.bytes) return set_err(PTL_ERR_ARG, "%s: field %d: offset = %d is not a multiple of its %d bytes (or negative)", who, f, q.offset, q.bytes);
        if ((int64_t)q.offset + q.bytes > L.pix)
            return set_err(PTL_ERR_ARG, "%s: field %d: offset %d + %d bytes lies past the pixel of %d bytes", who, f, q.offset, q.bytes, L.pix);
        if (q.shift < -31 || q.shift > 31) return set_err(PTL_ERR_ARG, "%s: field %d: shift = %d: -31 .. 31", who, f, q.shift);
        F.off[f] = q.offset; F.bytes[f] = q.bytes; F.mask[f] = q.mask ? q.mask : 0xffffffffu; F.shift[f] = q.shift;
    }
    HIPCHK(hipSetDevice(d->device_id));
    const size_t S = (size_t)n_sweeps, W = (size_t)L.W, image = (size_t)L.H * W;
    if (!d->d_fimg) HIPCHK(d->mem.alloc(&d->d_fimg, (size_t)PKT_MAX_FIELDS * d->max_sweeps * image));
    F.img_stride = image;
    for (int f = 0; f < n_fields; ++f) F.img[f] = d->d_fimg + (size_t)f * d->max_sweeps * image;
    rc = pktdec_run(d, packets, stride_bytes, n, sweep_of_packet, n_sweeps, d->o);
    if (rc) return rc;
    const hipStream_t st = d->stream;
    HIPCHK(d->prof.begin(st));
    hipLaunchKernelGGL(k_pkt_fields, dim3((unsigned)(n + (int64_t)n_sweeps * L.H)), dim3(PKT_THREADS), (size_t)L.stride, st, L, d->d_pkts, d->d_sop, (int)n,
                       d->o, F);
    HIPCHK(hipGetLastError());
    HIPCHK(d->prof.end(st));
    for (int f = 0; f < n_fields; ++f) HIPCHK(hipMemcpyAsync(field_out[f], F.img[f], S * image * 4, hipMemcpyDeviceToHost, st));
    if (range_out) HIPCHK(hipMemcpyAsync(range_out, d->d_img, S * image * 4, hipMemcpyDeviceToHost, st));
    if (col_ts_out) HIPCHK(hipMemcpyAsync(col_ts_out, d->o.ts, S * W * 8, hipMemcpyDeviceToHost, st));
    if (col_status_out) HIPCHK(hipMemcpyAsync(col_status_out, d->o.status, S * W * 2, hipMemcpyDeviceToHost, st));
    if (summary_out) HIPCHK(hipMemcpyAsync(summary_out, d->o.sum, S * sizeof(PktSummary), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PTL_OK;
}
// one sweep into a runner's slot (the image's first word at `slot`); returns when the slot is written, like the copy of ptl_*_upload_range
static int pktdec_into_slot(ptl_pktdec* d, const void* packets, int64_t n, void* slot, ptl_pkt_summary* summary, uint64_t* col_ts) {
    PktOut o = d->o;
    o.img = (unsigned*)slot;
    int rc = pktdec_run(d, packets, d->L.bytes, n, nullptr, 1, o);
    if (rc) return rc;
    if (summary) HIPCHK(hipMemcpyAsync(summary, o.sum, sizeof(PktSummary), hipMemcpyDeviceToHost, d->stream));
    if (col_ts) HIPCHK(hipMemcpyAsync(col_ts, o.ts, (size_t)d->L.W * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return PTL_OK;
}
extern "C" int ptl_seq_upload_packets(ptl_seq* s, ptl_pktdec* dec, int64_t k, const void* packets, int64_t n, ptl_pkt_summary* summary, uint64_t* col_ts) {
    if (!s || !dec || k < 0 || k >= s->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    int rc = pktdec_check(dec, packets, dec->L.bytes, n, nullptr, 1, "ptl_seq_upload_packets");
    if (rc) return rc;
    if ((int64_t)dec->L.H * dec->L.W != s->cfg.points_per_scan || dec->device_id != s->cfg.icp.device_id)
        return set_err(PTL_ERR_ARG, "ptl_seq_upload_packets: the decoder (%d x %d, device %d) does not match the runner (points_per_scan %lld, device %d)",
                       dec->L.H, dec->L.W, dec->device_id, (long long)s->cfg.points_per_scan, s->cfg.icp.device_id);
    HIPCHK(hipSetDevice(s->cfg.icp.device_id));
    const size_t slot = (size_t)s->cfg.points_per_scan * 12;
    rc = pktdec_into_slot(dec, packets, n, (char*)s->lane.d_scans + (size_t)k * slot, summary, col_ts);
    if (rc) return rc;
    s->is_range[(size_t)k] = 1;
    return PTL_OK;
}
extern "C" int ptl_batch_upload_packets(ptl_batch* b, int32_t s, ptl_pktdec* dec, int64_t k, const void* packets, int64_t n, ptl_pkt_summary* summary,
                                        uint64_t* col_ts) {
    if (!b || !dec || s < 0 || s >= b->S || k < 0 || k >= b->cfg.n_scans) return set_err(PTL_ERR_ARG, "bad argument");
    int rc = pktdec_check(dec, packets, dec->L.bytes, n, nullptr, 1, "ptl_batch_upload_packets");
    if (rc) return rc;
    if ((int64_t)dec->L.H * dec->L.W != b->cfg.points_per_scan || dec->L.W != b->cfg.icp.scan_cols || dec->device_id != b->cfg.icp.device_id)
        return set_err(PTL_ERR_ARG, "ptl_batch_upload_packets: the decoder (%d x %d, device %d) does not match the batch (points_per_scan %lld, scan_cols %d, device %d)",
                       dec->L.H, dec->L.W, dec->device_id, (long long)b->cfg.points_per_scan, b->cfg.icp.scan_cols, b->cfg.icp.device_id);
    if (!b->lut) return set_err(PTL_ERR_STATE, "set the LUT first (ptl_batch_set_lut)");
    HIPCHK(hipSetDevice(b->cfg.icp.device_id));
    rc = batch_ring_slot_free(b, s, k);
    if (rc) return rc;
    const size_t slot = (size_t)b->cfg.points_per_scan * (b->cfg.range_input ? 4 : 12);
    rc = pktdec_into_slot(dec, packets, n, (char*)b->lane[s].d_scans + (size_t)(k % b->ring) * slot, summary, col_ts);
    if (rc) return rc;
    if (b->ring < b->cfg.n_scans) b->up_hi[s] = k + 1;
    return PTL_OK;
}
