// diag.h -- everything the diagnostic builds add to the kernels, defined once: the build flavours, the named slots their values are
// kept in, one lap timer and one add.  The product build (no flavour) parses all of it and emits none of it.
//
//   make PHASES=1          -DGN_PHASE_CLOCKS   phase clocks and search statistics of the 8-lane Gauss-Newton loop (tools/phase_batch.py)
//   make IT0=1             -DGN_IT0_CLOCK      only the point loop of the first iteration against the others (tools/phase_batch.py)
//   make STAGES=1          -DSEQ_STAGE_CLOCKS  wall-clock ticks per stage and barrier wait of the free-running kernel (tools/stage_clocks.py)
//   make EXTRA=-DMAP_DIAG                      the sites that raise ERR_TABLE count themselves (tools/um_diag.py)
// Any of them may be built together: every value has a slot of its own.
//
// The slots are 64-bit integer words behind the per-workgroup clocks of Ctx::wg_clk - slot i at wg_clk[2 * Ctx::G + i], G the handle's
// gn_workgroups, whatever the team size - cleared by a cold start, read by ptl_icp_diag and named by ptl_diag_slot_name (Python:
// Icp.diag() / SeqRunner.diag() / BatchRunner.diag(s) return {name: value}).  Ticks are wall-clock ticks (100 MHz) for the sq_ / k1_ slots and
// cycle-counter ticks (what GN_CLK() reads) for the others.
#pragma once

namespace diag {
#ifdef GN_PHASE_CLOCKS
constexpr bool phases = true;
#else
constexpr bool phases = false;
#endif
#ifdef GN_IT0_CLOCK
constexpr bool it0 = true;
#else
constexpr bool it0 = false;
#endif
#ifdef SEQ_STAGE_CLOCKS
constexpr bool stages = true;
#else
constexpr bool stages = false;
#endif
#ifdef MAP_DIAG
constexpr bool map = true;
#else
constexpr bool map = false;
#endif
constexpr bool cycles = phases || it0;  // GN_CLK() reads the cycle counter
constexpr int flavours = (phases ? 1 : 0) | (it0 ? 2 : 0) | (stages ? 4 : 0) | (map ? 8 : 0);  // ptl_build_info [13]
}  // namespace diag

// The cycle counter where a flavour reads it, 0 in the product build: the always-on bookkeeping of the Gauss-Newton loops (ph[],
// DevState::gn_phase_clk) is written in terms of it and adds zeros there.  Eight 64-bit accumulators and the counter reads otherwise
// compete with the loop's live values for scalar and vector registers (the 32-lane kernel runs at its 128-VGPR cap and spills).
// A read that only PHASES uses is written `diag::phases ? GN_CLK() : 0ll`: an IT0 build times the point loop and reads nothing else.
#if defined(GN_PHASE_CLOCKS) || defined(GN_IT0_CLOCK)
#define GN_CLK() ((long long)__builtin_readcyclecounter())
#else
#define GN_CLK() (0ll)
#endif

// X(name, words): the one list of slots.  A name with several words reads name_0, name_1, ... through ptl_diag_slot_name.
#define DIAG_SLOT_LIST(X)                                                                                                                  \
    /* STAGES, workgroup 0 of the team (sq_prepare, sq_map_update): every stage and the barrier wait behind it */                          \
    X(sq_prologue, 1) X(sq_wait_prologue, 1) X(sq_deskew_vds1, 1) X(sq_wait_deskew_vds1, 1) X(sq_compact_fd, 1) X(sq_wait_compact_fd, 1)   \
    X(sq_vds2, 1) X(sq_wait_vds2, 1) X(sq_compact_src, 1)                                                                                  \
    X(sq_insert_a, 1) X(sq_wait_insert_a, 1) X(sq_insert_b, 1) X(sq_wait_insert_b, 1) X(sq_prune, 1)                                       \
    /* STAGES, inside K1 (d_deskew_vds1), thread 0 of that workgroup, every step waited out */                                             \
    X(k1_entry, 1) X(k1_load_deskew_store, 1) X(k1_claim, 1) X(k1_bid, 1) X(k1_slot1, 1) X(k1_count, 1)                                    \
    /* PHASES, gn8_search, all workgroups of the sequence: counts */                                                                       \
    X(searches, 1) X(survivor_rounds, 1) X(rows_rebuilt, 1)                                                                                \
    /* ... what bounds everybody outside the answer row (a scanned candidate | the box of a dropped voxel), and bound / distance of  */    \
    /* the winner in [1,1.2) [1.2,1.5) [1.5,2) [2,3) [3,..) */                                                                             \
    X(bound_candidate, 1) X(bound_box, 1) X(bound_ratio, 5)                                                                                \
    /* PHASES or IT0, gn8_body, workgroup 0: ticks of the point loop in the first iteration of a scan | in the others */                   \
    X(point_loop_first, 1) X(point_loop_others, 1)                                                                                         \
    /* PHASES, gn8_body, workgroup 0, iterations > 0: phase A per chunk, the search passes */                                              \
    X(phase_a_eval, 1) X(phase_a_compact, 1) X(phase_a_chunks, 1) X(search_pass_ticks, 1) X(search_passes, 1)                              \
    /* PHASES, gn8_search, thread 0 of the first teams' workgroups, iterations > 0, every step waited out */                               \
    X(search_row_key, 1) X(search_rebuild, 1) X(search_first_round, 1) X(search_survivors, 1) X(search_answer_row, 1) X(searches_timed, 1) \
    /* ... the same laps, same thread, in a scan's FIRST iteration (every point searches and rebuilds its row; same order as the set   */    \
    /* above: gn8_search adds one offset), and over all workgroups the first iteration's searches and survivor rounds */                  \
    X(search_it0_row_key, 1) X(search_it0_rebuild, 1) X(search_it0_first_round, 1) X(search_it0_survivors, 1) X(search_it0_answer_row, 1)  \
    X(searches_timed_it0, 1) X(searches_it0, 1) X(survivor_rounds_it0, 1)                                                                  \
    /* PHASES, gn8_search, all workgroups: searches whose place in the queue (front: row valid | back: rebuild) disagrees with pc_key[] */ \
    X(queue_kind_mismatch, 1)                                                                                                              \
    /* PHASES, serial tail of an iteration, workgroup 0 */                                                                                 \
    X(tail_sums, 1) X(tail_solve, 1) X(tail_exp_flags, 1) X(tails, 1)                                                                      \
    /* PHASES, workgroup 0, iterations > 0: why the answer row did not settle a point, and the searches by iteration index */              \
    X(miss_other_neighbour, 1) X(miss_voxel_changed, 1) X(miss_no_answer, 1) X(miss_same_neighbour, 1) X(misses_at_iteration, 24)          \
    /* MAP_DIAG: count per site that raised ERR_TABLE (insert a: no slot | insert a: table 3/4 full | insert b: list too long | */        \
    /* rebuild), and site + two values of a first occurrence */                                                                           \
    X(map_site, 4) X(map_first_site, 1) X(map_first_a, 1) X(map_first_b, 1)

enum DiagSlot {
#define X(name, words) D_##name, D_##name##_end_ = D_##name + (words) - 1,
    DIAG_SLOT_LIST(X)
#undef X
    DIAG_SLOTS
};
struct DiagSlotName { const char* base; int first, words; };
static const DiagSlotName DIAG_SLOT_NAMES[] = {
#define X(name, words) {#name, D_##name, words},
    DIAG_SLOT_LIST(X)
#undef X
};

// += v on slot `slot` of the context's handle, when the flavour ON is compiled in
template <bool ON, class CT>
__device__ __forceinline__ void diag_add(const CT& c, int slot, long long v = 1) {
    if constexpr (ON) atomicAdd((unsigned long long*)(c.wg_clk + 2 * c.G + slot), (unsigned long long)v);
}
// MAP_DIAG: a site that raises ERR_TABLE counts itself and leaves two values of its first occurrence
template <class CT>
__device__ __forceinline__ void diag_map_site(const CT& c, int site, long long a, long long b) {
    if constexpr (diag::map) {
        unsigned long long* w = (unsigned long long*)(c.wg_clk + 2 * c.G);
        if (atomicAdd(w + D_map_site + site, 1ull) == 0ull) { w[D_map_first_site] = (unsigned long long)site; w[D_map_first_a] = (unsigned long long)a; w[D_map_first_b] = (unsigned long long)b; }
    }
}
// The lap timer: lap(c, slot) adds the ticks since the previous lap (or the construction) to the slot, in the thread(s) with `me`.
// CYCLES: the cycle counter (GN_CLK()) instead of the 100 MHz wall clock.  WAIT: outstanding memory is waited out before the clock is read,
// so that a lap owns the latency of what it requested.
template <bool ON, bool CYCLES, bool WAIT>
struct DiagLap {
    long long t;
    bool me;
    static __device__ __forceinline__ long long now() { return CYCLES ? (long long)__builtin_readcyclecounter() : (long long)wall_clock64(); }
    __device__ __forceinline__ explicit DiagLap(bool me_) : t(now()), me(me_) {}
    template <class CT>
    __device__ __forceinline__ void lap(const CT& c, int slot) {
        if (WAIT) __builtin_amdgcn_s_waitcnt(0);
        const long long n = now();
        if (me) diag_add<true>(c, slot, n - t);
        t = n;
    }
};
template <bool CYCLES, bool WAIT>
struct DiagLap<false, CYCLES, WAIT> {
    __device__ __forceinline__ explicit DiagLap(bool) {}
    template <class CT>
    __device__ __forceinline__ void lap(const CT&, int) const {}
};
