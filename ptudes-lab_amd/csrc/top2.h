// top2.h -- what one lane of the voxel scan keeps of the stored points it has seen (scan_voxelsL in icp_kernels.h; compiled for
// the host as well: tests/hip/top2_probe.hip holds it against the three-branch rule it replaces).
#pragma once
#include "devmath.h"

// (bd, border, bp): the nearest candidate seen so far under (squared distance, then id); (b2d, b2o, b2p): the second under the
// same order; sd: the smallest distance among everything else.  Nothing seen yet: distances DBL_MAX, ids 0xFFFFFFFF.
struct Top2 {
    double bd, b2d, sd;
    unsigned border, b2o;
    V3 bp, b2p;
};
// one slot of a call: a stored point, its squared distance to the source point, its id (voxel * 32 + index), and whether the
// slot holds a point at all
struct Top2Cand {
    V3 p;
    double d2;
    unsigned id;
    bool act;
};

PTL_HD double top2_sel(bool c, double a, double b) { return c ? a : b; }
PTL_HD unsigned top2_sel(bool c, unsigned a, unsigned b) { return c ? a : b; }
PTL_HD V3 top2_sel(bool c, V3 a, V3 b) { return V3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }

// The state after the N slots of a call.  It does not depend on the order of the slots: the best and the second are the two
// smallest of {state, slots} under (distance, id), sd the smallest distance of the rest - exactly what
//     if (c < best) { sd = fmin(sd, b2d); second = best; best = c; }
//     else if (c < second) { sd = fmin(sd, b2d); second = c; }
//     else sd = fmin(sd, d2);
// leaves, slot after slot.  Both comparisons of a slot read the state as it was before the slot, and what follows them is
// selects: in a slot that holds points the 64 lanes of a wavefront take all three bodies between them, so the bodies cost
// their sum, and each of them was a compare -> scalar mask -> exec -> branch step of its own.
// An inactive slot is (+inf, 0xFFFFFFFF): it loses every comparison and leaves sd alone, so it is stepped over - the ONE
// branch per slot that is kept.  Voxels hold 7-8 points on average, so most slots of the second and third chunk of a voxel
// are empty in every lane of the wavefront and the branch skips them whole; paying the selects for them (the slot entered
// as +inf through one more select) measured 23 % slower than the three-branch rule.
// No NaN occurs (d2 is finite), so x < y ? x : y is fmin(x, y) value for value.
template <int N>
PTL_HD Top2 top2_update(Top2 s, const Top2Cand (&c)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (!c[j].act) continue;
        const double d = c[j].d2;
        const unsigned id = c[j].id;
        const bool lt1 = (d < s.bd) | ((d == s.bd) & (id < s.border));  // the slot beats the best
        const bool lt2 = (d < s.b2d) | ((d == s.b2d) & (id < s.b2o));   // ... the second
        const bool in2 = lt1 | lt2;
        const double out = top2_sel(in2, s.b2d, d);  // what leaves the two nearest: the old second, or the slot itself
        s.sd = top2_sel(out < s.sd, out, s.sd);
        // the second: the old best where the slot beats it, the slot where it beats the second only
        s.b2d = top2_sel(in2, top2_sel(lt1, s.bd, d), s.b2d);
        s.b2o = top2_sel(in2, top2_sel(lt1, s.border, id), s.b2o);
        s.b2p = top2_sel(in2, top2_sel(lt1, s.bp, c[j].p), s.b2p);
        s.bd = top2_sel(lt1, d, s.bd);
        s.border = top2_sel(lt1, id, s.border);
        s.bp = top2_sel(lt1, c[j].p, s.bp);
    }
    return s;
}
