"""Occupancy-grid cases whose answers are written out by hand: one sweep of 1 x 8 pixels from a sensor with identity rotation
at `origin`; a pixel is its end in the sensor frame (f32), (0, 0, 0) = no return.  Unless a case says otherwise the grid is 8 x 4 cells of 1 m
from (0, 0), step 0.5 (samples at t = 0.25, 0.75, 1.25, ...), margin 0.5, band [-0.5, 0.5], range [0, 16].  Coordinates are dyadic wherever a
comparison of the definition is meant to be exact; elsewhere every sample lies well inside its cell.  `free` / `hit`: {(ix, iy): count}, every
other cell 0; `counts`: the summary entries the case pins.  tests/test_occupancy_grid_cpu.py holds the restatement to these answers,
tests/test_gpu_occupancy_grid.py the device."""
import numpy as np

W = 8
BASE = dict(cell=1.0, x0=0.0, y0=0.0, nx=8, ny=4, z_lo=-0.5, z_hi=0.5, margin=0.5, step=0.5, min_range=0.0, max_range=16.0)


def _up32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _dn32(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def _up(x):
    return float(np.nextafter(x, np.inf))


def _case(name, origin, ends, free, hit, cfg=None, **counts):
    px = np.zeros((1, W, 3), dtype=np.float32)
    px[0, :len(ends)] = np.asarray(ends, dtype=np.float32)
    counts.setdefault("n_runs_voted", sum(free.values()))
    counts.setdefault("sum_free", sum(free.values()))
    counts.setdefault("sum_hit", sum(hit.values()))
    counts.setdefault("n_cells_free", len(free))
    counts.setdefault("n_cells_hit", len(hit))
    counts.setdefault("n_scans", 1)
    return dict(name=name, cfg=dict(BASE, **(cfg or {})), origin=np.asarray(origin, dtype=np.float64), xyz=px, free=free, hit=hit, counts=counts)


def hand_cases():
    out = []
    mid = [0.5, 0.5, 0.0]
    # 1. +x from (0.5, 0.5) to (4.5, 0.5): len 4, free samples t <= 3.5: x = 0.75, 1.25, ..., 3.75 -> cells 0 1 1 2 2 3 3; the end in cell 4
    out.append(_case("+x", mid, [[4, 0, 0]], {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}, {(4, 0): 1},
                     n_rays=1, n_no_return=W - 1, n_rays_out_of_range=0, n_ends_outside=0, box_ix0=0, box_iy0=0, box_ix1=4, box_iy1=0))
    # 2. an end exactly on the edge x = 2 (cell 2) and one f32 ulp either side; free samples at x = 0.75, 1.25 (cells 0, 1).  The ray that
    #    ends just below the edge hits cell 1, so its last run (cell 1) gives no free vote
    out.append(_case("an end on a cell edge", mid, [[1.5, 0, 0], [_dn32(1.5), 0, 0], [_up32(1.5), 0, 0]],
                     {(0, 0): 3, (1, 0): 2}, {(2, 0): 2, (1, 0): 1}, n_rays=3, n_no_return=W - 3))
    # 3. an end exactly on x0 + nx cell = 8: outside (fx < nx fails); free samples up to t = 6.75, x = 7.25: all eight cells of the row
    out.append(_case("an end on the grid's far edge", mid, [[7.5, 0, 0]], {(i, 0): 1 for i in range(8)}, {},
                     n_rays=1, n_ends_outside=1, box_ix1=7))
    # 4. the band at the end: rays straight up and down of len 0.5 (no free sample: t_0 = 0.25 > len - margin = 0), p.z - o.z exactly z_hi and
    #    z_lo count, one f32 ulp beyond each does not
    out.append(_case("the band at the end", mid, [[0, 0, 0.5], [0, 0, _up32(0.5)], [0, 0, -0.5], [0, 0, _dn32(-0.5)]], {}, {(0, 0): 2},
                     n_rays=4, n_no_return=W - 4))
    # 5. the band at a sample: straight up, len 4, margin 0, samples at p.z - o.z = 0.25, 0.75, ... exactly.  A band of [0.75, 0.75] holds one
    #    sample: the run of cell (0, 0) votes (the end, 4 m up, is out of the band: no hit takes the vote away); a band that begins one ulp
    #    above 0.75 and ends below 1.25 holds none
    out.append(_case("the band at a sample", mid, [[0, 0, 4]], {(0, 0): 1}, {}, cfg=dict(margin=0.0, z_lo=0.75, z_hi=0.75), n_rays=1))
    out.append(_case("the band one ulp above a sample", mid, [[0, 0, 4]], {}, {}, cfg=dict(margin=0.0, z_lo=_up(0.75), z_hi=1.0), n_rays=1,
                     box_ix0=0, box_iy0=0, box_ix1=-1, box_iy1=-1))
    # 6. t_k exactly len - margin: (0.25, 0.5, 0) -> (3.25, 0.5, 4), len 5, margin 0.25: t_9 = 4.75 = len - margin is the last free sample, at
    #    x = 3.1 (cell 3), 3.8 m up; the band [3.7, 3.9] holds that sample alone (t_8 is 3.4 m up) and not the end (4 m up)
    out.append(_case("t_k = len - margin", [0.25, 0.5, 0.0], [[3, 0, 4]], {(3, 0): 1}, {}, cfg=dict(margin=0.25, z_lo=3.7, z_hi=3.9), n_rays=1))
    # (a margin of 0.25 + 2^-50 makes len - margin the double just below 4.75: one ulp of margin itself would be rounded away in 5 - margin)
    out.append(_case("t_k one ulp past len - margin", [0.25, 0.5, 0.0], [[3, 0, 4]], {}, {}, cfg=dict(margin=0.25 + 2.0 ** -50, z_lo=3.7, z_hi=3.9),
                     n_rays=1))
    # 7. shorter than half a step: no sample, the hit only
    out.append(_case("a short ray", mid, [[0.125, 0, 0]], {}, {(0, 0): 1}, n_rays=1))
    # 8. the last run shares the end's cell: (0.5, 0.5, 0) -> (3.5, 0.5, 4), len 5, margin 0; samples at x = 0.5 + 0.6 t: cells 0 0 1 1 1 2 2 2 3 3,
    #    0.2 .. 3.8 m up.  With the end (exactly 4 m up) in the band it hits cell 3 and the last run gives nothing; out of the band there is no hit
    #    and the last run votes
    out.append(_case("the last run in the end's cell, end in the band", mid, [[3, 0, 4]], {(0, 0): 1, (1, 0): 1, (2, 0): 1}, {(3, 0): 1},
                     cfg=dict(margin=0.0, z_hi=4.0), n_rays=1))
    out.append(_case("the last run in the end's cell, end out of the band", mid, [[3, 0, 4]], {(i, 0): 1 for i in range(4)}, {},
                     cfg=dict(margin=0.0, z_hi=3.9), n_rays=1))
    # 9. out through the corner (0, 0) along the lattice diagonal: (1.75, 1.75) -> (-1.25, -1.25), len 3 sqrt 2, free samples t <= 3.74:
    #    x = y = 1.57 1.22 0.87 0.51 0.16 -0.19 -0.55: runs (1, 1), (0, 0), outside.  x and y are the same double, so no other cell is met
    out.append(_case("out through a corner", [1.75, 1.75, 0.0], [[-3, -3, 0]], {(1, 1): 1, (0, 0): 1}, {}, n_rays=1, n_ends_outside=1))
    # 10. an origin outside the grid, in through the corner: (-1.25, -1.25) -> (1.75, 1.75): x = y = -1.07 -0.72 -0.37 -0.01 0.34 0.69 1.05:
    #     runs outside, (0, 0), (1, 1); the end hits (1, 1), which takes the last run's vote
    out.append(_case("in through a corner", [-1.25, -1.25, 0.0], [[3, 3, 0]], {(0, 0): 1}, {(1, 1): 1}, n_rays=1))
    # 11. from the lattice point (1, 1): along the edge y = 1 (row 1: fy = 1 exactly) to x = 4 (an end on an edge: cell 4), samples at
    #     x = 1.25 1.75 2.25 2.75 3.25; along the edge x = 1 to y = 3, samples at y = 1.25 1.75 2.25; along the lattice diagonal to (3, 3),
    #     len 2 sqrt 2, free samples t <= 2.33: x = y = 1.18 1.53 1.88 2.24 2.59
    out.append(_case("along edges and a lattice diagonal", [1.0, 1.0, 0.0], [[3, 0, 0], [0, 2, 0], [2, 2, 0]],
                     {(1, 1): 3, (2, 1): 1, (3, 1): 1, (1, 2): 1, (2, 2): 1}, {(4, 1): 1, (1, 3): 1, (3, 3): 1}, n_rays=3))
    # 12. len exactly min_range and max_range are used, one f32 ulp outside is not; no return; NaN (a return, its len is NaN: out of range)
    out.append(_case("range limits, no return, NaN", mid, [[1, 0, 0], [4, 0, 0], [_dn32(1.0), 0, 0], [_up32(4.0), 0, 0], [0, 0, 0], [np.nan, 1, 0]],
                     {(0, 0): 2, (1, 0): 1, (2, 0): 1, (3, 0): 1}, {(1, 0): 1, (4, 0): 1}, cfg=dict(min_range=1.0, max_range=4.0),
                     n_rays=2, n_rays_out_of_range=3, n_no_return=3))
    # 13. long rays: len 20 (80 march samples, 81 with the end) and len 300 (1 200, 1 201 with the end) at step 0.25 through cells of 0.5 m:
    #     from (0.25, 0.25), x = 0.375, 0.625, ... up to t = 19.375 (cell 39), the end at 20.25 in cell 40; likewise along y up to cell 599
    free = {(i, 0): 1 for i in range(1, 40)}
    free.update({(0, j): 1 for j in range(1, 600)})
    free[(0, 0)] = 2
    out.append(_case("long rays", [0.25, 0.25, 0.0], [[20, 0, 0], [0, 300, 0]], free, {(40, 0): 1, (0, 600): 1},
                     cfg=dict(cell=0.5, nx=64, ny=640, step=0.25, margin=0.5, max_range=512.0), n_rays=2, n_runs_voted=640))
    return out


def case_arrays(case):
    """(free, hit) uint32 (ny, nx) of the case's answer"""
    cfg = case["cfg"]
    free, hit = np.zeros((cfg["ny"], cfg["nx"]), dtype=np.uint32), np.zeros((cfg["ny"], cfg["nx"]), dtype=np.uint32)
    for (ix, iy), v in case["free"].items():
        free[iy, ix] = v
    for (ix, iy), v in case["hit"].items():
        hit[iy, ix] = v
    return free, hit


def case_rays(case, col_poses=None):
    """(o, w, ret) of the case's sweep for the restatement; col_poses (W, 4, 4) as the device evaluated them, else the nominal pose"""
    from tests.helpers import occupancy_grid_numpy as og
    if col_poses is None:
        col_poses = np.tile(np.eye(4), (W, 1, 1))
        col_poses[:, :3, 3] = case["origin"]
    return og.rays_of_sweep(case["xyz"].astype(np.float64), np.any(case["xyz"] != 0.0, axis=2), col_poses)
