"""The occupancy grid: what the pass over a run's sweeps costs per 128 x 1024 sweep, beside the carve pass and the map build of
the same sweeps; one JSON line (profiles/r26_occupancy_grid_cost.json).

Expectation, written down before the first run.  DESIGN.md 3.24 measured that a ray march is bound by instruction issue.  The grid's march has
no hash probe and no point walk, but at the parameters used here (cells of 0.25 m, step 0.125 m) it takes twice the carve's samples per metre,
and every sample costs three fp64 divisions (t_k / len and the two cell coordinates, which the definition writes as divisions) beside some
twenty other fp64 operations.  So the time should go to the arithmetic of the sample loop, not to the atomics: only the samples inside the
height band can vote, a ray of a 90 degree beam fan leaves a band of +-0.5 m after a few metres, and a ray issues one atomic per cell, not per
sample - a few million scattered u32 atomics per sweep, which the L2 takes at tens of G/s.  The cells next to the sensor are the exception:
every ray crosses them, so some hundred thousand adds per sweep go to a handful of addresses; that is where merging in the wavefront could pay.
The guess: 0.3 - 0.6 ms per sweep, about the carve's one-lane-per-ray build (0.49 ms: half the samples, but probes) and three to four times
faster than the carve as shipped (1.65 ms); the GRID_MERGE build slower than the plain form, because its ballot loop runs at every sample
at which any lane of the wavefront changes cell, while the contended cells are few.  No rate is fixed in advance; what the run says is written
beside this text, and DESIGN.md 3.29 carries the correction if it disagrees.
Correction after the first run (profiles/r26_occupancy_grid_cost.json): wrong about the atomics.  With every lane issuing its own
atomic the pass took 2.19 ms per sweep, a third MORE than the carve as shipped, and the wavefront merge took 0.85 ms, 2.6 times less, with
equal counts: 1.5 million votes per sweep, of which 55 % go to the 1 % most-voted cells - the cells around the sensor that every ray crosses,
871 151 votes for one cell in 40 sweeps.  Adds to one address are taken one after the other; the arithmetic is not what bounds the plain form.
The merge became the default and the plain form the build option.

  cost     the scene of tools/map_carve_cost.py: the seed-1000 synthetic sequence of `--sweeps` sweeps of 128 x 1024, resident in a SeqRunner,
           ground-truth knots.  Alternated in one process, `--repeats` rounds after one warm-up round:
             build   SeqRunner.build_map into a fresh handle (0.5 m voxels): wall ms per sweep
             carve   Carver.add_run over the same resident sweeps against the first map: HIP-event ms per sweep
             grid    OccupancyGrid.add_run over the same resident sweeps into a cleared grid: HIP-event and wall ms per sweep (the product:
                     a wavefront merges equal cells before the atomic)
             plain   `--other-lib PATH`: the same add through a second copy of the library built with make EXTRA=-DGRID_MERGE=0 (every lane
                     its own atomic), loaded into this process beside the first (the handles of trajectory and runner are plain structs of
                     one layout); its counts must equal the product's
           median and spread (max - min).  Atomics per sweep (free + hit votes) and the share of them that goes to the 1 % most-voted cells.

python tools/occupancy_grid_cost.py [--sweeps 40] [--repeats 5] [--other-lib PATH] [--out profiles/r26_occupancy_grid_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import _lib as L  # noqa: E402
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

BOUNDS = 1.5
CELL, MAX_RANGE = 0.25, 60.0
EXPECTATION = ("bound by the fp64 arithmetic of the sample loop (three divisions per sample), not by the atomics; 0.3 - 0.6 ms per sweep, about "
               "the carve's one-lane-per-ray build and three to four times faster than the carve as shipped; the GRID_MERGE build slower than "
               "the plain form, the contended cells next to the sensor being few")


FIRST_RUN = ("with the plain atomic as the default build (code id 747c8e7dca3c, the merge build 34873ddab787): plain 2.1916 ms per sweep "
             "(spread 0.0010), merge 0.8473 ms (spread 0.0030), equal counts, carve 1.6481 ms, build 0.0833 ms; the expectation was wrong about "
             "the atomics, and the merge became the default")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def new_map(seq):
    return core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                    map_table_capacity=1 << 23)


class OtherGrid:
    """a grid handle of a second copy of the library (another build of the same sources), fed the first copy's trajectory and runner"""

    def __init__(self, path, cfg):
        self.lib = C.CDLL(path)
        for name, (res, args) in L.PROTOTYPES.items():
            if name.startswith("ptl_grid_") or name in ("ptl_last_error", "ptl_code_id"):
                f = getattr(self.lib, name)
                f.restype, f.argtypes = res, args
        self.code_id = self.lib.ptl_code_id().decode()
        self._h = C.c_void_p()
        self.check(self.lib.ptl_grid_create(0, C.byref(cfg), C.byref(self._h)))

    def check(self, rc):
        if rc:
            raise RuntimeError(f"{rc}: {self.lib.ptl_last_error().decode()}")

    def add_run(self, runner, traj, t0t1):
        t = np.ascontiguousarray(t0t1, dtype=np.float64).reshape(-1)
        nv, ns = C.c_int64(), C.c_int64()
        self.check(self.lib.ptl_grid_add_seq(self._h, runner._h, traj._h, L.dptr(t), 0, runner.n_scans - 1, C.byref(nv), C.byref(ns)))

    def read(self, nx, ny):
        free, hit = np.zeros((ny, nx), dtype=np.uint32), np.zeros((ny, nx), dtype=np.uint32)
        res = L.GridResult()
        u32p = C.POINTER(C.c_uint32)
        self.check(self.lib.ptl_grid_read(self._h, C.byref(res), 0, 0, nx, ny, free.ctypes.data_as(u32p), hit.ctypes.data_as(u32p)))
        return free, hit, res

    def clear(self):
        self.check(self.lib.ptl_grid_clear(self._h))

    def close(self):
        self.lib.ptl_grid_destroy(self._h)


def cost(n, repeats, other_lib):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(n):
        runner.upload_scan(k, seq.scan(k))
    t0t1 = sweep_times(seq)
    m = new_map(seq)
    runner.build_map(m, traj, t0t1)
    x0, y0, nx, ny = fly.grid_bounds(np.array([p[:3, 3] for _, p in knots]), CELL, MAX_RANGE)
    grid = core.OccupancyGrid(CELL, x0, y0, nx, ny, seq.W, seq.H * seq.W, max_range=MAX_RANGE)
    other = OtherGrid(os.path.abspath(other_lib), grid.cfg) if other_lib else None
    build_wall, carve_dev, grid_dev, grid_wall, plain_dev, plain_wall = [], [], [], [], [], []
    for rep in range(repeats + 1):  # (round 0: code object load, first touch)
        fresh = new_map(seq)
        core.device_sync()
        t0 = time.perf_counter()
        runner.build_map(fresh, traj, t0t1)
        bw = 1e3 * (time.perf_counter() - t0) / n
        fresh.close()
        car = core.Carver(m)
        before = car.votes().device_ms
        car.add_run(runner, traj, t0t1)
        cd = (car.votes().device_ms - before) / n
        car.close()
        grid.clear()
        before = grid.summary().device_ms
        core.device_sync()
        t0 = time.perf_counter()
        grid.add_run(runner, traj, t0t1)
        gw = 1e3 * (time.perf_counter() - t0) / n
        gd = (grid.summary().device_ms - before) / n  # (includes one summary's reduction: one launch over the cells)
        if other:
            other.clear()
            before = other.read(1, 1)[2].device_ms
            core.device_sync()
            t0 = time.perf_counter()
            other.add_run(runner, traj, t0t1)
            mw = 1e3 * (time.perf_counter() - t0) / n
            md = (other.read(1, 1)[2].device_ms - before) / n
        if rep:
            build_wall.append(bw); carve_dev.append(cd); grid_dev.append(gd); grid_wall.append(gw)
            if other:
                plain_dev.append(md); plain_wall.append(mw)
    c = grid.read()
    r = c.result
    votes = (c.free.astype(np.int64) + c.hit.astype(np.int64)).reshape(-1)
    touched = np.sort(votes[votes > 0])[::-1]
    top = touched[:max(1, len(touched) // 100)]
    cls = c.classify()
    out = {"sweeps": n, "shape": [seq.H, seq.W], "grid": [nx, ny], "map_voxel_size": 0.5,
           "parameters": {k: getattr(r, k) for k in ("cell", "x0", "y0", "z_lo", "z_hi", "margin", "step", "min_range", "max_range")},
           "build_wall_ms_per_sweep": stat(build_wall), "carve_device_ms_per_sweep": stat(carve_dev),
           "grid_device_ms_per_sweep": stat(grid_dev), "grid_wall_ms_per_sweep": stat(grid_wall),
           "per_sweep": {"rays": r.n_rays / n, "atomics": (r.sum_free + r.sum_hit) / n, "free_votes": r.sum_free / n, "hit_votes": r.sum_hit / n},
           "atomics_in_the_1_percent_most_voted_cells": {"cells": int(len(top)), "of_touched_cells": int(len(touched)),
                                                         "share": float(top.sum() / max(int(touched.sum()), 1)), "most_voted_cell": int(touched[0])},
           "summary": {k: int(getattr(r, k)) for k in ("n_scans", "n_scans_skipped", "n_rays", "n_rays_out_of_range", "n_no_return", "n_runs_voted",
                                                       "n_ends_outside", "n_cells_free", "n_cells_hit", "sum_free", "sum_hit")},
           "classes_default_policy": {"free": int((cls == 0).sum()), "occupied": int((cls == 1).sum()), "unknown": int((cls == 2).sum())}}
    if other:
        free, hit, _ = other.read(nx, ny)
        out["plain_device_ms_per_sweep"], out["plain_wall_ms_per_sweep"] = stat(plain_dev), stat(plain_wall)
        out["plain_code_id"], out["plain_build"] = other.code_id, "make EXTRA=-DGRID_MERGE=0"
        out["same_counts"] = bool(np.array_equal(free, c.free) and np.array_equal(hit, c.hit))
        out["plain_over_merge"] = out["plain_device_ms_per_sweep"]["median"] / out["grid_device_ms_per_sweep"]["median"]
        other.close()
    out["grid_over_carve"] = out["grid_device_ms_per_sweep"]["median"] / out["carve_device_ms_per_sweep"]["median"]
    for h in (grid, m, runner, traj):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="a library built with EXTRA=-DGRID_MERGE=0: loaded beside the product library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "occupancy grid: device and wall ms per 128 x 1024 sweep beside the carve pass and the map build of the same sweeps, atomics "
                   "per sweep and their share in the most-voted cells, the wavefront merge (the product) against the plain atomic (DESIGN.md 3.29)",
           "code_id": core.L.lib().ptl_code_id().decode(), "expectation_before_the_run": EXPECTATION,
           "first_run": FIRST_RUN}
    res.update(cost(a.sweeps, a.repeats, a.other_lib))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
