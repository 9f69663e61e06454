"""The fly-by renderer: what a frame costs on the device; one JSON line (profiles/r17_render_cost.json).

Nobody has measured any of this before, and no bar is set in advance: the table is the result.  What to look for, written down before the first
run: a frame reads every stored point once per frame (24 bytes each, plus 16 bytes of directory per block of the pool) and issues at most
point_px^2 64-bit atomics per point; in a dense coursing view most splats are occluded and the plain load in front of the atomic should remove
most of them; in the apex view the whole map falls into few pixels, the atomics collide on few lines, and the early reject matters most.

  map       `--sweeps` sweeps of the seed-1000 synthetic 128 x 1024 sequence into a 0.5 m map (SeqRunner.build_map, ground-truth knots)
  frames    1280 x 720, point_px 1, 2 and 3
  views     coursing: the camera of the fly-by's COURSING state half way along the trajectory (pitch -70, yaw 120, dolly -70: 25 m away);
            apex: the TO_THE_APEX end view (pitch 0, yaw 140, the apex dolly of the trajectory's extent - the synthetic trajectory stays in one
            hall, so this camera is still inside the map);
            far: the same from 600 m, where the whole map falls into a few dozen pixels across and the atomics collide most
  batches   1 and 16 frames per launch (the 16 frames turn the yaw by 0.5 degrees each)
  early     the plain load in front of the atomicMin on and off (ptl_render_debug_set_early_reject)
Per cell: HIP-event milliseconds per frame (device work only: clear, splat, resolve), median and spread of `--repeats` runs, the points in view
and the pixels covered.

python tools/render_cost.py [--sweeps 100] [--repeats 5] [--out profiles/r17_render_cost.json]"""
import argparse
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd import utils as pu  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

BOUNDS = 1.5
W, H = 1280, 720
FAR_M = 600.0


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def build_map(n):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    lut, scans = fly.synthetic_range_scans(seq)
    kt = np.arange(0, n * seq.scan_dt + 0.3, 0.02)
    knots = [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    runner.set_lut(lut)
    for k, sc in enumerate(scans):
        runner.upload_range(k, sc.range_mm)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    acc.add_run(runner, traj, sweep_times(seq))
    runner.close()
    traj.close()
    return acc, seq.gt_poses()


def views(poses):
    mm = np.zeros((3, 2))
    for p in poses:
        fly.update_min_max(mm, p[:3, 3])
    mid = np.array(poses[len(poses) // 2])
    coursing = fly.Camera(target=np.linalg.inv(mid), pitch=-70.0, yaw=120.0, dolly=-70.0)
    flat = mid.copy()
    flat[:3, :3] = np.eye(3)
    apex = fly.Camera(target=np.linalg.inv(flat), pitch=0.0, yaw=140.0, dolly=pu.estimate_apex_dolly(mm, 90.0))
    far = fly.Camera(target=np.linalg.inv(flat), pitch=0.0, yaw=140.0, dolly=100.0 * float(np.log(FAR_M / 50.0)))
    return {"coursing": coursing, "apex": apex, "far": far}


def cams_of(camera, n):
    out = []
    for i in range(n):
        c = copy.copy(camera)
        c.yaw = camera.yaw + 0.5 * i
        out.append(c.cam(W, H))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    acc, poses = build_map(a.sweeps)
    voxels, points = acc.map_size()
    z = acc.map_points()[:, 2]
    res = {"what": "fly-by renderer: device ms per 1280 x 720 frame (DESIGN.md 3.21)", "code_id": core.L.lib().ptl_code_id().decode(),
           "map": {"sequence": "make_sequence(seed=1000)", "sweeps": a.sweeps, "voxel_size": 0.5, "map_voxels": int(voxels), "map_points": int(points),
                   "pool_blocks": int(acc.icp.cfg.map_block_capacity)},
           "frame": [W, H], "cells": []}
    for name, camera in views(poses).items():
        for px in (1, 2, 3):
            for batch in (1, 16):
                r = core.Renderer(W, H, point_px=px, z_range=(float(z.min()), float(z.max())), max_frames_per_call=batch)
                cams = cams_of(camera, batch)
                for early in (True, False):
                    r.set_early_reject(early)
                    r.render(acc.icp, cams)  # (first call: code object load)
                    ms = []
                    for _ in range(a.repeats):
                        _, keys, in_view, t = r.render(acc.icp, cams, keys=True, timing=True)
                        ms.append(t / batch)
                    cell = {"view": name, "view_distance_m": camera.view_distance(), "point_px": px, "frames_per_launch": batch, "early_reject": early,
                            "device_ms_per_frame": stat(ms), "points_in_view": int(in_view[0]),
                            "pixels_covered": int((keys[0] != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())}
                    print(cell, flush=True)
                    res["cells"].append(cell)
                r.close()
    acc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
