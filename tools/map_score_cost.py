"""The map score: what the pass costs, and what it says about the four trajectories of DESIGN.md 3.14; one JSON line
(profiles/r13_map_score_cost.json).

Hypothesis, written down before the first run: the pass is bound by the 27 dependent table probes per voxel plus one read of the pool;
the re-reads of neighbouring voxels' points are served by L2.  Its time should therefore be near the export of the same map
(ptl_icp_map_points: one read of the pool) plus the probe chain, and far below the time the map took to build.

  cost      HIP-event time of the call's kernels (ptl_map_score_result.device_ms) and the wall time of the whole call, `--repeats` times on
            one map, median and spread (max - min); beside it the wall time of the export of the same map and of its build, same process:
              sweeps_200   200 sweeps of 128 x 1024 into a 0.5 m map (SeqRunner.build_map over resident range images, ground-truth knots)
              wobble_40    the 40-sweep 64 x 1024 wobble map of tools/map_cost.py sharpness() at 0.1 m (ground truth)
  sharpness the table of DESIGN.md 3.14 again - occupied 0.1 m voxels of the wobble map under four trajectories - with the score beside
            the count: mean plane variance, its square root in mm, mean entropy, scored and sparse points (radius = voxel size = 0.1).

python tools/map_score_cost.py [--sweeps 200] [--repeats 7] [--out profiles/r13_map_score_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

BOUNDS = 1.5
HYPOTHESIS = ("bound by the 27 dependent table probes per voxel plus one read of the pool, neighbours' re-reads served by L2: near the export "
              "of the same map plus the probe chain, far below the build")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def score_dict(s):
    return {"n_points": s.n_points, "n_scored": s.n_scored, "n_sparse": s.n_sparse, "mean_plane_var": s.mean_plane_var,
            "thickness_mm": s.thickness_mm, "mean_entropy": s.mean_entropy, "mean_neighbours": s.mean_neighbours, "radius": s.radius,
            "min_neighbours": s.min_neighbours, "sigma_floor": s.sigma_floor}


def time_score(m, repeats):
    """device and wall milliseconds of `repeats` scores of one map, the export's wall milliseconds beside them"""
    m.map_score()  # (first call: code object load)
    dev, wall, export = [], [], []
    for _ in range(repeats):
        core.device_sync()
        t0 = time.perf_counter()
        s = m.map_score()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(s.device_ms)
        t0 = time.perf_counter()
        pts = m.map_points()
        export.append(1e3 * (time.perf_counter() - t0))
    return {"score_device_ms": stat(dev), "score_wall_ms": stat(wall), "export_wall_ms": stat(export), "export_bytes": int(pts.nbytes),
            "score": score_dict(s)}


def cost_sweeps(n, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    lut, scans = fly.synthetic_range_scans(seq)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    runner.set_lut(lut)
    for k, sc in enumerate(scans):
        runner.upload_range(k, sc.range_mm)
    builds = []
    for _ in range(3):
        acc = fly.MapAccumulator(lut, voxel_size=0.5)
        core.device_sync()
        t0 = time.perf_counter()
        acc.add_run(runner, traj, sweep_times(seq))
        size = acc.map_size()
        builds.append(1e3 * (time.perf_counter() - t0))
        if len(builds) < 3:
            acc._icp.close()
    out = {"sweeps": n, "shape": [seq.H, seq.W], "voxel_size": 0.5, "map_voxels": int(size[0]), "map_points": int(size[1]),
           "build_wall_ms": stat(builds)}
    out.update(time_score(acc._icp, repeats))
    for h in (acc._icp, runner, traj):
        h.close()
    return out


def wobble(repeats, n=40, H=64, voxel=0.1):
    seq = synth.make_path_sequence(seed=2000, n_scans=n, H=H, W=1024, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)
    ends = [seq.imu_range_for_scan(k)[1] for k in range(n)]
    r = core.SeqRunner(n, seq.H * seq.W, ends[-1], max_range=70.0, min_range=1.0, use_imu_prediction=True)
    for k in range(n):
        r.upload_scan(k, seq.scan(k))
    r.upload_imu(seq.imu[: ends[-1]], ends)
    r.enable_smoother(True)
    r.run()
    o = r.results()
    sm = r.smooth(nav=False, cov=False)
    t0t1 = sweep_times(seq, n)
    mid = np.repeat(t0t1.mean(axis=1, keepdims=True), 2, axis=1)
    gk = gt_knots(seq, n)
    cases = {"ground_truth": (gk, t0t1), "ground_truth_one_pose_per_sweep": (gk, mid), "smoothed": (list(zip(sm["t"], sm["poses"])), t0t1),
             "filter": (list(zip(o["res_t"], o["res_poses"])), t0t1)}
    table = {"sweeps": n, "shape": [H, 1024], "voxel_size": voxel,
             "sequence": "make_path_sequence(seed=2000, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)"}
    cost = None
    for name, (knots, times) in cases.items():
        traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
        m = core.Icp(1.0e9, 0.0, voxel_size=voxel, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 22,
                     map_table_capacity=1 << 24)
        core.device_sync()
        t0 = time.perf_counter()
        n_valid, n_skipped = r.build_map(m, traj, times)
        vox, pts = m.map_size()
        build_ms = 1e3 * (time.perf_counter() - t0)
        if name == "ground_truth":
            cost = {"sweeps": n, "shape": [H, 1024], "voxel_size": voxel, "map_voxels": int(vox), "map_points": int(pts),
                    "build_wall_ms": build_ms}
            cost.update(time_score(m, repeats))
        s = m.map_score()
        table[name] = {"occupied_voxels": int(vox), "map_points": int(pts), "returns": int(n_valid), "skipped": int(n_skipped), **score_dict(s)}
        print(name, table[name], flush=True)
        m.close()
        traj.close()
    r.close()
    by_voxels = sorted(cases, key=lambda k: table[k]["occupied_voxels"])
    by_var = sorted(cases, key=lambda k: table[k]["mean_plane_var"])
    by_ent = sorted(cases, key=lambda k: table[k]["mean_entropy"])
    table["order_by_occupied_voxels"], table["order_by_mean_plane_var"], table["order_by_mean_entropy"] = by_voxels, by_var, by_ent
    return cost, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wobble_cost, table = wobble(a.repeats)
    res = {"what": "map score: cost of the pass beside export and build, the four-trajectory table of DESIGN.md 3.14 with the score (3.17)",
           "code_id": core.L.lib().ptl_code_id().decode(), "hypothesis": HYPOTHESIS,
           "cost": {"sweeps_200": cost_sweeps(a.sweeps, a.repeats), "wobble_40": wobble_cost}, "sharpness": table}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
