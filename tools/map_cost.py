"""The world map of a run: what its three forms cost, and what the map says about a trajectory; one JSON line
(profiles/r10_map_cost.json).

  cost      sweeps/s of building the map of n range-image sweeps (128 x 1024, voxel 0.5, ground-truth knots every 20 ms):
              three_call  TrajectoryEvaluator + MapAccumulator.update(scan): ptl_traj_poses_at -> ptl_lut_dewarp -> numpy mask -> ptl_icp_map_add
              fused       MapAccumulator.update(scan, traj): ptl_icp_map_add_posed_range
              resident    SeqRunner.build_map over sweeps that are already in HBM: ptl_seq_map_build (their upload is not timed: they
                          are there because the run registered them)
            alternated in one process, `--repeats` runs each on a fresh map handle; median and spread (max - min); the maps of the three
            forms are compared (bit-equal sorted rows).  bus_bytes_per_sweep: counted from the copies each form issues.
  sharpness occupied 0.1 m voxels of the map of a wobbling sequence (make_path_sequence wobble_deg=5, yaw_rate=0.5; 40 sweeps of
            64 x 1024) under four trajectories: ground truth, the filter's res_poses, the RTS smoothed poses, and ground truth with ONE
            pose per sweep (mid-sweep; no per-column poses).  Fewer occupied voxels = thinner walls.

python tools/map_cost.py [--sweeps 200] [--repeats 3] [--out profiles/r10_map_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd import utils as pu  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

BOUNDS = 1.5


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def sorted_rows(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def cost(n, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    H, W = seq.H, seq.W
    lut, scans = fly.synthetic_range_scans(seq)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    ev = pu.TrajectoryEvaluator(knots, time_bounds=BOUNDS)
    runner = core.SeqRunner(n, H * W, 0, with_ekf=False, scan_cols=W)
    runner.set_lut(lut)
    for k, sc in enumerate(scans):
        runner.upload_range(k, sc.range_mm)
    # column j of sweep k at t0 + (j / W)(t1 - t0): the resident form's convention.  The scans' own column stamps run the other way round
    # (ouster column order); for the comparison of the maps the per-call forms are also run once on the resident convention below.
    t0t1 = sweep_times(seq)

    def three_call(acc):
        for sc in scans:
            ev(sc)
            acc.update(sc)

    def fused(acc):
        for sc in scans:
            acc.update(sc, traj=traj)

    def resident(acc):
        acc.add_run(runner, traj, t0t1)

    forms = {"three_call": three_call, "fused": fused, "resident": resident}
    rates = {k: [] for k in forms}
    sizes = {}
    for _ in range(repeats):
        for name, fn in forms.items():
            acc = fly.MapAccumulator(lut, voxel_size=0.5)
            core.device_sync()
            t0 = time.perf_counter()
            fn(acc)
            size = acc.map_size()  # (waits for the map)
            rates[name].append(n / (time.perf_counter() - t0))
            sizes[name] = [int(v) for v in size] + [int(acc.returns)]
            acc._icp.close()
    # the three forms give one map: three_call == fused on the scans' own stamps, fused == resident on the resident convention
    a, b = fly.MapAccumulator(lut, voxel_size=0.5), fly.MapAccumulator(lut, voxel_size=0.5)
    three_call(a)
    fused(b)
    same_tf = bool(np.array_equal(sorted_rows(a.map_points()), sorted_rows(b.map_points())))
    a._icp.close()
    b._icp.close()
    a, b = fly.MapAccumulator(lut, voxel_size=0.5), fly.MapAccumulator(lut, voxel_size=0.5)
    for sc, (s0, s1) in zip(scans, t0t1):
        a._icp.map_add_posed(traj, s0 + (np.arange(W) / W) * (s1 - s0), range_mm=sc.range_mm, lut=lut)
    resident(b)
    same_fr = bool(np.array_equal(sorted_rows(a.map_points()), sorted_rows(b.map_points())))
    a._icp.close()
    b._icp.close()
    returns = sizes["fused"][2] / n
    nk = len(knots)
    bus = {
        # poses_at: knots (8 + 128 B each) and W stamps up, W poses and the outside count down; dewarp: range image and W poses up, H W points
        # and the count down; map_add: the returns up, the error word down
        "three_call": {"up": nk * 136 + W * 8 + H * W * 4 + W * 128 + returns * 24, "down": W * 128 + 4 + H * W * 24 + 4 + 4},
        # range image and W stamps up; count, flag and the error word down
        "fused": {"up": H * W * 4 + W * 8, "down": 8 + 4},
        # per CALL (all sweeps): the two totals and the error word down, nothing up
        "resident": {"up": 0, "down": (16 + 4) / n},
    }
    out = {"sweeps": n, "shape": [H, W], "voxel_size": 0.5, "knots": nk, "mean_returns_per_sweep": returns, "map_voxels_points_returns": sizes,
           "maps_bit_equal": {"three_call_vs_fused": same_tf, "fused_vs_resident": same_fr}, "bus_bytes_per_sweep": bus,
           "sweeps_per_s": {k: {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": v} for k, v in rates.items()}}
    for h in (runner, traj):
        h.close()
    return out


def sharpness(n=40, H=64, voxel=0.1):
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
    mid = np.repeat(t0t1.mean(axis=1, keepdims=True), 2, axis=1)  # t0 = t1: every column of a sweep at one instant
    gk = gt_knots(seq, n)
    cases = {"ground_truth": (gk, t0t1), "filter": (list(zip(o["res_t"], o["res_poses"])), t0t1),
             "smoothed": (list(zip(sm["t"], sm["poses"])), t0t1), "ground_truth_one_pose_per_sweep": (gk, mid)}
    out = {"sweeps": n, "shape": [H, 1024], "voxel_size": voxel, "sequence": "make_path_sequence(seed=2000, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)"}
    for name, (knots, times) in cases.items():
        traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
        m = core.Icp(1.0e9, 0.0, voxel_size=voxel, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 22,
                     map_table_capacity=1 << 24)
        n_valid, n_skipped = r.build_map(m, traj, times)
        vox, pts = m.map_size()
        out[name] = {"occupied_voxels": int(vox), "map_points": int(pts), "returns": int(n_valid), "skipped": int(n_skipped)}
        print(name, out[name], flush=True)
        m.close()
        traj.close()
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "world map of a run: cost of the three forms, map sharpness under four trajectories (DESIGN.md 3.14)",
           "code_id": core.L.lib().ptl_code_id().decode(), "cost": cost(a.sweeps, a.repeats), "sharpness": sharpness()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
