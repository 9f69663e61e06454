"""The map distance: what the pass costs per million queries, the lines it must touch, and the experiment DESIGN.md 3.14 left
open; one JSON line (profiles/r19_map_compare_cost.json).

Hypothesis, written down before the first run: the pass is bound by the random-line rate of DESIGN.md 3.9 (about 48 G lines/s), not by
arithmetic (a few dozen fp64 operations per stored point met) and not by the bus (the pool source moves nothing, the array source 24 bytes
per query).  Per query it must touch the table lines of 27 probes (2 x 2 x 2 bricks: at most 8 lines), one 16-byte directory word per occupied
neighbour and ceil(24 count / 128) point lines of each; neighbouring queries share most of them, so L2 should serve the larger part and the
time per million queries should lie well below (lines per query) x 10^6 / 48 G.  The map score of the same map gathers the same 27 voxels per
VOXEL (staged once in LDS for all its points) and then does far more arithmetic per pair: the yardstick.

  cost      the seed-1000 synthetic map of `--sweeps` sweeps at 0.5 m (range images, ground-truth knots: tools/render_cost.py's map) against the
            map the same ground-truth poses make of the same sweeps' xyz points.  Three forms alternated in one process, `--repeats` rounds after
            one warm-up round, HIP-event milliseconds (the result's device_ms), median and spread (max - min), per million queries:
              array   Icp.map_distance(map_points()): staged chunks of 2^17 queries (the wall time beside it: the bus and the host loop)
              pool    Icp.map_compare(map): the stored points walked on the device
              score   Icp.map_score() of the same map
  lines     counted from the code on a sample of the queries: probes, occupied neighbours (directory words) and point lines per query
  sharpness the 40-sweep wobble sequence of tools/map_cost.py / tools/map_score_cost.py at `--voxel` m: precision, recall and F at 0.05, 0.1 and
            0.2 m against the ground-truth map for the filter's map, the smoothed map and the one-pose-per-sweep map

python tools/map_compare_cost.py [--sweeps 100] [--repeats 7] [--voxel 0.2] [--out profiles/r19_map_compare_cost.json]"""
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
RANDOM_LINES_PER_S = 48.0e9
THRESHOLDS = (0.05, 0.1, 0.2)
HYPOTHESIS = ("bound by the random-line rate (DESIGN.md 3.9), not by arithmetic or the bus; L2 serves the lines neighbouring queries share, so "
              "the time per million queries lies well below lines-per-query x 1e6 / 48 G lines/s")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def dist_dict(d):
    return {"n_query": d.n_query, "n_matched": d.n_matched, "n_within": list(d.n_within), "mean_mm": 1e3 * d.mean_dist, "rms_mm": 1e3 * d.rms_dist}


def lines_per_query(ref_pts, queries, vs, sample=20000, seed=0):
    """what one query must touch, counted the way compare_kernels.h reads: 27 probes, one directory word per occupied neighbour voxel, and
    ceil(24 count / 128) lines of each one's points (a block starts on a line)"""
    off = 1 << 20
    key = lambda k: ((k[:, 0] + off) << 42) | ((k[:, 1] + off) << 21) | (k[:, 2] + off)  # noqa: E731
    keys, counts = np.unique(key(np.trunc(ref_pts / vs).astype(np.int64)), return_counts=True)
    rng = np.random.default_rng(seed)
    q = queries[rng.choice(len(queries), size=min(sample, len(queries)), replace=False)]
    k = np.trunc(q / vs).astype(np.int64)
    occupied, point_lines, points = np.zeros(len(q)), np.zeros(len(q)), np.zeros(len(q))
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                kk = key(k + np.array([dx, dy, dz]))
                pos = np.minimum(np.searchsorted(keys, kk), len(keys) - 1)
                hit = keys[pos] == kk
                c = np.where(hit, counts[pos], 0)
                occupied += hit
                points += c
                point_lines += np.ceil(c * 24 / 128)
    return {"sample": len(q), "probes": 27, "table_lines_at_most": 8, "occupied_neighbours": float(occupied.mean()),
            "point_lines": float(point_lines.mean()), "stored_points_met": float(points.mean()),
            "lines_per_query": float(8 + occupied.mean() / 8 + point_lines.mean())}  # (eight 16-byte directory words share a line)


def cost(n, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    lut, scans = fly.synthetic_range_scans(seq)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    runner.set_lut(lut)
    for k, sc in enumerate(scans):
        runner.upload_range(k, sc.range_mm)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    acc.add_run(runner, traj, sweep_times(seq))
    runner.close()
    # the reference: the same poses over the sweeps' xyz points
    r2 = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(n):
        r2.upload_scan(k, seq.scan(k))
    ref = core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                   map_table_capacity=1 << 23)
    r2.build_map(ref, traj, sweep_times(seq))
    r2.close()
    traj.close()
    m = acc.icp
    pts = m.map_points()
    nq = len(pts)
    dev = {"array": [], "pool": [], "score": []}
    wall = {"array": [], "pool": [], "score": []}
    last = {}
    for rep in range(repeats + 1):  # (round 0: code object load, first touch)
        for form in ("array", "pool", "score"):
            core.device_sync()
            t0 = time.perf_counter()
            if form == "array":
                r = ref.map_distance(pts, thresholds=THRESHOLDS)
            elif form == "pool":
                r = ref.map_compare(m, thresholds=THRESHOLDS)
            else:
                r = m.map_score()
            w = 1e3 * (time.perf_counter() - t0)
            if rep:
                dev[form].append(r.device_ms * 1e6 / nq)
                wall[form].append(w * 1e6 / nq)
            last[form] = r
    assert last["array"].n_within == last["pool"].n_within and last["array"].n_matched == last["pool"].n_matched
    lines = lines_per_query(ref.map_points(), pts, 0.5)
    floor_ms = lines["lines_per_query"] * 1e6 / RANDOM_LINES_PER_S * 1e3
    out = {"sweeps": n, "voxel_size": 0.5, "queries": nq, "map_size": list(m.map_size()), "reference_size": list(ref.map_size()),
           "device_ms_per_million_queries": {k: stat(v) for k, v in dev.items()}, "wall_ms_per_million_queries": {k: stat(v) for k, v in wall.items()},
           "accuracy": dist_dict(last["pool"]), "lines": lines, "ms_per_million_queries_if_every_line_came_from_hbm_at_the_random_line_rate": floor_ms}
    for h in (acc, ref):
        h.close()
    return out


def sharpness(voxel, n=40, H=64):
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
    # the ground truth in the filter's frame (the filter starts at the identity, the sequence anywhere): both trajectories agree at the first
    # corrected pose - a known rigid transform, not a registration of the clouds
    t_first = float(o["res_t"][0])
    to_filter = np.asarray(o["res_poses"][0]) @ np.linalg.inv(seq.pose_at(np.array([t_first - seq.t_base]))[0])
    gk = [(t, to_filter @ p) for t, p in gt_knots(seq, n)]
    cases = {"ground_truth": (gk, t0t1), "filter": (list(zip(o["res_t"], o["res_poses"])), t0t1),
             "smoothed": (list(zip(sm["t"], sm["poses"])), t0t1), "ground_truth_one_pose_per_sweep": (gk, mid)}
    table = {"sweeps": n, "shape": [H, 1024], "voxel_size": voxel, "max_dist": min(voxel, max(THRESHOLDS)), "thresholds": list(THRESHOLDS),
             "sequence": "make_path_sequence(seed=2000, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)"}
    maps = {}
    for name, (knots, times) in cases.items():
        traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
        m = core.Icp(1.0e9, 0.0, voxel_size=voxel, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 22,
                     map_table_capacity=1 << 24)
        r.build_map(m, traj, times)
        traj.close()
        maps[name] = m
    thr = [t for t in THRESHOLDS if t <= voxel]
    for name in ("filter", "smoothed", "ground_truth_one_pose_per_sweep", "ground_truth"):
        c = fly.compare_maps(maps[name], maps["ground_truth"], thresholds=thr, max_dist=table["max_dist"])
        table[name] = {"occupied_voxels": int(maps[name].map_size()[0]), "map_points": int(maps[name].map_size()[1]),
                       "precision": list(c.precision), "recall": list(c.recall), "f_score": list(c.f_score),
                       "accuracy": dist_dict(c.accuracy), "completeness": dist_dict(c.completeness),
                       "score_thickness_mm": maps[name].map_score().thickness_mm}
        print(name, table[name], flush=True)
    for m in maps.values():
        m.close()
    r.close()
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "map distance: device ms per million queries (array source, pool source, map score), lines per query, and the "
                   "four-trajectory experiment of DESIGN.md 3.14 as precision / recall / F (3.23)",
           "code_id": core.L.lib().ptl_code_id().decode(), "hypothesis": HYPOTHESIS, "cost": cost(a.sweeps, a.repeats)}
    print(json.dumps(res["cost"]), flush=True)
    res["sharpness"] = sharpness(a.voxel)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
