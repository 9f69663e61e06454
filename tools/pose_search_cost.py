"""The pose search: what scoring K candidate poses x n query points costs on the device, next to the existing path the bus
feeds, and where the time of one full localisation goes; one JSON line (profiles/r23_pose_search_cost.json).

Nobody had measured any of this before the first run of this tool; no figure of it is asserted anywhere.  Expectation written down before
that run: per candidate-point the pass does what the map distance does per query (27 probes side by side in a half-wave) plus twelve
multiply-adds, so its device time per candidate-point should be close to the map distance's per query - and it moves K x 128 + n x 24 bytes over
the bus where the map distance moves K x n x 24.  With few candidates (K = 64) only K of the device's 256 compute units have a workgroup: the
time per candidate-point should then be several times the large-K figure.

  map       the seed-1000 synthetic 128 x 1024 run of `--sweeps` sweeps at 0.5 m, as `ekf-bench ouster --synthetic 1000 --save-map` builds it
            (cli.ekf_bench._run_map_handle: the resident sweeps, every column at its own pose), under ground-truth knots
  poses     K = 16 yaws x K / 16 keyframes taken evenly along the ground-truth trajectory (fly.candidate_poses)
  points    n points of the last sweep, thinned to one per 0.5 m voxel (fly.MapLocalizer.query), a seeded choice of n of them
  search    Icp.pose_hits(points, poses): HIP-event milliseconds of the call (staging copies included), the wall time beside it
  distance  Icp.map_distance on the same K x n points, transformed on the host in the written order (numpy, not timed): the existing path.
            At K = 36 864, n = 2 048 that array is 75 M x 3 doubles, 1.8 GB, with temporaries of that size while it is made: the host needs
            about 8 GB free
  Both forms alternate in one process, `--repeats` rounds after one warm-up round; median and spread (max - min).  For K = 64 every
  candidate's hits are checked against the map distance's n_within on the way.
  locate    one fly.MapLocalizer.locate over 4 096 candidates at the defaults, split: search (device), align (wall: the `top` refinements
            end in a synchronising copy each), rescore (device), and the wall time of thinning the sweep (`query`: a scratch map per sweep)

python tools/pose_search_cost.py [--sweeps 100] [--repeats 5] [--out profiles/r23_pose_search_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd.cli.ekf_bench import _run_map_handle  # noqa: E402

KS = (64, 4096, 36864)
NS = (256, 2048)
N_YAW = 16
VOXEL = 0.5
EXPECTATION = ("device time per candidate-point close to the map distance's per query (the same 27 probes, twelve multiply-adds more), with "
               "K x 128 + n x 24 bytes over the bus instead of K x n x 24; at K = 64 only 64 of 256 compute units have a workgroup, so several "
               "times the large-K time per candidate-point")


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def transform_all(q, poses):
    """(K n, 3): every point of q (n, 3) under every pose (K, 4, 4), candidate-major, in the written order"""
    x, y, z = q[None, :, 0], q[None, :, 1], q[None, :, 2]
    P = poses[:, :, :, None]
    return np.stack([((P[:, r, 0] * x + P[:, r, 1] * y) + P[:, r, 2] * z) + P[:, r, 3] for r in range(3)], axis=2).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_sweeps = a.sweeps
    seq = synth.make_sequence(seed=1000, n_scans=n_sweeps)
    kt = np.arange(0, n_sweeps * seq.scan_dt + 0.3, 0.02)
    knots = [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]
    m, n_skipped = _run_map_handle(seq, 0, knots, VOXEL, 0)
    loc = fly.MapLocalizer(m, [np.eye(4)], n_yaw=1, query_voxel=VOXEL)
    query = loc.query(seq.scan(n_sweeps - 1))
    query = query[np.random.default_rng(0).permutation(len(query))]
    assert len(query) >= max(NS), (len(query), max(NS))
    res = {"what": "pose search: device ms and candidate-points per second of Icp.pose_hits for K candidates x n points, the map distance on "
                   "the same K x n transformed points beside it, and one full locate split into search, align and rescore (DESIGN.md 3.26)",
           "code_id": core.L.lib().ptl_code_id().decode(), "expectation_before_the_first_run": EXPECTATION, "sweeps": n_sweeps,
           "voxel_size": VOXEL, "map_size": list(m.map_size()), "sweeps_skipped": int(n_skipped), "thinned_sweep_points": len(query),
           "pose_chunk": core.build_info()["pose_chunk"], "n_yaw": N_YAW, "cases": []}
    for K in KS:
        times = np.linspace(0.0, (n_sweeps - 1) * seq.scan_dt, K // N_YAW)
        poses, _ = fly.candidate_poses(seq.pose_at(times), N_YAW)
        for n in NS:
            q = np.ascontiguousarray(query[:n])
            world = transform_all(q, poses)  # what the existing path needs from the bus
            dev = {"search": [], "distance": []}
            wall = {"search": [], "distance": []}
            for rep in range(a.repeats + 1):  # (round 0: code object load, first touch)
                for form in ("search", "distance"):
                    core.device_sync()
                    t0 = time.perf_counter()
                    if form == "search":
                        s, hits = m.pose_hits(q, poses)
                        ms = s.device_ms
                    else:
                        d = m.map_distance(world)
                        ms = d.device_ms
                    w = 1e3 * (time.perf_counter() - t0)
                    if rep:
                        dev[form].append(ms)
                        wall[form].append(w)
            assert int(hits[:, 0].astype(np.int64).sum()) == d.n_within[0], "the two paths count the same pairs"
            if K == 64:
                for k in range(K):
                    assert hits[k, 0] == m.map_distance(world[k * n:(k + 1) * n]).n_within[0], k
            case = {"K": K, "n": n, "candidate_points": K * n, "device_ms": {f: stat(v) for f, v in dev.items()},
                    "wall_ms": {f: stat(v) for f, v in wall.items()},
                    "candidate_points_per_second": {f: K * n / (1e-3 * float(np.median(v))) for f, v in dev.items()},
                    "bus_bytes": {"search": K * 128 + n * 24 + K * 4, "distance": K * n * 24},
                    "best_pose": int(s.best_pose[0]), "best_hits": int(s.best_hits[0])}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del world
    loc.close()
    times = np.linspace(0.0, (n_sweeps - 1) * seq.scan_dt, 4096 // N_YAW)
    loc = fly.MapLocalizer(m, seq.pose_at(times), n_yaw=N_YAW)
    loc.locate(seq.scan(n_sweeps - 1))  # (warm-up)
    rounds = []
    for _ in range(a.repeats):
        loc.search_ms = loc.align_ms = loc.rescore_ms = loc.query_ms = 0.0
        core.device_sync()
        t0 = time.perf_counter()
        fix = loc.locate(seq.scan(n_sweeps - 1))
        rounds.append({"wall_ms": 1e3 * (time.perf_counter() - t0), "search_device_ms": loc.search_ms, "align_wall_ms": loc.align_ms,
                       "rescore_device_ms": loc.rescore_ms, "query_wall_ms": loc.query_ms})
    truth = seq.gt_poses(0.5)[n_sweeps - 1]
    res["locate"] = {"candidates": len(loc.candidates), "top": loc.top, "query_voxel": loc.query_voxel, "n_query": fix.n_query,
                     "sigma": loc.sigma, "rounds": rounds, "median": {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]},
                     "candidate": fix.candidate, "fraction": fix.fraction, "runner_up_hits": fix.runner_up_hits, "iterations": fix.iterations,
                     "translation_from_ground_truth_m": float(np.linalg.norm(fix.pose[:3, 3] - truth[:3, 3]))}
    loc.close()
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
