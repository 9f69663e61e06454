"""Free space carved: what the second pass over a map's sweeps costs per 128 x 1024 sweep, beside the pass whose input it
re-reads; one JSON line (profiles/r20_map_carve_cost.json).

Expectation, written down before the first run: the table probes bound the pass, as they bound the Gauss-Newton search (a
dependent random line costs microseconds under load, about 48 G lines/s at best).  A ray of the synthetic room is some 10 - 30 m long: at a
step of 0.25 m that is 40 - 120 samples, about half as many distinct voxels, each one map_find - against ONE insert per return in the map
build.  Nearly all of those voxels are empty air, so a probe ends at the first empty slot of its home line; consecutive voxels of a ray share
2 x 2 x 2 bricks (one line per brick) and neighbouring rays share most of their voxels near the sensor, so L2 should serve the larger part.
The carve pass should therefore cost a small multiple of the map build per sweep (the build also compacts, inserts and allocates), and the
half-wave-per-ray mapping should beat one lane per ray clearly, because the latter walks its probes as a dependent chain.  No rate is fixed
in advance; whatever the run says is written beside this text, and DESIGN.md 3.24 carries the correction if it disagrees.
Correction after the first run (profiles/r20_map_carve_cost.json): wrong on all three counts.  The pass costs twenty builds per
sweep, the probes (6.5 G/s, mostly misses the Infinity Cache serves) do not bound it - instruction issue does - and one lane per ray is 3.4 x
faster than a half-wave per ray, which repeats a ray's set-up in 32 lanes and walks a found voxel's points in one.

  cost     the seed-1000 synthetic sequence of `--sweeps` sweeps of 128 x 1024 (bench.py's default workload: seed base 1000), resident in a
           SeqRunner, ground-truth knots, map at 0.5 m.  Alternated in one process, `--repeats` rounds after one warm-up round:
             build   SeqRunner.build_map into a fresh handle: wall ms around a call that ends in a device synchronise, per sweep
             carve   Carver.add_run over the same resident sweeps against the first map: the result's HIP-event ms, and the wall ms, per sweep
           median and spread (max - min).  Voxel visits and atomics (through + support votes) per sweep from the summary.
  lanes    `--other-lib PATH`: the same measurement in a child process that loads a library built with one lane per ray
           (make -C ptudes-lab_amd/csrc OUT=libptudes_mi_lane1.so EXTRA=-DCARVE_LANES=1); its votes must equal this library's
  flagged  what the policy flags on this STATIC scene (nothing moves in it: every flagged point is a false positive of the definition at
           these parameters), recorded, not asserted

python tools/map_carve_cost.py [--sweeps 40] [--repeats 5] [--other-lib PATH] [--out profiles/r20_map_carve_cost.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, synth  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

BOUNDS = 1.5
EXPECTATION = ("bound by the table probes (DESIGN.md 3.9), most of them misses served by L2; a small multiple of the map build per sweep; the "
               "half-wave-per-ray mapping clearly ahead of one lane per ray, whose probes form a dependent chain")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def new_map(seq):
    return core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                    map_table_capacity=1 << 23)


def cost(n, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(n):
        runner.upload_scan(k, seq.scan(k))
    t0t1 = sweep_times(seq)
    m = new_map(seq)
    runner.build_map(m, traj, t0t1)
    build_wall, carve_dev, carve_wall = [], [], []
    votes = None
    for rep in range(repeats + 1):  # (round 0: code object load, first touch)
        fresh = new_map(seq)
        core.device_sync()
        t0 = time.perf_counter()
        runner.build_map(fresh, traj, t0t1)
        bw = 1e3 * (time.perf_counter() - t0) / n
        fresh.close()
        car = core.Carver(m)
        before = car.votes().device_ms  # (the prefixes of create and this read's reduction)
        core.device_sync()
        t0 = time.perf_counter()
        car.add_run(runner, traj, t0t1)
        cw = 1e3 * (time.perf_counter() - t0) / n
        votes = car.votes()
        cd = (votes.device_ms - before) / n  # (includes the second read's reduction: one launch over the votes)
        car.close()
        if rep:
            build_wall.append(bw); carve_dev.append(cd); carve_wall.append(cw)
    dyn = votes.dynamic()
    # (block ids are handed out in the order the build's workgroups ask for them: rows are sorted before two processes' votes are compared)
    rows = np.column_stack([votes.xyz, votes.through.astype(np.float64), votes.support.astype(np.float64)])
    digest = hashlib.sha256(np.ascontiguousarray(rows[np.lexsort(rows.T[::-1])]).tobytes()).hexdigest()[:16]
    out = {"sweeps": n, "shape": [seq.H, seq.W], "voxel_size": 0.5, "map_size": list(m.map_size()),
           "parameters": {k: getattr(votes, k) for k in ("radius", "margin", "step", "min_range", "max_range")},
           "build_wall_ms_per_sweep": stat(build_wall), "carve_device_ms_per_sweep": stat(carve_dev), "carve_wall_ms_per_sweep": stat(carve_wall),
           "per_sweep": {"rays": votes.n_rays / n, "voxel_visits_in_map": votes.n_voxel_visits / n,
                         "atomics": (votes.sum_through + votes.sum_support) / n},
           "summary": {k: getattr(votes, k) for k in ("n_points", "n_scans", "n_scans_skipped", "n_rays", "n_rays_out_of_range", "n_no_return",
                                                      "n_voxel_visits", "n_points_through", "n_points_supported", "sum_through", "sum_support")},
           "flagged_on_a_static_scene": {"policy": "through >= 2 and through >= 0.5 (through + support)", "points": int(dyn.sum()),
                                         "of": int(len(dyn))},
           "votes_sha256_16": digest}
    for h in (m, runner, traj):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="a library built with EXTRA=-DCARVE_LANES=1: measured in a child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    res = {"what": "free space carved: device and wall ms per 128 x 1024 sweep beside the map build of the same sweeps, voxel visits and "
                   "atomics per sweep, half-wave per ray against one lane per ray (DESIGN.md 3.24)",
           "code_id": core.L.lib().ptl_code_id().decode(), "expectation_before_the_run": EXPECTATION, "half_wave_per_ray": cost(a.sweeps, a.repeats)}
    if a.child:
        print("CHILD " + json.dumps(res["half_wave_per_ray"]), flush=True)
        return
    print(json.dumps(res["half_wave_per_ray"]), flush=True)
    if a.other_lib:
        env = dict(os.environ, PTL_LIB_PATH=os.path.abspath(a.other_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweeps", str(a.sweeps), "--repeats", str(a.repeats), "--child"],
                           env=env, capture_output=True, text=True, timeout=900)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
        if p.returncode != 0 or not line:
            raise SystemExit(f"the one-lane-per-ray run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        res["one_lane_per_ray"] = json.loads(line[0][6:])
        res["same_votes"] = res["one_lane_per_ray"]["votes_sha256_16"] == res["half_wave_per_ray"]["votes_sha256_16"]
        res["one_lane_over_half_wave"] = (res["one_lane_per_ray"]["carve_device_ms_per_sweep"]["median"]
                                          / res["half_wave_per_ray"]["carve_device_ms_per_sweep"]["median"])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
