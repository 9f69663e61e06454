"""Rays cast through a saved map: what the cast of one 128 x 1024 sweep costs beside the carve of the same sweep on the same
map; one JSON line (profiles/r27_map_cast_cost.json).

Expectation, written down before the first run: NO SLOWER THAN THE CARVE PER SWEEP.  The carve (`Carver.add_posed`) is the
existing march: it runs every ray to its measured end and votes with one atomic per near point.  The cast uses the same half-wave-per-ray
march over the same samples but stops a ray after the round of 32 samples that holds its first hit, and issues no per-point atomics; against
that it marches the rays WITHOUT a hit to max_range (60 m here, beyond most measured ends) and keeps a five-word best per lane.  So the larger
the share of rays that hit (the radius drives it: vs / 10, vs / 5, vs / 2 are measured), the further the cast should be ahead.  The carve's
own measurement (profiles/r20_map_carve_cost.json) found the half-wave mapping bound by instruction issue, not by the probes: the early exit
removes issue slots, which is why it should show.  Nobody has measured this; whatever the run says is written beside this text, and DESIGN.md
3.30 carries the correction if it disagrees.

  workload  the seed-1000 synthetic sequence of `--sweeps` sweeps of 128 x 1024 (bench.py's default workload) as range images with their LUT,
            ground-truth knots, one map at 0.5 m of all of them (the per-call posed path).  `--cast-sweeps` of them, evenly spread, are timed.
  timing    per radius a Caster and a Carver on that map.  Both forms alternate in one process, sweep by sweep; `--repeats` rounds after one
            warm-up round; per round the HIP-event ms per sweep of each form (upload of the sweep, column table, the march - the same span in
            both handles; the carve's figure also holds one summary reduction per round, a single launch); median and spread (max - min).

python tools/map_cast_cost.py [--sweeps 100] [--cast-sweeps 10] [--repeats 5] [--out profiles/r27_map_cast_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402

BOUNDS = 1.5
VS = 0.5
EXPECTATION = ("no slower than the carve per sweep: the same half-wave march, but a ray stops after the round of its first hit and no per-point "
               "atomics are issued; rays without a hit go on to max_range, so the advantage should grow with the share of rays that hit (radius)")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def carve_device_ms(car):
    """the carve handle's device time so far, by a read of the summary alone (no per-point arrays: one reduction launch)"""
    res = core.L.CarveResult()
    core.L.check(core.L.lib().ptl_carve_read(car._h, C.byref(res), None, None, None, 0, None))
    return float(res.device_ms), res


def cost(n, n_cast, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    lut, scans = fly.synthetic_range_scans(seq)
    m = core.Icp(1.0e9, 0.0, voxel_size=VS, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                 map_table_capacity=1 << 23)
    for s in scans:
        m.map_add_posed(traj, np.asarray(s.timestamp, dtype=np.float64) * 1e-9, range_mm=s.range_mm, lut=lut)
    picked = [scans[i] for i in np.linspace(0, n - 1, n_cast).round().astype(int)]
    ts = [np.asarray(s.timestamp, dtype=np.float64) * 1e-9 for s in picked]
    out = {"sweeps_in_map": n, "sweeps_timed": len(picked), "shape": [seq.H, seq.W], "voxel_size": VS, "map_size": list(m.map_size()), "radii": {}}
    for name, radius in (("vs/10", VS / 10.0), ("vs/5", VS / 5.0), ("vs/2", VS / 2.0)):
        cas = core.Caster(m, radius=radius)
        cast_ms, carve_ms, counts = [], [], None
        for rep in range(repeats + 1):  # (round 0: code object load, first touch)
            car = core.Carver(m, radius=radius)
            before, _ = carve_device_ms(car)
            c_ms, counts = 0.0, dict(n_hit=0, n_miss=0, n_no_return=0, n_degenerate=0, n_voxel_visits=0)
            for s, t in zip(picked, ts):  # the two forms alternate sweep by sweep
                sw = cas.cast_range(traj, lut, s.range_mm, t)
                c_ms += sw.result["device_ms"]
                for k in counts:
                    counts[k] += sw.result[k]
                car.add_posed(traj, t, range_mm=s.range_mm, lut=lut)
            after, res = carve_device_ms(car)
            car.close()
            if rep:
                cast_ms.append(c_ms / len(picked)); carve_ms.append((after - before) / len(picked))
        cast_rays = counts["n_hit"] + counts["n_miss"]
        out["radii"][name] = {
            "radius": radius, "cast": {k: float(getattr(cas.cfg, k)) for k in ("radius", "step", "min_range", "max_range")},
            "carve": {k: float(getattr(res, k)) for k in ("radius", "margin", "step", "min_range", "max_range")},
            "cast_device_ms_per_sweep": stat(cast_ms), "carve_device_ms_per_sweep": stat(carve_ms),
            "cast_over_carve": float(np.median(cast_ms) / np.median(carve_ms)),
            "hit_share_of_cast_rays": counts["n_hit"] / max(cast_rays, 1),
            "per_sweep": {"cast_rays": cast_rays / len(picked), "cast_voxel_visits_in_map": counts["n_voxel_visits"] / len(picked),
                          "carve_rays": res.n_rays / len(picked), "carve_voxel_visits_in_map": res.n_voxel_visits / len(picked),
                          "carve_atomics": (res.sum_through + res.sum_support) / len(picked)}}
        print(name, json.dumps(out["radii"][name]), flush=True)
        cas.close()
    for h in (m, lut, traj):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--cast-sweeps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "rays cast through a saved map: HIP-event ms per 128 x 1024 sweep of Caster.cast_range beside Carver.add_posed of the same sweep "
                   "on the same map, at three radii (DESIGN.md 3.30)",
           "code_id": core.L.lib().ptl_code_id().decode(), "expectation_before_the_run": EXPECTATION}
    res.update(cost(a.sweeps, a.cast_sweeps, a.repeats))
    res["expectation_held"] = all(r["cast_over_carve"] <= 1.0 for r in res["radii"].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
