"""IMU deskew: what it costs and what it buys, one JSON line (profiles/r07_imu_deskew_cost.json).

  cost      forward rate with the mode off and on: the free-running batch (S sequences x n sweeps, the same sweeps for every sequence),
            the S=1 sequence runner and the fused per-call step; median of 3 runs, off and on alternated
  accuracy  the four trajectories of the issue's table (synth.make_path_sequence), KISS poses and res_poses against ground truth,
            position (m) and rotation (deg) RMSE after aligning the first pose, each mode at its own reference instant (KISS poses:
            mid-sweep for constant velocity, the filter's time at the update for IMU; res_poses: the filter's time)

python tools/imu_deskew_cost.py [--seqs 240] [--sweeps 40] [--out profiles/r07_imu_deskew_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, synth  # noqa: E402
from ptudes_lab_amd.sequence import sweep_times  # noqa: E402

KW = dict(max_range=70.0, min_range=1.0)
TRAJ = {"straight": dict(step_m=1.0), "wobble3": dict(step_m=1.0, wobble_deg=3.0),
        "wobble5_yaw0.5": dict(step_m=1.0, wobble_deg=5.0, yaw_rate=0.5),
        "ramp_yaw1_wobble5_2.5Hz": dict(step_m=0.5, ramp_sweeps=6, yaw_rate=1.0, wobble_deg=5.0, wobble_hz=2.5)}


def ends(seq, n):
    return [seq.imu_range_for_scan(k)[1] for k in range(n)]


def aligned_errors(P, G):
    A = P[0] @ np.linalg.inv(G[0])
    Ga = A @ G
    dp = P[:, :3, 3] - Ga[:, :3, 3]
    R = np.einsum("nji,njk->nik", Ga[:, :3, :3], P[:, :3, :3])
    ang = np.degrees(np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.sqrt(np.mean(np.sum(dp * dp, axis=1)))), float(np.sqrt(np.mean(ang ** 2)))


def seq_runner(seq, n, scans, imu_deskew, **over):
    r = core.SeqRunner(n, seq.H * seq.W, ends(seq, n)[-1], use_imu_prediction=True, imu_deskew=imu_deskew, **KW, **over)
    for k in range(n):
        r.upload_scan(k, scans[k])
    r.upload_imu(seq.imu[: ends(seq, n)[-1]], ends(seq, n))
    if imu_deskew:
        r.upload_sweep_times(sweep_times(seq, n))
    return r


def accuracy(n, H):
    out = {}
    for name, kw in TRAJ.items():
        seq = synth.make_path_sequence(seed=2000, n_scans=n, H=H, W=1024, **kw)
        scans = seq.scans(n)
        row = {"kwargs": kw}
        for mode in ("cv", "imu"):
            r = seq_runner(seq, n, scans, mode == "imu")
            r.run()
            o = r.results()
            g_kiss = seq.gt_poses(0.5)[:n] if mode == "cv" else seq.pose_at(o["res_t"] - seq.t_base)
            g_res = seq.pose_at(o["res_t"] - seq.t_base)
            kp, kr = aligned_errors(o["kiss_poses"], g_kiss)
            rp, rr = aligned_errors(o["res_poses"], g_res)
            row[mode] = dict(kiss_pos_rmse_m=kp, kiss_rot_rmse_deg=kr, res_pos_rmse_m=rp, res_rot_rmse_deg=rr,
                             modes=[int(m) for m in r.deskew_modes()])
            r.close()
        out[name] = row
        print(name, {m: (round(row[m]["kiss_pos_rmse_m"], 4), round(row[m]["res_pos_rmse_m"], 4)) for m in ("cv", "imu")}, flush=True)
    return out


def alternated(fn, reps=3):
    t = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            t[on].append(fn(on))
    return {"off": float(np.median(t[False])), "on": float(np.median(t[True])), "runs_off": t[False], "runs_on": t[True]}


def cost(S, n):
    seq = synth.make_path_sequence(seed=2000, n_scans=n, H=128, W=1024, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)
    scans = seq.scans(n)
    out = {}
    # S=1 sequence runner (default geometry): scans/s of run()
    runners = {on: seq_runner(seq, n, scans, on) for on in (False, True)}

    def s1(on):
        t0 = time.perf_counter()
        runners[on].run()
        return n / (time.perf_counter() - t0)
    out["seq_runner_S1_scans_per_s"] = alternated(s1)
    # (the rates include the registration's own work, which depends on the deskew: mean Gauss-Newton iterations per scan of each mode)
    out["seq_runner_S1_mean_gn_iterations"] = {("on" if on else "off"): float(np.mean([st["iterations"] for st in r.results()["stats"]]))
                                               for on, r in runners.items()}
    for r in runners.values():
        r.close()

    # fused per-call step: scans/s over the sweeps (a fresh handle pair per run)
    def percall(on):
        icp, e = core.Icp(**KW), core.Ekf()
        if on:
            e.enable_knots(64)
        t = sweep_times(seq, n)
        t0 = time.perf_counter()
        for k in range(n):
            a, b = seq.imu_range_for_scan(k)
            core.icp_ekf_step(icp, e, seq.imu[a:b], scans[k], use_imu_prediction=True, sweep=tuple(t[k]) if on else None)
        dt = time.perf_counter() - t0
        icp.close()
        e.close()
        return n / dt
    out["percall_step_scans_per_s"] = alternated(percall)

    # free-running batch: S sequences x n sweeps (the same sweeps and IMU for every sequence)
    b = core.BatchRunner(S, n, seq.H * seq.W, ends(seq, n)[-1], use_imu_prediction=True, **KW)
    for s in range(S):
        for k in range(n):
            b.upload_scan(s, k, scans[k])
        b.upload_imu(s, seq.imu[: ends(seq, n)[-1]], ends(seq, n))

    def batch(on):
        b.imu_deskew(on)
        if on:
            for s in range(S):
                b.upload_sweep_times(s, sweep_times(seq, n))
        core.device_sync()
        t0 = time.perf_counter()
        b.run()
        return S * n / (time.perf_counter() - t0)
    out[f"free_running_S{S}_x{n}_scans_per_s"] = alternated(batch)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=240)
    ap.add_argument("--sweeps", type=int, default=40)
    ap.add_argument("--acc-sweeps", type=int, default=40)
    ap.add_argument("--acc-beams", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "IMU deskew cost and accuracy (DESIGN.md 3.12)", "code_id": core.L.lib().ptl_code_id().decode(),
           "accuracy": {"sweeps": a.acc_sweeps, "beams": a.acc_beams, "trajectories": accuracy(a.acc_sweeps, a.acc_beams)},
           "cost": cost(a.seqs, a.sweeps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
