#!/usr/bin/env python3
"""What the fixed-interval RTS smoother costs on bench.py's default workload: 240 synthetic 128x1024 sequences (seeds 1000 + s), the
free-running driver, IMU prediction on.

  1. forward scans/s with the filter's history log off against on (the same handle, runs alternated, median of --repeats)
  2. ptl_batch_smooth: one launch smoothing 240 x N logged updates (wall time of the call, median of --repeats)
  3. the log's bytes (8 KB per update) and the backward pass's output rows

    python tools/smoother_cost.py --scans 40 --repeats 3 --out profiles/r07_smoother_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ptudes_lab_amd import core, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sequences", type=int, default=240)
    ap.add_argument("--scans", type=int, default=40, help="sweeps per sequence (every one resident, like bench.py)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    S, n = a.sequences, a.scans
    seqs = [synth.make_sequence(seed=1000 + s, n_scans=n) for s in range(S)]
    n_imu = seqs[0].imu_range_for_scan(n - 1)[1]
    b = core.BatchRunner(S, n, seqs[0].H * seqs[0].W, n_imu, use_imu_prediction=True, with_ekf=True, free_running=True)
    t0 = time.perf_counter()
    for s, sq in enumerate(seqs):
        for k in range(n):
            b.upload_scan(s, k, sq.scan(k))
        b.upload_imu(s, sq.imu[:n_imu], [sq.imu_range_for_scan(k)[1] for k in range(n)])
    print(f"{S} sequences x {n} sweeps rendered and uploaded in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def forward():
        t = time.perf_counter()
        b.run()
        return time.perf_counter() - t

    b.run()  # warm-up (first launch, code load)
    ref = [b.results(s)["res_poses"] for s in range(S)]
    t_off, t_on, t_smooth = [], [], []
    for _ in range(a.repeats):
        b.enable_smoother(False)
        t_off.append(forward())
        b.enable_smoother(True)
        t_on.append(forward())
        for s in (0, S - 1):
            assert np.array_equal(b.results(s)["res_poses"], ref[s]), "the log changed a forward result"
        for _ in range(1):
            t = time.perf_counter()
            b.smooth()
            t_smooth.append(time.perf_counter() - t)
    rows = sum(len(b.smoothed(s, nav=False, cov=False)["t"]) for s in range(S))
    med = statistics.median
    scans = S * n
    res = dict(
        workload=f"{S} sequences x {n} synthetic 128x1024 sweeps, free-running driver, use_imu_prediction",
        scans_per_run=scans,
        forward_s_log_off=t_off, forward_s_log_on=t_on,
        scans_per_s_log_off=scans / med(t_off), scans_per_s_log_on=scans / med(t_on),
        log_on_over_off=med(t_on) / med(t_off),
        smooth_s=t_smooth, smooth_ms_median=1e3 * med(t_smooth), smoothed_rows=rows,
        smooth_us_per_row_per_sequence=1e6 * med(t_smooth) / max(rows / S, 1),
        log_bytes_per_update=1024 * 8, log_bytes_total=S * n * 1024 * 8,
        smoother_output_bytes_total=S * n * 360 * 8,
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
