"""The cases of tests/test_gpu_search_chain_diag.py, run on whatever library PTL_LIB_PATH names: as a program it prints one JSON line.
  scene   the two scans of tests/helpers/search_chain_scenes.py as a batch of two on teams of two workgroups
  bench   10 sweeps of the benchmark's sequence of seed 1000 (IMU prediction, filter on) on a team of two"""
import json
import os
import sys

import numpy as np


def run_case(name):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core, synth
    from tests.helpers import search_chain_scenes as sc
    out = dict(build=core.build_info()["diagnostics"], members=[])
    if name == "scene":
        S = 2
        b = core.BatchRunner(S, 2, sc.N, 0, team_workgroups=2, max_range=sc.MAX_RANGE, min_range=sc.MIN_RANGE, with_ekf=False,
                             max_points_per_scan=sc.N, **sc.ICP)
        for s in range(S):
            b.upload_scan(s, 0, sc.frame0())
            b.upload_scan(s, 1, sc.frame1())
            b.upload_imu(s, np.zeros((0, 7)), [0, 0])
    else:
        S, n = 1, 10
        sq = synth.make_sequence(seed=1000, n_scans=n)
        n_imu = sq.imu_range_for_scan(n - 1)[1]
        b = core.BatchRunner(S, n, sq.H * sq.W, n_imu, use_imu_prediction=True, with_ekf=True, team_workgroups=2)
        for k in range(n):
            b.upload_scan(0, k, sq.scan(k))
        b.upload_imu(0, sq.imu[:n_imu], [sq.imu_range_for_scan(k)[1] for k in range(n)])
    b.run()
    assert b.status() == 0 and b.team_geometry()[0] == 2
    for s in range(S):
        res = b.results(s)
        out["members"].append(dict(diag=b.diag(s), exec=b.exec_counters(s), stats=res["stats"], kiss=np.ascontiguousarray(res["kiss_poses"]).tobytes().hex()))
    b.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    print("SEARCH_CHAIN_CASE " + json.dumps(run_case(sys.argv[1])))
