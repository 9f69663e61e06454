"""One case of tests/test_gpu_diag_build.py: the default synthetic sequence, 4 scans, filter on, run on whatever library PTL_LIB_PATH names (the
product library when unset).  `run_case(name)` returns plain JSON-able values (floating-point arrays as hex of their bytes: compared bit for
bit across processes); as a program it prints them as one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

N = 4
CASES = {
    "a": dict(runner="batch", S=2, team=32, kw={}),                    # teams of 32: per-workgroup words [0, 64) met the fixed slots 40 .. 63
    "b": dict(runner="batch", S=3, team=2, kw=dict(gn_workgroups=32)),   # 2 x 32 words allocated: the fixed slots 64 .. 70 lay behind them
    "c": dict(runner="seq", kw=dict(gn_workgroups=8, gn_lanes_per_point=8, gn_threads=512)),  # 16 words allocated
}


def _hex(a):
    return np.ascontiguousarray(a).tobytes().hex()


def _member(core, L, h, res):
    wc = (C.c_int64 * 1024)()
    L.check(L.lib().ptl_icp_gn_wg_clocks(h, wc, 512))
    return dict(kiss=_hex(res["kiss_poses"]), res=_hex(res["res_poses"]), stats=res["stats"], diag=core._diag(h), wg_clocks=[int(v) for v in wc])


def run_case(name):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import _lib as L, core, synth
    case = CASES[name]
    S = case.get("S", 1)
    seqs = [synth.make_sequence(seed=1000 + s, n_scans=N) for s in range(S)]
    n_imu = seqs[0].imu_range_for_scan(N - 1)[1]
    ends = lambda sq: [sq.imu_range_for_scan(k)[1] for k in range(N)]  # noqa: E731
    out = dict(build=core.build_info()["diagnostics"], gn_workgroups=None, members=[])
    if case["runner"] == "batch":
        b = core.BatchRunner(S, N, seqs[0].H * seqs[0].W, n_imu, use_imu_prediction=True, with_ekf=True, free_running=True,
                             team_workgroups=case["team"], **case["kw"])
        for s, sq in enumerate(seqs):
            for k in range(N):
                b.upload_scan(s, k, sq.scan(k))
            b.upload_imu(s, sq.imu[:n_imu], ends(sq))
        b.run()
        out["team"] = b.team_geometry()[0]
        out["gn_workgroups"] = int(b.cfg.icp.gn_workgroups)
        for s in range(S):
            h = C.c_void_p()
            L.check(L.lib().ptl_batch_icp(b._h, s, C.byref(h)))
            m = _member(core, L, h, b.results(s))
            m["exec"] = b.exec_counters(s)
            out["members"].append(m)
        L.check(L.lib().ptl_batch_reset(b._h))  # a cold start clears the slots with the rest of the state
        for s in range(S):
            out["members"][s]["diag_after_cold_start"] = b.diag(s)
        b.close()
    else:
        sq = seqs[0]
        r = core.SeqRunner(N, sq.H * sq.W, n_imu, use_imu_prediction=True, with_ekf=True, **case["kw"])
        for k in range(N):
            r.upload_scan(k, sq.scan(k))
        r.upload_imu(sq.imu[:n_imu], ends(sq))
        r.run()
        out["team"] = out["gn_workgroups"] = int(r.cfg.icp.gn_workgroups)
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        m = _member(core, L, h, r.results())
        # the linear system of some points against the map the run left, twice, with the slots read in between
        q = np.ascontiguousarray(sq.scan(N - 1).reshape(-1, 3)[::37][:1500], dtype=np.float64)
        lin = []
        for _ in range(2):
            sums, nc, cand = np.empty(27), C.c_int64(), C.c_int64()
            L.check(L.lib().ptl_icp_linear_system(h, L.dptr(q), len(q), 2.0, 0.5, L.dptr(sums), C.byref(nc), C.byref(cand)))
            lin.append([_hex(sums), nc.value, cand.value])
            m.setdefault("diag_after_lin", []).append(core._diag(h))
        dbg = (C.c_double * 32)()
        L.check(L.lib().ptl_icp_debug_sums(h, dbg))
        m["lin"], m["lin_kept"] = lin, [_hex(np.array(dbg[:27])), int(dbg[27]), int(dbg[28])]
        r.run(0)  # a cold start and no scan
        m["diag_after_cold_start"] = r.diag()
        out["members"].append(m)
        r.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    print("DIAG_CASE " + json.dumps(run_case(sys.argv[1])))
