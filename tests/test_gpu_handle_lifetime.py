"""Every handle of the host library gives back what it took (csrc/hip_own.h: one owner per handle, scoped temporaries): free device
memory, read from the HIP runtime itself (hipMemGetInfo through ctypes - no torch, no entry point of the library), does not drift over
create / use / close cycles, a creation that fails half-way leaves nothing behind, and neither does an error return between the
allocation of a call's temporaries and their release.  The smallest shapes the handles accept."""
import ctypes as C
import gc

import numpy as np
import pytest

from ptudes_lab_amd import _lib, core, synth

pytestmark = pytest.mark.gpu

H, W, N = 16, 64, 3
SMALL = dict(max_points_per_scan=H * W, scan_cols=W, map_block_capacity=4096, map_table_capacity=1 << 12, gn_workgroups=32)
KW = dict(max_range=70.0, min_range=1.0, **SMALL)
# Free memory after cycle 5 against free memory after cycle 2 (cycles 1 and 2 load the code objects and let the runtime's own pools of
# signals and scratch settle).  The bound is zero bytes.  (The parent commit's library, with its hand-kept free lists, is the yardstick
# should the runtime itself drift: its figure for the same test belongs here.  It has NOT been measured yet - no MI355X could be had
# when this test was written - so the constant is the bound as such and not a measured value.)
DRIFT_BYTES = 0


@pytest.fixture(scope="module")
def hip():
    """the HIP runtime the library is bound to, from the process's own map (a second copy of the runtime would see another context)"""
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "the library is loaded but no libamdhip64 is mapped"
    rt = C.CDLL(paths[0])
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rt.hipDeviceSynchronize.argtypes = []
    return rt


def _free_total(hip):
    gc.collect()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value, total.value


@pytest.fixture(scope="module")
def data():
    seq = synth.make_sequence(seed=1000, n_scans=N, H=H, W=W)
    ends = [seq.imu_range_for_scan(k)[1] for k in range(N)]
    rows = [ends[0] - 1, ends[1] - 1, ends[2] - 2, ends[2] - 1]  # 4 IMU rows: one before scan 0, one before scan 1, two before scan 2
    assert rows == sorted(set(rows)) and rows[0] >= 0
    k = np.arange(N)
    return dict(scans=[seq.scan(i) for i in range(N)], imu=np.ascontiguousarray(seq.imu[rows]), imu_end=[1, 2, 4],
                t0t1=np.stack([seq.t_base + k * seq.scan_dt, seq.t_base + (k + 1) * seq.scan_dt], axis=1))


def _icp(d):
    icp = core.Icp(70.0, 1.0, **SMALL)
    icp.register_frame(d["scans"][0])
    traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)])
    icp.map_add_posed(traj, np.linspace(0.1, 0.9, W), xyz=d["scans"][1], H=H)  # (allocates the handle's posed-scan words)
    icp.set_active_beams(H, H // 2)                                          # (and its row mask)
    traj.close()
    icp.close()


def _ekf(d):
    e = core.Ekf()
    e.enable_smoother(8)
    e.enable_knots(8)
    e.process_imu_batch(d["imu"])
    e.process_pose(np.eye(4))
    e.close()


def _lut(d):
    lut = core.Lut(H, W, np.linspace(45.0, -45.0, H), np.zeros(H))
    lut(np.full(H * W, 1000, dtype=np.uint32))
    lut.close()


def _traj(d):
    t = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)])
    core.traj_poses_at([0.0, 1.0], [np.eye(4), np.eye(4)], [0.5])
    t.close()


def _seq(d):
    r = core.SeqRunner(N, H * W, 4, use_imu_prediction=True, imu_deskew=True, **KW)
    for k in range(N):
        r.upload_scan(k, d["scans"][k])
    r.upload_imu(d["imu"], d["imu_end"])
    r.upload_sweep_times(d["t0t1"])
    r.run(1)
    r.close()


def _batch(d, free_running):
    b = core.BatchRunner(2, N, H * W, 4, use_imu_prediction=True, imu_deskew=True, free_running=free_running, **KW)
    b.enable_smoother()
    for s in range(2):
        for k in range(N):
            b.upload_scan(s, k, d["scans"][k])
        b.upload_imu(s, d["imu"], d["imu_end"])
        b.upload_sweep_times(s, d["t0t1"])
    b.run(1)
    b.close()


CYCLES = {"icp": _icp, "ekf": _ekf, "lut": _lut, "traj": _traj, "seq": _seq,
          "batch_free_running": lambda d: _batch(d, True), "batch_lockstep": lambda d: _batch(d, False)}


@pytest.mark.parametrize("kind", list(CYCLES))
def test_create_use_close_does_not_drift(hip, data, kind):
    free = []
    for _ in range(5):
        CYCLES[kind](data)
        free.append(_free_total(hip)[0])
    print(f"{kind}: free bytes after each cycle {free}, drift cycle 2 -> 5: {free[1] - free[4]}")
    assert abs(free[1] - free[4]) <= DRIFT_BYTES, free


def test_a_creation_that_fails_half_way_gives_everything_back(hip, data):
    """the sweep store (n_scans x points_per_scan x 12 bytes = 53 TB; a sweep stays at 1024 points, or the registration itself would be
    sized for it) is refused by the runtime after the registration and the filter of the sequence exist: the library's allocation
    error, and free memory where it was"""
    _seq(data)  # (code objects loaded, pools settled)
    before, total = _free_total(hip)
    n_scans = 1 << 32
    assert n_scans * H * W * 12 > 40 * total
    with pytest.raises(RuntimeError, match="ptl_seq_create: allocation failed"):
        core.SeqRunner(n_scans, H * W, 4, **KW)
    after = _free_total(hip)[0]
    print(f"failed creation: free before {before}, after {after}")
    assert after == before


def test_an_error_return_behind_a_temporarys_allocation_gives_it_back(hip):
    """ptl_traj_poses_at takes five temporaries; with n timestamps so many that the output rows (128 n bytes) exceed the device while the
    timestamps (8 n) fit, the fourth request fails behind three that succeeded - an error code before anything is read from the host
    arrays - and the three are given back"""
    core.traj_poses_at([0.0, 1.0], [np.eye(4), np.eye(4)], [0.5])
    before, total = _free_total(hip)
    n = total // 128 + 1
    kt, kp = np.array([0.0, 1.0]), np.stack([np.eye(4), np.eye(4)]).reshape(2, 16)
    ts, out, nout = np.zeros(1), np.zeros(16), C.c_int64()
    rc = _lib.lib().ptl_traj_poses_at(0, _lib.dptr(kt), _lib.dptr(kp), 2, 0.0, 0.0, _lib.dptr(ts), n, _lib.dptr(out), C.byref(nout))
    assert rc != 0
    after = _free_total(hip)[0]
    print(f"failed call: free before {before}, after {after}")
    assert after == before
