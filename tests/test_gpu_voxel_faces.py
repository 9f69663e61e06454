"""The voxel index where its exact-division fallback is taken (csrc/icp_kernels.h voxel_index): the division sits behind a branch that a
wavefront takes when any of its lanes lies within the tolerance of a voxel face.  The scenes of tests/helpers/voxel_face_scenes.py put, into
every 64-point wavefront of a 4096-point sweep, a few lanes exactly on faces of the two down-sampling sizes and of the map's voxel (and
float32 neighbours of such faces beside them), into one wavefront none and into one all 64: the branch not taken, partly taken, fully
taken.  tests/test_voxel_index_cpu.py shows without a GPU that the scenes are what they claim.

The sweep is scan 0 of a run; the sweep that follows comes from a moved sensor, carries face lanes in the sensor frame (down-sampling,
the first search's key) and 600 points that the Gauss-Newton iterations carry across a face of the map (phase A's and the search's key
change).  Drivers as in tests/test_gpu_downsample_edges.py: the per-call handle, the sequence runner, a batch of two sequences on teams of
two workgroups in the free-running kernel and the lockstep driver.  Reference: the CPU oracle - frame_downsample and source bit for bit
after either scan, the integer statistics equal (iterations, n_corr_last and sum_cand of the second scan among them), status 0, the
second pose within 1e-9 m / rad.  (A batch's handle reads frame_downsample from the first of the lane's two buffers: after scan 1 the
batch is held to the source cloud and the statistics.)

The runners take float32, where a coordinate is on a face exactly or far outside the tolerance, and on an exact face the fallback returns
what the product gave.  The per-call handle also takes float64: sweep0_f64() (0.7 m voxels) holds the coordinates where the division
changes the index."""
import ctypes as C

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import voxel_face_scenes as vf

pytestmark = pytest.mark.gpu

INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
POSE_TOL = 1e-9  # metres and radians: the bar of tests/test_gpu_search_edges.py
KW = dict(max_points_per_scan=vf.N, **vf.ICP)
RUN_KW = dict(max_range=vf.MAX_RANGE, min_range=vf.MIN_RANGE, with_ekf=False, **KW)


def _clouds(h):
    """(frame_downsample, source) of the last scan of an ICP handle"""
    out = []
    for fn in (L.lib().ptl_icp_last_frame_down, L.lib().ptl_icp_last_source):
        buf, w = np.empty((vf.N, 3)), C.c_int64()
        L.check(fn(h, L.dptr(buf), vf.N, C.byref(w)))
        out.append(buf[:w.value].copy())
    return out


def _check_clouds(got, ref, what, frame_down=True):
    for name, a, b in list(zip(("frame_downsample", "source"), got, ref))[0 if frame_down else 1:]:
        assert len(a) == len(b), (what, name, len(a), len(b))
        assert np.array_equal(a, b), (what, name)  # bit for bit


def _check_run(stats, poses, what):
    ref = vf.reference()
    assert len(stats) == 2, what
    for k in range(2):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (what, k, key, stats[k][key], ref["stats"][k][key])
        D = np.linalg.inv(ref["poses"][k]) @ poses[k]
        dt, dr = np.linalg.norm(D[:3, 3]), orc.rot_angle(D)
        assert dt <= POSE_TOL and dr <= POSE_TOL, (what, k, dt, dr)


def test_faces_per_call():
    ref = vf.reference()
    icp = core.Icp(vf.MAX_RANGE, vf.MIN_RANGE, **KW)
    try:
        poses = []
        for k, f in enumerate((vf.sweep0(), vf.sweep1())):
            poses.append(icp.register_frame(f, None))
            _check_clouds((icp.last_frame_down(), icp.last_source()), ref["clouds"][k], ("per call", k))
        _check_run(icp.stats, poses, "per call")
    finally:
        icp.close()


def test_faces_where_the_division_decides_per_call_float64():
    ref = vf.reference_f64()
    icp = core.Icp(vf.MAX_RANGE, vf.MIN_RANGE, voxel_size=vf.VOXEL_SIZE_F64, deskew=0, max_points_per_scan=vf.N)
    try:
        icp.register_frame(vf.sweep0_f64(), None)
        _check_clouds((icp.last_frame_down(), icp.last_source()), ref["clouds"][0], "per call, float64")
        for key in INT_STATS:
            assert icp.stats[0][key] == ref["stats"][0][key], (key, icp.stats[0][key], ref["stats"][0][key])
        m = icp.map_points()
        assert np.array_equal(m[np.lexsort(m.T[::-1])], ref["map0"])  # the map's voxels hold the oracle's points, bit for bit
    finally:
        icp.close()


def test_faces_sequence_runner():
    ref = vf.reference()
    r = core.SeqRunner(2, vf.N, 0, **RUN_KW)
    try:
        r.upload_scan(0, vf.sweep0())
        r.upload_scan(1, vf.sweep1())
        r.upload_imu(np.zeros((0, 7)), [0, 0])
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        r.run(1)
        _check_clouds(_clouds(h), ref["clouds"][0], ("sequence runner", 0))
        r.advance(1)
        _check_clouds(_clouds(h), ref["clouds"][1], ("sequence runner", 1))
        out = r.results()
        _check_run(out["stats"], out["kiss_poses"], "sequence runner")
    finally:
        r.close()


def test_faces_batch_of_two_on_teams_of_two_both_drivers():
    ref = vf.reference()
    b = core.BatchRunner(2, 2, vf.N, 0, team_workgroups=2, **RUN_KW)
    try:
        assert b.free_running and b.team_geometry()[0] == 2
        for s in range(2):
            b.upload_scan(s, 0, vf.sweep0())
            b.upload_scan(s, 1, vf.sweep1())
            b.upload_imu(s, np.zeros((0, 7)), [0, 0])
        for free in (True, False):
            what = "free-running" if free else "lockstep"
            if not free:
                b.set_driver(False)
            b.run(1)
            for k in range(2):
                if k:
                    b.enqueue(1)
                    b.wait()
                for s in range(2):
                    h = C.c_void_p()
                    L.check(L.lib().ptl_batch_icp(b._h, s, C.byref(h)))
                    _check_clouds(_clouds(h), ref["clouds"][k], (what, s, k), frame_down=(k == 0))
            assert b.status() == 0, (what, b.status())
            for s in range(2):
                out = b.results(s)
                _check_run(out["stats"], out["kiss_poses"], (what, s))
    finally:
        b.close()
