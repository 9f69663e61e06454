"""The 8-lane voxel scan (csrc/icp_kernels.h scan_voxelsL, csrc/top2.h) at the chunk boundaries of its voxels, on the scene of
tests/helpers/voxel_fill_scenes.py: a hand-built map on 0.5 m voxels whose voxels hold exactly 0 (absent), 1, 7, 8, 9, 16, 17 and 20 points
- 8 lanes x 3 chunks - built by three scans that register at the identity exactly, and one sweep of 1 024 source points, each in a cell of
its own.  The nearest stored point of the first iteration sits in chunk 0, 1 and 2, in each of the four voxels of the first round and in a
survivor round; there are exact ties inside one lane (stored indices l and l + 8), across lanes of one voxel and across voxels of one round,
decided by the id either way.  tests/test_voxel_fill_scenes_cpu.py shows all of that without a GPU, and that the oracle alone passes the
bars asked here.

Reference: the CPU oracle, which scans all 27 voxels - the source cloud bit for bit, every integer statistic equal (iterations, pairs and
candidate counts among them), the poses within 1e-9 m / rad; the members of a batch against the run alone bit for bit.  Drivers: the per-call
8-lane handle, the sequence runner, a batch of two on teams of two in the free-running kernel and the lockstep driver."""
import ctypes as C

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import voxel_fill_scenes as vf

pytestmark = pytest.mark.gpu

INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
POSE_TOL = 1e-9  # metres and radians
NS = vf.MAP_SCANS + 1
KW = dict(max_points_per_scan=vf.N, **vf.ICP)
RUN_KW = dict(max_range=vf.MAX_RANGE, min_range=vf.MIN_RANGE, with_ekf=False, **KW)


def _check_run(stats, poses, what):
    ref = vf.reference()
    assert len(stats) == NS, what
    for k in range(NS):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (what, k, key, stats[k][key], ref["stats"][k][key])
        D = np.linalg.inv(ref["poses"][k]) @ poses[k]
        dt, dr = np.linalg.norm(D[:3, 3]), orc.rot_angle(D)
        print(what, "scan", k, "dt %.3g dr %.3g iterations %d" % (dt, dr, stats[k]["iterations"]))
        assert dt <= POSE_TOL and dr <= POSE_TOL, (what, k, dt, dr)


def _source(h):
    buf, w = np.empty((vf.N, 3)), C.c_int64()
    L.check(L.lib().ptl_icp_last_source(h, L.dptr(buf), vf.N, C.byref(w)))
    return buf[:w.value].copy()


def _upload(r, s=None):
    for k, f in enumerate(vf.frames()):
        r.upload_scan(k, f) if s is None else r.upload_scan(s, k, f)
    r.upload_imu(np.zeros((0, 7)), [0] * NS) if s is None else r.upload_imu(s, np.zeros((0, 7)), [0] * NS)


@pytest.mark.parametrize("wgs", [32, 4])
def test_voxel_fill_per_call_8_lanes(wgs):
    icp = core.Icp(vf.MAX_RANGE, vf.MIN_RANGE, gn_lanes_per_point=8, gn_threads=512, gn_workgroups=wgs, **KW)
    try:
        poses = [icp.register_frame(f, None) for f in vf.frames()]
        assert np.array_equal(icp.last_source(), vf.reference()["source"])
        _check_run(icp.stats, poses, ("per call", wgs))
    finally:
        icp.close()


def _sequence_runner():
    r = core.SeqRunner(NS, vf.N, 0, **RUN_KW)
    try:
        _upload(r)
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        r.run()
        src = _source(h)
        out = r.results()
        return out["stats"], np.array(out["kiss_poses"]), src
    finally:
        r.close()


def test_voxel_fill_sequence_runner_and_batch_of_two_on_teams_of_two_both_drivers():
    stats1, poses1, src1 = _sequence_runner()
    assert np.array_equal(src1, vf.reference()["source"])
    _check_run(stats1, poses1, "sequence runner")
    b = core.BatchRunner(2, NS, vf.N, 0, team_workgroups=2, **RUN_KW)
    try:
        assert b.free_running and b.team_geometry()[0] == 2
        for s in range(2):
            _upload(b, s)
        for free in (True, False):
            what = "free-running" if free else "lockstep"
            if not free:
                b.set_driver(False)
            b.run()
            assert b.status() == 0, (what, b.status())
            outs = [b.results(s) for s in range(2)]
            for s in range(2):
                h = C.c_void_p()
                L.check(L.lib().ptl_batch_icp(b._h, s, C.byref(h)))
                assert np.array_equal(_source(h), vf.reference()["source"]), (what, s)
                _check_run(outs[s]["stats"], outs[s]["kiss_poses"], (what, s))
                assert np.array_equal(np.array(outs[s]["kiss_poses"]), np.array(outs[0]["kiss_poses"])), (what, s)  # member against member, bit for bit
            if free:
                # a team of two inside a batch against the same team alone (a batch of one): bit for bit
                one = core.BatchRunner(1, NS, vf.N, 0, team_workgroups=2, **RUN_KW)
                try:
                    _upload(one, 0)
                    one.run()
                    alone = one.results(0)
                    assert np.array_equal(np.array(alone["kiss_poses"]), np.array(outs[0]["kiss_poses"]))
                    assert [[st[k] for k in INT_STATS] for st in alone["stats"]] == [[st[k] for k in INT_STATS] for st in outs[0]["stats"]]
                finally:
                    one.close()
    finally:
        b.close()
