"""The first round of the 8-lane search and the kinds of its queue (csrc/icp_kernels.h gn8_search, phase B of gn8_body) on the scene of
tests/helpers/search_chain_scenes.py: one 4096-point sweep against a hand-built map on 0.5 m voxels, every source point in a cell of its own.

Idle slot: without a last winner outside the own voxel the second slot of the first round takes the third-nearest occupied box.  The cells
hold exactly three other boxes with the nearest neighbour in the third (the filled slot supplies the answer), four with it in the fourth (a
survivor round is still needed), an exact tie between the third box and the own voxel decided by the order id either way, zero, one and two
other boxes, one occupied box among 26 empty ones, nothing at all, and winners in another voxel (the slot stays theirs).
Mixed kinds: the sweep comes from a moved sensor; in iterations 1 and 2 a few hundred points cross a face of the map's voxels while their
neighbours in the same 64-point block stay, so that the search's wavefronts hold groups that read their row next to groups that rebuild it
without reading, and the rebuilding groups of one flush span several passes.  tests/test_search_chain_scenes_cpu.py shows all of that
without a GPU.

Reference: the CPU oracle, which scans all 27 voxels - the source cloud bit for bit, the integer statistics equal (iterations, pairs and
candidate counts among them), the pose within 1e-9 m / rad; the members of a batch against the run alone bit for bit.  Drivers: the per-call
8-lane handle (one-hop and generic exchange), the sequence runner, a batch of two on teams of two in the free-running kernel and the
lockstep driver."""
import ctypes as C

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import search_chain_scenes as sc

pytestmark = pytest.mark.gpu

INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
POSE_TOL = 1e-9  # metres and radians: the bar of tests/test_gpu_search_edges.py
KW = dict(max_points_per_scan=sc.N, **sc.ICP)
RUN_KW = dict(max_range=sc.MAX_RANGE, min_range=sc.MIN_RANGE, with_ekf=False, **KW)


def _check_run(stats, poses, what):
    ref = sc.reference()
    assert len(stats) == 2, what
    for k in range(2):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (what, k, key, stats[k][key], ref["stats"][k][key])
        D = np.linalg.inv(ref["poses"][k]) @ poses[k]
        dt, dr = np.linalg.norm(D[:3, 3]), orc.rot_angle(D)
        assert dt <= POSE_TOL and dr <= POSE_TOL, (what, k, dt, dr)


def _source(h):
    buf, w = np.empty((sc.N, 3)), C.c_int64()
    L.check(L.lib().ptl_icp_last_source(h, L.dptr(buf), sc.N, C.byref(w)))
    return buf[:w.value].copy()


@pytest.mark.parametrize("wgs", [32, 4])
def test_search_chain_per_call_8_lanes(wgs):
    icp = core.Icp(sc.MAX_RANGE, sc.MIN_RANGE, gn_lanes_per_point=8, gn_threads=512, gn_workgroups=wgs, **KW)
    try:
        poses = [icp.register_frame(f, None) for f in (sc.frame0(), sc.frame1())]
        assert np.array_equal(icp.last_source(), sc.reference()["source"])
        _check_run(icp.stats, poses, ("per call", wgs))
    finally:
        icp.close()


def _sequence_runner():
    r = core.SeqRunner(2, sc.N, 0, **RUN_KW)
    try:
        r.upload_scan(0, sc.frame0())
        r.upload_scan(1, sc.frame1())
        r.upload_imu(np.zeros((0, 7)), [0, 0])
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        r.run()
        src = _source(h)
        out = r.results()
        return out["stats"], np.array(out["kiss_poses"]), src
    finally:
        r.close()


def test_search_chain_sequence_runner_and_batch_of_two_on_teams_of_two_both_drivers():
    stats1, poses1, src1 = _sequence_runner()
    assert np.array_equal(src1, sc.reference()["source"])
    _check_run(stats1, poses1, "sequence runner")
    b = core.BatchRunner(2, 2, sc.N, 0, team_workgroups=2, **RUN_KW)
    try:
        assert b.free_running and b.team_geometry()[0] == 2
        for s in range(2):
            b.upload_scan(s, 0, sc.frame0())
            b.upload_scan(s, 1, sc.frame1())
            b.upload_imu(s, np.zeros((0, 7)), [0, 0])
        free_poses = None
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
                assert np.array_equal(_source(h), sc.reference()["source"]), (what, s)
                _check_run(outs[s]["stats"], outs[s]["kiss_poses"], (what, s))
                assert np.array_equal(np.array(outs[s]["kiss_poses"]), np.array(outs[0]["kiss_poses"])), (what, s)  # member against member, bit for bit
            if free:
                free_poses = np.array(outs[0]["kiss_poses"])
                # a team of two inside a batch against the same team alone (a batch of one): bit for bit
                one = core.BatchRunner(1, 2, sc.N, 0, team_workgroups=2, **RUN_KW)
                try:
                    one.upload_scan(0, 0, sc.frame0())
                    one.upload_scan(0, 1, sc.frame1())
                    one.upload_imu(0, np.zeros((0, 7)), [0, 0])
                    one.run()
                    alone = one.results(0)
                    assert np.array_equal(np.array(alone["kiss_poses"]), free_poses)
                    assert [[st[k] for k in INT_STATS] for st in alone["stats"]] == [[st[k] for k in INT_STATS] for st in outs[0]["stats"]]
                finally:
                    one.close()
    finally:
        b.close()
