"""The two voxel down-sampling passes with their winner counts on a block boundary (csrc/icp_kernels.h VdsPass, d_count_winners,
d_compact_winners): frame_downsample of 255 / 256 / 257 entries for the drivers that launch every stage (blocks of 256 points) and of
8191 / 8192 / 8193 for the free-running kernel (blocks of 512 x 16), the returns spread over the sweep or packed behind blocks without a
single one.  An off-by-one in a pass's length or in its block counts would hide anywhere else.  The scenes are
tests/helpers/downsample_scenes.py; tests/test_downsample_scenes_cpu.py shows without a GPU that they are what they claim.

Every scene is scan 0 of a run, followed by one ordinary sweep over the same cells, through the per-call handle, the sequence runner, and a
batch of two sequences with teams of two workgroups in both of its drivers.  Reference: the CPU oracle - frame_downsample and source bit for
bit after either scan, the integer statistics equal, status 0.  (A batch's handle reads frame_downsample from the first of the lane's two
buffers, which holds the even scans': after scan 1 the batch is held to the source cloud and to the statistics, n_down among them.)
"""
import ctypes as C

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import downsample_scenes as ds

pytestmark = pytest.mark.gpu

INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
KW = dict(max_points_per_scan=ds.N, **ds.ICP)
RUN_KW = dict(max_range=ds.MAX_RANGE, min_range=ds.MIN_RANGE, with_ekf=False, **KW)


def _clouds(h):
    """(frame_downsample, source) of the last scan of an ICP handle"""
    out = []
    for fn in (L.lib().ptl_icp_last_frame_down, L.lib().ptl_icp_last_source):
        buf, w = np.empty((ds.N, 3)), C.c_int64()
        L.check(fn(h, L.dptr(buf), ds.N, C.byref(w)))
        out.append(buf[:w.value].copy())
    return out


def _check_clouds(got, ref, what, frame_down=True):
    for name, a, b in list(zip(("frame_downsample", "source"), got, ref))[0 if frame_down else 1:]:
        assert len(a) == len(b), (what, name, len(a), len(b))
        assert np.array_equal(a, b), (what, name)  # bit for bit


def _check_stats(stats, ref, what):
    assert len(stats) == 2, what
    for k in range(2):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (what, k, key, stats[k][key], ref["stats"][k][key])


def _per_call(m, arrangement):
    ref = ds.reference(m, arrangement)
    icp = core.Icp(ds.MAX_RANGE, ds.MIN_RANGE, **KW)
    try:
        for k, f in enumerate((ds.sweep(m, arrangement), ds.follow_up(m))):
            icp.register_frame(f, None)
            _check_clouds((icp.last_frame_down(), icp.last_source()), ref["clouds"][k], ("per call", m, arrangement, k))
        _check_stats(icp.stats, ref, ("per call", m, arrangement))
    finally:
        icp.close()


def _sequence_runner(m, arrangement):
    ref = ds.reference(m, arrangement)
    r = core.SeqRunner(2, ds.N, 0, **RUN_KW)
    try:
        r.upload_scan(0, ds.sweep(m, arrangement))
        r.upload_scan(1, ds.follow_up(m))
        r.upload_imu(np.zeros((0, 7)), [0, 0])
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        r.run(1)
        _check_clouds(_clouds(h), ref["clouds"][0], ("sequence runner", m, arrangement, 0))
        r.advance(1)
        _check_clouds(_clouds(h), ref["clouds"][1], ("sequence runner", m, arrangement, 1))
        _check_stats(r.results()["stats"], ref, ("sequence runner", m, arrangement))
    finally:
        r.close()


def _batch(m):
    """both arrangements of m as the two sequences of one batch, teams of two workgroups, the free-running kernel and then the lockstep driver"""
    b = core.BatchRunner(2, 2, ds.N, 0, team_workgroups=2, **RUN_KW)
    try:
        assert b.free_running and b.team_geometry()[0] == 2
        for s, arrangement in enumerate(ds.ARRANGEMENTS):
            b.upload_scan(s, 0, ds.sweep(m, arrangement))
            b.upload_scan(s, 1, ds.follow_up(m))
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
                for s, arrangement in enumerate(ds.ARRANGEMENTS):
                    h = C.c_void_p()
                    L.check(L.lib().ptl_batch_icp(b._h, s, C.byref(h)))
                    _check_clouds(_clouds(h), ds.reference(m, arrangement)["clouds"][k], (what, m, arrangement, k), frame_down=(k == 0))
            assert b.status() == 0, (what, b.status())
            for s, arrangement in enumerate(ds.ARRANGEMENTS):
                _check_stats(b.results(s)["stats"], ds.reference(m, arrangement), (what, m, arrangement))
    finally:
        b.close()


@pytest.mark.parametrize("m", ds.COUNTS)
def test_winner_counts_on_a_block_boundary(m):
    for arrangement in ds.ARRANGEMENTS:
        _per_call(m, arrangement)
        _sequence_runner(m, arrangement)
    _batch(m)
