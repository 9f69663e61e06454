"""The map update where voxels are full: insert a settles a point whose voxel already holds max_points_per_voxel points where
it reads the voxel's table entry - no list push, no world-frame copy, "no slot" - and K1 keeps the deskewed point of run heads only.  The
scenes of tests/helpers/full_voxel_scenes.py fill their voxels at once (3 or 4 points per voxel);
tests/test_full_voxel_scenes_cpu.py shows that without a GPU.

References: the CPU oracle for every result - the map bit for bit where the points enter under a given pose, poses to 1e-9 and identical
integer statistics in the resident drivers (the bounds of tests/test_gpu_batch.py's long run) - and the oracle's own count of the points that
met a full voxel for the device's counter.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import full_voxel_scenes as fv
from tests.helpers import hash_scenes as hs

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9  # tests/test_gpu_batch.py test_free_running_batch_against_the_oracle_over_a_long_run
INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
ENTRY = np.dtype([("key", "<u8"), ("blk", "<i4"), ("head", "<i4")])  # tests/test_gpu_hash_tables.py


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def _dump(h):
    """ptl_icp_debug_table of an ICP handle: (table entries, block directory, error flags, n_live)"""
    h = getattr(h, "_h", h)
    info = (C.c_int64 * 8)()
    L.check(L.lib().ptl_icp_debug_table(h, None, 0, None, None, 0, info))
    slots, blocks = info[3] + 1, info[6]
    ent, bhdr, bfirst = np.empty(slots, dtype=ENTRY), np.empty((blocks, 4), dtype=np.int32), np.empty((blocks, 3))
    L.check(L.lib().ptl_icp_debug_table(h, ent.ctypes.data_as(C.c_void_p), slots, bhdr.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(bfirst), blocks, info))
    return ent, bhdr, info[2], info[1]


def _check_table(h, P, what):
    """after an update: no error, every live entry mirrors its block's count, no batch list and no pending count is left standing - a point
    that was dropped must not have joined a list nobody resets"""
    ent, bhdr, err, n_live = _dump(h)
    live = np.flatnonzero((ent["key"] != hs.EMPTY_KEY) & (ent["key"] != hs.TOMB_KEY))
    blocks = np.flatnonzero(bhdr[:, 0] > 0)
    assert err == 0 and len(live) == len(blocks) == n_live, (what, err, len(live), len(blocks), n_live)
    assert np.array_equal(np.sort(bhdr[blocks, 1]), live), what
    assert np.array_equal(ent["blk"][bhdr[blocks, 1]], blocks | bhdr[blocks, 0] << 24), what
    assert (ent["head"][live] == -1).all() and (bhdr[blocks, 2] == 0).all() and bhdr[blocks, 0].max() <= P, what
    return ent, live


def _map_of(h):
    """(size, sorted points) of the local map behind an ICP handle"""
    nv, npnt = C.c_int64(), C.c_int64()
    L.check(L.lib().ptl_icp_map_size(h, C.byref(nv), C.byref(npnt)))
    pts = np.empty((npnt.value + 8, 3))
    w = C.c_int64()
    L.check(L.lib().ptl_icp_map_points(h, L.dptr(pts), len(pts), C.byref(w)))
    return (nv.value, npnt.value), pts[:w.value]


def _cloud(h, fn, cap):
    out, w = np.empty((cap, 3)), C.c_int64()
    L.check(fn(h, L.dptr(out), cap, C.byref(w)))
    return out[:w.value].copy()


# ------------------------------------------------------------------------------------------------ 1. the stage, teacher-forced
def test_stage_insert_into_full_voxels():
    """three calls of map_add on a 2^12-slot table, 3 points per voxel (full_voxel_scenes.stage_scene): a run of 128 points that all meet full
    voxels, a wavefront that mixes full, filling and new voxels, a voxel one short of full with three candidates, full voxels behind collisions,
    and a prune that takes full voxels the same call touched - after every call the oracle's map bit for bit and a clean table"""
    sc = fv.stage_scene()
    ref = fv.stage_oracle(sc)
    icp = core.Icp(fv.STAGE_RANGE, 0.0, voxel_size=1.0, max_points_per_voxel=fv.STAGE_P, map_table_capacity=fv.STAGE_CAP, map_block_capacity=1 << 12,
                   max_points_per_scan=fv.STAGE_N_MAX)
    for i, (b, (size, pts, _)) in enumerate(zip(sc["batches"], ref)):
        icp.map_add(b, origin=sc["origin"] if i == 2 else None)
        assert icp.map_size() == size, (i, icp.map_size(), size)
        assert np.array_equal(_sorted_rows(icp.map_points()), pts), i  # bit for bit
        ent, live = _check_table(icp, fv.STAGE_P, i)
        if i == 0:  # the full voxels behind collisions are there: entries of colliding voxels away from their home slot, with a count of 3
            away = live[(hs.brick_slot(ent["key"][live], fv.STAGE_CAP - 1) != live) & np.isin(ent["key"][live], hs.pack_key(sc["colliding"]))]
            assert len(away) >= fv.N_COLLIDING - 16 and (ent["blk"][away] >> 24 == fv.STAGE_P).all(), len(away)
    icp.close()


# ------------------------------------------------------------------------------------------------ 2, 3. the resident drivers
BOX_KW = dict(max_range=fv.BOX_RANGE, min_range=fv.BOX_MIN, with_ekf=False, max_points_per_scan=fv.BOX_PTS, **fv.BOX_ICP)
# (two block classes need 5 points per voxel at least: those two runs hold 6, so that a voxel outgrows its 5-point block before it is full)
# driver -> (kind, workgroups per team (0: the batch's default, which the lockstep driver uses too), points per voxel, further settings)
BOX_DRIVERS = {
    "seq2": ("seq", 2, fv.BOX_P, {}), "free2": ("free", 2, fv.BOX_P, {}), "free2_4_per_thread": ("free", 2, fv.BOX_P, dict(per_thread=4)),
    "seq1": ("seq", 1, fv.BOX_P, {}), "free1": ("free", 1, fv.BOX_P, {}),
    "free0": ("free", 0, fv.BOX_P, {}), "lockstep0": ("lockstep", 0, fv.BOX_P, {}),
    "free2_p6": ("free", 2, fv.BOX_P_TWO_CLASSES, {}), "free2_p6_two_block_classes": ("free", 2, fv.BOX_P_TWO_CLASSES, dict(map_small_blocks=1 << 12)),
}
# the runs that must agree bit for bit: the same number of Gauss-Newton workgroups in each group
BOX_GROUPS = (("seq2", "free2", "free2_4_per_thread"), ("seq1", "free1"), ("free0", "lockstep0"), ("free2_p6", "free2_p6_two_block_classes"))
COUNTER = "dropped_full_voxel"


@functools.lru_cache(maxsize=None)
def _run_box(driver):
    """the box's sweeps through `driver`: (poses, stats, map size, map points as exported, drop counter or None)"""
    frames = fv.box_sweeps()
    kind, team, P, more = BOX_DRIVERS[driver]
    h = C.c_void_p()
    if kind == "seq":
        r = core.SeqRunner(fv.BOX_N, fv.BOX_PTS, 0, gn_workgroups=team, gn_lanes_per_point=8, gn_threads=512, **dict(BOX_KW, max_points_per_voxel=P))
        upload, imu, results = r.upload_scan, r.upload_imu, r.results
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
    else:
        kw = dict(BOX_KW, max_points_per_voxel=P, **{k: v for k, v in more.items() if k != "per_thread"})
        r = core.BatchRunner(1, fv.BOX_N, fv.BOX_PTS, 0, team_workgroups=team, free_running=(kind == "free"), **kw)
        assert r.free_running == (kind == "free") and (team == 0 or r.team_geometry()[0] == team)
        if "per_thread" in more:
            assert r.debug_map_points_per_thread(more["per_thread"]) == more["per_thread"]
        upload, imu, results = functools.partial(r.upload_scan, 0), functools.partial(r.upload_imu, 0), functools.partial(r.results, 0)
        L.check(L.lib().ptl_batch_icp(r._h, 0, C.byref(h)))
    try:
        for k, f in enumerate(frames):
            upload(k, f)
        imu(np.zeros((0, 7)), [0] * fv.BOX_N)
        r.run()
        out = results()
        size, pts = _map_of(h)
        _check_table(h, P, driver)
        return out["kiss_poses"], out["stats"], size, pts, (None if kind == "seq" else r.exec_counters(0)[COUNTER])
    finally:
        r.close()


@pytest.mark.parametrize("driver", list(BOX_DRIVERS))
def test_box_against_the_oracle(driver):
    """a sensor that stands still in a small box, 4 (6) points per voxel: from the second sweep on most points of a sweep meet a full voxel.  Every
    driver gives the oracle's poses to 1e-9, its integer statistics on every sweep and its final map; the batch drivers' counter of dropped
    points is the number the oracle's run gives - the path was taken, for exactly the points it is meant for"""
    ref = fv.box_reference(BOX_DRIVERS[driver][2])
    poses, stats, size, pts, dropped = _run_box(driver)
    assert len(poses) == len(stats) == fv.BOX_N
    dev = np.abs(poses - ref["poses"]).max()
    print(f"{driver}: poses within {dev:.3e} of the oracle's; dropped at full voxels {dropped}, oracle {sum(d for _, d in ref['per_sweep'])}")
    assert dev < POSE_TOL, dev
    for k in range(fv.BOX_N):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (driver, k, key, stats[k][key], ref["stats"][k][key])
    assert size == ref["size"], (size, ref["size"])
    a, b = pts[np.lexsort(np.round(pts, 6).T[::-1])], ref["map"][np.lexsort(np.round(ref["map"], 6).T[::-1])]
    assert np.abs(a - b).max() <= POSE_TOL, np.abs(a - b).max()  # (the points entered under registered poses: tests/test_gpu_search_edges.py _check_maps)
    if dropped is not None:
        assert dropped == sum(d for _, d in ref["per_sweep"]), (dropped, ref["per_sweep"])


def test_box_drivers_agree_bit_for_bit():
    """with the same number of Gauss-Newton workgroups the sequence runner, the free-running kernel (8 and 4 points per thread, one and two block
    classes) and the lockstep driver give the same bits: poses, statistics, map points, and the same count of dropped points"""
    for group in BOX_GROUPS:
        want = _run_box(group[0])
        for d in group[1:]:
            got = _run_box(d)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (d, group[0])
            assert np.array_equal(_sorted_rows(got[3]), _sorted_rows(want[3])), (d, group[0])
        counts = {_run_box(d)[4] for d in group if BOX_DRIVERS[d][0] != "seq"}
        assert len(counts) == 1 and None not in counts, counts


# ------------------------------------------------------------------------------------------------ 4. K1 keeps run heads only
def test_long_runs_of_equal_keys_in_the_first_downsampling_pass():
    """a flat wall close to the sensor: thirty consecutive points share a voxel of pass 1, so most lanes of a wavefront are no run head and
    store no point.  frame_downsample and the source cloud are the oracle's bit for bit, per call and in the batch"""
    f = fv.wall_sweep()
    n = len(f)
    ref = orc.ICP(fv.BOX_RANGE, fv.BOX_MIN, voxel_size=1.0, deskew=0)
    ref.register_frame(f.astype(np.float64), None)
    fd, src = ref.last_frame_down(), ref.last_source()
    assert 10 < len(src) < len(fd) < n // 32  # (long runs: 89 voxels of pass 1 for 4096 points, visited in 240 runs)
    kw = dict(voxel_size=1.0, deskew=0, max_points_per_scan=n)
    icp = core.Icp(fv.BOX_RANGE, fv.BOX_MIN, **kw)
    icp.register_frame(f, None)
    assert np.array_equal(icp.last_frame_down(), fd) and np.array_equal(icp.last_source(), src)
    b = core.BatchRunner(1, 1, n, 0, max_range=fv.BOX_RANGE, min_range=fv.BOX_MIN, with_ekf=False, **kw)
    assert b.free_running
    b.upload_scan(0, 0, f)
    b.upload_imu(0, np.zeros((0, 7)), [0])
    b.run()
    h = C.c_void_p()
    L.check(L.lib().ptl_batch_icp(b._h, 0, C.byref(h)))
    bfd, bsrc = _cloud(h, L.lib().ptl_icp_last_frame_down, n), _cloud(h, L.lib().ptl_icp_last_source, n)
    assert np.array_equal(bfd, icp.last_frame_down()) and np.array_equal(bsrc, icp.last_source())
    assert b.results(0)["stats"][0] == icp.stats[0]
    for x in (icp, b):
        x.close()
