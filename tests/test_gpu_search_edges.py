"""The voxel index, the first-point-per-voxel selections, the 27-voxel search, the gates and every form of the Gauss-Newton loop on the scenes
of tests/helpers/lattice_scenes.py, where the hard cases are the rule: exact ties between candidates (strictly smaller wins, an equal distance
goes to the earlier candidate in visiting order), distances that equal the correspondence gate, coordinates on voxel boundaries, ranges that
equal min_range / max_range / the prune distance.  The reference is the CPU oracle; tests/test_lattice_scenes_cpu.py shows, without a GPU,
that it agrees with its independent numpy restatement and with a brute-force search on every scene used here, that the scenes contain the
hard cases in numbers, and that the free-running triplets keep every decision 1e-6 m from flipping wherever device and oracle may differ by
rounding.  One scene ties exactly at the SECOND iteration as well (by exact arithmetic, not by luck): the only way to the tie-break of the 8-lane
kernel's answer row.

Kernel instances reached: k_gn_loop<20 | 0, false> in mode 1 (linear_system) and mode 0 (register_frame), k_gn_loop<20, true>,
k_gn_loop8<20 | 0, 32 | 16 | 8 | 0>, kx_seq_run (free-running batch, one and two block classes), kx_gn_loop<20> (lockstep batch), and the
stage kernels before and after them (deskew + range filter + both down-samplings, map insert, prune).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import lattice_scenes as ls

pytestmark = pytest.mark.gpu

INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")
POSE_TOL = 1e-9  # metres and radians: the bound test_throughput_kernel_8_lanes_per_point_vs_oracle uses
SMALL = dict(map_table_capacity=1 << 18, map_block_capacity=1 << 17)  # these maps hold a few ten thousand voxels at most


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def _same_map(icp, ref, what):
    assert icp.map_size() == (ref.num_voxels, ref.num_points), (what, icp.map_size(), ref.num_voxels, ref.num_points)
    assert np.array_equal(_sorted_rows(icp.map_points()), _sorted_rows(ref.points())), what  # bit for bit


# ------------------------------------------------------------------------------------------------ voxel index
@pytest.mark.parametrize("vs", ls.VOXEL_SIZES)
def test_voxel_index_on_boundaries_through_the_map(vs):
    """coordinates at k * vs and 1, 2 ulp either side, with companions inside the voxels on both sides, on each axis and in every octant:
    the map keeps the same points as the oracle's (int)(x / vs), with room for 20 per voxel and with room for 1"""
    cloud = ls.boundary_cloud(vs)
    for cap in (20, 1):
        icp = core.Icp(1e9, 0.0, voxel_size=vs, max_points_per_voxel=cap, max_points_per_scan=1 << 16, **SMALL)
        ref = orc.Map(vs, 1e9, cap)
        icp.map_add(cloud)
        ref.add_points(cloud)
        _same_map(icp, ref, (vs, cap))
        icp.close()


@pytest.mark.parametrize("vs,dtype", [(0.7, np.float64), (0.1, np.float64), (0.3, np.float64), (1.0, np.float64), (1.0, np.float32), (0.5, np.float32)])
def test_voxel_index_and_first_in_scan_order_through_the_downsample(vs, dtype):
    """frame 0 of a cloud on the boundaries of the 0.5 vs voxels, with exact duplicates and one voxel that holds thousands of points: both
    down-samplings keep the oracle's points, in its order; f32 input (dyadic values, exact) like f64"""
    rng = np.random.default_rng(11)
    cloud = ls.boundary_cloud(0.5 * vs, dtype=dtype)
    crowd = (np.array([3.0, -5.0, 7.0]) * vs + rng.integers(1, 255, (4000, 3)) * (0.5 * vs / 256)).astype(dtype)  # one 0.5 vs voxel; dyadic for dyadic vs
    x = np.concatenate([cloud, cloud[::25], crowd])
    x = x[rng.permutation(len(x))]
    icp = core.Icp(1e9, 1e-3, voxel_size=vs, **SMALL)
    ref = orc.ICP(1e9, 1e-3, voxel_size=vs)
    t01 = np.zeros(len(x))
    icp.register_frame(x, None if dtype == np.float32 else t01)
    ref.register_frame(x.astype(np.float64), t01)
    a, b = icp.stats[-1], ref.stats[-1]
    assert (a["n_valid"], a["n_down"], a["n_src"]) == (b["n_valid"], b["n_down"], b["n_src"]), (a, b)
    assert b["n_valid"] == len(x) and b["n_down"] < len(cloud) < len(x)
    assert np.array_equal(icp.last_frame_down(), ref.last_frame_down())
    assert np.array_equal(icp.last_source(), ref.last_source())
    _same_map(icp, ref.map, (vs, dtype))


# ------------------------------------------------------------------------------------------------ range gate, prune gate
@pytest.mark.parametrize("u", (-3, -2, -1, 0, 1, 2, 3))
def test_range_gate_and_prune_gate_at_the_limit(u):
    """points whose range is exactly min_range / max_range (u = 0) or u ulp of one coordinate off: r < max_range && r > min_range keeps the
    oracle's; voxels whose first point is exactly max_range (or u ulp off) from the prune origin go or stay as in the oracle (strict >)"""
    x = np.concatenate([ls.range_edge_points(ls.MIN_RANGE, (u,)), ls.range_edge_points(ls.MAX_RANGE, (u,))])
    icp = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, voxel_size=0.01, **SMALL)  # (voxels of 5 mm: the down-sampling merges nothing)
    ref = orc.ICP(ls.MAX_RANGE, ls.MIN_RANGE, voxel_size=0.01)
    t01 = np.zeros(len(x))
    icp.register_frame(x, t01)
    ref.register_frame(x, t01)
    assert icp.stats[-1]["n_valid"] == ref.stats[-1]["n_valid"], (icp.stats[-1], ref.stats[-1])
    assert icp.stats[-1]["n_down"] == ref.stats[-1]["n_down"] == ref.stats[-1]["n_valid"]
    assert np.array_equal(icp.last_frame_down(), ref.last_frame_down())
    for origin in (np.zeros(3), np.array([16.0, -8.0, 4.0])):
        first = ls.range_edge_points(ls.MAX_RANGE, (u,)) + origin
        pts = np.concatenate([first, first + 1e-3 * np.sign(first)])  # a second point per voxel, beyond the limit: the FIRST one decides
        m_gpu = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, **SMALL)
        m_ref = orc.Map(ls.VOXEL_SIZE, ls.MAX_RANGE, 20)
        m_gpu.map_add(pts, origin=origin)
        m_ref.add_points(pts)
        n_before = m_ref.num_voxels
        m_ref.prune(origin)
        _same_map(m_gpu, m_ref, (u, origin))
        if u == 0 and not origin.any():
            assert 0 < m_ref.num_voxels < n_before, (m_ref.num_voxels, n_before)
        m_gpu.close()


# ------------------------------------------------------------------------------------------------ ties and gates, 32-lane kernel
def _one_by_one(icp, ref, q, idx, M, what):
    """one query per call: with a single pair in the sums another target changes entries at order 1, so this identifies the chosen target"""
    for i in idx:
        s_ref, nc_ref, cand_ref = ref.linear_system(q[i:i + 1], M, M / 9.0)
        s_gpu, nc, cand = icp.linear_system(q[i:i + 1], M, M / 9.0)
        assert (nc, cand) == (nc_ref, cand_ref), (what, i, q[i], nc, cand, nc_ref, cand_ref)
        assert np.abs(s_gpu - s_ref).max() <= 1e-12 * np.abs(s_ref).max(), (what, i, q[i], s_gpu, s_ref)


@pytest.mark.parametrize("cap,wgs", [(20, 256), (5, 256), (32, 256), (20, 1)])
def test_tie_queries_on_the_32_lane_kernel(cap, wgs):
    """the tie grid against a block of the lattice: cell centres (8-way ties), face and edge midpoints, stored points, voxel boundaries,
    +0 and -0, nearest candidates at exactly the gate - all at once (pair and candidate counts), then a fixed subset one query per call"""
    m, q = ls.tie_queries()
    M = 0.5
    icp = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, max_points_per_voxel=cap, gn_workgroups=wgs, **SMALL)
    ref = orc.Map(ls.VOXEL_SIZE, ls.MAX_RANGE, cap)
    icp.map_add(m)
    ref.add_points(m)
    _same_map(icp, ref, cap)
    s_ref, nc_ref, cand_ref = ref.linear_system(q, M, M / 9.0)
    s_gpu, nc, cand = icp.linear_system(q, M, M / 9.0)
    assert (nc, cand) == (nc_ref, cand_ref)
    assert np.abs(s_gpu - s_ref).max() <= 1e-9 * np.abs(s_ref).max()
    idx = ls.pick_queries(m, q, M)
    assert 100 <= len(idx) <= 600
    _one_by_one(icp, ref, q, idx, M, cap)


@pytest.mark.parametrize("M", [0.75, 3 * 0.35])
@pytest.mark.parametrize("wgs", [256, 1])
def test_gate_queries_on_the_32_lane_kernel(M, wgs):
    """isolated map points, queries at exactly the gate and 1, 2, 3 ulp either side (sqrt(d2) < M as a squared comparison): every one alone"""
    m, q, _ = ls.gate_queries(M)
    icp = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, gn_workgroups=wgs, **SMALL)
    ref = orc.Map(ls.VOXEL_SIZE, ls.MAX_RANGE, 20)
    icp.map_add(m)
    ref.add_points(m)
    s_ref, nc_ref, cand_ref = ref.linear_system(q, M, M / 9.0)
    s_gpu, nc, cand = icp.linear_system(q, M, M / 9.0)
    assert (nc, cand) == (nc_ref, cand_ref) and 0 < nc_ref < len(q) == cand_ref
    assert len(q) <= 600
    _one_by_one(icp, ref, q, range(len(q)), M, M)


# ------------------------------------------------------------------------------------------------ triplets, every Gauss-Newton form
@functools.lru_cache(maxsize=None)
def _oracle_triplet(d, cap, th):
    """the oracle's run of a triplet, once: (poses, stats, sorted map after frame 0, sorted map after frame 1)"""
    ref = orc.ICP(ls.MAX_RANGE, ls.MIN_RANGE, max_points_per_voxel=cap, initial_threshold=th)
    t01, maps = ls.sweep_t01(), []
    for f in ls.sweep_triplet(d):
        ref.register_frame(f.astype(np.float64), t01)
        maps.append(_sorted_rows(ref.map.points()))
    return ref.poses(), ref.stats, maps[0], maps[1]


def _map_of(h):
    """sorted points of the local map behind an ICP handle"""
    nv, npnt = C.c_int64(), C.c_int64()
    L.check(L.lib().ptl_icp_map_size(h, C.byref(nv), C.byref(npnt)))
    pts = np.empty((npnt.value + 8, 3))
    w = C.c_int64()
    L.check(L.lib().ptl_icp_map_points(h, L.dptr(pts), len(pts), C.byref(w)))
    return _sorted_rows(pts[:w.value])


def _check_maps(maps, d, cap, th, what):
    """frame 0 enters the map under the identity: bit for bit.  Frame 1 enters under a pose that carries a Gauss-Newton sum (1e-15 m from the
    oracle's): the same number of points, each within POSE_TOL of the oracle's"""
    _, _, m0, m1 = _oracle_triplet(d, cap, th)
    assert np.array_equal(maps[0], m0), (what, d)
    assert maps[1].shape == m1.shape, (what, d, maps[1].shape, m1.shape)
    a, b = maps[1][np.lexsort(np.round(maps[1], 6).T[::-1])], m1[np.lexsort(np.round(m1, 6).T[::-1])]
    assert np.abs(a - b).max() <= POSE_TOL, (what, d, np.abs(a - b).max())


def _check_run(poses, stats, d, cap, th, what):
    ref_poses, ref_stats, _, _ = _oracle_triplet(d, cap, th)
    assert len(poses) == len(stats) == 3
    for k in range(3):
        for key in INT_STATS:
            assert stats[k][key] == ref_stats[k][key], (what, d, k, key, stats[k][key], ref_stats[k][key])
        D = np.linalg.inv(ref_poses[k]) @ poses[k]
        dt, dr = np.linalg.norm(D[:3, 3]), orc.rot_angle(D)
        assert dt <= POSE_TOL and dr <= POSE_TOL, (what, d, k, dt, dr)
    assert ref_stats[1]["iterations"] >= 2


PER_CALL_FORMS = {
    "sparse32": dict(),
    "dense32": dict(gn_workgroups=1, gn_threads=256),  # frame 1's hint is frame 0's n_src (343 > 8 groups): k_gn_loop<P, true>
    "lanes8_gc32": dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=32),
    "lanes8_gc16": dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=16),
    "lanes8_gc8": dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=8),
    "lanes8_gc0": dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=4),
}


def _settings(form):
    """(max_points_per_voxel, initial_threshold): 20 and 2.0 everywhere, 5 as well, and 0.25 on the 8-lane forms"""
    return [(20, 2.0), (5, 2.0)] + ([(20, 0.25)] if form.startswith("lanes8") else [])


@pytest.mark.parametrize("d", ls.DISPLACEMENTS)
@pytest.mark.parametrize("form", list(PER_CALL_FORMS))
def test_triplets_per_call(form, d):
    for cap, th in _settings(form):
        icp = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, max_points_per_voxel=cap, initial_threshold=th, max_points_per_scan=ls.SWEEP_H * ls.SWEEP_W,
                       **PER_CALL_FORMS[form])
        poses, maps = [], []
        for f in ls.sweep_triplet(d):
            poses.append(icp.register_frame(f, None))
            maps.append(_sorted_rows(icp.map_points()))
        _check_run(poses, icp.stats, d, cap, th, (form, cap, th))
        _check_maps(maps, d, cap, th, (form, cap, th))
        icp.close()


@pytest.mark.parametrize("d", ls.DISPLACEMENTS)
def test_triplets_seq_runner(d):
    """the device-resident loop, ICP only, 8-lane kernel"""
    n, frames = 3, ls.sweep_triplet(d)
    for cap, th in _settings("lanes8"):
        r = core.SeqRunner(n, ls.SWEEP_H * ls.SWEEP_W, 0, max_range=ls.MAX_RANGE, min_range=ls.MIN_RANGE, with_ekf=False, gn_workgroups=32,
                           gn_lanes_per_point=8, gn_threads=512, max_points_per_voxel=cap, initial_threshold=th)
        for k in range(n):
            r.upload_scan(k, frames[k])
        r.upload_imu(np.zeros((0, 7)), [0] * n)
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
        maps = []
        r.run(1)
        maps.append(_map_of(h))
        r.advance(1)
        maps.append(_map_of(h))
        r.advance(1)
        out = r.results()
        _check_run(out["kiss_poses"], out["stats"], d, cap, th, ("seq", cap, th))
        _check_maps(maps, d, cap, th, ("seq", cap, th))
        r.close()


@pytest.mark.parametrize("driver,th", [("free", 2.0), ("free", 0.25), ("free_two_block_classes", 2.0), ("lockstep32", 2.0)])
def test_triplets_as_the_sequences_of_one_batch(driver, th):
    """the four triplets side by side: kx_seq_run teams (one block class, and 5-point blocks that voxels outgrow), and the lockstep driver
    with the 32-lane kernel"""
    n, S = 3, len(ls.DISPLACEMENTS)
    over = dict(max_range=ls.MAX_RANGE, min_range=ls.MIN_RANGE, with_ekf=False, max_points_per_voxel=20, initial_threshold=th)
    if driver == "lockstep32":
        over.update(gn_lanes_per_point=32, gn_threads=1024, free_running=False)
    if driver == "free_two_block_classes":
        over.update(map_block_capacity=1 << 14, map_small_blocks=1 << 13)
    b = core.BatchRunner(S, n, ls.SWEEP_H * ls.SWEEP_W, 0, **over)
    assert b.free_running == (driver != "lockstep32")
    for s, d in enumerate(ls.DISPLACEMENTS):
        for k, f in enumerate(ls.sweep_triplet(d)):
            b.upload_scan(s, k, f)
        b.upload_imu(s, np.zeros((0, 7)), [0] * n)
    hs = []
    for s in range(S):
        h = C.c_void_p()
        L.check(L.lib().ptl_batch_icp(b._h, s, C.byref(h)))
        hs.append(h)
    maps = [[] for _ in range(S)]
    b.run(1)
    for s in range(S):
        maps[s].append(_map_of(hs[s]))
    b.enqueue(1)
    b.wait()
    for s in range(S):
        maps[s].append(_map_of(hs[s]))
    b.enqueue(1)
    b.wait()
    for s, d in enumerate(ls.DISPLACEMENTS):
        out = b.results(s)
        _check_run(out["kiss_poses"], out["stats"], d, 20, th, (driver, s))
        _check_maps(maps[s], d, 20, th, (driver, s))
    b.close()


# ------------------------------------------------------------------------------------------------ the answer row's tie-break
def _oracle_persistent_tie():
    ref = orc.ICP(ls.MAX_RANGE, ls.MIN_RANGE, initial_threshold=ls.PERSISTENT_TIE_THRESHOLD)
    f0, f1, _, _ = ls.persistent_tie_pair()
    for f in (f0, f1):
        ref.register_frame(f.astype(np.float64), ls.sweep_t01())
    return ref


def _check_persistent_tie(poses, stats, ref, what):
    for k in range(2):
        for key in INT_STATS:
            assert stats[k][key] == ref.stats[k][key], (what, k, key, stats[k][key], ref.stats[k][key])
        D = np.linalg.inv(ref.pose(k)) @ poses[k]
        assert np.linalg.norm(D[:3, 3]) <= POSE_TOL and orc.rot_angle(D) <= POSE_TOL, (what, k, poses[k])
    assert stats[1]["iterations"] == 2 and poses[1][1, 3] == 0.25, (what, stats[1], poses[1])


def test_a_tie_that_outlives_the_first_iteration():
    """64 source points, each exactly between four map points in x and z and 0.25 m from them in y, built so that the first step is exactly
    that 0.25 m on every implementation (tests/helpers/lattice_scenes.py persistent_tie_pair): at the second iteration every point is
    still 4-way tied, and the 8-lane kernel answers from its cached row - (distance, order id) among the row's candidates.  The earliest
    candidates balance and the loop stops after two iterations; any other choice walks on"""
    ref = _oracle_persistent_tie()
    f0, f1, _, _ = ls.persistent_tie_pair()
    th = ls.PERSISTENT_TIE_THRESHOLD
    for form, over in PER_CALL_FORMS.items():
        icp = core.Icp(ls.MAX_RANGE, ls.MIN_RANGE, initial_threshold=th, max_points_per_scan=ls.SWEEP_H * ls.SWEEP_W, **over)
        poses = [icp.register_frame(f, None) for f in (f0, f1)]
        _check_persistent_tie(poses, icp.stats, ref, form)
        icp.close()
    r = core.SeqRunner(2, ls.SWEEP_H * ls.SWEEP_W, 0, max_range=ls.MAX_RANGE, min_range=ls.MIN_RANGE, with_ekf=False, gn_workgroups=32,
                       gn_lanes_per_point=8, gn_threads=512, initial_threshold=th)
    b = core.BatchRunner(2, 2, ls.SWEEP_H * ls.SWEEP_W, 0, max_range=ls.MAX_RANGE, min_range=ls.MIN_RANGE, with_ekf=False, initial_threshold=th)
    for k, f in enumerate((f0, f1)):
        r.upload_scan(k, f)
        for s in range(2):
            b.upload_scan(s, k, f)
    r.upload_imu(np.zeros((0, 7)), [0, 0])
    for s in range(2):
        b.upload_imu(s, np.zeros((0, 7)), [0, 0])
    r.run()
    b.run()
    for what, out in (("seq", r.results()), ("batch 0", b.results(0)), ("batch 1", b.results(1))):
        _check_persistent_tie(out["kiss_poses"], out["stats"], ref, what)
    r.close()
    b.close()
