"""The pose search on the device (csrc/pose_kernels.h) against its numpy restatement (tests/helpers/pose_search_numpy.py):
the written-order transform followed by brute force over `map_points()` of the handle.  Every output is a count of integers: `hits`, the
best candidate and the counts of invalid inputs are compared exactly, without tolerances.  The one tolerance of this file belongs to the
end-to-end test and is derived there from the registration's own start-dependence.

Per-call `core.Icp` maps with small capacities."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.helpers import pose_search_cases as pc
from tests.helpers import pose_search_numpy as psn

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
PTL_ERR_ARG, PTL_ERR_CAPACITY = -1, -3


def _icp(voxel=pc.VS, P=20, n_max=1 << 14, **over):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    kw = dict(voxel_size=voxel, max_points_per_voxel=P, max_points_per_scan=n_max, **CAPS)
    kw.update(over)
    return core.Icp(1.0e9, 0.0, **kw)


def _lex(a):
    return np.lexsort(a.T[::-1])


def _check(icp, q, poses, max_dist=None, thresholds=None, what="", near=False):
    """pose_hits against the restatement over the handle's stored points: hits, best candidate and counts, exactly"""
    md = icp.cfg.voxel_size if max_dist is None else max_dist
    thr = (md,) if thresholds is None else tuple(thresholds)
    s, hits = icp.pose_hits(q, poses, max_dist=max_dist, thresholds=thresholds)
    want = psn.hits(q, poses, icp.map_points(), icp.cfg.voxel_size, md, thr, near=near)
    assert hits.dtype == np.int32 and hits.shape == want.shape, what
    bad = np.argwhere(hits != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], hits[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
    ws = psn.summary(q, poses, want)
    assert (s.n_points, s.n_invalid_points, s.n_poses, s.n_invalid_poses) == (ws["n_points"], ws["n_invalid_points"], ws["n_poses"], ws["n_invalid_poses"]), what
    assert (s.best_pose, s.best_hits) == (ws["best_pose"], ws["best_hits"]), (what, s, ws)
    assert s.max_dist == md and s.thresholds == thr
    return s, hits


@pytest.fixture(scope="module")
def lattice():
    icp = _icp()
    icp.map_add(pc.lattice_map())
    pts = icp.map_points()
    _, counts = np.unique(np.trunc(pts / pc.VS).astype(np.int64), axis=0, return_counts=True)
    assert counts.min() == 1 and counts.max() == 20 and len(pts) < len(pc.lattice_map()), "one to twenty points per voxel, and the cap binds"
    yield icp
    icp.close()


# 1. lattice maps: exact poses (the transform is exact), boundary pairs, equal thresholds; general rotations on the same map
def test_lattice_map_exact_and_general_poses(lattice):
    q = pc.lattice_queries()
    s, hits = _check(lattice, q, pc.exact_poses(), thresholds=pc.THRESHOLDS, what="exact poses")
    assert (hits[:, 1] == hits[:, 2]).all() and hits.min() > 0
    # the boundary pairs alone under the identity: at thr^2 and just below it a hit, just above it none - at a face, inside a voxel, in voxel 0
    b, hb = _check(lattice, q[:15], pc.exact_poses()[:1], thresholds=(pc.BOUNDARY_THR, pc.VS), what="boundary pairs")
    assert tuple(hb[0]) == (10, 15)
    for i in range(15):
        _, h1 = lattice.pose_hits(q[i:i + 1], pc.exact_poses()[:1], thresholds=(pc.BOUNDARY_THR,))
        assert h1[0, 0] == (0 if i % 3 == 2 else 1), i
    _check(lattice, q, pc.general_poses(), thresholds=pc.THRESHOLDS, what="general poses")
    _check(lattice, q, np.concatenate([pc.general_poses(), pc.exact_poses()]), max_dist=0.375, thresholds=(0.375,), what="max_dist below vs")


# 2. sizes around the mapping's edges
def test_point_and_candidate_counts(lattice):
    from ptudes_lab_amd import core
    chunk = core.build_info()["pose_chunk"]
    q = pc.lattice_queries()
    base = np.concatenate([pc.general_poses(), pc.exact_poses()])
    for n in (0, 1, 2, 3, 7, 8, 9, 255, 256, 257):
        for thr in ((pc.VS,), pc.THRESHOLDS):
            s, hits = _check(lattice, q[len(q) - n:], base[:3], thresholds=thr, what=f"n = {n}")
            if n == 0:  # the zero summary: no points, no hits, the first valid candidate leads with none
                assert (s.n_points, s.n_invalid_points, s.best_hits, s.best_pose) == (0, 0, (0,) * len(thr), (0,) * len(thr)) and not hits.any()
    rng = np.random.default_rng(41)
    for K in (0, 1, 2, chunk - 1, chunk, chunk + 1):
        poses = base[rng.integers(0, len(base), K)]
        for thr in ((pc.VS,), pc.THRESHOLDS):
            s, hits = _check(lattice, q[:9], poses, thresholds=thr, what=f"K = {K}")
            assert hits.shape == (K, len(thr))
            if K == 0:
                assert (s.best_pose, s.best_hits, s.n_poses) == ((-1,) * len(thr), (0,) * len(thr), 0)
    z = lattice.pose_hits(np.zeros((0, 3)), np.zeros((0, 4, 4)), per_pose=False)
    assert (z.n_points, z.n_poses, z.best_pose, z.best_hits, z.device_ms) == (0, 0, (-1,), (0,), 0.0)


# 3. invalid and out-of-range inputs
def test_invalid_points_poses_and_the_empty_map(lattice):
    from ptudes_lab_amd import core
    chunk = core.build_info()["pose_chunk"]
    q = pc.lattice_queries()[15:60].copy()
    q[4, 1], q[17, 0], q[30, 2] = np.nan, np.inf, -np.inf
    s, hits = _check(lattice, q, pc.exact_poses(), thresholds=pc.THRESHOLDS, what="non-finite points")
    assert s.n_invalid_points == 3  # (once each, not per candidate)
    # a NaN / inf candidate in the first, a middle and the last position of a chunk, and in the second chunk's first
    base = np.concatenate([pc.general_poses(), pc.exact_poses()])
    poses = base[np.arange(chunk + 2) % len(base)].copy()
    poses[0, 0, 0], poses[chunk // 2, 1, 3], poses[chunk - 1, 2, 2], poses[chunk, 0, 1] = np.nan, np.inf, np.nan, -np.inf
    poses[3, 3, 0] = np.nan  # (the bottom row is not read)
    s, hits = _check(lattice, q[:9], poses, thresholds=(0.25, pc.VS), what="non-finite candidates")
    assert s.n_invalid_poses == 4 and (hits[[0, chunk // 2, chunk - 1, chunk]] == -1).all() and (np.delete(hits, [0, chunk // 2, chunk - 1, chunk], 0) >= 0).all()
    # only invalid candidates: no winner
    s, hits = _check(lattice, q[:9], poses[[0, chunk // 2]], what="no valid candidate")
    assert (s.best_pose, s.best_hits, s.n_invalid_poses) == ((-1,), (0,), 2) and (hits == -1).all()
    # beyond the key range (2^20 voxels either side), and an overflow to inf on the way: zeros
    far = np.array([pc.pose(t=(0.5 * 2.0 ** 21, 0.0, 0.0)), pc.pose(t=(0.0, -1.0e300, 0.0)), pc.pose(t=(1.0e308, 0.0, 0.0)) * 1.0])
    far[2, 0, 0] = 1.0e308
    s, hits = _check(lattice, pc.lattice_queries(), far, what="out of range")
    assert not hits.any() and s.best_pose == (0,) and s.n_invalid_poses == 0
    # the smallest index among equal maxima
    same = base[[5, 2, 7, 2, 2, 7, 5]]
    s, hits = _check(lattice, pc.lattice_queries(), same, thresholds=pc.THRESHOLDS, what="equal maxima")
    for j in range(4):
        assert s.best_pose[j] == int(np.flatnonzero(hits[:, j] == hits[:, j].max())[0]) and (hits[:, j] == hits[:, j].max()).sum() >= 2
    empty = _icp()
    s, hits = _check(empty, q, base, thresholds=pc.THRESHOLDS, what="empty map")
    assert not hits.any() and s.best_pose == (0,) * 4 and s.n_invalid_points == 3
    empty.close()


# 4. second witness: the existing device path on points the host transformed in the written order
def test_second_witness_map_distance(lattice):
    q = pc.lattice_queries()
    poses = np.concatenate([pc.exact_poses(), pc.general_poses()])
    _, hits = lattice.pose_hits(q, poses, thresholds=pc.THRESHOLDS)
    for k, T in enumerate(poses):
        assert tuple(hits[k]) == lattice.map_distance(psn.transform(q, T), thresholds=pc.THRESHOLDS).n_within, k


# 5. read-only and repeatable
def _table_bytes(icp):
    from ptudes_lab_amd import _lib as L
    info = (C.c_int64 * 8)()
    L.check(L.lib().ptl_icp_debug_table(icp._h, None, 0, None, None, 0, info))
    slots, blocks = info[3] + 1, info[6]
    ent, bhdr, bfirst = np.empty(slots * 16, dtype=np.uint8), np.empty((blocks, 4), dtype=np.int32), np.empty((blocks, 3))
    L.check(L.lib().ptl_icp_debug_table(icp._h, ent.ctypes.data_as(C.c_void_p), slots, bhdr.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(bfirst),
                                        blocks, info))
    return ent.tobytes() + bhdr.tobytes() + bfirst.tobytes() + bytes(info)


def test_read_only_repeatable_and_independent_of_insertion_order():
    q = pc.lattice_queries()
    poses = np.concatenate([pc.exact_poses(), pc.general_poses()])
    # (every voxel below its cap, so that the stored SET does not depend on the order of insertion)
    cloud = pc.first_per_voxel(pc.lattice_map(), pc.VS, cap=20)
    a, b = _icp(), _icp()
    a.map_add(cloud)
    b.map_add(cloud[::-1])
    pa, pb = a.map_points(), b.map_points()
    assert len(pa) == len(cloud) and np.array_equal(pa[_lex(pa)], pb[_lex(pb)]) and not np.array_equal(pa, pb)
    table, pts = _table_bytes(a), pa.tobytes()
    s1, h1 = a.pose_hits(q, poses, thresholds=pc.THRESHOLDS)
    s2, h2 = a.pose_hits(q, poses, thresholds=pc.THRESHOLDS)
    s3 = a.pose_hits(q, poses, thresholds=pc.THRESHOLDS, per_pose=False)
    assert h1.tobytes() == h2.tobytes()
    for x in (s2, s3):
        assert (x.best_pose, x.best_hits, x.n_invalid_points, x.n_invalid_poses, x.n_points, x.n_poses) == \
               (s1.best_pose, s1.best_hits, s1.n_invalid_points, s1.n_invalid_poses, s1.n_points, s1.n_poses)
    assert _table_bytes(a) == table and a.map_points().tobytes() == pts
    sb, hb = b.pose_hits(q, poses, thresholds=pc.THRESHOLDS)
    assert np.array_equal(hb, h1) and (sb.best_pose, sb.best_hits) == (s1.best_pose, s1.best_hits)
    for h in (a, b):
        h.close()


def _refused(code, fn):
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn()
    if code == PTL_ERR_ARG:
        assert isinstance(e.value, ValueError)
    else:
        assert f"libptudes_mi error {code}:" in str(e.value), str(e.value)
    return str(e.value)


# 6. refusals before any HIP call: each names its numbers
def test_refusals(lattice):
    from ptudes_lab_amd import _lib
    q, poses = np.zeros((3, 3)), np.tile(np.eye(4), (2, 1, 1))
    msg = _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, max_dist=0.75))
    assert "max_dist = 0.75" in msg and "voxel size = 0.5" in msg
    assert "max_dist = 0" in _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, max_dist=0.0))
    _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, max_dist=float("nan")))
    msg = _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, thresholds=[0.2, 0.1]))
    assert "threshold 1 = 0.1" in msg and "threshold 0 = 0.2" in msg and "ascending" in msg
    assert "n_thresholds = 5" in _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, thresholds=[0.1] * 5))
    assert "n_thresholds = 0" in _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, thresholds=[]))
    msg = _refused(PTL_ERR_ARG, lambda: lattice.pose_hits(q, poses, thresholds=[0.1, 0.6]))
    assert "threshold 1 = 0.6" in msg and "max_dist = 0.5" in msg
    big = np.zeros(((1 << 20) + 1, 3))
    msg = _refused(PTL_ERR_CAPACITY, lambda: lattice.pose_hits(big, poses))
    assert str((1 << 20) + 1) in msg and str(1 << 20) in msg
    L = _lib.lib()
    cfg = _lib.PoseSearchCfg()
    _lib.check(L.ptl_pose_search_default_cfg(C.byref(cfg), 0.5))
    res = _lib.PoseSearchResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    blank = b"\x5a" * C.sizeof(res)
    hits = np.full((2, 1), -7, dtype=np.int32)
    hp = hits.ctypes.data_as(C.POINTER(C.c_int32))
    for args, words in (((_lib.dptr(q), -1, _lib.dptr(poses), 2), ["n = -1"]), ((None, 3, _lib.dptr(poses), 2), ["3 query points"]),
                        ((_lib.dptr(q), 3, _lib.dptr(poses), -4), ["n_poses = -4"]), ((_lib.dptr(q), 3, None, 2), ["2 candidates"])):
        assert L.ptl_icp_pose_hits(lattice._h, C.byref(cfg), args[0], args[1], args[2], args[3], C.byref(res), hp) == PTL_ERR_ARG
        assert all(w in L.ptl_last_error().decode() for w in words) and bytes(res) == blank and (hits == -7).all()
    # a foreign-size cfg: both sizes named, nothing written
    cfg.struct_size = 48
    assert L.ptl_icp_pose_hits(lattice._h, C.byref(cfg), _lib.dptr(q), 3, _lib.dptr(poses), 2, C.byref(res), hp) == PTL_ERR_ARG
    assert "48" in L.ptl_last_error().decode() and "56" in L.ptl_last_error().decode() and bytes(res) == blank and (hits == -7).all()
    # the handle is as usable as before; a null cfg takes the defaults
    assert L.ptl_icp_pose_hits(lattice._h, None, _lib.dptr(q), 3, _lib.dptr(poses), 2, C.byref(res), hp) == 0
    assert (res.max_dist, res.n_thresholds, res.thresholds[0], res.n_points, res.n_poses) == (0.5, 1, 0.5, 3, 2) and (hits >= 0).all()


# 7. end to end
# The registration's own start-dependence on this scene: Icp.align of the query on the map from the true pose of sweep 11 and from
# SPREAD_STARTS starts perturbed by up to half the candidate spacing (one keyframe step, 11.25 degrees of yaw).  The spread is the largest
# difference among those nine results; `locate` must come within twice that of the from-truth result.  The test measures the spread on the
# device at every run, prints it, and holds it against the figures recorded here, so that a change of the yardstick itself shows.
# Measured on an MI355X: spread 0.771 m and 0.349 rad; bound 1.542 m and 0.699 rad; `locate` against from-truth: 1.69e-3 m and 2.79e-5 rad.
# Of the eight perturbed starts four end within 5.8e-5 m and 2.3e-6 rad of the from-truth result and one within 1.7e-3 m and 2.8e-5 rad;
# three end in other minima (0.771 m / 0.152 rad, 0.626 m / 0.175 rad, 0.056 m / 0.175 rad): at sigma = 2 m the registration itself does
# not hold this scene from every start within half the candidate spacing.  The issue's bound is therefore loose here (it would pass a
# `locate` that is 1.5 m off); it is kept as the issue states it, and the test prints every start's result.
SPREAD_STARTS = 8
MEASURED_SPREAD_T, MEASURED_SPREAD_R = 0.771, 0.349  # metres, radians


def _rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


@pytest.fixture(scope="module")
def scene():
    return pc.end_to_end_scene()


def test_end_to_end_locate_and_track(scene):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core, fly
    e = pc.E2E
    m = core.map_from_points(scene["map_points"], voxel_size=pc.VS, max_points_per_scan=1 << 16, map_block_capacity=1 << 17,
                             map_table_capacity=1 << 19)
    pts = m.map_points()
    assert np.array_equal(pts[_lex(pts)], scene["map_points"][_lex(scene["map_points"])]), "the device map holds the restatement's stored set"
    loc = fly.MapLocalizer(m, scene["keyframes"], n_yaw=e["n_yaw"], top=4, query_voxel=e["query_voxel"])
    q = loc.query(scene["sweeps"][11])
    assert np.array_equal(q[_lex(q)], scene["query"][_lex(scene["query"])]), "the first point per voxel, as the restatement takes it"
    # the search: the device's best candidate is the restatement's, (keyframe 9, yaw 0) by the CPU test's precondition
    s, hits = _check(m, q, loc.candidates, what="end to end", near=True)
    assert s.best_pose == (e["true_candidate"],)
    fix = loc.locate(scene["sweeps"][11])
    assert fix.candidate == e["true_candidate"] and fix.n_query == len(q) and fix.hits == round(fix.fraction * len(q))
    sigma = float(m.cfg.initial_threshold)
    want, it = m.align(q, loc.candidates[e["true_candidate"]], 3.0 * sigma, sigma / 3.0)
    assert fix.pose.tobytes() == want.tobytes() and fix.iterations == it
    assert fix.hits == m.pose_hits(q, want[None])[1][0, -1] and 0 <= fix.runner_up_hits <= fix.hits
    # accuracy, judged against the registration itself
    truth = scene["gt"][11]
    from_truth, _ = m.align(q, truth, 3.0 * sigma, sigma / 3.0)
    half_step = 0.5 * max(float(np.linalg.norm(scene["gt"][b][:3, 3] - scene["gt"][a][:3, 3])) for a, b in ((0, 3), (3, 6), (6, 9)))
    half_yaw = 0.5 * 2.0 * np.pi / e["n_yaw"]
    rng = np.random.default_rng(13)
    results = [from_truth]
    for _ in range(SPREAD_STARTS):
        d = rng.normal(size=3)
        start = truth @ pc.pose((0.0, 0.0, rng.uniform(-half_yaw, half_yaw)), half_step * rng.uniform(0.0, 1.0) * d / np.linalg.norm(d))
        results.append(m.align(q, start, 3.0 * sigma, sigma / 3.0)[0])
    spread_t = max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a in results for b in results)
    spread_r = max(_rot_angle(a[:3, :3], b[:3, :3]) for a in results for b in results)
    err_t, err_r = float(np.linalg.norm(fix.pose[:3, 3] - from_truth[:3, 3])), _rot_angle(fix.pose[:3, :3], from_truth[:3, :3])
    print("perturbed starts against from-truth (m, rad): " + ", ".join(
        f"({np.linalg.norm(r[:3, 3] - from_truth[:3, 3]):.2e}, {_rot_angle(r[:3, :3], from_truth[:3, :3]):.2e})" for r in results[1:]))
    print(f"start-dependence of Icp.align over {SPREAD_STARTS} perturbed starts (half step {half_step:.4f} m, half yaw {np.degrees(half_yaw):.3f} deg): "
          f"{spread_t:.3e} m, {spread_r:.3e} rad; locate against from-truth: {err_t:.3e} m, {err_r:.3e} rad; bound {2 * spread_t:.3e} m, {2 * spread_r:.3e} rad")
    assert err_t <= 2.0 * spread_t and err_r <= 2.0 * spread_r
    assert spread_t <= 2.0 * MEASURED_SPREAD_T and spread_r <= 2.0 * MEASURED_SPREAD_R, "the yardstick moved: the recorded spread no longer describes it"
    # a sweep without a return is refused in words, before any device work
    with pytest.raises(ValueError, match="no return"):
        loc.locate(np.zeros((64, 3), dtype=np.float32))
    # a sweep of another scene fits worse
    wrong = fly.MapLocalizer(m, scene["keyframes"], n_yaw=e["n_yaw"], top=4, query_voxel=e["query_voxel"]).locate(scene["other_sweep"])
    print(f"fraction: true scene {fix.fraction:.4f}, another scene {wrong.fraction:.4f}")
    assert wrong.fraction < fix.fraction
    # track over sweeps 10 and 11: one search, then no re-localisation; the map is never added to
    tr = fly.MapLocalizer(m, scene["keyframes"], n_yaw=e["n_yaw"], top=4, query_voxel=e["query_voxel"])
    f10, f11 = tr.track(scene["sweeps"][10]), tr.track(scene["sweeps"][11])
    assert tr.relocalizations == 0 and f10.candidate == e["true_candidate"] and f11.candidate == -1 and len(tr.fixes) == 2
    assert f11.fraction >= tr.min_fraction and tr.search_ms > 0.0
    after = m.map_points()
    assert np.array_equal(after[_lex(after)], pts[_lex(pts)])
    m.close()


# 8. the command
def test_localize_command_on_the_map_a_run_saved(tmp_path):
    from click.testing import CliRunner
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    ply, kf, out_csv, out_kitti = (str(tmp_path / n) for n in ("map.ply", "kf.csv", "loc.csv", "loc.txt"))
    size = ["--synthetic", "1000", "--synthetic-size", "32x256", "--end-scan", "6"]
    res = run(ptudes_cli, ["ekf-bench", "ouster"] + size + ["--use-imu-prediction", "--save-map", ply, "--save-nc-gt-poses", kf])
    assert res.exit_code == 0, res.output
    res = run(ptudes_cli, ["localize"] + size + ["--map", ply, "--keyframes", kf, "--save-nc-gt-poses", out_csv, "--save-kitti-poses", out_kitti])
    assert res.exit_code == 0, res.output
    rows = pu.read_newer_college_gt(out_csv)
    assert len(rows) == 7 and len(np.loadtxt(out_kitti).reshape(-1, 12)) == 7
    assert re.search(r"sweeps localised: 7\b", res.output) and re.search(r"re-localisations: 0\b", res.output), res.output
    m = re.search(r"mean hit fraction: (\S+)", res.output)
    assert m and 0.5 <= float(m.group(1)) <= 1.0 and re.search(r"search device time: \S+ ms", res.output), res.output
    # the sweeps' poses are the mapping run's, to within the voxel size: the recording is the one the map was made from
    mapped = pu.read_newer_college_gt(kf)
    assert max(float(np.linalg.norm(a[1][:3, 3] - b[1][:3, 3])) for a, b in zip(rows, mapped)) < pc.VS
