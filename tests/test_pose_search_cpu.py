"""The pose search, the parts that need no GPU: the numpy restatement the GPU tests compare with
(tests/helpers/pose_search_numpy.py) against a brute force written out in scalars, the C-ABI surface and its refusals before any HIP call,
the candidate set, the top-M selection, the command's option handling, and the precondition of the end-to-end scene."""
import ctypes as C
import os

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from tests.helpers import pose_search_cases as pc
from tests.helpers import pose_search_numpy as psn
from tests.helpers.abi_surface import declared as _declared, exported as _exported, struct_fields as _header_fields

NEW = {"ptl_pose_search_sizeof_cfg", "ptl_pose_search_default_cfg", "ptl_icp_pose_hits"}
PTL_ERR_ARG = -1


# ---------------------------------------------------------------------------------------------- 1. the restatement
def _brute_hits(points, poses, ref, vs, thresholds):
    """hit counts in plain Python floats: the written-order transform, the exact minimum over ALL stored points of the written-order
    expression, the key-range rule - no numpy arithmetic, no neighbourhood"""
    out = []
    for T in poses:
        T = [[float(v) for v in row] for row in np.asarray(T)[:3]]
        if not all(np.isfinite(v) for row in T for v in row):
            out.append([-1] * len(thresholds))
            continue
        cnt = [0] * len(thresholds)
        for q in points:
            qx, qy, qz = (float(v) for v in q)
            w = [((T[r][0] * qx + T[r][1] * qy) + T[r][2] * qz) + T[r][3] for r in range(3)]
            if not all(np.isfinite(v) for v in w) or any(not -(1 << 20) <= int(v / vs) < (1 << 20) for v in w):
                continue
            best = float("inf")
            for p in ref:
                dx, dy, dz = float(p[0]) - w[0], float(p[1]) - w[1], float(p[2]) - w[2]
                d2 = (dx * dx + dy * dy) + dz * dz
                best = d2 if d2 < best else best
            for j, t in enumerate(thresholds):
                cnt[j] += 1 if best <= float(t) * float(t) else 0
        out.append(cnt)
    return np.array(out, dtype=np.int32).reshape(len(poses), len(thresholds))


def test_restatement_against_brute_force_on_the_hand_cases():
    ref, max_dist, thr, (w, q1), poses, want = pc.hand_scene()
    for q in (w, q1):
        got = psn.hits(q, poses, ref, pc.VS, max_dist, thr)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got, _brute_hits(q, poses, ref, pc.VS, thr))
        assert np.array_equal(got, psn.hits(q, poses, ref, pc.VS, max_dist, thr, near=True))
    # the answers computed by hand: the world points under the identity, the same points through the exact pose from its sensor frame
    assert tuple(psn.hits(w, poses, ref, pc.VS, max_dist, thr)[0]) == want
    assert tuple(psn.hits(q1, poses, ref, pc.VS, max_dist, thr)[1]) == want
    assert np.array_equal(psn.transform(q1, poses[1])[[2, 3, 4, 5, 9]], w[[2, 3, 4, 5, 9]])  # (exact: dyadic coordinates, a quarter turn)
    h = psn.hits(w, poses, ref, pc.VS, max_dist, thr)
    assert tuple(h[2]) == (-1, -1)
    s = psn.summary(w, poses, h)
    assert s == dict(n_points=len(w), n_invalid_points=2, n_poses=3, n_invalid_poses=1, best_pose=(0, 0), best_hits=want)
    # no candidate, and only invalid ones: no winner
    none = psn.summary(w, np.zeros((0, 4, 4)), np.zeros((0, 2), dtype=np.int32))
    assert (none["best_pose"], none["best_hits"], none["n_invalid_poses"]) == ((-1, -1), (0, 0), 0)
    only_bad = psn.summary(w, poses[2:], h[2:])
    assert (only_bad["best_pose"], only_bad["best_hits"], only_bad["n_invalid_poses"]) == ((-1, -1), (0, 0), 1)


def test_restatement_on_the_lattice_scene():
    """a subset of the lattice scene small enough for the scalar brute force, exact and general poses; and the neighbour-list path of the
    restatement against its brute-force path on the whole scene"""
    ref, q = pc.lattice_map(), pc.lattice_queries()
    poses = np.concatenate([pc.exact_poses(), pc.general_poses()])
    sub_ref = np.concatenate([ref[:300], pc.BOUNDARY_POINTS])
    sub_q = q[:40]
    got = psn.hits(sub_q, poses[[0, 1, 4, 9, 11]], sub_ref, pc.VS, pc.VS, pc.THRESHOLDS)
    assert np.array_equal(got, _brute_hits(sub_q, poses[[0, 1, 4, 9, 11]], sub_ref, pc.VS, pc.THRESHOLDS))
    full = psn.hits(q, poses, ref, pc.VS, pc.VS, pc.THRESHOLDS)
    assert np.array_equal(full, psn.hits(q, poses, ref, pc.VS, pc.VS, pc.THRESHOLDS, near=True))
    assert (full[:, 1] == full[:, 2]).all() and (np.diff(full, axis=1) >= 0).all() and full.min() > 0
    # the boundary pairs under the identity: at thr^2 and one ulp below it a hit at 0.25, one ulp above it not - five times over
    d2 = psn.mc.dist2(psn.transform(q[:15], np.eye(4)), ref, pc.VS, pc.VS).reshape(5, 3)
    t2 = pc.BOUNDARY_THR * pc.BOUNDARY_THR
    assert (d2[:, 0] == t2).all() and (d2[:, 1] < t2).all() and (d2[:, 2] > t2).all() and (d2[:, 2] <= pc.VS * pc.VS).all()
    # exact poses are exact: the transform of a dyadic point is the same in any order of the sum
    for T in pc.exact_poses():
        w = psn.transform(q[15:], T)
        assert np.array_equal(w, q[15:] @ T[:3, :3].T + T[:3, 3])


# ---------------------------------------------------------------------------------------------- 2. surface
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def test_surface_and_layout_of_the_pose_search():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= exported and NEW <= declared and declared == exported == set(_lib.PROTOTYPES)
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points and new structs change no existing struct or prototype
    # header <-> binding, field by field
    for cname, cls in (("ptl_pose_search_cfg", _lib.PoseSearchCfg), ("ptl_pose_search_result", _lib.PoseSearchResult)):
        want = [(f, CTYPES[t] if n is None else CTYPES[t] * n) for f, t, n in _header_fields(cname)]
        assert [(f, t) for f, t in cls._fields_] == want, cname
    assert L.ptl_pose_search_sizeof_cfg() == C.sizeof(_lib.PoseSearchCfg) == 56
    assert C.sizeof(_lib.PoseSearchResult) == 4 * 8 + 2 * 32 + 8 + 8 + 32 + 8
    from ptudes_lab_amd import core, fly
    assert hasattr(core.Icp, "pose_hits") and hasattr(core, "PoseHits") and hasattr(fly, "MapLocalizer") and hasattr(fly, "candidate_poses")
    assert core.build_info()["pose_chunk"] >= 2

    cfg = _lib.PoseSearchCfg()
    assert L.ptl_pose_search_default_cfg(C.byref(cfg), 0.5) == 0
    assert (cfg.max_dist, cfg.n_thresholds, list(cfg.thresholds)) == (0.5, 1, [0.5, 0.0, 0.0, 0.0]) and (cfg.struct_size, cfg.abi_version) == (56, 6)

    # a short, a long and a stale struct are refused without a byte written: the struct sits in front of a canary
    class Guarded(C.Structure):
        _fields_ = [("cfg", _lib.PoseSearchCfg), ("canary", C.c_uint8 * 32)]

    res = _lib.PoseSearchResult()
    xyz, poses = np.zeros((4, 3)), np.tile(np.eye(4), (2, 1, 1))
    for size, abi in ((48, 6), (56, 5), (64, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.cfg.struct_size, g.cfg.abi_version = size, abi
        before = bytes(g)
        rc = L.ptl_pose_search_default_cfg(C.cast(C.byref(g), C.POINTER(_lib.PoseSearchCfg)), 0.5)
        msg = L.ptl_last_error().decode()
        assert rc == PTL_ERR_ARG and str(size) in msg and str(abi) in msg and "56" in msg, msg
        assert bytes(g) == before
    assert L.ptl_pose_search_default_cfg(None, 0.5) == PTL_ERR_ARG
    cfg2 = _lib.PoseSearchCfg()
    assert L.ptl_pose_search_default_cfg(C.byref(cfg2), 0.0) == PTL_ERR_ARG and cfg2.max_dist == 0.0
    # no handle: refused before any HIP call (this machine may have no device at all)
    assert L.ptl_icp_pose_hits(None, C.byref(cfg), _lib.dptr(xyz), 4, _lib.dptr(poses), 2, C.byref(res), None) == PTL_ERR_ARG
    assert "null" in L.ptl_last_error().decode()
    assert L.ptl_icp_pose_hits(None, None, None, 0, None, 0, None, None) == PTL_ERR_ARG


# ---------------------------------------------------------------------------------------------- 3. candidates and selection
def test_candidate_poses_order_first_yaw_and_thinning():
    from ptudes_lab_amd import fly
    rng = np.random.default_rng(3)
    kf = np.array([pc.pose(rng.normal(size=3), (0.7 * i, 0.1 * i * i, 0.0)) for i in range(9)])
    cand, kept = fly.candidate_poses(kf, 8)
    assert cand.shape == (72, 4, 4) and list(kept) == list(range(9))
    for a in range(9):
        assert cand[8 * a].tobytes() == kf[a].tobytes()  # j = 0: the keyframe itself, bit for bit
        for j in range(1, 8):
            c, s = np.cos(2 * np.pi * j / 8), np.sin(2 * np.pi * j / 8)
            Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
            assert np.abs(cand[8 * a + j] - kf[a] @ Rz).max() < 1e-15 and np.array_equal(cand[8 * a + j][:3, 3], kf[a][:3, 3])
    # thinning by travelled distance: the path length since the last kept keyframe, along all keyframes
    step = np.linalg.norm(np.diff(kf[:, :3, 3], axis=0), axis=1)
    want, since = [0], 0.0
    for i in range(1, 9):
        since += step[i - 1]
        if since >= 2.0:
            want.append(i)
            since = 0.0
    cand2, kept2 = fly.candidate_poses(kf, 4, spacing=2.0)
    assert list(kept2) == want and 1 < len(want) < 9 and cand2.shape == (4 * len(want), 4, 4)
    assert all(cand2[4 * a].tobytes() == kf[i].tobytes() for a, i in enumerate(want))
    assert list(fly.candidate_poses(kf, 1, spacing=1.0e9)[1]) == [0]  # the first keyframe is always kept
    assert list(fly.candidate_poses(kf, 1, spacing=0.0)[1]) == list(range(9))
    assert fly.candidate_poses(np.zeros((0, 4, 4)), 4)[0].shape == (0, 4, 4)
    with pytest.raises(ValueError, match="n_yaw = 0"):
        fly.candidate_poses(kf, 0)
    with pytest.raises(ValueError, match="spacing = -1"):
        fly.candidate_poses(kf, 4, spacing=-1.0)


def test_top_candidates_break_ties_by_index():
    from ptudes_lab_amd import fly
    h = np.array([5, 9, 9, -1, 7, 9, 5, 0], dtype=np.int32)
    assert list(fly.top_candidates(h, 1)) == [1]
    assert list(fly.top_candidates(h, 4)) == [1, 2, 5, 4]
    assert list(fly.top_candidates(h, 6)) == [1, 2, 5, 4, 0, 6]
    assert list(fly.top_candidates(h, 100)) == [1, 2, 5, 4, 0, 6, 7]  # the invalid candidate never qualifies
    assert list(fly.top_candidates(np.array([-1, -1]), 3)) == [] and list(fly.top_candidates(h, 0)) == []


# ---------------------------------------------------------------------------------------------- 4. option handling
def test_localize_refuses_options_before_any_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    r = run(ptudes_cli, ["localize", "--help"])
    assert r.exit_code == 0
    for opt in ("--map", "--keyframes", "--yaws", "--keyframe-spacing", "--top", "--min-fraction", "--query-voxel", "--start-scan", "--end-scan",
                "--save-nc-gt-poses", "--save-kitti-poses", "--synthetic", "-m"):
        assert opt in r.output, opt
    m, k = tmp_path / "map.npy", tmp_path / "kf.csv"
    np.save(str(m), np.zeros((3, 3)))
    k.write_text("")
    base = ["localize", "--synthetic", "1000", "--map", str(m), "--keyframes", str(k)]
    for args, words in ((["localize", "--synthetic", "1"], ["--map"]),
                        (["localize", "--synthetic", "1", "--map", str(tmp_path / "no.ply"), "--keyframes", str(k)], ["no such file"]),
                        (["localize", "--synthetic", "1", "--map", str(k), "--keyframes", str(k)], [".ply or .npy"]),
                        (["localize", "--synthetic", "1", "--map", str(m)], ["--keyframes"]),
                        (["localize", "--synthetic", "1", "--map", str(m), "--keyframes", str(tmp_path / "no.csv")], ["no such file"]),
                        (base + ["--yaws", "0"], ["--yaws 0"]),
                        (base + ["--keyframe-spacing", "-1"], ["--keyframe-spacing -1"]),
                        (base + ["--top", "0"], ["--top 0"]),
                        (base + ["--min-fraction", "1.5"], ["--min-fraction 1.5", "[0, 1]"]),
                        (base + ["--query-voxel", "0"], ["--query-voxel 0"]),
                        (base + ["--start-scan", "-2"], ["--start-scan -2"]),
                        (base + ["--start-scan", "5", "--end-scan", "3"], ["--end-scan 3", "--start-scan 5"]),
                        (base + ["--synthetic-size", "32"], ["--synthetic-size 32", "HxW"]),
                        (["localize", "--map", str(m), "--keyframes", str(k)], ["SOURCE or --synthetic"]),
                        (["localize", str(m), "--map", str(m), "--keyframes", str(k)], [".bag"]),
                        (["localize", str(m), "--map", str(m), "--keyframes", str(k), "--synthetic-size", "32x256"], ["belongs to --synthetic"]),
                        (base, ["no pose in the file"])):
        r = run(ptudes_cli, args)
        assert r.exit_code != 0 and all(w in r.output for w in words), (args, r.output)
    r = run(ptudes_cli, ["ekf-bench", "ouster", "--synthetic-size", "32x256"])
    assert r.exit_code != 0 and "belongs to --synthetic" in r.output


# ---------------------------------------------------------------------------------------------- 5. the end-to-end scene's precondition
def test_the_true_candidate_leads_in_the_end_to_end_scene():
    """tests/test_gpu_pose_search.py's end-to-end test expects the search to pick (keyframe 9, yaw 0); that this is what the definition
    gives is checked here, in the restatement: at the last threshold (0.5 m) the true candidate's hits exceed every other candidate's.
    Measured: candidate 48 has 1804 hits of 2768 query points, the best other (candidate 32: keyframe 6, yaw 0) 1044 - a margin of 760."""
    from ptudes_lab_amd import fly
    s, e = pc.end_to_end_scene(), pc.E2E
    cand, kept = fly.candidate_poses(s["keyframes"], e["n_yaw"])
    assert len(cand) == 64 and cand[e["true_candidate"]].tobytes() == s["gt"][9].tobytes()
    h = psn.hits(s["query"], cand, s["map_points"], pc.VS, pc.VS, (pc.VS,), near=True)[:, -1]
    others = np.delete(h, e["true_candidate"])
    print(f"true candidate {e['true_candidate']}: {h[e['true_candidate']]} hits of {len(s['query'])}; best other: candidate "
          f"{int(np.argmax(np.where(np.arange(64) == e['true_candidate'], -1, h)))} with {others.max()}; margin {h[e['true_candidate']] - others.max()}")
    assert h[e["true_candidate"]] > others.max()
    assert list(fly.top_candidates(h, 1)) == [e["true_candidate"]]
