"""Free space carved on the device (csrc/carve_kernels.h) against its numpy restatement (tests/helpers/map_carve_numpy.py).
Every output is an integer, so everything is compared for equality: `through` and `support` of EVERY stored point (rows matched after a
lexicographic sort of (x, y, z, through, support): the pool order is unspecified) and every count of the summary.  The restatement takes the
map's stored points from the device (`map_points()`) and the column poses from the device (`traj_poses_at`, the one definition of the
geodesic): which points a voxel keeps and where a column's pose lies are tested elsewhere; what is tested here is the march and the vote.

Per-call `core.Icp` maps with small capacities; sweeps of 8 x 32 or smaller unless the case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import map_carve_cases as cc
from tests.helpers import map_carve_numpy as cv

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
PTL_ERR_ARG, PTL_ERR_CAPACITY, PTL_ERR_STATE = -1, -3, -4
VS = 0.5
BOUNDS = 0.5


def _core():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    return core


def _icp(W, n_max, vs=VS, P=20, **over):
    kw = dict(voxel_size=vs, max_points_per_voxel=P, scan_cols=W, max_points_per_scan=n_max, **CAPS)
    kw.update(over)
    return _core().Icp(1.0e9, 0.0, **kw)


def _lex(p):
    p = np.asarray(p, dtype=np.float64)
    return np.ascontiguousarray(p[np.lexsort(p.T[::-1])])


def _cfg_of(votes):
    return dict(radius=votes.radius, margin=votes.margin, step=votes.step, min_range=votes.min_range, max_range=votes.max_range)


def _check(map_icp, votes, sweeps, what=""):
    """a core.CarveVotes against the restatement on the handle's stored points: every point's two counts, every count of the summary"""
    stored = map_icp.map_points()
    assert votes.n_points == len(stored) == len(votes.xyz) == len(votes.through) == len(votes.support), what
    assert votes.through.dtype == np.uint32 and votes.support.dtype == np.uint32
    t, s, n = cv.carve(stored, sweeps, float(map_icp.cfg.voxel_size), _cfg_of(votes))
    got, want = cv.sorted_rows(votes.xyz, votes.through, votes.support), cv.sorted_rows(stored, t, s)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), got[bad[:5]], want[bad[:5]])
    for k in cv.COUNTS:
        assert getattr(votes, k) == n[k], (what, k, getattr(votes, k), n[k])
    return n


class _Knots:
    """a trajectory that rotates and translates within a sweep: knots every 50 ms"""

    def __init__(self, n_sweeps, dt=0.1, seed=0):
        from ptudes_lab_amd.utils import exp_pose6
        rng = np.random.default_rng(seed)
        self.dt = dt
        self.ts = np.arange(-1, 2 * n_sweeps + 2) * (dt / 2)
        twist = np.concatenate([rng.uniform(-0.6, 0.6, 3), rng.uniform(-2.0, 2.0, 3)])
        self.poses = np.array([exp_pose6(twist * t) for t in self.ts])
        self.traj = _core().Traj(self.ts, self.poses, BOUNDS, BOUNDS)

    def col_ts(self, k, W):
        return k * self.dt + (np.arange(W) / W) * self.dt

    def col_poses(self, ts):
        out, n_out = _core().traj_poses_at(self.ts, self.poses, ts, BOUNDS, BOUNDS)
        assert n_out == 0
        return out


def _random_sweeps(rng, n, H, W, reach=6.0, holes=0.1):
    """n sweeps of H x W f32 points in the sensor frame, (0, 0, 0) = no return; a few beyond any max_range used here"""
    out = []
    for _ in range(n):
        u = rng.normal(size=(H, W, 3))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        r = rng.uniform(0.2, reach, (H, W, 1)) * np.where(rng.random((H, W, 1)) < 0.03, 20.0, 1.0)
        x = (u * r).astype(np.float32)
        x[rng.random((H, W)) < holes] = 0.0
        out.append(x)
    return out


def _build_and_carve(H, W, P, n_sweeps=6, seed=0, cfg=None, order=None, vs=VS):
    """a map of n sweeps on a moving trajectory, carved by the same sweeps through the per-call xyz path: (map, carver, numpy sweeps)"""
    core = _core()
    rng = np.random.default_rng(seed)
    kn = _Knots(n_sweeps, seed=seed)
    xyz = _random_sweeps(rng, n_sweeps, H, W)
    m = _icp(W, max(H * W, 64), vs=vs, P=P)
    for k in range(n_sweeps):
        assert m.map_add_posed(kn.traj, kn.col_ts(k, W), xyz=xyz[k], H=H)[1] is False
    car = core.Carver(m, **(cfg or {}))
    sweeps = []
    for k in (range(n_sweeps) if order is None else order):
        ts = kn.col_ts(k, W)
        n_rays, skipped = car.add_posed(kn.traj, ts, xyz=xyz[k], H=H)
        sw = cv.rays_of_sweep(xyz[k].astype(np.float64), np.any(xyz[k] != 0.0, axis=2), kn.col_poses(ts))
        sweeps.append(sw)
        assert not skipped
    return m, car, sweeps, (kn, xyz)


# 1. the answers computed by hand
def test_hand_cases():
    core = _core()
    for case in cc.hand_cases():
        m = _icp(cc.W, 64, P=20)
        m.map_add(case["stored"])
        assert m.map_size()[1] == len(case["stored"]), case["name"]
        pose = np.eye(4)
        pose[:3, 3] = case["origin"]
        traj = core.Traj([0.0, 1.0], [pose, pose], BOUNDS, BOUNDS)
        ts = 0.25 + np.arange(cc.W) / 16.0
        poses, n_out = core.traj_poses_at([0.0, 1.0], [pose, pose], ts, BOUNDS, BOUNDS)
        assert n_out == 0 and (poses == pose[None]).all(), "the geodesic between equal poses is that pose, bit for bit"
        car = core.Carver(m, **case["cfg"])
        n_rays, skipped = car.add_posed(traj, ts, xyz=case["xyz"], H=1)
        v = car.votes()
        assert (n_rays, skipped) == (v.n_rays, False)
        n = _check(m, v, [cc.case_rays(case, poses)], case["name"])
        by_point = {p.tobytes(): (int(t), int(s)) for p, t, s in zip(v.xyz, v.through, v.support)}
        got = [list(by_point[np.ascontiguousarray(p).tobytes()]) for p in case["stored"]]
        assert got == case["expect"].tolist(), (case["name"], got)
        for k, want in case["counts"].items():
            assert getattr(v, k) == want == n[k], (case["name"], k)
        car.close(); traj.close(); m.close()


# 2. random scenes: 6 sweeps of 8 x 32 on a trajectory that rotates and translates within a sweep
@pytest.mark.parametrize("P", [1, 5, 20])
def test_random_scenes(P):
    m, car, sweeps, (kn, xyz) = _build_and_carve(8, 32, P, seed=P)
    v = car.votes()
    n = _check(m, v, sweeps, f"P = {P}")
    assert n["n_rays"] > 1000 and n["n_no_return"] > 50 and n["n_rays_out_of_range"] > 5 and n["sum_through"] > 0 and n["sum_support"] > 0
    # narrower parameters: min_range cuts the near points, a small margin and a coarse step
    car2 = _core().Carver(m, radius=0.1, margin=0.05, step=0.5, min_range=1.0, max_range=5.0)
    for k in range(6):
        car2.add_posed(kn.traj, kn.col_ts(k, 32), xyz=xyz[k], H=8)
    n2 = _check(m, car2.votes(), sweeps, f"P = {P}, narrow")
    assert n2["n_rays_out_of_range"] > n["n_rays_out_of_range"] and n2["sum_through"] > 0
    car.close(); car2.close(); m.close()


# ... and the workgroup and wavefront edges: H W = 1, 63, 65 and 257 pixels
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (5, 13), (1, 257)])
def test_pixel_counts_at_the_launch_edges(H, W):
    m, car, sweeps, _ = _build_and_carve(H, W, 5, n_sweeps=3, seed=H * W)
    n = _check(m, car.votes(), sweeps, f"{H} x {W}")
    assert n["n_rays"] + n["n_rays_out_of_range"] + n["n_no_return"] == 3 * H * W
    car.close(); m.close()


# 3. maps from hash_scenes: long probe chains, the cyclic wrap, tombstones
def _rays_at(points, rng, origin, H, W, through_frac=0.5):
    """H x W f32 sensor-frame ends (identity pose at `origin`): rays to some of `points`, half of them going on behind their point"""
    pick = points[rng.integers(0, len(points), H * W)] - origin
    pick = pick * np.where(rng.random((H * W, 1)) < through_frac, rng.uniform(1.2, 2.0, (H * W, 1)), 1.0)
    return pick.astype(np.float32).reshape(H, W, 3)


@pytest.mark.parametrize("scene", ["cluster", "wrap", "tombstones"])
def test_maps_with_long_chains_the_wrap_and_tombstones(scene):
    from tests.helpers import hash_scenes as hs
    core = _core()
    cap, H, W = 1 << 12, 8, 32
    rng = np.random.default_rng(7)
    if scene == "wrap":
        _, pts, _ = hs.wrap_scene(cap, 200)
    else:
        _, pts, _ = hs.cluster_scene(cap, 40, 200)
    # the sensor stands in the middle of the scene's voxels, a quarter into its own; the handle's max_range is the median distance of the points
    origin = np.trunc(np.median(pts, axis=0)) + 0.25
    far = np.linalg.norm(pts - origin, axis=1)
    reach = float(np.round(np.median(far)))
    m = core.Icp(reach, 0.0, voxel_size=1.0, scan_cols=W, max_points_per_scan=1 << 12, map_table_capacity=cap, map_block_capacity=1 << 12)
    m.map_add(pts)
    if scene == "tombstones":
        # the voxels farther than max_range from the origin leave the map and their slots stay as tombstones in the chains
        assert (far > reach + 2.0).sum() > 20 and (far < reach - 2.0).sum() > 20
        m.map_add(np.array([[0.25, 0.25, 0.25]]), origin=origin)
        assert m.map_size()[1] < len(pts)
    stored = m.map_points()
    pose = np.eye(4)
    pose[:3, 3] = origin
    traj = core.Traj([0.0, 1.0], [pose, pose], BOUNDS, BOUNDS)
    ts = np.arange(W) / (2.0 * W)
    car = core.Carver(m, radius=0.3, margin=0.5, step=0.5, max_range=250.0)
    sweeps = []
    for k in range(2):
        ends = _rays_at(pts if k else stored, rng, origin, H, W)  # (the second sweep also aims at the voxels that left the map)
        car.add_posed(traj, ts, xyz=ends, H=H)
        sweeps.append(cv.rays_of_sweep(ends.astype(np.float64), np.any(ends != 0.0, axis=2), np.tile(pose, (W, 1, 1))))
    n = _check(m, car.votes(), sweeps, scene)
    assert n["sum_through"] > 50 and n["sum_support"] > 50
    car.close(); traj.close(); m.close()


# ... and a map with small and full blocks: the map of a free-running batch with map_small_blocks (tests/test_gpu_map_compare.py's recipe)
def test_a_map_with_small_and_full_blocks():
    from ptudes_lab_amd import _lib as L
    from tests.helpers import full_voxel_scenes as fv
    core = _core()
    frames = fv.box_sweeps()
    P = fv.BOX_P_TWO_CLASSES
    kw = dict(max_range=fv.BOX_RANGE, min_range=fv.BOX_MIN, with_ekf=False, max_points_per_scan=fv.BOX_PTS, **fv.BOX_ICP)
    kw.update(max_points_per_voxel=P, map_small_blocks=1 << 12)
    r = core.BatchRunner(1, fv.BOX_N, fv.BOX_PTS, 0, team_workgroups=2, free_running=True, **kw)
    try:
        for k, f in enumerate(frames):
            r.upload_scan(0, k, f)
        r.upload_imu(0, np.zeros((0, 7)), [0] * fv.BOX_N)
        r.run()
        member = core.Icp.__new__(core.Icp)  # a view of the batch's own handle: the runner owns it
        member.cfg = core.icp_cfg(fv.BOX_RANGE, fv.BOX_MIN, **dict(fv.BOX_ICP, max_points_per_voxel=P))
        member._h = C.c_void_p()
        L.check(L.lib().ptl_batch_icp(r._h, 0, C.byref(member._h)))
        try:
            pts = member.map_points()
            _, counts = np.unique(np.trunc(pts / member.cfg.voxel_size).astype(np.int64), axis=0, return_counts=True)
            assert (counts <= 5).any() and (counts > 5).any(), "voxels of both block classes"
            W = int(member.cfg.scan_cols)
            H = fv.BOX_PTS // W
            traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
            ts = np.arange(W) / (2.0 * W)
            car = core.Carver(member, radius=0.2, margin=0.5, step=0.5, max_range=30.0)
            sweeps = []
            for k in (0, fv.BOX_N - 1):
                x = np.asarray(frames[k], dtype=np.float32).reshape(H, W, 3)[:, ::8] * np.float32(1.25 if k else 1.0)  # (the last one goes on behind the walls)
                full = np.zeros((H, W, 3), dtype=np.float32)
                full[:, :x.shape[1]] = x
                car.add_posed(traj, ts, xyz=full, H=H)
                sweeps.append(cv.rays_of_sweep(full.astype(np.float64), np.any(full != 0.0, axis=2), np.tile(np.eye(4), (W, 1, 1))))
            n = _check(member, car.votes(), sweeps, "two block classes")
            assert n["sum_through"] > 0 and n["sum_support"] > 0 and n["n_no_return"] > 0
            car.close(); traj.close()
        finally:
            member._h = None
    finally:
        r.close()


# 4. path agreement
def test_paths_agree():
    """range image + LUT = xyz of the LUT's points; add_run on a SeqRunner's and a BatchRunner's resident sweeps = per call; reverse order"""
    core = _core()
    H, W, N = 8, 32, 4
    rng = np.random.default_rng(11)
    kn = _Knots(N, seed=11)
    lut = core.Lut(H, W, np.linspace(20.0, -20.0, H), np.zeros(H), 0.0)
    rng_mm = [np.where(rng.random((H, W)) < 0.1, 0, rng.integers(300, 7000, (H, W))).astype(np.uint32) for _ in range(N)]
    m = _icp(W, H * W)
    for k in range(N):
        m.map_add_posed(kn.traj, kn.col_ts(k, W), range_mm=rng_mm[k], lut=lut)
    assert m.map_size()[1] > 200
    # (a) the range path against the restatement on the LUT's own points
    a = core.Carver(m)
    sweeps = []
    for k in range(N):
        a.add_posed(kn.traj, kn.col_ts(k, W), range_mm=rng_mm[k], lut=lut)
        sweeps.append(cv.rays_of_sweep(lut(rng_mm[k]).reshape(H, W, 3), rng_mm[k] != 0, kn.col_poses(kn.col_ts(k, W))))
    va = a.votes()
    _check(m, va, sweeps, "range path")
    rows_a = cv.sorted_rows(va.xyz, va.through, va.support)

    def same(v, what, rows=rows_a, ref=va):
        assert np.array_equal(cv.sorted_rows(v.xyz, v.through, v.support), rows), what
        assert all(getattr(v, k) == getattr(ref, k) for k in cv.COUNTS), what

    # (b) reverse order, and a second carver on the same map
    b = core.Carver(m)
    for k in reversed(range(N)):
        b.add_posed(kn.traj, kn.col_ts(k, W), range_mm=rng_mm[k], lut=lut)
    same(b.votes(), "reverse order")
    assert np.array_equal(b.votes().xyz, va.xyz) and np.array_equal(b.votes().through, va.through), "one pool order for one map"
    # (c) a batch's resident range images: sequence 1 of 2
    t0t1 = np.array([[k * kn.dt, (k + 1) * kn.dt] for k in range(N)])
    bt = core.BatchRunner(2, N, H * W, 0, max_range=100.0, min_range=0.0, with_ekf=False, range_input=True, scan_cols=W, **CAPS)
    bt.set_lut(lut)
    for s in range(2):
        for k in range(N):
            bt.upload_range(s, k, rng_mm[k] if s else rng_mm[0])
    c = core.Carver(m)
    assert c.add_run(bt, kn.traj, t0t1, s=1) == (va.n_rays, 0)
    same(c.votes(), "batch, resident range images")
    # (d) a SeqRunner's resident xyz sweeps against the per-call xyz path on a map of their own
    xyz = _random_sweeps(rng, N, H, W)
    m2 = _icp(W, H * W)
    sr = core.SeqRunner(N, H * W, 0, max_range=100.0, min_range=0.0, with_ekf=False, scan_cols=W, **CAPS)
    for k in range(N):
        sr.upload_scan(k, xyz[k])
    assert sr.build_map(m2, kn.traj, t0t1)[1] == 0
    d, e = core.Carver(m2), core.Carver(m2)
    n_rays, n_skipped = d.add_run(sr, kn.traj, t0t1)
    got = [e.add_posed(kn.traj, kn.col_ts(k, W), xyz=xyz[k], H=H) for k in range(N)]
    vd, ve = d.votes(), e.votes()
    assert (n_rays, n_skipped) == (sum(g[0] for g in got), 0) and vd.n_scans == N
    same(vd, "seq runner, resident xyz", cv.sorted_rows(ve.xyz, ve.through, ve.support), ve)
    # first / last, and a sweep outside the bounds is skipped as a whole and counted
    f = core.Carver(m2)
    late = t0t1.copy()
    late[2] += 100.0
    assert f.add_run(sr, kn.traj, late, first=1, last=3) == (got[1][0] + got[3][0], 1)
    vf = f.votes()
    assert (vf.n_scans, vf.n_scans_skipped, vf.n_rays) == (2, 1, got[1][0] + got[3][0])
    for x in (a, b, c, d, e, f, bt, sr, m, m2, lut):
        x.close()


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


def test_the_map_is_only_read():
    core = _core()
    H, W = 8, 32
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-6.0, 6.0, (H * W, 3))
    cloud /= np.maximum(np.abs(cloud).max(axis=1, keepdims=True) / 6.0, 1e-9)  # (on the faces of a cube: a scene a registration can hold on to)
    frame = (cloud + np.array([0.05, -0.02, 0.01])).astype(np.float32)
    poses = []
    for carve in (False, True):
        m = _icp(W, H * W, vs=1.0)
        m.map_add(cloud)
        # (map_points() hands the blocks out in the order its workgroups arrive: the rows are compared in lexicographic order)
        table, pts = _table_bytes(m), _lex(m.map_points()).tobytes()
        if carve:
            traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
            car = core.Carver(m)
            car.add_posed(traj, np.arange(W) / (2.0 * W), xyz=cloud.astype(np.float32).reshape(H, W, 3) * np.float32(1.1), H=H)
            v = car.votes()
            assert v.sum_through > 0
            assert _table_bytes(m) == table, "the table and the directory are byte-equal"
            assert _lex(m.map_points()).tobytes() == pts, "the points are byte-equal"
            car.close(); traj.close()
        poses.append(np.array([m.register_frame(frame), m.register_frame(frame)]))
        m.close()
    assert poses[0].tobytes() == poses[1].tobytes(), "a registration on the handle afterwards is bit-equal to one without the carve"


# 6. refusals, each before any HIP call and with the numbers
def _refused(code, fn, *words):
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn()
    if code == PTL_ERR_ARG:
        assert isinstance(e.value, ValueError), str(e.value)
    else:
        assert f"libptudes_mi error {code}:" in str(e.value), str(e.value)
    for w in words:
        assert str(w) in str(e.value), (w, str(e.value))
    return str(e.value)


def test_refusals():
    from ptudes_lab_amd import _lib as L
    core = _core()
    H, W = 4, 16
    m = _icp(W, H * W)
    m.map_add(np.array([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]))
    lib = L.lib()
    # cfg size or version
    for size, abi in ((40, L.ABI_VERSION), (48, L.ABI_VERSION + 1)):
        bad = core.carve_cfg(VS)
        bad.struct_size, bad.abi_version = size, abi
        h = C.c_void_p()
        assert lib.ptl_carve_create(m._h, C.byref(bad), C.byref(h)) == PTL_ERR_ARG and not h.value
        assert str(size) in lib.ptl_last_error().decode() and str(abi) in lib.ptl_last_error().decode()
    # each parameter bound
    for kw, words in ((dict(radius=0.0), ("radius", "0")), (dict(radius=-1.0), ("radius", "-1")), (dict(margin=-0.5), ("margin", "-0.5")),
                      (dict(step=0.0), ("step", "0")), (dict(step=0.75), ("step", "0.75", "0.5")), (dict(min_range=-1.0), ("min_range", "-1")),
                      (dict(min_range=3.0, max_range=3.0), ("max_range", "3")), (dict(step=0.25, max_range=16384.5), ("16384.5", "0.25", "65536")),
                      (dict(radius=float("nan")), ("radius",)), (dict(max_range=float("nan")), ("max_range",))):
        _refused(PTL_ERR_ARG, lambda: core.Carver(m, **kw), *words)
    core.Carver(m, step=0.25, max_range=16384.0).close()  # (exactly 65536 samples is allowed)
    # null pointers
    h = C.c_void_p()
    assert lib.ptl_carve_create(None, None, C.byref(h)) == PTL_ERR_ARG and lib.ptl_carve_create(m._h, None, None) == PTL_ERR_ARG
    car = core.Carver(m)
    traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
    ts = np.arange(W) / (2.0 * W)
    x = np.zeros((H, W, 3), dtype=np.float32)
    x[0, 0] = [3.0, 0.0, 0.0]  # one ray along +x through both points
    fp, dp = x.ctypes.data_as(C.POINTER(C.c_float)), L.dptr(ts)
    assert lib.ptl_carve_add_posed_xyz(None, traj._h, fp, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_posed_xyz(car._h, None, fp, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_posed_xyz(car._h, traj._h, None, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_posed_xyz(car._h, traj._h, fp, H, W, None, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_posed_range(car._h, traj._h, None, None, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_seq(car._h, None, traj._h, dp, 0, 0, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_add_batch(car._h, None, 0, traj._h, dp, 0, 0, None, None) == PTL_ERR_ARG
    assert lib.ptl_carve_read(car._h, None, None, None, None, 0, None) == PTL_ERR_ARG
    res = L.CarveResult()
    out = np.empty((2, 3))
    assert lib.ptl_carve_read(car._h, C.byref(res), L.dptr(out), None, None, 2, None) == PTL_ERR_ARG  # (the three arrays: all or none)
    assert "1 given" in lib.ptl_last_error().decode()
    # W or H W not the map handle's
    _refused(PTL_ERR_CAPACITY, lambda: car.add_posed(traj, np.arange(8) / 16.0, xyz=x[:, :8], H=H), "8 columns", W)
    _refused(PTL_ERR_CAPACITY, lambda: car.add_posed(traj, ts, xyz=np.zeros((H + 1, W, 3), dtype=np.float32), H=H + 1), (H + 1) * W, H * W)
    # different devices: with one device the rule is tested through the handle's device_id (its first member, an int)
    dev = C.c_int.from_address(traj._h.value)
    dev.value = 1
    _refused(PTL_ERR_ARG, lambda: car.add_posed(traj, ts, xyz=x, H=H), "device 1", "device 0")
    dev.value = 0
    # max_points too small
    t_, s_ = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.ptl_carve_read(car._h, C.byref(res), L.dptr(out), t_.ctypes.data_as(u32p), s_.ctypes.data_as(u32p), 1, None) == PTL_ERR_CAPACITY
    assert "2 points" in lib.ptl_last_error().decode() and "max_points = 1" in lib.ptl_last_error().decode()
    # the handle still works after all that; then a map_add between create and add: PTL_ERR_STATE, at the add and at the read
    assert car.add_posed(traj, ts, xyz=x, H=H) == (1, False)
    v = car.votes()
    assert (v.n_points, v.sum_through, v.n_rays, v.n_no_return) == (2, 2, 1, H * W - 1)
    m.map_add(np.array([[5.0, 5.0, 5.0]]))
    _refused(PTL_ERR_STATE, lambda: car.add_posed(traj, ts, xyz=x, H=H), "3 points", "2 at")
    _refused(PTL_ERR_STATE, lambda: car.votes(), "3 points")
    car2 = core.Carver(m)  # a new handle sees the new map
    assert car2.add_posed(traj, ts, xyz=x, H=H) == (1, False) and car2.votes().n_points == 3
    for x_ in (car, car2, traj, m):
        x_.close()


# 7. the moving-box scene: equality with the restatement (which meets the conditions: tests/test_map_carve_cpu.py), and carved()
def test_the_moving_box_scene():
    from ptudes_lab_amd import fly
    core = _core()
    scene = cv.moving_box_scene()
    H, W = scene[0][0].shape[:2]
    lut = core.Lut(H, W, np.zeros(H), np.zeros(H), 0.0)  # (MapAccumulator sizes its handle from a LUT; the sweeps go in as xyz)
    acc = fly.MapAccumulator(lut, voxel_size=cv.BOX_VS, max_points_per_voxel=cv.BOX_P, map_block_capacity=1 << 16, map_table_capacity=1 << 18)
    knots_t = np.arange(2 * len(scene)) * 0.5
    knots_p = np.repeat(np.array([pose for _, pose, _ in scene]), 2, axis=0)
    traj = core.Traj(knots_t, knots_p, 0.0, 0.0)
    col_ts = [k + 0.25 * np.arange(W) / W for k in range(len(scene))]  # sweep k lies between its own two knots
    for k, (xyz, _, _) in enumerate(scene):
        assert acc.icp.map_add_posed(traj, col_ts[k], xyz=xyz, H=H)[1] is False
    car = fly.MapCarver(acc, **{k: v for k, v in cv.BOX_CFG.items()})
    poses = []
    for k, (xyz, _, _) in enumerate(scene):
        car.carver.add_posed(traj, col_ts[k], xyz=xyz, H=H)
        poses.append(core.traj_poses_at(knots_t, knots_p, col_ts[k])[0])
    v = car.votes()
    sweeps, box = cv.moving_box_rays(scene, poses)
    _check(acc.icp, v, sweeps, "moving box")
    dyn = v.dynamic(2, 0.5)
    is_box = cv.on_box_mask(v.xyz, box)
    print(f"moving box on the device: {int((dyn & is_box).sum())} of {int(is_box.sum())} box points flagged, "
          f"{int((dyn & ~is_box).sum())} of {int((~is_box).sum())} static points")
    assert (dyn & ~is_box).sum() == 0 and (dyn & is_box).sum() >= 0.9 * is_box.sum() and is_box.sum() > 300
    clean = acc.carved(dyn, v.xyz)
    kept = clean.map_points()
    assert np.array_equal(cv.sorted_rows(kept, np.zeros(len(kept)), np.zeros(len(kept)))[:, :3],
                          cv.sorted_rows(v.xyz[~dyn], np.zeros((~dyn).sum()), np.zeros((~dyn).sum()))[:, :3]), "carved() holds exactly the kept points"
    assert clean.icp.cfg.voxel_size == cv.BOX_VS and clean.icp.cfg.max_points_per_voxel == cv.BOX_P
    for x in (car, clean, acc, traj, lut):
        x.close()


# 8. the command
def test_flyby_carves_and_writes_both_maps(tmp_path):
    import re
    from click.testing import CliRunner
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    p, m1, m2 = str(tmp_path / "p.csv"), str(tmp_path / "clean.ply"), str(tmp_path / "carved.ply")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "3", "--use-imu-prediction",
                                          "--save-nc-gt-poses", p])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "3", "--save-map", m1, "--carve",
                                          "--save-carved", m2, "--carve-min-through", "2", "--carve-min-fraction", "0.5"])
    assert res.exit_code == 0, res.output
    pts, sc = pu.load_map_ply(m2, scalars=True)
    assert set(sc) >= {"through", "support", "dynamic"}
    thr, sup, dyn = (np.asarray(sc[k]) for k in ("through", "support", "dynamic"))
    out = res.output
    g = re.search(r"points: (\d+) \(passed through (\d+), supported (\d+)\), votes through (\d+), support (\d+)", out)
    assert g, out
    assert [int(x) for x in g.groups()] == [len(pts), int((thr > 0).sum()), int((sup > 0).sum()), int(thr.sum()), int(sup.sum())]
    n_dyn = int(re.search(r"dynamic \(through >= 2, fraction >= 0.5\): (\d+) points", out).group(1))
    from ptudes_lab_amd import core
    assert n_dyn == int(dyn.sum()) == int(core.carve_dynamic(thr.astype(np.int64), sup.astype(np.int64)).sum())
    assert re.search(r"sweeps: 4 \(skipped 0\)", out), out
    clean = pu.load_map_ply(m1)
    keep = pts[dyn == 0]
    assert np.array_equal(clean[np.lexsort(clean.T[::-1])], keep[np.lexsort(keep.T[::-1])]), "the cleaned PLY is the unflagged rows of the carved PLY"


def test_ekf_bench_carves_the_map_of_its_run(tmp_path):
    import re
    from click.testing import CliRunner
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    m1, m2 = str(tmp_path / "clean.ply"), str(tmp_path / "carved.ply")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "3", "--use-imu-prediction", "--save-map", m1,
                                          "--map-score", "--carve", "--save-carved", m2, "--carve-radius", "0.1"])
    assert res.exit_code == 0, res.output
    out = res.output
    assert "carve: radius 0.1 m" in out and "before carving:" in out and "after carving:" in out and out.count("map score:") == 2
    pts, sc = pu.load_map_ply(m2, scalars=True)
    g = re.search(r"points: (\d+) \(passed through (\d+), supported (\d+)\), votes through (\d+), support (\d+)", out)
    assert [int(x) for x in g.groups()] == [len(pts), int((sc["through"] > 0).sum()), int((sc["support"] > 0).sum()),
                                            int(sc["through"].astype(np.int64).sum()), int(sc["support"].astype(np.int64).sum())]
    assert re.search(r"sweeps: 4 \(skipped 0\)", out), out
    clean, _ = pu.load_map_ply(m1, scalars=True)  # (with --map-score the cleaned map's PLY carries the score's scalars)
    keep = pts[sc["dynamic"] == 0]
    assert np.array_equal(clean[np.lexsort(clean.T[::-1])], keep[np.lexsort(keep.T[::-1])])
