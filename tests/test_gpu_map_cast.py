"""Rays cast through a map on the device (csrc/cast_kernels.h) against the numpy restatement (tests/helpers/map_cast_numpy.py).
Every output is an exact function of the stored points and the ray, so everything is compared for equality: `status`, `t_hit` and `len` with
array_equal (NaN equal to NaN: the len of a degenerate return), `index` as the row of `Caster.points()` it names - the restatement is handed
the stored points in that order - and every count of the summary.  There is no tolerance in this file.  The restatement takes the stored
points and the column poses from the device: which points a voxel keeps and where a column's pose lies are tested elsewhere; what is tested
here is the march and the choice of the hit.

Per-call `core.Icp` maps with small capacities; lattice maps of dyadic points with axis-aligned and quarter-turn poses, so that the posed
points are exact."""
import ctypes as C
import re
import struct
import zlib

import numpy as np
import pytest

from tests.helpers import map_cast_cases as cc
from tests.helpers import map_cast_numpy as mc

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


def _cfg_of(sw):
    return {k: sw.result[k] for k in ("radius", "step", "min_range", "max_range")}


def _check(cas, sw, rays, what="", stored=None):
    """a core.CastSweep against the restatement on the caster's stored points in pool order: every pixel's four outputs, every count"""
    stored = cas.points() if stored is None else stored
    vs = float(cas.map_icp.cfg.voxel_size)
    H, W = sw.status.shape
    st, th, ln, ix, n = mc.cast(stored, rays, vs, _cfg_of(sw), n_pixels=H * W)
    assert sw.status.dtype == np.uint8 and sw.index.dtype == np.int32 and sw.t_hit.dtype == np.float64 and sw.len.dtype == np.float64
    for name, got, want in (("status", sw.status, st), ("t_hit", sw.t_hit, th), ("len", sw.len, ln), ("index", sw.index, ix)):
        got = got.reshape(-1)
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
        assert len(bad) == 0, (what, name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    for k in mc.COUNTS:
        assert int(sw.result[k]) == n[k], (what, k, sw.result[k], n[k])
    return n


QUARTER_TURNS = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]),
                 np.array([[-1.0, 0, 0], [0, -1, 0], [0, 0, 1]]), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])]
DIRS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [0, 1, -1], [1, 0, 1], [1, 1, 1], [-1, 1, -1], [2, 1, 0], [3, -2, 1], [-1, 0, 0], [1, -1, 0]],
                dtype=np.float64)


def _lattice(rng, n_points, half=12):
    """points on the lattice of eighths in a cube of 2 half / 8 metres around the origin, voxel 0's double-width span inside it"""
    return rng.integers(-half, half, (n_points, 3)) / 8.0


def _lattice_sweep(rng, H, W, reach=32):
    """H x W f32 ends in the sensor frame: multiples of 1 / 8 along axes, face and space diagonals and a few general lattice directions; some
    random lattice ends; no-returns; NaN, inf; short rays that end before the first point and long ones that end behind the last"""
    n = H * W
    d = DIRS[rng.integers(0, len(DIRS), n)] * rng.integers(1, reach, (n, 1)) / 8.0
    some = rng.random(n) < 0.4
    d[some] = rng.integers(-reach, reach, (int(some.sum()), 3)) / 8.0
    d[rng.random(n) < 0.1] = 0.0
    x = d.astype(np.float32).reshape(H, W, 3)
    if n > 8:
        x.reshape(-1, 3)[3] = [np.nan, 0.0, 1.0]
        x.reshape(-1, 3)[5] = [0.0, np.inf, 0.0]
        x.reshape(-1, 3)[7] = [0.0, 0.0, 0.0]
    return x


def _still(pose, W):
    """a trajectory that holds one pose, the column times and the column poses as the device evaluates them (bit-equal to the pose)"""
    core = _core()
    traj = core.Traj([0.0, 1.0], [pose, pose], BOUNDS, BOUNDS)
    ts = 0.25 + np.arange(W) / (4.0 * W)
    poses, n_out = core.traj_poses_at([0.0, 1.0], [pose, pose], ts, BOUNDS, BOUNDS)
    assert n_out == 0 and (poses == pose[None]).all(), "the geodesic between equal poses is that pose, bit for bit"
    return traj, ts, poses


def _rays(xyz, poses):
    x = np.asarray(xyz, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return mc.rays_of_sweep(x.astype(np.float64), np.any(x != 0.0, axis=2), poses)


def _pose(turn, t):
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = QUARTER_TURNS[turn % len(QUARTER_TURNS)], t
    return pose


# 1. the answers computed by hand: every clause of the definition
def test_hand_cases():
    core = _core()
    for case in cc.hand_cases():
        m = _icp(cc.W, 64, P=20)
        if len(case["stored"]):
            m.map_add(case["stored"])
        assert m.map_size()[1] == len(case["stored"]), case["name"]
        pose = np.eye(4)
        pose[:3, 3] = case["origin"]
        traj, ts, poses = _still(pose, cc.W)
        cas = core.Caster(m, **case["cfg"])
        sw = cas.cast_xyz(traj, case["xyz"], 1, cc.W, ts)
        n = _check(cas, sw, cc.case_rays(case, poses), case["name"])
        pts = cas.points()
        assert np.array_equal(_lex(pts), _lex(case["stored"])), case["name"]
        classes = sw.changes(cc.CHANGE_MARGIN)
        for i, (want_st, want_row, want_t, want_class) in enumerate(case["expect"]):
            what = (case["name"], i)
            assert sw.status[0, i] == want_st and classes[0, i] == want_class, (what, sw.status[0, i], classes[0, i])
            if want_row >= 0:
                assert np.array_equal(pts[sw.index[0, i]], case["stored"][want_row]), (what, pts[sw.index[0, i]])
            else:
                assert sw.index[0, i] == -1 and sw.t_hit[0, i] == -1.0, what
            if want_t is not None:
                assert sw.t_hit[0, i] == want_t, (what, sw.t_hit[0, i])
        for k, want in case["counts"].items():
            assert sw.result[k] == want == n[k], (case["name"], k, sw.result[k])
        assert sw.result["skipped"] is False and sw.result["n_pixels"] == cc.W
        cas.close(); traj.close(); m.close()


# 2. lattice maps, quarter-turn poses, 1 .. 20 points per voxel, and the workgroup and wavefront edges of the pixel count
@pytest.mark.parametrize("H,W,P", [(1, 1, 1), (1, 31, 2), (2, 16, 3), (3, 11, 20), (7, 9, 5), (1, 64, 8), (5, 13, 13), (5, 51, 20), (4, 64, 6), (1, 257, 20)])
def test_lattice_maps_and_pixel_counts(H, W, P):
    core = _core()
    rng = np.random.default_rng(H * W + P)
    m = _icp(W, 1 << 12, P=P)
    m.map_add(_lattice(rng, 3000))
    stored = m.map_points()
    _, per_voxel = np.unique(np.trunc(stored / VS).astype(np.int64), axis=0, return_counts=True)
    assert per_voxel.max() == P and (P == 1 or per_voxel.min() < P), "voxels that are full and voxels that are not"
    hits = 0
    for turn, cfg in ((H + W, dict(radius=0.125, step=0.25, max_range=6.0)), (H * W + 1, dict(radius=0.25, step=0.5, min_range=0.5, max_range=3.0)), (P, {})):
        pose = _pose(turn, [0.125, -0.375, 0.25])
        traj, ts, poses = _still(pose, W)
        cas = core.Caster(m, **cfg)
        for _ in range(2 if H * W < 64 else 1):
            xyz = _lattice_sweep(rng, H, W)
            n = _check(cas, cas.cast_xyz(traj, xyz, H, W, ts), _rays(xyz, poses), f"{H} x {W}, P = {P}, turn {turn}, {cfg}")
            assert n["n_no_return"] + n["n_degenerate"] + n["n_hit"] + n["n_miss"] == H * W
            hits += n["n_hit"]
        cas.close(); traj.close()
    assert hits > 0
    m.close()


# ... and a map with small and full blocks: the map of a free-running batch with map_small_blocks (tests/test_gpu_map_carve.py's recipe)
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
            traj, ts, poses = _still(np.eye(4), W)
            cas = core.Caster(member, radius=0.2, step=0.5, max_range=30.0)
            full = np.zeros((H, W, 3), dtype=np.float32)
            x = np.asarray(frames[0], dtype=np.float32).reshape(H, W, 3)[:, ::8]
            full[:, :x.shape[1]] = x
            n = _check(cas, cas.cast_xyz(traj, full, H, W, ts), _rays(full, poses), "two block classes")
            assert n["n_hit"] > 100 and n["n_no_return"] > 0
            cas.close(); traj.close()
        finally:
            member._h = None
    finally:
        r.close()


# 3. a trajectory that moves within the sweep, a range image with its LUT, the virtual sweep, a sweep outside the bounds
def test_range_form_expected_and_a_skipped_sweep():
    """The range form is held to the restatement on the LUT's own fp64 points, `lut(range_mm)`, for equality.  It is NOT held to the xyz form of
    those points: `cast_xyz` takes f32 points, so its rays' ends are the fp64 ends rounded to f32, and `len`, `t_hit` and a point at the edge of
    the radius cannot be bit-equal between the two forms.  The restatement on the fp64 ends asks more: every output of the range form, exactly."""
    core = _core()
    from ptudes_lab_amd.utils import exp_pose6
    H, W = 8, 32
    rng = np.random.default_rng(11)
    kts = np.arange(-1, 6) * 0.05
    twist = np.concatenate([rng.uniform(-0.6, 0.6, 3), rng.uniform(-2.0, 2.0, 3)])
    kps = np.array([exp_pose6(twist * t) for t in kts])
    traj = core.Traj(kts, kps, BOUNDS, BOUNDS)
    ts = (np.arange(W) / W) * 0.1
    poses, n_out = core.traj_poses_at(kts, kps, ts, BOUNDS, BOUNDS)
    assert n_out == 0
    lut = core.Lut(H, W, np.linspace(20.0, -20.0, H), np.zeros(H), 0.0)
    m = _icp(W, 1 << 12)
    for k in range(3):
        r = np.where(rng.random((H, W)) < 0.1, 0, rng.integers(300, 5000, (H, W))).astype(np.uint32)
        m.map_add_posed(traj, ts, range_mm=r, lut=lut)
    m.map_add(rng.uniform(-4.0, 4.0, (4000, 3)))
    assert m.map_size()[1] > 3000
    cas = core.Caster(m, radius=0.2, max_range=12.0)
    rng_mm = np.where(rng.random((H, W)) < 0.1, 0, rng.integers(300, 7000, (H, W))).astype(np.uint32)
    # (a) the range form against the restatement on the LUT's own points
    a = cas.cast_range(traj, lut, rng_mm, ts)
    n = _check(cas, a, mc.rays_of_sweep(lut(rng_mm).reshape(H, W, 3), rng_mm != 0, poses), "range form")
    assert n["n_hit"] > 50 and n["n_no_return"] > 5
    # (b) two calls are bit-equal, and nothing is kept between calls
    b = cas.cast_range(traj, lut, rng_mm, ts)
    for f in ("status", "t_hit", "len", "index"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert {k: v for k, v in a.result.items() if k != "device_ms"} == {k: v for k, v in b.result.items() if k != "device_ms"}
    # (c) the virtual sweep is the cast of the constant image: every pixel is cast, the LUT's pixel (0, 0) included
    e = cas.expected(traj, lut, ts)
    const = np.full((H, W), 12000, dtype=np.uint32)
    c = cas.cast_range(traj, lut, const, ts)
    for f in ("status", "t_hit", "len", "index"):
        assert getattr(e, f).tobytes() == getattr(c, f).tobytes(), f
    _check(cas, e, mc.rays_of_sweep(lut(const).reshape(H, W, 3), const != 0, poses), "expected()")
    assert e.result["n_no_return"] == 0 and e.result["n_hit"] + e.result["n_miss"] == H * W
    mm = e.expected_range_mm()
    assert mm.dtype == np.uint32 and ((mm > 0) == (e.status == 1)).all() and np.array_equal(mm[e.status == 1], np.rint(e.t_hit[e.status == 1] * 1000.0))
    e2 = cas.expected(traj, lut, ts, ref_range=3000)  # (another reference range: the same directions up to the LUT's rounding)
    assert e2.result["n_hit"] + e2.result["n_miss"] == H * W
    # gather: the z of the hit points as a predicted field image
    z = e.gather(cas.points()[:, 2], fill=np.nan)
    assert np.array_equal(z[e.status == 1], cas.points()[e.index[e.status == 1], 2]) and np.isnan(z[e.status != 1]).all()
    # (d) a sweep with a column outside the trajectory's bounds is skipped as a whole and says so in every pixel
    late = ts.copy()
    late[W // 2] += 100.0
    s = cas.cast_range(traj, lut, rng_mm, late)
    _check(cas, s, None, "skipped")
    assert s.result["skipped"] is True and (s.status == 0).all() and (s.t_hit == -1.0).all() and (s.len == -1.0).all() and (s.index == -1).all()
    assert s.result["n_hit"] == 0 and s.result["n_pixels"] == H * W
    _check(cas, cas.cast_range(traj, lut, rng_mm, ts), mc.rays_of_sweep(lut(rng_mm).reshape(H, W, 3), rng_mm != 0, poses), "after the skipped one")
    # (e) the column times default to the first knot's: a pose held still
    d = cas.cast_range(traj, lut, rng_mm)
    p0, _ = core.traj_poses_at(kts, kps, np.full(W, kts[0]), BOUNDS, BOUNDS)
    _check(cas, d, mc.rays_of_sweep(lut(rng_mm).reshape(H, W, 3), rng_mm != 0, p0), "default column times")
    for x in (cas, traj, lut, m):
        x.close()


# 4. read-only and independent of the order the stored set went in
def _table_bytes(icp):
    from ptudes_lab_amd import _lib as L
    info = (C.c_int64 * 8)()
    L.check(L.lib().ptl_icp_debug_table(icp._h, None, 0, None, None, 0, info))
    slots, blocks = info[3] + 1, info[6]
    ent, bhdr, bfirst = np.empty(slots * 16, dtype=np.uint8), np.empty((blocks, 4), dtype=np.int32), np.empty((blocks, 3))
    L.check(L.lib().ptl_icp_debug_table(icp._h, ent.ctypes.data_as(C.c_void_p), slots, bhdr.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(bfirst),
                                        blocks, info))
    return ent.tobytes() + bhdr.tobytes() + bfirst.tobytes() + bytes(info)


def test_the_map_is_only_read_and_the_insertion_order_does_not_matter():
    core = _core()
    H, W = 4, 32
    rng = np.random.default_rng(5)
    cloud = np.unique(_lattice(rng, 1500), axis=0)  # (distinct points, fewer than P per voxel: the stored SET is the same in either order)
    key, per = np.unique(np.trunc(cloud / VS).astype(np.int64), axis=0, return_counts=True)
    pose = _pose(1, [0.125, -0.375, 0.25])
    traj, ts, poses = _still(pose, W)
    xyz = _lattice_sweep(rng, H, W)
    got = []
    for order in (cloud, cloud[::-1]):
        m = _icp(W, 1 << 12, P=32)
        assert per.max() <= 32
        m.map_add(order)
        table, pts = _table_bytes(m), _lex(m.map_points()).tobytes()
        cas = core.Caster(m, radius=0.25)
        sw = cas.cast_xyz(traj, xyz, H, W, ts)
        p = cas.points()
        _check(cas, sw, _rays(xyz, poses), "order")
        assert _table_bytes(m) == table, "the table and the directory are byte-equal"
        assert _lex(m.map_points()).tobytes() == pts and _lex(p).tobytes() == pts, "the points are byte-equal"
        hit = sw.status == 1
        got.append((sw.status.copy(), sw.t_hit.copy(), sw.len.copy(), p[sw.index[hit]], sw.result))
        cas.close(); m.close()
    a, b = got
    assert a[0].sum() > 20
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2], equal_nan=True) and np.array_equal(a[3], b[3])
    assert all(a[4][k] == b[4][k] for k in mc.COUNTS)
    traj.close()


# 5. a second witness from existing device code: the carve votes for what the cast hits
def test_every_hit_has_a_carve_vote():
    core = _core()
    rng = np.random.default_rng(3)
    m = _icp(1, 1 << 12, P=20)
    m.map_add(_lattice(rng, 3000))
    pose = _pose(2, [0.125, -0.375, 0.25])
    traj, ts, poses = _still(pose, 1)
    cfg = dict(radius=0.125, step=0.25, min_range=0.0, max_range=16.0)
    cas = core.Caster(m, **cfg)
    rays = []
    for i in range(24):  # every end lies outside the cube of stored points, so len > t_hit and the carve's march reaches the hit's voxel
        d = DIRS[i % len(DIRS)]
        x = (d * (24.0 / np.abs(d).max()) / 8.0).astype(np.float32).reshape(1, 1, 3)
        sw = cas.cast_xyz(traj, x, 1, 1, ts)
        _check(cas, sw, _rays(x, poses), f"ray {i}")
        if sw.status[0, 0] == 1:
            assert sw.len[0, 0] > sw.t_hit[0, 0]
            rays.append((x, int(sw.index[0, 0]), float(sw.len[0, 0] - sw.t_hit[0, 0])))
    assert len(rays) >= 12
    car = core.Carver(m, margin=max(r[2] for r in rays), **cfg)
    before = np.zeros(m.map_size()[1], dtype=np.int64)
    for x, index, _ in rays:
        assert car.add_posed(traj, ts, xyz=x, H=1) == (1, False)
        v = car.votes()
        now = v.through.astype(np.int64) + v.support
        assert now[index] > before[index], "the carve votes for the point the cast hit"
        assert np.array_equal(v.xyz, cas.points()), "one pool order"
        before = now
    for x_ in (car, cas, traj, m):
        x_.close()


# 6. refusals, each before any HIP call and with the numbers; PTL_ERR_STATE after a map_add
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
    for size, abi in ((32, L.ABI_VERSION), (40, L.ABI_VERSION + 1)):
        bad = core.cast_cfg(VS)
        bad.struct_size, bad.abi_version = size, abi
        h = C.c_void_p()
        assert lib.ptl_cast_create(m._h, C.byref(bad), C.byref(h)) == PTL_ERR_ARG and not h.value
        assert str(size) in lib.ptl_last_error().decode() and str(abi) in lib.ptl_last_error().decode()
    for kw, words in ((dict(radius=0.0), ("radius", "0")), (dict(radius=-1.0), ("radius", "-1")), (dict(step=0.0), ("step", "0")),
                      (dict(step=0.75), ("step", "0.75", "0.5")), (dict(min_range=-1.0), ("min_range", "-1")),
                      (dict(min_range=3.0, max_range=3.0), ("max_range", "3")), (dict(step=0.25, max_range=16384.5), ("16384.5", "0.25", "65536")),
                      (dict(radius=float("nan")), ("radius",)), (dict(max_range=float("nan")), ("max_range",))):
        _refused(PTL_ERR_ARG, lambda: core.Caster(m, **kw), *words)
    core.Caster(m, step=0.25, max_range=16384.0).close()  # (exactly 65536 samples is allowed)
    h = C.c_void_p()
    assert lib.ptl_cast_create(None, None, C.byref(h)) == PTL_ERR_ARG and lib.ptl_cast_create(m._h, None, None) == PTL_ERR_ARG
    cas = core.Caster(m)  # (cfg: the defaults)
    assert (cas.cfg.radius, cas.cfg.step, cas.cfg.min_range, cas.cfg.max_range) == (VS / 5.0, VS / 2.0, 0.0, 120.0 * VS)
    traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
    ts = np.arange(W) / (2.0 * W)
    x = np.zeros((H, W, 3), dtype=np.float32)
    x[0, 0] = [3.0, 0.0, 0.0]  # one ray along +x through both points
    fp, dp = x.ctypes.data_as(C.POINTER(C.c_float)), L.dptr(ts)
    nul = (None,) * 5
    assert lib.ptl_cast_posed_xyz(None, traj._h, fp, H, W, dp, *nul) == PTL_ERR_ARG
    assert lib.ptl_cast_posed_xyz(cas._h, None, fp, H, W, dp, *nul) == PTL_ERR_ARG
    assert lib.ptl_cast_posed_xyz(cas._h, traj._h, None, H, W, dp, *nul) == PTL_ERR_ARG
    assert lib.ptl_cast_posed_xyz(cas._h, traj._h, fp, H, W, None, *nul) == PTL_ERR_ARG
    assert lib.ptl_cast_posed_range(cas._h, traj._h, None, None, dp, *nul) == PTL_ERR_ARG
    assert lib.ptl_cast_points(cas._h, None, 2, None) == PTL_ERR_ARG
    # every output array may be null: the call still runs and counts
    res = L.CastResult()
    assert lib.ptl_cast_posed_xyz(cas._h, traj._h, fp, H, W, dp, C.byref(res), None, None, None, None) == 0
    assert (res.n_pixels, res.n_hit, res.n_no_return, res.skipped) == (H * W, 1, H * W - 1, 0)
    assert lib.ptl_cast_posed_xyz(cas._h, traj._h, fp, H, W, dp, *nul) == 0
    # W or H W not the map handle's
    _refused(PTL_ERR_CAPACITY, lambda: cas.cast_xyz(traj, x[:, :8], H, 8, np.arange(8) / 16.0), "8 columns", W)
    _refused(PTL_ERR_CAPACITY, lambda: cas.cast_xyz(traj, np.zeros((H + 1, W, 3), dtype=np.float32), H + 1, W, ts), (H + 1) * W, H * W)
    _refused(PTL_ERR_ARG, lambda: cas.cast_xyz(traj, np.zeros((0, W, 3), dtype=np.float32), 0, W, ts), "empty scan")
    # different devices: with one device the rule is tested through the handle's device_id (its first member, an int)
    dev = C.c_int.from_address(traj._h.value)
    dev.value = 1
    _refused(PTL_ERR_ARG, lambda: cas.cast_xyz(traj, x, H, W, ts), "device 1", "device 0")
    dev.value = 0
    # max_points too small
    out = np.empty((2, 3))
    assert lib.ptl_cast_points(cas._h, L.dptr(out), 1, None) == PTL_ERR_CAPACITY
    assert "2 points" in lib.ptl_last_error().decode() and "max_points = 1" in lib.ptl_last_error().decode()
    assert lib.ptl_cast_points(cas._h, L.dptr(out), -1, None) == PTL_ERR_ARG
    # the handle still works after all that; then a map_add between create and the next call: PTL_ERR_STATE, at the cast and at points()
    sw = cas.cast_xyz(traj, x, H, W, ts)
    assert (sw.result["n_hit"], sw.status[0, 0], sw.t_hit[0, 0], sw.len[0, 0]) == (1, 1, 1.0, 3.0)
    assert np.array_equal(cas.points()[sw.index[0, 0]], [1.0, 0.0, 0.0])
    m.map_add(np.array([[5.0, 5.0, 5.0]]))
    _refused(PTL_ERR_STATE, lambda: cas.cast_xyz(traj, x, H, W, ts), "3 points", "2 at")
    _refused(PTL_ERR_STATE, lambda: cas.points(), "3 points")
    cas2 = core.Caster(m)  # a new handle sees the new map
    assert cas2.cast_xyz(traj, x, H, W, ts).result["n_hit"] == 1 and len(cas2.points()) == 3
    for x_ in (cas, cas2, traj, m):
        x_.close()


# 7. the end-to-end scene equal to the restatement (which meets the issue's shares: tests/test_map_cast_cpu.py), through fly.SweepDiffer
def test_the_scene_with_a_box_the_map_has_never_seen():
    from ptudes_lab_amd import fly
    core = _core()
    seq = mc.scene_sequence()
    boxed = mc.scene_with_box(seq)
    H, W = seq.H, seq.W
    kts = np.arange(0, 24 * 4 + 1) * (seq.scan_dt / 4.0)
    kps = seq.pose_at(kts)
    traj = core.Traj(kts, kps, 0.0, 0.0)
    m = _icp(W, H * W, vs=mc.SCENE_VS, P=mc.SCENE_P, map_block_capacity=1 << 16, map_table_capacity=1 << 18)
    for k in mc.SCENE_MAP_SWEEPS:
        assert m.map_add_posed(traj, mc.scene_col_ts(seq, k), xyz=seq.scan(k).reshape(H, W, 3), H=H)[1] is False
    differ = fly.SweepDiffer(m, margin=mc.SCENE_MARGIN, **mc.SCENE_CFG)
    ts = mc.scene_col_ts(seq, mc.SCENE_SWEEP)
    poses, n_out = core.traj_poses_at(kts, kps, ts)
    assert n_out == 0
    stored = differ.caster.points()
    res = []
    for s in (seq, boxed):
        xyz = s.scan(mc.SCENE_SWEEP).reshape(H, W, 3)
        classes, counts = differ.update_xyz(xyz, H, W, traj, ts)
        sw = differ.last
        _check(differ.caster, sw, _rays(xyz, poses), "scene", stored=stored)
        assert np.array_equal(classes, mc.changes(sw.status, sw.t_hit, sw.len, mc.SCENE_MARGIN)) and sum(counts.values()) == H * W
        assert counts == {name: int((classes == i).sum()) for i, name in enumerate(core.CHANGE_NAMES)}
        assert fly.SweepDiffer.image(classes).shape == (H, W, 4)
        res.append((sw.status.reshape(-1), sw.t_hit.reshape(-1), sw.len.reshape(-1)))
    hit, agree, new_box, new_other, n_box = mc.scene_figures(res[0], res[1])
    print(f"scene on the device ({len(stored)} stored points): hit {hit:.4%} of the cast rays, agree {agree:.4%} of the hits, "
          f"new {new_box:.4%} of the box's {n_box} pixels, new {new_other:.4%} of the other pixels")
    for x in (differ, traj, m):
        x.close()


# 8. the command, on a map and poses that an ekf-bench run saved
def test_localize_reports_changes(tmp_path):
    from click.testing import CliRunner
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    ply, kf, out = (str(tmp_path / n) for n in ("map.ply", "kf.csv", "changes"))
    size = ["--synthetic", "1000", "--synthetic-size", "32x256", "--end-scan", "3"]
    res = run(ptudes_cli, ["ekf-bench", "ouster"] + size + ["--use-imu-prediction", "--save-map", ply, "--save-nc-gt-poses", kf])
    assert res.exit_code == 0, res.output
    res = run(ptudes_cli, ["localize"] + size + ["--map", ply, "--keyframes", kf, "--changes", "--cast-radius", "0.2", "--change-margin", "0.75",
                                                 "--cast-max-range", "40", "--save-changes", out])
    assert res.exit_code == 0, res.output
    assert "changes: radius 0.2 m" in res.output and "range [0, 40] m, margin 0.75 m" in res.output, res.output
    rows = re.findall(r"changes (\d{6}): none (\d+), agree (\d+), new (\d+), gone (\d+), unmapped (\d+)", res.output)
    assert [r[0] for r in rows] == [f"{k:06d}" for k in range(4)], res.output
    totals = np.zeros(5, dtype=np.int64)
    for k, r in enumerate(rows):
        n = np.array([int(v) for v in r[1:]])
        assert n.sum() == 32 * 256 and n[1] > 0.5 * n[1:].sum(), (k, n)  # the sweeps are the ones the map was made from: most returns agree
        totals += n
        png = open(f"{out}/changes_{k:06d}.png", "rb").read()
        assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (256, 32)
        raw = np.frombuffer(zlib.decompress(png[png.index(b"IDAT") + 4:-16]), dtype=np.uint8).reshape(32, 1 + 4 * 256)[:, 1:].reshape(32, 256, 4)
        colours, counts = np.unique(raw.reshape(-1, 4), axis=0, return_counts=True)
        assert sorted(counts.tolist()) == sorted(v for v in n.tolist() if v), "one fixed colour per class"
    m = re.search(r"changes, all sweeps: none (\d+), agree (\d+), new (\d+), gone (\d+), unmapped (\d+)", res.output)
    assert m and [int(v) for v in m.groups()] == totals.tolist(), res.output
