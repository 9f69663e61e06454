"""The map painted on the device (csrc/paint_kernels.h) against its restatement (tests/helpers/map_paint_numpy.py).  Every
output is an integer, so everything is compared for equality, with no tolerance anywhere: `sum` and `count` of EVERY stored point and every count
of the summary.  The restatement takes the stored points as the device returns them (the pool order is the map's business; that they are the
map's points is checked against `map_points()`) and the column poses from the device (`traj_poses_at`, the one definition of the geodesic).

The main property: a map built from sweeps S on trajectory T and painted with S on T has count >= 1 at every stored point, and the unmatched
rays are exactly the returns the build did not store.

Per-call `core.Icp` maps with small capacities; sweeps of H x 16 pixels with H W in {16, 64, 80, 256, 272}: under, at and across a wavefront and
a workgroup."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import map_paint_numpy as mp

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
PTL_ERR_ARG, PTL_ERR_CAPACITY, PTL_ERR_STATE = -1, -3, -4
VS = 0.5
BOUNDS = 0.5
W = 16
ROWS = [1, 4, 5, 16, 17]  # H W = 16, 64, 80, 256, 272
ALL_ONES = 0xffffffff


def _core():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    return core


def _icp(n_max, vs=VS, P=20, **over):
    kw = dict(voxel_size=vs, max_points_per_voxel=P, scan_cols=W, max_points_per_scan=n_max, **CAPS)
    kw.update(over)
    return _core().Icp(1.0e9, 0.0, **kw)


def _lex(p):
    p = np.asarray(p, dtype=np.float64)
    return np.ascontiguousarray(p[np.lexsort(p.T[::-1])])


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

    def col_ts(self, k):
        return k * self.dt + (np.arange(W) / W) * self.dt

    def col_poses(self, ts):
        out, n_out = _core().traj_poses_at(self.ts, self.poses, ts, BOUNDS, BOUNDS)
        assert n_out == 0
        return out


class _Scene:
    """n sweeps of H x 16 range images (a tenth of the pixels without a return; ranges of 0.8 .. 2.5 m under beams 1.25 degrees apart, so
    neighbouring beams share 0.5 m voxels) with a field image each: random u32 words, 0 and all ones among them, non-zero on the pixels without
    a return too"""

    def __init__(self, H, n=3, seed=0):
        core = _core()
        rng = np.random.default_rng(seed)
        self.H, self.n = H, n
        self.kn = _Knots(n, seed=seed)
        self.lut = core.Lut(H, W, np.linspace(10.0, -10.0, H), np.zeros(H), 0.0)
        self.rng_mm = [np.where(rng.random((H, W)) < 0.1, 0, rng.integers(800, 2500, (H, W))).astype(np.uint32) for _ in range(n)]
        self.field = []
        for _ in range(n):
            f = rng.integers(1, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
            f.reshape(-1)[rng.integers(0, H * W, 2)] = 0
            f.reshape(-1)[rng.integers(0, H * W, 2)] = ALL_ONES
            self.field.append(f)
        self.returns = [int((r != 0).sum()) for r in self.rng_mm]

    def build(self, P, which=None, vs=VS):
        m = _icp(max(self.H * W, 64), vs=vs, P=P)
        for k in (range(self.n) if which is None else which):
            nv, skipped = m.map_add_posed(self.kn.traj, self.kn.col_ts(k), range_mm=self.rng_mm[k], lut=self.lut)
            assert (nv, skipped) == (self.returns[k], False)
        return m

    def paint(self, painter, k, field=None):
        return painter.add_posed(self.kn.traj, self.kn.col_ts(k), self.field[k] if field is None else field, range_mm=self.rng_mm[k], lut=self.lut)

    def rays(self, k, field=None):
        p = self.lut(self.rng_mm[k]).reshape(self.H, W, 3)
        return mp.rays_of_sweep(p, self.rng_mm[k] != 0, self.kn.col_poses(self.kn.col_ts(k)), self.field[k] if field is None else field)

    def close(self):
        self.lut.close(); self.kn.traj.close()


def _check(map_icp, v, sweeps, what=""):
    """a core.PaintValues against the restatement: the returned points are the map's, every point's sum and count, every count of the summary"""
    stored = map_icp.map_points()
    assert v.result.n_points == len(stored) == len(v.xyz) == len(v.sum) == len(v.count), what
    assert v.sum.dtype == np.uint64 and v.count.dtype == np.uint32
    assert np.array_equal(_lex(v.xyz), _lex(stored)), what
    s, k, n = mp.paint(v.xyz, sweeps, float(map_icp.cfg.voxel_size))
    bad = np.flatnonzero((v.sum != s) | (v.count != k))
    assert len(bad) == 0, (what, len(bad), v.xyz[bad[:5]], v.sum[bad[:5]], s[bad[:5]], v.count[bad[:5]], k[bad[:5]])
    for key in mp.COUNTS:
        assert getattr(v.result, key) == n[key], (what, key, getattr(v.result, key), n[key])
    return n


def _rows(v):
    return mp.sorted_rows(v.xyz, v.sum, v.count)


def _counts(v):
    return [getattr(v.result, k) for k in mp.COUNTS]


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


# (a) the invariant, (b) the same sweeps twice, (n) the reverse order
@pytest.mark.parametrize("P", [1, 5, 20])
@pytest.mark.parametrize("H", ROWS)
def test_a_map_painted_by_the_sweeps_that_built_it(H, P):
    core = _core()
    sc = _Scene(H, seed=100 * H + P)
    m = sc.build(P)
    n_stored = m.map_size()[1]
    a = core.Painter(m)
    matched = [sc.paint(a, k) for k in range(sc.n)]
    sweeps = [sc.rays(k) for k in range(sc.n)]
    v = a.values()
    n = _check(m, v, sweeps, f"{H} x {W}, P = {P}")
    assert (v.count >= 1).all(), "every stored point is the end of one of the rays that built the map"
    assert v.result.n_points_painted == n_stored
    assert v.result.n_rays_unmatched == sum(sc.returns) - n_stored, "the unmatched rays are the returns the build did not store"
    assert v.result.n_no_return == sc.n * H * W - sum(sc.returns) > 0 or H == 1
    assert sum(x[0] for x in matched) == v.result.n_rays_matched and not any(x[1] for x in matched)
    if P == 1 and H >= 16:
        assert n["n_rays_unmatched"] > 0, "the scene has full voxels"
    # (b) once more: sums and counts double, the values stay after a read
    for k in range(sc.n):
        sc.paint(a, k)
    v2 = a.values()
    assert np.array_equal(v2.xyz, v.xyz) and np.array_equal(v2.sum, 2 * v.sum) and np.array_equal(v2.count, 2 * v.count)
    assert v2.result.n_rays_matched == 2 * v.result.n_rays_matched and v2.result.n_scans == 2 * sc.n and v2.result.sum_count == 2 * v.result.sum_count
    # (n) a second painter on the same map, the sweeps in reverse order
    b = core.Painter(m)
    for k in reversed(range(sc.n)):
        sc.paint(b, k)
    vb = b.values()
    assert np.array_equal(vb.xyz, v.xyz) and np.array_equal(vb.sum, v.sum) and np.array_equal(vb.count, v.count) and _counts(vb) == _counts(v)
    a.close(); b.close(); m.close(); sc.close()


# (c) a full voxel
def test_a_full_voxel_paints_only_its_stored_point():
    core = _core()
    m = _icp(64, P=1)
    traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
    ts = 0.25 + np.arange(W) / 64.0
    xyz = np.zeros((1, W, 3), dtype=np.float32)
    xyz[0, :4] = [[1.125, 0.125, 0.125], [1.25, 0.125, 0.125], [1.375, 0.125, 0.125], [2.125, 0.125, 0.125]]  # three in voxel (2, 0, 0), one in (4, 0, 0)
    field = np.arange(10, 10 + W, dtype=np.uint32).reshape(1, W)
    assert m.map_add_posed(traj, ts, xyz=xyz, H=1) == (4, False) and m.map_size() == (2, 2)
    p = core.Painter(m)
    assert p.add_posed(traj, ts, field, xyz=xyz, H=1) == (2, False)
    v = p.values()
    _check(m, v, [mp.rays_of_sweep(xyz.astype(np.float64), np.any(xyz != 0.0, axis=2), np.tile(np.eye(4), (W, 1, 1)), field)], "full voxel")
    got = {tuple(x): (int(s), int(k)) for x, s, k in zip(v.xyz, v.sum, v.count)}
    assert got == {(1.125, 0.125, 0.125): (10, 1), (2.125, 0.125, 0.125): (13, 1)}
    assert (v.result.n_rays_matched, v.result.n_rays_unmatched, v.result.n_no_return) == (2, 2, W - 4)
    p.close(); traj.close(); m.close()


# (d) absent voxels, (e) a foreign map, (g) a sweep outside the bounds, (h) no-return pixels, (f) 0 and all ones
def test_a_map_of_a_subset_of_the_sweeps():
    core = _core()
    sc = _Scene(5, seed=4)
    m = sc.build(5, which=[0, 1])
    p = core.Painter(m)
    for k in range(3):
        sc.paint(p, k)
    v = p.values()
    n = _check(m, v, [sc.rays(k) for k in range(3)], "subset")
    assert (v.count >= 1).all() and n["n_rays_unmatched"] >= sum(sc.returns[:2]) - m.map_size()[1] and n["n_rays_unmatched"] > 0
    p.close(); m.close(); sc.close()


def test_a_map_of_foreign_points():
    core = _core()
    sc = _Scene(5, seed=5)
    cloud = np.random.default_rng(5).uniform(-3.0, 3.0, (300, 3))
    m = core.map_from_points(cloud, voxel_size=VS, max_points_per_voxel=5, max_points_per_scan=512, scan_cols=W, **CAPS)
    p = core.Painter(m)
    for k in range(3):
        assert sc.paint(p, k) == (0, False)
    v = p.values()
    _check(m, v, [sc.rays(k) for k in range(3)], "foreign")
    assert not v.sum.any() and not v.count.any() and np.isnan(v.mean()).all()
    assert (v.result.n_points_painted, v.result.n_rays_matched, v.result.n_rays_unmatched, v.result.sum_count) == (0, 0, sum(sc.returns), 0)
    p.close(); m.close(); sc.close()


def test_skipped_sweeps_no_returns_and_the_ends_of_the_value_range():
    core = _core()
    H = 5
    sc = _Scene(H, seed=6)
    m = sc.build(20)
    p = core.Painter(m)
    # (f) three rays of all ones at every stored point of sweep 0, zeros from sweep 1: the u64 does not wrap, a zero counts
    ones, zeros = np.full((H, W), ALL_ONES, dtype=np.uint32), np.zeros((H, W), dtype=np.uint32)
    for _ in range(3):
        sc.paint(p, 0, ones)
    sc.paint(p, 1, zeros)
    sweeps = [sc.rays(0, ones)] * 3 + [sc.rays(1, zeros)]
    v = p.values()
    _check(m, v, sweeps, "all ones and zeros")
    assert int(v.sum.max()) == 3 * ALL_ONES > 1 << 33 and ((v.sum == 0) & (v.count >= 1)).any()
    assert np.array_equal(v.mean()[v.sum == 3 * ALL_ONES], np.full(int((v.sum == 3 * ALL_ONES).sum()), float(ALL_ONES)))
    # (g) a sweep with a column outside the bounds is skipped as a whole and counted
    late = sc.kn.col_ts(2) + 100.0
    assert p.add_posed(sc.kn.traj, late, sc.field[2], range_mm=sc.rng_mm[2], lut=sc.lut) == (0, True)
    one_late = sc.kn.col_ts(2).copy()
    one_late[W - 1] += 100.0
    assert p.add_posed(sc.kn.traj, one_late, sc.field[2], range_mm=sc.rng_mm[2], lut=sc.lut) == (0, True)
    # (h) pixels without a return that carry a field value add nothing
    none = np.zeros((H, W), dtype=np.uint32)
    assert p.add_posed(sc.kn.traj, sc.kn.col_ts(2), ones, range_mm=none, lut=sc.lut) == (0, False)
    v2 = p.values()
    sweeps += [None, None, mp.rays_of_sweep(np.zeros((H, W, 3)), none != 0, sc.kn.col_poses(sc.kn.col_ts(2)), ones)]
    _check(m, v2, sweeps, "skipped and empty sweeps")
    assert np.array_equal(v2.sum, v.sum) and np.array_equal(v2.count, v.count)
    assert (v2.result.n_scans, v2.result.n_scans_skipped, v2.result.n_no_return - v.result.n_no_return) == (5, 2, H * W)
    p.close(); m.close(); sc.close()


# (i) the xyz form
@pytest.mark.parametrize("H", [1, 17])
def test_the_xyz_form(H):
    """The sweeps as f32 points (the LUT's points rounded to f32) into a map of their own through the xyz calls: the invariant and the
    restatement as for the range form, and the same pixels without a return.  (The two forms cannot be held against each other bit by bit: the
    range form's sensor-frame points are doubles that no f32 holds.)"""
    core = _core()
    sc = _Scene(H, seed=9)
    xyz = [sc.lut(r).reshape(H, W, 3).astype(np.float32) for r in sc.rng_mm]
    m = _icp(max(H * W, 64), P=5)
    for k in range(sc.n):
        assert m.map_add_posed(sc.kn.traj, sc.kn.col_ts(k), xyz=xyz[k], H=H) == (sc.returns[k], False)
    p, q = core.Painter(m), core.Painter(sc.build(5))
    sweeps = []
    for k in range(sc.n):
        p.add_posed(sc.kn.traj, sc.kn.col_ts(k), sc.field[k], xyz=xyz[k], H=H)
        sc.paint(q, k)
        sweeps.append(mp.rays_of_sweep(xyz[k].astype(np.float64), np.any(xyz[k] != 0.0, axis=2), sc.kn.col_poses(sc.kn.col_ts(k)), sc.field[k]))
    v, vq = p.values(), q.values()
    _check(m, v, sweeps, "xyz form")
    assert (v.count >= 1).all() and v.result.n_rays_unmatched == sum(sc.returns) - m.map_size()[1]
    assert (v.result.n_no_return, v.result.n_scans) == (vq.result.n_no_return, vq.result.n_scans)
    assert v.result.n_rays_matched + v.result.n_rays_unmatched == vq.result.n_rays_matched + vq.result.n_rays_unmatched == sum(sc.returns)
    q.map_icp.close(); p.close(); q.close(); m.close(); sc.close()


# (j) a map with small and full blocks: the map of a free-running batch with map_small_blocks (tests/test_gpu_map_carve.py's recipe)
def test_a_map_with_small_and_full_blocks():
    """The batch registers its first sweep at the identity, so the points it stores of that sweep are the sweep's own f32 points as doubles: a
    paint of that sweep under the identity trajectory ends at them."""
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
            vs = float(member.cfg.voxel_size)
            Wm = int(member.cfg.scan_cols)
            H = fv.BOX_PTS // Wm
            traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
            ts = np.arange(Wm) / (2.0 * Wm)
            x = np.asarray(frames[0], dtype=np.float32).reshape(H, Wm, 3)
            field = np.random.default_rng(3).integers(0, 1 << 32, (H, Wm), dtype=np.uint64).astype(np.uint32)
            p = core.Painter(member)
            p.add_posed(traj, ts, field, xyz=x, H=H)
            v = p.values()
            n = _check(member, v, [mp.rays_of_sweep(x.astype(np.float64), np.any(x != 0.0, axis=2), np.tile(np.eye(4), (Wm, 1, 1)), field)],
                       "two block classes")
            assert n["n_rays_matched"] > 0 and n["n_rays_unmatched"] > 0
            keys = [mp.key_of([float(c) for c in q], vs) for q in v.xyz]
            per_voxel = {}
            for key in keys:
                per_voxel[key] = per_voxel.get(key, 0) + 1
            size = np.array([per_voxel[key] for key in keys])
            assert len(pts) == len(v.xyz) and ((size <= 5) & (v.count > 0)).any() and ((size > 5) & (v.count > 0)).any(), "painted points in both block classes"
            p.close(); traj.close()
        finally:
            member._h = None
    finally:
        r.close()


# (k) read-only
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
    sc = _Scene(16, seed=7)
    m = sc.build(5)
    # (map_points() hands the blocks out in the order its workgroups arrive: the rows are compared in lexicographic order)
    table, pts = _table_bytes(m), _lex(m.map_points()).tobytes()
    p = core.Painter(m)
    for k in range(sc.n):
        sc.paint(p, k)
    v = p.values()
    assert v.result.sum_count > 0
    assert _table_bytes(m) == table, "the table and the directory are byte-equal"
    assert _lex(m.map_points()).tobytes() == pts, "the points are byte-equal"
    p.close()
    assert _table_bytes(m) == table
    m.close(); sc.close()


# (l), (m) and the refusals with their numbers
def test_state_capacity_and_argument_refusals():
    from ptudes_lab_amd import _lib as L
    core = _core()
    H = 4
    sc = _Scene(H, seed=8)
    m = sc.build(5)
    n = m.map_size()[1]
    p = core.Painter(m)
    sc.paint(p, 0)
    lib = L.lib()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    # (m) too small a max_points: PTL_ERR_CAPACITY naming the count, the arrays and the count untouched
    xyz, s, k = np.full((n, 3), 7.0), np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint32)
    res, w = L.PaintResult(), C.c_int64(-5)
    rc = lib.ptl_paint_read(p._h, C.byref(res), L.dptr(xyz), s.ctypes.data_as(u64p), k.ctypes.data_as(u32p), n - 1, C.byref(w))
    msg = lib.ptl_last_error().decode()
    assert rc == PTL_ERR_CAPACITY and str(n) in msg and str(n - 1) in msg, msg
    assert (xyz == 7.0).all() and (s == 7).all() and (k == 7).all() and w.value == -5 and res.n_points == 0
    # two of the three arrays, a negative max_points
    assert lib.ptl_paint_read(p._h, C.byref(res), L.dptr(xyz), None, k.ctypes.data_as(u32p), n, None) == PTL_ERR_ARG
    assert "2 given" in lib.ptl_last_error().decode()
    assert lib.ptl_paint_read(p._h, C.byref(res), L.dptr(xyz), s.ctypes.data_as(u64p), k.ctypes.data_as(u32p), -1, None) == PTL_ERR_ARG
    assert "-1" in lib.ptl_last_error().decode()
    # the summary alone
    assert lib.ptl_paint_read(p._h, C.byref(res), None, None, None, 0, None) == 0 and res.n_points == n and res.n_scans == 1
    assert (xyz == 7.0).all()
    # the sweep's geometry against the map handle's
    wide = core.Lut(H, 2 * W, np.linspace(10.0, -10.0, H), np.zeros(H), 0.0)
    _refused(PTL_ERR_CAPACITY, lambda: p.add_posed(sc.kn.traj, np.arange(2 * W) / 1000.0, np.zeros((H, 2 * W)), range_mm=np.zeros((H, 2 * W)), lut=wide),
             2 * W, W, "scan_cols")
    tall = core.Lut(8, W, np.linspace(10.0, -10.0, 8), np.zeros(8), 0.0)
    _refused(PTL_ERR_CAPACITY, lambda: p.add_posed(sc.kn.traj, sc.kn.col_ts(0), np.zeros((8, W)), range_mm=np.zeros((8, W)), lut=tall),
             8 * W, 64, "max_points_per_scan")
    _refused(PTL_ERR_ARG, lambda: p.add_posed(sc.kn.traj, sc.kn.col_ts(0), np.zeros((H, W - 1)), range_mm=sc.rng_mm[0], lut=sc.lut), "field")
    before = p.values()
    # (l) a map updated after create
    m.map_add(np.array([[40.0, 40.0, 40.0]]))
    _refused(PTL_ERR_STATE, lambda: sc.paint(p, 1), n + 1, n, "ptl_paint_create")
    _refused(PTL_ERR_STATE, p.values, n + 1, n)
    q = core.Painter(m)  # a new painter sees the new point
    sc.paint(q, 0)
    vq = q.values()
    assert vq.result.n_points == n + 1 and vq.result.n_points_painted == before.result.n_points_painted
    assert np.array_equal(_rows(vq)[:, 3:].sum(axis=0), _rows(before)[:, 3:].sum(axis=0))
    for x in (p, q, wide, tall, m, sc):
        x.close()
