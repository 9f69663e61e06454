"""The occupancy grid on the device (csrc/grid_kernels.h) against its numpy restatement (tests/helpers/occupancy_grid_numpy.py).
Every output is an integer, so everything is compared for equality: `free` and `hit` of EVERY cell, every count of the summary and the touched
box.  The restatement takes the column poses from the device (`traj_poses_at`, the one definition of the geodesic): where a column's pose lies
is tested elsewhere; what is tested here is the march, the runs and the votes.  Sweeps of a few hundred pixels unless the case says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import occupancy_grid_cases as gc
from tests.helpers import occupancy_grid_numpy as og

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
PTL_ERR_ARG, PTL_ERR_CAPACITY, PTL_ERR_STATE = -1, -3, -4
BOUNDS = 0.5
GRIDS = {"1x1": dict(cell=4.0, x0=-1.0, y0=-1.0, nx=1, ny=1), "1x9": dict(cell=1.0, x0=0.25, y0=-4.5, nx=1, ny=9),
         "9x1": dict(cell=0.5, x0=-2.0, y0=0.0, nx=9, ny=1), "7x5": dict(cell=1.0, x0=-3.5, y0=-2.5, nx=7, ny=5),
         "64x64": dict(cell=0.25, x0=-8.0, y0=-8.0, nx=64, ny=64)}


def _core():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    return core


def _grid(cfg, W, n_max):
    return _core().OccupancyGrid(cfg["cell"], cfg["x0"], cfg["y0"], cfg["nx"], cfg["ny"], W, n_max,
                                 **{k: cfg[k] for k in ("z_lo", "z_hi", "margin", "step", "min_range", "max_range") if k in cfg})


def _cfg_of(res):
    return {k: getattr(res, k) for k in ("cell", "x0", "y0", "nx", "ny", "z_lo", "z_hi", "margin", "step", "min_range", "max_range")}


def _check(g, sweeps, what=""):
    """a core.OccupancyGrid against the restatement: every cell's two counts, every count of the summary, the touched box"""
    c = g.read()
    cfg = _cfg_of(c.result)
    assert c.free.dtype == np.uint32 and c.hit.dtype == np.uint32 and c.free.shape == c.hit.shape == (cfg["ny"], cfg["nx"]), what
    assert (c.cell, c.origin) == (cfg["cell"], (cfg["x0"], cfg["y0"]))
    free, hit, n = og.grid(sweeps, cfg)
    for name, got, want in (("free", c.free, free), ("hit", c.hit, hit)):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, name, len(bad), [(int(iy), int(ix), int(got[iy, ix]), int(want[iy, ix])) for iy, ix in bad[:5]])
    for k in og.COUNTS + og.BOX:
        assert getattr(c.result, k) == n[k], (what, k, getattr(c.result, k), n[k])
    return n


class _Knots:
    """a trajectory that rotates and translates within a sweep: knots every 50 ms"""

    def __init__(self, n_sweeps, dt=0.1, seed=0):
        from ptudes_lab_amd.utils import exp_pose6
        rng = np.random.default_rng(seed)
        self.dt = dt
        self.ts = np.arange(-1, 2 * n_sweeps + 2) * (dt / 2)
        twist = np.concatenate([rng.uniform(-0.6, 0.6, 3) * [0.2, 0.2, 1.0], rng.uniform(-2.0, 2.0, 3) * [1.0, 1.0, 0.1]])
        self.poses = np.array([exp_pose6(twist * t) for t in self.ts])
        self.traj = _core().Traj(self.ts, self.poses, BOUNDS, BOUNDS)

    def col_ts(self, k, W):
        return k * self.dt + (np.arange(W) / W) * self.dt

    def col_poses(self, ts):
        out, n_out = _core().traj_poses_at(self.ts, self.poses, ts, BOUNDS, BOUNDS)
        assert n_out == 0
        return out

    def rays(self, k, xyz):
        H, W = xyz.shape[:2]
        return og.rays_of_sweep(xyz.astype(np.float64), np.any(xyz != 0.0, axis=2), self.col_poses(self.col_ts(k, W)))


def _random_sweeps(rng, n, H, W, reach=6.0, holes=0.1):
    """n sweeps of H x W f32 points in the sensor frame, mostly near the horizontal, (0, 0, 0) = no return; a few beyond any max_range used
    here, a few on a lattice of eighths (cell edges)"""
    out = []
    for _ in range(n):
        u = rng.normal(size=(H, W, 3)) * np.array([1.0, 1.0, 0.15])
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        r = rng.uniform(0.05, reach, (H, W, 1)) * np.where(rng.random((H, W, 1)) < 0.03, 20.0, 1.0)
        x = u * r
        snap = rng.random((H, W)) < 0.2
        x[snap] = np.round(x[snap] * 8.0) / 8.0
        x = x.astype(np.float32)
        x[rng.random((H, W)) < holes] = 0.0
        out.append(x)
    return out


def _band(cfg, **over):
    return dict(dict(z_lo=-0.5, z_hi=0.5, margin=cfg["cell"], step=cfg["cell"] / 2.0, min_range=0.0, max_range=20.0), **cfg, **over)


# 1. the answers written out by hand
def test_hand_cases():
    core = _core()
    cases = gc.hand_cases()
    for case in cases:
        pose = np.eye(4)
        pose[:3, 3] = case["origin"]
        traj = core.Traj([0.0, 1.0], [pose, pose], BOUNDS, BOUNDS)
        ts = 0.25 + np.arange(gc.W) / 16.0
        poses, n_out = core.traj_poses_at([0.0, 1.0], [pose, pose], ts, BOUNDS, BOUNDS)
        assert n_out == 0 and (poses == pose[None]).all(), "the geodesic between equal poses is that pose, bit for bit"
        g = _grid(case["cfg"], gc.W, gc.W)
        n_rays, skipped = g.add_posed(traj, ts, xyz=case["xyz"], H=1)
        assert (n_rays, skipped) == (case["counts"]["n_rays"], False), case["name"]
        n = _check(g, [gc.case_rays(case, poses)], case["name"])
        c = g.read()
        want_free, want_hit = gc.case_arrays(case)
        assert np.array_equal(c.free, want_free) and np.array_equal(c.hit, want_hit), case["name"]
        for k, want in case["counts"].items():
            assert getattr(c.result, k) == want == n[k], (case["name"], k)
        g.close(); traj.close()


# 2. random scenes on a trajectory that rotates and translates within a sweep: H W = 1, 63, 65 and 257 pixels (the wavefront and workgroup
#    edges), grids of 1 x 1, 1 x 9, 9 x 1, 7 x 5 and 64 x 64 cells
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (5, 13), (1, 257)])
def test_random_scenes(H, W):
    rng = np.random.default_rng(H * W)
    N = 3
    kn = _Knots(N, seed=H * W)
    xyz = _random_sweeps(rng, N, H, W)
    sweeps = [kn.rays(k, xyz[k]) for k in range(N)]
    total = dict.fromkeys(("sum_free", "sum_hit", "n_ends_outside", "n_rays_out_of_range", "n_no_return"), 0)
    for name, gcfg in GRIDS.items():
        for cfg in (_band(gcfg), _band(gcfg, margin=0.0, step=gcfg["cell"] / 3.0, min_range=0.5, max_range=5.0, z_lo=-0.1, z_hi=0.3)):
            g = _grid(cfg, W, H * W)
            for k in range(N):
                assert g.add_posed(kn.traj, kn.col_ts(k, W), xyz=xyz[k], H=H)[1] is False
            n = _check(g, sweeps, f"{H} x {W}, grid {name}")
            assert n["n_rays"] + n["n_rays_out_of_range"] + n["n_no_return"] == N * H * W and n["sum_free"] == n["n_runs_voted"]
            for k in total:
                total[k] += n[k]
            g.close()
    if H * W > 1:
        assert all(v > 0 for v in total.values()), total
    kn.traj.close()


# 3. the grid stride: one sweep of 129 x 2 048 short rays is past the 262 144 lanes of a capped launch
def test_the_grid_stride():
    core = _core()
    H, W = 129, 2048
    rng = np.random.default_rng(129)
    az = 2.0 * np.pi * np.arange(W) / W
    r = rng.uniform(0.1, 1.5, (H, W))
    z = rng.uniform(-0.6, 0.6, (H, W))
    xyz = np.stack([r * np.cos(az)[None, :], r * np.sin(az)[None, :], z], axis=2).astype(np.float32)
    xyz[rng.random((H, W)) < 0.05] = 0.0
    xyz[H - 1, W - 3:] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.25]]  # the last pixels of the sweep, past the first stride
    kn = _Knots(1, seed=3)
    cfg = _band(dict(cell=0.25, x0=-2.0, y0=-2.0, nx=16, ny=16), margin=0.125)
    g = _grid(cfg, W, H * W)
    n_rays, skipped = g.add_posed(kn.traj, kn.col_ts(0, W), xyz=xyz, H=H)
    n = _check(g, [kn.rays(0, xyz)], "129 x 2048")
    assert H * W > 1024 * 256 and n_rays == n["n_rays"] > 240_000 and not skipped and n["sum_free"] > n["n_rays"] and n["sum_hit"] > 100_000
    g.close(); kn.traj.close()


# 4. path agreement
def test_paths_agree():
    """range image + LUT = xyz of the LUT's points; add_run on a SeqRunner's and a BatchRunner's resident sweeps = per call"""
    core = _core()
    H, W, N = 8, 32, 4
    rng = np.random.default_rng(11)
    kn = _Knots(N, seed=11)
    lut = core.Lut(H, W, np.linspace(6.0, -6.0, H), np.zeros(H), 0.0)
    rng_mm = [np.where(rng.random((H, W)) < 0.1, 0, rng.integers(300, 7000, (H, W))).astype(np.uint32) for _ in range(N)]
    cfg = _band(GRIDS["64x64"], max_range=6.0)
    # (a) the range path against the restatement on the LUT's own points
    a = _grid(cfg, W, H * W)
    sweeps = []
    for k in range(N):
        pts = lut(rng_mm[k]).reshape(H, W, 3)
        a.add_posed(kn.traj, kn.col_ts(k, W), range_mm=rng_mm[k], lut=lut)
        sweeps.append(og.rays_of_sweep(pts, rng_mm[k] != 0, kn.col_poses(kn.col_ts(k, W))))
    na = _check(a, sweeps, "range path")
    assert na["sum_free"] > 1000 and na["sum_hit"] > 100 and na["n_rays_out_of_range"] > 0 and na["n_no_return"] > 0
    ca = a.read()

    def same(g, what, ref=ca):
        c = g.read()
        assert np.array_equal(c.free, ref.free) and np.array_equal(c.hit, ref.hit), what
        assert all(getattr(c.result, k) == getattr(ref.result, k) for k in og.COUNTS + og.BOX), what

    # (b) a batch's resident range images: sequence 1 of 2
    t0t1 = np.array([[k * kn.dt, (k + 1) * kn.dt] for k in range(N)])
    bt = core.BatchRunner(2, N, H * W, 0, max_range=100.0, min_range=0.0, with_ekf=False, range_input=True, scan_cols=W, **CAPS)
    bt.set_lut(lut)
    for s in range(2):
        for k in range(N):
            bt.upload_range(s, k, rng_mm[k] if s else rng_mm[0])
    b = _grid(cfg, W, W)  # (the staging is not used by resident sweeps: max_pixels_per_scan may be smaller than a sweep)
    assert b.add_run(bt, kn.traj, t0t1, s=1) == (ca.result.n_rays, 0)
    same(b, "batch, resident range images")
    # (c) a SeqRunner's resident xyz sweeps against the per-call xyz path
    xyz = _random_sweeps(rng, N, H, W)
    sr = core.SeqRunner(N, H * W, 0, max_range=100.0, min_range=0.0, with_ekf=False, scan_cols=W, **CAPS)
    for k in range(N):
        sr.upload_scan(k, xyz[k])
    d, e = _grid(cfg, W, H * W), _grid(cfg, W, H * W)
    n_rays, n_skipped = d.add_run(sr, kn.traj, t0t1)
    got = [e.add_posed(kn.traj, kn.col_ts(k, W), xyz=xyz[k], H=H) for k in range(N)]
    assert (n_rays, n_skipped) == (sum(x[0] for x in got), 0) and d.summary().n_scans == N
    same(d, "seq runner, resident xyz", e.read())
    _check(e, [kn.rays(k, xyz[k]) for k in range(N)], "xyz path")
    # first / last, and a sweep outside the bounds is skipped as a whole and counted
    f = _grid(cfg, W, H * W)
    late = t0t1.copy()
    late[2] += 100.0
    assert f.add_run(sr, kn.traj, late, first=1, last=3) == (got[1][0] + got[3][0], 1)
    _check(f, [kn.rays(1, xyz[1]), None, kn.rays(3, xyz[3])], "first / last with a skipped sweep")
    for x in (a, b, d, e, f, bt, sr, lut, kn.traj):
        x.close()


# 5. order and state
def test_order_and_state():
    core = _core()
    H, W, N = 6, 20, 4
    rng = np.random.default_rng(21)
    kn = _Knots(N, seed=21)
    xyz = _random_sweeps(rng, N, H, W)
    sweeps = [kn.rays(k, xyz[k]) for k in range(N)]
    cfg = _band(GRIDS["64x64"])
    a, b = _grid(cfg, W, H * W), _grid(cfg, W, H * W)  # two handles on one device, fed in turn, b in reverse order
    for k in range(N):
        a.add_posed(kn.traj, kn.col_ts(k, W), xyz=xyz[k], H=H)
        b.add_posed(kn.traj, kn.col_ts(N - 1 - k, W), xyz=xyz[N - 1 - k], H=H)
        if k == 1:
            _check(a, sweeps[:2], "add, read")  # add, read, add, read: the counts stay
    n = _check(a, sweeps, "add, read, add, read")
    _check(b, sweeps, "reverse order")
    # a sub-rectangle is the slice of the full read; its origin is its own corner
    full = a.read()
    part = a.read(5, 9, 40, 17)
    assert np.array_equal(part.free, full.free[9:26, 5:45]) and np.array_equal(part.hit, full.hit[9:26, 5:45]) and part.free.shape == (17, 40)
    assert part.origin == (cfg["x0"] + 5 * cfg["cell"], cfg["y0"] + 9 * cfg["cell"]) and part.result.sum_free == full.result.sum_free
    one = a.read(63, 63, 1, 1)
    assert one.free.shape == (1, 1) and one.free[0, 0] == full.free[63, 63]
    # a skipped sweep counts nothing but itself
    before = a.read()
    assert a.add_posed(kn.traj, kn.col_ts(0, W) + 100.0, xyz=xyz[0], H=H) == (0, True)
    after = a.read()
    assert np.array_equal(after.free, before.free) and np.array_equal(after.hit, before.hit)
    assert (after.result.n_scans_skipped, after.result.n_scans, after.result.n_rays, after.result.n_no_return) == \
        (1, N, n["n_rays"], n["n_no_return"])
    # clear: everything back to zero, the parameters stay, and the handle counts again
    a.clear()
    z = a.read()
    assert not z.free.any() and not z.hit.any() and all(getattr(z.result, k) == 0 for k in og.COUNTS)
    assert (z.result.box_ix0, z.result.box_iy0, z.result.box_ix1, z.result.box_iy1) == (0, 0, -1, -1) and _cfg_of(z.result) == _cfg_of(full.result)
    a.add_posed(kn.traj, kn.col_ts(2, W), xyz=xyz[2], H=H)
    _check(a, [sweeps[2]], "after clear")
    _check(b, sweeps, "the other handle is untouched")
    for x in (a, b, kn.traj):
        x.close()


# 6. failure paths, each before any HIP call and with the numbers
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


def test_refusals_and_the_ray_capacity():
    from ptudes_lab_amd import _lib as L
    core = _core()
    H, W = 4, 16
    cfg = _band(GRIDS["7x5"])
    g = _grid(cfg, W, H * W)
    lib = L.lib()
    traj = core.Traj([0.0, 1.0], [np.eye(4), np.eye(4)], BOUNDS, BOUNDS)
    ts = np.arange(W) / (2.0 * W)
    x = np.zeros((H, W, 3), dtype=np.float32)
    x[0, 0] = [2.0, 0.0, 0.0]  # one ray along +x
    fp, dp = x.ctypes.data_as(C.POINTER(C.c_float)), L.dptr(ts)
    # null pointers
    assert lib.ptl_grid_add_posed_xyz(None, traj._h, fp, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_posed_xyz(g._h, None, fp, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_posed_xyz(g._h, traj._h, None, H, W, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_posed_xyz(g._h, traj._h, fp, H, W, None, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_posed_range(g._h, traj._h, None, None, dp, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_seq(g._h, None, traj._h, dp, 0, 0, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_add_batch(g._h, None, 0, traj._h, dp, 0, 0, None, None) == PTL_ERR_ARG
    assert lib.ptl_grid_read(g._h, None, 0, 0, 0, 0, None, None) == PTL_ERR_ARG
    # W or H W not the handle's; an empty scan
    _refused(PTL_ERR_CAPACITY, lambda: g.add_posed(traj, np.arange(8) / 16.0, xyz=x[:, :8], H=H), "8 columns", W)
    _refused(PTL_ERR_CAPACITY, lambda: g.add_posed(traj, ts, xyz=np.zeros((H + 1, W, 3), dtype=np.float32), H=H + 1), (H + 1) * W, H * W)
    assert lib.ptl_grid_add_posed_xyz(g._h, traj._h, fp, 0, W, dp, None, None) == PTL_ERR_ARG and "0 x 16" in lib.ptl_last_error().decode()
    # different devices: with one device the rule is tested through the handle's device_id (its first member, an int)
    dev = C.c_int.from_address(traj._h.value)
    dev.value = 1
    _refused(PTL_ERR_ARG, lambda: g.add_posed(traj, ts, xyz=x, H=H), "device 1", "device 0")
    dev.value = 0
    # a rectangle that is empty or not inside the grid; one array of the two
    for rect in ((0, 0, 8, 5), (0, 0, 7, 6), (-1, 0, 2, 2), (6, 4, 2, 1), (3, 3, 0, 1), (3, 3, 1, -1)):
        _refused(PTL_ERR_ARG, lambda: g.read(*rect), f"{rect[2]} x {rect[3]} cells at ({rect[0]}, {rect[1]})", "7 x 5")
    one = np.zeros(35, dtype=np.uint32)
    assert lib.ptl_grid_read(g._h, C.byref(L.GridResult()), 0, 0, 7, 5, one.ctypes.data_as(C.POINTER(C.c_uint32)), None) == PTL_ERR_ARG
    assert "1 given" in lib.ptl_last_error().decode()
    # a runner of another scan_cols, sweeps that do not exist
    sr = core.SeqRunner(2, 4 * 8, 0, max_range=100.0, min_range=0.0, with_ekf=False, scan_cols=8, **CAPS)
    t0t1 = np.array([[0.0, 0.1], [0.1, 0.2]])
    _refused(PTL_ERR_CAPACITY, lambda: g.add_run(sr, traj, t0t1), "scan_cols", 8, W)
    _refused(PTL_ERR_ARG, lambda: g.add_run(sr, traj, t0t1, first=1, last=2), "[1, 2] of 2")
    sr.close()
    # the handle still works after all that
    assert g.add_posed(traj, ts, xyz=x, H=H) == (1, False)
    c = g.read()
    assert (c.result.n_rays, c.result.n_no_return, c.result.sum_hit) == (1, H * W - 1, 1)
    # the ray capacity: the handle's count of used rays (its second member, a u64 behind the device id) stands just below 2^32 - 1; an add
    # whose pixels could carry it past is refused with the numbers before anything is launched, one that cannot is taken
    used = C.c_uint64.from_address(g._h.value + 8)
    assert used.value == 1
    used.value = 0xffffffff - H * W + 1
    msg = _refused(PTL_ERR_CAPACITY, lambda: g.add_posed(traj, ts, xyz=x, H=H), 0xffffffff - H * W + 1, f"{H * W} pixels", 0xffffffff)
    assert "ptl_grid_clear" in msg
    same = g.read()
    assert np.array_equal(same.free, c.free) and np.array_equal(same.hit, c.hit) and same.result.n_rays == 1, "a refused add counts nothing"
    used.value = 0xffffffff - H * W
    assert g.add_posed(traj, ts, xyz=x, H=H) == (1, False)
    assert used.value == 2, "the count is the device's again after an add"
    sr = core.SeqRunner(2, H * W, 0, max_range=100.0, min_range=0.0, with_ekf=False, scan_cols=W, **CAPS)
    for k in range(2):
        sr.upload_scan(k, x)
    used.value = 0xffffffff - 2 * H * W + 1
    _refused(PTL_ERR_CAPACITY, lambda: g.add_run(sr, traj, t0t1), f"{2 * H * W} pixels")
    used.value = 2
    assert g.add_run(sr, traj, t0t1) == (2, 0) and g.summary().n_rays == 4
    g.clear()
    assert used.value == 0
    for x_ in (sr, g, traj):
        x_.close()


# 7. the moving-box scene: equality with the restatement, which meets the conditions (tests/test_occupancy_grid_cpu.py)
def test_the_moving_box_scene():
    from ptudes_lab_amd import fly
    from tests.helpers import map_carve_numpy as cv
    from tests.test_occupancy_grid_cpu import BOX_ORIGIN_CELLS, BOX_TRAIL_CELLS, BOX_WALL_CELLS
    core = _core()
    scene = cv.moving_box_scene()
    H, W = scene[0][0].shape[:2]
    knots_t = np.arange(2 * len(scene)) * 0.5
    knots_p = np.repeat(np.array([pose for _, pose, _ in scene]), 2, axis=0)
    traj = core.Traj(knots_t, knots_p, 0.0, 0.0)
    col_ts = [k + 0.25 * np.arange(W) / W for k in range(len(scene))]  # sweep k lies between its own two knots
    cfg = og.BOX_GRID
    bounds = (cfg["x0"], cfg["y0"], cfg["x0"] + cfg["nx"] * cfg["cell"], cfg["y0"] + cfg["ny"] * cfg["cell"])
    b = fly.GridBuilder((H, W), bounds, cfg["cell"], **{k: cfg[k] for k in ("z_lo", "z_hi", "margin", "step", "min_range", "max_range")})
    poses = []
    for k, (xyz, _, _) in enumerate(scene):
        b.grid.add_posed(traj, col_ts[k], xyz=xyz, H=H)
        poses.append(core.traj_poses_at(knots_t, knots_p, col_ts[k])[0])
    sweeps, _ = cv.moving_box_rays(scene, poses)
    n = _check(b.grid, sweeps, "moving box")
    assert _cfg_of(b.grid.summary()) == cfg
    # the builder's counts are the touched box of the full read
    c, full = b.counts(), b.grid.read()
    x0, y0, x1, y1 = (n[k] for k in og.BOX)
    assert np.array_equal(c.free, full.free[y0:y1 + 1, x0:x1 + 1]) and np.array_equal(c.hit, full.hit[y0:y1 + 1, x0:x1 + 1])
    assert c.origin == (cfg["x0"] + x0 * cfg["cell"], cfg["y0"] + y0 * cfg["cell"])
    # and the conditions, on the device's counts
    cls = full.classify()
    at = lambda cells: np.array([cls[iy, ix] for ix, iy in cells])  # noqa: E731
    origins = {og.cell_of(float(o[0, 0]), float(o[0, 1]), cfg) for o, _, _ in sweeps}
    walls, trail = og.outline_cells(cfg), og.box_trail_cells(scene, sweeps, cfg)
    assert (len(origins), len(walls), len(trail)) == (BOX_ORIGIN_CELLS, BOX_WALL_CELLS, BOX_TRAIL_CELLS)
    assert (at(origins) == core.GRID_FREE).all() and (at(walls) == core.GRID_OCCUPIED).all() and (at(trail) == core.GRID_FREE).all()
    for x in (b, traj):
        x.close()


# 8. the command
def test_flyby_saves_the_grid(tmp_path):
    import re
    from click.testing import CliRunner
    from ptudes_lab_amd import fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    core = _core()
    p, prefix, npz = str(tmp_path / "p.csv"), str(tmp_path / "grid"), str(tmp_path / "counts.npz")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "2", "--use-imu-prediction",
                                          "--save-nc-gt-poses", p])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "1", "--save-grid", prefix,
                                          "--grid-cell", "0.5", "--grid-max-range", "30", "--grid-band", "-0.25,0.75", "--grid-min-hits", "3",
                                          "--save-grid-counts", npz])
    assert res.exit_code == 0, res.output
    assert sorted(os.listdir(tmp_path)) == ["counts.npz", "grid.pgm", "grid.yaml", "p.csv"]
    # the restatement on the same sweeps under the same trajectory, on the grid the command made of the poses
    gts = pu.read_newer_college_gt(p)
    inv0 = np.linalg.inv(gts[0][1])
    gts = [(t, inv0 @ q) for t, q in gts]
    kt, kp = [t for t, _ in gts], [q for _, q in gts]
    seq = synth.make_sequence(seed=1000, n_scans=2)
    lut, scans = fly.synthetic_range_scans(seq, 0, 1)
    x0, y0, nx, ny = fly.grid_bounds(np.array([q[:3, 3] for q in kp[:2]]), 0.5, 30.0)
    cfg = dict(og.defaults(0.5), x0=x0, y0=y0, nx=nx, ny=ny, max_range=30.0, z_lo=-0.25, z_hi=0.75)
    sweeps = []
    for s in scans:
        poses, n_out = core.traj_poses_at(kt, kp, np.asarray(s.timestamp, dtype=np.float64) * 1e-9, 1.5, 1.5)
        assert n_out == 0
        sweeps.append(og.rays_of_sweep(lut(s.range_mm).reshape(seq.H, seq.W, 3), s.range_mm != 0, poses))
    lut.close()
    free, hit, n = og.grid(sweeps, cfg)
    bx0, by0, bx1, by1 = (n[k] for k in og.BOX)
    want = og.classify(free, hit, min_hits=3)[by0:by1 + 1, bx0:bx1 + 1]
    classes, cell, origin = pu.load_occupancy_map(prefix)
    assert np.array_equal(classes, want) and cell == 0.5 and origin == (x0 + bx0 * 0.5, y0 + by0 * 0.5)
    assert (want == og.FREE).sum() > 1000 and (want == og.OCCUPIED).sum() > 50 and (want == og.UNKNOWN).sum() > 0
    z = np.load(npz)
    assert np.array_equal(z["free"], free[by0:by1 + 1, bx0:bx1 + 1]) and np.array_equal(z["hit"], hit[by0:by1 + 1, bx0:bx1 + 1])
    assert np.array_equal(z["classes"], want) and float(z["cell"]) == 0.5 and tuple(z["origin"]) == origin
    out = res.output
    g = re.search(r"sweeps: (\d+) \(skipped (\d+)\), rays (\d+) \(out of range (\d+), no return (\d+), ends outside the grid (\d+)\)", out)
    assert g and [int(v) for v in g.groups()] == [n[k] for k in ("n_scans", "n_scans_skipped", "n_rays", "n_rays_out_of_range", "n_no_return",
                                                                  "n_ends_outside")], out
    g = re.search(r"cells: crossed (\d+), hit (\d+), votes free (\d+), hit (\d+)", out)
    assert g and [int(v) for v in g.groups()] == [n[k] for k in ("n_cells_free", "n_cells_hit", "sum_free", "sum_hit")], out
    assert f"free {int((want == 0).sum())}, occupied {int((want == 1).sum())}, unknown {int((want == 2).sum())} of {want.size} cells read" in out
    assert f"grid: {nx} x {ny} cells of 0.5 m" in out and "Occupancy grid saved to:" in out


def test_ekf_bench_saves_the_grid_of_its_run(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    prefix = str(tmp_path / "run.png")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--synthetic-size", "32x256", "--end-scan", "2",
                                          "--use-imu-prediction", "--save-grid", prefix, "--grid-cell", "0.5", "--grid-max-range", "30"])
    assert res.exit_code == 0, res.output
    assert sorted(os.listdir(tmp_path)) == ["run.png", "run.yaml"]
    classes, cell, origin = pu.load_occupancy_map(prefix)
    assert cell == 0.5 and (classes == 0).sum() > 100 and (classes == 1).sum() > 10
    assert "sweeps: 3 (skipped 0)" in res.output and f"of {classes.size} cells read" in res.output
    assert "Map of scans" not in res.output, "the grid needs no map"
