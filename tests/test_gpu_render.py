"""The fly-by renderer on the device against its numpy restatement (tests/helpers/render_numpy.py), bit for bit: the keys
are minima over exactly rounded fp64 expressions in a fixed order, so there is nothing to tolerate - except the eye-dome shade, which goes
through log2 / exp (one 8-bit level).  Frames are 96 x 64, maps are built with Icp.map_add at voxel size 0.5."""
import os

import numpy as np
import pytest

from tests.helpers import render_numpy as rn

pytestmark = pytest.mark.gpu

W, H = 96, 64
CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
Z_RANGE = (-1.0, 4.0)
BOUNDS = 1.5


def _map(points=None, **kw):
    from ptudes_lab_amd import core
    m = core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=64, max_points_per_scan=8192, **{**CAPS, **kw})
    if points is not None and len(points):
        m.map_add(points)
    return m


def _sorted(p):
    return np.ascontiguousarray(p[np.lexsort(p.T[::-1])])


def _renderer(**kw):
    from ptudes_lab_amd import core
    kw.setdefault("z_range", Z_RANGE)
    return core.Renderer(W, H, **kw)


def _look(eye, forward, down, fx=40.0, fy=40.0, cx=W / 2.0, cy=H / 2.0, near=0.25, far=60.0):
    """camera at `eye` looking along `forward` with image-down along `down` (orthonormalised)"""
    from ptudes_lab_amd import _lib
    f = np.asarray(forward, dtype=np.float64)
    f = f / np.linalg.norm(f)
    d = np.asarray(down, dtype=np.float64)
    d = d - f * (d @ f)
    d = d / np.linalg.norm(d)
    r = np.cross(d, f)
    R = np.stack([r, d, f])
    c = _lib.RenderCam()
    c.view[:] = list(np.concatenate([R, (-R @ np.asarray(eye, dtype=np.float64))[:, None]], axis=1).reshape(12))
    c.fx, c.fy, c.cx, c.cy, c.near_m, c.far_m = fx, fy, cx, cy, near, far
    return c


def _identity_cam(near=0.5, far=64.0):
    from ptudes_lab_amd import _lib
    c = _lib.RenderCam()
    c.view[:] = list(np.eye(4)[:3].reshape(12))
    c.fx, c.fy, c.cx, c.cy, c.near_m, c.far_m = 32.0, 32.0, W / 2.0, H / 2.0, near, far
    return c


def _room():
    """three planes of a 10 x 8 x 3 room and scattered points: about 3 000"""
    rng = np.random.default_rng(7)
    floor = np.column_stack([rng.uniform(0, 10, 1000), rng.uniform(0, 8, 1000), rng.normal(0.0, 0.004, 1000)])
    wall_x = np.column_stack([10.0 + rng.normal(0.0, 0.004, 800), rng.uniform(0, 8, 800), rng.uniform(0, 3, 800)])
    wall_y = np.column_stack([rng.uniform(0, 10, 800), 8.0 + rng.normal(0.0, 0.004, 800), rng.uniform(0, 3, 800)])
    loose = rng.uniform([0.5, 0.5, 0.2], [9.5, 7.5, 2.8], (400, 3))
    return np.concatenate([floor, wall_x, wall_y, loose])


def _cams8():
    eye = [5.0, 4.0, 1.5]
    up = [0, 0, -1]
    return [_look(eye, [1, 0, 0], up), _look(eye, [-1, 0, 0], up), _look(eye, [0, 1, 0], up), _look(eye, [0, -1, 0], up),
            _look(eye, [0, 0, 1], [0, 1, 0]), _look(eye, [0, 0, -1], [0, -1, 0]),
            _look([1.0, 1.0, 2.7], [1.0, 0.8, -0.35], up),                        # oblique
            _look([5.0, 4.0, 40.0], [0, 0, -1], [0, -1, 0], near=1.0, far=100.0)]  # the apex: the whole room in a few dozen pixels


@pytest.fixture(scope="module")
def room():
    m = _map(_room())
    stored = m.map_points().copy()
    assert 2500 < len(stored) <= 3000
    yield m, stored
    m.close()


def _same(got, want, what=""):
    rgba, depth, keys, in_view = got
    wkeys, wrgba, wdepth, win = want
    assert np.array_equal(keys, wkeys), f"{what}: {int((keys != wkeys).sum())} keys differ"
    assert np.array_equal(in_view, win), (what, in_view, win)
    assert rgba.tobytes() == wrgba.tobytes(), what
    assert depth.tobytes() == wdepth.tobytes(), what


# ---------------------------------------------------------------------------------------------- 1. exact frame
@pytest.mark.parametrize("px", [1, 2, 3])
def test_exact_frames_of_a_room(room, px):
    m, stored = room
    cams = _cams8()
    r = _renderer(point_px=px)
    got = r.render(m, cams, depth=True, keys=True)
    want = rn.render(stored, cams, W, H, point_px=px, z_range=Z_RANGE)
    _same(got, want, f"point_px {px}")
    assert (got[3] > 0).all() and got[3].sum() > 5000 and (got[2] != rn.EMPTY).sum() > 1000  # the frames are not empty
    assert got[0].shape == (8, H, W, 4) and got[0].dtype == np.uint8
    r.close()


# ---------------------------------------------------------------------------------------------- 2. edges on a dyadic scene
def _dyadic_points():
    """camera at the identity, fx = fy = 32, principal point (48, 32): u = 32 x / z + 48, v = 32 y / z + 32; depths are powers of two"""
    def at(u, v, z):
        return [(u - 48.0) / 32.0 * z, (v - 32.0) / 32.0 * z, z]
    pts = []
    for z in (1.0, 2.0, 4.0, 8.0):
        pts += [at(56.0, 20.0, z),                 # u exactly an integer
                at(96.0, 10.0 + z, z),             # u exactly the width: column 96, outside for 1 pixel, straddles the right edge for 3
                at(-0.5, 12.0 + z, z),             # u in (-1, 0): column -1 (floor), not column 0 (truncation)
                at(0.25, 30.0 + z, z),             # column 0
                at(95.5, 40.0 + z, z),             # column width - 1
                at(30.0 + z, -0.5, z), at(40.0 + z, 0.0, z), at(50.0 + z, 63.75, z), at(60.0 + z, 64.0, z),  # the rows likewise
                at(0.0, 0.0, z), at(95.0, 63.0, z), at(-1.0, -1.0, z), at(96.0, 64.0, z), at(95.0, 0.0, z), at(0.0, 63.0, z)]  # the corners
    pts += [[0.25, 0.25, 0.5],                                   # zc == near: rejected
            [0.25, -0.25, float(np.nextafter(0.5, 1.0))],        # just beyond it: drawn
            [-0.5, 0.5, 64.0],                                   # zc == far: rejected
            [0.5, -0.5, float(np.nextafter(64.0, 0.0))],         # just inside: drawn
            [0.125, 0.125, -1.0], [0.0, 0.25, -8.0],             # behind the camera
            [1.0, 0.5, 2.0 ** -900], [-1.0, 0.25, 2.0 ** -800],  # x / zc = 2^900: beyond every pixel index (drawn by the tiny-near camera only if mishandled)
            [0.0, 0.0, 2.0 ** -700]]                             # ... and one on the axis: u = 48 exactly, however small zc
    return np.array(pts, dtype=np.float64)


@pytest.mark.parametrize("px", [1, 2, 3, 5])
def test_edges_on_a_dyadic_scene(px):
    pts = _dyadic_points()
    m = _map(pts)
    stored = m.map_points()
    o = np.lexsort(stored.T[::-1])
    assert np.array_equal(stored[o], pts[np.lexsort(pts.T[::-1])]), "every point is stored: the edge cases are all in the map"
    cams = [_identity_cam(), _identity_cam(near=2.0 ** -1000, far=64.0)]
    r = _renderer(point_px=px, z_range=(0.0, 16.0))
    got = r.render(m, cams, depth=True, keys=True)
    want = rn.render(stored, cams, W, H, point_px=px, z_range=(0.0, 16.0))
    _same(got, want, f"point_px {px}")
    keys = got[2]
    if px == 1:
        assert keys[0, 20, 56] != rn.EMPTY and (keys[0, :, 0] != rn.EMPTY).sum() >= 4  # the integer u; column 0 is hit
        assert (keys[0, 11:21, 0] == rn.EMPTY).all()  # u = -0.5 did not land in column 0 (rows 13 .. 20)
        assert keys[1, 32, 48] != rn.EMPTY             # the tiny-near camera draws the point on its axis
    m.close()
    r.close()


# ---------------------------------------------------------------------------------------------- 3. ties
def test_ties_resolve_to_the_smaller_word():
    # camera looking along +x: depth = x.  Two points 0.05 apart in height whose 2-pixel footprints share row 31, at depths that round to
    # the same float32; the palette over (0, 0.2) gives them different colours
    a, b = [4.0, 0.0, 0.1], [4.0 + 1e-9, 0.0, 0.15]
    assert np.float32(a[0]) == np.float32(b[0])
    cam = _look([0, 0, 0], [1, 0, 0], [0, 0, -1], fx=32.0, fy=32.0)
    pal = rn.default_palette_words()
    wa, wb = (int(pal[rn.palette_index(p[2], 0.0, 0.2)]) for p in (a, b))
    assert wa != wb
    frames = []
    for first, second in ((a, b), (b, a)):
        m = _map(np.array([first]))
        m.map_add(np.array([second]))
        r = _renderer(point_px=2, z_range=(0.0, 0.2))
        got = r.render(m, [cam], depth=True, keys=True)
        _same(got, rn.render(m.map_points(), [cam], W, H, point_px=2, z_range=(0.0, 0.2)))
        keys = got[2][0]
        shared = (int(np.float32(4.0).view(np.uint32)) << 32) | min(wa, wb)
        rows = np.flatnonzero((keys != rn.EMPTY).any(axis=1))
        assert list(rows) == [30, 31, 32] and int(keys[31, 48]) == shared, "the shared row holds the smaller word"
        frames.append(keys)
        m.close()
        r.close()
    assert np.array_equal(frames[0], frames[1])
    # the farther point closer by one float32 step wins whatever its colour
    c = [float(np.nextafter(np.float32(4.0), np.float32(0.0))), 0.0, 0.15]
    m = _map(np.array([a, c]))
    r = _renderer(point_px=2, z_range=(0.0, 0.2))
    keys = r.render(m, [cam], keys=True)[1][0]
    assert int(keys[31, 48]) == (int(np.float32(c[0]).view(np.uint32)) << 32) | wb
    m.close()
    r.close()


# ---------------------------------------------------------------------------------------------- 4. order independence
def test_frames_do_not_depend_on_the_order_of_the_points(room):
    _, stored = room
    # (the stored points of the room: at most 20 per voxel by construction, so no voxel overflows whatever the order)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(stored))
    a, b = _map(stored), _map(stored[order])
    pa, pb = a.map_points(), b.map_points()
    assert len(pa) == len(pb) == len(stored)
    assert np.array_equal(pa[np.lexsort(pa.T[::-1])], pb[np.lexsort(pb.T[::-1])]), "both maps store the same set"
    # (map_points() comes in the order the export's atomics land; the map score lists the points in pool order: block id, then slot)
    assert not np.array_equal(a.map_score(per_point=True)[1][0], b.map_score(per_point=True)[1][0]), "... in different pool order"
    cams = _cams8()
    r = _renderer(point_px=3)
    fa, fb = r.render(a, cams, depth=True, keys=True), r.render(b, cams, depth=True, keys=True)
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes()
    for h in (a, b, r):
        h.close()


# ---------------------------------------------------------------------------------------------- 5. batching
def test_batches_and_repeats_give_identical_output(room):
    m, stored = room
    cams = _cams8()[:5]
    outs = []
    for per_call in (1, 2, 8):
        r = _renderer(point_px=2, max_frames_per_call=per_call)
        r.set_overlay(np.array([[5.0, 4.0, 1.0], [6.0, 4.0, 1.0]]), (255, 0, 255, 255), 3)
        outs.append(r.render(m, cams, depth=True, keys=True))
        again = r.render(m, cams, depth=True, keys=True)
        for x, y in zip(outs[-1], again):
            assert x.tobytes() == y.tobytes(), f"rendering twice, {per_call} frames per call"
        r.close()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert x.tobytes() == y.tobytes()
    assert len(outs[0][0]) == 5
    r = _renderer()
    empty = r.render(m, [])
    assert empty[0].shape == (0, H, W, 4) and len(empty[1]) == 0
    r.close()


# ---------------------------------------------------------------------------------------------- 6. overlay
def test_overlay_alone_over_a_map_and_cleared():
    cam = _identity_cam()
    ov_xyz = np.array([[0.0, 0.0, 2.0], [0.5, 0.25, 4.0], [0.0, 0.0, 8.0], [-0.5, -0.5, 1.0]])
    ov_rgba = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [9, 8, 7, 6]], dtype=np.uint8)
    ov = (ov_xyz, rn.rgba_words(ov_rgba), 3)
    r = _renderer(point_px=1)
    r.set_overlay(ov_xyz, ov_rgba, 3)
    _same(r.render(None, [cam], depth=True, keys=True), rn.render(None, [cam], W, H, point_px=1, z_range=Z_RANGE, overlay=ov), "overlay alone")
    # a map point on the axis at depth 4: the overlay's point at depth 2 is in front of it, its point at depth 8 behind it
    pts = np.array([[0.0, 0.0, 4.0], [1.0, 0.5, 8.0], [-1.0, 0.5, 2.0]])
    m = _map(pts)
    got = r.render(m, [cam], depth=True, keys=True)
    _same(got, rn.render(m.map_points(), [cam], W, H, point_px=1, z_range=Z_RANGE, overlay=ov), "overlay over a map")
    assert tuple(got[0][0, 32, 48]) == (255, 0, 0, 255) and got[1][0, 32, 48] == 2.0  # in front: the overlay's colour as given
    assert got[3][0] == 3 + 4
    r.set_overlay(ov_xyz[2:3], ov_rgba[2:3], 3)  # only the point behind the map point
    got = r.render(m, [cam], depth=True, keys=True)
    _same(got, rn.render(m.map_points(), [cam], W, H, point_px=1, z_range=Z_RANGE, overlay=(ov_xyz[2:3], ov[1][2:3], 3)), "overlay behind")
    assert got[1][0, 32, 48] == 4.0 and got[1][0, 31, 48] == 8.0  # the map point's pixel; beside it the overlay's footprint shows
    r.set_overlay(np.zeros((0, 3)))
    _same(r.render(m, [cam], depth=True, keys=True), rn.render(m.map_points(), [cam], W, H, point_px=1, z_range=Z_RANGE), "overlay cleared")
    with pytest.raises(ValueError, match="point_px"):
        r.set_overlay(ov_xyz, ov_rgba, 6)
    m.close()
    r.close()


# ---------------------------------------------------------------------------------------------- 7. empty map
def test_an_empty_map_gives_background_and_zero_counts():
    m = _map()
    r = _renderer(background=(10, 20, 30, 255))
    rgba, depth, keys, in_view = r.render(m, _cams8()[:3], depth=True, keys=True)
    assert (keys == rn.EMPTY).all() and np.isinf(depth).all() and (in_view == 0).all()
    assert (rgba.reshape(-1, 4) == [10, 20, 30, 255]).all()
    rgba2, in_view2 = r.render(None, _cams8()[:1])
    assert (rgba2.reshape(-1, 4) == [10, 20, 30, 255]).all() and in_view2[0] == 0
    m.close()
    r.close()


# ---------------------------------------------------------------------------------------------- 8. eye-dome lighting
def test_eye_dome_lighting_within_one_level(room):
    m, stored = room
    cams = _cams8()
    for radius in (1, 2):
        r = _renderer(point_px=2, edl=0.7, edl_radius_px=radius)
        rgba, depth, keys, in_view = r.render(m, cams, depth=True, keys=True)
        wkeys, wrgba, wdepth, win = rn.render(stored, cams, W, H, point_px=2, z_range=Z_RANGE, edl_strength=0.7, edl_radius=radius)
        assert np.array_equal(keys, wkeys) and depth.tobytes() == wdepth.tobytes() and np.array_equal(in_view, win)
        diff = np.abs(rgba.astype(np.int16) - wrgba.astype(np.int16))
        share = float((diff.max(axis=3) > 0).mean())
        print(f"edl radius {radius}: {share:.6f} of the pixels differ from the restatement, by at most {int(diff.max())} level(s)")
        assert diff.max() <= 1
        assert np.array_equal(rgba[..., 3], wrgba[..., 3])
        plain = rn.render(stored, cams, W, H, point_px=2, z_range=Z_RANGE)[1]
        assert (rgba[..., :3].astype(np.int16) <= plain[..., :3].astype(np.int16) + 1).all() and (rgba != plain).any()  # it only darkens, and does
        r.close()


# ---------------------------------------------------------------------------------------------- 9. the map is only read
def test_the_map_is_not_written():
    from ptudes_lab_amd import core, synth
    seq = synth.make_sequence(seed=31, n_scans=3, H=32, W=256)
    cams = _cams8()
    poses = []
    for with_render in (False, True):
        icp = core.Icp(70.0, 1.0, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 16, map_table_capacity=1 << 18)
        r = _renderer(point_px=3, edl=0.5)
        out = []
        for k in range(3):
            out.append(icp.register_frame(seq.scan(k)).copy())
            if with_render:
                before_pts, before_size = _sorted(icp.map_points()), icp.map_size()
                f1 = r.render(icp, cams, depth=True, keys=True)
                # (the export hands the blocks out in the order its atomics land: the comparison is of the sorted points)
                assert icp.map_size() == before_size and _sorted(icp.map_points()).tobytes() == before_pts.tobytes()
                assert np.array_equal(f1[2], rn.render(before_pts, cams, W, H, point_px=3, z_range=Z_RANGE)[0])  # and it drew that map
        poses.append(np.array(out))
        icp.close()
        r.close()
    assert poses[0].tobytes() == poses[1].tobytes(), "a registration continued after a render gives the pose of one without"


# ---------------------------------------------------------------------------------------------- 10. the command
def test_flyby_writes_the_frames_of_the_camera_path(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd import core, fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    n = 6
    seq = synth.make_sequence(seed=1000, n_scans=n)
    p, out = str(tmp_path / "p.csv"), str(tmp_path / "frames")
    pu.save_poses_nc_gt_format(p, t=list(seq.t_base + (np.arange(n) + 0.5) * seq.scan_dt), poses=list(seq.gt_poses()))
    base = ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "5"]
    res = CliRunner().invoke(ptudes_cli, base + ["--save-frames", out, "--frame-size", "96x64", "--max-frames", "40"])
    assert res.exit_code == 0, res.output
    files = sorted(os.listdir(out))

    # the same run in-process
    rows = pu.read_newer_college_gt(p)
    pose0_inv = np.linalg.inv(rows[0][1])
    shifted = [(t, pose0_inv @ q) for t, q in rows]
    lut, scans = fly.synthetic_range_scans(seq, 0, 5)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    r = core.Renderer(W, H, point_px=2)
    states = []
    fb = fly.FlyBy(acc, r, shifted, fps=30, rate=1.0, time_bounds=BOUNDS, max_frames=40, on_state=states.append)
    mine = list(fb.frames(scans))
    assert len(mine) == 40 and files == [f"frame_{i:06d}.png" for i in range(len(mine))]
    assert [s for s, _ in mine] == ["BUILDING"] * 6 + ["TO_THE_BEGINNING"] * 34 and states == ["BUILDING", "TO_THE_BEGINNING"]
    for i in (0, 5, 6, 39):
        assert pu.load_png(os.path.join(out, files[i])).tobytes() == mine[i][1].tobytes(), f"frame {i}"
    assert (mine[5][1][..., :3] != 0).any() and (mine[39][1][..., :3] != 0).any()
    for line in ("map of scans: 0 - 5", "state: BUILDING", "state: TO..THE..BEGINNING", "playback: 1.0", f"map num points: {acc.map_size()[1]}",
                 "40 frames (96x64) saved to"):
        assert line in res.output, (line, res.output)
    assert res.output.count("state: ") == 2 and "NOTE: -r" not in res.output
    acc.close()
    r.close()

    # frame 0 = the one-scan map through the camera of the first BUILDING step, drawn directly
    acc1 = fly.MapAccumulator(lut, voxel_size=0.5)
    traj = core.Traj([t for t, _ in shifted], [q for _, q in shifted], BOUNDS, BOUNDS)
    acc1.update(scans[0], traj=traj)
    ts = np.asarray(scans[0].timestamp, dtype=np.float64) * 1e-9
    ends = pu.TrajectoryEvaluator(shifted, time_bounds=BOUNDS).poses_at([ts[0], ts[-1]])
    cam = fly.Camera()
    fly.BuildingState().update_camera(cam, ends[0])
    h = float(ends[0][2, 3])
    r1 = core.Renderer(W, H, point_px=2, z_range=(h - fly.BUILDING_Z_SPAN, h + fly.BUILDING_Z_SPAN))
    r1.set_overlay(ends[1][:3, 3].reshape(1, 3), fly.TRACK_RGBA, 3)
    frame0, in_view = r1.render(acc1.icp, [cam.cam(W, H)])
    assert frame0[0].tobytes() == pu.load_png(os.path.join(out, files[0])).tobytes() and in_view[0] > 1000
    want = rn.render(acc1.map_points(), [cam.cam(W, H)], W, H, point_px=2, z_range=(h - 10.0, h + 10.0),
                     overlay=(ends[1][:3, 3].reshape(1, 3), rn.rgba_words(np.array([fly.TRACK_RGBA], dtype=np.uint8)), 3))
    assert frame0.tobytes() == want[1].tobytes()
    for hnd in (acc1, traj, r1):
        hnd.close()

    # without --save-frames the command prints what it always printed
    res2 = CliRunner().invoke(ptudes_cli, base)
    assert res2.exit_code == 0, res2.output
    lines = res2.output.strip().split("\n")
    assert len(lines) == 4 and lines[0].startswith("NOTE: Therere where 0 skipped scans") and lines[1] == "map of scans: 0 - 5"
    assert lines[2].startswith("map num points: ") and lines[3].startswith("map voxels: ") and lines[3].endswith("(voxel size 0.5)")
    assert lines[2] in res.output and lines[3] in res.output  # the same map either way
    # -r scales the time step with --save-frames (twice the rate: half the frames of a transition) and its NOTE is not printed
    out2 = str(tmp_path / "frames2")
    res3 = CliRunner().invoke(ptudes_cli, base + ["--save-frames", out2, "--frame-size", "96x64", "-r", "2.0", "--max-frames", "120"])
    assert res3.exit_code == 0 and "NOTE: -r" not in res3.output and "playback: 2.0" in res3.output, res3.output
    assert "state: COURSING" in res3.output and len(os.listdir(out2)) == 120  # 6 + 99 of the transition, then coursing
