"""The fly-by renderer and camera path, the parts that need no GPU: the C-ABI surface and its refusals before any HIP call,
the camera states against hand-derived answers, the numpy restatement the GPU tests compare with (tests/helpers/render_numpy.py) against a
brute-force per-pixel loop, the PNG writer, and the command's option handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib, fly
from ptudes_lab_amd import utils as pu
from tests.helpers import render_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")
NEW = {"ptl_render_sizeof_cfg", "ptl_render_default_cfg", "ptl_render_create", "ptl_render_destroy", "ptl_render_set_palette",
       "ptl_render_set_z_range", "ptl_render_set_overlay", "ptl_render_frames", "ptl_render_debug_set_early_reject"}
PTL_ERR_ARG = -1


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"#define[^\n]*", " ", src)
    return set(re.findall(r"^[ \t]*(?:const\s+)?[A-Za-z_]\w*[\s\*]+(ptl_\w+)\s*\(", src, flags=re.M))


def _exported(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("nm (binutils) is needed to list the library's exported symbols")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptl_") and " T " in ln}


def _lib_or_fail():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    return _lib.lib()


def _cam(view=None, fx=32.0, fy=32.0, cx=8.0, cy=6.0, near=0.5, far=100.0):
    c = _lib.RenderCam()
    c.view[:] = list(np.eye(4)[:3].reshape(12) if view is None else np.asarray(view, dtype=np.float64)[:3].reshape(12))
    c.fx, c.fy, c.cx, c.cy, c.near_m, c.far_m = fx, fy, cx, cy, near, far
    return c


# ---------------------------------------------------------------------------------------------- 1. surface and refusals
def test_surface_of_the_renderer():
    L = _lib_or_fail()
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= declared and NEW <= exported
    assert declared == exported, "the header declares exactly what the library exports"
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert set(_lib.PROTOTYPES) == declared
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION
    assert L.ptl_sizeof_cfg(6) == -1  # the new struct has a function of its own
    assert L.ptl_render_sizeof_cfg() == C.sizeof(_lib.RenderCfg) == 64
    assert C.sizeof(_lib.RenderCam) == 18 * 8
    from ptudes_lab_amd import core
    for name in ("set_palette", "set_overlay", "render", "close"):
        assert hasattr(core.Renderer, name)

    cfg = _lib.RenderCfg()
    assert L.ptl_render_default_cfg(C.byref(cfg), 96, 64) == 0
    assert (cfg.width, cfg.height, cfg.point_px, cfg.max_frames_per_call, cfg.z_lo, cfg.z_hi) == (96, 64, 2, 16, -2.0, 10.0)
    assert (cfg.background_rgba, cfg.edl_strength, cfg.edl_radius_px, cfg.struct_size, cfg.abi_version) == (0xFF000000, 0.0, 1, 64, 6)

    class Guarded(C.Structure):
        _fields_ = [("cfg", _lib.RenderCfg), ("canary", C.c_uint8 * 32)]

    for size, abi in ((56, 6), (64, 5), (72, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.cfg.struct_size, g.cfg.abi_version = size, abi
        before = bytes(g)
        rc = L.ptl_render_default_cfg(C.cast(C.byref(g), C.POINTER(_lib.RenderCfg)), 96, 64)
        msg = L.ptl_last_error().decode()
        assert rc == PTL_ERR_ARG and str(size) in msg and str(abi) in msg and "64" in msg, msg
        assert bytes(g) == before
    assert L.ptl_render_default_cfg(None, 96, 64) == PTL_ERR_ARG


def test_argument_refusals_fire_without_a_device():
    L = _lib_or_fail()
    h = C.c_void_p()

    def create(**over):
        cfg = _lib.RenderCfg()
        assert L.ptl_render_default_cfg(C.byref(cfg), 96, 64) == 0
        for k, v in over.items():
            setattr(cfg, k, v)
        rc = L.ptl_render_create(C.byref(cfg), 0, C.byref(h))
        return rc, L.ptl_last_error().decode()

    for px in (0, 6, -1):
        rc, msg = create(point_px=px)
        assert rc == PTL_ERR_ARG and "point_px" in msg and str(px) in msg, msg
    for lo, hi in ((1.0, 1.0), (2.5, -3.5)):
        rc, msg = create(z_lo=lo, z_hi=hi)
        assert rc == PTL_ERR_ARG and f"{lo:g}" in msg and f"{hi:g}" in msg, msg
    # 16384 x 16384 pixels x 8 bytes = 2 GiB for one frame: above the stated bound of 1 GiB
    rc, msg = create(width=16384, height=16384, max_frames_per_call=1)
    assert rc == PTL_ERR_ARG and str(16384 * 16384 * 8) in msg and str(1 << 30) in msg, msg
    rc, msg = create(width=1280, height=720, max_frames_per_call=1000)
    assert rc == PTL_ERR_ARG and str(1280 * 720 * 8 * 1000) in msg, msg
    rc, msg = create(width=0)
    assert rc == PTL_ERR_ARG and "width" in msg
    rc, msg = create(max_frames_per_call=0)
    assert rc == PTL_ERR_ARG and "max_frames_per_call" in msg
    assert not h.value

    frames = L.ptl_render_frames
    assert frames(None, None, None, -3, None, None, None, None, None) == PTL_ERR_ARG
    assert "-3" in L.ptl_last_error().decode()
    for near, far in ((0.0, 10.0), (-1.0, 10.0), (2.0, 2.0), (5.0, 1.5)):
        cams = (_lib.RenderCam * 2)(_cam(), _cam(near=near, far=far))
        assert frames(None, None, cams, 2, None, None, None, None, None) == PTL_ERR_ARG
        msg = L.ptl_last_error().decode()
        assert "camera 1" in msg and f"{near:g}" in msg and f"{far:g}" in msg, msg
    assert frames(None, None, (_lib.RenderCam * 1)(_cam()), 1, None, None, None, None, None) == PTL_ERR_ARG  # no renderer
    assert L.ptl_render_set_overlay(None, None, None, 4, 7) == PTL_ERR_ARG and "7" in L.ptl_last_error().decode()
    assert L.ptl_render_set_overlay(None, None, None, -1, 1) == PTL_ERR_ARG
    assert L.ptl_render_set_z_range(None, 3.0, 3.0) == PTL_ERR_ARG and "3" in L.ptl_last_error().decode()
    assert L.ptl_render_set_palette(None, None) == PTL_ERR_ARG
    assert L.ptl_render_destroy(None) == 0


# ---------------------------------------------------------------------------------------------- 2. the camera path
def test_view_distance_inverts_estimate_apex_dolly():
    for D in (20.0, 50.0, 333.0):
        # a box whose diagonal d gives 1.4142 d / sin(90 deg) = D
        d = D / 1.4142
        mm = np.array([[0.0, d], [0.0, 0.0], [0.0, 0.0]])
        dolly = pu.estimate_apex_dolly(mm, 90.0)
        assert np.isclose(dolly, 100.0 * np.log(D / 50.0), rtol=1e-14, atol=1e-12)
        assert np.isclose(fly.Camera(dolly=dolly).view_distance(), D, rtol=1e-13)
    c = fly.Camera()
    assert (c.yaw, c.pitch, c.dolly, c.fov) == (140.0, 0.0, -100.0, 90.0)
    assert np.isclose(c.view_distance(), 50.0 / np.e)


def test_estimate_apex_dolly_at_hand_computed_inputs():
    # diagonal of a 30 x 40 x 0 box = 50; fov 90: D = 1.4142 * 50 / 1 = 70.71, dolly = 100 ln(1.4142)
    mm = np.array([[-10.0, 20.0], [5.0, 45.0], [1.0, 1.0]])
    assert np.isclose(pu.estimate_apex_dolly(mm, 90.0), 100.0 * np.log(1.4142), rtol=1e-14)
    # fov 30: sin = 0.5, D doubles
    assert np.isclose(pu.estimate_apex_dolly(mm, 30.0), 100.0 * np.log(2 * 1.4142), rtol=1e-13)
    # the floor: an empty box gives D = 0 -> max(0.001, D) / 50 -> 100 ln(2e-5) = -1082 -> -100
    assert pu.estimate_apex_dolly(np.zeros((3, 2)), 90.0) == -100
    # D = 50 / e^1.5 is below the floor's D = 50 / e
    mm = np.array([[0.0, 50.0 / np.exp(1.5) / 1.4142], [0.0, 0.0], [0.0, 0.0]])
    assert pu.estimate_apex_dolly(mm, 90.0) == -100
    mm = np.array([[0.0, 50.0 / np.exp(0.5) / 1.4142], [0.0, 0.0], [0.0, 0.0]])
    assert np.isclose(pu.estimate_apex_dolly(mm, 90.0), -50.0, rtol=1e-13)


def _pose(x=0.0, y=0.0, z=0.0, yaw_deg=0.0):
    T = np.eye(4)
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [x, y, z]
    return T


def test_prune_trajectory_keeps_the_hand_derived_knots():
    # x positions and headings; from the last kept knot: > 5 m, or > 5 deg, or the last pose
    steps = [(0.0, 0.0),    # 0 kept: the first
             (2.0, 0.0),    # 1  2 m
             (4.9, 0.0),    # 2  4.9 m
             (5.1, 0.0),    # 3  5.1 m from knot 0: kept (the 5 m rule)
             (6.0, 3.0),    # 4  0.9 m, 3 deg
             (6.5, 5.5),    # 5  1.4 m, 5.5 deg from knot 3: kept (the 5 deg rule)
             (7.0, 9.0),    # 6  3.5 deg from knot 5
             (11.4, 9.0),   # 7  4.9 m from knot 5 (arc length of the log's translation part: a little above the chord, still < 5)
             (11.6, 9.0),   # 8  5.1 m from knot 5: kept
             (12.0, 9.0)]   # 9  the last pose: kept whatever its distance
    poses = [(10.0 + 0.1 * i, _pose(x=x, yaw_deg=a)) for i, (x, a) in enumerate(steps)]
    assert pu.prune_trajectory_indices(poses) == [0, 3, 5, 8, 9]
    pruned = pu.prune_trajectory(poses)
    assert [t for t, _ in pruned] == [0.5, 1.5, 2.5, 3.5, 4.5]
    for (_, p), i in zip(pruned, [0, 3, 5, 8, 9]):
        assert np.array_equal(p, poses[i][1])
    # a window: its own first and last
    assert pu.prune_trajectory_indices(poses, start_idx=1, end_idx=4) == [1, 4]
    # exactly 5 m is not "more than 5 m"
    assert pu.prune_trajectory_indices([(0.0, _pose()), (1.0, _pose(x=5.0)), (2.0, _pose(x=5.5)), (3.0, _pose(x=6.0))]) == [0, 2, 3]
    # one scan selected: the successor is added so that a trajectory evaluator has two knots; none to add: one knot
    assert pu.prune_trajectory_indices(poses, start_idx=4, end_idx=4) == [4, 5]
    assert pu.prune_trajectory_indices(poses[:1]) == [0]
    with pytest.raises(AssertionError):
        pu.prune_trajectory_indices(poses, start_idx=5, end_idx=4)


def test_log_and_exp_pose_are_inverse_and_ordered_rotation_first():
    rng = np.random.default_rng(5)
    for _ in range(20):
        xi = np.concatenate([rng.normal(0, 0.8, 3), rng.normal(0, 5.0, 3)])
        T = pu.exp_pose6(xi)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-13)
        assert np.allclose(pu.log_pose(T), xi, atol=1e-11)
    assert np.allclose(pu.log_pose(_pose(x=3.0)), [0, 0, 0, 3, 0, 0])
    assert np.allclose(pu.log_pose(_pose(yaw_deg=90.0)), [0, 0, np.pi / 2, 0, 0, 0])
    from scipy.linalg import expm
    xi = np.array([0.3, -0.2, 0.5, 1.0, 2.0, -3.0])
    A = np.zeros((4, 4))
    A[:3, :3] = pu.vee(xi[:3])
    A[:3, 3] = xi[3:]
    assert np.allclose(pu.exp_pose6(xi), expm(A), atol=1e-13)


def test_camera_transition_reaches_its_targets_and_hands_over():
    target_pose = _pose(x=12.0, y=-3.0, z=1.5, yaw_deg=40.0)
    cam = fly.Camera(target=np.linalg.inv(_pose(x=-4.0, y=2.0)), yaw=10.0, pitch=-30.0, dolly=20.0)
    st = fly.CameraTransitionState(name="T", target=target_pose, pitch=-70, dolly=-55, yaw=120, velocity=0.15,
                                   next_state=fly.FlyingState.COURSING)
    dt = 1.0 / 30.0
    steps = 0
    while True:
        t_before = st._t
        nxt = st.update(dt, cam)
        if nxt is not None:
            break
        steps += 1
        assert steps < 1000
    assert nxt == fly.FlyingState.COURSING
    assert t_before + 0.15 * dt >= 1.0 and t_before < 1.0
    assert steps == int(np.ceil(1.0 / (0.15 * dt))) - 1 == 199
    # every step covers dt / (1 - t) of what is left: after the last step 1 - t is left of a linear path, so the camera is within
    # (1 - t) of the whole way of its goal
    left = 1.0 - st._t
    assert 0.0 < left <= 0.15 * dt + 1e-12
    assert abs(cam.pitch - -70) <= left * 40 + 1e-9 and abs(cam.dolly - -55) <= left * 75 + 1e-9 and abs(cam.yaw - 120) <= left * 110 + 1e-9
    d = pu.log_pose(np.asarray(cam.target) @ target_pose)
    whole = pu.log_pose(np.linalg.inv(_pose(x=-4.0, y=2.0)) @ target_pose)
    assert np.linalg.norm(d) <= left * np.linalg.norm(whole) * (1 + 1e-6) + 1e-9
    # ... and in the limit of its last step (the step that takes t to 1) it is there exactly
    cam2 = fly.Camera(target=np.linalg.inv(_pose(x=-4.0, y=2.0)), yaw=10.0, pitch=-30.0, dolly=20.0)
    st2 = fly.CameraTransitionState(name="T", target=target_pose, pitch=-70, dolly=-55, yaw=120, velocity=1.0)
    assert st2.update(0.25, cam2) is None and st2.update(0.25, cam2) is None
    assert st2.update(0.5 - 1e-13, cam2) is None
    assert np.allclose(np.linalg.inv(cam2.target), target_pose, atol=1e-9)
    assert np.allclose([cam2.pitch, cam2.dolly, cam2.yaw], [-70, -55, 120], atol=1e-9)
    # only what is asked for moves
    cam3 = fly.Camera(yaw=10.0, pitch=-30.0, dolly=20.0)
    st3 = fly.CameraTransitionState(name="A", target=None, pitch=0, yaw=None, dolly=None, velocity=1.0)
    st3.update(0.5, cam3)
    assert (cam3.yaw, cam3.dolly, cam3.pitch) == (10.0, 20.0, -15.0) and np.array_equal(cam3.target, np.eye(4))


class _Eval:
    """a trajectory evaluator that records what it is asked"""

    def __init__(self, t0, t1):
        self.start_time, self.end_time, self.asked = t0, t1, []

    def pose_at(self, t):
        self.asked.append(t)
        return _pose(x=10.0 * t, yaw_deg=5.0 * t)


def test_coursing_slows_to_min_duration_and_visits_pose_at_its_times():
    ev = _Eval(0.5, 4.5)  # 4 units at velocity 5 would take 0.8 s: slowed to 4 / 3 per second
    st = fly.CoursingState(ev, velocity=5.0, min_duration=3.0, next_state=fly.FlyingState.TO_THE_APEX)
    assert np.isclose(st._v, 4.0 / 3.0)
    cam = fly.Camera()
    dt, n = 1.0 / 30.0, 0
    while st.update(dt, cam) is None:
        n += 1
        assert np.allclose(np.linalg.inv(cam.target), _pose(x=10.0 * ev.asked[-1], yaw_deg=5.0 * ev.asked[-1]), atol=1e-12)
        assert n < 1000
    assert st.update(dt, cam) == fly.FlyingState.TO_THE_APEX
    assert n in (89, 90) and len(ev.asked) == n  # 3 s at 30 frames per second (the last step may fall to rounding)
    assert np.allclose(ev.asked, 0.5 + (4.0 / 3.0) * dt * np.arange(n), atol=1e-12)
    assert ev.asked[-1] <= 4.5
    # a long trajectory keeps its velocity
    assert fly.CoursingState(_Eval(0.0, 100.0), velocity=5.0)._v == 5.0


def test_building_state_moves_target_and_eases_the_dolly():
    cam = fly.Camera()
    mm = np.zeros((3, 2))
    st = fly.BuildingState(min_max=mm, next_state=fly.FlyingState.TO_THE_BEGINNING)
    st.update_camera(cam, _pose(x=30.0, y=40.0, z=0.0, yaw_deg=77.0))
    # the target is the inverse of the pose with the identity for its rotation
    assert np.allclose(cam.target, np.linalg.inv(_pose(x=30.0, y=40.0)))
    assert np.array_equal(mm, [[0.0, 30.0], [0.0, 40.0], [0.0, 0.0]])
    want = 100.0 * np.log(1.4142 * 50.0 / 50.0)
    assert np.isclose(cam.dolly, -100.0 + 0.05 * (want + 100.0))
    assert st.update(1.0, cam) == fly.FlyingState.TO_THE_BEGINNING


def test_camera_looks_down_at_pitch_zero_and_along_the_horizon_at_minus_ninety():
    cam = fly.Camera(yaw=0.0, pitch=0.0, dolly=0.0)  # 50 m above the target
    c = cam.cam(96, 64)
    assert (c.cx, c.cy) == (48.0, 32.0) and np.isclose(c.fx, 32.0) and c.fx == c.fy  # fov 90: fy = (H / 2) / tan(45 deg)
    V = np.array(c.view[:]).reshape(3, 4)
    assert np.allclose(V @ [0, 0, 0, 1], [0, 0, 50.0])      # the target's origin: straight ahead at the view distance
    assert np.allclose(V @ [0, 0, 10, 1], [0, 0, 40.0])     # higher is closer
    assert np.allclose(V @ [1, 0, 0, 1], [1, 0, 50.0])
    cam.pitch = -90.0
    V = cam.view_matrix()
    assert np.allclose(V @ [0, 0, 1, 1], [0, -1, 50.0, 1])  # up in the world is up in the image (-y)
    cam.target = np.linalg.inv(_pose(x=5.0, y=6.0, z=7.0))
    assert np.allclose(cam.view_matrix() @ [5, 6, 7, 1], [0, 0, 50.0, 1])


# ---------------------------------------------------------------------------------------------- 3. the restatement
def _brute(points, words, px, cam, W, H):
    """one pixel at a time, one point at a time, python floats: the definition read literally"""
    import math
    keys = [[0xFFFFFFFFFFFFFFFF] * W for _ in range(H)]
    v = list(cam.view[:])
    in_view = 0
    for (x, y, z), word in zip(points.tolist(), words.tolist()):
        xc = ((v[0] * x + v[1] * y) + v[2] * z) + v[3]
        yc = ((v[4] * x + v[5] * y) + v[6] * z) + v[7]
        zc = ((v[8] * x + v[9] * y) + v[10] * z) + v[11]
        if not (zc > cam.near_m) or zc >= cam.far_m:
            continue
        u, w = cam.fx * (xc / zc) + cam.cx, cam.fy * (yc / zc) + cam.cy
        col, row = math.floor(u), math.floor(w)
        key = (int(np.float32(zc).view(np.uint32)) << 32) | int(word)
        hit = False
        for py in range(H):
            for pxl in range(W):
                if row - (px - 1) // 2 <= py < row - (px - 1) // 2 + px and col - (px - 1) // 2 <= pxl < col - (px - 1) // 2 + px:
                    hit = True
                    keys[py][pxl] = min(keys[py][pxl], key)
        in_view += hit
    return np.array(keys, dtype=np.uint64), in_view


def test_restatement_agrees_with_a_per_pixel_loop():
    rng = np.random.default_rng(11)
    W, H = 16, 12
    pts = np.concatenate([rng.uniform(-3, 3, (150, 3)) + [0, 0, 4.0],
                          [[-0.125, 0.0, 2.0], [-0.25, -0.1875, 1.0], [0.25, 0.0, 0.5], [0.0, 0.0, -1.0], [1e300, 0.0, 1.0], [1.0, 1.0, 1e-300]]])
    pal = rn.default_palette_words()
    words = pal[rn.palette_index(pts[:, 2], -2.0, 10.0)]
    for px in (1, 2, 3, 5):
        for cam in (_cam(), _cam(view=_pose(x=0.5, yaw_deg=20.0), near=1.0, far=6.0)):
            keys = np.full((H, W), rn.EMPTY, dtype=np.uint64)
            n = rn.splat_into(keys, pts, words, px, cam)
            want, n_want = _brute(pts, words, px, cam, W, H)
            assert np.array_equal(keys, want) and n == n_want and n > 0
    # floor, not truncation: with the principal point at 0 the point (-1/64, 0, 1) projects to u = 32 * -1/64 = -0.5
    cam = _cam(cx=0.0, cy=0.0)
    keys = np.full((H, W), rn.EMPTY, dtype=np.uint64)
    assert rn.splat_into(keys, np.array([[-0.015625, 0.0, 1.0]]), pal[:1], 1, cam) == 0  # u = -0.5: column -1, not column 0
    assert (keys == rn.EMPTY).all()
    # resolve: background, colours, depth; EDL leaves an isolated pixel and a flat patch alone and darkens a pixel behind its neighbours
    keys = np.full((H, W), rn.EMPTY, dtype=np.uint64)
    near_key = (np.uint64(np.float32(2.0).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFF6496C8)
    far_key = (np.uint64(np.float32(8.0).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFF6496C8)
    keys[2, 2] = near_key
    keys[6, 5:8] = near_key
    keys[6, 6] = far_key
    rgba, depth = rn.resolve(keys, 0xFF102030)
    assert tuple(rgba[0, 0]) == (0x30, 0x20, 0x10, 0xFF) and tuple(rgba[2, 2]) == (0xC8, 0x96, 0x64, 0xFF)
    assert depth[2, 2] == 2.0 and np.isinf(depth[0, 0]) and depth[6, 6] == 8.0
    shaded, depth2 = rn.resolve(keys, 0xFF102030, edl_strength=0.5, edl_radius=1)
    assert np.array_equal(depth2, depth)
    assert tuple(shaded[2, 2]) == (0xC8, 0x96, 0x64, 0xFF) and tuple(shaded[0, 0]) == (0x30, 0x20, 0x10, 0xFF)
    # the far pixel: two neighbours (left, right) at log2 8 - log2 2 = 2 each, mean 2, s = exp(-1)
    s = np.exp(-1.0)
    assert tuple(shaded[6, 6]) == (int(np.floor(0xC8 * s + 0.5)), int(np.floor(0x96 * s + 0.5)), int(np.floor(0x64 * s + 0.5)), 0xFF)
    # its neighbours see it behind them: negative, clipped to 0, unshaded
    assert tuple(shaded[6, 5]) == (0xC8, 0x96, 0x64, 0xFF)


# ---------------------------------------------------------------------------------------------- 4. PNG
def test_png_round_trip_bit_for_bit(tmp_path):
    import struct
    import zlib
    rng = np.random.default_rng(2)
    for shape in ((64, 96, 4), (1, 1, 4), (7, 3, 4)):
        frame = rng.integers(0, 256, shape, dtype=np.uint8)
        p = str(tmp_path / f"f{shape[0]}.png")
        pu.save_png(p, frame)
        back = pu.load_png(p)
        assert back.dtype == np.uint8 and back.shape == frame.shape and back.tobytes() == frame.tobytes()
    raw = open(p, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR"
    assert struct.unpack(">IIBBBBB", raw[16:29]) == (3, 7, 8, 6, 0, 0, 0)  # 8-bit RGBA, no interlace
    n = struct.unpack(">I", raw[33:37])[0]
    assert raw[37:41] == b"IDAT"
    lines = np.frombuffer(zlib.decompress(raw[41:41 + n]), dtype=np.uint8).reshape(7, 1 + 12)
    assert not lines[:, 0].any() and lines[:, 1:].tobytes() == frame.tobytes()  # filter 0 on every line
    assert raw[-12:] == b"\x00\x00\x00\x00IEND\xaeB`\x82"
    with pytest.raises(ValueError):
        pu.save_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), dtype=np.uint8))
    (tmp_path / "not.png").write_bytes(b"hello")
    with pytest.raises(ValueError):
        pu.load_png(str(tmp_path / "not.png"))
    # no imaging package is imported
    src =open(os.path.join(ROOT, "ptudes-lab_amd", "utils.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(PIL|imageio|cv2|matplotlib|png)\b", src, flags=re.M)


# ---------------------------------------------------------------------------------------------- 5. option handling
def test_flyby_refuses_frame_options_before_any_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    r = run(ptudes_cli, ["flyby", "--help"])
    assert r.exit_code == 0
    for opt in ("--save-frames", "--frame-size", "--fps", "--max-frames", "--point-size", "--edl", "--z-range"):
        assert opt in r.output, opt
    poses = tmp_path / "p.csv"
    poses.write_text("")
    base = ["flyby", "--synthetic", "1", "--nc-gt-poses", str(poses)]
    for opt, val in (("--frame-size", "96x64"), ("--fps", "25"), ("--max-frames", "5"), ("--point-size", "3"), ("--edl", "0.5"),
                     ("--z-range", "-2,10")):
        r = run(ptudes_cli, base + [opt, val])
        assert r.exit_code != 0 and f"{opt} belongs to --save-frames" in r.output, (opt, r.output)
    out = str(tmp_path / "frames")
    for bad in ("96", "96x", "x64", "96*64", "0x64", "96x64x3", "-96x64", "99999x64"):
        r = run(ptudes_cli, base + ["--save-frames", out, "--frame-size", bad])
        assert r.exit_code != 0 and "--frame-size" in r.output and "WxH" in r.output, (bad, r.output)
    r = run(ptudes_cli, base + ["--save-frames", out, "--point-size", "6"])
    assert r.exit_code != 0 and "--point-size 6" in r.output
    r = run(ptudes_cli, base + ["--save-frames", out, "--z-range", "3,1"])
    assert r.exit_code != 0 and "--z-range" in r.output
    r = run(ptudes_cli, base + ["--save-frames", out, "--z-range", "abc"])
    assert r.exit_code != 0 and "LO,HI" in r.output
    r = run(ptudes_cli, base + ["--save-frames", out, "--fps", "0"])
    assert r.exit_code != 0 and "--fps" in r.output
    assert not os.path.exists(out)
