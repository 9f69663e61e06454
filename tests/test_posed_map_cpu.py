"""Posed scans into the world map, the parts that need no GPU: the C-ABI surface, the trajectory's validation (before any
HIP call), the numpy definition the GPU tests compare with (tests/helpers/posed_map_numpy.py) on known answers, the map files, and the
commands' option handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import expm
from scipy.spatial.transform import Rotation as Rot

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from ptudes_lab_amd import utils as pu
from tests.helpers import posed_map_numpy as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")
NEW = {"ptl_traj_create", "ptl_traj_destroy", "ptl_icp_map_add_posed_range", "ptl_icp_map_add_posed_xyz", "ptl_seq_map_build",
       "ptl_batch_map_build"}
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


def test_new_entry_points_are_exported_declared_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= exported, "not exported"
    assert declared == exported, "the header declares exactly what the library exports"
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert set(_lib.PROTOTYPES) == declared
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points change no struct or prototype
    from ptudes_lab_amd import core, fly
    assert all(hasattr(core, n) for n in ("Traj",)) and hasattr(core.Icp, "map_add_posed")
    assert hasattr(core.SeqRunner, "build_map") and hasattr(core.BatchRunner, "build_map") and hasattr(fly.MapAccumulator, "add_run")


def _traj_create(kt, kp):
    h = C.c_void_p()
    kt, kp = _lib.as_f64(kt), _lib.as_f64(kp).reshape(-1, 16)
    rc = _lib.lib().ptl_traj_create(0, _lib.dptr(kt), _lib.dptr(kp), len(kt), 1.5, 1.5, C.byref(h))
    return rc, _lib.lib().ptl_last_error().decode(), h


def test_traj_create_validates_before_any_device_call():
    eye = np.eye(4)
    rc, msg, h = _traj_create([10.0], [eye])
    assert rc == PTL_ERR_ARG and not h.value and ">= 2 knots" in msg and "knot 1" in msg
    rc, msg, h = _traj_create([10.0, 10.5, 10.5, 11.0], [eye] * 4)
    assert rc == PTL_ERR_ARG and not h.value and "knot 2" in msg
    rc, msg, h = _traj_create([10.0, 10.5, 10.4], [eye] * 3)
    assert rc == PTL_ERR_ARG and "knot 2" in msg
    from ptudes_lab_amd import core
    with pytest.raises(ValueError, match="knot 1"):
        core.Traj([3.0], [eye])


def _pose(rv, t):
    T = np.eye(4)
    T[:3, :3] = Rot.from_rotvec(rv).as_matrix()
    T[:3, 3] = t
    return T


def test_definition_motionless_sensor_is_the_plain_transform():
    rng = np.random.default_rng(2)
    H, W = 5, 12
    xyz = rng.normal(0, 8, (H, W, 3))
    xyz[1, 3] = 0.0  # no return
    xyz[4, 11] = 0.0
    T = _pose([0.3, -0.2, 0.9], [4.0, -2.0, 0.7])
    knots = [(100.0 + 0.1 * i, T) for i in range(5)]
    got = pm.posed_points(xyz, pm.sweep_column_times(100.05, 100.15, W), knots)
    keep = np.any(xyz != 0, axis=2)
    ref = xyz[keep] @ T[:3, :3].T + T[:3, 3]  # row-major pixel order, returns only
    assert got.shape == (H * W - 2, 3) and np.abs(got - ref).max() < 1e-14 * max(1.0, np.abs(ref).max())


def test_definition_constant_twist_puts_a_plane_back_on_the_plane():
    # the sensor moves with a constant twist while it sweeps; what it sees of the plane n.x = d, posed column by column, lies on the plane
    xi = np.zeros((4, 4))
    xi[:3, :3] = [[0, -0.4, 0.15], [0.4, 0, -0.1], [-0.15, 0.1, 0]]
    xi[:3, 3] = [1.2, -0.3, 0.1]
    n, d = np.array([0.2, 0.1, 1.0]) / np.linalg.norm([0.2, 0.1, 1.0]), -6.0
    H, W = 6, 32
    t0, t1 = 50.0, 50.1
    ts = pm.sweep_column_times(t0, t1, W)
    rng = np.random.default_rng(4)
    xyz = np.zeros((H, W, 3))
    for v in range(W):
        T = expm((ts[v] - 50.0) * xi)
        for u in range(H):
            ray = T[:3, :3] @ (np.array([np.cos(0.2 * v), np.sin(0.2 * v), -1.0 - 0.1 * u]) + 0.01 * rng.normal(size=3))
            lam = (d - n @ T[:3, 3]) / (n @ ray)
            assert lam > 0
            world = T[:3, 3] + lam * ray
            xyz[u, v] = T[:3, :3].T @ (world - T[:3, 3])
    knots = [(50.0 + t, expm(t * xi)) for t in (-0.05, 0.0, 0.03, 0.08, 0.2)]
    got = pm.posed_points(xyz, ts, knots)
    assert got.shape == (H * W, 3) and np.abs(got @ n - d).max() < 1e-12
    # with one pose for the whole sweep they do not
    one = pm.posed_points(xyz, np.full(W, t0), knots)
    assert np.abs(one @ n - d).max() > 1e-3


def test_definition_skips_a_sweep_with_one_column_outside_the_bounds():
    rng = np.random.default_rng(5)
    H, W = 3, 8
    sweeps = [rng.normal(0, 5, (H, W, 3)) for _ in range(3)]
    knots = [(10.0 + 0.1 * i, _pose([0, 0, 0.01 * i], [0.1 * i, 0, 0])) for i in range(11)]  # 10.0 .. 11.0
    ts = [pm.sweep_column_times(10.0 + 0.1 * k, 10.1 + 0.1 * k, W) for k in range(3)]
    ts[1] = ts[1].copy()
    ts[1][5] = 11.0 + 1.6  # one column 1.6 s past the last knot, bounds 1.5
    out, skipped = pm.posed_map_input(sweeps, ts, knots, time_bounds=1.5)
    assert skipped == 1 and len(out) == 2 and all(len(p) == H * W for p in out)
    ts[1][5] = 11.0 + 1.4
    out, skipped = pm.posed_map_input(sweeps, ts, knots, time_bounds=1.5)
    assert skipped == 0 and len(out) == 3


@pytest.mark.parametrize("ext", [".ply", ".npy"])
def test_map_files_round_trip_bit_exact(tmp_path, ext):
    rng = np.random.default_rng(7)
    pts = rng.normal(0, 40, (1237, 3))
    pts[3] = [np.nextafter(1.0, 2.0), -0.0, 1e-310]  # the doubles as they are
    path = str(tmp_path / ("map" + ext))
    pu.save_map_ply(path, pts)
    back = pu.load_map_ply(path)
    assert back.dtype == np.float64 and back.shape == pts.shape and back.tobytes() == pts.tobytes()
    if ext == ".ply":
        raw = open(path, "rb").read(200)
        head = raw.split(b"end_header\n")[0].decode().split("\n")
        assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0" and head[2] == f"element vertex {len(pts)}"
        assert head[3:6] == ["property double x", "property double y", "property double z"]
        assert head[6:] == [""] and os.path.getsize(path) == raw.index(b"end_header\n") + len("end_header\n") + 24 * len(pts)
    empty = str(tmp_path / ("empty" + ext))
    pu.save_map_ply(empty, np.zeros((0, 3)))
    assert pu.load_map_ply(empty).shape == (0, 3)


def test_commands_refuse_before_any_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    r = run(ptudes_cli, ["flyby", "--help"])
    assert r.exit_code == 0
    for opt in ("--synthetic", "-m, --meta", "--nc-gt-poses", "--kitti-poses", "--start-scan", "--end-scan", "--voxel-size", "--save-map",
                "-r, --rate", "--accum-map-ratio"):
        assert opt in r.output, opt
    poses = tmp_path / "p.txt"
    poses.write_text("1 0 0 0 0 1 0 0 0 0 1 0\n")
    r = run(ptudes_cli, ["flyby", "--synthetic", "1", "--kitti-poses", str(poses)])
    assert r.exit_code != 0 and "--kitti-poses is not supported" in r.output and "--nc-gt-poses" in r.output
    r = run(ptudes_cli, ["flyby", "--synthetic", "1"])
    assert r.exit_code != 0 and "Required one of --kitti-poses or --nc-gt-poses, but none was set." in r.output
    r = run(ptudes_cli, ["ekf-bench", "ouster", "--save-map", str(tmp_path / "x.ply"), "FILE"])
    assert r.exit_code != 0 and "--save-map needs --synthetic" in r.output and not (tmp_path / "x.ply").exists()
    r = run(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1", "--save-map", str(tmp_path / "x.ply"), "--map-from", "smoothed"])
    assert r.exit_code != 0 and "--save-smoothed-poses" in r.output
