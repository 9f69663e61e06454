"""Pose-file surface of the path: KITTI / Newer-College-GT writers and reader, timestamp matching.

Host-side mirror of the pose-file part of reference src/ptudes/utils.py (:22-36, :191-341): same
function names, argument meaning and byte-for-byte identical files, so `ptudes flyby --kitti-poses /
--nc-gt-poses` and `ptudes ekf-bench cmp` keep consuming what this package writes.  The viz / packet-IO
helpers of that file (PointViz, pcap/bag openers) are outside the pose path and are not provided.
"""
from typing import List, Optional, Tuple

import numpy as np
from scipy.spatial.transform import Rotation

# Newer College 2021 extrinsics (reference utils.py:20-26): IMU -> sensor, sensor -> base, both pure translations
NC_OS_IMU_TO_OS_SENSOR = np.eye(4)
NC_OS_IMU_TO_OS_SENSOR[:3, 3] = [-0.014, 0.012, 0.015]
NC_OS_SENSOR_TO_BASE = np.eye(4)
NC_OS_SENSOR_TO_BASE[:3, 3] = [0.001, 0.000, 0.091]
NC_OS_IMU_TO_BASE = NC_OS_SENSOR_TO_BASE @ NC_OS_IMU_TO_OS_SENSOR


def read_metadata_json(meta_path: str):
    """SensorInfo from a metadata .json (reference utils.py:157-168, including the lidar_mode back-fill for the
    Newer College 2020 beam_intrinsics files).  Needs ouster-sdk."""
    import json
    from ouster import client  # guarded: raises ImportError where ouster-sdk is absent
    with open(meta_path) as f:
        js = json.loads(f.read())
    if "beam_altitude_angles" in js and "beam_azimuth_angles" in js and "lidar_mode" not in js:
        print(f"WARNING: lidar_mode is not present in legacy metadata '{meta_path}' so using lidar_mode: 1024x10")
        js["lidar_mode"] = "1024x10"
    return client.SensorInfo(json.dumps(js))


def read_packet_source(file_path: str, meta=None):
    """Open PCAP or BAG based Ouster raw packet source (reference utils.py:171-187): a .pcap through ouster-sdk, a .bag
    or a directory of .bag files (sorted by name) through `bag.OusterRawBagSource`.  Both need ouster-sdk for the
    packet types; like the reference, anything else yields None."""
    import glob
    from pathlib import Path
    file = Path(file_path)
    if file.is_file():
        if file.suffix == ".pcap":
            from ouster import pcap  # guarded
            return pcap.Pcap(file_path, meta)
        elif file.suffix == ".bag":
            from .bag import OusterRawBagSource
            return OusterRawBagSource(file, meta)
    elif file.is_dir():
        from .bag import OusterRawBagSource
        bags_paths = sorted([Path(p) for p in glob.glob(str(Path(file) / "*.bag"))])
        return OusterRawBagSource(bags_paths, meta)


def vee(vec: np.ndarray) -> np.ndarray:
    """3-vector -> skew-symmetric matrix, hat(v) w = v x w (reference utils.py:28-36 names it `vee`)"""
    x, y, z = vec[0], vec[1], vec[2]
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def save_poses_kitti_format(filename: str, poses: List[np.ndarray], header: str = ""):
    """One row per pose: the top three rows of the 4x4, 12 numbers (reference utils.py:191-196)"""
    rows = np.array([np.asarray(p)[:3, :].reshape(12) for p in poses])
    np.savetxt(fname=filename, X=rows, header=header)


def save_poses_nc_gt_format(filename: str, t: List[float], poses: List[np.ndarray], header: str = ""):
    """Newer College ground-truth CSV: sec, nsec, x, y, z, qx, qy, qz, qw in the BASE frame; incoming poses
    are in the IMU (nav) frame (reference utils.py:199-228)."""
    t_arr = np.asarray(t, dtype=np.float64)
    base = np.einsum("nij,jk->nik", np.asarray(poses, dtype=np.float64), np.linalg.inv(NC_OS_IMU_TO_BASE))
    out = np.zeros((len(t_arr), 9))
    out[:, 0] = np.floor(t_arr)
    out[:, 1] = np.floor((t_arr - out[:, 0]) * 1e+9)
    out[:, 2:5] = base[:, :3, 3]
    out[:, 5:9] = Rotation.from_matrix(base[:, :3, :3]).as_quat()
    if header:
        header += "\n\n" + "sec,nsec,x,y,z,qx,qy,qz,qw"
    np.savetxt(fname=filename, X=out, delimiter=", ", header=header)


def read_newer_college_gt(data_path: str, to_os_imu: bool = True) -> List[Tuple[float, np.ndarray]]:
    """[(ts, pose4x4)] from a Newer College GT CSV, moved to the Ouster IMU nav frame (reference utils.py:231-252)"""
    d = np.loadtxt(data_path, delimiter=",")
    d = d.reshape(-1, 9) if d.ndim == 1 else d
    ts = d[:, 0] + d[:, 1] * 1e-9
    T = np.tile(np.eye(4), (len(d), 1, 1))
    T[:, :3, 3] = d[:, 2:5]
    T[:, :3, :3] = Rotation.from_quat(d[:, 5:9]).as_matrix()
    if to_os_imu:
        T = np.einsum("nij,jk->nik", T, NC_OS_IMU_TO_BASE)
    return list(zip(ts, T))


class _Cursor:
    """forward-only reader that raises StopIteration when exhausted (the reference walks Python iterators)"""

    def __init__(self, items):
        self.items, self.i = items, 0

    def take(self):
        if self.i >= len(self.items):
            raise StopIteration
        self.i += 1
        return self.items[self.i - 1]


def filter_nc_gt_by_close_ts(nc_gt, gt_t):
    """Greedy nearest-timestamp pairing of two non-decreasing streams (reference utils.py:255-302), including
    its corner behaviour: a candidate that loses the "closer than my successor" test is dropped, and the
    walk stops as soon as either stream runs out."""
    if not len(nc_gt):
        return nc_gt
    if not len(gt_t):
        return []
    nc_t = np.array([g[0] for g in nc_gt])
    tol = min(np.min(nc_t[1:] - nc_t[:-1]), np.min(np.array(gt_t[1:]) - np.array(gt_t[:-1])))
    a, b = _Cursor(list(nc_gt)), _Cursor(list(gt_t))
    out_gt, out_t = [], []
    try:
        n, g = a.take(), b.take()
        while True:
            while abs(n[0] - g) > tol:
                while n[0] < g - tol:
                    n = a.take()
                while g < n[0] - tol:
                    g = b.take()
            if n[0] < g:
                n2 = a.take()
                if abs(n[0] - g) < abs(n2[0] - g):
                    out_gt.append(n)
                    out_t.append(g)
                    n = n2
                    g = b.take()
            else:
                g2 = b.take()
                if abs(n[0] - g) < abs(n[0] - g2):
                    out_gt.append(n)
                    out_t.append(g)
                    n = a.take()
                    g = g2
    except StopIteration:
        pass
    return out_gt, out_t


def filter_nc_gt_by_cmp(nc_gt, nc_gt_cmp):
    """Closest subset of nc_gt_cmp in nc_gt, as two equally long [(t, pose)] lists (reference utils.py:305-325)"""
    cmp_t = [g[0] for g in nc_gt_cmp]
    matched_gt, matched_t = filter_nc_gt_by_close_ts(nc_gt, cmp_t)
    poses, idx = [], 0
    for t in matched_t:
        while cmp_t[idx] != t:
            idx += 1
        poses.append(nc_gt_cmp[idx][1])
        idx += 1
    assert len(poses) == len(matched_t)
    return matched_gt, list(zip(matched_t, poses))


def active_beam_rows(h: int, beams_num: int) -> np.ndarray:
    """rows kept by `reduce_active_beams` (reference utils.py:336): beams_num uniformly spread rows of h"""
    return np.linspace(0, h, num=beams_num, endpoint=False, dtype=int)


def reduce_active_beams(scan, beams_num: int):
    """Zero the RANGE (or xyz) of every row outside `active_beam_rows` (reference utils.py:328-341).
    `scan` is a (H, W) range image, a (H, W, 3) xyz image, or an ouster LidarScan."""
    if hasattr(scan, "field") and hasattr(scan, "h"):  # ouster LidarScan, only when ouster-sdk is present
        from ouster import client  # noqa: WPS433 (guarded import)
        arr, h = scan.field(client.ChanField.RANGE), scan.h
    else:
        arr, h = scan, scan.shape[0]
    drop = np.ones(h, dtype=bool)
    drop[active_beam_rows(h, beams_num)] = False
    arr[drop] = 0
    return scan


class TrajectoryEvaluator:
    """Poses along a time-stamped trajectory: the part of ouster.sdk.pose_util.TrajectoryEvaluator the reference uses
    (utils.py:368 `pose_scans_from_nc_gt`, cli/ekf_bench.py:489 / :537 `--use-gt-guess`; third-party, behaviour from its
    published description): SE(3) geodesic between the bracketing knots, the end segments extended by `time_bounds`
    seconds (a number, or (before, after)), ValueError further out.  The interpolation runs on the GPU
    (`ptl_traj_poses_at`): a sweep asks for 1024 or 2048 poses at once."""

    def __init__(self, poses, time_bounds=0.0, device_id: int = 0):
        poses = list(poses)
        if len(poses) < 2:
            raise ValueError("a trajectory needs at least two (ts, pose) knots")
        self._ts = np.array([p[0] for p in poses], dtype=np.float64)
        self._poses = np.array([np.asarray(p[1], dtype=np.float64) for p in poses])
        self._bounds = (float(time_bounds), float(time_bounds)) if np.isscalar(time_bounds) else tuple(map(float, time_bounds))
        self._device_id = device_id

    @property
    def start_time(self) -> float:
        return float(self._ts[0])

    @property
    def end_time(self) -> float:
        return float(self._ts[-1])

    def poses_at(self, ts) -> np.ndarray:
        from . import core
        ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
        out, outside = core.traj_poses_at(self._ts, self._poses, ts, self._bounds[0], self._bounds[1], self._device_id)
        if outside:
            raise ValueError(f"{outside} of {len(ts)} timestamps lie outside the trajectory "
                             f"({self._ts[0]} .. {self._ts[-1]}, bounds {self._bounds})")
        return out

    def pose_at(self, ts: float) -> np.ndarray:
        return self.poses_at([ts])[0]

    def __call__(self, scan, col_ts=None):
        """write the pose of every column of `scan` (ts of its columns in seconds) into scan.pose, like upstream"""
        col_ts = np.asarray(scan.timestamp, dtype=np.float64) * 1e-9 if col_ts is None else np.asarray(col_ts, dtype=np.float64)
        scan.pose[:] = self.poses_at(col_ts)


def pose_scans_from_nc_gt(source, nc_gt_poses_file: Optional[str] = None, nc_gt_poses=None, device_id: int = 0):
    """Give every scan of `source` the ground-truth pose of each of its columns (reference utils.py:344-392): scans whose
    columns are not all within 1.5 s of the trajectory are left out, and counted in the closing note.  A scan is
    anything with `timestamp` (W ns) and `pose` (W, 4, 4) - an ouster LidarScan, or `fly.PosedScan`."""
    gts = read_newer_college_gt(nc_gt_poses_file) if nc_gt_poses_file else nc_gt_poses
    traj_eval = TrajectoryEvaluator(gts, time_bounds=1.5, device_id=device_id)
    skipped_scans = 0
    for scan in source:
        if not (hasattr(scan, "timestamp") and hasattr(scan, "pose")):
            continue
        try:
            traj_eval(scan, col_ts=np.asarray(scan.timestamp, dtype=np.float64) * 1e-9)
        except ValueError:
            skipped_scans += 1
            continue
        yield scan
    print(f"NOTE: Therere where {skipped_scans} skipped scans that wasn't "
          "because they were outside of the NC GT poses available")


_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {n}\n"
               "property double x\nproperty double y\nproperty double z\nend_header\n")


_PLY_SCALARS = (("int", "neighbours"), ("double", "plane_var"), ("double", "entropy"))
_PLY_XYZ = [("double", "x"), ("double", "y"), ("double", "z")]
_PLY_SCORED_DTYPE = np.dtype([("xyz", "<f8", (3,)), ("neighbours", "<i4"), ("plane_var", "<f8"), ("entropy", "<f8")])
_PLY_DIST_DTYPE = np.dtype([("xyz", "<f8", (3,)), ("dist", "<f8")])
_PLY_CARVE = (("uint", "through"), ("uint", "support"), ("uchar", "dynamic"))
_PLY_CARVE_DTYPE = np.dtype([("xyz", "<f8", (3,)), ("through", "<u4"), ("support", "<u4"), ("dynamic", "u1")])
_PLY_PAINT_FIELDS = ("range", "reflectivity", "signal", "near_ir")
_PLY_PAINT_DTYPE = np.dtype([("xyz", "<f8", (3,)), ("mean", "<f8"), ("count", "<u4")])


def save_map_ply(path: str, xyz, scalars=None) -> None:
    """A point map (N, 3) to disk: PLY `binary_little_endian 1.0`, `element vertex N`, three `property double` x y z - the doubles
    as they are, so a map read back is bit-equal; a path ending in .npy uses np.save instead.
    scalars = (neighbours (N,) int, plane_var (N,), entropy (N,)) - the per-point values of a map score: three more
    properties behind x y z (`int neighbours`, `double plane_var`, `double entropy`); PLY only (a .npy map is the points and nothing else).
    scalars = {"dist": (N,)} - the per-point distance to a reference cloud (NaN = unmatched): one more property, `double dist`.
    scalars = {"through": (N,), "support": (N,), "dynamic": (N,)} - the votes of a carve and the host policy's flag: `uint
    through`, `uint support`, `uchar dynamic`.
    scalars = {FIELD: (N,), FIELD + "_count": (N,)}, FIELD one of range / reflectivity / signal / near_ir - a painted map: `double
    FIELD` (the mean of the field at the point, NaN where no ray ended) and `uint FIELD_count`; `load_map_ply(scalars=True)` gives the dict back.
    Without scalars the file is what it always was, byte for byte."""
    pts = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    if isinstance(scalars, dict) and list(scalars) == ["through", "support", "dynamic"]:
        # the votes of a carve: `uint through`, `uint support`, `uchar dynamic` (the host policy's flag) behind x y z
        cols = [np.asarray(scalars[k]).reshape(-1) for k in scalars]
        if any(len(c) != len(pts) for c in cols):
            raise ValueError("scalars: one through / support / dynamic value per point")
        if str(path).endswith(".npy"):
            raise ValueError("per-point scalars are written to a PLY file only: a .npy map holds the points")
        rec = np.empty(len(pts), dtype=_PLY_CARVE_DTYPE)
        rec["xyz"], rec["through"], rec["support"], rec["dynamic"] = pts, cols[0], cols[1], cols[2]
        extra = "".join(f"property {t} {name}\n" for t, name in _PLY_CARVE)
        with open(path, "wb") as f:
            f.write(_PLY_HEADER.format(n=len(pts)).replace("end_header\n", extra + "end_header\n").encode("ascii"))
            f.write(rec.tobytes())
        return
    if isinstance(scalars, dict) and len(scalars) == 2 and list(scalars)[1] == list(scalars)[0] + "_count":
        # a painted map: `double FIELD` (the mean of the field at the point, NaN = no ray ended there) and `uint FIELD_count`
        name = list(scalars)[0]
        if name not in _PLY_PAINT_FIELDS:
            raise ValueError(f"scalars: a painted map's field is one of {', '.join(_PLY_PAINT_FIELDS)}, not '{name}'")
        mean, count = np.asarray(scalars[name], dtype=np.float64).reshape(-1), np.asarray(scalars[name + "_count"]).reshape(-1)
        if len(mean) != len(pts) or len(count) != len(pts):
            raise ValueError(f"scalars: one {name} / {name}_count value per point")
        if str(path).endswith(".npy"):
            raise ValueError("per-point scalars are written to a PLY file only: a .npy map holds the points")
        rec = np.empty(len(pts), dtype=_PLY_PAINT_DTYPE)
        rec["xyz"], rec["mean"], rec["count"] = pts, mean, count
        with open(path, "wb") as f:
            f.write(_PLY_HEADER.format(n=len(pts)).replace("end_header\n", f"property double {name}\nproperty uint {name}_count\nend_header\n").encode("ascii"))
            f.write(rec.tobytes())
        return
    if isinstance(scalars, dict):
        if list(scalars) != ["dist"] or len(np.asarray(scalars["dist"]).reshape(-1)) != len(pts):
            raise ValueError("scalars: a dict holds `dist`, one value per point")
        if str(path).endswith(".npy"):
            raise ValueError("per-point scalars are written to a PLY file only: a .npy map holds the points")
        rec = np.empty(len(pts), dtype=_PLY_DIST_DTYPE)
        rec["xyz"], rec["dist"] = pts, np.asarray(scalars["dist"], dtype=np.float64).reshape(-1)
        with open(path, "wb") as f:
            f.write(_PLY_HEADER.format(n=len(pts)).replace("end_header\n", "property double dist\nend_header\n").encode("ascii"))
            f.write(rec.tobytes())
        return
    if scalars is not None:
        nb, pv, ent = (np.asarray(a).reshape(-1) for a in scalars)
        if not len(nb) == len(pv) == len(ent) == len(pts):
            raise ValueError("scalars: one neighbours / plane_var / entropy value per point")
    if str(path).endswith(".npy"):
        if scalars is not None:
            raise ValueError("per-point scalars are written to a PLY file only: a .npy map holds the points")
        np.save(path, pts)
        return
    with open(path, "wb") as f:
        if scalars is None:
            f.write(_PLY_HEADER.format(n=len(pts)).encode("ascii"))
            f.write(pts.astype("<f8", copy=False).tobytes())
            return
        extra = "".join(f"property {t} {name}\n" for t, name in _PLY_SCALARS)
        f.write(_PLY_HEADER.format(n=len(pts)).replace("end_header\n", extra + "end_header\n").encode("ascii"))
        rec = np.empty(len(pts), dtype=_PLY_SCORED_DTYPE)
        rec["xyz"], rec["neighbours"], rec["plane_var"], rec["entropy"] = pts, nb, pv, ent
        f.write(rec.tobytes())


def load_map_ply(path: str, scalars: bool = False):
    """(N, 3) float64 of a map written by `save_map_ply` (.npy: np.load), with or without per-point scalars.  Reads the PLY subset that
    function writes.  scalars=True: (points, (neighbours int32, plane_var, entropy)), the second None for a file without them and
    {"dist": (N,)} for a file with the distance to a reference cloud, {"through", "support", "dynamic"} for a file with a carve's votes."""
    if str(path).endswith(".npy"):
        pts = np.load(path).reshape(-1, 3)
        return (pts, None) if scalars else pts
    with open(path, "rb") as f:
        n, fmt, props = None, None, []
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        for raw in iter(f.readline, b""):
            w = raw.decode("ascii", "replace").split()
            if w[:1] == ["end_header"]:
                break
            if w[:1] == ["format"]:
                fmt = w[1]
            elif w[:2] == ["element", "vertex"]:
                n = int(w[2])
            elif w[:1] == ["element"]:
                raise ValueError(f"{path}: only a vertex element is read")
            elif w[:1] == ["property"]:
                props.append(tuple(w[1:]))
        else:
            raise ValueError(f"{path}: no end_header")
        scored = props == _PLY_XYZ + list(_PLY_SCALARS)
        with_dist = props == _PLY_XYZ + [("double", "dist")]
        if props == _PLY_XYZ + list(_PLY_CARVE) and fmt == "binary_little_endian" and n is not None:
            size = _PLY_CARVE_DTYPE.itemsize
            data = f.read(n * size)
            if len(data) != n * size:
                raise ValueError(f"{path}: {n} vertices announced, {len(data) // size} present")
            rec = np.frombuffer(data, dtype=_PLY_CARVE_DTYPE)
            pts = np.ascontiguousarray(rec["xyz"], dtype=np.float64)
            return (pts, {k: rec[k].copy() for _, k in _PLY_CARVE}) if scalars else pts
        painted = [nm for nm in _PLY_PAINT_FIELDS if props == _PLY_XYZ + [("double", nm), ("uint", nm + "_count")]]
        if painted and fmt == "binary_little_endian" and n is not None:
            size = _PLY_PAINT_DTYPE.itemsize
            data = f.read(n * size)
            if len(data) != n * size:
                raise ValueError(f"{path}: {n} vertices announced, {len(data) // size} present")
            rec = np.frombuffer(data, dtype=_PLY_PAINT_DTYPE)
            pts = np.ascontiguousarray(rec["xyz"], dtype=np.float64)
            return (pts, {painted[0]: rec["mean"].astype(np.float64), painted[0] + "_count": rec["count"].copy()}) if scalars else pts
        if with_dist and fmt == "binary_little_endian" and n is not None:
            data = f.read(n * 32)
            if len(data) != n * 32:
                raise ValueError(f"{path}: {n} vertices announced, {len(data) // 32} present")
            rec = np.frombuffer(data, dtype=_PLY_DIST_DTYPE)
            pts = np.ascontiguousarray(rec["xyz"], dtype=np.float64)
            return (pts, {"dist": rec["dist"].astype(np.float64)}) if scalars else pts
        if fmt != "binary_little_endian" or n is None or not (props == _PLY_XYZ or scored):
            raise ValueError(f"{path}: expected binary_little_endian, element vertex N, property double x y z"
                             " (optionally int neighbours, double plane_var, double entropy)")
        size = _PLY_SCORED_DTYPE.itemsize if scored else 24
        data = f.read(n * size)
    if len(data) != n * size:
        raise ValueError(f"{path}: {n} vertices announced, {len(data) // size} present")
    if not scored:
        pts = np.frombuffer(data, dtype="<f8").astype(np.float64).reshape(n, 3)
        return (pts, None) if scalars else pts
    rec = np.frombuffer(data, dtype=_PLY_SCORED_DTYPE)
    pts = np.ascontiguousarray(rec["xyz"], dtype=np.float64)
    extras = (rec["neighbours"].astype(np.int32), rec["plane_var"].astype(np.float64), rec["entropy"].astype(np.float64))
    return (pts, extras) if scalars else pts


def log_pose(pose: np.ndarray) -> np.ndarray:
    """SE(3) logarithm of a 4x4 pose as (rotation vector (3), translation part (3)) - the order of ouster-sdk's pose_util.log_pose, which
    the reference's camera path uses (fly.py:172, utils.py:143)"""
    T = np.asarray(pose, dtype=np.float64)
    w = Rotation.from_matrix(T[:3, :3]).as_rotvec()
    th = float(np.linalg.norm(w))
    W = vee(w)
    if th < 1e-8:
        Vinv = np.eye(3) - 0.5 * W + (W @ W) / 12.0
    else:
        Vinv = np.eye(3) - 0.5 * W + (1.0 / th ** 2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))) * (W @ W)
    return np.concatenate([w, Vinv @ T[:3, 3]])


def exp_pose6(xi: np.ndarray) -> np.ndarray:
    """SE(3) exponential of (rotation vector (3), translation part (3)): the inverse of `log_pose`"""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    W = vee(w)
    if th < 1e-8:
        V = np.eye(3) + 0.5 * W + (W @ W) / 6.0
    else:
        V = np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * (W @ W)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(w).as_matrix()
    T[:3, 3] = V @ v
    return T


def estimate_apex_dolly(min_max: np.ndarray, fov_deg: float) -> float:
    """The dolly at which the box between min_max[:, 0] and min_max[:, 1] fits the view (reference utils.py:107-111):
    D = 1.4142 d / sin(fov), dolly = max(-100, 100 ln(max(0.001, D) / 50))"""
    mm = np.asarray(min_max, dtype=np.float64)
    d = np.linalg.norm(mm[:, 1] - mm[:, 0])
    D = 1.4142 * d / np.sin(fov_deg * np.pi / 180)
    return float(max(-100, 100 * np.log(max(0.001, D) / 50.0)))


def prune_trajectory_indices(traj_poses, min_dist_m=5, min_dist_angle=5, start_idx=None, end_idx=None) -> List[int]:
    """indices of the knots `prune_trajectory` keeps (reference utils.py:122-153): the first, every one more than min_dist_m metres or
    min_dist_angle degrees (SE(3) logarithm) from the last kept one, the last in any case; a single knot gets its successor"""
    start_idx = 0 if start_idx is None else start_idx
    end_idx = len(traj_poses) - 1 if end_idx is None else end_idx
    assert start_idx <= end_idx, f"{start_idx = } should be lte {end_idx = }"
    assert start_idx < len(traj_poses) and end_idx < len(traj_poses), \
        f"{start_idx = } and {end_idx = } should be lt {len(traj_poses) = }"
    kept = [start_idx]
    last_pose_inv = np.linalg.inv(traj_poses[start_idx][1])
    for idx in range(start_idx + 1, end_idx + 1):
        p = traj_poses[idx][1]
        pd = log_pose(last_pose_inv @ p)
        pda, pdm = np.linalg.norm(pd[:3]), np.linalg.norm(pd[3:])
        if pda > min_dist_angle * np.pi / 180 or pdm > min_dist_m or idx == end_idx:
            kept.append(idx)
            last_pose_inv = np.linalg.inv(p)
    if len(kept) < 2 and end_idx + 1 < len(traj_poses):
        kept.append(end_idx + 1)
    return kept


def make_kiss_traj_poses(poses) -> List[Tuple[float, np.ndarray]]:
    """[(ts, pose)] with knot i at i + 0.5: the unit-spaced timestamps the reference's pruned camera trajectory gets from ouster-sdk's
    pose_util.make_kiss_traj_poses (third party; the offset only shifts the coursing clock, CoursingState walks first to last knot)"""
    return [(i + 0.5, np.asarray(p, dtype=np.float64)) for i, p in enumerate(poses)]


def prune_trajectory(traj_poses, min_dist_m=5, min_dist_angle=5, start_idx=None, end_idx=None) -> List[Tuple[float, np.ndarray]]:
    """Pruned poses without the knots close to each other, re-timed one per unit (reference utils.py:122-154)"""
    kept = prune_trajectory_indices(traj_poses, min_dist_m, min_dist_angle, start_idx, end_idx)
    return make_kiss_traj_poses([traj_poses[i][1] for i in kept])


_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    import struct
    import zlib
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def save_png(path: str, rgba) -> None:
    """An (H, W, 4) uint8 frame as a PNG: 8-bit RGBA, no interlace, every scan line with filter 0 - standard library only"""
    import struct
    import zlib
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("save_png: need an (H, W, 4) uint8 frame")
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 4 * w), dtype=np.uint8)
    raw[:, 1:] = a.reshape(h, 4 * w)
    with open(path, "wb") as f:
        f.write(_PNG_SIG + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def load_png(path: str) -> np.ndarray:
    """(H, W, 4) uint8 of a PNG written by `save_png` (8-bit RGBA, filter 0 on every line; anything else: ValueError)"""
    import struct
    import zlib
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, hdr, idat = 8, None, b""
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError(f"{path}: chunk {tag!r} fails its CRC")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None or hdr[2:] != (8, 6, 0, 0, 0):
        raise ValueError(f"{path}: expected 8-bit RGBA without interlace, as save_png writes it")
    w, h = hdr[0], hdr[1]
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    if raw.size != h * (1 + 4 * w):
        raise ValueError(f"{path}: {raw.size} bytes of image data, {h * (1 + 4 * w)} expected")
    raw = raw.reshape(h, 1 + 4 * w)
    if raw[:, 0].any():
        raise ValueError(f"{path}: a scan line uses a filter; save_png writes filter 0 only")
    return raw[:, 1:].reshape(h, w, 4).copy()


_MAP_GRAY = (254, 0, 205)  # pixel of class 0 free, 1 occupied, 2 unknown (core.GRID_*): what ROS map_server's files use


def _occupancy_paths(prefix: str):
    import os
    stem, ext = os.path.splitext(str(prefix))
    if ext.lower() == ".png":
        return str(prefix), stem + ".yaml"
    return str(prefix) + ".pgm", str(prefix) + ".yaml"


def save_occupancy_map(prefix: str, classes, cell: float, origin) -> Tuple[str, str]:
    """An occupancy grid as ROS map_server reads it: `prefix`.pgm (binary P5, 254 free, 0 occupied, 205 unknown; the FIRST image row is the
    LARGEST y) with `prefix`.yaml beside it (six lines: image, resolution, origin: [x, y, 0.0], negate: 0, occupied_thresh: 0.65, free_thresh:
    0.196).  classes: (ny, nx) with 0 free, 1 occupied, 2 unknown (core.grid_classify), row 0 the smallest y; origin: (x, y) of the corner of
    classes[0, 0].  A prefix that ends in .png writes that PNG (the same grey values, through `save_png`) and the .yaml beside it.  Standard
    library and numpy only.  Returns (image path, yaml path)"""
    import os
    c = np.asarray(classes)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1 or not np.isin(c, (0, 1, 2)).all():
        raise ValueError("save_occupancy_map: need an (ny, nx) array of the classes 0 free, 1 occupied, 2 unknown")
    if not float(cell) > 0.0:
        raise ValueError(f"save_occupancy_map: cell = {cell}: must be positive")
    gray = np.ascontiguousarray(np.array(_MAP_GRAY, dtype=np.uint8)[c.astype(np.int64)][::-1])
    image, yaml = _occupancy_paths(prefix)
    if image.lower().endswith(".png"):
        save_png(image, np.dstack([gray, gray, gray, np.full_like(gray, 255)]))
    else:
        with open(image, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (gray.shape[1], gray.shape[0]) + gray.tobytes())
    with open(yaml, "w") as f:
        f.write(f"image: {os.path.basename(image)}\nresolution: {float(cell)!r}\norigin: [{float(origin[0])!r}, {float(origin[1])!r}, 0.0]\n"
                "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")
    return image, yaml


def load_occupancy_map(prefix: str):
    """(classes (ny, nx) uint8 with row 0 the smallest y, cell, (x, y) of the corner of classes[0, 0]) of the files `save_occupancy_map(prefix,
    ...)` wrote; `prefix` may also name the .yaml itself.  A grey value other than 254 / 0 / 205 is a ValueError"""
    import os
    yaml = str(prefix) if str(prefix).endswith(".yaml") else _occupancy_paths(prefix)[1]
    meta = {}
    with open(yaml) as f:
        for line in f:
            if ":" in line:
                k, v = line.split(":", 1)
                meta[k.strip()] = v.strip()
    for k in ("image", "resolution", "origin"):
        if k not in meta:
            raise ValueError(f"{yaml}: no `{k}` line")
    if meta.get("negate", "0") != "0":
        raise ValueError(f"{yaml}: negate: {meta['negate']} is not written by save_occupancy_map")
    image = os.path.join(os.path.dirname(yaml), meta["image"])
    ox, oy = (float(v) for v in meta["origin"].strip("[]").split(",")[:2])
    if image.lower().endswith(".png"):
        gray = load_png(image)[:, :, 0]
    else:
        with open(image, "rb") as f:
            data = f.read()
        tokens, pos = [], 0
        while len(tokens) < 4:  # P5, width, height, maxval: separated by white space, one white-space byte before the pixels
            while data[pos:pos + 1].isspace():
                pos += 1
            end = pos
            while end < len(data) and not data[end:end + 1].isspace():
                end += 1
            tokens.append(data[pos:end])
            pos = end
        if tokens[0] != b"P5" or tokens[3] != b"255":
            raise ValueError(f"{image}: expected a binary P5 image with maxval 255")
        w, h = int(tokens[1]), int(tokens[2])
        gray = np.frombuffer(data, dtype=np.uint8, count=w * h, offset=pos + 1).reshape(h, w)
    classes = np.full(gray.shape, 255, dtype=np.uint8)
    for k, g in enumerate(_MAP_GRAY):
        classes[gray == g] = k
    if (classes == 255).any():
        raise ValueError(f"{image}: a grey value other than {_MAP_GRAY}")
    return np.ascontiguousarray(classes[::-1]), float(meta["resolution"]), (ox, oy)


def nc_gt_file_rows(t, poses) -> List[Tuple[float, np.ndarray]]:
    """[(ts, pose)] as `read_newer_college_gt` gives them back from the file `save_poses_nc_gt_format(t, poses)` writes (through the
    same text, in memory): what a later `flyby --nc-gt-poses` of that file works with"""
    import io
    buf = io.StringIO()
    save_poses_nc_gt_format(buf, t=t, poses=poses)
    buf.seek(0)
    return read_newer_college_gt(buf)


# ------------------------------------------------------------------------------------------------ places files
PLACE_CFG_KEYS = ("n_ring", "n_sector", "min_radius", "max_radius", "z_min", "z_step")


def _place_cfg_row(index) -> np.ndarray:
    return np.array([float(getattr(index.cfg, k)) for k in PLACE_CFG_KEYS])


def save_places(path: str, index, poses, stamps) -> None:
    """The entries of a `core.PlaceIndex` with the pose and stamp of the sweep behind each, as one .npz: cfg (the six parameters of
    PLACE_CFG_KEYS, float64), ring_edge2, sector_dir (the tables as the device uses them), desc (n, S, Rpad) uint8, infos (n, 9) int64, poses
    (n, 4, 4), stamps (n,).  `index` needs .cfg, .tables() and .descriptors() - nothing else is asked of it"""
    desc, infos = index.descriptors()
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    t = np.asarray(stamps, dtype=np.float64).reshape(-1)
    if len(P) != len(desc) or len(t) != len(desc):
        raise ValueError(f"save_places: {len(desc)} entries with {len(P)} poses and {len(t)} stamps")
    edge2, sdir = index.tables()
    with open(path, "wb") as f:  # (np.savez appends .npz to a bare name: the file is called what the caller said)
        np.savez(f, cfg=_place_cfg_row(index), ring_edge2=np.asarray(edge2), sector_dir=np.asarray(sdir), desc=desc, infos=infos, poses=P, stamps=t)


def load_places(path: str, index=None) -> dict:
    """The arrays of a file `save_places` wrote, as a dict (cfg is a dict of PLACE_CFG_KEYS).  With `index` the entries are APPENDED to it
    (`index.load`) - after the file's cfg and tables have been held against the handle's: any difference is a ValueError that names it, since
    descriptors binned by other tables do not compare"""
    with np.load(path) as z:
        missing = [k for k in ("cfg", "ring_edge2", "sector_dir", "desc", "infos", "poses", "stamps") if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a places file (no {', '.join(missing)})")
        out = {k: z[k] for k in z.files}
    n = len(out["desc"])
    if out["desc"].ndim != 3 or out["infos"].shape != (n, 9) or out["poses"].shape != (n, 4, 4) or out["stamps"].shape != (n,):
        raise ValueError(f"{path}: {n} descriptors with infos {out['infos'].shape}, poses {out['poses'].shape}, stamps {out['stamps'].shape}")
    if index is not None:
        have = _place_cfg_row(index)
        for k, a, b in zip(PLACE_CFG_KEYS, out["cfg"], have):
            if a != b:
                raise ValueError(f"{path}: {k} = {a:g} in the file, {b:g} in the handle: descriptors of other parameters do not compare")
        edge2, sdir = index.tables()
        for name, a, b in (("ring_edge2", out["ring_edge2"], edge2), ("sector_dir", out["sector_dir"], sdir)):
            if a.shape != np.shape(b) or not np.array_equal(a, b):
                raise ValueError(f"{path}: the table {name} differs from the handle's (another libm made it): the descriptors were binned "
                                 "by other edges and do not compare bit for bit")
        index.load(out["desc"], out["infos"])
    out["cfg"] = {k: (int(v) if k in ("n_ring", "n_sector") else float(v)) for k, v in zip(PLACE_CFG_KEYS, out["cfg"])}
    return out
