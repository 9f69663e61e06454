"""Thin object layer over the C-ABI: `Icp` (one KissICP-equivalent on one GPU), `Ekf`, `SeqRunner`
(the reference's driver loop, cli/ekf_bench.py:493-563, on a sequence resident in HBM)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def icp_cfg(max_range=100.0, min_range=5.0, **over):
    """Reference defaults for (max_range, min_range) (kiss.py:21-43) with overrides by field name."""
    cfg = L.IcpCfg()
    L.check(L.lib().ptl_icp_default_cfg(C.byref(cfg), float(max_range), float(min_range)))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise ValueError(f"unknown icp cfg field {k}")
        setattr(cfg, k, v)
    return cfg


def ekf_cfg(init_grav=None, init_bacc=None, init_bgyr=None, device_id=0):
    cfg = L.EkfCfg()
    L.check(L.lib().ptl_ekf_default_cfg(C.byref(cfg)))
    for name, val in (("init_grav", init_grav), ("init_bacc", init_bacc), ("init_bgyr", init_bgyr)):
        if val is not None:
            v = np.asarray(val, dtype=np.float64).reshape(3)
            setattr(cfg, name, (C.c_double * 3)(*v))
    cfg.device_id = device_id
    return cfg


@dataclass
class MapScore:
    """Summary of `Icp.map_score` (include/ptudes_mi.h ptl_map_score_result): counts, the means over the scored points, the parameters as
    used, and the HIP-event time of the call's kernels"""
    n_points: int
    n_scored: int
    n_sparse: int
    mean_plane_var: float
    mean_entropy: float
    mean_neighbours: float
    radius: float
    min_neighbours: int
    sigma_floor: float
    device_ms: float

    @property
    def thickness_mm(self):
        """sqrt(mean plane variance) in millimetres: the "wall thickness" of the map"""
        return 1000.0 * float(np.sqrt(self.mean_plane_var))

    def lines(self):
        """the block the commands print"""
        return [f"map score: radius {self.radius:g} m, min neighbours {self.min_neighbours}, sigma floor {self.sigma_floor:g} m",
                f"  points: {self.n_points} (scored {self.n_scored}, sparse {self.n_sparse}), mean neighbours {self.mean_neighbours:.2f}",
                f"  mean plane variance: {self.mean_plane_var:.6e} m^2 (wall thickness {self.thickness_mm:.3f} mm)",
                f"  mean map entropy: {self.mean_entropy:.6f}"]


@dataclass
class MapDistance:
    """Summary of `Icp.map_distance` / `Icp.map_compare` (include/ptudes_mi.h ptl_map_cmp_result): the queries' nearest-neighbour distances
    to a reference map's stored points - counts (exact), the sums over the matched queries, the parameters as used and the HIP-event time"""
    n_query: int
    n_invalid: int
    n_matched: int
    n_within: tuple        # one count per threshold: queries with d2 <= threshold^2
    sum_dist: float
    sum_dist2: float
    max_dist2_seen: float
    max_dist: float
    thresholds: tuple
    device_ms: float

    @property
    def mean_dist(self):
        """mean distance of the matched queries, metres (0 when there is none)"""
        return self.sum_dist / self.n_matched if self.n_matched else 0.0

    @property
    def rms_dist(self):
        return float(np.sqrt(self.sum_dist2 / self.n_matched)) if self.n_matched else 0.0

    @property
    def fractions(self):
        """n_within / n_query per threshold (0 without queries): precision of a map against a reference, recall the other way round"""
        return tuple(w / self.n_query if self.n_query else 0.0 for w in self.n_within)

    @classmethod
    def _from(cls, res):
        k = int(res.n_thresholds)
        return cls(int(res.n_query), int(res.n_invalid), int(res.n_matched), tuple(int(x) for x in res.n_within[:k]), float(res.sum_dist),
                   float(res.sum_dist2), float(res.max_dist2_seen), float(res.max_dist), tuple(float(x) for x in res.thresholds[:k]),
                   float(res.device_ms))


def map_cmp_cfg(voxel_size, max_dist=None, thresholds=None):
    """the _lib.MapCmpCfg of a reference map of that voxel size: max_dist defaults to the voxel size, thresholds to (max_dist,)"""
    cfg = L.MapCmpCfg()
    L.check(L.lib().ptl_map_cmp_default_cfg(C.byref(cfg), float(voxel_size)))
    if max_dist is not None:
        cfg.max_dist = float(max_dist)
    thr = [cfg.max_dist] if thresholds is None else [float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1)]
    cfg.n_thresholds = len(thr)  # (a count outside 1 .. 8 is the library's to refuse, with the number)
    for k, t in enumerate(thr[:8]):
        cfg.thresholds[k] = t
    return cfg


@dataclass
class PoseHits:
    """Summary of `Icp.pose_hits` (include/ptudes_mi.h ptl_pose_search_result): per threshold the largest hit count over the valid candidates
    and the smallest candidate index that attains it (-1 without a valid candidate), the counts of non-finite inputs, the parameters as used
    and the HIP-event time"""
    n_points: int
    n_invalid_points: int
    n_poses: int
    n_invalid_poses: int
    best_pose: tuple       # one index per threshold
    best_hits: tuple
    max_dist: float
    thresholds: tuple
    device_ms: float

    @property
    def fractions(self):
        """best_hits / n_points per threshold (0 without points)"""
        return tuple(h / self.n_points if self.n_points else 0.0 for h in self.best_hits)

    @classmethod
    def _from(cls, res):
        k = int(res.n_thresholds)
        return cls(int(res.n_points), int(res.n_invalid_points), int(res.n_poses), int(res.n_invalid_poses),
                   tuple(int(x) for x in res.best_pose[:k]), tuple(int(x) for x in res.best_hits[:k]), float(res.max_dist),
                   tuple(float(x) for x in res.thresholds[:k]), float(res.device_ms))


def pose_search_cfg(voxel_size, max_dist=None, thresholds=None):
    """the _lib.PoseSearchCfg of a map of that voxel size: max_dist defaults to the voxel size, thresholds to (max_dist,)"""
    cfg = L.PoseSearchCfg()
    L.check(L.lib().ptl_pose_search_default_cfg(C.byref(cfg), float(voxel_size)))
    if max_dist is not None:
        cfg.max_dist = float(max_dist)
    thr = [cfg.max_dist] if thresholds is None else [float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1)]
    cfg.n_thresholds = len(thr)  # (a count outside 1 .. 4 is the library's to refuse, with the number)
    for k, t in enumerate(thr[:4]):
        cfg.thresholds[k] = t
    return cfg


def map_from_points(points, voxel_size=0.5, max_points_per_voxel=20, device_id=0, max_points_per_scan=1 << 20, **over):
    """an `Icp` whose voxel map holds `points` (N, 3), added in chunks of at most its max_points_per_scan in array order (a voxel keeps its
    first max_points_per_voxel points): a reference map for `Icp.map_distance` / `Icp.map_compare` out of a bare cloud"""
    pts = L.as_f64(points).reshape(-1, 3)
    over.setdefault("map_block_capacity", 1 << 21)  # (fly.MapAccumulator's)
    over.setdefault("map_table_capacity", 1 << 23)
    icp = Icp(1.0e9, 0.0, voxel_size=voxel_size, max_points_per_voxel=max_points_per_voxel, device_id=device_id,
              max_points_per_scan=int(max_points_per_scan), **over)
    try:
        step = int(icp.cfg.max_points_per_scan)
        for off in range(0, len(pts), step):
            icp.map_add(pts[off:off + step])
    except Exception:
        icp.close()
        raise
    return icp


def _diag(icp_handle):
    """{name: value} of the named slots a diagnostic build collects for one registration handle (csrc/diag.h; all 0 in the product build),
    cumulative since its cold start; the names are the library's own (include/ptudes_mi.h ptl_icp_diag)"""
    n = L.lib().ptl_diag_slots()
    out = (C.c_int64 * n)()
    L.check(L.lib().ptl_icp_diag(icp_handle, out, n))
    return {L.lib().ptl_diag_slot_name(i).decode(): int(out[i]) for i in range(n)}


class Icp:
    def __init__(self, max_range=100.0, min_range=5.0, lazy_map_stats=False, **over):
        """lazy_map_stats: registrations return when the pose is there, before the scan's map update is complete (the per-scan rows then
        carry map_voxels = map_points = -1; `map_size()` gives them on demand) - include/ptudes_mi.h ptl_icp_set_lazy_map_stats"""
        self.cfg = icp_cfg(max_range, min_range, **over)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_icp_create(C.byref(self.cfg), C.byref(self._h)))
        if lazy_map_stats:
            L.check(L.lib().ptl_icp_set_lazy_map_stats(self._h, 1))
        self.stats = []

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_icp_destroy(self._h)
            self._h = None

    __del__ = close

    def register_frame(self, xyz, t01=None, guess=None, scan_ts=0.0):
        xyz = np.asarray(xyz)
        if xyz.dtype == np.float32:
            x = np.ascontiguousarray(xyz)
            dt = L.PTL_F32
        else:
            x = L.as_f64(xyz)
            dt = L.PTL_F64
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError("xyz must be (N, 3)")
        t = None if t01 is None else L.as_f64(t01)
        if t is not None and len(t) != len(x):
            raise ValueError("t01 must have one entry per point")
        g = None if guess is None else L.as_f64(guess).reshape(16)
        out = np.empty((4, 4))
        st = L.IcpStats()
        L.check(L.lib().ptl_icp_register_frame(self._h, x.ctypes.data_as(C.c_void_p), dt, len(x),
                                               None if t is None else L.dptr(t), float(scan_ts),
                                               None if g is None else L.dptr(g), L.dptr(out), C.byref(st)))
        self.stats.append(st.as_dict())
        return out

    def register_range(self, lut, range_mm, guess=None, scan_ts=0.0):
        """register a raw range image (H*W u32 mm); xyz, the RANGE != 0 mask and column times happen on device"""
        r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
        if r.size != lut.H * lut.W:
            raise ValueError("range image size mismatch")
        g = None if guess is None else L.as_f64(guess).reshape(16)
        out = np.empty((4, 4))
        st = L.IcpStats()
        L.check(L.lib().ptl_icp_register_range(self._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               float(scan_ts), None if g is None else L.dptr(g), L.dptr(out),
                                               C.byref(st)))
        self.stats.append(st.as_dict())
        return out

    def set_active_beams(self, H, beams_num):
        L.check(L.lib().ptl_icp_set_active_beams(self._h, int(H), int(beams_num)))

    @property
    def num_poses(self):
        n = C.c_int64()
        L.check(L.lib().ptl_icp_num_poses(self._h, C.byref(n)))
        return n.value

    def poses(self):
        n = self.num_poses
        out = np.empty((max(n, 1), 4, 4))
        w = C.c_int64()
        L.check(L.lib().ptl_icp_get_poses(self._h, L.dptr(out), n, C.byref(w)))
        return out[:w.value]

    def prediction(self):
        out = np.empty((4, 4))
        L.check(L.lib().ptl_icp_get_prediction(self._h, L.dptr(out)))
        return out

    def map_size(self):
        v, p = C.c_int64(), C.c_int64()
        L.check(L.lib().ptl_icp_map_size(self._h, C.byref(v), C.byref(p)))
        return v.value, p.value

    def map_points(self):
        _, p = self.map_size()
        out = np.empty((max(p, 1), 3))
        w = C.c_int64()
        L.check(L.lib().ptl_icp_map_points(self._h, L.dptr(out), p, C.byref(w)))
        return out[:w.value]

    def map_score(self, radius=None, min_neighbours=5, sigma_floor=None, per_point=False):
        """sharpness of the stored map without ground truth (include/ptudes_mi.h ptl_icp_map_score): a `MapScore`; with
        per_point also (xyz (N, 3), n (N,) int32, plane_var (N,), entropy (N,)) of every stored point in one common order (sparse points:
        NaN).  radius defaults to the voxel size (its upper bound), sigma_floor to voxel size / 100"""
        cfg = L.MapScoreCfg()
        L.check(L.lib().ptl_map_score_default_cfg(C.byref(cfg), float(self.cfg.voxel_size)))
        if radius is not None:
            cfg.radius = float(radius)
        cfg.min_neighbours = int(min_neighbours)
        if sigma_floor is not None:
            cfg.sigma_floor = float(sigma_floor)
        res = L.MapScoreResult()
        if not per_point:
            L.check(L.lib().ptl_icp_map_score(self._h, C.byref(cfg), C.byref(res), None, None, None, None, 0, None))
            return MapScore(*(getattr(res, k) for k, _ in res._fields_))
        _, p = self.map_size()
        xyz, n, pv, ent = np.empty((max(p, 1), 3)), np.empty(max(p, 1), dtype=np.int32), np.empty(max(p, 1)), np.empty(max(p, 1))
        w = C.c_int64()
        L.check(L.lib().ptl_icp_map_score(self._h, C.byref(cfg), C.byref(res), L.dptr(xyz), n.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(pv),
                                          L.dptr(ent), p, C.byref(w)))
        k = w.value
        return MapScore(*(getattr(res, f) for f, _ in res._fields_)), (xyz[:k], n[:k], pv[:k], ent[:k])

    def map_distance(self, points, max_dist=None, thresholds=None, per_point=False):
        """nearest-neighbour distance of `points` (N, 3) to this map's stored points (include/ptudes_mi.h ptl_icp_map_distance, DESIGN.md
        3.23): a `MapDistance`; with per_point also d2 (N,) in query order - the squared distance of a matched query, +inf for an unmatched
        one, NaN for a non-finite one.  max_dist defaults to the voxel size (its upper bound), thresholds to (max_dist,)"""
        cfg = map_cmp_cfg(self.cfg.voxel_size, max_dist, thresholds)
        q = L.as_f64(points).reshape(-1, 3)
        res = L.MapCmpResult()
        d2 = np.empty(len(q)) if per_point else None
        L.check(L.lib().ptl_icp_map_distance(self._h, C.byref(cfg), L.dptr(q) if len(q) else None, len(q), C.byref(res),
                                             None if d2 is None else L.dptr(d2)))
        return (MapDistance._from(res), d2) if per_point else MapDistance._from(res)

    def map_compare(self, src_icp, max_dist=None, thresholds=None, per_point=False):
        """the same with the stored points of `src_icp`'s map as the queries, walked on the device: nothing but the summary crosses the bus
        (ptl_icp_map_compare).  With per_point also (xyz (N, 3), d2 (N,)) of src's stored points in its pool order"""
        cfg = map_cmp_cfg(self.cfg.voxel_size, max_dist, thresholds)
        res = L.MapCmpResult()
        if not per_point:
            L.check(L.lib().ptl_icp_map_compare(self._h, src_icp._h, C.byref(cfg), C.byref(res), None, None, 0, None))
            return MapDistance._from(res)
        _, p = src_icp.map_size()
        xyz, d2 = np.empty((max(p, 1), 3)), np.empty(max(p, 1))
        w = C.c_int64()
        L.check(L.lib().ptl_icp_map_compare(self._h, src_icp._h, C.byref(cfg), C.byref(res), L.dptr(xyz), L.dptr(d2), p, C.byref(w)))
        return MapDistance._from(res), (xyz[:w.value], d2[:w.value])

    def pose_hits(self, points, poses, max_dist=None, thresholds=None, per_pose=True):
        """how many of `points` (N, 3), sensor frame, lie within each threshold of this map's stored points when posed by each of `poses`
        (K, 4, 4) (include/ptudes_mi.h ptl_icp_pose_hits): a `PoseHits`; with per_pose also the (K, T) int32 counts, -1 in the
        row of a candidate with a non-finite entry.  max_dist defaults to the voxel size (its upper bound), thresholds to (max_dist,)"""
        cfg = pose_search_cfg(self.cfg.voxel_size, max_dist, thresholds)
        q = L.as_f64(points).reshape(-1, 3)
        p = L.as_f64(poses).reshape(-1, 16)
        res = L.PoseSearchResult()
        hits = np.empty((len(p), max(0, min(int(cfg.n_thresholds), 4))), dtype=np.int32) if per_pose else None
        L.check(L.lib().ptl_icp_pose_hits(self._h, C.byref(cfg), L.dptr(q) if len(q) else None, len(q), L.dptr(p) if len(p) else None, len(p),
                                          C.byref(res), None if hits is None else hits.ctypes.data_as(C.POINTER(C.c_int32))))
        return (PoseHits._from(res), hits) if per_pose else PoseHits._from(res)

    def _cloud(self, fn):
        cap = int(self.cfg.max_points_per_scan)
        out = np.empty((cap, 3))
        w = C.c_int64()
        L.check(fn(self._h, L.dptr(out), cap, C.byref(w)))
        return out[:w.value].copy()

    def last_frame_down(self):
        return self._cloud(L.lib().ptl_icp_last_frame_down)

    def last_source(self):
        return self._cloud(L.lib().ptl_icp_last_source)

    def deskew_modes(self):
        """deskew mode per registered scan (0 none, 1 constant velocity, 2 IMU); include/ptudes_mi.h ptl_icp_deskew_modes"""
        return _modes(self.num_poses, lambda p, m, w: L.lib().ptl_icp_deskew_modes(self._h, p, m, w))

    def column_table(self):
        """the current per-column deskew table as (W, 4, 4) transforms"""
        W = self.cfg.scan_cols
        raw = np.empty(12 * W)
        L.check(L.lib().ptl_icp_column_table(self._h, L.dptr(raw)))
        raw = raw.reshape(12, W)
        T = np.tile(np.eye(4), (W, 1, 1))
        T[:, :3, :3] = raw[:9].T.reshape(W, 3, 3)
        T[:, :3, 3] = raw[9:].T
        return T

    def deskew(self, xyz, t01):
        x, t = L.as_f64(xyz), L.as_f64(t01)
        out = np.empty_like(x)
        L.check(L.lib().ptl_icp_deskew(self._h, L.dptr(x), L.dptr(t), len(x), L.dptr(out)))
        return out

    # stage-level entry points (teacher-forced parity)
    def map_add(self, xyz_world, origin=None):
        x = L.as_f64(xyz_world)
        o = None if origin is None else L.as_f64(origin)
        L.check(L.lib().ptl_icp_map_add(self._h, L.dptr(x), len(x), None if o is None else L.dptr(o),
                                        0 if o is None else 1))

    def map_add_posed(self, traj, col_ts, range_mm=None, lut=None, xyz=None, H=None):
        """one posed scan into the map, on the device (include/ptudes_mi.h ptl_icp_map_add_posed_*): every column gets its pose on `traj`
        at col_ts (W seconds), the sweep - a range image with its `lut`, or (H, W, 3) f32 `xyz` in the sensor frame with (0,0,0) = no
        return - is de-warped and its returns are added in scan order.  Returns (n_valid, skipped): a scan with a column outside the
        trajectory's bounds adds nothing"""
        t = L.as_f64(col_ts).reshape(-1)
        nv, sk = C.c_int64(), C.c_int32()
        if (range_mm is None) == (xyz is None):
            raise ValueError("give range_mm (with lut) or xyz")
        if range_mm is not None:
            if lut is None:
                raise ValueError("a range image needs its lut")
            r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
            if r.size != lut.H * lut.W or len(t) != lut.W:
                raise ValueError("need an H x W range image and one time per column")
            L.check(L.lib().ptl_icp_map_add_posed_range(self._h, traj._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), L.dptr(t),
                                                        C.byref(nv), C.byref(sk)))
        else:
            x = np.ascontiguousarray(xyz, dtype=np.float32)
            W = len(t)
            H = int(H) if H is not None else x.size // (3 * max(W, 1))
            if x.size != H * W * 3:
                raise ValueError("need H x W x 3 points and one time per column")
            L.check(L.lib().ptl_icp_map_add_posed_xyz(self._h, traj._h, x.ctypes.data_as(C.POINTER(C.c_float)), H, W, L.dptr(t),
                                                      C.byref(nv), C.byref(sk)))
        return nv.value, bool(sk.value)

    def linear_system(self, src_world, max_dist, kernel):
        s = L.as_f64(src_world)
        sums = np.empty(27)
        nc, cand = C.c_int64(), C.c_int64()
        L.check(L.lib().ptl_icp_linear_system(self._h, L.dptr(s), len(s), max_dist, kernel, L.dptr(sums),
                                              C.byref(nc), C.byref(cand)))
        return sums, nc.value, cand.value

    def diag(self):
        return _diag(self._h)

    def align(self, frame, guess, max_dist, kernel):
        f = L.as_f64(frame)
        g = L.as_f64(guess).reshape(16)
        out = np.empty((4, 4))
        it = C.c_int32()
        L.check(L.lib().ptl_icp_align(self._h, L.dptr(f), len(f), L.dptr(g), max_dist, kernel, L.dptr(out),
                                      C.byref(it)))
        return out, it.value


class Lut:
    """range image -> xyz on device (ouster client.XYZLut equivalent, reference kiss.py:28-29)"""

    def __init__(self, H, W, beam_altitude_deg, beam_azimuth_deg, lidar_origin_to_beam_origin_mm=0.0,
                 lidar_to_sensor_mm=None, extrinsic_m=None, device_id=0):
        self.H, self.W = int(H), int(W)
        alt, az = L.as_f64(beam_altitude_deg), L.as_f64(beam_azimuth_deg)
        if len(alt) != H or len(az) != H:
            raise ValueError("need one altitude / azimuth angle per row")
        T = L.as_f64(np.eye(4) if lidar_to_sensor_mm is None else lidar_to_sensor_mm).reshape(16)
        E = None if extrinsic_m is None else L.as_f64(extrinsic_m).reshape(16)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_lut_create(device_id, self.H, self.W, L.dptr(alt), L.dptr(az),
                                       float(lidar_origin_to_beam_origin_mm), L.dptr(T),
                                       None if E is None else L.dptr(E), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_lut_destroy(self._h)
            self._h = None

    __del__ = close

    def __call__(self, range_mm):
        r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
        if r.size != self.H * self.W:
            raise ValueError("range image size mismatch")
        out = np.empty((self.H * self.W, 3))
        L.check(L.lib().ptl_lut_apply(self._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), L.dptr(out)))
        return out


    def dewarp(self, range_mm, col_poses):
        """client.dewarp(XYZLut(scan), column_poses=scan.pose): (H*W, 3) world xyz and the number of returns"""
        r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
        P = L.as_f64(col_poses).reshape(-1, 16)
        if r.size != self.H * self.W or len(P) != self.W:
            raise ValueError("need an H x W range image and one 4x4 pose per column")
        out = np.empty((self.H * self.W, 3))
        nv = C.c_int64()
        L.check(L.lib().ptl_lut_dewarp(self._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), L.dptr(P), L.dptr(out), C.byref(nv)))
        return out, nv.value


def traj_poses_at(knot_ts, knot_poses, ts, bound_before=0.0, bound_after=0.0, device_id=0):
    """TrajectoryEvaluator.poses_at on device: (n, 4, 4) poses and the number of timestamps outside the bounds"""
    kt, kp, t = L.as_f64(knot_ts), L.as_f64(knot_poses).reshape(-1, 16), L.as_f64(ts).reshape(-1)
    if len(kt) != len(kp):
        raise ValueError("one pose per knot timestamp")
    out = np.empty((len(t), 4, 4))
    nout = C.c_int64()
    L.check(L.lib().ptl_traj_poses_at(device_id, L.dptr(kt), L.dptr(kp), len(kt), float(bound_before), float(bound_after),
                                      L.dptr(t), len(t), L.dptr(out), C.byref(nout)))
    return out, nout.value


class Traj:
    """A time-stamped trajectory resident on a device (include/ptudes_mi.h ptl_traj): knots (ts, 4x4 pose), the end segments extended by
    bound_before / bound_after seconds - TrajectoryEvaluator's knots kept in HBM for the posed-scan entry points"""

    def __init__(self, knot_ts, knot_poses, bound_before=0.0, bound_after=0.0, device_id=0):
        kt, kp = L.as_f64(knot_ts).reshape(-1), L.as_f64(knot_poses).reshape(-1, 16)
        if len(kt) != len(kp):
            raise ValueError("one pose per knot timestamp")
        self.n_knots, self.bounds, self.device_id = len(kt), (float(bound_before), float(bound_after)), int(device_id)
        self.t_first = float(kt[0]) if len(kt) else 0.0
        self._h = C.c_void_p()
        L.check(L.lib().ptl_traj_create(int(device_id), L.dptr(kt), L.dptr(kp), len(kt), float(bound_before), float(bound_after),
                                        C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_traj_destroy(self._h)
            self._h = None

    __del__ = close


def carve_dynamic(through, support, min_through=2, min_fraction=0.5):
    """HOST POLICY on the two counts of `Carver.votes()`, not part of the library's definition: a stored point counts as a moving object's
    when at least min_through rays went through it and they are at least min_fraction of the rays that met it,
    (through >= min_through) & (through >= min_fraction * (through + support)).  Returns a bool mask"""
    t, s = np.asarray(through, dtype=np.int64), np.asarray(support, dtype=np.int64)
    return (t >= int(min_through)) & (t >= float(min_fraction) * (t + s))


@dataclass
class CarveVotes:
    """What `Carver.votes()` returns (include/ptudes_mi.h ptl_carve_result): every stored point of the map in pool order with
    the rays that went through it and the rays that ended at it, and the summary - counts (all exact), the parameters as used, the HIP-event
    time of the handle's device work so far"""
    xyz: np.ndarray        # (N, 3)
    through: np.ndarray    # (N,) uint32
    support: np.ndarray    # (N,) uint32
    n_points: int
    n_scans: int
    n_scans_skipped: int
    n_rays: int
    n_rays_out_of_range: int
    n_no_return: int
    n_voxel_visits: int
    n_points_through: int
    n_points_supported: int
    sum_through: int
    sum_support: int
    radius: float
    margin: float
    step: float
    min_range: float
    max_range: float
    device_ms: float

    def dynamic(self, min_through=2, min_fraction=0.5):
        """`carve_dynamic` of these votes: host policy, not the library's"""
        return carve_dynamic(self.through, self.support, min_through, min_fraction)

    def lines(self, min_through=2, min_fraction=0.5):
        """the block the commands print"""
        n_dyn = int(self.dynamic(min_through, min_fraction).sum())
        return [f"carve: radius {self.radius:g} m, margin {self.margin:g} m, step {self.step:g} m, range [{self.min_range:g}, {self.max_range:g}] m",
                f"  sweeps: {self.n_scans} (skipped {self.n_scans_skipped}), rays {self.n_rays} (out of range {self.n_rays_out_of_range}, "
                f"no return {self.n_no_return}), voxel visits {self.n_voxel_visits}",
                f"  points: {self.n_points} (passed through {self.n_points_through}, supported {self.n_points_supported}), "
                f"votes through {self.sum_through}, support {self.sum_support}",
                f"  dynamic (through >= {int(min_through)}, fraction >= {float(min_fraction):g}): {n_dyn} points"]


def carve_cfg(voxel_size, radius=None, margin=None, step=None, min_range=None, max_range=None):
    """the _lib.CarveCfg of a map of that voxel size: the library's defaults with the given fields on top"""
    cfg = L.CarveCfg()
    L.check(L.lib().ptl_carve_default_cfg(C.byref(cfg), float(voxel_size)))
    for k, v in (("radius", radius), ("margin", margin), ("step", step), ("min_range", min_range), ("max_range", max_range)):
        if v is not None:
            setattr(cfg, k, float(v))
    return cfg


class Carver:
    """Free space carved (include/ptudes_mi.h ptl_carve_*): a second pass over the sweeps that built `map_icp`'s map, posed by
    the same trajectory, counts for every stored point the rays that went through it and the rays that ended at it.  The map is only read and
    must not be updated (nor closed) while the carver lives: a map updated since gives a RuntimeError at the next add or read"""

    def __init__(self, map_icp, radius=None, margin=None, step=None, min_range=None, max_range=None):
        self.map_icp = map_icp
        self.cfg = carve_cfg(map_icp.cfg.voxel_size, radius, margin, step, min_range, max_range)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_carve_create(map_icp._h, C.byref(self.cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_carve_destroy(self._h)
            self._h = None

    __del__ = close

    def add_posed(self, traj, col_ts, range_mm=None, lut=None, xyz=None, H=None):
        """one posed sweep, with the arguments of `Icp.map_add_posed`.  Returns (n_rays, skipped): the sweep's used rays; a sweep with a
        column outside the trajectory's bounds is skipped as a whole"""
        t = L.as_f64(col_ts).reshape(-1)
        nv, sk = C.c_int64(), C.c_int32()
        if (range_mm is None) == (xyz is None):
            raise ValueError("give range_mm (with lut) or xyz")
        if range_mm is not None:
            if lut is None:
                raise ValueError("a range image needs its lut")
            r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
            if r.size != lut.H * lut.W or len(t) != lut.W:
                raise ValueError("need an H x W range image and one time per column")
            L.check(L.lib().ptl_carve_add_posed_range(self._h, traj._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), L.dptr(t),
                                                      C.byref(nv), C.byref(sk)))
        else:
            x = np.ascontiguousarray(xyz, dtype=np.float32)
            W = len(t)
            H = int(H) if H is not None else x.size // (3 * max(W, 1))
            if x.size != H * W * 3:
                raise ValueError("need H x W x 3 points and one time per column")
            L.check(L.lib().ptl_carve_add_posed_xyz(self._h, traj._h, x.ctypes.data_as(C.POINTER(C.c_float)), H, W, L.dptr(t),
                                                    C.byref(nv), C.byref(sk)))
        return nv.value, bool(sk.value)

    def add_run(self, runner, traj, t0t1, s=None, first=0, last=None):
        """the RESIDENT sweeps [first, last] of a SeqRunner (s=None) or of sequence s of a BatchRunner, as `build_map` takes them: no sweep
        crosses the bus.  Returns (n_rays, n_skipped)"""
        t = _sweep_times(t0t1, runner.n_scans)
        last = runner.n_scans - 1 if last is None else int(last)
        nv, ns = C.c_int64(), C.c_int64()
        if s is None:
            L.check(L.lib().ptl_carve_add_seq(self._h, runner._h, traj._h, L.dptr(t), int(first), last, C.byref(nv), C.byref(ns)))
        else:
            L.check(L.lib().ptl_carve_add_batch(self._h, runner._h, int(s), traj._h, L.dptr(t), int(first), last, C.byref(nv), C.byref(ns)))
        return nv.value, ns.value

    def votes(self):
        """a `CarveVotes` of the sweeps added so far; more may be added and read again"""
        _, p = self.map_icp.map_size()
        xyz, thr, sup = np.empty((max(p, 1), 3)), np.zeros(max(p, 1), dtype=np.uint32), np.zeros(max(p, 1), dtype=np.uint32)
        res, w = L.CarveResult(), C.c_int64()
        u32p = C.POINTER(C.c_uint32)
        L.check(L.lib().ptl_carve_read(self._h, C.byref(res), L.dptr(xyz), thr.ctypes.data_as(u32p), sup.ctypes.data_as(u32p), p, C.byref(w)))
        k = w.value
        vals = [getattr(res, f) for f, _ in res._fields_]
        return CarveVotes(xyz[:k].copy(), thr[:k].copy(), sup[:k].copy(), *(int(v) for v in vals[:11]), *(float(v) for v in vals[11:]))


CAST_NONE, CAST_HIT, CAST_MISS, CAST_DEGENERATE = 0, 1, 2, 3                      # pixel status of a cast (include/ptudes_mi.h)
CHANGE_NONE, CHANGE_AGREE, CHANGE_NEW, CHANGE_GONE, CHANGE_UNMAPPED = 0, 1, 2, 3, 4  # classes of `cast_changes`
CHANGE_NAMES = ("none", "agree", "new", "gone", "unmapped")


def cast_changes(status, t_hit, length, margin):
    """HOST POLICY on the outputs of a cast, not part of the library's definition: a u8 class per pixel.  For a hit (status 1):
    AGREE |len - t_hit| <= margin, NEW len < t_hit - margin (the sweep ends in front of what the map holds), GONE len > t_hit + margin (the
    sweep goes on behind it); UNMAPPED a return that marched to max_range without a hit (status 2); NONE everything else - no return, or a
    degenerate one: nothing to say"""
    st, t, ln = np.asarray(status), np.asarray(t_hit, dtype=np.float64), np.asarray(length, dtype=np.float64)
    m = float(margin)
    if not m >= 0.0:
        raise ValueError(f"margin = {margin}: must be >= 0")
    out = np.full(st.shape, CHANGE_NONE, dtype=np.uint8)
    hit = st == CAST_HIT
    with np.errstate(invalid="ignore"):
        out[hit & (np.abs(ln - t) <= m)] = CHANGE_AGREE
        out[hit & (ln < t - m)] = CHANGE_NEW
        out[hit & (ln > t + m)] = CHANGE_GONE
    out[st == CAST_MISS] = CHANGE_UNMAPPED
    return out


@dataclass
class CastSweep:
    """What `Caster.cast_range` / `cast_xyz` return (include/ptudes_mi.h ptl_cast_result): per pixel (H, W) the status, the
    hit's distance along the ray (-1 unless a hit), the measured length (-1 unless a return) and the hit point's index in pool order (-1 unless
    a hit: a row of `Caster.points()` and of every per-point array in pool order); `result` the counts and the parameters as used"""
    status: np.ndarray   # (H, W) uint8
    t_hit: np.ndarray    # (H, W) float64
    len: np.ndarray      # (H, W) float64
    index: np.ndarray    # (H, W) int32
    result: dict
    voxel_size: float = 0.0

    def changes(self, margin=None):
        """`cast_changes` of this sweep (default margin: the map's voxel size, untuned): host policy, not the library's"""
        return cast_changes(self.status, self.t_hit, self.len, self.voxel_size if margin is None else margin)

    def expected_range_mm(self):
        """the range image the map predicts: t_hit in mm rounded to u32, 0 where there is no hit"""
        hit = self.status == CAST_HIT
        return np.where(hit, np.rint(np.where(hit, self.t_hit, 0.0) * 1000.0), 0.0).astype(np.uint32)

    def gather(self, values, fill=0):
        """per-pixel values of a per-point array in pool order (e.g. `PaintValues.mean()`): values[index] where there is a hit, else `fill`"""
        v = np.asarray(values)
        hit = self.index >= 0
        if hit.any() and int(self.index.max()) >= len(v):
            raise ValueError(f"a hit points at stored point {int(self.index.max())}, `values` has {len(v)} rows: not this map's pool order")
        out = np.empty(self.index.shape + v.shape[1:], dtype=np.result_type(v.dtype, np.asarray(fill).dtype))
        out[...] = fill
        out[hit] = v[self.index[hit]]
        return out


def change_counts(classes):
    """{name: pixels} of a class image of `cast_changes`"""
    n = np.bincount(np.asarray(classes, dtype=np.uint8).reshape(-1), minlength=len(CHANGE_NAMES))
    return {name: int(n[i]) for i, name in enumerate(CHANGE_NAMES)}


def cast_cfg(voxel_size, radius=None, step=None, min_range=None, max_range=None):
    """the _lib.CastCfg of a map of that voxel size: the library's defaults with the given fields on top"""
    cfg = L.CastCfg()
    L.check(L.lib().ptl_cast_default_cfg(C.byref(cfg), float(voxel_size)))
    for k, v in (("radius", radius), ("step", step), ("min_range", min_range), ("max_range", max_range)):
        if v is not None:
            setattr(cfg, k, float(v))
    return cfg


class Caster:
    """A sweep's rays cast through `map_icp`'s map (include/ptudes_mi.h ptl_cast_*): per pixel of a posed sweep the first
    stored point along the pixel's ray.  The map is only read and must not be updated (nor closed) while the caster lives: a map updated since
    gives a RuntimeError at the next call"""

    def __init__(self, map_icp, radius=None, step=None, min_range=None, max_range=None):
        self.map_icp = map_icp
        self.cfg = cast_cfg(map_icp.cfg.voxel_size, radius, step, min_range, max_range)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_cast_create(map_icp._h, C.byref(self.cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_cast_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _col_ts(traj, col_ts, W):
        """one time per column; None: every column at the trajectory's first knot time (a pose held still)"""
        return np.full(W, traj.t_first) if col_ts is None else L.as_f64(col_ts).reshape(-1)

    def _cast(self, H, W, call):
        st, t, ln, ix = np.zeros((H, W), dtype=np.uint8), np.empty((H, W)), np.empty((H, W)), np.empty((H, W), dtype=np.int32)
        res = L.CastResult()
        L.check(call(C.byref(res), st.ctypes.data_as(C.POINTER(C.c_uint8)), L.dptr(t), L.dptr(ln), ix.ctypes.data_as(C.POINTER(C.c_int32))))
        out = {f: getattr(res, f) for f, _ in res._fields_ if f != "reserved"}
        out["skipped"] = bool(out["skipped"])
        return CastSweep(st, t, ln, ix, out, float(self.map_icp.cfg.voxel_size))

    def cast_range(self, traj, lut, range_mm, col_ts=None):
        """one posed range image (H x W u32 mm, 0 = no return) of `lut`; col_ts one time per column (None: every column at the trajectory's
        first knot time) - returns a `CastSweep`"""
        r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
        t = self._col_ts(traj, col_ts, lut.W)
        if r.size != lut.H * lut.W or len(t) != lut.W:
            raise ValueError("need an H x W range image and one time per column")
        return self._cast(lut.H, lut.W, lambda *out: L.lib().ptl_cast_posed_range(self._h, traj._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                                   L.dptr(t), *out))

    def cast_xyz(self, traj, xyz, H, W, col_ts=None):
        """one posed sweep of H x W f32 points in the sensor frame, (0, 0, 0) = no return - returns a `CastSweep`"""
        x = np.ascontiguousarray(xyz, dtype=np.float32)
        H, W = int(H), int(W)
        t = self._col_ts(traj, col_ts, W)
        if x.size != H * W * 3 or len(t) != W:
            raise ValueError("need H x W x 3 points and one time per column")
        return self._cast(max(H, 1), max(W, 1), lambda *out: L.lib().ptl_cast_posed_xyz(self._h, traj._h, x.ctypes.data_as(C.POINTER(C.c_float)), H, W,
                                                                                        L.dptr(t), *out))

    def expected(self, traj, lut, col_ts=None, ref_range=None):
        """the VIRTUAL SWEEP the map predicts at the trajectory's poses: `cast_range` of a constant range image of `ref_range` mm (default
        max_range), so that every pixel of the LUT is cast; `expected_range_mm()` of the result is the predicted range image"""
        ref = int(round(self.cfg.max_range * 1000.0)) if ref_range is None else int(ref_range)
        if not 0 < ref < 1 << 32:
            raise ValueError(f"ref_range = {ref} mm: must be a positive u32")
        return self.cast_range(traj, lut, np.full((lut.H, lut.W), ref, dtype=np.uint32), col_ts)

    def points(self):
        """the map's stored points (N, 3) in pool order: `CastSweep.index` points into them"""
        _, p = self.map_icp.map_size()
        xyz, w = np.empty((max(p, 1), 3)), C.c_int64()
        L.check(L.lib().ptl_cast_points(self._h, L.dptr(xyz), p, C.byref(w)))
        return xyz[:w.value].copy()


@dataclass
class PaintValues:
    """What `Painter.values()` returns (include/ptudes_mi.h ptl_paint_result): every stored point of the map in pool order
    with the sum of the field values of the rays that ended at it and their number, and the summary - a `_lib.PaintResult`, all counts exact"""
    xyz: np.ndarray      # (N, 3)
    sum: np.ndarray      # (N,) uint64
    count: np.ndarray    # (N,) uint32
    result: object

    def mean(self):
        """fp64 sum / count per stored point, NaN where no ray ended at the point"""
        out = np.full(len(self.count), np.nan)
        hit = self.count > 0
        out[hit] = self.sum[hit].astype(np.float64) / self.count[hit].astype(np.float64)
        return out

    def lines(self):
        """the block the commands print"""
        r = self.result
        return [f"paint: sweeps {r.n_scans} (skipped {r.n_scans_skipped}), rays matched {r.n_rays_matched}, unmatched {r.n_rays_unmatched}, "
                f"no return {r.n_no_return}",
                f"  points: {r.n_points} (painted {r.n_points_painted}), values added {r.sum_count}"]


class Painter:
    """The map painted (include/ptudes_mi.h ptl_paint_*): a second pass over the sweeps that built `map_icp`'s map, posed by
    the same trajectory, each with a field image (H, W) uint32, sums for every stored point the field values of the rays that ended at it.
    The map is only read and must not be updated (nor closed) while the painter lives: a map updated since gives a RuntimeError at the next
    add or read"""

    def __init__(self, map_icp):
        self.map_icp = map_icp
        self._h = C.c_void_p()
        L.check(L.lib().ptl_paint_create(map_icp._h, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_paint_destroy(self._h)
            self._h = None

    __del__ = close

    def add_posed(self, traj, col_ts, field, range_mm=None, lut=None, xyz=None, H=None):
        """one posed sweep, with the arguments of `Icp.map_add_posed`, and its field image.  Returns (n_matched, skipped): the sweep's rays
        that ended at a stored point; a sweep with a column outside the trajectory's bounds is skipped as a whole"""
        t = L.as_f64(col_ts).reshape(-1)
        f = np.ascontiguousarray(field, dtype=np.uint32).reshape(-1)
        nv, sk = C.c_int64(), C.c_int32()
        u32p = C.POINTER(C.c_uint32)
        if (range_mm is None) == (xyz is None):
            raise ValueError("give range_mm (with lut) or xyz")
        if range_mm is not None:
            if lut is None:
                raise ValueError("a range image needs its lut")
            r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
            if r.size != lut.H * lut.W or len(t) != lut.W or f.size != r.size:
                raise ValueError("need an H x W range image, an H x W field image and one time per column")
            L.check(L.lib().ptl_paint_add_posed_range(self._h, traj._h, lut._h, r.ctypes.data_as(u32p), f.ctypes.data_as(u32p), L.dptr(t),
                                                      C.byref(nv), C.byref(sk)))
        else:
            x = np.ascontiguousarray(xyz, dtype=np.float32)
            W = len(t)
            H = int(H) if H is not None else x.size // (3 * max(W, 1))
            if x.size != H * W * 3 or f.size != H * W:
                raise ValueError("need H x W x 3 points, an H x W field image and one time per column")
            L.check(L.lib().ptl_paint_add_posed_xyz(self._h, traj._h, x.ctypes.data_as(C.POINTER(C.c_float)), f.ctypes.data_as(u32p), H, W,
                                                    L.dptr(t), C.byref(nv), C.byref(sk)))
        return nv.value, bool(sk.value)

    def values(self):
        """a `PaintValues` of the sweeps added so far; more may be added and read again"""
        _, p = self.map_icp.map_size()
        xyz, s, k = np.empty((max(p, 1), 3)), np.zeros(max(p, 1), dtype=np.uint64), np.zeros(max(p, 1), dtype=np.uint32)
        res, w = L.PaintResult(), C.c_int64()
        L.check(L.lib().ptl_paint_read(self._h, C.byref(res), L.dptr(xyz), s.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       k.ctypes.data_as(C.POINTER(C.c_uint32)), p, C.byref(w)))
        n = w.value
        return PaintValues(xyz[:n].copy(), s[:n].copy(), k[:n].copy(), res)


GRID_FREE, GRID_OCCUPIED, GRID_UNKNOWN = 0, 1, 2  # the classes of `grid_classify`
GRID_MAX_CELLS = 1 << 26


def grid_classify(free, hit, min_hits=2, min_fraction=0.25, min_free=1):
    """HOST POLICY on the two counts of `OccupancyGrid.read()`, not part of the library's definition, and its defaults are UNTUNED (nobody has
    run this on a real recording): a cell is occupied (GRID_OCCUPIED) iff hit >= min_hits and hit >= min_fraction * (hit + free); else free
    (GRID_FREE) iff free >= min_free; else unknown (GRID_UNKNOWN).  Returns a uint8 array of the counts' shape"""
    f, h = np.asarray(free, dtype=np.int64), np.asarray(hit, dtype=np.int64)
    occ = (h >= int(min_hits)) & (h >= float(min_fraction) * (h + f))
    out = np.full(f.shape, GRID_UNKNOWN, dtype=np.uint8)
    out[f >= int(min_free)] = GRID_FREE
    out[occ] = GRID_OCCUPIED
    return out


@dataclass
class GridCounts:
    """What `OccupancyGrid.read()` returns (include/ptudes_mi.h ptl_grid_result): the counts of a rectangle of cells, row-major
    (h, w) with ix along the columns - free[j, i] is cell (ix0 + i, iy0 + j) -, the cell size, the world coordinates of the rectangle's own
    corner, and the summary of the WHOLE grid (a `_lib.GridResult`, all counts exact)"""
    free: np.ndarray       # (h, w) uint32
    hit: np.ndarray        # (h, w) uint32
    cell: float
    origin: tuple          # (x, y) of the corner of free[0, 0]
    result: object

    def classify(self, min_hits=2, min_fraction=0.25, min_free=1):
        """`grid_classify` of these counts: host policy with untuned defaults, not the library's"""
        return grid_classify(self.free, self.hit, min_hits, min_fraction, min_free)

    def lines(self, min_hits=2, min_fraction=0.25, min_free=1):
        """the block the commands print"""
        r = self.result
        cls = self.classify(min_hits, min_fraction, min_free)
        return [f"grid: {r.nx} x {r.ny} cells of {r.cell:g} m from ({r.x0:g}, {r.y0:g}), band [{r.z_lo:g}, {r.z_hi:g}] m, margin {r.margin:g} m, "
                f"step {r.step:g} m, range [{r.min_range:g}, {r.max_range:g}] m",
                f"  sweeps: {r.n_scans} (skipped {r.n_scans_skipped}), rays {r.n_rays} (out of range {r.n_rays_out_of_range}, "
                f"no return {r.n_no_return}, ends outside the grid {r.n_ends_outside})",
                f"  cells: crossed {r.n_cells_free}, hit {r.n_cells_hit}, votes free {r.sum_free}, hit {r.sum_hit}, "
                f"touched box [{r.box_ix0}, {r.box_ix1}] x [{r.box_iy0}, {r.box_iy1}]",
                f"  classes (hits >= {int(min_hits)}, fraction >= {float(min_fraction):g}, free >= {int(min_free)}; untuned): "
                f"free {int((cls == GRID_FREE).sum())}, occupied {int((cls == GRID_OCCUPIED).sum())}, unknown {int((cls == GRID_UNKNOWN).sum())} "
                f"of {cls.size} cells read"]


def grid_cfg(cell, x0, y0, nx, ny, scan_cols, max_pixels_per_scan, z_lo=None, z_hi=None, margin=None, step=None, min_range=None, max_range=None):
    """the _lib.GridCfg of a grid of that cell size: the library's defaults with the bounds, the staging sizes and the given fields on top"""
    cfg = L.GridCfg()
    L.check(L.lib().ptl_grid_default_cfg(C.byref(cfg), float(cell)))
    cfg.x0, cfg.y0, cfg.nx, cfg.ny = float(x0), float(y0), int(nx), int(ny)
    cfg.scan_cols, cfg.max_pixels_per_scan = int(scan_cols), int(max_pixels_per_scan)
    for k, v in (("z_lo", z_lo), ("z_hi", z_hi), ("margin", margin), ("step", step), ("min_range", min_range), ("max_range", max_range)):
        if v is not None:
            setattr(cfg, k, float(v))
    return cfg


class OccupancyGrid:
    """The occupancy grid of a run (include/ptudes_mi.h ptl_grid_*): a pass over the sweeps of a run, posed by its trajectory,
    counts for every cell of a top-down grid the rays that crossed it (free) and the rays that ended in it (hit).  No map is involved.
    The grid is nx x ny cells of `cell` metres with the corner of cell (0, 0) at (x0, y0); scan_cols and max_pixels_per_scan size the
    handle's staging (W of every sweep, the largest H W of a per-call sweep)"""

    def __init__(self, cell, x0, y0, nx, ny, scan_cols, max_pixels_per_scan, device_id=0, **cfg):
        self.cfg = grid_cfg(cell, x0, y0, nx, ny, scan_cols, max_pixels_per_scan, **cfg)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_grid_create(int(device_id), C.byref(self.cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_grid_destroy(self._h)
            self._h = None

    __del__ = close

    def add_posed(self, traj, col_ts, range_mm=None, lut=None, xyz=None, H=None):
        """one posed sweep, with the arguments of `Carver.add_posed`.  Returns (n_rays, skipped): the sweep's used rays; a sweep with a
        column outside the trajectory's bounds is skipped as a whole"""
        t = L.as_f64(col_ts).reshape(-1)
        nv, sk = C.c_int64(), C.c_int32()
        if (range_mm is None) == (xyz is None):
            raise ValueError("give range_mm (with lut) or xyz")
        if range_mm is not None:
            if lut is None:
                raise ValueError("a range image needs its lut")
            r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
            if r.size != lut.H * lut.W or len(t) != lut.W:
                raise ValueError("need an H x W range image and one time per column")
            L.check(L.lib().ptl_grid_add_posed_range(self._h, traj._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), L.dptr(t),
                                                     C.byref(nv), C.byref(sk)))
        else:
            x = np.ascontiguousarray(xyz, dtype=np.float32)
            W = len(t)
            H = int(H) if H is not None else x.size // (3 * max(W, 1))
            if x.size != H * W * 3:
                raise ValueError("need H x W x 3 points and one time per column")
            L.check(L.lib().ptl_grid_add_posed_xyz(self._h, traj._h, x.ctypes.data_as(C.POINTER(C.c_float)), H, W, L.dptr(t),
                                                   C.byref(nv), C.byref(sk)))
        return nv.value, bool(sk.value)

    def add_run(self, runner, traj, t0t1, s=None, first=0, last=None):
        """the RESIDENT sweeps [first, last] of a SeqRunner (s=None) or of sequence s of a BatchRunner, as `build_map` takes them: no sweep
        crosses the bus.  Returns (n_rays, n_skipped)"""
        t = _sweep_times(t0t1, runner.n_scans)
        last = runner.n_scans - 1 if last is None else int(last)
        nv, ns = C.c_int64(), C.c_int64()
        if s is None:
            L.check(L.lib().ptl_grid_add_seq(self._h, runner._h, traj._h, L.dptr(t), int(first), last, C.byref(nv), C.byref(ns)))
        else:
            L.check(L.lib().ptl_grid_add_batch(self._h, runner._h, int(s), traj._h, L.dptr(t), int(first), last, C.byref(nv), C.byref(ns)))
        return nv.value, ns.value

    def summary(self):
        """the `_lib.GridResult` of the sweeps added so far, without any cell"""
        res = L.GridResult()
        L.check(L.lib().ptl_grid_read(self._h, C.byref(res), 0, 0, 0, 0, None, None))
        return res

    def read(self, ix0=0, iy0=0, w=None, h=None):
        """a `GridCounts` of the rectangle of w x h cells at (ix0, iy0) (default: the whole grid) for the sweeps added so far; more may be
        added and read again"""
        w = self.cfg.nx - int(ix0) if w is None else int(w)
        h = self.cfg.ny - int(iy0) if h is None else int(h)
        shape = (h, w) if h >= 1 and w >= 1 else (1, 1)  # (an empty rectangle still reaches the library, which refuses it with the numbers)
        free, hit = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32)
        res = L.GridResult()
        u32p = C.POINTER(C.c_uint32)
        L.check(L.lib().ptl_grid_read(self._h, C.byref(res), int(ix0), int(iy0), w, h, free.ctypes.data_as(u32p), hit.ctypes.data_as(u32p)))
        return GridCounts(free, hit, float(res.cell), (res.x0 + int(ix0) * res.cell, res.y0 + int(iy0) * res.cell), res)

    def clear(self):
        """all counts and counters back to zero; the parameters stay"""
        L.check(L.lib().ptl_grid_clear(self._h))


def place_cfg(**over):
    """the _lib.PlaceCfg: the library's defaults (UNTUNED: nobody has run this on a real recording) with the given fields on top"""
    cfg = L.PlaceCfg()
    L.check(L.lib().ptl_place_default_cfg(C.byref(cfg)))
    for k, v in over.items():
        if k not in ("n_ring", "n_sector", "min_radius", "max_radius", "z_min", "z_step", "capacity", "max_points_per_scan"):
            raise ValueError(f"ptl_place_cfg has no field {k!r}")
        setattr(cfg, k, int(v) if k in ("n_ring", "n_sector", "capacity", "max_points_per_scan") else float(v))
    return cfg


def place_infos_array(infos):
    """ctypes array of _lib.PlaceInfo -> (n, 9) int64, columns `_lib.PLACE_INFO_FIELDS`"""
    return np.array([[getattr(i, k) for k in L.PLACE_INFO_FIELDS] for i in infos], dtype=np.int64).reshape(-1, len(L.PLACE_INFO_FIELDS))


@dataclass
class PlaceMatch:
    """What `PlaceIndex.match` returns: per entry of [first, last] its best shift and distance (exact integers), and the best entry (-1 for
    an empty range) by smallest distance, ties to the smaller index.  The rigid guess that takes the query's coordinates into entry c's frame
    is `place_shift_pose(shift[c - first], n_sector)`"""
    first: int
    dist: np.ndarray       # (n,) uint32
    shift: np.ndarray      # (n,) int32
    best_entry: int
    best_dist: int
    best_shift: int
    device_ms: float


@dataclass
class PlaceLoops:
    """What `PlaceIndex.match_all` returns: for query entry first + k the best earlier entry[k] (-1: none qualified) at least min_gap entries
    before it, with its distance and shift"""
    first: int
    min_gap: int
    entry: np.ndarray      # (n,) int32
    dist: np.ndarray       # (n,) uint32
    shift: np.ndarray      # (n,) int32
    n_compared: int
    device_ms: float


def place_shift_pose(shift, n_sector):
    """Rz(-2 pi shift / n_sector) as a 4x4: takes the coordinates of a query matched at `shift` into the entry's frame"""
    t = -2.0 * np.pi * float(shift) / float(n_sector)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    return T


class PlaceIndex:
    """Revisited places (include/ptudes_mi.h ptl_place_*): a database of polar height descriptors of sweeps on the device,
    compared with a query at every heading.  Every output is an exact integer function of the points and the stored bytes.  The defaults of
    the parameters are the library's and UNTUNED"""

    def __init__(self, device_id=0, **cfg):
        self.cfg = place_cfg(**cfg)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_place_create(int(device_id), C.byref(self.cfg), C.byref(self._h)))
        self.n_ring, self.n_sector = int(self.cfg.n_ring), int(self.cfg.n_sector)
        self.r_pad = (self.n_ring + 3) // 4 * 4

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_place_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        n = C.c_int64()
        L.check(L.lib().ptl_place_size(self._h, C.byref(n)))
        return int(n.value)

    def tables(self):
        """(ring_edge2 (R + 1,), sector_dir (S, 2)) as the device uses them: part of the input to the definition"""
        e, d = np.empty(self.n_ring + 1), np.empty((self.n_sector, 2))
        L.check(L.lib().ptl_place_tables(self._h, L.dptr(e), L.dptr(d)))
        return e, d

    def profile(self, reset=False):
        """(HIP-event ms of the describe calls so far, their number)"""
        ms, n = C.c_double(), C.c_int64()
        L.check(L.lib().ptl_place_profile(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def describe(self, points, rot=None, keep=True):
        """The descriptor of a sweep: `points` an (n, 3) float32 / float64 array in the sensor frame, or a pair (lut, range image).  rot: a
        3x3 that levels the sweep (p' = rot p).  The descriptor lands in the query slot and, with keep, behind the last entry.  Returns
        (index, _lib.PlaceInfo), index = -1 without keep; a full database raises (RuntimeError, the numbers in the text) and the query slot
        still holds the descriptor"""
        r9 = None if rot is None else L.as_f64(rot).reshape(9)
        idx, info = C.c_int64(-1), L.PlaceInfo()
        if isinstance(points, tuple):
            lut, rng = points
            r = np.ascontiguousarray(rng, dtype=np.uint32).reshape(-1)
            if r.size != lut.H * lut.W:
                raise ValueError("range image size mismatch")
            rc = L.lib().ptl_place_describe_range(self._h, lut._h, r.ctypes.data_as(C.POINTER(C.c_uint32)), None if r9 is None else L.dptr(r9),
                                                  1 if keep else 0, C.byref(idx), C.byref(info))
        else:
            x = np.asarray(points)
            x = np.ascontiguousarray(x, dtype=np.float32 if x.dtype == np.float32 else np.float64).reshape(-1, 3)
            rc = L.lib().ptl_place_describe_xyz(self._h, x.ctypes.data_as(C.c_void_p), L.PTL_F32 if x.dtype == np.float32 else L.PTL_F64, len(x),
                                                None if r9 is None else L.dptr(r9), 1 if keep else 0, C.byref(idx), C.byref(info))
        L.check(rc)
        return int(idx.value), info

    def match(self, query=-1, first=0, last=None):
        """`query` (an entry index, -1: the query slot) against every entry of [first, last] (default: all) at every shift: a `PlaceMatch`"""
        last = len(self) - 1 if last is None else int(last)
        n = max(last - int(first) + 1, 0)
        dist, shift, res = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32), L.PlaceResult()
        L.check(L.lib().ptl_place_match(self._h, int(query), int(first), last, dist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        shift.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res)))
        return PlaceMatch(int(first), dist, shift, int(res.best_entry), int(res.best_dist), int(res.best_shift), float(res.device_ms))

    def match_all(self, min_gap, first=0, last=None):
        """the loop-closure batch form: every entry of [first, last] (default: all) against the entries at least min_gap before it: a
        `PlaceLoops`"""
        last = len(self) - 1 if last is None else int(last)
        n = max(last - int(first) + 1, 0)
        entry, dist, shift = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        res = L.PlaceResult()
        L.check(L.lib().ptl_place_match_all(self._h, int(first), last, int(min_gap), entry.ctypes.data_as(C.POINTER(C.c_int32)),
                                            dist.ctypes.data_as(C.POINTER(C.c_uint32)), shift.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res)))
        return PlaceLoops(int(first), int(min_gap), entry, dist, shift, int(res.n_compared), float(res.device_ms))

    def descriptors(self, first=0, last=None):
        """(desc (n, S, Rpad) uint8, infos (n, 9) int64 with the columns `_lib.PLACE_INFO_FIELDS`) of the entries [first, last]"""
        last = len(self) - 1 if last is None else int(last)
        n = max(last - int(first) + 1, 0)
        desc = np.zeros((n, self.n_sector, self.r_pad), dtype=np.uint8)
        infos = (L.PlaceInfo * max(n, 1))()
        L.check(L.lib().ptl_place_read(self._h, int(first), last, desc.ctypes.data_as(C.POINTER(C.c_uint8)), infos))
        return desc, place_infos_array(infos[:n])

    def load(self, desc, infos):
        """appends stored descriptors (n, S, Rpad) uint8 with their infos (n, 9) int64; a non-zero pad byte is refused (ValueError)"""
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.ndim != 3 or d.shape[1:] != (self.n_sector, self.r_pad):
            raise ValueError(f"descriptors of shape {d.shape}: this index holds (n, {self.n_sector}, {self.r_pad})")
        a = np.ascontiguousarray(infos, dtype=np.int64).reshape(-1, len(L.PLACE_INFO_FIELDS))
        if len(a) != len(d):
            raise ValueError(f"{len(d)} descriptors with {len(a)} infos")
        L.check(L.lib().ptl_place_load(self._h, len(d), d.ctypes.data_as(C.POINTER(C.c_uint8)), a.ctypes.data_as(C.POINTER(L.PlaceInfo))))

    def clear(self):
        """no entries; parameters and tables stay"""
        L.check(L.lib().ptl_place_clear(self._h))


def rgba_word(rgba):
    """(..., 4) uint8 R, G, B, A -> the uint32 words the renderer's keys carry (R the lowest byte)"""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.shape[-1] != 4:
        raise ValueError("rgba needs four bytes per colour")
    return a.view("<u4").reshape(a.shape[:-1]).astype(np.uint32)


def default_palette():
    """(256, 4) uint8: the renderer's default ramp (include/ptudes_mi.h ptl_render_set_palette)"""
    i = np.arange(256)
    return np.stack([i, 255 - np.abs(2 * i - 255), 255 - i, np.full(256, 255)], axis=1).astype(np.uint8)


class Renderer:
    """Frames of a map drawn on the device (include/ptudes_mi.h ptl_render): point splats of point_px pixels with a depth
    test, coloured by world height through a 256-entry palette over z_range, optionally shaded by eye-dome lighting (edl = its strength)."""

    def __init__(self, width, height, point_px=2, z_range=(-2.0, 10.0), background=(0, 0, 0, 255), edl=0.0, device_id=0,
                 max_frames_per_call=16, edl_radius_px=1):
        cfg = L.RenderCfg()
        L.check(L.lib().ptl_render_default_cfg(C.byref(cfg), int(width), int(height)))
        cfg.point_px, cfg.max_frames_per_call = int(point_px), int(max_frames_per_call)
        cfg.z_lo, cfg.z_hi = float(z_range[0]), float(z_range[1])
        cfg.background_rgba = int(rgba_word(np.asarray(background, dtype=np.uint8).reshape(4)))
        cfg.edl_strength, cfg.edl_radius_px = float(edl), int(edl_radius_px)
        self.cfg, self.width, self.height, self.device_id = cfg, int(width), int(height), int(device_id)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_render_create(C.byref(cfg), int(device_id), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_render_destroy(self._h)
            self._h = None

    __del__ = close

    def set_palette(self, rgba):
        """256 colours, (256, 4) uint8 R G B A"""
        w = np.ascontiguousarray(rgba_word(np.asarray(rgba, dtype=np.uint8).reshape(256, 4)))
        L.check(L.lib().ptl_render_set_palette(self._h, w.ctypes.data_as(C.POINTER(C.c_uint32))))

    def set_z_range(self, lo, hi):
        """world heights of palette entries 0 and 255 for the frames that follow"""
        L.check(L.lib().ptl_render_set_z_range(self._h, float(lo), float(hi)))
        self.cfg.z_lo, self.cfg.z_hi = float(lo), float(hi)

    def set_overlay(self, xyz, rgba=(255, 255, 255, 255), point_px=3):
        """the overlay cloud: (n, 3) world points with one colour each ((n, 4) uint8, or one colour for all); no points clears it"""
        x = L.as_f64(xyz).reshape(-1, 3)
        if len(x) == 0:
            L.check(L.lib().ptl_render_set_overlay(self._h, None, None, 0, int(point_px)))
            return
        col = np.asarray(rgba, dtype=np.uint8)
        w = np.ascontiguousarray(np.broadcast_to(rgba_word(col.reshape(-1, 4)), (len(x),)))
        L.check(L.lib().ptl_render_set_overlay(self._h, L.dptr(x), w.ctypes.data_as(C.POINTER(C.c_uint32)), len(x), int(point_px)))

    def set_point_colors(self, icp, rgba):
        """a colour of its own for every stored point of `icp`'s map (include/ptudes_mi.h ptl_render_set_point_colors): rgba
        words (n,) uint32 or (n, 4) uint8 R G B A in pool order - the order of `Painter.values()`, `Carver.votes()` and the per-point map
        score.  Frames of that handle then take a point's colour from its word instead of the height palette, until the colours are cleared;
        a map that has grown since needs them set again"""
        a = np.asarray(rgba)
        w = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) if a.dtype != np.uint8 else np.ascontiguousarray(rgba_word(a.reshape(-1, 4)))
        L.check(L.lib().ptl_render_set_point_colors(self._h, icp._h, w.ctypes.data_as(C.POINTER(C.c_uint32)), len(w)))

    def clear_point_colors(self):
        """back to the height palette for every map"""
        L.check(L.lib().ptl_render_set_point_colors(self._h, None, None, 0))

    def set_early_reject(self, on):
        """measurement hook: the plain load in front of the atomic on or off (the frames do not change)"""
        L.check(L.lib().ptl_render_debug_set_early_reject(self._h, 1 if on else 0))

    def render(self, icp, cams, depth=False, keys=False, timing=False):
        """the frames of `icp`'s map (None: the overlay only) through cams (a list of _lib.RenderCam): (n, H, W, 4) uint8, then the float32
        depth (n, H, W; +inf = empty) and / or the raw uint64 keys when asked, then the per-frame in-view counts (n,) int64; timing=True
        appends the HIP-event time of the launches in ms"""
        cams = list(cams)
        n = len(cams)
        arr = (L.RenderCam * max(n, 1))(*cams)
        H, W = self.height, self.width
        rgba = np.empty((n, H, W), dtype=np.uint32)
        d = np.empty((n, H, W), dtype=np.float32) if depth else None
        k = np.empty((n, H, W), dtype=np.uint64) if keys else None
        inv = np.zeros(n, dtype=np.int64)
        ms = C.c_double()
        L.check(L.lib().ptl_render_frames(self._h, None if icp is None else icp._h, arr, n, rgba.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          None if d is None else d.ctypes.data_as(C.POINTER(C.c_float)),
                                          None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          inv.ctypes.data_as(L.c_i64_p), C.byref(ms)))
        out = [rgba.view(np.uint8).reshape(n, H, W, 4)]
        if depth:
            out.append(d)
        if keys:
            out.append(k)
        out.append(inv)
        if timing:
            out.append(ms.value)
        return tuple(out)


class Ekf:
    def __init__(self, init_grav=None, init_bacc=None, init_bgyr=None, device_id=0):
        self.cfg = ekf_cfg(init_grav, init_bacc, init_bgyr, device_id)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_ekf_create(C.byref(self.cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_ekf_destroy(self._h)
            self._h = None

    __del__ = close

    def process_imu(self, lacc, avel, ts):
        a, w = L.as_f64(lacc), L.as_f64(avel)
        L.check(L.lib().ptl_ekf_process_imu(self._h, L.dptr(a), L.dptr(w), float(ts)))

    def process_imu_batch(self, rows):
        r = L.as_f64(rows)
        L.check(L.lib().ptl_ekf_process_imu_batch(self._h, L.dptr(r), len(r)))

    def process_pose(self, pose, meas_cov=None):
        p = L.as_f64(pose).reshape(16)
        c = None if meas_cov is None else L.as_f64(meas_cov).reshape(36)
        L.check(L.lib().ptl_ekf_process_pose(self._h, L.dptr(p), None if c is None else L.dptr(c)))

    def state(self):
        nav, cov = np.empty(19), np.empty((18, 18))
        L.check(L.lib().ptl_ekf_get_state(self._h, L.dptr(nav), L.dptr(cov)))
        return nav, cov

    @property
    def nav(self):
        return self.state()[0]

    @property
    def cov(self):
        return self.state()[1]

    def pose_mat(self):
        out = np.empty((4, 4))
        L.check(L.lib().ptl_ekf_pose_mat(self._h, L.dptr(out)))
        return out

    @property
    def ts(self):
        t = C.c_double()
        L.check(L.lib().ptl_ekf_ts(self._h, C.byref(t)))
        return t.value

    def enable_smoother(self, capacity):
        """a fresh, empty history log for `capacity` pose updates (0 = off); include/ptudes_mi.h ptl_ekf_log_enable"""
        L.check(L.lib().ptl_ekf_log_enable(self._h, int(capacity)))
        self._sm_cap = int(capacity)

    def smoother_log(self):
        """the raw history log (dict of per-entry arrays; core._LOG_FIELDS)"""
        return _smoother_log(getattr(self, "_sm_cap", 0), lambda p, m, n, o: L.lib().ptl_ekf_smoother_log(self._h, p, m, n, o))

    def smooth(self, nav=True, cov=True):
        """fixed-interval RTS smoother over the logged updates: dict(t, poses[, nav][, cov]), one row per update in update order"""
        return _smoothed(getattr(self, "_sm_cap", 0), nav, cov,
                         lambda p, t, n, c, w: L.lib().ptl_ekf_smooth(self._h, p, t, n, c, getattr(self, "_sm_cap", 0), w))


    def enable_knots(self, capacity):
        """a fresh, empty knot list of the IMU deskew for `capacity` knots (0 = off); include/ptudes_mi.h ptl_ekf_knots_enable"""
        L.check(L.lib().ptl_ekf_knots_enable(self._h, int(capacity)))
        self._knot_cap = int(capacity)

    def knots(self):
        """the raw knot list: ((n, 8) array [ts, pos(3), q xyzw(4)], overflow flag)"""
        return _knots(getattr(self, "_knot_cap", 0), lambda p, m, n, o: L.lib().ptl_ekf_knots(self._h, p, m, n, o))


# one knot of the IMU deskew (include/ptudes_mi.h PTL_KNOT_*)
KNOT_STRIDE = 8
DESKEW_NONE, DESKEW_CV, DESKEW_IMU = 0, 1, 2


def _knots(cap, call):
    raw = np.zeros((max(int(cap), 1), KNOT_STRIDE))
    n, ovf = C.c_int64(), C.c_int32()
    L.check(call(L.dptr(raw), raw.shape[0], C.byref(n), C.byref(ovf)))
    return raw[:min(n.value, raw.shape[0])].copy(), bool(ovf.value)


def _modes(n, call):
    out = np.zeros(max(int(n), 1), dtype=np.int32)
    w = C.c_int64()
    L.check(call(out.ctypes.data_as(C.POINTER(C.c_int32)), len(out), C.byref(w)))
    return out[:w.value].copy()


def _sweep_times(t0t1, n_scans):
    t = L.as_f64(t0t1).reshape(-1, 2)
    if len(t) != n_scans:
        raise ValueError("sweep times: one (t0, t1) row per scan")
    return np.ascontiguousarray(t)


def _smoothed(cap, nav, cov, call):
    """one smoothing call with `cap`-row host buffers -> dict(t, poses, nav?, cov?) of the rows written"""
    cap = max(int(cap), 1)
    p, t = np.empty((cap, 4, 4)), np.empty(cap)
    n = np.empty((cap, 19)) if nav else None
    c = np.empty((cap, 18, 18)) if cov else None
    w = C.c_int64()
    L.check(call(L.dptr(p), L.dptr(t), None if n is None else L.dptr(n), None if c is None else L.dptr(c), C.byref(w)))
    m = w.value
    out = dict(t=t[:m], poses=p[:m])
    if nav:
        out["nav"] = n[:m]
    if cov:
        out["cov"] = c[:m]
    return out


# one entry of the smoother's log (include/ptudes_mi.h PTL_SMOOTHER_LOG_*)
LOG_STRIDE = 1024
_LOG_FIELDS = (("ts", 0, ()), ("nav_pred", 1, (19,)), ("P_pred", 20, (18, 18)), ("Phi", 344, (18, 18)),
               ("nav_post", 668, (19,)), ("P_post", 687, (18, 18)))


def _smoother_log(cap, call):
    """one log read-out with a `cap`-entry host buffer -> dict(ts, nav_pred, P_pred, Phi, nav_post, P_post, overflow) of the entries"""
    raw = np.zeros((max(int(cap), 1), LOG_STRIDE))
    n, ovf = C.c_int64(), C.c_int32()
    L.check(call(L.dptr(raw), raw.shape[0], C.byref(n), C.byref(ovf)))
    m = min(n.value, raw.shape[0])
    out = {k: raw[:m, o:o + int(np.prod(shp or (1,)))].reshape((m,) + shp).copy() for k, o, shp in _LOG_FIELDS}
    out["overflow"] = bool(ovf.value)
    return out


# ---- what SeqRunner and BatchRunner share (they differ only by the batch's sequence index, which `call` carries)
def _seq_cfg(n_scans, points_per_scan, n_imu, max_range, min_range, use_imu_prediction, with_ekf, device_id, ekf, icp_over, **fields):
    """the runner's ptl_seq_cfg; fields: further ones by name (range_input, resident_scans)"""
    cfg = L.SeqCfg()
    for k, v in fields.items():
        setattr(cfg, k, v)
    cfg.icp = icp_cfg(max_range, min_range, device_id=device_id, **icp_over)
    cfg.ekf = ekf if ekf is not None else ekf_cfg(device_id=device_id)
    cfg.n_scans, cfg.points_per_scan, cfg.n_imu = n_scans, points_per_scan, n_imu
    cfg.use_imu_prediction = int(bool(use_imu_prediction))
    cfg.with_ekf = int(bool(with_ekf))
    return cfg


def _scan_f32(cfg, xyz_f32):
    x = np.ascontiguousarray(xyz_f32, dtype=np.float32)
    if x.size != cfg.points_per_scan * 3:
        raise ValueError("scan size mismatch")
    return x.ctypes.data_as(C.POINTER(C.c_float))


def _range_u32(cfg, range_mm):
    r = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
    if r.size != cfg.points_per_scan:
        raise ValueError("range image size mismatch")
    return r.ctypes.data_as(C.POINTER(C.c_uint32))


def _imu_args(n_scans, imu_rows, imu_end):
    """(rows or None, imu_end) pointers of an IMU upload"""
    r = L.as_f64(imu_rows).reshape(-1, 7) if len(imu_rows) else np.zeros((0, 7))
    e = np.ascontiguousarray(imu_end, dtype=np.int64)
    if len(e) != n_scans:
        raise ValueError("imu_end needs one entry per scan")
    return L.dptr(r) if len(r) else None, e.ctypes.data_as(L.c_i64_p)


def _results(n, with_ekf, call):
    """one results read-out with `n`-row host buffers -> dict(kiss_poses, stats[, res_poses, res_t]) of the rows written"""
    res_poses, res_t, kiss = np.empty((n, 4, 4)), np.empty(n), np.empty((n, 4, 4))
    stats = (L.IcpStats * n)()
    w = C.c_int64()
    L.check(call(L.dptr(res_poses), L.dptr(res_t), L.dptr(kiss), stats, n, C.byref(w)))
    m = w.value
    out = dict(kiss_poses=kiss[:m], stats=[stats[i].as_dict() for i in range(m)])
    if with_ekf:
        out.update(res_poses=res_poses[:m], res_t=res_t[:m])
    return out


def icp_ekf_step(icp: "Icp", ekf: "Ekf", imu_rows, xyz, t01=None, guess=None, use_imu_prediction=False, sweep=None):
    """One scan of the reference's loop body (cli/ekf_bench.py:493-563) in one host round trip (include/ptudes_mi.h ptl_icp_ekf_step):
    the IMU rows [ts, lacc, avel] that precede the scan, the registration (guess: the filter's pose when use_imu_prediction, else
    `guess` / constant velocity), the filter's update with the new pose.  Returns (kiss_pose, ekf_pose, ekf_ts); the stats row is
    appended to icp.stats like register_frame does.
    sweep=(t0, t1): IMU deskew - the scan's column table from the filter's knots (ekf.enable_knots first), sweep times on the IMU clock
    instead of t01 (include/ptudes_mi.h ptl_icp_ekf_step_imu_deskew)."""
    rows = L.as_f64(imu_rows).reshape(-1, 7) if len(imu_rows) else np.zeros((0, 7))
    xyz = np.asarray(xyz)
    if xyz.dtype == np.float32:
        x, dt = np.ascontiguousarray(xyz), L.PTL_F32
    else:
        x, dt = L.as_f64(xyz), L.PTL_F64
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("xyz must be (N, 3)")
    t = None if t01 is None else L.as_f64(t01)
    if t is not None and len(t) != len(x):
        raise ValueError("t01 must have one entry per point")
    g = None if guess is None else L.as_f64(guess).reshape(16)
    kiss, pose, ts, st = np.empty((4, 4)), np.empty((4, 4)), C.c_double(), L.IcpStats()
    if sweep is not None:
        if t is not None:
            raise ValueError("IMU deskew takes sweep times, not per-point t01")
        L.check(L.lib().ptl_icp_ekf_step_imu_deskew(icp._h, ekf._h, L.dptr(rows) if len(rows) else None, len(rows), x.ctypes.data_as(C.c_void_p),
                                                    dt, len(x), float(sweep[0]), float(sweep[1]), None if g is None else L.dptr(g),
                                                    int(bool(use_imu_prediction)), L.dptr(kiss), L.dptr(pose), C.byref(ts), C.byref(st)))
        icp.stats.append(st.as_dict())
        return kiss, pose, ts.value
    L.check(L.lib().ptl_icp_ekf_step(icp._h, ekf._h, L.dptr(rows) if len(rows) else None, len(rows), x.ctypes.data_as(C.c_void_p), dt, len(x),
                                     None if t is None else L.dptr(t), None if g is None else L.dptr(g), int(bool(use_imu_prediction)),
                                     L.dptr(kiss), L.dptr(pose), C.byref(ts), C.byref(st)))
    icp.stats.append(st.as_dict())
    return kiss, pose, ts.value


def device_sync(device_id=0):
    L.check(L.lib().ptl_device_sync(device_id))


def host_pin(array, device_id=0):
    """page-lock a C-contiguous numpy array the sweeps will be uploaded from (include/ptudes_mi.h ptl_host_pin); keep the array alive until host_unpin"""
    if not array.flags["C_CONTIGUOUS"]:
        raise ValueError("host_pin needs a C-contiguous array")
    L.check(L.lib().ptl_host_pin(device_id, C.c_void_p(array.ctypes.data), array.nbytes))


def host_unpin(array):
    L.check(L.lib().ptl_host_unpin(C.c_void_p(array.ctypes.data)))


def pkt_format(fmt):
    """ptl_pkt_format of a packets.OusterPacketFormat"""
    f = L.PktFormat()
    f.profile, f.pixels_per_column = fmt.profile_id, fmt.pixels_per_column
    f.columns_per_frame, f.columns_per_packet = fmt.columns_per_frame, fmt.columns_per_packet
    return f


def pkt_field(fmt, name):
    """the _lib.PktField of channel field `name` ("range", "reflectivity", "signal", "near_ir", "range2", "reflectivity2", "signal2", any
    case, or a PTL_PKT_FIELD_* id) in the profile of `fmt` (a packets.OusterPacketFormat or an L.PktFormat): the library's table (include/
    ptudes_mi.h, unpinned).  A ValueError naming profile and field where the profile has no such field"""
    f = fmt if isinstance(fmt, L.PktFormat) else pkt_format(fmt)
    if isinstance(name, str):
        if name.upper() not in L.PKT_FIELDS:
            raise ValueError(f"unknown lidar field '{name}' (known: {', '.join(n.lower() for n in L.PKT_FIELDS)})")
        fid = L.PKT_FIELDS.index(name.upper())
    else:
        fid = int(name)
    out = L.PktField()
    L.check(L.lib().ptl_pkt_field_default(C.byref(f), fid, C.byref(out)))
    return out


def pkt_packet_bytes(fmt):
    """the library's size of a lidar packet of `fmt` (a packets.OusterPacketFormat or an L.PktFormat)"""
    f = fmt if isinstance(fmt, L.PktFormat) else pkt_format(fmt)
    n = L.lib().ptl_pkt_packet_bytes(C.byref(f))
    if n < 0:
        L.check(int(n))
    return int(n)


def _packet_rows(fmt_bytes, packets):
    """(n, stride) u8 view of a packet buffer: rows are packets, the row stride is what the library is told"""
    a = packets if isinstance(packets, np.ndarray) else np.frombuffer(packets, dtype=np.uint8)
    if a.dtype != np.uint8:
        raise ValueError("packets: a uint8 buffer")
    if a.ndim == 1:
        if a.size % fmt_bytes:
            raise ValueError(f"packets: {a.size} bytes are not a whole number of {fmt_bytes}-byte packets")
        a = a.reshape(-1, fmt_bytes)
    if a.ndim != 2 or a.shape[1] < fmt_bytes or (len(a) and a.strides[1] != 1):
        raise ValueError(f"packets: (n, >= {fmt_bytes}) uint8 rows")
    return a


class PacketDecoder:
    """Lidar packets -> range images, column times, statuses and summaries on the device (include/ptudes_mi.h ptl_pktdec_*).
    fmt: a packets.OusterPacketFormat.  One decode call takes up to max_packets packets of up to max_sweeps sweeps."""

    def __init__(self, fmt, max_sweeps=8, max_packets=None, device_id=0):
        self.format, self.device_id = fmt, int(device_id)
        self._cfmt = pkt_format(fmt)
        self.packet_bytes = pkt_packet_bytes(self._cfmt)
        if self.packet_bytes != fmt.lidar_packet_size:
            raise RuntimeError(f"packet size: the library says {self.packet_bytes}, packets.OusterPacketFormat {fmt.lidar_packet_size}")
        per_sweep = -(-fmt.columns_per_frame // fmt.columns_per_packet)
        self.max_sweeps = int(max_sweeps)
        self.max_packets = int(max_packets) if max_packets else 2 * per_sweep * self.max_sweeps
        self._h = C.c_void_p()
        L.check(L.lib().ptl_pktdec_create(C.byref(self._cfmt), self.device_id, self.max_packets, self.max_sweeps, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ptl_pktdec_destroy(self._h)
            self._h = None

    __del__ = close

    def profile(self, enable=True, reset=False):
        """(device ms of the calls' four launches since the last reset, calls timed); include/ptudes_mi.h ptl_pktdec_profile"""
        ms, n = C.c_double(), C.c_int64()
        L.check(L.lib().ptl_pktdec_profile(self._h, int(enable), C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def decode_arrays(self, packets, sweep_of_packet, n_sweeps=None):
        """(range (S, H, W) u32, timestamp (S, W) u64, status (S, W) u16, [summary dict] * S)"""
        a = _packet_rows(self.packet_bytes, packets)
        sop = np.ascontiguousarray(sweep_of_packet, dtype=np.int32)
        if len(sop) != len(a):
            raise ValueError("one sweep index per packet")
        S = int(n_sweeps) if n_sweeps is not None else (int(sop.max()) + 1 if len(sop) else 0)
        H, W = self.format.pixels_per_column, self.format.columns_per_frame
        rng, ts, st = np.empty((S, H, W), np.uint32), np.empty((S, W), np.uint64), np.empty((S, W), np.uint16)
        sums = (L.PktSummary * max(S, 1))()
        L.check(L.lib().ptl_pktdec_decode(self._h, C.c_void_p(a.ctypes.data), a.strides[0] if len(a) else self.packet_bytes, len(a),
                                          sop.ctypes.data_as(C.POINTER(C.c_int32)), S, C.c_void_p(rng.ctypes.data),
                                          C.c_void_p(ts.ctypes.data), C.c_void_p(st.ctypes.data), C.cast(sums, C.c_void_p)))
        return rng, ts, st, [sums[i].as_dict() for i in range(S)]

    def decode_field_arrays(self, packets, sweep_of_packet, fields, n_sweeps=None):
        """`decode_arrays` and, from the same staged packets, the images of 1 .. 4 fields (names of `pkt_field`, or _lib.PktField
        descriptors): ([field image (S, H, W) u32 per field], range, timestamp, status, [summary dict] * S); include/ptudes_mi.h
        ptl_pktdec_decode_fields"""
        a = _packet_rows(self.packet_bytes, packets)
        sop = np.ascontiguousarray(sweep_of_packet, dtype=np.int32)
        if len(sop) != len(a):
            raise ValueError("one sweep index per packet")
        desc = [f if isinstance(f, L.PktField) else pkt_field(self.format, f) for f in fields]
        S = int(n_sweeps) if n_sweeps is not None else (int(sop.max()) + 1 if len(sop) else 0)
        H, W = self.format.pixels_per_column, self.format.columns_per_frame
        rng, ts, st = np.empty((S, H, W), np.uint32), np.empty((S, W), np.uint64), np.empty((S, W), np.uint16)
        imgs = [np.empty((S, H, W), np.uint32) for _ in desc]
        sums = (L.PktSummary * max(S, 1))()
        cdesc = (L.PktField * max(len(desc), 1))(*desc)
        outs = (C.c_void_p * max(len(desc), 1))(*[im.ctypes.data for im in imgs])
        L.check(L.lib().ptl_pktdec_decode_fields(self._h, C.c_void_p(a.ctypes.data), a.strides[0] if len(a) else self.packet_bytes, len(a),
                                                 sop.ctypes.data_as(C.POINTER(C.c_int32)), S, cdesc, len(desc), outs,
                                                 C.c_void_p(rng.ctypes.data), C.c_void_p(ts.ctypes.data), C.c_void_p(st.ctypes.data),
                                                 C.cast(sums, C.c_void_p)))
        return imgs, rng, ts, st, [sums[i].as_dict() for i in range(S)]

    def decode(self, packets, sweep_of_packet, n_sweeps=None, fields=()):
        """-> [packets.PacketScan], one per sweep; fields: names of `pkt_field` (at most 4) whose images each scan carries in `.fields`"""
        from .packets import PacketScan
        if not fields:
            rng, ts, st, sums = self.decode_arrays(packets, sweep_of_packet, n_sweeps)
            return [PacketScan(rng[i], ts[i], st[i], sums[i]["frame_id"], sums[i]) for i in range(len(sums))]
        names = [str(f).lower() for f in fields]
        imgs, rng, ts, st, sums = self.decode_field_arrays(packets, sweep_of_packet, names, n_sweeps)
        return [PacketScan(rng[i], ts[i], st[i], sums[i]["frame_id"], sums[i], fields={n: im[i] for n, im in zip(names, imgs)})
                for i in range(len(sums))]


def _upload_packets(call, dec, packets, W, want_ts):
    """one sweep's packets (tightly packed) into a runner's slot -> (summary dict, column times or None)"""
    a = _packet_rows(dec.packet_bytes, packets)
    if len(a) and (a.shape[1] != dec.packet_bytes or not a.flags["C_CONTIGUOUS"]):
        raise ValueError("upload_packets takes tightly packed packets")
    summ = L.PktSummary()
    ts = np.empty(W, np.uint64) if want_ts else None
    L.check(call(dec._h, C.c_void_p(a.ctypes.data), len(a), C.byref(summ), None if ts is None else C.c_void_p(ts.ctypes.data)))
    return summ.as_dict(), ts


class _Runner:
    """What SeqRunner and BatchRunner share: the entry points without a sequence index (ptl_seq_* / ptl_batch_* by _PREFIX)."""
    _PREFIX = ""

    def _c(self, name):
        return getattr(L.lib(), self._PREFIX + name)

    def _init_imu_deskew(self, imu_deskew, knot_capacity):
        """the constructor's imu_deskew: a handle it fails for is closed, not leaked"""
        self.knot_capacity = 0
        if imu_deskew:
            try:
                self.imu_deskew(True, knot_capacity)
            except Exception:
                self.close()
                raise

    def imu_deskew(self, on=True, knot_capacity=None):
        """the column tables from the filter's IMU-propagated trajectory, for every sequence (upload_sweep_times before running;
        knot_capacity defaults to n_imu + 1, enough for any split of the samples; include/ptudes_mi.h ptl_*_imu_deskew_enable)"""
        cap = int(self.cfg.n_imu) + 1 if knot_capacity is None else int(knot_capacity)
        L.check(self._c("imu_deskew_enable")(self._h, int(bool(on)), cap if on else 0))
        self.knot_capacity = cap if on else 0

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    __del__ = close

    def set_lut(self, lut, active_beams=0):
        self._lut = lut  # keep alive
        L.check(self._c("set_lut")(self._h, lut._h, int(active_beams)))

    def run(self, n=None):
        L.check(self._c("run")(self._h, self.n_scans if n is None else n))

    def enqueue(self, n):
        L.check(self._c("enqueue")(self._h, n))

    def wait(self):
        L.check(self._c("wait")(self._h))

    def profile(self, enable=True, reset=False):
        ms, n = C.c_double(), C.c_int64()
        L.check(self._c("profile")(self._h, int(enable), C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def _build_map(self, call, map_icp, traj, t0t1, first, last):
        t = _sweep_times(t0t1, self.n_scans)
        last = self.n_scans - 1 if last is None else int(last)
        nv, ns = C.c_int64(), C.c_int64()
        L.check(call(map_icp._h, traj._h, L.dptr(t), int(first), last, C.byref(nv), C.byref(ns)))
        return nv.value, ns.value

    def enable_smoother(self, on=True):
        """log the filter history of every sequence (capacity n_scans each) for smooth(); include/ptudes_mi.h ptl_*_smoother_enable"""
        L.check(self._c("smoother_enable")(self._h, int(bool(on))))


class SeqRunner(_Runner):
    """Whole sequence in HBM, no host round trip per scan."""
    _PREFIX = "ptl_seq_"

    def __init__(self, n_scans, points_per_scan, n_imu, *, max_range=70.0, min_range=1.0, use_imu_prediction=False,
                 with_ekf=True, device_id=0, ekf=None, imu_deskew=False, knot_capacity=None, **icp_over):
        """imu_deskew: the column tables from the filter's IMU-propagated trajectory (upload_sweep_times before running; knot_capacity
        defaults to n_imu + 1, enough for any split of the samples; include/ptudes_mi.h ptl_seq_imu_deskew_enable)"""
        self.cfg = _seq_cfg(n_scans, points_per_scan, n_imu, max_range, min_range, use_imu_prediction, with_ekf, device_id, ekf, icp_over)
        self._h = C.c_void_p()
        L.check(L.lib().ptl_seq_create(C.byref(self.cfg), C.byref(self._h)))
        self.n_scans = n_scans
        self._init_imu_deskew(imu_deskew, knot_capacity)

    def upload_sweep_times(self, t0t1):
        """(n_scans, 2) absolute (t0, t1) per sweep on the IMU clock"""
        t = _sweep_times(t0t1, self.n_scans)
        L.check(L.lib().ptl_seq_upload_sweep_times(self._h, L.dptr(t)))

    def deskew_modes(self):
        return _modes(self.n_scans, lambda p, m, w: L.lib().ptl_seq_deskew_modes(self._h, p, m, w))

    def knots(self):
        return _knots(self.knot_capacity, lambda p, m, n, o: L.lib().ptl_seq_knots(self._h, p, m, n, o))

    def build_map(self, map_icp, traj, t0t1, first=0, last=None):
        """the world map of the RESIDENT sweeps [first, last] into `map_icp` (an Icp used as a map container), posed by `traj`: column j of
        sweep k fires at t0 + (j / W)(t1 - t0) of t0t1[k].  No sweep crosses the bus and the runner is only read.  Returns
        (n_valid, n_skipped); include/ptudes_mi.h ptl_seq_map_build"""
        return self._build_map(lambda *a: L.lib().ptl_seq_map_build(self._h, *a), map_icp, traj, t0t1, first, last)

    def upload_scan(self, k, xyz_f32):
        L.check(L.lib().ptl_seq_upload_scan(self._h, k, _scan_f32(self.cfg, xyz_f32)))

    def upload_range(self, k, range_mm):
        L.check(L.lib().ptl_seq_upload_range(self._h, k, _range_u32(self.cfg, range_mm)))

    def upload_packets(self, dec, k, packets, col_ts=False):
        """sweep k decoded from its lidar packets straight into its slot (include/ptudes_mi.h ptl_seq_upload_packets): the slot then holds
        what upload_range of the decoded image leaves.  Returns the sweep's summary (dict), with col_ts=True (summary, column times ns)"""
        out = _upload_packets(lambda d, p, n, s, t: L.lib().ptl_seq_upload_packets(self._h, d, int(k), p, n, s, t), dec, packets,
                              dec.format.columns_per_frame, col_ts)
        return out if col_ts else out[0]

    def upload_imu(self, imu_rows, imu_end):
        L.check(L.lib().ptl_seq_upload_imu(self._h, *_imu_args(self.n_scans, imu_rows, imu_end)))

    def diag(self):
        h = C.c_void_p()
        L.check(L.lib().ptl_seq_icp(self._h, C.byref(h)))
        return _diag(h)

    def advance(self, n):
        L.check(L.lib().ptl_seq_advance(self._h, n))

    def copy_traj(self, dst_device_ptr, max_rows):
        rows = C.c_int64()
        L.check(L.lib().ptl_seq_copy_traj(self._h, C.c_void_p(dst_device_ptr), max_rows, C.byref(rows)))
        return rows.value

    def results(self):
        return _results(self.n_scans, self.cfg.with_ekf, lambda *a: L.lib().ptl_seq_results(self._h, *a))

    def traj_device(self):
        p, rows = C.c_void_p(), C.c_int64()
        L.check(L.lib().ptl_seq_traj_device(self._h, C.byref(p), C.byref(rows)))
        return p.value, rows.value

    def smoother_log(self):
        """the raw history log of the sequence's filter (dict of per-entry arrays; core._LOG_FIELDS)"""
        return _smoother_log(self.n_scans, lambda p, m, n, o: L.lib().ptl_seq_smoother_log(self._h, p, m, n, o))

    def smooth(self, nav=True, cov=True):
        """fixed-interval RTS smoother: dict(t, poses[, nav][, cov]), rows aligned with results()'s res_poses / res_t"""
        return _smoothed(self.n_scans, nav, cov, lambda p, t, n, c, w: L.lib().ptl_seq_smooth(self._h, p, t, n, c, w))


class BatchRunner(_Runner):
    """Up to 256 independent sequences on one GPU (lockstep: 32); sequence s lives on XCD s & 7 (the workgroups with
    blockIdx & 7 == s & 7).  Two drivers (`free_running`): True (the default with the 8-lane Gauss-Newton kernel) - one
    persistent launch carries up to `scans_per_launch` scans of every sequence, teams of `team_workgroups` workgroups take
    the scans of their XCD's sequences as they come free; False - lockstep, one launch per stage for all sequences, a step
    lasts as long as its slowest sequence.  Either way the per-sequence results are bit-identical to
    `SeqRunner(..., gn_workgroups=<workgroups per team>, gn_lanes_per_point=<the batch's>)`."""
    _PREFIX = "ptl_batch_"

    def __init__(self, n_sequences, n_scans, points_per_scan, n_imu, *, max_range=70.0, min_range=1.0,
                 use_imu_prediction=False, with_ekf=True, device_id=0, ekf=None, free_running=None, scans_per_launch=0,
                 team_workgroups=0, range_input=False, resident_scans=0, imu_deskew=False, knot_capacity=None, **icp_over):
        """range_input: every sweep will arrive as a raw range image (set_lut + upload_range) and stays one in HBM - 4 bytes per pixel
        resident instead of 12 (include/ptudes_mi.h ptl_seq_cfg.range_input).  resident_scans: R >= 2 = a ring of R sweep slots per sequence
        instead of all n_scans - sweeps are uploaded in order, later ones while a launch works on earlier ones (ptl_seq_cfg.resident_scans)"""
        icp_over.setdefault("gn_lanes_per_point", 8)  # a workgroup walks ~200 points per iteration here: the throughput form
        if icp_over["gn_lanes_per_point"] == 8:
            icp_over.setdefault("gn_threads", 512)
        cfg = _seq_cfg(n_scans, points_per_scan, n_imu, max_range, min_range, use_imu_prediction, with_ekf, device_id, ekf, icp_over,
                       range_input=int(bool(range_input)), resident_scans=int(resident_scans))
        self.cfg, self.S, self.n_scans = cfg, int(n_sequences), n_scans
        self._h = C.c_void_p()
        L.check(L.lib().ptl_batch_create(C.byref(cfg), self.S, C.byref(self._h)))
        self.free_running = (cfg.icp.gn_lanes_per_point == 8) if free_running is None else bool(free_running)
        if free_running is not None or scans_per_launch:
            L.check(L.lib().ptl_batch_set_driver(self._h, int(self.free_running), int(scans_per_launch)))
        if team_workgroups:
            L.check(L.lib().ptl_batch_set_team_workgroups(self._h, int(team_workgroups)))
        self._init_imu_deskew(imu_deskew, knot_capacity)

    def upload_sweep_times(self, s, t0t1):
        t = _sweep_times(t0t1, self.n_scans)
        L.check(L.lib().ptl_batch_upload_sweep_times(self._h, int(s), L.dptr(t)))

    def deskew_modes(self, s):
        return _modes(self.n_scans, lambda p, m, w: L.lib().ptl_batch_deskew_modes(self._h, int(s), p, m, w))

    def knots(self, s):
        return _knots(self.knot_capacity, lambda p, m, n, o: L.lib().ptl_batch_knots(self._h, int(s), p, m, n, o))

    def set_driver(self, free_running, scans_per_launch=0, team_workgroups=None):
        """choose the driver (and the team size) again for the same handle and sweeps: back to the cold start first"""
        L.check(L.lib().ptl_batch_reset(self._h))
        L.check(L.lib().ptl_batch_set_driver(self._h, int(bool(free_running)), int(scans_per_launch)))
        self.free_running = bool(free_running)
        if team_workgroups is not None:
            L.check(L.lib().ptl_batch_set_team_workgroups(self._h, int(team_workgroups)))

    def team_geometry(self):
        """(workgroups per team, teams that can get work) of the free-running kernel"""
        g, t = C.c_int32(), C.c_int32()
        L.check(L.lib().ptl_batch_team_workgroups(self._h, C.byref(g), C.byref(t)))
        return g.value, t.value

    EXEC_COUNTERS = ("searches", "rows_rebuilt", "map_points_read", "gn_iterations", "vds1_claims", "vds2_claims",
                     "point_iterations", "scans", "settled_nothing_in_reach", "dropped_full_voxel")

    def exec_counters(self, s):
        """executed-work counters of sequence s, cumulative since the cold start (include/ptudes_mi.h ptl_batch_exec_counters)"""
        out = (C.c_uint64 * 16)()
        L.check(L.lib().ptl_batch_exec_counters(self._h, s, out))
        return dict(zip(self.EXEC_COUNTERS, (int(v) for v in out)))

    def diag(self, s):
        h = C.c_void_p()
        L.check(L.lib().ptl_batch_icp(self._h, int(s), C.byref(h)))
        return _diag(h)

    def sched_counters(self, s):
        """where the scans of sequence s ran: scans taken by a team of another XCD, cross-XCD hand-overs, last XCC id + 1"""
        out = (C.c_uint64 * 4)()
        L.check(L.lib().ptl_batch_sched_counters(self._h, s, out))
        return dict(stolen=int(out[0]), cross_xcd_handovers=int(out[1]), last_xcc=int(out[2]) - 1)

    def status(self):
        """sticky status word of the free-running driver (include/ptudes_mi.h ptl_batch_status)"""
        v = C.c_uint32()
        L.check(L.lib().ptl_batch_status(self._h, C.byref(v)))
        return v.value

    def debug_stall_block(self, block, round=0):
        L.check(L.lib().ptl_batch_debug_stall_block(self._h, int(block), int(round)))

    def debug_map_points_per_thread(self, points=0):
        """test hook: the free-running map update's points per thread (0 = ask); returns the value in effect"""
        v = C.c_int32()
        L.check(L.lib().ptl_batch_debug_set_map_points_per_thread(self._h, int(points), C.byref(v)))
        return v.value

    def build_map(self, s, map_icp, traj, t0t1, first=0, last=None):
        """SeqRunner.build_map for sequence s of the batch (refused with a sweep ring: its sweeps are gone); ptl_batch_map_build"""
        return self._build_map(lambda *a: L.lib().ptl_batch_map_build(self._h, int(s), *a), map_icp, traj, t0t1, first, last)

    def upload_scan(self, s, k, xyz_f32):
        L.check(L.lib().ptl_batch_upload_scan(self._h, s, k, _scan_f32(self.cfg, xyz_f32)))

    def upload_range(self, s, k, range_mm):
        L.check(L.lib().ptl_batch_upload_range(self._h, s, k, _range_u32(self.cfg, range_mm)))

    def upload_packets(self, s, dec, k, packets, col_ts=False):
        """sweep k of sequence s decoded from its lidar packets straight into its slot (ptl_batch_upload_packets; see SeqRunner.upload_packets)"""
        out = _upload_packets(lambda d, p, n, sm, t: L.lib().ptl_batch_upload_packets(self._h, int(s), d, int(k), p, n, sm, t), dec, packets,
                              dec.format.columns_per_frame, col_ts)
        return out if col_ts else out[0]

    def upload_imu(self, s, imu_rows, imu_end):
        L.check(L.lib().ptl_batch_upload_imu(self._h, s, *_imu_args(self.n_scans, imu_rows, imu_end)))

    def results(self, s):
        return _results(self.n_scans, self.cfg.with_ekf, lambda *a: L.lib().ptl_batch_results(self._h, s, *a))

    def copy_traj(self, s, dst_device_ptr, max_rows):
        rows = C.c_int64()
        L.check(L.lib().ptl_batch_copy_traj(self._h, s, C.c_void_p(dst_device_ptr), max_rows, C.byref(rows)))
        return rows.value

    def seq_clocks(self, s):
        """per-scan mean microseconds of sequence s in the free-running kernel: (K0-K4, wait, GN, wait, map update, filter)"""
        out = (C.c_int64 * 8)()
        L.check(L.lib().ptl_batch_seq_clocks(self._h, s, out))
        n = max(out[6], 1)
        return tuple(out[i] / n / 100.0 for i in range(6))

    def seq_clocks_raw(self, s):
        """the same clocks as they are kept: (six sums of 100 MHz ticks since the cold start, scans) - a caller that wants the means over
        SOME of the scans (the timed ones, without the warm-up) takes differences"""
        out = (C.c_int64 * 8)()
        L.check(L.lib().ptl_batch_seq_clocks(self._h, s, out))
        return tuple(int(out[i]) for i in range(6)), int(out[6])

    def smooth(self):
        """the backward pass of every sequence in one launch (waits); smoothed(s) then gives sequence s's rows"""
        L.check(L.lib().ptl_batch_smooth(self._h))

    def smoother_log(self, s):
        """the raw history log of sequence s's filter (dict of per-entry arrays; core._LOG_FIELDS)"""
        return _smoother_log(self.n_scans, lambda p, m, n, o: L.lib().ptl_batch_smoother_log(self._h, s, p, m, n, o))

    def smoothed(self, s, nav=True, cov=True):
        """dict(t, poses[, nav][, cov]) of sequence s after smooth(), rows aligned with results(s)'s res_poses / res_t"""
        return _smoothed(self.n_scans, nav, cov, lambda p, t, n, c, w: L.lib().ptl_batch_smoothed(self._h, s, p, t, n, c, w))


BUILD_INFO = ("kcand", "ans_row_doubles", "lds_points", "seq_u", "seq_u2", "gn8_threads", "lanes_per_point", "spec", "surv",
              "prefetch", "keep_x1000", "tab_entry_bytes", "vds_entry_bytes", "diagnostics", "fast", "pose_chunk")


def build_info():
    """compile-time constants of the loaded library (include/ptudes_mi.h ptl_build_info)"""
    out = (C.c_int32 * 16)()
    L.check(L.lib().ptl_build_info(out))
    return dict(zip(BUILD_INFO, (int(v) for v in out)))

