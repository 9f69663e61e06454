"""The compute half of the reference's map fly-by (src/ptudes/fly.py:75-111, src/ptudes/cli/flyby.py): scans that
carry one pose per column are de-warped into the world frame and accumulated into a point map.  The reference hands
both to ouster-sdk's `ScansAccumulator` and draws the result in a window (out of scope here); this module keeps the
arithmetic: column poses from a time-stamped trajectory (`utils.TrajectoryEvaluator`, `utils.pose_scans_from_nc_gt`),
`client.dewarp` on the GPU (`ptl_lut_dewarp`), and the map as the voxel-hash map of the registration path
(`ptl_icp_map_add`: a voxel keeps its first points, deterministic) instead of ScansAccumulator's random subsample.
With a `core.Traj` the three steps run fused on the device (`ptl_icp_map_add_posed_range`), and `add_run` builds the map of a
runner's resident sweeps without moving them (`ptl_*_map_build`); DESIGN.md 3.14.
The camera path of the reference (fly.py:14-233) is here too, against the package's own `Camera` instead of the viewer's, and `FlyBy` draws
its frames on the device through `core.Renderer`; DESIGN.md 3.21."""
from dataclasses import dataclass, field
from enum import Enum
from typing import Optional

import numpy as np

from . import core
from .utils import estimate_apex_dolly, exp_pose6, log_pose, prune_trajectory


@dataclass
class PosedScan:
    """What the fly-by needs of an ouster LidarScan: the range image, column timestamps (ns) and column poses"""
    range_mm: np.ndarray                 # (H, W) uint32, 0 = no return
    timestamp: np.ndarray                # (W,) ns
    pose: Optional[np.ndarray] = field(default=None)  # (W, 4, 4), world <- sensor at the column's firing time

    def __post_init__(self):
        self.range_mm = np.ascontiguousarray(self.range_mm, dtype=np.uint32)
        if self.pose is None:
            self.pose = np.tile(np.eye(4), (self.range_mm.shape[1], 1, 1))


DEFAULT_COMPARE_THRESHOLDS = (0.05, 0.1, 0.2)  # metres


@dataclass
class MapComparison:
    """A map against a reference cloud, both directions of the nearest-neighbour distance: `accuracy` has the map's stored
    points as queries against the reference, `completeness` the reference's against the map (two core.MapDistance).  Per threshold:
    precision = accuracy's n_within / n_query, recall = completeness', F = 2 P R / (P + R) (0 when both are 0)."""
    accuracy: "core.MapDistance"
    completeness: "core.MapDistance"
    reference_name: str = "reference"
    reference_points: int = 0

    @property
    def thresholds(self):
        return self.accuracy.thresholds

    @property
    def precision(self):
        return self.accuracy.fractions

    @property
    def recall(self):
        return self.completeness.fractions

    @property
    def f_score(self):
        return tuple(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(self.precision, self.recall))

    def lines(self):
        """the block the commands print"""
        out = [f"map comparison: reference {self.reference_name} ({self.reference_points} points), max dist {self.accuracy.max_dist:g} m"]
        for name, d in (("accuracy (map -> reference)", self.accuracy), ("completeness (reference -> map)", self.completeness)):
            out.append(f"  {name}: {d.n_query} queries, {d.n_matched} matched, mean {1000.0 * d.mean_dist:.3f} mm, rms {1000.0 * d.rms_dist:.3f} mm")
        for t, p, r, f in zip(self.thresholds, self.precision, self.recall, self.f_score):
            out.append(f"  at {t:g} m: precision {p:.6f}, recall {r:.6f}, F {f:.6f}")
        return out


def compare_maps(map_icp, ref_icp, thresholds=DEFAULT_COMPARE_THRESHOLDS, max_dist=None, per_point=False, reference_name="reference"):
    """`MapComparison` of two map handles (core.Icp) on one device; per_point: also (xyz, d2) of the map's stored points against the reference"""
    thresholds = DEFAULT_COMPARE_THRESHOLDS if thresholds is None else thresholds
    acc = ref_icp.map_compare(map_icp, max_dist=max_dist, thresholds=thresholds, per_point=per_point)
    com = map_icp.map_compare(ref_icp, max_dist=max_dist, thresholds=thresholds)
    cmp_ = MapComparison(acc[0] if per_point else acc, com, reference_name, com.n_query)
    return (cmp_, acc[1]) if per_point else cmp_


def compare_handle(map_icp, reference, thresholds=DEFAULT_COMPARE_THRESHOLDS, max_dist=None, per_point=False, reference_name="reference"):
    """`compare_maps` of a map handle against `reference`: a core.Icp, a MapAccumulator, or an (N, 3) array, for which a reference handle is
    built for the call at the map's voxel size, points per voxel and capacities"""
    if isinstance(reference, MapAccumulator):
        reference = reference.icp
    if isinstance(reference, core.Icp):
        return compare_maps(map_icp, reference, thresholds, max_dist, per_point, reference_name)
    c = map_icp.cfg
    ref = core.map_from_points(reference, voxel_size=c.voxel_size, max_points_per_voxel=c.max_points_per_voxel, device_id=c.device_id,
                               map_block_capacity=c.map_block_capacity, map_table_capacity=c.map_table_capacity)
    try:
        return compare_maps(map_icp, ref, thresholds, max_dist, per_point, reference_name)
    finally:
        ref.close()


def carved_handle(map_icp, mask, xyz):
    """a new map handle (core.Icp) that holds the points of `xyz` (N, 3) that `mask` (N,) does not flag, with `map_icp`'s voxel size, points
    per voxel, scan geometry and capacities (core.map_from_points)"""
    mask, pts = np.asarray(mask, dtype=bool).reshape(-1), np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if len(mask) != len(pts):
        raise ValueError("one flag per point")
    c = map_icp.cfg
    return core.map_from_points(pts[~mask], voxel_size=c.voxel_size, max_points_per_voxel=c.max_points_per_voxel, device_id=c.device_id,
                                max_points_per_scan=max(int(c.max_points_per_scan), 1 << 16), scan_cols=c.scan_cols,
                                map_block_capacity=c.map_block_capacity, map_table_capacity=c.map_table_capacity)


class MapAccumulator:
    """Accumulates posed scans into a world-frame voxel map on the GPU (ScansAccumulator's map, deterministic form)."""

    def __init__(self, lut: core.Lut, voxel_size: float = 0.5, max_points_per_voxel: int = 20, max_range: float = 1.0e9,
                 device_id: int = 0, map_block_capacity: int = 1 << 21, map_table_capacity: int = 1 << 23):
        self.lut = lut
        # only the map of the handle is used: no registration happens here, the poses are given
        self._icp = core.Icp(max_range, 0.0, voxel_size=voxel_size, max_points_per_voxel=max_points_per_voxel,
                             scan_cols=lut.W, max_points_per_scan=lut.H * lut.W, device_id=device_id,
                             map_block_capacity=map_block_capacity, map_table_capacity=map_table_capacity)
        self.scans = 0
        self.returns = 0
        self.skipped = 0

    def update(self, scan, traj=None):
        """de-warp one posed scan and add its returns to the map; gives back their world coordinates.
        traj (a core.Traj): the fused path - the column poses come from `traj` at scan.timestamp on the device, scan.pose is ignored,
        the sweep goes up once and nothing but the count comes back: returns n_valid (0 for a scan skipped as outside the bounds,
        counted in `skipped`) instead of the points.  The map is the same, bit for bit."""
        if traj is not None:
            # (a packets.PacketScan calls its range image `range`; a PosedScan `range_mm`)
            range_mm = scan.range_mm if hasattr(scan, "range_mm") else scan.range
            n_valid, skipped = self._icp.map_add_posed(traj, np.asarray(scan.timestamp, dtype=np.float64) * 1e-9,
                                                       range_mm=range_mm, lut=self.lut)
            self.skipped += int(skipped)
            self.scans += 0 if skipped else 1
            self.returns += n_valid
            return n_valid
        xyz, n_valid = self.lut.dewarp(scan.range_mm, scan.pose)
        keep = np.asarray(scan.range_mm).reshape(-1) != 0
        pts = xyz[keep]
        self._icp.map_add(pts)
        self.scans += 1
        self.returns += n_valid
        return pts

    def add_run(self, runner, traj, t0t1, s=None, first=0, last=None):
        """the RESIDENT sweeps [first, last] of a core.SeqRunner (s=None) or of sequence s of a core.BatchRunner into the map, posed by
        `traj` with the sweep times t0t1 (n_scans, 2): no sweep crosses the bus.  Returns (n_valid, n_skipped)"""
        if s is None:
            n_valid, n_skipped = runner.build_map(self._icp, traj, t0t1, first, last)
        else:
            n_valid, n_skipped = runner.build_map(s, self._icp, traj, t0t1, first, last)
        n = (runner.n_scans - 1 if last is None else int(last)) - int(first) + 1
        self.scans += n - n_skipped
        self.skipped += n_skipped
        self.returns += n_valid
        return n_valid, n_skipped

    @property
    def icp(self):
        """the core.Icp whose voxel map this is (for Icp.map_score(per_point=True) and the like)"""
        return self._icp

    def close(self):
        self._icp.close()

    def map_size(self):
        return self._icp.map_size()

    def map_points(self) -> np.ndarray:
        return self._icp.map_points()

    def score(self, radius=None, min_neighbours=5, sigma_floor=None, per_point=False):
        """sharpness of the accumulated map without ground truth: core.Icp.map_score of the map handle"""
        return self._icp.map_score(radius=radius, min_neighbours=min_neighbours, sigma_floor=sigma_floor, per_point=per_point)

    def compare(self, reference, thresholds=DEFAULT_COMPARE_THRESHOLDS, max_dist=None, per_point=False, reference_name="reference"):
        """the accumulated map against a reference cloud, both directions: a `MapComparison`.  reference: a core.Icp (or a
        MapAccumulator) whose map is the reference, or an (N, 3) array - a reference handle is then built for the call at this map's voxel
        size and points per voxel, so a cloud this map wrote reloads completely.  max_dist defaults to the voxel size"""
        return compare_handle(self._icp, reference, thresholds, max_dist, per_point, reference_name)

    def carved(self, mask, xyz):
        """a NEW accumulator whose map holds the points of `xyz` (N, 3) that `mask` (N,) does not flag - `xyz` the stored points as a carve
        lists them (core.CarveVotes.xyz, pool order), `mask` e.g. CarveVotes.dynamic().  Built by core.map_from_points with this map's voxel
        size, points per voxel and capacities: the kept points are a subset of the stored ones, so the new map holds all of them.  This
        accumulator stays as it is"""
        out = MapAccumulator.__new__(MapAccumulator)
        out.lut, out.scans, out.returns, out.skipped = self.lut, self.scans, self.returns, self.skipped
        out._icp = carved_handle(self._icp, mask, xyz)
        return out


class MapCarver:
    """The second pass over the sweeps that built `acc`'s map: a core.Carver on the accumulator's map handle, fed the way the
    accumulator was.  cfg: radius, margin, step, min_range, max_range (defaults: the library's for the map's voxel size).  The map must not be
    updated while the carver lives"""

    def __init__(self, acc, **cfg):
        self.acc = acc
        self.carver = core.Carver(acc.icp, **cfg)

    def update(self, scan, traj):
        """one PosedScan or packets.PacketScan, posed by `traj` (a core.Traj) at its column timestamps, as MapAccumulator.update(scan, traj)
        adds it.  Returns the sweep's used rays (0 for a sweep skipped as outside the bounds)"""
        range_mm = scan.range_mm if hasattr(scan, "range_mm") else scan.range
        n_rays, _ = self.carver.add_posed(traj, np.asarray(scan.timestamp, dtype=np.float64) * 1e-9, range_mm=range_mm, lut=self.acc.lut)
        return n_rays

    def add_run(self, runner, traj, t0t1, s=None, first=0, last=None):
        """the RESIDENT sweeps [first, last] of a core.SeqRunner (s=None) or of sequence s of a core.BatchRunner, as MapAccumulator.add_run"""
        return self.carver.add_run(runner, traj, t0t1, s=s, first=first, last=last)

    def votes(self):
        return self.carver.votes()

    def carved(self, min_through=2, min_fraction=0.5):
        """(the accumulator without the points the host policy flags, the votes): MapAccumulator.carved of CarveVotes.dynamic"""
        v = self.votes()
        return self.acc.carved(v.dynamic(min_through, min_fraction), v.xyz), v

    def close(self):
        self.carver.close()


class SweepDiffer:
    """What a localised sweep sees that the map does not, and what the map holds that the sweep no longer sees: a
    core.Caster on a map handle (a core.Icp, or a MapAccumulator's), fed posed sweeps.  cfg: radius, step, min_range, max_range (defaults:
    the library's for the map's voxel size) and `margin` of the class policy `core.cast_changes` (default: the voxel size) - all untuned.
    The map handle's scan_cols must be the sweeps' W.  The map must not be updated while the differ lives"""
    COLORS = np.array([(0, 0, 0, 255), (128, 128, 128, 255), (255, 48, 48, 255), (48, 96, 255, 255), (255, 208, 0, 255)], dtype=np.uint8)

    def __init__(self, map_or_acc, lut=None, margin=None, **cfg):
        icp = map_or_acc.icp if isinstance(map_or_acc, MapAccumulator) else map_or_acc
        self.lut = lut if lut is not None else getattr(map_or_acc, "lut", None)
        self.margin = float(icp.cfg.voxel_size if margin is None else margin)
        if not self.margin > 0.0:
            raise ValueError(f"margin = {margin}: must be positive")
        self.caster = core.Caster(icp, **cfg)
        self.last = None  # the core.CastSweep of the last update

    def _classes(self, sweep):
        self.last = sweep
        classes = sweep.changes(self.margin)
        return classes, core.change_counts(classes)

    def update(self, scan, traj):
        """one PosedScan or packets.PacketScan (a range image of this differ's LUT), posed by `traj` (a core.Traj) at its column timestamps.
        Returns (the class image (H, W) u8 of `core.cast_changes`, {class name: pixels})"""
        if self.lut is None:
            raise ValueError("a range image needs the LUT this differ was made with")
        range_mm = scan.range_mm if hasattr(scan, "range_mm") else scan.range
        return self._classes(self.caster.cast_range(traj, self.lut, range_mm, np.asarray(scan.timestamp, dtype=np.float64) * 1e-9))

    def update_xyz(self, xyz, H, W, traj, col_ts=None):
        """the same for a sweep of H x W points in the sensor frame, (0, 0, 0) = no return"""
        return self._classes(self.caster.cast_xyz(traj, xyz, H, W, col_ts))

    @classmethod
    def image(cls, classes):
        """the class image as (H, W, 4) RGBA, one fixed colour per class: none black, agree grey, new red, gone blue, unmapped yellow"""
        return cls.COLORS[np.asarray(classes, dtype=np.uint8)]

    def close(self):
        self.caster.close()


class MapPainter:
    """The second pass over the sweeps that built `acc`'s map with a channel field each: a core.Painter on the accumulator's
    map handle, fed the way the accumulator was.  The map must not be updated while the painter lives"""

    def __init__(self, acc):
        self.acc = acc
        self.painter = core.Painter(acc.icp)

    def update(self, scan, traj, field):
        """one PosedScan or packets.PacketScan, posed by `traj` (a core.Traj) at its column timestamps, as MapAccumulator.update(scan, traj)
        adds it.  field: an (H, W) uint32 image of the sweep's pixels, or a name - "range" is the range image itself, any other name is looked
        up in scan.fields (packets.PacketFeed(fields=...)).  Returns the sweep's rays that ended at a stored point"""
        range_mm = scan.range_mm if hasattr(scan, "range_mm") else scan.range
        if isinstance(field, str):
            name = field.lower()
            fields = getattr(scan, "fields", None) or {}
            if name in fields:
                field = fields[name]
            elif name == "range":
                field = range_mm
            else:
                raise ValueError(f"the scan carries no field '{name}' (it has: {', '.join(['range'] + sorted(fields))})")
        n, _ = self.painter.add_posed(traj, np.asarray(scan.timestamp, dtype=np.float64) * 1e-9, field, range_mm=range_mm, lut=self.acc.lut)
        return n

    def values(self):
        return self.painter.values()

    def close(self):
        self.painter.close()


def grid_bounds(positions, cell, pad):
    """(x0, y0, nx, ny) of the grid that holds the xy of `positions` (N, >= 2) padded by `pad` metres, snapped outward to multiples of `cell`"""
    p = np.asarray(positions, dtype=np.float64).reshape(len(positions), -1)[:, :2]
    if len(p) == 0 or not np.isfinite(p).all():
        raise ValueError("the grid's bounds need at least one finite position")
    cell, pad = float(cell), float(pad)
    lo = np.floor((p.min(axis=0) - pad) / cell)
    hi = np.ceil((p.max(axis=0) + pad) / cell)
    n = np.maximum(hi - lo, 1.0)
    return float(lo[0] * cell), float(lo[1] * cell), int(n[0]), int(n[1])


class GridBuilder:
    """The occupancy grid of a run: a core.OccupancyGrid fed the way a MapAccumulator is.
    lut: the sweeps' core.Lut, or an (H, W) pair for sweeps that come as xyz (a runner's resident ones).
    traj_or_bounds: the grid's bounds (x0, y0, x1, y1) in metres (snapped outward to multiples of `cell` from x0, y0), or the trajectory's knots
    - [(t, pose)] as utils.read_newer_college_gt gives them, or an array of poses (N, 4, 4) or positions (N, 3) - whose positions, padded by
    max_range and snapped outward to multiples of `cell`, give the bounds.  A grid of more than 2^26 cells is refused with the count.
    cfg: z_lo, z_hi, margin, step, min_range, max_range (defaults: the library's for the cell size, untuned)"""

    def __init__(self, lut, traj_or_bounds, cell, device_id=0, **cfg):
        self.lut = lut if hasattr(lut, "_h") else None
        H, W = (lut.H, lut.W) if self.lut is not None else (int(lut[0]), int(lut[1]))
        cell = float(cell)
        if not cell > 0.0:
            raise ValueError(f"cell = {cell:g}: must be positive")
        max_range = 600.0 * cell if cfg.get("max_range") is None else float(cfg["max_range"])
        tb = traj_or_bounds
        if isinstance(tb, (tuple, list)) and len(tb) == 4 and all(np.isscalar(v) for v in tb):
            bx0, by0, bx1, by1 = (float(v) for v in tb)
            if not (bx1 > bx0 and by1 > by0):
                raise ValueError(f"grid bounds ({bx0:g}, {by0:g}, {bx1:g}, {by1:g}): X1 must be above X0 and Y1 above Y0")
            x0, y0, nx, ny = bx0, by0, max(int(np.ceil((bx1 - bx0) / cell)), 1), max(int(np.ceil((by1 - by0) / cell)), 1)
        else:
            if isinstance(tb, (tuple, list)) and len(tb) and isinstance(tb[0], (tuple, list)) and len(tb[0]) == 2:
                tb = [p for _, p in tb]
            a = np.asarray(tb, dtype=np.float64)
            pos = a[:, :3, 3] if a.ndim == 3 else a.reshape(len(a), -1)[:, :3]
            x0, y0, nx, ny = grid_bounds(pos, cell, max_range)
        if nx * ny > core.GRID_MAX_CELLS:
            raise ValueError(f"the grid would have {nx} x {ny} = {nx * ny} cells of {cell:g} m, the limit is {core.GRID_MAX_CELLS} (2^26): give "
                             "narrower bounds (--grid-bounds X0,Y0,X1,Y1), a larger cell or a shorter --grid-max-range")
        self.grid = core.OccupancyGrid(cell, x0, y0, nx, ny, W, H * W, device_id=device_id, **{k: v for k, v in cfg.items() if v is not None})

    def update(self, scan, traj):
        """one PosedScan or packets.PacketScan, posed by `traj` (a core.Traj) at its column timestamps, as MapAccumulator.update(scan, traj)
        adds it.  Returns the sweep's used rays (0 for a sweep skipped as outside the bounds)"""
        if self.lut is None:
            raise ValueError("a range image needs the builder's lut")
        range_mm = scan.range_mm if hasattr(scan, "range_mm") else scan.range
        n_rays, _ = self.grid.add_posed(traj, np.asarray(scan.timestamp, dtype=np.float64) * 1e-9, range_mm=range_mm, lut=self.lut)
        return n_rays

    def add_run(self, runner, traj, t0t1, s=None, first=0, last=None):
        """the RESIDENT sweeps [first, last] of a core.SeqRunner (s=None) or of sequence s of a core.BatchRunner, as MapAccumulator.add_run"""
        return self.grid.add_run(runner, traj, t0t1, s=s, first=first, last=last)

    def counts(self):
        """a core.GridCounts of the TOUCHED box only (the cells with any count; one empty cell when there is none): a grid sized by
        max_range is mostly cells no ray came near"""
        r = self.grid.summary()
        if r.box_ix1 < r.box_ix0:
            return self.grid.read(0, 0, 1, 1)
        return self.grid.read(r.box_ix0, r.box_iy0, r.box_ix1 - r.box_ix0 + 1, r.box_iy1 - r.box_iy0 + 1)

    def close(self):
        self.grid.close()


def scalar_colors(values, lo=None, hi=None, palette=None, unpainted=(128, 128, 128, 255)):
    """HOST POLICY, not part of the library's definition and not tuned: rgba words (n,) uint32 for per-point scalars (e.g. PaintValues.mean()),
    for core.Renderer.set_point_colors.  Linear between lo and hi: palette entry clamp(floor((v - lo) 256 / (hi - lo)), 0, 255) - lo and
    everything below it take entry 0, hi and everything above it entry 255; lo / hi default to the 1st / 99th percentile of the finite values
    (0 and 1 when there is none).  hi <= lo leaves no slope: values below lo take entry 0, all others entry 255.  A value that is not finite
    (a point no ray ended at) takes `unpainted`.  palette: (256, 4) uint8 R G B A, default the renderer's height ramp"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    finite = np.isfinite(v)
    if lo is None:
        lo = float(np.percentile(v[finite], 1.0)) if finite.any() else 0.0
    if hi is None:
        hi = float(np.percentile(v[finite], 99.0)) if finite.any() else 1.0
    lo, hi = float(lo), float(hi)
    pal = core.rgba_word(core.default_palette() if palette is None else np.asarray(palette, dtype=np.uint8).reshape(256, 4))
    idx = np.zeros(len(v), dtype=np.int64)
    x = np.where(finite, v, lo)
    if hi > lo:
        idx = np.clip(np.floor((x - lo) * (256.0 / (hi - lo))), 0.0, 255.0).astype(np.int64)
    else:
        idx = np.where(x < lo, 0, 255)
    words = np.asarray(pal, dtype=np.uint32)[idx]
    words[~finite] = core.rgba_word(np.asarray(unpainted, dtype=np.uint8).reshape(4))
    return words


# ------------------------------------------------------------------------------------------------ a sweep's pose in a saved map
def candidate_poses(keyframes, n_yaw, spacing=None):
    """Start poses for a search in a map: the keyframes (M, 4, 4) - poses the mapping run went through - thinned by travelled distance, each
    composed on the right with Rz(2 pi j / n_yaw), j = 0 .. n_yaw - 1.  Thinning: the first keyframe is kept; the path length
    sum |t_i - t_(i-1)| runs along ALL keyframes, and a keyframe is kept when that length since the last kept one has reached `spacing`
    (None or 0: every keyframe is kept).  Order: keyframe-major; j = 0 is the keyframe itself, bit for bit.
    Returns (poses (K, 4, 4), kept (K / n_yaw,) the indices of the kept keyframes)"""
    kf = np.asarray(keyframes, dtype=np.float64).reshape(-1, 4, 4)
    n_yaw = int(n_yaw)
    if n_yaw < 1:
        raise ValueError(f"n_yaw = {n_yaw}: at least one heading per keyframe")
    if spacing is not None and not spacing >= 0.0:
        raise ValueError(f"spacing = {spacing}: must not be negative")
    kept, since = [], 0.0
    for i in range(len(kf)):
        if i > 0:
            since += float(np.linalg.norm(kf[i, :3, 3] - kf[i - 1, :3, 3]))
        if i == 0 or not spacing or since >= spacing:
            kept.append(i)
            since = 0.0
    out = np.empty((len(kept) * n_yaw, 4, 4))
    for a, i in enumerate(kept):
        out[a * n_yaw] = kf[i]
        for j in range(1, n_yaw):
            out[a * n_yaw + j] = kf[i] @ _rot_z(360.0 * j / n_yaw)
    return out, np.asarray(kept, dtype=np.int64)


def top_candidates(hits, top):
    """indices of the `top` largest entries of `hits` (K,), largest first, ties broken by the smaller index; negative entries (invalid
    candidates) never qualify"""
    h = np.asarray(hits).reshape(-1).astype(np.int64)
    order = np.lexsort((np.arange(len(h)), -h))  # (primary key: hits descending; secondary: index ascending)
    order = order[h[order] >= 0]
    return order[:max(int(top), 0)]


@dataclass
class Localization:
    """One fix of `MapLocalizer`: the sweep's pose in the map's frame, the query points within the last threshold of the map at that pose
    (`hits` of `n_query`, `fraction` = hits / n_query), the candidate the pose was refined from (-1: tracked from the previous fixes), the
    hits of the best OTHER refined candidate (-1: there was none) and the Gauss-Newton iterations of the winning refinement"""
    pose: np.ndarray
    hits: int
    n_query: int
    fraction: float
    candidate: int
    runner_up_hits: int
    iterations: int


class MapLocalizer:
    """Finds and follows a sensor in a FROZEN map: `Icp.pose_hits` scores every candidate start pose on the device,
    `Icp.align` - the registration's own Gauss-Newton loop, which changes neither map nor trajectory - refines the best ones.  The map is
    never added to.
    map: a core.Icp, a MapAccumulator, or an (N, 3) array (a handle is then built by core.map_from_points and closed with this object);
    keyframes (M, 4, 4): poses the mapping run went through (`candidate_poses`).
    Policy, the caller's - the defaults are untuned: n_yaw headings per keyframe, keyframe `spacing` (metres), the `top` candidates that are
    refined, the hit fraction `min_fraction` below which `track` searches again, the side `query_voxel` of the voxels that thin a sweep.
    sigma: the registration threshold of the refinements - max_dist = 3 sigma, kernel = sigma / 3 as the registration path derives them
    (reference kiss.py:108-114) - fixed at the map handle's cfg.initial_threshold unless given: a frozen map has no trajectory to adapt it to.
    max_dist / thresholds: of the hit counts (defaults: the map's voxel size); selection and `fraction` use the LAST threshold."""

    def __init__(self, map, keyframes, n_yaw=16, spacing=None, top=4, min_fraction=0.5, query_voxel=1.0, sigma=None, max_dist=None,
                 thresholds=None, **map_kw):
        self._own = False
        if isinstance(map, MapAccumulator):
            map = map.icp
        if not isinstance(map, core.Icp):
            map = core.map_from_points(map, **map_kw)
            self._own = True
        self.icp = map
        self.candidates, self.kept = candidate_poses(keyframes, n_yaw, spacing)
        if not len(self.candidates):
            raise ValueError("no keyframe: nothing to search from")
        if int(top) < 1:
            raise ValueError(f"top = {top}: at least one candidate is refined")
        if not query_voxel > 0.0:
            raise ValueError(f"query_voxel = {query_voxel}: must be positive")
        self.n_yaw, self.top, self.min_fraction, self.query_voxel = int(n_yaw), int(top), float(min_fraction), float(query_voxel)
        self.sigma = float(map.cfg.initial_threshold if sigma is None else sigma)
        self.max_dist, self.thresholds = max_dist, thresholds
        self.fixes = []              # the poses of the sweeps so far, oldest first
        self.relocalizations = 0     # searches `track` ran because a tracked pose fell below min_fraction
        self.search_ms = self.align_ms = self.rescore_ms = 0.0  # device time of the searches / wall time of the refinements / device time of the rescoring
        self.query_ms = 0.0          # wall time of `query`: a scratch map handle is made and destroyed per sweep

    def close(self):
        if self._own and self.icp is not None:
            self.icp.close()
        self.icp = None

    def query(self, points):
        """the first point per voxel of side query_voxel of a sweep's returns (sensor frame; non-finite rows and the (0, 0, 0) of a pixel
        without a return are dropped): a scratch map of one point per voxel and its `map_points()`, sorted by (x, y, z) - the export's
        order is not specified, and the refinement's sums follow the order of its points: one sweep, one query, bit for bit"""
        import time
        t0 = time.perf_counter()
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        p = p[np.isfinite(p).all(axis=1) & (p != 0.0).any(axis=1)]
        if not len(p):
            return p
        scratch = core.map_from_points(p, voxel_size=self.query_voxel, max_points_per_voxel=1, device_id=self.icp.cfg.device_id,
                                       max_points_per_scan=max(len(p), 1024), map_block_capacity=max(len(p), 1024),
                                       map_table_capacity=1 << max(12, int(4 * len(p) - 1).bit_length()))
        try:
            out = scratch.map_points()
            return np.ascontiguousarray(out[np.lexsort(out.T[::-1])])
        finally:
            scratch.close()
            self.query_ms += 1000.0 * (time.perf_counter() - t0)

    def _checked_query(self, points):
        q = self.query(points)
        if not len(q):
            raise ValueError("the sweep has no return (no finite point other than (0, 0, 0)): nothing to localise")
        return q

    def _hits(self, q, poses):
        return self.icp.pose_hits(q, poses, max_dist=self.max_dist, thresholds=self.thresholds)

    def _refine(self, q, guess):
        return self.icp.align(q, guess, 3.0 * self.sigma, self.sigma / 3.0)

    def locate(self, points, query=None):
        """search: the hit counts of every candidate, the `top` of them (by hits at the last threshold, ties to the smaller index) refined by
        `Icp.align`, the refined poses scored once more; the best of those (ties to the better-ranked candidate) is the `Localization`.
        query: the thinned points when the caller has them already"""
        import time
        q = self._checked_query(points) if query is None else np.asarray(query, dtype=np.float64).reshape(-1, 3)
        if not len(q):
            raise ValueError("an empty query: nothing to localise")
        s, hits = self._hits(q, self.candidates)
        self.search_ms += s.device_ms
        order = top_candidates(hits[:, -1], self.top)
        if not len(order):
            raise RuntimeError("no valid candidate pose")
        t0 = time.perf_counter()
        refined = [self._refine(q, self.candidates[c]) for c in order]
        self.align_ms += 1000.0 * (time.perf_counter() - t0)
        s2, h2 = self._hits(q, np.array([r[0] for r in refined]))
        self.rescore_ms += s2.device_ms
        w = int(s2.best_pose[-1])
        if w < 0:
            raise RuntimeError("no refined pose is finite")
        others = np.delete(h2[:, -1], w)
        fix = Localization(refined[w][0], int(h2[w, -1]), len(q), int(h2[w, -1]) / len(q) if len(q) else 0.0, int(order[w]),
                           int(others.max()) if len(others) else -1, int(refined[w][1]))
        self.fixes.append(fix.pose)
        return fix

    def track(self, points):
        """the next sweep of a run: `Icp.align` from the constant-velocity guess off the last two fixes (the last fix itself after one; a
        search without any), one hit count at the result; below min_fraction the sweep is searched for again and counted"""
        if not self.fixes:
            return self.locate(points)
        q = self._checked_query(points)
        last = self.fixes[-1]
        guess = last @ (np.linalg.inv(self.fixes[-2]) @ last) if len(self.fixes) > 1 else last
        pose, it = self._refine(q, guess)
        s, h = self._hits(q, pose[None])
        self.rescore_ms += s.device_ms
        hits = int(h[0, -1])
        fraction = hits / len(q) if len(q) else 0.0
        if hits < 0 or fraction < self.min_fraction:
            self.relocalizations += 1
            return self.locate(points, query=q)
        self.fixes.append(pose)
        return Localization(pose, hits, len(q), fraction, -1, -1, int(it))


# ------------------------------------------------------------------------------------------------ revisited places
def thin_sweep(points, voxel, device_id=0):
    """`MapLocalizer.query`'s thinning as a function (that class is left as it is): the first point per voxel of side `voxel` of a sweep's
    returns, sorted by (x, y, z)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1) & (p != 0.0).any(axis=1)]
    if not len(p):
        return p
    scratch = core.map_from_points(p, voxel_size=voxel, max_points_per_voxel=1, device_id=device_id, max_points_per_scan=max(len(p), 1024),
                                   map_block_capacity=max(len(p), 1024), map_table_capacity=1 << max(12, int(4 * len(p) - 1).bit_length()))
    try:
        out = scratch.map_points()
        return np.ascontiguousarray(out[np.lexsort(out.T[::-1])])
    finally:
        scratch.close()


def place_candidates(dist, shift, poses, n_sector, place_top, first=0):
    """Start poses out of a `PlaceIndex.match`: the `place_top` entries with the smallest distance (ties to the smaller index), each at
    pose_entry @ Rz(-2 pi shift / n_sector) - the rigid guess that takes the query's coordinates through the entry's frame into the world.
    Returns (poses (K, 4, 4), entries (K,))"""
    d = np.asarray(dist).reshape(-1).astype(np.int64)
    s = np.asarray(shift).reshape(-1)
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if int(place_top) < 1:
        raise ValueError(f"place_top = {place_top}: at least one place is tried")
    if first + len(d) > len(P):
        raise ValueError(f"{len(d)} matched entries from {first} on, {len(P)} poses")
    order = np.lexsort((np.arange(len(d)), d))[:int(place_top)]
    out = np.array([P[first + c] @ core.place_shift_pose(int(s[c]), n_sector) for c in order]).reshape(-1, 4, 4)
    return out, first + order.astype(np.int64)


def loop_candidates(entry, dist, shift, n_cells, max_cell_dist, top, first=0):
    """Host policy on a `PlaceIndex.match_all`: the pairs (i, j = entry[i - first]) with cell_dist = dist / (n_cells[i] + n_cells[j]) <=
    max_cell_dist, the `top` smallest of them (ties to the smaller i).  n_cells: per ENTRY of the index.  A pair without a non-zero cell
    never qualifies.  Returns [(i, j, shift, dist, cell_dist)]"""
    out = []
    nc = np.asarray(n_cells).reshape(-1).astype(np.int64)
    for k, j in enumerate(np.asarray(entry).reshape(-1)):
        i = first + k
        cells = int(nc[i] + nc[j]) if j >= 0 else 0
        if j < 0 or cells == 0:
            continue
        cd = int(dist[k]) / cells
        if cd <= max_cell_dist:
            out.append((i, int(j), int(shift[k]), int(dist[k]), cd))
    out.sort(key=lambda r: (r[4], r[0]))
    return out[:max(int(top), 0)]


def _rot_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


@dataclass
class Loop:
    """One revisit found by `LoopFinder.find`: sweep i saw the place of the earlier sweep j (keyframe numbers).  shift, dist: the descriptors'
    exact match; cell_dist = dist / (n_cells_i + n_cells_j); T_ji_measured: sweep i's coordinates in sweep j's frame as `Icp.align` of i's
    points on j's gives it from Rz(-2 pi shift / S); fraction: i's points within the hit threshold of j's there; T_ji_odometry =
    inv(pose_j) pose_i; dt_m / drot_deg: the size of inv(T_ji_odometry) T_ji_measured - what the odometry is off by at this pair; accepted:
    fraction >= min_fraction"""
    i: int
    j: int
    shift: int
    dist: int
    cell_dist: float
    fraction: float
    T_ji_measured: np.ndarray
    T_ji_odometry: np.ndarray
    dt_m: float
    drot_deg: float
    accepted: bool = True


def loop_from(i, j, shift, dist, cell_dist, fraction, T_meas, pose_i, pose_j, min_fraction):
    """the `Loop` of a verified pair: the odometry's relative pose and its discrepancy against the measured one"""
    T_odo = np.linalg.inv(pose_j) @ pose_i
    D = np.linalg.inv(T_odo) @ T_meas
    return Loop(int(i), int(j), int(shift), int(dist), float(cell_dist), float(fraction), np.asarray(T_meas), T_odo,
                float(np.linalg.norm(D[:3, 3])), _rot_deg(D[:3, :3]), bool(fraction >= min_fraction))


class LoopFinder:
    """Loops within a run: a `core.PlaceIndex` of the keyframe sweeps and HOST POLICY on its exact integers.  Every default
    here is UNTUNED - nobody has run this on a real recording: `spacing` metres of travel between described sweeps (the thinning rule of
    `candidate_poses`), `query_voxel` of the points kept per keyframe (`thin_sweep`), `map_voxel` of the scratch map a pair is verified in.
    lut: needed for scans that carry a range image.  index: an existing PlaceIndex, else one is made from **place_cfg and closed with this"""

    def __init__(self, index=None, spacing=2.0, query_voxel=1.0, map_voxel=1.0, sigma=None, lut=None, device_id=0, **place_cfg):
        if not spacing >= 0.0:
            raise ValueError(f"spacing = {spacing}: must not be negative")
        if not query_voxel > 0.0 or not map_voxel > 0.0:
            raise ValueError(f"query_voxel = {query_voxel}, map_voxel = {map_voxel}: must be positive")
        self._own = index is None
        self.index = core.PlaceIndex(device_id=device_id, **place_cfg) if index is None else index
        self.spacing, self.query_voxel, self.map_voxel, self.sigma = float(spacing), float(query_voxel), float(map_voxel), sigma
        self.lut, self.device_id = lut, int(device_id)
        self.points, self.poses, self.stamps, self.infos = [], [], [], []
        self._last, self._since = None, 0.0
        self.match_ms = self.verify_ms = 0.0  # device time of match_all / wall time of the verifications

    def close(self):
        if self._own and self.index is not None:
            self.index.close()
        self.index = None

    def add(self, scan_or_points, pose, stamp):
        """the next sweep of the run at its odometry pose (4x4, world <- sensor).  Described and kept when the path length since the last kept
        sweep has reached `spacing` (the first always is).  scan_or_points: (N, 3) sensor-frame points, or a scan with a range image
        (range_mm / range; needs lut).  Returns the keyframe number, or -1 for a sweep passed over"""
        P = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        if self._last is not None:
            self._since += float(np.linalg.norm(P[:3, 3] - self._last[:3, 3]))
        keep = self._last is None or not self.spacing or self._since >= self.spacing
        self._last = P
        if not keep:
            return -1
        self._since = 0.0
        if hasattr(scan_or_points, "range_mm") or hasattr(scan_or_points, "range"):
            if self.lut is None:
                raise ValueError("a scan with a range image needs the LoopFinder's lut")
            rng = scan_or_points.range_mm if hasattr(scan_or_points, "range_mm") else scan_or_points.range
            k, info = self.index.describe((self.lut, rng), keep=True)
            xyz = self.lut(rng)
        else:
            xyz = np.asarray(scan_or_points)
            k, info = self.index.describe(xyz, keep=True)
        self.points.append(thin_sweep(xyz, self.query_voxel, self.device_id))
        self.poses.append(P.copy()); self.stamps.append(float(stamp)); self.infos.append(info.as_dict())
        return k

    def verify(self, i, j, shift):
        """(T_ji_measured, fraction): `Icp.align` of keyframe i's points on a scratch map of keyframe j's from Rz(-2 pi shift / S), and the
        share of i's points within the map's voxel size of a stored point there"""
        m = core.map_from_points(self.points[j], voxel_size=self.map_voxel, device_id=self.device_id,
                                 max_points_per_scan=max(len(self.points[j]), len(self.points[i]), 1024))
        try:
            sigma = float(m.cfg.initial_threshold if self.sigma is None else self.sigma)
            q = self.points[i]
            T, _ = m.align(q, core.place_shift_pose(shift, self.index.n_sector), 3.0 * sigma, sigma / 3.0)
            _, hits = m.pose_hits(q, T[None])
            return T, (int(hits[0, -1]) / len(q) if len(q) and hits[0, -1] >= 0 else 0.0)
        finally:
            m.close()

    def find(self, min_gap=50, max_cell_dist=20.0, top=16, min_fraction=0.5):
        """`match_all` over the keyframes, `loop_candidates`, each kept pair verified: the list of `Loop`s, best cell_dist first, accepted
        or not (`Loop.accepted`).  min_gap: in KEYFRAMES"""
        import time
        if not len(self.points):
            return []
        r = self.index.match_all(int(min_gap))
        self.match_ms += r.device_ms
        pairs = loop_candidates(r.entry, r.dist, r.shift, [f["n_cells"] for f in self.infos], max_cell_dist, top)
        t0 = time.perf_counter()
        out = []
        for i, j, s, d, cd in pairs:
            if not len(self.points[i]) or not len(self.points[j]):
                continue
            T, fraction = self.verify(i, j, s)
            out.append(loop_from(i, j, s, d, cd, fraction, T, self.poses[i], self.poses[j], min_fraction))
        self.verify_ms += 1000.0 * (time.perf_counter() - t0)
        return out


def loop_lines(loops):
    """the block `ekf-bench --find-loops` prints: the accepted loops and the odometry's discrepancy at each"""
    acc = [l for l in loops if l.accepted]
    lines = [f"loops: {len(acc)} accepted of {len(loops)} verified (every threshold is the caller's and untuned)"]
    for l in acc:
        lines.append(f"  keyframe {l.i} revisits {l.j}: shift {l.shift}, dist {l.dist} ({l.cell_dist:.2f} per cell), fraction {l.fraction:.3f}, "
                     f"odometry off by {l.dt_m:.3f} m, {l.drot_deg:.2f} deg")
    return lines


def save_loops_csv(path, loops, stamps=None):
    """one row per verified loop: i, j, [stamp_i, stamp_j,] shift, dist, cell_dist, fraction, accepted, dt_m, drot_deg, then T_ji_measured's
    top three rows"""
    with open(path, "w") as f:
        f.write("i,j," + ("stamp_i,stamp_j," if stamps is not None else "") + "shift,dist,cell_dist,fraction,accepted,dt_m,drot_deg," +
                ",".join(f"T{r}{c}" for r in range(3) for c in range(4)) + "\n")
        for l in loops:
            st = f"{stamps[l.i]!r},{stamps[l.j]!r}," if stamps is not None else ""
            f.write(f"{l.i},{l.j},{st}{l.shift},{l.dist},{l.cell_dist!r},{l.fraction!r},{int(l.accepted)},{l.dt_m!r},{l.drot_deg!r}," +
                    ",".join(repr(float(v)) for v in l.T_ji_measured[:3].reshape(-1)) + "\n")


class PlaceLocalizer(MapLocalizer):
    """`MapLocalizer` whose start poses come from places: the sweep is described, compared with every entry of a loaded
    places file at every heading, and the `place_top` best entries - each at pose_entry @ Rz(-2 pi shift / S) - are the candidates of
    `locate`, instead of keyframes x yaws.  Scoring, refinement, rescoring and `track` are MapLocalizer's.  place_top is UNTUNED.
    places: the path of a file `utils.save_places` wrote, or its loaded dict.  index: a PlaceIndex to load it into (default: one of the
    file's parameters, closed with this object)"""

    def __init__(self, map, places, place_top=4, index=None, device_id=0, **kw):
        from .utils import load_places
        if int(place_top) < 1:
            raise ValueError(f"place_top = {place_top}: at least one place is tried")
        data = load_places(places) if isinstance(places, str) else places
        if not len(data["poses"]):
            raise ValueError("the places file holds no entry: nothing to search from")
        self._own_index = index is None
        if index is None:
            index = core.PlaceIndex(device_id=device_id, capacity=max(len(data["desc"]), 1), **data["cfg"])
        self.index = index
        try:
            have = index.tables()
            if not (np.array_equal(have[0], data["ring_edge2"]) and np.array_equal(have[1], data["sector_dir"])):
                raise ValueError("the places file's tables differ from the handle's: its descriptors do not compare bit for bit")
            self.first = len(index)
            index.load(data["desc"], data["infos"])
            self.place_poses, self.place_top = np.asarray(data["poses"], dtype=np.float64).reshape(-1, 4, 4), int(place_top)
            self.places_tried = None     # the entries behind the last search's candidates
            self.place_ms = 0.0          # device time of the matches
            super().__init__(map, self.place_poses, n_yaw=1, **kw)
        except Exception:
            if self._own_index:
                index.close()
            raise

    def close(self):
        super().close()
        if self._own_index and self.index is not None:
            self.index.close()
        self.index = None

    def locate(self, points, query=None):
        self.index.describe(points, keep=False)
        m = self.index.match(-1, self.first, self.first + len(self.place_poses) - 1)
        self.place_ms += m.device_ms
        self.candidates, self.places_tried = place_candidates(m.dist, m.shift, self.place_poses, self.index.n_sector, self.place_top)
        return super().locate(points, query)


# ------------------------------------------------------------------------------------------------ the camera path
class FlyingState(Enum):
    """Camera movement states (reference fly.py:19-24)"""
    BUILDING = 0
    TO_THE_BEGINNING = 1
    COURSING = 2
    TO_THE_APEX = 3


def update_min_max(cmm: np.ndarray, new_point: np.ndarray):
    cmm[:, 0] = np.minimum(cmm[:, 0], new_point)
    cmm[:, 1] = np.maximum(cmm[:, 1], new_point)


def _rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, c, -s, 0.0], [0.0, s, c, 0.0], [0.0, 0.0, 0.0, 1.0]])


_LOOK_DOWN = np.diag([1.0, -1.0, -1.0, 1.0])  # target frame (z up) -> camera frame (+x right, +y down, +z forward) of a camera that looks straight down


@dataclass
class Camera:
    """The viewer camera the reference drives (ouster-sdk's viz.Camera through PointViz; third party), restated: it orbits the origin of the
    `target` frame.  target: 4x4, what the reference passes to set_target (the inverse of the pose looked at); yaw, pitch in degrees
    (pitch 0 looks straight down, -90 along the horizon); dolly: the view distance is 50 exp(dolly / 100); fov: vertical, degrees.
    The defaults are those of the reference's make_point_viz."""
    target: np.ndarray = field(default_factory=lambda: np.eye(4))
    yaw: float = 140.0
    pitch: float = 0.0
    dolly: float = -100.0
    fov: float = 90.0
    near: float = 0.1
    far: float = 1.0e4

    def view_distance(self) -> float:
        """inverts utils.estimate_apex_dolly: dolly = 100 ln(D / 50)"""
        return 50.0 * float(np.exp(self.dolly / 100.0))

    def view_matrix(self) -> np.ndarray:
        """world -> camera, 4x4: dolly translation . pitch . yaw . target"""
        dolly = np.eye(4)
        dolly[2, 3] = self.view_distance()
        return dolly @ _rot_x(self.pitch) @ _LOOK_DOWN @ _rot_z(self.yaw) @ np.asarray(self.target, dtype=np.float64)

    def cam(self, width: int, height: int):
        """the _lib.RenderCam of a width x height frame: fx = fy = (height / 2) / tan(fov / 2), principal point at the image centre"""
        from . import _lib
        c = _lib.RenderCam()
        c.view[:] = list(self.view_matrix()[:3, :].reshape(12))
        f = (height / 2.0) / np.tan(np.radians(self.fov) / 2.0)
        c.fx, c.fy, c.cx, c.cy, c.near_m, c.far_m = f, f, width / 2.0, height / 2.0, self.near, self.far
        return c


class FState:
    """Flyby states handler (reference fly.py:27-36); `update` progresses the state against a `Camera` and returns the next on transition"""

    def __init__(self, name: str) -> None:
        self.name = name

    def update(self, dt: float, cam: Camera):
        raise NotImplementedError


class BuildingState(FState):
    """The camera half of the reference's BuildingState (fly.py:95-106): the caller adds the scan to the map, this moves the camera along"""

    def __init__(self, min_max: Optional[np.ndarray] = None, next_state: Optional[FlyingState] = None) -> None:
        super().__init__("BUILDING")
        self._min_max = np.zeros((3, 2)) if min_max is None else min_max
        assert self._min_max.shape == (3, 2)
        self._next_state = next_state

    def update_camera(self, cam: Camera, first_column_pose: np.ndarray) -> None:
        scan_pose = np.array(first_column_pose, dtype=np.float64)
        scan_pose[:3, :3] = np.eye(3)
        cam.target = np.linalg.inv(scan_pose)
        update_min_max(self._min_max, scan_pose[:3, 3])
        dolly = estimate_apex_dolly(self._min_max, cam.fov)
        cam.dolly = cam.dolly + 0.05 * (dolly - cam.dolly)

    def update(self, dt: float, cam: Camera):
        return self._next_state


class CameraTransitionState(FState):
    """Transition camera to the target and/or pitch/dolly/yaw (reference fly.py:140-193)"""

    def __init__(self, name: str = "", target: Optional[np.ndarray] = None, pitch: Optional[float] = -70, dolly: Optional[float] = -70,
                 yaw: Optional[float] = 120, velocity: float = 1.0, next_state: Optional[FlyingState] = None) -> None:
        super().__init__(name)
        self._target = target
        self._pitch = pitch
        self._dolly = dolly
        self._yaw = yaw
        self._next_state = next_state
        self._t = 0
        self._v = velocity

    def update(self, dt: float, cam: Camera):
        curr_pitch, curr_dolly, curr_yaw = cam.pitch, cam.dolly, cam.yaw
        dt = self._v * dt
        if self._t + dt >= 1.0:
            return self._next_state
        if self._target is not None:
            curr_target = np.asarray(cam.target, dtype=np.float64)
            pose_d = log_pose(curr_target @ self._target)
            new_target = np.linalg.inv(curr_target) @ exp_pose6(dt / (1 - self._t) * pose_d)
            cam.target = np.linalg.inv(new_target)
        if self._pitch is not None:
            cam.pitch = curr_pitch + dt / (1 - self._t) * (self._pitch - curr_pitch)
        if self._dolly is not None:
            cam.dolly = curr_dolly + dt / (1 - self._t) * (self._dolly - curr_dolly)
        if self._yaw is not None:
            cam.yaw = curr_yaw + dt / (1 - self._t) * (self._yaw - curr_yaw)
        self._t += dt
        return None


class CoursingState(FState):
    """Follow the scans poses, i.e. set target along the traj eval poses (reference fly.py:196-233).  traj_eval: anything with `start_time`,
    `end_time` and `pose_at(t)` (utils.TrajectoryEvaluator)"""

    def __init__(self, traj_eval, start_time: Optional[float] = None, end_time: Optional[float] = None, velocity: float = 1.0,
                 min_duration: float = 3.0, next_state: Optional[FlyingState] = None) -> None:
        super().__init__("COURSING")
        self._start_t = traj_eval.start_time if start_time is None else start_time
        self._end_t = traj_eval.end_time if end_time is None else end_time
        self._traj_eval = traj_eval
        self._v = velocity
        # slowing down velocity so we have at least min_duration coursing time
        if self._v > 0 and self._end_t - self._start_t > 0 and (self._end_t - self._start_t) / self._v < min_duration:
            self._v = (self._end_t - self._start_t) / min_duration
        self._next_state = next_state
        self._t = self._start_t

    def update(self, dt: float, cam: Camera):
        dt = self._v * dt
        if self._t + dt > self._end_t:
            return self._next_state
        cam.target = np.linalg.inv(self._traj_eval.pose_at(self._t))
        self._t += dt
        return None


BUILDING_Z_SPAN = 10.0  # metres either side of the sensor's height: the palette range of the frames drawn while the map is still growing
TRACK_RGBA = (255, 255, 255, 255)


class FlyBy:
    """The reference's fly-by (cli/flyby.py:160-236) without a window: BUILDING (one frame per scan added, from the map so far), TO_THE_BEGINNING,
    COURSING, TO_THE_APEX, then it stops (the reference loops for ever).  acc: the MapAccumulator the scans go into; renderer: a core.Renderer;
    poses: [(ts, 4x4)] the trajectory the scans are posed on (as `flyby` shifts it); dt = rate / fps per frame (the reference ticks at 0.0333 s).
    z_range: fixed palette range, or None = the sensor's height +- BUILDING_Z_SPAN while building and the map's own z extent afterwards.
    `frames(scans)` yields (state name, (H, W, 4) uint8) frame by frame; the trajectory's positions are the overlay."""

    def __init__(self, acc, renderer, poses, fps: float = 30, rate: float = 1.0, time_bounds: float = 1.5, z_range=None,
                 max_frames: Optional[int] = None, track_px: int = 3, on_state=None, point_colors=None):
        self.acc, self.renderer, self.poses = acc, renderer, list(poses)
        # point_colors: a callable without arguments that returns one rgba word per stored point of acc's map in pool order
        # (core.Renderer.set_point_colors).  It is called ONCE, when BUILDING has ended and the map stands: the pool order moves while blocks
        # are added, so the BUILDING frames keep the height palette and the colours start with the first frame after them
        self.point_colors = point_colors
        self.dt = float(rate) / float(fps)
        self.time_bounds, self.z_range, self.max_frames, self.track_px = float(time_bounds), z_range, max_frames, int(track_px)
        self.camera = Camera()
        self.min_max = np.zeros((3, 2))
        self.res_poses = []
        self.on_state = on_state
        self.state_name = "BUILDING"
        self.n_frames = 0

    def _create_state(self, flying_state):
        cam = self.camera
        if flying_state == FlyingState.TO_THE_BEGINNING:
            return CameraTransitionState(name="TO_THE_BEGINNING", target=self.res_poses[0][1], velocity=0.15, next_state=FlyingState.COURSING)
        if flying_state == FlyingState.COURSING:
            from .utils import TrajectoryEvaluator
            pruned = prune_trajectory(self.res_poses)
            return CoursingState(TrajectoryEvaluator(pruned, time_bounds=1.0, device_id=self.renderer.device_id), velocity=5.0,
                                 next_state=FlyingState.TO_THE_APEX)
        if flying_state == FlyingState.TO_THE_APEX:
            dolly = estimate_apex_dolly(self.min_max, cam.fov)
            return CameraTransitionState(name="TO_THE_APEX", pitch=0, yaw=140, dolly=dolly, velocity=0.15,
                                         next_state=FlyingState.TO_THE_BEGINNING)
        raise ValueError(flying_state)

    def _enter(self, name):
        self.state_name = name
        if self.on_state is not None:
            self.on_state(name)

    def _full(self):
        return self.max_frames is not None and self.n_frames >= self.max_frames

    def frames(self, scans, traj=None):
        """scans: PosedScan-likes in order; traj: a core.Traj of `poses` for the fused map update (made here when None)"""
        from .utils import TrajectoryEvaluator
        r, W, H = self.renderer, self.renderer.width, self.renderer.height
        own_traj = traj is None
        if own_traj:
            traj = core.Traj([t for t, _ in self.poses], [p for _, p in self.poses], self.time_bounds, self.time_bounds, device_id=r.device_id)
        ev = TrajectoryEvaluator(self.poses, time_bounds=self.time_bounds, device_id=r.device_id)
        building = BuildingState(min_max=self.min_max, next_state=FlyingState.TO_THE_BEGINNING)
        self._enter(building.name)
        try:
            for scan in scans:
                before = self.acc.skipped
                self.acc.update(scan, traj=traj)
                if self.acc.skipped != before or self._full():  # (max_frames ends the frames, not the map)
                    continue
                ts = np.asarray(scan.timestamp, dtype=np.float64) * 1e-9
                ends = ev.poses_at([ts[0], ts[-1]])
                self.res_poses.append((float(ts[-1]), ends[1]))
                building.update_camera(self.camera, ends[0])
                if self.z_range is None:
                    h = float(ends[0][2, 3])
                    r.set_z_range(h - BUILDING_Z_SPAN, h + BUILDING_Z_SPAN)
                else:
                    r.set_z_range(*self.z_range)
                r.set_overlay(np.array([p[:3, 3] for _, p in self.res_poses]), TRACK_RGBA, self.track_px)
                rgba = r.render(self.acc.icp, [self.camera.cam(W, H)])[0]
                self.n_frames += 1
                yield self.state_name, rgba[0]
        finally:
            if own_traj:
                traj.close()
        if not self.res_poses or self._full():
            return
        if self.z_range is None:
            z = self.acc.map_points()[:, 2]
            lo, hi = (float(z.min()), float(z.max())) if len(z) else (0.0, 1.0)
            r.set_z_range(lo, hi if hi > lo else lo + 1.0)
        if self.point_colors is not None:
            r.set_point_colors(self.acc.icp, self.point_colors())
        state = self._create_state(building.update(self.dt, self.camera))
        self._enter(state.name)
        batch = int(r.cfg.max_frames_per_call)
        cams = []
        while not self._full():
            nxt = state.update(self.dt, self.camera)
            if nxt is not None:
                # the frames of the state that ends are drawn before the next state is announced
                yield from self._flush(cams)
                if state.name == "TO_THE_APEX":
                    break  # (the reference goes back to the beginning and loops for ever)
                state = self._create_state(nxt)
                self._enter(state.name)
                continue
            cams.append(self.camera.cam(W, H))
            self.n_frames += 1
            if len(cams) >= batch:
                yield from self._flush(cams)
        yield from self._flush(cams)

    def _flush(self, cams):
        if cams:
            rgba = self.renderer.render(self.acc.icp, cams)[0]
            del cams[:]
            for f in rgba:
                yield self.state_name, f


def synthetic_range_scans(seq, first=0, last=None):
    """The sweeps [first, last] of a synth.Sequence as a sensor would deliver them: (core.Lut, [PosedScan]) - range images in mm on the
    ouster column convention (column v looks along 2 pi (1 - v / W)), column timestamps in ns, the sequence's beam fan (45 .. -45 deg)"""
    H, W = seq.H, seq.W
    last = seq.n_scans - 1 if last is None else int(last)
    lut = core.Lut(H, W, np.linspace(45.0, -45.0, H), np.zeros(H), 0.0)
    src = (W - np.arange(W)) % W
    scans = []
    for k in range(int(first), last + 1):
        x = seq.scan(k).astype(np.float64).reshape(H, W, 3)
        rng_mm = np.round(np.linalg.norm(x, axis=2) * 1000.0).astype(np.uint32)[:, src]
        col_t = seq.t_base + (k + src / W) * seq.scan_dt
        scans.append(PosedScan(rng_mm, (col_t * 1e9).astype(np.int64)))
    return lut, scans


def sensor_lut(info, use_extrinsics=False, device_id=0):
    """core.Lut of a sensor's metadata (packets.read_metadata_json / ouster SensorInfo field names): beam angles, beam origin offset and
    lidar_to_sensor; use_extrinsics: the metadata's extrinsic on top, as the registration of `sequence.run_events` has it"""
    fmt = info.format
    ext = np.array(info.extrinsic, dtype=np.float64) if use_extrinsics and hasattr(info, "extrinsic") else None
    return core.Lut(fmt.pixels_per_column, fmt.columns_per_frame, info.beam_altitude_angles, info.beam_azimuth_angles,
                    info.lidar_origin_to_beam_origin_mm, np.array(info.lidar_to_sensor_transform, dtype=np.float64), ext, device_id=device_id)


def add_packet_bag(acc, bags, info, traj, start_scan=0, end_scan=None, device_id=0):
    """every sweep [start_scan, end_scan] of a raw packet bag (or list of bags) into `acc`, decoded by the package's own packet feed and posed by
    `traj` at its decoded column times (the fused per-call path); the feed is closed afterwards"""
    from . import packets as pk
    from .bag import OusterPacketBagSource
    feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info, device_id=device_id)
    try:
        for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
            if not hasattr(d, "lacc"):
                acc.update(d, traj=traj)
    finally:
        feed.close()


def paint_packet_bag(painter, bags, info, traj, field, start_scan=0, end_scan=None, device_id=0):
    """the counterpart of `add_packet_bag` for a `MapPainter`: the same sweeps of the same bag(s), decoded again by the package's packet feed -
    with the channel field `field` ("range", "reflectivity", "signal", "near_ir"; a ValueError naming profile and field where the sensor's
    profile has no such field) beside the range - and posed by `traj` at their decoded column times"""
    from . import packets as pk
    from .bag import OusterPacketBagSource
    name = str(field).lower()
    core.pkt_field(pk.OusterPacketFormat.from_info(info), name)  # (refused here, before the bag is opened)
    feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info, device_id=device_id, fields=() if name == "range" else (name,))
    try:
        for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
            if not hasattr(d, "lacc"):
                painter.update(d, traj, name)
    finally:
        feed.close()


def grid_packet_bag(builder, bags, info, traj, start_scan=0, end_scan=None, device_id=0):
    """the counterpart of `add_packet_bag` for a `GridBuilder`: the same sweeps of the same bag(s), decoded by the package's packet feed and
    posed by `traj` at their decoded column times"""
    from . import packets as pk
    from .bag import OusterPacketBagSource
    feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info, device_id=device_id)
    try:
        for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
            if not hasattr(d, "lacc"):
                builder.update(d, traj)
    finally:
        feed.close()


def loops_packet_bag(finder, bags, info, stamps, poses, start_scan=0, end_scan=None, device_id=0):
    """the counterpart of `add_packet_bag` for a `LoopFinder` (which needs its lut): sweep k of the same bag(s), decoded by the package's packet
    feed, at the k-th of `poses` / `stamps`; sweeps beyond the poses are left out"""
    from . import packets as pk
    from .bag import OusterPacketBagSource
    feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info, device_id=device_id)
    try:
        k = 0
        for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
            if not hasattr(d, "lacc") and k < len(poses):
                finder.add(d, poses[k], stamps[k])
                k += 1
    finally:
        feed.close()


def carve_packet_bag(carver, bags, info, traj, start_scan=0, end_scan=None, device_id=0):
    """the counterpart of `add_packet_bag` for a `MapCarver`: the same sweeps of the same bag(s), decoded again by the package's packet feed
    and posed by `traj` at their decoded column times"""
    from . import packets as pk
    from .bag import OusterPacketBagSource
    feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info, device_id=device_id)
    try:
        for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
            if not hasattr(d, "lacc"):
                carver.update(d, traj)
    finally:
        feed.close()

