"""The compute half of the reference's map fly-by (src/ptudes/fly.py:75-111, src/ptudes/cli/flyby.py): scans that
carry one pose per column are de-warped into the world frame and accumulated into a point map.  The reference hands
both to ouster-sdk's `ScansAccumulator` and draws the result (the viewer is out of scope here); this module keeps the
arithmetic: column poses from a time-stamped trajectory (`utils.TrajectoryEvaluator`, `utils.pose_scans_from_nc_gt`),
`client.dewarp` on the GPU (`ptl_lut_dewarp`), and the map as the voxel-hash map of the registration path
(`ptl_icp_map_add`: a voxel keeps its first points, deterministic) instead of ScansAccumulator's random subsample.
With a `core.Traj` the three steps run fused on the device (`ptl_icp_map_add_posed_range`), and `add_run` builds the map of a
runner's resident sweeps without moving them (`ptl_*_map_build`); DESIGN.md 3.14."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import core


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

