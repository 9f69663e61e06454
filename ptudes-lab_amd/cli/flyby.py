"""`flyby`: the headless form of reference src/ptudes/cli/flyby.py - the map its BUILDING state accumulates (cli/flyby.py:71-131,
utils.py:344-392, fly.py:75-111), without the viewer and the camera path.

Every scan gets the pose of each of its columns on the trajectory of a Newer College format poses file (moved to the start scan, as the
reference does), is de-warped and accumulated - on the GPU, fused (`fly.MapAccumulator.update(scan, traj=...)`).  The map is the
deterministic voxel map of the registration path (a voxel keeps its first points), not ScansAccumulator's random subsample:
`-r` / `--accum-map-ratio` are accepted for the option set only.  What the viewer's OSD shows is printed; `--save-map` writes the points.
FILE (.pcap / .bag) goes through ouster-sdk when it is importable; a raw packet .bag (or a directory of bags) goes through the package's
own packet decoder (packets.py) when it is not, or with --native-packets - every column is then posed at its decoded firing time;
`--synthetic SEED` runs the same path on the synthetic sequence.  `--map-score` prints the sharpness of the map without ground truth
 and, with `--save-map`, adds the per-point values to the PLY.
"""
from typing import Optional

import click
import numpy as np

from ..utils import read_newer_college_gt, save_map_ply

TIME_BOUNDS = 1.5  # seconds a column may lie outside the poses file (reference utils.py:368)


@click.command(name="flyby")
@click.argument("file", required=False, type=click.Path())
@click.option("-m", "--meta", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="sensor metadata .json of the PCAP / BAG (needed when it is not found next to FILE)")
@click.option("--kitti-poses", required=False, type=click.Path(dir_okay=False),
              help="poses file in KITTI format, one pose per scan (refused: its column timing is ouster-sdk's own)")
@click.option("--nc-gt-poses", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="poses file in Newer College ground-truth format")
@click.option("-r", "--rate", type=float, default=1.0, help="playback rate of the viewer (accepted for the option set; there is no playback)")
@click.option("--accum-map-ratio", type=float,
              help="ratio of random points per scan of the viewer's map (accepted for the option set; the voxel map replaces the random subsample)")
@click.option("--start-scan", type=int, default=0, help="first scan of the map (0-based)")
@click.option("--end-scan", type=int, help="last scan of the map (inclusive)")
@click.option("--voxel-size", type=float, default=0.5, help="voxel size of the map, metres (default 0.5)")
@click.option("--save-map", required=False, type=click.Path(dir_okay=False),
              help="write the map's points to this file: PLY (binary, double x y z), or .npy")
@click.option("--synthetic", type=int, default=None,
              help="build the map of the synthetic 128x1024 sequence with this seed instead of FILE (no ouster-sdk needed)")
@click.option("--native-packets", is_flag=True,
              help="read FILE (.bag, or a directory of bags) with the package's own packet decoder also when ouster-sdk is installed "
                   "(without ouster-sdk this is what happens anyway)")
@click.option("--map-score", is_flag=True,
              help="score the sharpness of the map without ground truth (mean plane variance and mean map entropy of the stored points' "
                   "neighbourhoods) and print it; with --save-map the PLY carries the per-point values")
@click.option("--score-radius", type=float, default=None,
              help="neighbourhood radius of --map-score, metres (default and upper bound: --voxel-size)")
def ptudes_flyby(file: Optional[str], meta: Optional[str], kitti_poses: Optional[str], nc_gt_poses: Optional[str], rate: float,
                 accum_map_ratio: Optional[float], start_scan: int, end_scan: Optional[int], voxel_size: float,
                 save_map: Optional[str], synthetic: Optional[int], native_packets: bool = False, map_score: bool = False,
                 score_radius: Optional[float] = None) -> None:
    """Map of the lidar scans with poses (the flyby visualizer's map, headless).

    Data is provided via FILE in Ouster raw packets formats (PCAP or BAG with lidar/imu packets), or --synthetic SEED.
    """
    if kitti_poses:
        raise click.ClickException("--kitti-poses is not supported here: the column timing of one-pose-per-scan files is defined inside "
                                   "ouster-sdk's pose_scans_from_kitti, which this build cannot read; use --nc-gt-poses")
    if not nc_gt_poses:
        raise click.ClickException("Required one of --kitti-poses or --nc-gt-poses, but none was set.")
    if synthetic is None and not file:
        raise click.ClickException("give FILE or --synthetic SEED")
    from .ekf_bench import score_options
    score = score_options(map_score, score_radius, voxel_size)
    native = False
    if synthetic is None:
        from pathlib import Path
        path = Path(file)
        is_bag = (path.is_file() and path.suffix == ".bag") or path.is_dir()
        try:
            import ouster.client as client
            from ouster.sdk.util import resolve_metadata
            native = native_packets
        except Exception:
            native = True
        if native and not is_bag:
            raise click.ClickException("reading .pcap needs ouster-sdk" + ("" if native_packets else ", which is not installed")
                                       + "; a raw packet .bag (or a directory of bags) is read by the package's own decoder; "
                                       "use --synthetic SEED to build the map of a synthetic sequence")
    if rate != 1.0 or accum_map_ratio is not None:
        print("NOTE: -r / --accum-map-ratio belong to the viewer: there is no playback, and the voxel map "
              f"(voxel size {voxel_size}) replaces the random subsample")
    from .. import core, fly

    gts_poses = read_newer_college_gt(nc_gt_poses)
    scans_num = len(gts_poses)
    start_scan = start_scan if start_scan < scans_num else 0
    end_scan = end_scan if end_scan is not None and start_scan <= end_scan < scans_num else scans_num - 1
    # all poses move to the start scan's (easier to compare various trajectories), reference cli/flyby.py:96-99
    pose0_inv = np.linalg.inv(gts_poses[start_scan][1])
    gts_poses = [(t, pose0_inv @ p) for t, p in gts_poses]

    if synthetic is not None:
        from .. import synth
        seq = synth.make_sequence(seed=synthetic, n_scans=end_scan + 1)
        lut, scans = fly.synthetic_range_scans(seq, start_scan, end_scan)
    elif native:
        from .. import packets as pk
        if not meta and path.is_file() and path.with_suffix(".json").is_file():
            meta = str(path.with_suffix(".json"))
        if not meta:
            raise click.ClickException("File not found, please specify a metadata file with `-m`")
        print(f"Reading metadata from: {meta}")
        info = pk.read_metadata_json(meta)
        lut = fly.sensor_lut(info)
        bags = sorted(path.glob("*.bag")) if path.is_dir() else path
        scans = None  # (fly.add_packet_bag below: a decoded sweep carries `range` and its decoded column times)
    else:
        from ..utils import read_metadata_json, read_packet_source
        meta = resolve_metadata(file, meta)
        if not meta:
            raise click.ClickException("File not found, please specify a metadata file with `-m`")
        print(f"Reading metadata from: {meta}")
        info = read_metadata_json(meta)
        lut = fly.sensor_lut(info)

        def real_scans():
            for idx, ls in enumerate(client.Scans(read_packet_source(file, meta=info))):
                if idx > end_scan:
                    break
                if idx >= start_scan:
                    yield fly.PosedScan(ls.field(client.ChanField.RANGE), np.asarray(ls.timestamp))
        scans = real_scans()

    traj = core.Traj([t for t, _ in gts_poses], [p for _, p in gts_poses], TIME_BOUNDS, TIME_BOUNDS)
    acc = fly.MapAccumulator(lut, voxel_size=voxel_size)
    if native:
        fly.add_packet_bag(acc, bags, info, traj, start_scan, end_scan)
    else:
        for scan in scans:
            acc.update(scan, traj=traj)
    print(f"NOTE: Therere where {acc.skipped} skipped scans that wasn't "
          "because they were outside of the NC GT poses available")
    voxels, points = acc.map_size()
    print(f"map of scans: {start_scan} - {end_scan}")
    print(f"map num points: {points}")
    print(f"map voxels: {voxels} (voxel size {voxel_size})")
    scalars = None
    if score is not None:
        ms, (pts, nb, pv, ent) = acc.score(per_point=True, **score)
        scalars = (nb, pv, ent)
        print("\n".join(ms.lines()))
    if save_map:
        if scalars is not None and save_map.endswith(".npy"):
            print("NOTE: a .npy map holds the points only; give --save-map a .ply path for the per-point scores")
            scalars = None
        save_map_ply(save_map, acc.map_points() if scalars is None else pts, scalars)
        print(f"Map saved to: {save_map}")
