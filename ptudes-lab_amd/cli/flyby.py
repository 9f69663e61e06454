"""`flyby`: the headless form of reference src/ptudes/cli/flyby.py - the map its BUILDING state accumulates (cli/flyby.py:71-131,
utils.py:344-392, fly.py:75-111), without the viewer's window; `--save-frames DIR` flies the reference's camera path (to the beginning, along
the trajectory, up to the apex) and writes every frame, drawn on the GPU, as a PNG.

Every scan gets the pose of each of its columns on the trajectory of a Newer College format poses file (moved to the start scan, as the
reference does), is de-warped and accumulated - on the GPU, fused (`fly.MapAccumulator.update(scan, traj=...)`).  The map is the
deterministic voxel map of the registration path (a voxel keeps its first points), not ScansAccumulator's random subsample:
`-r` / `--accum-map-ratio` are accepted for the option set only.  What the viewer's OSD shows is printed; `--save-map` writes the points.
FILE (.pcap / .bag) goes through ouster-sdk when it is importable; a raw packet .bag (or a directory of bags) goes through the package's
own packet decoder (packets.py) when it is not, or with --native-packets - every column is then posed at its decoded firing time;
`--synthetic SEED` runs the same path on the synthetic sequence.  `--map-score` prints the sharpness of the map without ground truth
 and, with `--save-map`, adds the per-point values to the PLY.  `--compare-map REF` measures the map against a reference
cloud on the GPU: accuracy, completeness, precision / recall / F per threshold.  `--carve` passes over the same sweeps a
second time and takes the points that later rays went through - a moving object's trail - out of the map before it is saved, scored or
compared (both maps' figures are printed); `--save-carved` writes every stored point with its votes.  The frames draw the
map as accumulated.  `--color-by range|reflectivity|signal|near_ir` paints the map: a second pass over the same sweeps gives every stored point
the mean of that lidar field over the rays that ended at it; `--save-painted` writes the points with it, and the frames after the map is built
take its colours.  `--save-grid PREFIX` passes over the same sweeps once more and writes the top-down occupancy grid of the run -
free, occupied and unknown cells - as PREFIX.pgm / PREFIX.yaml.
"""
from typing import Optional

import click
import numpy as np

from ..utils import read_newer_college_gt, save_map_ply

from .ekf_bench import carve_click_options as _carve_click_options
from .ekf_bench import compare_click_options as _compare_click_options
from .ekf_bench import grid_click_options as _grid_click_options

TIME_BOUNDS = 1.5  # seconds a column may lie outside the poses file (reference utils.py:368)


def frame_options(save_frames, frame_size, fps, max_frames, point_size, edl, z_range):
    """the options of --save-frames checked before a device is touched: None without it, else a dict with the defaults filled in"""
    given = {"--frame-size": frame_size, "--fps": fps, "--max-frames": max_frames, "--point-size": point_size, "--edl": edl, "--z-range": z_range}
    if not save_frames:
        for name, v in given.items():
            if v is not None:
                raise click.ClickException(f"{name} belongs to --save-frames")
        return None
    import re
    m = re.fullmatch(r"(\d+)x(\d+)", frame_size or "1280x720")
    if not m or not (1 <= int(m.group(1)) <= 16384 and 1 <= int(m.group(2)) <= 16384):
        raise click.ClickException(f"--frame-size {frame_size}: expected WxH with both in 1 .. 16384, like 1280x720")
    out = dict(dir=save_frames, width=int(m.group(1)), height=int(m.group(2)), fps=30.0 if fps is None else fps, max_frames=max_frames,
               point_px=2 if point_size is None else point_size, edl=0.0 if edl is None else edl, z_range=None)
    if not out["fps"] > 0:
        raise click.ClickException(f"--fps {fps}: must be positive")
    if max_frames is not None and max_frames < 0:
        raise click.ClickException(f"--max-frames {max_frames}: must not be negative")
    if not 1 <= out["point_px"] <= 5:
        raise click.ClickException(f"--point-size {point_size}: must be in 1 .. 5")
    if not out["edl"] >= 0:
        raise click.ClickException(f"--edl {edl}: must not be negative")
    if z_range is not None:
        try:
            lo, hi = (float(x) for x in z_range.split(","))
        except ValueError:
            raise click.ClickException(f"--z-range {z_range}: expected LO,HI")
        if not hi > lo:
            raise click.ClickException(f"--z-range {z_range}: HI must be above LO")
        out["z_range"] = (lo, hi)
    return out


COLOR_FIELDS = ("range", "reflectivity", "signal", "near_ir")


def paint_options(color_by, color_range, save_painted, synthetic, carve, kitti_poses):
    """the options of --color-by checked before a device is touched: None without it, else dict(field, lo, hi, save)"""
    if not color_by:
        for name, v in (("--color-range", color_range), ("--save-painted", save_painted)):
            if v is not None:
                raise click.ClickException(f"{name} belongs to --color-by")
        return None
    field = color_by.lower()
    if field not in COLOR_FIELDS:
        raise click.ClickException(f"--color-by {color_by}: one of {', '.join(COLOR_FIELDS)}")
    if synthetic is not None and field != "range":
        raise click.ClickException(f"--color-by {field}: the sweeps of --synthetic are range images only, they carry no {field}; --color-by range works")
    if carve:
        raise click.ClickException(f"--color-by {field} with --carve: painting a carved map is not supported (the paint is of the map as accumulated)")
    if kitti_poses:
        raise click.ClickException(f"--color-by {field} with --kitti-poses: the paint needs the column poses of --nc-gt-poses")
    lo = hi = None
    if color_range is not None:
        try:
            lo, hi = (float(x) for x in color_range.split(","))
        except ValueError:
            raise click.ClickException(f"--color-range {color_range}: expected LO,HI")
        if not hi > lo:
            raise click.ClickException(f"--color-range {color_range}: HI must be above LO")
    if save_painted is not None and not str(save_painted).endswith(".ply"):
        raise click.ClickException(f"--save-painted {save_painted}: a .ply path (the per-point values are written to a PLY file only)")
    return dict(field=field, lo=lo, hi=hi, save=save_painted)


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
@click.option("--save-frames", required=False, type=click.Path(file_okay=False),
              help="fly the reference's camera path (to the beginning, along the trajectory, up to the apex) and write every frame, drawn on "
                   "the GPU, to this directory as frame_000000.png, ...; -r then scales the time step as in the viewer")
@click.option("--frame-size", type=str, default=None, help="frame size WxH of --save-frames (default 1280x720)")
@click.option("--fps", type=float, default=None, help="frames per second of --save-frames (default 30)")
@click.option("--max-frames", type=int, default=None, help="stop --save-frames after this many frames")
@click.option("--point-size", type=int, default=None, help="pixels per map point of --save-frames, 1 .. 5 (default 2)")
@click.option("--edl", type=float, default=None, help="eye-dome lighting strength of --save-frames (default 0: off)")
@click.option("--z-range", type=str, default=None,
              help="heights LO,HI of the palette's ends for --save-frames (default: the map's own z extent once it is built; while it is "
                   "being built, the sensor's height +- 10 m)")
@click.option("--color-by", type=str, default=None,
              help="paint the map: a second pass over the same sweeps gives every stored point the mean of this lidar field (range, "
                   "reflectivity, signal or near_ir) over the rays that ended at it, and prints the counts.  With --save-frames the frames "
                   "AFTER the map is built take the field's colours; the frames drawn while it is being built keep the height palette "
                   "(the order of the stored points moves while the map grows)")
@click.option("--color-range", type=str, default=None,
              help="field values LO,HI of the palette's ends for --color-by (default: the 1st and 99th percentile of the painted points)")
@click.option("--save-painted", required=False, type=click.Path(dir_okay=False),
              help="write every stored point with FIELD (the mean, NaN where no ray ended) and FIELD_count to this PLY file")
@_compare_click_options
@_carve_click_options
@_grid_click_options
def ptudes_flyby(file: Optional[str], meta: Optional[str], kitti_poses: Optional[str], nc_gt_poses: Optional[str], rate: float,
                 accum_map_ratio: Optional[float], start_scan: int, end_scan: Optional[int], voxel_size: float,
                 save_map: Optional[str], synthetic: Optional[int], native_packets: bool = False, map_score: bool = False,
                 score_radius: Optional[float] = None, save_frames: Optional[str] = None, frame_size: Optional[str] = None,
                 fps: Optional[float] = None, max_frames: Optional[int] = None, point_size: Optional[int] = None,
                 edl: Optional[float] = None, z_range: Optional[str] = None, compare_map: Optional[str] = None,
                 compare_threshold: Optional[str] = None, compare_max_dist: Optional[float] = None, compare_pose: Optional[str] = None,
                 save_map_error: Optional[str] = None, carve: bool = False, save_carved: Optional[str] = None,
                 carve_radius: Optional[float] = None, carve_margin: Optional[float] = None, carve_max_range: Optional[float] = None,
                 carve_min_through: Optional[int] = None, carve_min_fraction: Optional[float] = None, color_by: Optional[str] = None,
                 color_range: Optional[str] = None, save_painted: Optional[str] = None, save_grid: Optional[str] = None,
                 grid_cell: Optional[float] = None, grid_band: Optional[str] = None, grid_margin: Optional[float] = None,
                 grid_max_range: Optional[float] = None, grid_bounds: Optional[str] = None, grid_min_hits: Optional[int] = None,
                 grid_min_fraction: Optional[float] = None, save_grid_counts: Optional[str] = None) -> None:
    """Map of the lidar scans with poses (the flyby visualizer's map, headless).

    Data is provided via FILE in Ouster raw packets formats (PCAP or BAG with lidar/imu packets), or --synthetic SEED.
    """
    frames = frame_options(save_frames, frame_size, fps, max_frames, point_size, edl, z_range)
    painting = paint_options(color_by, color_range, save_painted, synthetic, carve, kitti_poses)
    from .ekf_bench import compare_options, run_compare
    compare = compare_options(compare_map, compare_threshold, compare_max_dist, compare_pose, save_map_error, voxel_size)
    from .ekf_bench import carve_options, carve_report
    carving = carve_options(carve, save_carved, carve_radius, carve_margin, carve_max_range, carve_min_through, carve_min_fraction, voxel_size,
                            bool(save_map) or map_score or compare is not None)
    from .ekf_bench import grid_builder, grid_options, grid_report
    gridding = grid_options(save_grid, grid_cell, grid_band, grid_margin, grid_max_range, grid_bounds, grid_min_hits, grid_min_fraction,
                            save_grid_counts, kitti_poses)
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
    if frames is not None:
        if accum_map_ratio is not None:
            print(f"NOTE: --accum-map-ratio belongs to the viewer's map: the voxel map (voxel size {voxel_size}) replaces the random subsample")
    elif rate != 1.0 or accum_map_ratio is not None:
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
        if painting is not None:
            try:  # (the library's table, a host function: no device is touched)
                core.pkt_field(pk.OusterPacketFormat.from_info(info), painting["field"])
            except ValueError as e:
                raise click.ClickException(f"--color-by {painting['field']}: {e}")
        lut = fly.sensor_lut(info)
        bags =sorted(path.glob("*.bag")) if path.is_dir() else path
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
                    scan = fly.PosedScan(ls.field(client.ChanField.RANGE), np.asarray(ls.timestamp))
                    if painting is not None and painting["field"] != "range":
                        scan.fields = {painting["field"]: np.asarray(ls.field(getattr(client.ChanField, painting["field"].upper())), dtype=np.uint32)}
                    yield scan
        scans = real_scans()

    traj = core.Traj([t for t, _ in gts_poses], [p for _, p in gts_poses], TIME_BOUNDS, TIME_BOUNDS)
    acc = fly.MapAccumulator(lut, voxel_size=voxel_size)
    painted = []  # the core.PaintValues of --color-by, once the pass has run

    def paint_pass():
        # the second pass over the same sweeps with their field, on the map as it stands
        painter = fly.MapPainter(acc)
        try:
            if native:
                fly.paint_packet_bag(painter, bags, info, traj, painting["field"], start_scan, end_scan)
            else:
                for scan in (scans if isinstance(scans, list) else real_scans()):
                    painter.update(scan, traj, painting["field"])
            painted.append(painter.values())
        finally:
            painter.close()
        return painted[-1]

    def point_colors():
        return fly.scalar_colors(paint_pass().mean(), painting["lo"], painting["hi"])

    if frames is not None:
        import os
        from ..utils import save_png
        if native:
            def packet_scans():
                from ..bag import OusterPacketBagSource
                feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info)
                try:
                    for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
                        if not hasattr(d, "lacc"):
                            yield d
                finally:
                    feed.close()
            scans = packet_scans()
        os.makedirs(frames["dir"], exist_ok=True)
        renderer = core.Renderer(frames["width"], frames["height"], point_px=frames["point_px"], edl=frames["edl"])

        def osd(state):
            # the lines of the viewer's OSD (reference cli/flyby.py:164-172), once per state change
            print(f"map of scans: {start_scan} - {end_scan}")
            print(f"map num points: {acc.map_size()[1]}")
            print(f"state: {state.replace('_', '..')}")
            print(f"playback: {rate}")

        fb = fly.FlyBy(acc, renderer, gts_poses, fps=frames["fps"], rate=rate, time_bounds=TIME_BOUNDS, z_range=frames["z_range"],
                       max_frames=frames["max_frames"], on_state=osd, point_colors=point_colors if painting is not None else None)
        n_written = 0
        for _, rgba in fb.frames(scans, traj=traj):
            save_png(os.path.join(frames["dir"], f"frame_{n_written:06d}.png"), rgba)
            n_written += 1
        renderer.close()
        print(f"{n_written} frames ({frames['width']}x{frames['height']}) saved to: {frames['dir']}")
    elif native:
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
    if painting is not None:
        values = painted[-1] if painted else paint_pass()  # (the frames ran the pass when they got past BUILDING)
        name = painting["field"]
        print(f"painted by {name}:")
        print("\n".join(values.lines()))
        mean = values.mean()
        if np.isfinite(mean).any():
            print(f"  {name}: mean of the painted points {float(np.nanmean(mean)):.6g}, min {float(np.nanmin(mean)):.6g}, max {float(np.nanmax(mean)):.6g}")
        if painting["save"]:
            save_map_ply(painting["save"], values.xyz, {name: mean, name + "_count": values.count})
            print(f"Painted map saved to: {painting['save']}")
    if gridding is not None:
        # the occupancy grid of the same sweeps under the same trajectory: a pass of its own, it needs no map
        builder = grid_builder(lut, gts_poses[start_scan:end_scan + 1], gridding)
        try:
            if native:
                fly.grid_packet_bag(builder, bags, info, traj, start_scan, end_scan)
            else:
                for scan in (scans if isinstance(scans, list) else real_scans()):
                    builder.update(scan, traj)
            grid_report(builder.counts(), gridding)
        finally:
            builder.close()
    if carving is not None:
        # the second pass over the same sweeps; the frames above drew the map as accumulated
        carver = fly.MapCarver(acc, **carving["cfg"])
        if native:
            fly.carve_packet_bag(carver, bags, info, traj, start_scan, end_scan)
        else:
            for scan in (scans if isinstance(scans, list) else real_scans()):
                carver.update(scan, traj)
        votes = carver.votes()
        carver.close()
        if compare is not None or score is not None:
            print("before carving:")
        if compare is not None:
            run_compare(acc.icp, dict(compare, save_error=None))
        if score is not None:
            print("\n".join(acc.score(**score).lines()))
        clean = fly.MapAccumulator.__new__(fly.MapAccumulator)
        clean.lut, clean.scans, clean.returns, clean.skipped = acc.lut, acc.scans, acc.returns, acc.skipped
        clean._icp = carve_report(acc.icp, votes, carving)
        acc.close()
        acc = clean
        if compare is not None or score is not None:
            print("after carving:")
    if compare is not None:
        run_compare(acc.icp, compare)
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
