"""`localize`: the poses of a recording's sweeps in the frame of a map saved earlier (no reference counterpart).

`--map MAP.ply` and `--keyframes POSES.csv` come from one mapping run (`ekf-bench ouster --save-map MAP.ply --save-nc-gt-poses POSES.csv`):
the map's points and poses the run went through.  Every keyframe, turned through `--yaws` headings, is a candidate start pose; the first sweep
is searched for among all of them on the GPU (`Icp.pose_hits`), the best `--top` are refined by the registration's own Gauss-Newton loop
(`Icp.align`) and scored again.  The following sweeps are tracked from the previous fixes and searched for again when fewer than
`--min-fraction` of their points lie within a voxel size of the map.  The map is never added to.
With `--places FILE.npz` (the mapping run's `--save-places`) the candidates are instead the `--place-top` places whose polar height descriptor
matches the sweep's best, each at its matched heading; `--keyframes` and `--yaws` are then not given.
SOURCE is a raw packet .bag (or a directory of bags) read by the package's own packet decoder, with `-m META`; `--synthetic SEED` runs on the
synthetic sequence instead.  The sweeps' poses are written with `--save-nc-gt-poses` / `--save-kitti-poses`."""
from typing import Optional

import click
import numpy as np

from .ekf_bench import MAP_VOXEL_SIZE, parse_synthetic_size

DEFAULTS = dict(yaws=16, top=4, min_fraction=0.5, query_voxel=1.0)  # a caller's policy, untuned (fly.MapLocalizer)
DEFAULT_PLACE_TOP = 4  # places tried per search with --places, untuned (fly.PlaceLocalizer)


def localize_options(map_path, keyframes, yaws, keyframe_spacing, top, min_fraction, query_voxel, start_scan, end_scan, places=None,
                     place_top=None):
    """the options checked before any device is touched: a dict with the defaults filled in"""
    import os
    if not map_path:
        raise click.ClickException("--map MAP.ply is needed: the map to localise in")
    if not os.path.isfile(map_path):
        raise click.ClickException(f"--map {map_path}: no such file")
    if not str(map_path).endswith((".ply", ".npy")):
        raise click.ClickException(f"--map {map_path}: expected a .ply or .npy cloud")
    if places:
        # the start poses come from a places file instead of keyframes x yaws
        for opt, v in (("--keyframes", keyframes), ("--yaws", yaws), ("--keyframe-spacing", keyframe_spacing)):
            if v is not None:
                raise click.ClickException(f"{opt} does not go with --places: the places file carries the poses, the match their headings")
        if not os.path.isfile(places):
            raise click.ClickException(f"--places {places}: no such file")
        if not str(places).endswith(".npz"):
            raise click.ClickException(f"--places {places}: expected the .npz of a mapping run's --save-places")
        if place_top is not None and place_top < 1:
            raise click.ClickException(f"--place-top {place_top}: at least one place is tried")
    else:
        if place_top is not None:
            raise click.ClickException("--place-top belongs to --places")
        if not keyframes:
            raise click.ClickException("--keyframes POSES.csv is needed: the poses of the mapping run (its --save-nc-gt-poses)")
        if not os.path.isfile(keyframes):
            raise click.ClickException(f"--keyframes {keyframes}: no such file")
    out = dict(DEFAULTS, map=map_path, keyframes=keyframes, spacing=keyframe_spacing, start_scan=start_scan, end_scan=end_scan, places=places,
               place_top=DEFAULT_PLACE_TOP if place_top is None else place_top)
    for name, opt, v in (("yaws", "--yaws", yaws), ("top", "--top", top), ("min_fraction", "--min-fraction", min_fraction),
                         ("query_voxel", "--query-voxel", query_voxel)):
        if v is not None:
            out[name] = v
    if out["yaws"] < 1:
        raise click.ClickException(f"--yaws {out['yaws']}: at least one heading per keyframe")
    if keyframe_spacing is not None and not keyframe_spacing >= 0.0:
        raise click.ClickException(f"--keyframe-spacing {keyframe_spacing:g}: must not be negative")
    if out["top"] < 1:
        raise click.ClickException(f"--top {out['top']}: at least one candidate is refined")
    if not 0.0 <= out["min_fraction"] <= 1.0:
        raise click.ClickException(f"--min-fraction {out['min_fraction']:g}: a fraction in [0, 1]")
    if not out["query_voxel"] > 0.0:
        raise click.ClickException(f"--query-voxel {out['query_voxel']:g}: must be positive")
    if start_scan < 0:
        raise click.ClickException(f"--start-scan {start_scan}: must not be negative")
    if end_scan is not None and end_scan < start_scan:
        raise click.ClickException(f"--end-scan {end_scan} lies before --start-scan {start_scan}")
    return out


def change_options(changes, cast_radius, change_margin, cast_max_range, save_changes):
    """the options of --changes, checked before any device is touched: None without --changes, else the cfg of fly.SweepDiffer"""
    if not changes:
        for opt, v in (("--save-changes", save_changes), ("--cast-radius", cast_radius), ("--change-margin", change_margin),
                       ("--cast-max-range", cast_max_range)):
            if v is not None:
                raise click.ClickException(f"{opt} belongs to --changes")
        return None
    if cast_radius is not None and not cast_radius > 0.0:
        raise click.ClickException(f"--cast-radius {cast_radius:g}: must be positive")
    if change_margin is not None and not change_margin > 0.0:
        raise click.ClickException(f"--change-margin {change_margin:g}: must be positive")
    if cast_max_range is not None and not cast_max_range > 0.0:
        raise click.ClickException(f"--cast-max-range {cast_max_range:g}: must be positive")
    return dict(radius=cast_radius, margin=change_margin, max_range=cast_max_range)


def fix_knots(t, fix):
    """the knots of the trajectory that poses a sweep for --changes: its own fix, the same pose at two knot times.  A fix is one pose per
    sweep and every column is evaluated at the sweep's time, the last knot, so an earlier fix would not enter the pose"""
    return [t - 1.0, t], [fix, fix]


@click.command(name="localize")
@click.argument("source", required=False, type=click.Path())
@click.option("-m", "--meta", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="sensor metadata .json of SOURCE (needed when it is not found next to it)")
@click.option("--synthetic", type=int, default=None, help="localise the sweeps of the synthetic sequence with this seed instead of SOURCE")
@click.option("--synthetic-size", type=str, default=None, help="beams x columns HxW of the --synthetic sweeps (default 128x1024)")
@click.option("--map", "map_path", required=False, type=click.Path(dir_okay=False),
              help="the map to localise in: the points a mapping run wrote with --save-map (.ply, or .npy)")
@click.option("--keyframes", required=False, type=click.Path(dir_okay=False),
              help="poses of the mapping run in the map's frame, Newer College format (its --save-nc-gt-poses)")
@click.option("--yaws", type=int, default=None, help=f"headings tried per keyframe (default {DEFAULTS['yaws']}, untuned)")
@click.option("--keyframe-spacing", type=float, default=None, help="keep a keyframe every this many metres of travel (default: every keyframe)")
@click.option("--top", type=int, default=None, help=f"candidates refined by the registration (default {DEFAULTS['top']}, untuned)")
@click.option("--min-fraction", type=float, default=None,
              help=f"hit fraction below which a tracked sweep is searched for again (default {DEFAULTS['min_fraction']}, untuned)")
@click.option("--query-voxel", type=float, default=None,
              help=f"side of the voxels that thin a sweep to one point each, metres (default {DEFAULTS['query_voxel']}, untuned)")
@click.option("--places", required=False, type=click.Path(dir_okay=False),
              help="places of the mapping run (its --save-places .npz): the start poses are the best-matching places at the matched heading "
                   "instead of keyframes x yaws; excludes --keyframes")
@click.option("--place-top", type=int, default=None, help=f"--places: places tried per search (default {DEFAULT_PLACE_TOP}, untuned)")
@click.option("--start-scan", type=int, default=0, help="first sweep to localise (0-based)")
@click.option("--end-scan", type=int, help="last sweep to localise (inclusive)")
@click.option("--save-nc-gt-poses", required=False, type=click.Path(exists=False, dir_okay=False),
              help="write the sweeps' poses in the map's frame, Newer College format")
@click.option("--save-kitti-poses", required=False, type=click.Path(exists=False, dir_okay=False),
              help="write the sweeps' poses in the map's frame, KITTI format")
@click.option("--changes", is_flag=True, help="cast every sweep's rays through the map at its fix and print the pixels per class "
              "(agree / new / gone / unmapped)")
@click.option("--cast-radius", type=float, default=None, help="--changes: radius of a ray, metres (default: voxel size / 5, untuned)")
@click.option("--change-margin", type=float, default=None,
              help="--changes: a measured length within this of the map's is `agree`, metres (default: the voxel size, untuned)")
@click.option("--cast-max-range", type=float, default=None, help="--changes: how far a ray is marched, metres (default: 120 voxels, untuned)")
@click.option("--save-changes", required=False, type=click.Path(file_okay=False),
              help="--changes: write changes_%06d.png per sweep into this directory, one fixed colour per class")
def ptudes_localize(source: Optional[str], meta: Optional[str], synthetic: Optional[int], synthetic_size: Optional[str],
                    map_path: Optional[str], keyframes: Optional[str], yaws: Optional[int], keyframe_spacing: Optional[float],
                    top: Optional[int], min_fraction: Optional[float], query_voxel: Optional[float], start_scan: int,
                    end_scan: Optional[int], save_nc_gt_poses: Optional[str], save_kitti_poses: Optional[str], changes: bool,
                    cast_radius: Optional[float], change_margin: Optional[float], cast_max_range: Optional[float],
                    save_changes: Optional[str], places: Optional[str] = None, place_top: Optional[int] = None) -> None:
    """Poses of the sweeps of SOURCE in the frame of a saved map."""
    diff_cfg = change_options(changes, cast_radius, change_margin, cast_max_range, save_changes)
    opts = localize_options(map_path, keyframes, yaws, keyframe_spacing, top, min_fraction, query_voxel, start_scan, end_scan, places, place_top)
    if synthetic_size is not None and synthetic is None:
        raise click.ClickException("--synthetic-size belongs to --synthetic")
    H, W = parse_synthetic_size(synthetic_size)
    if synthetic is None:
        from pathlib import Path
        if not source:
            raise click.ClickException("give SOURCE or --synthetic SEED")
        path = Path(source)
        if not ((path.is_file() and path.suffix == ".bag") or path.is_dir()):
            raise click.ClickException(f"'{source}': SOURCE is a raw packet .bag or a directory of .bag files, read by the package's own decoder; "
                                       "--synthetic SEED runs the same path on a synthetic sequence")
        if not meta and path.is_file() and path.with_suffix(".json").is_file():
            meta = str(path.with_suffix(".json"))
        if not meta:
            raise click.ClickException("File not found, please specify a metadata file with `-m`")
    from ..utils import load_map_ply, read_newer_college_gt, save_poses_kitti_format, save_poses_nc_gt_format
    kf = place_data = None
    if opts["places"]:
        from ..utils import load_places
        try:
            place_data = load_places(opts["places"])
        except ValueError as e:
            raise click.ClickException(f"--places: {e}")
        if not len(place_data["poses"]):
            raise click.ClickException(f"--places {opts['places']}: no place in the file")
    else:
        kf = read_newer_college_gt(opts["keyframes"])
        if not kf:
            raise click.ClickException(f"--keyframes {opts['keyframes']}: no pose in the file")
    map_pts = np.ascontiguousarray(load_map_ply(opts["map"]), dtype=np.float64).reshape(-1, 3)
    from .. import fly

    if synthetic is not None:
        from .. import synth
        n_scans = (end_scan + 1) if end_scan is not None else 100
        seq = synth.make_sequence(seed=synthetic, n_scans=n_scans, H=H, W=W)
        points_per_sweep, sweep_hw = H * W, (H, W)

        def sweeps():
            for k in range(start_scan, n_scans):
                yield float(seq.t_base + (k + 1) * seq.scan_dt), seq.scan(k)
    else:
        from .. import packets as pk
        from ..bag import OusterPacketBagSource
        info = pk.read_metadata_json(meta)
        lut = fly.sensor_lut(info, use_extrinsics=True)  # (the registration's: lidar_to_sensor and the extrinsic)
        bags = sorted(path.glob("*.bag")) if path.is_dir() else path
        points_per_sweep, sweep_hw = lut.H * lut.W, (lut.H, lut.W)

        def sweeps():
            feed = pk.PacketFeed(OusterPacketBagSource(bags, info), info)
            try:
                for _, d in feed.withScanIdx(start_scan=start_scan, end_scan=end_scan):
                    if not hasattr(d, "lacc"):
                        yield d.ts, lut(d.range)  # (a pixel without a return is (0, 0, 0): MapLocalizer.query drops it)
            finally:
                feed.close()

    common = dict(top=opts["top"], min_fraction=opts["min_fraction"], query_voxel=opts["query_voxel"], voxel_size=MAP_VOXEL_SIZE,
                  max_points_per_scan=max(points_per_sweep, 1 << 16), **(dict(scan_cols=sweep_hw[1]) if diff_cfg else {}))
    if place_data is not None:
        loc = fly.PlaceLocalizer(map_pts, place_data, place_top=opts["place_top"], **common)
    else:
        loc = fly.MapLocalizer(map_pts, [p for _, p in kf], n_yaw=opts["yaws"], spacing=opts["spacing"], **common)
    print(f"map: {opts['map']} ({len(map_pts)} points, voxel size {MAP_VOXEL_SIZE})")
    if place_data is not None:
        print(f"places: {opts['places']} ({len(place_data['poses'])} places), the best {opts['place_top']} per search are the candidates")
    else:
        print(f"keyframes: {opts['keyframes']} ({len(kf)} poses, {len(loc.kept)} kept) x {opts['yaws']} yaws = {len(loc.candidates)} candidates")
    res_t, res_poses, fractions = [], [], []
    differ, totals = None, {}
    try:
        if diff_cfg is not None:
            import os
            from .. import core
            from ..utils import save_png
            differ = fly.SweepDiffer(loc.icp, **{k: v for k, v in diff_cfg.items() if v is not None})
            c = differ.caster.cfg
            print(f"changes: radius {c.radius:g} m, step {c.step:g} m, range [{c.min_range:g}, {c.max_range:g}] m, margin {differ.margin:g} m")
            if save_changes:
                os.makedirs(save_changes, exist_ok=True)
        for ts, xyz in sweeps():
            fix = loc.track(xyz)
            res_t.append(ts)
            res_poses.append(fix.pose)
            fractions.append(fix.fraction)
            if differ is not None:
                kt, kp = fix_knots(ts, fix.pose)
                traj = core.Traj(kt, kp, 0.0, 0.0)
                try:
                    classes, n = differ.update_xyz(np.asarray(xyz, dtype=np.float32), sweep_hw[0], sweep_hw[1], traj, np.full(sweep_hw[1], kt[-1]))
                finally:
                    traj.close()
                k = start_scan + len(res_poses) - 1
                print(f"changes {k:06d}: " + ", ".join(f"{name} {n[name]}" for name in core.CHANGE_NAMES))
                for name, v in n.items():
                    totals[name] = totals.get(name, 0) + v
                if save_changes:
                    save_png(os.path.join(save_changes, f"changes_{k:06d}.png"), differ.image(classes))
        relocalizations, search_ms, rescore_ms, query_ms = loc.relocalizations, loc.search_ms, loc.rescore_ms, loc.query_ms
    finally:
        if differ is not None:
            differ.close()
        loc.close()
    start_from = f"places {opts['places']}" if opts["places"] else f"keyframes {opts['keyframes']}"
    header = f"localize: map {opts['map']}, {start_from}\n(sweeps num: {len(res_poses)})"
    if save_kitti_poses:
        save_poses_kitti_format(save_kitti_poses, res_poses, header=header)
        print(f"Kitti poses saved to: {save_kitti_poses}")
    if save_nc_gt_poses:
        save_poses_nc_gt_format(save_nc_gt_poses, t=res_t, poses=res_poses, header=header)
        print(f"NC GT poses saved to: {save_nc_gt_poses}")
    print(f"sweeps localised: {len(res_poses)}")
    print(f"re-localisations: {relocalizations}")
    print(f"mean hit fraction: {float(np.mean(fractions)) if fractions else 0.0:.6f}")
    print(f"search device time: {search_ms + rescore_ms:.3f} ms (candidate searches {search_ms:.3f} ms, rescoring {rescore_ms:.3f} ms)")
    if diff_cfg is not None:
        print("changes, all sweeps: " + ", ".join(f"{name} {v}" for name, v in totals.items()))
        if save_changes:
            print(f"change images saved to: {save_changes}")
    print(f"sweep thinning: {query_ms:.3f} ms of wall time (a scratch one-point-per-voxel map per sweep)")
