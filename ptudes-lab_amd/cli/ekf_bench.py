"""`ekf-bench` commands: drop-in for the pose path of reference src/ptudes/cli/ekf_bench.py.

  sim     EKF with simulated IMU (reference :107-179) - the filter's known-answer harness
  nc      Newer College bag IMU + ground-truth pose corrections (reference :183-323)
  ouster  IMU + scans -> KissICP poses -> EKF smoothing, KITTI / NC-GT pose files out (reference :381-666)
  cmp     compare trajectories in Newer College format (reference :686-760)

Same option names, printed lines and output files.  Differences, all because ouster-sdk / rosbags are not
installable offline: `ouster` reads a .pcap only when ouster-sdk is importable; a .bag (or a directory of bags) goes through
ouster-sdk when it is importable and otherwise (or with --native-packets) through the package's own packet decoder
(packets.py); --synthetic SEED runs on a synthetic 128x1024 sequence; plotting options (-p) are not provided (the
OpenGL / matplotlib viewers are outside the path).  `nc` reads the bag with the package's own ROS1 reader (bag.py)
instead of rosbags.
"""
import os
from datetime import datetime
from itertools import count
from types import SimpleNamespace
from typing import List, Optional

import click
import numpy as np
import numpy.random as npr
from scipy.spatial.transform import Rotation

from ..ins.data import GRAV, IMU, calc_ate, ekf_traj_ate
from ..ins.es_ekf import ESEKF
from ..utils import (filter_nc_gt_by_close_ts, filter_nc_gt_by_cmp, read_newer_college_gt,
                     save_poses_kitti_format, save_poses_nc_gt_format)

DOWN = np.array([0, 0, -1])
UP = np.array([0, 0, 1])


@click.group(name="ekf-bench")
def ptudes_ekf_bench() -> None:
    """ES EKF benchmarks and experiments (MI355X-native pose path)."""


def sim_imu(acc_mean=np.zeros(3), acc_std=1.5, acc_noise_std=0.4, acc_bias=np.array([0.9, -0.2, -0.4]),
            gyr_mean=np.zeros(3), gyr_std=1.0, gyr_noise_std=0.2, gyr_bias=np.array([0.01, 0.03, -0.012]),
            gravity=GRAV * DOWN, freq=100):
    """(ideal, noisy) IMU pairs; the commanded acc/gyr are redrawn every 10 samples.  Draws from the legacy
    global numpy RNG in the reference's order, so `np.random.seed(s)` reproduces its streams (reference :44-79)."""
    dt = 1 / freq

    def draw():
        a = npr.normal(0.0, acc_std, 3) + acc_mean - gravity
        g = npr.normal(0.0, gyr_std, 3) + gyr_mean
        return a, g

    acc, gyr = draw()
    for idx in count():
        if idx % 10 == 0:
            acc, gyr = draw()
        acc_noise = npr.normal(0, acc_noise_std, 3)
        gyr_noise = npr.normal(0.0, gyr_noise_std, 3)
        yield (IMU(acc, gyr, idx * dt), IMU(acc + acc_noise + acc_bias, gyr + gyr_noise + gyr_bias, idx * dt))


@click.command(name="sim")
@click.option("-t", "--duration", type=float, default=2.0, help="seconds of simulated IMU samples to run (default 2.0)")
@click.option("-f", "--freq", type=float, default=100.0, help="IMU rate, Hz")
@click.option("--corr-t", type=float, default=0.1, help="seconds between two pose corrections of the filter (default 0.1)")
@click.option("--acc-noise-std", type=float, default=0.4, help="standard deviation of the accelerometer noise")
@click.option("--gyr-noise-std", type=float, default=0.4, help="standard deviation of the gyroscope noise")
@click.option("--smooth", is_flag=True, help="also run the fixed-interval RTS smoother and print its ATE next to the filter's, "
                                             "both at the update epochs")
def ptudes_ekf_sim(duration: float, corr_t: float, freq: float, acc_noise_std: float, gyr_noise_std: float,
                   smooth: bool = False) -> None:
    """EKF with simulated IMU measurements; the noise-free filter is the ground truth for pose corrections."""
    print("Using sim IMUs with params:")
    print(f"  freq: {freq} Hz")
    print(f"  acc_noise_std: {acc_noise_std}")
    print(f"  gyr_noise_std: {gyr_noise_std}")
    print(f"  correction dt: {corr_t:.02} s")
    print("Running EKF ... \n")
    ekf_gt, ekf = ESEKF(_logging=True), ESEKF(_logging=True)
    if smooth:  # at most one update per IMU sample
        ekf.enable_smoother(int(duration * freq) + 2)
    upd_gt, upd_filt = [], []
    start_ts = last_corr_t = ts = None
    for imu_ideal, imu_noisy in sim_imu(freq=freq, acc_noise_std=acc_noise_std, gyr_noise_std=gyr_noise_std):
        ts = imu_ideal.ts
        if start_ts is None:
            start_ts = last_corr_t = ts
        ekf_gt.processImu(imu_ideal)
        ekf.processImu(imu_noisy)
        if ts - last_corr_t > corr_t:
            ekf.processPose(ekf_gt.nav.pose_mat())
            last_corr_t = ts
            if smooth:
                upd_gt.append(ekf_gt.nav.pose_mat())
                upd_filt.append(ekf.nav.pose_mat())
        if ts - start_ts > duration:
            break
    print("Results:")
    print(f"processed duration: {ts - start_ts:0.04} s")
    print(f"updates num: {len(ekf._nav_update_idxs)}\n")
    print("NAV GT:\n", ekf_gt.nav)
    print("NAV:\n", ekf.nav)
    ate_rot, ate_trans = ekf_traj_ate(ekf_gt, ekf)
    print(f"ATE_rot:   {ate_rot:.04f} deg")
    print(f"ATE trans: {ate_trans:.04f} m")
    if smooth and upd_gt:
        # RMSE in the common frame (both filters start at the identity): the first-pose alignment of the ATE above would carry the
        # smoothed first pose's own error into every GT pose
        sm = ekf.smooth(nav=False, cov=False)
        gt = np.asarray(upd_gt)
        for label, poses in (("filtered", np.asarray(upd_filt)), ("RTS smoothed", sm["poses"])):
            d_t = np.linalg.norm(poses[:, :3, 3] - gt[:, :3, 3], axis=1)
            d_r = [np.linalg.norm(Rotation.from_matrix(a[:3, :3].T @ b[:3, :3]).as_rotvec()) for a, b in zip(poses, gt)]
            print(f"RMSE at the {len(gt)} updates ({label}): rot {np.degrees(np.sqrt(np.mean(np.square(d_r)))):.06f} deg, "
                  f"trans {np.sqrt(np.mean(np.square(d_t))):.06f} m")


@click.command(name="nc")
@click.argument("file", required=True, type=click.Path(exists=True))
@click.option("-m", "--meta", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="sensor metadata .json of the BAG (unused by this command, kept for the option set)")
@click.option("-g", "--gt-file", required=True, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="Newer College ground-truth CSV: its poses correct the filter and are what the result is compared with")
@click.option("-t", "--duration", type=float, default=0.0,
              help="seconds of data to process; 0 = to the end of the bag")
@click.option("--start-ts", type=float, default=0.0,
              help="seconds to skip from the first IMU sample (default 0.0)")
@click.option("-p", "--plot", required=False, type=str, help="Plotting option [graphs, point_viz] (not provided here)")
@click.option("--xy-plot", is_flag=True, help="(plots are not provided; accepted for the option set)")
@click.option("-i", "--imu-topic", required=False, default="/os_node/imu_packets", type=str,
              help="IMU topic: a sensor_msgs/Imu topic or an Ouster imu_packets topic")
def ptudes_ekf_nc(file: str, meta: Optional[str] = None, gt_file: Optional[str] = None, duration: float = 2.0,
                  start_ts: float = 0.0, plot: Optional[str] = None, xy_plot: bool = False,
                  imu_topic: Optional[str] = None) -> None:
    """EKF with Newer College Dataset IMUs topics.

    Ground truth (--gt-file) is used for pose correction.
    """
    from .. import bag  # IMUBagSource looked up at call time, as the reference imports it inside the command (:235)

    # the Ouster IMU's nav frame has gravity along -Z, the alphasense IMU's along +Z (reference :236-239)
    ouster_frame = imu_topic in ("/os_cloud_node/imu", "/os_node/imu_packets")
    init_grav = GRAV * (DOWN if ouster_frame else UP)
    print("init_grav = ", init_grav)
    print("Reading NC dataset:")
    print(f"  file: {file}")
    print(f"  topic: {imu_topic}")
    print(f"  gt file: {gt_file}")
    source = bag.IMUBagSource(file, imu_topic=imu_topic)
    if not gt_file:
        print("need gt now")
        return
    gt_rows = read_newer_college_gt(gt_file)
    gt_stamp = [row[0] for row in gt_rows]
    last_row = len(gt_rows) - 1
    print("Running EKF ... \n")
    ekf = ESEKF(init_grav=init_grav, _logging=bool(plot))
    corrections, estimates = [], []
    row = 0          # GT row that corrects the filter next
    origin = None    # inverse of the GT pose everything is expressed relative to
    ts, t_first = 0, -1
    for imu in source:
        ts = imu.ts
        if t_first < 0:
            t_first = ts
        elapsed = ts - t_first - start_ts
        if ts - t_first < start_ts:  # --start-ts: not there yet
            continue
        if origin is None:
            # the first GT row newer than the first sample that is processed (reference :283-287; a stream that starts
            # past the last row fails here, as it does there)
            while row < len(gt_rows) and ts >= gt_stamp[row]:
                row += 1
            origin = np.linalg.inv(gt_rows[row][1])
        ekf.processImu(imu)
        if ts >= gt_stamp[row]:
            target = origin @ gt_rows[row][1]
            ekf.processPose(target)
            corrections.append(target)
            estimates.append(ekf.nav.pose_mat())
            # past the last GT row the index stays: every further IMU sample is followed by a correction with that row
            row = min(row + 1, last_row)
        if duration > 0 and elapsed > duration:
            break
    print(f"scanned duration: {ts - t_first - start_ts:0.04} s")
    print(f"updates num: {len(estimates)}\n")
    if estimates:
        ate_rot, ate_trans = calc_ate(estimates, corrections)
        print(f"ATE_rot:   {ate_rot:.04f} deg")
        print(f"ATE trans: {ate_trans:.04f} m")
    if plot:
        print(f"WARNING: plot param '{plot}' doesn't supported")


def parse_synthetic_size(text):
    """(H, W) of --synthetic-size HxW, checked before any device is touched; None gives the 128x1024 default"""
    import re
    if text is None:
        return 128, 1024
    m = re.fullmatch(r"(\d+)x(\d+)", text)
    if not m or not (1 <= int(m.group(1)) <= 1024 and 16 <= int(m.group(2)) <= 8192):
        raise click.ClickException(f"--synthetic-size {text}: expected HxW with H in 1 .. 1024 and W in 16 .. 8192, like 128x1024")
    return int(m.group(1)), int(m.group(2))


def _synthetic_source(seed: int, n_scans: int, H: int = 128, W: int = 1024):
    from .. import synth
    from ..sequence import synthetic_events
    seq = synth.make_sequence(seed=seed, n_scans=n_scans, H=H, W=W)
    meta = SimpleNamespace(format=SimpleNamespace(columns_per_frame=seq.W, pixels_per_column=seq.H),
                           prod_line=f"SYNTH-OS-0-{seq.H}", mode=f"{seq.W}x10")
    return seq, meta, synthetic_events(seq)


MAP_VOXEL_SIZE = 0.5
MAP_TIME_BOUNDS = 1.5  # as the fly-by's pose_scans_from_nc_gt (reference utils.py:368)


def _run_map_handle(seq, first, knots, voxel_size, device_id, carve=None):
    """(map handle, n_skipped): the map of `run_map`, still on the device; with carve (`carve_options`) a third entry, the core.CarveVotes of
    a second pass over the same resident sweeps"""
    from .. import core
    from ..sequence import sweep_times
    traj = core.Traj([t for t, _ in knots], [p for _, p in knots], MAP_TIME_BOUNDS, MAP_TIME_BOUNDS, device_id=device_id)
    n = seq.n_scans
    runner = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, device_id=device_id, scan_cols=seq.W)
    for k in range(first, n):
        runner.upload_scan(k, seq.scan(k))
    map_icp = core.Icp(1.0e9, 0.0, voxel_size=voxel_size, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, device_id=device_id,
                       map_block_capacity=1 << 21, map_table_capacity=1 << 23)
    _, n_skipped = runner.build_map(map_icp, traj, sweep_times(seq), first=first)
    votes = None
    if carve is not None:
        carver = core.Carver(map_icp, **carve["cfg"])
        carver.add_run(runner, traj, sweep_times(seq), first=first)
        votes = carver.votes()
        carver.close()
    for h in (runner, traj):
        h.close()
    return (map_icp, n_skipped) if carve is None else (map_icp, n_skipped, votes)


def run_map(seq, first, knots, voxel_size=MAP_VOXEL_SIZE, device_id=0):
    """The world map of sweeps [first, n_scans) of a synthetic sequence under the trajectory `knots` [(ts, pose)]: the sweeps are
    uploaded once and the map is built where they lie (SeqRunner.build_map), every column at its own pose, bounds 1.5 s.
    Returns (map points (N, 3), voxels, n_skipped)."""
    map_icp, n_skipped = _run_map_handle(seq, first, knots, voxel_size, device_id)
    voxels, _ = map_icp.map_size()
    pts = map_icp.map_points()
    map_icp.close()
    return pts, voxels, n_skipped


def _bag_map(bags, info, start_scan, end_scan, knots, voxel_size=MAP_VOXEL_SIZE, device_id=0, carve=None):
    """... of a raw packet bag: a second pass over the bag through the package's packet feed, every decoded sweep into the map by the fused
    per-call path with its decoded column times (every column posed at its own firing time).  The LUT is the registration's
    (lidar_to_sensor and the extrinsic, sequence.run_events).  Returns the fly.MapAccumulator; with carve (`carve_options`) also the
    core.CarveVotes of a third pass over the bag."""
    from .. import core, fly
    lut = fly.sensor_lut(info, use_extrinsics=True, device_id=device_id)
    traj = core.Traj([t for t, _ in knots], [p for _, p in knots], MAP_TIME_BOUNDS, MAP_TIME_BOUNDS, device_id=device_id)
    acc = fly.MapAccumulator(lut, voxel_size=voxel_size, device_id=device_id)
    fly.add_packet_bag(acc, bags, info, traj, start_scan, end_scan, device_id=device_id)
    votes = None
    if carve is not None:
        carver = fly.MapCarver(acc, **carve["cfg"])
        fly.carve_packet_bag(carver, bags, info, traj, start_scan, end_scan, device_id=device_id)
        votes = carver.votes()
        carver.close()
    traj.close()
    lut.close()  # (the sweeps are in: the map no longer needs it)
    return acc if carve is None else (acc, votes)


def _finish_map(path, map_icp, score, compare=None, carved=None):
    """points (and, with `score` = keyword arguments of Icp.map_score, the per-point scalars) of a built map to `path` (nullable);
    compare (`compare_options`): the map against the reference cloud first, printed; carved = (core.CarveVotes, `carve_options`): the
    map's figures as accumulated are printed, the votes' block, and everything that follows works on the cleaned map;
    returns (voxels, points, MapScore | None)"""
    from ..utils import save_map_ply
    if carved is not None:
        if compare is not None or score is not None:
            print("before carving:")
        if compare is not None:
            run_compare(map_icp, dict(compare, save_error=None))
        if score is not None:
            print("\n".join(map_icp.map_score(**score).lines()))
        clean = carve_report(map_icp, *carved)
        map_icp.close()
        map_icp = clean
        if compare is not None or score is not None:
            print("after carving:")
    voxels, _ = map_icp.map_size()
    if compare is not None:
        run_compare(map_icp, compare)
    ms, scalars = None, None
    if score is not None:
        ms, (pts, nb, pv, ent) = map_icp.map_score(per_point=True, **score)
        scalars = (nb, pv, ent)
    else:
        pts = map_icp.map_points()
    if path:
        if scalars is not None and str(path).endswith(".npy"):
            print("NOTE: a .npy map holds the points only; give --save-map a .ply path for the per-point scores")
            scalars = None
        save_map_ply(path, pts, scalars)
    map_icp.close()
    return voxels, len(pts), ms


def _save_run_map(path, seq, first, rows_t, rows_p, score=None, compare=None, carve=None):
    """... under the rows as the poses file holds them (utils.nc_gt_file_rows): what `flyby --nc-gt-poses` of that file works with"""
    from ..utils import nc_gt_file_rows
    map_icp, n_skipped, *votes = _run_map_handle(seq, first, nc_gt_file_rows(rows_t, rows_p), MAP_VOXEL_SIZE, 0, carve)
    voxels, points, ms = _finish_map(path, map_icp, score, compare, (votes[0], carve) if carve is not None else None)
    return voxels, points, n_skipped, ms


COMPARE_OPTIONS = [
    click.option("--compare-map", required=False, type=click.Path(dir_okay=False),
                 help="compare the map with this reference cloud (.ply as --save-map writes it, or .npy): nearest-neighbour distance in both "
                      "directions on the GPU - accuracy (map to reference), completeness (reference to map), precision / recall / F per threshold"),
    click.option("--compare-threshold", type=str, default=None,
                 help="distance thresholds T1,T2,... of --compare-map, metres, ascending, at most 8 (default 0.05,0.1,0.2)"),
    click.option("--compare-max-dist", type=float, default=None,
                 help="largest distance at which a point of --compare-map counts as matched, metres (default and upper bound: the map's voxel size)"),
    click.option("--compare-pose", required=False, type=click.Path(dir_okay=False),
                 help="text file with 12 or 16 numbers, a row-major rigid transform applied to the points of --compare-map before the comparison "
                      "(a ground-truth cloud lives in its own frame)"),
    click.option("--save-map-error", required=False, type=click.Path(dir_okay=False),
                 help="write the map's points with their distance to --compare-map's cloud (PLY, double `dist`, NaN = unmatched)"),
]


def compare_click_options(f):
    for opt in reversed(COMPARE_OPTIONS):
        f = opt(f)
    return f


def compare_options(compare_map, compare_threshold, compare_max_dist, compare_pose, save_map_error, voxel_size):
    """the options of --compare-map checked before any device is touched: None without it, else a dict with the defaults filled in"""
    import os
    given = {"--compare-threshold": compare_threshold, "--compare-max-dist": compare_max_dist, "--compare-pose": compare_pose,
             "--save-map-error": save_map_error}
    if not compare_map:
        for name, v in given.items():
            if v is not None:
                raise click.ClickException(f"{name} belongs to --compare-map")
        return None
    if not os.path.isfile(compare_map):
        raise click.ClickException(f"--compare-map {compare_map}: no such file")
    if not str(compare_map).endswith((".ply", ".npy")):
        raise click.ClickException(f"--compare-map {compare_map}: expected a .ply or .npy cloud")
    max_dist = voxel_size if compare_max_dist is None else compare_max_dist
    if not 0.0 < max_dist <= voxel_size:
        raise click.ClickException(f"--compare-max-dist {max_dist:g}: the 27-voxel neighbourhood search needs 0 < max dist <= the map's voxel size "
                                   f"{voxel_size:g}")
    try:
        thr = [float(x) for x in (compare_threshold or "0.05,0.1,0.2").split(",")]
    except ValueError:
        raise click.ClickException(f"--compare-threshold {compare_threshold}: expected T1,T2,... (numbers)")
    if not 1 <= len(thr) <= 8:
        raise click.ClickException(f"--compare-threshold {compare_threshold}: {len(thr)} thresholds, 1 .. 8 are served")
    for k, t in enumerate(thr):
        if not 0.0 < t <= max_dist:
            raise click.ClickException(f"--compare-threshold {compare_threshold}: {t:g} is outside (0, max dist = {max_dist:g}]")
        if k and t < thr[k - 1]:
            raise click.ClickException(f"--compare-threshold {compare_threshold}: {t:g} follows {thr[k - 1]:g}: ascending order")
    pose = None
    if compare_pose is not None:
        try:
            vals = [float(x) for x in open(compare_pose).read().replace(",", " ").split()]
        except (OSError, ValueError) as e:
            raise click.ClickException(f"--compare-pose {compare_pose}: {e}")
        if len(vals) not in (12, 16) or not np.all(np.isfinite(vals)):
            raise click.ClickException(f"--compare-pose {compare_pose}: {len(vals)} numbers; expected 12 or 16 finite ones, a row-major rigid transform")
        if len(vals) == 16 and vals[12:] != [0.0, 0.0, 0.0, 1.0]:
            raise click.ClickException(f"--compare-pose {compare_pose}: the last row is {vals[12:]}, a rigid transform's is 0 0 0 1")
        pose = np.array(vals[:12], dtype=np.float64).reshape(3, 4)
        if np.abs(pose[:, :3] @ pose[:, :3].T - np.eye(3)).max() > 1e-6:
            raise click.ClickException(f"--compare-pose {compare_pose}: the 3 x 3 part is not a rotation (R R^T differs from 1 by more than 1e-6)")
    return dict(path=compare_map, thresholds=thr, max_dist=max_dist, pose=pose, save_error=save_map_error)


def load_reference(compare):
    """the reference cloud of `compare_options`, moved by its pose: ((R0 x + R1 y) + R2 z) + t per row, in that order"""
    from ..utils import load_map_ply
    ref = np.ascontiguousarray(load_map_ply(compare["path"]), dtype=np.float64).reshape(-1, 3)
    T = compare["pose"]
    if T is not None:
        x, y, z = ref[:, 0], ref[:, 1], ref[:, 2]
        ref = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)
    return ref


def run_compare(map_icp, compare):
    """--compare-map: the map of `map_icp` against the reference cloud, printed; --save-map-error's file.  Returns the fly.MapComparison"""
    from .. import fly
    from ..utils import save_map_ply
    ref = load_reference(compare)
    cmp_, (pts, d2) = fly.compare_handle(map_icp, ref, compare["thresholds"], compare["max_dist"], per_point=True, reference_name=compare["path"])
    print("\n".join(cmp_.lines()))
    if compare["save_error"]:
        dist = np.sqrt(d2)
        dist[~np.isfinite(d2)] = np.nan
        save_map_ply(compare["save_error"], pts, {"dist": dist})
        print(f"Map error saved to: {compare['save_error']}")
    return cmp_


CARVE_OPTIONS = [
    click.option("--carve", is_flag=True,
                 help="after the map is built, pass over the same sweeps again and count for every stored point the rays that went through it "
                      "and the rays that ended at it (GPU); the points the policy flags as a moving object's leave the map before it is "
                      "saved, scored or compared; needs --save-map, --map-score or --compare-map"),
    click.option("--save-carved", required=False, type=click.Path(dir_okay=False),
                 help="write EVERY stored point with its votes (PLY: uint through, uint support, uchar dynamic)"),
    click.option("--carve-radius", type=float, default=None, help="a point within this distance of a ray is met by it, metres (default: voxel size / 10)"),
    click.option("--carve-margin", type=float, default=None,
                 help="a point closer than this to a ray's end along the ray supports it instead, metres (default: the voxel size)"),
    click.option("--carve-max-range", type=float, default=None, help="longest ray used, metres (default: 120 voxel sizes)"),
    click.option("--carve-min-through", type=int, default=None, help="policy: rays through a point before it can count as moving (default 2)"),
    click.option("--carve-min-fraction", type=float, default=None,
                 help="policy: share of through among the rays that met the point, through / (through + support) (default 0.5)"),
]


def carve_click_options(f):
    for opt in reversed(CARVE_OPTIONS):
        f = opt(f)
    return f


def carve_options(carve, save_carved, carve_radius, carve_margin, carve_max_range, carve_min_through, carve_min_fraction, voxel_size, have_map):
    """the options of --carve checked before any device is touched: None without it, else a dict with the policy's defaults filled in"""
    given = {"--save-carved": save_carved, "--carve-radius": carve_radius, "--carve-margin": carve_margin, "--carve-max-range": carve_max_range,
             "--carve-min-through": carve_min_through, "--carve-min-fraction": carve_min_fraction}
    if not carve:
        for name, v in given.items():
            if v is not None:
                raise click.ClickException(f"{name} belongs to --carve")
        return None
    if not have_map:
        raise click.ClickException("--carve needs a map: --save-map, --map-score or --compare-map")
    if carve_radius is not None and not carve_radius > 0.0:
        raise click.ClickException(f"--carve-radius {carve_radius:g}: must be positive")
    if carve_margin is not None and not carve_margin >= 0.0:
        raise click.ClickException(f"--carve-margin {carve_margin:g}: must not be negative")
    if carve_max_range is not None and not 0.0 < carve_max_range <= 32768.0 * voxel_size:
        raise click.ClickException(f"--carve-max-range {carve_max_range:g}: must be in (0, {32768.0 * voxel_size:g}] (65536 steps of half a voxel)")
    if carve_min_through is not None and carve_min_through < 0:
        raise click.ClickException(f"--carve-min-through {carve_min_through}: must not be negative")
    if carve_min_fraction is not None and not 0.0 <= carve_min_fraction <= 1.0:
        raise click.ClickException(f"--carve-min-fraction {carve_min_fraction:g}: must be in [0, 1]")
    if save_carved and not str(save_carved).endswith(".ply"):
        raise click.ClickException(f"--save-carved {save_carved}: the votes are written to a .ply file")
    return dict(cfg=dict(radius=carve_radius, margin=carve_margin, max_range=carve_max_range), save=save_carved,
                min_through=2 if carve_min_through is None else carve_min_through,
                min_fraction=0.5 if carve_min_fraction is None else carve_min_fraction)


def carve_report(map_icp, votes, carve):
    """--carve: prints the votes' block, writes --save-carved's file and returns the cleaned map's handle (a new core.Icp; `map_icp` stays)"""
    from .. import fly
    from ..utils import save_map_ply
    dyn = votes.dynamic(carve["min_through"], carve["min_fraction"])
    print("\n".join(votes.lines(carve["min_through"], carve["min_fraction"])))
    if carve["save"]:
        save_map_ply(carve["save"], votes.xyz, {"through": votes.through, "support": votes.support, "dynamic": dyn.astype(np.uint8)})
        print(f"Carved map saved to: {carve['save']}")
    clean = fly.carved_handle(map_icp, dyn, votes.xyz)
    print(f"map after carving: {clean.map_size()[0]} voxels, {clean.map_size()[1]} points")
    return clean


GRID_OPTIONS = [
    click.option("--save-grid", required=False, type=click.Path(dir_okay=False),
                 help="after the trajectory is known, pass over the same sweeps and write the top-down occupancy grid of the run (GPU): "
                      "PREFIX.pgm (254 free, 0 occupied, 205 unknown) with PREFIX.yaml beside it, as ROS map_server reads them; a PREFIX "
                      "ending in .png writes that PNG instead of the .pgm"),
    click.option("--grid-cell", type=float, default=None, help="cell size of --save-grid, metres (default 0.25)"),
    click.option("--grid-band", type=str, default=None,
                 help="heights LO,HI relative to the sensor between which a ray counts for --save-grid, metres (default -0.5,0.5; untuned)"),
    click.option("--grid-margin", type=float, default=None,
                 help="a ray proves free space up to this distance before its end, metres (default: the cell size; untuned)"),
    click.option("--grid-max-range", type=float, default=None, help="longest ray used, metres (default: 600 cells; untuned)"),
    click.option("--grid-bounds", type=str, default=None,
                 help="X0,Y0,X1,Y1 of the grid in the trajectory's frame, metres (default: the trajectory's positions padded by --grid-max-range)"),
    click.option("--grid-min-hits", type=int, default=None, help="policy: rays that ended in a cell before it can count as occupied (default 2; untuned)"),
    click.option("--grid-min-fraction", type=float, default=None,
                 help="policy: share of hits among the rays that met the cell, hit / (hit + free) (default 0.25; untuned)"),
    click.option("--save-grid-counts", required=False, type=click.Path(dir_okay=False),
                 help="also write the counts of the touched box to this .npz: free, hit, classes (0 free, 1 occupied, 2 unknown), cell, origin"),
]
GRID_CELL = 0.25


def grid_click_options(f):
    for opt in reversed(GRID_OPTIONS):
        f = opt(f)
    return f


def _numbers(name, text, n, what):
    try:
        vals = [float(x) for x in text.split(",")]
    except ValueError:
        vals = []
    if len(vals) != n or not all(np.isfinite(vals)):
        raise click.ClickException(f"{name} {text}: expected {what}")
    return vals


def grid_options(save_grid, grid_cell, grid_band, grid_margin, grid_max_range, grid_bounds, grid_min_hits, grid_min_fraction, save_grid_counts,
                 kitti_poses=None):
    """the options of --save-grid checked before any device is touched: None without it, else a dict with the policy's defaults filled in"""
    given = {"--grid-cell": grid_cell, "--grid-band": grid_band, "--grid-margin": grid_margin, "--grid-max-range": grid_max_range,
             "--grid-bounds": grid_bounds, "--grid-min-hits": grid_min_hits, "--grid-min-fraction": grid_min_fraction,
             "--save-grid-counts": save_grid_counts}
    if not save_grid:
        for name, v in given.items():
            if v is not None:
                raise click.ClickException(f"{name} belongs to --save-grid")
        return None
    if kitti_poses:
        raise click.ClickException("--save-grid with --kitti-poses: the grid needs the column poses of --nc-gt-poses")
    cell = GRID_CELL if grid_cell is None else grid_cell
    if not (cell > 0.0 and np.isfinite(cell)):
        raise click.ClickException(f"--grid-cell {cell:g}: must be positive")
    z_lo = z_hi = None
    if grid_band is not None:
        z_lo, z_hi = _numbers("--grid-band", grid_band, 2, "LO,HI")
        if not z_lo <= z_hi:
            raise click.ClickException(f"--grid-band {grid_band}: LO must not be above HI")
    if grid_margin is not None and not grid_margin >= 0.0:
        raise click.ClickException(f"--grid-margin {grid_margin:g}: must not be negative")
    if grid_max_range is not None and not 0.0 < grid_max_range <= 32768.0 * cell:
        raise click.ClickException(f"--grid-max-range {grid_max_range:g}: must be in (0, {32768.0 * cell:g}] (65536 steps of half a cell)")
    bounds = None
    if grid_bounds is not None:
        bounds = tuple(_numbers("--grid-bounds", grid_bounds, 4, "X0,Y0,X1,Y1"))
        if not (bounds[2] > bounds[0] and bounds[3] > bounds[1]):
            raise click.ClickException(f"--grid-bounds {grid_bounds}: X1 must be above X0 and Y1 above Y0")
        nx, ny = int(np.ceil((bounds[2] - bounds[0]) / cell)), int(np.ceil((bounds[3] - bounds[1]) / cell))
        if nx * ny > 1 << 26:
            raise click.ClickException(f"--grid-bounds {grid_bounds}: {nx} x {ny} = {nx * ny} cells of {cell:g} m, the limit is {1 << 26} (2^26)")
    if grid_min_hits is not None and grid_min_hits < 0:
        raise click.ClickException(f"--grid-min-hits {grid_min_hits}: must not be negative")
    if grid_min_fraction is not None and not 0.0 <= grid_min_fraction <= 1.0:
        raise click.ClickException(f"--grid-min-fraction {grid_min_fraction:g}: must be in [0, 1]")
    if save_grid_counts and not str(save_grid_counts).endswith(".npz"):
        raise click.ClickException(f"--save-grid-counts {save_grid_counts}: the counts are written to a .npz file")
    return dict(prefix=save_grid, cell=cell, bounds=bounds, cfg=dict(z_lo=z_lo, z_hi=z_hi, margin=grid_margin, max_range=grid_max_range),
                min_hits=2 if grid_min_hits is None else grid_min_hits,
                min_fraction=0.25 if grid_min_fraction is None else grid_min_fraction, counts=save_grid_counts)


def grid_builder(lut, knots, grid):
    """the fly.GridBuilder of --save-grid (`grid_options`): --grid-bounds, else the positions of `knots` [(ts, pose)] padded by the longest ray;
    a grid too large is refused with its cell count"""
    from .. import fly
    try:
        return fly.GridBuilder(lut, grid["bounds"] if grid["bounds"] is not None else list(knots), grid["cell"], **grid["cfg"])
    except ValueError as e:
        raise click.ClickException(f"--save-grid: {e}")


def grid_report(counts, grid):
    """--save-grid: prints the counts' block and writes the files"""
    from ..utils import save_occupancy_map
    print("\n".join(counts.lines(grid["min_hits"], grid["min_fraction"])))
    classes = counts.classify(grid["min_hits"], grid["min_fraction"])
    image, yaml = save_occupancy_map(grid["prefix"], classes, counts.cell, counts.origin)
    print(f"Occupancy grid saved to: {image}, {yaml}")
    if grid["counts"]:
        np.savez(grid["counts"], free=counts.free, hit=counts.hit, classes=classes, cell=counts.cell, origin=np.asarray(counts.origin))
        print(f"Grid counts saved to: {grid['counts']}")


def _run_grid(seq, first, knots, grid, device_id=0):
    """--save-grid of a synthetic sequence: the sweeps [first, n_scans) are uploaded once and counted where they lie (OccupancyGrid.add_run),
    every column at its own pose, bounds 1.5 s; returns the core.GridCounts of the touched box"""
    from .. import core
    from ..sequence import sweep_times
    builder = grid_builder((seq.H, seq.W), knots, grid)
    traj = core.Traj([t for t, _ in knots], [p for _, p in knots], MAP_TIME_BOUNDS, MAP_TIME_BOUNDS, device_id=device_id)
    runner = core.SeqRunner(seq.n_scans, seq.H * seq.W, 0, with_ekf=False, device_id=device_id, scan_cols=seq.W)
    for k in range(first, seq.n_scans):
        runner.upload_scan(k, seq.scan(k))
    builder.add_run(runner, traj, sweep_times(seq), first=first)
    counts = builder.counts()
    for h in (runner, traj, builder):
        h.close()
    return counts


def _bag_grid(bags, info, start_scan, end_scan, knots, grid, device_id=0):
    """... of a raw packet bag: a pass over the bag through the package's packet feed, as `_bag_map` makes it"""
    from .. import core, fly
    lut = fly.sensor_lut(info, use_extrinsics=True, device_id=device_id)
    builder = grid_builder(lut, knots, grid)
    traj = core.Traj([t for t, _ in knots], [p for _, p in knots], MAP_TIME_BOUNDS, MAP_TIME_BOUNDS, device_id=device_id)
    fly.grid_packet_bag(builder, bags, info, traj, start_scan, end_scan, device_id=device_id)
    counts = builder.counts()
    for h in (traj, builder, lut):
        h.close()
    return counts


LOOP_OPTIONS = [
    click.option("--find-loops", is_flag=True,
                 help="after the run, describe a sweep every --loop-spacing metres of the filter's trajectory (polar height descriptors, GPU), "
                      "compare every one with all earlier ones at every heading, verify the best pairs by registration and print the accepted "
                      "loops with the odometry's discrepancy at each; every threshold is the caller's and untuned"),
    click.option("--loop-spacing", type=float, default=None, help="metres of travel between described sweeps (default 2; untuned)"),
    click.option("--loop-min-gap", type=int, default=None, help="a sweep is only compared with those at least this many described sweeps "
                                                                "before it (default 50; untuned)"),
    click.option("--loop-max-cell-dist", type=float, default=None,
                 help="policy: largest descriptor distance per occupied cell, dist / (cells_i + cells_j), of a pair worth verifying "
                      "(default 20; untuned)"),
    click.option("--loop-min-fraction", type=float, default=None,
                 help="policy: share of a sweep's points that must lie within a voxel of the other sweep's after registration (default 0.5; untuned)"),
    click.option("--save-loops", required=False, type=click.Path(dir_okay=False), help="write every verified pair to this .csv"),
    click.option("--save-places", required=False, type=click.Path(dir_okay=False),
                 help="write the described sweeps' descriptors with their poses and stamps to this .npz (what `localize --places` reads); "
                      "works without --find-loops too"),
]


def loop_click_options(f):
    for opt in reversed(LOOP_OPTIONS):
        f = opt(f)
    return f


def loop_options(find_loops, loop_spacing, loop_min_gap, loop_max_cell_dist, loop_min_fraction, save_loops, save_places):
    """the options of --find-loops / --save-places checked before any device is touched: None without either, else a dict with the policy's
    (untuned) defaults filled in"""
    given = {"--loop-min-gap": loop_min_gap, "--loop-max-cell-dist": loop_max_cell_dist, "--loop-min-fraction": loop_min_fraction,
             "--save-loops": save_loops}
    if not find_loops:
        for name, v in given.items():
            if v is not None:
                raise click.ClickException(f"{name} belongs to --find-loops")
        if not save_places:
            if loop_spacing is not None:
                raise click.ClickException("--loop-spacing belongs to --find-loops or --save-places")
            return None
    spacing = 2.0 if loop_spacing is None else loop_spacing
    if not (spacing >= 0.0 and np.isfinite(spacing)):
        raise click.ClickException(f"--loop-spacing {spacing:g}: must not be negative")
    if loop_min_gap is not None and loop_min_gap < 0:
        raise click.ClickException(f"--loop-min-gap {loop_min_gap}: must not be negative")
    if loop_max_cell_dist is not None and not loop_max_cell_dist >= 0.0:
        raise click.ClickException(f"--loop-max-cell-dist {loop_max_cell_dist:g}: must not be negative")
    if loop_min_fraction is not None and not 0.0 <= loop_min_fraction <= 1.0:
        raise click.ClickException(f"--loop-min-fraction {loop_min_fraction:g}: must be in [0, 1]")
    if save_loops and not str(save_loops).endswith(".csv"):
        raise click.ClickException(f"--save-loops {save_loops}: the loops are written to a .csv file")
    if save_places and not str(save_places).endswith(".npz"):
        raise click.ClickException(f"--save-places {save_places}: the places are written to a .npz file")
    return dict(find=bool(find_loops), spacing=spacing, min_gap=50 if loop_min_gap is None else loop_min_gap,
                max_cell_dist=20.0 if loop_max_cell_dist is None else loop_max_cell_dist,
                min_fraction=0.5 if loop_min_fraction is None else loop_min_fraction, save=save_loops, places=save_places)


def loop_report(finder, loops_opt):
    """--find-loops / --save-places once every sweep has been added: prints the loops' block and writes the files"""
    from .. import fly
    from ..utils import save_places
    print(f"Places: {len(finder.poses)} sweeps described, one per {loops_opt['spacing']:g} m")
    if loops_opt["find"]:
        loops = finder.find(min_gap=loops_opt["min_gap"], max_cell_dist=loops_opt["max_cell_dist"], min_fraction=loops_opt["min_fraction"])
        print("\n".join(fly.loop_lines(loops)))
        if loops_opt["save"]:
            fly.save_loops_csv(loops_opt["save"], loops, finder.stamps)
            print(f"Loops saved to: {loops_opt['save']}")
    if loops_opt["places"]:
        save_places(loops_opt["places"], finder.index, finder.poses, finder.stamps)
        print(f"Places saved to: {loops_opt['places']}")


def _run_loops(seq, first, rows_t, rows_p, loops_opt, device_id=0):
    """--find-loops of a synthetic sequence: sweep first + k at the k-th pose of the run"""
    from .. import fly
    finder = fly.LoopFinder(spacing=loops_opt["spacing"], device_id=device_id, max_points_per_scan=seq.H * seq.W)
    try:
        for k, (t, p) in enumerate(zip(rows_t, rows_p)):
            finder.add(seq.scan(first + k), p, t)
        loop_report(finder, loops_opt)
    finally:
        finder.close()


def _bag_loops(bags, info, start_scan, end_scan, rows_t, rows_p, loops_opt, device_id=0):
    """... of a raw packet bag: a pass over the bag through the package's packet feed, sweep k at the k-th pose of the run"""
    from .. import fly
    lut = fly.sensor_lut(info, use_extrinsics=True, device_id=device_id)
    finder = fly.LoopFinder(spacing=loops_opt["spacing"], lut=lut, device_id=device_id, max_points_per_scan=lut.H * lut.W)
    try:
        fly.loops_packet_bag(finder, bags, info, rows_t, rows_p, start_scan, end_scan, device_id=device_id)
        loop_report(finder, loops_opt)
    finally:
        finder.close()
        lut.close()


def score_options(map_score, score_radius, voxel_size):
    """the keyword arguments of Icp.map_score for --map-score / --score-radius, or None; refusals before any device is touched"""
    if score_radius is not None and not map_score:
        raise click.ClickException("--score-radius belongs to --map-score")
    if not map_score:
        return None
    if score_radius is not None and not 0.0 < score_radius <= voxel_size:
        raise click.ClickException(f"--score-radius {score_radius:g}: the 27-voxel neighbourhood search needs 0 < radius <= the map's voxel size "
                                   f"{voxel_size:g}")
    return dict(radius=score_radius)


@click.command(name="ouster")
@click.argument("file", required=False, type=click.Path())
@click.option("-m", "--meta", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="sensor metadata .json of the PCAP / BAG (needed when it is not found next to FILE)")
@click.option("--start-scan", type=int, default=0, help="first scan to use (0-based)")
@click.option("--end-scan", type=int, help="last scan to use (inclusive)")
@click.option("-p", "--plot", required=False, type=str,
              help="Plotting option [graphs, point_viz]: `graphs` prints the ground-truth comparison; the figures and the "
                   "viewer themselves are not part of this build")
@click.option("--use-imu-prediction", is_flag=True,
              help="hand the filter's predicted pose to KissICP as initial guess (loosely coupled lidar-inertial odometry)")
@click.option("--use-gt-guess", is_flag=True,
              help="hand the ground-truth pose (--gt-file, interpolated at the scan's timestamp) to KissICP as initial "
                   "guess (sanity testing only)")
@click.option("-g", "--gt-file", required=False, type=click.Path(exists=True, dir_okay=False, readable=True),
              help="Newer College ground-truth CSV to compare the result with")
@click.option("--kiss-min-range", type=float, default=1, help="KissICP: shortest range kept, metres (default 1)")
@click.option("--kiss-max-range", type=float, default=70, help="KissICP: longest range kept, metres (default 70)")
@click.option("--beams", type=int, default=0, help="keep only NUM evenly spaced beams (rows) of every scan; 0 = all")
@click.option("--save-kitti-poses", required=False, type=click.Path(exists=False, dir_okay=False),
              help="write the resulting poses to this file, KITTI format")
@click.option("--save-nc-gt-poses", required=False, type=click.Path(exists=False, dir_okay=False),
              help="write the resulting poses to this file, Newer College ground-truth format")
@click.option("--synthetic", type=int, default=None,
              help="Run on the synthetic 128x1024 sequence with this seed instead of FILE (no ouster-sdk needed)")
@click.option("--synthetic-size", type=str, default=None, help="beams x columns HxW of the --synthetic sweeps (default 128x1024)")
@click.option("--native-packets", is_flag=True,
              help="read FILE (.bag, or a directory of bags) with the package's own packet decoder also when ouster-sdk is installed "
                   "(without ouster-sdk this is what happens anyway)")
@click.option("--save-smoothed-poses", required=False, type=click.Path(exists=False, dir_okay=False),
              help="also run the fixed-interval RTS smoother over the whole run and write its poses to this file, Newer College "
                   "ground-truth format, with the timestamps of --save-nc-gt-poses; with -g, print its ATE")
@click.option("--imu-deskew", is_flag=True,
              help="deskew every sweep with the filter's IMU-propagated trajectory instead of KissICP's constant-velocity model "
                   "(the fused loop only; the call-by-call form, e.g. with -p, stays constant-velocity); needs --synthetic: "
                   "the sweep times of real recordings are not decoded here")
@click.option("--save-map", required=False, type=click.Path(dir_okay=False),
              help="after the run, build the world map of the sweeps (voxel size 0.5) with the poses of --map-from as they stand in the "
                   "poses file, every column at its own pose, and write its points to this file (PLY, or .npy); needs --synthetic or a "
                   "raw packet .bag read by the package's own decoder (its column times are decoded)")
@click.option("--map-from", type=click.Choice(["filter", "kiss", "smoothed"]), default="filter",
              help="trajectory of --save-map: the filter's poses (default), KissICP's own, or the RTS smoothed ones "
                   "(needs --save-smoothed-poses)")
@click.option("--map-score", is_flag=True,
              help="score the sharpness of that map without ground truth (mean plane variance and mean map entropy of the stored points' "
                   "neighbourhoods) and print it; with --save-map the PLY carries the per-point values; works without --save-map too")
@click.option("--score-radius", type=float, default=None, help="neighbourhood radius of --map-score, metres (default and upper bound: the "
                                                               "map's voxel size, 0.5)")
@compare_click_options
@carve_click_options
@grid_click_options
@loop_click_options
def ptudes_ekf_ouster(file: Optional[str], meta: Optional[str], start_scan: int, end_scan: Optional[int],
                      plot: Optional[str], use_imu_prediction: bool, use_gt_guess: bool, gt_file: Optional[str], beams: int,
                      save_kitti_poses: Optional[str], save_nc_gt_poses: Optional[str], kiss_min_range: float,
                      kiss_max_range: float, synthetic: Optional[int], save_smoothed_poses: Optional[str] = None,
                      imu_deskew: bool = False, save_map: Optional[str] = None, map_from: str = "filter",
                      native_packets: bool = False, map_score: bool = False, score_radius: Optional[float] = None,
                      compare_map: Optional[str] = None, compare_threshold: Optional[str] = None, compare_max_dist: Optional[float] = None,
                      compare_pose: Optional[str] = None, save_map_error: Optional[str] = None, carve: bool = False,
                      save_carved: Optional[str] = None, carve_radius: Optional[float] = None, carve_margin: Optional[float] = None,
                      carve_max_range: Optional[float] = None, carve_min_through: Optional[int] = None,
                      carve_min_fraction: Optional[float] = None, synthetic_size: Optional[str] = None,
                      save_grid: Optional[str] = None, grid_cell: Optional[float] = None, grid_band: Optional[str] = None,
                      grid_margin: Optional[float] = None, grid_max_range: Optional[float] = None, grid_bounds: Optional[str] = None,
                      grid_min_hits: Optional[int] = None, grid_min_fraction: Optional[float] = None,
                      save_grid_counts: Optional[str] = None, find_loops: bool = False, loop_spacing: Optional[float] = None,
                      loop_min_gap: Optional[int] = None, loop_max_cell_dist: Optional[float] = None,
                      loop_min_fraction: Optional[float] = None, save_loops: Optional[str] = None,
                      save_places: Optional[str] = None) -> None:
    """EKF with Ouster IMUs and scan KissICP poses updates (smoothing of the KissICP trajectory)."""
    if synthetic_size is not None and synthetic is None:
        raise click.ClickException("--synthetic-size belongs to --synthetic")
    synth_hw = parse_synthetic_size(synthetic_size)
    from ..ins.data import StreamStatsTracker
    from ..sequence import run_events
    from ..utils import TrajectoryEvaluator, active_beam_rows
    score = score_options(map_score, score_radius, MAP_VOXEL_SIZE)
    compare = compare_options(compare_map, compare_threshold, compare_max_dist, compare_pose, save_map_error, MAP_VOXEL_SIZE)
    want_map = bool(save_map) or map_score or compare is not None
    carving = carve_options(carve, save_carved, carve_radius, carve_margin, carve_max_range, carve_min_through, carve_min_fraction, MAP_VOXEL_SIZE,
                            want_map)
    gridding = grid_options(save_grid, grid_cell, grid_band, grid_margin, grid_max_range, grid_bounds, grid_min_hits, grid_min_fraction,
                            save_grid_counts)
    looping = loop_options(find_loops, loop_spacing, loop_min_gap, loop_max_cell_dist, loop_min_fraction, save_loops, save_places)
    # (the grid and the places are products of the same kind: a second pass over the sweeps)
    want_sweeps = want_map or gridding is not None or looping is not None
    if want_sweeps and map_from == "smoothed" and not save_smoothed_poses:
        raise click.ClickException("--map-from smoothed needs the smoother (--save-smoothed-poses)")
    if imu_deskew and (synthetic is None or plot):
        raise click.ClickException("--imu-deskew needs --synthetic and the fused loop (no -p)")
    if not gt_file and use_gt_guess:  # reference :416-418
        print("ERROR: --use-gt-guess requires the GT poses (--gt-file)")
        raise SystemExit(1)
    have_sdk = False
    if synthetic is None:
        try:
            import ouster.client  # noqa: F401
            from ouster.sdk.util import resolve_metadata
            have_sdk = True
        except Exception:
            pass
    if want_sweeps and synthetic is None:
        from pathlib import Path
        native_bag = bool(file) and (native_packets or not have_sdk) and ((Path(file).is_file() and Path(file).suffix == ".bag") or Path(file).is_dir())
        if not native_bag:
            raise click.ClickException("--save-map needs --synthetic or a raw packet .bag read by the package's own decoder (--native-packets): "
                                       "the sweep times of other recordings are not decoded here (the same holds for --map-score, --save-grid, --find-loops "
                                       "and --save-places)")
    bags = None
    if synthetic is None and (native_packets or not have_sdk):
        # the package's own feed (packets.py): raw payloads from the bag(s), batched on the host, decoded on the device
        from pathlib import Path
        from .. import packets as pk
        from ..bag import OusterPacketBagSource
        path = Path(file) if file else None
        if path is None or not ((path.is_file() and path.suffix == ".bag") or path.is_dir()):
            raise click.ClickException(f"'{file}': without ouster-sdk (or with --native-packets) FILE is a .bag or a directory of .bag files; "
                                       "reading .pcap needs ouster-sdk" + ("" if have_sdk else ", which is not installed")
                                       + " (IP-fragment reassembly is not built here); --synthetic SEED runs the same path on a synthetic sequence")
        if not meta and path.is_file() and path.with_suffix(".json").is_file():
            meta = str(path.with_suffix(".json"))
        if not meta:
            raise click.ClickException("File not found, please specify a metadata file with `-m`")
        info = pk.read_metadata_json(meta)
        bags = sorted(path.glob("*.bag")) if path.is_dir() else path
        data_source = pk.PacketFeed(OusterPacketBagSource(bags, info), info)
        seq = None
        events = ((("imu", d) if hasattr(d, "lacc") else ("lidar_scan", d))
                  for _, d in data_source.withScanIdx(start_scan=start_scan, end_scan=end_scan))
        start_scan_feed = 0  # withScanIdx already applied the range
    elif synthetic is None:
        # the reference's feed (ekf_bench.py:426-448): packets -> OusterLidarData -> (scan idx, LidarScan | IMU)
        from ..data import OusterLidarData
        from ..utils import read_metadata_json, read_packet_source
        meta = resolve_metadata(file, meta)
        if not meta:
            raise click.ClickException("File not found, please specify a metadata file with `-m`")
        info = read_metadata_json(meta)
        data_source = OusterLidarData(read_packet_source(file, meta=info))
        seq = None
        events = ((("imu", d) if hasattr(d, "lacc") else ("lidar_scan", d))
                  for _, d in data_source.withScanIdx(start_scan=start_scan, end_scan=end_scan))
        start_scan_feed = 0  # withScanIdx already applied the range
    else:
        n_scans = (end_scan + 1) if end_scan is not None else 100
        seq, info, events = _synthetic_source(synthetic, n_scans, *synth_hw)
        start_scan_feed = start_scan
    if synthetic is not None:
        file = f"synthetic:{synthetic}"
    display_header = f"data path: {file}\n"
    display_header += f"metadata path: {meta}\n\n"
    display_header += f"scans range: {start_scan} - {end_scan}\n"
    display_header += f"kiss min/max: {kiss_min_range} - {kiss_max_range}\n"
    display_header += f"use-imu-prediction: {use_imu_prediction}, use-gt-guess: {use_gt_guess}\n"
    display_header += f"beams: {beams or info.format.pixels_per_column}\n"
    display_header += f"sensor: {info.prod_line}, {info.mode}\n"
    print(display_header)
    log_metrics = bool(plot)
    print(f"metrics logging: {log_metrics}")

    # --use-gt-guess (reference :486-489, :536-542): the GT pose at the scan's last column, relative to the first one used
    gts = read_newer_college_gt(gt_file) if gt_file else []
    guess_fn = None
    if use_gt_guess:
        gt_traj = TrajectoryEvaluator(gts, time_bounds=1.0)
        origin = []

        def guess_fn(ts):
            gt_guess = gt_traj.pose_at(ts)
            if not origin:
                origin.append(np.linalg.inv(gt_guess))
            return origin[0] @ gt_guess

    def feed():
        scan_idx = 0
        for ev in events:
            if ev[0] == "scan":
                if scan_idx >= start_scan_feed:
                    xyz = ev[1]
                    if beams:
                        img = xyz.reshape(seq.H, seq.W, 3)
                        drop = np.ones(seq.H, dtype=bool)
                        drop[active_beam_rows(seq.H, beams)] = False
                        img[drop] = 0
                    yield ev
                scan_idx += 1
            elif ev[0] == "lidar_scan":  # ouster LidarScan (the packet feed applied start_scan / end_scan)
                if beams:
                    from ..utils import reduce_active_beams
                    # reference ekf_bench.py:520-521 (a packets.PacketScan: its range image)
                    reduce_active_beams(ev[1] if hasattr(ev[1], "field") else ev[1].range, beams)
                yield ev
            elif scan_idx >= start_scan_feed:  # IMUs before start_scan are dropped (reference data.py:76)
                yield ev

    stats = StreamStatsTracker(use_beams_num=32, metadata=info)  # reference :457
    out = run_events(feed(), info, kiss_min_range=kiss_min_range, kiss_max_range=kiss_max_range,
                     use_imu_prediction=use_imu_prediction, guess_fn=guess_fn, logging=log_metrics, stats=stats,
                     smooth=bool(save_smoothed_poses), imu_deskew=imu_deskew,
                     sweep_time_fn=(lambda ts: (ts - seq.scan_dt, ts)) if imu_deskew else None)
    res_t, res_poses, kiss_poses = out["res_t"], out["res_poses"], out["kiss_poses"]
    header = display_header + f"(scans/updates num: {len(res_poses)})\n"
    header += "time: " + datetime.now().strftime("%Y%m%d_%H%M%S")
    if save_kitti_poses:
        save_poses_kitti_format(save_kitti_poses, res_poses, header=header)
        print(f"Kitti poses saved to: {save_kitti_poses}")
    if save_nc_gt_poses:
        save_poses_nc_gt_format(save_nc_gt_poses, t=res_t, poses=res_poses, header=header)
        print(f"NC GT poses saved to: {save_nc_gt_poses}")
    if save_smoothed_poses:
        sm_t, sm_poses = list(out["smoothed_t"]), list(out["smoothed_poses"])
        save_poses_nc_gt_format(save_smoothed_poses, t=sm_t, poses=sm_poses, header=header)  # (stdout: only the ATE line below)
        if gts and sm_poses:
            gts_m, t_matched = filter_nc_gt_by_close_ts(gts, sm_t)
            if gts_m:
                at = {t: p for t, p in zip(sm_t, sm_poses)}
                sm_m = [at[t] for t in t_matched]
                pose0 = sm_m[0] @ np.linalg.inv(gts_m[0][1])
                ate_rot, ate_trans = calc_ate(sm_m, [pose0 @ g[1] for g in gts_m])
                print(f"ATE of the RTS smoothed poses ({len(gts_m)} poses): rot {ate_rot:.04f} deg, trans {ate_trans:.04f} m")
    if want_map:
        rows_t, rows_p = {"filter": (res_t, res_poses), "kiss": (res_t, kiss_poses),
                          "smoothed": (out.get("smoothed_t"), out.get("smoothed_poses"))}[map_from]
        if seq is not None:
            voxels, points, n_skipped, ms = _save_run_map(save_map, seq, start_scan, list(rows_t), list(rows_p), score=score, compare=compare,
                                                           carve=carving)
            print(f"Map of scans {start_scan} - {seq.n_scans - 1} ({map_from} poses, {n_skipped} skipped): {voxels} voxels, {points} points")
        else:
            from ..utils import nc_gt_file_rows
            if len(rows_t) < 2:
                raise click.ClickException("the map needs a trajectory of at least two poses")
            if beams:
                print("NOTE: --beams thins the scans of the registration only; the map takes every beam of every sweep")
            acc = _bag_map(bags, info, start_scan, end_scan, nc_gt_file_rows(list(rows_t), list(rows_p)), carve=carving)
            votes = None
            if carving is not None:
                acc, votes = acc
            voxels, points, ms = _finish_map(save_map, acc.icp, score, compare, (votes, carving) if carving is not None else None)
            print(f"Map of {acc.scans} scans from {start_scan} ({map_from} poses, {acc.skipped} skipped): {voxels} voxels, {points} points")
        if ms is not None:
            print("\n".join(ms.lines()))
        if save_map:
            print(f"Map saved to: {save_map}")
    if gridding is not None:
        # the occupancy grid of the same sweeps under the same trajectory; it needs no map
        from ..utils import nc_gt_file_rows
        rows_t, rows_p = {"filter": (res_t, res_poses), "kiss": (res_t, kiss_poses),
                          "smoothed": (out.get("smoothed_t"), out.get("smoothed_poses"))}[map_from]
        if len(rows_t) < 2:
            raise click.ClickException("the grid needs a trajectory of at least two poses")
        knots = nc_gt_file_rows(list(rows_t), list(rows_p))
        if seq is not None:
            grid_report(_run_grid(seq, start_scan, knots, gridding), gridding)
        else:
            grid_report(_bag_grid(bags, info, start_scan, end_scan, knots, gridding), gridding)
    if looping is not None:
        # revisited places along the filter's trajectory: sweep k of the run at its k-th pose
        if seq is not None:
            _run_loops(seq, start_scan, list(res_t), list(res_poses), looping)
        else:
            _bag_loops(bags, info, start_scan, end_scan, list(res_t), list(res_poses), looping)
    tm = out["timings"]
    if tm["n_imu"] and tm["n_corr"]:  # reference :590-595
        print("\nTimings:")
        print(f"  ESEKF imu process:      {tm['imu']:.05f} s per step")
        print(f"  ESEKF update:           {tm['corr']:.05f} s per update")
        print(f"  KissICP register frame: {tm['kiss']:.05f} s per frame")
        print(f"  Stats tracking:         {tm['track']:.05f} s per frame")
    if plot == "graphs":  # reference :599-660: the comparison is printed, the figures are not drawn here
        if gts and res_poses:
            gts, res_t_matched = filter_nc_gt_by_close_ts(gts, res_t)
            idx, kiss_m, res_m = 0, [], []
            for t_m in res_t_matched:
                while res_t[idx] != t_m:
                    idx += 1
                kiss_m.append(kiss_poses[idx])
                res_m.append(res_poses[idx])
                idx += 1
            if gts:
                pose0 = res_m[0] @ np.linalg.inv(gts[0][1])
                gt2 = [pose0 @ g[1] for g in gts]
                for label, poses in ((f"with ES EKF smoothing {len(gt2)} poses", res_m),
                                     (f"no-EKF, only KissICP {len(gt2)} poses", kiss_m)):
                    ate_rot, ate_trans = calc_ate(poses, gt2)
                    print(f"\nGround truth comparison ({label}):")
                    print(f"ATE_rot:   {ate_rot:.04f} deg")
                    print(f"ATE trans: {ate_trans:.04f} m")
        print("NOTE: the graphs themselves (matplotlib) are not part of this build")
    elif plot == "point_viz":
        print("NOTE: the point viewer (ouster-sdk PointViz) is not part of this build")
    elif plot:
        print(f"WARNING: plot param '{plot}' doesn't supported")


@click.command(name="cmp")
@click.argument("gt_file", required=True, type=click.Path(exists=True))
@click.argument("gt_file_cmp", required=False, type=click.Path(exists=True), nargs=-1)
def ptudes_ekf_cmp(gt_file: str, gt_file_cmp: List[str]) -> None:
    """Compare trajectories in Newer College Dataset Formats"""
    gts_all = read_newer_college_gt(gt_file)
    for cmp_file in gt_file_cmp:
        gts, gts_cmp = filter_nc_gt_by_cmp(gts_all, read_newer_college_gt(cmp_file))
        ate_rot, ate_trans = calc_ate([p for _, p in gts], [p for _, p in gts_cmp])
        name = os.path.splitext(os.path.basename(cmp_file))[0]
        print(f"\nTraj poses comparisons GT v. {name} ({len(gts)} poses):")
        print(f"ATE_rot:   {ate_rot:.04f} deg")
        print(f"ATE trans: {ate_trans:.04f} m")


ptudes_ekf_bench.add_command(ptudes_ekf_sim)
ptudes_ekf_bench.add_command(ptudes_ekf_nc)
ptudes_ekf_bench.add_command(ptudes_ekf_ouster)
ptudes_ekf_bench.add_command(ptudes_ekf_cmp)
