"""`flyby --color-by` end to end: the painted PLY of the command against the restatement (tests/helpers/map_paint_numpy.py) on
the synthetic sequence (range) and on a small raw packet bag written by the test's own encoder (reflectivity), and the frames after BUILDING
with the field's colours."""
import json
import os

import numpy as np
import pytest

from tests.helpers import map_paint_numpy as mp

pytestmark = pytest.mark.gpu

BOUNDS = 1.5


def _mean(total, count):
    out = np.full(len(count), np.nan)
    hit = count > 0
    out[hit] = total[hit].astype(np.float64) / count[hit].astype(np.float64)
    return out


def test_flyby_color_by_range_on_the_synthetic_sequence(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd import core, fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    n = 6
    seq = synth.make_sequence(seed=1000, n_scans=n)
    p, out, ply = str(tmp_path / "p.csv"), str(tmp_path / "frames"), str(tmp_path / "out.ply")
    pu.save_poses_nc_gt_format(p, t=list(seq.t_base + (np.arange(n) + 0.5) * seq.scan_dt), poses=list(seq.gt_poses()))
    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "5", "--color-by", "range",
                                          "--save-painted", ply, "--save-frames", out, "--max-frames", "4", "--frame-size", "64x48"])
    assert res.exit_code == 0, res.output
    assert len(os.listdir(out)) == 4 and "painted by range:" in res.output and f"Painted map saved to: {ply}" in res.output
    xyz, s = pu.load_map_ply(ply, scalars=True)
    assert list(s) == ["range", "range_count"] and len(xyz) > 10000 and f"map num points: {len(xyz)}" in res.output
    assert (s["range_count"] >= 1).all(), "every stored point is the end of one of the rays that built the map"
    # the restatement on the PLY's own points: the rays are the sweeps' pixels posed by the device's column poses
    rows = pu.read_newer_college_gt(p)
    pose0_inv = np.linalg.inv(rows[0][1])
    kt, kp = [t for t, _ in rows], [pose0_inv @ q for _, q in rows]
    lut, scans = fly.synthetic_range_scans(seq, 0, 5)
    sweeps = []
    for sc in scans:
        poses, n_out = core.traj_poses_at(kt, kp, np.asarray(sc.timestamp, dtype=np.float64) * 1e-9, BOUNDS, BOUNDS)
        assert n_out == 0
        sweeps.append(mp.rays_of_sweep(lut(sc.range_mm).reshape(seq.H, seq.W, 3), sc.range_mm != 0, poses, sc.range_mm))
    total, count, counts = mp.paint_arrays(xyz, sweeps, 0.5)
    assert np.array_equal(s["range_count"], count) and np.array_equal(s["range"], _mean(total, count))
    returns = sum(int((sc.range_mm != 0).sum()) for sc in scans)
    assert f"rays matched {counts['n_rays_matched']}, unmatched {returns - len(xyz)}" in res.output and counts["n_rays_unmatched"] == returns - len(xyz)
    lut.close()

    # the frames: BUILDING keeps the height palette, the colours start with the first frame after it
    lut, scans = fly.synthetic_range_scans(seq, 0, 5)
    shifted = list(zip(kt, kp))
    frames = []
    for colours in (False, True):
        acc = fly.MapAccumulator(lut, voxel_size=0.5)
        r = core.Renderer(64, 48, point_px=2)
        calls = []

        def words(acc=acc, calls=calls):
            painter = fly.MapPainter(acc)
            for sc in scans:
                painter.update(sc, traj, "range")
            v = painter.values()
            painter.close()
            calls.append(len(v.count))
            return fly.scalar_colors(v.mean())

        traj = core.Traj(kt, kp, BOUNDS, BOUNDS)
        fb = fly.FlyBy(acc, r, shifted, fps=30, rate=1.0, time_bounds=BOUNDS, max_frames=9, point_colors=words if colours else None)
        frames.append(list(fb.frames(scans, traj=traj)))
        assert calls == ([acc.map_size()[1]] if colours else []), "the colours are made once, when BUILDING has ended"
        traj.close(); r.close(); acc.close()
    plain, painted = frames
    assert [s for s, _ in painted] == [s for s, _ in plain] == ["BUILDING"] * 6 + ["TO_THE_BEGINNING"] * 3
    for i in range(6):
        assert painted[i][1].tobytes() == plain[i][1].tobytes(), f"BUILDING frame {i}"
    for i in range(6, 9):
        assert painted[i][1].tobytes() != plain[i][1].tobytes(), f"frame {i}: the field's colours, not the height palette"
    lut.close()


def test_flyby_color_by_reflectivity_on_a_packet_bag(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd import bag, core, synth
    from ptudes_lab_amd import packets as pk
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    from ptudes_lab_amd.ins.data import GRAV
    from tests import bagwriter as bw
    from tests.helpers import ouster_fields_numpy as ofn
    Hs, Ws, n = 16, 64, 4
    profile = "RNG19_RFL8_SIG16_NIR16"
    rng = np.random.default_rng(12)
    seq = synth.make_sequence(seed=1010, n_scans=n, H=Hs, W=Ws)
    meta = {"beam_altitude_angles": list(np.linspace(45.0, -45.0, Hs)), "beam_azimuth_angles": [0.0] * Hs,
            "lidar_origin_to_beam_origin_mm": 0.0, "lidar_mode": f"{Ws}x10", "prod_line": "OS-0-16",
            "lidar_to_sensor_transform": np.eye(4).reshape(-1).tolist(), "imu_to_sensor_transform": np.eye(4).reshape(-1).tolist(),
            "data_format": {"pixels_per_column": Hs, "columns_per_frame": Ws, "columns_per_packet": 16, "udp_profile_lidar": profile}}
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    conns = [("/os_node/lidar_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5),
             ("/os_node/imu_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5)]
    msgs, stream, t_bag, images = [], [], 10**9, []
    for k in range(n):
        a, e = seq.imu_range_for_scan(k)
        for i in range(a, e):
            ts_ns = int(round(seq.imu[i, 0] * 1e9))
            stream.append(("imu", bw.ouster_imu_packet(ts_ns, ts_ns, ts_ns, seq.imu[i, 1:4] / GRAV, np.degrees(seq.imu[i, 4:7]))))
        x = seq.scan(k).reshape(Hs, Ws, 3)
        img = np.round(np.linalg.norm(x[:, (Ws - np.arange(Ws)) % Ws, :], axis=2) * 1000.0).astype(np.uint32)
        img[rng.random((Hs, Ws)) < 0.1] = 0
        refl = ofn.random_field(rng, profile, "REFLECTIVITY", (Hs, Ws))
        t0 = int(round((seq.t_base + k * seq.scan_dt) * 1e9))
        ts = np.uint64(t0) + (np.arange(1, Ws + 1, dtype=np.uint64) * np.uint64(int(seq.scan_dt * 1e9) // Ws))
        images.append((img, refl, ts))
        stream += [("lidar", pkt) for pkt in ofn.encode_sweep(profile, img, ts, np.ones(Ws, np.uint16), 100 + k, 16, fields={"REFLECTIVITY": refl},
                                                              junk=rng)]
    for kind, buf in stream:
        t_bag += 1000
        msgs.append((0 if kind == "lidar" else 1, t_bag, bw.packet_msg(buf)))
    bw.write_bag(tmp_path / "x.bag", conns, msgs)
    kts = np.arange(0, n * seq.scan_dt + 0.3, 0.02)
    poses = str(tmp_path / "gt.csv")
    pu.save_poses_nc_gt_format(poses, t=[seq.t_base + float(t) for t in kts], poses=[seq.pose_at(np.array([t]))[0] for t in kts])
    ply = str(tmp_path / "painted.ply")
    base = ["flyby", str(tmp_path / "x.bag"), "-m", str(tmp_path / "meta.json"), "--nc-gt-poses", poses, "--native-packets"]
    res = CliRunner().invoke(ptudes_cli, base + ["--color-by", "reflectivity", "--save-painted", ply])
    assert res.exit_code == 0, res.output
    xyz, s = pu.load_map_ply(ply, scalars=True)
    assert list(s) == ["reflectivity", "reflectivity_count"] and len(xyz) > 500 and (s["reflectivity_count"] >= 1).all()
    info = pk.read_metadata_json(str(tmp_path / "meta.json"))
    rows = pu.read_newer_college_gt(poses)
    pose0_inv = np.linalg.inv(rows[0][1])
    kt, kp = [t for t, _ in rows], [pose0_inv @ q for _, q in rows]
    lut = core.Lut(Hs, Ws, info.beam_altitude_angles, info.beam_azimuth_angles, 0.0, np.eye(4))
    sweeps = []
    for img, refl, ts in images:
        col, n_out = core.traj_poses_at(kt, kp, ts.astype(np.float64) * 1e-9, BOUNDS, BOUNDS)
        assert n_out == 0
        sweeps.append(mp.rays_of_sweep(lut(img).reshape(Hs, Ws, 3), img != 0, col, refl))
    total, count, counts = mp.paint(xyz, sweeps, 0.5)
    assert np.array_equal(s["reflectivity_count"], count) and np.array_equal(s["reflectivity"], _mean(total, count))
    assert f"rays matched {counts['n_rays_matched']}, unmatched {counts['n_rays_unmatched']}" in res.output
    assert 0.0 <= np.nanmin(s["reflectivity"]) and np.nanmax(s["reflectivity"]) <= 255.0 and len(np.unique(s["reflectivity"])) > 50
    lut.close()
    # a profile without the field is refused naming both
    meta["data_format"]["udp_profile_lidar"] = "RNG15_RFL8_NIR8"
    (tmp_path / "meta8.json").write_text(json.dumps(meta))
    res = CliRunner().invoke(ptudes_cli, ["flyby", str(tmp_path / "x.bag"), "-m", str(tmp_path / "meta8.json"), "--nc-gt-poses", poses,
                                          "--native-packets", "--color-by", "signal"])
    assert res.exit_code != 0 and "RNG15_RFL8_NIR8" in res.output and "SIGNAL" in res.output, res.output
