"""Lidar packets decoded on the device (csrc/packet_kernels.h) against the plain-loop restatement
(tests/helpers/ouster_packets_numpy.py): integer work, so every comparison is bit-equality."""
import os

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import core, synth
from ptudes_lab_amd import packets as pk
from tests.helpers import ouster_packets_numpy as opn
from tests.test_packets_cpu import C_KAT, H_KAT, KATS, W_KAT, _info

pytestmark = pytest.mark.gpu

PROFILES = ["LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"]


def _sweep(rng, profile, H, W, max_mm=1 << 19):
    """a random sweep: image (multiples of 8 so that RNG15 holds it, ~10 % no return), column times, all columns valid"""
    top = min(max_mm, (1 << 15) * 8 if profile == "RNG15_RFL8_NIR8" else max_mm)
    img = (rng.integers(0, top // 8, (H, W), dtype=np.uint32) * 8).astype(np.uint32)
    img[rng.random((H, W)) < 0.1] = 0
    ts = (rng.integers(1, 1 << 40, dtype=np.uint64) + np.arange(W, dtype=np.uint64) * np.uint64(97_657))
    return img, ts, np.ones(W, np.uint16)


def _both(profile, H, W, C, bufs, sop, n_sweeps, dec=None, pinned=False):
    """device and restatement on the same packets; asserts equality and returns the device's arrays"""
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, C))
    own = dec is None
    dec = dec or core.PacketDecoder(fmt, max_sweeps=max(n_sweeps, 1), max_packets=max(len(bufs), 1))
    a = np.frombuffer(b"".join(bufs), dtype=np.uint8).reshape(len(bufs), fmt.lidar_packet_size).copy()
    if pinned:
        core.host_pin(a)
    try:
        got = dec.decode_arrays(a, sop, n_sweeps)
    finally:
        if pinned:
            core.host_unpin(a)
        if own:
            dec.close()
    want = opn.decode(profile, H, W, C, bufs, list(sop), n_sweeps)
    for g, w, name in zip(got[:3], want[:3], ("range", "timestamp", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (profile, H, W, name)
    assert got[3] == want[3], (profile, H, W)
    return got


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("H,W", [(16, 64), (32, 64), (128, 64)])
def test_small_sweeps_every_profile(profile, H, W):
    rng = np.random.default_rng(H)
    img, ts, st = _sweep(rng, profile, H, W)
    bufs = opn.encode_sweep(profile, img, ts, st, 41, 16, junk=rng)
    assert len(bufs) == 4
    r, t, s, sums = _both(profile, H, W, 16, bufs, np.zeros(4, np.int32), 1)
    assert np.array_equal(r[0], img) and np.array_equal(t[0], ts) and sums[0]["valid_columns"] == W


@pytest.mark.parametrize("profile", ["LEGACY", "RNG19_RFL8_SIG16_NIR16"])
def test_full_sweep_128x1024(profile):
    rng = np.random.default_rng(7)
    img, ts, st = _sweep(rng, profile, 128, 1024)
    bufs = opn.encode_sweep(profile, img, ts, st, 65535, 16)
    assert len(bufs) == 64
    r, t, s, sums = _both(profile, 128, 1024, 16, bufs, np.zeros(64, np.int32), 1)
    assert np.array_equal(r[0], img) and sums[0]["nonzero_ranges"] == np.count_nonzero(img) and sums[0]["frame_id"] == 65535


@pytest.mark.parametrize("kat", KATS)
def test_known_answer_packets_on_the_device(kat):
    profile, buf, want_rng, want_ts, want_st, want_sum = kat()
    r, t, s, sums = _both(profile, H_KAT, W_KAT, C_KAT, [bytes(buf)], np.zeros(1, np.int32), 1)
    assert r[0].tolist() == want_rng and t[0].tolist() == want_ts and s[0].tolist() == want_st
    assert {k: sums[0][k] for k in want_sum} == want_sum


H, W, C = 16, 64, 16


@pytest.mark.parametrize("profile", PROFILES)
def test_hard_cases(profile):
    rng = np.random.default_rng(11)
    img, ts, st = _sweep(rng, profile, H, W)
    # timestamps >= 2^60 with distinct high and low dwords, in odd columns (4-byte aligned only: the column stride is 12 or 20 mod 24)
    ts[1::2] = (np.uint64(1) << np.uint64(60)) + np.arange(W // 2, dtype=np.uint64) * np.uint64(0x1_0000_0003) + np.uint64(0xabcdef)
    assert all((int(v) >> 32) != (int(v) & 0xffffffff) for v in ts[1::2])
    # status bit 0 clear over garbage pixels
    st[[3, 17, 63]] = 0
    bufs = opn.encode_sweep(profile, img, ts, st, 500, C, junk=rng)
    want = img.copy()
    want[:, [3, 17, 63]] = 0
    r, t, s, sums = _both(profile, H, W, C, bufs, np.zeros(4, np.int32), 1)
    assert np.array_equal(r[0], want) and t[0][3] == 0 and t[0][1] == ts[1] and sums[0]["last_valid_id"] == 62
    assert sums[0]["last_valid_ts"] == int(ts[62]) and sums[0]["first_valid_ts"] == int(ts[0]) and sums[0]["valid_columns"] == W - 3
    # a missing packet: its 16 columns are zero
    r, t, s, sums = _both(profile, H, W, C, [bufs[0], bufs[1], bufs[3]], np.zeros(3, np.int32), 1)
    assert not r[0][:, 32:48].any() and not t[0][32:48].any() and sums[0]["valid_columns"] == W - 16 - 3
    # packets shuffled within the sweep: the same result
    order = [2, 0, 3, 1]
    r2 = _both(profile, H, W, C, [bufs[i] for i in order], np.zeros(4, np.int32), 1)
    assert np.array_equal(r2[0][0], want) and r2[3][0]["frame_id"] == 500
    # measurement_id >= W: ignored and counted
    ids = np.arange(W)
    ids[[5, 40]] = [W, 65535]
    odd = opn.encode_sweep(profile, img, ts, np.ones(W, np.uint16), 9, C, junk=rng, ids=ids)
    r, t, s, sums = _both(profile, H, W, C, odd, np.zeros(4, np.int32), 1)
    assert sums[0]["ignored_columns"] == 2 and not r[0][:, [5, 40]].any() and sums[0]["valid_columns"] == W - 2


@pytest.mark.parametrize("profile", ["LEGACY", "RNG15_RFL8_NIR8"])
def test_same_measurement_id_twice_the_later_wins(profile):
    rng = np.random.default_rng(13)
    img, ts, st = _sweep(rng, profile, H, W)
    other, ts2, _ = _sweep(rng, profile, H, W)
    bufs = opn.encode_sweep(profile, img, ts, st, 3, C)
    dup = opn.encode_sweep(profile, other, ts2, st, 3, C)[1]  # columns 16 .. 31 again, other pixels and times
    for pkts, winner, wts in (([bufs[0], bufs[1], dup, bufs[2], bufs[3]], other, ts2), ([bufs[0], dup, bufs[1], bufs[2], bufs[3]], img, ts)):
        r, t, s, sums = _both(profile, H, W, C, pkts, np.zeros(5, np.int32), 1)
        assert np.array_equal(r[0][:, 16:32], winner[:, 16:32]) and np.array_equal(t[0][16:32], wts[16:32])
        assert np.array_equal(r[0][:, :16], img[:, :16]) and sums[0]["valid_columns"] == W
    # ... also inside ONE packet: two columns of it name the same id
    ids = np.arange(W)
    ids[7] = 6
    one = opn.encode_sweep(profile, img, ts, st, 3, C, ids=ids)
    r, t, s, sums = _both(profile, H, W, C, one, np.zeros(4, np.int32), 1)
    assert np.array_equal(r[0][:, 6], img[:, 7]) and not r[0][:, 7].any() and sums[0]["valid_columns"] == W - 1


def test_three_sweeps_and_dropped_packets_in_one_launch_pinned_and_pageable():
    profile = "RNG19_RFL8_SIG16_NIR16"
    rng = np.random.default_rng(17)
    sweeps = [_sweep(rng, profile, H, W) for _ in range(3)]
    bufs, sop = [], []
    for k, (img, ts, st) in enumerate(sweeps):
        p = opn.encode_sweep(profile, img, ts, st, 65534 + k, C, junk=rng)
        bufs += p
        sop += [k] * len(p)
    # a late packet and junk, tagged -1, among them; sweep 1 arrives interleaved with sweep 2's first packet
    bufs.insert(6, bufs[0]); sop.insert(6, -1)
    bufs.insert(2, bytes(rng.integers(0, 256, len(bufs[0]), dtype=np.uint8))); sop.insert(2, -1)
    bufs[9], bufs[10] = bufs[10], bufs[9]; sop[9], sop[10] = sop[10], sop[9]
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, C))
    dec = core.PacketDecoder(fmt, max_sweeps=4, max_packets=16)
    outs = [_both(profile, H, W, C, bufs, np.array(sop, np.int32), 4, dec=dec, pinned=pinned) for pinned in (False, True)]
    for r, t, s, sums in outs:
        for k, (img, ts, st) in enumerate(sweeps):
            assert np.array_equal(r[k], img) and np.array_equal(t[k], ts) and sums[k]["frame_id"] == (65534 + k) & 0xffff
        assert not r[3].any() and sums[3] == dict.fromkeys(sums[3], 0)  # a sweep nobody names: zeros
    # the PacketScan view of the same call
    scans = dec.decode(np.frombuffer(b"".join(bufs), np.uint8).reshape(len(bufs), -1), sop, 4)
    assert scans[1].ts == int(sweeps[1][1][-1]) * 1e-9 and scans[1].frame_id == 65535 and scans[2].frame_id == 0
    # a strided buffer (rows padded to a multiple of 64 bytes) gives the same
    size = fmt.lidar_packet_size
    wide = np.zeros((len(bufs), (size + 63) // 64 * 64 + 64), np.uint8)
    wide[:, :size] = np.frombuffer(b"".join(bufs), np.uint8).reshape(len(bufs), size)
    got = dec.decode_arrays(wide, sop, 4)
    assert np.array_equal(got[0], outs[0][0]) and got[3] == outs[0][3]
    # arguments are refused on the host, before any launch
    a = wide[:, :size].copy()
    with pytest.raises(ValueError, match="names sweep 4"):
        dec.decode_arrays(a, [4] * len(a), 4)
    with pytest.raises(ValueError, match="created for 16"):
        dec.decode_arrays(np.zeros((17, size), np.uint8), [0] * 17, 1)
    with pytest.raises(ValueError, match="created for 4"):
        dec.decode_arrays(a, sop, 5)
    with pytest.raises(ValueError, match="4-byte aligned"):
        dec.decode_arrays(np.zeros((2, size + 2), np.uint8), [0, 0], 1)
    dec.close()


def test_track_scan_takes_a_decoded_scan():
    from ptudes_lab_amd.ins.data import StreamStatsTracker
    profile = "LEGACY"
    rng = np.random.default_rng(19)
    img, ts, st = _sweep(rng, profile, H, W)
    st[-1] = 0
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, C))
    dec = core.PacketDecoder(fmt, max_sweeps=1)
    scan = dec.decode(np.frombuffer(b"".join(opn.encode_sweep(profile, img, ts, st, 1, C)), np.uint8), [0] * 4, 1)[0]
    a, b = StreamStatsTracker(use_beams_num=8), StreamStatsTracker(use_beams_num=8)
    a.trackScan(scan)
    b.trackScan(scan.range, last_valid_column_ts_ns=int(ts[-2]))
    assert (a.range_mean, a.range_std, a._min_range, a._max_range, a._points_num) == (b.range_mean, b.range_std, b._min_range, b._max_range, b._points_num)
    assert a._points_num > 0 and a._t_span == b._t_span == [int(ts[-2]) * 1e-9] * 2


# ---------------------------------------------------------------------------------------------- into a runner's sweep slot
N_SCANS = 5


@pytest.fixture(scope="module")
def scene():
    """the smallest scene of tests/test_gpu_range_image.py: 5 sweeps of 128 x 1024, no filter - as range images and as RNG19 packets"""
    seq = synth.make_sequence(seed=1004, n_scans=N_SCANS)
    Hs, Ws = seq.H, seq.W
    fmt = pk.OusterPacketFormat.from_info(_info("RNG19_RFL8_SIG16_NIR16", Hs, Ws))
    imgs, pkts = [], []
    for k in range(N_SCANS):
        x = seq.scan(k).reshape(Hs, Ws, 3)
        img = np.round(np.linalg.norm(x[:, (Ws - np.arange(Ws)) % Ws, :], axis=2) * 1000.0).astype(np.uint32)
        ts = np.uint64(10**9 * (k + 1)) + np.arange(Ws, dtype=np.uint64) * np.uint64(97_656)
        imgs.append(img)
        pkts.append(np.frombuffer(b"".join(opn.encode_sweep(fmt.profile, img, ts, np.ones(Ws, np.uint16), k, 16)), np.uint8).copy())
    return seq, fmt, imgs, pkts


def test_seq_runner_upload_packets_equals_upload_range(scene):
    seq, fmt, imgs, pkts = scene
    lut = core.Lut(seq.H, seq.W, np.linspace(45.0, -45.0, seq.H), np.zeros(seq.H))
    dec = core.PacketDecoder(fmt, max_sweeps=1)
    outs = []
    for packets in (False, True):
        r = core.SeqRunner(N_SCANS, seq.H * seq.W, 0, max_range=70.0, min_range=1.0, with_ekf=False)
        r.set_lut(lut)
        for k in range(N_SCANS):
            if packets:
                summ, ts = r.upload_packets(dec, k, pkts[k], col_ts=True)
                assert summ["frame_id"] == k and summ["valid_columns"] == seq.W and summ["nonzero_ranges"] == np.count_nonzero(imgs[k])
                assert int(ts[-1]) == summ["last_valid_ts"] == 10**9 * (k + 1) + 1023 * 97_656
            else:
                r.upload_range(k, imgs[k])
        r.upload_imu(np.zeros((0, 7)), [0] * N_SCANS)
        r.run()
        outs.append(r.results())
        if packets:  # refused on the host
            small = core.PacketDecoder(pk.OusterPacketFormat.from_info(_info("LEGACY", 16, 64)), max_sweeps=1)
            with pytest.raises(ValueError, match="does not match the runner"):
                r.upload_packets(small, 0, np.zeros(small.packet_bytes, np.uint8))
            with pytest.raises(ValueError, match="bad argument"):
                r.upload_packets(dec, N_SCANS, pkts[0])
            small.close()
        r.close()
    assert np.array_equal(outs[0]["kiss_poses"], outs[1]["kiss_poses"]) and outs[0]["stats"] == outs[1]["stats"]
    dec.close()


@pytest.mark.parametrize("ring", [0, 2])
def test_batch_runner_upload_packets_equals_upload_range(scene, ring):
    seq, fmt, imgs, pkts = scene
    lut = core.Lut(seq.H, seq.W, np.linspace(45.0, -45.0, seq.H), np.zeros(seq.H))
    dec = core.PacketDecoder(fmt, max_sweeps=1)
    outs = []
    for packets in (False, True):
        b = core.BatchRunner(2, N_SCANS, seq.H * seq.W, 0, with_ekf=False, range_input=True, resident_scans=ring, scans_per_launch=1)
        b.set_lut(lut, active_beams=64)

        def up(s, k):
            if packets:
                assert b.upload_packets(s, dec, k, pkts[k])["frame_id"] == k
            else:
                b.upload_range(s, k, imgs[k])

        for s in range(2):
            b.upload_imu(s, np.zeros((0, 7)), [0] * N_SCANS)
        if not ring:
            for s in range(2):
                for k in range(N_SCANS):
                    up(s, k)
            b.run()
        else:
            if packets:  # the ring's own errors
                with pytest.raises(RuntimeError, match="in order"):
                    b.upload_packets(0, dec, 1, pkts[1])
            for s in range(2):
                for k in range(ring):
                    up(s, k)
            if packets:
                with pytest.raises(RuntimeError, match="still holds"):
                    b.upload_packets(0, dec, ring, pkts[ring])
            b.run(1)
            for k in range(1, N_SCANS):
                for s in range(2):
                    if k + ring - 1 < N_SCANS:
                        up(s, k + ring - 1)  # the slot of scan k - 1, known to be done
                b.enqueue(1)
                b.wait()
        outs.append([b.results(s) for s in range(2)])
        b.close()
    for s in range(2):
        assert np.array_equal(outs[0][s]["kiss_poses"], outs[1][s]["kiss_poses"]) and outs[0][s]["stats"] == outs[1][s]["stats"]
        assert len(outs[1][s]["kiss_poses"]) == N_SCANS
    dec.close()


# ---------------------------------------------------------------------------------------------- end to end: a bag through the command
def test_ekf_bench_ouster_on_a_raw_packet_bag(tmp_path):
    import json
    from click.testing import CliRunner
    from ptudes_lab_amd import bag
    from ptudes_lab_amd.cli.run import ptudes_cli
    from ptudes_lab_amd.ins.data import GRAV
    from ptudes_lab_amd.sequence import run_events
    from tests import bagwriter as bw
    Hs, Ws, n = 16, 64, 4
    profile = "RNG19_RFL8_SIG16_NIR16"
    seq = synth.make_sequence(seed=1010, n_scans=n, H=Hs, W=Ws)
    meta = {"beam_altitude_angles": list(np.linspace(45.0, -45.0, Hs)), "beam_azimuth_angles": [0.0] * Hs,
            "lidar_origin_to_beam_origin_mm": 0.0, "lidar_mode": f"{Ws}x10", "prod_line": "OS-0-16",
            "lidar_to_sensor_transform": np.eye(4).reshape(-1).tolist(), "imu_to_sensor_transform": np.eye(4).reshape(-1).tolist(),
            "data_format": {"pixels_per_column": Hs, "columns_per_frame": Ws, "columns_per_packet": 16, "udp_profile_lidar": profile}}
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    conns = [("/os_node/lidar_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5),
             ("/os_node/imu_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5)]
    msgs, stream, t_bag = [], [], 10**9
    for k in range(n):
        a, e = seq.imu_range_for_scan(k)
        for i in range(a, e):  # 48-byte IMU packets: g and deg/s as f32, the sensor's units
            ts_ns = int(round(seq.imu[i, 0] * 1e9))
            buf = bw.ouster_imu_packet(ts_ns, ts_ns, ts_ns, seq.imu[i, 1:4] / GRAV, np.degrees(seq.imu[i, 4:7]))
            assert len(buf) == 48
            stream.append(("imu", buf))
        x = seq.scan(k).reshape(Hs, Ws, 3)
        img = np.round(np.linalg.norm(x[:, (Ws - np.arange(Ws)) % Ws, :], axis=2) * 1000.0).astype(np.uint32)
        t0 = int(round((seq.t_base + k * seq.scan_dt) * 1e9))
        ts = np.uint64(t0) + (np.arange(1, Ws + 1, dtype=np.uint64) * np.uint64(int(seq.scan_dt * 1e9) // Ws))
        stream += [("lidar", p) for p in opn.encode_sweep(profile, img, ts, np.ones(Ws, np.uint16), 100 + k, 16)]
    for kind, buf in stream:
        t_bag += 1000
        msgs.append((0 if kind == "lidar" else 1, t_bag, bw.packet_msg(buf)))
    bw.write_bag(tmp_path / "x.bag", conns, msgs)

    out_csv = tmp_path / "out.csv"
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", str(tmp_path / "x.bag"), "-m", str(tmp_path / "meta.json"),
                                         "--save-nc-gt-poses", str(out_csv)])
    assert res.exit_code == 0, res.output
    assert "sensor: OS-0-16, 64x10" in res.output and f"data path: {tmp_path / 'x.bag'}" in res.output

    # the same events through the numpy restatement, into the same loop
    info = pk.read_metadata_json(str(tmp_path / "meta.json"))
    feed = pk.PacketFeed([(kind, buf, 0.0) for kind, buf in stream], info, decoder=opn.NumpyDecoder(profile, Hs, Ws, 16))
    events = [("imu", d) if hasattr(d, "lacc") else ("lidar_scan", d) for _, d in feed.withScanIdx()]
    assert sum(1 for ev in events if ev[0] == "lidar_scan") == n
    ref = run_events(iter(events), info, kiss_min_range=1.0, kiss_max_range=70.0)
    from ptudes_lab_amd.utils import save_poses_nc_gt_format
    want_csv = tmp_path / "want.csv"
    save_poses_nc_gt_format(str(want_csv), t=ref["res_t"], poses=ref["res_poses"], header="x")

    def rows(p):
        return [ln for ln in open(p).read().splitlines() if not ln.startswith("#")]

    assert len(rows(out_csv)) == len(ref["res_poses"]) >= n - 1 and rows(out_csv) == rows(want_csv)
    # the metadata beside FILE is found without -m; a .pcap stays with ouster-sdk
    os.rename(tmp_path / "meta.json", tmp_path / "x.json")
    res2 = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", str(tmp_path / "x.bag"), "--end-scan", "1"])
    assert res2.exit_code == 0 and "scans range: 0 - 1" in res2.output, res2.output
    (tmp_path / "y.pcap").write_bytes(b"")
    res3 = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", str(tmp_path / "y.pcap"), "-m", str(tmp_path / "x.json")])
    assert res3.exit_code != 0 and "reading .pcap needs ouster-sdk" in res3.output
