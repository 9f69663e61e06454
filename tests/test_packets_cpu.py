"""Lidar packets without ouster-sdk, host side: the format table, known-answer packets written at literal offsets, the
batching rule, the feed's event order against the reference's recorded one, the metadata reader, the ABI guard of ptl_pkt_format."""
import ctypes as C
import json
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from ptudes_lab_amd import packets as pk
from tests.helpers import ouster_packets_numpy as opn

PROFILES = ["LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"]


def _info(profile, H, W, C=16):
    return SimpleNamespace(format=SimpleNamespace(pixels_per_column=H, columns_per_frame=W, columns_per_packet=C,
                                                  udp_profile_lidar=profile))


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("profile,h,size", [
    ("LEGACY", 128, 24896), ("RNG19_RFL8_SIG16_NIR16", 128, 24832), ("RNG15_RFL8_NIR8", 128, 8448),
    ("RNG19_RFL8_SIG16_NIR16_DUAL", 128, 33024), ("LEGACY", 64, 12608), ("RNG19_RFL8_SIG16_NIR16", 64, 12544)])
def test_published_packet_sizes(profile, h, size):
    fmt = pk.OusterPacketFormat.from_info(_info(profile, h, 1024))
    assert fmt.lidar_packet_size == size
    assert opn.packet_size(profile, h, 16) == size  # the restatement's table, written separately
    from ptudes_lab_amd import core
    assert core.pkt_packet_bytes(fmt) == size       # the library's


def test_profile_names_and_unknown_profile():
    assert pk.OusterPacketFormat.from_info(_info("UDPProfileLidar.PROFILE_LIDAR_RNG15_RFL8_NIR8", 16, 64)).profile == "RNG15_RFL8_NIR8"
    with pytest.raises(ValueError, match="FUSA_RNG15_RFL8_NIR8_DUAL"):
        pk.OusterPacketFormat.from_info(_info("FUSA_RNG15_RFL8_NIR8_DUAL", 16, 64))


def test_field_offsets_are_4_byte_aligned_and_timestamps_are_not_8():
    for profile in PROFILES:
        fmt = pk.OusterPacketFormat.from_info(_info(profile, 16, 64))
        assert fmt.packet_header_size % 4 == 0 and fmt.col_size % 4 == 0 and fmt.pixel_size % 4 == 0 and fmt.col_header_size % 4 == 0
    fmt = pk.OusterPacketFormat.from_info(_info("RNG19_RFL8_SIG16_NIR16", 16, 64))
    assert (fmt.packet_header_size + fmt.col_size) % 8 == 4  # column 1's u64 timestamp


# ---------------------------------------------------------------------------------------------- known-answer packets, literal offsets
H_KAT, C_KAT, W_KAT = 2, 2, 4


def _decode_one(profile, buf):
    rng, ts, st, sums = opn.decode(profile, H_KAT, W_KAT, C_KAT, [bytes(buf)], [0], 1)
    return rng[0], ts[0], st[0], sums[0]


def kat_legacy():
    # H = 2, C = 2: column = 16 + 2 * 12 + 4 = 44 bytes, packet 88
    buf = bytearray(88)
    struct.pack_into("<QHHI", buf, 0, 0x1122334455667788, 1, 7, 0)       # column 0: ts, measurement id 1, frame 7, encoder
    struct.pack_into("<I", buf, 16, 0xfff00000 | 0x12345)                 # pixel 0: bits above the 20-bit mask set
    struct.pack_into("<I", buf, 28, 0x000fffff)                           # pixel 1
    struct.pack_into("<I", buf, 40, 0xffffffff)                           # status: valid
    struct.pack_into("<QHHI", buf, 44, 99, 2, 7, 0)                       # column 1: id 2 ...
    struct.pack_into("<I", buf, 60, 0xabcde)
    struct.pack_into("<I", buf, 84, 0)                                    # ... not valid
    return ("LEGACY", buf, [[0, 0x12345, 0, 0], [0, 0xfffff, 0, 0]], [0, 0x1122334455667788, 0, 0], [0, 0xffff, 0, 0],
            dict(frame_id=7, valid_columns=1, first_valid_id=1, last_valid_id=1, last_valid_ts=0x1122334455667788, nonzero_ranges=2))


def kat_rng19():
    # 32 header + 2 * (12 + 2 * 12) + 32 footer = 136
    buf = bytearray(136)
    struct.pack_into("<HH", buf, 0, 1, 513)                               # packet type, frame id
    struct.pack_into("<QHH", buf, 32, 5_000_000_001, 0, 1)                # column 0: ts, id 0, status valid
    struct.pack_into("<I", buf, 44, 0xfff80000 | 0x7ffff)                 # bits above the 19-bit mask set
    struct.pack_into("<I", buf, 56, 1000)
    struct.pack_into("<QHH", buf, 68, 5_000_000_002, 3, 0x8001)           # column 1: id 3, status valid + a high bit
    struct.pack_into("<I", buf, 80, 0)
    struct.pack_into("<I", buf, 92, 0x00080000)                           # only a bit above the mask: no return
    return ("RNG19_RFL8_SIG16_NIR16", buf, [[0x7ffff, 0, 0, 0], [1000, 0, 0, 0]], [5_000_000_001, 0, 0, 5_000_000_002],
            [1, 0, 0, 0x8001], dict(frame_id=513, valid_columns=2, first_valid_id=0, last_valid_id=3, nonzero_ranges=2))


def kat_rng15():
    # 32 + 2 * (12 + 2 * 4) + 32 = 104
    buf = bytearray(104)
    struct.pack_into("<HH", buf, 0, 1, 65535)
    struct.pack_into("<QHH", buf, 32, 1, 2, 1)
    struct.pack_into("<HBB", buf, 44, 0x7fff, 0xaa, 0xbb)                 # range 0x7fff -> 262136 mm; reflectivity, near-ir
    struct.pack_into("<HBB", buf, 48, 0x8000 | 5, 0xcc, 0xdd)             # bit 15 is not range
    struct.pack_into("<QHH", buf, 52, 2, 0, 0)                            # column 1 invalid, over garbage
    struct.pack_into("<HH", buf, 64, 0x1234, 0x5678)
    return ("RNG15_RFL8_NIR8", buf, [[0, 0, 262136, 0], [0, 0, 40, 0]], [0, 0, 1, 0], [0, 0, 1, 0],
            dict(frame_id=65535, valid_columns=1, nonzero_ranges=2))


def kat_dual():
    # 32 + 2 * (12 + 2 * 16) + 32 = 152
    buf = bytearray(152)
    struct.pack_into("<HH", buf, 0, 1, 9)
    struct.pack_into("<QHH", buf, 32, 77, 1, 1)
    struct.pack_into("<I", buf, 44, (0xc8 << 24) | 0x00080000 | 4321)     # byte 3 = reflectivity 200, bit 19 set: neither is range
    struct.pack_into("<I", buf, 48, (0x11 << 24) | 99999)                 # the SECOND return: not decoded
    struct.pack_into("<I", buf, 60, 0x7ffff)
    struct.pack_into("<QHH", buf, 76, 78, 2, 1)
    struct.pack_into("<I", buf, 88, (0xff << 24))                         # reflectivity only: no return
    return ("RNG19_RFL8_SIG16_NIR16_DUAL", buf, [[0, 4321, 0, 0], [0, 0x7ffff, 0, 0]], [0, 77, 78, 0], [0, 1, 1, 0],
            dict(frame_id=9, valid_columns=2, nonzero_ranges=2))


KATS = [kat_legacy, kat_rng19, kat_rng15, kat_dual]  # (tests/test_gpu_packet_decode.py runs the same packets through the device)


@pytest.mark.parametrize("kat", KATS)
def test_known_answer_packets(kat):
    profile, buf, want_rng, want_ts, want_st, want_sum = kat()
    assert len(buf) == opn.packet_size(profile, H_KAT, C_KAT)
    rng, ts, st, s = _decode_one(profile, buf)
    assert rng.tolist() == want_rng and ts.tolist() == want_ts and st.tolist() == want_st
    assert {k: s[k] for k in want_sum} == want_sum


@pytest.mark.parametrize("profile", PROFILES)
def test_encoder_round_trip_with_junk(profile):
    rng = np.random.default_rng(5)
    H, W, Cc = 4, 8, 4
    img = (rng.integers(0, 1 << 15, (H, W), dtype=np.uint32) << 3).astype(np.uint32)
    ts = rng.integers(1, 1 << 62, W, dtype=np.uint64)
    st = np.ones(W, np.uint16)
    st[5] = 0
    pkts = opn.encode_sweep(profile, img, ts, st, 1234, Cc, junk=rng)
    sop, n, bad = opn.batch(profile, H, Cc, pkts)
    assert sop.tolist() == [0, 0] and n == 1 and bad == 0
    r, t, s, sums = opn.decode(profile, H, W, Cc, pkts, sop, 1)
    want = img.copy()
    want[:, 5] = 0
    assert np.array_equal(r[0], want) and sums[0]["frame_id"] == 1234
    assert t[0].tolist() == [0 if j == 5 else int(ts[j]) for j in range(W)]
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, Cc))
    assert [fmt.frame_id(p) for p in pkts] == [1234, 1234] and fmt.lidar_packet_size == len(pkts[0])


# ---------------------------------------------------------------------------------------------- batching rule
def test_batching_rule_late_wrap_and_wrong_length():
    f = [65534, 65534, 65535, 65534, 65535, 0, 65535, 0, 5, 5]
    ln = [10, 10, 10, 10, 10, 10, 10, 9, 10, 10]
    sop, n, bad = pk.batch_packets(f, ln, 10)
    #       open 0      next  late  same  wrap  late  bad  jump
    assert sop.tolist() == [0, 0, 1, -1, 1, 2, -1, -1, 3, 3] and n == 4 and bad == 1
    # the restatement agrees on encoded packets
    img, ts, st = np.ones((2, 2), np.uint32), np.ones(2, np.uint64), np.ones(2, np.uint16)
    pkts = [opn.encode_sweep("LEGACY", img, ts, st, fid, 2)[0] for fid in f]
    pkts[7] = pkts[7][:-4]
    sop2, n2, bad2 = opn.batch("LEGACY", 2, 2, pkts)
    assert sop2.tolist() == sop.tolist() and (n2, bad2) == (n, bad)


def _golden_source(g, profile, H, W, Cc):
    img = np.full((H, Cc), 1000, np.uint32)
    out = []
    for kind, a, b in g["packets"]:
        if kind == "L":
            ids = np.arange(b, b + Cc)
            buf = opn.encode_packet(profile, H, a, ids, 1000 + ids.astype(np.uint64), np.ones(Cc, np.uint16), img.T)
            out.append(("lidar", buf, 0.0))
        else:
            out.append(("imu", struct.pack("<QQQ", a, a, a) + struct.pack("<6f", 0, 0, 1, 1, 2, 3), 0.0))
    return out


@pytest.mark.parametrize("profile", ["LEGACY", "RNG19_RFL8_SIG16_NIR16"])
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_feed_event_order_is_the_references(golden_dir, profile, chunk):
    g = json.load(open(os.path.join(golden_dir, "packet_feed.json")))
    H, W, Cc = 8, 64, 16
    src = _golden_source(g, profile, H, W, Cc)
    info = _info(profile, H, W, Cc)
    for name, kw in (("all", {}), ("from2", dict(start_scan=2)), ("from1to3", dict(start_scan=1, end_scan=3))):
        feed = pk.PacketFeed(src, info, decoder=opn.NumpyDecoder(profile, H, W, Cc), chunk_sweeps=chunk)
        ev = []
        for idx, d in feed.withScanIdx(**kw):
            ev.append([idx, 0, d.frame_id] if isinstance(d, pk.PacketScan) else [idx, 1, int(round(d.ts * 1e9))])
        assert ev == g["events"][name], (name, chunk)


def test_feed_drops_and_counts(golden_dir):
    H, W, Cc = 2, 4, 2
    img, ts, st = np.full((H, W), 8, np.uint32), np.arange(1, W + 1, dtype=np.uint64), np.ones(W, np.uint16)
    a, b = opn.encode_sweep("LEGACY", img, ts, st, 65535, Cc), opn.encode_sweep("LEGACY", 2 * img, ts + 10, st, 0, Cc)
    src = [("lidar", a[0], 0), ("lidar", b[0], 0), ("lidar", a[1], 0), ("lidar", b[1][:-4], 0), ("lidar", b[1], 0)]
    feed = pk.PacketFeed(src, _info("LEGACY", H, W, Cc), decoder=opn.NumpyDecoder("LEGACY", H, W, Cc))
    scans = [d for _, d in feed.withScanIdx()]
    assert [s.frame_id for s in scans] == [65535, 0] and (feed.dropped_late, feed.dropped_wrong_length) == (1, 1)
    assert scans[0].range.tolist() == [[8, 8, 0, 0]] * 2 and scans[1].range.tolist() == [[16] * 4] * 2
    assert scans[0].ts == 2e-9 and scans[1].last_valid_column_ts_ns == 14 and scans[1].timestamp.tolist() == [11, 12, 13, 14]


# ---------------------------------------------------------------------------------------------- metadata
def _flat_meta(h=16):
    return {"beam_altitude_angles": list(np.linspace(15, -15, h)), "beam_azimuth_angles": [1.5] * h,
            "lidar_origin_to_beam_origin_mm": 15.806, "lidar_mode": "512x10", "prod_line": "OS-1-16",
            "lidar_to_sensor_transform": [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 36.18, 0, 0, 0, 1],
            "imu_to_sensor_transform": [1, 0, 0, 6.253, 0, 1, 0, -11.775, 0, 0, 1, 7.645, 0, 0, 0, 1],
            "data_format": {"pixels_per_column": h, "columns_per_frame": 512, "columns_per_packet": 16,
                            "udp_profile_lidar": "RNG15_RFL8_NIR8", "pixel_shift_by_row": [0] * h}}


def _write(tmp_path, js, name="m.json"):
    p = tmp_path / name
    p.write_text(json.dumps(js))
    return str(p)


def test_metadata_flat(tmp_path):
    m = pk.read_metadata_json(_write(tmp_path, _flat_meta()))
    f = m.format
    assert (f.pixels_per_column, f.columns_per_frame, f.columns_per_packet, f.udp_profile_lidar) == (16, 512, 16, "RNG15_RFL8_NIR8")
    assert m.prod_line == "OS-1-16" and m.mode == "512x10" and m.lidar_origin_to_beam_origin_mm == 15.806
    assert m.lidar_to_sensor_transform[2, 3] == 36.18 and m.imu_to_sensor_transform[1, 3] == -11.775
    assert np.array_equal(m.extrinsic, np.eye(4)) and len(m.beam_altitude_angles) == 16 and m.beam_azimuth_angles[3] == 1.5
    assert pk.OusterPacketFormat.from_info(m).lidar_packet_size == 64 + 16 * (12 + 16 * 4)


def test_metadata_nested(tmp_path):
    fl = _flat_meta(32)
    js = {"beam_intrinsics": {k: fl[k] for k in ("beam_altitude_angles", "beam_azimuth_angles", "lidar_origin_to_beam_origin_mm")},
          "lidar_data_format": dict(fl["data_format"], udp_profile_lidar="RNG19_RFL8_SIG16_NIR16_DUAL"),
          "lidar_intrinsics": {"lidar_to_sensor_transform": fl["lidar_to_sensor_transform"]},
          "imu_intrinsics": {"imu_to_sensor_transform": fl["imu_to_sensor_transform"]},
          "sensor_info": {"prod_line": "OS-0-32"}, "config_params": {"lidar_mode": "512x20"},
          "extrinsic": [1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3, 0, 0, 0, 1]}
    m = pk.read_metadata_json(_write(tmp_path, js))
    assert m.format.udp_profile_lidar == "RNG19_RFL8_SIG16_NIR16_DUAL" and m.format.pixels_per_column == 32
    assert m.prod_line == "OS-0-32" and m.mode == "512x20" and m.extrinsic[:3, 3].tolist() == [1, 2, 3]
    del js["imu_intrinsics"]["imu_to_sensor_transform"]
    with pytest.raises(ValueError, match="'imu_to_sensor_transform' is missing in imu_intrinsics"):
        pk.read_metadata_json(_write(tmp_path, js))


def test_metadata_nc2020_backfill_and_missing_field(tmp_path, capsys):
    js = _flat_meta(64)
    del js["lidar_mode"], js["data_format"]
    path = _write(tmp_path, js)
    m = pk.read_metadata_json(path)
    assert capsys.readouterr().out == f"WARNING: lidar_mode is not present in legacy metadata '{path}' so using lidar_mode: 1024x10\n"
    f = m.format
    assert (m.mode, f.udp_profile_lidar, f.columns_per_packet, f.columns_per_frame, f.pixels_per_column) == ("1024x10", "LEGACY", 16, 1024, 64)
    assert pk.OusterPacketFormat.from_info(m).lidar_packet_size == 12608
    del js["prod_line"]
    with pytest.raises(ValueError, match="'prod_line' is missing"):
        pk.read_metadata_json(_write(tmp_path, js))
    del js["beam_azimuth_angles"]
    with pytest.raises(ValueError, match="'beam_azimuth_angles' is missing"):
        pk.read_metadata_json(_write(tmp_path, js))


# ---------------------------------------------------------------------------------------------- ABI guard
def test_pkt_format_abi_guard():
    from ptudes_lab_amd import _lib as L
    from ptudes_lab_amd import core
    fmt = core.pkt_format(pk.OusterPacketFormat.from_info(_info("LEGACY", 128, 1024)))
    assert L.lib().ptl_sizeof_cfg(4) == C.sizeof(L.PktFormat) and L.lib().ptl_pkt_packet_bytes(C.byref(fmt)) == 24896
    before = bytes(fmt)
    fmt.struct_size -= 4
    assert L.lib().ptl_pkt_packet_bytes(C.byref(fmt)) == -1 and b"struct_size" in L.lib().ptl_last_error()
    h = C.c_void_p()
    assert L.lib().ptl_pktdec_create(C.byref(fmt), 0, 64, 1, C.byref(h)) == -1 and not h.value
    fmt.struct_size += 4
    fmt.abi_version += 1
    assert L.lib().ptl_pktdec_create(C.byref(fmt), 0, 64, 1, C.byref(h)) == -1 and not h.value
    fmt.abi_version -= 1
    assert bytes(fmt) == before
    fmt.profile = 9
    assert L.lib().ptl_pkt_packet_bytes(C.byref(fmt)) == -1 and b"profile 9" in L.lib().ptl_last_error()


def test_track_scan_takes_a_packet_scan_signature():
    # (the reduction itself runs on the device: tests/test_gpu_packet_decode.py) - the scan carries what trackScan asks for
    s = pk.PacketScan(np.ones((2, 3), np.uint32), np.array([5, 6, 7], np.uint64), np.array([1, 1, 0], np.uint16), 3)
    assert (s.h, s.w, s.frame_id, s.last_valid_column_ts_ns, s.ts) == (2, 3, 3, 6, 6 * 1e-9) and not hasattr(s, "xyz")
