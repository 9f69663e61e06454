"""ARMED PIN for the packet path: `packets.OusterPacketFormat`, the batching rule and the decode restate what
ouster-sdk's `PacketFormat`, `ScanBatcher` and `LidarScan` do for the reference's feed (data.py:31-77) from Ouster's published packet
layouts, and are "parity unpinned" while the sdk is not installed.  These tests SKIP without it (`import ouster.client` fails) and hold the restatement against the real package the day it is there: packet sizes, the decoded RANGE /
timestamp / status of encoder-made packets, and the sweep boundaries.  Integer work: every comparison is equality."""
import json

import numpy as np
import pytest

try:
    import ouster.client as client
    import ouster.client._client as _client
except Exception as e:  # noqa: BLE001
    pytest.skip(f"ouster-sdk is not usable here: {e!r} - the packet path stays 'parity unpinned' (DESIGN.md 3.16)", allow_module_level=True)

import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import packets as pk  # noqa: E402
from tests.helpers import ouster_packets_numpy as opn  # noqa: E402

PROFILES = ["LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"]
H, W, C = 16, 512, 16


def _sdk_info(profile):
    info = client.SensorInfo.from_default(client.LidarMode.MODE_512x10)
    js = json.loads(info.updated_metadata_string() if hasattr(info, "updated_metadata_string") else info.original_string())
    fmt = js.get("lidar_data_format", js.get("data_format"))
    fmt.update(pixels_per_column=H, columns_per_frame=W, columns_per_packet=C, udp_profile_lidar=profile,
               pixel_shift_by_row=[0] * H, column_window=[0, W - 1])
    beam = js.get("beam_intrinsics", js)
    beam["beam_altitude_angles"] = list(np.linspace(15, -15, H))
    beam["beam_azimuth_angles"] = [0.0] * H
    return client.SensorInfo(json.dumps(js))


@pytest.mark.parametrize("profile", PROFILES)
def test_packet_sizes(profile):
    info = _sdk_info(profile)
    assert pk.OusterPacketFormat.from_info(info).lidar_packet_size == _client.PacketFormat.from_info(info).lidar_packet_size


@pytest.mark.parametrize("profile", PROFILES)
def test_decode_and_sweep_boundaries(profile):
    info = _sdk_info(profile)
    rng = np.random.default_rng(1)
    bufs = []
    for k in range(3):
        img = (rng.integers(0, 1 << 12, (H, W), dtype=np.uint32) * 8).astype(np.uint32)
        ts = np.uint64(10**9 * (k + 1)) + np.arange(W, dtype=np.uint64) * np.uint64(195_312)
        st = np.ones(W, np.uint16)
        st[rng.integers(0, W, 5)] = 0
        bufs += opn.encode_sweep(profile, img, ts, st, 65535 + k, C)
    bufs.insert(W // C + 3, bufs[0])  # a late packet of the frame closed before
    sop, n, _ = opn.batch(profile, H, C, bufs)
    want = opn.decode(profile, H, W, C, bufs, sop, n)
    batcher = _client.ScanBatcher(W, _client.PacketFormat.from_info(info))
    scans, ls = [], None
    for buf in bufs:
        if ls is None:
            ls = client.LidarScan(H, W, info.format.udp_profile_lidar, C)
        if batcher(client.LidarPacket(buf, info), ls):
            scans.append(ls)
            ls = None
    if ls is not None:
        scans.append(ls)
    assert len(scans) == n
    for k, scan in enumerate(scans):
        assert scan.frame_id == want[3][k]["frame_id"]
        assert np.array_equal(scan.field(client.ChanField.RANGE), want[0][k])
        assert np.array_equal(scan.timestamp, want[1][k]) and np.array_equal(scan.status & 1, want[2][k] & 1)
        assert client.last_valid_column_ts(scan) == want[3][k]["last_valid_ts"]
