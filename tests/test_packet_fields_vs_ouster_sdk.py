"""ARMED PIN for the channel-field table: the descriptors of `ptl_pkt_field_default` (include/ptudes_mi.h) and their
restatement (tests/helpers/ouster_fields_numpy.py) say where reflectivity, signal and near-infrared sit in a pixel of each lidar profile, from
Ouster's published layouts as remembered - "unpinned" while ouster-sdk is not installed.  These tests SKIP without it (`import ouster.client`
fails) and hold the table against the real package the day it is there: encoder-made packets with a known image per field go through
ouster-sdk's ScanBatcher, and every field the profile has must come back as written.  Integer work: every comparison is equality."""
import json

import numpy as np
import pytest

try:
    import ouster.client as client
    import ouster.client._client as _client
except Exception as e:  # noqa: BLE001
    pytest.skip(f"ouster-sdk is not usable here: {e!r} - the field table stays 'unpinned' (DESIGN.md 3.27)", allow_module_level=True)

import ptudes_lab_amd  # noqa: E402,F401
from tests.helpers import ouster_fields_numpy as ofn  # noqa: E402

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
def test_every_field_of_the_table_is_where_ouster_sdk_reads_it(profile):
    info = _sdk_info(profile)
    rng = np.random.default_rng(2)
    image = ofn.random_field(rng, profile, "RANGE", (H, W))
    fields = {n: ofn.random_field(rng, profile, n, (H, W)) for n in ofn.TABLE[profile] if n != "RANGE"}
    ts = np.uint64(10**9) + np.arange(W, dtype=np.uint64) * np.uint64(195_312)
    bufs = ofn.encode_sweep(profile, image, ts, np.ones(W, np.uint16), 7, C, fields=fields)
    batcher = _client.ScanBatcher(W, _client.PacketFormat.from_info(info))
    scan = client.LidarScan(H, W, info.format.udp_profile_lidar, C)
    for buf in bufs:
        batcher(client.LidarPacket(buf, info), scan)
    assert np.array_equal(scan.field(client.ChanField.RANGE), image)
    for name, want in fields.items():
        assert np.array_equal(scan.field(getattr(client.ChanField, name)), want), (profile, name)
