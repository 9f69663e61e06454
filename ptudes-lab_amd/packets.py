"""Ouster lidar packets without ouster-sdk: packet format, sensor metadata, frame batching and the feed.

The reference's feed (data.py:31-77) leans on three ouster-sdk types - `PacketFormat` (where the fields of a UDP payload are),
`ScanBatcher` (which packets form a sweep) and `LidarScan` (the staggered image).  This module restates what the pose path needs of
them from Ouster's published packet layouts:

  OusterPacketFormat   sizes and offsets of the four lidar profiles (host side: packet length, frame id)
  read_metadata_json   the sensor metadata .json as the attribute tree the package consumes (flat legacy and nested layouts)
  FrameBatcher,        the frame batching rule -> sweep_of_packet (2 bytes read per packet)
  batch_packets
  PacketScan           a decoded sweep: the duck type KissICPWrapper.register_frame and StreamStatsTracker.trackScan take
  PacketFeed           withScanIdx(start_scan=, end_scan=) -> (idx, PacketScan | IMU) in the reference's event order, the sweeps
                       decoded in chunks on the device (core.PacketDecoder, csrc/packet_kernels.h)

Everything is little-endian.  Unpinned against ouster-sdk while it is absent: tests/test_packets_vs_ouster_sdk.py is armed for the
day it is importable."""
import json
import struct
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Iterator, List, Optional, Tuple

import numpy as np

from .ins.data import IMU

PROFILES = ("LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL")
IMU_PACKET_BYTES = 48


def profile_name(profile) -> str:
    """`UDPProfileLidar.PROFILE_LIDAR_LEGACY`, `PROFILE_LIDAR_RNG19_...` or the bare name -> the bare name"""
    name = str(getattr(profile, "name", profile)).split(".")[-1]
    return name[len("PROFILE_LIDAR_"):] if name.startswith("PROFILE_LIDAR_") else name


@dataclass(frozen=True)
class OusterPacketFormat:
    """Byte layout of a lidar packet: [packet header | C columns of (column header, H pixels, column trailer) | packet footer].
    The range is the first field of a pixel: `range_bytes` wide, `range_mask` bits, value << `range_shift` = mm."""
    profile: str
    pixels_per_column: int
    columns_per_frame: int
    columns_per_packet: int
    packet_header_size: int
    col_header_size: int
    pixel_size: int
    col_trailer_size: int
    packet_footer_size: int
    range_bytes: int
    range_mask: int
    range_shift: int
    status_offset: int    # in the column; valid = bit 0
    status_bytes: int
    frame_id_offset: int  # in the packet (LEGACY: the first column's)

    @staticmethod
    def from_info(info) -> "OusterPacketFormat":
        f = info.format
        name = profile_name(f.udp_profile_lidar)
        H, W, C = int(f.pixels_per_column), int(f.columns_per_frame), int(f.columns_per_packet)
        modern = dict(packet_header_size=32, col_header_size=12, col_trailer_size=0, packet_footer_size=32, status_offset=10,
                      status_bytes=2, frame_id_offset=2, range_bytes=4, range_mask=0x0007ffff, range_shift=0)
        if name == "LEGACY":
            kw = dict(packet_header_size=0, col_header_size=16, pixel_size=12, col_trailer_size=4, packet_footer_size=0,
                      range_bytes=4, range_mask=0x000fffff, range_shift=0, status_offset=16 + 12 * H, status_bytes=4, frame_id_offset=10)
        elif name == "RNG19_RFL8_SIG16_NIR16":
            kw = dict(modern, pixel_size=12)
        elif name == "RNG15_RFL8_NIR8":
            kw = dict(modern, pixel_size=4, range_bytes=2, range_mask=0x7fff, range_shift=3)
        elif name == "RNG19_RFL8_SIG16_NIR16_DUAL":
            kw = dict(modern, pixel_size=16)
        else:
            raise ValueError(f"lidar profile '{name}' is not decoded here (known: {', '.join(PROFILES)})")
        return OusterPacketFormat(profile=name, pixels_per_column=H, columns_per_frame=W, columns_per_packet=C, **kw)

    @property
    def col_size(self) -> int:
        return self.col_header_size + self.pixels_per_column * self.pixel_size + self.col_trailer_size

    @property
    def lidar_packet_size(self) -> int:
        return self.packet_header_size + self.columns_per_packet * self.col_size + self.packet_footer_size

    imu_packet_size = IMU_PACKET_BYTES

    @property
    def profile_id(self) -> int:
        """PTL_PKT_* of include/ptudes_mi.h"""
        return PROFILES.index(self.profile)

    def frame_id(self, buf) -> int:
        return struct.unpack_from("<H", buf, self.frame_id_offset)[0]


# ---------------------------------------------------------------------------------------------- metadata
def _need(js: dict, key: str, where: str):
    if key not in js:
        raise ValueError(f"sensor metadata: field '{key}' is missing{where}")
    return js[key]


def _mat4(js: dict, key: str, where: str) -> np.ndarray:
    v = np.asarray(_need(js, key, where), dtype=np.float64)
    if v.size != 16:
        raise ValueError(f"sensor metadata: field '{key}'{where} needs 16 numbers, has {v.size}")
    return v.reshape(4, 4)


def metadata_from_dict(js: dict, source: str = "<dict>"):
    """The attribute tree of `read_metadata_json` from a parsed metadata document (flat legacy or nested)."""
    nested = "beam_intrinsics" in js or "lidar_data_format" in js or "sensor_info" in js
    if nested:
        beam = _need(js, "beam_intrinsics", "")
        fmt = js.get("lidar_data_format")
        lidar_intr = _need(js, "lidar_intrinsics", "")
        imu_intr = _need(js, "imu_intrinsics", "")
        sensor = _need(js, "sensor_info", "")
        config = js.get("config_params", {})
        w_beam, w_lidar, w_imu, w_sensor = " in beam_intrinsics", " in lidar_intrinsics", " in imu_intrinsics", " in sensor_info"
        mode = config.get("lidar_mode", js.get("lidar_mode"))
        if mode is None:
            raise ValueError("sensor metadata: field 'lidar_mode' is missing in config_params")
        profile = (fmt or {}).get("udp_profile_lidar", config.get("udp_profile_lidar"))
    else:
        beam = lidar_intr = imu_intr = sensor = js
        fmt = js.get("data_format")
        w_beam = w_lidar = w_imu = w_sensor = ""
        mode = js.get("lidar_mode")
        profile = (fmt or {}).get("udp_profile_lidar", js.get("udp_profile_lidar"))
    alt = np.asarray(_need(beam, "beam_altitude_angles", w_beam), dtype=np.float64)
    az = np.asarray(_need(beam, "beam_azimuth_angles", w_beam), dtype=np.float64)
    if mode is None:
        # the reference's back-fill (utils.py:161-167): Newer College 2020 metadata carries the beam angles but no lidar_mode
        print(f"WARNING: lidar_mode is not present in legacy metadata '{source}' so using lidar_mode: 1024x10")
        mode = "1024x10"
    if fmt is None:  # LEGACY, 16 columns per packet, W from lidar_mode and H from the beam count
        try:
            w = int(str(mode).split("x")[0])
        except ValueError:
            raise ValueError(f"sensor metadata: lidar_mode '{mode}' is not <columns>x<rate>") from None
        fmt = dict(pixels_per_column=len(alt), columns_per_frame=w, columns_per_packet=16)
        profile = profile or "LEGACY"
    where_fmt = " in lidar_data_format" if nested else " in data_format"
    h = int(_need(fmt, "pixels_per_column", where_fmt))
    if len(alt) != h or len(az) != h:
        raise ValueError(f"sensor metadata: {len(alt)} altitude / {len(az)} azimuth angles for pixels_per_column = {h}")
    extrinsic = np.asarray(js.get("extrinsic", (js.get("calibration_status", {}) or {}).get("extrinsic", np.eye(4).reshape(-1))),
                           dtype=np.float64)
    if extrinsic.size != 16:
        extrinsic = np.eye(4).reshape(-1)
    return SimpleNamespace(
        format=SimpleNamespace(pixels_per_column=h, columns_per_frame=int(_need(fmt, "columns_per_frame", where_fmt)),
                               columns_per_packet=int(_need(fmt, "columns_per_packet", where_fmt)),
                               udp_profile_lidar=profile_name(profile or "LEGACY"),
                               pixel_shift_by_row=list(fmt.get("pixel_shift_by_row", [0] * h))),
        beam_altitude_angles=alt, beam_azimuth_angles=az,
        lidar_origin_to_beam_origin_mm=float(_need(beam, "lidar_origin_to_beam_origin_mm", w_beam)),
        lidar_to_sensor_transform=_mat4(lidar_intr, "lidar_to_sensor_transform", w_lidar),
        imu_to_sensor_transform=_mat4(imu_intr, "imu_to_sensor_transform", w_imu),
        extrinsic=extrinsic.reshape(4, 4),
        prod_line=str(_need(sensor, "prod_line", w_sensor)), mode=str(mode))


def read_metadata_json(path: str):
    """Sensor metadata .json -> the attribute tree the package consumes (what ouster-sdk's SensorInfo gives the reference,
    utils.py:157-168): format.{pixels_per_column, columns_per_frame, columns_per_packet, udp_profile_lidar}, the beam angles,
    lidar_origin_to_beam_origin_mm, lidar_to_sensor_transform, imu_to_sensor_transform, extrinsic, prod_line, mode."""
    with open(path) as f:
        return metadata_from_dict(json.loads(f.read()), source=str(path))


# ---------------------------------------------------------------------------------------------- batching
class FrameBatcher:
    """The frame batching rule, one lidar packet at a time: the sweep index of a packet with frame id `f`,
    -1 for a late packet of the frame closed before."""

    def __init__(self):
        self.cur, self.sweep = None, -1

    def __call__(self, f: int) -> int:
        f = int(f) & 0xffff
        if self.cur is not None and f == ((self.cur - 1) & 0xffff):
            return -1
        if self.cur is None or f != self.cur:
            self.cur, self.sweep = f, self.sweep + 1
        return self.sweep


def batch_packets(frame_ids, lengths=None, packet_size: Optional[int] = None) -> Tuple[np.ndarray, int, int]:
    """The rule over the frame ids of lidar packets in arrival order (a packet of the wrong length is dropped and counted).
    Returns (sweep_of_packet int32[n] with -1 = dropped, number of sweeps, number of wrong-length packets)."""
    batcher, bad = FrameBatcher(), 0
    sop = np.full(len(frame_ids), -1, dtype=np.int32)
    for i, f in enumerate(frame_ids):
        if lengths is not None and lengths[i] != packet_size:
            bad += 1
            continue
        sop[i] = batcher(f)
    return sop, batcher.sweep + 1, bad


class PacketScan:
    """A decoded sweep: `range` (H, W) u32 mm staggered, `timestamp` (W,) u64 ns, `status` (W,) u16, `frame_id`, `h`, `w`,
    `ts` = the last valid column's time in seconds (ouster client.last_valid_column_ts) - what KissICPWrapper.register_frame takes
    for device-LUT input and StreamStatsTracker.trackScan for its span."""

    def __init__(self, range_mm, timestamp, status, frame_id, summary: Optional[dict] = None, fields: Optional[dict] = None):
        self.range = range_mm
        self.fields = dict(fields or {})  # name -> (H, W) u32 image of a channel field, staggered like `range` (PacketFeed(fields=...))
        self.timestamp, self.status, self.frame_id = timestamp, status, int(frame_id)
        self.h, self.w = range_mm.shape
        self.summary = summary
        valid = np.flatnonzero(np.asarray(status) & 1)
        self.last_valid_column_ts_ns = int(timestamp[valid[-1]]) if len(valid) else 0
        self.ts = self.last_valid_column_ts_ns * 1e-9


def imu_from_packet_bytes(buf: bytes) -> IMU:
    from .bag import decode_ouster_imu_packet
    return IMU.from_packet(decode_ouster_imu_packet(buf))


class PacketFeed:
    """Scans and IMU samples of a raw packet source, each with the index of the scan it belongs to: the reference's
    `OusterLidarData` (data.py:12-92) with the package's own batching rule and the device decode.
    source: iterable of ("lidar" | "imu", payload bytes, bag time) - bag.OusterPacketBagSource.  decoder: anything with
    `decode(packets (n, packet bytes) u8, sweep_of_packet) -> [PacketScan]` (default: core.PacketDecoder on `device_id`).
    Closed sweeps are held back until `chunk_sweeps` of them are complete, then decoded in one launch; the events leave in arrival order.
    fields: up to 4 channel fields ("reflectivity", "signal", "near_ir", ... - core.pkt_field) decoded beside the range from the same staged
    packets; each PacketScan then carries their (H, W) u32 images in `.fields`; the decoder must take `decode(..., fields=)`."""

    def __init__(self, source, info, device_id: int = 0, decoder=None, chunk_sweeps: int = 8, fields=()):
        self._source, self._info, self._device_id = source, info, device_id
        self.format = OusterPacketFormat.from_info(info)
        self._fields = tuple(str(f).lower() for f in fields)  # channel fields each PacketScan carries in `.fields` (core.pkt_field names)
        self._decoder = decoder
        self._chunk = max(1, int(chunk_sweeps))
        self.dropped_wrong_length = 0
        self.dropped_late = 0

    @property
    def metadata(self):
        return self._info

    def _dec(self):
        if self._decoder is None:
            from . import core
            self._decoder = core.PacketDecoder(self.format, max_sweeps=self._chunk, device_id=self._device_id)
        return self._decoder

    def _flush(self, pending) -> Iterator[Tuple[int, object]]:
        """decode the sweeps held in `pending` (events in arrival order; a sweep event is (idx, [payloads])) and let them go"""
        sweeps = [ev for ev in pending if isinstance(ev[1], list)]
        if sweeps:
            size = self.format.lidar_packet_size
            n = sum(len(ev[1]) for ev in sweeps)
            buf = np.empty((n, size), dtype=np.uint8)
            sop = np.empty(n, dtype=np.int32)
            i = 0
            for s, ev in enumerate(sweeps):
                for p in ev[1]:
                    buf[i] = np.frombuffer(p, dtype=np.uint8)
                    sop[i] = s
                    i += 1
            if self._fields:
                scans = iter(self._dec().decode(buf, sop, n_sweeps=len(sweeps), fields=self._fields))
            else:
                scans = iter(self._dec().decode(buf, sop, n_sweeps=len(sweeps)))
        for idx, d in pending:
            yield (idx, next(scans)) if isinstance(d, list) else (idx, d)

    def withScanIdx(self, *, start_scan: int = 0, end_scan: Optional[int] = None) -> Iterator[Tuple[int, object]]:
        """(scan index, PacketScan | IMU) in packet order, as data.OusterLidarData.withScanIdx: a sweep is emitted on the first packet of
        the next frame, IMU samples carry the open sweep's index, nothing before `start_scan`, the stream stops after scan `end_scan`,
        a trailing partial sweep is emitted at the end."""
        size = self.format.lidar_packet_size
        batcher, index, open_pkts = FrameBatcher(), 0, None
        created = False  # the reference makes the next LidarScan on the first packet BEHIND the one that closed a sweep (data.py:49-50)
        pending: List[Tuple[int, object]] = []
        held = 0
        for kind, buf, _ts in self._source:
            emit = index >= start_scan
            if kind == "imu":
                if emit:
                    pending.append((index, imu_from_packet_bytes(buf)))
                continue
            if kind != "lidar":
                continue
            if len(buf) != size:
                self.dropped_wrong_length += 1
                continue
            sweep = batcher(self.format.frame_id(buf))
            if sweep < 0:
                self.dropped_late += 1
                created = True
                continue
            created = sweep == index
            if not created:  # the first packet of the next frame closes the open sweep
                if emit:
                    pending.append((index, open_pkts))
                    held += 1
                open_pkts, index = None, sweep
                if end_scan is not None and index > end_scan:
                    yield from self._flush(pending)
                    return
                if held >= self._chunk:
                    yield from self._flush(pending)
                    pending, held = [], 0
            if open_pkts is None:
                open_pkts = []
            open_pkts.append(buf)
        if open_pkts is not None and created:
            pending.append((index, open_pkts))
        yield from self._flush(pending)

    def __iter__(self):
        return self.withScanIdx()

    def close(self) -> None:
        if hasattr(self._source, "close"):
            self._source.close()
