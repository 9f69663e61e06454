"""Ouster lidar packets in plain numpy / struct loops: an encoder (image -> packets) and the restatement of the batching rule and of the
decode (packets -> image, column times, statuses, summary) that the device decoder is held against.

Written from the format table of DESIGN.md 3.16, not from csrc/packet_kernels.h and not from ptudes_lab_amd/packets.py; it shares no
code with either.  Per profile: (packet header, column header, pixel, column trailer, packet footer) bytes, where the frame id, the
status and the range are, and the range's mask and shift.  Everything is little-endian."""
import struct

import numpy as np

#            pkt hdr, col hdr, pixel, trailer, footer, range fmt, mask,       shift
TABLE = {
    "LEGACY": (0, 16, 12, 4, 0, "<I", 0x000fffff, 0),
    "RNG19_RFL8_SIG16_NIR16": (32, 12, 12, 0, 32, "<I", 0x0007ffff, 0),
    "RNG15_RFL8_NIR8": (32, 12, 4, 0, 32, "<H", 0x7fff, 3),
    "RNG19_RFL8_SIG16_NIR16_DUAL": (32, 12, 16, 0, 32, "<I", 0x0007ffff, 0),
}


def packet_size(profile, H, C):
    ph, ch, px, tr, ft, _, _, _ = TABLE[profile]
    return ph + C * (ch + H * px + tr) + ft


def encode_packet(profile, H, frame_id, ids, ts, status, ranges, junk=None):
    """One packet of C = len(ids) columns: measurement ids, timestamps (ns), status words (bit 0 = valid), ranges (C, H) in mm
    (RNG15: must be multiples of 8).  junk: a numpy Generator - every byte the decoder must not read as range, time, id, status or
    frame id is random instead of 0, bits above the range mask included."""
    ph, ch, px, tr, ft, rfmt, mask, shift = TABLE[profile]
    C = len(ids)
    size = packet_size(profile, H, C)
    buf = bytearray(junk.integers(0, 256, size, dtype=np.uint8).tobytes() if junk is not None else bytes(size))
    if profile != "LEGACY":
        struct.pack_into("<HH", buf, 0, 1, frame_id & 0xffff)
    for c in range(C):
        o = ph + c * (ch + H * px + tr)
        struct.pack_into("<Q", buf, o, int(ts[c]))
        struct.pack_into("<H", buf, o + 8, int(ids[c]))
        if profile == "LEGACY":
            struct.pack_into("<H", buf, o + 10, frame_id & 0xffff)
            struct.pack_into("<I", buf, o + ch + H * px, 0xffffffff if status[c] & 1 else 0)
        else:
            struct.pack_into("<H", buf, o + 10, int(status[c]))
        for h in range(H):
            po = o + ch + h * px
            v = (int(ranges[c][h]) >> shift) & mask
            if junk is not None:  # the bits of the range word above the mask belong to other fields
                (old,) = struct.unpack_from(rfmt, buf, po)
                v |= old & ~mask & (0xffff if rfmt == "<H" else 0xffffffff)
            struct.pack_into(rfmt, buf, po, v)
    return bytes(buf)


def encode_sweep(profile, image, col_ts, status, frame_id, C, junk=None, ids=None):
    """The W / C packets of one sweep: image (H, W) u32 mm, col_ts (W,) ns, status (W,); ids: the measurement id written for each
    image column (default: its index)."""
    H, W = image.shape
    ids = np.arange(W) if ids is None else np.asarray(ids)
    out = []
    for a in range(0, W, C):
        sl = slice(a, a + C)
        out.append(encode_packet(profile, H, frame_id, ids[sl], col_ts[sl], status[sl], image[:, sl].T, junk))
    return out


def frame_id_of(profile, buf):
    return struct.unpack_from("<H", buf, 10 if profile == "LEGACY" else 2)[0]


def batch(profile, H, C, packets):
    """The batching rule: sweep_of_packet (int32, -1 = dropped), number of sweeps, wrong-length packets"""
    size = packet_size(profile, H, C)
    sop, cur, sweep, bad = [], None, -1, 0
    for buf in packets:
        if len(buf) != size:
            bad += 1
            sop.append(-1)
            continue
        f = frame_id_of(profile, buf)
        if cur is None:
            cur, sweep = f, 0
        elif f == cur:
            pass
        elif f == (cur - 1) % 65536:
            sop.append(-1)
            continue
        else:
            cur, sweep = f, sweep + 1
        sop.append(sweep)
    return np.array(sop, dtype=np.int32), sweep + 1, bad


def decode(profile, H, W, C, packets, sop, n_sweeps):
    """-> (range (S, H, W) u32, ts (S, W) u64, status (S, W) u16, [summary dict] * S), packet by packet in arrival order: a counted
    column overwrites what an earlier one left at its measurement id, so the later wins"""
    ph, ch, px, tr, ft, rfmt, mask, shift = TABLE[profile]
    rng = np.zeros((n_sweeps, H, W), np.uint32)
    ts = np.zeros((n_sweeps, W), np.uint64)
    st = np.zeros((n_sweeps, W), np.uint16)
    frame = [None] * n_sweeps
    ignored = [0] * n_sweeps
    for buf, s in zip(packets, sop):
        if s < 0:
            continue
        if frame[s] is None:
            frame[s] = frame_id_of(profile, buf)
        for c in range(C):
            o = ph + c * (ch + H * px + tr)
            (t,) = struct.unpack_from("<Q", buf, o)
            (mid,) = struct.unpack_from("<H", buf, o + 8)
            if profile == "LEGACY":
                (status,) = struct.unpack_from("<I", buf, o + ch + H * px)
            else:
                (status,) = struct.unpack_from("<H", buf, o + 10)
            if not status & 1:
                continue
            if mid >= W:
                ignored[s] += 1
                continue
            ts[s, mid], st[s, mid] = t, status & 0xffff
            for h in range(H):
                (v,) = struct.unpack_from(rfmt, buf, o + ch + h * px)
                rng[s, h, mid] = (v & mask) << shift
    sums = []
    for s in range(n_sweeps):
        valid = np.flatnonzero(st[s] & 1)
        sums.append(dict(frame_id=frame[s] or 0, valid_columns=len(valid),
                         first_valid_id=int(valid[0]) if len(valid) else 0, last_valid_id=int(valid[-1]) if len(valid) else 0,
                         first_valid_ts=int(ts[s, valid[0]]) if len(valid) else 0, last_valid_ts=int(ts[s, valid[-1]]) if len(valid) else 0,
                         nonzero_ranges=int(np.count_nonzero(rng[s])), ignored_columns=ignored[s]))
    return rng, ts, st, sums


class NumpyDecoder:
    """The decoder `packets.PacketFeed(decoder=...)` takes, on the host: the event order of the feed is testable without a GPU"""

    def __init__(self, profile, H, W, C):
        self.args = (profile, H, W, C)

    def decode(self, packets, sweep_of_packet, n_sweeps=None):
        from ptudes_lab_amd.packets import PacketScan
        bufs = [bytes(p) for p in np.asarray(packets)]
        S = int(n_sweeps) if n_sweeps is not None else int(max(sweep_of_packet)) + 1
        rng, ts, st, sums = decode(*self.args, bufs, list(sweep_of_packet), S)
        return [PacketScan(rng[i], ts[i], st[i], sums[i]["frame_id"], sums[i]) for i in range(S)]
