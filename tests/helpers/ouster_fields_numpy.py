"""The channel fields of Ouster lidar pixels in plain struct loops: the field table, an encoder that patches field values into
the packets of tests/helpers/ouster_packets_numpy.py (imported, not edited), and the restatement of the field decode the device is held against.

Written from the definition's text, not from csrc/packet_field_kernels.h: a field is `bytes` (1, 2 or 4) at byte `offset` of the pixel,
offset % bytes == 0; its value is (little-endian word & mask) << shift for shift >= 0 and >> -shift otherwise, as u32; mask == 0 means all bits.
A field image is u32[H][W] staggered like the range image: a counted column (status bit 0, measurement id < W) writes its image column, the
later in arrival order wins, what no counted column supplies is 0; a field is written whether or not the pixel's range is 0."""
import struct

import numpy as np

from tests.helpers import ouster_packets_numpy as opn

FIELD_IDS = ("RANGE", "REFLECTIVITY", "SIGNAL", "NEAR_IR", "RANGE2", "REFLECTIVITY2", "SIGNAL2")
#          name: (offset, bytes, mask, shift)
TABLE = {
    "LEGACY": {"RANGE": (0, 4, 0x000fffff, 0), "REFLECTIVITY": (4, 2, 0, 0), "SIGNAL": (6, 2, 0, 0), "NEAR_IR": (8, 2, 0, 0)},
    "RNG19_RFL8_SIG16_NIR16": {"RANGE": (0, 4, 0x0007ffff, 0), "REFLECTIVITY": (4, 1, 0, 0), "SIGNAL": (6, 2, 0, 0), "NEAR_IR": (8, 2, 0, 0)},
    "RNG15_RFL8_NIR8": {"RANGE": (0, 2, 0x7fff, 3), "REFLECTIVITY": (2, 1, 0, 0), "NEAR_IR": (3, 1, 0, 4)},
    "RNG19_RFL8_SIG16_NIR16_DUAL": {"RANGE": (0, 4, 0x0007ffff, 0), "REFLECTIVITY": (3, 1, 0, 0), "SIGNAL": (8, 2, 0, 0), "NEAR_IR": (12, 2, 0, 0),
                                    "RANGE2": (4, 4, 0x0007ffff, 0), "REFLECTIVITY2": (7, 1, 0, 0), "SIGNAL2": (10, 2, 0, 0)},
}
_FMT = {1: "<B", 2: "<H", 4: "<I"}


def pixel_size(profile):
    return opn.TABLE[profile][2]


def pixel_offset(profile, H, c, h):
    """byte of pixel h of column c in a packet"""
    ph, ch, px, tr = opn.TABLE[profile][:4]
    return ph + c * (ch + H * px + tr) + ch + h * px


def _bits(desc):
    """the mask that is applied to the field's word (all of its bits for mask == 0)"""
    _, nbytes, mask, _ = desc
    return mask if mask else (1 << (8 * nbytes)) - 1


def field_value(buf, at, desc):
    """the value of the field `desc` of the pixel that starts at byte `at` of buf"""
    off, nbytes, _, shift = desc
    (word,) = struct.unpack_from(_FMT[nbytes], buf, at + off)
    v = word & _bits(desc)
    return (v << shift if shift >= 0 else v >> -shift) & 0xffffffff


def representable(desc, raw):
    """the field values that raw words give: raw (integers, any shape) masked and shifted - what an encoder can write and a decoder gives back"""
    _, _, _, shift = desc
    v = np.asarray(raw, dtype=np.uint64) & np.uint64(_bits(desc))
    return ((v << np.uint64(shift)) if shift >= 0 else (v >> np.uint64(-shift))).astype(np.uint32)


def random_field(rng, profile, name, shape):
    """a field image of representable values, 0 and all ones among them"""
    desc = TABLE[profile][name]
    raw = rng.integers(0, _bits(desc) + 1, shape, dtype=np.uint64)
    flat = raw.reshape(-1)
    flat[rng.integers(0, flat.size, 2)] = 0
    flat[rng.integers(0, flat.size, 2)] = _bits(desc)
    return representable(desc, raw)


def patch_field(buf, at, desc, value):
    """writes `value` (a representable one) into the field of the pixel at byte `at` of the bytearray; the word's bits outside the mask stay"""
    off, nbytes, _, shift = desc
    m = _bits(desc)
    raw = (int(value) >> shift if shift >= 0 else int(value) << -shift) & m
    (old,) = struct.unpack_from(_FMT[nbytes], buf, at + off)
    struct.pack_into(_FMT[nbytes], buf, at + off, (old & ~m & ((1 << (8 * nbytes)) - 1)) | raw)


def encode_sweep(profile, image, col_ts, status, frame_id, C, fields=None, junk=None, ids=None):
    """opn.encode_sweep, then the images of `fields` (name -> (H, W) representable values) patched in at the table's offsets; every byte that is
    no field, time, id, status or frame id is random when `junk` is a Generator"""
    H, W = image.shape
    packets = opn.encode_sweep(profile, image, col_ts, status, frame_id, C, junk=junk, ids=ids)
    out = []
    for k, p in enumerate(packets):
        buf = bytearray(p)
        for name, img in (fields or {}).items():
            for c in range(C):
                for h in range(H):
                    patch_field(buf, pixel_offset(profile, H, c, h), TABLE[profile][name], img[h, k * C + c])
        out.append(bytes(buf))
    return out


def decode_fields(profile, H, W, C, packets, sop, n_sweeps, descs):
    """[field image (S, H, W) u32 per descriptor (offset, bytes, mask, shift)], packet by packet in arrival order"""
    ph, ch, px, tr = opn.TABLE[profile][:4]
    out = [np.zeros((n_sweeps, H, W), np.uint32) for _ in descs]
    for buf, s in zip(packets, sop):
        if s < 0:
            continue
        for c in range(C):
            o = ph + c * (ch + H * px + tr)
            (mid,) = struct.unpack_from("<H", buf, o + 8)
            if profile == "LEGACY":
                (status,) = struct.unpack_from("<I", buf, o + ch + H * px)
            else:
                (status,) = struct.unpack_from("<H", buf, o + 10)
            if not status & 1 or mid >= W:
                continue
            for img, desc in zip(out, descs):
                for h in range(H):
                    img[s, h, mid] = field_value(buf, o + ch + h * px, desc)
    return out
