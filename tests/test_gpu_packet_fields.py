"""The channel fields of lidar pixels decoded on the device (csrc/packet_field_kernels.h) against the plain-loop restatement
(tests/helpers/ouster_fields_numpy.py): integer work, so every comparison is bit-equality.  The four profiles times every field each has, H in
{1, 4, 5}, W in {16, 32}, C = 16; one and four fields in a call; junk in every byte that is no field; RANGE through the field path against
`range_out`, the second witness; everything ptl_pktdec_decode gives against the same call without fields."""
import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib, core
from ptudes_lab_amd import packets as pk
from tests.helpers import ouster_fields_numpy as ofn
from tests.helpers import ouster_packets_numpy as opn
from tests.test_packets_cpu import _info

pytestmark = pytest.mark.gpu

PROFILES = ["LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"]
C = 16


def _range_image(rng, profile, H, W):
    """multiples of 8 so that RNG15 holds it, about a fifth without a return"""
    top = (1 << 15) * 8 if profile == "RNG15_RFL8_NIR8" else 1 << 19
    img = (rng.integers(0, top // 8, (H, W), dtype=np.uint32) * 8).astype(np.uint32)
    img[rng.random((H, W)) < 0.2] = 0
    return img


def _sweep(rng, profile, H, W, frame, st=None, ids=None):
    ts = rng.integers(1, 1 << 40, dtype=np.uint64) + np.arange(W, dtype=np.uint64) * np.uint64(97_657)
    fields = {n: ofn.random_field(rng, profile, n, (H, W)) for n in ofn.TABLE[profile] if n != "RANGE"}
    return ofn.encode_sweep(profile, _range_image(rng, profile, H, W), ts, np.ones(W, np.uint16) if st is None else st, frame, C, fields=fields,
                            junk=rng, ids=ids)


def _scene(profile, H, W, seed):
    """three sweeps in one call: sweep 0 with a column whose status bit is clear, a column with measurement id >= W and its last packet a
    second time with other pixels (the later wins); a packet of junk that belongs to no sweep; sweep 1 without a packet; sweep 2 plain"""
    rng = np.random.default_rng(seed)
    st = np.ones(W, np.uint16)
    st[3] = 0
    ids = np.arange(W)
    ids[5] = W + 2
    first = _sweep(rng, profile, H, W, 10, st, ids)
    again = _sweep(rng, profile, H, W, 10, st, ids)[-1]
    last = _sweep(rng, profile, H, W, 12)
    junk = bytes(rng.integers(0, 256, len(first[0]), dtype=np.uint8))
    bufs = first + [junk, again] + last
    sop = [0] * len(first) + [-1, 0] + [2] * len(last)
    return bufs, np.array(sop, np.int32), 3


def _groups(profile):
    """every field alone, and all of them in calls of four (the last call filled up from the front)"""
    names = list(ofn.TABLE[profile])
    four = [names[i:i + 4] for i in range(0, len(names), 4)]
    four[-1] = (four[-1] + names)[:4]
    return [[n] for n in names] + four


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("H", [1, 4, 5])
@pytest.mark.parametrize("profile", PROFILES)
def test_every_field_of_every_profile(profile, H, W):
    bufs, sop, S = _scene(profile, H, W, seed=100 * H + W)
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, C))
    dec = core.PacketDecoder(fmt, max_sweeps=S, max_packets=len(bufs))
    a = np.frombuffer(b"".join(bufs), dtype=np.uint8).reshape(len(bufs), fmt.lidar_packet_size).copy()
    plain = dec.decode_arrays(a, sop, S)
    want_plain = opn.decode(profile, H, W, C, bufs, list(sop), S)
    assert all(np.array_equal(g, w) for g, w in zip(plain[:3], want_plain[:3])) and plain[3] == want_plain[3]
    # (at W = 16 the repeated packet is the sweep's only one: its column with id >= W is ignored a second time)
    assert plain[3][0]["ignored_columns"] == (2 if W == C else 1) and plain[3][0]["valid_columns"] == W - 2 and plain[3][1]["valid_columns"] == 0
    seen = set()
    for names in _groups(profile):
        descs = [ofn.TABLE[profile][n] for n in names]
        want = ofn.decode_fields(profile, H, W, C, bufs, list(sop), S, descs)
        got = dec.decode_field_arrays(a, sop, [n.lower() for n in names], S)
        again = dec.decode_field_arrays(a, sop, [n.lower() for n in names], S)
        for n, g, g2, w in zip(names, got[0], again[0], want):
            assert g.dtype == np.uint32 and g.shape == (S, H, W) and np.array_equal(g, w), (profile, H, W, names, n)
            assert np.array_equal(g, g2), "two calls are bit-equal"
            assert not g[1].any() and not g[0][:, [3, 5]].any(), "a sweep without packets, an invalid column, a column with id >= W: zeros"
            if n == "RANGE":
                assert np.array_equal(g, got[1]), "RANGE as a field is range_out"
            elif (g[got[1] == 0] != 0).any():
                seen.add(n)
        # range_out, col_ts, status and summary of the new call are those of ptl_pktdec_decode on the same bytes
        for k in range(3):
            assert np.array_equal(got[1 + k], plain[k]) and np.array_equal(again[1 + k], plain[k]), (profile, names, k)
        assert got[4] == plain[3] == again[4]
    if H > 1:
        assert seen == set(ofn.TABLE[profile]) - {"RANGE"}, "every field is written where the pixel's range is 0"
    # the PacketScan view
    first = [n.lower() for n in list(ofn.TABLE[profile])[:2]]
    scans = dec.decode(a, sop, S, fields=first)
    want = ofn.decode_fields(profile, H, W, C, bufs, list(sop), S, [ofn.TABLE[profile][n.upper()] for n in first])
    assert len(scans) == S and all(set(s.fields) == set(first) for s in scans)
    assert all(np.array_equal(scans[s].fields[n], want[i][s]) for s in range(S) for i, n in enumerate(first))
    assert np.array_equal(scans[2].range, plain[0][2]) and scans[0].fields["range"] is not scans[0].range
    dec.close()


@pytest.mark.parametrize("profile", PROFILES)
def test_field_values_zero_and_all_ones(profile):
    H, W = 4, 16
    fmt = pk.OusterPacketFormat.from_info(_info(profile, H, W, C))
    dec = core.PacketDecoder(fmt, max_sweeps=1, max_packets=1)
    ts, st = np.arange(1, W + 1, dtype=np.uint64), np.ones(W, np.uint16)
    names = [n for n in ofn.TABLE[profile] if n != "RANGE"]
    px = ofn.pixel_size(profile)
    (packet,) = opn.encode_sweep(profile, np.zeros((H, W), np.uint32), ts, st, 1, C)
    for fill in ("ones", "zeros"):
        # the opposite in every other bit of the pixel: zeros around fields of all ones (the range is 0 too), all ones around zero fields
        value = {n: int(ofn.representable(ofn.TABLE[profile][n], 0xffffffff)) if fill == "ones" else 0 for n in names}
        buf = bytearray(packet)
        for c in range(C):
            for h in range(H):
                at = ofn.pixel_offset(profile, H, c, h)
                buf[at:at + px] = (b"\x00" if fill == "ones" else b"\xff") * px
                for n in names:
                    ofn.patch_field(buf, at, ofn.TABLE[profile][n], value[n])
        a = np.frombuffer(bytes(buf), dtype=np.uint8).reshape(1, -1).copy()
        for group in (names[:4], names[-4:]):
            got = dec.decode_field_arrays(a, [0], [n.lower() for n in group], 1)
            want = ofn.decode_fields(profile, H, W, C, [bytes(buf)], [0], 1, [ofn.TABLE[profile][n] for n in group])
            for n, g, w in zip(group, got[0], want):
                assert np.array_equal(g, w) and np.array_equal(g[0], np.full((H, W), value[n], dtype=np.uint32)), (profile, fill, n)
                assert value[n] > 0 or fill == "zeros"
    dec.close()


def _refused(fn, *words):
    with pytest.raises(ValueError) as e:
        fn()
    for w in words:
        assert str(w) in str(e.value), (w, str(e.value))


def test_refusals_name_their_numbers():
    H, W = 4, 16
    rng = np.random.default_rng(5)
    fmt = pk.OusterPacketFormat.from_info(_info("RNG19_RFL8_SIG16_NIR16", H, W, C))
    dec = core.PacketDecoder(fmt, max_sweeps=1, max_packets=2)
    bufs = _sweep(rng, "RNG19_RFL8_SIG16_NIR16", H, W, 1)
    a = np.frombuffer(b"".join(bufs), dtype=np.uint8).reshape(1, -1).copy()

    def field(**kw):
        f = core.pkt_field(fmt, "signal")
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    good = dec.decode_field_arrays(a, [0], ["signal"], 1)[0][0]
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(offset=12, bytes=1)], 1), "offset 12 + 1 bytes", "pixel of 12 bytes")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(offset=10, bytes=4)], 1), "offset = 10", "4 bytes")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(offset=1, bytes=2)], 1), "offset = 1", "2 bytes")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(offset=-2)], 1), "offset = -2")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(bytes=3)], 1), "bytes = 3")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(shift=32)], 1), "shift = 32")
    _refused(lambda: dec.decode_field_arrays(a, [0], [], 1), "n_fields = 0", "1 .. 4")
    _refused(lambda: dec.decode_field_arrays(a, [0], ["signal"] * 5, 1), "n_fields = 5", "1 .. 4")
    _refused(lambda: dec.decode_field_arrays(a, [0], [field(struct_size=16)], 1), "ptl_pkt_field", 16, 24)
    _refused(lambda: dec.decode_field_arrays(a, [1], ["signal"], 1), "names sweep 1")
    _refused(lambda: dec.decode(a, [0], 1, fields=["range2"]), "RNG19_RFL8_SIG16_NIR16", "RANGE2")
    small = pk.OusterPacketFormat.from_info(_info("RNG15_RFL8_NIR8", H, W, C))
    _refused(lambda: core.pkt_field(small, "signal"), "RNG15_RFL8_NIR8", "SIGNAL")
    # a descriptor of the caller's own: the high byte of the signal, shifted down - and nothing above left the decoder in a bad state
    own = dec.decode_field_arrays(a, [0], [field(offset=7, bytes=1), field(mask=0xff00, shift=-8), "signal"], 1)[0]
    assert np.array_equal(own[0], good >> 8) and np.array_equal(own[1], good >> 8) and np.array_equal(own[2], good)
    assert isinstance(field(), _lib.PktField)
    dec.close()
