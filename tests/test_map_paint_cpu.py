"""The painted map, the parts that need no GPU: the restatement the GPU tests compare with (tests/helpers/map_paint_numpy.py)
against a brute force in Python scalars and against answers written down by hand, the C-ABI surface of ptl_paint_* with its layout and its
refusals before any HIP call, and the host side of core.PaintValues."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from tests.helpers import map_paint_numpy as mp
from tests.helpers.abi_surface import declared as _declared, exported as _exported, struct_fields as _header_fields

NEW = {"ptl_paint_sizeof_result", "ptl_paint_create", "ptl_paint_destroy", "ptl_paint_add_posed_range", "ptl_paint_add_posed_xyz",
       "ptl_paint_read"}
PTL_ERR_ARG = -1
VS = 0.5
ALL_ONES = 0xffffffff


def hand_case():
    """stored points, one sweep of rays under the identity pose, and the answer.  Voxel 0 of the truncating index spans (-vs, vs): the first
    three stored points and (0, 0, 0) share voxel (0, 0, 0); the two equal points at (1.75, 0, 0) are what a voxel with room stores of two equal
    returns"""
    stored = np.array([[0.25, 0.25, 0.25], [0.3, 0.1, 0.2], [-0.25, 0.25, 0.25], [1.75, 0.0, 0.0], [1.75, 0.0, 0.0], [0.0, 0.0, 0.0]])
    rays = [  # (end, has a return, field value)
        ((0.25, 0.25, 0.25), True, 7),            # at stored 0
        ((0.25, 0.25, 0.25), True, ALL_ONES),     # at stored 0 again: the sum passes 2^32
        ((1.75, 0.0, 0.0), True, 5),              # at stored 3 AND 4: one matched ray, two points painted
        ((0.26, 0.25, 0.25), True, 11),           # into the voxel of stored 0 .. 2 and 5, at none of them (a full voxel's later return)
        ((10.0, 10.0, 10.0), True, 13),           # into an absent voxel
        ((0.3, 0.1, 0.2), False, 99),             # no return, at the place of stored 1: adds nothing
        ((1.0e7, 0.0, 0.0), True, 17),            # outside the key range
        ((-0.0, 0.0, 0.0), True, 3),              # -0.0 == 0.0: at stored 5
        ((math.nan, 0.0, 0.0), True, 19),         # not finite
    ]
    w = np.array([r[0] for r in rays])
    sweep = (w, np.array([r[1] for r in rays]), np.array([r[2] for r in rays], dtype=np.uint32))
    want_sum = np.array([7 + ALL_ONES, 0, 0, 5, 5, 3], dtype=np.uint64)
    want_count = np.array([2, 0, 0, 1, 1, 1], dtype=np.uint32)
    counts = dict(n_points=6, n_points_painted=4, n_scans=1, n_scans_skipped=1, n_rays_matched=4, n_rays_unmatched=4, n_no_return=1, sum_count=5)
    return stored, [sweep, None], want_sum, want_count, counts


def test_restatement_against_brute_force_and_the_answers_by_hand():
    stored, sweeps, want_sum, want_count, counts = hand_case()
    for form in (mp.paint, mp.paint_brute, mp.paint_arrays):
        s, k, n = form(stored, sweeps, VS)
        assert s.dtype == np.uint64 and k.dtype == np.uint32
        assert np.array_equal(s, want_sum) and np.array_equal(k, want_count), (form.__name__, s.tolist(), k.tolist())
        assert n == counts, (form.__name__, n)
    # the same sweep twice: everything but the point count doubles
    s2, k2, n2 = mp.paint(stored, [sweeps[0], sweeps[0]], VS)
    assert np.array_equal(s2, 2 * want_sum) and np.array_equal(k2, 2 * want_count) and n2["n_rays_matched"] == 8 and n2["n_scans_skipped"] == 0
    # three rays of all ones at one point: the sum is exact in 64 bits
    one = (np.tile(stored[0], (3, 1)), np.ones(3, dtype=bool), np.full(3, ALL_ONES, dtype=np.uint32))
    s3, k3, _ = mp.paint(stored, [one], VS)
    assert int(s3[0]) == 3 * ALL_ONES > 1 << 33 and int(k3[0]) == 3


def test_restatement_against_brute_force_on_random_scenes():
    """random returns on a grid of eighths (many share a voxel, some coincide), a map of their first P points per voxel, painted by all of
    them: the invariant the GPU test asserts on the device holds for the restatement"""
    rng = np.random.default_rng(27)
    for P in (1, 2, 5):
        w = rng.integers(-24, 25, (120, 3)) / 8.0
        ret = rng.random(120) > 0.1
        value = rng.integers(0, 1 << 32, 120, dtype=np.uint64).astype(np.uint32)
        stored = mp.first_points_per_voxel(w[ret], VS, P)
        a, b = mp.paint(stored, [(w, ret, value)], VS), mp.paint_brute(stored, [(w, ret, value)], VS)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        c = mp.paint_arrays(stored, [(w, ret, value), None, (w[::-1], ret[::-1], value[::-1])], VS)
        assert np.array_equal(c[0], 2 * a[0]) and np.array_equal(c[1], 2 * a[1]) and c[2]["n_rays_unmatched"] == 2 * a[2]["n_rays_unmatched"]
        assert mp.paint_arrays(np.zeros((0, 3)), [(w, ret, value)], VS)[2]["n_rays_unmatched"] == int(ret.sum())
        assert (a[1] >= 1).all(), "every stored point is the end of one of the rays that built the map"
        assert a[2]["n_no_return"] == int((~ret).sum()) and a[2]["n_rays_matched"] + a[2]["n_rays_unmatched"] == int(ret.sum())
        rows = mp.sorted_rows(stored, a[0], a[1])
        assert np.array_equal(rows, mp.sorted_rows(stored[::-1], a[0][::-1], a[1][::-1])), "the rows do not depend on the order handed in"


def test_key_of_truncates_toward_zero_and_knows_the_key_range():
    assert mp.key_of((0.49, -0.49, 0.0), VS) == (0, 0, 0) and mp.key_of((0.5, -0.5, -0.75), VS) == (1, -1, -1)
    edge = float(1 << 20) * VS
    assert mp.key_of((edge - VS, 0.0, 0.0), VS) == ((1 << 20) - 1, 0, 0) and mp.key_of((edge, 0.0, 0.0), VS) is None
    assert mp.key_of((-edge, 0.0, 0.0), VS) == (-(1 << 20), 0, 0) and mp.key_of((-edge - VS, 0.0, 0.0), VS) is None
    assert mp.key_of((math.inf, 0.0, 0.0), VS) is None and mp.key_of((0.0, math.nan, 0.0), VS) is None


CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def test_surface_layout_and_refusals_before_any_hip_call():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= exported and NEW <= declared and declared == exported == set(_lib.PROTOTYPES)
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points and a new struct change no existing struct or prototype
    # header <-> binding, field by field
    want = [(f, CTYPES[t] if n is None else CTYPES[t] * n) for f, t, n in _header_fields("ptl_paint_result")]
    assert [(f, t) for f, t in _lib.PaintResult._fields_] == want
    assert [f for f, _ in want] == ["struct_size", "abi_version", "n_points", "n_points_painted", "n_scans", "n_scans_skipped", "n_rays_matched",
                                    "n_rays_unmatched", "n_no_return", "sum_count", "device_ms"]
    assert L.ptl_paint_sizeof_result() == C.sizeof(_lib.PaintResult) == 80
    fresh = _lib.PaintResult()
    assert (fresh.struct_size, fresh.abi_version) == (80, 6)

    # a short, a long and a stale result struct are refused without a byte written: the struct sits in front of a canary.  The check of the
    # two leading words comes before the handle is looked at, so a block of zeros stands in for one
    class Guarded(C.Structure):
        _fields_ = [("res", _lib.PaintResult), ("canary", C.c_uint8 * 32)]

    stand_in = (C.c_uint8 * 4096)()
    for size, abi in ((72, 6), (80, 5), (88, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.res.struct_size, g.res.abi_version = size, abi
        before = bytes(g)
        rc = L.ptl_paint_read(C.cast(stand_in, C.c_void_p), C.cast(C.byref(g), C.POINTER(_lib.PaintResult)), None, None, None, 0, None)
        msg = L.ptl_last_error().decode()
        assert rc == PTL_ERR_ARG and "ptl_paint_result" in msg and str(size) in msg and str(abi) in msg and "80" in msg, msg
        assert bytes(g) == before, "nothing is written on a mismatch"
    assert bytes(stand_in) == bytes(4096)

    # null arguments
    assert L.ptl_paint_create(None, None) == PTL_ERR_ARG and "ptl_paint_create" in L.ptl_last_error().decode()
    assert L.ptl_paint_create(None, C.byref(C.c_void_p())) == PTL_ERR_ARG
    assert L.ptl_paint_read(None, C.byref(_lib.PaintResult()), None, None, None, 0, None) == PTL_ERR_ARG
    assert L.ptl_paint_read(C.cast(stand_in, C.c_void_p), None, None, None, None, 0, None) == PTL_ERR_ARG
    assert L.ptl_paint_add_posed_range(None, None, None, None, None, None, None, None) == PTL_ERR_ARG
    assert "ptl_paint_add_posed_range" in L.ptl_last_error().decode()
    assert L.ptl_paint_add_posed_xyz(None, None, None, None, 1, 1, None, None, None) == PTL_ERR_ARG
    assert "ptl_paint_add_posed_xyz" in L.ptl_last_error().decode()
    assert L.ptl_paint_destroy(None) == 0


# ---------------------------------------------------------------------------------------------- packet fields
PROFILES = ["LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "RNG19_RFL8_SIG16_NIR16_DUAL"]
# known answers at LITERAL offsets of a pixel: profile -> [(field, byte offset, little-endian bytes written there, the value)]
KNOWN = {
    "LEGACY": [("RANGE", 0, b"\x45\x23\xf1\xff", 0x12345), ("REFLECTIVITY", 4, b"\xcd\xab", 0xabcd), ("SIGNAL", 6, b"\x34\x12", 0x1234),
               ("NEAR_IR", 8, b"\xfe\xca", 0xcafe)],
    "RNG19_RFL8_SIG16_NIR16": [("RANGE", 0, b"\x45\x23\xf9\xff", 0x12345), ("REFLECTIVITY", 4, b"\x5a", 0x5a), ("SIGNAL", 6, b"\x34\x12", 0x1234),
                               ("NEAR_IR", 8, b"\xfe\xca", 0xcafe)],
    "RNG15_RFL8_NIR8": [("RANGE", 0, b"\x34\x92", 0x1234 << 3), ("REFLECTIVITY", 2, b"\x5a", 0x5a), ("NEAR_IR", 3, b"\xa5", 0xa5 << 4)],
    "RNG19_RFL8_SIG16_NIR16_DUAL": [("RANGE", 0, b"\x45\x23\x01", 0x12345), ("REFLECTIVITY", 3, b"\x5a", 0x5a), ("RANGE2", 4, b"\x21\x43\x05", 0x54321),
                                    ("REFLECTIVITY2", 7, b"\xa5", 0xa5), ("SIGNAL", 8, b"\x34\x12", 0x1234), ("SIGNAL2", 10, b"\x78\x56", 0x5678),
                                    ("NEAR_IR", 12, b"\xfe\xca", 0xcafe)],
}


def _descriptor(profile, name):
    """(offset, bytes, mask, shift) of the library's table, or the refusal's text"""
    from ptudes_lab_amd import core
    fmt = _lib.PktFormat()
    fmt.profile, fmt.pixels_per_column, fmt.columns_per_frame, fmt.columns_per_packet = PROFILES.index(profile), 4, 16, 16
    try:
        d = core.pkt_field(fmt, name.lower())
    except ValueError as e:
        return str(e)
    return d.offset, d.bytes, d.mask, d.shift


@pytest.mark.parametrize("profile", PROFILES)
def test_field_extraction_on_known_answer_pixels(profile):
    from tests.helpers import ouster_fields_numpy as ofn
    px = ofn.pixel_size(profile)
    rng = np.random.default_rng(PROFILES.index(profile))
    assert sorted(n for n, *_ in KNOWN[profile]) == sorted(ofn.TABLE[profile]), "every field the profile has"
    for trial in range(4):
        # junk in every byte, then the known bytes at their literal offsets - in front of and behind the pixel too
        buf = bytearray(rng.integers(0, 256, px + 8, dtype=np.uint8).tobytes())
        for _, off, raw, _ in KNOWN[profile]:
            buf[4 + off:4 + off + len(raw)] = raw
        for name, _, _, want in KNOWN[profile]:
            assert ofn.field_value(bytes(buf), 4, ofn.TABLE[profile][name]) == want, (profile, name, trial)
    # a byte field whose neighbours are all ones, and one of all ones whose neighbours are zero
    for name, desc in ofn.TABLE[profile].items():
        if desc[1] != 1:
            continue
        ones = bytearray(b"\xff" * (px + 8))
        ones[4 + desc[0]] = 0x00
        assert ofn.field_value(bytes(ones), 4, desc) == 0, (profile, name)
        zeros = bytearray(px + 8)
        zeros[4 + desc[0]] = 0xff
        assert ofn.field_value(bytes(zeros), 4, desc) == (0xff << desc[3]), (profile, name)
    # the encoder's patch and the decode are inverse on representable values, and leave every other field alone
    for name, desc in ofn.TABLE[profile].items():
        buf = bytearray(rng.integers(0, 256, px, dtype=np.uint8).tobytes())
        others = {n: ofn.field_value(bytes(buf), 0, d) for n, d in ofn.TABLE[profile].items() if n != name}
        v = int(ofn.random_field(rng, profile, name, (8,))[5])
        ofn.patch_field(buf, 0, desc, v)
        assert ofn.field_value(bytes(buf), 0, desc) == v
        assert {n: ofn.field_value(bytes(buf), 0, d) for n, d in ofn.TABLE[profile].items() if n != name} == others, (profile, name)


def test_the_library_s_field_table_is_the_helper_s_and_the_header_s():
    from tests.helpers import ouster_fields_numpy as ofn
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    L = _lib.lib()
    assert {"ptl_pkt_sizeof_field", "ptl_pkt_field_default", "ptl_pktdec_decode_fields"} <= _declared() & _exported(_lib.LIB_PATH) & set(_lib.PROTOTYPES)
    want = [(f, CTYPES[t] if n is None else CTYPES[t] * n) for f, t, n in _header_fields("ptl_pkt_field")]
    assert [(f, t) for f, t in _lib.PktField._fields_] == want
    assert L.ptl_pkt_sizeof_field() == C.sizeof(_lib.PktField) == 24
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptudes_mi.h")).read()
    for i, name in enumerate(ofn.FIELD_IDS):
        assert f"#define PTL_PKT_FIELD_{name} {i}\n" in hdr and _lib.PKT_FIELDS[i] == name
    assert "#define PTL_PKT_MAX_FIELDS 4 " in hdr and _lib.PKT_MAX_FIELDS == 4
    for profile in PROFILES:
        for name in ofn.FIELD_IDS:
            got = _descriptor(profile, name)
            if name in ofn.TABLE[profile]:
                assert got == ofn.TABLE[profile][name], (profile, name, got)
                assert got[0] % got[1] == 0 and got[0] + got[1] <= ofn.pixel_size(profile)
            else:
                assert isinstance(got, str) and profile in got and name in got, (profile, name, got)  # (signal on RNG15_RFL8_NIR8 among them)
    from ptudes_lab_amd import core
    with pytest.raises(ValueError, match="unknown lidar field 'colour'"):
        core.pkt_field(_lib.PktFormat(), "colour")

    # a descriptor of another size or version is refused without a byte written
    class Guarded(C.Structure):
        _fields_ = [("f", _lib.PktField), ("canary", C.c_uint8 * 32)]

    fmt = _lib.PktFormat()
    fmt.profile, fmt.pixels_per_column, fmt.columns_per_frame, fmt.columns_per_packet = 1, 4, 16, 16
    for size, abi in ((16, 6), (24, 7), (32, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.f.struct_size, g.f.abi_version = size, abi
        before = bytes(g)
        assert L.ptl_pkt_field_default(C.byref(fmt), 1, C.cast(C.byref(g), C.POINTER(_lib.PktField))) == PTL_ERR_ARG
        msg = L.ptl_last_error().decode()
        assert "ptl_pkt_field" in msg and str(size) in msg and str(abi) in msg and "24" in msg, msg
        assert bytes(g) == before
    assert L.ptl_pkt_field_default(None, 0, None) == PTL_ERR_ARG
    assert L.ptl_pkt_field_default(C.byref(fmt), 7, C.byref(_lib.PktField())) == PTL_ERR_ARG and "7" in L.ptl_last_error().decode()
    assert L.ptl_pktdec_decode_fields(None, None, 0, 0, None, 1, None, 1, None, None, None, None, None) == PTL_ERR_ARG


def test_packet_scan_and_feed_carry_fields():
    from ptudes_lab_amd import packets as pk
    scan = pk.PacketScan(np.zeros((2, 4), np.uint32), np.zeros(4, np.uint64), np.ones(4, np.uint16), 7)
    assert scan.fields == {}
    img = np.arange(8, dtype=np.uint32).reshape(2, 4)
    assert pk.PacketScan(np.zeros((2, 4), np.uint32), np.zeros(4, np.uint64), np.ones(4, np.uint16), 7, fields={"signal": img}).fields["signal"] is img


def test_scalar_colors_ends_nan_and_no_slope():
    from ptudes_lab_amd import core, fly
    pal = core.rgba_word(core.default_palette())
    grey = int(core.rgba_word(np.array([128, 128, 128, 255], dtype=np.uint8)))
    v = np.array([-5.0, 10.0, 10.0 + 90.0 / 256.0, 55.0, 100.0 - 1e-9, 100.0, 1e9, np.nan, np.inf])
    w = fly.scalar_colors(v, lo=10.0, hi=100.0)
    assert w.dtype == np.uint32 and w.tolist() == [int(pal[0]), int(pal[0]), int(pal[1]), int(pal[128]), int(pal[255]), int(pal[255]),
                                                    int(pal[255]), grey, grey]
    # the default range: the 1st and 99th percentile of the finite values
    x = np.concatenate([np.arange(101.0), [np.nan]])
    d = fly.scalar_colors(x)
    assert np.array_equal(d, fly.scalar_colors(x, lo=1.0, hi=99.0)) and d[0] == pal[0] and d[100] == pal[255] and d[101] == grey and d[1] == pal[0] and d[99] == pal[255]
    # lo == hi: no slope - below it entry 0, everything else entry 255; no finite value at all: every point unpainted
    flat = fly.scalar_colors(np.array([1.0, 2.0, 3.0, np.nan]), lo=2.0, hi=2.0)
    assert flat.tolist() == [int(pal[0]), int(pal[255]), int(pal[255]), grey]
    assert fly.scalar_colors(np.full(3, 7.0)).tolist() == [int(pal[255])] * 3
    assert fly.scalar_colors(np.full(2, np.nan), unpainted=(1, 2, 3, 4)).tolist() == [0x04030201] * 2 and len(fly.scalar_colors(np.zeros(0))) == 0
    # a palette of the caller's
    own = np.zeros((256, 4), dtype=np.uint8)
    own[:, 0] = np.arange(256)
    assert fly.scalar_colors(np.array([0.0, 0.5, 1.0]), lo=0.0, hi=1.0, palette=own).tolist() == [0, 128, 255]


def test_painted_ply_round_trip(tmp_path):
    from ptudes_lab_amd.utils import load_map_ply, save_map_ply
    xyz = np.random.default_rng(2).normal(size=(5, 3))
    mean, count = np.array([1.5, np.nan, 3.0, 0.0, 4294967295.0]), np.array([2, 0, 1, 7, 3], dtype=np.uint32)
    path = str(tmp_path / "painted.ply")
    save_map_ply(path, xyz, {"reflectivity": mean, "reflectivity_count": count})
    head = open(path, "rb").read(400)
    assert b"property double reflectivity\nproperty uint reflectivity_count\nend_header\n" in head
    pts, s = load_map_ply(path, scalars=True)
    assert np.array_equal(pts, xyz) and np.array_equal(s["reflectivity"], mean, equal_nan=True) and np.array_equal(s["reflectivity_count"], count)
    assert np.array_equal(load_map_ply(path), xyz)
    with pytest.raises(ValueError, match="colour"):
        save_map_ply(path, xyz, {"colour": mean, "colour_count": count})
    with pytest.raises(ValueError, match="PLY file only"):
        save_map_ply(str(tmp_path / "m.npy"), xyz, {"range": mean, "range_count": count})


def test_the_command_refuses_before_any_device(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    poses = tmp_path / "p.csv"
    poses.write_text("")
    r = run(ptudes_cli, ["flyby", "--help"])
    assert r.exit_code == 0 and all(o in r.output for o in ("--color-by", "--color-range", "--save-painted")) and "height palette" in " ".join(r.output.split())
    base = ["flyby", "--synthetic", "1000", "--nc-gt-poses", str(poses)]
    for field in ("reflectivity", "signal", "near_ir"):
        r = run(ptudes_cli, base + ["--color-by", field])
        assert r.exit_code != 0 and field in r.output and "--synthetic" in r.output, r.output
    for extra, words in ((["--color-by", "colour"], ["colour", "reflectivity"]),
                         (["--color-by", "range", "--carve"], ["--carve", "range"]),
                         (["--color-by", "range", "--color-range", "5"], ["--color-range 5", "LO,HI"]),
                         (["--color-by", "range", "--color-range", "5,5"], ["HI must be above LO"]),
                         (["--color-by", "range", "--save-painted", "out.npy"], ["out.npy", ".ply"]),
                         (["--color-range", "0,1"], ["--color-range belongs to --color-by"]),
                         (["--save-painted", "x.ply"], ["--save-painted belongs to --color-by"])):
        r = run(ptudes_cli, base + extra)
        assert r.exit_code != 0 and all(w in r.output for w in words), (extra, r.output)
    r = run(ptudes_cli, ["flyby", "--synthetic", "1000", "--kitti-poses", str(poses), "--color-by", "range"])
    assert r.exit_code != 0 and "--kitti-poses" in r.output and "--color-by range" in r.output, r.output
    # a profile without the field: refused naming both, after the metadata is read and before a device is touched
    from ptudes_lab_amd import core, fly
    info = __import__("types").SimpleNamespace(format=__import__("types").SimpleNamespace(
        pixels_per_column=4, columns_per_frame=16, columns_per_packet=16, udp_profile_lidar="RNG15_RFL8_NIR8"))
    with pytest.raises(ValueError) as e:
        fly.paint_packet_bag(None, [], info, None, "signal")
    assert "RNG15_RFL8_NIR8" in str(e.value) and "SIGNAL" in str(e.value)
    assert {"MapPainter", "paint_packet_bag", "scalar_colors"} <= set(dir(fly)) and hasattr(core.Renderer, "set_point_colors")


def test_paint_values_mean_and_lines():
    from ptudes_lab_amd import core
    assert hasattr(core, "Painter") and {"add_posed", "values", "close"} <= set(dir(core.Painter))
    res = _lib.PaintResult()
    res.n_points, res.n_points_painted, res.n_scans, res.n_rays_matched, res.n_rays_unmatched, res.n_no_return, res.sum_count = 3, 2, 1, 4, 5, 6, 4
    v = core.PaintValues(np.zeros((3, 3)), np.array([10, 0, 3 * ALL_ONES], dtype=np.uint64), np.array([4, 0, 3], dtype=np.uint32), res)
    m = v.mean()
    assert m.dtype == np.float64 and m[0] == 2.5 and math.isnan(m[1]) and m[2] == float(ALL_ONES)
    text = "\n".join(v.lines())
    for word in ("matched 4", "unmatched 5", "no return 6", "points: 3", "painted 2", "values added 4"):
        assert word in text, (word, text)
