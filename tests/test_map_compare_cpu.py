"""The map distance, the parts that need no GPU: the C-ABI surface and its refusals before any HIP call, the numpy
restatement the GPU tests compare with (tests/helpers/map_compare_numpy.py) on answers computed by hand, the PLY with a per-point distance,
and the commands' option handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from ptudes_lab_amd import utils as pu
from tests.helpers import map_compare_numpy as mc
from tests.helpers.map_compare_cases import VS, hand_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")
NEW = {"ptl_map_cmp_sizeof_cfg", "ptl_map_cmp_default_cfg", "ptl_icp_map_distance", "ptl_icp_map_compare"}
PTL_ERR_ARG = -1


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"#define[^\n]*", " ", src)
    return set(re.findall(r"^[ \t]*(?:const\s+)?[A-Za-z_]\w*[\s\*]+(ptl_\w+)\s*\(", src, flags=re.M))


def _exported(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("nm (binutils) is needed to list the library's exported symbols")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptl_") and " T " in ln}


# ---------------------------------------------------------------------------------------------- 1. surface
def test_surface_of_the_map_distance():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= exported, "not exported"
    assert NEW <= declared, "not declared"
    assert declared == exported, "the header declares exactly what the library exports"
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert set(_lib.PROTOTYPES) == declared
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points and new structs change no existing struct or prototype
    assert L.ptl_sizeof_cfg(6) == -1                     # the new struct has a size function of its own
    assert L.ptl_map_cmp_sizeof_cfg() == C.sizeof(_lib.MapCmpCfg) == 88
    from ptudes_lab_amd import core, fly
    assert hasattr(core.Icp, "map_distance") and hasattr(core.Icp, "map_compare") and hasattr(core, "MapDistance")
    assert hasattr(core, "map_from_points") and hasattr(fly.MapAccumulator, "compare") and hasattr(fly, "MapComparison")

    # the defaults: a caller's choice echoed back, not tuned values
    cfg = _lib.MapCmpCfg()
    assert L.ptl_map_cmp_default_cfg(C.byref(cfg), 0.5) == 0
    assert (cfg.max_dist, cfg.n_thresholds, cfg.thresholds[0]) == (0.5, 1, 0.5) and list(cfg.thresholds[1:]) == [0.0] * 7
    assert (cfg.struct_size, cfg.abi_version) == (88, 6)

    # a short struct and a stale version are refused without a byte written: the struct sits in front of a canary
    class Guarded(C.Structure):
        _fields_ = [("cfg", _lib.MapCmpCfg), ("canary", C.c_uint8 * 32)]

    for size, abi in ((80, 6), (88, 5), (96, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.cfg.struct_size, g.cfg.abi_version = size, abi
        before = bytes(g)
        rc = L.ptl_map_cmp_default_cfg(C.cast(C.byref(g), C.POINTER(_lib.MapCmpCfg)), 0.5)
        msg = L.ptl_last_error().decode()
        assert rc == PTL_ERR_ARG and str(size) in msg and str(abi) in msg and "88" in msg, msg
        assert bytes(g) == before
    assert L.ptl_map_cmp_default_cfg(None, 0.5) == PTL_ERR_ARG
    cfg2 = _lib.MapCmpCfg()
    assert L.ptl_map_cmp_default_cfg(C.byref(cfg2), 0.0) == PTL_ERR_ARG and cfg2.max_dist == 0.0

    # no handle: refused before any HIP call (this machine may have no device at all)
    res = _lib.MapCmpResult()
    xyz = np.zeros((4, 3))
    assert L.ptl_icp_map_distance(None, C.byref(cfg), _lib.dptr(xyz), 4, C.byref(res), None) == PTL_ERR_ARG
    assert "null" in L.ptl_last_error().decode()
    assert L.ptl_icp_map_distance(None, None, None, 0, None, None) == PTL_ERR_ARG
    assert L.ptl_icp_map_compare(None, None, C.byref(cfg), C.byref(res), None, None, 0, None) == PTL_ERR_ARG
    assert "null" in L.ptl_last_error().decode()


# ---------------------------------------------------------------------------------------------- 2. known answers
def test_restatement_on_answers_computed_by_hand():
    ref, max_dist, cases = hand_cases()
    q = np.array([c[1] for c in cases])
    want = np.array([c[2] for c in cases])
    got = mc.dist2(q, ref, VS, max_dist)
    for (name, _, w), g in zip(cases, got):
        assert (np.isnan(g) and np.isnan(w)) or g == w, (name, g, w)
    # the pair one ulp beyond max_dist really is beyond it under the rounded expression, and the pair at max_dist is at it
    dx = np.nextafter(1.25, np.inf) - 1.0
    assert dx * dx > 0.25 * 0.25 and (1.25 - 1.0) ** 2 == 0.25 * 0.25
    thr = (0.125, 0.25)
    s = mc.summary(got, max_dist, thr)
    matched = want[np.isfinite(want)]
    assert (s["n_query"], s["n_invalid"], s["n_matched"]) == (len(cases), 2, len(matched)) and len(matched) == 4
    assert s["n_within"] == (1, 4)  # 0.125^2 = 0.015625: the face case alone; 0.25^2: every matched one
    assert s["sum_dist2"] == matched.sum() and s["max_dist2_seen"] == 0.0625
    assert abs(s["sum_dist"] - (0.25 + 0.125 + np.sqrt(0.046875) + 0.25)) <= 4 * np.finfo(float).eps
    # an empty reference: every finite query is unmatched; no queries: the zero summary
    e = mc.dist2(q, np.zeros((0, 3)), VS, max_dist)
    assert np.isinf(e[np.isfinite(q).all(axis=1)]).all() and np.isnan(e[~np.isfinite(q).all(axis=1)]).all()
    z = mc.summary(mc.dist2(np.zeros((0, 3)), ref, VS, max_dist), max_dist, thr)
    assert z == dict(n_query=0, n_invalid=0, n_matched=0, n_within=(0, 0), sum_dist=0.0, sum_dist2=0.0, max_dist2_seen=0.0)
    # precision / recall / F: 0 when both are 0
    a = dict(n_query=4, n_within=(0, 2))
    c = dict(n_query=8, n_within=(0, 8))
    assert mc.f_scores(a, c) == [(0.0, 0.0, 0.0), (0.5, 1.0, 2.0 * 0.5 / 1.5)]


def test_map_comparison_arithmetic():
    from ptudes_lab_amd import core, fly
    acc = core.MapDistance(4, 0, 3, (0, 2), 0.3, 0.05, 0.04, 0.5, (0.1, 0.2), 0.0)
    com = core.MapDistance(8, 1, 7, (0, 8), 0.7, 0.07, 0.04, 0.5, (0.1, 0.2), 0.0)
    cmp_ = fly.MapComparison(acc, com, "ref.ply", 8)
    assert cmp_.precision == (0.0, 0.5) and cmp_.recall == (0.0, 1.0) and cmp_.f_score == (0.0, 2.0 * 0.5 / 1.5)
    assert acc.mean_dist == 0.3 / 3 and acc.rms_dist == float(np.sqrt(0.05 / 3))
    empty = core.MapDistance(0, 0, 0, (0,), 0.0, 0.0, 0.0, 0.5, (0.5,), 0.0)
    assert empty.mean_dist == 0.0 and empty.rms_dist == 0.0 and empty.fractions == (0.0,)
    text = "\n".join(cmp_.lines())
    assert "ref.ply" in text and "8 points" in text and "precision 0.500000" in text and "recall 1.000000" in text and "mm" in text


# ---------------------------------------------------------------------------------------------- 3. the error map's file
def test_ply_with_a_distance_per_point(tmp_path):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(37, 3))
    dist = rng.uniform(0, 0.5, 37)
    dist[::5] = np.nan
    path = str(tmp_path / "err.ply")
    pu.save_map_ply(path, pts, {"dist": dist})
    assert pu.load_map_ply(path).tobytes() == pts.tobytes()
    back, extras = pu.load_map_ply(path, scalars=True)
    assert back.tobytes() == pts.tobytes() and list(extras) == ["dist"] and extras["dist"].tobytes() == dist.tobytes()
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert head[3:] == ["property double x", "property double y", "property double z", "property double dist", ""]
    with pytest.raises(ValueError, match="per point"):
        pu.save_map_ply(path, pts, {"dist": dist[:-1]})
    with pytest.raises(ValueError, match="PLY"):
        pu.save_map_ply(str(tmp_path / "err.npy"), pts, {"dist": dist})


# ---------------------------------------------------------------------------------------------- 4. option handling
def test_commands_refuse_compare_options_before_any_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    poses = tmp_path / "p.csv"
    poses.write_text("")
    ref = tmp_path / "ref.npy"
    np.save(str(ref), np.zeros((3, 3)))
    for cmd in (["flyby"], ["ekf-bench", "ouster"]):
        r = run(ptudes_cli, cmd + ["--help"])
        assert r.exit_code == 0
        for opt in ("--compare-map", "--compare-threshold", "--compare-max-dist", "--compare-pose", "--save-map-error"):
            assert opt in r.output, (cmd, opt)
    bad_pose = tmp_path / "bad_pose.txt"
    bad_pose.write_text("1 0 0 0 1 0 0 0 1\n")
    skew = tmp_path / "skew.txt"
    skew.write_text("2 0 0 0  0 1 0 0  0 0 1 0\n")
    for base in (["flyby", "--synthetic", "1", "--nc-gt-poses", str(poses)], ["ekf-bench", "ouster", "--synthetic", "1"]):
        for opt, val in (("--compare-threshold", "0.1"), ("--compare-max-dist", "0.2"), ("--compare-pose", str(bad_pose)),
                         ("--save-map-error", str(tmp_path / "e.ply"))):
            r = run(ptudes_cli, base + [opt, val])
            assert r.exit_code != 0 and f"{opt} belongs to --compare-map" in r.output, (base, opt, r.output)
        with_ref = base + ["--compare-map", str(ref)]
        r = run(ptudes_cli, base + ["--compare-map", str(tmp_path / "missing.ply")])
        assert r.exit_code != 0 and "no such file" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-max-dist", "0.75"])
        assert r.exit_code != 0 and "0.75" in r.output and "0.5" in r.output and "voxel size" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-max-dist", "0"])
        assert r.exit_code != 0 and "0 < max dist" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-threshold", "0.1,x"])
        assert r.exit_code != 0 and "0.1,x" in r.output and "numbers" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-threshold", "0.2,0.1"])
        assert r.exit_code != 0 and "ascending" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-threshold", "0.1,0.6"])
        assert r.exit_code != 0 and "0.6" in r.output and "max dist = 0.5" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-threshold", ",".join(["0.1"] * 9)])
        assert r.exit_code != 0 and "9 thresholds" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-pose", str(bad_pose)])
        assert r.exit_code != 0 and "9 numbers" in r.output and "12 or 16" in r.output
        r = run(ptudes_cli, with_ref + ["--compare-pose", str(skew)])
        assert r.exit_code != 0 and "not a rotation" in r.output
    r = run(ptudes_cli, ["flyby", "--synthetic", "1", "--nc-gt-poses", str(poses), "--voxel-size", "0.25", "--compare-map", str(ref),
                         "--compare-max-dist", "0.5"])
    assert r.exit_code != 0 and "0.5" in r.output and "0.25" in r.output
