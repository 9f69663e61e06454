"""The free-space carve, the parts that need no GPU: the march's geometry on the numpy restatement
(tests/helpers/map_carve_numpy.py) - no voxel recurs, every visited voxel is met by the segment -, the restatement's two forms against each
other, the host policy on the votes, the C-ABI surface with the refusals that come before any HIP call, and the moving-box scene on the
restatement alone: the conditions the definition has to meet there are shown without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from tests.helpers import map_carve_numpy as cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")
NEW = {"ptl_carve_sizeof_cfg", "ptl_carve_default_cfg", "ptl_carve_create", "ptl_carve_destroy", "ptl_carve_add_posed_range",
       "ptl_carve_add_posed_xyz", "ptl_carve_add_seq", "ptl_carve_add_batch", "ptl_carve_read"}
PTL_ERR_ARG = -1
VS = 0.5


def _rays():
    """(name, o, w, step): random rays, rays along voxel faces and lattice diagonals - dyadic coordinates at multiples of VS, negative ones
    and voxel 0 included"""
    rng = np.random.default_rng(24)
    out = []
    for i in range(40):
        o, w = rng.integers(-64, 65, 3) / 8.0, rng.integers(-64, 65, 3) / 8.0
        out.append((f"random dyadic {i}", o, w, VS / 2))
    for i in range(20):
        out.append((f"random {i}", rng.uniform(-9.0, 9.0, 3), rng.uniform(-9.0, 9.0, 3), rng.choice([VS, VS / 2, VS / 3, 0.07])))
    for axis in range(3):
        for sign in (1.0, -1.0):
            for face in (0.0, VS, -VS, 2 * VS, -3 * VS):
                o, w = np.array([face, face, face]), np.array([face, face, face])
                o[axis], w[axis] = -sign * 4.0, sign * 4.0  # (along an edge where three faces meet, through or beside voxel 0)
                out.append((f"face {axis} {sign} {face}", o, w, VS / 2))
                o2, w2 = o.copy(), w.copy()
                o2[(axis + 1) % 3] += VS / 4  # (in one face only)
                w2[(axis + 1) % 3] += VS / 4
                out.append((f"in-face {axis} {sign} {face}", o2, w2, VS))
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0, 0.0):
                dirn = np.array([sx, sy, sz])
                out.append((f"diagonal {dirn}", -3.0 * dirn, 3.0 * dirn, VS / 2))           # through the lattice points, the origin among them
                out.append((f"diagonal from 0 {dirn}", np.zeros(3), 4.0 * dirn, VS))
                out.append((f"diagonal off {dirn}", VS * np.array([1.0, 0.0, 0.0]) - 2.0 * dirn, VS * np.array([1.0, 0.0, 0.0]) + 2.5 * dirn, VS / 4))
    return out


def _voxel_box(key):
    """[lo, hi] of a voxel under the truncating index: index 0 spans (-VS, VS), every other index one VS"""
    lo = np.array([(k if k > 0 else k - 1) * VS for k in key], dtype=np.float64)
    hi = np.array([(k + 1 if k >= 0 else k) * VS for k in key], dtype=np.float64)
    return lo, hi


def test_no_voxel_recurs_after_it_has_been_left():
    n_multi = 0
    for name, o, w, step in _rays():
        keys = cv.march_keys([float(x) for x in o], [float(x) for x in w], VS, float(step))
        assert len(keys) >= 1, name
        assert len(set(keys)) == len(keys), (name, keys)
        n_multi += len(keys) > 3
    assert n_multi > 50, "the rays cross voxels"


def test_every_visited_voxel_is_met_by_the_segment_within_one_step():
    for name, o, w, step in _rays():
        o, w = np.asarray(o, dtype=np.float64), np.asarray(w, dtype=np.float64)
        keys, samples = cv.march_keys([float(x) for x in o], [float(x) for x in w], VS, float(step), with_samples=True)
        ln = float(np.linalg.norm(w - o))
        assert len(samples) == sum((k + 0.5) * step < ln for k in range(len(samples) + 1)) + 1, name
        assert samples[-1] == [float(x) for x in w], "the last sample is w itself"
        a = np.linspace(0.0, 1.0, max(2, int(16 * ln / step) + 2))[:, None]
        seg = o[None, :] + a * (w - o)[None, :]
        for key in keys:
            lo, hi = _voxel_box(key)
            gap = np.maximum(np.maximum(lo - seg, seg - hi), 0.0)
            dist = float(np.sqrt((gap * gap).sum(axis=1)).min())
            assert dist <= step, (name, key, dist, step)
        # and a step <= VS skips no voxel the centre line spends a whole step in: consecutive visited voxels are neighbours or the same
        for k0, k1 in zip(keys, keys[1:]):
            assert max(abs(a_ - b_) for a_, b_ in zip(k0, k1)) <= 1, (name, k0, k1)


def test_the_policy_function():
    from ptudes_lab_amd import core
    through = np.array([0, 1, 2, 2, 2, 3, 10, 5, 2**31], dtype=np.uint32)
    support = np.array([0, 0, 0, 2, 3, 100, 10, 6, 2**31], dtype=np.uint32)
    want = np.array([False, False, True, True, False, False, True, False, True])
    got = core.carve_dynamic(through, support)
    assert got.dtype == np.bool_ and (got == want).all()
    assert (cv.dynamic(through, support) == want).all()
    assert (core.carve_dynamic(through, support, min_through=1, min_fraction=0.0) == (through >= 1)).all()
    assert (core.carve_dynamic(through, support, min_through=3, min_fraction=1.0) == np.zeros(9, dtype=bool)).all()
    rng = np.random.default_rng(3)
    t, s = rng.integers(0, 9, 500).astype(np.uint32), rng.integers(0, 9, 500).astype(np.uint32)
    for mt, mf in ((2, 0.5), (1, 0.25), (4, 0.75)):
        assert (core.carve_dynamic(t, s, mt, mf) == cv.dynamic(t, s, mt, mf)).all()
    z = np.zeros((0, 3))
    v = core.CarveVotes(z, through[:0], support[:0], *([0] * 11), 0.05, 0.5, 0.25, 0.0, 60.0, 0.0)
    assert v.dynamic().shape == (0,) and len(v.lines()) == 4 and v.lines()[0].startswith("carve: radius 0.05 m")


def _random_scene(seed, n_sweeps=3, n_rays=60):
    rng = np.random.default_rng(seed)
    stored = rng.uniform(-3.0, 3.0, (400, 3))
    stored = np.vstack([stored, rng.integers(-12, 13, (200, 3)) / 4.0])  # (points on faces and lattice points)
    sweeps = []
    for _ in range(n_sweeps):
        o = np.tile(rng.uniform(-1.0, 1.0, 3), (n_rays, 1))
        hit = stored[rng.integers(0, len(stored), n_rays)] + rng.normal(0.0, 0.02, (n_rays, 3)) * (rng.random((n_rays, 1)) < 0.5)
        w = np.where(rng.random((n_rays, 1)) < 0.7, hit, o + (hit - o) * rng.uniform(1.0, 2.5, (n_rays, 1)))
        sweeps.append((o, w, rng.random(n_rays) < 0.9))
    sweeps.insert(1, None)
    return stored, sweeps


def test_the_two_forms_of_the_restatement_agree():
    for seed, cfg in ((1, dict(radius=0.05, margin=0.5, step=0.25, min_range=0.0, max_range=60.0)),
                      (2, dict(radius=0.2, margin=0.1, step=0.5, min_range=0.75, max_range=4.0)),
                      (3, dict(radius=0.01, margin=0.0, step=0.11, min_range=0.0, max_range=5.0))):
        stored, sweeps = _random_scene(seed)
        t0, s0, n0 = cv.carve_plain(stored, sweeps, VS, cfg)
        t1, s1, n1 = cv.carve(stored, sweeps, VS, cfg)
        assert n0 == n1, (seed, n0, n1)
        assert (t0 == t1).all() and (s0 == s1).all(), seed
        # (margin 0 leaves no room for support: t_p <= len is through already)
        assert n0["n_scans_skipped"] == 1 and n0["sum_through"] > 0 and (n0["sum_support"] > 0) == (cfg["margin"] > 0.0)
        assert n0["n_rays_out_of_range"] >= (seed == 2)


def test_hand_cases_on_both_forms_of_the_restatement():
    """the answers of tests/helpers/map_carve_cases.py, computed by hand: the GPU test holds the device to the same ones"""
    from tests.helpers import map_carve_cases as cc
    for case in cc.hand_cases():
        sweep = cc.case_rays(case)
        for form in (cv.carve_plain, cv.carve):
            t, s, n = form(case["stored"], [sweep], cc.VS, case["cfg"])
            got = np.column_stack([t, s]).astype(np.int64)
            assert (got == case["expect"]).all(), (case["name"], form.__name__, got.tolist())
            for k, v in case["counts"].items():
                assert n[k] == v, (case["name"], form.__name__, k, n[k], v)


def test_surface_and_refusals_before_any_hip_call():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[ \t]*(?:const\s+)?[A-Za-z_]\w*[\s\*]+(ptl_\w+)\s*\(", src, flags=re.M))
    assert NEW <= declared and NEW <= set(_lib.PROTOTYPES)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    L = _lib.lib()
    assert L.ptl_carve_sizeof_cfg() == C.sizeof(_lib.CarveCfg) == 48
    assert [L.ptl_sizeof_cfg(i) for i in range(6)] == [C.sizeof(t) for t in (_lib.IcpCfg, _lib.EkfCfg, _lib.SeqCfg, _lib.IcpStats, _lib.PktFormat,
                                                                             _lib.MapScoreCfg)] and L.ptl_sizeof_cfg(6) == -1
    cfg = _lib.CarveCfg()
    assert L.ptl_carve_default_cfg(C.byref(cfg), 0.5) == 0
    assert (cfg.radius, cfg.margin, cfg.step, cfg.min_range, cfg.max_range) == (0.5 / 10.0, 0.5, 0.25, 0.0, 60.0)
    assert cv.defaults(0.5) == dict(radius=cfg.radius, margin=cfg.margin, step=cfg.step, min_range=cfg.min_range, max_range=cfg.max_range)
    for size, abi in ((C.sizeof(_lib.CarveCfg) - 8, _lib.ABI_VERSION), (C.sizeof(_lib.CarveCfg), _lib.ABI_VERSION + 1)):
        bad = _lib.CarveCfg()
        bad.struct_size, bad.abi_version, bad.radius = size, abi, 123.0
        assert L.ptl_carve_default_cfg(C.byref(bad), 0.5) == PTL_ERR_ARG
        msg = L.ptl_last_error().decode()
        assert str(size) in msg and str(abi) in msg and "48" in msg, msg
        assert bad.radius == 123.0, "nothing is written on a mismatch"
    assert L.ptl_carve_default_cfg(None, 0.5) == PTL_ERR_ARG
    for vs in (0.0, -1.0, math.nan, math.inf):
        assert L.ptl_carve_default_cfg(C.byref(_lib.CarveCfg()), vs) == PTL_ERR_ARG
    assert L.ptl_carve_create(None, None, None) == PTL_ERR_ARG
    assert L.ptl_carve_read(None, None, None, None, None, 0, None) == PTL_ERR_ARG
    assert L.ptl_carve_destroy(None) == 0


def test_the_moving_box_scene_on_the_restatement_alone():
    """10 sweeps of 32 x 256; conditions: no static point is flagged, at least 90 % of the box's stored points are"""
    scene = cv.moving_box_scene()
    sweeps, box = cv.moving_box_rays(scene)
    world = np.vstack([w[ret] for _, w, ret in sweeps])
    stored = cv.first_points_per_voxel(world, cv.BOX_VS, cv.BOX_P)
    t, s, n = cv.carve(stored, sweeps, cv.BOX_VS, cv.BOX_CFG)
    is_box = cv.on_box_mask(stored, box)
    dyn = cv.dynamic(t, s, 2, 0.5)
    print(f"moving box: {int((dyn & is_box).sum())} of {int(is_box.sum())} box points flagged, {int((dyn & ~is_box).sum())} of "
          f"{int((~is_box).sum())} static points; counts {n}")
    assert n["n_scans"] == 10 and n["n_rays"] == 10 * 32 * 256 and n["n_no_return"] == 0
    assert is_box.sum() > 300
    assert (dyn & ~is_box).sum() == 0
    assert (dyn & is_box).sum() >= 0.9 * is_box.sum()
