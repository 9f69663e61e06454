"""The occupancy grid, the parts that need no GPU: the restatement the GPU tests compare with
(tests/helpers/occupancy_grid_numpy.py) in its two forms against each other and against the answers written out by hand
(tests/helpers/occupancy_grid_cases.py), the host policy on its boundaries, the map files' round trip, the C-ABI surface of ptl_grid_* with its
layout and its refusals before any HIP call, the commands' refusals, and the moving-box scene on the restatement alone: the conditions the
definition has to meet there are shown without a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib
from tests.helpers import occupancy_grid_cases as gc
from tests.helpers import occupancy_grid_numpy as og
from tests.helpers.abi_surface import declared as _declared, exported as _exported, struct_fields as _header_fields

NEW = {"ptl_grid_sizeof_cfg", "ptl_grid_sizeof_result", "ptl_grid_default_cfg", "ptl_grid_create", "ptl_grid_destroy",
       "ptl_grid_add_posed_range", "ptl_grid_add_posed_xyz", "ptl_grid_add_seq", "ptl_grid_add_batch", "ptl_grid_read", "ptl_grid_clear"}
PTL_ERR_ARG = -1
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    assert a[2] == b[2], (what, a[2], b[2])


def _random_scene(seed, n_sweeps=3, n_rays=400, reach=9.0):
    """rays from moving origins inside and outside a 7 x 5 grid, ends on a lattice of eighths (cell edges and corners among them) or anywhere,
    some pixels without a return, some rays too long, a skipped sweep"""
    rng = np.random.default_rng(seed)
    sweeps = []
    for _ in range(n_sweeps):
        o = rng.uniform(-2.0, 8.0, (n_rays, 3)) * np.array([1.0, 1.0, 0.1])
        w = np.where(rng.random((n_rays, 1)) < 0.5, rng.integers(-16, 72, (n_rays, 3)) / 8.0, rng.uniform(-3.0, reach, (n_rays, 3)))
        w[:, 2] = o[:, 2] + rng.uniform(-1.5, 1.5, n_rays) * (rng.random(n_rays) < 0.7)
        far = rng.random(n_rays) < 0.03
        w[far] = o[far] + (w[far] - o[far]) * 40.0
        sweeps.append((o, w, rng.random(n_rays) < 0.9))
    sweeps.insert(1, None)
    return sweeps


def test_the_two_forms_of_the_restatement_agree():
    for seed, cfg in ((1, dict(cell=1.0, x0=0.0, y0=0.0, nx=7, ny=5, z_lo=-0.5, z_hi=0.5, margin=1.0, step=0.5, min_range=0.0, max_range=60.0)),
                      (2, dict(cell=0.5, x0=-1.25, y0=0.5, nx=9, ny=1, z_lo=-0.25, z_hi=1.0, margin=0.1, step=0.5, min_range=0.75, max_range=6.0)),
                      (3, dict(cell=0.75, x0=1.0, y0=-2.0, nx=1, ny=9, z_lo=0.0, z_hi=0.0, margin=0.0, step=0.11, min_range=0.0, max_range=9.0)),
                      (4, dict(cell=8.0, x0=-1.0, y0=-1.0, nx=1, ny=1, z_lo=-9.0, z_hi=9.0, margin=0.3, step=0.7, min_range=0.0, max_range=30.0))):
        sweeps = _random_scene(seed)
        a, b = og.grid_plain(sweeps, cfg), og.grid(sweeps, cfg)
        _same(a, b, seed)
        n = a[2]
        assert n["n_scans"] == 3 and n["n_scans_skipped"] == 1 and n["n_rays"] > 500 and n["n_no_return"] > 50 and n["n_rays_out_of_range"] > 5
        assert n["sum_free"] == n["n_runs_voted"] > 0 and n["n_ends_outside"] > 0
        assert n["sum_hit"] <= n["n_rays"] - n["n_ends_outside"]
        # the order of the sweeps and of the rays does not matter
        back = [None if s is None else tuple(x[::-1] for x in s) for s in sweeps[::-1]]
        _same(og.grid(back, cfg), b, (seed, "reversed"))


def test_the_lockstep_form_takes_a_scene_of_1e5_rays():
    """the array form is what the GPU tests use on 10^5 rays; a sample of its rays, marched one by one in Python floats, votes the same"""
    cfg = dict(cell=0.5, x0=-4.0, y0=-4.0, nx=64, ny=64, z_lo=-0.5, z_hi=0.5, margin=0.5, step=0.25, min_range=0.0, max_range=40.0)
    rng = np.random.default_rng(5)
    n = 100_000
    o = np.tile(rng.uniform(8.0, 16.0, 3) * np.array([1.0, 1.0, 0.05]), (n, 1))
    u = rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.05])
    w = o + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.1, 20.0, (n, 1))
    ret = rng.random(n) < 0.95
    free, hit, cnt = og.grid([(o, w, ret)], cfg)
    assert cnt["n_rays"] == int(ret.sum()) and cnt["sum_free"] > 10 * n and cnt["sum_hit"] > n // 2
    pick = rng.choice(n, 2000, replace=False)
    _same(og.grid([(o[pick], w[pick], ret[pick])], cfg), og.grid_plain([(o[pick], w[pick], ret[pick])], cfg), "a sample of the rays")
    # the counts of the whole are the sums of the counts of its parts
    half = n // 2
    fa, ha, _ = og.grid([(o[:half], w[:half], ret[:half])], cfg)
    fb, hb, _ = og.grid([(o[half:], w[half:], ret[half:])], cfg)
    assert np.array_equal(fa + fb, free) and np.array_equal(ha + hb, hit)


def test_hand_cases_on_both_forms_of_the_restatement():
    """the answers of tests/helpers/occupancy_grid_cases.py, written out by hand: the GPU test holds the device to the same ones"""
    cases = gc.hand_cases()
    assert len(cases) >= 14
    for case in cases:
        sweep = gc.case_rays(case)
        want_free, want_hit = gc.case_arrays(case)
        for form in (og.grid_plain, og.grid):
            free, hit, n = form([sweep], case["cfg"])
            assert np.array_equal(free, want_free), (case["name"], form.__name__, np.argwhere(free != want_free).tolist()[:8])
            assert np.array_equal(hit, want_hit), (case["name"], form.__name__, np.argwhere(hit != want_hit).tolist()[:8])
            for k, v in case["counts"].items():
                assert n[k] == v, (case["name"], form.__name__, k, n[k], v)


def test_classify_on_its_boundaries():
    from ptudes_lab_amd import core
    #                 unknown  free   1 hit  occupied  3 of 12: 0.25    2 of 9    free wins   hits only  large
    free = np.array([[0,       1,     0,     0,        9,               7,        100,        0,         2**31]], dtype=np.uint32)
    hit = np.array([[0,        0,     1,     2,        3,               2,        2,          5,         2**31]], dtype=np.uint32)
    want = np.array([[2,       0,     2,     1,        1,               0,        0,          1,         1]], dtype=np.uint8)
    got = core.grid_classify(free, hit)
    assert got.dtype == np.uint8 and got.shape == free.shape and np.array_equal(got, want)
    assert np.array_equal(og.classify(free, hit), want)
    assert (core.GRID_FREE, core.GRID_OCCUPIED, core.GRID_UNKNOWN) == (og.FREE, og.OCCUPIED, og.UNKNOWN) == (0, 1, 2)
    # min_hits = 0 makes a cell without any count occupied (0 >= 0 and 0 >= 0): the policy is taken literally
    assert core.grid_classify([0], [0], min_hits=0)[0] == core.GRID_OCCUPIED
    assert np.array_equal(core.grid_classify(free, hit, min_hits=3, min_fraction=0.5, min_free=2), [[2, 2, 2, 2, 0, 0, 0, 1, 1]])
    rng = np.random.default_rng(3)
    f, h = rng.integers(0, 9, (20, 30)).astype(np.uint32), rng.integers(0, 5, (20, 30)).astype(np.uint32)
    for mh, mf, mfree in ((2, 0.25, 1), (1, 0.5, 3), (4, 0.0, 1), (0, 1.0, 0)):
        assert np.array_equal(core.grid_classify(f, h, mh, mf, mfree), og.classify(f, h, mh, mf, mfree))
    res = _lib.GridResult()
    res.nx, res.ny, res.cell = 30, 20, 0.5
    counts = core.GridCounts(f, h, 0.5, (-1.0, 2.0), res)
    assert np.array_equal(counts.classify(), og.classify(f, h))
    lines = counts.lines()
    assert len(lines) == 4 and lines[0].startswith("grid: 30 x 20 cells of 0.5 m") and "untuned" in lines[3]
    cls = og.classify(f, h)
    assert f"free {int((cls == 0).sum())}, occupied {int((cls == 1).sum())}, unknown {int((cls == 2).sum())} of 600 cells read" in lines[3]


def test_map_files_round_trip(tmp_path):
    from ptudes_lab_amd import utils as pu
    rng = np.random.default_rng(9)
    classes = rng.integers(0, 3, (5, 7)).astype(np.uint8)
    classes[0, :3] = [1, 0, 2]  # the row of the SMALLEST y: the LAST row of the image
    origin = (-12.25, 3.5)
    for prefix in (str(tmp_path / "map"), str(tmp_path / "shot.png")):
        image, yaml = pu.save_occupancy_map(prefix, classes, 0.25, origin)
        assert os.path.basename(yaml) == ("map.yaml" if prefix.endswith("map") else "shot.yaml")
        text = open(yaml).read().splitlines()
        assert text == [f"image: {os.path.basename(image)}", "resolution: 0.25", "origin: [-12.25, 3.5, 0.0]", "negate: 0", "occupied_thresh: 0.65",
                        "free_thresh: 0.196"]
        back, cell, org = pu.load_occupancy_map(prefix)
        assert np.array_equal(back, classes) and back.dtype == np.uint8 and cell == 0.25 and org == origin
        assert np.array_equal(pu.load_occupancy_map(yaml)[0], classes)
        if image.endswith(".pgm"):
            data = open(image, "rb").read()
            assert data.startswith(b"P5\n7 5\n255\n") and len(data) == len(b"P5\n7 5\n255\n") + 35
            px = np.frombuffer(data[-35:], dtype=np.uint8).reshape(5, 7)
            assert px[4, :3].tolist() == [0, 254, 205] and np.array_equal(px[::-1], np.array([254, 0, 205], dtype=np.uint8)[classes])
        else:
            rgba = pu.load_png(image)
            assert rgba.shape == (5, 7, 4) and rgba[4, :3, 0].tolist() == [0, 254, 205] and (rgba[..., 3] == 255).all()
            assert np.array_equal(rgba[..., 0], rgba[..., 1]) and np.array_equal(rgba[..., 0], rgba[..., 2])
    # a cell size and an origin that are no short decimals come back to the bit
    pu.save_occupancy_map(str(tmp_path / "odd"), classes, 0.1 + 0.2, (1.0 / 3.0, -2.0 / 7.0))
    _, cell, org = pu.load_occupancy_map(str(tmp_path / "odd"))
    assert cell == 0.1 + 0.2 and org == (1.0 / 3.0, -2.0 / 7.0)
    for bad in (np.zeros((0, 3)), np.zeros(4), np.full((2, 2), 3)):
        with pytest.raises(ValueError):
            pu.save_occupancy_map(str(tmp_path / "bad"), bad, 0.25, origin)
    with pytest.raises(ValueError):
        pu.save_occupancy_map(str(tmp_path / "bad"), classes, 0.0, origin)


def test_surface_layout_and_refusals_before_any_hip_call():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= exported and NEW <= declared and declared == exported == set(_lib.PROTOTYPES)
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points and new structs change no existing struct or prototype
    assert [L.ptl_sizeof_cfg(i) for i in range(6)] == [C.sizeof(t) for t in (_lib.IcpCfg, _lib.EkfCfg, _lib.SeqCfg, _lib.IcpStats, _lib.PktFormat,
                                                                             _lib.MapScoreCfg)] and L.ptl_sizeof_cfg(6) == -1
    # header <-> binding, field by field
    for name, binding, size in (("ptl_grid_cfg", _lib.GridCfg, 104), ("ptl_grid_result", _lib.GridResult, 200)):
        want = [(f, CTYPES[t] if n is None else CTYPES[t] * n) for f, t, n in _header_fields(name)]
        assert [(f, t) for f, t in binding._fields_] == want, name
        assert C.sizeof(binding) == size and (binding().struct_size, binding().abi_version) == (size, 6)
    assert L.ptl_grid_sizeof_cfg() == 104 and L.ptl_grid_sizeof_result() == 200
    assert [f for f, _ in _lib.GridCfg._fields_] == ["struct_size", "abi_version", "cell", "x0", "y0", "z_lo", "z_hi", "margin", "step", "min_range",
                                                     "max_range", "max_pixels_per_scan", "nx", "ny", "scan_cols"]
    # the defaults
    cfg = _lib.GridCfg()
    assert L.ptl_grid_default_cfg(C.byref(cfg), 0.25) == 0
    assert (cfg.cell, cfg.step, cfg.margin, cfg.min_range, cfg.max_range, cfg.z_lo, cfg.z_hi) == (0.25, 0.125, 0.25, 0.0, 150.0, -0.5, 0.5)
    assert (cfg.x0, cfg.y0, cfg.nx, cfg.ny, cfg.scan_cols, cfg.max_pixels_per_scan) == (0.0, 0.0, 0, 0, 0, 0), "the bounds have no default"
    d = og.defaults(0.25)
    assert d == {k: getattr(cfg, k) for k in d}
    for size, abi in ((96, 6), (104, 7), (112, 6)):
        bad = _lib.GridCfg()
        bad.struct_size, bad.abi_version, bad.cell = size, abi, 123.0
        assert L.ptl_grid_default_cfg(C.byref(bad), 0.5) == PTL_ERR_ARG
        msg = L.ptl_last_error().decode()
        assert "ptl_grid_cfg" in msg and str(size) in msg and str(abi) in msg and "104" in msg, msg
        assert bad.cell == 123.0, "nothing is written on a mismatch"
        h = C.c_void_p()
        assert L.ptl_grid_create(0, C.byref(bad), C.byref(h)) == PTL_ERR_ARG and not h.value
    assert L.ptl_grid_default_cfg(None, 0.5) == PTL_ERR_ARG
    for cell in (0.0, -1.0, math.nan, math.inf):
        assert L.ptl_grid_default_cfg(C.byref(_lib.GridCfg()), cell) == PTL_ERR_ARG

    # a short, a long and a stale result struct are refused without a byte written: the struct sits in front of a canary.  The check of the
    # two leading words comes before the handle is looked at, so a block of zeros stands in for one
    class Guarded(C.Structure):
        _fields_ = [("res", _lib.GridResult), ("canary", C.c_uint8 * 32)]

    stand_in = (C.c_uint8 * 4096)()
    for size, abi in ((192, 6), (200, 5), (208, 6)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        g.res.struct_size, g.res.abi_version = size, abi
        before = bytes(g)
        rc = L.ptl_grid_read(C.cast(stand_in, C.c_void_p), C.cast(C.byref(g), C.POINTER(_lib.GridResult)), 0, 0, 0, 0, None, None)
        msg = L.ptl_last_error().decode()
        assert rc == PTL_ERR_ARG and "ptl_grid_result" in msg and str(size) in msg and str(abi) in msg and "200" in msg, msg
        assert bytes(g) == before, "nothing is written on a mismatch"
    assert bytes(stand_in) == bytes(4096)
    # one array of the two, and a rectangle outside the grid (the stand-in's grid is 0 x 0): refused before the device is looked for
    one = (C.c_uint32 * 4)()
    assert L.ptl_grid_read(C.cast(stand_in, C.c_void_p), C.byref(_lib.GridResult()), 0, 0, 1, 1, one, None) == PTL_ERR_ARG
    assert "1 given" in L.ptl_last_error().decode()
    assert L.ptl_grid_read(C.cast(stand_in, C.c_void_p), C.byref(_lib.GridResult()), 3, 4, 2, 1, one, one) == PTL_ERR_ARG
    assert "2 x 1 cells at (3, 4)" in L.ptl_last_error().decode() and "0 x 0" in L.ptl_last_error().decode()

    # each parameter bound of ptl_grid_create, with its numbers
    def create(**over):
        c = _lib.GridCfg()
        assert L.ptl_grid_default_cfg(C.byref(c), 0.5) == 0
        c.nx, c.ny, c.scan_cols, c.max_pixels_per_scan = 8, 4, 16, 64
        for k, v in over.items():
            setattr(c, k, v)
        h = C.c_void_p()
        rc = L.ptl_grid_create(0, C.byref(c), C.byref(h))
        assert not h.value or rc == 0
        if h.value:
            L.ptl_grid_destroy(h)
        return rc, L.ptl_last_error().decode()

    for over, words in ((dict(cell=0.0), ("cell", "0")), (dict(cell=math.nan), ("cell",)), (dict(x0=math.inf), ("x0", "inf")),
                        (dict(nx=0), ("nx x ny", "0 x 4")), (dict(ny=-1), ("8 x -1",)), (dict(nx=8193, ny=8192), ("8193 x 8192", "67117056", "67108864")),
                        (dict(z_lo=0.5, z_hi=0.25), ("z_lo", "0.5", "0.25")), (dict(z_lo=math.nan), ("z_lo",)), (dict(margin=-0.5), ("margin", "-0.5")),
                        (dict(step=0.0), ("step", "0")), (dict(step=0.75), ("step", "0.75", "0.5")), (dict(min_range=-1.0), ("min_range", "-1")),
                        (dict(min_range=3.0, max_range=3.0), ("max_range", "3")), (dict(step=0.25, max_range=16384.5), ("16384.5", "0.25", "65536")),
                        (dict(max_range=math.nan), ("max_range",)), (dict(scan_cols=0), ("scan_cols", "0")),
                        (dict(max_pixels_per_scan=15), ("max_pixels_per_scan", "15", "16")),
                        (dict(max_pixels_per_scan=(1 << 24) + 1), ("max_pixels_per_scan", str((1 << 24) + 1), str(1 << 24)))):
        rc, msg = create(**over)
        assert rc == PTL_ERR_ARG and "ptl_grid_create" in msg, (over, rc, msg)
        for w in words:
            assert w in msg, (over, w, msg)
    rc, msg = create()  # a cfg within every bound gets past the checks: a handle, or - without a device - the backend's refusal
    assert rc == 0 or (rc != PTL_ERR_ARG and "no HIP device 0" in msg), (rc, msg)
    rc, msg = create(nx=8192, ny=8192, step=0.25, max_range=16384.0) if rc != 0 else (rc, msg)  # (exactly 2^26 cells and 65536 samples are allowed)
    assert rc != PTL_ERR_ARG

    # null arguments
    assert L.ptl_grid_create(0, None, C.byref(C.c_void_p())) == PTL_ERR_ARG and "ptl_grid_create" in L.ptl_last_error().decode()
    assert L.ptl_grid_create(0, C.byref(_lib.GridCfg()), None) == PTL_ERR_ARG
    assert L.ptl_grid_read(None, C.byref(_lib.GridResult()), 0, 0, 0, 0, None, None) == PTL_ERR_ARG
    assert L.ptl_grid_read(C.cast(stand_in, C.c_void_p), None, 0, 0, 0, 0, None, None) == PTL_ERR_ARG
    assert L.ptl_grid_add_posed_range(None, None, None, None, None, None, None) == PTL_ERR_ARG and "ptl_grid_add_posed_range" in L.ptl_last_error().decode()
    assert L.ptl_grid_add_posed_xyz(None, None, None, 1, 1, None, None, None) == PTL_ERR_ARG and "ptl_grid_add_posed_xyz" in L.ptl_last_error().decode()
    assert L.ptl_grid_add_seq(None, None, None, None, 0, 0, None, None) == PTL_ERR_ARG and "ptl_grid_add_seq" in L.ptl_last_error().decode()
    assert L.ptl_grid_add_batch(None, None, 0, None, None, 0, 0, None, None) == PTL_ERR_ARG and "ptl_grid_add_batch" in L.ptl_last_error().decode()
    assert L.ptl_grid_clear(None) == PTL_ERR_ARG
    assert L.ptl_grid_destroy(None) == 0


def test_the_builder_s_bounds_and_its_refusal():
    from ptudes_lab_amd import fly
    pos = np.array([[0.1, -0.2, 1.0], [3.3, 2.6, 1.2], [1.0, 5.05, 0.9]])
    x0, y0, nx, ny = fly.grid_bounds(pos, 0.5, 10.0)
    assert (x0, y0, nx, ny) == (-10.0, -10.5, 47, 52)  # floor((0.1 - 10) / 0.5) = -20, ceil((3.3 + 10) / 0.5) = 27; floor(-10.2 / 0.5) = -21, ceil(15.05 / 0.5) = 31
    assert x0 <= pos[:, 0].min() - 10.0 and x0 + nx * 0.5 >= pos[:, 0].max() + 10.0 and y0 + ny * 0.5 >= pos[:, 1].max() + 10.0
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, 3] = pos
    # too many cells: refused with the count, naming --grid-bounds, before a device is asked for (600 cells of padding either side at the
    # default max_range: (1200 + 7)^2 cells fit, a trajectory 5 km long does not)
    far = poses[:2].copy()
    far[:, :3, 3] = [[0.0, 0.0, 0.0], [5000.0, 5000.0, 0.0]]
    for knots in (far, [(float(i), p) for i, p in enumerate(far)], far[:, :3, 3]):
        with pytest.raises(ValueError) as e:
            fly.GridBuilder((4, 16), knots, 0.5)
        assert "--grid-bounds" in str(e.value) and "11200 x 11200 = 125440000 cells" in str(e.value) and str(1 << 26) in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        fly.GridBuilder((4, 16), (0.0, 0.0, 5000.0, 5000.0), 0.5)
    assert "10000 x 10000 = 100000000 cells" in str(e.value)
    for bad in ((0.0, 0.0, 0.0, 1.0), (0.0, 2.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            fly.GridBuilder((4, 16), bad, 0.5)
    with pytest.raises(ValueError):
        fly.GridBuilder((4, 16), poses, 0.0)


def test_the_commands_refuse_before_a_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    poses = str(tmp_path / "p.csv")
    open(poses, "w").write("# no pose is read: the options are refused first\n")
    prefix = str(tmp_path / "g")
    fly_ = ["flyby", "--synthetic", "1000", "--nc-gt-poses", poses]
    bench = ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "1"]
    for base in (fly_, bench):
        for opt, val in (("--grid-cell", "0.5"), ("--grid-band", "-1,1"), ("--grid-margin", "0.5"), ("--grid-max-range", "30"),
                         ("--grid-bounds", "0,0,1,1"), ("--grid-min-hits", "3"), ("--grid-min-fraction", "0.5"), ("--save-grid-counts", "c.npz")):
            res = CliRunner().invoke(ptudes_cli, base + [opt, val])
            assert res.exit_code != 0 and f"{opt} belongs to --save-grid" in res.output, (opt, res.output)
        for extra, words in ((["--grid-cell", "0"], ("--grid-cell 0", "positive")), (["--grid-cell", "nan"], ("--grid-cell",)),
                             (["--grid-band", "1"], ("--grid-band 1", "LO,HI")), (["--grid-band", "a,b"], ("LO,HI",)),
                             (["--grid-band", "1,0.5"], ("LO must not be above HI",)), (["--grid-margin", "-1"], ("--grid-margin -1",)),
                             (["--grid-max-range", "0"], ("--grid-max-range 0",)),
                             (["--grid-cell", "0.5", "--grid-max-range", "16385"], ("--grid-max-range 16385", "16384")),
                             (["--grid-bounds", "0,0,1"], ("X0,Y0,X1,Y1",)), (["--grid-bounds", "0,0,0,1"], ("X1 must be above X0",)),
                             (["--grid-cell", "0.5", "--grid-bounds", "0,0,5000,5000"], ("10000 x 10000 = 100000000 cells", str(1 << 26))),
                             (["--grid-min-hits", "-1"], ("--grid-min-hits -1",)), (["--grid-min-fraction", "1.5"], ("--grid-min-fraction 1.5", "[0, 1]")),
                             (["--save-grid-counts", "c.txt"], (".npz",))):
            res = CliRunner().invoke(ptudes_cli, base + ["--save-grid", prefix] + extra)
            assert res.exit_code != 0, (extra, res.output)
            for w in words:
                assert w in res.output, (extra, w, res.output)
    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--kitti-poses", poses, "--save-grid", prefix])
    assert res.exit_code != 0 and "--save-grid with --kitti-poses" in res.output and "--nc-gt-poses" in res.output
    assert os.listdir(tmp_path) == ["p.csv"], "nothing was written"


# what the restatement gives on the moving-box scene, recorded here: the GPU test only has to show equality with the restatement
BOX_ORIGIN_CELLS, BOX_WALL_CELLS, BOX_TRAIL_CELLS = 6, 144, 26


def test_the_moving_box_scene_on_the_restatement_alone():
    """carve's moving-box scene, 10 sweeps of 32 x 256, with the default policy: every cell that holds a used column's origin is free; no wall
    cell of the room's outline at band height is free; the cells crossed only by the box's trail are free and not occupied"""
    from tests.helpers import map_carve_numpy as cv
    scene = cv.moving_box_scene()
    sweeps, _ = cv.moving_box_rays(scene)
    cfg = og.BOX_GRID
    free, hit, n = og.grid(sweeps, cfg)
    assert n["n_scans"] == 10 and n["n_rays"] == 10 * 32 * 256 and n["n_no_return"] == 0 and n["n_rays_out_of_range"] == 0 and n["n_ends_outside"] == 0
    cls = og.classify(free, hit)
    at = lambda cells: np.array([cls[iy, ix] for ix, iy in cells])  # noqa: E731
    origins = {og.cell_of(float(o[0, 0]), float(o[0, 1]), cfg) for o, _, _ in sweeps}
    walls = og.outline_cells(cfg)
    trail = og.box_trail_cells(scene, sweeps, cfg)
    assert None not in origins | walls | trail and not (trail & walls) and not (origins & walls)
    print(f"moving box: {len(origins)} origin cells, {len(walls)} wall cells of which {int((at(walls) == og.OCCUPIED).sum())} occupied, "
          f"{len(trail)} trail cells; classes free {int((cls == 0).sum())}, occupied {int((cls == 1).sum())}, unknown {int((cls == 2).sum())}; {n}")
    assert (len(origins), len(walls), len(trail)) == (BOX_ORIGIN_CELLS, BOX_WALL_CELLS, BOX_TRAIL_CELLS)
    assert (at(origins) == og.FREE).all()
    assert (at(walls) != og.FREE).all() and (at(walls) == og.OCCUPIED).sum() == BOX_WALL_CELLS
    assert (at(trail) == og.FREE).all(), "free and not occupied"
    assert all(hit[iy, ix] > 0 and free[iy, ix] > hit[iy, ix] for ix, iy in trail), "the box was seen there, and seen through more often"
