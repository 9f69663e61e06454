"""Colours per stored point in the fly-by renderer (include/ptudes_mi.h ptl_render_set_point_colors) against the numpy
restatement of the frame (tests/helpers/render_numpy.py `splat_into` / `resolve`) given the same words row by row: bit for bit, keys included.
The rows come from `core.Painter(map).values().xyz`: the pool order the words are taken in."""
import numpy as np
import pytest

from tests.helpers import render_numpy as rn
from tests.test_gpu_render import CAPS, H, W, Z_RANGE, _cams8, _identity_cam, _map, _renderer, _room

pytestmark = pytest.mark.gpu


def _core():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    return core


def _pool_xyz(m):
    p = _core().Painter(m)
    try:
        return p.values().xyz
    finally:
        p.close()


def _frames(xyz, words, cams, px, **kw):
    """(keys, rgba, depth, in_view) of the restatement with a word per row"""
    n = len(cams)
    keys = np.full((n, H, W), rn.EMPTY, dtype=np.uint64)
    rgba, depth, in_view = np.zeros((n, H, W, 4), dtype=np.uint8), np.zeros((n, H, W), dtype=np.float32), np.zeros(n, dtype=np.int64)
    for f, cam in enumerate(cams):
        in_view[f] = rn.splat_into(keys[f], xyz, words, px, cam)
        rgba[f], depth[f] = rn.resolve(keys[f], **kw)
    return keys, rgba, depth, in_view


def _same(got, want, what):
    rgba, depth, keys, in_view = got
    wkeys, wrgba, wdepth, win = want
    assert np.array_equal(keys, wkeys), f"{what}: {int((keys != wkeys).sum())} keys differ"
    assert np.array_equal(in_view, win) and rgba.tobytes() == wrgba.tobytes() and depth.tobytes() == wdepth.tobytes(), what


@pytest.fixture(scope="module")
def room():
    m = _map(_room())
    xyz = _pool_xyz(m)
    stored = m.map_points()
    assert 2500 < len(xyz) <= 3000 and np.array_equal(xyz[np.lexsort(xyz.T[::-1])], stored[np.lexsort(stored.T[::-1])])
    words = np.random.default_rng(21).integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    yield m, xyz, words
    m.close()


@pytest.mark.parametrize("px", [1, 3])
def test_frames_take_a_point_s_colour_from_its_word(room, px):
    m, xyz, words = room
    cams = [_cams8()[0], _cams8()[6]]  # two frames in one call
    r = _renderer(point_px=px)
    before = r.render(m, cams, depth=True, keys=True)
    _same(before, rn.render(xyz, cams, W, H, point_px=px, z_range=Z_RANGE), "palette frames before")
    r.set_point_colors(m, words)
    got = r.render(m, cams, depth=True, keys=True)
    _same(got, _frames(xyz, words, cams, px), f"words, point_px {px}")
    assert (got[3] > 0).all() and not np.array_equal(got[2], before[2]) and np.array_equal(got[1], before[1]), "other colours, the same depths"
    # (n, 4) uint8 colours are the same words
    r.set_point_colors(m, words.view(np.uint8).reshape(-1, 4))
    _same(r.render(m, cams, depth=True, keys=True), _frames(xyz, words, cams, px), "uint8 colours")
    # another handle with the same points draws palette frames; this one again after clearing, bit-equal to the frames before
    other = _map(_room())
    _same(r.render(other, cams, depth=True, keys=True), rn.render(other.map_points(), cams, W, H, point_px=px, z_range=Z_RANGE), "another handle")
    other.close()
    _same(r.render(m, cams, depth=True, keys=True), _frames(xyz, words, cams, px), "still set")
    r.clear_point_colors()
    after = r.render(m, cams, depth=True, keys=True)
    assert all(np.array_equal(a, b) for a, b in zip(after, before)), "palette frames before setting and after clearing are bit-equal"
    r.close()


def test_words_with_the_overlay_and_eye_dome_lighting(room):
    """everything else of the frame is unchanged: the overlay is drawn behind the map's points under the same depth test, the shade is the
    restatement's within its one 8-bit level (log2 / exp, as tests/test_gpu_render.py holds it)"""
    m, xyz, words = room
    cams = [_cams8()[6]]
    ov = np.array([[3.0, 3.0, 1.0], [6.0, 5.0, 2.0], [8.0, 2.0, 0.5]])
    ov_words = np.array([0xFF0000FF, 0xFF00FF00, 0xFFFF0000], dtype=np.uint32)
    r = _renderer(point_px=2, edl=0.7)
    r.set_overlay(ov, ov_words.view(np.uint8).reshape(-1, 4), point_px=3)
    r.set_point_colors(m, words)
    rgba, depth, keys, in_view = r.render(m, cams, depth=True, keys=True)
    wkeys = np.full((1, H, W), rn.EMPTY, dtype=np.uint64)
    n = rn.splat_into(wkeys[0], xyz, words, 2, cams[0]) + rn.splat_into(wkeys[0], ov, ov_words, 3, cams[0])
    wrgba, wdepth = rn.resolve(wkeys[0], edl_strength=0.7, edl_radius=1)
    assert np.array_equal(keys, wkeys) and in_view[0] == n and depth[0].tobytes() == wdepth.tobytes()
    assert np.abs(rgba[0].astype(np.int64) - wrgba.astype(np.int64)).max() <= 1 and (rgba[0][..., 3] == wrgba[..., 3]).all()
    r.close()


def test_two_points_at_one_pixel_and_one_depth_resolve_to_the_smaller_word():
    core = _core()
    pts = np.array([[0.0, 0.0, 2.0], [0.001, 0.0, 2.0], [0.0, 0.002, 2.0], [1.0, 0.5, 4.0]])  # three in pixel (48, 32) at zc = 2, one elsewhere
    m = _map(pts)
    xyz = _pool_xyz(m)
    assert len(xyz) == 4
    cam = _identity_cam()
    r = _renderer(point_px=1)
    first = int(np.flatnonzero((xyz == pts[0]).all(axis=1))[0])
    for small in (0x00000001, 0xFFFFFFFE):
        words = np.full(4, 0xFFFFFFFF, dtype=np.uint32)
        words[[i for i in range(4) if i != first]] = [0x80000000, 0x7FFFFFFF, 0x12345678]
        words[first] = small
        r.set_point_colors(m, words)
        rgba, depth, keys, in_view = r.render(m, [cam], depth=True, keys=True)
        _same((rgba, depth, keys, in_view), _frames(xyz, words, [cam], 1), f"word {small:#x}")
        three = words[(xyz[:, 2] == 2.0)]
        assert int(keys[0, 32, 48] & np.uint64(0xFFFFFFFF)) == int(three.min()) and depth[0, 32, 48] == np.float32(2.0) and in_view[0] == 4
    r.close(); m.close()


def test_refusals_and_a_map_that_grew():
    core = _core()
    pts = _room()[:300]
    m = _map(pts)
    n = m.map_size()[1]
    r = _renderer()
    cams = [_cams8()[0]]
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError) as e:
            r.set_point_colors(m, np.zeros(bad, dtype=np.uint32))
        assert str(bad) in str(e.value) and str(n) in str(e.value), str(e.value)
        # (a refused set leaves the palette)
        _same(r.render(m, cams, depth=True, keys=True), rn.render(m.map_points(), cams, W, H, z_range=Z_RANGE), "after a refusal")
    words = np.arange(n, dtype=np.uint32) | np.uint32(0xFF000000)
    r.set_point_colors(m, words)
    r.render(m, cams)
    m.map_add(np.array([[5.0, 4.0, 2.0], [5.2, 4.0, 2.0]]))
    grown = m.map_size()[1]
    assert grown > n
    with pytest.raises(RuntimeError) as e:
        r.render(m, cams)
    assert "libptudes_mi error -4:" in str(e.value) and str(grown) in str(e.value) and str(n) in str(e.value), str(e.value)
    # set again for the map as it is, or clear: both draw
    xyz = _pool_xyz(m)
    words = np.arange(grown, dtype=np.uint32) | np.uint32(0xFF000000)
    r.set_point_colors(m, words)
    _same(r.render(m, cams, depth=True, keys=True), _frames(xyz, words, cams, 2), "set again")
    m.map_add(np.array([[5.4, 4.0, 2.0]]))
    r.clear_point_colors()
    _same(r.render(m, cams, depth=True, keys=True), rn.render(m.map_points(), cams, W, H, z_range=Z_RANGE), "cleared")
    empty = _map()
    with pytest.raises(ValueError):
        r.set_point_colors(empty, np.zeros(3, dtype=np.uint32))
    r.set_point_colors(empty, np.zeros(0, dtype=np.uint32))  # (no colours: clears)
    for x in (r, m, empty):
        x.close()
