"""The check of a handle's map score (`Icp.map_score(per_point=True)`) against tests/helpers/map_score_numpy.py run on `map_points()` of the
same handle, with the bounds tests/test_gpu_map_score.py derives in its docstring.  Shared by that file and tests/test_gpu_hash_tables.py."""
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps


def lex(p):
    p = np.asarray(p)
    return np.lexsort((p[:, 2], p[:, 1], p[:, 0]))


def bounds(P, radius, floor, h):
    atol_l = 8 * 27 * P * EPS * radius ** 2
    return atol_l, 1.5 * atol_l / floor ** 2 + 8 * EPS * np.maximum(1.0, np.abs(h))


def sorted_score(icp, **kw):
    s, (xyz, n, pv, ent) = icp.map_score(per_point=True, **kw)
    o = lex(xyz)
    return s, xyz[o], n[o], pv[o], ent[o]


def check(icp, P, radius=None, min_neighbours=5, sigma_floor=None, want_sparse=None):
    """the device's per-point values and summary of `icp`'s map against the restatement on map_points() of the same handle"""
    from tests.helpers import map_score_numpy as ms
    vs = float(icp.cfg.voxel_size)
    r = vs if radius is None else radius
    floor = vs / 100.0 if sigma_floor is None else sigma_floor
    size_before = icp.map_size()
    pts = icp.map_points()
    pts = pts[lex(pts)]
    s, xyz, n, pv, ent = sorted_score(icp, radius=radius, min_neighbours=min_neighbours, sigma_floor=sigma_floor)
    assert icp.map_size() == size_before and len(pts) == size_before[1] == s.n_points
    assert np.array_equal(xyz, pts), "every stored point, once, bit for bit"
    after = icp.map_points()
    assert np.array_equal(after[lex(after)], pts), "scoring does not touch the map"
    rn, rpv, rent, _ = ms.score_points(pts, r, min_neighbours, floor)
    assert np.array_equal(n, rn), f"{int((n != rn).sum())} neighbour counts differ"
    sparse = rn < min_neighbours
    assert np.array_equal(np.isnan(pv), sparse) and np.array_equal(np.isnan(ent), sparse)
    ok = ~sparse
    atol_l, atol_h = bounds(P, r, floor, rent[ok])
    d_l = np.abs(pv[ok] - rpv[ok]).max() if ok.any() else 0.0
    d_h = (np.abs(ent[ok] - rent[ok]) / atol_h).max() if ok.any() else 0.0
    print(f"{len(pts)} points, {int(ok.sum())} scored, neighbours {rn.min()} .. {rn.max()}: plane_var differs by {d_l:.3e} (bound {atol_l:.3e}), "
          f"entropy by {d_h:.3e} of its bound")
    assert d_l <= atol_l and d_h <= 1.0
    ref = ms.summary(rn, rpv, rent, min_neighbours)
    assert (s.n_points, s.n_scored, s.n_sparse) == (ref["n_points"], ref["n_scored"], ref["n_sparse"])
    assert (s.radius, s.min_neighbours, s.sigma_floor) == (r, min_neighbours, floor)
    assert s.mean_neighbours == pytest.approx(ref["mean_neighbours"], rel=4 * EPS)  # integers below 2^53: one division apart
    if ref["n_scored"]:
        k = ref["n_scored"]
        assert abs(s.mean_plane_var - ref["mean_plane_var"]) <= (k - 1) * EPS * ref["mean_plane_var"] + atol_l
        assert abs(s.mean_entropy - ref["mean_entropy"]) <= (k - 1) * EPS * np.abs(rent[ok]).sum() / k + atol_h.max()
    else:
        assert s.mean_plane_var == 0.0 and s.mean_entropy == 0.0
    if want_sparse is not None:
        assert (ref["n_sparse"] > 0) == want_sparse
    return s, ref
