"""The definition of a posed map's input, in numpy: sweeps + knots + column times -> world points in scan order.  TEST INFRASTRUCTURE
ONLY.  Built on oracle/dewarp.py's `poses_at` (the SE(3) geodesic between the bracketing knots, the end segments extended by the
bounds) and `dewarp` (every pixel with its column's pose):

* a sweep is (H, W, 3) sensor-frame points, (0, 0, 0) = no return; pixel order is row-major (row u, column v -> u W + v),
* column v of a sweep fires at col_ts[v]; with sweep times (t0, t1): t0 + (v / W)(t1 - t0),
* a sweep with ANY column outside [first knot - before, last knot + after] is skipped as a whole (reference utils.py:379-384),
* the result keeps the pixels with a return, in pixel order.
"""
import numpy as np

from oracle import dewarp as od
from oracle import lut as olut


def sweep_column_times(t0, t1, W):
    return t0 + (np.arange(W) / W) * (t1 - t0)


def posed_points(xyz_hw3, col_ts, knots, time_bounds=1.5):
    """world points (n, 3) of one sweep in scan order, or None when the sweep is skipped"""
    xyz = np.asarray(xyz_hw3, dtype=np.float64)
    try:
        poses = od.poses_at(knots, np.asarray(col_ts, dtype=np.float64), time_bounds=time_bounds)
    except ValueError:
        return None
    keep = np.any(xyz != 0.0, axis=2)
    return od.dewarp(xyz, poses)[keep]


def range_image_points(range_mm, alt_deg, az_deg):
    """(H, W, 3) sensor-frame points of a range image (mm) under the beam fan (alt, az), range 0 -> (0, 0, 0)"""
    H, W = range_mm.shape
    return olut.apply(*olut.xyz_lut(H, W, alt_deg, az_deg, 0.0, np.eye(4)), range_mm).reshape(H, W, 3)


def posed_map_input(sweeps, col_ts_list, knots, time_bounds=1.5):
    """per sweep: world points in scan order (skipped sweeps left out), and the number of skipped sweeps"""
    out, skipped = [], 0
    for xyz, ts in zip(sweeps, col_ts_list):
        p = posed_points(xyz, ts, knots, time_bounds)
        if p is None:
            skipped += 1
        else:
            out.append(p)
    return out, skipped
