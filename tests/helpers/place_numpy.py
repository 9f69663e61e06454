"""The definition of the place descriptors and their comparison (include/ptudes_mi.h ptl_place_*) restated in numpy, with
the tables as an ARGUMENT: the tests hand it the tables the device uses, so that libm against numpy does not matter.  numpy's float64
elementwise arithmetic rounds every operation once and never contracts, which is the written order the definition asks for."""
import numpy as np

INFO_FIELDS = ("n_points", "n_no_return", "n_non_finite", "n_out_of_radius", "n_no_sector", "n_below", "n_used", "n_cells", "sum_levels")
DEFAULTS = dict(n_ring=20, n_sector=60, min_radius=1.0, max_radius=80.0, z_min=-2.0, z_step=0.0625)


def tables(n_ring, n_sector, min_radius, max_radius):
    """the tables as the definition words them, from numpy's cos / sin"""
    e = max_radius * np.arange(n_ring + 1, dtype=np.float64) / float(n_ring)
    edge2 = e * e
    edge2[0] = min_radius * min_radius
    t = 2.0 * np.pi * np.arange(n_sector, dtype=np.float64) / float(n_sector)
    return edge2, np.stack([np.cos(t), np.sin(t)], axis=1)


def r_pad(n_ring):
    return (n_ring + 3) // 4 * 4


def bins(points, edge2, sdir, z_min, z_step, rot=None, no_return=None):
    """per point (ring, sector, level, why): why 0 = used, else the index of the counter that took it (1 no return .. 5 below)"""
    p = np.asarray(points)
    p = p.astype(np.float64).reshape(-1, 3)  # (float32 input is converted first)
    n = len(p)
    R, S = len(edge2) - 1, len(sdir)
    why = np.zeros(n, dtype=np.int64)
    nor = (p == 0.0).all(axis=1) if no_return is None else np.asarray(no_return, dtype=bool)
    why[nor] = 1
    with np.errstate(all="ignore"):
        why[(why == 0) & ~np.isfinite(p).all(axis=1)] = 2
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        if rot is not None:
            r = np.asarray(rot, dtype=np.float64).reshape(9)
            x, y, z = ((r[0] * x + r[1] * y) + r[2] * z, (r[3] * x + r[4] * y) + r[5] * z, (r[6] * x + r[7] * y) + r[8] * z)
        rho2 = x * x + y * y
        inside = (edge2[0] <= rho2) & (rho2 < edge2[R])
        why[(why == 0) & ~inside] = 3
        ring = (edge2[None, :R] <= rho2[:, None]).sum(axis=1) - 1  # the largest i with edge2[i] <= rho2 (the edges increase)
        c = sdir[None, :, 0] * y[:, None] - sdir[None, :, 1] * x[:, None]  # (n, S)
        ok = (c >= 0.0) & (np.roll(c, -1, axis=1) < 0.0)
        sector = np.where(ok.any(axis=1), ok.argmax(axis=1), -1)  # the smallest such j
        why[(why == 0) & (sector < 0)] = 4
        h = (z - z_min) / z_step
        why[(why == 0) & ~(h >= 0.0)] = 5
        level = np.where(h >= 254.0, 255, 1 + np.where((h >= 0.0) & (h < 254.0), h, 0.0).astype(np.int64))
    return ring, sector, level, why


def describe(points, edge2, sdir, z_min, z_step, rot=None, no_return=None):
    """(desc (S, Rpad) uint8, info dict) of a set of points"""
    R, S = len(edge2) - 1, len(sdir)
    ring, sector, level, why = bins(points, edge2, sdir, z_min, z_step, rot, no_return)
    desc = np.zeros((S, r_pad(R)), dtype=np.uint8)
    use = why == 0
    np.maximum.at(desc, (sector[use], ring[use]), level[use].astype(np.uint8))
    info = dict(n_points=len(why), n_no_return=int((why == 1).sum()), n_non_finite=int((why == 2).sum()), n_out_of_radius=int((why == 3).sum()),
                n_no_sector=int((why == 4).sum()), n_below=int((why == 5).sum()), n_used=int(use.sum()), n_cells=int((desc != 0).sum()),
                sum_levels=int(desc.astype(np.int64).sum()))
    return desc, info


def info_row(info):
    return [info[k] for k in INFO_FIELDS]


def infos_of(descs):
    """(n, 9) int64 infos of descriptors made by hand: only n_cells and sum_levels are filled"""
    d = np.asarray(descs)
    out = np.zeros((len(d), len(INFO_FIELDS)), dtype=np.int64)
    out[:, INFO_FIELDS.index("n_cells")] = (d != 0).sum(axis=(1, 2))
    out[:, INFO_FIELDS.index("sum_levels")] = d.astype(np.int64).sum(axis=(1, 2))
    return out


def dists(q, c):
    """dist(q, c, s) for every s: (S,) int64"""
    q, c = np.asarray(q, dtype=np.int64), np.asarray(c, dtype=np.int64)
    return np.array([np.abs(np.roll(q, -s, axis=0) - c).sum() for s in range(len(q))], dtype=np.int64)


def best_shift(q, c):
    """(dist, shift): the smallest dist, ties to the smaller shift"""
    d = dists(q, c)
    s = int(d.argmin())
    return int(d[s]), s


def match(q, entries):
    """(dist (n,), shift (n,), best_entry or -1): ties between entries go to the smaller index"""
    got = [best_shift(q, c) for c in entries]
    dist = np.array([g[0] for g in got], dtype=np.uint32)
    shift = np.array([g[1] for g in got], dtype=np.int32)
    return dist, shift, (int(dist.argmin()) if len(got) else -1)


def pair_table(entries, full_rows=None):
    """(dist (n, n), shift (n, n)): [i, j] = best_shift(entries[i], entries[j]) - the same sums, a query against many entries per numpy call.
    full_rows: the queries whose whole row is wanted; every other row is filled up to j = i only (what `match_all` reads), -1 beyond"""
    e = np.asarray(entries).astype(np.int16)
    n, S = len(e), e.shape[1] if len(e) else 0
    dist, shift = np.full((n, n), -1, dtype=np.int64), np.full((n, n), -1, dtype=np.int64)
    for i in range(n):
        m = n if full_rows is None or i in full_rows else i + 1
        d = np.array([np.abs(np.roll(e[i], -s, axis=0)[None] - e[:m]).sum(axis=(1, 2), dtype=np.int64) for s in range(S)])  # (S, m)
        shift[i, :m] = d.argmin(axis=0)  # (the first minimum: the smaller shift)
        dist[i, :m] = d.min(axis=0)
    return dist, shift


def match_all(entries, min_gap, first=0, last=None, table=None):
    """(entry, dist, shift) per query i in [first, last]: the best over j <= i - min_gap, ties to the smaller j, then the smaller shift.
    table: `pair_table` of (at least) these entries, when the caller has it"""
    last = len(entries) - 1 if last is None else last
    td, ts = pair_table(entries) if table is None else table
    entry, dist, shift = [], [], []
    for i in range(first, last + 1):
        best = (-1, 0, 0)
        for j in range(0, i - min_gap + 1):
            if best[0] < 0 or td[i, j] < best[1]:
                best = (j, int(td[i, j]), int(ts[i, j]))
        entry.append(best[0]); dist.append(best[1]); shift.append(best[2])
    return np.array(entry, dtype=np.int32), np.array(dist, dtype=np.uint32), np.array(shift, dtype=np.int32)
