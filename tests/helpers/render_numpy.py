"""The fly-by renderer (csrc/render_kernels.h) restated in numpy fp64 with the same operation order: splat with a depth test
into 64-bit keys, then resolve.  Input: the stored points in ANY order (Icp.map_points()) - a pixel's key is a minimum, so the order cannot
matter.  A camera is anything with view[12], fx, fy, cx, cy, near_m, far_m (_lib.RenderCam)."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def rgba_words(rgba):
    """(..., 4) uint8 R, G, B, A -> uint32 words, R the lowest byte"""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    return a.view("<u4").reshape(a.shape[:-1]).astype(np.uint32)


def default_palette_words():
    i = np.arange(256)
    return rgba_words(np.stack([i, 255 - np.abs(2 * i - 255), 255 - i, np.full(256, 255)], axis=1).astype(np.uint8))


def palette_index(z, z_lo, z_hi):
    zscale = 256.0 / (z_hi - z_lo)
    with np.errstate(invalid="ignore"):
        t = np.floor((np.asarray(z, dtype=np.float64) - z_lo) * zscale)
        return np.where(t >= 255.0, 255, np.where(t > 0.0, t, 0)).astype(np.int64)


def project(xyz, cam):
    """(zc, floor(u), floor(v), passed the depth test) per point, in the kernel's operation order"""
    v = np.array(cam.view[:], dtype=np.float64)
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xc = ((v[0] * x + v[1] * y) + v[2] * z) + v[3]
    yc = ((v[4] * x + v[5] * y) + v[6] * z) + v[7]
    zc = ((v[8] * x + v[9] * y) + v[10] * z) + v[11]
    with np.errstate(all="ignore"):
        ok = (zc > cam.near_m) & ~(zc >= cam.far_m)
        u = cam.fx * (xc / zc) + cam.cx
        w = cam.fy * (yc / zc) + cam.cy
        return zc, np.floor(u), np.floor(w), ok


def splat_into(keys, xyz, words, px, cam):
    """draws the points into keys (H, W) uint64 in place; returns the number of points in view"""
    H, W = keys.shape
    zc, fu, fv, ok = project(xyz, cam)
    with np.errstate(invalid="ignore"):
        ok = ok & (fu >= -8.0) & (fu < W + 8) & (fv >= -8.0) & (fv < H + 8)
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return 0
    half = (px - 1) // 2
    x0, y0 = fu[idx].astype(np.int64) - half, fv[idx].astype(np.int64) - half
    key = (zc[idx].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(words, dtype=np.uint32)[idx].astype(np.uint64)
    flat = keys.reshape(-1)
    seen = np.zeros(len(idx), dtype=bool)
    for dy in range(px):
        for dx in range(px):
            xx, yy = x0 + dx, y0 + dy
            m = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.minimum.at(flat, yy[m] * W + xx[m], key[m])
            seen |= m
    return int(seen.sum())


def resolve(keys, background_word=0xFF000000, edl_strength=0.0, edl_radius=1):
    """keys (H, W) -> (rgba (H, W, 4) uint8, depth (H, W) float32 with +inf for empty)"""
    H, W = keys.shape
    empty = keys == EMPTY
    words = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    if edl_strength > 0.0:
        with np.errstate(all="ignore"):
            l2 = np.log2(depth.astype(np.float64))
        total, n = np.zeros((H, W)), np.zeros((H, W), dtype=np.int64)
        r = int(edl_radius)
        for dx, dy in ((-r, 0), (r, 0), (0, -r), (0, r)):  # left, right, up, down: the kernel's order
            ys, xs = np.arange(H)[:, None] + dy, np.arange(W)[None, :] + dx
            inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
            yy, xx = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
            nb_ok = inside & ~empty[yy, xx]
            nb_l2 = l2[yy, xx]
            total = np.where(nb_ok, total + (l2 - nb_l2), total)
            n = n + nb_ok
        with np.errstate(all="ignore"):
            m = np.where(n > 0, total / np.maximum(n, 1), 0.0)
            s = np.exp(-edl_strength * np.where(m > 0.0, m, 0.0))
        out = words & np.uint32(0xFF000000)
        for ch in range(3):
            c = ((words >> np.uint32(8 * ch)) & np.uint32(0xFF)).astype(np.float64)
            with np.errstate(all="ignore"):
                cc = np.floor(c * s + 0.5)
            out = out | ((np.where(empty, 0.0, cc).astype(np.int64) & 0xFF).astype(np.uint32) << np.uint32(8 * ch))
        words = out
    words = np.where(empty, np.uint32(background_word), words).astype(np.uint32)
    depth[empty] = np.inf
    return np.ascontiguousarray(words).view(np.uint8).reshape(H, W, 4), depth


def render(points, cams, width, height, point_px=2, palette_words=None, z_range=(-2.0, 10.0), background_word=0xFF000000, edl_strength=0.0,
           edl_radius=1, overlay=None):
    """frames of the stored `points` (N, 3; None or empty: none) and the overlay (xyz (M, 3), words (M,), point_px) through cams:
    (keys (n, H, W) uint64, rgba (n, H, W, 4) uint8, depth (n, H, W) float32, in_view (n,) int64)"""
    pal = default_palette_words() if palette_words is None else np.asarray(palette_words, dtype=np.uint32)
    pts = np.zeros((0, 3)) if points is None else np.asarray(points, dtype=np.float64).reshape(-1, 3)
    words = pal[palette_index(pts[:, 2], z_range[0], z_range[1])]
    n = len(cams)
    keys = np.full((n, height, width), EMPTY, dtype=np.uint64)
    rgba = np.zeros((n, height, width, 4), dtype=np.uint8)
    depth = np.zeros((n, height, width), dtype=np.float32)
    in_view = np.zeros(n, dtype=np.int64)
    for f, cam in enumerate(cams):
        in_view[f] += splat_into(keys[f], pts, words, point_px, cam)
        if overlay is not None and len(overlay[0]):
            in_view[f] += splat_into(keys[f], overlay[0], overlay[1], overlay[2], cam)
        rgba[f], depth[f] = resolve(keys[f], background_word, edl_strength, edl_radius)
    return keys, rgba, depth, in_view
