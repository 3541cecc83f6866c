"""NumPy restatement of the image-mapping kernels (pycamset_amd/csrc/ba_imagemap.hpp): what "correct" means for the device.

Every function takes ``dtype`` (np.float64 or np.longdouble) and does all of its arithmetic in it.  The statements are sequential in
everything that has an order (fixed-point steps, taps, rows before columns); they are vectorised over points and pixels only, which
have none.  Nothing here touches a device.

Conventions: a camera is a row ``intr`` = [fx, cx, fy, cy, k0, k1, p0, p1, k2]; ``ext`` is a (3, 4) world -> camera [R | t]; pixel
coordinates are (x, y) = (column, row) with the pixel centre at the integer; images are (H, W, C); maps are (2, Hd, Wd), plane 0 the
source x."""
from __future__ import annotations

import numpy as np

NEAREST, BILINEAR, BICUBIC = "nearest", "bilinear", "bicubic"
INTERPOLATIONS = (NEAREST, BILINEAR, BICUBIC)
CUBIC_A = -0.75


def _cam(intr, dtype):
    return [dtype(v) for v in np.asarray(intr, dtype=np.float64)]


def undistort_points(pts, intr, iters=5, dtype=np.float64):
    """nb_undistort_prealloc (optimisation/compiled_helpers.py:373-398) with ``iters`` fixed-point steps."""
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = _cam(intr, dtype)
    p = np.asarray(pts, dtype=dtype).reshape(-1, 2)
    x0, y0 = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        k_inv = 1 / (1 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2))
        xD = 2 * p0 * x * y + p1 * (r2 + 2 * (x * x))
        yD = p0 * (r2 + 2 * (y * y)) + 2 * p1 * x * y
        x, y = (x0 - xD) * k_inv, (y0 - yD) * k_inv
    return np.stack([x * fx + cx, y * fy + cy], axis=1)


def project(intr, V, X, dtype=np.float64):
    """The forward model as the engine evaluates it (csrc/ba_device.hpp eval_detection): rotate by V, divide by z, Brown-Conrady, K.
    X: (n, 3).  -> (u, v, z)."""
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = _cam(intr, dtype)
    V = np.asarray(V, dtype=dtype)
    X = np.asarray(X, dtype=dtype)
    x = V[0, 0] * X[:, 0] + V[0, 1] * X[:, 1] + V[0, 2] * X[:, 2]
    y = V[1, 0] * X[:, 0] + V[1, 1] * X[:, 1] + V[1, 2] * X[:, 2]
    z = V[2, 0] * X[:, 0] + V[2, 1] * X[:, 1] + V[2, 2] * X[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz = 1 / z
        a, b = x * iz, y * iz
        a2, b2, ab = a * a, b * b, a * b
        r2 = a2 + b2
        r4 = r2 * r2
        r6 = r4 * r2
        kup = 1 + k0 * r2 + k1 * r4 + k2 * r6
        xD = a * kup + 2 * p0 * ab + p1 * (r2 + 2 * a2)
        yD = b * kup + p0 * (r2 + 2 * b2) + 2 * p1 * ab
        return xD * fx + cx, yD * fy + cy, z


def distort_points(pts, intr, dtype=np.float64):
    """nb_distort (optimisation/compiled_helpers.py:463-490): ideal pixel -> detected pixel."""
    fx, cx, fy, cy = _cam(intr, dtype)[:4]
    p = np.asarray(pts, dtype=dtype).reshape(-1, 2)
    X = np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, np.ones(p.shape[0], dtype=dtype)], axis=1)
    u, v, _ = project(intr, np.eye(3), X, dtype)
    return np.stack([u, v], axis=1)


def pixel_rays(pts, intr, ext=None, normalised=False, world=False, distort=True, iters=5, dtype=np.float64):
    """vector_cam_points (utils/general_utils.py:432-454) behind nb_undistort_arr: the ray of every pixel, (n, 3)."""
    fx, cx, fy, cy = _cam(intr, dtype)[:4]
    p = np.asarray(pts, dtype=dtype).reshape(-1, 2)
    if distort:
        p = undistort_points(p, intr, iters, dtype)
    x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    z = np.ones_like(x)
    if normalised:
        inv = 1 / np.sqrt(x * x + y * y + 1)
        x, y, z = x * inv, y * inv, inv
    if world:
        E = np.asarray(ext, dtype=dtype)
        return np.stack([E[0, k] * x + E[1, k] * y + E[2, k] * z for k in range(3)], axis=1)   # R^T
    return np.stack([x, y, z], axis=1)


def pixel_grid(W, H):
    """(H * W, 2) pixel coordinates (x, y) in image order."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx.ravel(), yy.ravel()], axis=1)


def camera_position(ext, dtype=np.float64):
    E = np.asarray(ext, dtype=dtype)
    return np.array([-(E[0, k] * E[0, 3] + E[1, k] * E[1, 3] + E[2, k] * E[2, 3]) for k in range(3)], dtype=dtype)


def ray_map(intr, W, H, ext=None, normalised=False, world=False, distort=True, iters=5, depth=None, dtype=np.float64):
    """sensor_map / world_sensor_map: (H, W, 3).  With ``depth`` (H, W): position + ray * depth, NaN where the depth is not finite."""
    r = pixel_rays(pixel_grid(W, H), intr, ext, normalised, world, distort, iters, dtype)
    if depth is not None:
        d = np.asarray(depth).astype(dtype).reshape(-1)
        pos = camera_position(ext, dtype) if world else np.zeros(3, dtype=dtype)
        with np.errstate(invalid="ignore"):
            r = np.where(np.isfinite(d)[:, None], pos[None, :] + r * d[:, None], dtype(np.nan))
    return r.reshape(H, W, 3)


def build_maps(intr, Wd, Hd, R_new=None, K_new=None, dtype=np.float64):
    """cv2.initUndistortRectifyMap: (2, Hd, Wd); NaN where Z <= 0."""
    Kn = _cam(intr, dtype)[:4] if K_new is None else [dtype(v) for v in np.asarray(K_new, dtype=np.float64)]
    V = np.eye(3) if R_new is None else np.asarray(R_new, dtype=np.float64).T
    g = pixel_grid(Wd, Hd).astype(dtype)
    X = np.stack([(g[:, 0] - Kn[1]) / Kn[0], (g[:, 1] - Kn[3]) / Kn[2], np.ones(g.shape[0], dtype=dtype)], axis=1)
    u, v, z = project(intr, V, X, dtype)
    bad = ~(z > 0)
    u, v = np.where(bad, dtype(np.nan), u), np.where(bad, dtype(np.nan), v)
    return np.stack([u.reshape(Hd, Wd), v.reshape(Hd, Wd)])


def cubic_weights(t):
    """Keys' kernel, a = -0.75, for the taps at -1, 0, 1, 2 (cv2's interpolateCubic)."""
    A = t.dtype.type(CUBIC_A)
    w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
    w1 = ((A + 2) * t - (A + 3)) * t * t + 1
    w2 = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1
    return [w0, w1, w2, 1 - w0 - w1 - w2]


def _tap(src, x, y, border, dtype):
    """Values (n, C) of the taps and whether each lies inside."""
    Hs, Ws = src.shape[:2]
    inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
    val = np.broadcast_to(border, (x.shape[0], src.shape[2])).astype(dtype).copy()
    val[inside] = src[y[inside], x[inside]].astype(dtype)
    return val, inside


def border_value(border, C, img_dtype):
    """The border as a value of the image's own type, per channel."""
    b = np.zeros(C) if border is None else np.broadcast_to(np.asarray(border, dtype=np.float64), (C,))
    if np.dtype(img_dtype) == np.uint8:
        return np.clip(np.rint(np.nan_to_num(b, nan=0.0)), 0, 255)
    return b.astype(np.float32).astype(np.float64)


def remap(src, maps, interpolation=BILINEAR, border=None, dtype=np.float64):
    """cv2.remap with BORDER_CONSTANT on one image (Hs, Ws, C) of uint8 or float32.  -> dict(out (Hd, Wd, C) of the image's type, valid
    (Hd, Wd) uint8, raw (Hd, Wd, C) the unrounded values in ``dtype``)."""
    src = np.asarray(src)
    if src.ndim == 2:
        src = src[:, :, None]
    Hs, Ws, C = src.shape
    Hd, Wd = maps.shape[1:]
    sx, sy = np.asarray(maps[0], dtype=dtype).reshape(-1), np.asarray(maps[1], dtype=dtype).reshape(-1)
    bval = border_value(border, C, src.dtype).astype(dtype)
    n = sx.shape[0]
    ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(np.where(np.isfinite(sx), sx, 0)) < 2 ** 30) & (np.abs(np.where(np.isfinite(sy), sy, 0)) < 2 ** 30)
    sxs, sys_ = np.where(ok, sx, dtype(-10)), np.where(ok, sy, dtype(-10))   # a coordinate that is no number: no tap inside
    every, some = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    if interpolation == NEAREST:
        raw, inside = _tap(src, np.rint(sxs).astype(np.int64), np.rint(sys_).astype(np.int64), bval, dtype)
        every, some = inside.copy(), inside.copy()
    elif interpolation == BILINEAR:
        xf, yf = np.floor(sxs), np.floor(sys_)
        fx, fy = (sxs - xf)[:, None], (sys_ - yf)[:, None]
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        rows = []
        for j in range(2):
            t0, i0 = _tap(src, x0, y0 + j, bval, dtype)
            t1, i1 = _tap(src, x0 + 1, y0 + j, bval, dtype)
            every, some = every & i0 & i1, some | i0 | i1
            rows.append(t0 * (1 - fx) + t1 * fx)
        raw = rows[0] * (1 - fy) + rows[1] * fy
    elif interpolation == BICUBIC:
        xf, yf = np.floor(sxs), np.floor(sys_)
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        wx, wy = cubic_weights(sxs - xf), cubic_weights(sys_ - yf)
        raw = np.zeros((n, C), dtype=dtype)
        for j in range(4):
            row = np.zeros((n, C), dtype=dtype)
            for i in range(4):
                t, inside = _tap(src, x0 - 1 + i, y0 - 1 + j, bval, dtype)
                every, some = every & inside, some | inside
                row = row + wx[i][:, None] * t
            raw = raw + wy[j][:, None] * row
    else:
        raise ValueError(f"unknown interpolation {interpolation!r}")
    raw = np.where(some[:, None], raw, bval[None, :])
    if src.dtype == np.uint8:
        out = np.clip(np.rint(raw), 0, 255).astype(np.uint8)
    else:
        out = raw.astype(np.float64).astype(np.float32)
    return {"out": out.reshape(Hd, Wd, C), "valid": every.astype(np.uint8).reshape(Hd, Wd), "raw": raw.reshape(Hd, Wd, C), "some": some.reshape(Hd, Wd)}
