"""NumPy restatement of the triangulation refinement (include/pcs_hip.h pcs_tri_refine, csrc/ba_tri_refine.hpp): the projection
model of the reference's Camera.project_points(distort=True) (cameras/camera.py:242-272, nb_distort_prealloc at :32-56), its
analytic 2 x 3 Jacobian, and the per-point Levenberg-Marquardt loop with the same acceptance and stopping rules."""
from __future__ import annotations

import numpy as np

NOT_REFINED, CONVERGED, MAX_ITER, NO_DECREASE = 0, 1, 2, 3
LAMBDA0, LAMBDA_MAX, LAMBDA_MIN = 1e-4, 1e10, 1e-15


def project(X, P, K, D):
    """pi(X) for one camera: h = P [X; 1], pinhole pixel (h0 / h2, h1 / h2), then the Brown-Conrady distortion with fx = K00,
    fy = K11, (cx, cy) = K[0:2, 2], D = [k0, k1, p0, p1, k2].  Returns (uv (2,), depth h2)."""
    h = P[:, :3] @ X + P[:, 3]
    a, b = h[0] / h[2], h[1] / h[2]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k0, k1, p0, p1, k2 = D
    x, y = (a - cx) / fx, (b - cy) / fy
    r2 = x * x + y * y
    kup = 1 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3
    xD = x * kup + 2 * p0 * x * y + p1 * (r2 + 2 * x * x)
    yD = y * kup + p0 * (r2 + 2 * y * y) + 2 * p1 * x * y
    return np.array([xD * fx + cx, yD * fy + cy]), h[2]


def jacobian(X, P, K, D):
    """d pi / d X (2 x 3), analytic."""
    h = P[:, :3] @ X + P[:, 3]
    a, b = h[0] / h[2], h[1] / h[2]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k0, k1, p0, p1, k2 = D
    x, y = (a - cx) / fx, (b - cy) / fy
    r2 = x * x + y * y
    kup = 1 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3
    kd = k0 + 2 * k1 * r2 + 3 * k2 * r2 ** 2
    cross = 2 * x * y * kd + 2 * p0 * x + 2 * p1 * y
    dxx = kup + 2 * x * x * kd + 2 * p0 * y + 6 * p1 * x
    dyy = kup + 2 * y * y * kd + 6 * p0 * y + 2 * p1 * x
    duv_dab = np.array([[dxx, fx * cross / fy], [fy * cross / fx, dyy]])
    dab_dX = np.stack([P[0, :3] - a * P[2, :3], P[1, :3] - b * P[2, :3]]) / h[2]
    return duv_dab @ dab_dX


def residuals(X, cams, uv, P, K, D):
    """(n_v, 2) uv - pi(X) and the depths (n_v,)."""
    out = np.empty((len(cams), 2))
    depth = np.empty(len(cams))
    for i, c in enumerate(cams):
        p, depth[i] = project(X, P[c], K[c], D[c])
        out[i] = uv[i] - p
    return out, depth


def _sums(X, cams, uv, P, K, D):
    r, depth = residuals(X, cams, uv, P, K, D)
    H, g = np.zeros((3, 3)), np.zeros(3)
    for i, c in enumerate(cams):
        J = jacobian(X, P[c], K[c], D[c])
        H += J.T @ J
        g += J.T @ r[i]
    return H, g, float(np.sum(r * r)), int(np.sum(~(depth > 0)))


def rms(X, cams, uv, P, K, D):
    r, _ = residuals(X, cams, uv, P, K, D)
    return float(np.sqrt(np.sum(r * r) / len(cams)))


def refine_point(X0, cams, uv, P, K, D, max_iter=10, ftol=1e-10, xtol=1e-10, gtol=0.0):
    """The device's per-point LM.  -> (X, iterations, status)."""
    X = np.asarray(X0, dtype=np.float64).copy()
    H, g, cost, bad = _sums(X, cams, uv, P, K, D)
    if not (np.all(np.isfinite(X)) and np.isfinite(cost) and bad == 0 and len(cams) > 0):
        return X, 0, NOT_REFINED
    lam, it = LAMBDA0, 0
    while True:
        if np.max(np.abs(g)) <= gtol:
            return X, it, CONVERGED
        if it >= max_iter:
            return X, it, MAX_ITER
        A = H + lam * np.diag(np.diag(H))
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return X, it, NO_DECREASE
        d = np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.all(np.isfinite(d)):
            return X, it, NO_DECREASE
        T = X + d
        Ht, gt, ct, badt = _sums(T, cams, uv, P, K, D)
        it += 1
        small = np.linalg.norm(d) <= xtol * (xtol + np.linalg.norm(X))
        if badt == 0 and ct < cost:
            flat = cost - ct <= ftol * cost
            X, H, g, cost = T, Ht, gt, ct
            lam = max(lam * 0.1, LAMBDA_MIN)
            if flat or small:
                return X, it, CONVERGED
        else:
            lam *= 10.0
            if small:
                return X, it, CONVERGED
            if lam > LAMBDA_MAX:
                return X, it, NO_DECREASE


def refine_all(pts_dlt, rec, start, P, K, D, **opts):
    """Every point of a grouped table (rows [cam, ..., u, v], start (n_pts + 1)).  -> (points, iterations, status)."""
    n = len(start) - 1
    out, its, st = np.empty((n, 3)), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for j in range(n):
        rows = rec[start[j]:start[j + 1]]
        out[j], its[j], st[j] = refine_point(pts_dlt[j], rows[:, 0].astype(int), rows[:, -2:], P, K, D, **opts)
    return out, its, st
