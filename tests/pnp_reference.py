"""NumPy restatement of the batched target-pose estimation (include/pcs_hip.h pcs_pnp_run, csrc/ba_pnp.hpp), one view at a time:
the undistortion that feeds the start, the linear start (planarity test on the scatter of the view's template points; homography
with h33 = 1 for planar views, 3 x 4 DLT with p34 = 1 otherwise; the second pose of the planar ambiguity), and the 6-parameter
Levenberg-Marquardt on the measured pixels with the damping policy, accept rule, stopping rules and status codes of the
triangulation refinement (tests/tri_refine_reference.py).

Conventions: ``cam9`` = [fx, cx, fy, cy, k0, k1, p0, p1, k2] (the engine's intrinsics slab row); a pose is [rotvec(3), t(3)] with
X_cam = R(rotvec) X_target + t and |rotvec| <= pi."""
from __future__ import annotations

import numpy as np

NOT_ESTIMATED, CONVERGED, MAX_ITER, NO_DECREASE = 0, 1, 2, 3
LAMBDA0, LAMBDA_MAX, LAMBDA_MIN = 1e-4, 1e10, 1e-15
PLANAR_RATIO = 1e-3   # OpenCV's rule for its iterative PnP start: planar when lambda_min / lambda_mid of the scatter is below this
DEFAULTS = {"max_iter": 10, "ftol": 1e-10, "xtol": 1e-10, "gtol": 0.0}


# ---- rotations ------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """exp([r]x) from the half angle: sin(th) = 2 s c, 1 - cos(th) = 2 s^2 (no cancellation at small angles)."""
    r = np.asarray(r, dtype=np.float64)
    th2 = float(r @ r)
    if th2 < 1e-16:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        s, c = np.sin(0.5 * th), np.cos(0.5 * th)
        A, B = 2.0 * s * c / th, 2.0 * s * s / th2
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    return np.eye(3) + A * K + B * (np.outer(r, r) - th2 * np.eye(3))


def rotvec_of(R):
    """Rotation matrix -> Rodrigues vector with |r| <= pi, through the quaternion (largest-pivot branch): finite at angle pi."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        S = 2.0 * np.sqrt(tr + 1.0)
        q = (0.25 * S, (R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S)
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        S = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = ((R[2, 1] - R[1, 2]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S)
    elif R[1, 1] >= R[2, 2]:
        S = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = ((R[0, 2] - R[2, 0]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S)
    else:
        S = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = ((R[1, 0] - R[0, 1]) / S, (R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S)
    w, v = q[0], np.array(q[1:])
    if w < 0.0:
        w, v = -w, -v
    n = np.sqrt(v @ v)
    k = 2.0 * np.arctan2(n, w) / n if n > 1e-150 else 2.0
    return k * v


def jacobi_eigh3(S, sweeps=8):
    """Cyclic Jacobi on a symmetric 3 x 3: (eigenvalues (3,), eigenvectors in the columns), unsorted — the device's routine."""
    A = np.array(S, dtype=np.float64)
    V = np.eye(3)
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p, q]
            if apq == 0.0 or not np.isfinite(apq):
                continue
            with np.errstate(over="ignore"):
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            if not np.isfinite(theta):
                t = 0.0
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            J = np.eye(3)
            J[p, p] = J[q, q] = c
            J[p, q], J[q, p] = s, -s
            A = J.T @ A @ J
            A[p, q] = A[q, p] = 0.0
            V = V @ J
    return np.diag(A).copy(), V


def nearest_rotation(M):
    """Polar factor M (M'M)^(-1/2) through the Jacobi eigenvectors of M'M, and the mean singular value."""
    lam, V = jacobi_eigh3(M.T @ M)
    sig = np.sqrt(lam)
    return M @ (V * (1.0 / sig)) @ V.T, float(np.sum(sig) / 3.0)


# ---- camera model ---------------------------------------------------------------------------------------------------------------
def undistort_normalised(uv, cam9):
    """Five fixed-point steps of the Brown-Conrady inverse (the triangulation's undistortion), in normalised image coordinates."""
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = cam9
    x0, y0 = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        k_inv = 1.0 / (1.0 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3)
        xD = 2.0 * p0 * x * y + p1 * (r2 + 2.0 * x * x)
        yD = p0 * (r2 + 2.0 * y * y) + 2.0 * p1 * x * y
        x, y = (x0 - xD) * k_inv, (y0 - yD) * k_inv
    return np.stack([x, y], axis=1)


def project(R, t, X, cam9):
    """Pixels (n, 2) of the template points X (n, 3) under the pose, d pixel / d X_cam (n, 2, 3), X_cam (n, 3)."""
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = cam9
    Y = X @ R.T + t
    iz = 1.0 / Y[:, 2]
    x, y = Y[:, 0] * iz, Y[:, 1] * iz
    r2 = x * x + y * y
    kup = 1.0 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3
    kd = k0 + 2.0 * k1 * r2 + 3.0 * k2 * r2 ** 2
    xD = x * kup + 2.0 * p0 * x * y + p1 * (r2 + 2.0 * x * x)
    yD = y * kup + p0 * (r2 + 2.0 * y * y) + 2.0 * p1 * x * y
    cross = 2.0 * x * y * kd + 2.0 * p0 * x + 2.0 * p1 * y
    dxx = kup + 2.0 * x * x * kd + 2.0 * p0 * y + 6.0 * p1 * x
    dyy = kup + 2.0 * y * y * kd + 6.0 * p0 * y + 2.0 * p1 * x
    ux, uy, vx, vy = fx * dxx, fx * cross, fy * cross, fy * dyy
    Jc = np.empty((X.shape[0], 2, 3))
    Jc[:, 0, 0], Jc[:, 0, 1], Jc[:, 0, 2] = ux * iz, uy * iz, -(ux * x + uy * y) * iz
    Jc[:, 1, 0], Jc[:, 1, 1], Jc[:, 1, 2] = vx * iz, vy * iz, -(vx * x + vy * y) * iz
    return np.stack([xD * fx + cx, yD * fy + cy], axis=1), Jc, Y


def residuals(pose, X, uv, cam9):
    """(n, 2) uv - pi(R X + t) of a pose vector."""
    return uv - project(rodrigues(pose[:3]), np.asarray(pose[3:], dtype=np.float64), X, cam9)[0]


def rms(pose, X, uv, cam9):
    r = residuals(pose, X, uv, cam9)
    return float(np.sqrt(np.sum(r * r) / X.shape[0]))


def jacobian(R, t, X, cam9):
    """d pixel / d (d omega, d t) (2 n, 6) for R <- exp(d omega) R, t <- t + d t: d X_cam = -[R X]x d omega + d t."""
    _, Jc, Y = project(R, t, X, cam9)
    Yr = Y - t
    J = np.empty((X.shape[0], 2, 6))
    for k in range(2):
        a = Jc[:, k, :]
        J[:, k, :3] = np.cross(Yr, a)     # a . (-[Yr]x e_j) = (Yr x a)_j
        J[:, k, 3:] = a
    return J.reshape(-1, 6)


def left_jacobian(r):
    """J_l(r) of SO(3): exp([d]x) R(r) = R(r + J_l(r)^-1 d) to first order, so d / d r = (d / d d) J_l(r)."""
    th2 = float(r @ r)
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    if th2 < 1e-12:
        return np.eye(3) + 0.5 * K + K @ K / 6.0
    th = np.sqrt(th2)
    return np.eye(3) + (1.0 - np.cos(th)) / th2 * K + (th - np.sin(th)) / (th2 * th) * (K @ K)


def _sums(R, t, X, uv, cam9):
    """H = J'J (6 x 6), g = J'r, cost, number of points with depth <= 0 or non-finite."""
    p, _, Y = project(R, t, X, cam9)
    r = uv - p
    J2 = jacobian(R, t, X, cam9)
    return J2.T @ J2, J2.T @ r.reshape(-1), float(np.sum(r * r)), int(np.sum(~(Y[:, 2] > 0)))


def _ldl_solve(A, b):
    """LDL' without pivoting; None when a pivot is not positive and finite or the solution is not finite."""
    n = A.shape[0]
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = A[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
        if not (D[j] > 0.0 and D[j] < np.inf):
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
    y = np.linalg.solve(L, b)
    x = np.linalg.solve(L.T, y / D)
    return x if np.all(np.isfinite(x)) else None


# ---- (b) the linear start ---------------------------------------------------------------------------------------------------------
def _fit_projective(q, xn):
    """Least squares of the projective map with its last element 1: q (n, d) -> xn (n, 2); unknowns [row 0 (d + 1), row 1 (d + 1),
    row 2 (d)], normal equations of size 3 d + 2 in the block form the device accumulates."""
    n, d = q.shape
    qt = np.concatenate([q, np.ones((n, 1))], axis=1)
    x, y = xn[:, 0], xn[:, 1]
    w = x * x + y * y
    A = qt.T @ qt
    B1, B2 = -(qt * x[:, None]).T @ q, -(qt * y[:, None]).T @ q
    C = (q * w[:, None]).T @ q
    m = d + 1
    N = np.zeros((3 * d + 2, 3 * d + 2))
    N[:m, :m] = N[m:2 * m, m:2 * m] = A
    N[:m, 2 * m:], N[m:2 * m, 2 * m:] = B1, B2
    N[2 * m:, :m], N[2 * m:, m:2 * m] = B1.T, B2.T
    N[2 * m:, 2 * m:] = C
    rhs = np.concatenate([qt.T @ x, qt.T @ y, -(q.T @ w)])
    return _ldl_solve(N, rhs)


def linear_start(keys, uv, cam9, points):
    """-> (pose (6,), alt (6,), planar): the start, the second pose of the planar ambiguity (NaN for a 3-D view), whether the view
    is planar.  NaN poses when the fit fails."""
    nan6 = np.full(6, np.nan)
    X = points[keys]
    n = X.shape[0]
    xn = undistort_normalised(uv, cam9)
    c = X.sum(axis=0) / n
    Q = X - c
    S = Q.T @ Q
    lam, E = jacobi_eigh3(S)
    # three distinct indices: the first minimum, then the first maximum of the other two.  Equal eigenvalues (an isotropic target,
    # such as the corners of a cube) are simply not planar.
    i_min = int(np.argmin(lam))
    a, b = (k for k in range(3) if k != i_min)
    i_max, i_mid = (a, b) if lam[a] >= lam[b] else (b, a)
    s = np.sqrt((lam[0] + lam[1] + lam[2]) / n)
    lam_mid = lam[i_mid]
    planar = bool(lam[i_min] < PLANAR_RATIO * lam_mid)
    with np.errstate(all="ignore"):
        if planar:
            e3, e1 = E[:, i_min], E[:, i_max]
            e2 = np.cross(e3, e1)
            h = _fit_projective(np.stack([Q @ e1, Q @ e2], axis=1) / s, xn)
            if h is None:
                return nan6, nan6.copy(), True
            c1, c2, c3 = np.array([h[0], h[3], h[6]]), np.array([h[1], h[4], h[7]]), np.array([h[2], h[5], 1.0])
            nrm = np.sqrt(0.5 * (c1 @ c1 + c2 @ c2))
            Rp, _ = nearest_rotation(np.stack([c1, c2, np.cross(c1, c2) / nrm], axis=1) / nrm)
            tp = (s / nrm) * c3
            R = Rp @ np.stack([e1, e2, e3], axis=0)
            v = tp / np.sqrt(tp @ tp)
            R2 = (2.0 * np.outer(v, v) - np.eye(3)) @ R @ (2.0 * np.outer(e3, e3) - np.eye(3))
            pose = np.concatenate([rotvec_of(R), tp - R @ c])
            alt = np.concatenate([rotvec_of(R2), tp - R2 @ c])
        else:
            p = _fit_projective(Q / s, xn)
            if p is None:
                return nan6, nan6.copy(), False
            M = np.array([p[0:3], p[4:7], p[8:11]])
            if not np.linalg.det(M) > 0.0:
                return nan6, nan6.copy(), False
            R, sig = nearest_rotation(M)
            tp = (s / sig) * np.array([p[3], p[7], 1.0])
            pose, alt = np.concatenate([rotvec_of(R), tp - R @ c]), nan6.copy()
    if not np.all(np.isfinite(pose)):
        return nan6, nan6.copy(), planar
    if not np.all(np.isfinite(alt)):
        alt = nan6.copy()
    return pose, alt, planar


# ---- (c) the LM -------------------------------------------------------------------------------------------------------------------
def lm_pose(pose0, X, uv, cam9, max_iter=10, ftol=1e-10, xtol=1e-10, gtol=0.0):
    """The device's per-view LM from one start.  -> (pose, iterations, status, cost, cost at the start); status NOT_ESTIMATED when the
    start is not finite or has a point behind the camera.  A pose that never moved is returned with the start's bits."""
    pose0 = np.asarray(pose0, dtype=np.float64)
    if not np.all(np.isfinite(pose0)):
        return np.full(6, np.nan), 0, NOT_ESTIMATED, np.nan, np.nan
    R, t = rodrigues(pose0[:3]), pose0[3:].copy()
    H, g, cost, bad = _sums(R, t, X, uv, cam9)
    cost0 = cost
    if not (np.isfinite(cost) and bad == 0):
        return np.full(6, np.nan), 0, NOT_ESTIMATED, np.nan, cost0
    lam, it, moved = LAMBDA0, 0, False

    def out(status):
        return (np.concatenate([rotvec_of(R), t]) if moved else pose0.copy()), it, status, cost, cost0

    while True:
        if np.max(np.abs(g)) <= gtol:
            return out(CONVERGED)
        if it >= max_iter:
            return out(MAX_ITER)
        d = _ldl_solve(H + lam * np.diag(np.diag(H)), g)
        if d is None:
            return out(NO_DECREASE)
        Rt, tt = rodrigues(d[:3]) @ R, t + d[3:]
        Ht, gt, ct, badt = _sums(Rt, tt, X, uv, cam9)
        it += 1
        small = np.sqrt(d @ d) <= xtol * (xtol + np.sqrt(3.0 + t @ t))   # the size of [R | t] (Frobenius)
        if badt == 0 and ct < cost:
            flat = cost - ct <= ftol * cost
            R, t, H, g, cost, moved = Rt, tt, Ht, gt, ct, True
            lam = max(lam * 0.1, LAMBDA_MIN)
            if flat or small:
                return out(CONVERGED)
        else:
            lam *= 10.0
            if small:
                return out(CONVERGED)
            if lam > LAMBDA_MAX:
                return out(NO_DECREASE)


def solve_view(keys, uv, cam9, points, min_points=6, start=None, alt=None, **opts):
    """One view: start (or the given ``start`` / ``alt``), LM from it, for a planar view with at least one trial allowed also LM from
    the second pose, the lower final cost kept.  -> dict(pose, pose_init, pose_alt, rms, rms_init, iterations, status, n)."""
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.shape[0]
    o = dict(DEFAULTS)
    o.update(opts)
    nan6 = np.full(6, np.nan)
    res = dict(pose=nan6, pose_init=nan6.copy(), pose_alt=nan6.copy(), rms=np.nan, rms_init=np.nan, iterations=0, status=NOT_ESTIMATED, n=n)
    if n < min_points or n == 0:
        return res
    if start is None:
        start, alt, _ = linear_start(keys, uv, cam9, points)
    res["pose_init"], res["pose_alt"] = np.array(start, dtype=np.float64), nan6.copy() if alt is None else np.array(alt, dtype=np.float64)
    X = points[keys]
    pose, it, st, cost, cost0 = lm_pose(res["pose_init"], X, uv, cam9, **o)
    if st == NOT_ESTIMATED:
        return res
    if o["max_iter"] > 0 and np.all(np.isfinite(res["pose_alt"])):
        p2, it2, st2, c2, _ = lm_pose(res["pose_alt"], X, uv, cam9, **o)
        if st2 != NOT_ESTIMATED and c2 < cost:
            pose, it, st, cost = p2, it2, st2, c2
    res.update(pose=pose, iterations=it, status=st, rms=float(np.sqrt(cost / n)), rms_init=float(np.sqrt(cost0 / n)))
    return res


def group_views(dct, n_imgs):
    """Rows of the (N, 5) table [cam, im, key, u, v] by view: (sorted table, view ids (cam * n_imgs + im), start (n_views + 1))."""
    d = np.asarray(dct, dtype=np.float64)
    vid = d[:, 0].astype(np.int64) * n_imgs + d[:, 1].astype(np.int64)
    order = np.argsort(vid, kind="stable")
    d, vid = d[order], vid[order]
    ids, first = np.unique(vid, return_index=True)
    return d, ids, np.concatenate([first, [d.shape[0]]]).astype(np.int64)


class ViewPosesRef:
    pass


def estimate_view_poses(dct, points, intr, n_cams=None, n_imgs=None, min_points=6, **opts):
    """The whole table through ``solve_view``: an object with the fields of ``compiled_helpers.ViewPoses``."""
    d = np.asarray(dct, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    intr = np.asarray(intr, dtype=np.float64)
    C = intr.shape[0] if n_cams is None else n_cams
    I = (int(d[:, 1].max()) + 1 if d.shape[0] else 0) if n_imgs is None else n_imgs
    out = ViewPosesRef()
    out.poses, out.poses_init, out.poses_alt = (np.full((C, I, 6), np.nan) for _ in range(3))
    out.rms, out.rms_init = np.full((C, I), np.nan), np.full((C, I), np.nan)
    out.status, out.iterations, out.n_points = (np.zeros((C, I), dtype=np.int32) for _ in range(3))
    ds, ids, start = group_views(d, I)
    for k, v in enumerate(ids):
        rows = ds[start[k]:start[k + 1]]
        c, i = divmod(int(v), I)
        r = solve_view(rows[:, 2].astype(np.int64), rows[:, 3:5], intr[c], points, min_points=min_points, **opts)
        out.poses[c, i], out.poses_init[c, i], out.poses_alt[c, i] = r["pose"], r["pose_init"], r["pose_alt"]
        out.rms[c, i], out.rms_init[c, i] = r["rms"], r["rms_init"]
        out.status[c, i], out.iterations[c, i], out.n_points[c, i] = r["status"], r["iterations"], r["n"]
    return out
