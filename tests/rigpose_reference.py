"""NumPy restatement of the per-image target pose in a calibrated rig (include/pcs_hip.h pcs_rigpose_run, csrc/ba_rigpose.hpp), one
image at a time: the 6-parameter Levenberg-Marquardt over the detections of ALL cameras that see the image, every camera's extrinsics
and intrinsics fixed, with the trial sequence, damping policy, accept rule, stopping rules and status codes of the PnP's LM
(tests/pnp_reference.py ``lm_pose``).  Projection and Jacobian helpers are the PnP restatement's, imported, not copied.

Conventions: the unknown is T = (R, t), target -> world, as [rotvec, t]; ``ext`` (C, 3, 4) = [Re | te] world -> camera;
``intr`` (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2].  Residual of a detection (c, k): uv - project_c(Re (R X_k + t) + te).  Update
R <- exp([d omega]x) R, t <- t + d t, so d X_cam = Re (-[R X]x d omega + d t)."""
from __future__ import annotations

import numpy as np

from tests.pnp_reference import (CONVERGED, DEFAULTS, LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, MAX_ITER, NO_DECREASE, NOT_ESTIMATED, _ldl_solve, project,  # noqa: F401
                                 rodrigues, rotvec_of)


def project_in(dtype, R, t, X, cam9):
    """``pnp_reference.project`` with every array in ``dtype``.  The PnP restatement's routine returns its Jacobian in a float64 array,
    whatever the inputs; the extended-precision yardstick of the Hessian needs the same formulas carried in np.longdouble.  Rounded
    to float64 the two agree to a few units in the last place (tests/test_rigpose_reference.py)."""
    if dtype is np.float64:
        return project(R, t, X, cam9)
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = (dtype(v) for v in cam9)
    Y = X @ R.T + t
    iz = 1 / Y[:, 2]
    x, y = Y[:, 0] * iz, Y[:, 1] * iz
    r2 = x * x + y * y
    kup = 1 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3
    kd = k0 + 2 * k1 * r2 + 3 * k2 * r2 ** 2
    xD = x * kup + 2 * p0 * x * y + p1 * (r2 + 2 * x * x)
    yD = y * kup + p0 * (r2 + 2 * y * y) + 2 * p1 * x * y
    cross = 2 * x * y * kd + 2 * p0 * x + 2 * p1 * y
    dxx = kup + 2 * x * x * kd + 2 * p0 * y + 6 * p1 * x
    dyy = kup + 2 * y * y * kd + 6 * p0 * y + 2 * p1 * x
    ux, uy, vx, vy = fx * dxx, fx * cross, fy * cross, fy * dyy
    Jc = np.empty((X.shape[0], 2, 3), dtype=dtype)
    Jc[:, 0, 0], Jc[:, 0, 1], Jc[:, 0, 2] = ux * iz, uy * iz, -(ux * x + uy * y) * iz
    Jc[:, 1, 0], Jc[:, 1, 1], Jc[:, 1, 2] = vx * iz, vy * iz, -(vx * x + vy * y) * iz
    return np.stack([xD * fx + cx, yD * fy + cy], axis=1), Jc, Y


def image_residuals(pose, X, uv, cams, intr, ext, dtype=np.float64):
    """(n, 2) uv - projection of the template points X (n, 3) seen by the cameras ``cams`` (n,) under the image pose."""
    return _rows(rodrigues(np.asarray(pose[:3], dtype=np.float64)).astype(dtype), np.asarray(pose[3:], dtype=dtype), X, uv, cams, intr, ext, dtype)[0]


def _rows(R, t, X, uv, cams, intr, ext, dtype=np.float64):
    """Residuals (n, 2), Jacobian (2 n, 6) with respect to (d omega, d t) of the image pose, points not in front of their camera."""
    X, uv = np.asarray(X, dtype=dtype), np.asarray(uv, dtype=dtype)
    n = X.shape[0]
    Y = X @ R.T                      # R X: what the rotation increment turns
    Xw = Y + t
    r = np.empty((n, 2), dtype=dtype)
    J = np.empty((n, 2, 6), dtype=dtype)
    bad = 0
    for c in np.unique(cams):        # one camera at a time: the PnP restatement's projection at the "pose" (Re, te) of the camera
        sel = np.nonzero(cams == c)[0]
        Re, te = np.asarray(ext[c][:, :3], dtype=dtype), np.asarray(ext[c][:, 3], dtype=dtype)
        pix, Jc, Z = project_in(dtype, Re, te, Xw[sel], np.asarray(intr[c], dtype=dtype))
        r[sel] = uv[sel] - pix
        bad += int(np.sum(~(Z[:, 2] > 0)))
        for k in range(2):
            a = Jc[:, k, :] @ Re        # Re' a per row: d pixel / d X_world
            J[sel, k, :3] = np.cross(Y[sel], a)       # a . (-[R X]x e_j) = ((R X) x a)_j
            J[sel, k, 3:] = a
    return r, J.reshape(-1, 6), bad


def sums(pose_R, t, X, uv, cams, intr, ext, dtype=np.float64):
    """H = J'J (6 x 6), g = J'r, cost, number of points with depth <= 0 or non-finite (each behind ITS camera)."""
    r, J, bad = _rows(pose_R, t, X, uv, cams, intr, ext, dtype)
    return J.T @ J, J.T @ r.reshape(-1), float(np.sum(r * r)), bad


def hessian_at(pose, X, uv, cams, intr, ext, dtype=np.float64):
    """J'J at a pose vector, in ``dtype`` (np.longdouble: the yardstick of the device's Hessian)."""
    R = rodrigues(np.asarray(pose[:3], dtype=np.float64))
    if dtype is not np.float64:      # the rotation matrix itself in extended precision
        r = np.asarray(pose[:3], dtype=dtype)
        th2 = r @ r
        th = np.sqrt(th2)
        Kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dtype)
        if th2 < 1e-16:
            A, B = 1 - th2 / 6, dtype(0.5) - th2 / 24
        else:
            s, c = np.sin(th / 2), np.cos(th / 2)
            A, B = 2 * s * c / th, 2 * s * s / th2
        R = np.eye(3, dtype=dtype) + A * Kx + B * (np.outer(r, r) - th2 * np.eye(3, dtype=dtype))
    return sums(R.astype(dtype), np.asarray(pose[3:], dtype=dtype), X, uv, cams, intr, ext, dtype)[0]


def lm_image_pose(pose0, X, uv, cams, intr, ext, max_iter=10, ftol=1e-10, xtol=1e-10, gtol=0.0, margins=None):
    """The device's per-image LM from one start.  -> (pose, iterations, status, cost, cost at the start, H at the returned pose);
    status NOT_ESTIMATED (NaN pose) when the start is not finite or has a point behind its camera.  A pose that never moved is
    returned with the start's bits.  ``margins``: a list that receives, per trial, how far its decisions were from going the other
    way: |cost - trial cost| / cost (accept or reject) and, for an accepted trial, |(cost - trial cost) / cost - ftol| (flat or not)."""
    pose0 = np.asarray(pose0, dtype=np.float64)
    nanH = np.full((6, 6), np.nan)
    if not np.all(np.isfinite(pose0)):
        return np.full(6, np.nan), 0, NOT_ESTIMATED, np.nan, np.nan, nanH
    R, t = rodrigues(pose0[:3]), pose0[3:].copy()
    H, g, cost, bad = sums(R, t, X, uv, cams, intr, ext)
    cost0 = cost
    if not (np.isfinite(cost) and bad == 0):
        return np.full(6, np.nan), 0, NOT_ESTIMATED, np.nan, cost0, nanH
    lam, it, moved = LAMBDA0, 0, False

    def out(status):
        return (np.concatenate([rotvec_of(R), t]) if moved else pose0.copy()), it, status, cost, cost0, H

    while True:
        if np.max(np.abs(g)) <= gtol:
            return out(CONVERGED)
        if it >= max_iter:
            return out(MAX_ITER)
        d = _ldl_solve(H + lam * np.diag(np.diag(H)), g)
        if d is None:
            return out(NO_DECREASE)
        Rt, tt = rodrigues(d[:3]) @ R, t + d[3:]
        Ht, gt, ct, badt = sums(Rt, tt, X, uv, cams, intr, ext)
        it += 1
        small = np.sqrt(d @ d) <= xtol * (xtol + np.sqrt(3.0 + t @ t))   # the size of [R | t] (Frobenius)
        if margins is not None and badt == 0:
            margins.append(abs(cost - ct) / cost)
            if ct < cost:
                margins.append(abs((cost - ct) / cost - ftol))
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


def group_images(dct):
    """Rows of the (N, 5) table [cam, im, key, u, v] by image, inside an image by (camera, key): (sorted table, image ids, start)."""
    d = np.asarray(dct, dtype=np.float64)
    order = np.lexsort((d[:, 2], d[:, 0], d[:, 1]))
    d = d[order]
    ids, first = np.unique(d[:, 1].astype(np.int64), return_index=True)
    return d, ids, np.concatenate([first, [d.shape[0]]]).astype(np.int64)


class ImagePosesRef:
    pass


def localise_target(dct, points, intr, ext, poses_init, n_imgs=None, min_points=6, **opts):
    """The whole table through ``lm_image_pose`` from the starts ``poses_init`` (I, 6): an object with the fields of
    ``compiled_helpers.ImagePoses`` (``residuals`` in the order of the SORTED table, next to ``table``; ``margin`` (I,) the smallest
    decision margin of the image's trials, inf without a trial)."""
    d = np.asarray(dct, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    intr, ext = np.asarray(intr, dtype=np.float64), np.asarray(ext, dtype=np.float64)
    poses_init = np.asarray(poses_init, dtype=np.float64)
    I = poses_init.shape[0] if n_imgs is None else n_imgs
    o = dict(DEFAULTS)
    o.update(opts)
    out = ImagePosesRef()
    out.poses, out.poses_init = np.full((I, 6), np.nan), poses_init.copy()
    out.rms, out.rms_init = np.full(I, np.nan), np.full(I, np.nan)
    out.status, out.iterations, out.n_points, out.n_cams = (np.zeros(I, dtype=np.int32) for _ in range(4))
    out.hessian = np.full((I, 6, 6), np.nan)
    ds, ids, start = group_images(d)
    out.table, out.residuals = ds, np.full((ds.shape[0], 2), np.nan)
    out.margin = np.full(I, np.inf)
    for k, i in enumerate(ids):
        rows = ds[start[k]:start[k + 1]]
        n = rows.shape[0]
        cams, keys, uv = rows[:, 0].astype(np.int64), rows[:, 2].astype(np.int64), rows[:, 3:5]
        out.n_points[i], out.n_cams[i] = n, np.unique(cams).shape[0]
        if n < min_points:
            continue
        margins = []
        pose, it, st, cost, cost0, H = lm_image_pose(poses_init[i], points[keys], uv, cams, intr, ext, margins=margins, **o)
        out.margin[i] = min(margins, default=np.inf)
        if st == NOT_ESTIMATED:
            continue
        out.poses[i], out.iterations[i], out.status[i], out.hessian[i] = pose, it, st, H
        out.rms[i], out.rms_init[i] = np.sqrt(cost / n), np.sqrt(cost0 / n)
        out.residuals[start[k]:start[k + 1]] = image_residuals(pose, points[keys], uv, cams, intr, ext)
    return out


def start_from_views(dct, points, intr, ext, n_imgs, view_poses):
    """The start ``compiled_helpers.rig_pose_start`` takes, from given view poses (C, I, 6) (target -> camera): every camera's estimate
    W[c', i] = inv(E_c') M[c', i] of the image pose, scored by the summed reprojection error |r| over ALL detections of the image; the
    finite candidate of lowest error, ties to the lowest camera.  NaN where there is none."""
    from pycamset_amd.pose_seeding import pose_from_4x4, pose_to_4x4, rigid_inverse, to_4x4

    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    E = to_4x4(np.asarray(ext, dtype=np.float64))
    W = rigid_inverse(E)[:, None] @ pose_to_4x4(np.asarray(view_poses, dtype=np.float64))
    cand = pose_from_4x4(W)
    ds, ids, start = group_images(dct)
    out = np.full((n_imgs, 6), np.nan)
    for k, i in enumerate(ids):
        rows = ds[start[k]:start[k + 1]]
        cams, keys, uv = rows[:, 0].astype(np.int64), rows[:, 2].astype(np.int64), rows[:, 3:5]
        best = np.inf
        for c in range(cand.shape[0]):
            if not np.all(np.isfinite(cand[c, i])):
                continue
            with np.errstate(all="ignore"):
                r = image_residuals(cand[c, i], points[keys], uv, cams, intr, ext)
                err = float(np.sum(np.sqrt(np.sum(r * r, axis=1))))
            if np.isfinite(err) and err < best:
                best, out[i] = err, cand[c, i]
    return out
