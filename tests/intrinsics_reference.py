"""NumPy restatement of the intrinsics estimation from planar views (include/pcs_hip.h pcs_intr_run, csrc/ba_intrinsics.hpp), written
from Z. Zhang, "A flexible new technique for camera calibration" (PAMI 2000, section 3.1 with the skew fixed at zero) and from the
documented behaviour of OpenCV's initCameraMatrix2D (principal point at the image centre, two focal lengths by least squares).

Per (camera, image, board) group: the plane frame of the group's template points (centroid, cyclic-Jacobi eigenvectors of the
scatter, the PnP start's planarity rule), Hartley-normalised pixels, the homography with h33 = 1 from the 8 x 8 normal equations
(LDL' without pivoting), de-normalised to pixels <- metric plane frame.  Per camera: N H, the joint scaling of (h1, h2) by their root-mean-square length, the two
constraints per group on b = (B11, B22, B13, B23, B33), V'V, its smallest eigenvector by cyclic Jacobi (full model) or the 2 x 2
block for (1 / fx^2, 1 / fy^2) (focal model), the model selection and the status codes of the device.

``dtype=np.longdouble`` switches every step to extended precision: the difference between the two runs is the rounding sensitivity
of an input, which the device tests take as their yardstick."""
from __future__ import annotations

import numpy as np

NOT_ESTIMATED, FULL, FOCAL, FOCAL_FALLBACK = 0, 1, 2, 3
GROUP_TOO_FEW, GROUP_USED, GROUP_NOT_PLANAR, GROUP_NOT_FINITE, GROUP_FIT_FAILED = 0, 1, 2, 3, 4
PLANAR_RATIO = 1e-3
RANK_TOL = 1e-12
SWEEPS3, SWEEPS5 = 8, 12


def jacobi_eigh(S, sweeps, dtype=np.float64):
    """Cyclic Jacobi on a symmetric matrix: (eigenvalues, eigenvectors in the columns), unsorted — the device's routine, any size."""
    A = np.array(S, dtype=dtype)
    n = A.shape[0]
    V = np.eye(n, dtype=dtype)
    one = dtype(1.0)
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0.0 or not np.isfinite(apq):
                    continue
                with np.errstate(over="ignore"):
                    theta = (A[q, q] - A[p, p]) / (2 * apq)
                    t = (one if theta >= 0.0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                if not np.isfinite(theta):
                    t = dtype(0.0)
                c = one / np.sqrt(t * t + one)
                s = t * c
                J = np.eye(n, dtype=dtype)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
    return np.diag(A).copy(), V


def ldl_solve(A, b, dtype=np.float64):
    """LDL' without pivoting; None when a pivot is not positive and finite or the solution is not finite."""
    n = A.shape[0]
    L, D = np.eye(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for j in range(n):
        D[j] = A[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
        if not (D[j] > 0.0 and D[j] < np.inf):
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
    x = np.array(b, dtype=dtype)
    for i in range(n):
        x[i] = x[i] - np.sum(L[i, :i] * x[:i])
    x = x / D
    for i in range(n - 1, -1, -1):
        x[i] = x[i] - np.sum(L[i + 1:, i] * x[i + 1:])
    return x if np.all(np.isfinite(x)) else None


def fit_projective_plane(q, xn, dtype=np.float64):
    """The map q (n, 2) -> xn (n, 2) with its last element 1: unknowns [row 0 (3), row 1 (3), row 2 (2)], the 8 x 8 normal equations
    in the block form the device accumulates."""
    n = q.shape[0]
    qt = np.concatenate([q, np.ones((n, 1), dtype=dtype)], axis=1)
    x, y = xn[:, 0], xn[:, 1]
    w = x * x + y * y
    A = qt.T @ qt
    B1, B2 = -(qt * x[:, None]).T @ q, -(qt * y[:, None]).T @ q
    C = (q * w[:, None]).T @ q
    N = np.zeros((8, 8), dtype=dtype)
    N[:3, :3] = N[3:6, 3:6] = A
    N[:3, 6:], N[3:6, 6:] = B1, B2
    N[6:, :3], N[6:, 3:6] = B1.T, B2.T
    N[6:, 6:] = C
    return ldl_solve(N, np.concatenate([qt.T @ x, qt.T @ y, -(q.T @ w)]), dtype)


def group_homography(keys, uv, points, min_points=13, dtype=np.float64):
    """One group -> dict(status, H (3, 3) pixels <- metric plane frame, frame (9,) = [c, e1, e2], pix (3,) = pixel centroid and mean
    distance from it, n)."""
    nan = dtype(np.nan)
    out = dict(status=GROUP_USED, H=np.full((3, 3), nan, dtype=dtype), frame=np.full(9, nan, dtype=dtype), pix=np.full(3, nan, dtype=dtype), n=len(keys))
    n = len(keys)
    if n == 0 or n < min_points:
        out["status"] = GROUP_TOO_FEW
        return out
    X = np.asarray(points, dtype=dtype)[np.asarray(keys, dtype=np.int64)]
    m = np.asarray(uv, dtype=dtype)
    c = X.sum(axis=0) / n
    Q = X - c
    lam, E = jacobi_eigh(Q.T @ Q, SWEEPS3, dtype)
    i_min = int(np.argmin(lam))
    a, b = (k for k in range(3) if k != i_min)
    i_max, i_mid = (a, b) if lam[a] >= lam[b] else (b, a)
    s = np.sqrt((lam[0] + lam[1] + lam[2]) / n)
    with np.errstate(all="ignore"):
        mu = m.sum(axis=0) / n
        d = np.sum(np.sqrt(np.sum((m - mu) ** 2, axis=1))) / n
    out["pix"] = np.array([mu[0], mu[1], d], dtype=dtype)
    if not (np.all(np.isfinite(mu)) and d > 0.0 and d < np.inf):
        out["status"] = GROUP_NOT_FINITE
        return out
    if not lam[i_min] < dtype(PLANAR_RATIO) * lam[i_mid]:
        out["status"] = GROUP_NOT_PLANAR
        return out
    e3, e1 = E[:, i_min], E[:, i_max]
    e2 = np.cross(e3, e1)
    k = np.sqrt(dtype(2.0)) / d
    with np.errstate(all="ignore"):
        h = fit_projective_plane(np.stack([Q @ e1, Q @ e2], axis=1) / s, (m - mu) * k, dtype)
    H = None
    if h is not None:
        Hn = np.array([[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], 1.0]], dtype=dtype)
        Tinv = np.array([[1 / k, 0, mu[0]], [0, 1 / k, mu[1]], [0, 0, 1]], dtype=dtype)
        H = Tinv @ Hn @ np.diag(np.array([1 / s, 1 / s, 1], dtype=dtype))
    if H is None or not np.all(np.isfinite(H)):
        out["status"] = GROUP_FIT_FAILED
        return out
    out["H"], out["frame"] = H, np.concatenate([c, e1, e2])
    return out


def _constraint(a, c):
    return np.array([a[0] * c[0], a[1] * c[1], a[0] * c[2] + a[2] * c[0], a[1] * c[2] + a[2] * c[1], a[2] * c[2]])


def camera_closed_form(groups, res=None, model="full", dtype=np.float64):
    """The groups of ONE camera (dicts of ``group_homography``) -> (intr (9,), status, groups used, eigenvalue ratio).  ``res`` = (h, w)
    or None; ``model`` = "full" or "focal" ("auto" is resolved by the caller)."""
    nan = dtype(np.nan)
    used = [g for g in groups if g["status"] == GROUP_USED]
    row = np.full(9, nan, dtype=dtype)
    if not used:
        return row, NOT_ESTIMATED, 0, nan
    cnt = np.array([g["n"] for g in used], dtype=dtype)
    pix = np.stack([g["pix"] for g in used])
    if res is not None:
        rh, rw = dtype(res[0]), dtype(res[1])
        c0, sc = np.array([(rw - 1) / 2, (rh - 1) / 2], dtype=dtype), (rw + rh) / 2
    else:
        w = cnt.sum()
        c0, sc = (cnt[:, None] * pix[:, :2]).sum(axis=0) / w, (cnt * pix[:, 2]).sum() / w
    N = np.array([[1 / sc, 0, -c0[0] / sc], [0, 1 / sc, -c0[1] / sc], [0, 0, 1]], dtype=dtype)
    rows = []
    for g in used:
        Hn = N @ g["H"]
        h1, h2 = Hn[:, 0], Hn[:, 1]
        k = 1 / np.sqrt((h1 @ h1 + h2 @ h2) / 2)
        h1, h2 = h1 * k, h2 * k
        rows += [_constraint(h1, h2), (_constraint(h1, h1) - _constraint(h2, h2)) / 2]   # the half: see csrc/ba_intrinsics.hpp
    V = np.stack(rows).astype(dtype)
    M = V.T @ V
    lam, E = jacobi_eigh(M, SWEEPS5, dtype)
    order = np.argsort(lam, kind="stable")
    with np.errstate(all="ignore"):
        ratio = lam[order[0]] / lam[order[1]]
    if model == "full" and len(used) >= 2 and lam[order[1]] > dtype(RANK_TOL) * lam.max():
        B11, B22, B13, B23, B33 = E[:, order[0]]
        with np.errstate(all="ignore"):
            lm = B33 - B13 * B13 / B11 - B23 * B23 / B22
            if B11 * B22 > 0.0 and lm / B11 > 0.0:
                full = np.array([np.sqrt(lm / B11) * sc, -B13 / B11 * sc + c0[0], np.sqrt(lm / B22) * sc, -B23 / B22 * sc + c0[1]], dtype=dtype)
                if np.all(np.isfinite(full)):
                    row[:4], row[4:] = full, 0.0
                    return row, FULL, len(used), ratio
    with np.errstate(all="ignore"):
        det = M[0, 0] * M[1, 1] - M[0, 1] * M[0, 1]
        r0, r1 = -M[0, 4], -M[1, 4]
        ia, ib = (r0 * M[1, 1] - r1 * M[0, 1]) / det, (r1 * M[0, 0] - r0 * M[0, 1]) / det
        ok = det > dtype(RANK_TOL) * (M[0, 0] * M[1, 1]) and 0.0 < ia < np.inf and 0.0 < ib < np.inf
    if not ok:
        return row, NOT_ESTIMATED, len(used), ratio
    row[:4], row[4:] = [sc / np.sqrt(ia), c0[0], sc / np.sqrt(ib), c0[1]], 0.0
    return row, (FOCAL_FALLBACK if model == "full" else FOCAL), len(used), ratio


def group_rows(dct, n_imgs, board_of_key, n_boards):
    """Rows of the (N, 5) table [cam, im, key, u, v] by (camera, image, board) group, keys ascending inside a group:
    (sorted table, group index (n_groups, 3) = [cam, im, board], start (n_groups + 1))."""
    d = np.asarray(dct, dtype=np.float64)
    key = d[:, 2].astype(np.int64)
    gid = (d[:, 0].astype(np.int64) * n_imgs + d[:, 1].astype(np.int64)) * n_boards + np.asarray(board_of_key, dtype=np.int64)[key]
    order = np.lexsort((key, gid))
    d, gid = d[order], gid[order]
    ids, first = np.unique(gid, return_index=True)
    index = np.stack([ids // (n_imgs * n_boards), (ids // n_boards) % n_imgs, ids % n_boards], axis=1) if len(ids) else np.zeros((0, 3), dtype=np.int64)
    return d, index.astype(np.int64), np.concatenate([first, [d.shape[0]]]).astype(np.int64)


class IntrinsicsRef:
    pass


def estimate_intrinsics(dct, points, *, n_cams=None, n_imgs=None, board_of_key=None, res=None, model="auto", min_points=13, dtype=np.float64, **_):
    """The whole table: an object with the closed-form fields of ``compiled_helpers.IntrinsicsEstimate`` (``intr_init`` is ``intr``:
    the restatement has no refinement; options of the refinement are accepted and ignored)."""
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    C = (int(d[:, 0].max()) + 1 if d.shape[0] else 0) if n_cams is None else int(n_cams)
    I = (int(d[:, 1].max()) + 1 if d.shape[0] else 0) if n_imgs is None else int(n_imgs)
    bok = np.zeros(pts.shape[0], dtype=np.int64) if board_of_key is None else np.asarray(board_of_key, dtype=np.int64)
    nb = int(bok.max()) + 1 if bok.shape[0] else 1
    res_c = None if res is None else np.broadcast_to(np.asarray(res, dtype=np.float64), (C, 2))
    if model == "auto":
        model = "focal" if res is not None else "full"
    ds, index, start = group_rows(d, I, bok, nb)
    groups = [group_homography(ds[start[k]:start[k + 1], 2].astype(np.int64), ds[start[k]:start[k + 1], 3:5], pts, min_points, dtype)
              for k in range(len(index))]
    out = IntrinsicsRef()
    out.group_index = index
    out.group_status = np.array([g["status"] for g in groups], dtype=np.int32)
    out.group_counts = np.array([g["n"] for g in groups], dtype=np.int32)
    out.homographies = np.stack([g["H"] for g in groups]) if groups else np.zeros((0, 3, 3), dtype=dtype)
    out.plane_frames = np.stack([g["frame"] for g in groups]) if groups else np.zeros((0, 9), dtype=dtype)
    out.intr, out.status = np.full((C, 9), np.nan, dtype=dtype), np.zeros(C, dtype=np.int32)
    out.n_groups, out.eig_ratio = np.zeros(C, dtype=np.int32), np.full(C, np.nan, dtype=dtype)
    for c in range(C):
        mine = [g for g, ix in zip(groups, index) if ix[0] == c]
        out.intr[c], out.status[c], out.n_groups[c], out.eig_ratio[c] = camera_closed_form(mine, None if res_c is None else res_c[c], model, dtype)
    out.intr_init = out.intr
    return out


def plane_maps(homographies, frames):
    """(n, 3, 4): pixels <- template coordinates on each group's plane, H [e1'; e2'; 0] | H [-e1.c; -e2.c; 1], element (2, 3) = 1.
    Unlike the homography this does not depend on the choice of the in-plane axes."""
    H = np.asarray(homographies).reshape(-1, 3, 3)
    F = np.asarray(frames).reshape(-1, 9)
    out = np.empty((H.shape[0], 3, 4), dtype=H.dtype)
    for k in range(H.shape[0]):
        c, e1, e2 = F[k, :3], F[k, 3:6], F[k, 6:]
        T = np.zeros((3, 4), dtype=H.dtype)
        T[0, :3], T[1, :3] = e1, e2
        T[0, 3], T[1, 3], T[2, 3] = -(e1 @ c), -(e2 @ c), 1.0
        P = H[k] @ T
        out[k] = P / P[2, 3]
    return out
