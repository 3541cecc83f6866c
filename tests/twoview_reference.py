"""NumPy restatement of the two-view consensus (include/pcs_hip.h pcs_twoview_run, csrc/ba_twoview.hpp), one pair at a time and generic
in the dtype, so that it runs in float64 and in ``np.longdouble``: the five undistortion steps, the counter-based sampler (that of
``pnp_consensus_reference``), the normalised eight-point fit with its own cyclic Jacobi, the essential projection, the Sampson score,
the selection rules, the fit over the inliers, the four (R, +-t) and the cheirality count.

Sums run in row order here and in lane order on the device; everything else is the device's formula."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.pnp_consensus_reference import sample_positions

OK, TOO_FEW, DEGENERATE, NO_CHEIRALITY = 0, 1, 2, 3
SAMPLE, SWEEPS, RANK_RATIO = 8, 10, 1e-12
DEFAULTS = {"n_hypotheses": 64, "inlier_px": 2.0, "seed": 0, "min_points": 16}


def undistort(uv, cam9, dtype=np.float64):
    """Five fixed-point steps of the Brown-Conrady inverse, back to (undistorted) pixels."""
    fx, cx, fy, cy, k0, k1, p0, p1, k2 = (dtype(v) for v in cam9)
    uv = np.asarray(uv, dtype=dtype).reshape(-1, 2)
    x0, y0 = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        k_inv = 1 / (1 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2))
        xD = 2 * p0 * x * y + p1 * (r2 + 2 * (x * x))
        yD = p0 * (r2 + 2 * (y * y)) + 2 * p1 * x * y
        x, y = (x0 - xD) * k_inv, (y0 - yD) * k_inv
    return np.stack([x * fx + cx, y * fy + cy], axis=1)


def jacobi_eigh(S, sweeps, dtype=np.float64):
    """Cyclic Jacobi on a symmetric matrix, rotation by rotation as the device applies it: (eigenvalues, eigenvectors in the columns),
    unsorted."""
    A = np.array(S, dtype=dtype)
    n = A.shape[0]
    V = np.eye(n, dtype=dtype)
    one = dtype(1)
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq, app, aqq = A[p, q], A[p, p], A[q, q]
                if apq == 0 or not np.isfinite(apq):
                    continue
                with np.errstate(over="ignore"):
                    theta = (aqq - app) / (2 * apq)
                    t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                if not np.isfinite(theta):
                    t = dtype(0)
                c = one / np.sqrt(t * t + one)
                s = t * c
                cp, cq = A[:, p].copy(), A[:, q].copy()      # A J
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                rp, rq = A[p, :].copy(), A[q, :].copy()      # J' (A J)
                A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                A[p, p], A[q, q] = app - t * apq, aqq + t * apq
                A[p, q] = A[q, p] = 0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(A).copy(), V


def affine(p, q, u, v, dtype):
    return np.array([[p, 0, u], [0, q, v], [0, 0, 1]], dtype=dtype)


def inverse_pinhole(cam9, dtype):
    fx, cx, fy, cy = (dtype(v) for v in cam9[:4])
    return affine(1 / fx, 1 / fy, -cx / fx, -cy / fy, dtype)


def sampson(F, und):
    """Sampson distance of the rows (xa, ya, xb, yb) in undistorted pixels."""
    xa, ya, xb, yb = und[:, 0], und[:, 1], und[:, 2], und[:, 3]
    l0, l1, l2 = F[0, 0] * xa + F[0, 1] * ya + F[0, 2], F[1, 0] * xa + F[1, 1] * ya + F[1, 2], F[2, 0] * xa + F[2, 1] * ya + F[2, 2]
    r0, r1 = F[0, 0] * xb + F[1, 0] * yb + F[2, 0], F[0, 1] * xb + F[1, 1] * yb + F[2, 1]
    num = xb * l0 + yb * l1 + l2
    with np.errstate(all="ignore"):
        return num * num / (l0 * l0 + l1 * l1 + r0 * r0 + r1 * r1)


@dataclass
class Fit:
    ok: bool
    E0: np.ndarray
    E: np.ndarray
    v1: np.ndarray
    v2: np.ndarray
    s1: float
    s2: float


def eight_point(und, cam_a, cam_b, dtype=np.float64):
    """The normalised eight-point fit of the rows and its projection onto the essential manifold."""
    fxa, cxa, fya, cya = (dtype(v) for v in cam_a[:4])
    fxb, cxb, fyb, cyb = (dtype(v) for v in cam_b[:4])
    with np.errstate(all="ignore"):
        xa, ya, xb, yb = und[:, 0] - cxa, und[:, 1] - cya, und[:, 2] - cxb, und[:, 3] - cyb
        inv_n = 1 / dtype(und.shape[0])
        mxa, mya, mxb, myb = np.sum(xa) * inv_n, np.sum(ya) * inv_n, np.sum(xb) * inv_n, np.sum(yb) * inv_n
        sa = np.sqrt(2 / (np.sum(xa * xa + ya * ya) * inv_n - (mxa * mxa + mya * mya)))
        sb = np.sqrt(2 / (np.sum(xb * xb + yb * yb) * inv_n - (mxb * mxb + myb * myb)))
        xa, ya, xb, yb = sa * (xa - mxa), sa * (ya - mya), sb * (xb - mxb), sb * (yb - myb)
        rows = np.stack([xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, np.ones_like(xa)], axis=1)
        M = rows.T @ rows
        d, V = jacobi_eigh(M, SWEEPS, dtype)
        jmin = int(np.argmin(d)) if np.all(np.isfinite(d)) else 0
        dmax = np.max(d)
        dsec = np.min(np.delete(d, jmin))
        f = V[:, jmin]
        ok = bool(dmax > 0 and dsec > dtype(RANK_RATIO) * dmax and np.all(np.isfinite(f)))
        Na, Nb = affine(sa * fxa, sa * fya, -sa * mxa, -sa * mya, dtype), affine(sb * fxb, sb * fyb, -sb * mxb, -sb * myb, dtype)
        E0 = Nb.T @ f.reshape(3, 3) @ Na
        e, W = jacobi_eigh(E0.T @ E0, 8, dtype)
        k3 = 0 if e[0] <= e[1] and e[0] <= e[2] else (1 if e[1] <= e[2] else 2)
        sg = np.sqrt(np.maximum(e, 0))
        s1, s2 = (sg[1] if k3 == 0 else sg[0]), (sg[1] if k3 == 2 else sg[2])
        v1, v2 = W[:, 1 if k3 == 0 else 0].copy(), W[:, 1 if k3 == 2 else 2].copy()
        sm = (s1 + s2) / 2
        E = E0 @ ((sm / s1) * np.outer(v1, v1) + (sm / s2) * np.outer(v2, v2))
        ok = ok and bool(s1 > 0 and s2 > 0 and np.all(np.isfinite(E)))
    return Fit(ok, E0, E, v1, v2, s1, s2)


def fundamental(E, cam_a, cam_b, dtype):
    return inverse_pinhole(cam_b, dtype).T @ E @ inverse_pinhole(cam_a, dtype)


def two_view_pair(uv_a, uv_b, cam_a, cam_b, pair_index, n_hypotheses=64, inlier_px=2.0, seed=0, min_points=16, dtype=np.float64):
    """One pair: dict of T (3, 4), info (5,) = [n, inliers, front, status, winning hypothesis], stats (3,) = [score, rms, parallax],
    inlier (n,) bool, scores (H,), e2 (n,) at the winner (None without one)."""
    n = int(np.asarray(uv_a).reshape(-1, 2).shape[0])
    nan = dtype(np.nan)
    out = {"T": np.full((3, 4), nan, dtype=dtype), "info": np.array([n, 0, 0, TOO_FEW, -1], dtype=np.int32),
           "stats": np.full(3, nan, dtype=dtype), "inlier": np.zeros(n, dtype=bool), "scores": None, "e2": None}
    if n < max(SAMPLE, int(min_points)):
        return out
    und = np.concatenate([undistort(uv_a, cam_a, dtype), undistort(uv_b, cam_b, dtype)], axis=1)
    tau2 = dtype(inlier_px) * dtype(inlier_px)
    scores = np.full(n_hypotheses, np.inf, dtype=dtype)
    Fs = [None] * n_hypotheses
    for h in range(n_hypotheses):
        fit = eight_point(und[sample_positions(seed, pair_index, n, h, SAMPLE)], cam_a, cam_b, dtype)
        F = fundamental(fit.E, cam_a, cam_b, dtype)
        if fit.ok and np.all(np.isfinite(F)):
            e2 = sampson(F, und)
            with np.errstate(invalid="ignore"):
                scores[h] = np.sum(np.where(e2 <= tau2, e2, tau2))
            Fs[h] = F
    out["scores"] = scores
    win = int(np.argmin(scores))
    out["info"][3] = DEGENERATE
    out["stats"][0] = scores[win]
    if not scores[win] < np.inf:
        return out
    e2 = sampson(Fs[win], und)
    with np.errstate(invalid="ignore"):
        inl = e2 <= tau2
    n_inl = int(np.sum(inl))
    out["inlier"], out["e2"] = inl, e2
    out["info"][1], out["info"][4] = n_inl, win
    if n_inl < SAMPLE:
        return out
    fit = eight_point(und[inl], cam_a, cam_b, dtype)
    if not fit.ok:
        return out
    F = fundamental(fit.E, cam_a, cam_b, dtype)
    with np.errstate(all="ignore"):
        u1, u2 = fit.E0 @ fit.v1 / fit.s1, fit.E0 @ fit.v2 / fit.s2
        u3, v3 = np.cross(u1, u2), np.cross(fit.v1, fit.v2)
        u3 = u3 * (1 / np.sqrt(u3 @ u3))
        D, Cm = np.outer(u2, fit.v1) - np.outer(u1, fit.v2), np.outer(u3, v3)
        Rs = (Cm + D, Cm - D)
        ia, ib = inverse_pinhole(cam_a, dtype), inverse_pinhole(cam_b, dtype)
        ui = und[inl]
        one = np.ones(n_inl, dtype=dtype)
        A = np.stack([ia[0, 0] * ui[:, 0] + ia[0, 2], ia[1, 1] * ui[:, 1] + ia[1, 2], one], axis=1)
        Bv = np.stack([ib[0, 0] * ui[:, 2] + ib[0, 2], ib[1, 1] * ui[:, 3] + ib[1, 2], one], axis=1)
        bb, bt = np.sum(Bv * Bv, axis=1), Bv @ u3
        cnt, ang = [0] * 4, [dtype(0)] * 4
        for c, R in enumerate(Rs):
            r = A @ R.T
            rr, rb, rt = np.sum(r * r, axis=1), np.sum(r * Bv, axis=1), r @ u3
            det, la, lb = rr * bb - rb * rb, rb * bt - rt * bb, rr * bt - rb * rt
            cr = np.cross(r, Bv)
            a = np.arctan2(np.sqrt(np.sum(cr * cr, axis=1)), rb)
            pos, neg = (det > 0) & (la > 0) & (lb > 0), (det > 0) & (la < 0) & (lb < 0)
            cnt[2 * c], cnt[2 * c + 1] = int(np.sum(pos)), int(np.sum(neg))
            ang[2 * c], ang[2 * c + 1] = np.sum(np.where(pos, a * a, 0)), np.sum(np.where(neg, a * a, 0))
        cand = int(np.argmax(cnt))   # ties go to the lower candidate
        n_front = cnt[cand]
        out["info"][2] = n_front
        if n_front == 0:
            out["info"][3] = NO_CHEIRALITY
            return out
        rms, parallax = np.sqrt(np.sum(sampson(F, ui)) / n_inl), np.sqrt(ang[cand] / n_front)
        T = np.concatenate([Rs[cand // 2], ((-1 if cand & 1 else 1) * u3)[:, None]], axis=1)
    if not (np.all(np.isfinite(T)) and np.isfinite(rms) and np.isfinite(parallax)):
        return out
    out["T"], out["info"][3] = T, OK
    out["stats"][1], out["stats"][2] = rms, parallax
    out["candidate"] = cand
    return out


def correspondences(dct, n_cams, pairs=None, min_points=16):
    """The correspondence table of ``compiled_helpers.estimate_two_view``: a point is a key, a camera's pixel of a key is that of its
    lowest image, two cameras correspond where both see the key; rows of a pair ascend in the key.
    -> (pairs (P, 2), start (P + 1,), keys (n_corr,), uv_a, uv_b)."""
    d = np.asarray(dct, dtype=np.float64)
    seen = [dict() for _ in range(n_cams)]
    for row in d[np.lexsort((d[:, 1], d[:, 2], d[:, 0]))][::-1]:   # descending, so that the lowest image is written last
        seen[int(row[0])][int(row[2])] = row[3:5]
    if pairs is None:
        pairs = [(a, b) for a in range(n_cams) for b in range(a + 1, n_cams) if len(seen[a].keys() & seen[b].keys()) >= min_points]
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    keys, ua, ub, start = [], [], [], [0]
    for a, b in pairs:
        common = sorted(seen[int(a)].keys() & seen[int(b)].keys())
        keys += common
        ua += [seen[int(a)][k] for k in common]
        ub += [seen[int(b)][k] for k in common]
        start.append(len(keys))
    return (pairs, np.array(start, dtype=np.int64), np.array(keys, dtype=np.int64), np.array(ua, dtype=np.float64).reshape(-1, 2),
            np.array(ub, dtype=np.float64).reshape(-1, 2))


def estimate_pairs(uv_a, uv_b, start, pairs, intr, dtype=np.float64, **opts):
    """Every pair of a grouped table: stacked T (P, 3, 4), info (P, 5), stats (P, 3), inlier (n_corr,), and the per-pair dicts."""
    res = [two_view_pair(uv_a[start[p]:start[p + 1]], uv_b[start[p]:start[p + 1]], intr[a], intr[b], p, dtype=dtype, **opts)
           for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2))]
    P = len(res)
    return (np.array([r["T"] for r in res], dtype=dtype).reshape(P, 3, 4), np.array([r["info"] for r in res], dtype=np.int32).reshape(P, 5),
            np.array([r["stats"] for r in res], dtype=dtype).reshape(P, 3),
            np.concatenate([r["inlier"] for r in res]) if P else np.zeros(0, dtype=bool), res)


def run_table(table, opts, dtype=np.float64):
    return estimate_pairs(table["uv_a"], table["uv_b"], table["start"], table["pairs"], table["intr"], dtype=dtype, **opts)


def relative_gap(a, b):
    """max |a - b| / |b| over the entries where b is finite and not zero; entries that are not finite must be the same in both."""
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b)), "non-finite entries differ"
    fin &= b != 0
    return float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))) if np.any(fin) else 0.0


def pose_gap(T, T_ref):
    """max |T - T_ref| / max(|T_ref|, 1) over the finite entries; NaN poses must be NaN in both."""
    T, T_ref = np.asarray(T, dtype=np.longdouble).ravel(), np.asarray(T_ref, dtype=np.longdouble).ravel()
    fin = np.isfinite(T_ref)
    assert np.array_equal(fin, np.isfinite(T)), "NaN poses differ"
    return float(np.max(np.abs(T[fin] - T_ref[fin]) / np.maximum(np.abs(T_ref[fin]), 1))) if np.any(fin) else 0.0


def rounding(inputs):
    """float64 against extended precision on every input: name -> (d_T, d_s, float64 result), d_T over the entries of T against
    max(|entry|, 1), d_s relative over the scores of every hypothesis and the stats.  The discrete outputs must agree."""
    out = {}
    for name, (table, opts) in inputs.items():
        r64, rld = run_table(table, opts), run_table(table, opts, np.longdouble)
        assert np.array_equal(r64[1], rld[1]) and np.array_equal(r64[3], rld[3]), name
        d_s = relative_gap(r64[2], rld[2])
        for a, b in zip(r64[4], rld[4]):
            if a["scores"] is not None:
                d_s = max(d_s, relative_gap(a["scores"], b["scores"]))
        out[name] = (pose_gap(r64[0], rld[0]), d_s, r64)
    return out


# ---- seed_scene restated on the restatements (pnp_reference, tri_refine_reference) ---------------------------------------------------
def dlt_point(cams, uv, P, intr):
    """The reference's n-view DLT: undistorted pixels, M = [P_i | -x_i e_i], the right singular vector of the smallest singular value."""
    n = len(cams)
    Mx = np.zeros((3 * n, 4 + n))
    for i, c in enumerate(cams):
        x = undistort(uv[i], intr[c])[0]
        Mx[3 * i:3 * i + 3, :4] = P[c]
        Mx[3 * i:3 * i + 3, 4 + i] = -np.array([x[0], x[1], 1.0])
    X = np.linalg.svd(Mx)[2][-1]
    return X[:3] / X[3]


def seed_scene(dct, intr, n_cams, ref_cam=0, baseline=1.0, n_hypotheses=64, inlier_px=2.0, seed=0, min_points=16):
    """``pose_seeding.seed_scene`` step by step: dict(extr, points, placed, round_of_camera, first_pair, frame_cam, two_view)."""
    from scipy.spatial.transform import Rotation

    from tests import pnp_reference as pref
    from tests import tri_refine_reference as tref

    d = np.asarray(dct, dtype=np.float64)
    intr = np.asarray(intr, dtype=np.float64)
    C, n_keys = int(n_cams), int(d[:, 2].max()) + 1
    pairs, start, keys, ua, ub = correspondences(d, C, min_points=min_points)
    T, info, stats, inl, _ = estimate_pairs(ua, ub, start, pairs, intr, n_hypotheses=n_hypotheses, inlier_px=inlier_px, seed=seed, min_points=min_points)
    with np.errstate(invalid="ignore"):
        quality = np.where(info[:, 3] == OK, info[:, 2] * np.sin(stats[:, 2]), -np.inf)
    p0 = int(np.argmax(quality))
    a, b = int(pairs[p0, 0]), int(pairs[p0, 1])
    M = {a: np.eye(4), b: np.eye(4)}
    M[b][:3, :3], M[b][:3, 3] = T[p0, :, :3], baseline * T[p0, :, 3]
    round_of = {a: 0, b: 0}
    bad = set(keys[start[p0]:start[p0 + 1]][~inl[start[p0]:start[p0 + 1]]].tolist())
    obs = [dict() for _ in range(C)]                       # camera -> key -> pixel of the lowest image
    for row in d[np.lexsort((d[:, 1], d[:, 2], d[:, 0]))][::-1]:
        obs[int(row[0])][int(row[2])] = row[3:5]
    Kmat = np.zeros((C, 3, 3))
    Kmat[:, 0, 0], Kmat[:, 0, 2], Kmat[:, 1, 1], Kmat[:, 1, 2], Kmat[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0

    def triangulate():
        P = {c: Kmat[c] @ M[c][:3] for c in M}
        pts = np.full((n_keys, 3), np.nan)
        for k in range(n_keys):
            cams = [c for c in sorted(M) if k in obs[c]]
            if len(cams) >= 2 and not (len(M) == 2 and k in bad):   # the first pair alone: its inliers only
                uv = np.array([obs[c][k] for c in cams])
                X, _, _ = tref.refine_point(dlt_point(cams, uv, P, intr), cams, uv, P, Kmat, intr[:, 4:9])
                if np.all(np.isfinite(X)):
                    pts[k] = X
        return pts

    rnd = 0
    while True:
        pts = triangulate()
        have = np.all(np.isfinite(pts), axis=1)
        cand = [c for c in range(C) if c not in M and sum(have[k] for k in obs[c]) >= min_points]
        if not cand:
            break
        table = np.array([[c, 0, k, *obs[c][k]] for c in cand for k in sorted(obs[c]) if have[k]], dtype=np.float64)
        vp = pref.estimate_view_poses(table, np.where(have[:, None], pts, 0.0), intr, n_cams=C, n_imgs=1, min_points=min_points)
        new = [c for c in cand if vp.status[c, 0] == pref.CONVERGED and np.all(np.isfinite(vp.poses[c, 0]))]
        if not new:
            break
        rnd += 1
        for c in new:
            M[c] = np.eye(4)
            M[c][:3, :3], M[c][:3, 3] = Rotation.from_rotvec(vp.poses[c, 0, :3]).as_matrix(), vp.poses[c, 0, 3:]
            round_of[c] = rnd
    frame = ref_cam if ref_cam in M else a
    F = M[frame].copy()
    extr = np.full((C, 6), np.nan)
    for c in M:
        Mc = M[c] @ np.linalg.inv(F)
        extr[c, :3], extr[c, 3:] = Rotation.from_matrix(Mc[:3, :3]).as_rotvec(), Mc[:3, 3]
    return {"extr": extr, "points": pts @ F[:3, :3].T + F[:3, 3], "placed": np.array([c in M for c in range(C)]),
            "round_of_camera": np.array([round_of.get(c, -1) for c in range(C)]), "first_pair": (a, b), "frame_cam": frame,
            "two_view": (pairs, T, info, stats, inl)}


def align_similarity(X, Y):
    """The similarity (s, R, t) with Y ~ s R X + t in the least-squares sense (Umeyama), over the rows where both are finite."""
    ok = np.all(np.isfinite(X), axis=1) & np.all(np.isfinite(Y), axis=1)
    X, Y = X[ok], Y[ok]
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    U, S, Vt = np.linalg.svd((Y - my).T @ (X - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / np.sum((X - mx) ** 2)
    return s, R, my - s * R @ mx


def scene_gap(extr, points, rig):
    """After the similarity that takes the seeded points to the true ones: (largest point error / scene size, largest camera-centre error
    / scene size, largest rotation error in radians) over what was seeded."""
    from scipy.spatial.transform import Rotation

    s, R, t = align_similarity(points, rig["points"])
    ok = np.all(np.isfinite(points), axis=1)
    size = np.linalg.norm(rig["points"].max(axis=0) - rig["points"].min(axis=0))
    e_pts = np.max(np.linalg.norm(points[ok] @ (s * R).T + t - rig["points"][ok], axis=1)) / size
    e_c, e_r = 0.0, 0.0
    for c in np.nonzero(np.all(np.isfinite(extr), axis=1))[0]:
        Rc = Rotation.from_rotvec(extr[c, :3]).as_matrix()
        centre = s * R @ (-Rc.T @ extr[c, 3:]) + t                  # the seeded camera centre in the true frame
        e_c = max(e_c, np.linalg.norm(centre - (-rig["R"][c].T @ rig["t"][c])) / size)
        e_r = max(e_r, np.linalg.norm(Rotation.from_matrix(Rc @ R.T @ rig["R"][c].T).as_rotvec()))   # X_c = Rc R' X_true...
    return float(e_pts), float(e_c), float(e_r)
