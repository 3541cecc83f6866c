"""NumPy restatement of the batched point-set registration (include/pcs_hip.h pcs_align_run, csrc/ba_align.hpp), one problem at a time
and generic in the dtype, so that it runs in float64 and in ``np.longdouble``: the two-pass sums, Horn's 4 x 4 matrix, the cyclic Jacobi
of ``twoview_reference``, the quaternion, scale, translation, conditioning and statuses; the counter-based sampler (that of
``pnp_consensus_reference``), the truncated score, the selection and the fit over the flags; and the front ends on top of it.

Sums run in row order here and in lane order on the device; everything else is the device's formula."""
from __future__ import annotations

import numpy as np

from tests.pnp_consensus_reference import sample_positions
from tests.twoview_reference import jacobi_eigh

OK, TOO_FEW, DEGENERATE, NONFINITE, NO_CONSENSUS = 0, 1, 2, 3, 4
SAMPLE, SWEEPS = 3, 10
DEFAULTS = {"model": "rigid", "n_hypotheses": 0, "inlier_dist": None, "seed": 0, "min_points": 3, "rank_tol": 1e-10}


def usable_rows(src, dst, w):
    finite = np.all(np.isfinite(src), axis=1) & np.all(np.isfinite(dst), axis=1)
    return finite, finite & (w > 0)


def seq_sum(a):
    """The sum over the first axis, one row after the other (np.sum adds pairwise)."""
    return np.cumsum(a, axis=0)[-1]


def sums(src, dst, w, used, dtype):
    """(sum w, centroid of x, centroid of y, S = sum w x~ y~', sum w |x~|^2) over the rows in ``used`` (at least one), in row order."""
    x, y, ww = src[used], dst[used], w[used]
    with np.errstate(all="ignore"):
        sw = seq_sum(ww)
        cx, cy = seq_sum(ww[:, None] * x) / sw, seq_sum(ww[:, None] * y) / sw
        xc, yc = x - cx, y - cy
        wx = ww[:, None] * xc
        return sw, cx, cy, seq_sum(wx[:, :, None] * yc[:, None, :]), seq_sum(seq_sum((wx * xc).T))


def closed_form(S, sxx, cx, cy, similarity, rank_tol, dtype=np.float64):
    """-> (status, R, A = s R, t, s, conditioning)."""
    nan = dtype(np.nan)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]], dtype=dtype)
    lam, V = jacobi_eigh(N, SWEEPS, dtype)
    if not (np.all(np.isfinite(lam)) and np.isfinite(sxx)):
        return NONFINITE, None, None, None, nan, nan
    k1 = int(np.argmax(lam))                      # ties: the lower index
    l1, l2, l4 = lam[k1], np.max(np.delete(lam, k1)), np.min(lam)
    with np.errstate(all="ignore"):
        cond = (l1 - l2) / (l1 - l4)
        s = l1 / sxx if similarity else dtype(1)
    if not l1 - l4 > 0:
        return DEGENERATE, None, None, None, nan, dtype(0)
    if not cond > dtype(rank_tol):
        return DEGENERATE, None, None, None, nan, cond
    q = V[:, k1]
    qn = 1 / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    w, x, y, z = q[0] * qn, q[1] * qn, q[2] * qn, q[3] * qn
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=dtype)
    A = s * R
    t = cy - A @ cx
    if not (np.isfinite(s) and np.all(np.isfinite(A)) and np.all(np.isfinite(t))):
        return NONFINITE, None, None, None, nan, cond
    return OK, R, A, t, s, cond


def distance2(A, t, src, dst):
    with np.errstate(all="ignore"):
        e = dst - src @ A.T - t
        return np.sum(e * e, axis=1)


def fit(src, dst, w, mask=None, model="rigid", min_points=3, rank_tol=1e-10, dtype=np.float64):
    """``align_fit_kernel`` on one problem: dict of status, R, t, scale, rms, cond, n_used, used (n,) bool, dist (n,)."""
    n = src.shape[0]
    nan = dtype(np.nan)
    finite, usable = usable_rows(src, dst, w)
    used = usable if mask is None else usable & mask
    out = {"status": OK, "R": np.full((3, 3), nan, dtype=dtype), "t": np.full(3, nan, dtype=dtype), "scale": nan, "rms": nan, "cond": nan,
           "n_used": int(np.sum(used)), "used": np.zeros(n, dtype=bool), "dist": np.full(n, nan, dtype=dtype)}
    if np.sum(usable) < min_points:
        out["status"] = NONFINITE if n > 0 and not np.any(finite) else TOO_FEW
        return out
    if np.sum(used) < min_points:
        out["status"] = NO_CONSENSUS
        return out
    sw, cx, cy, S, sxx = sums(src, dst, w, used, dtype)
    status, R, A, t, s, cond = closed_form(S, sxx, cx, cy, model == "similarity", rank_tol, dtype)
    out["status"], out["cond"] = status, cond
    if status != OK:
        return out
    d2 = distance2(A, t, src, dst)
    with np.errstate(all="ignore"):
        rms = np.sqrt(seq_sum(w[used] * d2[used]) / sw)
    if not np.isfinite(rms):
        out["status"] = NONFINITE
        return out
    with np.errstate(invalid="ignore"):
        out.update(R=R, t=t, scale=s, rms=rms, used=used, dist=np.sqrt(d2))
    return out


def hypothesis(src, dst, w, problem_index, h, seed, model, rank_tol, dtype=np.float64):
    """[s R | t] of the triple that hypothesis h draws, or None."""
    n = src.shape[0]
    if n < SAMPLE:
        return None
    pick = sample_positions(seed, problem_index, n, h, SAMPLE)
    x, y, ww = src[pick], dst[pick], w[pick]
    if not np.all(usable_rows(x, y, ww)[1]):
        return None
    _, cx, cy, S, sxx = sums(x, y, ww, np.ones(SAMPLE, dtype=bool), dtype)
    status, _, A, t, _, _ = closed_form(S, sxx, cx, cy, model == "similarity", rank_tol, dtype)
    return (A, t) if status == OK else None


def score_of(hyp, src, dst, usable, tau2):
    if hyp is None:
        return np.inf
    d2 = distance2(hyp[0], hyp[1], src, dst)
    with np.errstate(invalid="ignore"):
        return seq_sum(np.where(usable & (d2 <= tau2), d2, tau2))


def align_problem(src, dst, w=None, problem_index=0, model="rigid", n_hypotheses=0, inlier_dist=None, seed=0, min_points=3, rank_tol=1e-10,
                  dtype=np.float64):
    """One problem: the dict of ``fit`` plus n_inliers, hypothesis, score, scores (H,) and d2 (n,) at the winner."""
    src, dst = np.asarray(src, dtype=dtype).reshape(-1, 3), np.asarray(dst, dtype=dtype).reshape(-1, 3)
    n = src.shape[0]
    w = np.ones(n, dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
    nan = dtype(np.nan)
    if not n_hypotheses:
        out = fit(src, dst, w, None, model, min_points, rank_tol, dtype)
        out.update(n_inliers=out["n_used"], hypothesis=-1, score=nan, scores=None, d2=None)
        return out
    usable = usable_rows(src, dst, w)[1]
    tau2 = dtype(inlier_dist) * dtype(inlier_dist)
    if n < SAMPLE:
        mask, win, best, scores, d2, n_inl = np.ones(n, dtype=bool), -1, nan, None, None, n
    else:
        hyps = [hypothesis(src, dst, w, problem_index, h, seed, model, rank_tol, dtype) for h in range(n_hypotheses)]
        scores = np.array([score_of(hp, src, dst, usable, tau2) for hp in hyps], dtype=dtype)
        win = int(np.argmin(scores))              # ties: the lower hypothesis
        best = scores[win]
        if not best < np.inf:
            mask, win, d2 = np.zeros(n, dtype=bool), -1, None
        else:
            d2 = distance2(hyps[win][0], hyps[win][1], src, dst)
            with np.errstate(invalid="ignore"):
                mask = usable & (d2 <= tau2)
        n_inl = int(np.sum(mask))
    out = fit(src, dst, w, mask, model, min_points, rank_tol, dtype)
    out.update(n_inliers=n_inl, hypothesis=win, score=best, scores=scores, d2=d2, mask=mask)
    return out


def align_table(src, dst, start, weights=None, dtype=np.float64, **opts):
    """Every problem of a table: dict of stacked R (P, 3, 3), t (P, 3), scale, rms, score, cond (P,), info (P, 4) int32 = [rows used,
    inliers, status, hypothesis], inlier (n,) bool, dist (n,), and the per-problem dicts in ``problems``."""
    src, dst, start = np.asarray(src).reshape(-1, 3), np.asarray(dst).reshape(-1, 3), np.asarray(start, dtype=np.int64)
    res = []
    for j in range(start.shape[0] - 1):
        a, b = int(start[j]), int(start[j + 1])
        res.append(align_problem(src[a:b], dst[a:b], None if weights is None else np.asarray(weights)[a:b], j, dtype=dtype, **opts))
    P = len(res)
    cons = bool(opts.get("n_hypotheses", 0))
    return {"R": np.array([r["R"] for r in res], dtype=dtype).reshape(P, 3, 3), "t": np.array([r["t"] for r in res], dtype=dtype).reshape(P, 3),
            "scale": np.array([r["scale"] for r in res], dtype=dtype), "rms": np.array([r["rms"] for r in res], dtype=dtype),
            "score": np.array([r["score"] for r in res], dtype=dtype), "cond": np.array([r["cond"] for r in res], dtype=dtype),
            "info": np.array([[r["n_used"], r["n_inliers"], r["status"], r["hypothesis"]] for r in res], dtype=np.int32).reshape(P, 4),
            "inlier": np.concatenate([(r["mask"] if cons else r["used"]) for r in res]) if P else np.zeros(0, dtype=bool),
            "dist": np.concatenate([r["dist"] for r in res]) if P else np.zeros(0, dtype=dtype), "problems": res}


# ---- independent statements of the same fit, for the CPU checks -------------------------------------------------------------------------
def kabsch_umeyama(src, dst, w=None, similarity=False):
    """The SVD form in float64 (Kabsch 1976 / Umeyama 1991), weighted: (s, R, t)."""
    X, Y = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    w = np.ones(X.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    mx, my = w @ X / w.sum(), w @ Y / w.sum()
    U, sig, Vt = np.linalg.svd((Y - my).T @ (w[:, None] * (X - mx)))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = float(np.sum(sig * np.diag(D)) / np.sum(w * np.sum((X - mx) ** 2, axis=1))) if similarity else 1.0
    return s, R, my - s * R @ mx


def svd_conditioning(src, dst, w=None):
    """(sigma_2 + d sigma_3) / (sigma_1 + sigma_2) of the weighted cross-covariance."""
    X, Y = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    w = np.ones(X.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    mx, my = w @ X / w.sum(), w @ Y / w.sum()
    M = (w[:, None] * (X - mx)).T @ (Y - my)
    sig = np.linalg.svd(M, compute_uv=False)
    return (sig[1] + np.sign(np.linalg.det(M)) * sig[2]) / (sig[0] + sig[1])


def transform_gap(a, b, size=1.0):
    """(max |dR|, max |dt| / size, max |ds| / s) between two results of ``align_table`` over the problems that are OK in ``b``; the
    statuses must agree."""
    assert np.array_equal(a["info"][:, 2], b["info"][:, 2]), (a["info"][:, 2], b["info"][:, 2])
    ok = b["info"][:, 2] == OK
    if not np.any(ok):
        return 0.0, 0.0, 0.0
    ld = np.longdouble
    dR = np.max(np.abs(np.asarray(a["R"], dtype=ld)[ok] - np.asarray(b["R"], dtype=ld)[ok]))
    dt = np.max(np.abs(np.asarray(a["t"], dtype=ld)[ok] - np.asarray(b["t"], dtype=ld)[ok]) / np.broadcast_to(np.asarray(size, dtype=ld), ok.shape)[ok][:, None])
    sb = np.asarray(b["scale"], dtype=ld)[ok]
    ds = np.max(np.abs(np.asarray(a["scale"], dtype=ld)[ok] - sb) / sb)
    return float(dR), float(dt), float(ds)


# ---- the front ends -----------------------------------------------------------------------------------------------------------------
def rotvec_of(R):
    from scipy.spatial.transform import Rotation

    return Rotation.from_matrix(np.asarray(R, dtype=np.float64)).as_rotvec()


def register_target(points_by_image, template, dtype=np.float64, **opts):
    """``compiled_helpers.register_target``: one problem per image over the finite rows, template -> image points; poses (I, 6) =
    [rotvec, t], NaN where the status is not OK, and the table result."""
    pts, tmpl = np.asarray(points_by_image, dtype=np.float64), np.asarray(template, dtype=np.float64)
    I, K = pts.shape[0], pts.shape[1]
    res = align_table(np.broadcast_to(tmpl, (I, K, 3)).reshape(-1, 3), pts.reshape(-1, 3), np.arange(I + 1, dtype=np.int64) * K, dtype=dtype, **opts)
    poses = np.full((I, 6), np.nan)
    for i in np.nonzero(res["info"][:, 2] == OK)[0]:
        poses[i, :3], poses[i, 3:] = rotvec_of(res["R"][i]), np.asarray(res["t"][i], dtype=np.float64)
    return poses, res


def align_scene(extr, points, reference_points, model="similarity", dtype=np.float64, **opts):
    """``pose_seeding.align_scene`` on bare arrays: extr (C, 6) [rotvec, t] world -> camera (NaN: not placed), points (K, 3), the
    reference (K, 3) with NaN where unknown.  -> (extr', points', (s, R, t), status)."""
    from scipy.spatial.transform import Rotation

    extr, points = np.asarray(extr, dtype=np.float64), np.asarray(points, dtype=np.float64)
    res = align_table(points, np.asarray(reference_points, dtype=np.float64), np.array([0, points.shape[0]]), model=model, dtype=dtype, **opts)
    if res["info"][0, 2] != OK:
        return extr, points, None, int(res["info"][0, 2])
    s, R, t = float(res["scale"][0]), np.asarray(res["R"][0], dtype=np.float64), np.asarray(res["t"][0], dtype=np.float64)
    out = np.full_like(extr, np.nan)
    for c in np.nonzero(np.all(np.isfinite(extr), axis=1))[0]:
        Rc = Rotation.from_rotvec(extr[c, :3]).as_matrix() @ R.T
        out[c, :3], out[c, 3:] = Rotation.from_matrix(Rc).as_rotvec(), s * extr[c, 3:] - Rc @ t
    return out, s * points @ R.T + t, (s, R, t), OK


def gauge_transform(extr, poses, points, ref_points, visible, scale="similarity", pairs=None, dtype=np.float64, **opts):
    """``SelfBundleHandler.apply_gauge_transform`` on bare arrays: -> (extr', poses', points', s).  ``pairs`` (n, 2): the feature pairs of
    the "distances" scale."""
    from scipy.spatial.transform import Rotation

    def to4(p):
        M = np.tile(np.eye(4), (p.shape[0], 1, 1))
        M[:, :3, :3], M[:, :3, 3] = Rotation.from_rotvec(p[:, :3]).as_matrix(), p[:, 3:]
        return M

    def from4(M):
        return np.concatenate([Rotation.from_matrix(M[:, :3, :3]).as_rotvec(), M[:, :3, 3]], axis=1)

    extr, poses = np.asarray(extr, dtype=np.float64), np.asarray(poses, dtype=np.float64)
    pts, ref = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(ref_points, dtype=np.float64).reshape(-1, 3)
    vm = np.asarray(visible, dtype=bool)
    start = np.array([0, int(np.sum(vm))])
    if scale == "distances":
        a, b = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
        s = float(np.mean(np.linalg.norm(ref[a] - ref[b], axis=1) / np.linalg.norm(pts[a] - pts[b], axis=1)))
        res = align_table(s * pts[vm], ref[vm], start, model="rigid", dtype=dtype, **opts)
    else:
        res = align_table(pts[vm], ref[vm], start, model="similarity", dtype=dtype, **opts)
        s = float(res["scale"][0])
    assert res["info"][0, 2] == OK
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = np.asarray(res["R"][0], dtype=np.float64), np.asarray(res["t"][0], dtype=np.float64)
    Ui = np.linalg.inv(U)
    P, E = to4(poses), to4(extr)
    P[:, :3, 3] *= s
    E[:, :3, 3] *= s
    return from4(E @ Ui), from4(U @ P @ Ui), s * pts @ U[:3, :3].T + U[:3, 3], s
