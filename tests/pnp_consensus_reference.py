"""NumPy restatement of the consensus stage in front of the batched target-pose estimation (include/pcs_hip.h pcs_pnp_set_consensus,
csrc/ba_pnp_consensus.hpp), one view at a time: the counter-based sampler in uint64 arithmetic, the hypotheses through
``pnp_reference.linear_start`` on the sampled rows, the truncated score, the selection rules and the inlier flags, and
``pnp_reference.solve_view`` on the inliers.

A view's rows are taken sorted by key, as ``compiled_helpers.group_by_view`` hands them to the device."""
from __future__ import annotations

import numpy as np

from tests import pnp_reference as ref

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)
DEFAULTS = {"n_hypotheses": 64, "sample_size": 6, "inlier_px": 8.0, "seed": 0}


def mix64(z):
    """The splitmix64 finaliser: 64-bit multiplies, shifts and xors, wrapping."""
    with np.errstate(over="ignore"):
        z = U64(z)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def sample_positions(seed, cam, n, hyp, sample_size):
    """``sample_size`` distinct positions in [0, n), ascending: a pure function of (seed, camera, n, hypothesis).  Partial Fisher-Yates
    on the identity permutation, kept sparse as on the device (step i swaps positions i and j >= i)."""
    with np.errstate(over="ignore"):
        k = mix64(U64(seed) + GOLDEN)
        k = mix64(k ^ U64(cam))
        k = mix64(k ^ U64(n))
        k = mix64(k ^ U64(hyp))
        moved, pick = {}, []
        for i in range(sample_size):
            r = mix64(k + U64(i + 1) * GOLDEN)
            j = i + int(r % U64(n - i))
            vi, vj = moved.get(i, i), moved.get(j, j)
            moved[j] = vi
            pick.append(vj)
    return np.sort(np.array(pick, dtype=np.int64))


def squared_errors(pose, X, uv, cam9):
    """(e^2 (n,), usable (n,)): squared pixel error of every observation; usable = finite and in front of the camera."""
    with np.errstate(all="ignore"):
        p, _, Y = ref.project(ref.rodrigues(pose[:3]), np.asarray(pose[3:], dtype=np.float64), X, cam9)
        r = uv - p
        e2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        return e2, (Y[:, 2] > 0.0) & np.isfinite(e2)


def score_of(pose, X, uv, cam9, tau2):
    """sum min(e^2, tau^2); tau^2 for a non-finite measurement or projection or a depth <= 0; +inf for a non-finite candidate."""
    if not np.all(np.isfinite(pose)):
        return np.inf
    e2, usable = squared_errors(pose, X, uv, cam9)
    return float(np.sum(np.where(usable & (e2 <= tau2), e2, tau2)))


def consensus_view(keys, uv, cam, cam9, points, min_points=6, n_hypotheses=64, sample_size=6, inlier_px=8.0, seed=0, **opts):
    """One view.  -> dict(inliers (n,) bool, n_inliers, hypothesis (-1: none), candidate (0 start, 1 second pose), n_finite, used,
    score, scores (H, 2), result = ``solve_view`` on the inliers with ``n`` the view's observation count)."""
    order = np.argsort(np.asarray(keys), kind="stable")
    keys, uv = np.asarray(keys, dtype=np.int64)[order], np.asarray(uv, dtype=np.float64)[order]
    n, tau2 = keys.shape[0], float(inlier_px) ** 2
    X = points[keys]
    out = dict(hypothesis=-1, candidate=0, n_finite=0, used=1, score=np.inf, scores=np.full((n_hypotheses, 2), np.inf))
    if n < sample_size:   # the plain path
        flags = np.ones(n, dtype=bool)
        out.update(used=0, score=np.nan)
    else:
        poses = np.full((n_hypotheses, 2, 6), np.nan)
        for h in range(n_hypotheses):
            pos = sample_positions(seed, cam, n, h, sample_size)
            poses[h, 0], poses[h, 1], _ = ref.linear_start(keys[pos], uv[pos], cam9, points)
            out["scores"][h] = [score_of(poses[h, c], X, uv, cam9, tau2) for c in range(2)]
        out["n_finite"] = int(np.sum(np.isfinite(out["scores"][:, 0])))
        flat = out["scores"].ravel()   # candidate 2 h + c: argmin takes the first of equal scores
        best = int(np.argmin(flat))
        if np.isfinite(flat[best]):
            e2, usable = squared_errors(poses[best // 2, best % 2], X, uv, cam9)
            flags = usable & (e2 <= tau2)
            out.update(hypothesis=best // 2, candidate=best % 2, score=float(flat[best]))
        else:
            flags = np.zeros(n, dtype=bool)
    res = ref.solve_view(keys[flags], uv[flags], cam9, points, min_points=min_points, **opts)
    res["n"] = n
    inl = np.empty(n, dtype=bool)
    inl[order] = flags
    out.update(inliers=inl, n_inliers=int(flags.sum()), result=res)
    return out


def estimate_view_poses(dct, points, intr, n_imgs, min_points=6, **kw):
    """The whole table: {(cam, im): (rows of the table, ``consensus_view`` of them)}."""
    d = np.asarray(dct, dtype=np.float64)
    vid = d[:, 0].astype(np.int64) * n_imgs + d[:, 1].astype(np.int64)
    out = {}
    for v in np.unique(vid):
        rows = np.nonzero(vid == v)[0]
        c, i = divmod(int(v), n_imgs)
        out[(c, i)] = (rows, consensus_view(d[rows, 2].astype(np.int64), d[rows, 3:5], c, intr[c], points, min_points=min_points, **kw))
    return out
