"""NumPy restatement of the consensus stage in front of the planar homographies of the intrinsics estimation (include/pcs_hip.h
pcs_intr_set_consensus, csrc/ba_intr_consensus.hpp), one (camera, image, board) group at a time: the counter-based sampler of
``pnp_consensus_reference``, the hypotheses through ``intrinsics_reference.group_homography`` on the sampled rows, the truncated score of
the transfer error, the selection rules and the inlier flags, then ``group_homography`` on the inliers and ``camera_closed_form`` over a
camera's groups with the inlier counts as weights.

A group's rows are taken sorted by key, as ``compiled_helpers.group_by_board`` hands them to the device."""
from __future__ import annotations

import numpy as np

from tests import intrinsics_reference as ref
from tests.pnp_consensus_reference import sample_positions

DEFAULTS = {"n_hypotheses": 64, "sample_size": 6, "inlier_px": 8.0, "seed": 0}


def squared_errors(H, frame, X, uv):
    """(e^2 (n,), usable (n,)) of the transfer error uv - H q, q the plane coordinates in the hypothesis' frame; usable = finite and
    p_z > 0 (on the camera's side of the plane's horizon)."""
    c, e1, e2 = frame[:3], frame[3:6], frame[6:]
    with np.errstate(all="ignore"):
        Q = X - c
        q = np.stack([Q @ e1, Q @ e2, np.ones(X.shape[0])], axis=1)
        p = q @ np.asarray(H, dtype=np.float64).T
        r = uv - p[:, :2] / p[:, 2:3]
        e2_ = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        return e2_, (p[:, 2] > 0.0) & np.isfinite(e2_)


def score_of(hyp, X, uv, tau2):
    """sum min(e^2, tau^2); tau^2 for a non-finite measurement or projection or p_z <= 0; +inf for a hypothesis that is not USED."""
    if hyp["status"] != ref.GROUP_USED:
        return np.inf
    e2, usable = squared_errors(hyp["H"], hyp["frame"], X, uv)
    return float(np.sum(np.where(usable & (e2 <= tau2), e2, tau2)))


def select(scores):
    """(hypothesis or -1, score): the first of the lowest scores; -1 and +inf when none is finite."""
    scores = np.asarray(scores, dtype=np.float64)
    best = int(np.argmin(scores)) if scores.shape[0] else -1
    if best < 0 or not np.isfinite(scores[best]):
        return -1, np.inf
    return best, float(scores[best])


def consensus_group(keys, uv, cam, points, min_points=13, n_hypotheses=64, sample_size=6, inlier_px=8.0, seed=0, score_fn=score_of):
    """One group.  -> dict(inliers (n,) bool in the order of ``keys``, n_inliers, hypothesis (-1: none), n_finite, used, score,
    scores (H,), gap = relative distance of the winner's score from the best score of ANOTHER sample (inf where there is none),
    result = ``group_homography`` on the inliers with ``n`` the group's observation count and ``n_inliers`` beside it)."""
    order = np.argsort(np.asarray(keys), kind="stable")
    keys, uv = np.asarray(keys, dtype=np.int64)[order], np.asarray(uv, dtype=np.float64)[order]
    n, tau2 = keys.shape[0], float(inlier_px) ** 2
    X = np.asarray(points, dtype=np.float64)[keys]
    out = dict(hypothesis=-1, n_finite=0, used=1, score=np.inf, scores=np.full(n_hypotheses, np.inf), gap=np.inf)
    flags = np.ones(n, dtype=bool)   # rules (a) and (b): the whole group goes on
    if n < max(sample_size, min_points):
        out.update(used=0, score=np.nan)
    else:
        hyps, samples = [], []
        for h in range(n_hypotheses):
            pos = sample_positions(seed, cam, n, h, sample_size)
            samples.append(tuple(pos))
            hyps.append(ref.group_homography(keys[pos], uv[pos], points, min_points=sample_size))
            out["scores"][h] = score_fn(hyps[h], X, uv, tau2)
        out["n_finite"] = int(np.sum(np.isfinite(out["scores"])))
        best, score = select(out["scores"])
        out.update(hypothesis=best, score=score)
        if best >= 0:
            # Two hypotheses that drew the SAME sample go through the same arithmetic on the same numbers: their scores are equal bit
            # for bit here and on the device, and the lower one wins in both.  What rounding can decide is the order of different samples.
            rest = [out["scores"][h] for h in range(n_hypotheses) if samples[h] != samples[best] and np.isfinite(out["scores"][h])]
            if rest:
                out["gap"] = float((min(rest) - score) / min(rest)) if min(rest) > 0 else 0.0
            e2, usable = squared_errors(hyps[best]["H"], hyps[best]["frame"], X, uv)
            flags = usable & (e2 <= tau2)
    res = ref.group_homography(keys[flags], uv[flags], points, min_points=min_points)
    res["n_inliers"], res["n"] = res["n"], n
    inl = np.empty(n, dtype=bool)
    inl[order] = flags
    out.update(inliers=inl, n_inliers=int(flags.sum()), result=res)
    return out


def estimate_intrinsics(dct, points, *, n_cams=None, n_imgs=None, board_of_key=None, res=None, model="auto", min_points=13, consensus=0,
                        sample_size=6, inlier_px=8.0, seed=0, **_):
    """The whole table: the closed-form fields of ``compiled_helpers.IntrinsicsEstimate`` with its five consensus fields, plus
    ``group_gap`` and ``group_finite``.  ``consensus=0`` is ``intrinsics_reference.estimate_intrinsics``."""
    if not consensus:
        return ref.estimate_intrinsics(dct, points, n_cams=n_cams, n_imgs=n_imgs, board_of_key=board_of_key, res=res, model=model, min_points=min_points)
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    C = (int(d[:, 0].max()) + 1 if d.shape[0] else 0) if n_cams is None else int(n_cams)
    I = (int(d[:, 1].max()) + 1 if d.shape[0] else 0) if n_imgs is None else int(n_imgs)
    bok = np.zeros(pts.shape[0], dtype=np.int64) if board_of_key is None else np.asarray(board_of_key, dtype=np.int64)
    nb = int(bok.max()) + 1 if bok.shape[0] else 1
    res_c = None if res is None else np.broadcast_to(np.asarray(res, dtype=np.float64), (C, 2))
    if model == "auto":
        model = "focal" if res is not None else "full"
    key = d[:, 2].astype(np.int64)
    gid = (d[:, 0].astype(np.int64) * I + d[:, 1].astype(np.int64)) * nb + bok[key]
    ids = np.unique(gid)
    index = np.stack([ids // (I * nb), (ids // nb) % I, ids % nb], axis=1).astype(np.int64) if len(ids) else np.zeros((0, 3), dtype=np.int64)
    out = ref.IntrinsicsRef()
    out.inliers = np.zeros(d.shape[0], dtype=bool)
    cons = []
    for g, ix in zip(ids, index):
        rows = np.nonzero(gid == g)[0]
        c = consensus_group(key[rows], d[rows, 3:5], int(ix[0]), pts, min_points=min_points, n_hypotheses=consensus, sample_size=sample_size,
                            inlier_px=inlier_px, seed=seed)
        out.inliers[rows] = c["inliers"]
        cons.append(c)
    groups = [c["result"] for c in cons]
    out.group_index = index
    out.group_status = np.array([g["status"] for g in groups], dtype=np.int32)
    out.group_counts = np.array([g["n"] for g in groups], dtype=np.int32)
    out.group_inliers = np.array([c["n_inliers"] for c in cons], dtype=np.int32)
    out.group_hypothesis = np.array([c["hypothesis"] for c in cons], dtype=np.int32)
    out.group_consensus_used = np.array([c["used"] for c in cons], dtype=bool)
    out.group_score = np.array([c["score"] for c in cons], dtype=np.float64)
    out.group_gap = np.array([c["gap"] for c in cons], dtype=np.float64)
    out.group_finite = np.array([c["n_finite"] for c in cons], dtype=np.int32)
    out.homographies = np.stack([g["H"] for g in groups]) if groups else np.zeros((0, 3, 3))
    out.plane_frames = np.stack([g["frame"] for g in groups]) if groups else np.zeros((0, 9))
    out.intr, out.status = np.full((C, 9), np.nan), np.zeros(C, dtype=np.int32)
    out.n_groups, out.eig_ratio = np.zeros(C, dtype=np.int32), np.full(C, np.nan)
    for c in range(C):   # the camera's pixel centroid weights its groups by the rows they were fitted to: the inliers
        mine = [dict(g, n=g["n_inliers"]) for g, ix in zip(groups, index) if ix[0] == c]
        out.intr[c], out.status[c], out.n_groups[c], out.eig_ratio[c] = ref.camera_closed_form(mine, None if res_c is None else res_c[c], model)
    out.intr_init = out.intr
    return out
