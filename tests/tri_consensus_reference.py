"""NumPy restatement of the view-pair consensus in front of the batched triangulation (include/pcs_hip.h pcs_tri_set_consensus,
csrc/ba_tri_consensus.hpp): the sampler bit for bit, the pair enumeration, the truncated score, the tie rule and the flags.

Hypothesis points are the DLT formulation of the oracle (oracle/ba_oracle.py: undistort, then the smallest right singular vector of the
stacked [P_i | -x_i] matrix) for the two sampled views, restated here with one refinement: LAPACK's SVD leaves that vector with an error of
eps * sigma_max / (gap to the next singular value) — sigma_max ~ 2e3 (pixels), the gap down to 0.2 for a pair with a short baseline — and
two steps of inverse iteration on the QR factor of the same matrix take most of it out.  Measured against 50-digit arithmetic on the pairs
that win on the rigs of tests/tri_consensus_inputs.py: the SVD alone is off by up to 4.0e-13 in the point, which moves a score of
0.2 px^2 (three views that fit well) by 3.4e-9 relative; refined, by 1.4e-14 and 1e-10, which is also where the device's DLT is.
The projection is the one of tests/tri_refine_reference.py, vectorised over candidates and views."""
from __future__ import annotations

import numpy as np

from oracle import ba_oracle as orc

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MIN_VIEWS = 3


def mix64(z: int) -> int:
    """The splitmix64 finaliser on Python integers (cons_mix64)."""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def n_used(V: int, H: int) -> int:
    """Hypotheses of a point with V views that carry a pair."""
    return 0 if V < MIN_VIEWS else min(H, V * (V - 1) // 2)


def exhaustive(V: int, H: int) -> bool:
    return V * (V - 1) // 2 <= H


def pair(seed: int, j: int, V: int, H: int, h: int):
    """The pair (a < b) of hypothesis h of point j with V >= 3 views; None for an unused hypothesis."""
    seed, j, V, H, h = int(seed), int(j), int(V), int(H), int(h)   # Python integers: the 64-bit products below are taken modulo 2^64 by hand
    if h >= n_used(V, H):
        return None
    if exhaustive(V, H):
        a, rem = 0, h
        while rem >= V - 1 - a:
            rem -= V - 1 - a
            a += 1
        return a, a + 1 + rem
    k = mix64(seed + GOLDEN)
    k = mix64(k ^ j)
    k = mix64(k ^ V)
    k = mix64(k ^ h)
    r = mix64(k + GOLDEN)
    p, q = r % V, (r >> 32) % (V - 1)
    q += 1 if q >= p else 0
    return min(p, q), max(p, q)


def pairs(seed: int, j: int, V: int, H: int):
    return [pair(seed, j, V, H, h) for h in range(n_used(V, H))]


def dlt_pairs(Pa, Pb, ua, ub):
    """The DLT points of n two-view systems: projection matrices (n, 3, 4) and undistorted pixels (n, 2) of either view -> (n, 3);
    NaN where a pixel is not finite."""
    n = Pa.shape[0]
    X = np.full((n, 3), np.nan)
    ok = np.all(np.isfinite(ua), axis=1) & np.all(np.isfinite(ub), axis=1)
    if not ok.any():
        return X
    M = np.zeros((int(ok.sum()), 6, 6))
    M[:, :3, :4], M[:, 3:, :4] = Pa[ok], Pb[ok]
    M[:, :2, 4], M[:, 2, 4] = -ua[ok], -1.0
    M[:, 3:5, 5], M[:, 5, 5] = -ub[ok], -1.0
    v = np.linalg.svd(M)[2][:, -1, :]
    try:
        R = np.linalg.qr(M, mode="r")
        with np.errstate(all="ignore"):
            for _ in range(2):   # inverse iteration: (R'R) w = v
                w = np.linalg.solve(R, np.linalg.solve(np.swapaxes(R, 1, 2), v[..., None]))[..., 0]
                w = w / np.linalg.norm(w, axis=1, keepdims=True)
                v = np.where(np.all(np.isfinite(w), axis=1, keepdims=True), w, v)
    except np.linalg.LinAlgError:   # an exactly singular factor: the SVD's vector stays
        pass
    with np.errstate(all="ignore"):
        X[ok] = v[:, :3] / v[:, 3:4]
    return X


def project_many(X, cams, P, K, D):
    """pi_c(X) for candidates X (H, 3) and cameras cams (V,): uv (H, V, 2) and depths (H, V)."""
    Pc, Kc, Dc = P[cams], K[cams], D[cams]
    h = np.einsum("vik,hk->hvi", Pc[:, :, :3], X) + Pc[None, :, :, 3]
    with np.errstate(all="ignore"):
        a, b = h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]
        fx, fy, cx, cy = Kc[:, 0, 0], Kc[:, 1, 1], Kc[:, 0, 2], Kc[:, 1, 2]
        k0, k1, p0, p1, k2 = (Dc[:, i] for i in range(5))
        x, y = (a - cx) / fx, (b - cy) / fy
        r2 = x * x + y * y
        kup = 1 + k0 * r2 + k1 * r2 ** 2 + k2 * r2 ** 3
        xD = x * kup + 2 * p0 * x * y + p1 * (r2 + 2 * x * x)
        yD = y * kup + p0 * (r2 + 2 * y * y) + 2 * p1 * x * y
    return np.stack([xD * fx + cx, yD * fy + cy], axis=-1), h[..., 2]


def errors(X, cams, uv, P, K, D):
    """e^2 (H, V) and `usable` (H, V): finite and in front of the camera."""
    p, depth = project_many(np.atleast_2d(X), cams, P, K, D)
    with np.errstate(all="ignore"):
        e2 = np.sum((uv[None] - p) ** 2, axis=-1)
        usable = np.isfinite(e2) & (depth > 0)
    return e2, usable


def consensus_point(j, cams, uv, P, K, D, H, inlier_px, seed):
    """One point -> dict: flags (V,) bool, cinfo [inliers, winner or -1, finite hypotheses, used], score, scores (H,) (+inf beyond the
    used ones), pairs, candidates (H, 3)."""
    V, tau2 = len(cams), inlier_px * inlier_px
    if V < MIN_VIEWS:
        return dict(flags=np.ones(V, dtype=bool), cinfo=[V, -1, 0, 0], score=np.nan, scores=np.full(H, np.inf), pairs=[],
                    candidates=np.full((H, 3), np.nan))
    pr = pairs(seed, j, V, H)
    with np.errstate(all="ignore"):
        ud = np.array([orc.undistort(uv[v], K[cams[v]], D[cams[v]]) for v in range(V)])
    cand = np.full((H, 3), np.nan)
    ia, ib = np.array([a for a, _ in pr]), np.array([b for _, b in pr])
    cand[: len(pr)] = dlt_pairs(P[cams[ia]], P[cams[ib]], ud[ia], ud[ib])
    fin = np.all(np.isfinite(cand), axis=1)
    e2, usable = errors(np.where(fin[:, None], cand, 0.0), cams, uv, P, K, D)
    per_view = np.where(usable & (e2 <= tau2), e2, tau2)
    scores = np.where(fin, per_view.sum(axis=1), np.inf)
    n_fin = int(fin.sum())
    if n_fin == 0:
        return dict(flags=np.zeros(V, dtype=bool), cinfo=[0, -1, 0, 1], score=np.inf, scores=scores, pairs=pr, candidates=cand)
    win = int(np.argmin(scores))   # the first of equal minima: ties go to the lower hypothesis
    flags = usable[win] & (e2[win] <= tau2)
    n_in = int(flags.sum())
    if n_in < 2:
        flags, n_in = np.zeros(V, dtype=bool), 0
    return dict(flags=flags, cinfo=[n_in, win, n_fin, 1], score=float(scores[win]), scores=scores, pairs=pr, candidates=cand)


def best_two_gap(res) -> float:
    """Relative gap between the best two scores of DISTINCT pairs (inf when there is no second finite one)."""
    best = {}
    for pr, s in zip(res["pairs"], res["scores"]):
        if np.isfinite(s):
            best[pr] = min(s, best.get(pr, np.inf))
    s = sorted(best.values())
    if len(s) < 2:
        return np.inf
    return (s[1] - s[0]) / s[1] if s[1] > 0 else 0.0


def consensus_table(rec, start, P, K, D, H, inlier_px=8.0, seed=0):
    """The stage on a grouped table (rows [cam, ..., u, v], start (n_pts + 1)) -> inlier (n_obs,) bool, cinfo (n_pts, 4) int32,
    score (n_pts,), gap (n_pts,)."""
    n = len(start) - 1
    inlier = np.zeros(rec.shape[0], dtype=bool)
    cinfo, score, gap = np.zeros((n, 4), dtype=np.int32), np.empty(n), np.full(n, np.inf)
    for j in range(n):
        rows = rec[start[j]:start[j + 1]]
        r = consensus_point(j, rows[:, 0].astype(int), rows[:, -2:], P, K, D, H, inlier_px, seed)
        inlier[start[j]:start[j + 1]] = r["flags"]
        cinfo[j], score[j] = r["cinfo"], r["score"]
        if r["cinfo"][3]:
            gap[j] = best_two_gap(r)
    return inlier, cinfo, score, gap
