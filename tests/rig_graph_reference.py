"""NumPy restatement of the view-graph seeding (``pose_seeding.estimate_camera_relative_poses_graph``, csrc/ba_riggraph.hpp), written
from the specification and not from the kernels: plain loops, every sum sequential in the stated order.

M[c, i]: view transform target -> camera c in image i (NaN = not estimated).  T_ab^(i) = M[a, i] inv(M[b, i]) takes camera-b coordinates to
camera-a coordinates.  E_c: world -> camera c.  pbar, rho: centroid of the template and RMS distance of its points from it.

1. edges      per pair a < b with n >= 1 shared images: candidates T_ab^(i); d(T_i, T_j)^2 = (rho^2 / 3)(6 - 2 tr(R_i' R_j))
              + |(R_i - R_j) m_b + t_i - t_j|^2 with m_b the mean of M[b, j] pbar over the shared images (increasing j); the medoid
              minimises S_i = sum_j d(T_i, T_j) (increasing j, ties to the lowest image); sigma = S / (n - 1), 0 for n = 1.
              6 - 2 tr(R_i' R_j) is evaluated as |R_i - R_j|_F^2, the same number without the cancellation, and d(T_i, T_i) = 0.
2. tree       edge cost sigma + rho / n; Dijkstra from ref_cam, ties to the lower camera index; E_ref = I, E_c = T[c, parent] E_parent;
              unreachable cameras raise ValueError naming them.
3. scoring    W[c', i] = inv(E_c') M[c', i]; per view (c, i) and candidate c' the sum over the view's detections (key order) of
              |project_c(E_c W[c', i] p_k) - uv| with the legacy cost's formulas (P = K E pre-multiplied, Brown-Conrady); errors[c', i]
              adds the views of image i in view order; best_cam = argmin over finite entries, ties to the lowest camera (camera c is
              no candidate for the medoid image of the edge to its parent: there its estimate repeats the parent's); an image
              without a finite candidate is missing and takes the previous non-missing pose (the first one when none precedes it).
4. re-basing  the world becomes the target of ref_pose (the first non-missing image when that is missing).

``dtype=np.longdouble`` runs step 1 and the sums of step 3 (and the transforms they are made of) in extended precision: the
difference to float64 is the rounding error of this restatement, from which the GPU tests take their tolerance."""
from types import SimpleNamespace

import numpy as np


def rodrigues(r, dtype=np.float64):
    r = np.asarray(r, dtype=dtype)
    th2 = r @ r
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dtype)
    if th2 < 1e-16:
        A, B = 1 - th2 / 6, dtype(0.5) - th2 / 24
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1 - np.cos(th)) / th2
    return np.eye(3, dtype=dtype) + A * K + B * (K @ K)


def view_matrices(view_poses, dtype=np.float64):
    """(C, I, 6) -> (C, I, 3, 4) rows [R | t]; NaN where a pose has a non-finite entry."""
    vp = np.asarray(view_poses, dtype=np.float64)
    C, I = vp.shape[:2]
    M = np.full((C, I, 3, 4), np.nan, dtype=dtype)
    for c in range(C):
        for i in range(I):
            if np.all(np.isfinite(vp[c, i])):
                M[c, i, :, :3] = rodrigues(vp[c, i, :3], dtype)
                M[c, i, :, 3] = vp[c, i, 3:].astype(dtype)
    return M


def compose(A, B):
    """[R | t] of A B for 3 x 4 rigid transforms."""
    out = np.empty((3, 4), dtype=np.result_type(A, B))
    out[:, :3] = A[:, :3] @ B[:, :3]
    out[:, 3] = A[:, :3] @ B[:, 3] + A[:, 3]
    return out


def inverse(A):
    out = np.empty_like(A)
    out[:, :3] = A[:, :3].T
    out[:, 3] = -(A[:, :3].T @ A[:, 3])
    return out


def template_frame(points, dtype=np.float64):
    pts = np.asarray(points, dtype=dtype).reshape(-1, 3)
    pbar = pts.sum(axis=0) / pts.shape[0]
    rho = np.sqrt(np.sum((pts - pbar) ** 2) / pts.shape[0])
    return pbar, rho


def edge_consensus(view_poses, points, dtype=np.float64):
    """Step 1 -> an object with the fields of ``compiled_helpers.EdgeConsensus``."""
    M = view_matrices(view_poses, dtype)
    C, I = M.shape[:2]
    pbar, rho = template_frame(points, dtype)
    have = ~np.isnan(M[:, :, 0, 0])
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    P = len(pairs)
    out = SimpleNamespace(pairs=np.array(pairs, dtype=np.int64).reshape(P, 2), n=np.zeros(P, dtype=np.int64), medoid=np.full(P, -1, dtype=np.int64),
                          T=np.full((P, 3, 4), np.nan, dtype=dtype), sigma=np.full(P, np.nan, dtype=dtype), score=np.full(P, np.nan, dtype=dtype),
                          runner_up=np.full(P, np.nan, dtype=dtype), centroid=pbar, rho=rho)
    for p, (a, b) in enumerate(pairs):
        shared = [i for i in range(I) if have[a, i] and have[b, i]]
        n = len(shared)
        if n == 0:
            continue
        cand = [compose(M[a, i], inverse(M[b, i])) for i in shared]
        m_b = np.zeros(3, dtype=dtype)
        for j in shared:
            m_b = m_b + (M[b, j, :, :3] @ pbar + M[b, j, :, 3])
        m_b = m_b / n
        S = []
        for x, Ti in enumerate(cand):
            s = dtype(0)
            for y, Tj in enumerate(cand):
                if x == y:
                    continue
                dR = Ti[:, :3] - Tj[:, :3]
                w = dR @ m_b + (Ti[:, 3] - Tj[:, 3])
                s = s + np.sqrt(rho * rho / 3 * np.sum(dR * dR) + np.sum(w * w))
            S.append(s)
        S = np.array(S, dtype=dtype)
        k = int(np.argmin(S))                                  # the first of equal minima: the lowest image
        out.n[p], out.medoid[p], out.T[p] = n, shared[k], cand[k]
        out.score[p] = S[k]
        out.sigma[p] = S[k] / (n - 1) if n > 1 else 0
        out.runner_up[p] = np.min(np.delete(S, k)) if n > 1 else np.inf
    return out


def shortest_path_tree(C, pairs, cost, ref_cam):
    """Step 2: textbook Dijkstra on a dense cost matrix -> (parents, cameras in the order they were settled)."""
    w = {}
    for (a, b), c in zip(pairs, cost):
        if np.isfinite(c):
            w[(int(a), int(b))] = w[(int(b), int(a))] = float(c)
    dist, parent, done, order = {ref_cam: 0.0}, {ref_cam: -1}, set(), []
    while True:
        open_ = [(d, c) for c, d in dist.items() if c not in done]
        if not open_:
            break
        d, u = min(open_)                                       # equal distances: the lower camera
        done.add(u)
        order.append(u)
        for v in range(C):
            if v in done or (u, v) not in w:
                continue
            nd = d + w[(u, v)]
            if v not in dist or nd < dist[v] or (nd == dist[v] and u < parent[v]):
                dist[v], parent[v] = nd, u
    return np.array([parent.get(c, -1) for c in range(C)], dtype=np.int64), order


def group_views(dct, n_imgs):
    """Rows sorted by (camera, image, key) -> (sorted table, view ids cam * n_imgs + im, start (n_views + 1))."""
    d = np.asarray(dct, dtype=np.float64)
    order = np.lexsort((d[:, 2], d[:, 1], d[:, 0]))
    d = d[order]
    vid = d[:, 0].astype(np.int64) * n_imgs + d[:, 1].astype(np.int64)
    ids, first = np.unique(vid, return_index=True)
    return d, ids, np.concatenate([first, [d.shape[0]]]).astype(np.int64)


def reprojection_norms(rows, X, P, cam9, dtype):
    """|project(P [X; 1]) - uv| per detection with the legacy cost's formulas (compiled_helpers.py:518-549)."""
    cam9 = np.asarray(cam9, dtype=dtype)
    fx, cx, fy, cy, k0, k1, q0, q1, k2 = cam9
    p = X @ P[:, :3].T + P[:, 3]
    p0, p1 = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    x, y = (p0 - cx) / fx, (p1 - cy) / fy
    r2 = x * x + y * y
    kup = 1 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2)
    xD = x * kup + 2 * q0 * x * y + q1 * (r2 + 2 * x * x)
    yD = y * kup + q0 * (r2 + 2 * y * y) + 2 * q1 * x * y
    eu, ev = (xD * fx + cx) - rows[:, 3].astype(dtype), (yD * fy + cy) - rows[:, 4].astype(dtype)
    return np.sqrt(eu * eu + ev * ev)


def score_candidates(dct, points, intr, view_poses, ext, n_imgs, dtype=np.float64, cost_fn=None):
    """Step 3 up to the error matrix -> (W (C, I, 3, 4), errors (C, I)).  ``cost_fn`` (signature of ``bundle_adjustment_costfn``): the
    residuals come from it, one call per candidate camera over the whole table, instead of from ``reprojection_norms``."""
    M = view_matrices(view_poses, dtype)
    C, I = M.shape[:2]
    E = np.asarray(ext, dtype=dtype).reshape(C, 3, 4)
    pts = np.asarray(points, dtype=dtype).reshape(-1, 3)
    intr = np.asarray(intr, dtype=np.float64)
    W = np.full((C, I, 3, 4), np.nan, dtype=dtype)
    for c in range(C):
        for i in range(I):
            if not np.isnan(M[c, i, 0, 0]):
                W[c, i] = compose(inverse(E[c]), M[c, i])
    Kmat = np.zeros((C, 3, 3), dtype=dtype)
    Kmat[:, 0, 0], Kmat[:, 0, 2], Kmat[:, 1, 1], Kmat[:, 1, 2], Kmat[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1
    proj = Kmat @ E
    ds, ids, start = group_views(dct, I)
    norms = np.full((C, ds.shape[0]), np.nan, dtype=dtype)
    for cp in range(C):
        if cost_fn is not None:
            imlocs = np.einsum("iab,kb->ika", W[cp, :, :, :3], pts) + W[cp, :, None, :, 3]
            r = np.asarray(cost_fn(ds, imlocs.astype(np.float64), proj.astype(np.float64), Kmat.astype(np.float64), np.ascontiguousarray(intr[:, 4:9])))
            norms[cp] = np.sqrt(np.sum(r.reshape(-1, 2) ** 2, axis=1))
            continue
        for k, v in enumerate(ids):
            c, i = divmod(int(v), I)
            if np.isnan(W[cp, i, 0, 0]):
                continue
            rows = ds[start[k]:start[k + 1]]
            X = pts[rows[:, 2].astype(np.int64)] @ W[cp, i, :, :3].T + W[cp, i, :, 3]
            norms[cp, start[k]:start[k + 1]] = reprojection_norms(rows, X, proj[c], intr[c], dtype)
    errors = np.full((C, I), np.nan, dtype=dtype)
    partial = np.full((C, len(ids)), np.nan, dtype=dtype)
    for cp in range(C):
        for k, v in enumerate(ids):                              # views in (camera, image) order: an image's views in view order
            i = int(v) % I
            if np.isnan(W[cp, i, 0, 0]):
                continue
            s = dtype(0)
            for x in norms[cp, start[k]:start[k + 1]]:
                s = s + x
            partial[cp, k] = s
            errors[cp, i] = s if np.isnan(errors[cp, i]) else errors[cp, i] + s
    score_candidates.last_partial = partial
    return W, errors


def seed(dct, points, intr, n_cams, n_imgs, view_poses, ref_cam=0, ref_pose=0, dtype=np.float64, cost_fn=None):
    """Steps 1-4 on given view poses -> a namespace: edges; parents; E (C, 3, 4) before re-basing; W, errors; best_cam (-1: missing),
    missing, per_im_error; extr (C, 3, 4) and poses (I, 3, 4) after re-basing (poses[ref] is exactly [I | 0]); ref: the image whose
    target is the world."""
    C, I = n_cams, n_imgs
    edges = edge_consensus(view_poses, points, dtype)
    cost = np.array([float(edges.sigma[p] + edges.rho / edges.n[p]) if edges.n[p] > 0 else np.inf for p in range(len(edges.n))])
    parents, order = shortest_path_tree(C, edges.pairs, cost, ref_cam)
    lost = [c for c in range(C) if c not in order]
    if lost:
        raise ValueError(f"cameras {lost} are not reachable from camera {ref_cam}")
    index = {(int(a), int(b)): p for p, (a, b) in enumerate(edges.pairs)}
    E = np.zeros((C, 3, 4), dtype=dtype)
    E[ref_cam, :, :3] = np.eye(3)
    dependent = set()   # (c, i): i is the medoid image of the edge c - parent, where W[c, i] repeats W[parent, i]: no candidate of its own
    for c in order[1:]:
        p = int(parents[c])
        T = edges.T[index[(c, p)]] if c < p else inverse(edges.T[index[(p, c)]])
        E[c] = compose(T, E[p])
        dependent.add((c, int(edges.medoid[index[(min(c, p), max(c, p))]])))
    W, errors = score_candidates(dct, points, intr, view_poses, E, I, dtype, cost_fn)
    best_cam, missing, per_im = np.full(I, -1, dtype=np.int64), np.ones(I, dtype=bool), np.full(I, np.nan, dtype=dtype)
    second = np.full(I, np.inf, dtype=dtype)
    for i in range(I):
        fin = [(errors[c, i], c) for c in range(C) if np.isfinite(errors[c, i]) and (c, i) not in dependent]
        if fin:
            fin.sort()
            per_im[i], best_cam[i], missing[i] = fin[0][0], fin[0][1], False
            if len(fin) > 1:
                second[i] = fin[1][0]
    if missing.all():
        raise ValueError("no image has a pose")
    pose = np.zeros((I, 3, 4), dtype=dtype)
    first = int(np.argmin(missing))
    for i in range(I):
        pose[i] = W[best_cam[i], i] if not missing[i] else (pose[i - 1] if i > first else W[best_cam[first], first])
    ref = ref_pose if not missing[ref_pose] else first
    P_ref = pose[ref].copy()
    poses = np.array([compose(inverse(P_ref), pose[i]) for i in range(I)])
    extr = np.array([compose(E[c], P_ref) for c in range(C)])
    poses[ref, :, :3], poses[ref, :, 3] = np.eye(3), 0
    return SimpleNamespace(edges=edges, edge_cost=cost, parents=parents, E=E, W=W, errors=errors, partial=score_candidates.last_partial, best_cam=best_cam,
                           missing=missing, per_im_error=per_im, second_error=second, extr=extr, poses=poses, ref=ref)


def gaps(res):
    """(smallest relative gap between the medoid's score and the runner-up's over the pairs with n >= 3, smallest relative gap between
    the lowest and second lowest candidate error over the images with two finite candidates); inf where there is no such pair / image.
    A pair with n = 2 has no gap to speak of: S_0 = d(T_0, T_1) and S_1 = d(T_1, T_0) are one number, bit for bit (every term of d is a
    square of a difference), so the lower image wins on any machine."""
    e = res.edges
    g_edge = [float((e.runner_up[p] - e.score[p]) / e.runner_up[p]) for p in range(len(e.n)) if e.n[p] >= 3 and e.runner_up[p] > 0]
    g_im = [float((res.second_error[i] - res.per_im_error[i]) / res.second_error[i]) for i in range(len(res.missing))
            if np.isfinite(res.second_error[i]) and res.second_error[i] > 0]
    return min(g_edge, default=np.inf), min(g_im, default=np.inf)
