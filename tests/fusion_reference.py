"""The depth-map fusion rule of include/pcs_hip.h ("Depth-map fusion", csrc/ba_fusion.hpp) restated in NumPy: TEST INFRASTRUCTURE.

Two forms of the same rule: ``fuse`` works on whole maps with masks, ``fuse_loop`` walks pixel by pixel with early exits and plain
indexing.  Both take the arithmetic type (float64 or ``np.longdouble``) and share only the four formulas below, which are written once
in the order the header states (plain IEEE operations, sums of three products left to right), so the two forms agree bit for bit.

Both also return the CLOSEST CALL: over every decision taken, the smallest distance to its threshold, each relative to the quantity's
scale.  The decisions, in the order a neighbour meets them (a later one is taken only when the earlier ones passed):
  sign of Y_z          |Y_z| / (|R20 X0| + |R21 X1| + |R22 X2| + |t2|)
  rounding             the distance of u + 0.5 (and v + 0.5) to the nearest integer, / s_u = |fx| max(|Y_x / Y_z|, 1) + |cx| (s_v alike)
  image bounds         the distance of u + 0.5 to 0 and W (v + 0.5 to 0 and H), / W (H)
  sign of Y'_z         as Y_z, with view i's row
  pixel tolerance      |d - px_tol| / max(s_x', s_y'), d = sqrt((x' - x)^2 + (y' - y)^2)
  depth tolerance      ||Y'_z - z| - rel_tol z| / max(|Y'_z|, z)
``fuse`` returns the quantities themselves too (``decisions``, each divided by its scale, NaN where the decision was not taken), from
which tests/fusion_inputs.py measures FUSE_DECISION_GAP."""
import numpy as np

INVALID_DEPTH, FEW_VIEWS, DUPLICATE = 1, 2, 4
MAX_NEIGHBOURS = 32


def as_csr(neighbours):
    """A list of index sequences or a (nbr_start, nbr) pair -> (nbr_start int32 (V + 1), nbr int32)."""
    if isinstance(neighbours, tuple) and len(neighbours) == 2 and np.ndim(neighbours[0]) == 1 and np.ndim(neighbours[1]) == 1 and len(neighbours[0]) > 0 \
            and len(neighbours[1]) == np.asarray(neighbours[0])[-1]:
        return np.asarray(neighbours[0], dtype=np.int32), np.asarray(neighbours[1], dtype=np.int32)
    lens = [len(l) for l in neighbours]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nbr = np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in neighbours] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return start, nbr


def valid_depth(z):
    return np.isfinite(z) & (z > 0)


def to_world(K, P, x, y, z):
    """X = R^T (z ((x - cx) / fx, (y - cy) / fy, 1) - t); K = [fx, cx, fy, cy], P = [R | t] row-major (12)."""
    c0 = z * ((x - K[1]) / K[0]) - P[3]
    c1 = z * ((y - K[3]) / K[2]) - P[7]
    c2 = z - P[11]
    return (P[0] * c0 + P[4] * c1) + P[8] * c2, (P[1] * c0 + P[5] * c1) + P[9] * c2, (P[2] * c0 + P[6] * c1) + P[10] * c2


def to_view(P, X0, X1, X2):
    """Y = R X + t"""
    return ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3], ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7], ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11]


def project(K, Y0, Y1, Y2):
    return K[0] * (Y0 / Y2) + K[1], K[2] * (Y1 / Y2) + K[3]


def pixel_scale(K, Y0, Y1, Y2):
    """The scale of the projection (u, v) of Y: the magnitudes its terms reach, |fx| max(|Y0 / Y2|, 1) + |cx| and the same for v."""
    return np.abs(K[0]) * np.maximum(np.abs(Y0 / Y2), 1) + np.abs(K[1]), np.abs(K[2]) * np.maximum(np.abs(Y1 / Y2), 1) + np.abs(K[3])


def z_scale(P, X0, X1, X2):
    return np.abs(P[8] * X0) + np.abs(P[9] * X1) + np.abs(P[10] * X2) + np.abs(P[11])


def _prepare(depth, K, ext, neighbours, transform, dtype):
    T = np.dtype(dtype).type
    D = np.asarray(depth)
    assert D.ndim == 3 and D.dtype in (np.float32, np.float64)
    V = D.shape[0]
    Kt = np.asarray(K, dtype=np.float64).reshape(V, 4).astype(T)
    Pt = np.asarray(ext, dtype=np.float64).reshape(V, 12).astype(T)
    start, nbr = as_csr(neighbours)
    assert len(start) == V + 1
    Tm = None if transform is None else np.asarray(transform, dtype=np.float64)[:3].reshape(12).astype(T)
    return T, D.astype(T), Kt, Pt, start, nbr, Tm


def _finish(T, V, H, W, valid, support, X, S, Pt, Tm, min_views, unique, partners, start, nbr):
    """Steps 3 to 6 on whole maps (shared: they hold no floating-point decision)."""
    count = np.zeros((V, H, W), dtype=np.uint8)
    for b in range(MAX_NEIGHBOURS):
        count += ((support >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    kept = valid & (count >= min_views)
    status = np.where(~valid, INVALID_DEPTH, np.where(kept, 0, FEW_VIEWS)).astype(np.uint8)
    if unique:
        dup = np.zeros_like(kept)
        for i in range(V):
            for k in range(start[i], start[i + 1]):
                j = int(nbr[k])
                if j >= i:
                    continue
                bit = ((support[i] >> np.uint32(k - start[i])) & np.uint32(1)).astype(bool)
                qx, qy = partners[k]
                dup[i] |= kept[i] & bit & kept[j][qy, qx]
        status[dup] = DUPLICATE
    mask = status == 0
    m = (count.astype(np.int64) + 1).astype(T)
    F = np.stack([S[..., c] / m for c in range(3)], axis=-1)
    with np.errstate(all="ignore"):
        fz = np.stack([to_view(Pt[i], F[i, ..., 0], F[i, ..., 1], F[i, ..., 2])[2] for i in range(V)])
        if Tm is not None:
            F = np.stack(to_view(Tm, F[..., 0], F[..., 1], F[..., 2]), axis=-1)
    nan = T(np.nan)
    points = np.where(mask[..., None], F, nan)
    return dict(points=points, fused_depth=np.where(mask, fz, nan), mask=mask.astype(np.uint8), count=count, support=support, status=status,
                counts=mask.reshape(V, -1).sum(axis=1).astype(np.int64))


def fuse(depth, K, ext, neighbours, px_tol=1.0, rel_tol=0.01, min_views=2, unique=False, transform=None, dtype=np.float64):
    """The vectorised form.  depth (V, H, W) float32 / float64; K (V, 4); ext (V, 3, 4) or (V, 12).  -> dict(points (V, H, W, 3) and
    fused_depth of ``dtype`` (not rounded to float32), mask, count, support, status, counts, closest, decisions)."""
    T, D, Kt, Pt, start, nbr, Tm = _prepare(depth, K, ext, neighbours, transform, dtype)
    V, H, W = D.shape
    half, tol, rel = T(0.5), T(px_tol), T(rel_tol)
    tol2 = tol * tol
    xs, ys = np.meshgrid(np.arange(W).astype(T), np.arange(H).astype(T))
    valid = valid_depth(D)
    support = np.zeros((V, H, W), dtype=np.uint32)
    X = np.zeros((V, H, W, 3), dtype=T)
    S = np.zeros((V, H, W, 3), dtype=T)
    E = len(nbr)
    dec = np.full((6, E, H, W), np.nan, dtype=T)
    partners = [None] * E
    closest = np.inf

    def near(a, reached):
        nonlocal closest
        a = np.asarray(a, dtype=np.float64)[reached]
        if a.size:
            closest = min(closest, float(np.min(a)))

    with np.errstate(all="ignore"):
        for i in range(V):
            z = D[i]
            X0, X1, X2 = to_world(Kt[i], Pt[i], xs, ys, z)
            X[i] = np.stack([X0, X1, X2], axis=-1)
            S0, S1, S2 = X0, X1, X2
            for k in range(start[i], start[i + 1]):
                j = int(nbr[k])
                Y0, Y1, Y2 = to_view(Pt[j], X0, X1, X2)
                s1 = z_scale(Pt[j], X0, X1, X2)
                dec[0, k] = np.where(valid[i], Y2 / s1, np.nan)
                near(np.abs(Y2) / s1, valid[i])
                ok = valid[i] & (Y2 > 0)
                u, v = project(Kt[j], Y0, Y1, Y2)
                ur, vr = u + half, v + half
                su, sv = pixel_scale(Kt[j], Y0, Y1, Y2)
                dec[1, k], dec[2, k] = np.where(ok, ur / su, np.nan), np.where(ok, vr / sv, np.nan)
                near(np.abs(ur - np.rint(ur)) / su, ok)
                near(np.abs(vr - np.rint(vr)) / sv, ok)
                near(np.minimum(np.abs(ur), np.abs(ur - W)) / W, ok)
                near(np.minimum(np.abs(vr), np.abs(vr - H)) / H, ok)
                fu, fv = np.floor(ur), np.floor(vr)
                ok = ok & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
                qx, qy = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
                partners[k] = (qx, qy)
                zj = np.where(ok, D[j][qy, qx], 0)
                ok = ok & valid_depth(zj)
                P0, P1, P2 = to_world(Kt[j], Pt[j], qx.astype(T), qy.astype(T), zj)
                B0, B1, B2 = to_view(Pt[i], P0, P1, P2)
                s4 = z_scale(Pt[i], P0, P1, P2)
                dec[3, k] = np.where(ok, B2 / s4, np.nan)
                near(np.abs(B2) / s4, ok)
                ok = ok & (B2 > 0)
                xr, yr = project(Kt[i], B0, B1, B2)
                dx, dy = xr - xs, yr - ys
                d2 = dx * dx + dy * dy
                sp = np.maximum(*pixel_scale(Kt[i], B0, B1, B2))
                sd = np.maximum(np.abs(B2), z)
                dq = np.abs(B2 - z) - rel * z
                dec[4, k], dec[5, k] = np.where(ok, np.sqrt(d2) / sp, np.nan), np.where(ok, dq / sd, np.nan)
                near(np.abs(np.sqrt(d2) - tol) / sp, ok)
                near(np.abs(dq) / sd, ok)
                ok = ok & (d2 <= tol2) & (np.abs(B2 - z) <= rel * z)
                support[i] |= np.where(ok, np.uint32(1) << np.uint32(k - start[i]), np.uint32(0)).astype(np.uint32)
                S0, S1, S2 = np.where(ok, S0 + P0, S0), np.where(ok, S1 + P1, S1), np.where(ok, S2 + P2, S2)
            S[i] = np.stack([S0, S1, S2], axis=-1)
    out = _finish(T, V, H, W, valid, support, X, S, Pt, Tm, min_views, unique, partners, start, nbr)
    out.update(closest=closest, decisions=dec, surface=X)
    return out


def fuse_loop(depth, K, ext, neighbours, px_tol=1.0, rel_tol=0.01, min_views=2, unique=False, transform=None, dtype=np.float64):
    """The plain loop form: one pixel, one neighbour at a time, leaving at the first failed step."""
    T, D, Kt, Pt, start, nbr, Tm = _prepare(depth, K, ext, neighbours, transform, dtype)
    V, H, W = D.shape
    half, tol, rel = T(0.5), T(px_tol), T(rel_tol)
    tol2 = tol * tol
    valid = np.zeros((V, H, W), dtype=bool)
    support = np.zeros((V, H, W), dtype=np.uint32)
    count = np.zeros((V, H, W), dtype=np.uint8)
    F = np.full((V, H, W, 3), np.nan, dtype=T)
    fz = np.full((V, H, W), np.nan, dtype=T)
    partner = {}
    closest = np.inf
    with np.errstate(all="ignore"):
        for i in range(V):
            for y in range(H):
                for x in range(W):
                    z = D[i, y, x]
                    if not (np.isfinite(z) and z > 0):
                        continue
                    valid[i, y, x] = True
                    xt, yt = T(x), T(y)
                    X = to_world(Kt[i], Pt[i], xt, yt, z)
                    S = X
                    bits = 0
                    for k in range(start[i], start[i + 1]):
                        j = int(nbr[k])
                        Y = to_view(Pt[j], *X)
                        closest = min(closest, float(np.abs(Y[2]) / z_scale(Pt[j], *X)))
                        if not Y[2] > 0:
                            continue
                        u, v = project(Kt[j], *Y)
                        ur, vr = u + half, v + half
                        su, sv = pixel_scale(Kt[j], *Y)
                        closest = min(closest, float(np.abs(ur - np.rint(ur)) / su), float(np.abs(vr - np.rint(vr)) / sv),
                                      float(min(np.abs(ur), np.abs(ur - W)) / W), float(min(np.abs(vr), np.abs(vr - H)) / H))
                        fu, fv = np.floor(ur), np.floor(vr)
                        if not (0 <= fu < W and 0 <= fv < H):
                            continue
                        qx, qy = int(fu), int(fv)
                        zj = D[j, qy, qx]
                        if not (np.isfinite(zj) and zj > 0):
                            continue
                        Pw = to_world(Kt[j], Pt[j], T(qx), T(qy), zj)
                        B = to_view(Pt[i], *Pw)
                        closest = min(closest, float(np.abs(B[2]) / z_scale(Pt[i], *Pw)))
                        if not B[2] > 0:
                            continue
                        xr, yr = project(Kt[i], *B)
                        dx, dy = xr - xt, yr - yt
                        d2 = dx * dx + dy * dy
                        sp, sd = max(*pixel_scale(Kt[i], *B)), max(np.abs(B[2]), z)
                        closest = min(closest, float(np.abs(np.sqrt(d2) - tol) / sp), float(np.abs(np.abs(B[2] - z) - rel * z) / sd))
                        if not (d2 <= tol2 and np.abs(B[2] - z) <= rel * z):
                            continue
                        bits |= 1 << (k - start[i])
                        partner[(i, y, x, k)] = (j, qy, qx)
                        S = (S[0] + Pw[0], S[1] + Pw[1], S[2] + Pw[2])
                    support[i, y, x] = bits
                    c = bin(bits).count("1")
                    count[i, y, x] = c
                    m = T(c + 1)
                    f = (S[0] / m, S[1] / m, S[2] / m)
                    fz[i, y, x] = to_view(Pt[i], *f)[2]
                    F[i, y, x] = f if Tm is None else to_view(Tm, *f)
    kept = valid & (count >= min_views)
    status = np.where(~valid, INVALID_DEPTH, np.where(kept, 0, FEW_VIEWS)).astype(np.uint8)
    if unique:
        for (i, y, x, k), (j, qy, qx) in partner.items():
            if j < i and kept[i, y, x] and kept[j, qy, qx]:
                status[i, y, x] = DUPLICATE
    mask = status == 0
    nan = T(np.nan)
    return dict(points=np.where(mask[..., None], F, nan), fused_depth=np.where(mask, fz, nan), mask=mask.astype(np.uint8), count=count, support=support, status=status,
                counts=mask.reshape(V, -1).sum(axis=1).astype(np.int64), closest=closest)


def compact(points, mask, values=None):
    """The masked points per view in row-major pixel order, with the values when given."""
    out = []
    for i in range(mask.shape[0]):
        idx = np.flatnonzero(mask[i])
        p = points[i].reshape(-1, 3)[idx]
        out.append(p if values is None else (p, values[i].reshape(-1)[idx]))
    return out


def view_neighbours(view_vectors, min_angle, max_angle, max_views):
    """The rule of pycamset_amd.fusion.view_neighbours on unit view vectors, one view at a time (for the tie test)."""
    v = np.asarray(view_vectors, dtype=np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    out = []
    for i in range(len(v)):
        cand = []
        for j in range(len(v)):
            a = np.degrees(np.arccos(np.clip(v[i] @ v[j], -1.0, 1.0)))
            if j != i and min_angle < a < max_angle:
                cand.append((a, j))
        if len(cand) >= max_views:   # fewer: index order, as the reference returns them
            cand = sorted(cand)[:max_views]
        out.append([j for _, j in cand])
    return out
