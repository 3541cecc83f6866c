"""NumPy restatement of the stereo matcher's rule (include/pcs_hip.h, pcs_stereo_*; csrc/ba_stereo.hpp), of the reprojection and of the
compaction.  Everything about the matcher is integer arithmetic: the device is held to bit-equality with ``match``.  ``match_loops``
states the same rule pixel by pixel, straight from the definitions, and is compared with ``match`` on a small crop."""
import numpy as np

NOT_STRICT, TEXTURE, UNIQUENESS, LEFT_RIGHT, VALIDITY = 1, 2, 4, 8, 16
BIG = np.int64(1) << 40
NO_DR = -32768


def prefilter(I, cap):
    I = np.asarray(I).astype(np.int64)
    if cap == 0:
        return I
    H, W = I.shape
    up, dn = I[np.maximum(np.arange(H) - 1, 0)], I[np.minimum(np.arange(H) + 1, H - 1)]
    P = np.full((H, W), cap, dtype=np.int64)
    if W > 2:
        g = (up[:, 2:] - up[:, :-2]) + 2 * (I[:, 2:] - I[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
        P[:, 1:-1] = np.clip(g, -cap, cap) + cap
    return P


def box_sum(A, r):
    """Sum of A over the (2r + 1)^2 window about every pixel whose window lies inside; 0 elsewhere."""
    H, W = A.shape
    out = np.zeros((H, W), dtype=np.int64)
    if H < 2 * r + 1 or W < 2 * r + 1:
        return out
    S = np.zeros((H + 1, W + 1), dtype=np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(A, axis=0), axis=1)
    k = 2 * r + 1
    out[r:H - r, r:W - r] = S[k:, k:] - S[:-k, k:] - S[k:, :-k] + S[:-k, :-k]
    return out


def cost_volume(PL, PR, min_disp, D, r):
    """-> C (D, H, W) int64 and its domain (D, H, W) bool: C[k, y, x] is the cost of d = min_disp + k at the LEFT pixel (y, x)."""
    H, W = PL.shape
    C = np.zeros((D, H, W), dtype=np.int64)
    ok = np.zeros((D, H, W), dtype=bool)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    inside = (ys >= r) & (ys <= H - 1 - r) & (xs >= r) & (xs <= W - 1 - r)
    for k in range(D):
        d = min_disp + k
        AD = np.zeros((H, W), dtype=np.int64)
        lo, hi = max(0, d), min(W, W + d)   # left columns x with 0 <= x - d < W
        if hi > lo:
            AD[:, lo:hi] = np.abs(PL[:, lo:hi] - PR[:, lo - d:hi - d])
        C[k] = box_sum(AD, r)
        ok[k] = inside & (xs - d >= r) & (xs - d <= W - 1 - r)
    return C, ok


def _finish(C_star, m, p, interior):
    den = 2 * (m + p - 2 * C_star)
    use = interior & (den != 0)
    safe = np.where(use, den, 1)
    return np.where(use, np.floor_divide(32 * (m - p) + safe, 2 * safe), 0)


def match(L, R, num_disp, block, min_disp=0, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=15, lr_max_diff=-1, valid=None):
    """-> dict(disp int16, cost int32, status uint8, d_star, offset, strict, C, ok) for one pair (H, W)."""
    D, r, cap = int(num_disp), block // 2, int(prefilter_cap)
    PL, PR = prefilter(L, cap), prefilter(R, cap)
    H, W = PL.shape
    C, ok = cost_volume(PL, PR, min_disp, D, r)
    strict = ok.all(axis=0)
    Cm = np.where(ok, C, BIG)
    k_star = np.argmin(Cm, axis=0)   # the first, i.e. the smallest d, of the smallest cost
    C_star = np.take_along_axis(Cm, k_star[None], axis=0)[0]
    d_star = min_disp + k_star
    status = np.zeros((H, W), dtype=np.int64)
    if cap > 0:
        status |= np.where(box_sum(np.abs(PL - cap), r) < texture_threshold, TEXTURE, 0)
    ks = np.arange(D)[:, None, None]
    if uniqueness_ratio > 0:
        far = np.abs(ks - k_star[None]) >= 2
        c2 = np.where(far & ok, C, BIG).min(axis=0)
        status |= np.where((c2 < BIG) & (100 * c2 <= (100 + uniqueness_ratio) * C_star), UNIQUENESS, 0)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    xr = np.clip(xs - d_star, 0, W - 1)   # in range on every strict pixel
    if lr_max_diff >= 0:
        d_R = right_disparity(Cm, min_disp)
        status |= np.where(np.abs(d_star - d_R[ys, xr]) > lr_max_diff, LEFT_RIGHT, 0)
    if valid is not None:
        vL, vR = (np.asarray(v) for v in valid)
        status |= np.where((vL == 0) | (vR[ys, xr] == 0), VALIDITY, 0)
    interior = (k_star > 0) & (k_star < D - 1)
    m = np.take_along_axis(C, np.clip(k_star - 1, 0, D - 1)[None], axis=0)[0]
    p = np.take_along_axis(C, np.clip(k_star + 1, 0, D - 1)[None], axis=0)[0]
    offset = _finish(C_star, m, p, interior)
    status = np.where(strict, status, NOT_STRICT)
    disp = np.where(status == 0, 16 * d_star + offset, 16 * (min_disp - 1))
    cost = np.where(strict, C_star, -1)
    return dict(disp=disp.astype(np.int16), cost=cost.astype(np.int32), status=status.astype(np.uint8), d_star=d_star, offset=np.where(strict, offset, 0), strict=strict,
                C=C, ok=ok, m=m, p=p)


def right_disparity(Cm, min_disp):
    """d_R (H, W): per RIGHT pixel x2 the smallest d minimising C(y, x2 + d, d) over the d for which it is defined; NO_DR when none is."""
    D, H, W = Cm.shape
    CR = np.full((D, H, W), BIG, dtype=np.int64)
    for k in range(D):
        d = min_disp + k
        lo, hi = max(0, -d), min(W, W - d)   # right columns x2 with 0 <= x2 + d < W
        if hi > lo:
            CR[k][:, lo:hi] = Cm[k][:, lo + d:hi + d]
    k_R = np.argmin(CR, axis=0)
    return np.where(CR.min(axis=0) < BIG, min_disp + k_R, NO_DR)


def match_loops(L, R, num_disp, block, min_disp=0, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=15, lr_max_diff=-1, valid=None):
    """The rule pixel by pixel, every window summed from its definition.  -> (disp, cost, status)."""
    D, r, cap = int(num_disp), block // 2, int(prefilter_cap)
    I = [np.asarray(L).astype(int), np.asarray(R).astype(int)]
    H, W = I[0].shape
    P = []
    for im in I:
        Q = np.zeros((H, W), dtype=int)
        for y in range(H):
            for x in range(W):
                if cap == 0:
                    Q[y, x] = im[y, x]
                elif x == 0 or x == W - 1:
                    Q[y, x] = cap
                else:
                    ym, yp = max(y - 1, 0), min(y + 1, H - 1)
                    g = (im[ym, x + 1] - im[ym, x - 1]) + 2 * (im[y, x + 1] - im[y, x - 1]) + (im[yp, x + 1] - im[yp, x - 1])
                    Q[y, x] = min(max(g, -cap), cap) + cap
        P.append(Q)
    PL, PR = P
    ds = list(range(min_disp, min_disp + D))

    def defined(y, x, d):
        return r <= y <= H - 1 - r and r <= x <= W - 1 - r and r <= x - d <= W - 1 - r

    def cost(y, x, d):
        return int(np.abs(PL[y - r:y + r + 1, x - r:x + r + 1] - PR[y - r:y + r + 1, x - d - r:x - d + r + 1]).sum())

    def d_right(y, x2):
        best = None
        for d in ds:
            if defined(y, x2 + d, d):
                c = cost(y, x2 + d, d)
                if best is None or c < best[0]:
                    best = (c, d)
        return best[1]

    disp = np.full((H, W), 16 * (min_disp - 1), dtype=np.int16)
    cst = np.full((H, W), -1, dtype=np.int32)
    status = np.full((H, W), NOT_STRICT, dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            if not all(defined(y, x, d) for d in ds):
                continue
            costs = [cost(y, x, d) for d in ds]
            c_star = min(costs)
            k = costs.index(c_star)
            d_star = ds[k]
            st = 0
            if cap > 0 and int(np.abs(PL[y - r:y + r + 1, x - r:x + r + 1] - cap).sum()) < texture_threshold:
                st |= TEXTURE
            if uniqueness_ratio > 0 and any(abs(j - k) >= 2 and 100 * costs[j] <= (100 + uniqueness_ratio) * c_star for j in range(D)):
                st |= UNIQUENESS
            if lr_max_diff >= 0 and abs(d_star - d_right(y, x - d_star)) > lr_max_diff:
                st |= LEFT_RIGHT
            if valid is not None and (valid[0][y, x] == 0 or valid[1][y, x - d_star] == 0):
                st |= VALIDITY
            off = 0
            if 0 < k < D - 1:
                m, p = costs[k - 1], costs[k + 1]
                den = 2 * (m + p - 2 * c_star)
                if den != 0:
                    off = (32 * (m - p) + den) // (2 * den)   # Python's // floors
            cst[y, x], status[y, x] = c_star, st
            if st == 0:
                disp[y, x] = 16 * d_star + off
    return disp, cst, status


def match_stack(Ls, Rs, *args, valid=None, **kw):
    """``match`` over (n, H, W) stacks -> (disp, cost, status) stacks."""
    outs = [match(Ls[i], Rs[i], *args, valid=None if valid is None else (valid[0][i], valid[1][i]), **kw) for i in range(len(Ls))]
    return tuple(np.stack([o[k] for o in outs]) for k in ("disp", "cost", "status"))


def reproject(disp, Q, depth_range=None, transform=None, invalid=None, real=np.float64):
    """(X, Y, Z, Wh) = Q (x, y, disp / 16, 1), point = (X, Y, Z) / Wh, in the arithmetic ``real`` (float64 or longdouble), the sums taken
    left to right.  ``disp`` (n, H, W) int16, ``Q`` (4, 4) or (n, 4, 4).  -> points (n, H, W, 3) of ``real`` (NaN where the mask is 0),
    mask (n, H, W) uint8, z (n, H, W) before the transform."""
    disp = np.asarray(disp)
    n, H, W = disp.shape
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (n, 4, 4)).astype(real)
    x = np.arange(W, dtype=real)[None, None, :]
    y = np.arange(H, dtype=real)[None, :, None]
    d = disp.astype(real) / real(16)
    q = lambda i, j: Q[:, i, j][:, None, None]
    rows = [((q(i, 0) * x + q(i, 1) * y) + q(i, 2) * d) + q(i, 3) for i in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        pts = np.stack([rows[0] / rows[3], rows[1] / rows[3], rows[2] / rows[3]], axis=-1)
    z = pts[..., 2].copy()
    lo, hi = (-np.inf, np.inf) if depth_range is None else depth_range
    mask = np.all(np.isfinite(pts), axis=-1) & (z >= lo) & (z <= hi)
    if invalid is not None:
        mask &= disp != invalid
    if transform is not None:
        T = np.asarray(transform, dtype=np.float64).astype(real)
        with np.errstate(invalid="ignore"):
            pts = np.stack([((T[i, 0] * pts[..., 0] + T[i, 1] * pts[..., 1]) + T[i, 2] * pts[..., 2]) + T[i, 3] for i in range(3)], axis=-1)
    pts = np.where(mask[..., None], pts, real(np.nan))
    return pts, mask.astype(np.uint8), z


def compact(points, mask, values=None):
    """Per pair the masked points (and values) in row-major pixel order."""
    out = []
    for i in range(points.shape[0]):
        idx = np.flatnonzero(mask[i])
        p = points[i].reshape(-1, 3)[idx]
        out.append(p if values is None else (p, values[i].reshape(-1)[idx]))
    return out
