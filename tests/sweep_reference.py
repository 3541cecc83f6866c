"""NumPy restatement of the plane sweep's rule (include/pcs_hip.h, "Plane-sweep multi-view depth"; csrc/ba_sweep.hpp).  The warp is
float64 in the order the header writes; everything behind the rounding to sixteenths is integer arithmetic, so the device is held to
bit-equality with ``sweep``.  ``sweep_loops`` states the same rule as a plain loop over (pixel, plane, neighbour), straight from the
definitions with Python scalars, and must agree with ``sweep`` exactly.  ``decision_margins`` measures how far the inputs keep from the
two floating-point decisions of the rule (the rounding to a sixteenth, the sign of n_2) and how far float64 is from longdouble there."""
import math

import numpy as np

from tests.sgm_reference import census, popcount
from tests.stereo_reference import _finish

NOT_STRICT, NO_VIEW, UNIQUENESS = 1, 2, 4
BIG = 1 << 40


def lists_of(neighbours, V):
    if isinstance(neighbours, tuple) and len(neighbours) == 2 and len(neighbours[0]) == V + 1 and np.ndim(neighbours[0]) == 1:
        start, nbr = neighbours
        return [[int(j) for j in nbr[start[v]:start[v + 1]]] for v in range(V)]
    return [[int(j) for j in l] for l in neighbours]


def warp_table(Ki, Pi, Kj, Pj, dtype=np.float64):
    """Step 1, the host's part: -> (A (3, 3), b (3,)) of ``dtype``, every operation in the order of the header."""
    T = dtype
    Ki, Kj = [T(v) for v in Ki], [T(v) for v in Kj]
    Pi, Pj = np.asarray(Pi).reshape(3, 4), np.asarray(Pj).reshape(3, 4)
    Ri, ti = [[T(v) for v in row[:3]] for row in Pi], [T(row[3]) for row in Pi]
    Rj, tj = [[T(v) for v in row[:3]] for row in Pj], [T(row[3]) for row in Pj]
    M = [[(Rj[a][0] * Ri[b][0] + Rj[a][1] * Ri[b][1]) + Rj[a][2] * Ri[b][2] for b in range(3)] for a in range(3)]
    c = [tj[a] - ((M[a][0] * ti[0] + M[a][1] * ti[1]) + M[a][2] * ti[2]) for a in range(3)]
    N = [[Kj[0] * M[0][b] + Kj[1] * M[2][b] for b in range(3)], [Kj[2] * M[1][b] + Kj[3] * M[2][b] for b in range(3)], [M[2][b] for b in range(3)]]
    A = np.zeros((3, 3), dtype=T)
    for a in range(3):
        A[a, 0] = N[a][0] / Ki[0]
        A[a, 1] = N[a][1] / Ki[2]
        A[a, 2] = (N[a][2] - A[a, 0] * Ki[1]) - A[a, 1] * Ki[3]
    b = np.array([Kj[0] * c[0] + Kj[1] * c[2], Kj[2] * c[1] + Kj[3] * c[2], c[2]], dtype=T)
    return A, b


def project(A, b, z, xs, ys):
    """Step 1, the device's part -> (n_2, 16 u + 0.5, 16 v + 0.5) in the dtype of the arguments."""
    T = A.dtype.type
    n = [T(z) * ((A[a, 0] * xs + A[a, 1] * ys) + A[a, 2]) + b[a] for a in range(3)]
    with np.errstate(all="ignore"):
        u, v = n[0] / n[2], n[1] / n[2]
        return n[2], T(16) * u + T(0.5), T(16) * v + T(0.5)


def sample(I, A, b, z):
    """Step 2 for every pixel of the reference view -> (g int64 (H, W), valid bool)."""
    H, W = I.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    n2, tu, tv = project(A, b, z, xs, ys)
    with np.errstate(all="ignore"):
        qu, qv = np.floor(tu), np.floor(tv)
        valid = (n2 > 0) & (qu >= 0) & (qu < 16 * (W - 1)) & (qv >= 0) & (qv < 16 * (H - 1))   # a comparison with a NaN is False
    iu, iv = np.where(valid, qu, 0).astype(np.int64), np.where(valid, qv, 0).astype(np.int64)
    x0, fx, y0, fy = iu >> 4, iu & 15, iv >> 4, iv & 15
    J = I.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)   # in range wherever valid; clipped for the rest
    g = (16 - fx) * (16 - fy) * J[y0, x0] + fx * (16 - fy) * J[y0, x1] + (16 - fx) * fy * J[y1, x0] + fx * fy * J[y1, x1]
    return np.where(valid, g, 0), valid


def _window(a, rx, ry, reduce):
    """``reduce`` over the (2 rx + 1) x (2 ry + 1) window about every pixel whose window lies inside; -> (result, inside)."""
    H, W = a.shape
    inside = np.zeros((H, W), dtype=bool)
    out = np.zeros((H, W), dtype=a.dtype)
    if H < 2 * ry + 1 or W < 2 * rx + 1:
        return out, inside
    inside[ry:H - ry, rx:W - rx] = True
    acc = None
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            part = a[ry + j:H - ry + j, rx + i:W - rx + i]
            acc = part.copy() if acc is None else reduce(acc, part)
    out[ry:H - ry, rx:W - rx] = acc
    return out, inside


def strict_mask(W, H, cw, ch, r):
    m = np.zeros((H, W), dtype=bool)
    rw, rh = cw // 2, ch // 2
    if H - rh - r > rh + r and W - rw - r > rw + r:
        m[rh + r:H - rh - r, rw + r:W - rw - r] = True
    return m


def view_costs(images, K, P, i, lst, zrow, cw, ch, r, tau):
    """Steps 1 to 4 for reference view i -> C (D, H, W) int64 (meaningful on the strict pixels)."""
    H, W = images[i].shape
    rw, rh = cw // 2, ch // 2
    ref, _ = census(images[i], cw, ch)
    C = np.zeros((len(zrow), H, W), dtype=np.int64)
    warps = [warp_table(K[i], P[i], K[j], P[j]) for j in lst]
    for k, z in enumerate(zrow):
        for j, (A, b) in zip(lst, warps):
            g, valid = sample(images[j], A, b, z)
            desc, _ = census(g, cw, ch)
            ok, inside = _window(valid, rw, rh, np.logical_and)
            ok &= inside
            h = np.where(ok, popcount(desc ^ ref), 0)
            okb, inb = _window(ok, r, r, np.logical_and)
            s, _ = _window(h, r, r, np.add)
            C[k] += np.where(okb & inb, np.minimum(s, tau), tau)
    return C


def decide(C, strict, zrow, tau, n_list, uniq):
    """Step 5 -> (depth float64, level int32, cost int32, status uint8) of one view."""
    D = C.shape[0]
    k_star = np.argmin(C, axis=0)   # the first, i.e. the smallest k, of the smallest cost
    C_star = np.take_along_axis(C, k_star[None], axis=0)[0]
    interior = (k_star > 0) & (k_star < D - 1)
    m = np.take_along_axis(C, np.clip(k_star - 1, 0, D - 1)[None], axis=0)[0]
    p = np.take_along_axis(C, np.clip(k_star + 1, 0, D - 1)[None], axis=0)[0]
    f = _finish(C_star, m, p, interior)
    status = np.where(C_star >= tau * n_list, NO_VIEW, 0)
    if uniq > 0:
        far = np.abs(np.arange(D)[:, None, None] - k_star[None]) >= 2
        c2 = np.where(far, C, BIG).min(axis=0)
        status = np.where((status == 0) & (c2 < BIG) & (100 * c2 <= (100 + uniq) * C_star), UNIQUENESS, status)
    status = np.where(strict, status, NOT_STRICT)
    zs = zrow[k_star]
    zn = zrow[np.clip(k_star + np.sign(f), 0, D - 1)]
    depth = zs + (np.abs(f) / 16.0) * (zn - zs)
    depth = np.where(status == 0, depth, np.nan)
    level = np.where(strict, 16 * k_star + f, -16)
    cost = np.where(strict, C_star, -1)
    return depth, level.astype(np.int32), cost.astype(np.int32), status.astype(np.uint8)


def sweep(images, K, ext, neighbours, planes, census=(5, 5), box=2, truncate=None, uniqueness_ratio=0):
    """-> dict(depth float64 (V, H, W), level int32, cost int32, status uint8)."""
    images = np.asarray(images)
    V, H, W = images.shape
    cw, ch = census
    tau = (cw * ch - 1) * (2 * box + 1) ** 2 // 4 if truncate is None else int(truncate)
    K, P = np.asarray(K, dtype=np.float64), np.asarray(ext, dtype=np.float64).reshape(V, 12)
    z = np.asarray(planes, dtype=np.float64)
    z = z[None] if z.ndim == 1 else z
    lists = lists_of(neighbours, V)
    strict = strict_mask(W, H, cw, ch, box)
    out = dict(depth=np.zeros((V, H, W)), level=np.zeros((V, H, W), np.int32), cost=np.zeros((V, H, W), np.int32), status=np.zeros((V, H, W), np.uint8))
    for i in range(V):
        zrow = z[i if z.shape[0] > 1 else 0]
        C = view_costs(images, K, P, i, lists[i], zrow, cw, ch, box, tau)
        out["depth"][i], out["level"][i], out["cost"][i], out["status"][i] = decide(C, strict, zrow, tau, len(lists[i]), int(uniqueness_ratio))
    return out


def sweep_loops(images, K, ext, neighbours, planes, census=(5, 5), box=2, truncate=None, uniqueness_ratio=0):
    """The rule as a plain loop over (pixel, plane, neighbour) with Python scalars (IEEE doubles and unbounded integers)."""
    images = np.asarray(images)
    V, H, W = images.shape
    cw, ch = census
    rw, rh, r = cw // 2, ch // 2, box
    tau = (cw * ch - 1) * (2 * r + 1) ** 2 // 4 if truncate is None else int(truncate)
    K, P = np.asarray(K, dtype=np.float64), np.asarray(ext, dtype=np.float64).reshape(V, 12)
    z = np.asarray(planes, dtype=np.float64)
    z = z[None] if z.ndim == 1 else z
    D = z.shape[1]
    lists = lists_of(neighbours, V)
    I = [[[int(v) for v in row] for row in img] for img in images]
    out = dict(depth=np.full((V, H, W), np.nan), level=np.full((V, H, W), -16, np.int32), cost=np.full((V, H, W), -1, np.int32), status=np.full((V, H, W), NOT_STRICT, np.uint8))
    offsets = [(dx, dy) for dy in range(-rh, rh + 1) for dx in range(-rw, rw + 1) if (dx, dy) != (0, 0)]
    for i in range(V):
        zrow = [float(v) for v in z[i if z.shape[0] > 1 else 0]]
        warps = {}
        for j in lists[i]:
            A, b = warp_table(K[i], P[i], K[j], P[j])
            warps[j] = ([[float(v) for v in row] for row in A], [float(v) for v in b])
        samples, hammings = {}, {}

        def g_of(j, k, x, y):
            """the warped sample, None where invalid"""
            key = (j, k, x, y)
            if key not in samples:
                A, b = warps[j]
                n = [zrow[k] * ((A[a][0] * x + A[a][1] * y) + A[a][2]) + b[a] for a in range(3)]
                val = None
                tu, tv = (16.0 * (n[0] / n[2]) + 0.5, 16.0 * (n[1] / n[2]) + 0.5) if n[2] > 0 else (math.nan, math.nan)
                if math.isfinite(tu) and math.isfinite(tv):   # an infinite coordinate lies outside, a NaN fails every comparison
                    qu, qv = math.floor(tu), math.floor(tv)
                    if 0 <= qu < 16 * (W - 1) and 0 <= qv < 16 * (H - 1):
                        x0, fx, y0, fy = qu >> 4, qu & 15, qv >> 4, qv & 15
                        Ij = I[j]
                        val = (16 - fx) * (16 - fy) * Ij[y0][x0] + fx * (16 - fy) * Ij[y0][x0 + 1] + (16 - fx) * fy * Ij[y0 + 1][x0] + fx * fy * Ij[y0 + 1][x0 + 1]
                samples[key] = val
            return samples[key]

        def h_of(j, k, x, y):
            """the Hamming distance of the two descriptors at (x, y), None where the warped one is invalid"""
            key = (j, k, x, y)
            if key not in hammings:
                centre = g_of(j, k, x, y)
                h = None if centre is None else 0
                for dx, dy in offsets:
                    if h is None:
                        break
                    g = g_of(j, k, x + dx, y + dy)
                    if g is None:
                        h = None
                    else:
                        h += int(g < centre) != int(I[i][y + dy][x + dx] < I[i][y][x])
                hammings[key] = h
            return hammings[key]

        for y in range(rh + r, H - rh - r):
            for x in range(rw + r, W - rw - r):
                C = []
                for k in range(D):
                    total = 0
                    for j in lists[i]:
                        hs = [h_of(j, k, x + bx, y + by) for by in range(-r, r + 1) for bx in range(-r, r + 1)]
                        total += tau if any(h is None for h in hs) else min(tau, sum(hs))
                    C.append(total)
                ks = min(range(D), key=lambda k: (C[k], k))
                f = 0
                if 0 < ks < D - 1:
                    den = 2 * (C[ks - 1] + C[ks + 1] - 2 * C[ks])
                    if den != 0:
                        f = (32 * (C[ks - 1] - C[ks + 1]) + den) // (2 * den)
                status = 0
                if C[ks] >= tau * len(lists[i]):
                    status = NO_VIEW
                elif uniqueness_ratio > 0 and any(100 * C[k] <= (100 + uniqueness_ratio) * C[ks] for k in range(D) if abs(k - ks) >= 2):
                    status = UNIQUENESS
                out["level"][i, y, x], out["cost"][i, y, x], out["status"][i, y, x] = 16 * ks + f, C[ks], status
                if status == 0:
                    zn = zrow[ks + (1 if f > 0 else -1 if f < 0 else 0)]
                    out["depth"][i, y, x] = zrow[ks] + (abs(f) / 16.0) * (zn - zrow[ks])
    return out


def decision_margins(images, K, ext, neighbours, planes, **_):
    """Over every (view, neighbour, plane, pixel): how close 16 u + 0.5 and 16 v + 0.5 come to an integer and n_2 to 0, and how far
    float64 is from longdouble in the same quantities.  The roundings are looked at where they can decide anything: on samples with
    n_2 > 0 whose 16 u + 0.5 lies in [-1, 16 W] and 16 v + 0.5 in [-1, 16 H]; a sample further outside is invalid whichever way its
    rounding goes.  -> dict(closest_t, gap_t (sixteenths), closest_n2, gap_n2)."""
    images = np.asarray(images)
    V, H, W = images.shape
    K, P = np.asarray(K, dtype=np.float64), np.asarray(ext, dtype=np.float64).reshape(V, 12)
    z = np.asarray(planes, dtype=np.float64)
    z = z[None] if z.ndim == 1 else z
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xl, yl = xs.astype(np.longdouble), ys.astype(np.longdouble)
    res = dict(closest_t=np.inf, gap_t=0.0, closest_n2=np.inf, gap_n2=0.0)
    for i, lst in enumerate(lists_of(neighbours, V)):
        for j in lst:
            A, b = warp_table(K[i], P[i], K[j], P[j])
            Al, bl = warp_table(K[i], P[i], K[j], P[j], np.longdouble)
            for zk in z[i if z.shape[0] > 1 else 0]:
                n2, tu, tv = project(A, b, zk, xs, ys)
                n2l, tul, tvl = project(Al, bl, zk, xl, yl)
                res["closest_n2"] = min(res["closest_n2"], float(np.min(np.abs(n2))))
                res["gap_n2"] = max(res["gap_n2"], float(np.max(np.abs(n2 - n2l))))
                with np.errstate(all="ignore"):
                    near = (n2 > 0) & (tu >= -1) & (tu <= 16 * W) & (tv >= -1) & (tv <= 16 * H)
                if near.any():
                    for t, tl in ((tu[near], tul[near]), (tv[near], tvl[near])):
                        res["closest_t"] = min(res["closest_t"], float(np.min(np.abs(t - np.rint(t)))))
                        res["gap_t"] = max(res["gap_t"], float(np.max(np.abs(t - tl))))
    return res
