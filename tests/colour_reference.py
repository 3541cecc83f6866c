"""The colour rule of include/pcs_hip.h ("Colour of surface points from the images", csrc/ba_tsdf_colour.hpp) restated in NumPy: TEST
INFRASTRUCTURE.

Two forms of the same rule, as tests/raycast_reference.py has them.  ``colour`` works on all points at once with masks and takes the
arithmetic type (float64 or ``np.longdouble``); ``colour_point`` handles ONE point with early exits and Python floats (IEEE doubles).
Every formula is written in the order the header states, so the two forms agree bit for bit in float64.  ``point_normals`` /
``point_normal`` do the same for the cast's normal rule at arbitrary points, through the sample function of tests/raycast_reference.py.

Both return the CLOSEST CALL per point: over every decision the point took, the smallest distance to its threshold, each relative to
the quantity's scale.  A decision counts once the decisions before it have passed.  In the order a (point, view) pair meets them:
  Y_2 > 0                Y_2 / max(((|R_20 X_0| + |R_21 X_1|) + |R_22 X_2|) + |t_2|, 1)
  in the image           min(min(u, (W - 1) - u) / su, min(w, (H - 1) - w) / sw) with su = max(|u|, W), sw = max(|w|, H)
  the two floors         the distance of u (w) to the nearest integer m, when 0 < m < W - 1 (H - 1), else 0.5, / su (sw).  At the ends
                         the clamp picks the same cell from both sides.
  the nearest pixel      the distance of u + 0.5 (w + 0.5) to the nearest integer, / su (sw); with visibility maps
  visibility             ((d + tol) - Y_2) / max(|d| + tol, |Y_2|) for a valid d
  c > cos_min            c - cos_min; with normals
and per point:
  the best view          the difference of the two largest c, when two views or more contribute; with normals (without, every c is 1
                         exactly and the tie rule decides)
  the uint8 rounding     per channel the distance of the colour to the nearest k + 0.5, / max(|colour|, 1); when a view contributes
``colour`` returns the quantities themselves too (``decisions``, NaN where the decision was not taken); tests/colour_inputs.py measures
COLOUR_DECISION_GAP from them."""
import math

import numpy as np

from tests import raycast_reference as ray

ROW = 20   # doubles per source view: K, [R | t] row-major, the centre C, one unused
MODES = ("blend", "best")


def source_rows(K, ext, dtype=np.float64):
    """The table of the source views, (V, 20): K, the 3 x 4 [R | t] row-major, C_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2), 0."""
    T = np.dtype(dtype).type
    Ka = np.asarray(K, dtype=np.float64).reshape(-1, 4).astype(T)
    P = np.asarray(ext, dtype=np.float64).reshape(-1, 3, 4).astype(T)
    rows = np.zeros((len(Ka), ROW), dtype=T)
    rows[:, :4] = Ka
    rows[:, 4:16] = P.reshape(-1, 12)
    rows[:, 16:19] = ray.render_rows(K, ext, T)[:, 13:16]
    return rows


def as_images(images):
    """(V, H, W) or (V, H, W, C) -> (V, H, W, C)."""
    im = np.asarray(images)
    return im[..., None] if im.ndim == 3 else im


def round_u8(v):
    """The FP64 value rounded half-to-even and saturated; a NaN gives 0."""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(v, dtype=np.float64))
        return np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0)).astype(np.uint8)


def to_output(colour, dtype):
    return round_u8(colour) if np.dtype(dtype) == np.dtype(np.uint8) else np.asarray(colour, dtype=np.float64).astype(np.float32)


def _clamp(c, top, T):
    c = np.where(c > 0, c, T(0))
    return np.where(c < top, c, T(top))


def colour(points, K, ext, width, height, images, normals=None, visibility=None, occlusion_tol=0.0, cos_min=0.0, mode="blend", fill=None, dtype=np.float64):
    """The vectorised form.  ``points`` (N, 3); ``images`` (V, H, W[, C]) uint8 or float32; ``visibility`` (V, H, W) or None.
    -> dict(colour (N, C) of ``dtype``, NOT rounded to the output type, weight (N) of ``dtype``, count (N) int64, best (N) int64, closest
    (N) float64, decisions: name -> (N, V[, ...]) or (N[, C]))."""
    T = np.dtype(dtype).type
    assert mode in MODES
    rows = source_rows(K, ext, T)
    im = as_images(images)
    V, H, W, C = im.shape
    assert V == len(rows) and (W, H) == (int(width), int(height)) and W >= 2 and H >= 2 and C in (1, 3, 4)
    X = np.asarray(points).reshape(-1, 3).astype(T)
    N = len(X)
    nrm = None if normals is None else np.asarray(normals).reshape(-1, 3).astype(T)
    tol, cmin = T(occlusion_tol), T(cos_min)
    fl = np.zeros(C, dtype=T) if fill is None else np.asarray(fill, dtype=np.float64).astype(T)
    S, Wt = np.zeros((N, C), dtype=T), np.zeros(N, dtype=T)
    count, best, best_c = np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=T)
    second_c = np.full(N, -np.inf, dtype=T)
    closest = np.full(N, np.inf)
    dec = dict(front=np.full((N, V), np.nan, dtype=T), inside=np.full((N, V), np.nan, dtype=T), floor=np.full((N, V, 2), np.nan, dtype=T),
               nearest=np.full((N, V, 2), np.nan, dtype=T), visible=np.full((N, V), np.nan, dtype=T), angle=np.full((N, V), np.nan, dtype=T),
               best=np.full(N, np.nan, dtype=T), u8=np.full((N, C), np.nan, dtype=T))
    one = T(1)

    def near(mask, a):
        a = np.abs(np.asarray(a, dtype=np.float64))
        keep = mask & ~np.isnan(a)
        closest[keep] = np.minimum(closest[keep], a[keep])

    with np.errstate(all="ignore"):
        for v in range(V):
            fx, cx, fy, cy = rows[v, :4]
            R, Cv = rows[v, 4:16].reshape(3, 4), rows[v, 16:19]
            Y = [((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + R[a, 3] for a in range(3)]
            sY = np.maximum(((np.abs(R[2, 0] * X[:, 0]) + np.abs(R[2, 1] * X[:, 1])) + np.abs(R[2, 2] * X[:, 2])) + np.abs(R[2, 3]), one)
            live = np.ones(N, dtype=bool)
            dec["front"][:, v] = Y[2] / sY
            near(live, dec["front"][:, v])
            ok = Y[2] > 0
            u, w = fx * (Y[0] / Y[2]) + cx, fy * (Y[1] / Y[2]) + cy
            su, sw = np.maximum(np.abs(u), T(W)), np.maximum(np.abs(w), T(H))
            q = np.minimum(np.minimum(u, T(W - 1) - u) / su, np.minimum(w, T(H - 1) - w) / sw)
            dec["inside"][ok, v] = q[ok]
            near(ok, q)
            ok = ok & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
            for k, (p, n, s) in enumerate(((u, W, su), (w, H, sw))):
                m = np.rint(p)
                q = np.where((m > 0) & (m < n - 1), np.abs(p - m), T(0.5)) / s
                dec["floor"][ok, v, k] = q[ok]
                near(ok, q)
            if visibility is not None:
                for k, (p, s) in enumerate(((u, su), (w, sw))):
                    t = p + T(0.5)
                    q = np.abs(t - np.rint(t)) / s
                    dec["nearest"][ok, v, k] = q[ok]
                    near(ok, q)
                qx, qy = _clamp(np.floor(u + T(0.5)), W - 1, T).astype(np.int64), _clamp(np.floor(w + T(0.5)), H - 1, T).astype(np.int64)
                d = np.asarray(visibility[v])[qy, qx].astype(T)
                valid = (d > 0) & (d < np.inf)
                q = ((d + tol) - Y[2]) / np.maximum(np.abs(d) + tol, np.abs(Y[2]))
                dec["visible"][ok & valid, v] = q[ok & valid]
                near(ok & valid, q)
                ok = ok & valid & (Y[2] <= d + tol)
            c = np.ones(N, dtype=T)
            if nrm is not None:
                e = [Cv[a] - X[:, a] for a in range(3)]
                length = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                c = ((nrm[:, 0] * e[0] + nrm[:, 1] * e[1]) + nrm[:, 2] * e[2]) / length
                dec["angle"][ok, v] = (c - cmin)[ok]
                near(ok, c - cmin)
                ok = ok & (c > cmin)
            x0, y0 = _clamp(np.floor(u), W - 2, T), _clamp(np.floor(w), H - 2, T)
            f0, f1 = u - x0, w - y0
            e0, e1 = one - f0, one - f1
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            img = im[v]
            A, B, Cc, D = img[yi, xi].astype(T), img[yi, xi + 1].astype(T), img[yi + 1, xi].astype(T), img[yi + 1, xi + 1].astype(T)
            top, bot = e0[:, None] * A + f0[:, None] * B, e0[:, None] * Cc + f0[:, None] * D
            I = e1[:, None] * top + f1[:, None] * bot
            better = ok & ((best < 0) | (c > best_c))
            second_c = np.where(better, np.where(best >= 0, best_c, second_c), np.where(ok, np.maximum(second_c, c), second_c))
            best, best_c = np.where(better, v, best), np.where(better, c, best_c)
            if mode == "best":
                S = np.where(better[:, None], I, S)
            else:
                S = np.where(ok[:, None], S + c[:, None] * I, S)
            Wt = np.where(ok, Wt + c, Wt)
            count = count + ok
        some = count > 0
        value = S if mode == "best" else S / Wt[:, None]
        out = np.where(some[:, None], value, fl[None, :])
        if nrm is not None:
            two = count >= 2
            dec["best"][two] = (best_c - second_c)[two]
            near(two, best_c - second_c)
        q = np.abs(out - (np.floor(out) + T(0.5))) / np.maximum(np.abs(out), one)
        dec["u8"][some] = q[some]
        near(some, np.min(q, axis=1))
    return dict(colour=out, weight=Wt, count=count, best=best, closest=closest, decisions=dec)


def colour_point(X, rows, width, height, images, normal=None, visibility=None, occlusion_tol=0.0, cos_min=0.0, mode="blend", fill=None):
    """The plain loop form: ONE point ``X`` (3 numbers) against the views of ``rows`` (``source_rows`` in float64), in Python floats.
    -> (colour [C], weight, count, best, closest)."""
    im = as_images(images)
    V, H, W, C = im.shape
    X = [float(x) for x in X]
    n = None if normal is None else [float(x) for x in normal]
    tol, cmin = float(occlusion_tol), float(cos_min)
    S, Wt, count, best, best_c, second_c = [0.0] * C, 0.0, 0, -1, 0.0, -math.inf
    closest = math.inf

    def near(q):
        nonlocal closest
        if q == q:
            closest = min(closest, abs(q))

    def div(a, b):
        if b == 0.0:
            return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b

    def clamp(c, top):
        c = c if c > 0 else 0.0
        return int(c if c < top else float(top))

    for v in range(V):
        row = [float(c) for c in rows[v]]
        fx, cx, fy, cy = row[:4]
        R, Cv = [row[4 + 4 * a:8 + 4 * a] for a in range(3)], row[16:19]
        Y = [((R[a][0] * X[0] + R[a][1] * X[1]) + R[a][2] * X[2]) + R[a][3] for a in range(3)]
        sY = max(((abs(R[2][0] * X[0]) + abs(R[2][1] * X[1])) + abs(R[2][2] * X[2])) + abs(R[2][3]), 1.0)
        near(Y[2] / sY)
        if not Y[2] > 0:
            continue
        u, w = fx * div(Y[0], Y[2]) + cx, fy * div(Y[1], Y[2]) + cy
        su, sw = max(abs(u), float(W)), max(abs(w), float(H))
        near(min(div(min(u, float(W - 1) - u), su), div(min(w, float(H - 1) - w), sw)) if u == u and w == w else math.nan)
        if not (0 <= u <= W - 1 and 0 <= w <= H - 1):
            continue
        for p, m_top, s in ((u, W, su), (w, H, sw)):
            m = round(p)
            near((abs(p - m) if 0 < m < m_top - 1 else 0.5) / s)
        if visibility is not None:
            for p, s in ((u, su), (w, sw)):
                t = p + 0.5
                near(abs(t - round(t)) / s)
            d = float(visibility[v][clamp(float(math.floor(w + 0.5)), H - 1), clamp(float(math.floor(u + 0.5)), W - 1)])
            if not (d > 0 and d < math.inf):
                continue
            near(((d + tol) - Y[2]) / max(abs(d) + tol, abs(Y[2])))
            if not Y[2] <= d + tol:
                continue
        c = 1.0
        if n is not None:
            e = [Cv[a] - X[a] for a in range(3)]
            length = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            c = div((n[0] * e[0] + n[1] * e[1]) + n[2] * e[2], length)
            near(c - cmin)
            if not c > cmin:
                continue
        x0, y0 = clamp(float(math.floor(u)), W - 2), clamp(float(math.floor(w)), H - 2)
        f0, f1 = u - float(x0), w - float(y0)
        e0, e1 = 1.0 - f0, 1.0 - f1
        I = []
        for k in range(C):
            A, B, Cc, D = float(im[v, y0, x0, k]), float(im[v, y0, x0 + 1, k]), float(im[v, y0 + 1, x0, k]), float(im[v, y0 + 1, x0 + 1, k])
            top, bot = e0 * A + f0 * B, e0 * Cc + f0 * D
            I.append(e1 * top + f1 * bot)
        better = best < 0 or c > best_c
        if better:
            if best >= 0:
                second_c = best_c
            best, best_c = v, c
        else:
            second_c = max(second_c, c)
        for k in range(C):
            if mode == "best":
                S[k] = I[k] if better else S[k]
            else:
                S[k] = S[k] + c * I[k]
        Wt = Wt + c
        count += 1
    if count == 0:
        return [0.0 if fill is None else float(fill[k]) for k in range(C)], 0.0, 0, -1, closest
    out = [S[k] if mode == "best" else div(S[k], Wt) for k in range(C)]
    if n is not None and count >= 2:
        near(best_c - second_c)
    q = [abs(o - (math.floor(o) + 0.5)) / max(abs(o), 1.0) if math.isfinite(o) else math.nan for o in out]
    near(math.nan if any(x != x for x in q) else min(q))
    return out, Wt, count, best, closest


def view_points(K_render, ext_render, width, height, depth, dtype=np.float64):
    """The points of the pixels of render views: X_a = C_a + z w_a by the cast's ray formulas.  ``depth`` (R, H, W).
    -> (points (R, H, W, 3) of ``dtype``, live (R, H, W): the depth is finite and > 0)."""
    T = np.dtype(dtype).type
    rows = ray.render_rows(K_render, ext_render, T)
    W, H = int(width), int(height)
    ys, xs = np.meshgrid(np.arange(H).astype(T), np.arange(W).astype(T), indexing="ij")
    z = np.asarray(depth).astype(T)
    out = np.zeros((len(rows), H, W, 3), dtype=T)
    with np.errstate(all="ignore"):
        for r in range(len(rows)):
            fx, cx, fy, cy = rows[r, :4]
            R, C = rows[r, 4:13].reshape(3, 3), rows[r, 13:16]
            r0, r1 = (xs - cx) / fx, (ys - cy) / fy
            for a in range(3):
                wa = (R[0, a] * r0 + R[1, a] * r1) + R[2, a] * T(1)
                out[r, :, :, a] = C[a] + z[r] * wa
        return out, (z > 0) & (z < np.inf)


def colour_views(K_render, ext_render, r_width, r_height, depth, K, ext, width, height, images, normal_map=None, **kw):
    """``colour`` on the pixels of render views; a pixel whose depth is not finite or not > 0 takes the fill.  Outputs in image order."""
    dtype = kw.get("dtype", np.float64)
    pts, live = view_points(K_render, ext_render, r_width, r_height, depth, dtype)
    X = np.where(live[..., None], pts, np.nan).reshape(-1, 3)   # a NaN point is rejected by every view: the fill
    r = colour(X, K, ext, width, height, images, normals=None if normal_map is None else np.asarray(normal_map).reshape(-1, 3), **kw)
    shape = live.shape
    return dict(colour=r["colour"].reshape(shape + (-1,)), weight=r["weight"].reshape(shape), count=r["count"].reshape(shape), best=r["best"].reshape(shape),
                closest=r["closest"].reshape(shape), decisions=r["decisions"], points=pts, live=live)


def point_normals(vol, points, min_weight=2, dtype=np.float64):
    """The cast's normal rule at arbitrary points, vectorised.  -> dict(normal (N, 3) of ``dtype`` (not rounded to float32), status (N)
    uint8: 0 with a normal, 1 without, closest (N) float64, decisions: box (N, 18), cell (N, 18), G (N))."""
    T = np.dtype(dtype).type
    X = np.asarray(points).reshape(-1, 3).astype(T)
    N = len(X)
    dims = vol.dims
    o, s = [T(c) for c in vol.origin], T(vol.voxel)
    D, obs = ray.node_values(vol, min_weight, T)
    h = [T(n - 1) for n in dims]
    one, zero = T(1), T(0)
    normal, status, closest = np.full((N, 3), np.nan, dtype=T), np.ones(N, dtype=np.uint8), np.full(N, np.inf)
    dec = dict(box=np.full((N, 18), np.nan, dtype=T), cell=np.full((N, 18), np.nan, dtype=T), G=np.full(N, np.nan, dtype=T))
    if min(dims) < 2 or N == 0:
        return dict(normal=normal, status=status, closest=closest, decisions=dec)

    def near(mask, a):
        a = np.abs(np.asarray(a, dtype=np.float64))
        keep = mask & ~np.isnan(a)
        closest[keep] = np.minimum(closest[keep], a[keep])

    with np.errstate(all="ignore"):
        g = [(X[:, a] - o[a]) / s for a in range(3)]
        sc = [np.maximum(np.abs(g[a]), one) for a in range(3)]
        ok, G = np.ones(N, dtype=bool), [np.zeros(N, dtype=T) for _ in range(3)]
        for a in range(3):
            Tab = []
            for k, sgn in enumerate((one, -one)):
                ga = list(g)
                ga[a] = g[a] + sgn
                box = np.stack([np.minimum(ga[b], h[b] - ga[b]) / sc[b] for b in range(3)], axis=-1)
                dec["box"][ok, 6 * a + 3 * k:6 * a + 3 * k + 3] = box[ok]
                near(ok, np.min(np.abs(box), axis=-1))
                inb = np.ones(N, dtype=bool)
                for b in range(3):
                    inb = inb & (ga[b] >= 0) & (ga[b] <= h[b])
                take = ok & inb
                cell = np.stack([np.where((np.rint(ga[b]) > 0) & (np.rint(ga[b]) < h[b]), np.abs(ga[b] - np.rint(ga[b])), T(0.5)) / sc[b] for b in range(3)], axis=-1)
                dec["cell"][take, 6 * a + 3 * k:6 * a + 3 * k + 3] = cell[take]
                near(take, np.min(cell, axis=-1))
                gs = [np.where(take, x, zero) for x in ga]   # a sample that is not taken reads node 0 and is dropped
                valid, Tv = ray.sample(D, obs, dims, gs, T)
                ok = take & valid
                Tab.append(Tv)
            G[a] = Tab[0] - Tab[1]
        length = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
        dec["G"][ok] = length[ok]
        near(ok, length)
        ok = ok & (length > 0)
        for a in range(3):
            normal[ok, a] = (G[a] / length)[ok]
        status[ok] = 0
    return dict(normal=normal, status=status, closest=closest, decisions=dec)


def point_normal(vol, X, min_weight=2):
    """The plain loop form for ONE point, in Python floats.  -> ((n0, n1, n2), status, closest)."""
    nan = math.nan
    dims = vol.dims
    o, s = vol.origin, vol.voxel
    h = [float(n - 1) for n in dims]
    closest = math.inf
    none = ((nan, nan, nan), 1)
    if min(dims) < 2:
        return none + (closest,)

    def value(i, j, l):
        wgt, sm = int(vol.weight[l, j, i]), float(vol.sum[l, j, i])
        if wgt == 0:
            return (nan if sm == 0 or sm != sm else math.copysign(math.inf, sm)), False
        return sm / float(wgt), wgt >= min_weight

    def sample(g):
        c, f = [], []
        for a in range(3):
            fl = float(math.floor(g[a]))
            ca = fl if fl > 0 else 0.0
            ca = ca if ca < dims[a] - 2 else float(dims[a] - 2)
            fa = g[a] - ca
            fa = fa if fa > 0 else 0.0
            fa = fa if fa < 1 else 1.0
            c.append(int(ca)), f.append(fa)
        Dc, valid = [], True
        for k in range(8):
            d, ob = value(c[0] + (k & 1), c[1] + (k >> 1 & 1), c[2] + (k >> 2 & 1))
            Dc.append(d)
            valid = valid and ob
        e = [1.0 - fa for fa in f]
        xx = [e[0] * Dc[2 * m] + f[0] * Dc[2 * m + 1] for m in range(4)]
        yy = [e[1] * xx[0] + f[1] * xx[1], e[1] * xx[2] + f[1] * xx[3]]
        return valid, e[2] * yy[0] + f[2] * yy[1]

    g = [(float(X[a]) - float(o[a])) / float(s) for a in range(3)]
    sc = [max(abs(g[a]), 1.0) if g[a] == g[a] else nan for a in range(3)]
    G = []
    for a in range(3):
        Tab = []
        for sgn in (1.0, -1.0):
            ga = list(g)
            ga[a] = g[a] + sgn
            box = [min(ga[b], h[b] - ga[b]) / sc[b] if ga[b] == ga[b] else nan for b in range(3)]
            if all(x == x for x in box):   # a NaN coordinate fails the test below whatever its distance
                closest = min(closest, min(abs(x) for x in box))
            if not all(0 <= ga[b] <= h[b] for b in range(3)):
                return none + (closest,)
            for b in range(3):
                m = round(ga[b])
                closest = min(closest, (abs(ga[b] - m) if 0 < m < h[b] else 0.5) / sc[b])
            valid, Tv = sample(ga)
            if not valid:
                return none + (closest,)
            Tab.append(Tv)
        G.append(Tab[0] - Tab[1])
    length = math.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
    if length == length:
        closest = min(closest, abs(length))
    if not length > 0:
        return none + (closest,)
    return (G[0] / length, G[1] / length, G[2] / length), 0, closest
