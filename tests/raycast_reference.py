"""The ray-cast rule of include/pcs_hip.h ("Ray-cast of the TSDF volume", csrc/ba_tsdf_raycast.hpp) restated in NumPy: TEST INFRASTRUCTURE.

Two forms of the same rule, as tests/tsdf_reference.py has them.  ``raycast`` works on all pixels of a view at once with masks and takes
the arithmetic type (float64 or ``np.longdouble``); ``raycast_pixel`` marches ONE ray with early exits, plain indexing and Python floats
(IEEE doubles).  Every formula is written in the order the header states, so the two forms agree bit for bit in float64.  Neither skips
empty space: skipping changes no bit, and the device is held to this form with and without it.

Both return the CLOSEST CALL per pixel: over every decision the ray took, the smallest distance to its threshold, each relative to the
quantity's scale.  The decisions, in the order a ray meets them:
  z0 <= z1             |z1 - z0| / max(|z0|, |z1|), once the ray has passed the gw_a == 0 tests (z1 finite)
  N = floor(q)         the distance of q = (z1 - z0) / dz to the nearest integer, / max(q, 1)
  the cell of g_a      for every evaluated sample (and the hit point) and axis: the distance of g_a to the nearest integer m, when
                       0 < m < h_a, / s_a = max(|gc_a| + |z gw_a|, 1).  At m <= 0 and m >= h_a the clamp picks the same cell from both
                       sides and the blend is continuous: no decision.
  T > 0, T <= 0        |T| of every VALID evaluated sample (|D| <= 1: the scale is 1)
  in the box           for the six samples of the normal, as far as they are taken: min(coordinate, h_b - coordinate) on every axis b, / s_b
  |G| > 0              |G| when the six samples are there
``raycast`` returns the quantities themselves too (``decisions``, each divided by its scale, NaN where the decision was not taken);
tests/raycast_inputs.py measures RAY_DECISION_GAP from them."""
import math

import numpy as np

MAX_STEPS = 113513   # 64 sqrt(3) 1024 + 1, rounded up
HIT, NO_NORMAL, NO_CROSSING, MISSED = 0, 1, 2, 3


def render_rows(K, ext, dtype=np.float64):
    """The table of the render views, (V, 16): K, the nine entries of R row-major, C_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2)."""
    T = np.dtype(dtype).type
    Ka = np.asarray(K, dtype=np.float64).reshape(-1, 4).astype(T)
    P = np.asarray(ext, dtype=np.float64).reshape(-1, 3, 4).astype(T)
    rows = np.zeros((len(Ka), 16), dtype=T)
    rows[:, :4] = Ka
    rows[:, 4:13] = P[:, :, :3].reshape(-1, 9)
    for a in range(3):
        rows[:, 13 + a] = -((P[:, 0, a] * P[:, 0, 3] + P[:, 1, a] * P[:, 1, 3]) + P[:, 2, a] * P[:, 2, 3])
    return rows


def node_values(vol, min_weight, dtype=np.float64):
    """-> (D = sum / weight (nz, ny, nx) of ``dtype``, OBSERVED)."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        return vol.sum.astype(T) / vol.weight.astype(T), vol.weight >= min_weight


def _cell(g, n, T):
    fl = np.floor(g)
    c = np.where(fl > 0, fl, T(0))
    return np.where(c < n - 2, c, T(n - 2))


def _frac(g, c, T):
    f = g - c
    f = np.where(f > 0, f, T(0))
    return np.where(f < 1, f, T(1))


def sample(D, obs, dims, g, T):
    """T(g) for arrays g = (g0, g1, g2).  -> (VALID, value)."""
    c = [_cell(g[a], dims[a], T) for a in range(3)]
    f = [_frac(g[a], c[a], T) for a in range(3)]
    ci = [x.astype(np.int64) for x in c]
    Dc, valid = [], np.ones(g[0].shape, dtype=bool)
    for k in range(8):
        i, j, l = ci[0] + (k & 1), ci[1] + (k >> 1 & 1), ci[2] + (k >> 2 & 1)
        Dc.append(D[l, j, i])
        valid = valid & obs[l, j, i]
    one = T(1)
    e = [one - f[a] for a in range(3)]
    with np.errstate(all="ignore"):
        x = [e[0] * Dc[2 * m] + f[0] * Dc[2 * m + 1] for m in range(4)]
        y = [e[1] * x[0] + f[1] * x[1], e[1] * x[2] + f[1] * x[3]]
        return valid, e[2] * y[0] + f[2] * y[1]


def raycast(vol, K, ext, width, height, min_weight=2, step=None, z_near=0.0, z_far=np.inf, dtype=np.float64, normals=True):
    """The vectorised form.  -> dict(depth (V, H, W) of ``dtype``, normal (V, H, W, 3) of ``dtype`` (not rounded to float32), status
    uint8, closest (V, H, W) float64, decisions: name -> array, samples: the number of samples evaluated)."""
    T = np.dtype(dtype).type
    rows = render_rows(K, ext, T)
    V, W, H = len(rows), int(width), int(height)
    dims = vol.dims
    o, s = [T(c) for c in vol.origin], T(vol.voxel)
    step = s if step is None else T(step)
    assert 1 <= min_weight <= 65535 and step >= s / 64 and 0 <= z_near < z_far
    D, obs = node_values(vol, min_weight, T)
    h = [T(n - 1) for n in dims]
    P = H * W
    out = dict(depth=np.full((V, P), np.nan, dtype=T), normal=np.full((V, P, 3), np.nan, dtype=T), status=np.full((V, P), MISSED, dtype=np.uint8), closest=np.full((V, P), np.inf))
    dec = dict(clip=np.full((V, P), np.nan, dtype=T), floor=np.full((V, P), np.nan, dtype=T), box=np.full((V, P, 18), np.nan, dtype=T), G=np.full((V, P), np.nan, dtype=T),
               hit_g=np.full((V, P, 3), np.nan, dtype=T))
    march_g, march_T = [], []
    n_samples = 0
    ys, xs = np.meshgrid(np.arange(H).astype(T), np.arange(W).astype(T), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    one, zero = T(1), T(0)

    def near(v, idx, a):
        a = np.asarray(a, dtype=np.float64)
        keep = ~np.isnan(a)
        np.minimum.at(out["closest"][v], idx[keep], a[keep])

    with np.errstate(all="ignore"):
        for v in range(V):
            fx, cx, fy, cy = rows[v, :4]
            R, C = rows[v, 4:13].reshape(3, 3), rows[v, 13:16]
            r0, r1 = (xs - cx) / fx, (ys - cy) / fy
            w = [(R[0, a] * r0 + R[1, a] * r1) + R[2, a] * one for a in range(3)]
            gc = [(C[a] - o[a]) / s for a in range(3)]
            gw = [w[a] / s for a in range(3)]
            z0, z1 = np.full(P, T(z_near)), np.full(P, T(z_far))
            inbox = np.full(P, all(n >= 2 for n in dims))
            for a in range(3):
                along = gw[a] == 0
                t0, t1 = (zero - gc[a]) / gw[a], (h[a] - gc[a]) / gw[a]
                lo, hi = np.where(t0 < t1, t0, t1), np.where(t0 < t1, t1, t0)
                z0, z1 = np.where(~along & (lo > z0), lo, z0), np.where(~along & (hi < z1), hi, z1)
                inbox = inbox & (~along | bool(gc[a] >= 0 and gc[a] <= h[a]))
            allp = np.arange(P)
            dec["clip"][v] = np.where(inbox & np.isfinite(z1), (z1 - z0) / np.maximum(np.abs(z0), np.abs(z1)), np.nan)
            near(v, allp, np.abs(dec["clip"][v]))
            inbox = inbox & (z0 <= z1)
            dz = step / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
            q = (z1 - z0) / dz
            inbox = inbox & (q <= MAX_STEPS)
            qs = np.maximum(q, one)
            dec["floor"][v] = np.where(inbox, q / qs, np.nan)
            near(v, allp, np.where(inbox, np.abs(q - np.rint(q)) / qs, np.nan))
            N = np.where(inbox, np.floor(q), -1).astype(np.int64)
            out["status"][v][inbox] = NO_CROSSING
            prev_valid, prev_T, prev_z, hit = np.zeros(P, dtype=bool), np.zeros(P, dtype=T), np.zeros(P, dtype=T), np.zeros(P, dtype=bool)
            mg, mT = np.full((int(N.max()) + 1, P, 3), np.nan, dtype=T), np.full((int(N.max()) + 1, P), np.nan, dtype=T)

            def cell_calls(idx, z, g):
                for a in range(3):
                    sc = np.maximum(np.abs(gc[a]) + np.abs(z * gw[a][idx]), one)
                    m = np.rint(g[a])
                    near(v, idx, np.where((m > 0) & (m < h[a]), np.abs(g[a] - m) / sc, np.nan))
                return [g[a] / np.maximum(np.abs(gc[a]) + np.abs(z * gw[a][idx]), one) for a in range(3)]

            for n in range(int(N.max()) + 1):
                idx = np.nonzero(inbox & ~hit & (N >= n))[0]
                if not idx.size:
                    break
                z = z0[idx] + T(n) * dz[idx]
                g = [gc[a] + z * gw[a][idx] for a in range(3)]
                valid, Tv = sample(D, obs, dims, g, T)
                n_samples += idx.size
                mg[n, idx] = np.stack(cell_calls(idx, z, g), axis=-1)
                mT[n, idx] = np.where(valid, Tv, np.nan)
                near(v, idx, np.where(valid, np.abs(Tv), np.nan))
                is_hit = (n >= 1) & prev_valid[idx] & valid & (prev_T[idx] > 0) & (Tv <= 0)
                hi_ = idx[is_hit]
                out["depth"][v][hi_] = prev_z[hi_] + dz[hi_] * (prev_T[hi_] / (prev_T[hi_] - Tv[is_hit]))
                out["status"][v][hi_] = HIT
                hit[hi_] = True
                prev_valid[idx], prev_T[idx], prev_z[idx] = valid, Tv, z
            march_g.append(mg), march_T.append(mT)
            idx = np.nonzero(hit)[0]
            if normals and idx.size:
                z = out["depth"][v][idx]
                g = [gc[a] + z * gw[a][idx] for a in range(3)]
                dec["hit_g"][v][idx] = np.stack(cell_calls(idx, z, g), axis=-1)
                sc = [np.maximum(np.abs(gc[a]) + np.abs(z * gw[a][idx]), one) for a in range(3)]
                ok, G = np.ones(idx.size, dtype=bool), [np.zeros(idx.size, dtype=T) for _ in range(3)]
                for a in range(3):
                    Tab = []
                    for k, sgn in enumerate((one, -one)):
                        ga = list(g)
                        ga[a] = g[a] + sgn
                        box = np.stack([np.minimum(ga[b], h[b] - ga[b]) / sc[b] for b in range(3)], axis=-1)
                        dec["box"][v][idx[ok], 6 * a + 3 * k:6 * a + 3 * k + 3] = box[ok]
                        near(v, idx[ok], np.min(np.abs(box[ok]), axis=-1))
                        inb = np.ones(idx.size, dtype=bool)
                        for b in range(3):
                            inb = inb & (ga[b] >= 0) & (ga[b] <= h[b])
                        take = ok & inb
                        gs = [np.where(take, x, zero) for x in ga]   # a sample that is not taken reads node 0 and is dropped
                        valid, Tv = sample(D, obs, dims, gs, T)
                        ok = take & valid
                        Tab.append(Tv)
                    G[a] = Tab[0] - Tab[1]
                length = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
                dec["G"][v][idx[ok]] = length[ok]
                near(v, idx[ok], np.abs(length[ok]))
                ok = ok & (length > 0)
                for a in range(3):
                    out["normal"][v][idx[ok], a] = (G[a] / length)[ok]
                out["status"][v][idx[~ok]] = NO_NORMAL
    depth_n = max(m.shape[0] for m in march_T)
    pad = lambda m: np.concatenate([m, np.full((depth_n - m.shape[0],) + m.shape[1:], np.nan, dtype=T)])
    dec["march_g"], dec["march_T"] = np.stack([pad(m) for m in march_g]), np.stack([pad(m) for m in march_T])
    return dict(depth=out["depth"].reshape(V, H, W), normal=out["normal"].reshape(V, H, W, 3), status=out["status"].reshape(V, H, W), closest=out["closest"].reshape(V, H, W),
                decisions=dec, samples=n_samples)


def raycast_pixel(vol, row, x, y, min_weight=2, step=None, z_near=0.0, z_far=math.inf, normals=True):
    """The plain loop form: the ray of pixel (x, y) of the view with table row ``row`` (16 floats), in Python floats.
    -> (depth, (n0, n1, n2), status, closest)."""
    nan = math.nan
    dims = vol.dims
    o, s = vol.origin, vol.voxel
    step = s if step is None else float(step)
    row = [float(c) for c in row]
    fx, cx, fy, cy = row[:4]
    R, C = row[4:13], row[13:16]
    h = [float(n - 1) for n in dims]
    closest = math.inf

    def value(i, j, l):
        wgt = int(vol.weight[l, j, i])
        sm = float(vol.sum[l, j, i])
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

    r0, r1 = (float(x) - cx) / fx, (float(y) - cy) / fy
    w = [(R[a] * r0 + R[3 + a] * r1) + R[6 + a] * 1.0 for a in range(3)]
    gc = [(C[a] - o[a]) / s for a in range(3)]
    gw = [w[a] / s for a in range(3)]
    missed = (nan, (nan, nan, nan), MISSED)
    if not all(n >= 2 for n in dims):
        return missed + (closest,)
    z0, z1 = float(z_near), float(z_far)
    inbox = True
    for a in range(3):
        if gw[a] == 0:
            inbox = inbox and 0 <= gc[a] <= h[a]
            continue
        t0, t1 = (0.0 - gc[a]) / gw[a], (h[a] - gc[a]) / gw[a]
        lo, hi = (t0, t1) if t0 < t1 else (t1, t0)
        z0, z1 = (lo if lo > z0 else z0), (hi if hi < z1 else z1)
    if not inbox:
        return missed + (closest,)
    if math.isfinite(z1):
        closest = min(closest, abs((z1 - z0) / max(abs(z0), abs(z1))))
    if not z0 <= z1:
        return missed + (closest,)
    dz = step / math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    q = (z1 - z0) / dz
    if not q <= MAX_STEPS:
        return missed + (closest,)
    closest = min(closest, abs(q - round(q)) / max(q, 1.0))
    N = math.floor(q)

    def cell_calls(z, g):
        best = math.inf
        for a in range(3):
            m = round(g[a])
            if 0 < m < h[a]:
                best = min(best, abs(g[a] - m) / max(abs(gc[a]) + abs(z * gw[a]), 1.0))
        return best

    depth, prev = nan, None
    for n in range(N + 1):
        z = z0 + float(n) * dz
        g = [gc[a] + z * gw[a] for a in range(3)]
        valid, Tv = sample(g)
        closest = min(closest, cell_calls(z, g))
        if valid:
            closest = min(closest, abs(Tv))
        if prev is not None and prev[0] and valid and prev[1] > 0 and Tv <= 0:
            depth = prev[2] + dz * (prev[1] / (prev[1] - Tv))
            break
        prev = (valid, Tv, z)
    if depth != depth:
        return nan, (nan, nan, nan), NO_CROSSING, closest
    if not normals:
        return depth, (nan, nan, nan), HIT, closest
    g = [gc[a] + depth * gw[a] for a in range(3)]
    closest = min(closest, cell_calls(depth, g))
    sc = [max(abs(gc[a]) + abs(depth * gw[a]), 1.0) for a in range(3)]
    G = []
    for a in range(3):
        Tab = []
        for sgn in (1.0, -1.0):
            ga = list(g)
            ga[a] = g[a] + sgn
            closest = min(closest, min(abs(min(ga[b], h[b] - ga[b]) / sc[b]) for b in range(3)))
            if not all(0 <= ga[b] <= h[b] for b in range(3)):
                return depth, (nan, nan, nan), NO_NORMAL, closest
            valid, Tv = sample(ga)
            if not valid:
                return depth, (nan, nan, nan), NO_NORMAL, closest
            Tab.append(Tv)
        G.append(Tab[0] - Tab[1])
    length = math.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
    closest = min(closest, abs(length))
    if not length > 0:
        return depth, (nan, nan, nan), NO_NORMAL, closest
    return depth, (G[0] / length, G[1] / length, G[2] / length), HIT, closest
