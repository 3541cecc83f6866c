"""NumPy restatement of the PatchMatch rule (include/pcs_hip.h, "PatchMatch multi-view depth"; csrc/ba_patchmatch.hpp).  The plane
arithmetic and the warp are float64 in the order the header writes; the random numbers are exact; everything behind the rounding to
sixteenths is integer arithmetic, so the device is held to bit-equality with ``patchmatch``.  ``patchmatch_loops`` states the same rule
as a plain loop over (view, pixel, candidate, neighbour, window position) with Python scalars and must agree with ``patchmatch``
exactly.  ``decision_margins`` measures how far a run keeps from the floating-point decisions of the rule (the rounding to a sixteenth,
the signs of n_2 and omega) and how far float64 is from longdouble there."""
import math

import numpy as np

from tests.sweep_reference import lists_of, warp_table

NOT_STRICT, NO_VIEW = 1, 2
MASK = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-5, 0), (5, 0), (0, -5), (0, 5))
GAP_EVERY = 8   # the longdouble side of decision_margins looks at every 8th pixel of a call


# ---- the generator of csrc/ba_consensus.hpp --------------------------------------------------------------------------------------------
def mix_int(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def keys(seed, view, pix, t):
    k = mix_int((seed + GOLDEN) & MASK)
    k = mix_int(k ^ view)
    return mix(mix(np.uint64(k) ^ np.asarray(pix).astype(np.uint64)) ^ np.uint64(t))


def rand(k, d):
    with np.errstate(over="ignore"):
        r = mix(k + np.uint64(((d + 1) * GOLDEN) & MASK))
    return (r >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ---- the set-up both forms share -------------------------------------------------------------------------------------------------------
class Setup:
    def __init__(self, images, K, ext, neighbours, depth_range, census=(7, 7), stride=2, truncate=None, max_slant=70.0, seed=0):
        from pycamset_amd.patchmatch import check_patchmatch_args   # host NumPy: wrange and slope_max as the library forms them

        self.images = np.asarray(images)
        self.V, self.H, self.W = V, H, W = self.images.shape
        Ka, P, start, nbr, wrange, slope, cw, ch, s, tau, seed, _, _, _ = check_patchmatch_args(V, W, H, W, K, ext, neighbours, depth_range, census, stride, truncate, max_slant, seed)
        self.K, self.P, self.lists = Ka, P, lists_of((start, nbr), V)
        self.wrange = np.broadcast_to(wrange, (V, 2)) if wrange.shape[0] == 1 else wrange
        self.sigma, self.rw, self.rh, self.s, self.tau, self.seed = slope, cw // 2, ch // 2, s, tau, seed
        self.warps = [[warp_table(Ka[i], P[i], Ka[j], P[j]) for j in self.lists[i]] for i in range(V)]
        self.long_warps = None
        self.strict = np.zeros((H, W), dtype=bool)
        x0, y0 = self.rw * s, self.rh * s
        if H - y0 > y0 and W - x0 > x0:
            self.strict[y0:H - y0, x0:W - x0] = True
        self.window = [(dx, dy) for dy in range(-self.rh, self.rh + 1) for dx in range(-self.rw, self.rw + 1) if (dx, dy) != (0, 0)]

    def is_strict(self, x, y):
        return self.rw * self.s <= x <= self.W - 1 - self.rw * self.s and self.rh * self.s <= y <= self.H - 1 - self.rh * self.s


def new_probe():
    return dict(closest_t=np.inf, gap_t=0.0, closest_n2=np.inf, gap_n2=0.0, closest_om=np.inf, gap_om=0.0, samples=0)


def _project(A, b, om, xd, yd):
    """Step 2 -> (n_2, 16 u + 0.5, 16 v + 0.5) in the dtype of the arguments."""
    T = A.dtype.type
    n = [((A[c, 0] * xd + A[c, 1] * yd) + A[c, 2]) + om * b[c] for c in range(3)]
    with np.errstate(all="ignore"):
        return n[2], T(16) * (n[0] / n[2]) + T(0.5), T(16) * (n[1] / n[2]) + T(0.5)


def _sample(S, i, slot, w, a, b, xs, ys, sx, sy, probe=None):
    """Steps 2 and 3 for the pixels (xs, ys) (N,) of view i at the window offsets (sx, sy) in pixels, integer columns (P, 1)
    -> (g int64 (P, N), valid)."""
    A, bv = S.warps[i][slot]
    I = S.images[S.lists[i][slot]]
    H, W = S.H, S.W
    with np.errstate(invalid="ignore"):
        om = (w + a * sx.astype(np.float64)) + b * sy.astype(np.float64)
        n2, tu, tv = _project(A, bv, om, (xs + sx).astype(np.float64), (ys + sy).astype(np.float64))
    with np.errstate(all="ignore"):
        qu, qv = np.floor(tu), np.floor(tv)
        valid = (om > 0) & (n2 > 0) & (qu >= 0) & (qu < 16 * (W - 1)) & (qv >= 0) & (qv < 16 * (H - 1))   # a comparison with a NaN is False
    if probe is not None and len(xs):
        _look(S, probe, i, slot, w, a, b, xs, ys, sx, sy, om, n2, tu, tv)
    iu, iv = np.where(valid, qu, 0).astype(np.int64), np.where(valid, qv, 0).astype(np.int64)
    x0, fx, y0, fy = iu >> 4, iu & 15, iv >> 4, iv & 15
    J = I.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)   # in range wherever valid; clipped for the rest
    g = (16 - fx) * (16 - fy) * J[y0, x0] + fx * (16 - fy) * J[y0, x1] + (16 - fx) * fy * J[y1, x0] + fx * fy * J[y1, x1]
    return np.where(valid, g, 0), valid


def _look(S, probe, i, slot, w, a, b, xs, ys, sx, sy, om, n2, tu, tv):
    """decision_margins' look at one call of _sample.  Closeness over every sample; the longdouble side over every GAP_EVERY-th.  The
    roundings are looked at where they can decide anything: omega > 0, n_2 > 0, 16 u + 0.5 in [-1, 16 W], 16 v + 0.5 in [-1, 16 H]."""
    L = np.longdouble
    w, a, b, xs, ys, sx, sy = (np.broadcast_to(v, om.shape).ravel() for v in (w, a, b, xs, ys, sx, sy))
    om, n2, tu, tv = om.ravel(), n2.ravel(), tu.ravel(), tv.ravel()
    fin = np.isfinite(om)
    probe["samples"] += int(fin.sum())
    if not fin.any():
        return
    probe["closest_om"] = min(probe["closest_om"], float(np.min(np.abs(om[fin]))))
    probe["closest_n2"] = min(probe["closest_n2"], float(np.min(np.abs(n2[fin]))))
    with np.errstate(all="ignore"):
        near = fin & (om > 0) & (n2 > 0) & (tu >= -1) & (tu <= 16 * S.W) & (tv >= -1) & (tv <= 16 * S.H)
    for t in (tu[near], tv[near]):
        if t.size:
            probe["closest_t"] = min(probe["closest_t"], float(np.min(np.abs(t - np.rint(t)))))
    if S.long_warps is None:
        S.long_warps = [[warp_table(S.K[v], S.P[v], S.K[j], S.P[j], L) for j in S.lists[v]] for v in range(S.V)]
    Al, bl = S.long_warps[i][slot]
    e = slice(None, None, GAP_EVERY)
    with np.errstate(invalid="ignore"):
        oml = (w[e].astype(L) + a[e].astype(L) * sx[e].astype(L)) + b[e].astype(L) * sy[e].astype(L)
        n2l, tul, tvl = _project(Al, bl, oml, (xs[e] + sx[e]).astype(L), (ys[e] + sy[e]).astype(L))
    f, nr = fin[e], near[e]
    if f.any():
        probe["gap_om"] = max(probe["gap_om"], float(np.max(np.abs(om[e][f] - oml[f]))))
        probe["gap_n2"] = max(probe["gap_n2"], float(np.max(np.abs(n2[e][f] - n2l[f]))))
    if nr.any():
        probe["gap_t"] = max(probe["gap_t"], float(np.max(np.abs(tu[e][nr] - tul[nr]))), float(np.max(np.abs(tv[e][nr] - tvl[nr]))))


def cost(S, i, xs, ys, w, a, b, probe=None):
    """C of the planes (w, a, b) at the strict pixels (xs, ys) of view i -> int64."""
    C = np.zeros(len(xs), dtype=np.int64)
    Ii = S.images[i].astype(np.int64)
    sx = S.s * np.array([0] + [dx for dx, _ in S.window])[:, None]   # the centre first
    sy = S.s * np.array([0] + [dy for _, dy in S.window])[:, None]
    ref = Ii[ys + sy, xs + sx]
    ref_bits = ref[1:] < ref[0]
    for slot in range(len(S.lists[i])):
        g, valid = _sample(S, i, slot, w, a, b, xs, ys, sx, sy, probe)
        h = np.sum((g[1:] < g[0]) != ref_bits, axis=0)
        C += np.where(valid.all(axis=0), np.minimum(h, S.tau), S.tau)
    return C


def admissible(S, i, w, a, b):
    lo, hi = S.wrange[i]
    with np.errstate(invalid="ignore"):
        sw = S.sigma[i] * w
        return (w >= lo) & (w <= hi) & (np.abs(a) <= sw) & (np.abs(b) <= sw)


def draw(S, i, k, d):
    lo, hi = S.wrange[i]
    w = lo + rand(k, d) * (hi - lo)
    sw = S.sigma[i] * w
    return w, sw * (2.0 * rand(k, d + 1) - 1.0), sw * (2.0 * rand(k, d + 2) - 1.0)


def initialise(S, depth=None, planes=None, probe=None):
    """t = 0 -> (plane (V, H, W, 3) float64, cost (V, H, W) int32)."""
    plane, cst = np.full((S.V, S.H, S.W, 3), np.nan), np.full((S.V, S.H, S.W), -1, dtype=np.int32)
    ys, xs = np.nonzero(S.strict)
    for i in range(S.V):
        lo, hi = S.wrange[i]
        w, a, b = draw(S, i, keys(S.seed, i, ys * S.W + xs, 0), 0)
        if planes is not None:
            p = np.asarray(planes)[i][ys, xs]
            have = admissible(S, i, p[:, 0], p[:, 1], p[:, 2])
            w, a, b = np.where(have, p[:, 0], w), np.where(have, p[:, 1], a), np.where(have, p[:, 2], b)
        elif depth is not None:
            d = np.asarray(depth)[i][ys, xs].astype(np.float64)
            with np.errstate(all="ignore"):
                have = np.isfinite(d) & (d > 0)
                w0 = 1.0 / d
                w0 = np.where(w0 < lo, lo, np.where(w0 > hi, hi, w0))
            w, a, b = np.where(have, w0, w), np.where(have, 0.0, a), np.where(have, 0.0, b)
        plane[i, ys, xs] = np.stack([w, a, b], axis=1)
        cst[i, ys, xs] = cost(S, i, xs, ys, w, a, b, probe)
    return plane, cst


def half_iteration(S, plane, cst, it, colour, probe=None):
    """One colour of iteration ``it``, in place: it reads only pixels of the other colour, which it does not write."""
    ys, xs = np.nonzero(S.strict)
    pick = ((xs + ys) & 1) == colour
    ys, xs = ys[pick], xs[pick]
    rho, half_it = 2.0 ** -(2 + it), 2.0 ** -(1 + it)
    for i in range(S.V):
        cur = plane[i, ys, xs]
        w, a, b, c = cur[:, 0].copy(), cur[:, 1].copy(), cur[:, 2].copy(), cst[i, ys, xs].astype(np.int64)

        def offer(cw, ca, cb, have):
            ok = have & admissible(S, i, cw, ca, cb)
            if ok.any():
                C = cost(S, i, xs[ok], ys[ok], cw[ok], ca[ok], cb[ok], probe)
                better = C < c[ok]
                idx = np.nonzero(ok)[0][better]
                w[idx], a[idx], b[idx], c[idx] = cw[idx], ca[idx], cb[idx], C[better]

        for ox, oy in OFFSETS:
            qx, qy = xs + ox, ys + oy
            have = (qx >= 0) & (qx < S.W) & (qy >= 0) & (qy < S.H)
            have &= S.strict[np.clip(qy, 0, S.H - 1), np.clip(qx, 0, S.W - 1)]
            q = plane[i, np.clip(qy, 0, S.H - 1), np.clip(qx, 0, S.W - 1)]
            offer((q[:, 0] - q[:, 1] * float(ox)) - q[:, 2] * float(oy), q[:, 1], q[:, 2], have)
        k = keys(S.seed, i, ys * S.W + xs, 1 + 2 * it + colour)
        every = np.ones(len(xs), dtype=bool)
        offer(w * (1.0 + rho * (2.0 * rand(k, 0) - 1.0)), a.copy(), b.copy(), every)
        delta = (S.sigma[i] * w) * half_it
        offer(w.copy(), a + delta * (2.0 * rand(k, 1) - 1.0), b + delta * (2.0 * rand(k, 2) - 1.0), every)
        delta = (S.sigma[i] * w) * half_it
        offer(w * (1.0 + rho * (2.0 * rand(k, 3) - 1.0)), a + delta * (2.0 * rand(k, 4) - 1.0), b + delta * (2.0 * rand(k, 5) - 1.0), every)
        offer(*draw(S, i, k, 6), every)
        plane[i, ys, xs] = np.stack([w, a, b], axis=1)
        cst[i, ys, xs] = c.astype(np.int32)


def finish(S, plane, cst):
    """-> (depth float64, normal float64 (V, H, W, 3), status uint8)."""
    xs, ys = np.meshgrid(np.arange(S.W, dtype=np.float64), np.arange(S.H, dtype=np.float64))
    depth, normal, status = np.full(cst.shape, np.nan), np.full(plane.shape, np.nan), np.zeros(cst.shape, dtype=np.uint8)
    for i in range(S.V):
        st = np.where(~S.strict, NOT_STRICT, np.where(cst[i] >= S.tau * len(S.lists[i]), NO_VIEW, 0)).astype(np.uint8)
        fx, cx, fy, cy = S.K[i]
        w, a, b = plane[i, ..., 0], plane[i, ..., 1], plane[i, ..., 2]
        with np.errstate(all="ignore"):
            m = [a * fx, b * fy, (w + a * (cx - xs)) + b * (cy - ys)]
            l = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            n = np.stack([-m[0] / l, -m[1] / l, -m[2] / l], axis=-1)
            d = 1.0 / w
        status[i], depth[i], normal[i] = st, np.where(st == 0, d, np.nan), np.where((st == 0)[..., None], n, np.nan)
    return depth, normal, status


def patchmatch(images, K, ext, neighbours, depth_range, depth=None, planes=None, iterations=3, first_iteration=0, census=(7, 7), stride=2, truncate=None, max_slant=70.0,
               seed=0, probe=None):
    """-> dict(depth float64 (V, H, W), normal float64 (V, H, W, 3), plane float64 (V, H, W, 3), cost int32, status uint8)."""
    S = Setup(images, K, ext, neighbours, depth_range, census, stride, truncate, max_slant, seed)
    plane, cst = initialise(S, depth, planes, probe)
    for it in range(first_iteration, first_iteration + iterations):
        for colour in (0, 1):
            half_iteration(S, plane, cst, it, colour, probe)
    d, n, st = finish(S, plane, cst)
    return dict(depth=d, normal=n, plane=plane, cost=cst, status=st)


def decision_margins(**case):
    """A run of ``patchmatch`` that looks at every sample it evaluates (those the device skips behind the first invalid sample of a
    window included): how close 16 u + 0.5 and 16 v + 0.5 come to an integer, n_2 and omega to 0, and how far float64 is from longdouble
    in the same quantities.  -> dict(closest_t, gap_t (sixteenths), closest_n2, gap_n2, closest_om, gap_om, samples)."""
    probe = new_probe()
    patchmatch(**case, probe=probe)
    return probe


# ---- the same rule with Python scalars ---------------------------------------------------------------------------------------------------
def patchmatch_loops(images, K, ext, neighbours, depth_range, depth=None, planes=None, iterations=3, first_iteration=0, census=(7, 7), stride=2, truncate=None,
                     max_slant=70.0, seed=0):
    S = Setup(images, K, ext, neighbours, depth_range, census, stride, truncate, max_slant, seed)
    V, H, W, s, tau = S.V, S.H, S.W, S.s, S.tau
    I = [[[int(v) for v in row] for row in img] for img in S.images]
    warps = [[([[float(v) for v in row] for row in A], [float(v) for v in b]) for A, b in per] for per in S.warps]
    nan = math.nan
    plane = [[[(nan, nan, nan) for _ in range(W)] for _ in range(H)] for _ in range(V)]
    cst = [[[-1] * W for _ in range(H)] for _ in range(V)]

    def key(i, x, y, t):
        k = mix_int((S.seed + GOLDEN) & MASK)
        k = mix_int(k ^ i)
        k = mix_int(k ^ (y * W + x))
        return mix_int(k ^ t)

    def r(k, d):
        return float(mix_int((k + (d + 1) * GOLDEN) & MASK) >> 11) * 2.0 ** -53

    def adm(i, p):
        lo, hi = (float(v) for v in S.wrange[i])
        sw = float(S.sigma[i]) * p[0]
        return lo <= p[0] <= hi and abs(p[1]) <= sw and abs(p[2]) <= sw   # a comparison with a NaN is False

    def fresh(i, k, d):
        lo, hi = (float(v) for v in S.wrange[i])
        w = lo + r(k, d) * (hi - lo)
        sw = float(S.sigma[i]) * w
        return (w, sw * (2.0 * r(k, d + 1) - 1.0), sw * (2.0 * r(k, d + 2) - 1.0))

    def g_of(i, slot, p, x, y, sx, sy):
        """the warped sample, None where invalid"""
        A, b = warps[i][slot]
        om = (p[0] + p[1] * float(sx)) + p[2] * float(sy)
        xd, yd = float(x + sx), float(y + sy)
        n = [((A[c][0] * xd + A[c][1] * yd) + A[c][2]) + om * b[c] for c in range(3)]
        if not (om > 0 and n[2] > 0):
            return None
        tu, tv = 16.0 * (n[0] / n[2]) + 0.5, 16.0 * (n[1] / n[2]) + 0.5
        if not (math.isfinite(tu) and math.isfinite(tv)):   # an infinite coordinate lies outside, a NaN fails every comparison
            return None
        qu, qv = math.floor(tu), math.floor(tv)
        if not (0 <= qu < 16 * (W - 1) and 0 <= qv < 16 * (H - 1)):
            return None
        x0, fx, y0, fy = qu >> 4, qu & 15, qv >> 4, qv & 15
        Ij = I[S.lists[i][slot]]
        return (16 - fx) * (16 - fy) * Ij[y0][x0] + fx * (16 - fy) * Ij[y0][x0 + 1] + (16 - fx) * fy * Ij[y0 + 1][x0] + fx * fy * Ij[y0 + 1][x0 + 1]

    def C_of(i, p, x, y):
        total = 0
        for slot in range(len(S.lists[i])):
            centre = g_of(i, slot, p, x, y, 0, 0)
            h = None if centre is None else 0
            for dx, dy in S.window:
                if h is None:
                    break
                g = g_of(i, slot, p, x, y, s * dx, s * dy)
                if g is None:
                    h = None
                else:
                    h += int(g < centre) != int(I[i][y + s * dy][x + s * dx] < I[i][y][x])
            total += tau if h is None else min(tau, h)
        return total

    for i in range(V):
        lo, hi = (float(v) for v in S.wrange[i])
        for y in range(H):
            for x in range(W):
                if not S.is_strict(x, y):
                    continue
                p = None
                if planes is not None:
                    q = tuple(float(v) for v in planes[i][y][x])
                    p = q if adm(i, q) else None
                elif depth is not None:
                    d = float(depth[i][y][x])
                    if math.isfinite(d) and d > 0:
                        p = (min(max(1.0 / d, lo), hi), 0.0, 0.0)
                if p is None:
                    p = fresh(i, key(i, x, y, 0), 0)
                plane[i][y][x], cst[i][y][x] = p, C_of(i, p, x, y)
    for it in range(first_iteration, first_iteration + iterations):
        rho, half_it = 2.0 ** -(2 + it), 2.0 ** -(1 + it)
        for colour in (0, 1):
            before = [[row[:] for row in pl] for pl in plane]
            for i in range(V):
                sig = float(S.sigma[i])
                for y in range(H):
                    for x in range(W):
                        if not S.is_strict(x, y) or (x + y) & 1 != colour:
                            continue
                        cur, c = plane[i][y][x], cst[i][y][x]
                        k = key(i, x, y, 1 + 2 * it + colour)
                        for n_c in range(12):
                            if n_c < 8:
                                ox, oy = OFFSETS[n_c]
                                if not S.is_strict(x + ox, y + oy):
                                    continue
                                q = before[i][y + oy][x + ox]
                                cand = ((q[0] - q[1] * float(ox)) - q[2] * float(oy), q[1], q[2])
                            elif n_c == 11:
                                cand = fresh(i, k, 6)
                            else:
                                w, a, b = cur
                                delta = (sig * w) * half_it
                                if n_c == 8:
                                    cand = (w * (1.0 + rho * (2.0 * r(k, 0) - 1.0)), a, b)
                                elif n_c == 9:
                                    cand = (w, a + delta * (2.0 * r(k, 1) - 1.0), b + delta * (2.0 * r(k, 2) - 1.0))
                                else:
                                    cand = (w * (1.0 + rho * (2.0 * r(k, 3) - 1.0)), a + delta * (2.0 * r(k, 4) - 1.0), b + delta * (2.0 * r(k, 5) - 1.0))
                            if adm(i, cand):
                                C = C_of(i, cand, x, y)
                                if C < c:
                                    cur, c = cand, C
                        plane[i][y][x], cst[i][y][x] = cur, c
    P, Cn = np.array(plane, dtype=np.float64).reshape(V, H, W, 3), np.array(cst, dtype=np.int32).reshape(V, H, W)
    d, n, st = finish(S, P, Cn)
    return dict(depth=d, normal=n, plane=P, cost=Cn, status=st)
