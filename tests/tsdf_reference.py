"""The TSDF volume and surface-nets rule of include/pcs_hip.h ("TSDF volume and surface extraction", csrc/ba_tsdf.hpp) restated in NumPy:
TEST INFRASTRUCTURE.

Two forms of the same rule.  ``integrate`` / ``extract`` work on whole grids with masks and take the arithmetic type (float64 or
``np.longdouble``); ``integrate_loop`` / ``extract_loop`` walk node by node and cell by cell with early exits, plain indexing and Python
floats (IEEE doubles).  Every formula is written in the order the header states (plain IEEE operations, sums of three products left to
right), so the two forms agree bit for bit in float64.

Both also return the CLOSEST CALL, as tests/fusion_reference.py does: over every decision taken, the smallest distance to its threshold,
each relative to the quantity's scale.  The decisions, in the order a (node, view) test meets them (a later one is taken only when the
earlier ones passed):
  sign of Y_z          |Y_z| / (|R20 X0| + |R21 X1| + |R22 X2| + |t2|)
  rounding             the distance of u + 0.5 (and v + 0.5) to the nearest integer, / s_u = |fx| max(|Y_x / Y_z|, 1) + |cx| (s_v alike)
  image bounds         the distance of u + 0.5 to 0 and W (v + 0.5 to 0 and H), / W (H)
  sdf >= -trunc        |sdf + trunc| / max(d, Y_z)
and at extraction, for every observed node,
  D < 0                |D| / the node's scale: the largest max(d, Y_z) / trunc over the tests that added to it (at least 1), the size of
                       the terms whose difference D is.
``integrate`` returns the quantities themselves too (``decisions``, each divided by its scale, NaN where the decision was not taken), and
``extract`` returns D over its scale (``decision``); tests/tsdf_inputs.py measures TSDF_DECISION_GAP from them."""
import math

import numpy as np

MAX_DIM, MAX_WEIGHT = 1024, 65535
EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))   # the order the crossings are added in
RING = ((-1, -1), (0, -1), (0, 0), (-1, 0))   # (dU, dV) of the four cells around a grid edge
UV = ((1, 2), (2, 0), (0, 1))                 # (U, V) of edge axis A


def corner(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


class Volume:
    """sum (nz, ny, nx) of ``sum_dtype`` and weight uint16, both 0; ``scale`` (float64, not part of the rule) is what the D < 0
    decision of a node is measured against; ``n_integrated`` the number of views integrated so far."""

    def __init__(self, origin, voxel, dims, sum_dtype=np.float32):
        nx, ny, nz = (int(d) for d in dims)
        assert all(1 <= d <= MAX_DIM for d in (nx, ny, nz)) and voxel > 0
        self.origin, self.voxel, self.dims = tuple(float(o) for o in origin), float(voxel), (nx, ny, nz)
        self.sum = np.zeros((nz, ny, nx), dtype=sum_dtype)
        self.weight = np.zeros((nz, ny, nx), dtype=np.uint16)
        self.scale = np.ones((nz, ny, nx))
        self.n_integrated = 0

    def copy(self):
        v = Volume(self.origin, self.voxel, self.dims, self.sum.dtype)
        v.sum, v.weight, v.scale, v.n_integrated = self.sum.copy(), self.weight.copy(), self.scale.copy(), self.n_integrated
        return v


def valid_depth(z):
    return np.isfinite(z) & (z > 0)


def to_view(P, X0, X1, X2):
    """Y = R X + t; P = [R | t] row-major (12)"""
    return ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3], ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7], ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11]


def project(K, Y0, Y1, Y2):
    return K[0] * (Y0 / Y2) + K[1], K[2] * (Y1 / Y2) + K[3]


def _views(views, V):
    lst = list(range(V)) if views is None else [int(v) for v in views]
    assert all(0 <= v < V for v in lst)
    return lst


def integrate(vol, depth, K, ext, trunc, views=None, dtype=np.float64):
    """The vectorised form; ``vol`` is updated in place.  depth (V, H, W) float32 / float64; K (V, 4); ext (V, 3, 4) or (V, 12).
    -> dict(closest, decisions (4 + 1, len(list), nz, ny, nx): Y_z, u + 0.5, v + 0.5, sdf + trunc, each over its scale)."""
    T = np.dtype(dtype).type
    D = np.asarray(depth)
    assert D.ndim == 3 and D.dtype in (np.float32, np.float64) and trunc > 0
    V, H, W = D.shape
    Kt, Pt = np.asarray(K, dtype=np.float64).reshape(V, 4).astype(T), np.asarray(ext, dtype=np.float64).reshape(V, 12).astype(T)
    lst = _views(views, V)
    assert vol.n_integrated + len(lst) <= MAX_WEIGHT
    nx, ny, nz = vol.dims
    o, s, tr, half, one = [T(c) for c in vol.origin], T(vol.voxel), T(trunc), T(0.5), T(1.0)
    kk, jj, ii = np.meshgrid(np.arange(nz).astype(T), np.arange(ny).astype(T), np.arange(nx).astype(T), indexing="ij")
    X0, X1, X2 = o[0] + s * ii, o[1] + s * jj, o[2] + s * kk
    S, Wt = vol.sum.astype(T), vol.weight.astype(np.int64)
    dec = np.full((4, len(lst)) + S.shape, np.nan, dtype=T)
    closest = np.inf

    def near(a, reached):
        nonlocal closest
        a = np.asarray(a, dtype=np.float64)[reached]
        if a.size:
            closest = min(closest, float(np.min(a)))

    with np.errstate(all="ignore"):
        for n, v in enumerate(lst):
            Y0, Y1, Y2 = to_view(Pt[v], X0, X1, X2)
            s1 = np.abs(Pt[v][8] * X0) + np.abs(Pt[v][9] * X1) + np.abs(Pt[v][10] * X2) + np.abs(Pt[v][11])
            dec[0, n] = Y2 / s1
            near(np.abs(Y2) / s1, np.ones(S.shape, dtype=bool))
            ok = Y2 > 0
            u, w = project(Kt[v], Y0, Y1, Y2)
            ur, wr = u + half, w + half
            su = np.abs(Kt[v][0]) * np.maximum(np.abs(Y0 / Y2), 1) + np.abs(Kt[v][1])
            sw = np.abs(Kt[v][2]) * np.maximum(np.abs(Y1 / Y2), 1) + np.abs(Kt[v][3])
            dec[1, n], dec[2, n] = np.where(ok, ur / su, np.nan), np.where(ok, wr / sw, np.nan)
            near(np.abs(ur - np.rint(ur)) / su, ok)
            near(np.abs(wr - np.rint(wr)) / sw, ok)
            near(np.minimum(np.abs(ur), np.abs(ur - W)) / W, ok)
            near(np.minimum(np.abs(wr), np.abs(wr - H)) / H, ok)
            fu, fw = np.floor(ur), np.floor(wr)
            ok = ok & (fu >= 0) & (fu < W) & (fw >= 0) & (fw < H)
            qx, qy = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fw, 0).astype(np.int64)
            d = np.where(ok, D[v][qy, qx].astype(T), 0)
            ok = ok & valid_depth(d)
            sdf = d - Y2
            sc = np.maximum(d, Y2)
            dec[3, n] = np.where(ok, (sdf + tr) / sc, np.nan)
            near(np.abs(sdf + tr) / sc, ok)
            ok = ok & (sdf >= -tr)
            S = np.where(ok, S + np.minimum(one, sdf / tr), S)
            Wt = Wt + ok
            vol.scale = np.where(ok, np.maximum(vol.scale, (sc / tr).astype(np.float64)), vol.scale)
    vol.sum, vol.weight = S.astype(vol.sum.dtype), Wt.astype(np.uint16)
    vol.n_integrated += len(lst)
    return dict(closest=closest, decisions=dec)


def integrate_loop(vol, depth, K, ext, trunc, views=None):
    """The plain loop form in float64 (Python floats): one node, one view at a time, leaving at the first failed step.  -> dict(closest)."""
    D = np.asarray(depth)
    V, H, W = D.shape
    Kl, Pl = np.asarray(K, dtype=np.float64).reshape(V, 4).tolist(), np.asarray(ext, dtype=np.float64).reshape(V, 12).tolist()
    lst = _views(views, V)
    assert vol.n_integrated + len(lst) <= MAX_WEIGHT
    nx, ny, nz = vol.dims
    o, s, tr = vol.origin, vol.voxel, float(trunc)
    closest = math.inf
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                X0, X1, X2 = o[0] + s * float(i), o[1] + s * float(j), o[2] + s * float(k)
                S, Wn, scale = float(vol.sum[k, j, i]), int(vol.weight[k, j, i]), float(vol.scale[k, j, i])
                for v in lst:
                    P, Kv = Pl[v], Kl[v]
                    Y0, Y1, Y2 = to_view(P, X0, X1, X2)
                    closest = min(closest, abs(Y2) / (abs(P[8] * X0) + abs(P[9] * X1) + abs(P[10] * X2) + abs(P[11])))
                    if not Y2 > 0:
                        continue
                    u, w = project(Kv, Y0, Y1, Y2)
                    ur, wr = u + 0.5, w + 0.5
                    su, sw = abs(Kv[0]) * max(abs(Y0 / Y2), 1) + abs(Kv[1]), abs(Kv[2]) * max(abs(Y1 / Y2), 1) + abs(Kv[3])
                    if not (math.isfinite(ur) and math.isfinite(wr)):
                        continue
                    closest = min(closest, abs(ur - round(ur)) / su, abs(wr - round(wr)) / sw, min(abs(ur), abs(ur - W)) / W, min(abs(wr), abs(wr - H)) / H)
                    fu, fw = math.floor(ur), math.floor(wr)
                    if not (0 <= fu < W and 0 <= fw < H):
                        continue
                    d = float(D[v, fw, fu])
                    if not (math.isfinite(d) and d > 0):
                        continue
                    sdf = d - Y2
                    closest = min(closest, abs(sdf + tr) / max(d, Y2))
                    if not sdf >= -tr:
                        continue
                    S, Wn, scale = S + min(1.0, sdf / tr), Wn + 1, max(scale, max(d, Y2) / tr)
                vol.sum[k, j, i], vol.weight[k, j, i], vol.scale[k, j, i] = S, Wn, scale
    vol.n_integrated += len(lst)
    return dict(closest=closest)


def extract(vol, min_weight=2, dtype=np.float64):
    """The vectorised form.  -> dict(vertices (n_v, 3) of ``dtype`` (not rounded to float32), quads (n_q, 4) int32, active (cells),
    inside, observed, D, closest, decision (D over the node's scale, NaN where not observed))."""
    T = np.dtype(dtype).type
    assert 1 <= min_weight <= MAX_WEIGHT
    nx, ny, nz = vol.dims
    obs = vol.weight >= min_weight
    with np.errstate(all="ignore"):
        D = vol.sum.astype(T) / vol.weight.astype(T)
    inside = obs & (D < 0)
    decision = np.where(obs, D / vol.scale.astype(T), np.nan)
    closest = float(np.min(np.abs(decision[obs]))) if obs.any() else np.inf
    cz, cy, cx = max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)
    sub = lambda a, c: a[corner(c)[2]:corner(c)[2] + cz, corner(c)[1]:corner(c)[1] + cy, corner(c)[0]:corner(c)[0] + cx]
    n_obs = sum(sub(obs, c).astype(np.int64) for c in range(8))
    n_in = sum(sub(inside, c).astype(np.int64) for c in range(8))
    active = (n_obs == 8) & (n_in > 0) & (n_in < 8) if cz * cy * cx else np.zeros((cz, cy, cx), dtype=bool)
    acc = [np.zeros((cz, cy, cx), dtype=T) for _ in range(3)]
    cnt = np.zeros((cz, cy, cx), dtype=np.int64)
    with np.errstate(all="ignore"):
        for a, b in EDGES:
            cross = active & (sub(inside, a) != sub(inside, b))
            Da, Db = sub(D, a), sub(D, b)
            t = Da / (Da - Db)
            axis = (b - a).bit_length() - 1
            for c in range(3):
                p = t if c == axis else T(corner(a)[c])
                acc[c] = np.where(cross, acc[c] + p, acc[c])
            cnt = cnt + cross
        kk, jj, ii = np.nonzero(active)   # row-major: the order of the cells' linear index
        m = cnt[kk, jj, ii].astype(T)
        o, s = [T(c) for c in vol.origin], T(vol.voxel)
        verts = np.stack([o[0] + s * (ii.astype(T) + acc[0][kk, jj, ii] / m), o[1] + s * (jj.astype(T) + acc[1][kk, jj, ii] / m),
                          o[2] + s * (kk.astype(T) + acc[2][kk, jj, ii] / m)], axis=-1).reshape(-1, 3)
    number = np.full((cz, cy, cx), -1, dtype=np.int64)
    number[kk, jj, ii] = np.arange(len(kk))
    quads = []
    dims = (nx, ny, nz)
    for A in range(3):
        U, Vx = UV[A]
        e = [0, 0, 0]
        e[A] = 1
        flag = np.zeros((nz, ny, nx), dtype=bool)
        lo = [slice(0, dims[c] - e[c]) for c in range(3)]
        hi = [slice(e[c], dims[c]) for c in range(3)]
        flag[lo[2], lo[1], lo[0]] = obs[lo[2], lo[1], lo[0]] & obs[hi[2], hi[1], hi[0]] & (inside[lo[2], lo[1], lo[0]] != inside[hi[2], hi[1], hi[0]])
        kq, jq, iq = np.nonzero(flag)   # node linear order
        n = np.stack([iq, jq, kq])
        ids = []
        ok = np.ones(len(iq), dtype=bool)
        for dU, dV in RING:
            c = n.copy()
            c[U] += dU
            c[Vx] += dV
            inb = np.ones(len(iq), dtype=bool)
            for ax in range(3):
                inb &= (c[ax] >= 0) & (c[ax] < dims[ax] - 1)
            cc = np.where(inb, c, 0)
            num = np.where(inb, number[cc[2], cc[1], cc[0]] if cz * cy * cx else -1, -1)
            ok &= num >= 0
            ids.append(num)
        q = np.stack(ids, axis=-1).reshape(-1, 4)
        q = np.where(inside[kq, jq, iq][:, None], q, q[:, ::-1])
        quads.append(q[ok])
    quads = np.concatenate(quads).astype(np.int32).reshape(-1, 4)
    return dict(vertices=verts, quads=quads, active=active, inside=inside, observed=obs, D=D, closest=closest, decision=decision)


def extract_loop(vol, min_weight=2):
    """The plain loop form in float64 (Python floats).  -> dict(vertices (n_v, 3) float64, quads (n_q, 4) int32, closest)."""
    nx, ny, nz = vol.dims
    o, s = vol.origin, vol.voxel
    S, Wt = vol.sum.astype(np.float64).tolist(), vol.weight.tolist()
    closest = math.inf
    D = [[[None] * nx for _ in range(ny)] for _ in range(nz)]   # None: not observed
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                if Wt[k][j][i] >= min_weight:
                    D[k][j][i] = S[k][j][i] / float(Wt[k][j][i])
                    closest = min(closest, abs(D[k][j][i]) / float(vol.scale[k, j, i]))
    number, verts = {}, []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                Dc = [D[k + corner(c)[2]][j + corner(c)[1]][i + corner(c)[0]] for c in range(8)]
                if any(d is None for d in Dc):
                    continue
                ins = [d < 0 for d in Dc]
                if all(ins) or not any(ins):
                    continue
                acc, cnt = [0.0, 0.0, 0.0], 0
                for a, b in EDGES:
                    if ins[a] == ins[b]:
                        continue
                    p = [float(x) for x in corner(a)]
                    p[(b - a).bit_length() - 1] = Dc[a] / (Dc[a] - Dc[b])
                    acc = [acc[c] + p[c] for c in range(3)]
                    cnt += 1
                number[(i, j, k)] = len(verts)
                verts.append((o[0] + s * (float(i) + acc[0] / float(cnt)), o[1] + s * (float(j) + acc[1] / float(cnt)), o[2] + s * (float(k) + acc[2] / float(cnt))))
    quads = []
    for A in range(3):
        U, Vx = UV[A]
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    n = [i, j, k]
                    m = list(n)
                    m[A] += 1
                    if m[A] >= (nx, ny, nz)[A]:
                        continue
                    Da, Db = D[k][j][i], D[m[2]][m[1]][m[0]]
                    if Da is None or Db is None or (Da < 0) == (Db < 0):
                        continue
                    ids = []
                    for dU, dV in RING:
                        c = list(n)
                        c[U] += dU
                        c[Vx] += dV
                        ids.append(number.get(tuple(c)))
                    if any(x is None for x in ids):
                        continue
                    quads.append(ids if Da < 0 else ids[::-1])
    return dict(vertices=np.array(verts, dtype=np.float64).reshape(-1, 3), quads=np.array(quads, dtype=np.int32).reshape(-1, 4), closest=closest)
