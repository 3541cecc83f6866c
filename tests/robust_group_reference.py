"""NumPy restatement of the robust instantiations of the two group-LM kernels (csrc/ba_rigpose.hpp, csrc/ba_tri_refine.hpp;
include/pcs_hip.h pcs_rigpose_set_loss, pcs_tri_set_refine_loss), one group at a time.  Rows and sums are those of
tests/rigpose_reference.py and tests/tri_refine_reference.py, imported, not copied; the trial loop is theirs, restated once for both
with the sums as a function: damping, accept rule, stops and status codes are unchanged, the rows are scaled by scipy's
linearisation of the loss and the cost every rule looks at is sum rho0.

``robust_scale`` is the device's ``robust_rho`` (csrc/ba_device.hpp): with z = (f / f_scale)^2 per scalar residual f,
s = sqrt(max(rho'(z) + 2 z rho''(z), EPS)), row of J -> s J, f -> rho'(z) f / s, rho0 = f_scale^2 rho(z)."""
from __future__ import annotations

import numpy as np

from tests import rigpose_reference as rig
from tests import tri_refine_reference as tri
from tests.pnp_reference import _ldl_solve, rodrigues, rotvec_of

KINDS = ("huber", "soft_l1", "cauchy", "arctan")
EPS = np.finfo(np.float64).eps
NOT_ESTIMATED, CONVERGED, MAX_ITER, NO_DECREASE = 0, 1, 2, 3
LAMBDA0, LAMBDA_MAX, LAMBDA_MIN = 1e-4, 1e10, 1e-15
assert (rig.LAMBDA0, rig.LAMBDA_MAX, rig.LAMBDA_MIN) == (tri.LAMBDA0, tri.LAMBDA_MAX, tri.LAMBDA_MIN) == (LAMBDA0, LAMBDA_MAX, LAMBDA_MIN)


def rho(f, kind, f_scale):
    """(rho0, rho1, rho2) per scalar residual in scipy's convention: f_scale^2 rho(z), rho'(z), rho''(z) / f_scale^2."""
    f = np.asarray(f, dtype=np.float64)
    z = (f / f_scale) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "linear":
            r0, r1, r2 = z, np.ones_like(z), np.zeros_like(z)
        elif kind == "huber":
            inside = z <= 1.0
            sq = np.sqrt(z)
            r0 = np.where(inside, z, 2.0 * sq - 1.0)
            r1 = np.where(inside, 1.0, 1.0 / sq)
            r2 = np.where(inside, 0.0, -0.5 * r1 / z)
        elif kind == "soft_l1":
            t = 1.0 + z
            st = np.sqrt(t)
            r0, r1 = 2.0 * (st - 1.0), 1.0 / st
            r2 = -0.5 * r1 / t
        elif kind == "cauchy":
            r0, r1 = np.log1p(z), 1.0 / (1.0 + z)
            r2 = -r1 * r1
        elif kind == "arctan":
            r0, r1 = np.arctan(z), 1.0 / (1.0 + z * z)
            r2 = -2.0 * z * r1 * r1
        else:
            raise ValueError(kind)
    return f_scale ** 2 * r0, r1, r2 / f_scale ** 2


def robust_scale(f, kind, f_scale):
    """-> (s, rf, rho0): the row scale, the scaled residual rho1 f / s and rho0, per scalar residual."""
    f = np.asarray(f, dtype=np.float64)
    r0, r1, r2 = rho(f, kind, f_scale)
    js = r1 + 2.0 * r2 * f * f
    s = np.sqrt(np.where(js < EPS, EPS, js))     # keeps a NaN, as the device's clamp does
    return s, r1 * f / s, r0


def scaled_sums(r, J, kind, f_scale):
    """From raw residuals (n, 2) and Jacobian (2 n, p): H = sum s^2 J'J, g = sum J' rho1 f, sum rho0, sum r^2."""
    f = r.reshape(-1)
    s, rf, r0 = robust_scale(f, kind, f_scale)
    Js = J * s[:, None]
    return Js.T @ Js, Js.T @ rf, float(np.sum(r0)), float(np.sum(f * f))


# ---- the trial loop of both kernels -----------------------------------------------------------------------------------------------
def lm_group(x0, evaluate, advance, size, solve, max_iter, ftol, xtol, gtol):
    """``evaluate(x) -> (H, g, cost, bad, raw)``, ``advance(x, d) -> x``, ``size(x)`` the length xtol compares a step with,
    ``solve(A, g) -> d or None``.  -> dict(x, it, status, cost, cost0, raw, raw0, H, moved); status NOT_ESTIMATED when the start is
    unusable (a non-finite cost or a point behind its camera)."""
    x = x0
    H, g, cost, bad, raw = evaluate(x)
    out = dict(x=x, it=0, status=NOT_ESTIMATED, cost=cost, cost0=cost, raw=raw, raw0=raw, H=H, moved=False)
    if not (np.isfinite(cost) and bad == 0):
        return out
    lam = LAMBDA0

    def done(status):
        out.update(x=x, status=status, cost=cost, raw=raw, H=H)
        return out

    while True:
        if np.max(np.abs(g)) <= gtol:
            return done(CONVERGED)
        if out["it"] >= max_iter:
            return done(MAX_ITER)
        d = solve(H + lam * np.diag(np.diag(H)), g)
        if d is None:
            return done(NO_DECREASE)
        xt = advance(x, d)
        Ht, gt, ct, badt, rawt = evaluate(xt)
        out["it"] += 1
        small = np.sqrt(d @ d) <= xtol * (xtol + size(x))
        if badt == 0 and ct < cost:
            flat = cost - ct <= ftol * cost
            x, H, g, cost, raw = xt, Ht, gt, ct, rawt
            out["moved"] = True
            lam = max(lam * 0.1, LAMBDA_MIN)
            if flat or small:
                return done(CONVERGED)
        else:
            lam *= 10.0
            if small:
                return done(CONVERGED)
            if lam > LAMBDA_MAX:
                return done(NO_DECREASE)


# ---- rig pose ----------------------------------------------------------------------------------------------------------------------
def rigpose_sums(R, t, X, uv, cams, intr, ext, kind, f_scale):
    r, J, bad = rig._rows(R, t, X, uv, cams, intr, ext)
    return scaled_sums(r, J, kind, f_scale) + (bad,)


def lm_image_pose(pose0, X, uv, cams, intr, ext, kind="linear", f_scale=1.0, max_iter=10, ftol=1e-10, xtol=1e-10, gtol=0.0):
    """The device's per-image LM under a loss.  -> dict(pose, it, status, cost, cost0 (sum rho0), raw, raw0 (sum r^2), H); a pose that
    never moved keeps the start's bits; NOT_ESTIMATED: NaN pose."""
    pose0 = np.asarray(pose0, dtype=np.float64)
    nan = dict(pose=np.full(6, np.nan), it=0, status=NOT_ESTIMATED, cost=np.nan, cost0=np.nan, raw=np.nan, raw0=np.nan, H=np.full((6, 6), np.nan))
    if not np.all(np.isfinite(pose0)):
        return nan

    def evaluate(x):
        H, g, c, raw, bad = rigpose_sums(x[0], x[1], X, uv, cams, intr, ext, kind, f_scale)
        return H, g, c, bad, raw

    def solve(A, g):
        return _ldl_solve(A, g)

    o = lm_group((rodrigues(pose0[:3]), pose0[3:].copy()), evaluate, lambda x, d: (rodrigues(d[:3]) @ x[0], x[1] + d[3:]),
                 lambda x: np.sqrt(3.0 + x[1] @ x[1]), solve, max_iter, ftol, xtol, gtol)
    if o["status"] == NOT_ESTIMATED:
        return nan
    R, t = o["x"]
    o["pose"] = np.concatenate([rotvec_of(R), t]) if o["moved"] else pose0.copy()
    return o


class Result:
    pass


def localise_target(dct, points, intr, ext, poses_init, kind="linear", f_scale=1.0, n_imgs=None, min_points=6, **opts):
    """The whole table through ``lm_image_pose``: the fields of ``compiled_helpers.ImagePoses`` (``residuals`` in the order of the
    SORTED table ``table``; ``cost`` / ``cost_init`` = 0.5 sum rho0)."""
    d = np.asarray(dct, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    poses_init = np.asarray(poses_init, dtype=np.float64)
    I = poses_init.shape[0] if n_imgs is None else n_imgs
    out = Result()
    out.poses, out.poses_init = np.full((I, 6), np.nan), poses_init.copy()
    out.rms, out.rms_init, out.cost, out.cost_init = (np.full(I, np.nan) for _ in range(4))
    out.status, out.iterations, out.n_points, out.n_cams = (np.zeros(I, dtype=np.int32) for _ in range(4))
    out.hessian = np.full((I, 6, 6), np.nan)
    ds, ids, start = rig.group_images(d)
    out.table, out.residuals = ds, np.full((ds.shape[0], 2), np.nan)
    for k, i in enumerate(ids):
        rows = ds[start[k]:start[k + 1]]
        n = rows.shape[0]
        cams, keys, uv = rows[:, 0].astype(np.int64), rows[:, 2].astype(np.int64), rows[:, 3:5]
        out.n_points[i], out.n_cams[i] = n, np.unique(cams).shape[0]
        if n < min_points:
            continue
        o = lm_image_pose(poses_init[i], points[keys], uv, cams, intr, ext, kind, f_scale, **opts)
        if o["status"] == NOT_ESTIMATED:
            continue
        out.poses[i], out.iterations[i], out.status[i], out.hessian[i] = o["pose"], o["it"], o["status"], o["H"]
        out.rms[i], out.rms_init[i] = np.sqrt(o["raw"] / n), np.sqrt(o["raw0"] / n)
        out.cost[i], out.cost_init[i] = 0.5 * o["cost"], 0.5 * o["cost0"]
        out.residuals[start[k]:start[k + 1]] = rig.image_residuals(o["pose"], points[keys], uv, cams, intr, ext)
    return out


def robust_hessian_at(pose, X, uv, cams, intr, ext, kind, f_scale, dtype=np.float64):
    """sum s^2 J'J at a pose vector with rows and scales carried in ``dtype`` (np.longdouble: the yardstick of the device's robust
    Hessian; the rational parts of the loss are evaluated in that precision, only the comparison z <= 1 of huber is a decision)."""
    R = rodrigues(np.asarray(pose[:3], dtype=np.float64))
    if dtype is not np.float64:
        r = np.asarray(pose[:3], dtype=dtype)
        th2 = r @ r
        th = np.sqrt(th2)
        Kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dtype)
        s, c = np.sin(th / 2), np.cos(th / 2)
        A, B = (1 - th2 / 6, dtype(0.5) - th2 / 24) if th2 < 1e-16 else (2 * s * c / th, 2 * s * s / th2)
        R = np.eye(3, dtype=dtype) + A * Kx + B * (np.outer(r, r) - th2 * np.eye(3, dtype=dtype))
    res, J, _ = rig._rows(R.astype(dtype), np.asarray(pose[3:], dtype=dtype), X, uv, cams, intr, ext, dtype)
    f = res.reshape(-1)
    fs = dtype(f_scale)
    z = (f / fs) ** 2
    one = dtype(1)
    if kind == "huber":
        js = np.where(z <= 1, one, 0 * one)    # outside: rho1 + 2 z rho2 = 1 / sqrt z - 1 / sqrt z = 0
    elif kind == "soft_l1":
        js = 1 / np.sqrt(1 + z) - z / ((1 + z) * np.sqrt(1 + z))
    elif kind == "cauchy":
        js = 1 / (1 + z) - 2 * z / (1 + z) ** 2
    elif kind == "arctan":
        js = 1 / (1 + z * z) - 4 * z * z / (1 + z * z) ** 2
    else:
        js = np.ones_like(z)
    js = np.where(js < EPS, dtype(EPS), js)
    return (J * js[:, None]).T @ J


# ---- triangulation refinement --------------------------------------------------------------------------------------------------------
def tri_sums(X, cams, uv, P, K, D, kind, f_scale):
    r, depth = tri.residuals(X, cams, uv, P, K, D)
    J = np.concatenate([tri.jacobian(X, P[c], K[c], D[c]) for c in cams]) if len(cams) else np.zeros((0, 3))
    return scaled_sums(r, J, kind, f_scale) + (int(np.sum(~(depth > 0))),)


def refine_point(X0, cams, uv, P, K, D, kind="linear", f_scale=1.0, max_iter=10, ftol=1e-10, xtol=1e-10, gtol=0.0):
    """The device's per-point LM under a loss.  -> dict(X, it, status, cost, cost0 (sum rho0), raw, raw0 (sum r^2)); NOT_REFINED (0)
    returns the start unchanged.  The residual enters g with the sign of the restatement it extends: r = uv - pi, J = d pi / d X."""
    X0 = np.asarray(X0, dtype=np.float64).copy()

    def evaluate(x):
        H, g, c, raw, bad = tri_sums(x, cams, uv, P, K, D, kind, f_scale)
        return H, g, c, bad, raw

    def solve(A, g):
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None
        d = np.linalg.solve(L.T, np.linalg.solve(L, g))
        return d if np.all(np.isfinite(d)) else None

    if not (np.all(np.isfinite(X0)) and len(cams) > 0):
        with np.errstate(all="ignore"):
            _, _, c, bad, raw = evaluate(X0) if len(cams) else (0, 0, 0.0, 0, 0.0)
        return dict(X=X0, it=0, status=NOT_ESTIMATED, cost=c, cost0=c, raw=raw, raw0=raw)
    o = lm_group(X0, evaluate, lambda x, d: x + d, lambda x: np.linalg.norm(x), solve, max_iter, ftol, xtol, gtol)
    o["X"] = o["x"]
    return o
