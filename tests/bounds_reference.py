"""A NumPy restatement of the bounded Levenberg-Marquardt loop (include/pcs_hip.h pcs_set_bounds, DESIGN section 4 "Parameter bounds"),
written from the documented rules, not from the kernels: the loop of tests/lm_reference.py with the active set, the step cut at the first
bound, the cut step's predicted reduction and the stop rules of a cut trial.  It works on dense J and r over the FREE vector (the oracle
closures of tests/weights_reference.py, or a ChainProblem's own).

    fixed_eff, n   = active_set(x, g, lo, hi, fixed)      what bounds_active_kernel writes
    alpha, hit, x_new, delta = truncate(x, d, lo, hi)     what bounds_truncate_kernel writes, bit for bit
    res            = solve(fun, jac, x0, lo, hi, ...)     the whole loop; res.trials = one record per decided trial

tests/test_bounds_reference.py pins it against scipy on the CPU; tests/test_gpu_bounds.py compares the device against it."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import lm_reference as LR


def active_set(x, g, lo, hi, fixed=None, pin=None):
    """(fixed_eff as bool, number of entries the bounds added): fixed, or lo == hi, or on a bound with the gradient pointing out, or on
    a bound and pinned by an earlier trial (``pin``: the entries ``pinned`` named since the last accepted trial)."""
    x, g, lo, hi = (np.asarray(a, dtype=np.float64) for a in (x, g, lo, hi))
    fixed = np.zeros(x.shape[0], bool) if fixed is None else np.asarray(fixed).astype(bool)
    bound = (lo == hi) | ((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0))
    if pin is not None:
        bound = bound | (np.asarray(pin).astype(bool) & ((x <= lo) | (x >= hi)))
    return fixed | bound, int(np.count_nonzero(bound & ~fixed))


def pinned(x, d, lo, hi):
    """On (or beyond) a bound with the step pointing out of the box: the entry's own component of the step is dropped, and it takes no
    part in alpha (it would make alpha = 0 and stall the loop).  It is remembered (``solve``'s pin) until a trial is accepted: if this
    trial is rejected the next one holds the entry in its active set."""
    x, d, lo, hi = (np.asarray(a, dtype=np.float64) for a in (x, d, lo, hi))
    return ((d > 0.0) & (x >= hi)) | ((d < 0.0) & (x <= lo))


def fractions(x, d, lo, hi):
    """alpha_i: the fraction of d_i that takes x_i to the bound d_i moves towards (inf: none, or pinned)."""
    x, d, lo, hi = (np.asarray(a, dtype=np.float64) for a in (x, d, lo, hi))
    f = np.full(x.shape[0], np.inf)
    pin = pinned(x, d, lo, hi)
    up = (d > 0.0) & (hi < np.inf) & ~pin
    dn = (d < 0.0) & (lo > -np.inf) & ~pin
    with np.errstate(all="ignore"):
        f[up] = (hi[up] - x[up]) / d[up]
        f[dn] = (lo[dn] - x[dn]) / d[dn]
    return f


def truncate(x, d, lo, hi):
    """(alpha, index that set it or -1, x_new, delta).  alpha = min(1, min_i alpha_i), ties to the lowest index;
    x_new = min(max(x + alpha d, lo), hi) with the hitting entry exactly on its bound; delta = x_new - x — except that with alpha = 1
    an entry no bound touches keeps d and x + d as they are.  Pinned entries (``pinned``) stay where they are."""
    x, d, lo, hi = (np.asarray(a, dtype=np.float64) for a in (x, d, lo, hi))
    f = fractions(x, d, lo, hi)
    k = int(np.argmin(f)) if f.size else -1          # the first of equal minima
    cut = f.size > 0 and f[k] < 1.0
    alpha = float(f[k]) if cut else 1.0
    hit = k if cut else -1
    pin = pinned(x, d, lo, hi)
    t = x + alpha * np.where(pin, 0.0, d)
    c = np.minimum(np.maximum(t, lo), hi)
    if cut:
        c[hit] = hi[hit] if d[hit] > 0.0 else lo[hit]
    keep = np.isnan(t) | (((c == t) & ~pin) if not cut else np.zeros(x.shape[0], bool))
    x_new = np.where(keep, x + d, c)
    delta = np.where(keep, d, c - x)
    return alpha, hit, x_new, delta


def predicted_reduction(lam, dvec, gm, delta, alpha) -> float:
    """-(1 - alpha / 2) g'delta + 0.5 lam delta'D delta of the cut step, in long double, rounded once (alpha = 1: lm_reference's)."""
    L = LR.LD
    dvec, gm, delta = (np.asarray(a, dtype=L) for a in (dvec, gm, delta))
    return float(L(0.5) * L(lam) * np.sum(dvec * delta * delta) - (L(1.0) - L(0.5) * L(alpha)) * np.sum(gm * delta))


def decide(t: LR.TrialInputs, ctrl, alpha):
    """lm_reference.decide for a trial whose step kept the fraction ``alpha``: a cut trial (alpha < 1) triggers neither ftol nor xtol;
    it counts towards the limits and takes the damping rule as usual, except that an accepted cut trial never LOWERS lambda."""
    if not alpha < 1.0:
        return LR.decide(t, ctrl)
    c = np.array(ctrl, dtype=np.float64)
    c[LR.FTOL], c[LR.XTOL] = -np.inf, 0.0
    out = LR.decide(t, c)
    out.ctrl[LR.FTOL], out.ctrl[LR.XTOL] = ctrl[LR.FTOL], ctrl[LR.XTOL]
    if out.branch == "accept" and out.lam_next < t.lam:   # the gain ratio of a cut step says nothing about the whole one: the damping is not shed on it
        out.lam_next = float(t.lam)
        out.stats[11] = out.lam_next
    return out


@dataclass
class BoundedResult:
    x: np.ndarray
    cost: float                 # 0.5 sum r^2
    grad: np.ndarray
    active_mask: np.ndarray     # -1 at the lower bound, +1 at the upper, 0 otherwise (scipy's convention)
    status: int                 # the loop's stop code (lm_reference.CODES)
    n_truncated: int
    trials: list = field(default_factory=list)   # dicts: accepted, alpha, n_active, lam, c_old, c_new, code
    history: list = field(default_factory=list)


def final_mask(x, g, lo, hi):
    am = np.zeros(x.shape[0], dtype=np.int64)
    am[(x <= lo) & ((g > 0.0) | (lo == hi))] = -1
    am[(x >= hi) & (g < 0.0)] = 1
    return am


def solve(fun, jac, x0, lo, hi, *, max_iter=50, ftol=1e-8, xtol=1e-8, gtol=1e-8, lam0=1e-5, lam_grow0=1e3, rejection_limit=12):
    """The bounded loop on dense J = jac(x), r = fun(x) over the free vector."""
    x = np.array(x0, dtype=np.float64)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), x.shape).copy()
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), x.shape).copy()

    def state(x):
        J = jac(x)
        J = J.toarray() if hasattr(J, "toarray") else np.asarray(J)
        r = np.asarray(fun(x), dtype=np.float64)
        return J.T @ J, J.T @ r, float(r @ r)

    ctrl = LR.make_ctrl(max_iter=max_iter, ftol=ftol, xtol=xtol, gtol=gtol, rejection_limit=rejection_limit, lam_grow0=lam_grow0)
    H, g, c = state(x)
    lam = float(lam0)
    trials, history, n_truncated = [], [0.5 * c], 0
    code = 5 if max_iter <= 0 else 0
    pin = np.zeros(x.shape[0], bool)
    while code == 0 and len(trials) < rejection_limit * max_iter + 16:
        fixed_eff, n_active = active_set(x, g, lo, hi, pin=pin)
        mask = ~fixed_eff
        status = 0
        try:
            d = LR.reference_step(H, g, mask, lam)
        except np.linalg.LinAlgError:
            d, status = np.zeros_like(x), 2
        d = np.where(mask, d, 0.0)
        alpha, hit, x_new, delta = truncate(x, d, lo, hi)
        pin = pin | pinned(x, d, lo, hi)
        dvec = np.where(mask, np.maximum(np.diag(H), 1e-300), 0.0)
        gm = np.where(mask, g, 0.0)
        pred = predicted_reduction(lam, dvec, gm, delta, alpha)
        H_new, g_new, c_new = state(x_new)
        t = LR.TrialInputs(c_old=c, c_new=c_new, pred=pred, gmax=float(np.max(np.abs(gm))) if gm.size else 0.0, delta=delta, x_free=x[mask], lam=lam, status=status)
        out = decide(t, ctrl, alpha)
        ctrl, code = out.ctrl, out.code
        if out.branch in ("accept", "reject") and alpha < 1.0:
            n_truncated += 1
        trials.append(dict(accepted=out.accepted, n_pinned=int(np.count_nonzero(pinned(x, d, lo, hi))), alpha=alpha, hit=hit, n_active=n_active, lam=lam, c_old=c, c_new=c_new, code=code, branch=out.branch,
                           gmax=t.gmax, rho=out.rho, near=out.near_threshold))
        lam = out.lam_next
        if out.accepted:
            pin = np.zeros(x.shape[0], bool)
            x, H, g, c = x_new, H_new, g_new, c_new
            history.append(0.5 * c)
    return BoundedResult(x=x, cost=0.5 * c, grad=g, active_mask=final_mask(x, g, lo, hi), status=code, n_truncated=n_truncated, trials=trials, history=history)


# ------------------------------------------------------------------------------------------------ the test problems, chosen on the CPU
# Boxes on ring-4 that put the constrained minimum clearly ON the bounds, chosen before any GPU run (tests/test_bounds_reference.py pins
# them against scipy): the focal length fx of camera 2 at most 2 % below its true value, and the z translation of camera 1's extrinsics
# 2 % short of its true value.  Both are well determined by the data (the scaled gradient on either bound is some 1e-2 of the residual
# norm, thousands of times the convergence tolerance), so the active set is no coin toss.  The start sits 5 % inside either bound, so the
# first steps are cut.  Boxes on the distortion terms were tried and dropped: ring-4's views determine k2 and k3 so poorly that scipy's
# trf runs out of evaluations (status 0) with them, and which of them end up on a bound then depends on where each solver stops.
# The free-point chain knows no poses, so ring-4's table is relabelled for it: every (image, key) becomes a point of its own in image 0
# (216 points at their posed positions, 648 coordinates — the trailing group of 3), cameras 0 and 1 are fixed entirely (extrinsics AND
# intrinsics: they triangulate the points and set the scale, which free points and free cameras leave open), cameras 2 and 3 are free.
# Box: fx of camera 2 at most 2 % below truth (binds), the z translation of camera 2 2 % short of truth (set, does NOT bind: the free
# points take up what a pose could not — both solvers agree on that).  Tried and dropped: only camera 0's extrinsics fixed (scipy status
# 0 after 600 evaluations with nothing active, the reference on the fx bound at a lower cost: the gauge is open), and a second focal
# bound, fy of camera 3 (both solvers end with both bounds active, but scipy runs out of its 600 evaluations: status 0).
CHAINS = ("template", "self", "free")
TRIAL_ITERS, SOLVE_ITERS, SCIPY_NFEV = 12, 100, 600
FX_CAM, EXT_CAM = 2, 1


def interior(x0, lo, hi, rel=1e-3):
    """x0 moved strictly inside the box (scipy's trf wants a strictly feasible start): ``rel`` of the box width, or of max(1, |bound|)."""
    with np.errstate(invalid="ignore"):
        span = np.where(np.isfinite(hi - lo), hi - lo, np.maximum(1.0, np.abs(np.where(np.isfinite(lo), lo, hi))))
        x = np.where(np.isfinite(lo), np.maximum(x0, lo + rel * span), x0)
        return np.where(np.isfinite(hi), np.minimum(x, hi - rel * span), x)


@dataclass
class Problem:
    rig: object
    h: object
    x0: np.ndarray            # feasible; the bounded entries 5 % inside their bounds
    x0_interior: np.ndarray   # the same for scipy (strictly feasible; identical here)
    fun: object
    jac: object
    lo: np.ndarray
    hi: np.ndarray
    designed_mask: np.ndarray
    # the initial damping of the trial-by-trial comparison.  The free chain takes 1e-2: from its start the nearly undamped first step of
    # the default 1e-5 overshoots to a cost of 1.4e18 (and is rejected), and a cost at such a point amplifies the last bits of the step
    # by eleven orders of magnitude — nothing two correct solvers agree on to 1e-10
    lam0: float = 1e-5


def _box(n, rig, fx_at, tz_at, x0):
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    designed = np.zeros(n, dtype=np.int64)
    x0 = x0.copy()
    fx = float(rig.intr_true[FX_CAM, 0])
    hi[fx_at], designed[fx_at], x0[fx_at] = 0.98 * fx, 1, 0.93 * fx
    tz = float(rig.extr_true[EXT_CAM, 5])
    if tz > 0:
        hi[tz_at], designed[tz_at] = 0.98 * tz, 1
    else:
        lo[tz_at], designed[tz_at] = 0.98 * tz, -1
    x0[tz_at] = 0.93 * tz
    return lo, hi, designed, x0


def _free_problem() -> Problem:
    from pycamset_amd import handlers, synthetic
    from pycamset_amd.detections import TargetDetection
    from tests import weights_reference as W
    from tests.test_host_logic import DuckCamset, DuckTarget
    rig = W.ring4()
    K, C = rig.n_keys, rig.n_cams
    det = rig.detections.copy()
    det[:, 2] = det[:, 1] * K + det[:, 2]
    det[:, 1] = 0
    R = synthetic._rot(rig.poses_true[:, :3])
    pts_true = (np.einsum("iab,kb->ika", R, rig.points) + rig.poses_true[:, None, 3:]).reshape(-1, 3)
    pts0 = pts_true + 0.02 * np.random.default_rng(5).standard_normal(pts_true.shape)
    fixed = {f"cam_{c}": {"ext": rig.extr_true[c].copy(), "int": rig.intr_true[c].copy()} for c in (0, 1)}
    names = [f"cam_{i}" for i in range(C)]
    h = handlers.FreePointBundleHandler(DuckCamset(C), DuckTarget(pts0), TargetDetection(names, det), fixed_params=fixed, options={"verbosity": 0})
    bp = h.bundlePrimitive
    assert bp.intr_unfixed.tolist() == [False, False, True, True] and bp.extr_unfixed.tolist() == [False, False, True, True]
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), pts0.ravel()[bp.bdpt_unfixed]])
    fun, jac = W.oracle_closures(h, "free", None)
    n = x0.shape[0]
    fx_at, tz_at = 0, 18 + 5                       # free vector: 9 per free camera (2, 3), 6 per free camera, the points
    lo, hi, designed = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n, dtype=np.int64)
    fx, tz = float(rig.intr_true[2, 0]), float(rig.extr_true[2, 5])
    hi[fx_at], designed[fx_at], x0[fx_at] = 0.98 * fx, 1, 0.93 * fx
    if tz > 0:
        hi[tz_at] = 0.98 * tz
    else:
        lo[tz_at] = 0.98 * tz
    x0[tz_at] = 0.93 * tz
    return Problem(rig=rig, h=h, x0=x0, x0_interior=interior(x0, lo, hi), fun=fun, jac=jac, lo=lo, hi=hi, designed_mask=designed, lam0=1e-2)


def problem(chain) -> Problem:
    from tests import weights_reference as W
    if chain == "free":
        return _free_problem()
    rig, h, x0 = W.ring4_handler(chain)
    fun, jac = W.oracle_closures(h, chain, rig.points if chain == "template" else None)
    # free vector: 9 per camera (all free), then 6 per camera 1.. (camera 0's extrinsics are fixed)
    lo, hi, designed, x0 = _box(x0.shape[0], rig, 9 * FX_CAM, 9 * rig.n_cams + 6 * (EXT_CAM - 1) + 5, x0)
    return Problem(rig=rig, h=h, x0=x0, x0_interior=interior(x0, lo, hi), fun=fun, jac=jac, lo=lo, hi=hi, designed_mask=designed)


def genchain_box(rig, prob):
    """The same box for the four-block generated chain of tests/test_gpu_prior.py (free vector: the intrinsics, the extrinsics of
    cameras 1.., the poses): (lo, hi, designed active mask); the caller clips its start into the box."""
    lo, hi, designed, _ = _box(prob.x0.shape[0], rig, 9 * FX_CAM, 9 * rig.n_cams + 6 * (EXT_CAM - 1) + 5, prob.x0)
    return lo, hi, designed
