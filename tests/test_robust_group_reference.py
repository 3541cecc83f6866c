"""The robust group-LM restatement (tests/robust_group_reference.py) without a GPU: its loss arithmetic against scipy's, its minimisers
against scipy.optimize.least_squares(loss=, f_scale=) and against the noise-free truth, on the fixtures the device is tested with
(tests/test_gpu_robust_groups.py), and the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.optimize._lsq.common import scale_for_robust_loss_function
from scipy.optimize._lsq.least_squares import construct_loss_function

from oracle import ba_oracle as orc
from pycamset_amd import _capi, diagnostics, find_target, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from tests import pnp_reference as pnp
from tests import rigpose_reference as rigref
from tests import robust_group_reference as ref
from tests import tri_refine_reference as triref
from tests.test_pnp_reference import CUBE
from tests.test_rigpose_reference import ext_of, image_pose_error, perturbed_truth, viewing_distance

F_SCALE = 1.0
TIGHT = dict(max_iter=100, ftol=1e-14, xtol=1e-14)

# ---- the rig-pose fixture -------------------------------------------------------------------------------------------------------------
RIG_SIZES = {0: 5, 1: 6, 2: 17, 3: 40, 4: 70, 5: 40}   # detections kept per image; image 6 keeps all of them and starts from NaN
RIG_OUTLIERS = {2: 1, 3: 3, 4: 3, 5: 1}                # detections displaced by 25-60 px
NAN_START, N_RIG_IMAGES = 6, 7
_rig = {}


def rig_fixture():
    """4 cameras x 7 images of the cube, 0.3 px noise, pruned per image to ``RIG_SIZES`` (5: below min_points; 6: min_points; 17: one
    lane of a 16-lane group owns two; 70: lanes wrap at 64 lanes too), 1 or 3 detections per ``RIG_OUTLIERS`` image displaced by
    25-60 px in a random direction.  The start is what a user of a finished calibration has: the LINEAR fit of the contaminated
    detections (the linear restatement from 0.02 rad / 2 mm off the truth), which the outliers have pulled; image 6 starts from NaN.
    -> (rig, table, start, E, viewing distance, outlier mask of the table)."""
    if not _rig:
        rig = synthetic.make_rig("robust-rigpose", 4, N_RIG_IMAGES, CUBE, seed=41, noise_px=0.3)
        det = rig.detections.copy()
        rng = np.random.default_rng(8)
        keep = np.ones(det.shape[0], dtype=bool)
        bad = np.zeros(det.shape[0], dtype=bool)
        for im, n in RIG_SIZES.items():
            rows = rng.permutation(np.nonzero(det[:, 1] == im)[0])
            keep[rows[n:]] = False
            for q in rows[:RIG_OUTLIERS.get(im, 0)]:
                ang, size = rng.uniform(0, 2 * np.pi), rng.uniform(25.0, 60.0)
                det[q, 3:5] += size * np.array([np.cos(ang), np.sin(ang)])
                bad[q] = True
        det, bad = det[keep], bad[keep]
        E = ext_of(rig)
        off = perturbed_truth(rig, seed=4)
        lin = rigref.localise_target(det, rig.points, rig.intr_true, E, off)
        start = np.where(np.isfinite(lin.poses), lin.poses, off)   # image 0 (five detections) has no linear fit: it keeps a finite start
        start[NAN_START] = np.nan
        _rig.update(v=(rig, det, start, E, viewing_distance(rig), bad))
    return _rig["v"]


def image_rows(det, points, i):
    rows = rigref.group_images(det[det[:, 1] == i])[0]
    return points[rows[:, 2].astype(int)], rows[:, 3:5], rows[:, 0].astype(int)


# ---- the triangulation fixture --------------------------------------------------------------------------------------------------------
TRI_VIEWS = [1, 2, 4, 7, 24, 25, 30, 7]   # views per point: 24 = G V register views, 25 one more; the last point starts behind a camera
TRI_OUTLIERS = {2: 6.0, 3: 40.0, 5: 40.0, 6: 40.0}   # the 4-, 7-, 25- and 30-view points have one view displaced by this many pixels
TRI_F_SCALE = 3.0                         # ten times the pixel noise
BEHIND = 7
_tri = {}


def tri_fixture():
    """The 32-camera synthetic rig (two rings, 0.3 px noise); eight features that all cameras see, pruned to ``TRI_VIEWS`` views,
    one view of each ``TRI_OUTLIERS`` point displaced in a random direction.  The DLT start is the plain one: it spreads an outlier
    over all views of the point, and with four views (a quarter of the data wrong) the inliers start about half the displacement
    off.  huber, cauchy and arctan have no curvature beyond f_scale (s^2 is clamped to EPS there), so a start with EVERY residual
    beyond f_scale is not improved; the four-view point is therefore displaced by 2 f_scale, the others by 40 px.
    -> (rec rows [cam, im, key, u, v], start, P, K, D, truth (8, 3))."""
    if not _tri:
        rig = synthetic.make_rig("robust-tri", 32, 1, synthetic.ccube_points(5, 30.0), seed=63, visibility=1.0, n_rings=2, noise_px=0.3)
        im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
        d = rig.detections
        d = d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))]
        keys, counts = np.unique(d[:, 2].astype(int), return_counts=True)
        full = keys[counts >= 30][: len(TRI_VIEWS)]
        assert len(full) == len(TRI_VIEWS)
        rng = np.random.default_rng(2)
        rec, start = [], [0]
        for j, (k, n) in enumerate(zip(full, TRI_VIEWS)):
            rows = d[d[:, 2] == k]
            rows = rows[np.sort(rng.permutation(rows.shape[0])[:n])].copy()
            if j in TRI_OUTLIERS:
                ang = rng.uniform(0, 2 * np.pi)
                rows[rng.integers(n), 3:5] += TRI_OUTLIERS[j] * np.array([np.cos(ang), np.sin(ang)])
            rec.append(rows)
            start.append(start[-1] + n)
        _tri.update(v=(np.concatenate(rec), np.array(start, dtype=np.int64), P, K, D, im[0, full]))
    return _tri["v"]


def centres_of(P):
    return np.stack([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P])


def tri_starts(rec, start, P, K, D):
    """The starts the device would take: the DLT points, NaN below two views, and the ``BEHIND`` point mirrored behind its first camera."""
    dlt = orc.triangulate_full(rec, P, start, K, D)
    dlt[np.diff(start) < 2] = np.nan
    dlt[BEHIND] = 2 * centres_of(P)[int(rec[start[BEHIND], 0])] - dlt[BEHIND]
    return dlt


# ---- 1. the loss arithmetic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("f_scale", [1.0, 0.37, 12.5])
def test_robust_scale_is_scipys(kind, f_scale):
    """rho0, the row scale and the scaled residual against scipy's ``construct_loss_function`` and ``scale_for_robust_loss_function``
    for |f| / f_scale from 1e-8 to 1e4 (both signs) and f = 0.  rho0 and rho1 to 8 ulp: the two evaluate the same expressions in
    another order (scipy forms rho2 f^2 with rho2 divided by f_scale^2 first).  s^2 = rho1 + 2 z rho'' is a DIFFERENCE of two terms
    of size rho1, each rounded to a few ulp, so s^2 is compared ABSOLUTELY, to 8 ulp of rho1, over the whole range; the product
    s (rho1 f / s) = rho1 f to 8 ulp; and where nothing cancels (rho1 <= 2 s^2) s itself to 3 ulp and rho1 f / s to 8."""
    q = np.concatenate([[0.0], np.logspace(-8, 4, 97), -np.logspace(-8, 4, 97), [1.0, -1.0, 1.0 - 1e-12, 1.0 + 1e-12]])
    f = q * f_scale
    s, rf, r0 = ref.robust_scale(f, kind, f_scale)
    rho = construct_loss_function(f.shape[0], kind, f_scale)(f)
    J_sp, f_sp = scale_for_robust_loss_function(np.ones((f.shape[0], 1)), f.copy(), rho)   # scipy scales in place
    ulp = 8 * np.finfo(np.float64).eps
    assert np.all(np.abs(r0 - rho[0]) <= ulp * np.abs(rho[0]))
    assert np.all(np.abs(s * s - J_sp[:, 0] ** 2) <= ulp * rho[1]) and np.all(s > 0)
    assert np.all(np.abs(rf * s - f_sp * J_sp[:, 0]) <= ulp * np.abs(rho[1] * f))
    clear = rho[1] <= 2.0 * J_sp[:, 0] ** 2                          # nothing cancels
    assert clear.sum() > 100 and np.all(np.abs(s - J_sp[:, 0])[clear] <= 3 * np.finfo(np.float64).eps * J_sp[:, 0][clear])
    assert np.all(np.abs(rf - f_sp)[clear] <= ulp * np.abs(f_sp)[clear])
    assert s[0] == 1.0 and rf[0] == 0.0 and r0[0] == 0.0
    # what the user thresholds: rho1
    assert np.allclose(diagnostics.robust_weights(f, kind, f_scale), rho[1], rtol=ulp, atol=0)


def test_linear_kind_is_the_plain_restatement():
    rig, det, start, E, _, _ = rig_fixture()
    X, uv, cams = image_rows(det, rig.points, 3)
    a = ref.lm_image_pose(start[3], X, uv, cams, rig.intr_true, E)
    b = rigref.lm_image_pose(start[3], X, uv, cams, rig.intr_true, E)
    assert np.array_equal(a["pose"], b[0]) and (a["it"], a["status"], a["cost"], a["cost0"]) == b[1:5] and a["raw"] == a["cost"]
    assert np.all(diagnostics.robust_weights([[0.5, np.nan]], "linear")[0, :1] == 1.0) and np.isnan(diagnostics.robust_weights([np.nan], "cauchy")[0])


# ---- 2. convergence against scipy ------------------------------------------------------------------------------------------------------
def stationarity_radius(H, cost, scale, size):
    """The bound of tests/test_gpu_rigpose.py ``test_against_the_joint_solve_with_every_camera_fixed`` with the robust H and cost: a
    solver that stops on ftol is within sqrt(ftol S / lambda_min(H)) of the minimum (S = sum rho0, the cost it watches), one that stops
    on xtol has moved by less than xtol (xtol + size).  ``scale``: the diagonal that makes the coordinates comparable."""
    lam = np.linalg.eigvalsh(scale @ H @ scale)[0]
    return float(np.sqrt(TIGHT["ftol"] * cost / lam) + TIGHT["xtol"] * (TIGHT["xtol"] + size))


@pytest.mark.parametrize("kind", ref.KINDS)
def test_rig_pose_restatement_converges_to_scipys_minimum(kind):
    """Every image of the fixture that is estimated, run to ftol = xtol = 1e-14 (100 trials).  The gradient of scipy's robust cost at
    the result, as the Gauss-Newton step it asks for (robust H, update coordinates, translation relative to the viewing distance), is
    within the stationarity radius.  huber and soft_l1: the pose equals ``least_squares(method="trf")`` from the same start within the
    two solvers' radii.  cauchy and arctan are not convex: zero gradient, and a cost not above scipy's (1e-12 relative: rounding)."""
    rig, det, start, E, dist, _ = rig_fixture()
    Sc = np.diag([1.0, 1.0, 1.0, dist, dist, dist])
    for i in range(1, NAN_START):
        X, uv, cams = image_rows(det, rig.points, i)
        o = ref.lm_image_pose(start[i], X, uv, cams, rig.intr_true, E, kind, F_SCALE, **TIGHT)
        assert o["status"] in (ref.CONVERGED, ref.NO_DECREASE) and o["it"] < 100, (i, o["status"], o["it"])
        fun = lambda p: rigref.image_residuals(p, X, uv, cams, rig.intr_true, E).ravel()   # noqa: E731

        def jac(p):
            J = -rigref._rows(pnp.rodrigues(p[:3]), p[3:], X, uv, cams, rig.intr_true, E)[1]
            J[:, :3] = J[:, :3] @ pnp.left_jacobian(p[:3])
            return J

        f = fun(o["pose"])
        rho = construct_loss_function(f.shape[0], kind, F_SCALE)(f)
        assert abs(0.5 * np.sum(rho[0]) - 0.5 * o["cost"]) <= 1e-12 * o["cost"]
        J = rigref._rows(pnp.rodrigues(o["pose"][:3]), o["pose"][3:], X, uv, cams, rig.intr_true, E)[1]
        J_sp, _ = scale_for_robust_loss_function(J.copy(), f.copy(), rho)
        H_sp = J_sp.T @ J_sp
        step = np.linalg.solve(H_sp, J.T @ (rho[1] * f))            # the gradient of scipy's robust cost, as a step
        radius = stationarity_radius(H_sp, o["cost"], Sc, 4.0)
        size = float(np.linalg.norm(np.linalg.solve(Sc, step)))
        sp = least_squares(fun, start[i], jac=jac, method="trf", loss=kind, f_scale=F_SCALE, xtol=1e-14, ftol=1e-14, gtol=1e-14, max_nfev=400)
        ang, dt = image_pose_error(o["pose"], sp.x, dist)
        print(f"{kind} image {i}: trials {o['it']}, step {size:.2e}, radius {radius:.2e}; scipy: angle {ang:.2e}, translation {dt:.2e}, "
              f"cost {0.5 * o['cost']:.12g} / {sp.cost:.12g}")
        assert size <= radius, (i, size, radius)
        if kind in ("huber", "soft_l1"):
            assert max(ang, dt) <= 2 * radius, (i, ang, dt, radius)
        else:
            assert 0.5 * o["cost"] <= sp.cost * (1 + 1e-12), (i, o["cost"], sp.cost)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_refinement_restatement_converges_to_scipys_minimum(kind):
    """The same for every refined point of the triangulation fixture (coordinates in metres: no scaling)."""
    rec, start, P, K, D, _ = tri_fixture()
    dlt = tri_starts(rec, start, P, K, D)
    for j in range(len(TRI_VIEWS)):
        rows = rec[start[j]:start[j + 1]]
        cams, uv = rows[:, 0].astype(int), rows[:, -2:]
        o = ref.refine_point(dlt[j], cams, uv, P, K, D, kind, TRI_F_SCALE, **TIGHT)
        if TRI_VIEWS[j] < 2 or j == BEHIND:
            assert o["status"] == ref.NOT_ESTIMATED and o["it"] == 0 and np.array_equal(o["X"], dlt[j], equal_nan=True)
            continue
        assert o["status"] in (ref.CONVERGED, ref.NO_DECREASE) and o["it"] < 100, (j, o["status"], o["it"])
        fun = lambda X: triref.residuals(X, cams, uv, P, K, D)[0].ravel()   # noqa: E731
        jac = lambda X: -np.concatenate([triref.jacobian(X, P[c], K[c], D[c]) for c in cams])   # noqa: E731
        f = fun(o["X"])
        rho = construct_loss_function(f.shape[0], kind, TRI_F_SCALE)(f)
        J = -jac(o["X"])
        J_sp, _ = scale_for_robust_loss_function(J.copy(), f.copy(), rho)
        H_sp = J_sp.T @ J_sp
        step = np.linalg.solve(H_sp, J.T @ (rho[1] * f))
        radius = stationarity_radius(H_sp, o["cost"], np.eye(3), float(np.linalg.norm(o["X"])))
        sp = least_squares(fun, dlt[j], jac=jac, method="trf", loss=kind, f_scale=TRI_F_SCALE, xtol=1e-14, ftol=1e-14, gtol=1e-14, max_nfev=400)
        dist = float(np.linalg.norm(o["X"] - sp.x))
        print(f"{kind} point {j} ({TRI_VIEWS[j]} views): trials {o['it']}, step {np.linalg.norm(step):.2e}, radius {radius:.2e}; scipy: distance {dist:.2e}, "
              f"cost {0.5 * o['cost']:.12g} / {sp.cost:.12g}")
        assert np.linalg.norm(step) <= radius, (j, np.linalg.norm(step), radius)
        if kind in ("huber", "soft_l1"):
            assert dist <= 2 * radius, (j, dist, radius)
        else:
            assert 0.5 * o["cost"] <= sp.cost * (1 + 1e-12), (j, o["cost"], sp.cost)


# ---- how far the robust Hessian moves with the pose (the device's bound where its trial count differs) ----------------------------------
# The robust H depends on the pose through the weights s^2(f) as well as through J.  Measured here on the restatement, per loss: the
# largest change of an entry (scaled by sqrt(H_ii H_jj)) per unit of pose (radians; translation relative to the viewing distance) at
# the default-tolerance results of the fixture's images, 2.68 / 744 / 966 / 9.05e3 (arctan: its s^2 falls steepest between inlier and
# outlier), with a margin of about 2.  tests/test_gpu_robust_groups.py multiplies it by the flat radius.
H_SENSITIVITY = {"huber": 6.0, "soft_l1": 1.5e3, "cauchy": 2.0e3, "arctan": 2.0e4}


def hessian_sensitivity(kind, eps=1e-7):
    """max over the images of sqrt(sum_k S_k^2), S_k the largest scaled entry change per unit step along pose axis k (central pair):
    an upper bound of the directional derivative for any unit direction."""
    rig, det, start, E, dist, _ = rig_fixture()
    r = ref.localise_target(det, rig.points, rig.intr_true, E, start, kind, F_SCALE)
    worst = 0.0
    for i in range(1, NAN_START):
        X, uv, cams = image_rows(det, rig.points, i)

        def H_at(d):
            R, t = pnp.rodrigues(d[:3]) @ pnp.rodrigues(r.poses[i, :3]), r.poses[i, 3:] + dist * d[3:]
            return ref.rigpose_sums(R, t, X, uv, cams, rig.intr_true, E, kind, F_SCALE)[0]

        H0 = H_at(np.zeros(6))
        sc = np.sqrt(np.outer(np.diag(H0), np.diag(H0)))
        S = [max(np.max(np.abs(H_at(sign * eps * np.eye(6)[k]) - H0) / sc) for sign in (1.0, -1.0)) / eps for k in range(6)]
        worst = max(worst, float(np.sqrt(np.sum(np.square(S)))))
    return worst


@pytest.mark.parametrize("kind", ref.KINDS)
def test_hessian_sensitivity_is_within_the_figure_the_device_test_uses(kind):
    s = hessian_sensitivity(kind)
    print(f"{kind}: scaled Hessian change per unit of pose {s:.3g}, figure {H_SENSITIVITY[kind]:.3g}")
    assert H_SENSITIVITY[kind] / 4.0 <= s <= H_SENSITIVITY[kind]


# ---- 3. what the loss is for ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_robust_results_are_closer_to_the_truth_where_an_outlier_sits(kind):
    """At the default tolerances, on every image / point that holds an outlier: the robust result is closer to the noise-free truth
    than the linear one (a property of the fixtures' seeds, asserted for the restatement alone)."""
    rig, det, start, E, dist, _ = rig_fixture()
    lin = ref.localise_target(det, rig.points, rig.intr_true, E, start)
    rob = ref.localise_target(det, rig.points, rig.intr_true, E, start, kind, F_SCALE)
    for i in RIG_OUTLIERS:
        e_lin, e_rob = max(image_pose_error(lin.poses[i], rig.poses_true[i], dist)), max(image_pose_error(rob.poses[i], rig.poses_true[i], dist))
        print(f"{kind} image {i}: linear {e_lin:.2e}, robust {e_rob:.2e}, rms {lin.rms[i]:.3f} / {rob.rms[i]:.3f}, trials {rob.iterations[i]}")
        assert e_rob < e_lin and rob.cost[i] <= rob.cost_init[i] and rob.rms[i] >= lin.rms[i]
    rec, tstart, P, K, D, truth = tri_fixture()
    dlt = tri_starts(rec, tstart, P, K, D)
    for j in TRI_OUTLIERS:
        rows = rec[tstart[j]:tstart[j + 1]]
        cams, uv = rows[:, 0].astype(int), rows[:, -2:]
        a, b = ref.refine_point(dlt[j], cams, uv, P, K, D), ref.refine_point(dlt[j], cams, uv, P, K, D, kind, TRI_F_SCALE)
        e_lin, e_rob = np.linalg.norm(a["X"] - truth[j]), np.linalg.norm(b["X"] - truth[j])
        print(f"{kind} point {j} ({TRI_VIEWS[j]} views): linear {e_lin:.2e} m, robust {e_rob:.2e} m, trials {b['it']}")
        assert e_rob < e_lin


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def test_loss_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 113
    k, fs = ctypes.c_int(7), ctypes.c_double(7.0)
    for setter, getter, costs in ((lib.pcs_rigpose_set_loss, lib.pcs_rigpose_get_loss, lib.pcs_rigpose_costs),
                                  (lib.pcs_tri_set_refine_loss, lib.pcs_tri_get_refine_loss, lib.pcs_tri_refine_costs)):
        assert setter(None, _capi.LOSS_IDS["huber"], 1.0) == _capi.PCS_ERR_ARG and b"bad arguments" in lib.pcs_last_error()
        assert getter(None, ctypes.byref(k), ctypes.byref(fs)) == _capi.PCS_ERR_ARG and (k.value, fs.value) == (7, 7.0)
        assert costs(None, None) == _capi.PCS_ERR_ARG and b"bad arguments" in lib.pcs_last_error()


def test_python_front_ends_validate_the_loss_before_the_device():
    rig, det, start, E, _, _ = rig_fixture()
    rec, tstart, P, K, D, _ = tri_fixture()
    for kw in ({"loss": "l2"}, {"loss": None}, {"loss": 3}, {"f_scale": 0.0}, {"f_scale": -1.0}, {"f_scale": float("nan")}, {"f_scale": float("inf")},
               {"f_scale": "x"}):
        with pytest.raises(ValueError):
            hip_ch.localise_target(det, rig.points, rig.intr_true, E, poses_init=start, **kw)
        with pytest.raises(ValueError):
            find_target.find_target_poses(det, rig.points, rig.intr_true, E, **kw)
        with pytest.raises(ValueError):
            find_target.find_target_pose_at_timestep(det, rig.points, rig.intr_true, E, **kw)
        with pytest.raises(ValueError):
            hip_ch.refine_triangulation(rec, P, tstart, K, D, **kw)
        with pytest.raises(ValueError):
            hip_ch.multi_cam_triangulate(rec, P, K, D, refine=True, **kw)
        with pytest.raises(ValueError):
            diagnostics.robust_weights(np.zeros(3), **kw)
    e = hip_ch.localise_target(det[:0], rig.points, rig.intr_true, E, n_imgs=2, loss="cauchy", f_scale=2.0)
    assert (e.loss, e.f_scale) == ("cauchy", 2.0) and e.cost.shape == (2,) and np.all(np.isnan(e.cost)) and np.all(np.isnan(e.cost_init))


def test_covariance_under_a_loss_uses_the_robust_cost():
    """sigma^2 = 2 cost / (2 n - 6) on the returned H; ``absolute_sigma`` ignores it."""
    rng = np.random.default_rng(2)
    A = rng.normal(size=(1, 20, 6))
    H = np.einsum("ina,inb->iab", A, A)
    n = np.array([10], dtype=np.int32)
    res = hip_ch.ImagePoses(poses=np.zeros((1, 6)), poses_init=np.zeros((1, 6)), rms=np.array([5.0]), rms_init=np.ones(1), status=np.ones(1, dtype=np.int32),
                            iterations=np.ones(1, dtype=np.int32), n_points=n, n_cams=n, hessian=H, cost=np.array([3.5]), cost_init=np.array([4.0]),
                            loss="huber", f_scale=1.0)
    assert np.allclose(res.covariance()[0], 2 * 3.5 / 14 * np.linalg.inv(H[0]), rtol=1e-12)
    assert np.allclose(res.covariance(absolute_sigma=True)[0], np.linalg.inv(H[0]), rtol=1e-12)
