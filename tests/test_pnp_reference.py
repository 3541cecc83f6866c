"""The batched target-pose estimation without a GPU: the NumPy restatement (tests/pnp_reference.py) against
scipy.optimize.least_squares and against the truth of noise-free rigs, the view-graph logic of
``pose_seeding.estimate_camera_relative_poses`` with the restatement and the oracle's legacy cost injected, the layout of
``calc_initial_params``, and the argument checks of the C entry points and of the Python front end."""
import ctypes

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, pose_seeding, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import pnp_reference as ref

CUBE = synthetic.ccube_points(5, 30.0)        # 6 faces x 16 points; keys 0..15 are one face
PLANE = synthetic.charuco_points(6)           # 5 x 5 corners
# the 8 corners of a cube with dyadic coordinates: centroid and scatter are exact in any summation order, the scatter is
# 2^-9 I, so its three eigenvalues are EQUAL (an isotropic target: no smallest, middle and largest to tell apart)
CORNERS = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) / 64.0
TARGETS = {"cube": CUBE, "face": CUBE, "planar": PLANE, "corners": CORNERS}


def true_view_poses(rig):
    """(C, I, 6): the composed true transform extr_true[c] o poses_true[i], target -> camera."""
    Re, Rp = Rotation.from_rotvec(rig.extr_true[:, :3]), Rotation.from_rotvec(rig.poses_true[:, :3])
    out = np.empty((rig.n_cams, rig.n_imgs, 6))
    for c in range(rig.n_cams):
        for i in range(rig.n_imgs):
            out[c, i, :3] = (Re[c] * Rp[i]).as_rotvec()
            out[c, i, 3:] = Re[c].apply(rig.poses_true[i, 3:]) + rig.extr_true[c, 3:]
    return out


def pose_error(a, b):
    """(rotation angle between two poses in radians, translation difference relative to the viewing distance |t_b|)."""
    ang = (Rotation.from_rotvec(a[:3]).inv() * Rotation.from_rotvec(b[:3])).magnitude()
    return float(ang), float(np.linalg.norm(a[3:] - b[3:]) / np.linalg.norm(b[3:]))


def truth_rig(kind, noise_px=0.0, seed=7, visibility=1.0):
    """(rig, table) of the kinds of view: a cube seen across faces, a planar board, cube views restricted to one face, and the
    exactly isotropic corners of a cube."""
    rig = synthetic.make_rig(f"pnp-{kind}", 3, 3, TARGETS[kind], seed=seed, noise_px=noise_px, visibility=visibility)
    det = rig.detections
    return rig, (det[det[:, 2] < 16] if kind == "face" else det)


def assert_recovers_truth(vp, rig):
    T = true_view_poses(rig)
    assert np.all(vp.n_points >= 6)
    for c in range(rig.n_cams):
        for i in range(rig.n_imgs):
            ang, dt = pose_error(vp.poses[c, i], T[c, i])
            assert vp.status[c, i] == ref.CONVERGED, (c, i, vp.status[c, i])
            assert ang <= 1e-8 and dt <= 1e-8, (c, i, ang, dt)
            assert vp.rms[c, i] < 1e-8, (c, i, vp.rms[c, i])
            assert np.linalg.norm(vp.poses[c, i, :3]) <= np.pi


def test_corner_target_is_exactly_isotropic():
    lam, _ = ref.jacobi_eigh3(CORNERS.T @ CORNERS)
    assert CORNERS.sum(axis=0).tolist() == [0.0, 0.0, 0.0] and lam.tolist() == [2.0 ** -9] * 3


@pytest.mark.parametrize("kind", ["cube", "planar", "face", "corners"])
def test_noise_free_views_recover_the_truth(kind):
    """``corners``: three equal eigenvalues of the scatter are a perfectly conditioned 3-D view, not a refused one."""
    rig, det = truth_rig(kind)
    vp = ref.estimate_view_poses(det, rig.points, rig.intr_true, 3, 3)
    assert_recovers_truth(vp, rig)
    planar = kind in ("planar", "face")
    assert np.all(np.isfinite(vp.poses_alt).all(axis=-1) == planar)   # the second start exists exactly for planar views


def flat_radius(H, cost, dist, eps=1e-12):
    """How far two minimisers that both stop where the cost is flat to rounding can be apart.  A residual is the difference of two
    pixel coordinates near 1e3, each known to ~1e-13 px, so sum r^2 of a 0.3 px fit is known to eps ~ 1e-12 relative; within
    d' H d / 2 <= eps * cost of the minimum no trial can be told from it.  The radius of that region along its weakest direction
    is sqrt(2 eps cost / lambda_min(H)), with the translation columns of H scaled by the viewing distance (radians against
    relative translation).  The tilt of a planar target is the weakest direction of these small rigs (a 30 mm target at
    0.2 m): there the radius is 1e-8 to 3e-7."""
    S = np.diag([1.0, 1.0, 1.0, dist, dist, dist])
    return float(np.sqrt(2.0 * eps * cost / np.linalg.eigvalsh(S @ H @ S)[0]))


@pytest.mark.parametrize("kind", ["cube", "planar", "face", "corners"])
def test_restatement_matches_scipy_from_its_own_start(kind):
    """scipy's MINPACK LM with xtol = ftol = gtol = 1e-15 runs until the cost is flat to rounding.  Run to the same tolerances
    (ftol = xtol = 1e-15, up to 50 trials) the restatement is compared as tests/test_tri_refine.py compares the triangulation:
    its cost is not above scipy's by more than 1e-12 relative, J'r vanishes to 1e-6 of |J| |r|, and the poses agree to 1e-9
    (radians; translation relative to the viewing distance).  That fixed figure holds for every 3-D view.  For planar and
    single-face views it is the radius over which the cost is flat to rounding where that is larger (``flat_radius``: the tilt
    of a small planar target is weakly determined).

    At the DEFAULT ftol = 1e-10 the restatement stops as soon as a trial lowers the cost by less than ftol * cost; the steps of
    a converging Gauss-Newton iteration shrink, so what is left above the minimum is below that last decrease:
    cost <= scipy's cost * (1 + ftol).  (Measured, not asserted: the default stop leaves the rotation about 2e-7 rad from the
    minimiser.  A cost 1e-10 above the minimum is all that ftol promises.)"""
    from scipy.optimize import least_squares

    rig, det = truth_rig(kind, noise_px=0.3, seed=11)
    ds, ids, start = ref.group_views(det, 3)
    for k, v in enumerate(ids):
        rows = ds[start[k]:start[k + 1]]
        cam9 = rig.intr_true[int(v) // 3]
        keys, uv = rows[:, 2].astype(int), rows[:, 3:5]
        X = rig.points[keys]
        r = ref.solve_view(keys, uv, cam9, rig.points)
        assert r["status"] == ref.CONVERGED and 1 <= r["iterations"] <= 10
        assert r["rms"] <= r["rms_init"]
        fun = lambda p: ref.residuals(p, X, uv, cam9).ravel()   # noqa: E731

        def jac(p):   # analytic, in the rotation vector: the restatement's left-increment Jacobian times J_l(r)
            J = -ref.jacobian(ref.rodrigues(p[:3]), p[3:], X, cam9)
            J[:, :3] = J[:, :3] @ ref.left_jacobian(p[:3])
            return J

        best = None
        for s0 in (r["pose_init"], r["pose_alt"]):   # the restatement keeps the better of its two starts: so does the comparison
            if np.all(np.isfinite(s0)):
                sp = least_squares(fun, s0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
                if best is None or sp.cost < best.cost:
                    best = sp
        c_ref, c_sp = np.sum(fun(r["pose"]) ** 2), 2.0 * best.cost
        assert c_ref <= c_sp * (1 + 1e-10) + 1e-24, (k, c_ref, c_sp)
        t = ref.solve_view(keys, uv, cam9, rig.points, max_iter=50, ftol=1e-15, xtol=1e-15)
        c_tight = np.sum(fun(t["pose"]) ** 2)
        assert c_tight <= c_sp * (1 + 1e-12) + 1e-24, (k, c_tight, c_sp)
        ang, dt = pose_error(t["pose"], best.x)
        H, g, cost, bad = ref._sums(ref.rodrigues(t["pose"][:3]), t["pose"][3:], X, uv, cam9)
        tol = 1e-9 if kind in ("cube", "corners") else max(1e-9, flat_radius(H, cost, np.linalg.norm(best.x[3:])))
        print(f"view {k}: angle {ang:.2e} rad, translation {dt:.2e}, bound {tol:.2e}")
        assert ang <= tol and dt <= tol, (k, ang, dt, tol)
        assert bad == 0 and np.max(np.abs(g) / np.sqrt(np.diag(H))) <= 1e-6 * np.sqrt(max(cost, 1e-30))


def test_reference_status_codes_and_rotation_helpers():
    rig, det = truth_rig("cube", noise_px=0.3)
    rows = det[(det[:, 0] == 1) & (det[:, 1] == 2)]
    keys, uv, cam9 = rows[:, 2].astype(int), rows[:, 3:5], rig.intr_true[1]
    r0 = ref.solve_view(keys, uv, cam9, rig.points, max_iter=0)
    assert r0["status"] == ref.MAX_ITER and r0["iterations"] == 0 and np.array_equal(r0["pose"], r0["pose_init"]) and r0["rms"] == r0["rms_init"]
    assert ref.solve_view(keys[:5], uv[:5], cam9, rig.points)["status"] == ref.NOT_ESTIMATED
    behind = r0["pose_init"].copy()
    behind[5] = -behind[5]
    rb = ref.solve_view(keys, uv, cam9, rig.points, start=behind)
    assert rb["status"] == ref.NOT_ESTIMATED and np.all(np.isnan(rb["pose"]))
    bad = uv.copy()
    bad[3, 0] = np.nan
    assert ref.solve_view(keys, bad, cam9, rig.points)["status"] == ref.NOT_ESTIMATED
    # rotation vector <-> matrix, angles near 0 and near pi included
    rng = np.random.default_rng(0)
    for ang in (0.0, 1e-12, 1e-5, 0.3, 2.0, np.pi - 1e-9, np.pi):
        ax = rng.normal(size=3)
        rv = ang * ax / np.linalg.norm(ax)
        R = ref.rodrigues(rv)
        assert np.allclose(R, Rotation.from_rotvec(rv).as_matrix(), atol=1e-15)
        back = ref.rotvec_of(R)
        assert np.all(np.isfinite(back)) and np.linalg.norm(back) <= np.pi + 1e-15
        assert np.allclose(ref.rodrigues(back), R, atol=1e-14)
    S = rng.normal(size=(3, 3))
    S = S @ S.T
    lam, V = ref.jacobi_eigh3(S)
    assert np.allclose(V @ np.diag(lam) @ V.T, S, atol=1e-14) and np.allclose(np.sort(lam), np.linalg.eigvalsh(S), atol=1e-14)


# ---- the view graph ---------------------------------------------------------------------------------------------------------------
def seed(rig, det, **kw):
    return pose_seeding.estimate_camera_relative_poses(det, rig.points, rig.intr_true, rig.n_cams, rig.n_imgs, view_pose_fn=ref.estimate_view_poses,
                                                       cost_fn=orc.legacy_cost, **kw)


def assert_poses_close(a, b, tol=1e-8):
    for x, y in zip(a, b):
        ang = (Rotation.from_rotvec(x[:3]).inv() * Rotation.from_rotvec(y[:3])).magnitude()
        assert ang <= tol and np.linalg.norm(x[3:] - y[3:]) <= tol * 0.2, (x, y)


def in_frame_of(rig, ref_pose):
    """(extr, poses) of the truth with the world moved to the target of ``ref_pose``."""
    T = pose_seeding.pose_to_4x4(rig.poses_true)
    E = pose_seeding.pose_to_4x4(rig.extr_true)
    return pose_seeding.pose_from_4x4(E @ T[ref_pose]), pose_seeding.pose_from_4x4(np.linalg.inv(T[ref_pose]) @ T)


def test_view_graph_returns_the_truth_on_a_noise_free_rig():
    rig, det = truth_rig("cube")
    extr, poses, err, missing = seed(rig, det)
    assert extr.shape == (3, 6) and poses.shape == (3, 6) and err.shape == (3,) and missing.shape == (3,)
    assert_poses_close(extr, rig.extr_true)
    assert_poses_close(poses, rig.poses_true)
    assert np.array_equal(poses[0], np.zeros(6)) and not missing.any() and err.max() < 1e-6
    extr2, poses2, _, _ = seed(rig, det, ref_pose=2)
    e_t, p_t = in_frame_of(rig, 2)
    assert_poses_close(extr2, e_t)
    assert_poses_close(poses2, p_t)


def test_unseen_reference_pose_is_replaced_and_missing_views_are_forward_filled():
    rig, det = truth_rig("cube")
    cut = det[~((det[:, 0] == 1) & (det[:, 1] == 1))]          # camera 1 does not see image 1
    extr, poses, err, missing = seed(rig, cut, ref_pose=1)     # -> image 0, the first one every camera sees
    assert_poses_close(extr, rig.extr_true)
    assert_poses_close(poses, rig.poses_true)                  # image 1 takes another camera's estimate, not camera 1's filled-in one
    assert not missing.any() and err.max() < 1e-6
    cut = det[~((det[:, 0] == 2) & (det[:, 1] == 2))]
    extr, poses, err, _ = seed(rig, cut)
    assert_poses_close(poses, rig.poses_true)
    assert err.max() < 1e-6
    gone = det[det[:, 1] != 1]                                  # nobody sees image 1: filled from image 0, reported missing
    _, poses, _, missing = seed(rig, gone)
    assert list(missing) == [False, True, False]
    assert_poses_close(poses[1:2], np.zeros((1, 6)))


def test_no_fully_shared_pose_raises():
    rig, det = truth_rig("cube")
    cut = det[det[:, 0] != det[:, 1]]                           # camera c misses image c: no image is seen by all
    with pytest.raises(ValueError):
        seed(rig, cut)


# ---- calc_initial_params ---------------------------------------------------------------------------------------------------------------
class DuckCamset:
    def __init__(self, n):
        self._names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self._names)

    def get_n_cams(self):
        return len(self._names)


class DuckTarget:
    def __init__(self, points):
        self.point_data = np.array(points, dtype=np.float64)[None]


def test_calc_initial_params_layout(monkeypatch):
    monkeypatch.setattr(hip_ch, "estimate_view_poses", ref.estimate_view_poses)
    monkeypatch.setattr(hip_ch, "bundle_adjustment_costfn", orc.legacy_cost)
    rig, det = truth_rig("cube")
    td = TargetDetection([f"cam_{i}" for i in range(3)], det)
    h = handlers.TemplateBundleHandler(DuckCamset(3), DuckTarget(rig.points), td)
    with pytest.raises(ValueError):
        h.calc_initial_params()                                 # the duck camset holds no intrinsics
    x = h.calc_initial_params(rig.intr_true)
    bp = h.bundlePrimitive
    assert x.shape == (9 * 3 + 6 * 3 + 6 * 2,) == (bp.pose_end,)
    assert np.array_equal(x[:27].reshape(3, 9), rig.intr_true)
    assert_poses_close(x[27:45].reshape(3, 6), rig.extr_true)
    assert_poses_close(x[45:].reshape(2, 6), rig.poses_true[1:])   # pose 0 is fixed
    assert list(h.missing_poses) == [False, False, False]
    with pytest.raises(NotImplementedError, match="calc_initial_params"):
        h.get_initial_params()                                  # nothing is stored
    h.set_initial_params(x)
    assert h.get_initial_params() is x
    x_template = x
    intr, extr, poses = h.get_bundle_adjustment_inputs(x)
    assert np.array_equal(intr, rig.intr_true) and np.array_equal(poses[0], np.zeros(6))
    # fixed cameras are left out, and a camera's fixed intrinsics are the ones the poses are estimated with
    fixed = {"cam_0": {"ext": rig.extr_true[0].copy()}, "cam_1": {"int": rig.intr_true[1].copy()}}
    h = handlers.TemplateBundleHandler(DuckCamset(3), DuckTarget(rig.points), td, fixed_params=fixed)
    wrong = rig.intr_true.copy()
    wrong[1, 0] *= 1.2
    x = h.calc_initial_params(wrong)
    assert x.shape == (9 * 2 + 6 * 2 + 6 * 2,)
    assert np.array_equal(x[:18].reshape(2, 9), rig.intr_true[[0, 2]])
    assert_poses_close(x[18:30].reshape(2, 6), rig.extr_true[1:])
    # the self chain appends its free point scalars
    hs = handlers.SelfBundleHandler(DuckCamset(3), DuckTarget(rig.points), td)
    xs = hs.calc_initial_params(rig.intr_true)
    assert xs.shape == (hs.bundlePrimitive.bdpt_end,) and np.array_equal(xs[:57], x_template)
    assert np.array_equal(xs[57:], hs.flat_point_data[hs.bundlePrimitive.bdpt_unfixed])


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_pnp_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 105
    vp = ctypes.c_void_p
    h = vp()
    assert lib.pcs_pnp_create(None, 0, 3, 8) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_create(ctypes.byref(h), 0, 0, 8) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_create(ctypes.byref(h), 0, 3, 0) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_destroy(None) == _capi.PCS_OK
    assert lib.pcs_pnp_set_cameras(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_set_template(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_set_observations(None, 0, None, None, 0, None, None) == _capi.PCS_ERR_ARG
    ok = (10, 1e-10, 1e-10, 0.0, 6, 0)
    none7 = (None,) * 7
    assert lib.pcs_pnp_run(None, *ok, *none7) == _capi.PCS_ERR_ARG
    assert b"NULL handle" in lib.pcs_last_error()
    for bad in ((-1, 1e-10, 1e-10, 0.0, 6, 0), (10, -1.0, 1e-10, 0.0, 6, 0), (10, 1e-10, float("nan"), 0.0, 6, 0), (10, 1e-10, 1e-10, float("inf"), 6, 0),
                (10, 1e-10, 1e-10, 0.0, 0, 0), (10, 1e-10, 1e-10, 0.0, 6, 2)):
        assert lib.pcs_pnp_run(vp(1), *bad, *none7) == _capi.PCS_ERR_ARG   # options are checked before the handle is touched
        assert b"bad options" in lib.pcs_last_error()
    assert lib.pcs_pnp_results(None, None, None, None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_last_kernel_ms(None, None) == _capi.PCS_ERR_ARG


def test_python_front_end_validates_before_the_device():
    rig, det = truth_rig("cube")
    for kw in ({"max_iter": -1}, {"max_iter": 2.5}, {"ftol": -1e-3}, {"xtol": float("nan")}, {"gtol": "x"}, {"min_points": 0}, {"min_points": 1.5}):
        with pytest.raises(ValueError):
            hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, **kw)
    with pytest.raises(ValueError):
        hip_ch.estimate_view_poses(det[:, :4], rig.points, rig.intr_true)
    with pytest.raises(ValueError):
        hip_ch.estimate_view_poses(det, rig.points, rig.intr_true[:2])   # camera 2 has no intrinsics
    e = hip_ch.estimate_view_poses(det[:0], rig.points, rig.intr_true, n_imgs=2, return_residuals=True)   # an empty table needs no device
    assert e.poses.shape == (3, 2, 6) and np.all(np.isnan(e.poses)) and np.all(e.status == 0) and e.residuals.shape == (0, 2)
    assert (hip_ch.PNP_NOT_ESTIMATED, hip_ch.PNP_CONVERGED, hip_ch.PNP_MAX_ITER, hip_ch.PNP_NO_DECREASE) == (
        _capi.PNP_NOT_ESTIMATED, _capi.PNP_CONVERGED, _capi.PNP_MAX_ITER, _capi.PNP_NO_DECREASE) == (
        ref.NOT_ESTIMATED, ref.CONVERGED, ref.MAX_ITER, ref.NO_DECREASE)
    order, ids, start = hip_ch.group_by_view(det, 3)
    assert order is None and len(ids) == 9 and start[-1] == det.shape[0]
    perm = np.random.default_rng(0).permutation(det.shape[0])
    order, ids2, start2 = hip_ch.group_by_view(det[perm], 3)
    assert np.array_equal(ids, ids2) and np.array_equal(start, start2) and np.array_equal(det[perm][order], det)   # keys too: the same order reaches the device
