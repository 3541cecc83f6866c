"""The triangulation refinement without a GPU: the NumPy restatement (tests/tri_refine_reference.py) against finite differences and
scipy.optimize.least_squares, and the argument checks of the C entry points and of the Python front end."""
import ctypes

import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from tests import tri_refine_reference as ref


def small_rig(n_cams=5, seed=3, noise_px=0.5, dist_scale=20.0):
    """Cameras of a synthetic rig with their distortion scaled by ``dist_scale`` (strong distortion: the model is exercised well
    away from the pinhole) and measurements projected through that model plus Gaussian noise."""
    rig = synthetic.make_rig("tri-ref", n_cams, 2, synthetic.ccube_points(3, 30.0), seed=seed, noise_px=0.0, n_rings=2 if n_cams >= 4 else 1)
    im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
    return project_table(rig.detections, im, P, K, dist_scale * D, noise_px, seed) + (P, K, dist_scale * D)


def project_table(det, im, P, K, D, noise_px, seed):
    """(rec, start, truth): the rig's table grouped by feature, its measurements replaced by the model's projection of the true point
    plus noise, and the true point of every kept feature."""
    d = det[np.lexsort((det[:, 0], det[:, 2], det[:, 1]))].copy()
    rng = np.random.default_rng(seed)
    for i, row in enumerate(d):
        d[i, -2:] = ref.project(im[int(row[1]), int(row[2])], P[int(row[0])], K[int(row[0])], D[int(row[0])])[0]
    d[:, -2:] += rng.normal(0, noise_px, (d.shape[0], 2))
    rec, start = hip_ch.group_reconstructable(d)
    first = rec[start[:-1]]
    return rec, start, im[first[:, 1].astype(int), first[:, 2].astype(int)]


def test_jacobian_matches_central_differences():
    rec, start, truth, P, K, D = small_rig()
    rng = np.random.default_rng(0)
    for j in range(0, len(start) - 1, 3):
        X = truth[j] + rng.normal(0, 1e-3, 3)
        for c in rec[start[j]:start[j + 1], 0].astype(int):
            J = ref.jacobian(X, P[c], K[c], D[c])
            num = np.empty((2, 3))
            for k in range(3):
                h = 1e-6 * max(1.0, abs(X[k]))
                e = np.zeros(3)
                e[k] = h
                num[:, k] = (ref.project(X + e, P[c], K[c], D[c])[0] - ref.project(X - e, P[c], K[c], D[c])[0]) / (2 * h)
            assert np.allclose(J, num, rtol=1e-6, atol=1e-6 * np.abs(J).max()), (J, num)


def test_reference_minimiser_matches_scipy_and_is_stationary():
    from scipy.optimize import least_squares

    rec, start, truth, P, K, D = small_rig()
    dlt = orc.triangulate_full(rec, P, start, K, D)
    pts, its, st = ref.refine_all(dlt, rec, start, P, K, D)
    assert np.all(st == ref.CONVERGED) and its.max() <= 10
    centres = np.stack([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P])
    for j in range(len(start) - 1):
        rows = rec[start[j]:start[j + 1]]
        cams, uv = rows[:, 0].astype(int), rows[:, -2:]
        fun = lambda X: ref.residuals(X, cams, uv, P, K, D)[0].ravel()   # noqa: E731
        jac = lambda X: -np.concatenate([ref.jacobian(X, P[c], K[c], D[c]) for c in cams])   # noqa: E731
        sp = least_squares(fun, dlt[j], jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        c_ref, c_sp = np.sum(fun(pts[j]) ** 2), np.sum(fun(sp.x) ** 2)
        assert c_ref <= c_sp * (1 + 1e-12) + 1e-24
        # the position is compared on the scale of the viewing distance (the target sits near the origin, so |X| says little);
        # both minimisers stop where the cost is flat to rounding
        depth = np.mean(np.linalg.norm(centres[cams] - sp.x, axis=1))
        assert np.linalg.norm(pts[j] - sp.x) <= 1e-9 * depth
        # first-order optimality: J'r vanishes to rounding relative to |J| |r|
        H, g, cost, _ = ref._sums(pts[j], cams, uv, P, K, D)
        scale = np.sqrt(np.max(np.diag(H)) * max(cost, 1e-30))
        assert np.max(np.abs(g)) <= 1e-6 * scale
        # never worse than the DLT start
        assert ref.rms(pts[j], cams, uv, P, K, D) <= ref.rms(dlt[j], cams, uv, P, K, D)


def test_reference_status_codes():
    rec, start, truth, P, K, D = small_rig(noise_px=0.0)
    rows = rec[start[0]:start[1]]
    cams, uv = rows[:, 0].astype(int), rows[:, -2:]
    dlt = orc.triangulate_full(rows, P, np.array([0, len(rows)]), K, D)[0]
    X, it, st = ref.refine_point(dlt, cams, uv, P, K, D, max_iter=0)
    assert it == 0 and st == ref.MAX_ITER and np.array_equal(X, dlt)
    X, it, st = ref.refine_point(np.full(3, np.nan), cams, uv, P, K, D)
    assert st == ref.NOT_REFINED and it == 0
    # a start behind the cameras: mirror the point through the first camera's centre
    C = -np.linalg.solve(P[cams[0]][:, :3], P[cams[0]][:, 3])
    X, it, st = ref.refine_point(2 * C - dlt, cams, uv, P, K, D)
    assert st == ref.NOT_REFINED
    X, it, st = ref.refine_point(dlt, cams, uv, P, K, D)
    assert st == ref.CONVERGED and ref.rms(X, cams, uv, P, K, D) < 1e-9


def test_refine_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 104
    vp = ctypes.c_void_p
    ok = (10, 1e-10, 1e-10, 0.0, 0)
    assert lib.pcs_tri_refine(None, *ok, None, None, None, None, None) == _capi.PCS_ERR_ARG
    assert b"NULL handle" in lib.pcs_last_error()
    for bad in ((-1, 1e-10, 1e-10, 0.0, 0), (10, -1.0, 1e-10, 0.0, 0), (10, 1e-10, float("nan"), 0.0, 0), (10, 1e-10, 1e-10, float("inf"), 0),
                (10, 1e-10, 1e-10, 0.0, 2)):
        # options are checked before the handle: a bad option is reported as such even with a (dummy) handle
        assert lib.pcs_tri_refine(vp(1), *bad, None, None, None, None, None) == _capi.PCS_ERR_ARG
        assert b"bad options" in lib.pcs_last_error()
    assert lib.pcs_tri_refined(None, None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_tri_last_refine_ms(None, None) == _capi.PCS_ERR_ARG


def test_python_front_end_validates_options():
    rec, start, _, P, K, D = small_rig()
    for kw in ({"max_iter": -1}, {"max_iter": 2.5}, {"max_iter": True}, {"ftol": -1e-3}, {"xtol": float("nan")}, {"gtol": "x"}):
        with pytest.raises(ValueError):
            hip_ch.refine_triangulation(rec, P, start, K, D, **kw)
        with pytest.raises(ValueError):
            hip_ch.multi_cam_triangulate(rec, P, K, D, refine=True, **kw)
    with pytest.raises(ValueError):
        hip_ch.refine_triangulation(rec[:, :2], P, start, K, D)
    assert hip_ch.check_refine_options(3, 0, 1e-3, 0.5) == (3, 0.0, 1e-3, 0.5)
    assert hip_ch.REFINE_DEFAULTS["max_iter"] == 10
    assert (hip_ch.TRI_NOT_REFINED, hip_ch.TRI_CONVERGED, hip_ch.TRI_MAX_ITER, hip_ch.TRI_NO_DECREASE) == (
        _capi.TRI_NOT_REFINED, _capi.TRI_CONVERGED, _capi.TRI_MAX_ITER, _capi.TRI_NO_DECREASE)
