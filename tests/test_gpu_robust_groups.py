"""Robust losses in the two group-LM kernels on the GPU (include/pcs_hip.h pcs_rigpose_set_loss, pcs_tri_set_refine_loss;
csrc/ba_rigpose.hpp, csrc/ba_tri_refine.hpp) against their NumPy restatement (tests/robust_group_reference.py, itself pinned to scipy's
loss arithmetic, to ``least_squares(loss=, f_scale=)`` and to the noise-free truth in tests/test_robust_group_reference.py, on the
fixtures used here).

Tolerances are those of tests/test_gpu_rigpose.py and tests/test_gpu_tri_refine.py for the same quantities.  Device and restatement run
the same LM from the same start; where they take the same number of trials they differ by rounding only and agree to 1e-9.  Where a
late trial changes the cost by less than its rounding the order of a sum decides whether it is accepted, the trial counts differ, and
the rig poses agree to the radius over which the (robust) cost is flat to rounding (``flat_radius`` with the robust H and sum rho0),
the rule of tests/test_gpu_rigpose.py; the refined points keep the unconditional 1e-9 of the depth of tests/test_gpu_tri_refine.py."""
import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as hip_ch
from tests import rigpose_reference as rigref
from tests import robust_group_reference as ref
from tests import tri_refine_reference as triref
from tests.test_pnp_reference import flat_radius
from tests.test_robust_group_reference import (BEHIND, F_SCALE, H_SENSITIVITY, NAN_START, N_RIG_IMAGES, RIG_OUTLIERS, RIG_SIZES, TRI_F_SCALE, TRI_OUTLIERS, TRI_VIEWS,
                                               centres_of, rig_fixture, tri_fixture)
from tests.test_rigpose_reference import image_pose_error

pytestmark = pytest.mark.gpu

WIDTHS = (16, 64)
_refs = {}


def rig_reference(kind):
    """The restatement's result on the rig fixture, once per loss."""
    if kind not in _refs:
        rig, det, start, E, _, _ = rig_fixture()
        _refs[kind] = ref.localise_target(det, rig.points, rig.intr_true, E, start, kind, F_SCALE)
    return _refs[kind]


def localise(kind, lanes, det=None, **kw):
    rig, table, start, E, _, _ = rig_fixture()
    return hip_ch.localise_target(table if det is None else det, rig.points, rig.intr_true, E, poses_init=start, group_lanes=lanes, return_residuals=True,
                                  loss=kind, f_scale=F_SCALE, **kw)


FIELDS = ("poses", "rms", "rms_init", "cost", "cost_init", "hessian", "status", "iterations", "n_points", "n_cams")


def same_bits(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=getattr(a, n).dtype.kind == "f") for n in FIELDS)


def scaled(H):
    d = np.sqrt(np.diag(H).astype(np.float64))
    return np.outer(d, d)


# ---- rig pose ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", WIDTHS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_rig_pose_parity_with_the_restatement(kind, lanes):
    """Counts and NaN pattern equal.  Per estimated image, with the same number of trials: status equal, pose to 1e-9 (radians;
    translation relative to the viewing distance), rms and cost to 1e-9 relative.  With another number of trials: the pose to the flat
    radius (1e-9 at least); the cost is flat there by construction (1e-12 relative, asserted at 1e-9), and the plain RMS moves by at
    most |d| j for a pose difference d, j = sqrt(lambda_max(J'J) / n) pixels per unit of pose.  The Hessian entries (scaled by
    sqrt(H_ii H_jj)): 1e-9 with the same number of trials; otherwise the flat radius times ``H_SENSITIVITY``, the restatement's own
    change of the robust H per unit of pose, measured on the CPU (tests/test_robust_group_reference.py), 1e-9 at least.  rms_init and
    cost_init do not depend on the trials: 1e-12.  Residuals: the restatement's projection at the device's pose, 1e-9 px."""
    rig, det, start, E, dist, _ = rig_fixture()
    res, r = localise(kind, lanes), rig_reference(kind)
    assert (res.loss, res.f_scale) == (kind, F_SCALE) and res.poses.shape == (N_RIG_IMAGES, 6)
    assert [int(res.n_points[im]) for im in RIG_SIZES] == list(RIG_SIZES.values())
    assert np.array_equal(res.n_points, r.n_points) and np.array_equal(res.n_cams, r.n_cams)
    assert np.array_equal(res.status != 0, r.status != 0), (res.status, r.status)
    assert np.array_equal(res.poses_init, start, equal_nan=True)
    Sc = np.diag([1.0, 1.0, 1.0, dist, dist, dist])
    for i in range(N_RIG_IMAGES):
        sel = det[:, 1] == i
        if i in (0, NAN_START):   # five detections: below min_points; a NaN start
            assert r.status[i] == 0 and res.status[i] == hip_ch.RIGPOSE_NOT_ESTIMATED and res.iterations[i] == 0
            assert np.all(np.isnan(res.poses[i])) and np.all(np.isnan(res.hessian[i])) and np.all(np.isnan(res.residuals[sel]))
            assert np.isnan(res.rms[i]) and np.isnan(res.rms_init[i]) and np.isnan(res.cost[i]) and np.isnan(res.cost_init[i])
            continue
        same = res.iterations[i] == r.iterations[i]
        tol = 1e-9 if same else max(1e-9, flat_radius(r.hessian[i], 2.0 * r.cost[i], dist))
        ang, dt = image_pose_error(res.poses[i], r.poses[i], dist)
        rows = rigref.group_images(det[sel])[0]
        X, uv, cams = rig.points[rows[:, 2].astype(int)], rows[:, 3:5], rows[:, 0].astype(int)
        J = rigref._rows(ref.rodrigues(r.poses[i, :3]), r.poses[i, 3:], X, uv, cams, rig.intr_true, E)[1]
        j_px = float(np.sqrt(np.linalg.eigvalsh(Sc @ (J.T @ J) @ Sc)[-1] / rows.shape[0]))
        rms_tol = 1e-9 * r.rms[i] if same else max(1e-9 * r.rms[i], tol * j_px)
        h_tol = 1e-9 if same else max(1e-9, H_SENSITIVITY[kind] * tol)
        e_h = float(np.max(np.abs(res.hessian[i] - r.hessian[i]) / scaled(r.hessian[i])))
        print(f"{kind} {lanes} lanes image {i} n = {res.n_points[i]}: angle {ang:.2e}, translation {dt:.2e}, bound {tol:.1e}; trials {res.iterations[i]} / "
              f"{r.iterations[i]}, status {res.status[i]} / {r.status[i]}; rms {abs(res.rms[i] - r.rms[i]):.2e} (bound {rms_tol:.1e}), "
              f"cost {abs(res.cost[i] - r.cost[i]) / r.cost[i]:.2e}, hessian {e_h:.2e} (bound {h_tol:.1e})")
        assert ang <= tol and dt <= tol, (i, ang, dt, tol)
        assert abs(res.rms[i] - r.rms[i]) <= rms_tol and abs(res.cost[i] - r.cost[i]) <= 1e-9 * r.cost[i]
        assert abs(res.rms_init[i] - r.rms_init[i]) <= 1e-12 * r.rms_init[i] + 1e-12 and abs(res.cost_init[i] - r.cost_init[i]) <= 1e-12 * r.cost_init[i]
        assert res.cost[i] <= res.cost_init[i] and np.array_equal(res.hessian[i], res.hessian[i].T)
        assert e_h <= h_tol, (i, e_h, h_tol)
        if same:
            assert res.status[i] == r.status[i]
        r_np = rigref.image_residuals(res.poses[i], rig.points[det[sel, 2].astype(int)], det[sel, 3:5], det[sel, 0].astype(int), rig.intr_true, E)
        assert np.allclose(res.residuals[sel], r_np, rtol=0, atol=1e-9)
        assert abs(res.rms[i] - np.sqrt(np.sum(r_np * r_np) / rows.shape[0])) <= 1e-12 * res.rms[i] + 1e-12   # the PLAIN pixel RMS
    for i in RIG_OUTLIERS:   # what the loss is for, on the device as well
        e_lin = max(image_pose_error(start[i], rig.poses_true[i], dist))
        assert max(image_pose_error(res.poses[i], rig.poses_true[i], dist)) < e_lin


@pytest.mark.parametrize("lanes", WIDTHS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_rig_pose_robust_hessian_in_extended_precision(kind, lanes):
    """With max_iter = 0 the returned pose is the start and ``hessian`` the robust sum s^2 J'J there (the outliers' rows clamped to
    EPS).  The yardstick of tests/test_gpu_rigpose.py: the restatement in np.longdouble; the device's distance from it (entries scaled
    by sqrt(H_ii H_jj), the largest over the images) may be 4 times the float64 restatement's own."""
    rig, det, start, E, _, _ = rig_fixture()
    z = localise(kind, lanes, max_iter=0)
    d_dev = d_np = 0.0
    for i in range(1, NAN_START):
        rows = rigref.group_images(det[det[:, 1] == i])[0]
        args = (start[i], rig.points[rows[:, 2].astype(int)], rows[:, 3:5], rows[:, 0].astype(int), rig.intr_true, E, kind, F_SCALE)
        H_ld, H_np = ref.robust_hessian_at(*args, dtype=np.longdouble), ref.robust_hessian_at(*args)
        s = scaled(H_ld)
        e_dev, e_np = float(np.max(np.abs(z.hessian[i] - H_ld) / s)), float(np.max(np.abs(H_np - H_ld) / s))
        print(f"{kind} image {i}: device {e_dev:.2e}, float64 restatement {e_np:.2e}")
        d_dev, d_np = max(d_dev, e_dev), max(d_np, e_np)
        assert z.status[i] == hip_ch.RIGPOSE_MAX_ITER and np.array_equal(z.poses[i], start[i]) and z.cost[i] == z.cost_init[i] and z.rms[i] == z.rms_init[i]
    print(f"{kind} {lanes} lanes: device {d_dev:.3e}, restatement {d_np:.3e}, ratio {d_dev / d_np:.2f}")
    assert d_np > 0 and d_dev <= 4.0 * d_np, (d_dev, d_np)


@pytest.mark.parametrize("lanes", WIDTHS)
def test_rig_pose_order_repeat_and_the_linear_keyword(lanes):
    """Two runs and the shuffled table give the same bits under every loss; ``loss="linear"`` gives the bits of a call without the
    keyword (and of the restatement's cost: half the sum of squares); under a loss ``covariance()`` uses the robust H and cost."""
    rig, det, start, E, _, _ = rig_fixture()
    perm = np.random.default_rng(3).permutation(det.shape[0])
    for kind in ref.KINDS:
        base = localise(kind, lanes)
        again, shuffled = localise(kind, lanes), localise(kind, lanes, det=det[perm])
        assert same_bits(again, base) and np.array_equal(again.residuals, base.residuals, equal_nan=True)
        assert same_bits(shuffled, base) and np.array_equal(shuffled.residuals, base.residuals[perm], equal_nan=True)
    plain = hip_ch.localise_target(det, rig.points, rig.intr_true, E, poses_init=start, group_lanes=lanes, return_residuals=True)
    lin = localise("linear", lanes)
    assert same_bits(lin, plain) and np.array_equal(lin.residuals, plain.residuals, equal_nan=True) and plain.loss == "linear"
    est = plain.status != 0
    assert np.allclose(plain.cost[est], 0.5 * plain.rms[est] ** 2 * plain.n_points[est], rtol=1e-14, atol=0) and np.all(np.isnan(plain.cost[~est]))
    assert not same_bits(base, plain)
    cov = base.covariance()
    for i in range(1, NAN_START):
        want = 2.0 * base.cost[i] / (2 * base.n_points[i] - 6) * np.linalg.inv(base.hessian[i])
        assert np.allclose(cov[i], want, rtol=1e-12, atol=0)
    assert np.all(np.isnan(cov[[0, NAN_START]]))


def test_rig_localiser_loss_belongs_to_the_handle_and_error_paths():
    """A bad kind or f_scale is refused (PCS_ERR_ARG) and leaves the previous loss in force; the costs of a handle that has not run are
    PCS_ERR_STATE; the loss survives new observations."""
    rig, det, start, E, _, _ = rig_fixture()
    lib = _capi.lib()
    loc = hip_ch.RigLocaliser(4, rig.points.shape[0])
    assert loc.get_loss() == ("linear", 1.0)
    loc.set_loss("cauchy", 2.5)
    for kind, fs in ((-1, 1.0), (5, 1.0), (1, 0.0), (1, -2.0), (1, float("nan")), (1, float("inf"))):
        assert lib.pcs_rigpose_set_loss(loc._h, kind, fs) == _capi.PCS_ERR_ARG
        assert loc.get_loss() == ("cauchy", 2.5)
    with pytest.raises(ValueError):
        loc.set_loss("tukey")
    with pytest.raises(_capi.PcsError) as e:
        loc.costs()
    assert e.value.code == _capi.PCS_ERR_STATE
    order, ids, first = hip_ch.group_by_image(det)
    ds = det[order]
    loc.set_loss("huber", F_SCALE)
    loc.set_cameras(rig.intr_true)
    loc.set_extrinsics(E)
    loc.set_template(rig.points)
    loc.set_observations(ds[:, 2].astype(np.int32), ds[:, 0].astype(np.int32), ds[:, 3:5], first)
    with pytest.raises(_capi.PcsError) as e:
        loc.costs()                                  # observations set, no run yet
    assert e.value.code == _capi.PCS_ERR_STATE
    loc.set_start(start[ids])
    assert loc.get_loss() == ("huber", F_SCALE)      # new cameras and observations keep it
    loc.run(group_lanes=16)
    want = localise("huber", 16)
    pose, rms, info, hess, _ = loc.results()
    assert np.array_equal(pose, want.poses[ids], equal_nan=True) and np.array_equal(loc.costs()[:, 0], want.cost[ids], equal_nan=True)
    loc.close()


# ---- triangulation refinement --------------------------------------------------------------------------------------------------------------
def refine_on_handle(kind):
    """The fixture through the handle: the DLT run writes to a caller buffer, where the ``BEHIND`` point is mirrored behind its first
    camera before the refinement reads it.  -> (TriangulationResult, costs (n, 2), the starts the refinement read)."""
    import torch

    rec, start, P, K, D, _ = tri_fixture()
    n = len(start) - 1
    tri = hip_ch.Triangulator(32)
    tri.set_cameras(P, K, D)
    tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
    d_pts = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tri.run(d_pts.data_ptr(), stream)
    torch.cuda.synchronize()
    pts = d_pts.cpu().numpy()
    pts[BEHIND] = 2 * centres_of(P)[int(rec[start[BEHIND], 0])] - pts[BEHIND]
    d_pts.copy_(torch.from_numpy(pts))
    torch.cuda.synchronize()
    tri.set_refine_loss(kind, TRI_F_SCALE)
    tri.refine(residuals=True, stream=stream)
    res = tri.refined(points_dlt=pts)
    costs = tri.refine_costs()
    tri.close()
    return res, costs, pts


@pytest.mark.parametrize("kind", ref.KINDS)
def test_refinement_parity_with_the_restatement(kind):
    """The restatement from the device's own starts.  The one-view point (NaN start) and the point that starts behind a camera:
    NOT_REFINED, no trial, the start's bits.  Otherwise the bounds of tests/test_gpu_tri_refine.py, whatever the trial counts: the
    point to 1e-9 of the viewing distance (two views: the robust costs to 1e-10 relative plus 1e-12 sqrt(cost), the valley of that
    file); the status equal where the trial counts are.  rms_dlt: 1e-12 (the start is common); cost: 1e-9 relative.  rms against the
    restatement's: 1e-9 relative plus what the point bound allows to first order, twice |grad rms| times 1e-9 of the depth, with
    grad rms = J'r / (n rms) of the PLAIN residuals taken from the restatement at its own result (the robust minimum is no minimum of
    the plain RMS, so that gradient does not vanish).  Residuals: the restatement's at the device's point, 1e-9 px."""
    rec, start, P, K, D, _ = tri_fixture()
    res, costs, pts = refine_on_handle(kind)
    C = centres_of(P)
    assert np.array_equal(res.n_views, TRI_VIEWS) and np.all(np.isnan(pts[0])) and np.array_equal(res.cost, costs[:, 0], equal_nan=True)
    for j in range(len(TRI_VIEWS)):
        rows = rec[start[j]:start[j + 1]]
        cams, uv = rows[:, 0].astype(int), rows[:, -2:]
        o = ref.refine_point(pts[j], cams, uv, P, K, D, kind, TRI_F_SCALE)
        r_np, _ = triref.residuals(res.points[j], cams, uv, P, K, D)
        if TRI_VIEWS[j] < 2 or j == BEHIND:
            assert o["status"] == 0 and res.status[j] == hip_ch.TRI_NOT_REFINED and res.iterations[j] == 0
            assert np.array_equal(res.points[j], pts[j], equal_nan=True)
            if j == BEHIND:
                assert abs(costs[j, 0] - 0.5 * o["cost"]) <= 1e-12 * o["cost"] and costs[j, 0] == costs[j, 1]
                assert np.allclose(res.residuals[start[j]:start[j + 1]], r_np, rtol=0, atol=1e-9 * np.abs(r_np).max())
            else:
                assert np.isnan(res.rms[j]) and np.isnan(costs[j, 0])
            continue
        same = res.iterations[j] == o["it"]
        depth = float(np.mean(np.linalg.norm(C[cams] - o["X"], axis=1)))
        dist = float(np.linalg.norm(res.points[j] - o["X"]))
        tol = 1e-9 * depth
        raw = float(np.sum(r_np * r_np))
        r_ref, _ = triref.residuals(o["X"], cams, uv, P, K, D)
        J_ref = np.concatenate([triref.jacobian(o["X"], P[c], K[c], D[c]) for c in cams])
        rms_ref = float(np.sqrt(o["raw"] / len(cams)))
        rms_tol = 1e-9 * rms_ref + 2.0 * float(np.linalg.norm(J_ref.T @ r_ref.reshape(-1))) / (len(cams) * rms_ref) * tol
        print(f"{kind} point {j} ({TRI_VIEWS[j]} views): distance {dist:.2e}, bound {tol:.1e}; trials {res.iterations[j]} / {o['it']}, status {res.status[j]} / "
              f"{o['status']}; cost {abs(costs[j, 0] - 0.5 * o['cost']) / (0.5 * o['cost']):.2e}, rms {abs(res.rms[j] - rms_ref):.2e} (bound {rms_tol:.1e})")
        if same:
            assert res.status[j] == o["status"]
        if len(cams) >= 3:
            assert dist <= tol, (j, dist, tol)
            assert abs(res.rms[j] - rms_ref) <= rms_tol, (j, res.rms[j], rms_ref, rms_tol)
        else:
            c_dev = ref.tri_sums(res.points[j], cams, uv, P, K, D, kind, TRI_F_SCALE)[2]
            assert abs(c_dev - o["cost"]) <= 1e-10 * o["cost"] + 1e-12 * np.sqrt(o["cost"]), (j, c_dev, o["cost"])
        assert abs(costs[j, 0] - 0.5 * o["cost"]) <= 1e-9 * 0.5 * o["cost"] and costs[j, 0] <= costs[j, 1]
        assert abs(costs[j, 1] - 0.5 * o["cost0"]) <= 1e-12 * o["cost0"]
        assert abs(res.rms_dlt[j] - np.sqrt(o["raw0"] / len(cams))) <= 1e-12 * res.rms_dlt[j] + 1e-12
        assert abs(res.rms[j] - np.sqrt(raw / len(cams))) <= 1e-12 * res.rms[j] + 1e-12                 # the PLAIN pixel RMS at the device's point
        assert np.max(np.abs(res.residuals[start[j]:start[j + 1]] - r_np)) <= 1e-9


def test_refinement_order_repeat_linear_keyword_and_error_paths():
    """Through the front ends: a second run and the points in another order give the same bits under every loss; ``loss="linear"``
    gives the bits of a call without the keyword; ``multi_cam_triangulate`` passes the loss on.  The handle refuses a bad kind or
    f_scale and keeps its loss; costs before a refinement are PCS_ERR_STATE."""
    rec, start, P, K, D, truth = tri_fixture()
    n = len(start) - 1
    perm = np.random.default_rng(1).permutation(n)
    rows = np.concatenate([np.arange(start[j], start[j + 1]) for j in perm])
    pstart = np.append(0, np.cumsum(np.diff(start)[perm]))
    names = ("points", "points_dlt", "rms", "rms_dlt", "cost", "n_views", "iterations", "status")
    plain = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    for kind in ref.KINDS + ("linear",):
        a = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True, loss=kind, f_scale=TRI_F_SCALE)
        b = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True, loss=kind, f_scale=TRI_F_SCALE)
        p = hip_ch.refine_triangulation(rec[rows], P, pstart, K, D, return_residuals=True, loss=kind, f_scale=TRI_F_SCALE)
        for f in names:
            assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (kind, f)
            assert np.array_equal(getattr(p, f), getattr(a, f)[perm], equal_nan=True), (kind, f)
            assert kind != "linear" or np.array_equal(getattr(a, f), getattr(plain, f), equal_nan=True), f
        assert np.array_equal(a.residuals, b.residuals, equal_nan=True) and np.array_equal(p.residuals, a.residuals[rows], equal_nan=True)
        if kind != "linear":
            assert not np.array_equal(a.points, plain.points, equal_nan=True)
            for j in TRI_OUTLIERS:   # what the loss is for, on the device as well
                assert np.linalg.norm(a.points[j] - truth[j]) < np.linalg.norm(plain.points[j] - truth[j]), (kind, j)
    ok = np.diff(start) >= 2
    assert np.allclose(plain.cost[ok], 0.5 * plain.rms[ok] ** 2 * plain.n_views[ok], rtol=1e-14, atol=0)
    table = rec[np.diff(start).repeat(np.diff(start)) >= 2]   # the front end keeps features seen by at least two cameras
    m = hip_ch.multi_cam_triangulate(table, P, K, D, refine=True, return_result=True, loss="cauchy", f_scale=TRI_F_SCALE)
    want = hip_ch.refine_triangulation(rec[start[1]:], P, start[1:] - start[1], K, D, loss="cauchy", f_scale=TRI_F_SCALE)
    assert np.array_equal(m.points, want.points) and np.array_equal(m.cost, want.cost)
    lib = _capi.lib()
    tri = hip_ch.Triangulator(32)
    assert tri.get_refine_loss() == ("linear", 1.0)
    tri.set_refine_loss("arctan", 0.5)
    for kind, fs in ((-1, 1.0), (5, 1.0), (2, 0.0), (2, float("nan")), (2, float("inf"))):
        assert lib.pcs_tri_set_refine_loss(tri._h, kind, fs) == _capi.PCS_ERR_ARG
        assert tri.get_refine_loss() == ("arctan", 0.5)
    tri.set_cameras(P, K, D)
    tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
    tri.run()
    with pytest.raises(_capi.PcsError) as e:
        tri.refine_costs()                           # a run, no refinement yet
    assert e.value.code == _capi.PCS_ERR_STATE and tri.get_refine_loss() == ("arctan", 0.5)
    tri.close()
