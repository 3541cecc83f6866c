"""The triangulation refinement on the GPU (include/pcs_hip.h pcs_tri_refine) against its NumPy restatement
(tests/tri_refine_reference.py, itself pinned to scipy.optimize.least_squares in tests/test_tri_refine.py).

Tolerances.  The device and the restatement run the same LM from the same DLT start (the device's own DLT points), so they take the
same trials; they differ by the rounding of the kernel's reciprocals (tri_rcp: 1-2 ulp) and of the summation order, which moves the
accepted points by a few ulp of the cost.  Where a point is well determined (>= 3 views) the minimum is a sharp bowl and the points
agree to 1e-9 of the viewing distance (the targets sit near the origin, so |X| is no scale; 1e-9 of 0.2 m is 0.2 nm, against a
position noise of ~50 um at 0.3 px).  A two-view point close to its baseline is determined only along the rays: the cost is flat to
rounding over a stretch far longer than that, and the two minimisers stop at different places of the same valley — there the costs
agree to 1e-10 relative, plus 1e-12 px * sqrt(cost) for points that fit to a thousandth of a pixel: evaluating the cost itself
rounds each residual (a difference of two pixel coordinates near 1e3) by ~1e-13 px, which moves sum r^2 by ~2 sum |r| 1e-13."""
import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from tests import tri_refine_reference as ref
from tests.test_tri_refine import project_table

pytestmark = pytest.mark.gpu


def rig_inputs(rig):
    im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
    d = rig.detections
    d = d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))]
    rec, start = hip_ch.group_reconstructable(d)
    return rec, start, P, K, D, im, d


def centres_of(P):
    return np.stack([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P])


def point_cost(X, rows, P, K, D):
    r, _ = ref.residuals(X, rows[:, 0].astype(int), rows[:, -2:], P, K, D)
    return float(np.sum(r * r))


def assert_matches_reference(res, rec, start, P, K, D, sel=None):
    sel = np.arange(len(start) - 1) if sel is None else sel
    C = centres_of(P)
    for j in sel:
        rows = rec[start[j]:start[j + 1]]
        cams, uv = rows[:, 0].astype(int), rows[:, -2:]
        X, _, _ = ref.refine_point(res.points_dlt[j], cams, uv, P, K, D)
        if len(cams) >= 3:
            depth = np.mean(np.linalg.norm(C[cams] - X, axis=1))
            assert np.linalg.norm(res.points[j] - X) <= 1e-9 * depth, (j, np.linalg.norm(res.points[j] - X) / depth)
        else:
            c_dev, c_ref = point_cost(res.points[j], rows, P, K, D), point_cost(X, rows, P, K, D)
            assert abs(c_dev - c_ref) <= 1e-10 * c_ref + 1e-12 * np.sqrt(c_ref), (j, c_dev, c_ref)


@pytest.mark.parametrize("n_cams,vis", [(2, 1.0), (5, 0.5), (5, 1.0), (32, 0.5), (32, 1.0)])
def test_refinement_matches_reference_and_is_never_worse(n_cams, vis):
    """Parity with the restatement; rms <= rms_dlt exactly; rms_dlt is the NumPy RMS at the DLT points to 1e-12 relative, plus
    1e-12 px for points that fit to a few hundredths of a pixel (a residual is the difference of two pixel coordinates near 1e3,
    each known to ~1e-13 px).  With 32 cameras a point has up to 32 views: more than the G V = 24 register views, so the global
    path runs."""
    rig = synthetic.make_rig("tri-refine", n_cams, 3, synthetic.ccube_points(5, 30.0), seed=90 + n_cams, visibility=vis,
                             n_rings=2 if n_cams >= 4 else 1)
    rec, start, P, K, D, _, _ = rig_inputs(rig)
    if n_cams == 32 and vis == 1.0:
        assert np.diff(start).min() > 24
    res = hip_ch.refine_triangulation(rec, P, start, K, D)
    n = len(start) - 1
    assert res.points.shape == (n, 3) and res.rms.shape == (n,) and res.residuals is None
    assert np.array_equal(res.points_dlt, hip_ch.nb_triangulate_full(rec, P, start, K, D))
    assert np.array_equal(res.n_views, np.diff(start))
    assert np.all(res.rms <= res.rms_dlt)
    assert np.all(np.isin(res.status, [hip_ch.TRI_CONVERGED, hip_ch.TRI_MAX_ITER, hip_ch.TRI_NO_DECREASE]))
    assert np.all((res.iterations >= 1) & (res.iterations <= hip_ch.REFINE_DEFAULTS["max_iter"]))
    for j in range(n):
        rows = rec[start[j]:start[j + 1]]
        r_np = ref.rms(res.points_dlt[j], rows[:, 0].astype(int), rows[:, -2:], P, K, D)
        assert abs(res.rms_dlt[j] - r_np) <= 1e-12 * r_np + 1e-12
    sel = np.arange(n) if n_cams < 32 else np.arange(0, n, 7)
    assert_matches_reference(res, rec, start, P, K, D, sel)


def test_refinement_accuracy_against_the_truth():
    """Noise-free measurements: the truth to 1e-9 of the viewing distance and below 1e-9 px.  Noisy measurements (0.5 px) with strong
    distortion (20 x the rig's coefficients, where the DLT's five fixed-point undistortion steps are far from exact): the refined
    points are closer to the truth (median) and fit better (mean RMS) than the DLT points."""
    rig = synthetic.make_rig("tri-acc", 8, 3, synthetic.ccube_points(5, 30.0), seed=5, noise_px=0.0, visibility=0.6, n_rings=2)
    im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
    C = centres_of(P)
    rec, start, truth = project_table(rig.detections, im, P, K, D, 0.0, 1)
    res = hip_ch.refine_triangulation(rec, P, start, K, D)
    depth = np.linalg.norm(truth - C.mean(axis=0), axis=1)
    assert np.all(np.linalg.norm(res.points - truth, axis=1) <= 1e-9 * depth)
    assert res.rms.max() < 1e-9
    rec, start, truth = project_table(rig.detections, im, P, K, 20.0 * D, 0.5, 2)
    res = hip_ch.refine_triangulation(rec, P, start, K, 20.0 * D)
    e_ref, e_dlt = np.linalg.norm(res.points - truth, axis=1), np.linalg.norm(res.points_dlt - truth, axis=1)
    assert np.median(e_ref) < np.median(e_dlt)
    assert res.rms.mean() < res.rms_dlt.mean() and np.all(res.rms <= res.rms_dlt)


def test_refinement_edge_cases():
    """No points; max_iter = 0 returns the DLT bits; a start behind a camera is not refined and keeps its bits; a non-finite
    measurement affects only its own point."""
    import torch
    rig = synthetic.make_rig("tri-edge", 6, 3, synthetic.ccube_points(4, 30.0), seed=11, visibility=0.8, n_rings=2)
    rec, start, P, K, D, _, _ = rig_inputs(rig)
    e = hip_ch.refine_triangulation(rec[:0], P, np.array([0]), K, D, return_residuals=True)
    assert e.points.shape == (0, 3) and e.rms.shape == (0,) and e.residuals.shape == (0, 2)
    base = hip_ch.refine_triangulation(rec, P, start, K, D)
    r0 = hip_ch.refine_triangulation(rec, P, start, K, D, max_iter=0)
    assert np.array_equal(r0.points, r0.points_dlt) and np.all(r0.iterations == 0) and np.all(r0.status == hip_ch.TRI_MAX_ITER)
    assert np.array_equal(r0.rms, r0.rms_dlt) and np.array_equal(r0.rms_dlt, base.rms_dlt)
    # a start behind the first camera of point k: the run writes to a caller buffer, which is edited before the refinement reads it
    n, k = len(start) - 1, 7
    tri = hip_ch.Triangulator(rig.n_cams)
    tri.set_cameras(P, K, D)
    tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
    d_pts = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tri.run(d_pts.data_ptr(), stream)
    torch.cuda.synchronize()
    pts = d_pts.cpu().numpy()
    c0 = int(rec[start[k], 0])
    behind = 2 * centres_of(P)[c0] - pts[k]
    pts[k] = behind
    d_pts.copy_(torch.from_numpy(pts))
    torch.cuda.synchronize()
    tri.refine(stream=stream)
    res = tri.refined(points_dlt=pts)
    assert res.status[k] == hip_ch.TRI_NOT_REFINED and res.iterations[k] == 0 and np.array_equal(res.points[k], behind)
    rows = rec[start[k]:start[k + 1]]
    assert abs(res.rms[k] - ref.rms(behind, rows[:, 0].astype(int), rows[:, -2:], P, K, D)) <= 1e-12 * res.rms[k]
    others = np.arange(n) != k
    assert np.array_equal(res.points[others], base.points[others]) and np.array_equal(res.rms[others], base.rms[others])
    tri.close()
    # a NaN measurement
    bad = rec.copy()
    bad[start[k] + 1, -1] = np.nan
    rb = hip_ch.refine_triangulation(bad, P, start, K, D)
    assert rb.status[k] == hip_ch.TRI_NOT_REFINED and np.array_equal(rb.points[k], rb.points_dlt[k], equal_nan=True)
    assert np.array_equal(rb.points[others], base.points[others]) and np.array_equal(rb.rms[others], base.rms[others])
    assert np.array_equal(rb.status[others], base.status[others]) and np.array_equal(rb.iterations[others], base.iterations[others])


def test_refinement_is_deterministic_and_permutation_equivariant():
    rig = synthetic.make_rig("tri-perm", 12, 6, synthetic.ccube_points(5, 30.0), seed=21, visibility=0.45, n_rings=2)
    rec, start, P, K, D, _, _ = rig_inputs(rig)
    a = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    b = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    for f in ("points", "points_dlt", "rms", "rms_dlt", "n_views", "iterations", "status", "residuals"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    perm = np.random.default_rng(1).permutation(len(start) - 1)
    rows = np.concatenate([np.arange(start[j], start[j + 1]) for j in perm])
    pstart = np.append(0, np.cumsum(np.diff(start)[perm]))
    p = hip_ch.refine_triangulation(rec[rows], P, pstart, K, D, return_residuals=True)
    for f in ("points", "points_dlt", "rms", "rms_dlt", "n_views", "iterations", "status"):
        assert np.array_equal(getattr(p, f), getattr(a, f)[perm]), f
    assert np.array_equal(p.residuals, a.residuals[rows])


def test_refinement_through_the_handle():
    """Device-resident inputs and outputs give the host path's bits; a refinement on a caller stream is ordered after the run on that
    stream; misuse fails with PCS_ERR_STATE."""
    import torch
    rig = synthetic.make_rig("tri-rh", 6, 5, synthetic.charuco_points(7, 6.0), seed=4, visibility=0.7, n_rings=2)
    rec, start, P, K, D, _, _ = rig_inputs(rig)
    host = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    n, n_obs = len(start) - 1, rec.shape[0]
    tri = hip_ch.Triangulator(rig.n_cams)
    with pytest.raises(_capi.PcsError) as ex:
        tri.refine()
    assert ex.value.code == _capi.PCS_ERR_STATE
    tri.set_cameras(P, K, D)
    cam = rec[:, 0].astype(np.int32)
    tri.set_observations(cam, rec[:, -2:], start)
    with pytest.raises(_capi.PcsError) as ex:
        tri.refine()                                   # observations set, no run yet
    assert ex.value.code == _capi.PCS_ERR_STATE
    tri.run()
    with pytest.raises(_capi.PcsError) as ex:
        tri.refined()                                  # a run, no refinement yet
    assert ex.value.code == _capi.PCS_ERR_STATE
    # device-resident in and out, on torch's stream
    d_cam, d_uv = torch.from_numpy(cam).cuda(), torch.from_numpy(np.ascontiguousarray(rec[:, -2:])).cuda()
    d_st = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int64)).cuda()
    d_pts, d_ref = (torch.zeros((n, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    d_rms = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    d_info = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    d_res = torch.zeros((n_obs, 2), dtype=torch.float64, device="cuda")
    tri.set_observations_device(n_obs, d_cam.data_ptr(), d_uv.data_ptr(), n, d_st.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        tri.run(d_pts.data_ptr(), stream)
        tri.refine(residuals=True, d_pts=d_ref.data_ptr(), d_rms=d_rms.data_ptr(), d_info=d_info.data_ptr(), d_resid=d_res.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_pts.cpu().numpy(), host.points_dlt) and np.array_equal(d_ref.cpu().numpy(), host.points)
    rms, info = d_rms.cpu().numpy(), d_info.cpu().numpy()
    assert np.array_equal(rms[:, 0], host.rms) and np.array_equal(rms[:, 1], host.rms_dlt)
    assert np.array_equal(info[:, 0], host.iterations) and np.array_equal(info[:, 1], host.status) and np.array_equal(info[:, 2], host.n_views)
    assert np.array_equal(d_res.cpu().numpy(), host.residuals)
    with pytest.raises(_capi.PcsError) as ex:
        tri.refined()                                  # the outputs went to caller buffers
    assert ex.value.code == _capi.PCS_ERR_STATE
    assert tri.last_refine_ms() > 0
    # handle-owned outputs, run and refinement on a side stream with no synchronisation by the caller
    tri.set_observations(cam, rec[:, -2:], start)
    side = torch.cuda.Stream()
    for _ in range(3):
        tri.run(None, side.cuda_stream)
        tri.refine(residuals=True, stream=side.cuda_stream)
        r = tri.refined()
        assert np.array_equal(r.points, host.points) and np.array_equal(r.points_dlt, host.points_dlt)
        assert np.array_equal(r.residuals, host.residuals)
    tri.close()


def test_multi_cam_triangulate_refines():
    """The front end: refine=True equals refine_triangulation on the host-grouped table (device grouping and host fallback);
    refine=False returns nb_triangulate_full's bits; the residuals are the NumPy model's at the returned points, in row order."""
    rig = synthetic.make_rig("tri-fe", 5, 6, synthetic.ccube_points(6, 30.0), seed=75, visibility=0.45, n_rings=2)
    rec, start, P, K, D, _, d = rig_inputs(rig)
    want = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    got = hip_ch.multi_cam_triangulate(d, P, K, D, refine=True, return_result=True, return_residuals=True)
    for f in ("points", "points_dlt", "rms", "rms_dlt", "n_views", "iterations", "status", "residuals"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert np.array_equal(hip_ch.multi_cam_triangulate(d, P, K, D, refine=True), want.points)
    assert np.array_equal(hip_ch.multi_cam_triangulate(d, P, K, D), hip_ch.nb_triangulate_full(rec, P, start, K, D))
    dlt_only = hip_ch.multi_cam_triangulate(d, P, K, D, return_result=True)
    assert np.array_equal(dlt_only.points, want.points_dlt) and np.array_equal(dlt_only.rms, want.rms_dlt)
    for j in range(len(start) - 1):
        rows = rec[start[j]:start[j + 1]]
        r, _ = ref.residuals(got.points[j], rows[:, 0].astype(int), rows[:, -2:], P, K, D)
        assert np.max(np.abs(got.residuals[start[j]:start[j + 1]] - r)) <= 1e-9
    # a table that is not grouped by feature: the host grouping, then the same refinement
    dd = rig.detections
    rec2, start2 = hip_ch.group_reconstructable(dd)
    a = hip_ch.multi_cam_triangulate(dd, P, K, D, refine=True, return_result=True)
    b = hip_ch.refine_triangulation(rec2, P, start2, K, D)
    assert np.array_equal(a.points, b.points) and np.array_equal(a.status, b.status)
    assert hip_ch.multi_cam_triangulate(d[:0], P, K, D, refine=True).shape == (0, 3)


def test_refinement_at_scale():
    rig = synthetic.make_rig("tri-big", 32, 40, synthetic.ccube_points(), seed=77, visibility=0.3215, n_rings=2)
    rec, start, P, K, D, _, _ = rig_inputs(rig)
    n = len(start) - 1
    assert n > 15000 and rec.shape[0] > 1.5e5
    res = hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True)
    for f in ("points", "rms", "rms_dlt", "residuals"):
        assert np.isfinite(getattr(res, f)).all(), f
    assert np.all(res.rms <= res.rms_dlt) and np.all(res.status != hip_ch.TRI_NOT_REFINED)
    assert_matches_reference(res, rec, start, P, K, D, np.arange(0, n, 41))
