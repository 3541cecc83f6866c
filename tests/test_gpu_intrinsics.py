"""The intrinsics estimation from planar views on the GPU (include/pcs_hip.h pcs_intr_run, csrc/ba_intrinsics.hpp) against its NumPy
restatement (tests/intrinsics_reference.py, itself pinned to noise-free truth in tests/test_intrinsics_reference.py).

Tolerances.  For every input the restatement runs in float64 and in extended precision; the difference is the rounding sensitivity of
that input (a smallest eigenvector magnifies rounding by the inverse of the eigenvalue gap, and how much depends on the views).  The
kernel sums across 16 lanes in another order, contracts to FMAs and uses refined reciprocals, so it gets 10 x that difference, with
a floor of 1e-12 relative.  Homographies are compared as maps pixels <- template coordinates (``plane_maps``: the in-plane axes of a
square grid are any orthogonal pair, and rounding picks them).  Measured deviations: profiles/r12/README.md."""
import numpy as np
import pytest

from pycamset_amd import handlers, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import intrinsics_reference as ref
from tests.test_intrinsics_reference import PLANE, RES, TRUTH_RTOL, ResCamset, rel_err, rig_of
from tests.test_pnp_reference import DuckCamset

pytestmark = pytest.mark.gpu

G = 16   # lanes per group and per camera (csrc/pcs_intrinsics.inc INTR_G)


def bound(a64, ext, scale):
    """10 x |float64 - extended| of the restatement, floor 1e-12, relative to ``scale``."""
    return np.maximum(10.0 * np.abs(np.asarray(a64, dtype=np.float64) - np.asarray(ext, dtype=np.float64)), 1e-12 * scale)


def assert_matches_restatement(est, det, points, label, **kw):
    r = ref.estimate_intrinsics(det, points, **kw)
    x = ref.estimate_intrinsics(det, points, **kw, dtype=np.longdouble)
    assert np.array_equal(est.group_index, r.group_index) and np.array_equal(est.group_status, r.group_status)
    assert np.array_equal(est.group_counts, r.group_counts) and np.array_equal(est.status, r.status) and np.array_equal(est.n_groups, r.n_groups)
    used = r.group_status == ref.GROUP_USED
    P_dev, P_ref, P_ext = (ref.plane_maps(o.homographies[used], o.plane_frames[used]) for o in (est, r, x))
    scale = np.abs(P_ref).max(axis=(1, 2), keepdims=True)
    dP, bP = np.abs(P_dev - P_ref), bound(P_ref, P_ext, scale)
    ok = r.status != ref.NOT_ESTIMATED
    dK, bK = np.abs(est.intr[ok, :4] - r.intr[ok, :4]), bound(r.intr[ok, :4], x.intr[ok, :4], np.abs(r.intr[ok, :4]))
    print(f"{label}: plane maps off by {np.max(dP / scale):.2e} of their size (bound {np.max(bP / scale):.2e}), worst ratio to the bound {np.max(dP / bP):.2f}; "
          f"intrinsics off by {np.max(dK / np.abs(r.intr[ok, :4])):.2e} relative (bound {np.max(bK / np.abs(r.intr[ok, :4])):.2e}), worst ratio {np.max(dK / bK):.2f}")
    assert np.all(dP <= bP) and np.all(dK <= bK)
    assert np.all(est.intr[ok, 4:] == 0.0) and np.all(np.isnan(est.intr[~ok])) and np.all(np.isnan(est.homographies[~used]))


@pytest.mark.parametrize("kind", ["plane", "cube"])
@pytest.mark.parametrize("noise_px", [0.0, 0.3])
@pytest.mark.parametrize("model", ["full", "focal"])
def test_parity_with_the_restatement(kind, noise_px, model):
    rig, intr, _, det, bok = rig_of(kind, noise_px=noise_px, tilt=3.5 if noise_px else 1.0, n_imgs=12 if noise_px else 6)
    kw = dict(n_cams=3, n_imgs=12 if noise_px else 6, board_of_key=bok, model=model, res=RES if model == "focal" else None)
    est = hip_ch.estimate_intrinsics(det, rig.points, **kw)
    assert est.intr.shape == (3, 9) and est.lm is None and est.intr_init is None
    assert np.all(est.status == (hip_ch.INTR_FULL if model == "full" else hip_ch.INTR_FOCAL))
    assert_matches_restatement(est, det, rig.points, f"{kind} noise {noise_px} {model}", **kw)


@pytest.mark.parametrize("kind", ["plane", "cube"])
def test_noise_free_truth_from_the_device(kind):
    rig, intr, _, det, bok = rig_of(kind)
    est = hip_ch.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full")
    print(f"{kind}: relative error of the device's full model {rel_err(est.intr, intr):.2e}, eigenvalue ratio {np.abs(est.eig_ratio).max():.1e}")
    assert np.all(est.status == hip_ch.INTR_FULL) and rel_err(est.intr, intr) <= TRUTH_RTOL and np.abs(est.eig_ratio).max() < 1e-12
    auto = hip_ch.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok)              # no res: auto is the full model
    assert np.array_equal(auto.intr, est.intr) and np.array_equal(auto.status, est.status)
    auto = hip_ch.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, res=RES)     # res: auto is the focal model
    assert np.all(auto.status == hip_ch.INTR_FOCAL) and np.all(auto.intr[:, [1, 3]] == 499.5)


def shapes_table():
    """One camera, 17 images of a 9 x 9 board (81 keys), 0.3 px noise, tilts scaled by 3.5; images 0..4 cut to 12, 13, 16, 17 and 65 rows."""
    rig = synthetic.make_rig("intr-shapes", 1, 17, synthetic.charuco_points(10), seed=33, noise_px=0.0)
    poses = rig.poses_true.copy()
    poses[:, :3] *= 3.5
    intr = rig.intr_true.copy()
    intr[:, 4:] = 0.0
    uv, _ = synthetic.project_dense(intr, rig.extr_true, poses, rig.points)
    det = rig.detections.copy()
    det[:, 3:] = uv[0, det[:, 1].astype(int), det[:, 2].astype(int)] + np.random.default_rng(5).normal(0, 0.3, (det.shape[0], 2))
    sizes = {0: 12, 1: 13, 2: G, 3: G + 1, 4: 4 * G + 1}
    keep = np.ones(det.shape[0], dtype=bool)
    rng = np.random.default_rng(6)
    for im, n in sizes.items():
        rows = np.nonzero(det[:, 1] == im)[0]
        keep[rng.permutation(rows)[n:]] = False
    return rig, det[keep], sizes


def same_bits(a, b, fields=("intr", "status", "n_groups", "eig_ratio", "homographies", "plane_frames", "group_status", "group_counts", "group_index")):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=getattr(a, f).dtype.kind == "f") for f in fields)


def test_shapes_at_which_the_kernels_can_go_wrong():
    """Groups of 12 (refused), 13, G, G + 1 and 4 G + 1 observations; 17 groups: one whole block of 16 groups and a block with one
    live group; a NaN measurement; a non-planar group; a shuffled table; two runs."""
    rig, det, sizes = shapes_table()
    kw = dict(n_cams=1, n_imgs=17, model="full")
    base = hip_ch.estimate_intrinsics(det, rig.points, **kw)
    assert base.group_counts[:5].tolist() == list(sizes.values()) and len(base.group_status) == 17
    assert base.group_status.tolist() == [hip_ch.INTR_GROUP_TOO_FEW] + [hip_ch.INTR_GROUP_USED] * 16
    assert np.all(np.isnan(base.homographies[0])) and np.all(np.isfinite(base.homographies[1:])) and base.n_groups[0] == 16 and base.status[0] == hip_ch.INTR_FULL
    assert_matches_restatement(base, det, rig.points, "shapes", **kw)
    again = hip_ch.estimate_intrinsics(det, rig.points, **kw)
    assert same_bits(again, base)                                                        # two runs
    perm = np.random.default_rng(7).permutation(det.shape[0])
    assert same_bits(hip_ch.estimate_intrinsics(det[perm], rig.points, **kw), base)       # a shuffled table
    # a NaN measurement drops only its own group: the camera's result is that of a run without the group, bit for bit
    bad = det.copy()
    bad[np.nonzero(det[:, 1] == 7)[0][2], 4] = np.nan
    b = hip_ch.estimate_intrinsics(bad, rig.points, **kw)
    without = hip_ch.estimate_intrinsics(det[det[:, 1] != 7], rig.points, **kw)
    assert b.group_status[7] == hip_ch.INTR_GROUP_NOT_FINITE and np.all(np.isnan(b.homographies[7])) and b.n_groups[0] == 15
    assert np.array_equal(b.intr, without.intr) and np.array_equal(b.eig_ratio, without.eig_ratio) and np.array_equal(b.status, without.status)
    others = np.arange(17) != 7
    assert np.array_equal(b.homographies[others], base.homographies[others], equal_nan=True)
    # a non-planar group: image 9 takes a bent copy of the board (the template gets 81 more keys, lifted out of the plane)
    bent = rig.points.copy()
    bent[:, 2] = 40.0 * bent[:, 0] ** 2
    pts2 = np.concatenate([rig.points, bent])
    det2 = det.copy()
    det2[det[:, 1] == 9, 2] += 81
    n = hip_ch.estimate_intrinsics(det2, pts2, **kw)
    assert n.group_status[9] == hip_ch.INTR_GROUP_NOT_PLANAR and n.n_groups[0] == 15
    assert np.array_equal(n.homographies[np.arange(17) != 9], base.homographies[np.arange(17) != 9], equal_nan=True)
    assert_matches_restatement(n, det2, pts2, "shapes, one bent board", **kw)


def test_seventeen_cameras_and_no_groups():
    """17 cameras (two blocks of the camera kernel, the second with one live group of lanes): camera 5 has no rows, camera 11 a
    single group (the full model falls back to the focal one).  Then the handle with no groups at all."""
    rig, intr, _, det, _ = rig_of("plane", n_cams=17, n_imgs=4, tilt=2.0)
    det = det[(det[:, 0] != 5) & ((det[:, 0] != 11) | (det[:, 1] == 1))]
    kw = dict(n_cams=17, n_imgs=4, model="full")
    est = hip_ch.estimate_intrinsics(det, rig.points, **kw)
    want = np.full(17, hip_ch.INTR_FULL)
    want[5], want[11] = hip_ch.INTR_NOT_ESTIMATED, hip_ch.INTR_FOCAL_FALLBACK
    assert est.status.tolist() == want.tolist() and est.n_groups[5] == 0 and est.n_groups[11] == 1 and np.all(np.isnan(est.intr[5])) and np.isnan(est.eig_ratio[5])
    full = want == hip_ch.INTR_FULL
    assert rel_err(est.intr[full], intr[full]) <= TRUTH_RTOL
    assert_matches_restatement(est, det, rig.points, "17 cameras", **kw)
    h = hip_ch.IntrinsicsEstimator(3, PLANE.shape[0])
    h.set_template(PLANE)
    h.set_observations(np.zeros(0, dtype=np.int32), np.zeros((0, 2)), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    h.run("full", 13, None)
    K, cinfo, eig, H, frames, ginfo, pix = h.results()
    assert np.all(np.isnan(K)) and np.all(cinfo == 0) and np.all(np.isnan(eig)) and H.shape == (0, 9) and ginfo.shape == (0, 2)
    h.close()


XTOL = 1e-12


def test_refinement_returns_the_truth_of_a_distorted_noise_free_rig():
    """The closed form knows no distortion; the LM behind it does.  Stopped by xtol alone (ftol = gtol = 0: the cost of a noise-free rig
    goes to zero, where a relative decrease and an absolute gradient mean nothing), the solve ends when a step is below
    xtol (xtol + |x|), |x| the norm of the free vector, which the focal lengths dominate.  Steps of a converging Gauss-Newton iteration shrink
    quadratically, so what is left is below the last step: every intrinsic within 10 x xtol x |x| of the truth.  That norm-wise figure
    is loose for the five distortion terms (size 1e-3 to 1e-1), and a bound of 10 x xtol x their own size would be below what the
    pixels can tell: a wrong distortion value shows in the residuals instead.  A pixel coordinate near 1e3 carries 1.1e-13 px of
    rounding, the projection a few such roundings; an RMS below 1e-10 px means no parameter is off by more than rounding allows."""
    rig, intr, _, det, bok = rig_of("cube", distort=True)
    est = hip_ch.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full", refine=True, max_iter=100, xtol=XTOL, ftol=0.0, gtol=0.0)
    assert np.all(est.status == hip_ch.INTR_FULL) and np.all(est.intr_init[:, 4:] == 0.0)
    size = float(np.linalg.norm(est.lm.x))
    err = np.abs(est.intr - intr)
    print(f"closed form off by {rel_err(est.intr_init, intr):.2e} relative; refined: worst error {err.max():.2e} against 10 xtol |x| = {10 * XTOL * size:.2e}; "
          f"RMS {est.rms_init.max():.2e} -> {est.rms.max():.2e} px in {est.lm.nit} iterations, status {est.lm.status}")
    print("error per intrinsic (worst camera): " + " ".join(f"{e:.1e}" for e in err.max(axis=0)))
    assert np.all(err <= 10 * XTOL * size) and np.all(est.rms <= est.rms_init) and np.all(est.rms <= 1e-10)


@pytest.mark.parametrize("kind", ["plane", "cube"])
def test_refinement_of_a_noisy_rig_ends_below_the_truth(kind):
    """0.3 px noise on a distorted rig: the minimum of the reprojection error lies below the error at the true parameters (true
    intrinsics, each view's true pose), per camera and in total."""
    from tests import pnp_reference as pnp
    from tests.test_pnp_reference import true_view_poses

    rig, intr, poses, det, bok = rig_of(kind, noise_px=0.3, tilt=3.5, n_imgs=12, distort=True)
    est = hip_ch.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=12, board_of_key=bok, model="full", refine=True)
    rig.poses_true = poses
    T = true_view_poses(rig)
    sq, cnt = np.zeros(3), np.zeros(3)
    for c in range(3):
        for i in range(12):
            rows = det[(det[:, 0] == c) & (det[:, 1] == i)]
            r = pnp.residuals(T[c, i], rig.points[rows[:, 2].astype(int)], rows[:, 3:5], intr[c])
            sq[c] += np.sum(r * r)
            cnt[c] += rows.shape[0]
    rms_true = np.sqrt(sq / cnt)
    print(f"{kind}: RMS at the closed form {est.rms_init}, refined {est.rms}, at the truth {rms_true}; LM status {est.lm.status} after {est.lm.nit} iterations")
    assert np.all(est.status == hip_ch.INTR_FULL) and np.all(np.isfinite(est.intr))
    assert np.all(est.rms <= rms_true) and np.all(est.rms <= est.rms_init)


def test_from_detections_to_a_finished_calibration_without_intrinsics():
    """The route of tests/test_gpu_pnp.py::test_from_detections_to_a_finished_calibration on the same rig, with the faces of the cube
    as boards and a camset that holds only ``res``: calc_initial_params estimates the intrinsics itself.  The solve ends at the cost of
    the solve started with the rig's jiggled true intrinsics, to the solver's ftol."""
    from pycamset_amd import device_solver

    rig = synthetic.config_rig(1, n_imgs=6)
    td = TargetDetection([f"cam_{i}" for i in range(rig.n_cams)], rig.detections)

    class Target:
        point_data = rig.points.reshape(6, -1, 3).copy()

    def solve(camset, intr):
        h = handlers.TemplateBundleHandler(camset, Target(), td)
        x0 = h.calc_initial_params(intr)
        h.set_initial_params(x0)
        return device_solver.lm_solve(h, h.get_initial_params()), x0, h

    own, x0, h = solve(ResCamset(rig.n_cams), None)
    given, _, _ = solve(DuckCamset(rig.n_cams), rig.intr)
    assert x0.shape == (9 * 3 + 6 * 3 + 6 * 5,) and np.all(np.isfinite(x0)) and np.all(h.initial_intrinsics.status != hip_ch.INTR_NOT_ESTIMATED)
    print(f"cost without intrinsics {own.cost:.12e}, with them {given.cost:.12e}; start off by {rel_err(x0[:27].reshape(3, 9), rig.intr_true):.2e}")
    assert abs(own.cost - given.cost) <= 1e-8 * given.cost


def test_intrinsics_estimator_orders_runs_across_streams():
    """The fence of the handle, driven as tests/test_gpu_pnp.py drives the pose estimator's: run A on a caller stream, new
    observations and run B on the handle's stream without a synchronisation by the caller, run C with the whole table (buffers
    grow), then the full model on the caller stream and the focal one behind it on the handle's stream into the same outputs."""
    import torch

    rig, det, _ = shapes_table()
    kw = dict(n_cams=1, n_imgs=17)
    want = hip_ch.estimate_intrinsics(det, rig.points, model="full", **kw)
    want_f = hip_ch.estimate_intrinsics(det, rig.points, model="focal", **kw)
    assert not np.array_equal(want.intr, want_f.intr)
    order, gid, start = hip_ch.group_by_board(det, 17, np.zeros(81, dtype=np.int64), 1)
    ds = det if order is None else det[order]
    key, uv, gcam = ds[:, 2].astype(np.int32), ds[:, 3:5], np.zeros(17, dtype=np.int32)
    half = 8
    want_h = hip_ch.estimate_intrinsics(ds[: start[half]], rig.points, model="full", **kw)
    est = hip_ch.IntrinsicsEstimator(1, 81)
    est.set_template(rig.points)
    est.set_observations(key[: start[half]], uv[: start[half]], start[: half + 1], gcam[:half])

    def assert_result(w, n):
        K, cinfo, eig, H, frames, ginfo, _ = est.results()
        assert np.array_equal(K, w.intr) and np.array_equal(cinfo[:, 0], w.status) and np.array_equal(eig, w.eig_ratio)
        assert np.array_equal(H.reshape(-1, 3, 3), w.homographies[:n], equal_nan=True) and np.array_equal(ginfo[:, 0], w.group_status[:n])

    side = torch.cuda.Stream()
    est.run("full", stream=side.cuda_stream)                                                      # run A: the caller's stream
    est.set_observations(key[: start[half]], uv[: start[half]], start[: half + 1], gcam[:half])   # no synchronisation by the caller
    est.run("full")                                                                               # run B: the handle's own stream
    assert_result(want_h, half)
    est.set_observations(key, uv, start, gcam)                                                    # the whole table: the buffers grow
    est.run("full", stream=side.cuda_stream)                                                      # run C
    assert_result(want, 17)
    est.run("full", stream=side.cuda_stream)                                                      # back to back: one model ...
    est.run("focal")                                                                              # ... and the other behind it
    assert_result(want_f, 17)
    est.close()
