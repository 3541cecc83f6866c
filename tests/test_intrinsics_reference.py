"""The intrinsics estimation from planar views without a GPU: the NumPy restatement (tests/intrinsics_reference.py) against the truth
of noise-free rigs and against its own extended-precision run, its statuses, ``calc_initial_params`` without intrinsics with the
restatement injected, and the argument checks of the C entry points and of the Python front end.

Measured figures and the bounds derived from them are recorded in profiles/r12/README.md."""
import ctypes

import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import intrinsics_reference as ref
from tests import pnp_reference as pnp_ref
from tests.test_pnp_reference import CUBE, PLANE, DuckCamset, assert_poses_close

FACE_OF_KEY = np.repeat(np.arange(6), CUBE.shape[0] // 6)      # ccube_points lists its six faces one after the other
FACE_NORMALS = np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0]], dtype=np.float64)
RES = (1000, 1000)
# Relative error of (fx, cx, fy, cy) of the restatement on the noise-free, distortion-free rigs below, measured here: 2.56e-13 (plane),
# 2.06e-14 (cube), against 8.69e-14 / 1.90e-14 in extended precision on the same float64 pixels.  The bound is 100 x the larger figure.
TRUTH_RTOL = max(100 * 2.56e-13, 1e-12)


def rig_of(kind, *, noise_px=0.0, distort=False, tilt=1.0, seed=7, n_cams=3, n_imgs=6):
    """(rig, intr (C, 9), poses, table, board_of_key) of ``make_rig``'s geometry, re-projected: without distortion unless ``distort``,
    the rotation part of the target poses scaled by ``tilt``, the cube's faces as boards with the faces that look away from a camera
    removed, Gaussian noise added last (its own generator: the same noise whatever the other switches)."""
    from scipy.spatial.transform import Rotation

    pts = PLANE if kind == "plane" else CUBE
    rig = synthetic.make_rig(f"intr-{kind}", n_cams, n_imgs, pts, seed=seed, noise_px=0.0)
    intr = rig.intr_true.copy()
    if not distort:
        intr[:, 4:] = 0.0
    poses = rig.poses_true.copy()
    poses[:, :3] *= tilt
    uv, _ = synthetic.project_dense(intr, rig.extr_true, poses, pts)
    det = rig.detections.copy()
    c, i, k = (det[:, j].astype(int) for j in range(3))
    det[:, 3:] = uv[c, i, k]
    bok = None
    if kind == "cube":
        bok = FACE_OF_KEY
        Rc = Rotation.from_rotvec(rig.extr_true[:, :3]).as_matrix()
        Rp = Rotation.from_rotvec(poses[:, :3]).as_matrix()
        R = np.einsum("cab,ibd->ciad", Rc, Rp)                                       # target -> camera
        t = np.einsum("cab,ib->cia", Rc, poses[:, 3:]) + rig.extr_true[:, None, 3:]
        n_cam = np.einsum("ciad,fd->cifa", R, FACE_NORMALS)                          # face normals in the camera
        centre = np.einsum("ciad,fd->cifa", R, FACE_NORMALS * 0.015) + t[:, :, None, :]
        front = np.einsum("cifa,cifa->cif", n_cam, centre) < -0.15 * np.linalg.norm(centre, axis=-1)   # seen at less than about 81 degrees
        det = det[front[c, i, bok[k]]]
    if noise_px:
        det = det.copy()
        det[:, 3:] += np.random.default_rng(1000 + seed).normal(0, noise_px, (det.shape[0], 2))
    return rig, intr, poses, det, bok


def rel_err(got, truth):
    return float(np.max(np.abs(np.asarray(got[:, :4], dtype=np.float64) - truth[:, :4]) / np.abs(truth[:, :4])))


@pytest.mark.parametrize("kind", ["plane", "cube"])
def test_full_model_returns_the_truth_of_noise_free_rigs(kind):
    rig, intr, _, det, bok = rig_of(kind)
    r = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full")
    x = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full", dtype=np.longdouble)
    assert np.all(r.status == ref.FULL) and np.all(r.group_status == ref.GROUP_USED)
    assert np.all(r.n_groups == (6 if kind == "plane" else np.bincount(r.group_index[:, 0], minlength=3)))
    if kind == "cube":
        assert 6 <= r.n_groups.min() and 6 < r.n_groups.max() < 36 and len(np.unique(r.group_index[:, 2])) > 1   # at least a face per view, never all six
    print(f"{kind}: relative error float64 {rel_err(r.intr, intr):.2e}, extended {rel_err(x.intr, intr):.2e}; eigenvalue ratio {np.abs(r.eig_ratio).max():.1e}")
    assert rel_err(r.intr, intr) <= TRUTH_RTOL
    assert np.all(r.intr[:, 4:] == 0.0) and np.abs(r.eig_ratio).max() < 1e-12


@pytest.mark.parametrize("kind", ["plane", "cube"])
def test_focal_model_is_as_far_off_as_its_fixed_principal_point(kind):
    """res = (1000, 1000) puts the principal point at 499.5; the true ones are 500 +- 20.  What that costs the focal lengths is a
    property of the input: the extended-precision run shows it, and the float64 run lies within that deviation (plus the full
    model's bound: the two runs round differently)."""
    rig, intr, _, det, bok = rig_of(kind)
    r = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, res=RES)   # auto -> focal
    x = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, res=RES, model="focal", dtype=np.longdouble)
    assert np.all(r.status == ref.FOCAL) and np.all(r.intr[:, [1, 3]] == 499.5)
    dev = np.abs(np.asarray(x.intr[:, [0, 2]], dtype=np.float64) - intr[:, [0, 2]]) / intr[:, [0, 2]]
    got = np.abs(r.intr[:, [0, 2]] - intr[:, [0, 2]]) / intr[:, [0, 2]]
    print(f"{kind}: focal-length deviation of the focal model, extended precision {dev.max():.2e}, float64 {got.max():.2e}")
    assert np.all(got <= dev + TRUTH_RTOL) and dev.max() < 0.2


@pytest.mark.parametrize("kind", ["plane", "cube"])
def test_distorted_noise_free_rigs_give_a_start(kind):
    """The closed form knows no distortion: with it the result is a start, not the answer (the refinement's test is in the GPU file)."""
    rig, intr, _, det, bok = rig_of(kind, distort=True)
    r = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full")
    print(f"{kind}: relative error of the closed form under distortion {rel_err(r.intr, intr):.2e}")
    assert np.all(r.status == ref.FULL) and np.all(r.group_status == ref.GROUP_USED) and np.all(np.isfinite(r.intr))


# What "the refinement converges from this start" asks of a start.  OpenCV's own start (initCameraMatrix2D) puts the principal point
# at the image centre whatever the lens, tens of pixels off on real cameras, and takes focal lengths from a least-squares fit that
# this much inconsistency bends by some percent; calibrateCamera converges from there as a matter of routine.  A fifth of the focal
# length and a fifth of the image half-width (100 px here) is a start of that kind.  The refinement's own test
# (tests/test_gpu_intrinsics.py) starts from the closed form of exactly these rigs and has to end at the truth's RMS.
NOISY_RTOL = 0.20


@pytest.mark.parametrize("kind,model", [("plane", "full"), ("plane", "focal"), ("cube", "full"), ("cube", "focal")])
def test_noisy_rigs_with_tilted_boards_give_a_start_the_refinement_can_use(kind, model):
    """0.3 px noise.  ``make_rig``'s pose spread (0.15 rad) leaves the full model of the 5 x 5 board unconstrained, so the rotations
    are scaled by 3.5 (standard deviation about 0.5 rad per axis) and twelve images are taken."""
    rig, intr, poses, det, bok = rig_of(kind, noise_px=0.3, tilt=3.5, n_imgs=12)
    assert 0.3 < np.abs(poses[:, :3]).max() < 1.2
    r = ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=12, board_of_key=bok, model=model, res=RES if model == "focal" else None)
    assert np.all(r.status == (ref.FULL if model == "full" else ref.FOCAL))
    f_err = np.abs(r.intr[:, [0, 2]] - intr[:, [0, 2]]) / intr[:, [0, 2]]
    c_err = np.abs(r.intr[:, [1, 3]] - intr[:, [1, 3]]) / 500.0
    print(f"{kind} {model}: focal lengths off by {f_err.max():.2e}, principal point by {c_err.max():.2e} of the half-width; eigenvalue ratio {np.abs(r.eig_ratio).max():.1e}")
    assert f_err.max() <= NOISY_RTOL and c_err.max() <= NOISY_RTOL


def test_statuses():
    rig, intr, _, det, _ = rig_of("plane", n_cams=4)
    # camera 3 has no rows at all, camera 2 a single group; camera 1 has one group of 12 observations (refused) among its six
    cut = det[(det[:, 0] < 2) | ((det[:, 0] == 2) & (det[:, 1] == 4))]
    short = (cut[:, 0] == 1) & (cut[:, 1] == 3)
    cut = cut[~short | (np.cumsum(short) <= 12)]
    r = ref.estimate_intrinsics(cut, rig.points, n_cams=4, n_imgs=6, model="full")
    assert r.status.tolist() == [ref.FULL, ref.FULL, ref.FOCAL_FALLBACK, ref.NOT_ESTIMATED] and r.n_groups.tolist() == [6, 5, 1, 0]
    assert np.all(np.isnan(r.intr[3])) and np.isnan(r.eig_ratio[3])
    assert r.group_status[(r.group_index[:, 0] == 1) & (r.group_index[:, 1] == 3)].tolist() == [ref.GROUP_TOO_FEW]
    assert rel_err(r.intr[:2], intr[:2]) <= TRUTH_RTOL
    # one group: two equations for (1 / fx^2, 1 / fy^2) about the mean pixel: a rough but positive answer
    assert np.all(r.intr[2, [0, 2]] > 0) and np.all(r.intr[2, 4:] == 0) and abs(r.intr[2, 0] - intr[2, 0]) < 0.5 * intr[2, 0]
    # min_points is the caller's: with 12 the short group is used as well
    assert ref.estimate_intrinsics(cut, rig.points, n_cams=4, n_imgs=6, model="full", min_points=12).n_groups.tolist() == [6, 6, 1, 0]
    # a non-finite measurement drops its group only
    bad = cut.copy()
    bad[np.nonzero((cut[:, 0] == 0) & (cut[:, 1] == 2))[0][3], 4] = np.inf
    b = ref.estimate_intrinsics(bad, rig.points, n_cams=4, n_imgs=6, model="full")
    assert b.group_status[(b.group_index[:, 0] == 0) & (b.group_index[:, 1] == 2)].tolist() == [ref.GROUP_NOT_FINITE] and b.n_groups[0] == 5
    assert b.status[0] == ref.FULL and rel_err(b.intr[:1], intr[:1]) <= TRUTH_RTOL
    # the whole cube passed as ONE board is not planar: no group is used, no camera estimated
    rig_c = rig_of("cube")[0]
    n = ref.estimate_intrinsics(rig_c.detections, rig_c.points, n_cams=3, n_imgs=6)   # every view holds all six faces
    assert np.all(n.group_status == ref.GROUP_NOT_PLANAR) and np.all(n.status == ref.NOT_ESTIMATED) and np.all(np.isnan(n.intr))


def test_fronto_parallel_views_are_not_estimated():
    """Boards parallel to the image plane (rotations about the optical axis, any translation): the third components of h1 and h2
    vanish, every row of V has only its first two entries, and those are proportional to (fx^2, -fy^2) in all views: V'V has rank one.
    The full model finds more than one vanishing eigenvalue and falls back; the focal system is singular (its two columns are
    parallel); the camera is NOT_ESTIMATED, with either model.  A fallback status would promise focal lengths nothing constrains."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(3)
    intr = np.array([[1000.0, 510.0, 1040.0, 492.0, 0, 0, 0, 0, 0]])
    rows = []
    for im in range(5):
        R = Rotation.from_rotvec([0, 0, rng.uniform(-1, 1)]).as_matrix()
        Xc = PLANE @ R.T + np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.15, 0.3)])
        uv = np.stack([intr[0, 0] * Xc[:, 0] / Xc[:, 2] + intr[0, 1], intr[0, 2] * Xc[:, 1] / Xc[:, 2] + intr[0, 3]], axis=1)
        rows.append(np.column_stack([np.zeros(25), np.full(25, im), np.arange(25), uv]))
    det = np.concatenate(rows)
    for model, res in (("full", None), ("focal", RES), ("focal", None)):
        r = ref.estimate_intrinsics(det, PLANE, n_cams=1, n_imgs=5, model=model, res=res)
        assert np.all(r.group_status == ref.GROUP_USED) and r.n_groups[0] == 5
        assert r.status[0] == ref.NOT_ESTIMATED and np.all(np.isnan(r.intr)), (model, r.status, r.intr)


# ---- calc_initial_params without intrinsics ----------------------------------------------------------------------------------------
class ResCamera:
    res = RES


class ResCamset(DuckCamset):
    """Holds the image size of every camera and nothing else."""

    def __getitem__(self, idc):
        return ResCamera()


class FaceTarget:
    """The cube with its faces as the first key axis: point_data (6, 16, 3), as a Ccube lays them out."""

    def __init__(self):
        self.point_data = CUBE.reshape(6, -1, 3).copy()


def test_calc_initial_params_without_intrinsics(monkeypatch):
    calls = []

    def restatement(*a, **kw):
        calls.append(kw)
        return ref.estimate_intrinsics(*a, **kw)

    monkeypatch.setattr(hip_ch, "estimate_intrinsics", restatement)
    monkeypatch.setattr(hip_ch, "estimate_view_poses", pnp_ref.estimate_view_poses)
    monkeypatch.setattr(hip_ch, "bundle_adjustment_costfn", orc.legacy_cost)
    rig, intr, poses, det, bok = rig_of("cube", n_imgs=3)
    assert np.all(poses[0] == 0)
    td = TargetDetection([f"cam_{i}" for i in range(3)], det)
    h = handlers.TemplateBundleHandler(ResCamset(3), FaceTarget(), td)
    assert h.initial_intrinsics is None
    x = h.calc_initial_params()                                  # no intr, and the camset holds none
    bp = h.bundlePrimitive
    assert x.shape == (9 * 3 + 6 * 3 + 6 * 2,) == (bp.pose_end,) and np.all(np.isfinite(x))
    kw = calls[0]
    assert kw["refine"] is True and np.array_equal(kw["res"], np.full((3, 2), 1000.0)) and np.array_equal(kw["board_of_key"], bok) and kw["n_cams"] == 3
    est = h.initial_intrinsics
    assert np.all(est.status == ref.FOCAL) and np.array_equal(x[:27].reshape(3, 9), est.intr)
    # the focal model's intrinsics are a few percent off (its principal point is the image centre); the poses follow them
    assert np.all(np.abs(x[:27].reshape(3, 9)[:, :4] - intr[:, :4]) <= 0.05 * intr[:, :4])
    assert_poses_close(x[27:45].reshape(3, 6), rig.extr_true, tol=0.1)
    assert_poses_close(x[45:].reshape(2, 6), poses[1:], tol=0.1)
    # a camera with fixed intrinsics keeps them; a free camera without an estimate is named
    fixed = {"cam_1": {"int": intr[1].copy()}}
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), td, fixed_params=fixed)   # no res either: the full model
    x = h.calc_initial_params()
    assert x.shape == (9 * 2 + 6 * 3 + 6 * 2,) and np.all(h.initial_intrinsics.status == ref.FULL) and calls[-1]["res"] is None
    assert np.abs(x[:18].reshape(2, 9)[:, :4] - intr[[0, 2], :4]).max() <= 1e-9 * 1100
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), TargetDetection(td.cam_names, det[(det[:, 0] != 1) | (det[:, 2] % 16 < 10)]), fixed_params=fixed)
    h.calc_initial_params()                                      # camera 1 has ten points per face, fewer than min_points, but its intrinsics are fixed
    assert h.initial_intrinsics.status[1] == ref.NOT_ESTIMATED
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), TargetDetection(td.cam_names, det[(det[:, 0] != 2) | (det[:, 2] % 16 < 10)]), fixed_params=fixed)
    with pytest.raises(ValueError, match=r"holds no intrinsics.*\['cam_2'\]"):
        h.calc_initial_params()
    # callers that bring intrinsics see what they saw before: nothing is estimated
    n = len(calls)
    x = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), td).calc_initial_params(intr)
    assert len(calls) == n and np.array_equal(x[:27].reshape(3, 9), intr)


def test_a_keys_board_is_its_first_key_axis(monkeypatch):
    """(faces, n, 3), (faces, rows, cols, 3) and (n, 3) layouts of ``target.point_data``: the face, the face, one board."""
    seen = []

    def restatement(*a, **kw):
        seen.append(kw["board_of_key"])
        return ref.estimate_intrinsics(*a, **kw)

    monkeypatch.setattr(hip_ch, "estimate_intrinsics", restatement)
    monkeypatch.setattr(hip_ch, "estimate_view_poses", pnp_ref.estimate_view_poses)
    monkeypatch.setattr(hip_ch, "bundle_adjustment_costfn", orc.legacy_cost)

    class Target:
        def __init__(self, point_data):
            self.point_data = point_data

    rig, intr, _, det, bok = rig_of("cube", n_imgs=2)
    td = TargetDetection([f"cam_{i}" for i in range(3)], det)
    for shape in ((6, 16, 3), (6, 4, 4, 3)):
        h = handlers.TemplateBundleHandler(DuckCamset(3), Target(CUBE.reshape(shape).copy()), td)
        x = h.calc_initial_params()
        assert np.array_equal(seen[-1], bok) and np.all(h.initial_intrinsics.status == ref.FULL)
        assert np.abs(x[:27].reshape(3, 9)[:, :4] - intr[:, :4]).max() <= 1e-9 * 1100
    rig, intr, _, det, _ = rig_of("plane", n_imgs=3)
    h = handlers.TemplateBundleHandler(DuckCamset(3), Target(PLANE.copy()), TargetDetection(td.cam_names, det))
    h.calc_initial_params()
    assert np.array_equal(seen[-1], np.zeros(25, dtype=int)) and np.all(h.initial_intrinsics.status == ref.FULL)


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_intr_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 106
    vp = ctypes.c_void_p
    h = vp()
    assert lib.pcs_intr_create(None, 0, 3, 8) == _capi.PCS_ERR_ARG
    assert lib.pcs_intr_create(ctypes.byref(h), 0, 0, 8) == _capi.PCS_ERR_ARG
    assert lib.pcs_intr_create(ctypes.byref(h), 0, 3, 0) == _capi.PCS_ERR_ARG
    assert lib.pcs_intr_destroy(None) == _capi.PCS_OK
    assert lib.pcs_intr_set_template(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_intr_set_observations(None, 0, None, None, 0, None, None) == _capi.PCS_ERR_ARG
    none8 = (None,) * 8
    assert lib.pcs_intr_run(None, 0, 13, None, *none8) == _capi.PCS_ERR_ARG
    assert b"NULL handle" in lib.pcs_last_error()
    for model, min_points in ((-1, 13), (3, 13), (1, 3), (2, 0)):
        assert lib.pcs_intr_run(vp(1), model, min_points, None, *none8) == _capi.PCS_ERR_ARG   # options are checked before the handle is touched
        assert b"bad options" in lib.pcs_last_error()
    assert lib.pcs_intr_results(None, *(None,) * 7) == _capi.PCS_ERR_ARG
    assert lib.pcs_intr_last_kernel_ms(None, None) == _capi.PCS_ERR_ARG


def test_python_front_end_validates_before_the_device():
    rig, _, _, det, bok = rig_of("cube", n_imgs=2)
    ok = dict(n_cams=3, n_imgs=2, board_of_key=bok)
    for kw in ({"model": "zhang"}, {"min_points": 3}, {"min_points": 13.5}, {"res": (1000,)}, {"res": (1000, -1)}, {"res": np.ones((2, 2))},
               {"res": (np.nan, 1000)}, {"board_of_key": bok[:-1]}, {"board_of_key": bok.astype(float)}, {"board_of_key": -bok}, {"n_cams": 2},
               {"n_imgs": 1}, {"max_iter": 5}):
        with pytest.raises(ValueError):
            hip_ch.estimate_intrinsics(det, rig.points, **{**ok, **kw})
    with pytest.raises(ValueError):
        hip_ch.estimate_intrinsics(det[:, :4], rig.points, **ok)
    with pytest.raises(ValueError):
        hip_ch.estimate_intrinsics(det, rig.points[:-1], **ok)   # the last key has no template point
    e = hip_ch.estimate_intrinsics(det[:0], rig.points, **ok, res=RES, refine=True)   # an empty table needs no device
    assert e.intr.shape == (3, 9) and np.all(np.isnan(e.intr)) and np.all(e.status == 0) and e.homographies.shape == (0, 3, 3)
    assert np.all(np.isnan(e.rms)) and e.lm is None and np.array_equal(e.intr_init, e.intr, equal_nan=True)
    assert (hip_ch.INTR_NOT_ESTIMATED, hip_ch.INTR_FULL, hip_ch.INTR_FOCAL, hip_ch.INTR_FOCAL_FALLBACK) == (
        _capi.INTR_NOT_ESTIMATED, _capi.INTR_FULL, _capi.INTR_FOCAL, _capi.INTR_FOCAL_FALLBACK) == (ref.NOT_ESTIMATED, ref.FULL, ref.FOCAL, ref.FOCAL_FALLBACK)
    assert (hip_ch.INTR_GROUP_TOO_FEW, hip_ch.INTR_GROUP_USED, hip_ch.INTR_GROUP_NOT_PLANAR, hip_ch.INTR_GROUP_NOT_FINITE, hip_ch.INTR_GROUP_FIT_FAILED) == (
        ref.GROUP_TOO_FEW, ref.GROUP_USED, ref.GROUP_NOT_PLANAR, ref.GROUP_NOT_FINITE, ref.GROUP_FIT_FAILED)
    # the host grouping: one order whatever the table's, the same groups as the restatement's
    order, gid, start = hip_ch.group_by_board(det, 2, bok, 6)
    ds, index, start_ref = ref.group_rows(det, 2, bok, 6)
    assert np.array_equal(start, start_ref) and np.array_equal(gid, (index[:, 0] * 2 + index[:, 1]) * 6 + index[:, 2])
    assert np.array_equal(det if order is None else det[order], ds)
    perm = np.random.default_rng(0).permutation(det.shape[0])
    order2, gid2, start2 = hip_ch.group_by_board(det[perm], 2, bok, 6)
    assert np.array_equal(gid, gid2) and np.array_equal(start, start2) and np.array_equal(det[perm][order2], ds)
