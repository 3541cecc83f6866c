"""The view-graph seeding without a GPU: ``pose_seeding.estimate_camera_relative_poses_graph`` with the NumPy restatements injected
(tests/pnp_reference.py for the view poses, tests/rig_graph_reference.py for the edges, and for the scores with the oracle's legacy
cost as the residual), against the truth of noise-free rigs and against the existing reference path; the restatement's own pipeline
against the same truth; and the tie condition of every noisy input the GPU tests reuse (tests/rig_graph_inputs.py).

The float64 / extended-precision differences from which tests/test_gpu_rig_graph.py takes its tolerances are printed by
``test_rounding_of_the_restatement`` (``pytest -s``) and recorded in profiles/r13/README.md."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, pose_seeding
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import pnp_reference as pnp
from tests import rig_graph_inputs as inputs
from tests import rig_graph_reference as ref
from tests.test_pnp_reference import DuckCamset, DuckTarget, assert_poses_close, in_frame_of, seed as seed_reference, truth_rig

HOOKS = dict(view_pose_fn=pnp.estimate_view_poses, edge_fn=ref.edge_consensus, score_fn=functools.partial(ref.score_candidates, cost_fn=orc.legacy_cost))


def seed_graph(rig, det, **kw):
    hooks = dict(HOOKS)
    hooks.update(kw)
    return pose_seeding.estimate_camera_relative_poses_graph(det, rig.points, rig.intr_true, rig.n_cams, rig.n_imgs, **hooks)


def assert_truth(rig, extr, poses, ref_pose=0):
    e_t, p_t = in_frame_of(rig, ref_pose)
    assert_poses_close(extr, e_t)
    assert_poses_close(poses, p_t)
    assert np.array_equal(poses[ref_pose], np.zeros(6))


@pytest.mark.parametrize("ref_pose", [0, 2])
def test_fully_visible_rig_gives_the_truth_and_the_reference_paths_result(ref_pose):
    rig, det = truth_rig("cube")
    extr, poses, err, missing, g = seed_graph(rig, det, ref_pose=ref_pose, return_graph=True)
    assert extr.shape == (3, 6) and poses.shape == (3, 6) and err.shape == (3,) and missing.shape == (3,) and not missing.any()
    assert_truth(rig, extr, poses, ref_pose)
    assert err.max() < 1e-6 and list(g.parents) == [-1, 0, 0] and list(g.n) == [3, 3, 3] and g.errors.shape == (3, 3)
    extr_r, poses_r, _, missing_r = seed_reference(rig, det, ref_pose=ref_pose)
    assert_poses_close(extr, extr_r)
    assert_poses_close(poses, poses_r)
    assert np.array_equal(missing, missing_r)
    assert len(seed_graph(rig, det, ref_pose=ref_pose)) == 4


def test_no_common_image_gives_the_truth_where_the_reference_path_raises():
    rig, det = truth_rig("cube")
    cut = det[det[:, 0] != det[:, 1]]                           # camera c misses image c: no image is seen by all
    with pytest.raises(ValueError, match="Couldn't find an initial pose"):
        seed_reference(rig, cut)
    extr, poses, err, missing, g = seed_graph(rig, cut, return_graph=True)
    assert_truth(rig, extr, poses)
    assert not missing.any() and err.max() < 1e-6 and list(g.n) == [1, 1, 1]
    assert np.all(np.isnan(g.errors[[0, 1, 2], [0, 1, 2]])) and np.isfinite(g.errors).sum() == 6   # no forward fill: the unseen views have no candidate


def test_chain_rig_follows_the_chain():
    rig, det = inputs.chain_rig(noise_px=0.0)
    with pytest.raises(ValueError):
        seed_reference(rig, det)
    extr, poses, err, missing, g = seed_graph(rig, det, return_graph=True)
    assert_truth(rig, extr, poses)
    assert list(g.parents) == [-1, 0, 1, 2, 3] and not missing.any() and err.max() < 1e-6
    near = np.abs(g.pairs[:, 0] - g.pairs[:, 1]) == 1
    assert np.all(g.n[near] == 2) and np.all(g.n[~near] == 0) and np.all(np.isinf(g.edge_cost[~near])) and np.all(g.medoid[~near] == -1)
    extr, poses, _, _, g = seed_graph(rig, det, ref_cam=2, ref_pose=5, return_graph=True)   # the tree from the middle of the chain
    assert list(g.parents) == [1, 2, -1, 2, 3]
    assert_truth(rig, extr, poses, 5)


def corrupting(c, i, angle=0.5):
    """A view_pose_fn whose pose of view (c, i) is rotated by ``angle`` rad about the camera's x axis."""
    from scipy.spatial.transform import Rotation

    def fn(*a, **kw):
        vp = pnp.estimate_view_poses(*a, **kw)
        vp.poses[c, i, :3] = (Rotation.from_rotvec([angle, 0, 0]) * Rotation.from_rotvec(vp.poses[c, i, :3])).as_rotvec()
        return vp
    return fn


def test_one_wrong_view_is_outvoted():
    rig, det = truth_rig("cube")                                 # three shared images per pair
    extr, poses, err, missing, g = seed_graph(rig, det, view_pose_fn=corrupting(1, 1), return_graph=True)
    assert_truth(rig, extr, poses)                               # the reference path would take camera 1's extrinsics from this view for ref_pose = 1
    assert g.best_cam[1] in (0, 2) and g.medoid[0] != 1 and g.medoid[2] != 1 and g.errors[1, 1] > 1e3 * err[1]   # pairs (0, 1) and (1, 2) hold camera 1
    extr1, _, _, _ = pose_seeding.estimate_camera_relative_poses(det, rig.points, rig.intr_true, 3, 3, ref_pose=1, view_pose_fn=corrupting(1, 1), cost_fn=orc.legacy_cost)
    with pytest.raises(AssertionError):
        assert_poses_close(extr1, in_frame_of(rig, 1)[0])


def test_an_edge_of_one_shared_image_is_used_when_it_is_the_only_connection():
    rig, det = truth_rig("cube")
    cut = det[(det[:, 0] != 2) | (det[:, 1] == 2)]               # camera 2 sees image 2 only
    extr, poses, _, missing, g = seed_graph(rig, cut, return_graph=True)
    assert_truth(rig, extr, poses)
    assert list(g.n) == [3, 1, 1] and list(g.sigma[1:]) == [0.0, 0.0] and np.all(g.medoid[1:] == 2) and np.all(np.isinf(g.gap[1:]))
    assert np.array_equal(g.edge_cost[1:], [g.rho, g.rho]) and list(g.parents) == [-1, 0, 0]   # equal costs: the lower camera is the parent
    pbar, rho = ref.template_frame(rig.points)
    assert abs(g.rho - rho) <= 1e-15 * rho and rho > 0


def test_unreachable_cameras_are_named():
    rig, det = truth_rig("cube")
    cut = det[((det[:, 0] == 2) & (det[:, 1] == 2)) | ((det[:, 0] != 2) & (det[:, 1] != 2))]   # {0, 1} on images 0, 1; camera 2 alone on image 2
    with pytest.raises(ValueError, match=r"\[2\]"):
        seed_graph(rig, cut)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        seed_graph(rig, cut, ref_cam=2)
    with pytest.raises(ValueError, match=r"cameras \[2\]"):
        ref.seed(cut, rig.points, rig.intr_true, 3, 3, pnp.estimate_view_poses(cut, rig.points, rig.intr_true, 3, 3).poses)


def test_an_image_without_a_candidate_is_missing_and_filled():
    rig, det = truth_rig("cube")
    gone = det[det[:, 1] != 1]                                   # nobody sees image 1: filled from image 0, reported missing
    extr, poses, err, missing, g = seed_graph(rig, gone, return_graph=True)
    assert list(missing) == [False, True, False] and g.best_cam[1] == -1 and np.isnan(err[1]) and np.all(np.isnan(g.errors[:, 1]))
    assert_poses_close(extr, rig.extr_true)
    assert_poses_close(poses[[0, 2]], rig.poses_true[[0, 2]])
    assert_poses_close(poses[1:2], np.zeros((1, 6)), tol=1e-14)           # the copy of pose 0, re-based like every pose
    gone = det[det[:, 1] != 0]                                   # the reference pose itself: the first non-missing image is the world
    extr, poses, _, missing, _ = seed_graph(rig, gone, return_graph=True)
    assert list(missing) == [True, False, False] and np.array_equal(poses[1], np.zeros(6))
    assert_poses_close(poses[0:1], np.zeros((1, 6)), tol=1e-14)
    e_t, p_t = in_frame_of(rig, 1)
    assert_poses_close(extr, e_t)
    assert_poses_close(poses[1:], p_t[1:])


def test_restatement_pipeline_agrees_with_the_product_host_code():
    """Steps 2 and 4 exist twice (pose_seeding, vectorised; the restatement, loops): on the noisy chain rig both give the same tree and,
    from the same edges and scores, the same extrinsics and poses to rounding."""
    rig, det = inputs.chain_rig()
    vp = pnp.estimate_view_poses(det, rig.points, rig.intr_true, 5, 8)
    r = ref.seed(det, rig.points, rig.intr_true, 5, 8, vp.poses, ref_cam=1, ref_pose=3)
    extr, poses, err, missing, g = seed_graph(rig, det, ref_cam=1, ref_pose=3, view_pose_fn=lambda *a, **k: vp, score_fn=ref.score_candidates, return_graph=True)
    assert np.array_equal(g.parents, r.parents) and np.array_equal(g.best_cam, r.best_cam) and np.array_equal(g.medoid, r.edges.medoid)
    assert np.array_equal(missing, r.missing) and np.allclose(err, r.per_im_error, rtol=1e-9, atol=0) and np.allclose(g.errors, r.errors, rtol=1e-9, atol=0, equal_nan=True)
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(g.pairs)}
    want = sorted((c, int(g.medoid[pair_of[(min(c, int(q)), max(c, int(q)))]])) for c, q in enumerate(g.parents) if q >= 0)
    assert sorted((int(c), int(i)) for c, i in zip(*np.nonzero(g.dependent))) == want and len(want) == 4
    assert np.all(np.isfinite(g.errors[g.dependent])) and not np.any(g.best_cam[[i for _, i in want]] == [c for c, _ in want])
    assert_poses_close(extr, pose_seeding.pose_from_4x4(pose_seeding.to_4x4(r.extr)), tol=1e-12)
    assert_poses_close(poses, pose_seeding.pose_from_4x4(pose_seeding.to_4x4(r.poses)), tol=1e-12)
    # the oracle's legacy cost as the residual gives the same errors to rounding
    _, e_orc = ref.score_candidates(det, rig.points, rig.intr_true, vp.poses, r.E, 8, cost_fn=orc.legacy_cost)
    assert np.allclose(e_orc, r.errors, rtol=1e-9, atol=0, equal_nan=True)


def noisy_inputs():
    """(name, dct or None, rig, view poses, n_cams, n_imgs) of every noisy input of tests/test_gpu_rig_graph.py.  The GPU tests feed the
    device PnP's poses, which differ from the restatement's by 1e-9 relative at most (tests/test_gpu_pnp.py): far below the gaps asked for."""
    for kind, vis in inputs.PARITY_RIGS:
        rig, det = inputs.parity_rig(kind, vis)
        yield f"{kind}-{vis}", det, rig, pnp.estimate_view_poses(det, rig.points, rig.intr_true, 3, 3).poses, 3, 3
    rig, det = inputs.chain_rig()
    yield "chain", det, rig, pnp.estimate_view_poses(det, rig.points, rig.intr_true, 5, 8).poses, 5, 8
    for n in inputs.TILE_IMAGES:
        rig, vp = inputs.perturbed_view_poses(2, n)
        yield f"tile-{n}", None, rig, vp, 2, n


def rel_transforms(a, b, rho):
    """Largest element-relative difference of 3 x 4 transforms: rotation entries against max(|entry|, 1), translations against max(|entry|, rho)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    scale = np.maximum(np.abs(b), np.array([1, 1, 1, float(rho)], dtype=np.longdouble))
    d = np.abs(a - b) / scale
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def rel_costs(a, b):
    """Largest relative difference of positive costs (entries that are 0, NaN or inf in the reference must be equal)."""
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    pos = np.isfinite(b) & (b > 0)
    assert np.array_equal(np.asarray(a[~pos], dtype=np.float64), np.asarray(b[~pos], dtype=np.float64), equal_nan=True)
    return float(np.max(np.abs(a[pos] - b[pos]) / b[pos])) if pos.any() else 0.0


def test_tie_condition_of_every_noisy_input():
    """The discrete outputs (medoid, best_cam) can be compared exactly only where rounding cannot flip them: the relative gap between
    best and runner-up exceeds 1e-6 for the medoid score of every pair and for the per-image error of every image.

    Two ties are structural and cannot be moved by a seed; both are decided without rounding having a say.  A pair with exactly two
    shared images (every pair of the 5 x 8 chain rig) has S_0 = d(T_0, T_1) = d(T_1, T_0) = S_1 bit for bit, asserted below, so the lower
    image is the medoid on any machine: the gap is asked of pairs with n >= 3.  And camera c's estimate of the medoid image of the edge to
    its parent repeats the parent's (E_c is made from that view), so c is no candidate there (``RigGraphInfo.dependent``); before that
    rule the per-image gap of the fully visible cube rig was 5.8e-13."""
    for name, det, rig, vp, C, I in noisy_inputs():
        if det is None:
            e = ref.edge_consensus(vp, rig.points)
            g_edge, g_im = min(float((e.runner_up[p] - e.score[p]) / e.runner_up[p]) for p in range(len(e.n)) if e.n[p] >= 2), np.inf
        else:
            r = ref.seed(det, rig.points, rig.intr_true, C, I, vp)
            g_edge, g_im = ref.gaps(r)
            two = r.edges.n == 2
            assert np.array_equal(r.edges.score[two], r.edges.runner_up[two]) and np.all(r.edges.medoid[two] >= 0)
        print(f"{name}: medoid gap {g_edge:.3e}, per-image error gap {g_im:.3e}")
        assert g_edge > 1e-6 and g_im > 1e-6, name


def test_rounding_of_the_restatement():
    """float64 against extended precision on the inputs of the GPU parity test: the figures the GPU tolerances are 8 x of, printed for
    profiles/r13/README.md.  Asserted here: both precisions take the same discrete decisions, and the differences are rounding-sized."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    worst_t, worst_c = 0.0, 0.0
    for name, det, rig, vp, C, I in noisy_inputs():
        if det is None:
            continue
        a, b = ref.seed(det, rig.points, rig.intr_true, C, I, vp), ref.seed(det, rig.points, rig.intr_true, C, I, vp, dtype=np.longdouble)
        assert np.array_equal(a.edges.medoid, b.edges.medoid) and np.array_equal(a.parents, b.parents) and np.array_equal(a.best_cam, b.best_cam)
        rho = float(a.edges.rho)
        t = max(rel_transforms(a.edges.T, b.edges.T, rho), rel_transforms(a.W, b.W, rho), rel_transforms(a.extr, b.extr, rho), rel_transforms(a.poses, b.poses, rho))
        c = max(rel_costs(a.edges.sigma, b.edges.sigma), rel_costs(a.errors, b.errors), rel_costs(a.per_im_error, b.per_im_error))
        print(f"{name}: transforms {t:.3e}, costs {c:.3e}")
        worst_t, worst_c = max(worst_t, t), max(worst_c, c)
    print(f"largest: transforms {worst_t:.3e}, costs {worst_c:.3e}")
    assert worst_t < 1e-11 and worst_c < 1e-9


# ---- calc_initial_params ---------------------------------------------------------------------------------------------------------------
def test_calc_initial_params_seeding(monkeypatch):
    monkeypatch.setattr(hip_ch, "estimate_view_poses", pnp.estimate_view_poses)
    monkeypatch.setattr(hip_ch, "bundle_adjustment_costfn", orc.legacy_cost)
    monkeypatch.setattr(hip_ch, "rig_edge_consensus", ref.edge_consensus)
    monkeypatch.setattr(hip_ch, "rig_candidate_scores", ref.score_candidates)
    rig, det = truth_rig("cube")
    names = [f"cam_{i}" for i in range(3)]
    h = handlers.TemplateBundleHandler(DuckCamset(3), DuckTarget(rig.points), TargetDetection(names, det))
    x_ref = h.calc_initial_params(rig.intr_true)
    for mode in ("graph", "auto"):
        x = h.calc_initial_params(rig.intr_true, seeding=mode)
        assert x.shape == x_ref.shape and np.array_equal(x[:27], x_ref[:27])
        assert_poses_close(x[27:].reshape(-1, 6), x_ref[27:].reshape(-1, 6))
    assert np.array_equal(h.calc_initial_params(rig.intr_true, seeding="auto"), x_ref)   # auto is the reference path where that works
    with pytest.raises(ValueError, match="seeding"):
        h.calc_initial_params(rig.intr_true, seeding="tree")
    cut = det[det[:, 0] != det[:, 1]]
    h = handlers.TemplateBundleHandler(DuckCamset(3), DuckTarget(rig.points), TargetDetection(names, cut))
    with pytest.raises(ValueError, match="Couldn't find an initial pose"):
        h.calc_initial_params(rig.intr_true)
    x_graph = h.calc_initial_params(rig.intr_true, seeding="graph")
    assert list(h.missing_poses) == [False, False, False]
    assert np.array_equal(h.calc_initial_params(rig.intr_true, seeding="auto"), x_graph)
    assert_poses_close(x_graph[27:45].reshape(3, 6), rig.extr_true)
    assert_poses_close(x_graph[45:].reshape(2, 6), rig.poses_true[1:])


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_rig_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 107
    h = ctypes.c_void_p()
    assert lib.pcs_rig_create(None, 0, 3, 3, 8) == _capi.PCS_ERR_ARG
    for bad in ((0, 3, 8), (3, 0, 8), (3, 3, 0), (46341, 1, 8), (40000, 60000, 8)):
        assert lib.pcs_rig_create(ctypes.byref(h), 0, *bad) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_destroy(None) == _capi.PCS_OK
    assert lib.pcs_rig_set_cameras(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_set_template(None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_set_observations(None, 0, None, None, 0, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_set_view_poses(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_set_extrinsics(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_run_edges(None, None) == _capi.PCS_ERR_ARG and b"NULL handle" in lib.pcs_last_error()
    assert lib.pcs_rig_run_scores(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_edges(None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_results(None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_rig_last_kernel_ms(None, None, None, None) == _capi.PCS_ERR_ARG


def test_python_front_end_validates_before_the_device():
    rig, det = truth_rig("cube")
    with pytest.raises(ValueError):
        hip_ch.rig_edge_consensus(np.zeros((3, 3, 5)), rig.points)
    with pytest.raises(ValueError):
        hip_ch.rig_candidate_scores(det[:, :4], rig.points, rig.intr_true, np.zeros((3, 3, 6)), np.zeros((3, 3, 4)), 3)
    with pytest.raises(ValueError):
        hip_ch.rig_candidate_scores(det, rig.points, rig.intr_true, np.zeros((2, 3, 6)), np.zeros((2, 3, 4)), 3)   # camera 2 has no poses
    for kw in ({"ref_cam": 3}, {"ref_pose": -1}):
        with pytest.raises(ValueError, match="ref_cam"):
            seed_graph(rig, det, **kw)
    assert hip_ch.camera_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    parents, order = pose_seeding.shortest_path_tree(4, hip_ch.camera_pairs(4), np.array([1.0, 2.0, np.inf, 1.0, np.inf, np.inf]), 0)
    assert list(parents) == [-1, 0, 0, -1] and order == [0, 1, 2]   # 0-2 direct and 0-1-2 cost the same: the lower parent; camera 3 is not reached
