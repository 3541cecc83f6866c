"""The view-graph seeding on the GPU (include/pcs_hip.h pcs_rig_*, csrc/ba_riggraph.hpp) against its NumPy restatement
(tests/rig_graph_reference.py, itself pinned to noise-free truth in tests/test_rig_graph_reference.py).  Both sides get the same view
poses, the device PnP's.

Tolerances (profiles/r13/README.md).  The restatement in float64 against itself in extended precision on the inputs of the parity test
(``test_rounding_of_the_restatement``, CPU) differs by at most 1.858e-14 in the transforms (element-relative: rotation entries
against max(|entry|, 1), translations against max(|entry|, rho)) and by 1.248e-12 in the costs (relative).  The device is allowed 8 x
that: fused multiply-adds, and another association inside sums of a few hundred terms.  The discrete outputs must be identical;
tests/test_rig_graph_reference.py::test_tie_condition_of_every_noisy_input shows that rounding cannot flip them on these inputs."""
import numpy as np
import pytest

from pycamset_amd import handlers, pose_seeding, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import rig_graph_inputs as inputs
from tests import rig_graph_reference as ref
from tests.test_pnp_reference import CUBE, DuckCamset, DuckTarget, truth_rig
from tests.test_rig_graph_reference import rel_costs, rel_transforms

pytestmark = pytest.mark.gpu

TOL_T = 8 * 1.858e-14   # transforms
TOL_C = 8 * 1.248e-12   # costs


def device_poses(rig, det, n_cams, n_imgs):
    return hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=n_imgs)


def seed_device(rig, det, vp, **kw):
    return pose_seeding.estimate_camera_relative_poses_graph(det, rig.points, rig.intr_true, rig.n_cams, rig.n_imgs, view_pose_fn=lambda *a, **k: vp,
                                                             return_graph=True, **kw)


def assert_edges_match(e, r, what):
    assert np.array_equal(e.n, r.n) and np.array_equal(e.medoid, r.medoid), what
    rho = float(r.rho)
    dt, dc = rel_transforms(e.T, r.T, rho), rel_costs(e.sigma, r.sigma)
    print(f"{what}: edges T {dt:.2e} (bound {TOL_T:.2e}), sigma {dc:.2e} (bound {TOL_C:.2e})")
    assert dt <= TOL_T and dc <= TOL_C, what
    assert abs(e.rho - rho) <= 4e-16 * rho


def assert_matches_restatement(rig, det, vp, what, **kw):
    extr, poses, err, missing, g = seed_device(rig, det, vp, **kw)
    r = ref.seed(det, rig.points, rig.intr_true, rig.n_cams, rig.n_imgs, vp.poses, **kw)
    assert np.array_equal(g.n, r.edges.n) and np.array_equal(g.medoid, r.edges.medoid) and np.array_equal(g.parents, r.parents), what
    assert np.array_equal(g.best_cam, r.best_cam) and np.array_equal(missing, r.missing), what
    rho = float(r.edges.rho)
    M = lambda p: pose_seeding.pose_to_4x4(p)[:, :3, :]   # noqa: E731
    d = {"T": rel_transforms(g.T, r.edges.T, rho), "extr": rel_transforms(M(extr), r.extr, rho), "poses": rel_transforms(M(poses), r.poses, rho),
         "sigma": rel_costs(g.sigma, r.edges.sigma), "errors": rel_costs(g.errors, r.errors), "per_im_error": rel_costs(err, r.per_im_error)}
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f" (bounds: transforms {TOL_T:.2e}, costs {TOL_C:.2e})")
    assert max(d["T"], d["extr"], d["poses"]) <= TOL_T and max(d["sigma"], d["errors"], d["per_im_error"]) <= TOL_C, (what, d)
    return g, r


@pytest.mark.parametrize("kind,vis", inputs.PARITY_RIGS)
def test_parity_with_the_restatement(kind, vis):
    rig, det = inputs.parity_rig(kind, vis)
    assert_matches_restatement(rig, det, device_poses(rig, det, 3, 3), f"{kind}-{vis}")


def test_parity_on_the_chain_rig():
    rig, det = inputs.chain_rig()
    g, _ = assert_matches_restatement(rig, det, device_poses(rig, det, 5, 8), "chain")
    assert list(g.parents) == [-1, 0, 1, 2, 3]
    assert_matches_restatement(rig, det, device_poses(rig, det, 5, 8), "chain from camera 3", ref_cam=3, ref_pose=6)


@pytest.mark.parametrize("n_imgs", inputs.TILE_IMAGES)
def test_edge_kernel_at_the_tile_boundaries(n_imgs):
    """C = 2, one pair, n = TILE - 1, TILE, TILE + 1 and 2 TILE + 1 candidates; with n_imgs = 2 TILE + 1 every other image of camera 1 is
    taken away as well, so that tiles hold candidates and gaps."""
    rig, vp = inputs.perturbed_view_poses(2, n_imgs)
    assert_edges_match(hip_ch.rig_edge_consensus(vp, rig.points), ref.edge_consensus(vp, rig.points), f"n = {n_imgs}")
    if n_imgs == 2 * inputs.TILE + 1:
        vp = vp.copy()
        vp[1, 1::2] = np.nan
        e = hip_ch.rig_edge_consensus(vp, rig.points)
        assert e.n[0] == inputs.TILE + 1
        assert_edges_match(e, ref.edge_consensus(vp, rig.points), "every other image")


def test_pairs_with_one_and_with_no_shared_image():
    rig, vp = inputs.perturbed_view_poses(3, 4)
    vp = vp.copy()
    vp[0, 1:] = np.nan          # camera 0 has image 0 only
    vp[2, 0] = np.nan           # camera 2 has images 1..3: pair (0, 1) n = 1, pair (0, 2) n = 0, pair (1, 2) n = 3
    vp[1, 2, 4] = np.nan        # a pose with one non-finite entry is no pose: pair (1, 2) n = 2
    e, r = hip_ch.rig_edge_consensus(vp, rig.points), ref.edge_consensus(vp, rig.points)
    assert list(e.n) == [1, 0, 2] and list(e.medoid) == [0, -1, 1]
    assert e.sigma[0] == 0.0 and np.isinf(e.runner_up[0]) and np.isnan(e.sigma[1]) and np.all(np.isnan(e.T[1])) and e.score[2] == e.runner_up[2]
    assert_edges_match(e, r, "n = 1, 0, 2")


def shapes_table():
    """The noisy cube rig (3 x 3) with view (0, 1) cut to one detection, view (1, 2) to 17 (one more than the lane group), image 2 kept
    by camera 1 only (an image with a single view), and the rows shuffled (a table not sorted by camera)."""
    rig, det = inputs.parity_rig("cube", 1.0)
    keep = np.ones(det.shape[0], dtype=bool)
    for (c, i), n in {(0, 1): 1, (1, 2): inputs.G + 1, (0, 2): 0, (2, 2): 0}.items():
        keep[np.nonzero((det[:, 0] == c) & (det[:, 1] == i))[0][n:]] = False
    det = det[keep]
    return rig, det[np.random.default_rng(3).permutation(det.shape[0])]


def test_scoring_at_the_shapes_at_which_it_can_go_wrong():
    rig, det = shapes_table()
    vp = device_poses(rig, det, 3, 3)
    assert np.all(np.isnan(vp.poses[0, 1])) and vp.n_points[0, 1] == 1 and vp.n_points[1, 2] == inputs.G + 1 and vp.n_points[2, 2] == 0
    g, r = assert_matches_restatement(rig, det, vp, "shapes")
    assert np.isnan(g.errors[0, 1]) and np.isfinite(g.errors[1:, 1]).all()       # the one-detection view is scored for the other cameras' candidates
    assert g.best_cam[2] == 1 and np.isnan(g.errors[[0, 2], 2]).all()
    # the partial sums per (candidate, view), the same table sorted
    ds, ids, start = ref.group_views(det, 3)
    W, errors = hip_ch.rig_candidate_scores(ds, rig.points, rig.intr_true, vp.poses, r.E, 3)
    graph = hip_ch._rig_graph(0, 3, 3, rig.points.shape[0])
    _, errors2, partial = graph.results(partial=True)
    assert np.array_equal(errors, errors2, equal_nan=True) and partial.shape == (3, len(ids))
    assert rel_costs(partial, r.partial) <= TOL_C and rel_transforms(W, r.W, float(r.edges.rho)) <= TOL_T
    _, shuffled = hip_ch.rig_candidate_scores(det, rig.points, rig.intr_true, vp.poses, r.E, 3)
    assert np.array_equal(errors, shuffled, equal_nan=True)                       # sorted or shuffled: the same bits


def test_a_camera_without_any_view_pose_is_reported_unreachable():
    rig, det = inputs.parity_rig("cube", 1.0)
    vp = device_poses(rig, det, 3, 3)
    vp.poses[2] = np.nan
    with pytest.raises(ValueError, match=r"cameras \[2\]"):
        seed_device(rig, det, vp)


def test_two_runs_give_the_same_bits():
    rig, det = inputs.chain_rig()
    vp = device_poses(rig, det, 5, 8)
    a, b = seed_device(rig, det, vp), seed_device(rig, det, vp)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y, equal_nan=True)
    for name in ("n", "medoid", "sigma", "gap", "T", "parents", "best_cam", "errors"):
        assert np.array_equal(getattr(a[4], name), getattr(b[4], name), equal_nan=True), name
    rig, poses = inputs.perturbed_view_poses(2, 2 * inputs.TILE + 1)
    e1, e2 = hip_ch.rig_edge_consensus(poses, rig.points), hip_ch.rig_edge_consensus(poses, rig.points)
    assert np.array_equal(e1.T, e2.T) and np.array_equal(e1.score, e2.score) and np.array_equal(e1.runner_up, e2.runner_up)


@pytest.mark.parametrize("unseen", [None, 2])
def test_fully_visible_ring_agrees_with_the_existing_device_path(unseen):
    """Ring-8 (8 cameras x 4 images of the cube), ``ref_pose`` 0 and a ``ref_pose`` nobody sees (both paths then take image 0).

    The ring is noise-free on purpose.  The two paths are different estimators: the existing one takes camera c's extrinsics from its
    view of the reference image alone, this one from the medoid image of a tree edge.  Where the view poses are consistent with one rig
    (no noise) both must give the same transforms to the parity tolerance, which is asserted; with 0.3 px of noise they differ by the
    noise of the view poses, which is printed and not asserted.  Figures: profiles/r13/README.md."""
    rig, det = inputs.ring_rig(8, 4, noise_px=0.0)
    ref_pose = 0
    if unseen is not None:
        det, ref_pose = det[det[:, 1] != unseen], unseen
    vp = device_poses(rig, det, 8, 4)
    extr, poses, err, missing, g = seed_device(rig, det, vp, ref_pose=ref_pose)
    extr_r, poses_r, err_r, missing_r = pose_seeding.estimate_camera_relative_poses(det, rig.points, rig.intr_true, 8, 4, ref_pose=ref_pose,
                                                                                    view_pose_fn=lambda *a, **k: vp)
    assert np.array_equal(missing, missing_r) and list(missing) == [i == unseen for i in range(4)]
    rho = g.rho
    M = lambda p: pose_seeding.pose_to_4x4(p)[:, :3, :]   # noqa: E731
    d_e, d_p = rel_transforms(M(extr), M(extr_r), rho), rel_transforms(M(poses), M(poses_r), rho)
    print(f"ring-8, ref_pose {ref_pose}: extr {d_e:.2e}, poses {d_p:.2e} (bound {TOL_T:.2e})")
    assert d_e <= TOL_T and d_p <= TOL_T
    if unseen is None:   # measured only: the same ring with 0.3 px of noise
        rig, det = inputs.ring_rig(8, 4)
        vp = device_poses(rig, det, 8, 4)
        a = seed_device(rig, det, vp)
        b = pose_seeding.estimate_camera_relative_poses(det, rig.points, rig.intr_true, 8, 4, view_pose_fn=lambda *x, **k: vp)
        print(f"ring-8 with 0.3 px noise (not asserted): extr {rel_transforms(M(a[0]), M(b[0]), rho):.2e}, poses {rel_transforms(M(a[1]), M(b[1]), rho):.2e}")


def test_a_pose_for_an_image_without_detections_is_no_candidate():
    """View poses from the full table, scored against a table that has lost every row of image 1: W[:, 1] is finite, but no view of the
    image exists, so its errors are NaN (not an empty sum of 0 that would win every argmin) and the image is missing."""
    rig, det = inputs.parity_rig("cube", 1.0)
    vp = device_poses(rig, det, 3, 3)
    g, r = assert_matches_restatement(rig, det[det[:, 1] != 1], vp, "image without detections")
    assert np.all(np.isnan(g.errors[:, 1])) and g.best_cam[1] == -1 and np.all(np.isnan(r.errors[:, 1]))


def test_from_a_neighbours_only_ring_to_a_finished_calibration():
    """A ring of 4 cameras, 8 images, every image kept by two neighbouring cameras only: ``calc_initial_params()`` raises,
    ``seeding="graph"`` and ``"auto"`` give the same start, and ``lm_solve`` from it ends with the cost of the solve started from the
    rig's jiggled truth, to the criterion of tests/test_gpu_pnp.py::test_from_detections_to_a_finished_calibration."""
    from pycamset_amd import device_solver

    rig, det = inputs.ring_rig(4, 8, neighbours_only=True)
    td = TargetDetection([f"cam_{i}" for i in range(4)], det)

    def solve(x0_of):
        h = handlers.TemplateBundleHandler(DuckCamset(4), DuckTarget(rig.points), td)
        x0 = x0_of(h)
        h.set_initial_params(x0)
        return device_solver.lm_solve(h, h.get_initial_params()), x0

    h = handlers.TemplateBundleHandler(DuckCamset(4), DuckTarget(rig.points), td)
    with pytest.raises(ValueError, match="Couldn't find an initial pose"):
        h.calc_initial_params(rig.intr)
    x_graph = h.calc_initial_params(rig.intr, seeding="graph")
    assert np.array_equal(h.calc_initial_params(rig.intr, seeding="auto"), x_graph) and not np.any(h.missing_poses)
    seeded, x0 = solve(lambda hh: hh.calc_initial_params(rig.intr, seeding="auto"))
    truth, _ = solve(lambda hh: np.concatenate([rig.intr.ravel(), rig.extr.ravel(), rig.poses[1:].ravel()]))
    assert np.array_equal(x0, x_graph) and x0.shape == (9 * 4 + 6 * 4 + 6 * 7,) and np.all(np.isfinite(x0))
    print(f"cost from the seeded start {seeded.cost:.12e}, from the jiggled truth {truth.cost:.12e}")
    assert abs(seeded.cost - truth.cost) <= 1e-8 * truth.cost
