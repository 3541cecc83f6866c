"""The batched point-set registration on the device (include/pcs_hip.h pcs_align_run, csrc/ba_align.hpp) against its NumPy restatement
(tests/align_reference.py), at the smallest shapes at which the kernels can go wrong, and the front ends built on it.

The bounds.  ALIGN_GAP (tests/align_inputs.py) is the largest float64-versus-extended difference of the restatement over the parity
inputs, as (|dR|, |dt| / scene size, |ds| / s) = (7.35e-15, 1.15e-9, 1.25e-15); tests/test_align_reference.py recomputes it.  The device
is held to 8 x these: the margin covers the butterfly sums of the device against the sequential ones of the restatement over at most 257
rows, and fused multiply-adds, the margin the other suites use.  The discrete outputs (rows used, inliers, status, hypothesis, flags) must
be identical, which the conditions asserted in tests/test_align_reference.py (no distance at the threshold, a clear winner) make a fair
demand."""
import ctypes
import functools

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as ch
from tests import align_inputs as inp
from tests import align_reference as ref

pytestmark = pytest.mark.gpu
MARGIN = 8.0
MODELS = ("rigid", "similarity")


@functools.lru_cache(maxsize=None)
def parity_tables():
    return inp.parity_inputs()


@functools.lru_cache(maxsize=None)
def consensus_tables():
    return inp.consensus_inputs()


@functools.lru_cache(maxsize=None)
def restated(kind, name, model, weighted, H):
    """The restatement's float64 result of one input, computed once and left unchanged."""
    tb = (parity_tables() if kind == "parity" else consensus_tables())[name]
    return ref.align_table(tb["src"], tb["dst"], tb["start"], tb["weights"] if weighted else None, model=model, n_hypotheses=H,
                           inlier_dist=inp.INLIER_DIST if H else None, seed=inp.SEED)


def run_device(src, dst, start, weights=None, model="rigid", H=0, lanes=0, min_points=3, aligner=None):
    """-> the dict of ``align_reference.align_table`` from the device."""
    al = aligner or ch.PointAligner()
    try:
        al.set_points(src, dst, start, weights)
        al.set_consensus(H, inp.INLIER_DIST if H else 0.0, inp.SEED)
        al.run(model=model, min_points=min_points, group_lanes=lanes)
        T, scale, info, stats, inl, dist = al.results()
    finally:
        if aligner is None:
            al.close()
    return {"R": T[:, :, :3], "t": T[:, :, 3], "scale": scale, "rms": stats[:, 0], "score": stats[:, 1], "cond": stats[:, 2], "info": info,
            "inlier": inl, "dist": dist, "T": T}


def check_against(dev, res, size, reach, what):
    assert np.array_equal(dev["info"], res["info"]), (what, dev["info"].tolist(), res["info"].tolist())
    assert np.array_equal(dev["inlier"], res["inlier"]), what
    gap = ref.transform_gap(dev, res, size)
    print(f"{what}: gap {gap[0]:.2e} {gap[1]:.2e} {gap[2]:.2e} (bounds {MARGIN * inp.ALIGN_GAP[0]:.2e} {MARGIN * inp.ALIGN_GAP[1]:.2e} {MARGIN * inp.ALIGN_GAP[2]:.2e})")
    assert all(g <= MARGIN * b for g, b in zip(gap, inp.ALIGN_GAP)), (what, gap)
    ok = res["info"][:, 2] == ref.OK
    assert np.all(np.isfinite(dev["T"][ok])) and np.all(np.isnan(dev["T"][~ok])) and np.all(np.isnan(dev["scale"][~ok])) and np.all(np.isnan(dev["rms"][~ok])), what
    assert np.all(np.abs(np.linalg.det(dev["R"][ok]) - 1.0) <= 16 * np.finfo(np.float64).eps), what      # proper rotations
    # a distance moves by at most |dR| s |x| + |ds| |x| + |dt|: the three bounds on the reach of the problem's coordinates
    d_bound = MARGIN * ((inp.ALIGN_GAP[0] + inp.ALIGN_GAP[2]) * 2.0 * reach + inp.ALIGN_GAP[1] * float(np.max(size)))
    assert np.array_equal(np.isnan(dev["dist"]), np.isnan(np.asarray(res["dist"], dtype=np.float64))), what
    fin = np.isfinite(dev["dist"])
    assert np.all(np.abs(dev["dist"][fin] - np.asarray(res["dist"], dtype=np.float64)[fin]) <= d_bound), what
    assert np.all(np.abs(dev["rms"][ok] - np.asarray(res["rms"], dtype=np.float64)[ok]) <= d_bound), what
    assert np.allclose(dev["cond"][ok], np.asarray(res["cond"], dtype=np.float64)[ok], rtol=0, atol=1e-13), what


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (16, 64))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ("batch", "single", "planar", "mirrored", "offset"))
def test_parity_with_the_restatement(name, model, weighted, lanes):
    """'batch': 37 problems of 3, 4, 15, 16, 17, 33, 63, 64, 65 and 257 rows with empty ones between; 'single': one problem; 'planar',
    'mirrored' (det R = +1 all the same), 'offset' (both centroids 1e6 from the origin)."""
    tb = parity_tables()[name]
    dev = run_device(tb["src"], tb["dst"], tb["start"], tb["weights"] if weighted else None, model=model, lanes=lanes)
    reach = float(np.max(np.abs(tb["src"])) + np.max(np.abs(tb["dst"])))
    check_against(dev, restated("parity", name, model, weighted, 0), tb["size"], reach, f"{name}-{model}-w{int(weighted)}-G{lanes}")
    if name == "batch":
        assert np.array_equal(dev["info"][:, 2] == ref.TOO_FEW, np.diff(tb["start"]) == 0)


def test_width_rule_and_two_runs_give_the_same_bits():
    tb = parity_tables()["batch"]
    a = run_device(tb["src"], tb["dst"], tb["start"], tb["weights"], model="similarity")
    b = run_device(tb["src"], tb["dst"], tb["start"], tb["weights"], model="similarity")
    narrow = run_device(tb["src"], tb["dst"], tb["start"], tb["weights"], model="similarity", lanes=16)
    for k in ("T", "scale", "rms", "cond", "dist", "info", "inlier"):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k].tobytes() == narrow[k].tobytes(), k          # a mean of 31 rows per problem: 16 lanes
    one = parity_tables()["planar"]
    big = inp.sub_table(one, [3])                                  # 257 rows in one problem: a mean of 256 rows or more, 64 lanes
    assert run_device(*big)["T"].tobytes() == run_device(*big, lanes=64)["T"].tobytes()


# ---- statuses -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (16, 64))
def test_statuses_and_untouched_neighbours(lanes):
    st = inp.status_inputs()
    dev = run_device(st["src"], st["dst"], st["start"], lanes=lanes)
    res = ref.align_table(st["src"], st["dst"], st["start"])
    print("status", dev["info"][:, 2].tolist(), "rows used", dev["info"][:, 0].tolist(), "conditioning", dev["cond"].tolist())
    assert np.array_equal(dev["info"][:, 2], st["expected"]) and np.array_equal(dev["info"], res["info"])
    bad = dev["info"][:, 2] != ref.OK
    assert np.all(np.isnan(dev["T"][bad])) and np.all(np.isnan(dev["scale"][bad])) and np.all(np.isnan(dev["rms"][bad]))
    j = st["nan_row_problem"]
    a = int(st["start"][j])
    assert dev["info"][j, 0] == st["start"][j + 1] - a - 1 and not dev["inlier"][a + 7] and np.isnan(dev["dist"][a + 7])
    assert dev["cond"][5] <= 1e-10 and np.isnan(dev["cond"][1])
    alone = run_device(*inp.sub_table(st, st["good"]), lanes=lanes)
    for k in ("T", "scale", "rms", "cond"):
        assert dev[k][st["good"]].tobytes() == alone[k].tobytes(), k   # the bits of a run without the bad problems


def test_min_points_and_zero_weights():
    tb = parity_tables()["batch"]
    dev = run_device(tb["src"], tb["dst"], tb["start"], tb["weights"], min_points=16)
    used = np.array([int(np.sum(tb["weights"][a:b] > 0)) for a, b in zip(tb["start"][:-1], tb["start"][1:])])
    assert np.array_equal(dev["info"][:, 0], used)
    assert np.array_equal(dev["info"][:, 2] == ref.OK, used >= 16) and np.array_equal(dev["info"][:, 2] == ref.TOO_FEW, used < 16)
    assert np.array_equal(dev["inlier"], (tb["weights"] > 0) & np.repeat(used >= 16, np.diff(tb["start"])))


# ---- consensus ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (16, 64))
@pytest.mark.parametrize("H", inp.HYPOTHESES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ("clean", "outliers"))
def test_consensus_matches_the_restatement(name, model, H, lanes):
    """The same hypothesis, flags and counts, exactly; the transform within the parity bounds; the score within 8 x the relative
    rounding of a sum of at most 257 squared distances, each of which moves by twice the distance bound."""
    tb = consensus_tables()[name]
    dev = run_device(tb["src"], tb["dst"], tb["start"], model=model, H=H, lanes=lanes)
    res = restated("consensus", name, model, False, H)
    reach = float(np.max(np.abs(tb["src"])) + np.max(np.abs(tb["dst"])))
    check_against(dev, res, tb["size"], reach, f"{name}-{model}-H{H}-G{lanes}")
    sc, sc_r = dev["score"], np.asarray(res["score"], dtype=np.float64)
    assert np.array_equal(np.isnan(sc), np.isnan(sc_r)) and np.array_equal(np.isinf(sc), np.isinf(sc_r))
    fin = np.isfinite(sc_r)
    d_bound = MARGIN * ((inp.ALIGN_GAP[0] + inp.ALIGN_GAP[2]) * 2.0 * reach + inp.ALIGN_GAP[1] * float(np.max(tb["size"])))
    assert np.all(np.abs(sc[fin] - sc_r[fin]) <= 257 * 2.0 * inp.INLIER_DIST * d_bound + MARGIN * 257 * np.finfo(np.float64).eps * sc_r[fin])


@pytest.mark.parametrize("model", MODELS)
def test_consensus_off_and_all_inliers_keep_the_plain_bits(model):
    tb = consensus_tables()["clean"]
    al = ch.PointAligner()
    try:
        plain = run_device(tb["src"], tb["dst"], tb["start"], model=model, aligner=al)
        cons = run_device(tb["src"], tb["dst"], tb["start"], model=model, H=64, aligner=al)
        off = run_device(tb["src"], tb["dst"], tb["start"], model=model, H=0, aligner=al)       # the same handle, switched off again
        again = run_device(tb["src"], tb["dst"], tb["start"], model=model, H=64, aligner=al)
    finally:
        al.close()
    assert np.all(cons["inlier"]) and np.all(cons["info"][np.diff(tb["start"]) >= 3, 3] >= 0)
    for k in ("T", "scale", "rms", "cond", "dist", "inlier"):
        assert plain[k].tobytes() == cons[k].tobytes(), k
        assert plain[k].tobytes() == off[k].tobytes(), k
    for k in ("T", "scale", "rms", "cond", "dist", "inlier", "info", "score"):
        assert cons[k].tobytes() == again[k].tobytes(), k
    assert np.all(off["info"][:, 3] == -1) and np.all(np.isnan(off["score"]))


@pytest.mark.parametrize("model", MODELS)
def test_consensus_recovers_the_clean_fit_where_the_plain_fit_does_not(model):
    tb = consensus_tables()["outliers"]
    clean_w = (~tb["outlier"]).astype(np.float64)
    cons = run_device(tb["src"], tb["dst"], tb["start"], model=model, H=64)
    plain = run_device(tb["src"], tb["dst"], tb["start"], model=model)
    clean = ref.align_table(tb["src"], tb["dst"], tb["start"], clean_w, model=model)
    big = np.nonzero(np.diff(tb["start"]) >= 20)[0]
    assert np.array_equal(cons["inlier"], ~tb["outlier"])
    pick = {k: (v[big] if k in ("R", "t", "scale") else v) for k, v in cons.items()}
    pick["info"] = clean["info"][big]
    gap = ref.transform_gap(pick, {"R": clean["R"][big], "t": clean["t"][big], "scale": clean["scale"][big], "info": clean["info"][big]}, tb["size"][big])
    print(model, "gap to the fit of the clean rows", gap)
    assert all(g <= MARGIN * b for g, b in zip(gap, inp.ALIGN_GAP)), gap
    miss = np.max(np.abs(plain["R"][big] - np.asarray(clean["R"], dtype=np.float64)[big]), axis=(1, 2))
    assert np.all(miss > 1e-3), miss                              # the plain fit is bent by the outliers


# ---- the front ends --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def triangulated_rig():
    """(rig, ext (C, 3, 4), points by image (I, K, 3) triangulated on the device from noise-free pixels, their largest error)."""
    from pycamset_amd.pose_seeding import intrinsic_matrices, pose_to_4x4

    rig = inp.overlap_rig(0.0)
    E = pose_to_4x4(rig.extr_true)[:, :3, :]
    d = rig.detections[np.lexsort((rig.detections[:, 0], rig.detections[:, 2], rig.detections[:, 1]))]
    rec, start = ch.group_reconstructable(d)
    Km = intrinsic_matrices(rig.intr_true)
    X = ch.nb_triangulate_full(rec, Km @ E, start, Km, rig.intr_true[:, 4:9])
    by_image = np.full((rig.n_imgs, rig.n_keys, 3), np.nan)
    head = rec[start[:-1]]
    by_image[head[:, 1].astype(int), head[:, 2].astype(int)] = X
    Rp = np.stack([ref_rot(p) for p in rig.poses_true[:, :3]])
    truth = np.einsum("iab,kb->ika", Rp, rig.points_true) + rig.poses_true[:, None, 3:]
    return rig, E, by_image, float(np.nanmax(np.abs(by_image - truth)))


def ref_rot(rv):
    from scipy.spatial.transform import Rotation

    return Rotation.from_rotvec(rv).as_matrix()


def test_register_target_matches_the_true_poses():
    """Against the restatement on the same triangulated points: the parity bounds (a rotation vector moves like R).  Against truth: a
    fit over K points that are each off by at most e turns by at most e / (r cond), r the RMS radius of the target, and its
    translation moves by at most e plus that turn times the distance of the centroid; a factor 4 on both."""
    rig, E, by_image, e_tri = triangulated_rig()
    assert np.all(np.isfinite(by_image))
    by_image = by_image.copy()
    by_image[1, ::3] = np.nan                                      # an image that lacks a third of its features
    poses = ch.register_target(by_image, rig.points_true)
    res = ch.register_target.last
    poses_r, tab = ref.register_target(by_image, rig.points_true)
    assert np.array_equal(res.status, tab["info"][:, 2]) and np.all(res.status == ch.ALIGN_OK) and res.n_used[1] == 64
    size = float(np.linalg.norm(np.ptp(rig.points_true, axis=0)))
    assert np.max(np.abs(poses[:, :3] - poses_r[:, :3])) <= MARGIN * inp.ALIGN_GAP[0] * 4.0     # |d rotvec| <= 2 |dR|_F <= 4 max |dR| or so
    assert np.max(np.abs(poses[:, 3:] - poses_r[:, 3:])) <= MARGIN * inp.ALIGN_GAP[1] * size
    r = float(np.sqrt(np.mean(np.sum((rig.points_true - rig.points_true.mean(axis=0)) ** 2, axis=1))))
    turn = 4.0 * e_tri / (r * float(np.min(res.conditioning)))
    print("triangulation error", e_tri, "pose error", np.max(np.abs(poses - rig.poses_true), axis=0), "bounds", turn, 4.0 * e_tri + turn * float(np.linalg.norm(rig.points_true.mean(axis=0))))
    assert np.max(np.abs(poses[:, :3] - rig.poses_true[:, :3])) <= turn
    assert np.max(np.abs(poses[:, 3:] - rig.poses_true[:, 3:])) <= 4.0 * e_tri + turn * float(np.linalg.norm(rig.points_true.mean(axis=0)))


def test_rig_pose_start_3d_lets_the_localiser_converge_where_the_pnp_start_does():
    """0.3 px noise: both starts end in the same minimum, poses within 10 x the xtol of the solve relative to the pose's size, and
    ``find_target_poses(start="triangulation")`` is that path."""
    from pycamset_amd import find_target
    from pycamset_amd.pose_seeding import pose_to_4x4

    rig = inp.overlap_rig(0.3)
    E = pose_to_4x4(rig.extr_true)[:, :3, :]
    start3d = ch.rig_pose_start_3d(rig.detections, rig.points_true, rig.intr_true, E, rig.n_imgs)
    assert start3d.shape == (rig.n_imgs, 6) and np.all(np.isfinite(start3d))
    xtol = 1e-10
    a = ch.localise_target(rig.detections, rig.points_true, rig.intr_true, E, n_imgs=rig.n_imgs, poses_init=start3d, xtol=xtol, ftol=1e-14, gtol=1e-14, max_iter=100)
    b = ch.localise_target(rig.detections, rig.points_true, rig.intr_true, E, n_imgs=rig.n_imgs, xtol=xtol, ftol=1e-14, gtol=1e-14, max_iter=100)
    c = find_target.find_target_poses(rig.detections, rig.points_true, rig.intr_true, E, start="triangulation", xtol=xtol, ftol=1e-14, gtol=1e-14, max_iter=100)
    print("start error", np.max(np.abs(start3d - rig.poses_true)), "difference of the ends", np.max(np.abs(a.poses - b.poses)), "rms", a.rms.tolist())
    assert np.all(a.status == ch.RIGPOSE_CONVERGED) and np.all(b.status == ch.RIGPOSE_CONVERGED)
    assert np.max(np.abs(a.poses - b.poses)) <= 10.0 * xtol * max(1.0, float(np.max(np.abs(b.poses))))
    assert a.poses.tobytes() == c.poses.tobytes()
    with pytest.raises(ValueError):
        find_target.find_target_poses(rig.detections, rig.points_true, rig.intr_true, E, start="guess")


def test_align_scene_brings_the_seed_onto_truth_and_keeps_every_reprojection():
    """chain_rig(0.0): after ``align_scene`` onto the true points the seed IS the truth within 8 x SCENE_GAP (relative to the scene's
    size; the seed itself is that close, tests/test_gpu_twoview.py), and every pixel stays where it was within 1e-9 px: a pixel of about
    1e3 moves by a few of its units in the last place, 2e-13, times the few dozen operations between the two parameterisations."""
    from pycamset_amd import pose_seeding, synthetic
    from tests import twoview_inputs as ti

    rig = ti.chain_rig(0.0)
    seed = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, consensus=ti.SCENE_HYPOTHESES)
    known = rig["points"].copy()
    known[::2] = np.nan                                            # every other key surveyed
    out = pose_seeding.align_scene(seed, known)
    size = float(np.linalg.norm(rig["points"].max(axis=0) - rig["points"].min(axis=0)))
    e_pts = float(np.max(np.abs(out.points - rig["points"]))) / size
    centres = np.stack([-ref_rot(out.extr[c, :3]).T @ out.extr[c, 3:] for c in range(5)])
    true_centres = np.stack([-rig["R"][c].T @ rig["t"][c] for c in range(5)])
    e_c = float(np.max(np.abs(centres - true_centres))) / size
    print("scale", out.alignment.scale[0], "point error", e_pts, "centre error", e_c, "bound", MARGIN * ti.SCENE_GAP)
    assert out.frame_cam == -1 and seed.frame_cam == 0 and out.placed.all()
    assert e_pts <= MARGIN * ti.SCENE_GAP and e_c <= MARGIN * ti.SCENE_GAP
    zero = np.zeros((1, 6))
    for c in range(5):
        uv0, _ = synthetic.project_dense(rig["intr"][c:c + 1], seed.extr[c:c + 1], zero, seed.points)
        uv1, _ = synthetic.project_dense(rig["intr"][c:c + 1], out.extr[c:c + 1], zero, out.points)
        assert np.max(np.abs(uv1 - uv0)) <= 1e-9, c
    with pytest.raises(ValueError, match="too few"):
        pose_seeding.align_scene(seed, rig["points"][:2])              # two control points


def test_free_point_handler_takes_control_points():
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests import twoview_inputs as ti
    from tests.test_host_logic import DuckCamset, DuckTarget

    rig = ti.chain_rig(0.0)
    names = [f"cam_{i}" for i in range(5)]
    h = handlers.FreePointBundleHandler(DuckCamset(5), DuckTarget(np.zeros((60, 3))), TargetDetection(names, rig["dct"]), options={"verbosity": 0})
    x0 = h.calc_initial_params(rig["intr"], seeding="scene", scene_opts={"consensus": ti.SCENE_HYPOTHESES, "control_points": rig["points"][:12]})
    size = float(np.linalg.norm(rig["points"].max(axis=0) - rig["points"].min(axis=0)))
    assert h.scene_seed.frame_cam == -1 and np.max(np.abs(x0[-180:].reshape(60, 3) - rig["points"])) <= 64 * MARGIN * ti.SCENE_GAP * size   # 12 control points carry 60: a lever of a few


@pytest.mark.parametrize("scale", ("similarity", "distances"))
def test_apply_gauge_transform_keeps_the_residual_vector(scale):
    """The handler's own residual closure before and after: the change is held to 8 x GAUGE_CLOSURE_GAP, what the restatement causes
    through the oracle's closure (tests/test_align_reference.py); the first pose stays the identity."""
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget

    rig, extr, poses, pts = inp.gauge_state()
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    target = DuckTarget(rig.points_true)
    target.valid_map = np.array([(a, a + 1) for a in range(rig.n_keys - 1) if (a + 1) % 6])
    h = handlers.SelfBundleHandler(DuckCamset(rig.n_cams), target, TargetDetection(names, rig.detections), options={"verbosity": 0})
    loss = h.op_fun.make_full_loss_fn(h._flat_detections(), None)
    r0 = np.array(loss(h.op_fun.build_param_list(rig.intr_true, extr, poses, pts), None)).ravel()
    proj, e2, p2, x2 = h.apply_gauge_transform(rig.intr_true, extr, poses, pts, scale=scale)
    r1 = np.array(loss(h.op_fun.build_param_list(proj, e2, p2, x2), None)).ravel()
    e_r, p_r, x_r, s_r = ref.gauge_transform(extr, poses, pts, rig.points_true, h.visible_feature_mask, scale=scale, pairs=target.valid_map)
    change = float(np.max(np.abs(r1 - r0)))
    print(scale, "change of the residual vector", change, "bound", MARGIN * inp.GAUGE_CLOSURE_GAP, "first pose", p2[0].tolist())
    assert np.max(np.abs(x2 - x_r)) <= 1e-12 and np.max(np.abs(e2 - e_r)) <= 1e-12 and np.max(np.abs(p2 - p_r)) <= 1e-12
    assert np.max(np.abs(p2[0])) <= 1e-14
    assert proj is rig.intr_true
    assert change <= MARGIN * inp.GAUGE_CLOSURE_GAP
    h.op_fun.engine.close()


# ---- the Python front door and the C ABI -----------------------------------------------------------------------------------------------
def test_align_points_shapes_and_the_alignment_object():
    tb = parity_tables()["single"]
    one = ch.align_points(tb["src"], tb["dst"], model="similarity")
    stack = ch.align_points(np.stack([tb["src"][:32], tb["src"][32:64]]), np.stack([tb["dst"][:32], tb["dst"][32:64]]), model="similarity")
    assert one.R.shape == (1, 3, 3) and stack.R.shape == (2, 3, 3) and one.status[0] == ch.ALIGN_OK
    M = one.matrix()[0]
    assert np.allclose(M[:3, :3], one.scale[0] * one.R[0]) and np.allclose(M[:3, 3], one.t[0]) and M[3].tolist() == [0, 0, 0, 1]
    moved = one.apply(tb["src"])
    assert np.allclose(np.linalg.norm(moved - tb["dst"], axis=1), one.distances, rtol=0, atol=1e-12)
    assert stack.apply(np.stack([tb["src"][:32], tb["src"][32:64]])).shape == (2, 32, 3)
    assert ch.last_align_kernel_ms is not None and set(ch.last_align_kernel_ms) == set(ch.ALIGN_STAGES)
    for bad in ({"consensus": 8}, {"consensus": 257, "inlier_dist": 1.0}, {"consensus": 8, "inlier_dist": 0.0}, {"model": "affine"}, {"min_points": 2},
                {"rank_tol": 1.0}, {"group_lanes": 32}, {"weights": -np.ones(65)}):
        with pytest.raises(ValueError):
            ch.align_points(tb["src"], tb["dst"], **bad)


def test_c_abi_refusals():
    lib = _capi.lib()
    assert lib.pcs_version() >= 121
    tb = parity_tables()["single"]
    al = ch.PointAligner()
    try:
        x, y = np.ascontiguousarray(tb["src"]), np.ascontiguousarray(tb["dst"])
        n = x.shape[0]

        def set_points(start, w=None):
            st = np.asarray(start, dtype=np.int64)
            return lib.pcs_align_set_points(al._h, n, al._ptr(x), al._ptr(y), al._ptr(w), st.shape[0] - 1, al._ptr(st))

        assert lib.pcs_align_run(al._h, 0, 3, 1e-10, 0, 0, None, None) == _capi.PCS_ERR_STATE          # no points yet
        assert set_points([0, n]) == _capi.PCS_OK
        for start in ([1, n], [0, n - 1], [0, 40, 30, n]):
            assert set_points(start) == _capi.PCS_ERR_ARG, start
            assert b"start_inds" in lib.pcs_last_error()
        w = np.ones(n)
        w[5] = -1.0
        assert set_points([0, n], w) == _capi.PCS_ERR_ARG and b"weight 5" in lib.pcs_last_error()
        w[5] = np.nan
        assert set_points([0, n], w) == _capi.PCS_ERR_ARG
        assert lib.pcs_align_set_consensus(al._h, 257, 0.1, 0) == _capi.PCS_ERR_RANGE
        assert lib.pcs_align_set_consensus(al._h, -1, 0.1, 0) == _capi.PCS_ERR_RANGE
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.pcs_align_set_consensus(al._h, 8, tau, 0) == _capi.PCS_ERR_ARG, tau
        assert lib.pcs_align_set_consensus(al._h, 16, 0.25, 9) == _capi.PCS_OK and al.get_consensus() == (16, 0.25, 9)
        assert lib.pcs_align_set_consensus(al._h, 300, 0.5, 1) == _capi.PCS_ERR_RANGE and al.get_consensus() == (16, 0.25, 9)   # refused: unchanged
        for args in ((2, 3, 1e-10, 0, 0), (0, 2, 1e-10, 0, 0), (0, 3, -1.0, 0, 0), (0, 3, 1e-10, 32, 0), (0, 3, 1e-10, 0, 1)):
            assert lib.pcs_align_run(al._h, *args, None, None) == _capi.PCS_ERR_ARG, args
        ms = (ctypes.c_float * 4)()
        assert lib.pcs_align_last_kernel_ms(al._h, ms) == _capi.PCS_ERR_STATE                           # the refused calls queued nothing
        assert lib.pcs_align_results(al._h, None, None, None, None, None, None) == _capi.PCS_ERR_STATE
        # the refused tables left the accepted one in force
        al.n_problems, al.n_rows = 1, n
        al.set_consensus(0)
        al.run()
        T = al.results()[0]
        assert np.all(np.isfinite(T))
        assert lib.pcs_align_destroy(None) == _capi.PCS_OK and lib.pcs_align_create(None, 0) == _capi.PCS_ERR_ARG
    finally:
        al.close()


def test_a_caller_buffer_for_T_and_an_empty_table():
    import torch

    tb = parity_tables()["batch"]
    P = tb["start"].shape[0] - 1
    al = ch.PointAligner()
    try:
        al.set_points(tb["src"], tb["dst"], tb["start"])
        al.run()
        T = al.results()[0]
        buf = torch.full((P, 12), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        al.run(d_T=buf.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert buf.cpu().numpy().reshape(P, 3, 4).tobytes() == T.tobytes()
        assert al.results()[0] is None                                                                  # T went to the caller's buffer
        host = np.empty((P, 12))
        assert _capi.lib().pcs_align_results(al._h, al._ptr(host), None, None, None, None, None) == _capi.PCS_ERR_STATE
        al.set_points(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(1, dtype=np.int64))
        al.run()
        assert al.results()[0].shape == (0, 3, 4)
    finally:
        al.close()
