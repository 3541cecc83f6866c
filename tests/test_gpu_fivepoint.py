"""The five-point solver and the pose refinement of the two-view consensus on the device (include/pcs_hip.h pcs_twoview_set_solver,
csrc/ba_fivepoint.hpp) against their NumPy restatement (tests/fivepoint_reference.py), at the smallest shapes at which the kernels can go
wrong.

The bounds.  tests/test_fivepoint_reference.py runs the restatement in float64 and in extended precision on the parity inputs
(tests/fivepoint_inputs.py parity_inputs: the 3-camera rig of 40 keys with 0.2 px noise at H = 1, 16, 17, and one pair at each of the
sizes 5, 6, 15, 16, 17, 33, 64, 65, 257, at 0 and at 10 refinement trials) and pins what it measures as fivepoint_inputs.D_T = 2.1e-10
(largest gap of an entry of T against max(|entry|, 1)) and D_S = 1.2e-7 (largest gap of a hypothesis' best score or of a statistic against
max(|entry|, 1e-12 px^2)).  The device is held to 8 x these, 1.7e-9 for T and 9.6e-7 for scores and statistics: the project's margin for
fused multiply-adds and another association inside short sums (tests/test_gpu_twoview.py).  The discrete outputs (info, inlier flags) must be
identical, which the tie conditions of the CPU file make a fair demand.  The root index of a winner is no output: the basis of the null
space is fixed by rounding noise, so the order of a hypothesis' roots may differ while its essential matrices agree."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as ch
from tests import fivepoint_inputs as fi
from tests import fivepoint_reference as fp
from tests import twoview_inputs as ti
from tests import twoview_reference as tv

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope="module")
def restated():
    """refine_iters -> (inputs, name -> float64 result of the restatement): computed once and left unchanged."""
    out = {}
    for refine in (0, 10):
        inputs = fi.parity_inputs(refine)
        out[refine] = (inputs, {name: fp.run_table(table, opts) for name, (table, opts) in inputs.items()})
    return out


def run_device(table, opts, group_lanes=0, stream=None, est=None, set_solver=True):
    own = est is None
    est = est or ch.TwoViewEstimator(table["intr"].shape[0])
    try:
        est.set_cameras(table["intr"])
        est.set_correspondences(table["uv_a"], table["uv_b"], table["start"], table["pairs"])
        est.set_consensus(opts["n_hypotheses"], opts["inlier_px"], opts["seed"])
        if set_solver:
            est.set_solver(opts.get("solver", "eight-point"), opts.get("refine_iters", 0))
        est.run(min_points=opts["min_points"], group_lanes=group_lanes, stream=stream)
        return est.results()
    finally:
        if own:
            est.close()


def check_against(dev, ref, what):
    T, info, stats, inl = dev
    T_r, info_r, stats_r, inl_r = ref[:4]
    g_T, g_s = tv.pose_gap(T, T_r), fp.stats_gap(stats, stats_r)
    print(f"{what}: T gap {g_T:.2e} (bound {MARGIN * fi.D_T:.2e}), stats gap {g_s:.2e} (bound {MARGIN * fi.D_S:.2e}), info {info.tolist()}")
    assert np.array_equal(info, info_r), (what, info.tolist(), info_r.tolist())
    assert np.array_equal(inl, inl_r), what
    assert g_T <= MARGIN * fi.D_T and g_s <= MARGIN * fi.D_S, (what, g_T, g_s)
    ok = info[:, 3] == fp.OK
    assert np.all(np.isfinite(T[ok])) and np.all(np.isnan(T[~ok])) and np.all(np.isnan(stats[~ok, 1:])), what


@pytest.mark.parametrize("refine", (0, 10))
@pytest.mark.parametrize("H", fi.PARITY_HYPOTHESES)
def test_parity_with_the_restatement(restated, H, refine):
    """The 3-camera rig, 40 keys, 0.2 px noise: info and inlier flags identical, T within 8 x D_T, scores and statistics within 8 x D_S."""
    inputs, ref = restated[refine]
    table, opts = inputs[f"rig3-H{H}"]
    check_against(run_device(table, opts), ref[f"rig3-H{H}"], f"rig3-H{H} refine {refine}")


@pytest.mark.parametrize("refine", (0, 10))
@pytest.mark.parametrize("n", fi.BOUNDARY_N)
def test_lane_stride_boundaries(restated, n, refine):
    """One pair of n rows: the sample is the whole pair (5: DEGENERATE, five rows fit every root), one row more, around the lane stride,
    around a wave, past 256."""
    inputs, ref = restated[refine]
    table, opts = inputs[f"pair-n{n}"]
    check_against(run_device(table, opts), ref[f"pair-n{n}"], f"pair-n{n} refine {refine}")


@pytest.mark.parametrize("n", (65, 257))
def test_both_group_widths_agree(restated, n):
    """16 and 64 lanes per pair sum in another order: the same discrete outputs, floats within the same bounds."""
    inputs, ref = restated[10]
    table, opts = inputs[f"pair-n{n}"]
    for lanes in (16, 64):
        check_against(run_device(table, opts, group_lanes=lanes), ref[f"pair-n{n}"], f"pair-n{n} lanes {lanes}")


@pytest.mark.parametrize("scene", sorted(fi.CAPABILITY_SCENES))
def test_planar_scenes_are_recovered(scene):
    """planar_rig(40, 0, 0.2, seed) / planar_rig(48, 12, 0.2, seed), seeds 0 .. 7 (none left out), H = 16, tau = 2 px, 10 refinement
    trials, one table per seed as in the CPU file: every pair OK with all but at most 2 rows as inliers, rotation and translation direction
    within 2 x CAPABILITY_POSE_ERROR = 1.04e-2 rad of truth.  (The eight-point path is not OK or more than 0.1 rad off on 8 of the 8 planar
    seeds, tests/test_fivepoint_reference.py.)"""
    est = ch.TwoViewEstimator(2)
    try:
        for seed in fi.CAPABILITY_SEEDS:
            rig, table = fi.capability_table(scene, 0.2, seed)
            T, info, stats, inl = run_device(table, fi.CAPABILITY_OPTS, est=est)
            R, t = ti.relative_pose(rig, 0, 1)
            n = int(info[0, 0])
            err = fp.pose_error(T[0], R, t) if info[0, 3] == fp.OK else (np.inf, np.inf)
            print(f"{scene} seed {seed}: info {info[0].tolist()} rms {stats[0, 1]:.3f} px, error {err[0]:.2e} / {err[1]:.2e} rad")
            assert info[0, 3] == fp.OK and info[0, 1] >= n - 2, (scene, seed, info[0].tolist())
            assert max(err) <= 2.0 * fi.CAPABILITY_POSE_ERROR, (scene, seed, err)
    finally:
        est.close()


def test_eight_point_with_refinement(restated):
    """arc_rig(2, 40, 0.2, seed=11), eight-point hypotheses and refit, then 10 refinement trials: parity with the restatement, and an RMS
    Sampson distance not above the unrefined run's (restatement: 0.365 -> 0.130 px)."""
    table, opts = fi.eight_point_refined_input()
    dev = run_device(table, opts)
    check_against(dev, fp.run_table(table, opts), "eight-point refined")
    plain = run_device(table, {**opts, "refine_iters": 0})
    print("rms", plain[2][0, 1], "->", dev[2][0, 1])
    assert dev[1][0, 3] == fp.OK and dev[2][0, 1] <= plain[2][0, 1] and np.array_equal(dev[3], plain[3])


def test_pairs_that_must_not_run(restated):
    """Pairs of 0 and 4 rows around an OK pair: TOO_FEW with NaN T, and the OK pair's bytes are those of a table that holds it alone."""
    inputs = restated[10][0]
    table, opts = inputs["pair-n33"]
    four = ti.table_of(ti.one_pair(4), 2, 1)
    intr = np.concatenate([table["intr"], table["intr"][:1]])   # cameras 0, 1 and a third for the other pairs
    mixed = {"intr": intr, "pairs": np.array([[0, 2], [0, 1], [1, 2]], dtype=np.int32), "start": np.array([0, 0, 33, 37], dtype=np.int64),
             "uv_a": np.concatenate([table["uv_a"], four["uv_a"]]), "uv_b": np.concatenate([table["uv_b"], four["uv_b"]])}
    # the sampler is keyed by the pair index: the lone table holds an empty pair in front, so that the OK pair keeps index 1
    alone = {**table, "intr": intr, "pairs": np.array([[0, 2], [0, 1]], dtype=np.int32), "start": np.array([0, 0, 33], dtype=np.int64)}
    T, info, stats, inl = run_device(mixed, opts)
    T1, info1, stats1, inl1 = run_device(alone, opts)
    assert info[:, 3].tolist() == [fp.TOO_FEW, fp.OK, fp.TOO_FEW] and info[:, 0].tolist() == [0, 33, 4]
    assert np.all(np.isnan(T[[0, 2]])) and np.all(np.isnan(stats[[0, 2]])) and not inl[33:].any()
    assert info[[0, 2], 1:3].tolist() == [[0, 0], [0, 0]] and info[[0, 2], 4].tolist() == [-1, -1]
    assert T[1].tobytes() == T1[1].tobytes() and stats[1].tobytes() == stats1[1].tobytes()
    assert np.array_equal(info[1], info1[1]) and np.array_equal(inl[:33], inl1)


def test_repeatability(restated):
    """Two runs of the same table, and a run on a caller stream, return identical bytes in every output."""
    import torch

    table, opts = restated[10][0]["rig3-H16"]
    est = ch.TwoViewEstimator(3)
    try:
        first = run_device(table, opts, est=est)
        second = run_device(table, opts, est=est)
        s = torch.cuda.Stream()
        third = run_device(table, opts, est=est, stream=s.cuda_stream)
        s.synchronize()
        for other in (second, third):
            for a, b in zip(first, other):
                assert a.tobytes() == b.tobytes()
        ms = est.last_kernel_ms()
        assert set(ms) == set(ch.TWOVIEW_STAGES) and all(v >= 0.0 for v in ms.values())
    finally:
        est.close()


def test_defaults_are_untouched():
    """A handle on which set_solver was never called and one set to ("eight-point", 0) return the same bytes."""
    table, opts = ti.parity_inputs()["rig3-H16"]
    never = run_device(table, opts, set_solver=False)
    stated = run_device(table, {**opts, "solver": "eight-point", "refine_iters": 0})
    for a, b in zip(never, stated):
        assert a.tobytes() == b.tobytes()
    est = ch.TwoViewEstimator(2)
    try:
        assert est.get_solver() == ("eight-point", 0)
    finally:
        est.close()


def test_refusals_leave_the_handle_usable(restated):
    """An unknown solver, refine_iters of -1 and 51 and a NULL handle are refused, keep the previous setting and leave the handle usable."""
    table, opts = restated[10][0]["pair-n33"]
    est = ch.TwoViewEstimator(2)
    try:
        before = run_device(table, opts, est=est)
        lib = _capi.lib()
        assert lib.pcs_twoview_set_solver(est._h, 2, 0) == _capi.PCS_ERR_ARG
        assert lib.pcs_twoview_set_solver(est._h, -1, 0) == _capi.PCS_ERR_ARG
        assert lib.pcs_twoview_set_solver(est._h, _capi.TWOVIEW_FIVE_POINT, -1) == _capi.PCS_ERR_RANGE
        assert lib.pcs_twoview_set_solver(est._h, _capi.TWOVIEW_EIGHT_POINT, 51) == _capi.PCS_ERR_RANGE
        assert lib.pcs_twoview_set_solver(None, _capi.TWOVIEW_FIVE_POINT, 0) == _capi.PCS_ERR_ARG
        assert lib.pcs_twoview_get_solver(None, None, None) == _capi.PCS_ERR_ARG
        solver, iters = ctypes.c_int(-7), ctypes.c_int(-7)
        assert lib.pcs_twoview_get_solver(est._h, ctypes.byref(solver), None) == _capi.PCS_OK and solver.value == _capi.TWOVIEW_FIVE_POINT
        assert lib.pcs_twoview_get_solver(est._h, None, ctypes.byref(iters)) == _capi.PCS_OK and iters.value == 10
        assert est.get_solver() == ("five-point", 10)
        for bad in (("seven-point", 0), ("five-point", 51), ("five-point", -1)):
            with pytest.raises(ValueError):
                est.set_solver(*bad)
        est.run(min_points=opts["min_points"])
        for a, b in zip(before, est.results()):
            assert a.tobytes() == b.tobytes()
        dct, intr = ti.parity_rig()["dct"], ti.parity_rig()["intr"]
        for kw in ({"solver": "5pt"}, {"refine_iters": 51}, {"refine_iters": -1}, {"refine_iters": 2.5}):
            with pytest.raises(ValueError):
                ch.estimate_two_view(dct, intr, **kw)
        assert lib.pcs_version() >= 120
    finally:
        est.close()


def test_outliers_on_a_plane():
    """planar_rig(60, 0, 0.0, 3) with 30 % of camera b's pixels replaced by random ones: no moved row is an inlier, every unmoved one is,
    and the pose is within the clean bound (fivepoint_inputs.clean_pose_bound of the fixture's undistortion residual).  Without noise
    every sample of five unmoved rows gives the true pose and a score of 18 tau^2 plus rounding, so the winning hypothesis is not
    compared: any of them has these flags and this pose."""
    rig, uv_a, uv_b, bad, moved = fi.planar_outlier_pair()
    opts = {"n_hypotheses": 64, "inlier_px": fi.INLIER_PX, "seed": 0, "min_points": 16, "solver": "five-point", "refine_iters": 10}
    table = {"intr": rig["intr"], "pairs": np.array([[0, 1]], dtype=np.int32), "start": np.array([0, uv_a.shape[0]], dtype=np.int64), "uv_a": uv_a, "uv_b": bad}
    T, info, stats, inl = run_device(table, opts)
    R, t = ti.relative_pose(rig, 0, 1)
    err, bound = max(np.abs(T[0, :, :3] - R).max(), np.abs(T[0, :, 3] - t).max()), fi.clean_pose_bound(fi.undistortion_residual(rig))
    print("info", info.tolist(), "pose error", err, "bound", bound)
    assert info[0, 3] == fp.OK and not (inl & moved).any() and np.array_equal(inl, ~moved) and info[0, :3].tolist() == [60, 42, 42]
    assert err <= bound


def test_entry_point_passes_the_solver_through(restated):
    """``estimate_two_view(solver=, refine_iters=)`` returns the handle's results on the same table."""
    table, opts = restated[10][0]["rig3-H16"]
    res = ch.estimate_two_view(ti.parity_rig()["dct"], table["intr"], consensus=16, inlier_px=fi.INLIER_PX, seed=0, min_points=16, solver="five-point",
                               refine_iters=10)
    T, info, stats, inl = run_device(table, opts)
    assert res.T.tobytes() == T.tobytes() and np.array_equal(res.status, info[:, 3]) and np.array_equal(res.inliers, inl)
    plain = ch.estimate_two_view(ti.parity_rig()["dct"], table["intr"], consensus=16, inlier_px=fi.INLIER_PX, seed=0, min_points=16)
    T8 = run_device(*ti.parity_inputs()["rig3-H16"], set_solver=False)[0]
    assert plain.T.tobytes() == T8.tobytes()   # the shared handle went back to the defaults


def test_scene_seed_on_a_mostly_planar_chain():
    """planar_chain_rig(0.0): 5 cameras, 60 keys, 80 % of them on the facing plane, camera i shares keys only with i +- 1 and i +- 2.
    ``seed_scene(two_view_solver="five-point", two_view_refine=10)`` places every camera, and after a similarity alignment extrinsics and
    points agree with truth within 8 x fivepoint_inputs.SCENE_GAP = 3.4e-12 (SCENE_GAP: what the restatement pipeline reaches on this
    input, tests/test_fivepoint_reference.py)."""
    from pycamset_amd import pose_seeding

    rig = fi.planar_chain_rig(0.0)
    got = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, consensus=ti.SCENE_HYPOTHESES, two_view_solver="five-point", two_view_refine=10)
    gap = tv.scene_gap(got.extr, got.points, rig)
    print("first pair", got.first_pair, "rounds", got.round_of_camera.tolist(), "gap", gap, "bound", MARGIN * fi.SCENE_GAP)
    assert got.placed.all() and np.all(np.isfinite(got.points)) and got.extr[0].tolist() == [0.0] * 6
    assert np.all(got.two_view.status == ch.TWOVIEW_OK)
    assert max(gap) <= MARGIN * fi.SCENE_GAP


def test_calc_initial_params_passes_the_solver_through():
    """``FreePointBundleHandler.calc_initial_params(seeding="scene", scene_opts={"two_view_solver": ..., "two_view_refine": ...})`` reaches
    ``seed_scene``: the seed kept on the handler is that of the direct call, and an unknown solver is refused."""
    from pycamset_amd import handlers, pose_seeding
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget

    rig = fi.planar_chain_rig(0.0)
    names = [f"cam_{i}" for i in range(5)]
    h = handlers.FreePointBundleHandler(DuckCamset(5), DuckTarget(np.zeros((60, 3))), TargetDetection(names, rig["dct"]), options={"verbosity": 0})
    opts = {"consensus": ti.SCENE_HYPOTHESES, "two_view_solver": "five-point", "two_view_refine": 10}
    x0 = h.calc_initial_params(rig["intr"], seeding="scene", scene_opts=opts)
    direct = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, **opts)
    assert np.all(np.isfinite(x0)) and h.scene_seed.placed.all()
    assert h.scene_seed.extr.tobytes() == direct.extr.tobytes() and h.scene_seed.two_view.T.tobytes() == direct.two_view.T.tobytes()
    with pytest.raises(ValueError):
        h.calc_initial_params(rig["intr"], seeding="scene", scene_opts={"two_view_solver": "six-point"})
