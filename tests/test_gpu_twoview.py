"""The two-view consensus on the device (include/pcs_hip.h pcs_twoview_run, csrc/ba_twoview.hpp) against its NumPy restatement
(tests/twoview_reference.py), at the smallest shapes at which the kernels can go wrong.

The bounds.  ``twoview_reference.rounding`` runs the restatement in float64 and in extended precision on the parity inputs
(tests/twoview_inputs.py parity_inputs: the 3-camera rig of 40 keys with 0.2 px noise at H = 1, 16, 17, and one pair at each of the sizes
8, 15, 16, 17, 33, 64, 65, 257): d_T is the largest gap of an entry of T against max(|entry|, 1), d_s the largest relative gap of a
hypothesis score or a statistic.  Measured (tests/test_twoview_reference.py prints them; profiles/r26/README.md): d_T = 3.4e-13 (the pair
of 8 rows, whose sample is the whole pair), d_s = 2.0e-9 (one hypothesis of the rig).  The device is held to 8 x these, 2.7e-12 for T and
1.6e-8 for scores and statistics: the project's margin for fused multiply-adds and another association inside short sums
(tests/test_gpu_rig_graph.py).  The discrete outputs (info, inlier flags) must be identical, which the tie conditions of
``test_tie_condition_of_every_input`` make a fair demand.  F's sign is free, so hypotheses are compared through the winner's index and score."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as ch
from tests import twoview_inputs as ti
from tests import twoview_reference as tv

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope="module")
def measured():
    """(inputs, rounding of the restatement per input, d_T, d_s): computed once and left unchanged."""
    inputs = ti.parity_inputs()
    rd = tv.rounding(inputs)
    return inputs, rd, max(v[0] for v in rd.values()), max(v[1] for v in rd.values())


def run_device(table, opts, group_lanes=0, stream=None, est=None):
    own = est is None
    est = est or ch.TwoViewEstimator(table["intr"].shape[0])
    try:
        est.set_cameras(table["intr"])
        est.set_correspondences(table["uv_a"], table["uv_b"], table["start"], table["pairs"])
        est.set_consensus(opts["n_hypotheses"], opts["inlier_px"], opts["seed"])
        est.run(min_points=opts["min_points"], group_lanes=group_lanes, stream=stream)
        return est.results()
    finally:
        if own:
            est.close()


def check_against(dev, ref, d_T, d_s, what):
    T, info, stats, inl = dev
    T_r, info_r, stats_r, inl_r = ref[:4]
    g_T, g_s = tv.pose_gap(T, T_r), tv.relative_gap(stats, stats_r)
    print(f"{what}: T gap {g_T:.2e} (bound {MARGIN * d_T:.2e}), stats gap {g_s:.2e} (bound {MARGIN * d_s:.2e}), info {info.tolist()}")
    assert np.array_equal(info, info_r), (what, info.tolist(), info_r.tolist())
    assert np.array_equal(inl, inl_r), what
    assert g_T <= MARGIN * d_T and g_s <= MARGIN * d_s, (what, g_T, g_s)
    ok = info[:, 3] == tv.OK
    assert np.all(np.isfinite(T[ok])) and np.all(np.isnan(T[~ok])) and np.all(np.isnan(stats[~ok, 1:])), what


@pytest.mark.parametrize("H", ti.PARITY_HYPOTHESES)
def test_parity_with_the_restatement(measured, H):
    """The 3-camera rig, 40 keys, 0.2 px noise: info and inlier flags identical, T within 8 x d_T = 2.7e-12, scores and statistics within
    8 x d_s = 1.6e-8 (module docstring)."""
    inputs, rd, d_T, d_s = measured
    table, opts = inputs[f"rig3-H{H}"]
    check_against(run_device(table, opts), rd[f"rig3-H{H}"][2], d_T, d_s, f"rig3-H{H}")


@pytest.mark.parametrize("n", ti.BOUNDARY_N[:-1])
def test_lane_stride_boundaries(measured, n):
    inputs, rd, d_T, d_s = measured
    table, opts = inputs[f"pair-n{n}"]
    check_against(run_device(table, opts), rd[f"pair-n{n}"][2], d_T, d_s, f"pair-n{n}")


@pytest.mark.parametrize("n", (65, 257))
def test_both_group_widths_agree(measured, n):
    """16 and 64 lanes per pair sum in another order: the same discrete outputs, floats within the same bounds."""
    inputs, rd, d_T, d_s = measured
    table, opts = inputs[f"pair-n{n}"]
    for lanes in (16, 64):
        check_against(run_device(table, opts, group_lanes=lanes), rd[f"pair-n{n}"][2], d_T, d_s, f"pair-n{n} lanes {lanes}")


def test_pairs_that_must_not_run(measured):
    """Pairs of 0 and 7 rows around an OK pair: TOO_FEW with NaN T, and the OK pair's bits are those of a table that holds it alone."""
    inputs = measured[0]
    table, opts = inputs["pair-n33"]
    seven = ti.table_of(ti.one_pair(7), 2, 1)
    intr = np.concatenate([table["intr"], table["intr"][:1]])   # cameras 0, 1 and a third for the other pairs
    mixed = {"intr": intr, "pairs": np.array([[0, 2], [0, 1], [1, 2]], dtype=np.int32), "start": np.array([0, 0, 33, 40], dtype=np.int64),
             "uv_a": np.concatenate([table["uv_a"], seven["uv_a"]]), "uv_b": np.concatenate([table["uv_b"], seven["uv_b"]])}
    alone = {**table, "intr": intr}
    # the sampler is keyed by the pair index: the lone table holds an empty pair in front, so that the OK pair keeps index 1
    alone = {**alone, "pairs": np.array([[0, 2], [0, 1]], dtype=np.int32), "start": np.array([0, 0, 33], dtype=np.int64)}
    T, info, stats, inl = run_device(mixed, opts)
    T1, info1, stats1, inl1 = run_device(alone, opts)
    assert info[:, 3].tolist() == [tv.TOO_FEW, tv.OK, tv.TOO_FEW] and info[:, 0].tolist() == [0, 33, 7]
    assert np.all(np.isnan(T[[0, 2]])) and np.all(np.isnan(stats[[0, 2]])) and not inl[33:].any()
    assert info[[0, 2], 1:3].tolist() == [[0, 0], [0, 0]] and info[[0, 2], 4].tolist() == [-1, -1]
    assert T[1].tobytes() == T1[1].tobytes() and stats[1].tobytes() == stats1[1].tobytes()
    assert np.array_equal(info[1], info1[1]) and np.array_equal(inl[:33], inl1)


@pytest.mark.parametrize("which", ("coplanar", "identical"))
def test_degenerate_input(which):
    """Coplanar points and two identical cameras: a status that is not OK, or n_front / parallax as the restatement reports them; never a
    NaN reported as OK."""
    rig = ti.coplanar_pair() if which == "coplanar" else ti.identical_cameras()
    table = ti.table_of(rig, 2, 8)
    opts = {"n_hypotheses": 16, "inlier_px": ti.INLIER_PX, "seed": 0, "min_points": 8}
    T, info, stats, inl = run_device(table, opts)
    T_r, info_r, stats_r, inl_r, _ = tv.run_table(table, opts)
    print(which, info.tolist(), stats.tolist(), "restatement", info_r.tolist(), stats_r.tolist())
    ok = info[:, 3] == tv.OK
    assert np.all(np.isfinite(T[ok])) and np.all(np.isfinite(stats[ok])) and np.all(np.isnan(T[~ok]))
    if ok[0]:   # accepted: then as the restatement accepts it
        assert info_r[0, 3] == tv.OK and info[0, 2] == info_r[0, 2]
        assert abs(stats[0, 2] - stats_r[0, 2]) <= 1e-6 * max(1.0, stats_r[0, 2])


def test_repeatability(measured):
    """Two runs of the same table, and a run on a caller stream, return identical bytes in every output."""
    import torch

    table, opts = measured[0]["rig3-H16"]
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


def test_outliers():
    """30 % of a pair's rows replaced by random pixels: the inliers are the restatement's and exactly the unmoved rows, and the pose is that
    of the clean table (bound: tests/test_twoview_reference.py test_consensus_returns_the_unmoved_rows)."""
    rig, uv_a, uv_b, bad, moved = ti.outlier_pair()
    opts = {"n_hypotheses": 64, "inlier_px": ti.INLIER_PX, "seed": 0, "min_points": 16}
    table = {"intr": rig["intr"], "pairs": np.array([[0, 1]], dtype=np.int32), "start": np.array([0, uv_a.shape[0]], dtype=np.int64), "uv_a": uv_a, "uv_b": bad}
    T, info, stats, inl = run_device(table, opts)
    _, info_r, _, inl_r, _ = tv.run_table(table, opts)
    assert info[0, 3] == tv.OK and np.array_equal(inl, inl_r) and np.array_equal(inl, ~moved) and np.array_equal(info, info_r)
    R, t = ti.relative_pose(rig, 0, 1)
    assert np.abs(T[0, :, :3] - R).max() <= ti.CLEAN_POSE_BOUND and np.abs(T[0, :, 3] - t).max() <= ti.CLEAN_POSE_BOUND


def test_entry_point_builds_the_table_from_detections(measured):
    """``estimate_two_view`` on the flat table: the pairs, rows and results of the handle on the restatement's table."""
    table, opts = measured[0]["rig3-H16"]
    res = ch.estimate_two_view(ti.parity_rig()["dct"], table["intr"], consensus=16, inlier_px=ti.INLIER_PX, seed=0, min_points=16)
    T, info, stats, inl = run_device(table, opts)
    assert np.array_equal(res.pairs, table["pairs"]) and np.array_equal(res.start, table["start"])
    assert np.array_equal(res.uv_a, table["uv_a"]) and np.array_equal(res.uv_b, table["uv_b"])
    assert res.T.tobytes() == T.tobytes() and np.array_equal(res.status, info[:, 3]) and np.array_equal(res.inliers, inl)
    assert np.array_equal(res.parallax, stats[:, 2], equal_nan=True)


def test_refusals_leave_the_handle_usable(measured):
    """Every argument error is raised without touching the device, and afterwards the handle still runs a good table."""
    table, opts = measured[0]["pair-n33"]
    good = (table["uv_a"], table["uv_b"], table["start"], table["pairs"])
    est = ch.TwoViewEstimator(2)
    try:
        before = run_device(table, opts, est=est)

        def refused(code, *args):
            with pytest.raises(_capi.PcsError) as e:
                est.set_correspondences(*args)
            assert e.value.code == code, e.value

        refused(_capi.PCS_ERR_RANGE, good[0], good[1], good[2], np.array([[0, 2]]))
        refused(_capi.PCS_ERR_ARG, good[0], good[1], good[2], np.array([[1, 0]]))
        refused(_capi.PCS_ERR_ARG, good[0], good[1], good[2], np.array([[1, 1]]))
        refused(_capi.PCS_ERR_ARG, np.concatenate([good[0]] * 2), np.concatenate([good[1]] * 2), np.array([0, 40, 33, 66]), np.array([[0, 1]] * 3))
        refused(_capi.PCS_ERR_ARG, good[0], good[1], np.array([1, 33]), good[3])
        for bad in (np.nan, np.inf):
            uv = good[1].copy()
            uv[5, 1] = bad
            refused(_capi.PCS_ERR_ARG, good[0], uv, good[2], good[3])
            refused(_capi.PCS_ERR_ARG, uv, good[1], good[2], good[3])
        lib = _capi.lib()
        for H in (0, 257, -1):
            assert lib.pcs_twoview_set_consensus(est._h, H, 2.0, 0) == _capi.PCS_ERR_RANGE
        for px in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.pcs_twoview_set_consensus(est._h, 16, px, 0) == _capi.PCS_ERR_ARG
        assert est.get_consensus() == (opts["n_hypotheses"], opts["inlier_px"], opts["seed"])
        assert lib.pcs_twoview_run(est._h, 0, 0, 0, None, None) == _capi.PCS_ERR_ARG
        assert lib.pcs_twoview_run(est._h, 8, 32, 0, None, None) == _capi.PCS_ERR_ARG
        assert lib.pcs_twoview_run(est._h, 8, 0, 1, None, None) == _capi.PCS_ERR_ARG
        h = ctypes.c_void_p()
        assert lib.pcs_twoview_create(ctypes.byref(h), 0, 1) == _capi.PCS_ERR_ARG
        # the refused tables left the good one in place
        est.run(min_points=opts["min_points"])
        for a, b in zip(before, est.results()):
            assert a.tobytes() == b.tobytes()
        dct = ti.parity_rig()["dct"]
        intr = ti.parity_rig()["intr"]
        for kw in ({"consensus": 0}, {"consensus": 257}, {"inlier_px": 0.0}, {"inlier_px": float("nan")}, {"seed": -1}, {"min_points": 0},
                   {"pairs": np.array([[1, 0]])}, {"pairs": np.array([[0, 3]])}, {"group_lanes": 32}):
            with pytest.raises(ValueError):
                ch.estimate_two_view(dct, intr, **kw)
        bad = dct.copy()
        bad[3, 4] = np.nan
        with pytest.raises(ValueError):
            ch.estimate_two_view(bad, intr)
    finally:
        est.close()


# ---- end to end: a seed for target-free bundle adjustment ------------------------------------------------------------------------------
def test_scene_seed_places_every_camera_of_the_chain_rig():
    """5 cameras, 60 keys, camera i shares keys only with i +- 1 and i +- 2, noise-free: every camera is placed, in the rounds of the
    restatement, and after a similarity alignment extrinsics and points agree with truth within 8 x SCENE_GAP = 4.5e-11 (SCENE_GAP: what
    the restatement pipeline reaches on this input, tests/test_twoview_reference.py)."""
    from pycamset_amd import pose_seeding

    rig = ti.chain_rig(0.0)
    ref = tv.seed_scene(rig["dct"], rig["intr"], 5, n_hypotheses=ti.SCENE_HYPOTHESES)
    got = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, consensus=ti.SCENE_HYPOTHESES)
    gap = tv.scene_gap(got.extr, got.points, rig)
    print("first pair", got.first_pair, "rounds", got.round_of_camera.tolist(), "gap", gap, "bound", MARGIN * ti.SCENE_GAP)
    assert got.placed.all() and got.first_pair == ref["first_pair"] and np.array_equal(got.round_of_camera, ref["round_of_camera"])
    assert got.round_of_camera.max() == 2 and np.all(np.isfinite(got.points)) and got.extr[0].tolist() == [0.0] * 6
    assert max(gap) <= MARGIN * ti.SCENE_GAP


def test_free_point_solve_from_the_scene_seed():
    """0.3 px noise: the device LM solve of the free chain started from ``calc_initial_params(seeding="scene")`` and the same solve started
    from the truth perturbed by 1 % end at costs that agree within 10 x the ftol given to both."""
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from pycamset_amd.device_solver import lm_solve
    from tests.test_host_logic import DuckCamset, DuckTarget

    rig = ti.chain_rig(0.3)
    extr_true, pts_true = ti.in_camera_frame(rig, 0)
    names = [f"cam_{i}" for i in range(5)]
    fixed = {n: {"int": rig["intr"][i].copy()} for i, n in enumerate(names)}
    fixed["cam_0"]["ext"] = np.zeros(6)
    ftol = 1e-9
    costs = []
    for start in ("scene", "truth"):
        h = handlers.FreePointBundleHandler(DuckCamset(5), DuckTarget(np.zeros((60, 3))), TargetDetection(names, rig["dct"]), fixed_params=fixed,
                                            options={"verbosity": 0})
        bp = h.bundlePrimitive
        if start == "scene":
            x0 = h.calc_initial_params(rig["intr"], seeding="scene", scene_opts={"consensus": ti.SCENE_HYPOTHESES})
            assert h.scene_seed.placed.all()
        else:
            rng = np.random.default_rng(7)
            x0 = np.concatenate([rig["intr"][bp.intr_unfixed].ravel(), extr_true[bp.extr_unfixed].ravel(), pts_true.ravel()[bp.bdpt_unfixed]])
            x0 = x0 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, x0.shape))
        assert x0.shape == (24 + 180,) and np.all(np.isfinite(x0))
        res = lm_solve(h, x0.copy(), max_iter=200, ftol=ftol, xtol=1e-15, gtol=1e-15)
        print(start, "cost", res.cost, "start cost", res.history[0], "nfev", res.nfev, res.message)
        costs.append(res.cost)
        h.op_fun.engine.close()
    rms = np.sqrt(costs[0] / rig["dct"].shape[0])
    assert rms < 0.5, rms   # back at the 0.3 px measurement noise
    assert abs(costs[0] - costs[1]) <= 10.0 * ftol * max(costs), costs


def test_scene_seeding_names_what_it_could_not_seed():
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget

    rig = ti.chain_rig(0.0)
    d = rig["dct"]
    d = d[~((d[:, 0] == 4) & (d[:, 2] >= 30))]     # camera 4 keeps 10 keys: fewer than min_points
    names = [f"cam_{i}" for i in range(5)]
    h = handlers.FreePointBundleHandler(DuckCamset(5), DuckTarget(np.zeros((60, 3))), TargetDetection(names, d), options={"verbosity": 0})
    with pytest.raises(ValueError, match="cam_4"):
        h.calc_initial_params(rig["intr"], seeding="scene", scene_opts={"consensus": ti.SCENE_HYPOTHESES})
    with pytest.raises(ValueError):
        h.calc_initial_params(rig["intr"], seeding="reference", scene_opts={})
