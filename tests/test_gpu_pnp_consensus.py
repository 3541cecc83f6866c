"""Consensus sampling in front of the batched target-pose estimation on the GPU (include/pcs_hip.h pcs_pnp_set_consensus,
csrc/ba_pnp_consensus.hpp) against the plain run and against its NumPy restatement (tests/pnp_consensus_reference.py, itself checked
on the CPU in tests/test_pnp_consensus_reference.py).

Tolerances.  Start and LM behind the stage are the unchanged kernels on the compacted table, so wherever the inlier set is known the
outputs are compared BITWISE with a plain run on those rows.  The winner's score is a sum of n <= 54 squared pixel errors of a pose that
the device and NumPy compute with different rounding (reciprocals, summation order: 1e-6 relative in the start, the figure of
tests/test_gpu_pnp.py, damped by the score's flatness near its minimum); the issue sets 1e-9 relative, which is asserted."""
import functools

import numpy as np
import pytest

from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import pnp_consensus_inputs as inp
from tests import pnp_consensus_reference as cons_ref
from tests import pnp_reference as ref
from tests.intr_consensus_inputs import move_rows
from tests.test_pnp_consensus_reference import restated
from tests.test_pnp_reference import CUBE, DuckCamset, DuckTarget, assert_poses_close, pose_error, true_view_poses, truth_rig

pytestmark = pytest.mark.gpu

CONS = dict(consensus=64, sample_size=6, inlier_px=8.0, seed=0)
BITS = ("poses", "poses_init", "poses_alt", "rms", "rms_init", "status", "iterations")


def assert_same_bits(a, b, fields=BITS, where=None):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        if where is not None:
            x, y = x[where], y[where]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name


def per_view_counts(det, mask, C, I):
    out = np.zeros((C, I), dtype=np.int64)
    np.add.at(out, (det[mask, 0].astype(int), det[mask, 1].astype(int)), 1)
    return out


@pytest.mark.parametrize("kind", inp.KINDS)
def test_clean_table_gives_the_plain_bits(kind):
    """No outliers: every detection is an inlier, the compacted table is the table, and every output is bitwise the plain run's."""
    rig, det = truth_rig(kind, noise_px=0.3, seed=21)
    plain = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3)
    got = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3, **CONS)
    assert plain.inliers is None and plain.n_inliers is None and plain.hypothesis is None
    assert_same_bits(got, plain, BITS + ("n_points",))
    assert got.inliers.dtype == bool and got.inliers.shape == (det.shape[0],) and got.inliers.all()
    assert np.array_equal(got.n_inliers, plain.n_points) and np.all((got.hypothesis >= 0) & (got.hypothesis < 64))
    assert np.all(got.status != hip_ch.PNP_NOT_ESTIMATED)


@pytest.mark.parametrize("kind", inp.KINDS)
def test_corrupted_table_gives_the_bits_of_the_clean_rows(kind):
    """15 % of every view moved by 30 to 200 px: the plain run is wrong, the consensus run finds exactly the rows that were not moved and
    returns, bit for bit, the plain run on those rows."""
    rig, det, clean = inp.corrupted_rig(kind)
    T = true_view_poses(rig)
    plain = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3)
    worst = max(np.inf if not np.all(np.isfinite(plain.poses[c, i])) else pose_error(plain.poses[c, i], T[c, i])[0] for c in range(3) for i in range(3))
    print(f"{kind}: worst pose error of the plain run on the corrupted table {worst:.3f} rad")
    assert worst > 0.1   # the input exercises the feature
    got = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3, **CONS)
    want = hip_ch.estimate_view_poses(det[clean], rig.points, rig.intr_true, n_imgs=3)
    assert np.array_equal(got.inliers, clean)
    assert_same_bits(got, want)
    assert np.array_equal(got.n_inliers, want.n_points) and np.array_equal(got.n_points, per_view_counts(det, np.ones_like(clean), 3, 3))
    assert np.all(got.status != hip_ch.PNP_NOT_ESTIMATED) and np.all(got.rms < 1.0)   # 0.3 px of noise on the rows that are left


@pytest.mark.parametrize("kind", inp.KINDS)
def test_parity_with_the_restatement(kind):
    """Per view: the winning hypothesis, the inlier count, the flags, and the winner's score to 1e-9 relative.  A view may be left out of
    the index comparison only where the restatement's best two scores are within 1e-9 relative, at most one per rig; with the inputs
    chosen none is (tests/test_pnp_consensus_reference.py::test_corruption_seed_needs_no_exception)."""
    rig, det, clean, res = restated(kind)
    order, ids, start = hip_ch.group_by_view(det, 3)
    ds = det if order is None else det[order]
    est = hip_ch.PoseEstimator(3, rig.points.shape[0])
    est.set_cameras(rig.intr_true)
    est.set_template(rig.points)
    est.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (ids // 3).astype(np.int32))
    est.set_consensus(64, 6, 8.0, 0)
    assert est.get_consensus() == (64, 6, 8.0, 0)
    est.run()
    pose, init, alt = est.results()[:3]
    flags, cinfo, score = est.consensus_results()
    est.close()
    left_out = 0
    for k, v in enumerate(ids):
        rows, r = res[(int(v) // 3, int(v) % 3)]
        s = np.sort(r["scores"].ravel())
        tie = s[1] - s[0] <= 1e-9 * s[0]
        left_out += int(tie)
        print(f"view {int(v)}: hypothesis {cinfo[k, 1]} / {r['hypothesis']}, inliers {cinfo[k, 0]} / {r['n_inliers']}, "
              f"score {score[k]:.12e} / {r['score']:.12e} (rel {abs(score[k] - r['score']) / r['score']:.1e}), finite {cinfo[k, 2]} / {r['n_finite']}")
        if not tie:
            assert cinfo[k, 1] == r["hypothesis"]
        # the number of finite hypotheses is printed, not compared: whether a nearly degenerate sample passes the pivot and determinant
        # tests of the linear start is decided by the sign of a rounding error (measured: 42 against 43 in one view of the cube rig)
        assert cinfo[k, 0] == r["n_inliers"] and cinfo[k, 3] == 1 and 1 <= cinfo[k, 2] <= 64
        mine = np.zeros(det.shape[0], dtype=bool)
        mine[order[start[k]:start[k + 1]] if order is not None else np.arange(start[k], start[k + 1])] = flags[start[k]:start[k + 1]]
        assert np.array_equal(mine[rows], r["inliers"])
        assert abs(score[k] - r["score"]) <= 1e-9 * r["score"]
        view = ds[start[k]:start[k + 1]][flags[start[k]:start[k + 1]]]
        again = ref.solve_view(view[:, 2].astype(int), view[:, 3:5], rig.intr_true[int(v) // 3], rig.points, start=init[k], alt=alt[k])
        ang, dt = pose_error(pose[k], again["pose"])
        assert ang <= 1e-9 and dt <= 1e-9, (k, ang, dt)   # the restatement's LM from the device's starts on the inliers: the figure of tests/test_gpu_pnp.py
    assert left_out <= 1


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
BOARD = synthetic.charuco_points(18)                                       # 17 x 17 corners: a view of 289 observations
LINE = np.stack([np.arange(8) * 0.01, np.zeros(8), np.zeros(8)], axis=1)   # exactly collinear: centroid and scatter are exact
TEMPLATE = np.concatenate([CUBE, BOARD, LINE])
SIZES = {0: 5, 1: 6, 2: 13, 3: 16, 4: 65}
DENSE_IM, LINE_IM, NAN_IM = 5, 6, 7


def shapes_table():
    """One camera, 17 images of the cube (0.3 px noise): views of 5, exactly 6 (the sample), 13, 16 and 65 observations, one view of the
    dense board (289), one of 8 collinear points (no finite hypothesis), full views of 96; 10 % of the 65-point view, of the board
    view and of image 8 moved by 30 to 200 px.  -> (table, clean mask, intrinsics)."""
    rig = synthetic.make_rig("pnp-shapes", 1, 17, CUBE, seed=33, noise_px=0.3)
    dense = synthetic.make_rig("pnp-shapes", 1, 17, BOARD, seed=33, noise_px=0.3)   # the same seed: the same camera and poses
    assert np.array_equal(rig.intr_true, dense.intr_true)
    det = rig.detections
    rng = np.random.default_rng(5)
    keep = (det[:, 1] != DENSE_IM) & (det[:, 1] != LINE_IM)
    for im, n in SIZES.items():
        rows = np.nonzero(det[:, 1] == im)[0]
        if n == 6:   # the view of exactly one sample lies on one face of the cube: a homography of six points, which fits them all
            keep[rows[det[rows, 2] >= 16]] = False
            rows = rows[det[rows, 2] < 16]
        keep[rng.permutation(rows)[n:]] = False
    board = dense.detections[dense.detections[:, 1] == DENSE_IM].copy()
    board[:, 2] += CUBE.shape[0]
    line = np.zeros((8, 5))
    line[:, 1], line[:, 2] = LINE_IM, CUBE.shape[0] + BOARD.shape[0] + np.arange(8)
    line[:, 3], line[:, 4] = 500.0 + 20.0 * np.arange(8), 400.0
    det = np.concatenate([det[keep], board, line])
    clean = np.ones(det.shape[0], dtype=bool)
    for im in (4, DENSE_IM, 8):
        rows = np.nonzero(det[:, 1] == im)[0]
        hit = rng.permutation(rows)[: rows.shape[0] // 10]
        ang, mag = rng.uniform(0.0, 2.0 * np.pi, hit.shape[0]), rng.uniform(30.0, 200.0, hit.shape[0])
        det[hit, 3] += mag * np.cos(ang)
        det[hit, 4] += mag * np.sin(ang)
        clean[hit] = False
    return det, clean, rig.intr_true


def test_shapes_at_which_the_kernels_can_go_wrong():
    det, clean, intr = shapes_table()
    run = lambda d, **kw: hip_ch.estimate_view_poses(d, TEMPLATE, intr, n_imgs=17, min_points=4, **kw)   # noqa: E731
    counts = per_view_counts(det, np.ones_like(clean), 1, 17)
    assert [int(counts[0, im]) for im in SIZES] == list(SIZES.values()) and counts[0, DENSE_IM] == 289 > 256 and counts[0, LINE_IM] == 8
    base = run(det, return_residuals=True, **CONS)
    want = run(det[clean])
    # exactly the rows that were not moved, except the collinear view, which has no finite hypothesis and so no inlier
    expect = clean & (det[:, 1] != LINE_IM)
    assert np.array_equal(base.inliers, expect)
    assert_same_bits(base, want)
    assert_same_bits(base, run(det[base.inliers]))   # by construction: start and LM ran on the flagged rows
    assert np.array_equal(base.n_points, counts) and np.array_equal(base.n_inliers, per_view_counts(det, expect, 1, 17))
    # 5 observations, fewer than the sample: the plain path with the plain bits, consensus not used
    assert base.hypothesis[0, 0] == -1 and base.n_inliers[0, 0] == 5
    plain = run(det)
    assert_same_bits(base, plain, where=(slice(None), [0, 1, 2, 3]))   # these views hold no moved row
    assert base.status[0, 1] != hip_ch.PNP_NOT_ESTIMATED and base.n_inliers[0, 1] == 6   # a view of exactly the sample: every hypothesis is the view
    # collinear: not estimated, and the neighbours kept their bits (compared above)
    assert base.status[0, LINE_IM] == hip_ch.PNP_NOT_ESTIMATED and np.all(np.isnan(base.poses[0, LINE_IM])) and base.hypothesis[0, LINE_IM] == -1
    assert np.isnan(base.rms[0, LINE_IM]) and base.n_inliers[0, LINE_IM] == 0
    others = np.arange(17) != LINE_IM
    sure = others & (np.arange(17) != 0)   # five points are fewer than the 3-D DLT takes: whatever the plain path gives
    assert np.all(base.status[0, sure] != hip_ch.PNP_NOT_ESTIMATED) and np.all(base.hypothesis[0, sure] >= 0)
    # residuals of ALL rows at the returned pose, outliers included, in the table's order
    for i in range(17):
        sel = det[:, 1] == i
        if i == LINE_IM:
            assert np.all(np.isnan(base.residuals[sel]))
            continue
        r_np = ref.residuals(base.poses[0, i], TEMPLATE[det[sel, 2].astype(int)], det[sel, 3:5], intr[0])
        assert np.allclose(base.residuals[sel], r_np, rtol=0, atol=1e-9, equal_nan=True)
    moved = np.sqrt(np.sum(base.residuals[~clean] ** 2, axis=1))
    assert moved.shape[0] > 40 and moved.min() > 20.0   # the residuals of the moved rows are there, and large
    # two runs, a shuffled table, another seed
    again = run(det, return_residuals=True, **CONS)
    assert_same_bits(again, base, BITS + ("n_points", "inliers", "n_inliers", "hypothesis", "residuals"))
    perm = np.random.default_rng(9).permutation(det.shape[0])
    shuffled = run(det[perm], return_residuals=True, **CONS)
    assert_same_bits(shuffled, base, BITS + ("n_points", "n_inliers", "hypothesis"))
    assert np.array_equal(shuffled.inliers, base.inliers[perm]) and np.array_equal(shuffled.residuals, base.residuals[perm], equal_nan=True)
    other = run(det, **dict(CONS, seed=12345))
    assert np.array_equal(other.inliers, base.inliers) and not np.array_equal(other.hypothesis, base.hypothesis)
    assert_same_bits(other, base)
    # H = 1 and 5: whatever a single sample finds, the record is consistent, two runs agree, and a view that kept every row has the plain bits
    for H in (1, 5):
        few = run(det, **dict(CONS, consensus=H))
        assert_same_bits(run(det, **dict(CONS, consensus=H)), few, BITS + ("inliers", "n_inliers", "hypothesis"))
        assert np.array_equal(few.n_inliers, per_view_counts(det, few.inliers, 1, 17)) and np.all(few.hypothesis < H)
        whole = few.n_inliers[0] == counts[0]
        assert whole[0] and np.all(few.status[0, few.n_inliers[0] < 4] == hip_ch.PNP_NOT_ESTIMATED)
        assert_same_bits(few, plain, where=(slice(None), np.nonzero(whole)[0]))
    # max_iter = 0: the start's bits on the inliers
    z = run(det, max_iter=0, **CONS)
    assert np.array_equal(z.poses, z.poses_init, equal_nan=True) and np.array_equal(z.poses_init, base.poses_init, equal_nan=True)
    assert np.all(z.status[0, sure] == hip_ch.PNP_MAX_ITER) and np.all(z.iterations == 0) and np.array_equal(z.inliers, base.inliers)
    # a NaN measurement is never an inlier: its view is estimated from the rest, all other views keep their bits
    bad = det.copy()
    row = np.nonzero(det[:, 1] == NAN_IM)[0][2]
    bad[row, 4] = np.nan
    b = run(bad, **CONS)
    assert not b.inliers[row] and np.array_equal(np.delete(b.inliers, row), np.delete(base.inliers, row))
    assert b.status[0, NAN_IM] != hip_ch.PNP_NOT_ESTIMATED and b.n_inliers[0, NAN_IM] == counts[0, NAN_IM] - 1 and b.n_points[0, NAN_IM] == counts[0, NAN_IM]
    assert_same_bits(b, run(np.delete(det, row, axis=0)[np.delete(clean, row)]))
    assert_same_bits(b, base, where=(slice(None), np.arange(17) != NAN_IM))
    assert run(bad).status[0, NAN_IM] == hip_ch.PNP_NOT_ESTIMATED   # what it costs the plain run
    # one view, and no views
    one = run(det[det[:, 1] == 4], **CONS)
    assert_same_bits(one, base, where=(slice(None), [4]))
    assert np.array_equal(one.inliers, base.inliers[det[:, 1] == 4]) and one.n_inliers[0, 4] == base.n_inliers[0, 4]
    e = run(det[:0], **CONS)
    assert np.all(np.isnan(e.poses)) and np.all(e.status == 0) and np.all(e.n_points == 0) and e.inliers.shape == (0,) and np.all(e.n_inliers == 0)


# ---- view counts around one view per thread of the scan ------------------------------------------------------------------------------------
SCAN_VIEWS = (1, 1023, 1025, 2049)
SCAN_CONS = dict(consensus=4, sample_size=6, inlier_px=8.0, seed=0)
# Chosen on the CPU: with these seeds tests/pnp_consensus_reference.py finds exactly the unmoved rows in each of the 2 049 views and
# estimates every one of them from those rows, at 0.1 px of noise and at 0.3 px.  The linear start of six random corners is all a view
# of six rows has (every sample is the view) and amplifies the noise; 0.1 px leaves a factor of three to the device's other rounding.
SCAN_RIG_SEED, SCAN_DRAW_SEED = 41, 1
SCAN_TARGET, SCAN_NOISE_PX = BOARD, 0.1


@functools.lru_cache(maxsize=None)
def scan_table():
    """One camera, 2 049 images of the board of 17 x 17 corners, 6 to 12 detections per view by a seeded draw; a table of V views is its first
    V images.  In every 7th view two detections are moved by 30 to 200 px.  With four hypotheses a moved row can sit in every sample of
    its view, and a view of fewer than eight rows has no sample of six without one, so a view that is hit draws its count from 8 to 12
    and its two moved rows come from outside the sample of hypothesis 0 (the sampler is a pure function of seed, camera, count and
    hypothesis), which the test asserts.  -> (table, clean mask, intrinsics)."""
    V, K = max(SCAN_VIEWS), SCAN_TARGET.shape[0]
    rig = synthetic.make_rig("pnp-scan", 1, V, SCAN_TARGET, seed=SCAN_RIG_SEED, noise_px=SCAN_NOISE_PX)
    det = rig.detections.copy()
    assert det.shape[0] == V * K and np.array_equal(det[:, 1], np.repeat(np.arange(V), K))   # image by image, keys ascending
    rng = np.random.default_rng(SCAN_DRAW_SEED)
    keep, clean = np.zeros(det.shape[0], dtype=bool), np.ones(det.shape[0], dtype=bool)
    for i in range(V):
        hit = i % 7 == 0
        n = int(rng.integers(8 if hit else 6, 13))
        rows = np.sort(rng.permutation(np.arange(i * K, (i + 1) * K))[:n])
        keep[rows] = True
        if hit:
            move_rows(det, clean, np.delete(rows, cons_ref.sample_positions(SCAN_CONS["seed"], 0, n, 0, 6)), 2, rng)
    return det[keep], clean[keep], rig.intr_true


@pytest.mark.parametrize("V", SCAN_VIEWS)
def test_view_counts_on_either_side_of_one_view_per_scan_thread(V):
    """The scan of the inlier counts gives each of its 1 024 threads a contiguous stretch of the views: V = 1 leaves 1 023 of them an
    empty stretch, 1 023 and 1 025 lie on either side of one view per thread, 2 049 cuts the last stretch short.  As in
    test_corrupted_table_gives_the_bits_of_the_clean_rows: exactly the unmoved rows, and the bits of the plain run on them."""
    det, clean, intr = scan_table()
    first = det[:, 1] < V
    det, clean = det[first], clean[first]
    counts = per_view_counts(det, np.ones_like(clean), 1, V)
    assert counts.min() >= 6 and counts.max() <= 12 and (V == 1 or np.unique(counts).shape[0] == 7)
    moved = per_view_counts(det, ~clean, 1, V)[0]
    assert np.array_equal(moved, np.where(np.arange(V) % 7 == 0, 2, 0))
    for i in np.nonzero(moved)[0]:   # at least one sample of the view holds no moved row (rows of a view: keys ascending, as on the device)
        c = clean[det[:, 1] == i]
        assert any(c[cons_ref.sample_positions(SCAN_CONS["seed"], 0, c.shape[0], h, 6)].all() for h in range(SCAN_CONS["consensus"]))
    want = hip_ch.estimate_view_poses(det[clean], SCAN_TARGET, intr, n_imgs=V)
    assert np.all(want.status != hip_ch.PNP_NOT_ESTIMATED)   # the input: every view is estimated from its unmoved rows
    got = hip_ch.estimate_view_poses(det, SCAN_TARGET, intr, n_imgs=V, **SCAN_CONS)
    assert np.array_equal(got.inliers, clean)
    assert_same_bits(got, want)
    assert np.array_equal(got.n_inliers, want.n_points) and np.array_equal(got.n_points, counts)


def test_handle_state_between_consensus_and_plain_runs():
    """Through the cached handle: a consensus run, a plain run, a consensus run on a larger table (every buffer of the stage grows).  The
    plain run has the plain bits and no consensus results; the second consensus run is what a fresh handle returns; a refused setting
    keeps the previous one."""
    rig, det, clean = inp.corrupted_rig("cube")
    small = det[det[:, 1] == 0]
    hip_ch._pnp_cache.clear()
    first = hip_ch.estimate_view_poses(small, rig.points, rig.intr_true, n_imgs=3, **CONS)
    est = hip_ch._pose_estimator(0, 3, rig.points.shape[0])
    assert est.get_consensus() == (64, 6, 8.0, 0) and est.consensus_results()[1].shape == (3, 4)
    plain = hip_ch.estimate_view_poses(small, rig.points, rig.intr_true, n_imgs=3)
    assert est is hip_ch._pose_estimator(0, 3, rig.points.shape[0]) and est.get_consensus()[0] == 0
    with pytest.raises(_capi.PcsError) as err:
        est.consensus_results()
    assert err.value.code == _capi.PCS_ERR_STATE
    second = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3, **CONS)
    lib = _capi.lib()
    for args in ((-1, 6, 8.0, 0), (64, 3, 8.0, 0), (64, 17, 8.0, 0), (64, 6, 0.0, 0), (64, 6, float("nan"), 0), (64, 6, float("inf"), 0), (5000, 6, 8.0, 0)):
        assert lib.pcs_pnp_set_consensus(est._h, *args) == _capi.PCS_ERR_ARG
    assert est.get_consensus() == (64, 6, 8.0, 0)
    hip_ch._pnp_cache.clear()
    fresh_plain = hip_ch.estimate_view_poses(small, rig.points, rig.intr_true, n_imgs=3)
    hip_ch._pnp_cache.clear()
    fresh = hip_ch.estimate_view_poses(det, rig.points, rig.intr_true, n_imgs=3, **CONS)
    assert_same_bits(plain, fresh_plain, BITS + ("n_points",))
    assert_same_bits(second, fresh, BITS + ("n_points", "inliers", "n_inliers", "hypothesis"))
    assert np.array_equal(second.inliers, clean) and np.array_equal(first.inliers, clean[det[:, 1] == 0])
    assert not np.array_equal(plain.poses, first.poses, equal_nan=True)


# ---- where view poses are made -----------------------------------------------------------------------------------------------------------
def test_the_keyword_reaches_the_stage_wherever_view_poses_are_made():
    """The corrupted cube rig.  ``resect_cameras(consensus=64)``: every camera is one view of all its images (288 detections, 42 moved);
    the restatement finds exactly the unmoved rows there too (checked on the CPU with ``resect_cameras(view_pose_fn=...)`` around
    tests/pnp_consensus_reference.py), so the result has the bits of the resection from the unmoved rows.  ``rig_pose_start(consensus=)``
    is what ``localise_target(start_consensus=)`` starts from, and both seedings take ``view_consensus`` or a ``functools.partial``."""
    import functools

    from pycamset_amd import pose_seeding

    rig, det, clean = inp.corrupted_rig("cube")
    got = pose_seeding.resect_cameras(det, rig.points, rig.intr_true, rig.poses_true, **CONS)
    want = pose_seeding.resect_cameras(det[clean], rig.points, rig.intr_true, rig.poses_true)
    plain = pose_seeding.resect_cameras(det, rig.points, rig.intr_true, rig.poses_true)
    assert_same_bits(got, want, ("poses", "rms", "rms_init", "status", "iterations"))
    assert np.all(got.n_points == 288) and np.all(want.n_points == 246) and np.all(got.rms < 1.0) and not np.any(plain.rms < 5.0)
    E = pose_seeding.pose_to_4x4(rig.extr_true)[:, :3, :]
    start = hip_ch.rig_pose_start(det, rig.points, rig.intr_true, E, 3, consensus=64)
    loc = hip_ch.localise_target(det, rig.points, rig.intr_true, E, n_imgs=3, start_consensus=64)
    assert np.array_equal(loc.poses_init, start) and np.all(np.isfinite(start))
    assert not np.array_equal(start, hip_ch.rig_pose_start(det, rig.points, rig.intr_true, E, 3))
    for seeding in (pose_seeding.estimate_camera_relative_poses, pose_seeding.estimate_camera_relative_poses_graph):
        a = seeding(det, rig.points, rig.intr_true, 3, 3, view_consensus=64)
        b = seeding(det, rig.points, rig.intr_true, 3, 3, view_pose_fn=functools.partial(hip_ch.estimate_view_poses, **CONS))
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        try:   # the plain seeding of this table: other extrinsics, or no seed at all where a view was lost
            assert not np.array_equal(a[0], seeding(det, rig.points, rig.intr_true, 3, 3)[0])
        except ValueError as e:
            assert "initial pose" in str(e) or "No image" in str(e)
        with pytest.raises(ValueError, match="view_consensus"):
            seeding(det, rig.points, rig.intr_true, 3, 3, view_pose_fn=hip_ch.estimate_view_poses, view_consensus=64)


# ---- downstream --------------------------------------------------------------------------------------------------------------------------
def ring_with_moved_detections(noise_px, seed=5):
    """ring-8-small with 3 % of its detections moved by 20 to 50 px: the recipe of tests/test_gpu_robust_loss._outlier_problem."""
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8, noise_px=noise_px)
    det = rig.detections.copy()
    rng = np.random.default_rng(seed)
    bad = rng.choice(det.shape[0], max(1, int(0.03 * det.shape[0])), replace=False)
    ang, mag = rng.uniform(0, 2 * np.pi, bad.size), rng.uniform(20.0, 50.0, bad.size)
    det[bad, 3] += mag * np.cos(ang)
    det[bad, 4] += mag * np.sin(ang)
    return rig, det


def ring_handler(rig, det, **options):
    return handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection([f"cam_{i}" for i in range(rig.n_cams)], det),
                                          options=dict({"verbosity": 0}, **options))


def test_consensus_seed_of_a_calibration_with_wrong_detections():
    """Without noise the detections that were not moved are exact, so the consensus seed is the truth to the tolerance of the seeding
    tests on a clean table (``assert_poses_close``, 1e-8), image by image and camera by camera: no moved detection reached a view pose.
    With 0.3 px of noise, the robust solve from the consensus seed ends with a focal error no larger than from the plain seed.

    Both seeds lie in the basin of one minimum of the cauchy objective (3 % of the detections moved by 20 to 50 px bend a view of
    about 50 detections by a few pixels), so the comparison is about that minimum and not about where a stop rule fires: the solve runs
    with ftol = xtol = gtol = 0 until no trial lowers the cost.  Measured on an MI355X, focal error in px from the plain / the
    consensus seed: at the default tolerances 1e-8 3.1458883 / 3.1465012 (18 / 17 trials; the stop rule, not the minimum), at 1e-11
    3.1453058 / 3.1452980, at 1e-14 3.14527807 / 3.14527769, at 0 3.14527671 / 3.14527664 (costs 1185.753304986038 /
    1185.7533049860365).  At the minimum the two agree to 1e-7 px, the width over which the cost is flat to rounding; the solves
    therefore run in the engine's deterministic mode, where every sum has a fixed order and two runs give the same bits (measured
    there: 3.145276710692997 / 3.145276649778907, both costs 1185.7533049860367, 33 / 32 trials)."""
    from pycamset_amd.device_solver import lm_solve

    rig, det = ring_with_moved_detections(0.0)
    h = ring_handler(rig, det, view_consensus=64)   # the handler option
    intr, extr, poses = h.get_bundle_adjustment_inputs(h.calc_initial_params(rig.intr_true))[:3]
    assert not np.any(h.missing_poses) and np.array_equal(poses[0], np.zeros(6))
    assert_poses_close(extr, rig.extr_true)
    assert_poses_close(poses, rig.poses_true)

    rig, det = ring_with_moved_detections(0.3)
    focal = {}
    for name, n_hyp in (("plain", 0), ("consensus", 64)):
        h = ring_handler(rig, det)
        x0 = h.calc_initial_params(rig.intr, view_consensus=n_hyp)
        assert np.all(np.isfinite(x0))
        h.set_initial_params(x0)
        lm_solve(h, h.get_initial_params(), max_iter=0)   # evaluates the start: the handler's engine exists from here on
        h.op_fun.engine.set_option("deterministic", 1)    # every sum of the solve in a fixed order: the comparison is the same in every run
        res = lm_solve(h, h.get_initial_params(), max_iter=800, ftol=0.0, xtol=0.0, gtol=0.0, loss="cauchy", f_scale=1.0)
        got = np.asarray(h.get_bundle_adjustment_inputs(res.x)[0])
        focal[name] = float(np.max(np.abs(got[:, [0, 2]] - rig.intr_true[:, [0, 2]])))
        print(f"{name} seed: focal error after the cauchy solve {focal[name]!r} px, cost {res.cost!r}, {res.nit} trials ({res.message})")
    assert focal["consensus"] <= focal["plain"]
