"""The consensus stage in front of the planar homographies without a GPU: the NumPy restatement (tests/intr_consensus_reference.py) on the
corrupted rigs and on the shapes table of tests/intr_consensus_inputs.py, its selection rules, ``calc_initial_params`` with the
restatement injected, and the argument checks of the C entry points and of the Python front end."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd.detections import TargetDetection
from tests import intr_consensus_inputs as inp
from tests import intr_consensus_reference as cref
from tests import intrinsics_reference as ref
from tests import pnp_reference as pnp_ref
from tests.pnp_consensus_reference import sample_positions
from tests.test_intrinsics_reference import FaceTarget, rig_of
from tests.test_pnp_reference import CUBE, DuckCamset

CONS = dict(consensus=64, sample_size=6, inlier_px=8.0, seed=0)
# What the GPU parity test may leave to the tie rule: the device and NumPy round the homography of a sample differently (1e-12 relative
# on well-conditioned samples, more on nearly degenerate ones), so the order of two DIFFERENT samples is the same on both only where
# their scores differ by more than that.  The issue's figure.
GAP = 1e-9


@functools.lru_cache(maxsize=None)
def restated(kind):
    """-> (rig, true intrinsics, corrupted table, board_of_key, clean mask, restatement with the stage).  Computed once, never changed."""
    rig, intr, det, bok, clean = inp.corrupted_rig(kind)
    r = cref.estimate_intrinsics(det, rig.points, n_cams=inp.N_CAMS, n_imgs=inp.N_IMGS, board_of_key=bok, model="full", **CONS)
    return rig, intr, det, bok, clean, r


@functools.lru_cache(maxsize=None)
def restated_shapes():
    det, clean = inp.shapes_table()
    r = cref.estimate_intrinsics(det, inp.TEMPLATE, n_cams=inp.SHAPES_CAMS, n_imgs=inp.SHAPES_IMGS, board_of_key=inp.SHAPES_BOARD_OF_KEY, model="full",
                                 min_points=4, **CONS)
    return det, clean, r


@pytest.mark.parametrize("kind", inp.KINDS)
def test_plain_restatement_loses_every_camera_of_the_corrupted_rigs(kind):
    """The input exercises the feature: 15 % of every group moved costs the closed form all three cameras, with either model."""
    rig, intr, det, bok, clean = inp.corrupted_rig(kind)
    assert 0.1 < 1.0 - clean.mean() < 0.2
    for model, res in (("full", None), ("focal", (1000, 1000))):
        r = ref.estimate_intrinsics(det, rig.points, n_cams=inp.N_CAMS, n_imgs=inp.N_IMGS, board_of_key=bok, model=model, res=res)
        assert np.all(r.status == ref.NOT_ESTIMATED), (model, r.status)
    ok = ref.estimate_intrinsics(det[clean], rig.points, n_cams=inp.N_CAMS, n_imgs=inp.N_IMGS, board_of_key=bok, model="full")
    assert np.all(ok.status == ref.FULL)


@pytest.mark.parametrize("kind", inp.KINDS)
def test_corruption_seeds_need_no_exception(kind):
    """With the committed corruption seed the restatement finds exactly the uncorrupted set in every group, and no winner is within
    1e-9 relative of another sample's score: the GPU parity test needs no exception.  The result is the plain restatement on the
    unmoved rows, and ``group_counts`` stays the observation count."""
    rig, intr, det, bok, clean, r = restated(kind)
    print(f"{kind}: {len(r.group_gap)} groups of {np.unique(r.group_counts).tolist()} observations, smallest gap {r.group_gap.min():.2e}")
    assert np.array_equal(r.inliers, clean) and r.group_gap.min() > GAP
    assert np.all(r.group_consensus_used) and np.all(r.group_hypothesis >= 0) and np.all(r.status == ref.FULL)
    want = ref.estimate_intrinsics(det[clean], rig.points, n_cams=inp.N_CAMS, n_imgs=inp.N_IMGS, board_of_key=bok, model="full")
    for name in ("intr", "status", "n_groups", "eig_ratio", "homographies", "plane_frames", "group_status"):
        assert np.array_equal(getattr(r, name), getattr(want, name), equal_nan=True), name
    assert np.array_equal(r.group_inliers, want.group_counts)
    assert np.array_equal(r.group_counts, ref.estimate_intrinsics(det, rig.points, n_cams=3, n_imgs=6, board_of_key=bok, model="full").group_counts)
    errs = np.abs(r.intr[:, :4] - intr[:, :4]) / intr[:, :4]
    # printed, not bounded: make_rig's pose spread (0.15 rad) leaves the full model of the 5 x 5 board weakly constrained with or without
    # moved rows (tests/test_intrinsics_reference.py); what the stage owes is the result of the unmoved rows, asserted above
    print(f"{kind}: relative error of the closed form on the inliers {errs.max():.2e}")


def test_shapes_table_needs_no_exception():
    det, clean, r = restated_shapes()
    counts = sorted(r.group_counts.tolist())
    assert {3, 5, 6, 8, 13, 16, 17, 65, 289} == set(counts) and len(counts) == 35 and 16 * len(counts) > 2 * 256
    assert sorted(set(range(inp.SHAPES_CAMS)) - set(r.group_index[:, 0].tolist())) == list(inp.EMPTY_CAMS)
    assert np.array_equal(r.inliers, clean) and (~clean).sum() == 2 + 6 + 29
    gap = r.group_gap[np.isfinite(r.group_gap)]
    print(f"shapes: smallest gap {gap.min():.2e} over {gap.shape[0]} groups")
    assert gap.min() > GAP
    by = {tuple(ix): k for k, ix in enumerate(r.group_index.tolist())}
    # (a) fewer observations than max(sample, min_points): not used; three rows are fewer than min_points as well
    for g, status in (((2, 0, 0), ref.GROUP_TOO_FEW), ((2, 0, 1), ref.GROUP_USED)):
        k = by[g]
        assert not r.group_consensus_used[k] and r.group_hypothesis[k] == -1 and np.isnan(r.group_score[k]) and r.group_status[k] == status
    # exactly the sample: every hypothesis is the group, an exact tie, the lowest wins
    k = by[(2, 0, 4)]
    assert r.group_hypothesis[k] == 0 and r.group_inliers[k] == 6 and r.group_consensus_used[k] and r.group_gap[k] == np.inf
    # (b) the collinear group: used, no finite hypothesis, every row goes on, the plain status
    k = by[(2, 1, inp.LINE_BOARD)]
    assert r.group_consensus_used[k] and r.group_hypothesis[k] == -1 and r.group_score[k] == np.inf and r.group_finite[k] == 0
    assert r.group_inliers[k] == 8 and r.group_status[k] == ref.GROUP_NOT_PLANAR


def test_selection_rules():
    rig, _, _, det, bok = rig_of("cube", noise_px=0.3, n_imgs=1)
    g = det[(det[:, 0] == 0) & (bok[det[:, 2].astype(int)] == bok[int(det[0, 2])])]
    keys, uv = g[:, 2].astype(np.int64), g[:, 3:5]
    assert keys.shape[0] == 16
    # a tie: every hypothesis scores the same, the lowest wins; the first of two equal minima wins
    tie = cref.consensus_group(keys, uv, 0, CUBE, n_hypotheses=8, score_fn=lambda *a: 3.0)
    assert tie["hypothesis"] == 0 and tie["score"] == 3.0
    assert cref.select([5.0, 2.0, 2.0, np.inf]) == (1, 2.0) and cref.select([np.inf, np.inf]) == (-1, np.inf)
    # samples of 4 out of 16: C(16, 4) = 1820 against 512 draws, two hypotheses draw the same sample and tie exactly
    many = cref.consensus_group(keys, uv, 0, CUBE, min_points=4, n_hypotheses=512, sample_size=4)
    samples = [tuple(sample_positions(0, 0, 16, h, 4)) for h in range(512)]
    assert len(set(samples)) < 512
    first = {}
    for h, s in enumerate(samples):
        first.setdefault(s, h)
    assert all(many["scores"][h] == many["scores"][first[s]] for h, s in enumerate(samples))   # bit for bit
    assert many["hypothesis"] == first[samples[many["hypothesis"]]]
    # (a) a group shorter than the sample, or than min_points: not used, all rows go on, the plain result
    for n, mp, S in ((5, 4, 6), (12, 13, 6), (7, 4, 8)):
        short = cref.consensus_group(keys[:n], uv[:n], 0, CUBE, min_points=mp, sample_size=S)
        assert short["used"] == 0 and short["hypothesis"] == -1 and np.isnan(short["score"]) and short["inliers"].all()
        plain = ref.group_homography(keys[:n], uv[:n], CUBE, min_points=mp)
        assert short["result"]["status"] == plain["status"] and np.array_equal(short["result"]["H"], plain["H"], equal_nan=True)
    # (b) no finite hypothesis: used, all rows go on and the final fit names the reason, as the plain run does
    line = np.stack([np.arange(8) * 0.01, np.zeros(8), np.zeros(8)], axis=1)
    uv8 = np.stack([500.0 + 20.0 * np.arange(8), np.full(8, 400.0)], axis=1)
    col = cref.consensus_group(np.arange(8), uv8, 0, line, min_points=4)
    assert col["used"] == 1 and col["hypothesis"] == -1 and col["score"] == np.inf and col["n_finite"] == 0 and col["inliers"].all()
    assert col["result"]["status"] == ref.GROUP_NOT_PLANAR == ref.group_homography(np.arange(8), uv8, line, min_points=4)["status"]
    bad = uv.copy()
    bad[:, 1] = np.nan
    nf = cref.consensus_group(keys, bad, 0, CUBE)
    assert nf["used"] == 1 and nf["hypothesis"] == -1 and nf["inliers"].all() and nf["result"]["status"] == ref.GROUP_NOT_FINITE
    # one NaN measurement: never an inlier, the group is estimated from the rest
    one = uv.copy()
    one[3, 0] = np.nan
    r = cref.consensus_group(keys, one, 0, CUBE)
    assert r["hypothesis"] >= 0 and not r["inliers"][3] and r["n_inliers"] == 15 and r["result"]["status"] == ref.GROUP_USED and r["n_finite"] < 64
    # the rows come in any order: the flags follow them
    perm = np.random.default_rng(1).permutation(16)
    p = cref.consensus_group(keys[perm], one[perm], 0, CUBE)
    assert np.array_equal(p["inliers"], r["inliers"][perm]) and p["score"] == r["score"] and p["hypothesis"] == r["hypothesis"]


# ---- calc_initial_params ---------------------------------------------------------------------------------------------------------------
def test_calc_initial_params_reaches_the_stage(monkeypatch):
    calls = []

    def restatement(*a, **kw):
        calls.append(kw)
        return cref.estimate_intrinsics(*a, **kw)

    rig, intr, det, bok, clean, _ = restated("cube")
    moved = {tuple(r) for r in det[~clean, :3].astype(int).tolist()}

    def view_poses(dct, *a, **kw):
        """The plain PnP restatement on the rows that were not moved: a stand-in for ``view_consensus``, whose own tests are
        tests/test_pnp_consensus_reference.py and tests/test_gpu_pnp_consensus.py.  This test is about the stage in front of it."""
        dct = np.asarray(dct)
        return pnp_ref.estimate_view_poses(dct[[tuple(r) not in moved for r in dct[:, :3].astype(int).tolist()]], *a, **kw)

    monkeypatch.setattr(hip_ch, "estimate_intrinsics", restatement)
    monkeypatch.setattr(hip_ch, "estimate_view_poses", view_poses)
    monkeypatch.setattr(hip_ch, "bundle_adjustment_costfn", orc.legacy_cost)
    td = TargetDetection([f"cam_{i}" for i in range(3)], det)
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), td)
    with pytest.raises(ValueError, match="do not give an estimate"):
        h.calc_initial_params()
    assert calls[-1]["consensus"] == 0
    with pytest.raises(ValueError, match="do not give an estimate"):
        h.calc_initial_params(intrinsics_consensus=0)
    h.calc_initial_params(intrinsics_consensus=64)   # the keyword
    assert calls[-1]["consensus"] == 64 and calls[-1]["refine"] is True and np.array_equal(calls[-1]["board_of_key"], bok)
    est = h.initial_intrinsics
    assert np.all(est.status == ref.FULL) and np.array_equal(est.inliers, clean)
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), td, options={"intrinsics_consensus": 32})   # the handler option
    x = h.calc_initial_params()
    assert calls[-1]["consensus"] == 32 and np.all(np.isfinite(x)) and np.array_equal(x[:27].reshape(3, 9), h.initial_intrinsics.intr)
    h.calc_initial_params(intrinsics_consensus=64)   # the keyword goes before the option
    assert calls[-1]["consensus"] == 64
    n = len(calls)
    handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), td).calc_initial_params(intr, intrinsics_consensus=64)   # intrinsics brought: nothing estimated
    assert len(calls) == n


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_consensus_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 117
    assert lib.pcs_intr_set_consensus(None, 64, 6, 8.0, 0) == _capi.PCS_ERR_ARG and b"NULL handle" in lib.pcs_last_error()
    assert lib.pcs_intr_get_consensus(None, None, None, None, None) == _capi.PCS_ERR_ARG and b"NULL handle" in lib.pcs_last_error()
    assert lib.pcs_intr_consensus_results(None, None, None, None) == _capi.PCS_ERR_ARG and b"NULL handle" in lib.pcs_last_error()
    for name in ("pcs_intr_set_consensus", "pcs_intr_get_consensus", "pcs_intr_consensus_results"):
        assert name in _capi.SYMBOLS
    assert _capi.SYMBOLS["pcs_intr_set_consensus"] == _capi.SYMBOLS["pcs_pnp_set_consensus"]
    assert _capi.SYMBOLS["pcs_intr_get_consensus"] == _capi.SYMBOLS["pcs_pnp_get_consensus"]
    assert _capi.SYMBOLS["pcs_intr_consensus_results"] == _capi.SYMBOLS["pcs_pnp_consensus_results"]
    assert ctypes.sizeof(ctypes.c_uint64) == 8


def test_python_front_end_validates_the_consensus_options_before_the_device():
    rig, _, _, det, bok = rig_of("cube", n_imgs=2)
    ok = dict(n_cams=3, n_imgs=2, board_of_key=bok)
    for kw in ({"consensus": -1}, {"consensus": 4097}, {"consensus": 6.0}, {"consensus": True}, {"consensus": 64, "sample_size": 3},
               {"consensus": 64, "sample_size": 17}, {"sample_size": 3}, {"consensus": 64, "inlier_px": 0.0}, {"inlier_px": float("nan")},
               {"consensus": 64, "inlier_px": float("inf")}, {"inlier_px": "wide"}, {"consensus": 64, "seed": -1}, {"seed": 2 ** 64}):
        with pytest.raises(ValueError, match="consensus|sample_size|inlier_px|seed"):
            hip_ch.estimate_intrinsics(det, rig.points, **{**ok, **kw})
    # named keywords: they do not fall into the refinement's options
    with pytest.raises(ValueError, match="belong to the refinement"):
        hip_ch.estimate_intrinsics(det, rig.points, **ok, max_iter=5, consensus=64)
    # an empty table needs no device: the five fields are there with the stage and None without it
    e = hip_ch.estimate_intrinsics(det[:0], rig.points, **ok, **CONS)
    assert e.inliers.shape == (0,) and e.inliers.dtype == bool and e.group_inliers.shape == (0,) and e.group_hypothesis.shape == (0,)
    assert e.group_consensus_used.shape == (0,) and e.group_score.shape == (0,) and np.all(e.status == 0)
    p = hip_ch.estimate_intrinsics(det[:0], rig.points, **ok)
    assert p.inliers is None and p.group_inliers is None and p.group_hypothesis is None and p.group_consensus_used is None and p.group_score is None
    h = handlers.TemplateBundleHandler(DuckCamset(3), FaceTarget(), TargetDetection([f"cam_{i}" for i in range(3)], det))
    with pytest.raises(ValueError, match="consensus"):
        h.calc_initial_params(intrinsics_consensus=-3)
