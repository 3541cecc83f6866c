"""The consensus stage of the batched target-pose estimation without a GPU: the sampler and the NumPy restatement
(tests/pnp_consensus_reference.py) on the corrupted rigs of tests/pnp_consensus_inputs.py, and the argument checks of the new C entry
points and of the Python front end."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as hip_ch
from tests import pnp_consensus_inputs as inp
from tests import pnp_consensus_reference as cref
from tests import pnp_reference as ref

_RESTATED = {}


def restated(kind):
    """The restatement of one corrupted rig, computed once."""
    if kind not in _RESTATED:
        rig, det, clean = inp.corrupted_rig(kind)
        _RESTATED[kind] = (rig, det, clean, cref.estimate_view_poses(det, rig.points, rig.intr_true, 3, **inp.CONSENSUS))
    return _RESTATED[kind]


def test_mix64_is_splitmix64():
    """The first outputs of splitmix64 from state 0 (Vigna's reference implementation): the finaliser of state + golden."""
    assert int(cref.mix64(cref.GOLDEN)) == 0xE220A8397B1DCDAF
    with np.errstate(over="ignore"):
        assert int(cref.mix64(cref.GOLDEN + cref.GOLDEN)) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("n,size", [(4, 4), (6, 6), (7, 6), (16, 6), (17, 16), (54, 6), (300, 6), (2 ** 40, 16)])
def test_sampler_positions_are_distinct_ascending_and_in_range(n, size):
    for hyp in range(64):
        pos = cref.sample_positions(5, 2, n, hyp, size)
        assert pos.shape == (size,) and pos.dtype == np.int64
        assert pos[0] >= 0 and pos[-1] < n and np.all(np.diff(pos) > 0)
    if n == size:
        assert pos.tolist() == list(range(n))


def test_sampler_is_a_pure_function_of_its_key():
    """Same (seed, camera, n, hypothesis): same positions, whatever was drawn before; each of the four changes the draw; over many
    hypotheses every position of the view is drawn about equally often (6 of 30: a fifth each)."""
    a = cref.sample_positions(9, 1, 30, 4, 6)
    cref.sample_positions(1, 0, 12, 0, 6)
    assert np.array_equal(a, cref.sample_positions(9, 1, 30, 4, 6))
    others = [cref.sample_positions(*k, 6) for k in ((10, 1, 30, 4), (9, 2, 30, 4), (9, 1, 31, 4), (9, 1, 30, 5))]
    assert all(not np.array_equal(a, o) for o in others)
    hits = np.zeros(30)
    for hyp in range(2000):
        hits[cref.sample_positions(0, 0, 30, hyp, 6)] += 1
    assert np.all(np.abs(hits / 2000 - 0.2) < 0.04)   # binomial sd sqrt(0.2 * 0.8 / 2000) = 0.009: more than four sd


@pytest.mark.parametrize("kind", inp.KINDS)
def test_plain_start_fails_on_the_corrupted_rigs(kind):
    """What the feature is for: with 15 % of every view moved by 30 to 200 px, ``solve_view`` on all rows is NaN or far off in at least
    one view."""
    from tests.test_pnp_reference import pose_error, true_view_poses
    rig, det, clean, _ = restated(kind)
    T = true_view_poses(rig)
    plain = ref.estimate_view_poses(det, rig.points, rig.intr_true, 3, 3)
    worst = max(np.inf if not np.all(np.isfinite(plain.poses[c, i])) else pose_error(plain.poses[c, i], T[c, i])[0] for c in range(3) for i in range(3))
    assert worst > 0.1


@pytest.mark.parametrize("kind", inp.KINDS)
def test_consensus_finds_exactly_the_uncorrupted_set(kind):
    """In EVERY view the inlier set is the uncorrupted set and the pose is ``solve_view`` on the clean rows, bit for bit."""
    rig, det, clean, res = restated(kind)
    assert len(res) == 9
    for (c, i), (rows, r) in res.items():
        assert int(round(inp.FRACTION * rows.shape[0])) >= 2 and clean[rows].sum() < rows.shape[0]
        assert np.array_equal(r["inliers"], clean[rows]), (kind, c, i)
        assert r["used"] == 1 and r["n_inliers"] == clean[rows].sum() and 0 <= r["hypothesis"] < 64 and r["n_finite"] >= 1
        keep = rows[clean[rows]]
        keep = keep[np.argsort(det[keep, 2], kind="stable")]
        want = ref.solve_view(det[keep, 2].astype(np.int64), det[keep, 3:5], rig.intr_true[c], rig.points)
        got = r["result"]
        assert got["status"] == want["status"] != ref.NOT_ESTIMATED and got["n"] == rows.shape[0]
        assert np.array_equal(got["pose"], want["pose"]) and got["rms"] == want["rms"] and got["iterations"] == want["iterations"]
        assert got["rms"] < 1.0   # 0.3 px noise


def test_corruption_seed_needs_no_exception():
    """The GPU parity test may leave a view out of the index comparison only where the restatement's best two scores are within
    1e-9 relative: with the chosen corruption seed no view is."""
    for kind in inp.KINDS:
        for (c, i), (rows, r) in restated(kind)[3].items():
            s = np.sort(r["scores"].ravel())
            assert np.isfinite(s[1]) and s[1] - s[0] > 1e-9 * s[0], (kind, c, i, s[:2])


def test_selection_rules():
    """Fewer observations than the sample: the plain path.  Collinear detections: no finite hypothesis, not estimated.  A NaN
    measurement is never an inlier and does not cost the view."""
    rig, det, clean = inp.corrupted_rig("cube", fraction=0.0)
    rows = np.nonzero((det[:, 0] == 1) & (det[:, 1] == 2))[0]
    keys, uv, cam9 = det[rows, 2].astype(np.int64), det[rows, 3:5], rig.intr_true[1]
    few = cref.consensus_view(keys[:5], uv[:5], 1, cam9, rig.points, min_points=4, **inp.CONSENSUS)
    assert few["used"] == 0 and few["inliers"].all() and few["hypothesis"] == -1 and np.isnan(few["score"])
    plain = ref.solve_view(keys[:5][np.argsort(keys[:5])], uv[:5][np.argsort(keys[:5])], cam9, rig.points, min_points=4)
    assert np.array_equal(few["result"]["pose"], plain["pose"], equal_nan=True)
    line = np.arange(8)
    pts = np.stack([line * 0.01, np.zeros(8), np.zeros(8)], axis=1)
    flat = cref.consensus_view(line, np.stack([500.0 + 20 * line, np.full(8, 400.0)], axis=1), 0, cam9, pts, **inp.CONSENSUS)
    assert flat["n_finite"] == 0 and flat["hypothesis"] == -1 and not flat["inliers"].any() and flat["result"]["status"] == ref.NOT_ESTIMATED
    bad = uv.copy()
    bad[3, 1] = np.nan
    r = cref.consensus_view(keys, bad, 1, cam9, rig.points, **inp.CONSENSUS)
    assert not r["inliers"][3] and r["n_inliers"] == len(keys) - 1 and r["result"]["status"] == ref.CONVERGED


def test_argument_checks_need_no_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 115
    assert lib.pcs_pnp_set_consensus(None, 64, 6, 8.0, 0) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_get_consensus(None, None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_pnp_consensus_results(None, None, None, None) == _capi.PCS_ERR_ARG
    assert b"pcs_pnp_consensus_results" in lib.pcs_last_error()
    for kw in (dict(consensus=-1), dict(consensus=True), dict(consensus=1.5), dict(consensus=64, sample_size=3), dict(consensus=64, sample_size=17),
               dict(consensus=64, inlier_px=0.0), dict(consensus=64, inlier_px=np.nan), dict(consensus=64, inlier_px=np.inf),
               dict(consensus=64, inlier_px="wide"), dict(consensus=64, seed=-1), dict(consensus=64, seed=2 ** 64)):
        with pytest.raises(ValueError):
            hip_ch.estimate_view_poses(np.zeros((0, 5)), np.zeros((4, 3)), np.ones((1, 9)), n_imgs=1, **kw)
    out = hip_ch.estimate_view_poses(np.zeros((0, 5)), np.zeros((4, 3)), np.ones((1, 9)), n_imgs=2, consensus=64)
    assert out.inliers.shape == (0,) and out.n_inliers.shape == (1, 2) and np.all(out.hypothesis == -1)
    out = hip_ch.estimate_view_poses(np.zeros((0, 5)), np.zeros((4, 3)), np.ones((1, 9)), n_imgs=2)
    assert out.inliers is None and out.n_inliers is None and out.hypothesis is None
    assert ctypes.sizeof(ctypes.c_uint64) == 8
