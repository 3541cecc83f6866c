"""The view-pair consensus in front of the batched triangulation on the GPU (include/pcs_hip.h pcs_tri_set_consensus,
csrc/ba_tri_consensus.hpp) against the plain run and against its NumPy restatement (tests/tri_consensus_reference.py).

What is compared bit for bit: the stage compacts the table to the inliers and runs the unchanged kernels on it, so a point's DLT point,
refined point, RMS values, trial count and status are those of a plain run on the table WITHOUT the rejected rows, whatever else the table
holds; the residuals of the kept rows are the same projection at the same point.  What is compared to 1e-9 relative: the winner's score,
where the device's hypothesis points (its own DLT) and the restatement's (the oracle's SVD) differ by rounding."""
import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as hip_ch
from tests import tri_consensus_inputs as inp
from tests import tri_consensus_reference as cref

pytestmark = pytest.mark.gpu

H64 = inp.CONSENSUS["n_hypotheses"]
POINT_FIELDS = ("points", "points_dlt", "rms", "rms_dlt", "iterations", "status")


def refine(rec, start, P, K, D, consensus=0, **kw):
    return hip_ch.refine_triangulation(rec, P, start, K, D, return_residuals=True, consensus=consensus, **kw)


def assert_same_points(a, b, sel_a=slice(None), sel_b=slice(None), what=""):
    for f in POINT_FIELDS:
        assert np.array_equal(getattr(a, f)[sel_a], getattr(b, f)[sel_b], equal_nan=True), (what, f)


def assert_same_result(a, b, what=""):
    assert_same_points(a, b, what=what)
    assert np.array_equal(a.n_views, b.n_views), what
    assert np.array_equal(a.residuals, b.residuals, equal_nan=True), what
    assert np.array_equal(a.cost, b.cost, equal_nan=True), what
    for f in ("inliers", "n_inliers", "consensus_used", "score"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), (what, f)


def assert_is_plain_run_on_kept_rows(res, rec, start, P, K, D, keep, points=None, what=""):
    """``res`` (a run with the stage) against a plain run on the table without the rows where ``keep`` is False, for ``points`` (bool)."""
    n = len(start) - 1
    points = np.ones(n, dtype=bool) if points is None else points
    drec, dstart = inp.deleted_table(rec, start, keep)
    plain = refine(drec, dstart, P, K, D)
    assert_same_points(res, plain, points, points, what)
    assert np.array_equal(res.n_views, np.diff(start)), what
    assert np.array_equal(res.n_inliers[points], plain.n_views[points]), what
    rows = np.repeat(points, np.diff(start))
    assert np.array_equal(res.residuals[rows & keep], plain.residuals[np.repeat(points, np.diff(dstart))], equal_nan=True), what
    return plain


def test_clean_table_gives_the_plain_bits():
    rec, start, P, K, D, _ = inp.clean_rig("tri-perm")
    plain, cons = refine(rec, start, P, K, D), refine(rec, start, P, K, D, H64)
    assert_same_points(cons, plain)
    assert np.array_equal(cons.n_views, plain.n_views) and np.array_equal(cons.residuals, plain.residuals)
    assert np.array_equal(cons.cost, plain.cost)
    assert plain.inliers is None and plain.n_inliers is None and plain.consensus_used is None and plain.score is None
    assert cons.inliers.dtype == bool and cons.inliers.shape == (rec.shape[0],) and cons.inliers.all()
    assert np.array_equal(cons.n_inliers, np.diff(start)) and np.array_equal(cons.consensus_used, np.diff(start) >= 3)
    assert np.array_equal(hip_ch.nb_triangulate_full(rec, P, start, K, D, consensus=H64), plain.points_dlt)


@pytest.mark.parametrize("name", inp.RIGS)
def test_corrupted_table_returns_the_points_of_the_unmoved_rows(name):
    """Fails without the stage: the plain run on the corrupted table is further from the truth at every point with a moved view."""
    _, start, P, K, D, truth = inp.clean_rig(name)
    rec, clean = inp.corrupted_rig(name)
    many, rows = np.diff(start) >= inp.MIN_VIEWS_CHECKED, inp.many_views(start)
    cons = refine(rec, start, P, K, D, H64)
    assert np.array_equal(cons.inliers[rows], clean[rows])
    assert np.all(cons.consensus_used[many]) and np.all(np.isfinite(cons.score[many]))
    assert_is_plain_run_on_kept_rows(cons, rec, start, P, K, D, clean | ~rows, many, name)
    wrong = refine(rec, start, P, K, D)
    e_cons, e_wrong = np.linalg.norm(cons.points - truth, axis=1)[many], np.linalg.norm(wrong.points - truth, axis=1)[many]
    print(name, "median distance to the truth: consensus", np.median(e_cons), "plain", np.median(e_wrong), "smallest ratio", (e_wrong / e_cons).min())
    assert np.all(e_wrong > e_cons)
    assert np.median(e_wrong) > 10.0 * np.median(e_cons)


def device_stage(rec, start, P, K, D, n_hypotheses, inlier_px=8.0, seed=0):
    """The stage alone, through a handle of its own -> (inlier, cinfo, score)."""
    tri = hip_ch.Triangulator(P.shape[0])
    tri.set_cameras(P, K, D)
    tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
    tri.set_consensus(n_hypotheses, inlier_px, seed)
    tri.run()
    out = tri.consensus_results()
    tri.close()
    return out


def assert_parity(dev, restated, start, max_left_out, skip=None, what=""):
    """Per point: consensus used, winning hypothesis, inlier count, flags, score to 1e-9 relative.  A point is left out of the index
    comparison (winner, count, flags) only where the restatement's best two scores of distinct pairs are within 1e-9 relative.
    ``skip``: points whose expectation is a stated rule, checked by the caller."""
    (d_inl, d_cinfo, d_score), (inlier, cinfo, score, gap) = dev, restated
    n = len(start) - 1
    take = np.ones(n, dtype=bool) if skip is None else ~skip
    used = cinfo[:, 3] == 1
    assert np.array_equal(d_cinfo[:, 3], cinfo[:, 3]), what
    assert np.array_equal(np.isnan(d_score), ~used), what
    assert np.array_equal(np.isinf(d_score[take]), np.isinf(score[take])), what
    fin = used & np.isfinite(score) & take
    rel = np.abs(d_score[fin] - score[fin]) / score[fin]
    print(what, "largest relative score difference", rel.max() if rel.size else 0.0, "| finite hypotheses differ at",
          int(np.sum(d_cinfo[:, 2] != cinfo[:, 2])), "points")
    assert np.all(rel <= 1e-9), what
    close = used & ~(gap > 1e-9) & take
    assert close.sum() <= max_left_out, (what, np.nonzero(close)[0])
    cmp = take & ~close
    assert np.array_equal(d_cinfo[cmp, 1], cinfo[cmp, 1]), what
    assert np.array_equal(d_cinfo[cmp, 0], cinfo[cmp, 0]), what
    rows = np.repeat(cmp, np.diff(start))
    assert np.array_equal(d_inl[rows], inlier[rows]), what


@pytest.mark.parametrize("name", inp.RIGS)
def test_parity_with_the_restatement(name):
    _, start, P, K, D, _ = inp.clean_rig(name)
    rec, _ = inp.corrupted_rig(name)
    dev = device_stage(rec, start, P, K, D, **inp.CONSENSUS)
    assert_parity(dev, inp.restated(name), start, max_left_out=0, what=name)   # at most one may be left out; with the committed inputs none is


# ---- shapes at which the kernels can go wrong -------------------------------------------------------------------------------------------
SHAPES = ("none-first", "one", "two", "three", "six", "seven", "twenty-eight", "thirty-three", "one-camera", "all-nan", "scattered", "nan-view")
N_PAIRS = 5200   # two-view points behind the named ones: the scan's 1 024 threads get stretches of 6 points, and 155 threads none


def shapes_table():
    """One small table on the 32 cameras of tri-refine -> (rec, start, P, K, D, index of each named point).  Measurements are the model's
    projection of a true point plus 0.3 px noise; moved views are moved by 80 px."""
    _, _, P, K, D, truth = inp.clean_rig("tri-refine")
    rng = np.random.default_rng(7)
    groups = []

    def views(X, cams, moved=()):
        cams = np.asarray(cams, dtype=int)
        uv, depth = cref.project_many(X[None], cams, P, K, D)
        assert np.all(depth > 0)
        uv = uv[0] + rng.normal(0, 0.3, (len(cams), 2))
        for m in moved:
            uv[m] += 80.0 * np.array([np.cos(m), np.sin(m)])
        return cams, uv

    X = truth[: len(SHAPES)]
    groups.append(views(X[0], []))
    groups.append(views(X[1], [3]))
    groups.append(views(X[2], [3, 9]))
    groups.append(views(X[3], [1, 12, 20]))
    groups.append(views(X[4], [0, 5, 11, 16, 22, 27], moved=[2]))                    # 15 pairs = H: exhaustive at the boundary
    groups.append(views(X[5], [0, 5, 11, 16, 22, 27, 30], moved=[4]))                # 21 pairs > H = 15: sampled
    groups.append(views(X[6], np.arange(28), moved=[3, 25]))                         # past the 24 register views of the default kernel
    groups.append(views(X[7], np.append(np.arange(32), 0), moved=[10, 32]))
    groups.append(views(X[8], [5, 5, 5, 5]))                                         # rays of one camera meet at its centre: depth 0
    cams, uv = views(X[9], [2, 8, 14])
    groups.append((cams, np.full_like(uv, np.nan)))                                  # no finite hypothesis
    cams, uv = views(X[10], [4, 13, 21])
    groups.append((cams, uv + rng.uniform(100.0, 200.0, uv.shape) * rng.choice([-1.0, 1.0], uv.shape)))   # no two views agree on a point
    cams, uv = views(X[11], [6, 10, 15, 19, 24])
    uv[1, 1] = np.nan
    groups.append((cams, uv))
    for i in range(N_PAIRS):
        groups.append(views(truth[i % len(truth)], [i % 31, i % 31 + 1]))
    groups.append(views(X[0], []))                                                   # the last point of the table has no views
    counts = np.array([len(c) for c, _ in groups])
    start = np.append(0, np.cumsum(counts))
    rec = np.zeros((start[-1], 5))
    rec[:, 0] = np.concatenate([c for c, _ in groups])
    rec[:, 2] = np.repeat(np.arange(len(groups)), counts)
    rec[:, -2:] = np.concatenate([u for _, u in groups])
    return rec, start, P, K, D, {name: i for i, name in enumerate(SHAPES)}


@pytest.mark.parametrize("H", [15, 1, 256])
def test_shapes_at_which_the_kernels_can_go_wrong(H):
    rec, start, P, K, D, at = shapes_table()
    n = len(start) - 1
    assert n >= 5000 + len(SHAPES) and start[-1] == start[-2] and np.diff(start)[at["twenty-eight"]] > 24
    restated = cref.consensus_table(rec, start, P, K, D, H, 8.0, 0)
    inlier, cinfo, score, gap = restated
    res = refine(rec, start, P, K, D, H)
    dev = device_stage(rec, start, P, K, D, H)
    assert np.array_equal(dev[0], res.inliers) and np.array_equal(dev[1][:, 0], res.n_inliers) and np.array_equal(dev[2], res.score, equal_nan=True)
    # the one-camera point goes by the rules (below): its candidates are the camera centre to rounding, where depth and finiteness are rounding's
    skip = np.zeros(n, dtype=bool)
    skip[at["one-camera"]] = True
    assert_parity(dev, restated, start, max_left_out=0, skip=skip, what=f"shapes H={H}")
    d_inl, d_cinfo, d_score = dev
    views = np.diff(start)
    # the plain path: fewer than three views, all flagged, consensus not used
    few = views < 3
    assert np.all(d_cinfo[few, 3] == 0) and np.all(d_cinfo[few, 1] == -1) and np.array_equal(d_cinfo[few, 0], views[few])
    assert d_inl[np.repeat(few, views)].all() and np.all(np.isnan(d_score[few]))
    assert np.all(np.isnan(res.points[views < 2])) and np.all(np.isfinite(res.points[views == 2]))
    # every point: the bits of the plain run on the kept rows (compaction across workgroups, beyond the register views, empty points)
    assert_is_plain_run_on_kept_rows(res, rec, start, P, K, D, d_inl, what=f"shapes H={H}")
    if H == 15:
        assert cref.exhaustive(6, H) and not cref.exhaustive(7, H)
        for name, moved in (("six", [2]), ("seven", [4]), ("twenty-eight", [3, 25]), ("thirty-three", [10, 32])):
            j = at[name]
            want = np.ones(views[j], dtype=bool)
            want[moved] = False
            assert np.array_equal(d_inl[start[j]:start[j + 1]], want), name
        assert d_cinfo[at["six"], 2] == 15 and d_inl[start[at["three"]]:start[at["three"] + 1]].all()
    # a point without a finite hypothesis, and points whose winner has fewer than two inliers: no row kept, NaN
    j = at["all-nan"]
    assert d_score[j] == np.inf and list(d_cinfo[j]) == [0, -1, 0, 1] and np.all(np.isnan(res.points[j])) and np.all(np.isnan(res.points_dlt[j]))
    j = at["scattered"]
    assert cinfo[j, 0] == 0 and cinfo[j, 1] >= 0   # the restatement: a winner, and nothing kept of it
    assert d_cinfo[j, 0] == 0 and d_cinfo[j, 3] == 1 and d_cinfo[j, 1] >= 0 and not d_inl[start[j]:start[j + 1]].any()
    assert np.all(np.isnan(res.points[j])) and np.isnan(res.rms[j]) and res.status[j] == hip_ch.TRI_NOT_REFINED
    # Views of one camera: every pair's rays meet at the camera centre, where the depth is 0 to rounding and the projection 0 / 0, so
    # whether a candidate is finite, in front, or an inlier of its own ray is rounding's.  The rules that hold whatever it is: without a
    # finite candidate the score is +inf, nothing is kept and the point is NaN; fewer than two inliers keep nothing; and (above) the
    # outputs are those of the plain run on the kept rows.
    j = at["one-camera"]
    print(f"shapes H={H} one-camera: cinfo", d_cinfo[j], "score", d_score[j], "point", res.points[j])
    assert d_cinfo[j, 3] == 1 and d_cinfo[j, 0] != 1
    if d_cinfo[j, 2] == 0:
        assert d_score[j] == np.inf and d_cinfo[j, 1] == -1
    if d_score[j] == np.inf or d_cinfo[j, 0] == 0:
        assert d_cinfo[j, 0] == 0 and not d_inl[start[j]:start[j + 1]].any() and np.all(np.isnan(res.points[j]))
    # a NaN measurement is never an inlier and touches only its own point
    j = at["nan-view"]
    assert not d_inl[start[j] + 1] and np.isnan(res.residuals[start[j] + 1, 1]) and np.all(np.isfinite(res.points[j]))
    fixed = rec.copy()
    fixed[start[j] + 1, -2:] = cref.project_many(res.points[j][None], rec[start[j] + 1: start[j] + 2, 0].astype(int), P, K, D)[0][0, 0]
    other = refine(fixed, start, P, K, D, H)
    rest = np.arange(n) != j
    assert_same_points(other, res, rest, rest, "nan-view")
    rows = np.repeat(rest, views)
    assert np.array_equal(other.inliers[rows], res.inliers[rows]) and np.array_equal(other.score[rest], res.score[rest], equal_nan=True)
    assert np.array_equal(other.residuals[rows], res.residuals[rows], equal_nan=True)


def test_two_runs_agree_and_a_point_depends_on_its_index_and_rows_only():
    """The sampler is keyed by the point's index (pcs_hip.h), so a permuted table draws other pairs; what holds instead: a point's result
    depends on nothing but (its index, its rows) — here every other point keeps index and rows while all the others get other rows."""
    _, start, P, K, D, _ = inp.clean_rig("tri-refine")
    rec, _ = inp.corrupted_rig("tri-refine")
    a, b = refine(rec, start, P, K, D, H64), refine(rec, start, P, K, D, H64)
    assert_same_result(a, b, "two runs")
    n = len(start) - 1
    assert not all(cref.exhaustive(int(v), H64) for v in np.diff(start))   # the sampler is in play
    kept = np.arange(n) % 2 == 0
    src = np.where(kept, np.arange(n), (np.arange(n) + 2 * (n // 4) + 1) % n)
    rows = np.concatenate([np.arange(start[j], start[j + 1]) for j in src])
    start2 = np.append(0, np.cumsum(np.diff(start)[src]))
    c = refine(rec[rows], start2, P, K, D, H64)
    assert_same_points(c, a, kept, kept, "other neighbours")
    ra, rc = np.repeat(kept, np.diff(start)), np.repeat(kept, np.diff(start2))
    assert np.array_equal(c.inliers[rc], a.inliers[ra]) and np.array_equal(c.residuals[rc], a.residuals[ra])
    assert np.array_equal(c.score[kept], a.score[kept], equal_nan=True) and np.array_equal(c.n_inliers[kept], a.n_inliers[kept])
    assert not np.array_equal(c.points[~kept], a.points[~kept], equal_nan=True)


def handle_result(tri, **kw):
    tri.run(**kw)
    tri.refine(residuals=True, **kw)
    return tri.with_consensus(tri.refined())


def test_handle_state():
    import torch

    _, start, P, K, D, _ = inp.clean_rig("tri-refine")
    rec, _ = inp.corrupted_rig("tri-refine")
    small_n = 60
    srec, sstart = rec[: start[small_n]], start[: small_n + 1]
    cam = rec[:, 0].astype(np.int32)

    def fresh(rec_, start_, *setting):
        t = hip_ch.Triangulator(P.shape[0])
        t.set_cameras(P, K, D)
        t.set_observations(rec_[:, 0].astype(np.int32), rec_[:, -2:], start_)
        t.set_consensus(*setting)
        out = handle_result(t)
        t.close()
        return out

    tri = hip_ch.Triangulator(P.shape[0])
    assert tri.get_consensus() == (0, 8.0, 0)
    tri.set_cameras(P, K, D)
    tri.set_observations(srec[:, 0].astype(np.int32), srec[:, -2:], sstart)
    tri.set_consensus(H64, 6.0, 5)
    assert tri.get_consensus() == (H64, 6.0, 5)
    first = handle_result(tri)
    assert_same_result(first, fresh(srec, sstart, H64, 6.0, 5), "first")
    # a refused setting keeps the previous one
    for bad in ((257, 8.0, 0), (-1, 8.0, 0), (64, 0.0, 0), (64, float("nan"), 0)):
        with pytest.raises(_capi.PcsError) as ex:
            tri._call("pcs_tri_set_consensus", tri._h, *bad)
        assert ex.value.code == _capi.PCS_ERR_ARG
    assert tri.get_consensus() == (H64, 6.0, 5)
    # plain: the plain bits, and no consensus results
    tri.set_consensus(0)
    plain = handle_result(tri)
    assert plain.inliers is None
    assert_same_result(plain, fresh(srec, sstart), "plain after consensus")
    with pytest.raises(_capi.PcsError) as ex:
        tri.consensus_results()
    assert ex.value.code == _capi.PCS_ERR_STATE
    # consensus on a larger table: the setting survives new observations, the buffers grow
    tri.set_consensus(**inp.CONSENSUS)
    tri.set_observations(cam, rec[:, -2:], start)
    assert tri.get_consensus() == (H64, 8.0, 0)
    host = handle_result(tri)
    assert_same_result(host, fresh(rec, start, H64, 8.0, 0), "larger table")
    assert tri.last_kernel_ms() > 0.0 and tri.last_refine_ms() > 0.0
    # device-resident observations
    d_cam, d_uv = torch.from_numpy(cam).cuda(), torch.from_numpy(np.ascontiguousarray(rec[:, -2:])).cuda()
    d_st = torch.from_numpy(np.array(start, dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    tri.set_observations_device(rec.shape[0], d_cam.data_ptr(), d_uv.data_ptr(), len(start) - 1, d_st.data_ptr())
    assert_same_result(handle_result(tri), host, "device-resident")
    # the grouping on the device: the rig's table is grouped by feature and every feature kept
    ids = rec[:, 1:-2].astype(np.int64)
    feat = np.ravel_multi_index(ids.T, ids.max(axis=0) + 1).astype(np.int32)
    d_feat = torch.from_numpy(feat).cuda()
    torch.cuda.synchronize()
    n_pts, n_kept, grouped = tri.group_table_device(rec.shape[0], d_cam.data_ptr(), d_feat.data_ptr(), d_uv.data_ptr(), int(feat.max()) + 1)
    assert grouped and n_pts == len(start) - 1 and n_kept == rec.shape[0]
    assert_same_result(handle_result(tri), host, "grouped on the device")
    tri.close()


def test_front_end_on_both_grouping_paths_and_with_a_loss():
    _, start, P, K, D, _ = inp.clean_rig("tri-perm")
    rec, clean = inp.corrupted_rig("tri-perm")
    kw = dict(consensus=H64, inlier_px=8.0, seed=0)
    want = refine(rec, start, P, K, D, H64)
    got = hip_ch.multi_cam_triangulate(rec, P, K, D, refine=True, return_result=True, return_residuals=True, **kw)
    assert_same_result(got, want, "device grouping")
    rows = inp.many_views(start)
    assert np.array_equal(got.inliers[rows], clean[rows])
    assert np.array_equal(hip_ch.multi_cam_triangulate(rec, P, K, D, **kw), want.points_dlt)
    dlt_only = hip_ch.multi_cam_triangulate(rec, P, K, D, return_result=True, **kw)
    assert np.array_equal(dlt_only.points, want.points_dlt) and np.array_equal(dlt_only.inliers, want.inliers)
    # a table that is not grouped by feature: the host grouping, then the same stage
    dd = rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]
    rec2, start2 = hip_ch.group_reconstructable(dd)
    a = hip_ch.multi_cam_triangulate(dd, P, K, D, refine=True, return_result=True, return_residuals=True, **kw)
    assert_same_result(a, refine(rec2, start2, P, K, D, H64), "host grouping")
    assert a.inliers is not None and a.inliers.shape == (rec2.shape[0],)
    # loss= and consensus= combine: the robust refinement of the kept rows
    many = np.diff(start) >= inp.MIN_VIEWS_CHECKED
    both = refine(rec, start, P, K, D, H64, loss="huber", f_scale=1.0)
    drec, dstart = inp.deleted_table(rec, start, clean | ~rows)
    robust = refine(drec, dstart, P, K, D, loss="huber", f_scale=1.0)
    assert_same_points(both, robust, many, many, "loss and consensus")
    assert np.array_equal(both.cost[many], robust.cost[many]) and np.array_equal(both.inliers, want.inliers)
    assert not np.array_equal(both.points[many], want.points[many])
    # the stage stays off where it is not asked for: the shared handle states its setting on every call
    assert hip_ch.refine_triangulation(rec, P, start, K, D).inliers is None
