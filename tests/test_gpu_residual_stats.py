"""The per-group residual statistics on the GPU (include/pcs_hip.h pcs_stats_*, csrc/ba_groupstats.hpp) against their NumPy restatement
(tests/stats_reference.py, pinned to a case worked by hand in tests/test_stats_reference.py).

Tolerances.  count, n_nonfinite, argmax, max_e, median and mad are compared BIT FOR BIT with the restatement applied to the device's own
error array e, which separates the selection from the rounding of e.  e itself agrees with np.hypot within 4 * 2^-53 * e: two squares,
one sum and one root, each correctly rounded, against a correctly rounded result.  A sum over n finite rows whose absolute terms add up
to S agrees within (n - 1) * 2^-52 * S: two summation orders, each off by at most (n - 1) * 2^-53 * S."""
import numpy as np
import pytest

from pycamset_amd import _capi, diagnostics, handlers, synthetic
from pycamset_amd.detections import TargetDetection
from pycamset_amd.optimisation_handling import mean_reprojection_error
from tests import stats_reference as ref
from tests.test_pnp_reference import DuckCamset, DuckTarget

pytestmark = pytest.mark.gpu

EXACT = ("count", "n_nonfinite", "argmax", "max_e", "median", "mad")
SUMS = ("sum_e", "sum_e2", "sum_ru", "sum_rv")


def same_bits(a, b):
    """Equal as bit patterns; a NaN equals a NaN whatever its payload."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def device_stats(cam, img, key, resid, counts):
    """-> ({grouping: {field: (groups,)}}, e (n,), the handle) of one run on a device copy of ``resid`` (n, 2)."""
    import torch

    st = diagnostics.ResidualStats(*counts)
    st.set_groups(cam, img, key)
    d_resid = torch.from_numpy(np.ascontiguousarray(resid, dtype=np.float64)).cuda()
    st.run(d_resid.data_ptr())
    out = fetch(st)
    e = st.errors()
    st._resid = d_resid   # the run's input lives as long as the handle
    return out, e, st


def fetch(st):
    out = {}
    for grouping in ref.GROUPINGS:
        g = st.results(grouping)
        out[grouping] = {f: np.asarray(getattr(g, "max" if f == "max_e" else f)).reshape(-1) for f in ref.FIELDS}
    return out


def assert_matches(dev, e_dev, cam, img, key, resid, counts, rows=None):
    """The checks of the module docstring.  ``rows``: the table rows the restatement's row numbers stand for (a table with rows deleted)."""
    want = ref.all_group_stats(resid, cam, img, key, counts, e=e_dev)
    for grouping in ref.GROUPINGS:
        d, w = dev[grouping], want[grouping]
        for f in EXACT:
            wf = w[f]
            if f == "argmax" and rows is not None:
                wf = np.where(wf >= 0, rows[np.maximum(wf, 0)], -1)
            assert same_bits(d[f], wf), (grouping, f, d[f], wf)
        for k, f in enumerate(SUMS):
            bound = np.maximum(w["count"] - 1, 0) * 2.0 ** -52 * w["abs"][k]
            err = np.abs(d[f] - w[f])
            print(f"{grouping:8s} {f:7s} worst error / bound {np.max(err / np.where(bound > 0, bound, 1)):.3f}, zero-bound groups off by {err[bound == 0].max(initial=0.0):.1e}")
            assert np.all(err <= bound), (grouping, f, err, bound)


def assert_errors_match(e_dev, resid):
    h = ref.errors(resid)
    fin = np.isfinite(h)
    assert np.array_equal(fin, np.isfinite(e_dev))
    rel = np.abs(e_dev[fin] - h[fin]) / np.where(h[fin] > 0, h[fin], 1)
    print(f"e against np.hypot: worst {rel.max(initial=0.0) / 2.0 ** -53:.2f} * 2^-53")
    assert np.all(np.abs(e_dev[fin] - h[fin]) <= 4 * 2.0 ** -53 * h[fin])


# ---- the boundary table --------------------------------------------------------------------------------------------------------------
COUNTS = (3, 5, 70)
VIEW_SIZES = [[0, 1, 2, 3, 63], [64, 65, 7, 10, 70], [0, 0, 0, 0, 0]]   # camera 2 has no rows at all
EQUAL_VIEW, TIE_VIEW = (1, 2), (1, 3)


def boundary_table(seed=0):
    """285 rows (not a multiple of 64) in shuffled order: view sizes 0, 1, 2, 3 (empty, odd, even), 63, 64, 65 (the wave boundary) and
    70; one view with all errors equal (MAD 0); duplicated error values everywhere, and in one view the LARGEST error of its camera, of
    its image and of the table twice (ties of argmax)."""
    rng = np.random.default_rng(seed)
    cam, img, key = [], [], []
    for c, sizes in enumerate(VIEW_SIZES):
        for i, n in enumerate(sizes):
            cam += [c] * n
            img += [i] * n
            key += list(rng.permutation(COUNTS[2])[:n])
    cam, img, key = (np.array(a, dtype=np.int32) for a in (cam, img, key))
    n = cam.shape[0]
    resid = rng.normal(0.0, 0.4, (n, 2))
    dup = rng.permutation(n)[:60]
    resid[dup[:30]] = resid[dup[30:]]                                 # thirty pairs of equal errors
    equal = np.nonzero((cam == EQUAL_VIEW[0]) & (img == EQUAL_VIEW[1]))[0]
    resid[equal] = [[3, 4], [-3, 4], [4, 3], [5, 0], [0, -5], [-4, -3], [3, -4]]   # all of them e = 5 exactly
    tie = np.nonzero((cam == TIE_VIEW[0]) & (img == TIE_VIEW[1]))[0]
    resid[tie[[2, 7]]] = [[30, 40], [-40, 30]]                        # e = 50 twice
    order = rng.permutation(n)
    return cam[order], img[order], key[order], resid[order]


@pytest.fixture(scope="module")
def boundary():
    cam, img, key, resid = boundary_table()
    dev, e, st = device_stats(cam, img, key, resid, COUNTS)
    return dict(cam=cam, img=img, key=key, resid=resid, dev=dev, e=e, st=st)


def test_boundary_table_matches_the_restatement(boundary):
    b = boundary
    assert b["cam"].shape[0] == 285 and b["cam"].shape[0] % 64
    assert not np.all(np.diff(b["cam"].astype(np.int64) * 5 + b["img"]) >= 0)   # the rows are not grouped
    assert_errors_match(b["e"], b["resid"])
    assert_matches(b["dev"], b["e"], b["cam"], b["img"], b["key"], b["resid"], COUNTS)
    view = b["st"].results("view")
    assert view.count.shape == (3, 5) and np.array_equal(view.count, VIEW_SIZES)
    assert np.all(np.isnan(view.median[2])) and np.all(view.argmax[2] == -1) and np.isnan(view.rms[0, 0])
    assert view.mad[EQUAL_VIEW] == 0.0 and view.median[EQUAL_VIEW] == 5.0
    # the largest error is there twice: the lower row wins in every group that holds both
    both = np.nonzero(b["e"] == 50.0)[0]
    assert both.shape == (2,)
    for grouping, g in (("view", TIE_VIEW[0] * 5 + TIE_VIEW[1]), ("camera", TIE_VIEW[0]), ("image", TIE_VIEW[1]), ("overall", 0)):
        assert b["dev"][grouping]["argmax"][g] == both.min() and b["dev"][grouping]["max_e"][g] == 50.0


def test_two_runs_give_the_same_bits(boundary):
    b = boundary
    b["st"].run(b["st"]._resid.data_ptr())
    again, e = fetch(b["st"]), b["st"].errors()
    assert same_bits(e, b["e"])
    for grouping in ref.GROUPINGS:
        for f in ref.FIELDS:
            assert same_bits(again[grouping][f], b["dev"][grouping][f]), (grouping, f)


def test_row_order_does_not_change_the_order_statistics(boundary):
    b = boundary
    order = np.random.default_rng(99).permutation(b["cam"].shape[0])
    dev, e, _ = device_stats(b["cam"][order], b["img"][order], b["key"][order], b["resid"][order], COUNTS)
    assert same_bits(e, b["e"][order])
    for grouping in ref.GROUPINGS:
        for f in ("count", "n_nonfinite", "max_e", "median", "mad"):
            assert same_bits(dev[grouping][f], b["dev"][grouping][f]), (grouping, f)
        worst = dev[grouping]["argmax"]
        assert same_bits(np.where(worst >= 0, e[np.maximum(worst, 0)], np.nan), b["dev"][grouping]["max_e"])   # one of the equal maxima


def test_a_single_row():
    cam, img, key = (np.array([v], dtype=np.int32) for v in (1, 4, 69))
    resid = np.array([[-0.3, 0.4]])
    dev, e, st = device_stats(cam, img, key, resid, COUNTS)
    assert_errors_match(e, resid)
    assert_matches(dev, e, cam, img, key, resid, COUNTS)
    assert dev["overall"]["count"][0] == 1 and dev["overall"]["mad"][0] == 0.0 and dev["overall"]["median"][0] == e[0]
    assert dev["camera"]["count"].tolist() == [0, 1, 0] and np.isnan(dev["camera"]["median"][0])
    index_ms, error_ms, stats_ms = st.last_kernel_ms()
    assert index_ms > 0 and error_ms >= 0 and stats_ms > 0   # several launches; the error kernel alone may be below the clock's step


def test_one_long_group():
    """20 011 rows, 9 001 of them in camera 0 and all of them in the overall group: a group spans many strides of its workgroup, and
    the sort many chunks."""
    rng = np.random.default_rng(3)
    n, counts = 20011, (2, 3, 50)
    cam = (rng.permutation(n) >= 9001).astype(np.int32)
    img, key = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    resid = rng.normal(0.0, 0.5, (n, 2))
    resid[rng.permutation(n)[:500]] = resid[rng.permutation(n)[:500]]   # equal errors, some of them around the median
    dev, e, _ = device_stats(cam, img, key, resid, counts)
    assert dev["camera"]["count"].tolist() == [9001, 11010]
    assert_errors_match(e, resid)
    assert_matches(dev, e, cam, img, key, resid, counts)


def test_non_finite_rows_are_counted_and_left_out(boundary):
    b = boundary
    cam, img, key, resid = b["cam"], b["img"], b["key"], b["resid"].copy()
    n = cam.shape[0]
    single = int(np.nonzero((cam == 0) & (img == 1))[0][0])            # the only row of its view: the view becomes empty
    full = np.nonzero((cam == 1) & (img == 0))[0]                      # the 64-row view: 61 rows are left
    bad = np.array([single, full[0], full[10], full[63], int(np.nonzero((cam == 1) & (img == 4))[0][5])])
    resid[bad] = [[np.nan, 0.1], [np.inf, 0.2], [0.3, -np.inf], [np.nan, np.nan], [1e200, 1e200]]   # the last one: e overflows
    dev, e, _ = device_stats(cam, img, key, resid, COUNTS)
    assert not np.any(np.isfinite(e[bad])) and np.all(np.isfinite(np.delete(e, bad)))
    kept = np.setdiff1d(np.arange(n), bad)
    # every statistic but n_nonfinite is that of the table without those rows ...
    want_bad = ref.all_group_stats(resid, cam, img, key, COUNTS, e=e)
    for grouping in ref.GROUPINGS:
        assert np.array_equal(dev[grouping]["n_nonfinite"], want_bad[grouping]["n_nonfinite"]), grouping
        dev[grouping]["n_nonfinite"][:] = 0
    assert_matches(dev, e[kept], cam[kept], img[kept], key[kept], resid[kept], COUNTS, rows=kept)
    # ... and the counts are these
    assert want_bad["overall"]["n_nonfinite"][0] == 5 and dev["overall"]["count"][0] == n - 5
    assert dev["view"]["count"][0 * 5 + 1] == 0 and dev["view"]["argmax"][0 * 5 + 1] == -1 and np.isnan(dev["view"]["median"][0 * 5 + 1])
    assert dev["view"]["count"][1 * 5 + 0] == 61 and want_bad["view"]["n_nonfinite"][1 * 5 + 0] == 3


# ---- through the engine --------------------------------------------------------------------------------------------------------------
def small_problem(outliers=None, planted=None):
    """Config 1's geometry with 8 images (3 cameras, the cube target at visibility 0.2, 0.3 px noise): 2 322 detections."""
    rig = synthetic.config_rig(1, n_imgs=8)
    det = rig.detections.copy()
    if planted is not None:
        det[det[:, 1] == planted, 3:] += PLANTED_OFFSET
    td = TargetDetection([f"cam_{i}" for i in range(rig.n_cams)], det)
    h = handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), td, options=None if outliers is None else {"outliers": outliers})
    x_true = np.concatenate([rig.intr_true.ravel(), rig.extr_true.ravel(), rig.poses_true[1:].ravel()])   # pose 0 is fixed at zero
    return rig, h, x_true


def assert_report_matches(report, table, resid, counts):
    resid = np.asarray(resid, dtype=np.float64).reshape(-1, 2)
    cam, img, key = (table[:, k].astype(np.int64) for k in range(3))
    e = report.errors()
    assert report.n == table.shape[0] == e.shape[0]
    assert_errors_match(e, resid)
    dev = {}
    for grouping, g in zip(ref.GROUPINGS, (report.per_camera, report.per_image, report.per_key, report.per_view, report.overall)):
        dev[grouping] = {f: np.asarray(getattr(g, "max" if f == "max_e" else f)).reshape(-1) for f in ref.FIELDS}
    assert_matches(dev, e, cam, img, key, resid, counts)
    want = ref.all_group_stats(resid, cam, img, key, counts, e=e)
    s, n = want["overall"], int(want["overall"]["count"][0])
    # overall.mean is mean_reprojection_error's figure: the same sum in another order, over n
    assert abs(report.overall.mean[0] - mean_reprojection_error(resid.reshape(-1))) <= (n - 1) * 2.0 ** -52 * s["abs"][0, 0] / n
    assert same_bits(report.per_view.rms, np.sqrt(np.where(want["view"]["count"] > 0, report.per_view.sum_e2.reshape(-1) / np.maximum(want["view"]["count"], 1), np.nan)))
    worst = report.worst(5)
    assert worst[0] == report.overall.argmax[0] and np.all(np.diff(e[worst]) <= 0) and e[worst[-1]] >= np.sort(e)[-5]


def test_report_of_a_template_handler_at_the_truth():
    rig, h, x = small_problem()
    report = diagnostics.reprojection_report(h, x)
    resid = h.make_loss_fun()(x)
    assert_report_matches(report, h._flat_detections(), resid, (rig.n_cams, rig.n_imgs, rig.n_keys))
    assert report.per_view.rms.shape == (rig.n_cams, rig.n_imgs)
    assert 0.3 < report.overall.mean[0] < 0.45 and report.overall.n_nonfinite[0] == 0       # 0.3 px noise per coordinate
    assert report.outlier_images() is None and report.outlier_views() is None
    with pytest.raises(ValueError, match="device"):
        diagnostics.reprojection_report(h, x, device=h.op_fun.device + 1)
    again = diagnostics.reprojection_report(h, x)                                           # the cached index, the same bits
    assert same_bits(again.per_key.median, report.per_key.median) and same_bits(again.per_view.sum_e, report.per_view.sum_e)
    assert same_bits(again.errors(), report.errors())


def test_report_of_a_chain_problem():
    from pycamset_amd import function_blocks as fb

    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()   # a generated chain
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr_true, rig.extr_true, np.zeros((rig.n_imgs, 6)), rig.poses_true], template=rig.points,
                                 unfixed=[None, fix_ext, np.zeros((rig.n_imgs, 6), dtype=bool), None])
    report = diagnostics.reprojection_report(prob, prob.x0)
    assert_report_matches(report, prob.det, prob.make_loss_fun()(prob.x0), (rig.n_cams, rig.n_imgs, rig.n_keys))
    assert 0.3 < report.overall.mean[0] < 0.45


# ---- a planted outlier ---------------------------------------------------------------------------------------------------------------
# Every detection of image 4 is moved by this many pixels.  With the NumPy oracle's residuals at the truth and the restatement, the MAD
# score |v - median| / MAD of image 4's mean error is 258 and no other image's exceeds 1.3; with the per-image error of the seeding
# (NumPy PnP restatement, the oracle's legacy cost) image 4 scores 227 and no other image more than 3.1.  The threshold is 20.
PLANTED_IMAGE, PLANTED_OFFSET = 4, (3.0, -2.0)


def test_planted_outlier_image_is_found_and_excluded():
    rig, h, x = small_problem(outliers="y", planted=PLANTED_IMAGE)
    report = diagnostics.reprojection_report(h, x)
    scores = ref.mad_score(report.per_image.mean)
    print("MAD scores of the per-image mean error:", np.round(scores, 2))
    assert list(report.outlier_images()) == [PLANTED_IMAGE]
    views = report.outlier_views()
    assert views is not None and set(map(tuple, views)) == {(c, PLANTED_IMAGE) for c in range(rig.n_cams)}
    assert np.all(h._flat_detections()[report.worst(20), 1] == PLANTED_IMAGE)
    # seeding: under "y" the image is marked missing and its rows are dropped ...
    x0 = h.calc_initial_params(rig.intr_true)
    print("MAD scores of the seeding's per-image error:", np.round(ref.mad_score(h.initial_per_im_error), 2))
    assert list(np.nonzero(h.missing_poses)[0]) == [PLANTED_IMAGE]
    left = h.get_detection_data(flatten=True)
    assert not np.any(left[:, 1] == PLANTED_IMAGE) and left.shape[0] == np.count_nonzero(h._flat_detections()[:, 1] != PLANTED_IMAGE)
    # ... under the default and under "n" nothing changes: no image is missing, and the start vector is the same
    for answer in (None, "n"):
        _, hd, _ = small_problem(outliers=answer, planted=PLANTED_IMAGE)
        xd = hd.calc_initial_params(rig.intr_true)
        assert not np.any(hd.missing_poses) and hd.missing_poses.shape == (rig.n_imgs,)
        assert np.array_equal(xd, x0)
        assert hd.get_detection_data(flatten=True).shape[0] == hd._flat_detections().shape[0]


# ---- error codes ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch

    st = diagnostics.ResidualStats(2, 3, 4)
    resid = torch.zeros(6, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(_capi.PcsError) as err:
        st.run(resid.data_ptr())                                      # no groups yet
    assert err.value.code == _capi.PCS_ERR_STATE
    ok = (np.array([0, 1, 1, 0, 1, 0]), np.array([0, 1, 2, 2, 1, 0]), np.array([3, 2, 1, 0, 0, 3]))
    for col, value in ((0, 2), (0, -1), (1, 3), (2, 4)):              # an id outside [0, count), host and device arrays
        ids = [a.copy() for a in ok]
        ids[col][4] = value
        with pytest.raises(_capi.PcsError) as err:
            st.set_groups(*ids)
        assert err.value.code == _capi.PCS_ERR_RANGE and "row 4" in str(err.value)
        d_ids = [torch.from_numpy(a.astype(np.int32)).cuda() for a in ids]
        with pytest.raises(_capi.PcsError) as err:
            st.set_groups_device(6, *(d.data_ptr() for d in d_ids))
        assert err.value.code == _capi.PCS_ERR_RANGE and "row 4" in str(err.value)
        with pytest.raises(_capi.PcsError) as err:
            st.run(resid.data_ptr())                                  # the refused table left no groups behind
        assert err.value.code == _capi.PCS_ERR_STATE
    d_ids = [torch.from_numpy(a.astype(np.int32)).cuda() for a in ok]
    st.set_groups_device(6, *(d.data_ptr() for d in d_ids))
    with pytest.raises(_capi.PcsError) as err:
        st.results("camera")                                          # no run on these groups
    assert err.value.code == _capi.PCS_ERR_STATE
    with pytest.raises(_capi.PcsError) as err:
        st._call("pcs_stats_run", st._h, st._addr(resid.data_ptr()), 2, None, None, None, None)   # an unknown flag
    assert err.value.code == _capi.PCS_ERR_ARG
    # a run that wrote the errors and the values elsewhere: the counts can be fetched, the rest cannot
    e_out = torch.full((6,), -1.0, dtype=torch.float64, device="cuda")
    v_out = torch.full((7, st.n_groups), -1.0, dtype=torch.float64, device="cuda")
    st.run(resid.data_ptr(), d_errors=e_out.data_ptr(), d_values=v_out.data_ptr())
    count = np.empty(2, dtype=np.int32)
    st._call("pcs_stats_results", st._h, 0, st._ptr(count), *([None] * 9))
    assert count.tolist() == [3, 3]
    with pytest.raises(_capi.PcsError) as err:
        st.results("camera")
    assert err.value.code == _capi.PCS_ERR_STATE and "caller" in str(err.value)
    with pytest.raises(_capi.PcsError) as err:
        st.errors()
    assert err.value.code == _capi.PCS_ERR_STATE
    torch.cuda.synchronize()
    assert torch.all(e_out == 0.0) and torch.all(v_out[0] == 0.0)     # all residuals are zero: e = 0, sum_e = 0
    assert float(v_out[5, -1]) == 0.0 and float(v_out[6, -1]) == 0.0  # the overall median and MAD
    # the same run into the handle's own buffers, then without the order statistics
    st.run(resid.data_ptr())
    assert st.results("image").count.tolist() == [2, 2, 2]
    st.run(resid.data_ptr(), order_statistics=False)
    g = st.results("overall")
    assert g.count[0] == 6 and np.isnan(g.median[0]) and np.isnan(g.mad[0]) and g.max[0] == 0.0
    st.close()
