"""Every triangulation kernel the library can launch (csrc/ba_triangulate.hpp), at its own limits.

pcs_tri_create reads PCS_TRI_LANES, PCS_TRI_VARIANT and PCS_TRI_NO_SORT; pcs_tri_run dispatches on them to eleven instantiations:
triangulate_kernel<1|2|4|8|16> (every view in the global scratch) and triangulate_reg_kernel<1,8>, <2,8>, <4,6>, <4,8>, <8,8>, <16,8>
(G lanes per point, V views per lane in registers, the rest in the scratch).  The other test files run <4,6> with sorted points only.
Here every test sets the switches, constructs its own Triangulator (nb_triangulate_full caches a handle) and first asserts
``launch_config()``, so that a misspelt switch cannot test the default eleven times.

One boundary table, built once: 260 cameras, 300 points whose view counts are every G V of the eleven kernels (8, 16, 24, 32, 64, 128)
with both neighbours, 2..5 views, and 255, 256, 257, 260 views — the last bucket of the visiting order (tri_order_*_kernel clamps at
255).  300 points end in a wave that mixes live and dead groups for G = 1, 2, 4, 8; at G = 16 they fill 75 waves and a wholly dead
wave follows (the six-point table of the tests below ends in a mixed wave for every G).  The measurement noise stays on: on
noise-free data a dropped view moves no point.

Tolerance: the rule of tests/test_gpu_triangulate.py (svd_tolerances).  On this table every point with at least four views sits at the
rule's 1e-10 floor and the worst point at 2e-9, asserted as conditions of the input, so the conditioning bound cannot hide a failure."""
import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import synthetic
from pycamset_amd import compiled_helpers as hip_ch
from tests import tri_refine_reference as ref
from tests.test_gpu_tri_refine import assert_matches_reference
from tests.test_gpu_triangulate import svd_tolerances

pytestmark = pytest.mark.gpu

SWITCHES = ("PCS_TRI_LANES", "PCS_TRI_VARIANT", "PCS_TRI_NO_SORT")
SCRATCH = [(1, 0), (2, 0), (4, 0), (8, 0), (16, 0)]
REGISTER = [(1, 1), (2, 1), (4, 1), (4, 3), (8, 1), (16, 1)]
VARIANTS = SCRATCH + REGISTER
COUNTS = [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260]
N_CAMS = 260
REFINE_FIELDS = ("points", "points_dlt", "rms", "rms_dlt", "n_views", "iterations", "status", "residuals")


def expected_config(lanes, variant, no_sort=False):
    """(lanes, register views per lane, register kernel, sorted) as pcs_tri_launch_config reports them."""
    if variant == 0:
        return (lanes, 0, 0, 0)
    return (lanes, 6 if (lanes == 4 and variant != 3) else 8, 1, 0 if no_sort else 1)


def make_handle(monkeypatch, lanes=None, variant=None, no_sort=False, n_cams=N_CAMS):
    """A Triangulator created under the given switches (None: unset); what it will launch is asserted before it is returned."""
    for name, value in zip(SWITCHES, (lanes, variant, 1 if no_sort else None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    tri = hip_ch.Triangulator(n_cams)
    want = expected_config(4 if lanes is None else lanes, 1 if variant is None else variant, no_sort)
    assert tri.launch_config() == want, (lanes, variant, no_sort, tri.launch_config())
    return tri


def run_dlt(tri, t, rec=None, start=None, D=None):
    rec = t["rec"] if rec is None else rec
    start = t["start"] if start is None else start
    tri.set_cameras(t["P"], t["K"], t["D"] if D is None else D)
    tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
    tri.run()
    return tri.points()


@pytest.fixture(scope="module")
def table():
    """The boundary table, its oracle points (with and without distortion) and its per-point tolerances; read-only."""
    rig = synthetic.make_rig("tri-variants", N_CAMS, 2, synthetic.ccube_points(6, 30.0), seed=300, visibility=1.0, n_rings=2)
    im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
    d = rig.detections
    feature = d[:, 1].astype(np.int64) * rig.n_keys + d[:, 2].astype(np.int64)
    n_features = rig.n_imgs * rig.n_keys
    rng = np.random.default_rng(1)
    keep_cams = np.zeros((n_features, N_CAMS), dtype=bool)
    for f in range(n_features):                                    # feature order, one generator
        keep_cams[f, rng.permutation(N_CAMS)[:COUNTS[f % len(COUNTS)]]] = True
    d = d[keep_cams[feature, d[:, 0].astype(np.int64)]]
    d = d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))]                 # (image, key, camera)
    rec, start = hip_ch.group_reconstructable(d)
    views = np.diff(start)
    assert start.shape[0] - 1 == 300 and rec.shape[0] == 20106
    assert sorted(set(views.tolist())) == COUNTS
    for lanes, variant in REGISTER:                                # every register/scratch cut with its neighbours on both sides
        cut = lanes * expected_config(lanes, variant)[1]
        assert {cut - 1, cut, cut + 1} <= set(views.tolist()), (lanes, variant)
    assert (views > 255).sum() >= 2 and (views >= 255).sum() >= 4  # the clamped bucket of the visiting order
    for lanes in (1, 2, 4, 8):                                     # the last live wave mixes live and dead groups; at 16 lanes the 300
        assert (300 * lanes) % 64 != 0                             # points fill 75 waves and a whole dead wave follows (the six-point
    assert (300 * 16) % 256 != 0                                   # table below ends in a mixed wave at 16 lanes too)
    tol = svd_tolerances(rec, start, P, K, D)
    assert tol[views >= 4].max() == 1e-10
    assert tol.max() <= 2e-9
    t = {"rig": rig, "rec": rec, "start": start, "views": views, "P": P, "K": K, "D": D, "tol": tol,
         "ref": orc.triangulate_full(rec, P, start, K, D), "ref0": orc.triangulate_full(rec, P, start, K, np.zeros_like(D))}
    for a in (rec, start, views, tol, t["ref"], t["ref0"]):
        a.setflags(write=False)
    return t


_dlt_points = {}   # (lanes, variant) -> the points of the sorted run on the boundary table, shared between the tests


def dlt_points(monkeypatch, table, lanes, variant):
    key = (lanes, variant)
    if key not in _dlt_points:
        tri = make_handle(monkeypatch, lanes, variant)
        _dlt_points[key] = run_dlt(tri, table)
        tri.close()
    return _dlt_points[key]


def rel_err(pts, want):
    return np.linalg.norm(pts - want, axis=1) / np.linalg.norm(want, axis=1)


def config_under(monkeypatch, lanes=None, variant=None, no_sort=None):
    """launch_config() of a handle created with the switches set to these strings (None: unset)."""
    for name, value in zip(SWITCHES, (lanes, variant, no_sort)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    tri = hip_ch.Triangulator(3)
    cfg = tri.launch_config()
    tri.close()
    return cfg


def test_switches_select_the_kernel_and_invalid_values_fall_back(monkeypatch):
    assert config_under(monkeypatch) == (4, 6, 1, 1)
    assert config_under(monkeypatch, no_sort="1") == (4, 6, 1, 0)
    for lanes, variant in VARIANTS:
        for no_sort in (False, True):
            assert config_under(monkeypatch, str(lanes), str(variant), "1" if no_sort else None) == expected_config(lanes, variant, no_sort)
    for bad in ("3", "0", "32", "-4", "four", ""):                 # not a lane count: the default geometry
        assert config_under(monkeypatch, lanes=bad) == (4, 6, 1, 1), bad
    for variant in ("2", "3", "7"):                                # eight register views at every lane count but four
        assert config_under(monkeypatch, "8", variant) == (8, 8, 1, 1), variant
    assert config_under(monkeypatch, "4", "7") == (4, 6, 1, 1)     # not a variant: the default
    assert config_under(monkeypatch, "3", "0") == (4, 0, 0, 0)


@pytest.mark.parametrize("lanes,variant", VARIANTS)
def test_variant_matches_svd_oracle(monkeypatch, table, lanes, variant):
    t = table
    pts = dlt_points(monkeypatch, t, lanes, variant)
    tri = make_handle(monkeypatch, lanes, variant)
    pts0 = run_dlt(tri, t, D=np.zeros_like(t["D"]))                # distortion switched off, at 10 * tol like the existing test
    tri.close()
    ratio, ratio0 = rel_err(pts, t["ref"]) / t["tol"], rel_err(pts0, t["ref0"]) / (10 * t["tol"])
    for n in COUNTS:
        sel = t["views"] == n
        print(f"tri-variant G={lanes} variant={variant} views={n}: worst err/tol {ratio[sel].max():.3e}, without distortion {ratio0[sel].max():.3e}")
    assert np.all(ratio <= 1.0), (float(ratio.max()), int(t["views"][np.argmax(ratio)]))
    assert np.all(ratio0 <= 1.0), (float(ratio0.max()), int(t["views"][np.argmax(ratio0)]))


def test_variants_agree_with_each_other(monkeypatch, table):
    """Measured, not bounded beyond what parity implies: two results within tol of the oracle differ by at most 2 tol."""
    t = table
    well = t["views"] >= 4
    pts = {v: dlt_points(monkeypatch, t, *v) for v in VARIANTS}
    worst = (0.0, None, None)
    for i, a in enumerate(VARIANTS):
        for b in VARIANTS[i + 1:]:
            diff = float(rel_err(pts[a][well], pts[b][well]).max())
            if diff > worst[0]:
                worst = (diff, a, b)
    print(f"tri-variant largest relative difference between two variants (>= 4 views): {worst[0]:.3e} between {worst[1]} and {worst[2]}")
    assert worst[0] <= 2e-10


@pytest.mark.parametrize("lanes,variant", VARIANTS)
def test_points_do_not_depend_on_their_neighbours(monkeypatch, table, lanes, variant):
    t = table
    rec, start = t["rec"], t["start"]
    pts = dlt_points(monkeypatch, t, lanes, variant)
    tri = make_handle(monkeypatch, lanes, variant)
    assert np.array_equal(run_dlt(tri, t), pts)
    tri.run()                                                      # a second run on the same handle and observations
    assert np.array_equal(tri.points(), pts)
    perm = np.random.default_rng(2).permutation(len(start) - 1)
    rows = np.concatenate([np.arange(start[j], start[j + 1]) for j in perm])
    pstart = np.append(0, np.cumsum(t["views"][perm]))
    assert np.array_equal(run_dlt(tri, t, rec[rows], pstart), pts[perm])
    tri.close()
    if variant != 0:                                               # table order: a wave mixes 2-view and 260-view points
        tri = make_handle(monkeypatch, lanes, variant, no_sort=True)
        assert np.array_equal(run_dlt(tri, t), pts)
        tri.run()
        assert np.array_equal(tri.points(), pts)
        assert np.array_equal(run_dlt(tri, t, rec[rows], pstart), pts[perm])
        tri.close()


def refine_on(tri, t, rec=None, start=None):
    run_dlt(tri, t, rec, start)
    tri.refine(residuals=True)
    return tri.refined()


def test_refinement_without_the_order_array(monkeypatch, table):
    """triangulate_refine_kernel<4,6> walks the points in the run's order; without one (PCS_TRI_NO_SORT) every output has the bits of the
    default handle's."""
    t = table
    tri = make_handle(monkeypatch)
    want = refine_on(tri, t)
    tri.close()
    tri = make_handle(monkeypatch, no_sort=True)
    got = refine_on(tri, t)
    tri.close()
    assert np.array_equal(want.n_views, t["views"])
    for f in REFINE_FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


def test_refinement_after_a_scratch_kernel_run(monkeypatch, table):
    """The refinement of a handle whose run never builds a visiting order (PCS_TRI_VARIANT=0), against the NumPy restatement under the
    rules of tests/test_gpu_tri_refine.py; two points of every view count."""
    t = table
    rec, start, P, K, D = t["rec"], t["start"], t["P"], t["K"], t["D"]
    tri = make_handle(monkeypatch, 4, 0)
    res = refine_on(tri, t)
    tri.close()
    assert np.array_equal(res.points_dlt, dlt_points(monkeypatch, t, 4, 0))
    assert np.array_equal(res.n_views, t["views"])
    assert np.all(res.rms <= res.rms_dlt)
    assert np.all(np.isin(res.status, [hip_ch.TRI_CONVERGED, hip_ch.TRI_MAX_ITER, hip_ch.TRI_NO_DECREASE]))
    sel = np.concatenate([np.flatnonzero(t["views"] == n)[:2] for n in COUNTS])
    for j in sel:
        rows = rec[start[j]:start[j + 1]]
        r_np = ref.rms(res.points_dlt[j], rows[:, 0].astype(int), rows[:, -2:], P, K, D)
        assert abs(res.rms_dlt[j] - r_np) <= 1e-12 * r_np + 1e-12
        r, _ = ref.residuals(res.points[j], rows[:, 0].astype(int), rows[:, -2:], P, K, D)
        assert np.max(np.abs(res.residuals[start[j]:start[j + 1]] - r)) <= 1e-9
    assert_matches_reference(res, rec, start, P, K, D, sel)


# ---- fewer than two views -------------------------------------------------------------------------------------------------------------
FEW_VIEWS = [2, 0, 1, 3, 2, 0]   # a point without views in the middle, one with a single view, one without views whose start is n_obs
FEW_GOOD, FEW_BAD = [0, 3, 4], [1, 2, 5]


def few_view_tables(t):
    """The six-point table (rows of six features of the boundary table, cut to FEW_VIEWS) and the table of its three good points alone."""
    rec, start = t["rec"], t["start"]
    src = np.flatnonzero(t["views"] >= 3)[:6]
    rows = [rec[start[j]:start[j] + n] for j, n in zip(src, FEW_VIEWS)]
    six = (np.concatenate(rows), np.append(0, np.cumsum(FEW_VIEWS)))
    own = (np.concatenate([rows[k] for k in FEW_GOOD]), np.append(0, np.cumsum([FEW_VIEWS[k] for k in FEW_GOOD])))
    assert six[1][-1] == six[0].shape[0] == 8 and six[1][5] == six[1][6]
    return six, own


@pytest.mark.parametrize("lanes,variant", VARIANTS)
def test_fewer_than_two_views_give_nan_and_disturb_nobody(monkeypatch, table, lanes, variant):
    import torch
    t = table
    (rec6, start6), (rec3, start3) = few_view_tables(t)
    for no_sort in ([False] if variant == 0 else [False, True]):
        tri = make_handle(monkeypatch, lanes, variant, no_sort=no_sort)
        want = run_dlt(tri, t, rec3, start3)
        assert np.isfinite(want).all()
        pts = run_dlt(tri, t, rec6, start6)
        assert np.array_equal(pts[FEW_GOOD], want) and np.isnan(pts[FEW_BAD]).all()
        # caller tensors of exactly n_obs elements: nothing behind the last observation belongs to the table
        d_cam = torch.from_numpy(rec6[:, 0].astype(np.int32)).cuda()
        d_uv = torch.from_numpy(np.ascontiguousarray(rec6[:, -2:])).cuda()
        d_start = torch.from_numpy(np.ascontiguousarray(start6, dtype=np.int64)).cuda()
        assert d_cam.numel() == 8 and d_uv.numel() == 16
        torch.cuda.synchronize()
        tri.set_observations_device(8, d_cam.data_ptr(), d_uv.data_ptr(), 6, d_start.data_ptr())
        tri.run()
        dev = tri.points()
        assert np.array_equal(dev[FEW_GOOD], want) and np.isnan(dev[FEW_BAD]).all()
        tri.close()


def test_fewer_than_two_views_are_not_refined(monkeypatch, table):
    t = table
    (rec6, start6), (rec3, start3) = few_view_tables(t)
    tri = make_handle(monkeypatch)
    want = refine_on(tri, t, rec3, start3)
    got = refine_on(tri, t, rec6, start6)
    tri.close()
    assert np.array_equal(got.n_views, FEW_VIEWS)
    assert np.all(got.status[FEW_BAD] == hip_ch.TRI_NOT_REFINED) and np.all(got.iterations[FEW_BAD] == 0)
    assert np.isnan(got.points[FEW_BAD]).all() and np.isnan(got.points_dlt[FEW_BAD]).all()
    assert np.isnan(got.rms[FEW_BAD]).all() and np.isnan(got.rms_dlt[FEW_BAD]).all()
    assert np.isnan(got.residuals[start6[2]]).all()                # the single view of point 2
    for f in REFINE_FIELDS[:-1]:
        assert np.array_equal(getattr(got, f)[FEW_GOOD], getattr(want, f)), f
    good_rows = np.concatenate([np.arange(start6[k], start6[k + 1]) for k in FEW_GOOD])
    assert np.array_equal(got.residuals[good_rows], want.residuals)
    assert np.all(want.status != hip_ch.TRI_NOT_REFINED)
