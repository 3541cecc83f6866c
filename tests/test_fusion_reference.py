"""The depth-map fusion without a GPU: the NumPy restatement against itself (tests/fusion_reference.py: loop form, vectorised form,
float64, longdouble), the conditions on the inputs that license the device test's exact comparisons (tests/test_gpu_fusion.py), the
properties of the rule on rendered maps, the neighbour lists against the reference's own ``calc_pairs`` (tests/golden/view_pairs.npz),
and every argument error of ``pycamset_amd.fusion`` and of the C entry points."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from pycamset_amd import _capi, fusion
from tests import fusion_inputs as inp
from tests import fusion_reference as ref

MARGIN = 8.0
GOLDEN = Path(__file__).resolve().parent / "golden" / "view_pairs.npz"
EXACT = ("mask", "count", "support", "status", "counts")


def small():
    D, K, E = inp.ring(5, 24, 16, 7.0, 303, False, 404)
    return dict(depth=D, K=K, ext=E, neighbours=inp.nearest_lists(5, 3))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("opts", [dict(), dict(unique=True, min_views=1, transform=inp.TRANSFORM), dict(px_tol=0.4, rel_tol=0.004, min_views=3)])
def test_loop_and_vectorised_forms_agree_bit_for_bit(dtype, opts):
    a = small()
    v, l = ref.fuse(**a, **opts, dtype=dtype), ref.fuse_loop(**a, **opts, dtype=dtype)
    for k in EXACT:
        assert np.array_equal(v[k], l[k]), k
    for k in ("points", "fused_depth"):
        assert v[k].dtype == np.dtype(dtype) and np.array_equal(v[k], l[k], equal_nan=True), k
    assert v["closest"] == l["closest"] and 0 < v["closest"] < 1
    assert v["mask"].any() and (v["status"] == ref.INVALID_DEPTH).any() and (v["status"] == ref.FEW_VIEWS).any()
    if opts.get("unique"):
        assert (v["status"] == ref.DUPLICATE).any()


def measured_gaps():
    gp = gd = 0.0
    for a, o in inp.gap_inputs():
        r, l = ref.fuse(**a, **o), ref.fuse(**a, **o, dtype=np.longdouble)
        for k in EXACT:
            assert np.array_equal(r[k], l[k]), k
        assert np.array_equal(np.isnan(r["decisions"]), np.isnan(l["decisions"]))
        m = r["mask"].astype(bool)
        if m.any():
            big = float(np.max(np.abs(l["points"][m])))
            gp = max(gp, float(np.max(np.abs(r["points"][m] - l["points"][m]))) / big, float(np.max(np.abs(r["fused_depth"][m] - l["fused_depth"][m]))) / big)
        taken = ~np.isnan(r["decisions"])
        if taken.any():
            gd = max(gd, float(np.max(np.abs(r["decisions"][taken] - l["decisions"][taken]))))
    return gp, gd


def test_fuse_gaps_are_the_pinned_ones():
    gp, gd = measured_gaps()
    print("FUSE_GAP measured", gp, "FUSE_DECISION_GAP measured", gd)
    assert 0.5 * inp.FUSE_GAP <= gp <= inp.FUSE_GAP
    assert 0.5 * inp.FUSE_DECISION_GAP <= gd <= inp.FUSE_DECISION_GAP


@pytest.mark.parametrize("name", list(inp.CASES))
def test_no_decision_of_a_device_input_sits_near_its_threshold(name):
    """What licenses the exact comparison of mask, count, support and status on the device: over every decision the rule takes on this
    input, the distance to the threshold is at least MARGIN x FUSE_DECISION_GAP.  A seed that fails this is replaced HERE."""
    a, o = inp.CASES[name]()
    r = ref.fuse(**a, **o)
    print(name, "closest call", r["closest"], "needed", MARGIN * inp.FUSE_DECISION_GAP)
    assert r["closest"] >= MARGIN * inp.FUSE_DECISION_GAP
    assert np.array_equal(r["counts"], r["mask"].reshape(len(r["mask"]), -1).sum(axis=1))


def test_cases_reach_what_they_are_for():
    out = {n: ref.fuse(**inp.CASES[n]()[0], **inp.CASES[n]()[1]) for n in ("nbr32", "empty_list", "facing", "no_overlap", "unique", "nbr2", "shape_1x1")}
    assert out["nbr32"]["count"].max() == 32 and (out["nbr32"]["support"] == np.uint32(0xFFFFFFFF)).any()
    e = out["empty_list"]
    valid = ref.valid_depth(inp.CASES["empty_list"]()[0]["depth"][4])
    assert np.all(e["status"][4][valid] == ref.FEW_VIEWS) and np.all(e["status"][4][~valid] == ref.INVALID_DEPTH) and e["mask"][3].any()
    f = out["facing"]   # views 0 and 1 never support one another (bit 0 of each is the other); view 2 supports view 0
    assert not (f["support"][0] & 1).any() and not (f["support"][1] & 1).any() and (f["support"][0] & 2).any() and not f["mask"][1].any()
    n = out["no_overlap"]   # only the neighbour that shares the view's part of the plane ever counts
    assert np.all(n["support"][0] & ~np.uint32(1) == 0) and np.all(n["support"][2] & ~np.uint32(1) == 0) and n["mask"].any()
    assert (out["unique"]["status"] == ref.DUPLICATE).any()
    st = out["nbr2"]["status"]
    D = inp.CASES["nbr2"]()[0]["depth"]
    for kind in inp.INVALID_KINDS:   # every kind of invalid depth is among the inputs and gets status 1
        where = np.isnan(D) if kind != kind else D == kind
        assert where.any() and np.all(st[where] == ref.INVALID_DEPTH)
    assert np.all((st == ref.INVALID_DEPTH) == ~ref.valid_depth(D))


def test_noise_free_plane_keeps_what_enough_neighbours_see_and_fuses_onto_the_surface():
    """The plane alone, nothing occluded.  A neighbour SEES the surface point of a pixel when the point lies in front of it and projects
    to a pixel of its map.  Every pixel with at least min_views such neighbours is kept.  The fused point is the mean of surface points
    (the pixel's own and its partners', up to half a pixel of the neighbour apart), so what is true of it is that it lies ON the true
    surface: its distance from the plane is held to MARGIN x FUSE_GAP of the largest coordinate.  (The property as first worded,
    "the fused point is the true surface point", holds only for count = 0; the sphere test below bounds the departure on a curved surface.)"""
    D, K, E = inp.plane_ring()
    V, H, W = D.shape
    nb = inp.nearest_lists(V, 3)
    min_views = 2
    r = ref.fuse(D, K, E, nb, min_views=min_views)
    L = np.longdouble
    xs, ys = np.meshgrid(np.arange(W).astype(L), np.arange(H).astype(L))
    sees = np.zeros((V, H, W), dtype=int)
    for i in range(V):
        X = ref.to_world(K[i].astype(L), E[i].reshape(12).astype(L), xs, ys, D[i].astype(L))
        for j in nb[i]:
            Y = ref.to_view(E[j].reshape(12).astype(L), *X)
            u, v = ref.project(K[j].astype(L), *Y)
            sees[i] += (Y[2] > 0) & (np.floor(u + 0.5) >= 0) & (np.floor(u + 0.5) < W) & (np.floor(v + 0.5) >= 0) & (np.floor(v + 0.5) < H)
    enough = sees >= min_views
    assert enough.sum() > 0.5 * enough.size and (~enough).any()
    assert np.all(r["mask"][enough] == 1)
    assert np.array_equal(r["count"], sees)   # on this scene every neighbour that sees the point agrees with it
    n, h = inp.PLANE
    m = r["mask"].astype(bool)
    P = r["points"][m].astype(L)
    dist = np.abs(P @ n.astype(L) - L(h))
    big = float(np.max(np.abs(P)))
    print("distance from the plane: largest", float(dist.max()), "bound", MARGIN * inp.FUSE_GAP * big)
    assert float(dist.max()) <= MARGIN * inp.FUSE_GAP * big


def test_noise_free_sphere_fused_points_lie_inside_it_by_no_more_than_the_cap_of_what_was_merged():
    """The curved case of the property above.  The fused point is NOT the pixel's own surface point: it is the mean of that point X and
    the partners' X_j, and on a convex surface a mean of surface points lies inside.  How far is bounded by the rule itself.  A
    consistent X_j, seen from view i, has a depth z' within rel_tol z of z and a ray r' within px_tol / min(fx, fy) of the pixel's ray
    r (|r| <= the image corner's), so |X_j - X| = |z' r' - z r| <= c = rel_tol z |r| + (1 + rel_tol) z px_tol / min(fx, fy).  Points of a
    sphere of radius R within a chord c of X all have p . x >= R - c^2 / (2 R) along X's radius x, and so has their mean: the fused
    point lies between the surface and c^2 / (2 R) below it."""
    D, K, E = inp.sphere_ring()
    V, H, W = D.shape
    px_tol, rel_tol = 1.0, 0.01
    L = np.longdouble
    r = ref.fuse(D, K, E, inp.nearest_lists(V, 3), px_tol=px_tol, rel_tol=rel_tol, dtype=L)
    centre, radius = inp.SPHERE
    m = r["mask"].astype(bool)
    below = L(radius) - np.sqrt(np.sum((r["points"][m] - centre.astype(L)) ** 2, axis=1))
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([np.sqrt(1.0 + ((xs - K[i, 1]) / K[i, 0]) ** 2 + ((ys - K[i, 3]) / K[i, 2]) ** 2) for i in range(V)])[m]
    fmin = np.broadcast_to(np.minimum(K[:, 0], K[:, 2])[:, None, None], D.shape)[m]
    c = rel_tol * D[m] * ray + (1.0 + rel_tol) * D[m] * px_tol / fmin
    cap = c * c / (2.0 * radius)
    eps = MARGIN * inp.FUSE_GAP * float(np.max(np.abs(r["points"][m])))
    print("kept", int(m.sum()), "below the surface: smallest", float(below.min()), "largest", float(below.max()), "largest share of the cap", float(np.max(below / cap)),
          "largest cap", float(cap.max()))
    assert m.sum() > 1000 and np.all(below >= -eps) and np.all(below <= cap + eps)
    assert float(below.max()) > 1e3 * eps   # the departure from the pixel's own surface point is real, not rounding


def test_every_pixel_of_a_wrong_depth_patch_is_rejected():
    for noise in (None, 101):
        D, K, E = inp.ring(10, 64, 48, 8.0, noise, True, None)
        r = ref.fuse(D, K, E, inp.nearest_lists(10, 4))
        clean = ref.fuse(inp.ring(10, 64, 48, 8.0, noise, False, None)[0], K, E, inp.nearest_lists(10, 4))
        for v, y0, y1, x0, x1, _ in inp.PATCHES:
            assert not r["mask"][v, y0:y1, x0:x1].any() and np.all(r["status"][v, y0:y1, x0:x1] == ref.FEW_VIEWS)
            assert clean["mask"][v, y0:y1, x0:x1].sum() > 0.5 * (y1 - y0) * (x1 - x0)   # the same pixels pass with their true depth


def test_unique_leaves_no_kept_pixel_with_a_kept_partner_in_a_lower_view():
    a, o = inp.CASES["unique"]()
    plain, uniq = ref.fuse(**a, **dict(o, unique=False)), ref.fuse(**a, **o)
    D, K, E = a["depth"], a["K"], a["ext"].reshape(-1, 12)
    V, H, W = D.shape
    start, nbr = ref.as_csr(a["neighbours"])
    kept3 = plain["mask"].astype(bool)
    assert np.array_equal(uniq["support"], plain["support"]) and np.array_equal(uniq["mask"][0], plain["mask"][0])   # view 0 owns all it keeps
    assert np.all(uniq["mask"] <= plain["mask"]) and uniq["mask"].sum() < plain["mask"].sum()
    checked = 0
    for i, y, x in np.argwhere(kept3):
        X = ref.to_world(K[i], E[i], np.float64(x), np.float64(y), D[i, y, x])
        partner_kept = False
        for k in range(start[i], start[i + 1]):
            j = int(nbr[k])
            if j < i and (int(plain["support"][i, y, x]) >> (k - start[i])) & 1:
                u, v = ref.project(K[j], *ref.to_view(E[j], *X))
                partner_kept |= bool(kept3[j, int(np.floor(v + 0.5)), int(np.floor(u + 0.5))])
        assert bool(uniq["mask"][i, y, x]) == (not partner_kept)
        assert (uniq["status"][i, y, x] == ref.DUPLICATE) == partner_kept
        checked += partner_kept
    assert checked > 100


# ---- neighbour lists ---------------------------------------------------------------------------------------------------------------------------
def test_view_neighbours_equals_the_references_calc_pairs():
    g = np.load(GOLDEN)
    for s, (seed, n, spread, lo, hi, mv) in enumerate(g["sets"]):
        vec, want = g[f"vectors_{s}"], [row[row >= 0] for row in g[f"lists_{s}"]]
        got = fusion.neighbours_of_directions(vec, lo, hi, int(mv))
        assert len(got) == int(n) and all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(got, want)), s
        assert [list(l) for l in got] == ref.view_neighbours(vec, lo, hi, int(mv))
    lens = [len(row[row >= 0]) for row in g["lists_2"]]
    assert min(lens) == 0 and max(lens) == 4   # short lists (index order) and full ones (nearest first) are both among the sets


def test_view_neighbours_takes_the_third_row_and_breaks_ties_to_the_lower_index():
    s, c = np.sin(0.2), np.cos(0.2)
    vec = np.array([[0.0, 0.0, 1.0], [0.0, -s, c], [s, 0.0, c], [-s, 0.0, c], [0.0, s, c]])   # views 1 .. 4 at exactly one angle from view 0
    assert list(fusion.neighbours_of_directions(vec, 3.0, 45.0, 2)[0]) == [1, 2]
    assert list(fusion.neighbours_of_directions(vec, 3.0, 45.0, 4)[0]) == [1, 2, 3, 4]
    assert list(fusion.neighbours_of_directions(vec, 3.0, 45.0, 9)[0]) == [1, 2, 3, 4]
    assert list(fusion.neighbours_of_directions(vec, 12.0, 45.0, 9)[0]) == [] and list(fusion.neighbours_of_directions(vec, 3.0, 11.0, 9)[0]) == []   # strictly inside
    K, E = inp.ring_views(6, 64, 48, 8.0)
    got = fusion.view_neighbours(E, 3.0, 20.0, 9)
    assert [list(l) for l in got] == [list(l) for l in fusion.neighbours_of_directions(E[:, 2, :3], 3.0, 20.0, 9)]
    assert list(got[0]) == [1, 2] and list(got[2]) == [0, 1, 3, 4]
    E4 = np.concatenate([E, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (6, 1, 1))], axis=1)
    assert all(np.array_equal(a, b) for a, b in zip(fusion.view_neighbours(E4, 3.0, 20.0, 9), got))
    for bad in (dict(min_angle=5.0, max_angle=5.0), dict(max_views=0), dict(max_views=33), dict(min_angle=np.nan)):
        with pytest.raises(ValueError, match="min_angle|max_views"):
            fusion.view_neighbours(E, **bad)
    with pytest.raises(ValueError, match="ext"):
        fusion.view_neighbours(E[0])


def test_rectified_view():
    K, E = inp.ring_views(2, 64, 48, 8.0)
    R = inp.look_at((0.3, 0.1, -1.0))[:, :3]
    Kn, P = fusion.rectified_view(E[0], R, [70.0, 31.0, 70.0, 23.0])
    assert np.array_equal(Kn, [70.0, 31.0, 70.0, 23.0]) and np.allclose(P, R @ E[0], atol=0) and P.shape == (3, 4)
    with pytest.raises(ValueError):
        fusion.rectified_view(E[0], R[:2], Kn)


# ---- argument errors: none of them needs a GPU ----------------------------------------------------------------------------------------------
def good():
    K, E = inp.ring_views(3, 8, 6, 8.0)
    return dict(n_views=3, width=8, height=6, K=K, ext=E, neighbours=[[1, 2], [0], []])


@pytest.mark.parametrize("change,name", [
    (dict(n_views=0), "depth"), (dict(width=0), "depth"), (dict(height=65536), "depth"),
    (dict(K=np.ones((2, 4))), "K"), (dict(K=np.array([[1.0, 0, 0.0, 0]] * 3)), "K"), (dict(K=np.full((3, 4), np.inf)), "K"),
    (dict(ext=np.zeros((2, 3, 4))), "ext"), (dict(ext=np.full((3, 3, 4), np.nan)), "ext"), (dict(ext=None), "ext"),
    (dict(neighbours=[[1], [0]]), "neighbours"), (dict(neighbours=[[1], [0], [3]]), "neighbours"), (dict(neighbours=[[1], [0], [-1]]), "neighbours"),
    (dict(neighbours=[[0], [0], []]), "neighbours"), (dict(neighbours=[[1, 1], [0], []]), "neighbours"), (dict(neighbours=[[1.5], [0], []]), "neighbours"),
    (dict(neighbours=(np.array([0, 2, 1, 3]), np.array([1, 2, 0]))), "neighbours"), (dict(neighbours=(np.array([1, 2, 3, 3]), np.array([1, 2, 0]))), "neighbours"),
    (dict(neighbours=(np.array([0, 1, 2, 4]), np.array([1, 2, 0]))), "neighbours"), (dict(neighbours=5), "neighbours"),
    (dict(px_tol=0.0), "px_tol"), (dict(px_tol=np.inf), "px_tol"), (dict(px_tol="1"), "px_tol"), (dict(rel_tol=-0.01), "rel_tol"), (dict(rel_tol=np.nan), "rel_tol"),
    (dict(min_views=0), "min_views"), (dict(min_views=33), "min_views"), (dict(min_views=2.0), "min_views"), (dict(min_views=True), "min_views"),
    (dict(transform=np.zeros((3, 3))), "transform"), (dict(transform=np.full((3, 4), np.nan)), "transform"),
    (dict(dtype=np.float16), "dtype"), (dict(dtype=np.int32), "dtype"),
])
def test_check_fuse_args_names_the_argument(change, name):
    with pytest.raises(ValueError, match=rf"^{name}\b"):
        fusion.check_fuse_args(**dict(good(), **change))


def test_check_fuse_args_accepts_and_normalises():
    K, P, start, nbr, px, rel, mv, T, f32 = fusion.check_fuse_args(**good(), transform=np.eye(4))
    assert K.shape == (3, 4) and P.shape == (3, 12) and start.dtype == nbr.dtype == np.int32 and list(start) == [0, 2, 3, 3] and list(nbr) == [1, 2, 0]
    assert (px, rel, mv, f32) == (1.0, 0.01, 2, True) and T.shape == (12,)
    out = fusion.check_fuse_args(**dict(good(), neighbours=(start, nbr)))
    assert list(out[2]) == [0, 2, 3, 3] and list(out[3]) == [1, 2, 0]
    many = [[j for j in range(34) if j != i][:32] for i in range(34)]
    K34, E34 = inp.ring_views(34, 8, 6, 1.0)
    assert len(fusion.check_fuse_args(34, 8, 6, K34, E34, many)[3]) == 34 * 32
    many[5] = [j for j in range(34) if j != 5]
    with pytest.raises(ValueError, match="^neighbours.*33"):
        fusion.check_fuse_args(34, 8, 6, K34, E34, many)


def test_fuse_depth_maps_refuses_bad_inputs_before_the_device():
    D, K, E = inp.ring(5, 24, 16, 7.0, 303, False, 404)
    nb = inp.nearest_lists(5, 2)
    for args, kw, name in (((D[0], K, E, nb), {}, "depth"), ((D.astype(np.float16), K, E, nb), {}, "depth"), ((D, K[:4], E, nb), {}, "K"),
                           ((D, K, E, nb), dict(min_views=0), "min_views"), ((D, K, E, nb), dict(values=np.zeros((5, 16, 23), dtype=np.uint8)), "values"),
                           ((D, K, E, nb), dict(dtype=np.int8), "dtype")):
        with pytest.raises(ValueError, match=rf"^{name}\b"):
            fusion.fuse_depth_maps(*args, **kw)
    with pytest.raises(ValueError, match="^pairs"):
        fusion.fuse_stereo_pairs(np.zeros((3, 8, 8), dtype=np.uint8), np.zeros((3, 9)), np.zeros((3, 3, 4)), [(0, 3)], 16)
    with pytest.raises(ValueError, match="^pairs"):
        fusion.fuse_stereo_pairs(np.zeros((3, 8, 8), dtype=np.uint8), np.zeros((3, 9)), np.zeros((3, 3, 4)), [], 16)


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 125
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    K, E = inp.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    ARG = _capi.PCS_ERR_ARG
    assert lib.pcs_fuse_create(None, 0) == ARG and lib.pcs_fuse_destroy(None) == _capi.PCS_OK
    # pcs_fuse_set_views: each refusal names its argument; the handle is looked at last
    bad_K, inf_K, bad_P = K.copy(), K.copy(), P.copy()
    bad_K[1, 2], inf_K[2, 1], bad_P[0, 7] = 0.0, np.inf, np.nan
    for args, word in (((0, 8, 6, dp(K), dp(P)), "n_views"), ((32768, 8, 6, dp(K), dp(P)), "n "), ((3, 0, 6, dp(K), dp(P)), "width"), ((3, 8, 65536, dp(K), dp(P)), "height"),
                       ((3, 8, 6, None, dp(P)), "K"), ((3, 8, 6, dp(K), None), "P"), ((3, 8, 6, dp(bad_K), dp(P)), "K of view 1"), ((3, 8, 6, dp(inf_K), dp(P)), "K of view 2"),
                       ((3, 8, 6, dp(K), dp(bad_P)), "P of view 0"), ((3, 8, 6, dp(K), dp(P)), "NULL handle")):
        assert lib.pcs_fuse_set_views(None, *args) == ARG and word in _err(), (word, _err())
    # pcs_fuse_set_neighbours
    too_many = np.concatenate([[0], np.full(3, 33)])
    for start, nbr, n, word in (([0, 1, 2, 3], [1, 0, 0], 0, "n 0"), (None, [1], 3, "nbr_start"), ([1, 1, 2, 3], [1, 0, 0], 3, "begin at 0"), ([0, 2, 1, 3], [1, 2, 0], 3, "non-decreasing"),
                                (too_many, np.arange(33) % 3, 3, "more than 32"), ([0, 1, 2, 3], None, 3, "nbr must be given"), ([0, 1, 2, 3], [1, 0, 3], 3, "outside"),
                                ([0, 1, 2, 3], [1, -1, 0], 3, "outside"), ([0, 1, 2, 3], [1, 1, 0], 3, "own neighbour"), ([0, 2, 2, 3], [1, 1, 0], 3, "twice"),
                                ([0, 1, 2, 3], [1, 0, 0], 3, "NULL handle"), ([0, 0, 0, 0], None, 3, "NULL handle")):
        rc = lib.pcs_fuse_set_neighbours(None, None if start is None else ip(start), None if nbr is None else ip(nbr), n)
        assert rc == ARG and word in _err(), (word, _err())
    # pcs_fuse_run: (d_depth, depth_dtype, px_tol, rel_tol, min_views, unique, T, d_points, points_dtype, d_mask, d_count, d_support, d_status, d_fused, fused_dtype, d_counts, stream)
    ok = dict(d_depth=64, depth_dtype=1, px_tol=1.0, rel_tol=0.01, min_views=2, unique=0, T=None, d_points=64, points_dtype=1, d_mask=64, d_count=None, d_support=None,
              d_status=None, d_fused=None, fused_dtype=0, d_counts=None, stream=None)
    nanT = np.full(12, np.nan)
    for change, word in ((dict(depth_dtype=2), "depth_dtype"), (dict(px_tol=0.0), "px_tol"), (dict(px_tol=float("nan")), "px_tol"), (dict(rel_tol=float("inf")), "rel_tol"),
                         (dict(rel_tol=-1.0), "rel_tol"), (dict(min_views=0), "min_views"), (dict(min_views=33), "min_views"), (dict(unique=2), "unique"), (dict(T=dp(nanT)), "T is"),
                         (dict(points_dtype=2), "points_dtype"), (dict(d_fused=64, fused_dtype=5), "fused_dtype"), (dict(d_depth=None), "d_depth"), (dict(d_points=None), "d_points"),
                         (dict(d_mask=None), "d_mask"), (dict(), "NULL handle")):
        a = dict(ok, **change)
        assert lib.pcs_fuse_run(None, *a.values()) == ARG and word in _err(), (word, _err())
    f = ctypes.c_float()
    assert lib.pcs_fuse_last_kernel_ms(None, ctypes.byref(f), ctypes.byref(f), ctypes.byref(f)) == ARG
    if lib.pcs_device_count() == 0:   # no device: no handle, and never a CPU fallback
        with pytest.raises(_capi.PcsError) as e:
            fusion.DepthFuser(0)
        assert e.value.code == _capi.PCS_ERR_NODEVICE
