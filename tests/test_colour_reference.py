"""The colour rule without a GPU: the two forms of the NumPy restatement (tests/colour_reference.py) against each other, the margins of
every input set of the device tests (tests/colour_inputs.py), the properties that make the rule a colouring of the surface (the
textured plane's mesh takes the texture, a plane point hidden by the sphere takes nothing from the view it is hidden from, the best
view is the blend of one, one view without normals is bilinear sampling), ``write_ply`` and the host-side argument checks of
pycamset_amd/volume.py and the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

from pycamset_amd import _capi, volume
from tests import colour_inputs as inp
from tests import colour_reference as col
from tests import fusion_inputs as fi

MARGIN = inp.MARGIN
ALL = list(inp.CASES)

MEDIAN_TEXTURE_ERROR = inp.MEDIAN_TEXTURE_ERROR


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    return inp.run_reference(inp.get(name), mode)


@pytest.mark.parametrize("name", ALL)
def test_the_two_forms_agree_exactly(name):
    """Every third point (3 shares no factor with the 15- and 9-wide grids the points come from), both modes."""
    case = inp.get(name)
    rows = col.source_rows(case["K"], case["ext"])
    for mode in col.MODES:
        want = reference(name, mode)
        for i in range(0, len(case["points"]), 3):
            c, wt, count, best, closest = col.colour_point(case["points"][i], rows, case["width"], case["height"], case["images"], None if case["normals"] is None else case["normals"][i],
                                                           case["visibility"], case["occlusion_tol"], case["cos_min"], mode, case["fill"])
            assert (count, best) == (want["count"][i], want["best"][i]), (name, mode, i)
            assert np.array_equal(np.array(c + [wt]), np.append(want["colour"][i], want["weight"][i]), equal_nan=True), (name, mode, i)
            assert closest == want["closest"][i], (name, mode, i)


@pytest.mark.parametrize("name", inp.VOLUME_CASES)
def test_the_two_forms_of_the_point_normals_agree_exactly(name):
    vol, X = inp.integrated(inp.get(name)), inp.normal_points(name)
    want = col.point_normals(vol, X, 2)
    assert (want["status"] == 0).sum() >= 100 and (want["status"] == 1).sum() >= 5
    for i in range(len(X)):
        n, status, closest = col.point_normal(vol, X[i], 2)
        assert status == want["status"][i] and np.array_equal(np.array(n), want["normal"][i], equal_nan=True) and closest == want["closest"][i], (name, i)


@pytest.mark.parametrize("name", ALL)
def test_no_decision_of_an_input_set_sits_near_its_threshold(name):
    """Every point of every case, in both modes: zero points are excluded."""
    need = MARGIN * inp.COLOUR_DECISION_GAP
    for mode in col.MODES:
        r = reference(name, mode)
        worst = float(r["closest"].min()) if len(r["closest"]) else np.inf
        print(f"{name} {mode}: closest call {worst:.2e} (needed {need:.2e})")
        assert worst >= need


@pytest.mark.parametrize("name", inp.VOLUME_CASES)
def test_no_decision_of_the_render_views_and_the_point_normals_sits_near_its_threshold(name):
    need = MARGIN * inp.COLOUR_DECISION_GAP
    case = inp.get(name)
    worst = min(float(inp.run_views_reference(case, name, k, mode)["closest"].min()) for k in range(len(case["render"])) for mode in col.MODES)
    worst_n = float(col.point_normals(inp.integrated(case), inp.normal_points(name), 2)["closest"].min())
    print(f"{name}: closest call of the render views {worst:.2e}, of the point normals {worst_n:.2e} (needed {need:.2e})")
    assert worst >= need and worst_n >= need


def test_the_gaps_are_the_restatements_own():
    g, ng, dg = inp.measure_gaps()
    print(f"COLOUR_GAP measured {g[0]:.2e} ({g[1]}), recorded {inp.COLOUR_GAP:.2e}; COLOUR_NORMAL_GAP measured {ng[0]:.2e} ({ng[1]}), recorded {inp.COLOUR_NORMAL_GAP:.2e}; "
          f"COLOUR_DECISION_GAP measured {dg[0]:.2e} ({dg[1]}), recorded {inp.COLOUR_DECISION_GAP:.2e}")
    assert g[0] <= inp.COLOUR_GAP <= 2 * g[0] and ng[0] <= inp.COLOUR_NORMAL_GAP <= 2 * ng[0] and dg[0] <= inp.COLOUR_DECISION_GAP <= 2 * dg[0]
    assert inp.MARGIN == 8.0


def test_cases_cover_what_the_kernel_branches_on():
    cases = {n: inp.get(n) for n in ALL}
    assert {c["images"].shape[3] for c in cases.values()} == {1, 3, 4} and {c["images"].dtype for c in cases.values()} == {np.dtype(np.uint8), np.dtype(np.float32)}
    assert {c["points"].dtype for c in cases.values()} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {len(cases[f"n_{n}"]["points"]) for n in inp.SIZES} == set(inp.SIZES) == {0, 1, 63, 64, 65, 257}
    assert {c["normals"] is None for c in cases.values()} == {True, False} and {c["visibility"] is None for c in cases.values()} == {True, False}
    assert {c["visibility"].dtype for c in cases.values() if c["visibility"] is not None} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert len(cases["one_view"]["K"]) == 1 and len(cases["views_40"]["K"]) == 40 and cases["image_2x2"]["images"].shape[1:3] == (2, 2)
    c = cases["with_nans"]
    assert np.isnan(c["points"]).any() and np.isnan(c["normals"]).any() and not np.isnan(c["points"]).all(axis=1).all()
    D = c["visibility"]
    assert np.isnan(D).any() and (D == 0).any() and (D < 0).any() and np.isposinf(D).any()
    r = reference("with_nans", "blend")
    assert np.all(r["count"][np.isnan(c["points"]).any(axis=1) | np.isnan(c["normals"]).any(axis=1)] == 0)
    assert reference("views_40", "blend")["count"].max() == 40 and reference("views_40", "blend")["best"].max() > 32
    # facing: no wall point of view 0 is coloured by view 1 or the other way round; no_overlap: by views 0 and 1, or by none
    f = col.colour(cases["facing"]["points"], cases["facing"]["K"], cases["facing"]["ext"], 64, 48, cases["facing"]["images"])
    assert f["count"].max() <= 2 and np.all(f["decisions"]["front"][:63, 1] < 0) and np.all(f["decisions"]["front"][63:, 0] < 0)
    r = reference("no_overlap", "blend")
    assert set(np.unique(r["best"])) <= {-1, 0, 1} and np.all(r["count"][-20:] == 0) and (r["count"] == 2).sum() >= 30
    for name in inp.VOLUME_CASES:
        assert [(v["width"], v["height"]) for v in cases[name]["render"]] == [(40, 30), (13, 7), (1, 1)]
    assert cases["textured_plane"]["images"].shape == (6, 40, 48, 1)


@pytest.mark.parametrize("mode", col.MODES)
def test_the_mesh_of_the_textured_plane_takes_the_texture(mode):
    """The vertices of the plane's mesh against fusion_inputs.texture at the vertex.  The images are the texture sampled once per pixel
    and rounded to uint8, the texture's finest period is about 0.1 m = 12 pixels, and the vertices lie within a fraction of a voxel of
    the plane: the colour is the texture up to the bilinear interpolation of a curved signal, some grey levels."""
    case = inp.get("textured_plane")
    r = reference("textured_plane", mode)
    some = r["count"] > 0
    X = case["points"][some]
    err = np.abs(r["colour"][some, 0] - fi.texture(X[:, 0], X[:, 1]))
    print(f"{mode}: {int(some.sum())} of {len(some)} vertices coloured, |colour - texture| median {np.median(err):.2f}, max {err.max():.2f} grey levels; "
          f"the texture spans {np.ptp(fi.texture(X[:, 0], X[:, 1])):.0f}")
    assert some.sum() >= 60 and np.all(r["count"][some] == 6)
    assert np.median(err) <= 2.0 * MEDIAN_TEXTURE_ERROR[mode]
    assert np.all(r["colour"][~some, 0] == 17.0) and np.all(r["best"][~some] == -1) and np.all(r["weight"][~some] == 0)


def _analytic_visibility(case):
    """Per (plane point, view), from the geometry alone: ``seen`` — in front, in the image and the segment from the centre to the point
    misses the sphere; ``decided`` — the nearest pixel's own ray meets the same surface first as the point's ray, and where that is the
    sphere it does so more than twice occlusion_tol in front of the point."""
    K, E, W, H, tol = case["K"], case["ext"], case["width"], case["height"], case["occlusion_tol"]
    centre, radius = fi.SPHERE
    n, h = fi.PLANE
    X = case["points"]
    plane = np.abs(X @ n - h) < 1e-9
    seen, decided = np.zeros((len(X), len(K)), dtype=bool), np.zeros((len(X), len(K)), dtype=bool)
    with np.errstate(all="ignore"):
        for v in range(len(K)):
            R, t = E[v][:, :3], E[v][:, 3]
            C = -R.T @ t
            Y = X @ R.T + t
            u, w = K[v, 0] * Y[:, 0] / Y[:, 2] + K[v, 1], K[v, 2] * Y[:, 1] / Y[:, 2] + K[v, 3]
            inside = (Y[:, 2] > 0) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
            d, oc = X - C, C - centre
            A, B, Cq = np.sum(d * d, axis=1), d @ oc, oc @ oc - radius ** 2
            disc = B * B - A * Cq
            s = (-B - np.sqrt(disc)) / A
            hidden = (disc > 0) & (s > 0) & (s < 1)
            seen[:, v] = inside & ~hidden
            qx, qy = np.floor(u + 0.5), np.floor(w + 0.5)
            Xq, _, surf = inp.cast_points(K[v], E[v], qx, qy)
            zq = (Xq @ R.T + t)[:, 2]
            decided[:, v] = ~inside | np.where(hidden, (surf == 1) & (Y[:, 2] - zq > 2 * tol), (surf == 0) & (np.abs(zq - Y[:, 2]) < 0.5 * tol))
    return plane, seen, decided


def test_a_plane_point_the_sphere_hides_from_a_view_takes_nothing_from_it():
    """count against an analytic visibility count wherever every view of the point is decided; without the maps the same points DO take
    the hidden views' contribution, and their colour shows it: the test can see a leak."""
    case = inp.get("plane_sphere_no_normals")
    plane, seen, decided = _analytic_visibility(case)
    r = reference("plane_sphere_no_normals", "blend")
    leaky = reference("plane_sphere_neither", "blend")
    pick = plane & decided.all(axis=1)
    hidden_somewhere = pick & (leaky["count"] > seen.sum(axis=1))
    print(f"{int(plane.sum())} plane points, {int(pick.sum())} decided in every view, {int(hidden_somewhere.sum())} of them hidden from a view that has them in its image")
    assert pick.sum() >= 150 and hidden_somewhere.sum() >= 20
    assert np.array_equal(r["count"][pick], seen.sum(axis=1)[pick])
    for v in range(len(case["K"])):   # view by view: a hidden view never contributes, a seeing one always does
        alone = col.colour(case["points"], case["K"][v:v + 1], case["ext"][v:v + 1], case["width"], case["height"], case["images"][v:v + 1], visibility=case["visibility"][v:v + 1],
                           occlusion_tol=case["occlusion_tol"])
        assert np.array_equal(alone["count"][pick] == 1, seen[pick, v])
    # channel 0 of the images is 60 + gradient on the plane and 180 + gradient on the sphere: a hidden view that leaks in lifts the blend of
    # at most six views by some 120 / 6 = 20
    with_maps, without = r["colour"][hidden_somewhere, 0], leaky["colour"][hidden_somewhere, 0]
    print(f"channel 0 of the hidden points: without maps above with maps by {np.min(without - with_maps):.1f} to {np.max(without - with_maps):.1f}")
    assert np.all(without > with_maps + 10.0)


@pytest.mark.parametrize("name", ["plane_sphere", "views_40", "no_overlap", "textured_plane"])
def test_best_equals_blend_where_one_view_contributes(name):
    """(c I) / c is I up to two roundings: 2^-52 relative; where c is 1 exactly (no normals) it is I."""
    blend, best = reference(name, "blend"), reference(name, "best")
    assert np.array_equal(blend["count"], best["count"]) and np.array_equal(blend["best"], best["best"]) and np.array_equal(blend["weight"], best["weight"])
    one = blend["count"] == 1
    assert one.sum() >= 1 or name == "textured_plane"
    assert np.all(np.abs(blend["colour"][one] - best["colour"][one]) <= 2.0 ** -52 * np.abs(best["colour"][one]))
    assert np.array_equal(col.round_u8(blend["colour"][one]), col.round_u8(best["colour"][one]))
    none = blend["count"] == 0
    assert np.array_equal(blend["colour"][none], best["colour"][none])
    plain_a, plain_b = (inp.run_reference(dict(inp.get(name), normals=None), m) for m in col.MODES)
    one = plain_a["count"] == 1
    assert np.array_equal(plain_a["colour"][one], plain_b["colour"][one])


def test_one_view_without_normals_is_plain_bilinear_sampling():
    """Against a bilinear interpolation written independently (weights (1 - a)(1 - b) ... on the four taps, u and w from a matrix product).
    u and w each carry a few roundings of a number below 48, at most 48 x 2^-50 together, and a step of that size along either axis moves
    the sample by at most 255 times it; the blend's own roundings (255 x 2^-50) are smaller."""
    case = inp.get("one_view")
    r = reference("one_view", "blend")
    K, E, im = case["K"][0], case["ext"][0], case["images"][0].astype(np.float64)
    Y = case["points"] @ E[:, :3].T + E[:, 3]
    with np.errstate(all="ignore"):
        u, w = K[0] * Y[:, 0] / Y[:, 2] + K[1], K[2] * Y[:, 1] / Y[:, 2] + K[3]
    inside = (Y[:, 2] > 0) & (u >= 0) & (u <= 47) & (w >= 0) & (w <= 39)
    assert np.array_equal(r["count"], inside.astype(np.int64)) and inside.sum() >= 80 and (~inside).sum() >= 20
    x0, y0 = np.floor(u[inside]).astype(int), np.floor(w[inside]).astype(int)
    a, b = (u[inside] - x0)[:, None], (w[inside] - y0)[:, None]
    want = (1 - a) * (1 - b) * im[y0, x0] + a * (1 - b) * im[y0, x0 + 1] + (1 - a) * b * im[y0 + 1, x0] + a * b * im[y0 + 1, x0 + 1]
    assert np.max(np.abs(r["colour"][inside] - want)) <= 2 * 255.0 * 48.0 * 2.0 ** -50 + 255.0 * 2.0 ** -50
    assert np.all(r["weight"][inside] == 1.0) and np.all(r["best"][inside] == 0) and np.all(r["colour"][~inside] == 0.0)
    assert np.array_equal(reference("one_view", "best")["colour"], r["colour"])


def test_the_rounding_to_uint8_is_half_to_even_and_saturates():
    assert col.round_u8([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, -3.0, 300.0, np.nan, 127.49999]).tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0, 127]


def _ply_of_today(vertices, faces):
    """The text ``write_ply`` wrote before it took colours and normals."""
    v, f = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64)
    text = (f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    text += "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v)
    return text + "".join(f"{len(row)} " + " ".join(str(int(i)) for i in row) + "\n" for row in f)


def test_write_ply_without_the_new_arguments_writes_todays_bytes(tmp_path):
    m = inp.mesh("textured_plane")
    V, Q = m["vertices"], m["quads"]
    volume.write_ply(tmp_path / "plain.ply", V, Q)
    assert (tmp_path / "plain.ply").read_bytes() == _ply_of_today(V, Q).encode()
    volume.write_ply(tmp_path / "tri.ply", V.astype(np.float32), volume.quads_to_triangles(Q))
    assert (tmp_path / "tri.ply").read_bytes() == _ply_of_today(V.astype(np.float32), volume.quads_to_triangles(Q)).encode()
    colours = col.round_u8(reference("textured_plane", "blend")["colour"])
    normals = inp.get("textured_plane")["normals"]
    volume.write_ply(tmp_path / "full.ply", V, Q, colours=np.repeat(colours, 3, axis=1), normals=np.nan_to_num(normals))
    lines = (tmp_path / "full.ply").read_text().split("\n")
    head = lines[:lines.index("end_header")]
    assert head[3:] == ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
                        "property uchar green", "property uchar blue", f"element face {len(Q)}", "property list uchar int vertex_indices"]
    row = lines[len(head) + 1].split()
    assert len(row) == 9 and [int(x) for x in row[6:]] == [int(colours[0, 0])] * 3 and np.allclose([float(x) for x in row[:3]], V[0])
    assert lines[len(head) + 1 + len(V)] == "4 " + " ".join(str(int(i)) for i in Q[0])
    volume.write_ply(tmp_path / "grey.ply", V, Q, colours=colours[:, 0])   # one channel: grey on all three
    grey = (tmp_path / "grey.ply").read_text().split("\n")
    assert grey[grey.index("end_header") + 1].split()[3:] == [str(int(colours[0, 0]))] * 3
    for kw, word in ((dict(colours=colours[:-1]), "colours"), (dict(colours=np.zeros((len(V), 2))), "colours"), (dict(normals=normals[:, :2]), "normals")):
        with pytest.raises(ValueError) as e:
            volume.write_ply(tmp_path / "bad.ply", V, Q, **kw)
        assert word in str(e.value)


def test_check_colour_args_refuses_each_bad_argument_by_name():
    K, E = fi.ring_views(3, 8, 6, 8.0)
    im, D, n = np.zeros((3, 6, 8, 3), dtype=np.uint8), np.ones((3, 6, 8), dtype=np.float32), np.zeros((5, 3), dtype=np.float32)
    a = volume.check_colour_args(im, K, E)
    assert (a["width"], a["height"], a["channels"], a["image_dtype"], a["dtype"], a["mode"], a["cos_min"]) == (8, 6, 3, "uint8", "uint8", "blend", 0.0) and a["fill"].tolist() == [0, 0, 0]
    assert a["K"].shape == (3, 4) and a["P"].shape == (3, 12)
    a = volume.check_colour_args(im[..., 0].astype(np.float32), K, E, normals=n, n_points=5, visibility=D, occlusion_tol=0.0, cos_min=0.5, mode="best", fill=7, dtype=np.uint8)
    assert (a["channels"], a["image_dtype"], a["dtype"], a["mode"], a["occlusion_tol"], a["cos_min"]) == (1, "float32", "uint8", "best", 0.0, 0.5) and a["fill"].tolist() == [7.0]
    bad_K = K.copy()
    bad_K[1, 2] = 0.0
    ok = dict(images=im, K=K, ext=E, normals=n, n_points=5, visibility=D, occlusion_tol=0.01)
    for change, word in ((dict(images=im[0, 0]), "images"), (dict(images=im[..., :2]), "images"), (dict(images=im.astype(np.float64)), "images"), (dict(images=[[1]]), "images"),
                         (dict(images=im[:, :1]), "images"), (dict(images=im[:, :, :1]), "images"), (dict(images=im[:0]), "images"), (dict(K=bad_K), "K"), (dict(K=K[:2]), "K"),
                         (dict(K=np.where(K > 0, np.nan, K)), "K"), (dict(ext=E[:2]), "ext"), (dict(ext=np.where(E > 5, np.inf, E) * np.inf), "ext"), (dict(normals=n[:4]), "normals"),
                         (dict(normals=n[:, :2]), "normals"), (dict(normals=n.astype(np.int32)), "normals"), (dict(visibility=D[:2]), "visibility"),
                         (dict(visibility=D.astype(np.float16)), "visibility"), (dict(occlusion_tol=None), "occlusion_tol"), (dict(occlusion_tol=-0.1), "occlusion_tol"),
                         (dict(occlusion_tol=np.nan), "occlusion_tol"), (dict(occlusion_tol=np.inf), "occlusion_tol"), (dict(cos_min=-0.1), "cos_min"), (dict(cos_min=1.0), "cos_min"),
                         (dict(cos_min=np.nan), "cos_min"), (dict(cos_min="0"), "cos_min"), (dict(mode="mean"), "mode"), (dict(fill=[1, 2]), "fill"), (dict(fill=np.inf), "fill"),
                         (dict(fill="red"), "fill"), (dict(dtype=np.float64), "dtype"), (dict(dtype="colour"), "dtype")):
        with pytest.raises(ValueError) as e:
            volume.check_colour_args(**dict(ok, **change))
        assert word in str(e.value), (change, str(e.value))
    X = np.zeros((5, 3))
    for f, word in ((lambda: volume.colour_points(X[:, :2], im, K, E), "points"), (lambda: volume.colour_points(X.astype(np.int64), im, K, E), "points"),
                    (lambda: volume.colour_points(X, im, K, E, mode="mean"), "mode"), (lambda: volume.colour_points(X, im, K, E, visibility=D), "occlusion_tol"),
                    (lambda: volume.colour_points(X, im, K, E, volume=3), "volume"), (lambda: volume.vertex_normals(None, X), "volume"),
                    (lambda: volume.colour_surface(None, X, im, K, E), "volume"), (lambda: volume.colour_views(None, K, E, 8, 6, im, K, E), "volume"),
                    (lambda: volume.mesh_views(D, K, E, [[0, 0, 0], [1, 1, 1]], 0.1, cos_min=0.2), "images")):
        with pytest.raises(ValueError) as e:
            f()
        assert word in str(e.value), str(e.value)   # every one is refused before anything touches the device


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 129
    for name in ("pcs_tsdf_point_normals", "pcs_tsdf_colour_points", "pcs_tsdf_colour_views", "pcs_tsdf_colour_last_kernel_ms"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert _capi.COLOUR_MODE_IDS == {"blend": 0, "best": 1}
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    K, E = fi.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    bad_K = K.copy()
    bad_K[1, 2] = 0.0
    bad_P = P.copy()
    bad_P[2, 5] = np.inf
    ARG = _capi.PCS_ERR_ARG
    good = dict(n=5, pts=64, pdt=1, nrm=64, V=3, w=8, h=6, K=dp(K), P=dp(P), img=64, pitch=24, ch=3, idt=0, vis=64, vdt=1, tol=0.01, cmin=0.0, mode=0, fill=None, col=64, cdt=0)
    source = ((dict(V=0), "n_views"), (dict(w=1), "width"), (dict(h=1), "height"), (dict(w=65536), "width"), (dict(K=None), "K"), (dict(K=dp(bad_K)), "K of view 1"), (dict(P=None), "P"),
              (dict(P=dp(bad_P)), "P of view 2"), (dict(ch=2), "channels"), (dict(idt=2), "image_dtype"), (dict(pitch=23), "pitch"), (dict(idt=1, pitch=98), "pitch"),
              (dict(idt=1, pitch=95), "pitch"), (dict(img=None), "d_images"), (dict(idt=1, pitch=96, img=66), "d_images"), (dict(vdt=2), "visibility_dtype"), (dict(tol=-1.0), "occlusion_tol"),
              (dict(tol=np.nan), "occlusion_tol"), (dict(tol=np.inf), "occlusion_tol"), (dict(cmin=1.0), "cos_min"), (dict(cmin=-0.5), "cos_min"), (dict(cmin=np.nan), "cos_min"),
              (dict(mode=2), "mode"), (dict(fill=dp([0.0, np.inf, 0.0])), "fill[1]"), (dict(cdt=2), "colour_dtype"), (dict(col=None), "d_colour"), (dict(), "NULL handle"),
              (dict(vis=None, tol=np.nan, nrm=None), "NULL handle"))

    def points(a):
        return lib.pcs_tsdf_colour_points(None, a["n"], a["pts"], a["pdt"], a["nrm"], a["V"], a["w"], a["h"], a["K"], a["P"], a["img"], a["pitch"], a["ch"], a["idt"], a["vis"], a["vdt"],
                                          a["tol"], a["cmin"], a["mode"], a["fill"], a["col"], a["cdt"], None, None, None, None)

    for change, word in ((dict(n=-1), "n "), (dict(pdt=2), "point_dtype"), (dict(pts=None), "d_points")) + source:
        assert points(dict(good, **change)) == ARG and word in _err(), (change, word, _err())

    render = dict(R=1, rw=13, rh=7, Kr=dp(K[:1]), Pr=dp(P[:1]), depth=64, ddt=1)

    def views(a):
        return lib.pcs_tsdf_colour_views(None, a["R"], a["rw"], a["rh"], a["Kr"], a["Pr"], a["depth"], a["ddt"], a["nrm"], a["V"], a["w"], a["h"], a["K"], a["P"], a["img"], a["pitch"],
                                         a["ch"], a["idt"], a["vis"], a["vdt"], a["tol"], a["cmin"], a["mode"], a["fill"], a["col"], a["cdt"], None, None, None, None)

    for change, word in ((dict(R=0), "n_views"), (dict(rw=0), "width"), (dict(Kr=None), "K_render"), (dict(Pr=None), "K_render"), (dict(ddt=2), "depth_dtype"), (dict(depth=None), "d_depth")) + source:
        assert views({**good, **render, **change}) == ARG and word in _err(), (change, word, _err())
    for change, word in ((dict(n=-1), "n "), (dict(pdt=2), "point_dtype"), (dict(pts=None), "d_points"), (dict(mw=0), "min_weight"), (dict(mw=65536), "min_weight"), (dict(out=None), "d_normals"),
                         (dict(), "NULL handle")):
        a = dict(dict(n=5, pts=64, pdt=0, mw=2, out=64), **change)
        assert lib.pcs_tsdf_point_normals(None, a["n"], a["pts"], a["pdt"], a["mw"], a["out"], None, None) == ARG and word in _err(), (change, word, _err())
    f = ctypes.c_float()
    assert lib.pcs_tsdf_colour_last_kernel_ms(None, ctypes.byref(f), ctypes.byref(f)) == ARG
