"""Fixed inputs of the colour tests, built from what tests/fusion_inputs.py, tests/tsdf_inputs.py and tests/raycast_inputs.py provide:
nothing is committed but this code.  ``CASES`` names every input set the device tests use (tests/test_gpu_colour.py);
tests/test_colour_reference.py asserts for each of them that no decision of the rule sits near its threshold.

A case is a dict: the source views (``K``, ``ext``, ``width``, ``height``), their ``images`` (V, H, W, C), the ``points`` (N, 3) with
``normals`` (N, 3) float32 or None, the ``visibility`` maps (V, H, W) or None, ``occlusion_tol``, ``cos_min`` and ``fill``.  Points are
cast analytically through pixel positions OFF the pixel grid (x + 0.37, y + 0.21) or are mesh vertices: a point cast through a pixel
centre would project onto an integer of its own view, on the threshold of both floors.  A case with a ``volume`` (the inputs of a
tests/tsdf_inputs.py case) also has ``render``, the three render views of tests/raycast_inputs.py (40 x 30, 13 x 7, 1 x 1) for
``colour_views``, and ``min_weight``.

COLOUR_GAP, COLOUR_NORMAL_GAP and COLOUR_DECISION_GAP are the float64-versus-longdouble gaps of the restatement
(tests/colour_reference.py) over ``CASES`` in both modes.  COLOUR_GAP: the largest |float64 - longdouble| colour or weight, relative to
the largest colour (weight) of the case.  COLOUR_NORMAL_GAP: the same for the components of the point normals (unit vectors:
absolute).  COLOUR_DECISION_GAP: the same for the decision quantities, each relative to its scale.  Measured on the CPU with

    python -m tests.colour_inputs

which printed ``COLOUR_GAP 7.0e-15 (no_overlap)  COLOUR_NORMAL_GAP 4.5e-16 (plane_sphere)  COLOUR_DECISION_GAP 6.4e-14 (no_overlap)``; the
constants below are those figures rounded up in the second digit.  tests/test_colour_reference.py recomputes all three and holds the
constants to be no smaller.  The colour's gap, and through the uint8 rounding the decisions', comes from the random images of
``no_overlap``, whose neighbouring pixels differ by up to 255: a rounding of u of 1e-14 pixel moves the sample by that times the difference."""
import functools

import numpy as np

from tests import colour_reference as col
from tests import fusion_inputs as fi
from tests import raycast_inputs as ri
from tests import raycast_reference as ray
from tests import tsdf_inputs as ti
from tests import tsdf_reference as tref

COLOUR_GAP = 7.1e-15
COLOUR_NORMAL_GAP = 4.6e-16
COLOUR_DECISION_GAP = 6.5e-14
MARGIN = ti.MARGIN

# The restatement's own median |vertex colour - texture at the vertex| over the coloured vertices of the textured plane's mesh (grey
# levels), as tests/test_colour_reference.py::test_the_mesh_of_the_textured_plane_takes_the_texture printed it; the tests assert twice
# this ("Colour of the surface").
MEDIAN_TEXTURE_ERROR = {"blend": 1.95, "best": 1.51}

SIZES = (0, 1, 63, 64, 65, 257)   # below, at and above a wave; more than one workgroup of 256


def cast_points(Kv, Ev, px, py, plane=fi.PLANE, sphere=fi.SPHERE):
    """The surface points on the rays of view (Kv, Ev) through the pixel positions (px, py), which need not be integers.
    -> (points (n, 3) float64, NaN where the ray meets nothing; normals (n, 3) float64 pointing outward; surface (n): 0 plane, 1 sphere, -1)."""
    R, t = Ev[:, :3], Ev[:, 3]
    d = np.stack([(px - Kv[1]) / Kv[0], (py - Kv[3]) / Kv[2], np.ones_like(px)], axis=-1) @ R
    o = -(R.T @ t)
    z, surf = np.full(len(px), np.inf), np.full(len(px), -1)
    nrm = np.full((len(px), 3), np.nan)
    with np.errstate(all="ignore"):
        if plane is not None:
            s = (plane[1] - plane[0] @ o) / (d @ plane[0])
            hit = s > 0
            z, surf = np.where(hit, s, z), np.where(hit, 0, surf)
            nrm[hit] = plane[0] if plane[0] @ (o - plane[0] * plane[1]) > 0 else -plane[0]
        if sphere is not None:
            oc = o - sphere[0]
            A, B, C = np.sum(d * d, axis=-1), d @ oc, oc @ oc - sphere[1] ** 2
            disc = B * B - A * C
            s = (-B - np.sqrt(disc)) / A
            hit = (disc > 0) & (s > 0) & (s < z)
            z, surf = np.where(hit, s, z), np.where(hit, 1, surf)
            X = o + s[:, None] * d
            nrm[hit] = ((X - sphere[0]) / sphere[1])[hit]
        X = o + z[:, None] * d
    X[surf < 0] = np.nan
    return X, nrm, surf


def grid_positions(W, H, nx, ny):
    """nx x ny pixel positions off the grid, over the image and a little past its border."""
    xs, ys = np.meshgrid(np.linspace(-1.63, W + 0.63, nx), np.linspace(-1.29, H + 0.29, ny))
    return xs.reshape(-1) + 0.0071, ys.reshape(-1) + 0.0043


def surface_images(K, E, W, H, plane=fi.PLANE, sphere=fi.SPHERE):
    """Images (V, H, W, 3) uint8 that are a different constant per surface plus a gradient: plane 60 / 90 / 120, sphere 180 / 200 / 220,
    nothing 10; the gradient 0.5 x + 0.25 y.  A plane point coloured through an occluding sphere is off by about 100."""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    out = np.zeros((len(K), H, W, 3), dtype=np.uint8)
    base = {0: (60.0, 90.0, 120.0), 1: (180.0, 200.0, 220.0), -1: (10.0, 10.0, 10.0)}
    for v in range(len(K)):
        _, _, surf = cast_points(K[v], E[v], xs.reshape(-1), ys.reshape(-1), plane, sphere)
        surf = surf.reshape(H, W)
        for k in range(3):
            level = np.select([surf == 0, surf == 1], [base[0][k], base[1][k]], base[-1][k])
            out[v, :, :, k] = np.rint(level + 0.5 * xs + 0.25 * ys).astype(np.uint8)
    return out


def random_images(V, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(V, H, W, C)).astype(np.uint8)


def with_images(case, channels, image_dtype):
    """The case with ``channels`` channels of ``image_dtype``, derived from its own images: channel k is channel k mod C0, turned round and
    shifted (uint8), or scaled and offset beyond [0, 255] (float32: the float output is not bounded, the uint8 one saturates)."""
    im = case["images"]
    C0 = im.shape[3]
    chans = []
    for k in range(channels):
        src = im[..., k % C0].astype(np.float64)
        if k >= C0:
            src = 255.0 - src if k % 2 else np.floor(0.5 * src) + 37.0
        chans.append(src)
    out = np.stack(chans, axis=-1)
    if np.dtype(image_dtype) == np.dtype(np.float32):
        out = (1.37 * out - 41.3).astype(np.float32)
    else:
        out = out.astype(np.uint8)
    fill = None if case["fill"] is None else [case["fill"][k % len(case["fill"])] for k in range(channels)]
    return dict(case, images=np.ascontiguousarray(out), fill=fill)


def with_points(case, n, dtype=np.float64):
    """The first ``n`` points of the case (repeated with a small shift when it has fewer), as ``dtype``."""
    X, nr = case["points"], case["normals"]
    reps = -(-max(n, 1) // max(len(X), 1))
    shift = (np.arange(reps)[:, None, None] * np.array([0.00113, -0.00071, 0.00057])).astype(np.float64)
    Xs = (X[None] + shift).reshape(-1, 3)[:n]
    return dict(case, points=np.ascontiguousarray(Xs.astype(dtype)), normals=None if nr is None else np.ascontiguousarray(np.tile(nr, (reps, 1))[:n]))


def _case(K, E, W, H, images, points, normals=None, visibility=None, occlusion_tol=0.0, cos_min=0.0, fill=None, **more):
    im = col.as_images(images)
    return dict(K=np.ascontiguousarray(K[:, :4]), ext=np.ascontiguousarray(E), width=W, height=H, images=np.ascontiguousarray(im), points=np.ascontiguousarray(points, dtype=np.float64),
                normals=None if normals is None else np.ascontiguousarray(normals, dtype=np.float32), visibility=None if visibility is None else np.array(visibility), occlusion_tol=occlusion_tol, cos_min=cos_min, fill=fill,
                **more)


@functools.lru_cache(maxsize=None)
def _integrated(key):
    vol, _ = ti.run_reference(VOLUMES[key]())
    for a in (vol.sum, vol.weight):
        a.setflags(write=False)
    return vol


def integrated(case):
    """The volume of a case from the restatement of the integration (tests/tsdf_reference.py), read-only."""
    return _integrated(case["volume_key"])


def _textured_volume():
    images, intr, ext = fi.stereo_ring(6, 7.0)
    K = intr[:, :4]
    D = fi.render(K, ext, 48, 40, plane=(np.array([0.0, 0.0, 1.0]), fi.STEREO_Z0), sphere=None)
    return ti._case((D, K, ext), (-0.2213, -0.1507, 0.9187), 0.02, (17, 14, 9), 0.06, min_weights=(2,))


def _sphere_volume():
    return ti._case(fi.ring(6, 48, 40, 8.0), (-0.47, -0.52, -0.61), 0.06, (19, 18, 23), 0.15, min_weights=(2,))


VOLUMES = {"textured_plane": _textured_volume, "plane_sphere": _sphere_volume}


@functools.lru_cache(maxsize=None)
def model_depth(key, min_weight=2):
    """The model's own depth in the source views of a volume, float32 as ``raycast_views`` returns it by default; read-only."""
    c = VOLUMES[key]()
    H, W = c["depth"].shape[1:]
    d = ray.raycast(_integrated(key), c["K"], c["ext"], W, H, min_weight, normals=False)["depth"].astype(np.float32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mesh(key, min_weight=2):
    return tref.extract(_integrated(key), min_weight)


def _with_volume(key, case):
    vc = VOLUMES[key]()
    return dict(case, volume=vc, volume_key=key, render=ri.render_views(vc), min_weight=2)


def textured_plane():
    """The six-camera ring of the textured plane, cropped to 48 x 40; the points are the vertices of the plane's mesh, the normals the
    restatement's point normals, the visibility the model's own depth."""
    images, intr, ext = fi.stereo_ring(6, 7.0)
    vol = _integrated("textured_plane")
    X = mesh("textured_plane")["vertices"]
    n = col.point_normals(vol, X, 2)["normal"].astype(np.float32)
    return _with_volume("textured_plane", _case(intr, ext, 48, 40, images[:, :40, :48], X, n, model_depth("textured_plane"), np.sqrt(3.0) * 0.02, 0.1, [17.0]))


def plane_sphere(visibility=True, normals=True):
    """The ring of plane and sphere: the analytic surface points of views 0 and 5 and analytic depth maps as the visibility; the sphere
    hides a part of the plane from every view."""
    D, K, E = fi.ring(6, 48, 40, 8.0)
    X, n = [], []
    for v in (0, 5):
        Xv, nv, surf = cast_points(K[v], E[v], *grid_positions(48, 40, 15, 11))
        X.append(Xv), n.append(nv)
    X, n = np.concatenate(X), np.concatenate(n)
    return _with_volume("plane_sphere", _case(K, E, 48, 40, surface_images(K, E, 48, 40), X, n if normals else None, np.array(D) if visibility else None, 0.06, 0.05, [1.0, 2.0, 3.0]))


def facing():
    """Views 0 and 1 face each other: every wall point of either lies behind the other."""
    D, K, E = fi.facing_pair()
    X0, n0, _ = cast_points(K[0], E[0], *grid_positions(64, 48, 9, 7), plane=(np.array([0.0, 0.0, 1.0]), 4.0), sphere=None)
    X1, n1, _ = cast_points(K[1], E[1], *grid_positions(64, 48, 9, 7), plane=(np.array([0.0, 0.0, 1.0]), -2.6), sphere=None)
    return _case(K, E, 64, 48, random_images(3, 48, 64, 1, 11), np.concatenate([X0, X1]), np.concatenate([n0, n1]), np.array(D), 0.05, 0.0)


def no_overlap():
    """Four views in two pairs that share nothing: the points of view 0 are coloured by views 0 and 1, points far from all by none."""
    D, K, E = fi.no_overlap()
    X, n, _ = cast_points(K[0], E[0], *grid_positions(64, 48, 9, 7), sphere=None)
    far = X[:20] + (0.0, 30.0, 0.0)
    return _case(K, E, 64, 48, random_images(4, 48, 64, 3, 12), np.concatenate([X, far]), np.concatenate([n, n[:20]]), np.array(D), 0.05, 0.0, [255.0, 0.0, 128.0])


def one_view():
    """One source view, no normals, no visibility: plain bilinear sampling."""
    D, K, E = fi.ring(1, 48, 40, 8.0)
    X, _, _ = cast_points(K[0], E[0], *grid_positions(48, 40, 13, 11))
    return _case(K, E, 48, 40, random_images(1, 40, 48, 3, 13), X)


def views_40():
    """40 source views: more than a 32-bit mask holds and more than one batch of scalar loads."""
    D, K, E = fi.ring(40, 24, 16, 2.0)
    X, n = [], []
    for v in (3, 21, 38):
        Xv, nv, _ = cast_points(K[v], E[v], *grid_positions(24, 16, 9, 7))
        X.append(Xv), n.append(nv)
    return _case(K, E, 24, 16, surface_images(K, E, 24, 16), np.concatenate(X), np.concatenate(n), np.array(D), 0.12, 0.2, [9.0, 8.0, 7.0])


def image_2x2():
    """Images of 2 x 2: one bilinear cell, both floors clamp."""
    K, E = fi.ring_views(3, 2, 2, 8.0)
    rng = np.random.default_rng(14)
    X = rng.uniform(-0.55, 0.55, size=(90, 3))
    n = np.tile(np.array([0.0, 0.0, -1.0]), (90, 1))
    return _case(K, E, 2, 2, random_images(3, 2, 2, 4, 15), X, n, None, 0.0, 0.3, [1.0, 2.0, 3.0, 4.0])


def with_nans():
    """The plane-and-sphere case with NaN points and NaN normals among the real ones, and every kind of invalid entry in the maps."""
    c = plane_sphere()
    X, n = c["points"].copy(), c["normals"].copy()
    X[5::17, 1] = np.nan
    n[3::13, 2] = np.nan
    D = fi.add_invalid(c["visibility"], 303)
    assert all((np.isnan(D).any(), (D == 0).any(), (D < 0).any(), np.isposinf(D).any()))
    return dict(c, points=X, normals=n, visibility=D)


# name -> () -> the case: every input set of tests/test_gpu_colour.py
CASES = {
    "textured_plane": textured_plane,
    "plane_sphere": plane_sphere,
    "plane_sphere_no_visibility": lambda: plane_sphere(visibility=False),
    "plane_sphere_no_normals": lambda: plane_sphere(normals=False),
    "plane_sphere_neither": lambda: plane_sphere(False, False),
    "plane_sphere_f32_maps": lambda: dict(plane_sphere(), visibility=np.where(np.isfinite(plane_sphere()["visibility"]), plane_sphere()["visibility"], np.nan).astype(np.float32)),
    "with_nans": with_nans,
    "facing": facing,
    "no_overlap": no_overlap,
    "one_view": one_view,
    "views_40": views_40,
    "image_2x2": image_2x2,
}
for _c, _t in ((1, np.uint8), (4, np.uint8), (1, np.float32), (3, np.float32), (4, np.float32)):
    CASES[f"views_40_c{_c}_{np.dtype(_t).name}"] = functools.partial(lambda c, t: with_images(views_40(), c, t), _c, _t)
for _n in SIZES:
    CASES[f"n_{_n}"] = functools.partial(lambda n: with_points(views_40(), n), _n)
CASES["points_f32"] = lambda: with_points(plane_sphere(), 330, np.float32)
VOLUME_CASES = ("textured_plane", "plane_sphere")


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


def run_reference(case, mode="blend", dtype=np.float64):
    return col.colour(case["points"], case["K"], case["ext"], case["width"], case["height"], case["images"], normals=case["normals"], visibility=case["visibility"],
                      occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], mode=mode, fill=case["fill"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def render_inputs(name, k, dtype=np.float64):
    """The cast of render view k of a volume case by the restatement: what ``colour_views`` starts from.  -> (depth (1, H, W) float32,
    normal (1, H, W, 3) float32)."""
    case = get(name)
    view = case["render"][k]
    r = ray.raycast(integrated(case), view["K"], view["ext"], view["width"], view["height"], case["min_weight"])
    return r["depth"].astype(np.float32), r["normal"].astype(np.float32)


def run_views_reference(case, name, k, mode="blend", dtype=np.float64):
    view = case["render"][k]
    depth, normal = render_inputs(name, k)
    return col.colour_views(view["K"], view["ext"], view["width"], view["height"], depth, case["K"], case["ext"], case["width"], case["height"], case["images"], normal_map=normal,
                            visibility=model_depth(case["volume_key"]), occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], mode=mode, fill=case["fill"], dtype=dtype)


def normal_points(name):
    """The points the point normals are tested at: the case's own and a few outside the box, on its faces' far side, and NaN."""
    case = get(name)
    vc = case["volume"]
    o, s, d = np.array(vc["origin"]), vc["voxel"], np.array(vc["dims"])
    extra = np.array([o - 0.37 * s, o + s * (d - 1) + 0.21 * s, o + s * (d - 1) * (0.5, 0.5, 1.7), [np.nan, 0.0, 0.0], o + s * (d - 1) * 0.4137])
    return np.concatenate([mesh(case["volume_key"])["vertices"], case["points"][:40], extra])


def _gap(a, b):
    both = np.isfinite(a.astype(np.float64)) & np.isfinite(b.astype(np.float64))
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def _result_gaps(r64, rL, name, g, dg):
    L = np.longdouble
    assert np.array_equal(r64["count"], rL["count"]) and np.array_equal(r64["best"], rL["best"]), name
    for key in ("colour", "weight"):
        big = float(np.nanmax(np.abs(rL[key]))) if rL[key].size and np.isfinite(rL[key].astype(np.float64)).any() else 1.0
        g = max(g, (_gap(r64[key].astype(L), rL[key]) / (big or 1.0), name))
    for key, q in rL["decisions"].items():
        assert np.array_equal(np.isnan(q), np.isnan(r64["decisions"][key])), (name, key)
        dg = max(dg, (_gap(r64["decisions"][key].astype(L), q), name))
    return g, dg


def measure_gaps():
    """-> ((COLOUR_GAP, case), (COLOUR_NORMAL_GAP, case), (COLOUR_DECISION_GAP, case)), float64 against longdouble."""
    L = np.longdouble
    g, ng, dg = (0.0, None), (0.0, None), (0.0, None)
    for name in CASES:
        case = get(name)
        for mode in col.MODES:
            g, dg = _result_gaps(run_reference(case, mode), run_reference(case, mode, L), name, g, dg)
    for name in VOLUME_CASES:
        case = get(name)
        for k in range(len(case["render"])):
            g, dg = _result_gaps(run_views_reference(case, name, k), run_views_reference(case, name, k, dtype=L), name, g, dg)
        n64, nL = col.point_normals(integrated(case), normal_points(name), 2), col.point_normals(integrated(case), normal_points(name), 2, L)
        assert np.array_equal(n64["status"], nL["status"]), name
        ng = max(ng, (_gap(n64["normal"].astype(L), nL["normal"]), name))
        for key, q in nL["decisions"].items():
            assert np.array_equal(np.isnan(q), np.isnan(n64["decisions"][key])), (name, key)
            dg = max(dg, (_gap(n64["decisions"][key].astype(L), q), name))
    return g, ng, dg


if __name__ == "__main__":
    g, ng, dg = measure_gaps()
    print(f"COLOUR_GAP {g[0]:.1e} ({g[1]})  COLOUR_NORMAL_GAP {ng[0]:.1e} ({ng[1]})  COLOUR_DECISION_GAP {dg[0]:.1e} ({dg[1]})")
    for name in CASES:
        case = get(name)
        for mode in col.MODES:
            r = run_reference(case, mode)
            worst = {k: float(np.nanmin(np.abs(v.astype(np.float64)))) if np.isfinite(v.astype(np.float64)).any() else np.inf for k, v in r["decisions"].items()}
            print(f"{name} {mode}: {len(case['points'])} points, count histogram {np.bincount(r['count'], minlength=1).tolist()}, closest call {r['closest'].min() if len(r['closest']) else np.inf:.2e} "
                  f"({min(worst, key=worst.get)})")
    for name in VOLUME_CASES:
        case = get(name)
        n = col.point_normals(integrated(case), normal_points(name), 2)
        print(f"{name}: {len(n['status'])} normal points, {int((n['status'] == 0).sum())} with a normal, closest call {n['closest'].min():.2e}")
        for k in range(len(case["render"])):
            r = run_views_reference(case, name, k)
            print(f"{name} render view {k}: {int(r['live'].sum())} live pixels, count histogram {np.bincount(r['count'].reshape(-1)).tolist()}, closest call {r['closest'].min():.2e}")
