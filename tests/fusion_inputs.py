"""Fixed inputs of the depth-map fusion tests, from seeded generators and analytic rendering: nothing is committed but this code.

Depth maps are rendered by intersecting every pixel's ray with a plane and a sphere, in ``np.longdouble`` and rounded once, for a small
ring of pinhole views that look at one point.  ``CASES`` names every input set the device tests use; tests/test_fusion_reference.py
asserts for each of them that no decision of the rule sits near its threshold."""
import functools

import numpy as np

# The float64-versus-longdouble gap of the restatement (tests/fusion_reference.py) over gap_inputs(): FUSE_GAP the largest |float64 -
# longdouble| coordinate of the fused points (and fused depth) over the masked pixels, relative to the largest coordinate; FUSE_DECISION_GAP the same for
# the decision quantities, each relative to its scale.  tests/test_fusion_reference.py recomputes both.
FUSE_GAP = 4.2e-16
FUSE_DECISION_GAP = 8.0e-16

PLANE = (np.array([0.12, -0.07, -1.0]) / np.linalg.norm([0.12, -0.07, -1.0]), -0.6 / np.linalg.norm([0.12, -0.07, -1.0]))   # n . X = h: through about (0, 0, 0.6)
SPHERE = (np.array([0.11, 0.04, -0.08]), 0.42)
TRANSFORM = np.array([[np.cos(0.3), 0.0, np.sin(0.3), 0.2], [0.0, 1.0, 0.0, -0.1], [-np.sin(0.3), 0.0, np.cos(0.3), 1.5]])


def look_at(centre, target=(0.0, 0.0, 0.0), roll=0.0):
    """-> (3, 4) world -> view of a camera at ``centre`` whose axis meets ``target``; rows right, down, forward."""
    c, tgt = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (tgt - c) / np.linalg.norm(tgt - c)
    r = np.cross([0.0, 1.0, 0.0], f)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    r, d = np.cos(roll) * r + np.sin(roll) * d, -np.sin(roll) * r + np.cos(roll) * d
    R = np.stack([r, d, f])
    return np.concatenate([R, (-R @ c)[:, None]], axis=1)


def ring_views(V, W, H, step_deg, radius=2.0):
    """V views on an arc about the origin, ``step_deg`` apart, with small differences in height, roll, focal length and centre."""
    K, E = np.zeros((V, 4)), np.zeros((V, 3, 4))
    for v in range(V):
        a = np.radians(step_deg) * (v - 0.5 * (V - 1)) + 0.003
        c = radius * (1.0 + 0.02 * np.sin(1.7 * v)) * np.array([np.sin(a), 0.11 * np.sin(2.3 * v + 0.4), -np.cos(a)])
        E[v] = look_at(c, target=(0.013, -0.007, 0.021), roll=0.02 * np.cos(1.3 * v))
        f = 0.93 * W * (1.0 + 0.015 * np.sin(0.9 * v))
        K[v] = [f, 0.5 * (W - 1) + 0.31 * np.sin(v + 0.2), f * 1.004, 0.5 * (H - 1) - 0.27 * np.cos(1.1 * v)]
    return K, E


def render(K, E, W, H, plane=PLANE, sphere=SPHERE):
    """z-depth maps (V, H, W) float64 of a plane (n, h) and a sphere (centre, radius), either may be None; +inf where a ray meets
    nothing.  Computed in longdouble and rounded once."""
    L = np.longdouble
    xs, ys = np.meshgrid(np.arange(W).astype(L), np.arange(H).astype(L))
    out = np.full((len(K), H, W), np.inf)
    for v in range(len(K)):
        Kv, R, t = K[v].astype(L), E[v][:, :3].astype(L), E[v][:, 3].astype(L)
        ray = np.stack([(xs - Kv[1]) / Kv[0], (ys - Kv[3]) / Kv[2], np.ones_like(xs)], axis=-1)   # z = 1: the parameter is the z-depth
        d = ray @ R          # R^T ray, per pixel
        o = -(R.T @ t)
        z = np.full((H, W), np.inf, dtype=L)
        with np.errstate(all="ignore"):
            if plane is not None:
                n, h = plane[0].astype(L), L(plane[1])
                s = (h - n @ o) / (d @ n)
                z = np.where(s > 0, np.minimum(z, s), z)
            if sphere is not None:
                c, r = sphere[0].astype(L), L(sphere[1])
                oc = o - c
                A, B, C = np.sum(d * d, axis=-1), np.sum(d * oc, axis=-1), oc @ oc - r * r
                disc = B * B - A * C
                s = (-B - np.sqrt(disc)) / A
                z = np.where((disc > 0) & (s > 0), np.minimum(z, s), z)
        out[v] = z.astype(np.float64)
    return out


def nearest_lists(V, n, descending=False):
    """View i's neighbours: the n views nearest in index (i - 1, i + 1, i - 2, ...); ``descending``: sorted from high to low."""
    out = []
    for i in range(V):
        l = [j for k in range(1, V) for j in (i - k, i + k) if 0 <= j < V][:n]
        out.append(sorted(l, reverse=True) if descending else l)
    return out


def add_noise(depth, seed, sigma=0.002):
    rng = np.random.default_rng(seed)
    return depth * (1.0 + sigma * rng.standard_normal(depth.shape))


PATCHES = ((0, 5, 15, 8, 24, 1.3), (2, 20, 40, 30, 50, 0.75), (3, 28, 36, 36, 60, 1.2))   # (view, y0, y1, x0, x1, factor)


def add_patches(depth, patches=PATCHES):
    out = depth.copy()
    for v, y0, y1, x0, x1, s in patches:
        out[v, y0:y1, x0:x1] *= s
    return out


INVALID_KINDS = (np.nan, np.inf, -np.inf, 0.0, -1.5)


def add_invalid(depth, seed):
    """Every kind of invalid depth, each at about 2 % of the pixels."""
    rng = np.random.default_rng(seed)
    out = depth.copy()
    pick = rng.integers(0, 50, size=depth.shape)
    for k, val in enumerate(INVALID_KINDS):
        out[pick == k] = val
    return out


@functools.lru_cache(maxsize=None)
def ring(V=10, W=64, H=48, step=8.0, noise_seed=None, patches=False, invalid_seed=None):
    """-> (depth (V, H, W) float64 read-only, K, E)."""
    K, E = ring_views(V, W, H, step)
    D = render(K, E, W, H)
    if noise_seed is not None:
        D = add_noise(D, noise_seed)
    if patches:
        D = add_patches(D)
    if invalid_seed is not None:
        D = add_invalid(D, invalid_seed)
    for a in (D, K, E):
        a.setflags(write=False)
    return D, K, E


@functools.lru_cache(maxsize=None)
def plane_ring(V=6, W=64, H=48, step=5.0):
    """Noise-free, the plane alone: nothing occludes, every view sees the plane wherever it looks."""
    K, E = ring_views(V, W, H, step)
    D = render(K, E, W, H, sphere=None)
    for a in (D, K, E):
        a.setflags(write=False)
    return D, K, E


@functools.lru_cache(maxsize=None)
def sphere_ring(V=6, W=64, H=48, step=5.0):
    """Noise-free, the sphere alone: every valid depth is a point of the sphere (+inf beside it)."""
    K, E = ring_views(V, W, H, step)
    D = render(K, E, W, H, plane=None)
    for a in (D, K, E):
        a.setflags(write=False)
    return D, K, E


@functools.lru_cache(maxsize=None)
def facing_pair(W=64, H=48):
    """Views 0 and 1 face each other.  View 0 (at z = -2, looking along +z) sees a wall at z = 4, beyond view 1 (at z = 3.2, looking
    along -z), which sees a wall at z = -2.6, beyond view 0: every surface point of either lies BEHIND the other.  View 2 stands beside
    view 0 and sees view 0's wall."""
    K = np.array([[60.0, 31.3, 60.5, 23.6], [58.0, 31.9, 58.2, 23.2], [61.0, 31.6, 61.3, 23.9]])
    E = np.stack([look_at((0.02, 0.01, -2.0)), look_at((-0.03, 0.02, 3.2), roll=0.03), look_at((0.25, -0.02, -2.0))])
    D = render(K, E, W, H, plane=(np.array([0.0, 0.0, 1.0]), 4.0), sphere=None)
    D[1] = render(K[1:2], E[1:2], W, H, plane=(np.array([0.0, 0.0, 1.0]), -2.6), sphere=None)[0]
    for a in (D, K, E):
        a.setflags(write=False)
    return D, K, E


@functools.lru_cache(maxsize=None)
def no_overlap(W=64, H=48):
    """Views 0, 1 look at one part of the plane, views 2, 3 at a part four metres to the side: neither pair's points fall into the other's images."""
    K, E = ring_views(2, W, H, 6.0)
    shift = np.array([4.0, 0.0, 0.0])
    E2 = E.copy()
    E2[:, :, 3] = E[:, :, 3] - E[:, :, :3] @ shift
    K, E = np.concatenate([K, K * 1.01]), np.concatenate([E, E2])
    D = render(K, E, W, H, sphere=None)
    for a in (D, K, E):
        a.setflags(write=False)
    return D, K, E


def _case(D, K, E, nb, **opts):
    return dict(depth=np.array(D), K=K, ext=E, neighbours=nb), opts   # a writable copy of the cached map: the caller may hand it to torch


def _ring_case(n=None, lists=None, dtype=np.float64, crop=None, V=10, W=64, H=48, step=8.0, noise=101, patches=True, invalid=202, **opts):
    D, K, E = ring(V, W, H, step, noise, patches, invalid)
    if crop is not None:   # the top-left crop of every map: the same views with a smaller sensor
        D = np.ascontiguousarray(D[:, :crop[1], :crop[0]])
    return _case(D.astype(dtype), K, E, nearest_lists(len(K), n) if lists is None else lists, **opts)


def _empty_list_case():
    nb = nearest_lists(10, 2)
    nb[4] = []
    return _ring_case(lists=nb)


# name -> () -> (inputs of fuse_depth_maps, options): every input set of tests/test_gpu_fusion.py
CASES = {
    "nbr1": lambda: _ring_case(1, min_views=1),
    "nbr2": lambda: _ring_case(2),
    "nbr9": lambda: _ring_case(9, min_views=3),
    "nbr32": lambda: _ring_case(32, V=33, W=24, H=16, step=2.0, patches=False, min_views=4),
    "empty_list": _empty_list_case,
    "descending": lambda: _ring_case(lists=nearest_lists(10, 4, descending=True), unique=True),
    "shape_67x45": lambda: _ring_case(3, W=67, H=45, patches=False),
    "shape_w_below_tile": lambda: _ring_case(3, crop=(20, 45), W=67, H=45, patches=False),
    "shape_h_below_tile": lambda: _ring_case(3, crop=(67, 5), W=67, H=45, patches=False),
    "shape_h1": lambda: _ring_case(3, crop=(64, 1), patches=False, min_views=1),
    "shape_1x1": lambda: _ring_case(3, crop=(1, 1), patches=False, min_views=1),
    "min_views_1": lambda: _ring_case(4, min_views=1),
    "min_views_len": lambda: _ring_case(4, min_views=4),
    "tight": lambda: _ring_case(4, px_tol=0.25, rel_tol=0.002),
    "loose": lambda: _ring_case(4, px_tol=3.0, rel_tol=0.05),
    "depth_f32": lambda: _ring_case(4, dtype=np.float32),
    "transform": lambda: _ring_case(4, transform=TRANSFORM),
    "unique": lambda: _ring_case(4, unique=True),
    "unique_f32": lambda: _ring_case(6, dtype=np.float32, unique=True, min_views=3, transform=TRANSFORM),
    "noise_free": lambda: _ring_case(4, noise=None, patches=False, invalid=None),
    "facing": lambda: _case(*facing_pair(), [[1, 2], [0, 2], [1, 0]], min_views=1),
    "no_overlap": lambda: _case(*no_overlap(), [[1, 2, 3], [0, 3], [3, 0, 1], [2, 1]], min_views=1),
}


def gap_inputs():
    """The input sets FUSE_GAP and FUSE_DECISION_GAP are measured over: every case of the device tests."""
    return [make() for make in CASES.values()]


# ---- a ring of cameras looking at a textured plane: the images of fuse_stereo_pairs ------------------------------------------------------------
STEREO_Z0, STEREO_RES = 1.0, (96, 64)


def texture(X, Y):
    return 127.5 + 45.0 * np.sin(61.0 * X + 2.0 * np.sin(23.0 * Y)) + 40.0 * np.sin(47.0 * Y + 13.0 * X * X) + 35.0 * np.sin(29.0 * (X + Y) + 5.0 * np.cos(37.0 * X))


@functools.lru_cache(maxsize=None)
def stereo_ring(C=5, step=7.0):
    """C distortion-free cameras on an arc one metre from the point (0, 0, Z0) of the textured plane Z = Z0, ``step`` degrees apart.
    -> (images (C, H, W) uint8, intr (C, 9), ext (C, 3, 4))."""
    W, H = STEREO_RES
    intr, ext, images = np.zeros((C, 9)), np.zeros((C, 3, 4)), np.zeros((C, H, W), dtype=np.uint8)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for c in range(C):
        a = np.radians(step) * (c - 0.5 * (C - 1))
        centre = np.array([np.sin(a), 0.004 * np.sin(2.0 * c), STEREO_Z0 - np.cos(a)])
        ext[c] = look_at(centre, target=(0.0, 0.0, STEREO_Z0), roll=0.004 * np.cos(c))
        intr[c, :4] = [118.0 + 0.7 * c, 47.1 + 0.2 * c, 118.6 + 0.6 * c, 31.6 - 0.15 * c]
        ray = np.stack([(xs - intr[c, 1]) / intr[c, 0], (ys - intr[c, 3]) / intr[c, 2], np.ones_like(xs)], axis=-1) @ ext[c][:, :3]
        s = (STEREO_Z0 - centre[2]) / ray[..., 2]
        P = centre + s[..., None] * ray
        images[c] = np.clip(np.rint(texture(P[..., 0], P[..., 1])), 0, 255).astype(np.uint8)
    return images, intr, ext
