"""The NumPy restatement of the image-mapping kernels (tests/imagemap_reference.py) against what it must reproduce — the reference's own
nb_undistort_arr / nb_distort (golden), exact identities, torch's grid_sample as an independent sampler — the properties of
imaging.rectify_pair, and the conditions that the device tests (tests/test_gpu_imagemap.py) rely on, asserted on the restatement alone.
The argument errors of the front ends are here too: they are raised before anything touches a device.  No device here."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest

from pycamset_amd import _capi, imaging
from tests import imagemap_inputs as inp
from tests import imagemap_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "undistort_points.npz"
W, H = inp.SENSOR
VIEWS = inp.views()


def view_of(name, cam):
    R, K = VIEWS[name]
    return (None if R is None else R[cam]), (None if K is None else K[cam])


@functools.lru_cache(maxsize=None)
def maps_of(name, cam, dst, ld=False):
    R, K = view_of(name, cam)
    return ref.build_maps(inp.INTR[cam], dst[0], dst[1], R, K, dtype=np.longdouble if ld else np.float64)


@functools.lru_cache(maxsize=None)
def remapped(name, dst, interpolation, dtype, C, ld=False):
    """The restatement's remap of the batch under one view: a list of dicts, one per image.  The extended-precision twin runs the
    sampler in extended precision over the extended-precision map."""
    imgs = inp.images(dtype, C)
    return [ref.remap(imgs[i], maps_of(name, cam, dst, ld), interpolation, inp.BORDER[dtype][:C], dtype=np.longdouble if ld else np.float64)
            for i, cam in enumerate(inp.BATCH_CAMS)]


ALL_REMAPS = [(v, d, ip, dt, C) for v in VIEWS for d in inp.DESTS for ip in ref.INTERPOLATIONS for dt in inp.DTYPES for C in inp.CHANNELS]


# ---- golden and round trip ---------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_golden():
    g = np.load(GOLDEN)
    assert np.array_equal(g["points"], inp.points()) and np.array_equal(g["intr"], inp.INTR), "the golden was made from other inputs"
    for c in range(inp.N_CAMS):
        for kind, fn in (("undistort", ref.undistort_points), ("distort", ref.distort_points)):
            ours, theirs = fn(inp.points(), inp.INTR[c]), g[f"{kind}_{c}"]
            rel = np.max(np.abs(ours - theirs) / np.abs(theirs))
            print(f"camera {c} {kind}: largest relative difference to the reference {rel:.2e}")
            assert rel <= 1e-14, (c, kind, rel)


def test_distort_of_undistort_returns_the_point_as_far_as_five_steps_go():
    for c in range(inp.N_CAMS):
        p = ref.pixel_grid(W, H).astype(np.float64)
        back = ref.distort_points(ref.undistort_points(p, inp.INTR[c]), inp.INTR[c])
        print(f"camera {c}: largest |distort(undistort(p)) - p| over the sensor after 5 steps: {np.max(np.abs(back - p)):.3e} px")
    assert np.max(np.abs(ref.distort_points(ref.undistort_points(p, inp.INTR[2]), inp.INTR[2]) - p)) == 0.0   # no distortion: exact


# ---- identity properties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", inp.DESTS)
def test_identity_view_without_distortion_is_the_pixel_grid_exactly(dst):
    m = maps_of("identity", 2, dst)
    g = ref.pixel_grid(*dst)
    assert np.array_equal(m[0].ravel(), g[:, 0]) and np.array_equal(m[1].ravel(), g[:, 1])


@pytest.mark.parametrize("dtype", inp.DTYPES)
@pytest.mark.parametrize("interpolation", ref.INTERPOLATIONS)
def test_an_integer_shift_of_the_centre_shifts_the_image_exactly(interpolation, dtype):
    dx, dy = 3, -2
    K_new = inp.INTR[2, :4] + np.array([0.0, dx, 0.0, dy])
    m = ref.build_maps(inp.INTR[2], W, H, None, K_new)
    g = ref.pixel_grid(W, H)
    assert np.array_equal(m[0].ravel(), g[:, 0] - dx) and np.array_equal(m[1].ravel(), g[:, 1] - dy)
    for C in inp.CHANNELS:
        src = inp.images(dtype, C)[0]
        border = np.asarray(inp.BORDER[dtype][:C])
        out = ref.remap(src, m, interpolation, border)["out"]
        expect = np.empty_like(src)
        expect[:] = border.astype(src.dtype)
        ys, xs = np.arange(H), np.arange(W)
        oky, okx = (ys - dy >= 0) & (ys - dy < H), (xs - dx >= 0) & (xs - dx < W)
        expect[np.ix_(oky, okx)] = src[np.ix_(ys[oky] - dy, xs[okx] - dx)]
        assert np.array_equal(out, expect), (interpolation, dtype, C)


@pytest.mark.parametrize("dtype,value", [("uint8", 173), ("float32", 0.7)])
def test_a_bicubic_remap_of_a_constant_image_is_constant(dtype, value):
    src = np.full((H, W, 1), value, dtype=dtype)
    for name in VIEWS:
        m = maps_of(name, 1, inp.DESTS[0])
        out = ref.remap(src, m, ref.BICUBIC, [float(src[0, 0, 0])])["out"]
        assert np.all(out == src[0, 0, 0]), name   # also at the border and where no tap is inside: the border value is the constant


# ---- map against rays ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", range(inp.N_CAMS))
def test_rays_projected_without_distortion_land_on_the_undistorted_points(cam):
    g = ref.pixel_grid(W, H)
    pinhole = np.concatenate([inp.INTR[cam, :4], np.zeros(5)])
    for normalised in (False, True):
        rays = ref.pixel_rays(g, inp.INTR[cam], normalised=normalised)
        u, v, z = ref.project(pinhole, np.eye(3), rays)
        d = np.max(np.abs(np.stack([u, v], axis=1) - ref.undistort_points(g, inp.INTR[cam])))
        print(f"camera {cam} normalised={normalised}: {d:.2e} px")
        assert d <= 64 * np.finfo(np.float64).eps * max(W, H) and np.all(z > 0)   # a handful of roundings at coordinates below 64 px


# ---- rectify_pair ----------------------------------------------------------------------------------------------------------------------------
def stereo_pair():
    from scipy.spatial.transform import Rotation

    Ra = Rotation.from_rotvec([0.02, -0.05, 0.01]).as_matrix()
    ea = np.concatenate([Ra, np.array([[0.1], [-0.05], [0.2]])], axis=1)
    Rrel = Rotation.from_rotvec([0.03, 0.06, -0.02]).as_matrix()           # X_b = Rrel X_a + T: b sits to the right of a
    T = np.array([-0.30, 0.012, 0.02])
    eb = np.concatenate([Rrel @ Ra, (Rrel @ ea[:, 3] + T)[:, None]], axis=1)
    return inp.INTR[0], ea, inp.INTR[1], eb


def restated_undistort(pts, intr):
    return ref.undistort_points(pts, intr)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_rectify_pair_rotations_rows_disparity_and_q(alpha):
    ka, ea, kb, eb = stereo_pair()
    R_a, R_b, K_new, Q = imaging.rectify_pair(ka, ea, kb, eb, inp.SENSOR, alpha=alpha, undistort=restated_undistort)
    for R in (R_a, R_b):
        assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.max(np.abs(R.T @ R - np.eye(3))) <= 1e-14
    rng = np.random.default_rng(3)
    Xa = rng.uniform([-0.3, -0.2, 1.5], [0.3, 0.2, 3.0], size=(200, 3))
    Xw = (Xa - ea[:, 3]) @ ea[:, :3]                                         # R^T (X - t)
    Xb = Xw @ eb[:, :3].T + eb[:, 3]
    assert np.all(Xa[:, 2] > 0) and np.all(Xb[:, 2] > 0)
    f, cx, _, cy = K_new
    pa, pb = Xa @ R_a.T, Xb @ R_b.T
    ua, va = f * pa[:, 0] / pa[:, 2] + cx, f * pa[:, 1] / pa[:, 2] + cy
    ub, vb = f * pb[:, 0] / pb[:, 2] + cx, f * pb[:, 1] / pb[:, 2] + cy
    print(f"alpha {alpha}: f {f:.3f}, largest row difference {np.max(np.abs(va - vb)):.2e} px, disparity {np.min(ua - ub):.3f} .. {np.max(ua - ub):.3f}")
    assert np.max(np.abs(va - vb)) <= 1e-9
    assert np.all(ua - ub > 0)
    hom = np.stack([ua, va, ua - ub, np.ones_like(ua)], axis=1) @ Q.T
    assert np.max(np.abs(hom[:, :3] / hom[:, 3:] - pa) / np.linalg.norm(pa, axis=1, keepdims=True)) <= 1e-9


def test_rectify_pair_outline_rules():
    ka, ea, kb, eb = stereo_pair()
    # alpha = 1: every border pixel of both sources maps inside the new image
    R_a, R_b, K_new, _ = imaging.rectify_pair(ka, ea, kb, eb, inp.SENSOR, alpha=1.0, undistort=restated_undistort)
    border = np.concatenate(imaging._outline(inp.SENSOR))
    for K, R in ((ka, R_a), (kb, R_b)):
        rays = ref.pixel_rays(border, K) @ R.T
        u, v = K_new[0] * rays[:, 0] / rays[:, 2] + K_new[1], K_new[2] * rays[:, 1] / rays[:, 2] + K_new[3]
        assert u.min() >= 0 and u.max() <= W - 1 and v.min() >= 0 and v.max() <= H - 1, (u.min(), u.max(), v.min(), v.max())
    # alpha = 0: every destination pixel of both maps inside its source
    R_a, R_b, K_new, _ = imaging.rectify_pair(ka, ea, kb, eb, inp.SENSOR, alpha=0.0, undistort=restated_undistort)
    for K, R in ((ka, R_a), (kb, R_b)):
        m = ref.build_maps(K, W, H, R, K_new)
        assert m[0].min() >= 0 and m[0].max() <= W - 1 and m[1].min() >= 0 and m[1].max() <= H - 1, (m[0].min(), m[0].max(), m[1].min(), m[1].max())


# ---- the gap ---------------------------------------------------------------------------------------------------------------------------------
def measured_gap():
    gap = np.zeros(4)
    pts = inp.points()
    g = ref.pixel_grid(W, H)
    for c in range(inp.N_CAMS):
        for fn, args in ((ref.undistort_points, (5,)), (ref.undistort_points, (1,)), (ref.distort_points, ())):
            gap[0] = max(gap[0], np.max(np.abs(fn(pts, inp.INTR[c], *args) - fn(pts, inp.INTR[c], *args, dtype=np.longdouble))))
        for normalised in (False, True):
            for world in (False, True):
                for distort in (False, True):
                    for p in (pts, g):
                        a = ref.pixel_rays(p, inp.INTR[c], inp.EXT[c], normalised, world, distort)
                        b = ref.pixel_rays(p, inp.INTR[c], inp.EXT[c], normalised, world, distort, dtype=np.longdouble)
                        gap[1] = max(gap[1], np.max(np.abs(a - b)))
        for name in VIEWS:
            for dst in inp.DESTS:
                a, b = maps_of(name, c, dst), maps_of(name, c, dst, True)
                assert np.array_equal(np.isnan(a), np.isnan(b))
                fin = np.isfinite(a)
                gap[2] = max(gap[2], float(np.max(np.abs(a - b)[fin] / inp.map_scale(a[fin]), initial=0.0)))
    for key in ALL_REMAPS:
        for a, b in zip(remapped(*key), remapped(*key, True)):
            assert np.array_equal(a["valid"], b["valid"]) and np.array_equal(a["some"], b["some"]), key
            gap[3] = max(gap[3], np.max(np.abs(a["raw"] - b["raw"])) / inp.image_range(key[3]))
    return gap


def test_imagemap_gap_is_the_pinned_one():
    gap = measured_gap()
    print("IMAGEMAP_GAP measured", gap)
    pinned = np.array(inp.IMAGEMAP_GAP)
    assert np.all(gap <= pinned) and np.all(gap >= 0.5 * pinned), (gap, pinned)


# ---- conditions the device tests rely on -------------------------------------------------------------------------------------------------
def test_no_sampled_coordinate_sits_where_a_decision_flips():
    """Within 1e-6 px of a coordinate at which a tap enters or leaves the source (validity, the border's share) or, for nearest, at
    which the chosen pixel changes, two correct evaluations may decide differently.  A coordinate exactly ON such a value is no risk
    when it is exact in both precisions — the dyadic camera 2 under the identity view produces integers, identically everywhere."""
    for name in VIEWS:
        for dst in inp.DESTS:
            for cam in set(inp.BATCH_CAMS):
                m, mld = maps_of(name, cam, dst), maps_of(name, cam, dst, True)
                for axis, size in ((0, W), (1, H)):
                    s, sld = m[axis].ravel(), mld[axis].ravel()
                    s, sld = s[np.isfinite(s)], sld[np.isfinite(s)]
                    exact = (s == sld) & (s == np.rint(s))
                    for ip in ref.INTERPOLATIONS:
                        for k in inp.flip_values(ip, size):
                            near = (np.abs(s - k) < 1e-6) & ~exact
                            assert not np.any(near), (name, dst, cam, ip, k, s[near])
                    inside = (s > -1) & (s < size) & ~exact
                    half = np.abs(s[inside] - np.floor(s[inside]) - 0.5)
                    assert not np.any(half < 1e-6), (name, dst, cam, "nearest")


def test_few_uint8_values_sit_near_a_rounding_tie():
    """The only uint8 pixels on which the device may differ from the restatement (by one grey level) are those whose unrounded value
    lies within 8 x the value gap of a half-integer: fewer than 1 % of every result."""
    tol = 8.0 * inp.IMAGEMAP_GAP[3] * 255.0
    worst = 0.0
    for key in ALL_REMAPS:
        if key[3] != "uint8":
            continue
        for r in remapped(*key):
            share = float(np.mean(inp.near_tie_mask(r["raw"], tol)))
            worst = max(worst, share)
            assert share < 0.01, (key, share)
    print(f"largest share of near ties: {worst:.4%} (tolerance {tol:.2e} grey levels)")


# ---- independent check of the sampler --------------------------------------------------------------------------------------------------------
def grid_sample_reference(src, maps, interpolation):
    """torch.nn.functional.grid_sample (align_corners=True, zero padding) on one float32 image (Hs, Ws, C) over a map (2, Hd, Wd)."""
    import torch

    Hs, Ws = src.shape[:2]
    grid = torch.from_numpy(np.stack([2.0 * maps[0] / (Ws - 1) - 1.0, 2.0 * maps[1] / (Hs - 1) - 1.0], axis=-1).astype(np.float32))[None]
    out = torch.nn.functional.grid_sample(torch.from_numpy(np.ascontiguousarray(src.transpose(2, 0, 1)))[None], grid, mode=interpolation, padding_mode="zeros",
                                          align_corners=True)
    return out[0].permute(1, 2, 0).numpy()


def measured_grid_sample_gap():
    gap = {}
    for ip in (ref.BILINEAR, ref.BICUBIC):
        worst = 0.0
        for name in VIEWS:
            for dst in inp.DESTS:
                for C in inp.CHANNELS:
                    imgs = inp.images("float32", C)
                    for i, cam in enumerate(inp.BATCH_CAMS):
                        m = maps_of(name, cam, dst)
                        ours = ref.remap(imgs[i], m, ip, None)["out"]
                        theirs = grid_sample_reference(imgs[i], m, ip)
                        ok = np.isfinite(m[0]) & np.isfinite(m[1])
                        if np.any(ok):
                            worst = max(worst, float(np.max(np.abs(ours[ok].astype(np.float64) - theirs[ok]))) / inp.image_range("float32"))
        gap[ip] = worst
    return gap


def test_grid_sample_agrees_with_the_restatement():
    gap = measured_grid_sample_gap()
    print("GRID_SAMPLE_GAP measured", gap)
    for k, ip in enumerate((ref.BILINEAR, ref.BICUBIC)):
        assert 0.25 * inp.GRID_SAMPLE_GAP[k] <= gap[ip] <= inp.GRID_SAMPLE_GAP[k], (ip, gap[ip], inp.GRID_SAMPLE_GAP[k])


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------
def raises_naming(name, fn, *args, **kw):
    with pytest.raises((ValueError, _capi.PcsError)) as e:
        fn(*args, **kw)
    assert name in str(e.value), (name, str(e.value))
    if isinstance(e.value, _capi.PcsError):
        assert e.value.code == _capi.PCS_ERR_ARG


def test_argument_errors_are_raised_before_the_device_and_name_the_argument():
    pts, imgs = inp.points(), inp.images("uint8", 1)
    cams = np.array(inp.BATCH_CAMS)
    # wrong slab shapes
    raises_naming("intr", imaging.undistort_points, pts, inp.INTR[:, :8])
    raises_naming("intr", imaging.sensor_map, np.zeros((2, 9)), inp.SENSOR)
    raises_naming("ext", imaging.pixel_rays, pts, inp.INTR, ext=np.zeros((3, 5)), world=True)
    raises_naming("ext", imaging.pixel_rays, pts, inp.INTR, world=True)
    raises_naming("pts", imaging.distort_points, np.zeros((4, 3)), inp.INTR)
    raises_naming("R_new", imaging.undistort_images, imgs, cams, inp.INTR, R_new=np.zeros((2, 3, 3)))
    raises_naming("K_new", imaging.undistort_rectify_map, inp.INTR, (8, 8), K_new=np.zeros((3, 5)))
    raises_naming("depth", imaging.sensor_map, inp.INTR, inp.SENSOR, depth=np.zeros((3, 3)))
    # C = 2
    raises_naming("C", imaging.undistort_images, np.zeros((5, H, W, 2), dtype=np.uint8), cams, inp.INTR)
    raises_naming("C", imaging.check_remap_args, 5, 2, "uint8", inp.SENSOR, W * 2, inp.SENSOR, W * 2, "bilinear")
    raises_naming("dtype", imaging.check_remap_args, 5, 1, "float64", inp.SENSOR, W * 8, inp.SENSOR, W * 8, "bilinear")
    # unknown interpolation
    raises_naming("interpolation", imaging.undistort_images, imgs, cams, inp.INTR, interpolation="lanczos")
    raises_naming("interpolation", imaging.remap_images, imgs, np.zeros((2, 4, 4), dtype=np.float32), interpolation="area")
    # pitch below the row size
    raises_naming("src_pitch", imaging.check_remap_args, 5, 3, "uint8", inp.SENSOR, W * 3 - 1, inp.SENSOR, W * 3, "bilinear")
    raises_naming("dst_pitch", imaging.check_remap_args, 5, 1, "float32", inp.SENSOR, W * 4, (67, 45), 67 * 4 - 4, "nearest")
    raises_naming("pitch", imaging.check_remap_args, 5, 1, "float32", inp.SENSOR, W * 4 + 2, inp.SENSOR, W * 4, "nearest")
    # a camera index out of range
    raises_naming("cams", imaging.undistort_images, imgs, [0, 1, 2, 3, 0], inp.INTR)
    raises_naming("cams", imaging.undistort_points, pts, inp.INTR, cams=np.full(pts.shape[0], -1))
    raises_naming("cam", imaging.sensor_map, inp.INTR, inp.SENSOR, cam=3)
    raises_naming("map_index", imaging.remap_images, imgs, np.zeros((2, 2, 4, 4), dtype=np.float32), map_index=[0, 1, 2, 0, 0])
    raises_naming("iters", imaging.undistort_points, pts, inp.INTR, iters=-1)
    raises_naming("mode", imaging.sensor_map, inp.INTR, inp.SENSOR, mode="fisheye")


def test_the_c_abi_refuses_a_null_handle_without_a_device():
    lib = _capi.lib()
    assert lib.pcs_imap_create(None, 0) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_set_cameras(None, 1, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_set_view(None, None, None) == _capi.PCS_ERR_ARG and b"pcs_imap_set_view" in lib.pcs_last_error()
    assert lib.pcs_imap_points(None, 0, 0, None, 0, None, 5, 0, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_rays(None, 0, 1, 1, 0, 5, None, 0, None, 0, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_build_maps(None, 0, 1, 1, None, 0, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_remap(None, 0, None, None, 1, 1, 1, 0, 1, None, 1, 1, 1, None, 0, 0, 0, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_last_kernel_ms(None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_imap_destroy(None) == _capi.PCS_OK
