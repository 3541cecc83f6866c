"""The image-mapping kernels on the device (include/pcs_hip.h pcs_imap_*, csrc/ba_imagemap.hpp) against their NumPy restatement
(tests/imagemap_reference.py), at the smallest shapes at which they can go wrong, and the front ends of pycamset_amd/imaging.py.

The bounds.  IMAGEMAP_GAP (tests/imagemap_inputs.py) is the largest float64-versus-extended difference of the restatement over the
fixed inputs, per output kind: point (px), ray component, map coordinate (px, relative beyond the sensor: map_scale), interpolated
value (relative to the image's range); tests/test_imagemap_reference.py recomputes it.  The device is held to MARGIN = 8 x these: the
margin the other suites use for a different order of the same operations and fused multiply-adds.  What is discrete must be identical:
validity planes, NaN patterns, and 8-bit results except on the pixels whose unrounded value lies within the bound of a rounding tie
(there: one grey level), which the conditions asserted in tests/test_imagemap_reference.py make a fair demand."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, imaging
from tests import imagemap_inputs as inp
from tests import imagemap_reference as ref
from tests import test_imagemap_reference as cpu

pytestmark = pytest.mark.gpu
MARGIN = 8.0
G_POINT, G_RAY, G_MAP, G_VALUE = inp.IMAGEMAP_GAP
W, H = inp.SENSOR
EPS = float(np.finfo(np.float64).eps)
DEV = torch.device("cuda", 0)
VIEWS = inp.views()
ROW_CAMS = np.arange(inp.points().shape[0]) % inp.N_CAMS   # the camera of every point of the point tests


@functools.lru_cache(maxsize=None)
def mapper():
    m = imaging.ImageMapper(0)
    m.set_cameras(inp.INTR, inp.EXT)
    return m


def per_camera(fn, pts, *args, **kw):
    """The restatement row by row: ``fn(points of camera c, intr[c], ...)`` scattered back."""
    out = None
    for c in range(inp.N_CAMS):
        rows = ROW_CAMS == c
        r = fn(pts[rows], inp.INTR[c], *args, **{k: (v[c] if k == "ext" else v) for k, v in kw.items()})
        if out is None:
            out = np.empty((pts.shape[0], r.shape[1]))
        out[rows] = r
    return out


# ---- points ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [5, 1])
def test_undistort_and_distort_points(iters):
    pts = inp.points()
    dev = imaging.undistort_points(pts, inp.INTR, ROW_CAMS, iters=iters)
    d = np.max(np.abs(dev - per_camera(ref.undistort_points, pts, iters)))
    print(f"undistort iters={iters}: {d:.2e} px (bound {MARGIN * G_POINT:.2e})")
    assert d <= MARGIN * G_POINT
    dev = imaging.distort_points(pts, inp.INTR, ROW_CAMS)
    d = np.max(np.abs(dev - per_camera(ref.distort_points, pts)))
    print(f"distort: {d:.2e} px")
    assert d <= MARGIN * G_POINT


@pytest.mark.parametrize("iters", [5, 1])
@pytest.mark.parametrize("distort", [True, False])
@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("mode", ["linear", "normalised"])
def test_pixel_rays(mode, world, distort, iters):
    pts = inp.points()
    dev = imaging.pixel_rays(pts, inp.INTR, ROW_CAMS, ext=inp.EXT, mode=mode, world=world, distort=distort, iters=iters)
    want = per_camera(ref.pixel_rays, pts, ext=inp.EXT, normalised=mode == "normalised", world=world, distort=distort, iters=iters)
    d = np.max(np.abs(dev - want))
    print(f"rays {mode} world={world} distort={distort} iters={iters}: {d:.2e} (bound {MARGIN * G_RAY:.2e})")
    assert dev.shape == (pts.shape[0], 3) and d <= MARGIN * G_RAY


def test_the_reference_golden_through_the_device():
    g = np.load(cpu.GOLDEN)
    for c in range(inp.N_CAMS):
        for kind, fn in (("undistort", imaging.undistort_points), ("distort", imaging.distort_points)):
            dev, theirs = fn(g["points"], inp.INTR, c), g[f"{kind}_{c}"]
            assert np.all(np.abs(dev - theirs) <= MARGIN * G_POINT + 1e-14 * np.abs(theirs)), (c, kind, np.max(np.abs(dev - theirs)))


def test_a_point_tensor_on_the_device_stays_there_and_one_index_serves_all_rows():
    pts = inp.points()
    t = torch.from_numpy(pts).to(DEV)
    out = imaging.undistort_points(t, inp.INTR, cams=1)
    assert isinstance(out, torch.Tensor) and out.device == t.device
    assert np.array_equal(out.cpu().numpy(), imaging.undistort_points(pts, inp.INTR, np.full(pts.shape[0], 1)))


# ---- ray maps ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [inp.SENSOR, (1, 1)])
@pytest.mark.parametrize("distort", [True, False])
@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("mode", ["linear", "normalised"])
def test_sensor_map(mode, world, distort, res):
    for cam in range(inp.N_CAMS):
        ext = inp.EXT if world else None
        dev = imaging.sensor_map(inp.INTR, res, mode=mode, distort=distort, ext=ext, cam=cam)
        want = ref.ray_map(inp.INTR[cam], res[0], res[1], inp.EXT[cam], mode == "normalised", world, distort)
        assert dev.shape == (res[1], res[0], 3) and dev.dtype == np.float64
        assert np.max(np.abs(dev - want)) <= MARGIN * G_RAY, (cam, np.max(np.abs(dev - want)))
        dev32 = imaging.sensor_map(inp.INTR, res, mode=mode, distort=distort, ext=ext, cam=cam, dtype=np.float32)
        assert dev32.dtype == np.float32 and np.array_equal(dev32, dev.astype(np.float32))   # the float64 result rounded once


@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("depth_dtype", [np.float64, np.float32])
def test_depth_to_points(world, depth_dtype):
    depth = inp.depth_image().astype(depth_dtype)
    for cam in (0, 1):
        dev = imaging.depth_to_points(depth, inp.INTR, ext=inp.EXT if world else None, cam=cam)
        want = ref.ray_map(inp.INTR[cam], W, H, inp.EXT[cam], False, world, True, depth=depth)
        nan = ~np.isfinite(depth)
        assert np.array_equal(np.isnan(dev), np.broadcast_to(nan[:, :, None], dev.shape)) and np.array_equal(np.isnan(want), np.isnan(dev))
        # |ray error| x |depth| plus the rounding of position + ray * depth itself
        bound = MARGIN * G_RAY * float(np.nanmax(np.abs(depth[~nan]))) + 4 * EPS * float(np.max(np.abs(want[~nan])))
        assert np.max(np.abs(dev[~nan] - want[~nan])) <= bound


# ---- maps -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", inp.DESTS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_undistort_rectify_map(name, dst):
    R, K = VIEWS[name]
    dev = imaging.undistort_rectify_map(inp.INTR, dst, R, K, dtype=np.float64)
    dev32 = imaging.undistort_rectify_map(inp.INTR, dst, R, K)
    assert dev.shape == (inp.N_CAMS, 2, dst[1], dst[0]) and dev32.dtype == np.float32
    behind = 0
    for cam in range(inp.N_CAMS):
        want = cpu.maps_of(name, cam, dst)
        assert np.array_equal(np.isnan(dev[cam]), np.isnan(want)) and np.array_equal(np.isnan(dev32[cam]), np.isnan(want))
        fin = ~np.isnan(want)
        behind += int(np.sum(~fin))
        err = np.abs(dev[cam][fin] - want[fin]) / inp.map_scale(want[fin])
        assert np.max(err, initial=0.0) <= MARGIN * G_MAP, (cam, np.max(err))
        near = fin & (np.abs(np.where(fin, want, 0.0)) < 1e6)
        err32 = np.abs(dev32[cam][near].astype(np.float64) - want[near])
        assert np.all(err32 <= MARGIN * G_MAP * inp.map_scale(want[near]) + np.spacing(np.abs(want[near]).astype(np.float32)))
    one = imaging.undistort_rectify_map(inp.INTR, dst, R, K, cams=1, dtype=np.float64)
    assert one.shape == (2, dst[1], dst[0]) and np.array_equal(one, dev[1], equal_nan=True)
    if name == "past90" and dst == inp.DESTS[0]:
        assert behind > 0   # the view does look behind the camera


# ---- remap ------------------------------------------------------------------------------------------------------------------------------------
SENTINEL = {"uint8": 77, "float32": -123.5}


def padded(n, height, width, C, dtype, pad, fill=None, data=None):
    """A device tensor (n, height, width, C) whose rows lie ``pad`` elements apart more than they need: (view, whole buffer)."""
    buf = torch.full((n, height, width * C + pad), SENTINEL[dtype] if fill is None else fill, dtype=getattr(torch, dtype), device=DEV)
    view = buf[:, :, : width * C].view(n, height, width, C)
    if data is not None:
        view.copy_(torch.from_numpy(data).to(DEV))
    return view, buf


def run_remap(imgs, dst, interpolation, border, pad, cams, maps=None):
    """One launch through the handle: -> (out (n, Hd, Wd, C), valid (n, Hd, Wd)) as NumPy arrays; checks that the padding stays."""
    n, _, _, C = imgs.shape
    dtype = str(imgs.dtype)
    item = imgs.dtype.itemsize
    src, _ = padded(n, H, W, C, dtype, pad, data=imgs)
    out, obuf = padded(n, dst[1], dst[0], C, dtype, pad)
    valid = torch.full((n, dst[1], dst[0]), 9, dtype=torch.uint8, device=DEV)
    kw = {}
    if maps is not None:
        kw = dict(d_map=maps.data_ptr(), map_f32=maps.dtype == torch.float32, n_maps=maps.shape[0])
    mapper().remap(cams, src.data_ptr(), (W, H), C, dtype, (W * C + pad) * item, out.data_ptr(), dst, (dst[0] * C + pad) * item, interpolation=interpolation, border=border,
                   d_valid=valid.data_ptr(), stream=torch.cuda.current_stream(0).cuda_stream, **kw)
    torch.cuda.synchronize()
    if pad:
        assert bool(torch.all(obuf[:, :, dst[0] * C:] == SENTINEL[dtype])), "the remap wrote into the row padding"
    return out.cpu().numpy(), valid.cpu().numpy()


def check_remap(out, valid, want, dtype, what, extra=0.0, coord_ulp=None):
    """Device results of the batch against the restatement's.  ``extra``: what a float32 map adds to the value bound (absolute)."""
    rng = inp.image_range(dtype)
    bound = MARGIN * G_VALUE * rng + extra
    for i, r in enumerate(want):
        assert valid is None or np.array_equal(valid[i], r["valid"]), (what, i, "validity")
        raw = r["raw"].astype(np.float64)
        if dtype == "uint8":
            if extra == 0.0:
                tie = inp.near_tie_mask(raw, bound)
                diff = np.abs(out[i].astype(np.int64) - r["out"].astype(np.int64))
                assert np.all(diff[~tie] == 0) and np.all(diff <= 1), (what, i, int(diff.max()), int(np.sum(diff[~tie] != 0)))
            else:
                assert np.all(np.abs(out[i].astype(np.float64) - np.clip(raw, 0, 255)) <= 0.5 + bound), (what, i)
        else:
            err = np.abs(out[i].astype(np.float64) - raw)
            lim = bound + 0.51 * np.spacing(np.abs(raw).astype(np.float32)).astype(np.float64)
            assert np.all(err <= lim), (what, i, float(np.max(err - lim)))


@functools.lru_cache(maxsize=None)
def lipschitz(interpolation):
    """How fast the interpolant can change per pixel of coordinate change, in units of the image's largest difference D between any
    two values (border included), derived from the weights themselves.  Along one axis the value is sum w_i(t) v_i with sum w_i = 1, so
    its slope is sum w_i'(t) v_i = sum w_i'(t) (v_i - c) <= (sum |w_i'|) D / 2; the other axis only mixes such values with weights of
    absolute sum S = max_t sum |w_i(t)|.  Bilinear: w = (1 - t, t): slope <= D, S = 1."""
    if interpolation == ref.BILINEAR:
        return 1.0
    t = np.linspace(0.0, 1.0, 20001)
    w = np.stack(ref.cubic_weights(t))
    slope = np.max(np.sum(np.abs(np.gradient(w, t, axis=1)), axis=0)) / 2.0
    return float(slope * np.max(np.sum(np.abs(w), axis=0)))


@pytest.mark.parametrize("pad", inp.PITCH_PAD)
@pytest.mark.parametrize("dst", inp.DESTS)
@pytest.mark.parametrize("C", inp.CHANNELS)
@pytest.mark.parametrize("dtype", inp.DTYPES)
@pytest.mark.parametrize("interpolation", ref.INTERPOLATIONS)
def test_remap_fused_and_mapped(interpolation, dtype, C, dst, pad):
    imgs = inp.images(dtype, C)
    border = inp.BORDER[dtype][:C]
    D = max(float(imgs.max()), max(border)) - min(float(imgs.min()), min(border))
    m = mapper()
    for name, (R, K) in VIEWS.items():
        want = cpu.remapped(name, dst, interpolation, dtype, C)
        m.set_view(R, K)
        fused, fvalid = run_remap(imgs, dst, interpolation, border, pad, inp.BATCH_CAMS)
        check_remap(fused, fvalid, want, dtype, (name, "fused"))
        maps64 = torch.empty((inp.N_CAMS, 2, dst[1], dst[0]), dtype=torch.float64, device=DEV)
        maps32 = torch.empty((inp.N_CAMS, 2, dst[1], dst[0]), dtype=torch.float32, device=DEV)
        for cam in range(inp.N_CAMS):
            m.build_maps(cam, dst[0], dst[1], maps64[cam].data_ptr(), out_f32=False, stream=torch.cuda.current_stream(0).cuda_stream)
            m.build_maps(cam, dst[0], dst[1], maps32[cam].data_ptr(), out_f32=True, stream=torch.cuda.current_stream(0).cuda_stream)
        mapped, mvalid = run_remap(imgs, dst, interpolation, border, pad, inp.BATCH_CAMS, maps64)
        check_remap(mapped, mvalid, want, dtype, (name, "mapped float64"))
        # fused against mapped: both within the bound of the restatement, so within twice the bound of each other
        assert np.array_equal(fvalid, mvalid)
        if dtype == "float32":
            assert np.max(np.abs(fused.astype(np.float64) - mapped)) <= 2 * MARGIN * G_VALUE * inp.image_range(dtype) + np.spacing(np.float32(D))
        else:
            assert np.max(np.abs(fused.astype(np.int64) - mapped)) <= 1
        # a float32 map: every coordinate moves by up to half a float32 ulp per axis
        mapped32, _ = run_remap(imgs, dst, interpolation, border, pad, inp.BATCH_CAMS, maps32)
        if interpolation == ref.NEAREST:
            # the chosen pixel can change only where a coordinate lies within a float32 ulp of a half-integer
            for i, cam in enumerate(inp.BATCH_CAMS):
                c64 = cpu.maps_of(name, cam, dst)
                with np.errstate(invalid="ignore"):
                    ulp = np.spacing(np.abs(c64).astype(np.float32)).astype(np.float64)
                    risky = np.any(np.abs(c64 - np.floor(c64) - 0.5) <= 2 * ulp, axis=0)
                same = mapped32[i] == mapped[i]
                assert np.all(same[~risky]), (name, "mapped float32", i)
        else:
            # a coordinate whose taps can reach the source is below max(W, H) + 3 in size; one further out gives the border either way,
            # and the interpolant is continuous where a tap enters or leaves (its weight is 0 there)
            ulp = float(np.spacing(np.float32(max(W, H) + 3)))
            extra = lipschitz(interpolation) * D * 2 * (0.5 * ulp)
            check_remap(mapped32, None, want, dtype, (name, "mapped float32"), extra=extra)


def test_a_batch_equals_single_image_calls_bit_for_bit():
    imgs = inp.images("uint8", 3)
    border = inp.BORDER["uint8"]
    m = mapper()
    m.set_view(*VIEWS["rot7"])
    dst = inp.DESTS[0]
    for interpolation in ref.INTERPOLATIONS:
        batch, bvalid = run_remap(imgs, dst, interpolation, border, 5, inp.BATCH_CAMS)
        for i, cam in enumerate(inp.BATCH_CAMS):
            one, ovalid = run_remap(imgs[i:i + 1], dst, interpolation, border, 0, [cam])
            assert np.array_equal(one[0], batch[i]) and np.array_equal(ovalid[0], bvalid[i]), (interpolation, i)


def test_smaller_shapes_after_larger_ones_on_one_handle():
    m = mapper()
    m.set_view(*VIEWS["shift_zoom"])
    imgs = inp.images("float32", 1)
    run_remap(imgs, inp.DESTS[0], ref.BICUBIC, inp.BORDER["float32"][:1], 5, inp.BATCH_CAMS)
    small, svalid = run_remap(imgs[:2], inp.DESTS[2], ref.BICUBIC, inp.BORDER["float32"][:1], 0, inp.BATCH_CAMS[:2])
    want = cpu.remapped("shift_zoom", inp.DESTS[2], ref.BICUBIC, "float32", 1)[:2]
    check_remap(small, svalid, want, "float32", "small after large")
    # other cameras for the same two images: the indices are uploaded again
    other, ovalid = run_remap(imgs[:2], inp.DESTS[2], ref.BICUBIC, inp.BORDER["float32"][:1], 0, [1, 0])
    want = [ref.remap(imgs[i], cpu.maps_of("shift_zoom", cam, inp.DESTS[2]), ref.BICUBIC, inp.BORDER["float32"][:1]) for i, cam in enumerate([1, 0])]
    check_remap(other, ovalid, want, "float32", "other cameras")


# ---- independent sampler check ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,interpolation", [(0, ref.BILINEAR), (1, ref.BICUBIC)])
def test_mapped_remap_agrees_with_grid_sample_on_the_same_device(k, interpolation):
    worst = 0.0
    for name in VIEWS:
        for C in inp.CHANNELS:
            imgs = inp.images("float32", C)
            dst = inp.DESTS[0]
            maps = np.stack([cpu.maps_of(name, cam, dst) for cam in range(inp.N_CAMS)]).astype(np.float32)
            d_maps = torch.from_numpy(maps).to(DEV)
            out = imaging.remap_images(torch.from_numpy(imgs).to(DEV), d_maps, inp.BATCH_CAMS, interpolation=interpolation)
            grid = torch.stack([2.0 * d_maps[:, 0] / (W - 1) - 1.0, 2.0 * d_maps[:, 1] / (H - 1) - 1.0], dim=-1)[inp.BATCH_CAMS]
            theirs = torch.nn.functional.grid_sample(torch.from_numpy(imgs).to(DEV).permute(0, 3, 1, 2), grid, mode=interpolation, padding_mode="zeros",
                                                     align_corners=True).permute(0, 2, 3, 1)
            ok = torch.isfinite(d_maps).all(dim=1)[inp.BATCH_CAMS]
            worst = max(worst, float((out - theirs).abs()[ok].max()) / inp.image_range("float32"))
    print(f"{interpolation}: device remap against grid_sample {worst:.2e} of the range (bound {8 * inp.GRID_SAMPLE_GAP[k]:.2e})")
    assert worst <= 8 * inp.GRID_SAMPLE_GAP[k]


# ---- front ends -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", inp.DTYPES)
def test_undistort_images_with_a_device_tensor_returns_one_equal_to_the_numpy_path(dtype):
    imgs = inp.images(dtype, 3)
    host, hvalid = imaging.undistort_images(imgs, inp.BATCH_CAMS, inp.INTR, interpolation="bicubic", border=inp.BORDER[dtype], return_valid=True)
    assert isinstance(host, np.ndarray) and host.shape == imgs.shape and host.dtype == imgs.dtype
    t = torch.from_numpy(imgs).to(DEV)
    dev, dvalid = imaging.undistort_images(t, inp.BATCH_CAMS, inp.INTR, interpolation="bicubic", border=inp.BORDER[dtype], return_valid=True)
    assert isinstance(dev, torch.Tensor) and dev.device == t.device and dev.dtype == t.dtype
    assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(dvalid.cpu().numpy(), hvalid)
    want = cpu.remapped("identity", inp.SENSOR, "bicubic", dtype, 3) if inp.SENSOR in inp.DESTS else [
        ref.remap(imgs[i], cpu.maps_of("identity", cam, inp.SENSOR), "bicubic", inp.BORDER[dtype]) for i, cam in enumerate(inp.BATCH_CAMS)]
    check_remap(host, hvalid, want, dtype, "undistort_images")
    # out=: a padded device tensor is written in place; the mapped method gives the same picture
    out, obuf = padded(len(inp.BATCH_CAMS), H, W, 3, dtype, 5)
    res = imaging.undistort_images(t, inp.BATCH_CAMS, inp.INTR, interpolation="bicubic", border=inp.BORDER[dtype], out=out)
    assert res is out and np.array_equal(out.cpu().numpy(), host) and bool(torch.all(obuf[:, :, W * 3:] == SENTINEL[dtype]))
    two_step = imaging.undistort_images(imgs, inp.BATCH_CAMS, inp.INTR, interpolation="bicubic", border=inp.BORDER[dtype], method="mapped")
    D = float(imgs.max()) - float(imgs.min())   # the border values lie inside
    lim = 1 if dtype == "uint8" else lipschitz("bicubic") * D * float(np.spacing(np.float32(W))) + float(np.spacing(np.float32(D)))
    assert np.max(np.abs(two_step.astype(np.float64) - host.astype(np.float64))) <= lim
    mono = imaging.undistort_images(imgs[:, :, :, 0].copy(), inp.BATCH_CAMS, inp.INTR)   # (n, H, W) comes back as (n, H, W)
    assert mono.shape == imgs.shape[:3]


def test_rectify_images_puts_corresponding_features_on_one_row():
    """Two synthetic views of a textured plane: bright blobs at known 3-D points.  Where each blob lands in the rectified images is
    computed from the geometry, not detected: both images must show it there, on the same row."""
    ka, ea, kb, eb = cpu.stereo_pair()
    Z0 = 2.0
    gx, gy = np.meshgrid([-0.4, -0.1, 0.2], [-0.25, 0.0, 0.25])
    jitter = np.random.default_rng(11).uniform(-0.02, 0.02, size=(9, 2))
    feats = np.concatenate([np.stack([gx.ravel(), gy.ravel()], axis=1) + jitter, np.full((9, 1), Z0)], axis=1)   # world points on the plane z = Z0
    sigma = 0.06   # about a pixel in either source: four to five sigma between neighbours

    def render(K, E):
        g = ref.pixel_grid(W, H)
        rays = ref.pixel_rays(g, K, E, world=True)
        pos = ref.camera_position(E)
        lam = (Z0 - pos[2]) / rays[:, 2]
        X = pos[None, :] + rays * lam[:, None]
        val = sum(np.exp(-((X[:, 0] - f[0]) ** 2 + (X[:, 1] - f[1]) ** 2) / (2 * sigma ** 2)) for f in feats)
        return val.reshape(1, H, W).astype(np.float32)

    ia, ib = render(ka, ea), render(kb, eb)
    ra, rb, Q = imaging.rectify_images(ia, ib, ka, ea, kb, eb, alpha=0.0)
    R_a, R_b, K_new, _ = imaging.rectify_images.last
    assert ra.shape == ia.shape and rb.shape == ib.shape and Q.shape == (4, 4)
    f, cx, _, cy = K_new
    seen = 0
    for X in feats:
        pa, pb = R_a @ (ea[:, :3] @ X + ea[:, 3]), R_b @ (eb[:, :3] @ X + eb[:, 3])
        ua, va, ub, vb = f * pa[0] / pa[2] + cx, f * pa[1] / pa[2] + cy, f * pb[0] / pb[2] + cx, f * pb[1] / pb[2] + cy
        assert abs(va - vb) <= 0.5
        for img, u, v in ((ra[0], ua, va), (rb[0], ub, vb)):
            if not (3 <= u <= W - 4 and 3 <= v <= H - 4):
                continue
            seen += 1
            y0, x0 = int(round(v)), int(round(u))
            patch = img[y0 - 3:y0 + 4, x0 - 3:x0 + 4]
            py, px = np.unravel_index(np.argmax(patch), patch.shape)
            assert patch.max() > 0.5 and abs(py - 3) <= 1 and abs(px - 3) <= 1, (u, v, py, px, float(patch.max()))
    assert seen >= 8


# ---- argument errors through the C ABI on a live handle --------------------------------------------------------------------------------------
def test_the_c_abi_names_the_offending_argument():
    lib = _capi.lib()
    m = mapper()
    cams = (ctypes.c_int32 * 2)(0, 1)
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())

    def remap(n=2, cams=cams, C=1, dtype=0, spitch=8, dpitch=8, interp=1, dmap=None, n_maps=0):
        return lib.pcs_imap_remap(m._h, n, cams, p, 8, 8, C, dtype, spitch, p, 8, 8, dpitch, dmap, 0, n_maps, interp, None, None, None)

    for call, word in ((lambda: remap(C=2), b"channels"), (lambda: remap(interp=7), b"interpolation"), (lambda: remap(spitch=7), b"src_pitch"),
                       (lambda: remap(dpitch=7), b"dst_pitch"), (lambda: remap(cams=(ctypes.c_int32 * 2)(0, 3)), b"cams"), (lambda: remap(dtype=5), b"dtype"),
                       (lambda: remap(dmap=p, n_maps=1), b"cams"), (lambda: lib.pcs_imap_build_maps(m._h, 9, 4, 4, p, 1, None), b"cam"),
                       (lambda: lib.pcs_imap_points(m._h, 5, 1, None, 0, p, 5, 0, p, None), b"mode"),
                       (lambda: lib.pcs_imap_points(m._h, 0, 1, None, 0, p, 500, 0, p, None), b"iters"),
                       (lambda: lib.pcs_imap_rays(m._h, 0, 0, 4, 0, 5, None, 0, p, 0, None), b"width")):
        assert call() == _capi.PCS_ERR_ARG and word in lib.pcs_last_error(), (word, lib.pcs_last_error())
    bad = np.array(inp.INTR)
    bad[1, 0] = 0.0
    with pytest.raises(ValueError, match="intr"):
        imaging.ImageMapper(0).set_cameras(bad)
    fresh = imaging.ImageMapper(0)
    assert lib.pcs_imap_set_view(fresh._h, None, None) == _capi.PCS_ERR_STATE
    ms = ctypes.c_float()
    assert lib.pcs_imap_last_kernel_ms(fresh._h, ctypes.byref(ms)) == _capi.PCS_ERR_STATE
    imaging.undistort_points(inp.points(), inp.INTR)
    assert imaging._mapper(0).last_kernel_ms() >= 0.0
