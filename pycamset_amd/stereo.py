"""Dense stereo on the device: block matching or semi-global matching on a rectified pair, disparity to points, the masked cloud
(include/pcs_hip.h pcs_stereo_*, csrc/ba_stereo.hpp, csrc/ba_stereo_sgm.hpp).

The second half of the reference's ``stereo_reconstruct`` (reconstruction/reconstruction_utils.py:170-223) — ``cv2.StereoBM_create(...)
.compute(r0, r1) / 16``, ``cv2.reprojectImageTo3D`` and the NaN / inf / depth mask of ``depth_image_ptcloud_mask`` (:24-38) /
``disparity_to_ptcld`` (:110-137) — behind ``imaging.rectify_images``.  OpenCV's matcher is not reproduced bit for bit: the rule is the
library's own, all integers, stated in include/pcs_hip.h.  ``method="sgm"`` is the other branch of that function, ``matlab_stereo``
(:140-167, MATLAB's ``disparitySGM``): a census cost aggregated along 4 or 8 paths, again by the library's own integer rule.

Conventions.  Images are 8-bit single channel, (H, W) or (n, H, W).  Disparities are int16 sixteenths of a pixel, d = u_left - u_right,
with 16 (min_disp - 1) where no disparity was accepted (cv2's convention).  NumPy arrays are copied to the device and results come back
as NumPy arrays; torch tensors on the device are used in place (a padded row pitch included) and the results are torch tensors.  There
is no CPU fallback; the argument checks raise ValueError before anything touches the device."""
from __future__ import annotations

import numpy as np

from ._capi import STEREO_LEFT_RIGHT, STEREO_NOT_STRICT, STEREO_TEXTURE, STEREO_UNIQUENESS, STEREO_VALIDITY  # noqa: F401  (re-exported)
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg
from .imaging import _device_of, _is_tensor, _pitched, _result, _stream, _to_device, _torch, check_ext, rectify_images

MAX_DISP, MAX_BLOCK, MAX_CAP, MAX_PAIRS = 1024, 31, 63, 32767
SGM_MAX_DISP, SGM_MAX_BITS, SGM_MAX_P = 256, 64, 1023
NO_INVALID = -(1 << 31)   # pcs_stereo_reproject: every disparity counts
FLOAT_INVALID = -32768    # what a NaN of a float disparity becomes


def check_match_args(n, width, height, left_pitch, right_pitch, num_disp, block, min_disp, prefilter_cap, texture_threshold, uniqueness_ratio, lr_max_diff):
    """The checks of pcs_stereo_match on the host; the ValueError names the argument.  Pitches are in bytes."""
    def integer(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: expected an integer, got {v!r}")
        return int(v)

    num_disp, block, min_disp = integer(num_disp, "num_disp"), integer(block, "block"), integer(min_disp, "min_disp")
    cap, tex = integer(prefilter_cap, "prefilter_cap"), integer(texture_threshold, "texture_threshold")
    uniq, lr = integer(uniqueness_ratio, "uniqueness_ratio"), integer(lr_max_diff, "lr_max_diff")
    if not 0 <= n <= MAX_PAIRS:
        raise ValueError(f"images: at most {MAX_PAIRS} pairs per call, got {n}")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"images: width and height must be in [1, 65535], got {width} x {height}")
    if not -MAX_DISP <= min_disp <= MAX_DISP:
        raise ValueError(f"min_disp: expected an integer in [-{MAX_DISP}, {MAX_DISP}], got {min_disp}")
    if not 1 <= num_disp <= MAX_DISP:
        raise ValueError(f"num_disp: expected an integer in [1, {MAX_DISP}], got {num_disp}")
    if not 3 <= block <= MAX_BLOCK or block % 2 == 0:
        raise ValueError(f"block: expected an odd integer in [3, {MAX_BLOCK}], got {block}")
    if not 0 <= cap <= MAX_CAP:
        raise ValueError(f"prefilter_cap: expected an integer in [0, {MAX_CAP}], got {cap}")
    if tex < 0 or (cap == 0 and tex != 0):
        raise ValueError(f"texture_threshold: expected >= 0, and 0 with prefilter_cap = 0, got {tex}")
    if not 0 <= uniq <= 100:
        raise ValueError(f"uniqueness_ratio: expected an integer in [0, 100], got {uniq}")
    if lr < -1:
        raise ValueError(f"lr_max_diff: expected >= -1, got {lr}")
    if left_pitch < width or right_pitch < width:
        raise ValueError(f"pitch: {min(left_pitch, right_pitch)} bytes is below the row size {width}")
    return num_disp, block, min_disp, cap, tex, uniq, lr


def check_sgm_args(n, width, height, left_pitch, right_pitch, num_disp, census, min_disp, p1, p2, paths, uniqueness_ratio, lr_max_diff):
    """The checks of pcs_stereo_sgm on the host; the ValueError names the argument.  ``census`` = (width, height) of the window."""
    def integer(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: expected an integer, got {v!r}")
        return int(v)

    try:
        cw, ch = census
    except (TypeError, ValueError):
        raise ValueError(f"census: expected (width, height), got {census!r}") from None
    cw, ch, num_disp, min_disp = integer(cw, "census"), integer(ch, "census"), integer(num_disp, "num_disp"), integer(min_disp, "min_disp")
    p1, p2, paths = integer(p1, "p1"), integer(p2, "p2"), integer(paths, "paths")
    uniq, lr = integer(uniqueness_ratio, "uniqueness_ratio"), integer(lr_max_diff, "lr_max_diff")
    if not 0 <= n <= MAX_PAIRS:
        raise ValueError(f"images: at most {MAX_PAIRS} pairs per call, got {n}")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"images: width and height must be in [1, 65535], got {width} x {height}")
    if not -MAX_DISP <= min_disp <= MAX_DISP:
        raise ValueError(f"min_disp: expected an integer in [-{MAX_DISP}, {MAX_DISP}], got {min_disp}")
    if not 1 <= num_disp <= SGM_MAX_DISP:
        raise ValueError(f"num_disp: expected an integer in [1, {SGM_MAX_DISP}], got {num_disp}")
    if cw < 3 or ch < 3 or cw % 2 == 0 or ch % 2 == 0 or cw * ch - 1 > SGM_MAX_BITS:
        raise ValueError(f"census: expected odd sides >= 3 with width * height - 1 <= {SGM_MAX_BITS}, got {cw} x {ch}")
    if not 0 <= p1 <= p2:
        raise ValueError(f"p1: expected 0 <= p1 <= p2, got p1 = {p1}, p2 = {p2}")
    if p2 > SGM_MAX_P:
        raise ValueError(f"p2: expected at most {SGM_MAX_P}, got {p2}")
    if paths not in (4, 8):
        raise ValueError(f"paths: expected 4 or 8, got {paths}")
    if not 0 <= uniq <= 100:
        raise ValueError(f"uniqueness_ratio: expected an integer in [0, 100], got {uniq}")
    if lr < -1:
        raise ValueError(f"lr_max_diff: expected >= -1, got {lr}")
    if left_pitch < width or right_pitch < width:
        raise ValueError(f"pitch: {min(left_pitch, right_pitch)} bytes is below the row size {width}")
    return num_disp, cw, ch, min_disp, p1, p2, paths, uniq, lr


def sgm_pair_bytes(width, height, num_disp):
    """Bytes of workspace one pair takes in ``match_sgm`` (csrc/ba_stereo_sgm.hpp sgm_pair_bytes): the aggregated volume, uint16 with the
    disparities rounded up to a multiple of 4, and the two 64-bit census planes."""
    return 2 * height * width * ((int(num_disp) + 3) & ~3) + 16 * height * width


class StereoMatcher(_Handle):
    """Owner of one ``pcs_stereo_matcher`` handle (include/pcs_hip.h): the workspace (two prefiltered planes, the right-anchored disparity,
    the compaction's counts) stays on the device across calls; images, disparities and points are raw device addresses used in place."""

    _create, _destroy = "pcs_stereo_create", "pcs_stereo_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)

    def match(self, n, width, height, d_left, left_pitch, d_right, right_pitch, d_disp, *, num_disp, block, min_disp=0, prefilter_cap=31, texture_threshold=10,
              uniqueness_ratio=15, lr_max_diff=-1, d_valid_left=None, d_valid_right=None, d_cost=None, d_status=None, stream=None):
        a = check_match_args(n, width, height, left_pitch, right_pitch, num_disp, block, min_disp, prefilter_cap, texture_threshold, uniqueness_ratio, lr_max_diff)
        num_disp, block, min_disp, cap, tex, uniq, lr = a
        self._call("pcs_stereo_match", self._h, int(n), int(width), int(height), self._addr(d_left), int(left_pitch), self._addr(d_right), int(right_pitch), min_disp,
                   num_disp, block, cap, tex, uniq, lr, self._addr(d_valid_left), self._addr(d_valid_right), self._addr(d_disp), self._addr(d_cost), self._addr(d_status),
                   _stream_arg(stream))

    def match_sgm(self, n, width, height, d_left, left_pitch, d_right, right_pitch, d_disp, *, num_disp, census=(9, 7), min_disp=0, p1=8, p2=32, paths=8,
                  uniqueness_ratio=15, lr_max_diff=-1, d_valid_left=None, d_valid_right=None, d_cost=None, d_status=None, stream=None):
        a = check_sgm_args(n, width, height, left_pitch, right_pitch, num_disp, census, min_disp, p1, p2, paths, uniqueness_ratio, lr_max_diff)
        num_disp, cw, ch, min_disp, p1, p2, paths, uniq, lr = a
        self._call("pcs_stereo_sgm", self._h, int(n), int(width), int(height), self._addr(d_left), int(left_pitch), self._addr(d_right), int(right_pitch), min_disp,
                   num_disp, cw, ch, p1, p2, paths, uniq, lr, self._addr(d_valid_left), self._addr(d_valid_right), self._addr(d_disp), self._addr(d_cost),
                   self._addr(d_status), _stream_arg(stream))

    def set_sgm_workspace(self, nbytes: int = 0):
        """The bytes ``match_sgm`` may hold for the aggregated volume and the census planes (0: the library's default, 16 GiB); a batch is
        walked in chunks of pairs that fit.  A limit below ``sgm_pair_bytes`` of a call makes that call raise."""
        self._call("pcs_stereo_set_sgm_workspace", self._h, int(nbytes))

    def reproject(self, n, width, height, d_disp, Q, d_points, d_mask, *, invalid=NO_INVALID, z_range=(-np.inf, np.inf), T=None, f32=True, d_counts=None, stream=None):
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 16)
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(12)
        self._call("pcs_stereo_reproject", self._h, int(n), int(width), int(height), self._addr(d_disp), int(invalid), self._ptr(Q), Q.shape[0], float(z_range[0]),
                   float(z_range[1]), self._ptr(T), self._addr(d_points), int(f32), self._addr(d_mask), self._addr(d_counts), _stream_arg(stream))

    def compact(self, n, width, height, d_points, f32, d_mask, d_out_points, d_counts, *, d_values=None, values_pitch=0, d_out_values=None, stream=None):
        self._call("pcs_stereo_compact", self._h, int(n), int(width), int(height), self._addr(d_points), int(f32), self._addr(d_mask), self._addr(d_values),
                   int(values_pitch), self._addr(d_out_points), self._addr(d_out_values), self._addr(d_counts), _stream_arg(stream))

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_stereo_last_kernel_ms")


_matcher_cache: dict = {}


def _matcher(device: int) -> StereoMatcher:
    return _cached_handle(_matcher_cache, int(device), lambda: StereoMatcher(device))


def _plane_stack(a, name):
    """-> ((n, H, W) view, single)"""
    if a.ndim == 2:
        return a[None], True
    if a.ndim == 3:
        return a, False
    raise ValueError(f"{name}: expected (H, W) or (n, H, W), got shape {tuple(a.shape)}")


def _u8_on_device(a, name, dev):
    """An 8-bit (n, H, W) stack as a device tensor usable in place -> (tensor, row pitch in bytes)."""
    torch = _torch()
    dt = str(a.dtype).replace("torch.", "")
    if dt != "uint8":
        raise ValueError(f"{name}: expected uint8, got {dt}")
    if _is_tensor(a) and a.is_cuda and _pitched(a[..., None]) is not None:
        return a, _pitched(a[..., None])
    t = _to_device(a, torch.uint8, dev)
    return t, int(t.shape[2])


def stereo_match(left, right, num_disp, block=None, min_disp=0, prefilter_cap=None, texture_threshold=None, uniqueness_ratio=15, lr_max_diff=-1, valid=None,
                 return_cost=False, return_status=False, as_float=False, device=None, method="block", census=(9, 7), p1=8, p2=32, paths=8):
    """Block matching on rectified pairs: ``cv2.StereoBM_create(numDisparities=num_disp, blockSize=block).compute(left, right)`` by the
    rule of include/pcs_hip.h.  ``left`` / ``right``: (H, W) or (n, H, W) uint8.  The disparities searched are ``min_disp .. min_disp +
    num_disp - 1`` (negative allowed).  ``lr_max_diff`` >= 0 adds the left-right check; ``valid`` = (valid_left, valid_right) are the
    planes of ``rectify_images(return_valid=True)``.  -> int16 sixteenths (16 (min_disp - 1) where nothing was accepted), or with
    ``as_float`` float32 pixels with NaN there; then the int32 winning cost (``return_cost``; -1 outside the strict band) and the uint8
    status bits STEREO_* (``return_status``).

    ``method="sgm"``: semi-global matching instead (the reference's ``matlab_stereo``): the Hamming distance of ``census`` = (width, height)
    descriptors, aggregated along ``paths`` = 4 or 8 directions with the penalties ``p1`` <= ``p2``; num_disp <= 256.  It has no block, no
    prefilter and no texture measure: ``block``, ``prefilter_cap`` or ``texture_threshold`` given with it raise.  The defaults
    (``method="block"``, prefilter_cap 31, texture_threshold 10) are the block matcher as before."""
    if method not in ("block", "sgm"):
        raise ValueError(f"method: expected 'block' or 'sgm', got {method!r}")
    sgm = method == "sgm"
    if sgm:
        for v, name in ((block, "block"), (prefilter_cap, "prefilter_cap"), (texture_threshold, "texture_threshold")):
            if v is not None:
                raise ValueError(f"{name}: the block matcher's; method='sgm' takes census, p1, p2 and paths")
    else:
        if block is None:
            raise ValueError("block: method='block' needs the block size")
        prefilter_cap = 31 if prefilter_cap is None else prefilter_cap
        texture_threshold = 10 if texture_threshold is None else texture_threshold
    torch = _torch()
    L, single = _plane_stack(left, "left")
    R, _ = _plane_stack(right, "right")
    if tuple(L.shape) != tuple(R.shape):
        raise ValueError(f"right: expected the shape of left, {tuple(left.shape)}, got {tuple(right.shape)}")
    n, H, W = (int(v) for v in L.shape)
    if sgm:
        check_sgm_args(n, W, H, W, W, num_disp, census, min_disp, p1, p2, paths, uniqueness_ratio, lr_max_diff)
    else:
        check_match_args(n, W, H, W, W, num_disp, block, min_disp, prefilter_cap, texture_threshold, uniqueness_ratio, lr_max_diff)
    for a, name in ((L, "left"), (R, "right")):
        if str(a.dtype).replace("torch.", "") != "uint8":
            raise ValueError(f"{name}: expected uint8, got {a.dtype}")
    vs = [None, None]
    if valid is not None:
        if len(valid) != 2:
            raise ValueError("valid: expected (valid_left, valid_right)")
        for k, v in enumerate(valid):
            vs[k], _ = _plane_stack(v, "valid")
            if tuple(vs[k].shape) != (n, H, W):
                raise ValueError(f"valid: expected planes of shape {(n, H, W)}, got {tuple(v.shape)}")
    as_tensor = _is_tensor(left) and left.is_cuda
    dev = _device_of(left, right, device=device)
    m = _matcher(dev)
    dL, pL = _u8_on_device(L, "left", dev)
    dR, pR = _u8_on_device(R, "right", dev)
    dv = [None if v is None else _to_device(v, torch.uint8, dev) for v in vs]
    disp = torch.empty((n, H, W), dtype=torch.int16, device=dL.device)
    cost = torch.empty((n, H, W), dtype=torch.int32, device=dL.device) if return_cost else None
    status = torch.empty((n, H, W), dtype=torch.uint8, device=dL.device) if return_status else None
    common = dict(num_disp=num_disp, min_disp=min_disp, uniqueness_ratio=uniqueness_ratio, lr_max_diff=lr_max_diff, d_valid_left=None if dv[0] is None else dv[0].data_ptr(),
                  d_valid_right=None if dv[1] is None else dv[1].data_ptr(), d_cost=None if cost is None else cost.data_ptr(),
                  d_status=None if status is None else status.data_ptr(), stream=_stream(dev))
    if sgm:
        m.match_sgm(n, W, H, dL.data_ptr(), pL, dR.data_ptr(), pR, disp.data_ptr(), census=census, p1=p1, p2=p2, paths=paths, **common)
    else:
        m.match(n, W, H, dL.data_ptr(), pL, dR.data_ptr(), pR, disp.data_ptr(), block=block, prefilter_cap=prefilter_cap, texture_threshold=texture_threshold, **common)
    if as_float:
        f = disp.to(torch.float32) / 16.0
        disp = torch.where(disp == 16 * (int(min_disp) - 1), torch.full_like(f, float("nan")), f)
    outs = [_result(o[0] if single else o, as_tensor) for o in (disp, cost, status) if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def disparity_to_points(disp, Q, depth_range=None, transform=None, values=None, compact=False, dtype=np.float32, invalid=None, device=None):
    """``cv2.reprojectImageTo3D`` and the reference's mask: (X, Y, Z, Wh) = Q (x, y, disp / 16, 1) in FP64, point = (X, Y, Z) / Wh.
    ``disp``: (H, W) or (n, H, W), int16 sixteenths (``invalid``: the value that marks a rejected pixel, 16 (min_disp - 1) of the match;
    None: every value counts) or float32 / float64 pixels with NaN where rejected.  ``Q`` (4, 4) or (n, 4, 4).  ``depth_range`` (lo, hi):
    the mask keeps lo <= z <= hi, z in the rectified frame.  ``transform`` (3, 4): rectified frame -> the caller's, applied to the
    points.  -> (points (..., 3) of ``dtype`` with NaN where the mask is 0, mask uint8).  With ``compact``: a list with one entry per
    pair, the masked points (M_i, 3) in row-major pixel order, or (points, values (M_i,)) with ``values`` (the left image, uint8)."""
    torch = _torch()
    D, single = _plane_stack(disp, "disp")
    n, H, W = (int(v) for v in D.shape)
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    Qa = np.asarray(Q, dtype=np.float64)
    if Qa.shape not in ((4, 4), (n, 4, 4)) or not np.all(np.isfinite(Qa)):
        raise ValueError(f"Q: expected finite (4, 4) or ({n}, 4, 4), got shape {np.shape(Q)}")
    T = None
    if transform is not None:
        T = np.asarray(transform, dtype=np.float64)
        if T.shape == (4, 4):
            T = T[:3]
        if T.shape != (3, 4) or not np.all(np.isfinite(T)):
            raise ValueError(f"transform: expected a finite (3, 4) or (4, 4), got shape {np.shape(transform)}")
    lo, hi = (-np.inf, np.inf) if depth_range is None else (float(depth_range[0]), float(depth_range[1]))
    if lo != lo or hi != hi:
        raise ValueError("depth_range: NaN is no bound (use -inf / +inf)")
    if not 0 <= n <= MAX_PAIRS:
        raise ValueError(f"disp: at most {MAX_PAIRS} pairs per call, got {n}")
    as_tensor = _is_tensor(disp) and disp.is_cuda
    dev = _device_of(disp, values, device=device)
    name = str(D.dtype).replace("torch.", "")
    if name == "int16":
        d16 = _to_device(D, torch.int16, dev)
        inv = NO_INVALID if invalid is None else int(invalid)
    elif name in ("float32", "float64"):
        f = _to_device(D, getattr(torch, name), dev)
        d16 = torch.where(torch.isnan(f), torch.full_like(f, float(FLOAT_INVALID)), torch.round(f * 16.0)).to(torch.int16)
        inv = FLOAT_INVALID
    else:
        raise ValueError(f"disp: expected int16 sixteenths or float pixels, got {name}")
    dv = None
    if values is not None:
        V, _ = _plane_stack(values, "values")
        if tuple(V.shape) != (n, H, W):
            raise ValueError(f"values: expected the shape of disp, {(n, H, W)}, got {tuple(values.shape)}")
        dv, pv = _u8_on_device(V, "values", dev)
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    m = _matcher(dev)
    pts = torch.empty((n, H, W, 3), dtype=torch.float32 if f32 else torch.float64, device=d16.device)
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=d16.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=d16.device)
    m.reproject(n, W, H, d16.data_ptr(), Qa, pts.data_ptr(), mask.data_ptr(), invalid=inv, z_range=(lo, hi), T=T, f32=f32, d_counts=counts.data_ptr(), stream=_stream(dev))
    if not compact:
        return _result(pts[0] if single else pts, as_tensor), _result(mask[0] if single else mask, as_tensor)
    out_pts = torch.empty((n * H * W, 3), dtype=pts.dtype, device=pts.device)
    out_val = torch.empty((n * H * W,), dtype=torch.uint8, device=pts.device) if dv is not None else None
    m.compact(n, W, H, pts.data_ptr(), f32, mask.data_ptr(), out_pts.data_ptr(), counts.data_ptr(), d_values=None if dv is None else dv.data_ptr(),
              values_pitch=0 if dv is None else pv, d_out_values=None if out_val is None else out_val.data_ptr(), stream=_stream(dev))
    ends = np.cumsum(counts.cpu().numpy())
    clouds = []
    for i in range(n):
        a, b = int(ends[i - 1]) if i else 0, int(ends[i])
        p = _result(out_pts[a:b], as_tensor)
        clouds.append(p if out_val is None else (p, _result(out_val[a:b], as_tensor)))
    return clouds


def stereo_reconstruct(images_a, images_b, intr_a, ext_a, intr_b, ext_b, num_disp=256, block=None, depth_range=(0.0, 2.0), frame="rectified", alpha: float = 1.0,
                       interpolation: str = "bicubic", dtype=np.float32, compact=True, device=None, method="block", **match_options):
    """The reference's ``stereo_reconstruct`` (reconstruction/reconstruction_utils.py:170-223) on the device: ``imaging.rectify_images
    (return_valid=True)`` -> ``stereo_match`` -> ``disparity_to_points`` with the left (camera a's) rectified grey value per point.
    ``frame``: 'rectified' (camera a's rectified frame, as the reference returns) or 'world' ((R_a E_a)^-1 applied).  ``Q`` fixes the sign
    of d = u_a - u_b: when camera a is the right-hand one the searched range is mirrored to [-(min_disp + num_disp - 1), -min_disp], so
    that a pair works in either order.  ``method``: 'block' (``block`` defaults to the reference's 25) or 'sgm' (the reference's
    ``matlab=True``; ``census``, ``p1``, ``p2``, ``paths`` among the options).  -> ``compact``: a list of (points (M_i, 3), grey (M_i,)) per
    pair; else (points, mask).
    ``stereo_reconstruct.last`` holds (rectified a, rectified b, Q, disparity, min_disp used)."""
    if frame not in ("rectified", "world"):
        raise ValueError(f"frame: expected 'rectified' or 'world', got {frame!r}")
    min_disp = int(match_options.pop("min_disp", 0))
    dev = _device_of(images_a, images_b, device=device)
    ra, rb, Q, va, vb = rectify_images(images_a, images_b, intr_a, ext_a, intr_b, ext_b, alpha, interpolation=interpolation, return_valid=True, device=dev)
    R_a = rectify_images.last[0]
    # Z = f / (d Q[3, 2]) must be positive in front of the cameras: Q[3, 2] = -1 / tx, tx < 0 when camera a is the left-hand one
    if Q[3, 2] < 0:
        min_disp = -(min_disp + int(num_disp) - 1)
    if method == "block" and block is None:
        block = 25
    disp = stereo_match(ra, rb, num_disp, block, min_disp=min_disp, valid=(va, vb), device=dev, method=method, **match_options)
    T = None
    if frame == "world":
        E = check_ext(ext_a, 1)[0].reshape(3, 4)
        M = R_a @ E[:, :3]   # world -> rectified: X_r = M X_w + R_a t
        T = np.concatenate([M.T, -(M.T @ (R_a @ E[:, 3]))[:, None]], axis=1)
    stereo_reconstruct.last = (ra, rb, Q, disp, min_disp)
    return disparity_to_points(disp, Q, depth_range=depth_range, transform=T, values=ra, compact=compact, dtype=dtype, invalid=16 * (min_disp - 1), device=dev)
