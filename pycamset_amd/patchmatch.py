"""PatchMatch multi-view depth on the device: a slanted plane per pixel of every view, spread between neighbouring pixels and refined by
random perturbation (include/pcs_hip.h pcs_pm_*, csrc/ba_patchmatch.hpp).

The plane sweep (``sweep.py``) tests fronto-parallel planes from a table.  The program the reference writes its rig out for (ACMMP:
reconstruction/acmmp_utils.py, ``ReconParams``, ``Camera.to_MVSnet_txt``) is a PatchMatch method: every pixel carries a plane (depth and
normal), which is what gives unbiased depth on surfaces seen obliquely, depth finer than a plane table and a normal per pixel.
``refine_depth_maps`` takes the sweep's depth maps as a start, or starts from nothing, and returns depth maps that
``fusion.fuse_depth_maps`` and ``volume.integrate_depth_maps`` take unchanged.  The rule is the library's own (stated in full in
include/pcs_hip.h, restated in NumPy in tests/patchmatch_reference.py); ACMMP is not reproduced.

Conventions follow ``sweep.py``: distortion-free pinholes ``K = [fx, cx, fy, cy]`` with ``[R | t]`` world -> view; NumPy arrays are
copied to the device and results come back as NumPy arrays; torch tensors on the device are used in place and the results are torch
tensors.  There is no CPU fallback; the argument checks raise ValueError before anything touches the device."""
from __future__ import annotations

import numpy as np

from ._capi import PM_MAX_NEIGHBOURS, PM_NO_VIEW, PM_NOT_STRICT  # noqa: F401  (re-exported)
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg
from .imaging import _device_of, _is_tensor, _result, _stream, _to_device, _torch
from .stereo import _u8_on_device
from .sweep import check_sweep_args

MAX_STRIDE = 4
MAX_ITERATION = 1000


def check_patchmatch_args(n_views, width, height, pitch, K, ext, neighbours, depth_range, census=(7, 7), stride=2, truncate=None, max_slant=70.0, seed=0, iterations=3,
                          first_iteration=0, dtype=np.float32):
    """The checks of pcs_pm_set_views, pcs_pm_set_neighbours, pcs_pm_init and pcs_pm_iterate on the host; the ValueError names the
    argument.  ``depth_range`` = (z_min, z_max) or one such row per view; ``truncate`` defaults to (cw ch - 1) // 4.
    -> (K (V, 4), P (V, 12), nbr_start int32, nbr int32, wrange (n, 2) float64 = [1 / z_max, 1 / z_min], slope_max (V,) float64 =
    tan(max_slant) / min(|fx|, |fy|), cw, ch, stride, truncate, seed, iterations, first_iteration, f32)."""
    def integer(v, name, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name}: expected an integer in [{lo}, {hi}], got {v!r}")
        return int(v)

    Ka, P, start, nbr, _, cw, ch, _, truncate, _, f32 = check_sweep_args(n_views, width, height, pitch, K, ext, neighbours, [1.0], census, 0, truncate, 0, dtype)
    try:
        zr = np.asarray(depth_range, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"depth_range: expected (z_min, z_max) or one such row per view, got {depth_range!r}") from None
    if zr.ndim == 1:
        zr = zr[None]
    if zr.ndim != 2 or zr.shape[1:] != (2,) or zr.shape[0] not in (1, n_views):
        raise ValueError(f"depth_range: expected (z_min, z_max) or ({n_views}, 2), got shape {np.shape(depth_range)}")
    if not np.all(np.isfinite(zr)) or np.any(zr[:, 0] <= 0) or np.any(zr[:, 0] >= zr[:, 1]):
        raise ValueError(f"depth_range: expected finite 0 < z_min < z_max, got {depth_range!r}")
    wrange = np.ascontiguousarray(np.stack([1.0 / zr[:, 1], 1.0 / zr[:, 0]], axis=1))
    stride = integer(stride, "stride", 1, MAX_STRIDE)
    if isinstance(max_slant, bool) or not isinstance(max_slant, (int, float, np.integer, np.floating)) or not 0.0 < float(max_slant) < 90.0:
        raise ValueError(f"max_slant: expected degrees in (0, 90), got {max_slant!r}")
    slope = np.tan(np.radians(float(max_slant))) / np.minimum(np.abs(Ka[:, 0]), np.abs(Ka[:, 2]))
    seed = integer(seed, "seed", 0, 2 ** 64 - 1)
    first_iteration = integer(first_iteration, "first_iteration", 0, MAX_ITERATION)
    iterations = integer(iterations, "iterations", 0, MAX_ITERATION - first_iteration)
    return Ka, P, start, nbr, wrange, np.ascontiguousarray(slope), cw, ch, stride, truncate, seed, iterations, first_iteration, f32


class PatchMatcher(_Handle):
    """Owner of one ``pcs_patchmatch`` handle (include/pcs_hip.h): the neighbour lists, the warp table and the per-view bounds stay on
    the device across calls; images, planes, costs and outputs are raw device addresses used in place."""

    _create, _destroy = "pcs_pm_create", "pcs_pm_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)

    def set_views(self, width, height, K, P):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_pm_set_views", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P))

    def set_neighbours(self, nbr_start, nbr):
        nbr_start, nbr = np.ascontiguousarray(nbr_start, dtype=np.int32), np.ascontiguousarray(nbr, dtype=np.int32)
        self._call("pcs_pm_set_neighbours", self._h, self._ptr(nbr_start), self._ptr(nbr) if nbr.size else None, len(nbr_start) - 1)

    def _search(self, wrange, slope_max, census, stride, truncate, seed):
        wrange = np.ascontiguousarray(wrange, dtype=np.float64).reshape(-1, 2)
        slope_max = np.ascontiguousarray(slope_max, dtype=np.float64)
        truncate = (int(census[0]) * int(census[1]) - 1) // 4 if truncate is None else truncate
        return (wrange, slope_max), (self._ptr(wrange), wrange.shape[0], self._ptr(slope_max), int(census[0]), int(census[1]), int(stride), int(truncate),
                                     self._ct.c_uint64(int(seed)))

    def init(self, d_images, pitch, wrange, slope_max, d_plane, d_cost, *, census=(7, 7), stride=2, truncate=None, seed=0, d_start_depth=None, start_f32=True,
             start_planes=False, stream=None):
        keep, args = self._search(wrange, slope_max, census, stride, truncate, seed)
        self._call("pcs_pm_init", self._h, self._addr(d_images), int(pitch), *args, self._addr(d_start_depth), int(bool(start_f32)), int(bool(start_planes)),
                   self._addr(d_plane), self._addr(d_cost), _stream_arg(stream))

    def iterate(self, first_iteration, n_iterations, d_images, pitch, wrange, slope_max, d_plane, d_cost, *, census=(7, 7), stride=2, truncate=None, seed=0, stream=None):
        keep, args = self._search(wrange, slope_max, census, stride, truncate, seed)
        self._call("pcs_pm_iterate", self._h, int(first_iteration), int(n_iterations), self._addr(d_images), int(pitch), *args, self._addr(d_plane), self._addr(d_cost),
                   _stream_arg(stream))

    def finish(self, d_plane, d_cost, d_depth, *, census=(7, 7), stride=2, truncate=None, f32=True, d_normal=None, d_status=None, stream=None):
        truncate = (int(census[0]) * int(census[1]) - 1) // 4 if truncate is None else truncate
        self._call("pcs_pm_finish", self._h, int(census[0]), int(census[1]), int(stride), int(truncate), self._addr(d_plane), self._addr(d_cost), self._addr(d_depth),
                   int(bool(f32)), self._addr(d_normal), self._addr(d_status), _stream_arg(stream))

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_pm_last_kernel_ms")


_matcher_cache: dict = {}


def _matcher(device: int) -> PatchMatcher:
    return _cached_handle(_matcher_cache, int(device), lambda: PatchMatcher(device))


def refine_depth_maps(images, K, ext, neighbours, depth_range, depth=None, *, planes=None, iterations=3, first_iteration=0, census=(7, 7), stride=2, truncate=None,
                      max_slant=70.0, seed=0, dtype=np.float32, return_normal=False, return_plane=False, return_cost=False, return_status=False, device=None):
    """One z-depth map per view by PatchMatch over its neighbours (the rule of include/pcs_hip.h).  ``images`` (V, H, W) uint8, the
    undistorted images; ``K`` (V, 4) = [fx, cx, fy, cy]; ``ext`` (V, 3, 4) world -> view; ``neighbours`` as for ``sweep_depth_maps``;
    ``depth_range`` = (z_min, z_max), or one row per view: the bounds of the search.  ``depth`` (V, H, W) float32 or float64: a start,
    e.g. the sweep's maps — an invalid entry (NaN, <= 0) starts at random; ``planes`` (V, H, W, 3) float64: the state a former call
    returned (``return_plane``), to continue it with ``first_iteration`` = the iterations done; neither: every pixel starts at random.
    Every pixel holds a plane (w, a, b): inverse depth at the pixel and its change per pixel in x and y.  Its cost is the Hamming
    distance of ``census`` = (width, height) descriptors, taken at every ``stride``-th pixel, of the reference image and of each
    neighbour warped through the plane, truncated at ``truncate`` per neighbour (default: a quarter of the full scale) and added over
    the neighbours.  An iteration offers each pixel the planes of 8 pixels around it and 4 random changes of its own, smaller with
    every iteration; a plane steeper than ``max_slant`` degrees against the viewing direction is never taken.  ``seed`` fixes the
    random numbers: equal arguments give equal bits.
    -> depth (V, H, W) of ``dtype``, NaN where nothing was accepted[, normal (V, H, W, 3) of ``dtype``, unit, in the view's frame,
    facing the camera (``return_normal``)][, plane (V, H, W, 3) float64 (``return_plane``)][, cost int32, -1 outside the strict
    rectangle (``return_cost``)][, status uint8, PM_NOT_STRICT or PM_NO_VIEW (``return_status``)]; a tuple when any of them is asked for."""
    torch = _torch()
    if getattr(images, "ndim", None) != 3:
        raise ValueError(f"images: expected (V, H, W) uint8, got shape {tuple(getattr(images, 'shape', ()))}")
    V, H, W = (int(v) for v in images.shape)
    as_tensor = _is_tensor(images) and images.is_cuda
    if str(images.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"images: expected uint8, got {images.dtype}")
    Ka, P, start, nbr, wrange, slope, cw, ch, stride, truncate, seed, iterations, first_iteration, f32 = check_patchmatch_args(
        V, W, H, W, K, ext, neighbours, depth_range, census, stride, truncate, max_slant, seed, iterations, first_iteration, dtype)
    if depth is not None and planes is not None:
        raise ValueError("planes: a start depth and start planes exclude each other")
    start_f32 = True
    if depth is not None:
        dt = str(getattr(depth, "dtype", "")).replace("torch.", "")
        if tuple(getattr(depth, "shape", ())) != (V, H, W) or dt not in ("float32", "float64"):
            raise ValueError(f"depth: expected ({V}, {H}, {W}) float32 or float64, got shape {tuple(getattr(depth, 'shape', ()))} of {dt or type(depth).__name__}")
        start_f32 = dt == "float32"
    if planes is not None:
        dt = str(getattr(planes, "dtype", "")).replace("torch.", "")
        if tuple(getattr(planes, "shape", ())) != (V, H, W, 3) or dt != "float64":
            raise ValueError(f"planes: expected ({V}, {H}, {W}, 3) float64, got shape {tuple(getattr(planes, 'shape', ()))} of {dt or type(planes).__name__}")
    dev = _device_of(images, depth, planes, device=device)
    I, pitch = _u8_on_device(images, "images", dev)
    pm = _matcher(dev)
    pm.set_views(W, H, Ka, P)
    pm.set_neighbours(start, nbr)
    d0 = None if depth is None else _to_device(depth, torch.float32 if start_f32 else torch.float64, dev)
    # the state is the caller's to keep: a given plane map is copied, never changed
    plane = torch.empty((V, H, W, 3), dtype=torch.float64, device=I.device) if planes is None else _to_device(planes, torch.float64, dev).clone()
    cost = torch.empty((V, H, W), dtype=torch.int32, device=I.device)
    out = torch.empty((V, H, W), dtype=torch.float32 if f32 else torch.float64, device=I.device)
    normal = torch.empty((V, H, W, 3), dtype=out.dtype, device=I.device) if return_normal else None
    status = torch.empty((V, H, W), dtype=torch.uint8, device=I.device) if return_status else None
    ptr = lambda t: None if t is None else t.data_ptr()
    kw = dict(census=(cw, ch), stride=stride, truncate=truncate, stream=_stream(dev))
    pm.init(I.data_ptr(), pitch, wrange, slope, plane.data_ptr(), cost.data_ptr(), seed=seed, d_start_depth=ptr(d0), start_f32=start_f32, start_planes=planes is not None, **kw)
    pm.iterate(first_iteration, iterations, I.data_ptr(), pitch, wrange, slope, plane.data_ptr(), cost.data_ptr(), seed=seed, **kw)
    pm.finish(plane.data_ptr(), cost.data_ptr(), out.data_ptr(), f32=f32, d_normal=ptr(normal), d_status=ptr(status), **kw)
    outs = [out, normal, plane if return_plane else None, cost if return_cost else None, status]
    outs = [_result(o, as_tensor) for o in outs if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)
