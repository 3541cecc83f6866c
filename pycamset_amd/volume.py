"""Depth maps to a surface mesh on the device: the TSDF volume and the surface-nets extraction (include/pcs_hip.h pcs_tsdf_*,
csrc/ba_tsdf.hpp).

The reference draws everything as ``pyvista`` meshes and leaves the step from views to a surface to the external multi-view program
and to whatever mesher the user runs on that program's cloud.  ``sweep_depth_maps`` / ``stereo_match`` give per-view depth maps and
``fuse_depth_maps`` a de-duplicated cloud; this module integrates the same depth maps into a truncated signed distance volume — free
space is carved: a wrong depth in one view is out-voted by the views that see through it — and extracts a connected quad mesh from it
by naive surface nets.  The rule is stated in full in include/pcs_hip.h and restated in NumPy in tests/tsdf_reference.py.

Conventions follow ``fusion.py``.  Views are DISTORTION-FREE pinholes ``K = [fx, cx, fy, cy]`` with ``[R | t]`` world -> view; depths are
z-depths, float32 or float64, invalid where NaN, +-inf or <= 0.  NumPy arrays are copied to the device and results come back as NumPy
arrays; torch tensors on the device are used in place and the results are torch tensors.  There is no CPU fallback; the argument checks
raise ValueError before anything touches the device.

``raycast_views`` renders the volume back into any pinhole view by marching the distance field (csrc/ba_tsdf_raycast.hpp): the model's
depth and normal per pixel, which says what a view sees of the surface; ``depth_residuals`` holds it against measured depth maps, the
dense counterpart of the reprojection statistics.

Not done here: per-view weights, colour or intensity per vertex (``raycast_views`` gives the visibility it needs), marching cubes, a
sparse or hashed volume, mesh smoothing or simplification, distorted views (undistort first: ``imaging.undistort_images``)."""
from __future__ import annotations

import numpy as np

from ._capi import TSDF_MAX_DIM, TSDF_MAX_WEIGHT, TSDF_RAYCAST_NO_SKIP
from .compiled_helpers import _Handle
from .engine import _stream_arg
from .fusion import MAX_SIDE, MAX_VIEWS
from .imaging import _device_of, _is_tensor, _result, _stream, _to_device, _torch, check_ext


def _number(val, name, positive=True):
    if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) or not np.isfinite(val) or (positive and not val > 0):
        raise ValueError(f"{name}: expected a finite number{' > 0' if positive else ''}, got {val!r}")
    return float(val)


def check_tsdf_args(n_views, width, height, K, ext, origin, voxel, dims, trunc, views=None, n_integrated=0, dtype=np.float32):
    """The checks of pcs_tsdf_set_views, pcs_tsdf_set_grid and pcs_tsdf_integrate on the host; the ValueError names the argument.
    ``n_integrated``: the views the volume already holds.  -> (K (V, 4), P (V, 12), origin (3,), voxel, (nx, ny, nz), trunc, views int32
    or None, f32)."""
    if not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"depth: between 1 and {MAX_VIEWS} views per call, got {n_views}")
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"depth: width and height must be in [1, {MAX_SIDE}], got {width} x {height}")
    Ka = np.asarray(K, dtype=np.float64)
    if Ka.shape != (n_views, 4):
        raise ValueError(f"K: expected ({n_views}, 4) rows [fx, cx, fy, cy], got shape {np.shape(K)}")
    if not np.all(np.isfinite(Ka)) or np.any(Ka[:, 0] == 0) or np.any(Ka[:, 2] == 0):
        raise ValueError("K: every entry must be finite and the focal lengths non-zero")
    P = check_ext(ext, n_views)
    if P is None or not np.all(np.isfinite(P)):
        raise ValueError(f"ext: expected finite ({n_views}, 3, 4) world -> view")
    try:
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError(f"origin: expected three finite numbers, got {origin!r}")
    voxel = _number(voxel, "voxel")
    try:
        d = tuple(dims)
    except TypeError:
        d = ()
    if len(d) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= TSDF_MAX_DIM for n in d):
        raise ValueError(f"dims: expected three integers (nx, ny, nz) in [1, {TSDF_MAX_DIM}], got {dims!r}")
    trunc = _number(trunc, "trunc")
    lst = None
    if views is not None:
        lst = np.asarray(views).reshape(-1)
        if lst.size and not np.issubdtype(lst.dtype, np.integer):
            raise ValueError(f"views: expected integer indices, got {lst.dtype}")
        if lst.size > TSDF_MAX_WEIGHT:
            raise ValueError(f"views: at most {TSDF_MAX_WEIGHT} entries, got {lst.size}")
        if np.any(lst < 0) or np.any(lst >= n_views):
            raise ValueError(f"views: an index outside [0, {n_views})")
        lst = np.ascontiguousarray(lst, dtype=np.int32)
    m = n_views if lst is None else len(lst)
    if n_integrated + m > TSDF_MAX_WEIGHT:
        raise ValueError(f"views: {m} more after {n_integrated} integrated could take a weight past {TSDF_MAX_WEIGHT}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    return np.ascontiguousarray(Ka), P, o, voxel, tuple(int(n) for n in d), trunc, lst, np.dtype(dtype) == np.dtype(np.float32)


class _DeviceArray:
    """Handle-owned device memory as ``__cuda_array_interface__``: torch takes it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


class TsdfVolume(_Handle):
    """Owner of one ``pcs_tsdf_volume`` handle (include/pcs_hip.h): the view table, the volume (``sum`` and ``weight`` per node) and
    the extraction's workspace stay on the device across calls; depth maps, vertices and quads are raw device addresses."""

    _create, _destroy = "pcs_tsdf_create", "pcs_tsdf_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)
        self.origin, self.voxel, self.dims, self.f32, self.n_integrated = None, None, None, True, 0
        self.as_tensor = False   # what integrate_depth_maps saw last: the form extract_surface answers in

    def set_views(self, width, height, K, P):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_tsdf_set_views", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P))

    def set_grid(self, origin, voxel, dims, f32=True):
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        self._call("pcs_tsdf_set_grid", self._h, self._ptr(o), float(voxel), int(dims[0]), int(dims[1]), int(dims[2]), int(bool(f32)))
        self.origin, self.voxel, self.dims, self.f32, self.n_integrated = o.copy(), float(voxel), tuple(int(d) for d in dims), bool(f32), 0

    def reset(self):
        self._call("pcs_tsdf_reset", self._h)
        self.n_integrated = 0

    def integrate(self, d_depth, depth_f32, n_views, trunc, views=None, stream=None):
        """``views`` None: all ``n_views`` views of the table in order; an empty list leaves the volume as it is."""
        lst = None if views is None else np.ascontiguousarray(views, dtype=np.int32).reshape(-1)
        m = int(n_views) if lst is None else len(lst)
        buf = lst if lst is None or lst.size else np.zeros(1, dtype=np.int32)   # an empty list still hands over a pointer: NULL means all views
        self._call("pcs_tsdf_integrate", self._h, self._addr(d_depth), int(bool(depth_f32)), self._ptr(buf), m, float(trunc), _stream_arg(stream))
        self.n_integrated += m

    def volume(self):
        """-> (sum (nz, ny, nx) float32 / float64, weight uint16): torch tensors ON the handle's memory (no copy), valid until the next
        ``set_grid``.  Synchronise the stream an integration was queued on before reading them elsewhere.  torch implements few
        operations on uint16: convert the weights (``.to(torch.int32)``) before comparing or summing them."""
        s, w = self._ct.c_void_p(), self._ct.c_void_p()
        self._call("pcs_tsdf_volume_ptrs", self._h, self._ct.byref(s), self._ct.byref(w))
        torch = _torch()
        nx, ny, nz = self.dims
        dev = torch.device("cuda", self.device)
        return (torch.as_tensor(_DeviceArray(s.value, (nz, ny, nx), "<f4" if self.f32 else "<f8"), device=dev),
                torch.as_tensor(_DeviceArray(w.value, (nz, ny, nx), "<u2"), device=dev))

    def extract_count(self, min_weight=2, stream=None):
        nv, nq = self._ct.c_int64(0), self._ct.c_int64(0)
        self._call("pcs_tsdf_extract_count", self._h, int(min_weight), self._ct.byref(nv), self._ct.byref(nq), _stream_arg(stream))
        return int(nv.value), int(nq.value)

    def extract_write(self, d_vertices, f32, d_quads, stream=None):
        self._call("pcs_tsdf_extract_write", self._h, self._addr(d_vertices), int(bool(f32)), self._addr(d_quads), _stream_arg(stream))

    def raycast(self, width, height, K, P, min_weight, step, z_near, z_far, d_depth, depth_f32, d_normal=None, d_status=None, skip=True, stream=None):
        """The thin call of ``pcs_tsdf_raycast``: ``K`` (V, 4) and ``P`` (V, 12) on the host, the outputs raw device addresses
        (``d_normal`` and ``d_status`` may be None)."""
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_tsdf_raycast", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P), int(min_weight), float(step), float(z_near), float(z_far),
                   self._addr(d_depth), int(bool(depth_f32)), self._addr(d_normal), self._addr(d_status), 0 if skip else TSDF_RAYCAST_NO_SKIP, _stream_arg(stream))

    def raycast_count_samples(self, d_samples, stream=None):
        """For measurements: the last cast over again in a separate launch that writes the samples each pixel evaluated to ``d_samples``
        (V, H, W) uint32; the cast's outputs are not touched."""
        self._call("pcs_tsdf_raycast_count_samples", self._h, self._addr(d_samples), _stream_arg(stream))

    def raycast_last_kernel_ms(self):
        """-> (mask, cast) in ms of the last cast; NaN for a part that did not run."""
        out = []
        for k in range(2):
            ms = self._ct.c_float(0.0)
            args = [None, None]
            args[k] = self._ct.byref(ms)
            rc = getattr(self._capi.lib(), "pcs_tsdf_raycast_last_kernel_ms")(self._h, *args)
            out.append(float(ms.value) if rc == 0 else float("nan"))
        return tuple(out)

    def last_kernel_ms(self):
        """-> (integrate, count, write) in ms; NaN for a part that has not run."""
        out = []
        for k in range(3):
            ms = self._ct.c_float(0.0)
            args = [None, None, None]
            args[k] = self._ct.byref(ms)
            rc = getattr(self._capi.lib(), "pcs_tsdf_last_kernel_ms")(self._h, *args)
            out.append(float(ms.value) if rc == 0 else float("nan"))
        return tuple(out)


def integrate_depth_maps(depth, K, ext, origin, voxel, dims, trunc=None, views=None, dtype=np.float32, volume=None, device=None):
    """Integrate z-depth maps into a TSDF volume (the rule of include/pcs_hip.h).  ``depth`` (V, H, W) float32 / float64; ``K`` (V, 4) =
    [fx, cx, fy, cy]; ``ext`` (V, 3, 4) world -> view; the grid: ``origin`` (3,), ``voxel`` size, ``dims`` = (nx, ny, nz) node counts,
    each at most 1024.  ``trunc`` defaults to ``3 * voxel``.  ``views``: the ordered list of views to integrate (default: all, in order).
    ``dtype``: of the per-node sum, float32 or float64.  ``volume``: a ``TsdfVolume`` from an earlier call to continue (its grid is
    kept; ``origin``, ``voxel``, ``dims`` and ``dtype`` must then be None or the same).  -> the ``TsdfVolume``."""
    torch = _torch()
    if getattr(depth, "ndim", None) != 3:
        raise ValueError(f"depth: expected (V, H, W), got shape {tuple(getattr(depth, 'shape', ()))}")
    name = str(depth.dtype).replace("torch.", "")
    if name not in ("float32", "float64"):
        raise ValueError(f"depth: expected float32 or float64, got {name}")
    V, H, W = (int(v) for v in depth.shape)
    if volume is not None:
        if not isinstance(volume, TsdfVolume) or volume.dims is None:
            raise ValueError("volume: expected a TsdfVolume with a grid")
        origin = volume.origin if origin is None else origin
        voxel = volume.voxel if voxel is None else voxel
        dims = volume.dims if dims is None else dims
        dtype = (np.float32 if volume.f32 else np.float64) if dtype is None else dtype
    if trunc is None:
        trunc = 3 * _number(voxel, "voxel")
    Ka, P, o, voxel, dims, trunc, lst, f32 = check_tsdf_args(V, W, H, K, ext, origin, voxel, dims, trunc, views, 0 if volume is None else volume.n_integrated, dtype)
    if volume is not None and (not np.array_equal(o, volume.origin) or voxel != volume.voxel or dims != volume.dims or f32 != volume.f32):
        raise ValueError("volume: origin, voxel, dims and dtype must be those of the volume that is continued")
    dev = _device_of(depth, device=device) if volume is None else volume.device
    D = _to_device(depth, getattr(torch, name), dev)
    vol = TsdfVolume(dev) if volume is None else volume
    vol.set_views(W, H, Ka, P)
    if volume is None:
        vol.set_grid(o, voxel, dims, f32)
    vol.as_tensor = _is_tensor(depth) and depth.is_cuda
    vol.integrate(D.data_ptr(), name == "float32", V, trunc, lst, stream=_stream(dev))
    torch.cuda.current_stream(dev).synchronize()   # D may be a temporary copy: the integration has read it before it goes
    return vol


def extract_surface(volume, min_weight=2, dtype=np.float32, triangles=False):
    """The quad mesh of a volume by naive surface nets: one vertex per cell the surface passes through with all eight corners seen by
    at least ``min_weight`` views, one quad per grid edge that crosses the surface, its normal pointing from inside to outside.
    -> (vertices (n_v, 3) of ``dtype``, faces (n_q, 4) int32), or faces (2 n_q, 3) with ``triangles``: quad (a, b, c, d) split into
    (a, b, c), (a, c, d) on the host.  Tensors on the device when the volume was integrated from tensors on the device."""
    torch = _torch()
    if not isinstance(volume, TsdfVolume) or volume.dims is None:
        raise ValueError("volume: expected a TsdfVolume with a grid")
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, np.integer)) or not 1 <= min_weight <= TSDF_MAX_WEIGHT:
        raise ValueError(f"min_weight: expected an integer in [1, {TSDF_MAX_WEIGHT}], got {min_weight!r}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    dev = torch.device("cuda", volume.device)
    s = _stream(volume.device)
    nv, nq = volume.extract_count(int(min_weight), stream=s)
    verts = torch.empty((nv, 3), dtype=torch.float32 if f32 else torch.float64, device=dev)
    quads = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    volume.extract_write(verts.data_ptr() if nv else None, f32, quads.data_ptr() if nq else None, stream=s)
    if triangles:
        quads = quads_to_triangles(quads)
    return _result(verts, volume.as_tensor), _result(quads, volume.as_tensor)


def check_raycast_args(n_views, width, height, K, ext, voxel, min_weight=2, step=None, z_near=0.0, z_far=np.inf, dtype=np.float32):
    """The checks of pcs_tsdf_raycast on the host; the ValueError names the argument.  ``voxel``: of the volume that is cast.
    -> (K (V, 4), P (V, 12), min_weight, step, z_near, z_far, f32)."""
    if not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"K: between 1 and {MAX_VIEWS} views per call, got {n_views}")
    for val, name in ((width, "width"), (height, "height")):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or not 1 <= val <= MAX_SIDE:
            raise ValueError(f"{name}: expected an integer in [1, {MAX_SIDE}], got {val!r}")
    Ka = np.asarray(K, dtype=np.float64)
    if Ka.shape != (n_views, 4):
        raise ValueError(f"K: expected ({n_views}, 4) rows [fx, cx, fy, cy], got shape {np.shape(K)}")
    if not np.all(np.isfinite(Ka)) or np.any(Ka[:, 0] == 0) or np.any(Ka[:, 2] == 0):
        raise ValueError("K: every entry must be finite and the focal lengths non-zero")
    P = check_ext(ext, n_views)
    if P is None or not np.all(np.isfinite(P)):
        raise ValueError(f"ext: expected finite ({n_views}, 3, 4) world -> view")
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, np.integer)) or not 1 <= min_weight <= TSDF_MAX_WEIGHT:
        raise ValueError(f"min_weight: expected an integer in [1, {TSDF_MAX_WEIGHT}], got {min_weight!r}")
    voxel = _number(voxel, "voxel")
    step = voxel if step is None else _number(step, "step")
    if not step >= voxel / 64.0:
        raise ValueError(f"step: {step!r} is below voxel / 64 = {voxel / 64.0!r}")
    for val, name in ((z_near, "z_near"), (z_far, "z_far")):
        if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) or val != val:
            raise ValueError(f"{name}: expected a number, got {val!r}")
    if not (0.0 <= z_near < z_far) or not np.isfinite(z_near):
        raise ValueError(f"z_near: expected 0 <= z_near < z_far, got {z_near!r} and z_far {z_far!r}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    return np.ascontiguousarray(Ka), P, int(min_weight), step, float(z_near), float(z_far), np.dtype(dtype) == np.dtype(np.float32)


def _n_views(K):
    shape = np.shape(K)
    if len(shape) != 2:
        raise ValueError(f"K: expected (V, 4) rows [fx, cx, fy, cy], got shape {shape}")
    return shape[0]


def raycast_views(volume, K, ext, width, height, *, min_weight=2, step=None, z_near=0.0, z_far=np.inf, dtype=np.float32, normals=True, status=False, skip=True):
    """Depth and normal maps of a volume as seen by the pinhole views ``K`` (V, 4) = [fx, cx, fy, cy], ``ext`` (V, 3, 4) world -> view,
    of ``width`` x ``height`` pixels, by marching the distance field (the rule of include/pcs_hip.h): the views need not be the ones that
    were integrated.  ``min_weight``: a node counts when at least that many views saw it, as in ``extract_surface``.  ``step``: the
    distance between samples along a ray, default the voxel size, at least voxel / 64.  ``z_near``, ``z_far``: the z-depth range.
    -> depth (V, H, W) of ``dtype``, NaN where the ray meets no surface, and normals (V, H, W, 3) float32 in the world frame pointing
    from inside to outside (None with ``normals=False``); with ``status=True`` also the uint8 status (0 hit, 1 hit without normal, 2 no
    crossing, 3 missed the box or the z-range).  ``skip=False`` casts without the empty-space mask: the same bits, for measuring.
    Tensors on the device when the volume was integrated from tensors on the device, NumPy otherwise."""
    torch = _torch()
    if not isinstance(volume, TsdfVolume) or volume.dims is None:
        raise ValueError("volume: expected a TsdfVolume with a grid")
    Ka, P, min_weight, step, z_near, z_far, f32 = check_raycast_args(_n_views(K), width, height, K, ext, volume.voxel, min_weight, step, z_near, z_far, dtype)
    V, W, H = len(Ka), int(width), int(height)
    dev = torch.device("cuda", volume.device)
    depth = torch.empty((V, H, W), dtype=torch.float32 if f32 else torch.float64, device=dev)
    normal = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev) if normals else None
    stat = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if status else None
    volume.raycast(W, H, Ka, P, min_weight, step, z_near, z_far, depth.data_ptr(), f32, None if normal is None else normal.data_ptr(), None if stat is None else stat.data_ptr(),
                   skip=skip, stream=_stream(volume.device))
    out = (_result(depth, volume.as_tensor), None if normal is None else _result(normal, volume.as_tensor))
    return out + (_result(stat, volume.as_tensor),) if status else out


def depth_residuals(volume, depth, K, ext, **raycast_arguments):
    """The model against measured depth maps, the check to run after ``mesh_views`` / ``integrate_depth_maps``: casts the views of
    ``depth`` (V, H, W) and -> (residual (V, H, W) = model - depth where both are valid, NaN elsewhere; stats (V, 3) float64 = per view the
    count of valid residuals, their median and the median absolute deviation from it: NaN for a view without one).  The keyword
    arguments are those of ``raycast_views`` (the residual has its ``dtype``); the statistics are computed with torch on the device.
    Tensors when the volume was integrated from tensors on the device, NumPy otherwise."""
    torch = _torch()
    if getattr(depth, "ndim", None) != 3:
        raise ValueError(f"depth: expected (V, H, W), got shape {tuple(getattr(depth, 'shape', ()))}")
    for key in ("normals", "status"):
        if key in raycast_arguments:
            raise ValueError(f"{key}: not an argument of depth_residuals")
    V, H, W = (int(v) for v in depth.shape)
    if _n_views(K) != V:
        raise ValueError(f"K: expected ({V}, 4), one row per depth map, got shape {np.shape(K)}")
    as_tensor = volume.as_tensor if isinstance(volume, TsdfVolume) else False
    try:
        if isinstance(volume, TsdfVolume):
            volume.as_tensor = True
        model, _ = raycast_views(volume, K, ext, W, H, normals=False, **raycast_arguments)
    finally:
        if isinstance(volume, TsdfVolume):
            volume.as_tensor = as_tensor
    D = _to_device(depth, model.dtype, volume.device)
    ok = torch.isfinite(model) & torch.isfinite(D) & (D > 0)
    res = torch.where(ok, model - D, torch.full_like(model, float("nan")))
    stats = torch.full((V, 3), float("nan"), dtype=torch.float64, device=res.device)
    for v in range(V):
        r = res[v][ok[v]].to(torch.float64)
        stats[v, 0] = float(r.numel())
        if r.numel():
            med = r.median()
            stats[v, 1], stats[v, 2] = med, (r - med).abs().median()
    return _result(res, as_tensor), _result(stats, as_tensor)


def quads_to_triangles(quads):
    """Quad (a, b, c, d) -> triangles (a, b, c), (a, c, d), keeping the orientation.  (m, 4) -> (2 m, 3); NumPy or torch."""
    tri = quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)
    return tri.contiguous() if _is_tensor(tri) else np.ascontiguousarray(tri)


def grid_from_bounds(bounds, voxel):
    """Two corners -> (origin (3,), dims): nodes from the lower corner in steps of ``voxel`` up to the first at or past the upper one."""
    b = np.asarray(bounds, dtype=np.float64)
    if b.shape != (2, 3) or not np.all(np.isfinite(b)) or np.any(b[1] < b[0]):
        raise ValueError(f"bounds: expected two finite corners (2, 3), lower then upper, got {bounds!r}")
    voxel = _number(voxel, "voxel")
    dims = tuple(int(n) for n in np.ceil((b[1] - b[0]) / voxel - 1e-9).astype(np.int64) + 1)
    return b[0].copy(), dims


def mesh_views(depth, K, ext, bounds, voxel, *, trunc=None, views=None, min_weight=2, dtype=np.float32, triangles=False, device=None):
    """One call from depth maps to a mesh: ``integrate_depth_maps`` on the grid that covers ``bounds`` (two corners, (2, 3)) in steps of
    ``voxel``, then ``extract_surface``.  -> (vertices, faces)."""
    origin, dims = grid_from_bounds(bounds, voxel)
    vol = integrate_depth_maps(depth, K, ext, origin, voxel, dims, trunc=trunc, views=views, device=device)
    try:
        return extract_surface(vol, min_weight=min_weight, dtype=dtype, triangles=triangles)
    finally:
        vol.close()


def volume_from_points(points, voxel, margin=None):
    """``bounds`` (2, 3) for ``mesh_views`` from a cloud, e.g. the output of ``fuse_depth_maps``: the box of the finite points, grown by
    ``margin`` (default ``4 * voxel``: the truncation band and a cell to spare)."""
    p = points.detach().cpu().numpy() if _is_tensor(points) else np.asarray(points)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    p = p[np.all(np.isfinite(p), axis=1)]
    if not len(p):
        raise ValueError("points: no finite point")
    voxel = _number(voxel, "voxel")
    margin = 4 * voxel if margin is None else _number(margin, "margin", positive=False)
    return np.stack([p.min(axis=0) - margin, p.max(axis=0) + margin])


def write_ply(path, vertices, faces):
    """An ASCII PLY of a mesh: ``vertices`` (n, 3), ``faces`` (m, 3) or (m, 4) vertex numbers."""
    v = vertices.detach().cpu().numpy() if _is_tensor(vertices) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if _is_tensor(faces) else np.asarray(faces)
    v, f = np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64)
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError(f"faces: expected (m, 3) or (m, 4), got shape {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces: a vertex number outside the vertices")
    with open(path, "w") as out:
        out.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for x, y, z in v:
            out.write(f"{x:.9g} {y:.9g} {z:.9g}\n")
        for row in f:
            out.write(f"{len(row)} " + " ".join(str(int(i)) for i in row) + "\n")
