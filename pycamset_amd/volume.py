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

``colour_points`` / ``colour_surface`` / ``colour_views`` bring the images back onto the geometry (csrc/ba_tsdf_colour.hpp): per mesh
vertex, or per pixel of a rendered view, the colour of the source views that see the point, with the model's own depth in each source
view deciding the occlusion and the normal deciding the weight.

Not done here: per-view weights, marching cubes, a sparse or hashed volume, mesh smoothing or simplification, distorted views
(undistort first: ``imaging.undistort_images``), texture atlases and UV maps, exposure or white-balance compensation between views,
colour stored in the volume during integration, seam levelling."""
from __future__ import annotations

import numpy as np

from ._capi import COLOUR_MODE_IDS, IMAP_DTYPE_IDS, TSDF_MAX_DIM, TSDF_MAX_WEIGHT, TSDF_RAYCAST_NO_SKIP
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

    def point_normals(self, n, d_points, point_f32, min_weight, d_normals, d_status=None, stream=None):
        """The thin call of ``pcs_tsdf_point_normals``: raw device addresses."""
        self._call("pcs_tsdf_point_normals", self._h, int(n), self._addr(d_points), int(bool(point_f32)), int(min_weight), self._addr(d_normals), self._addr(d_status),
                   _stream_arg(stream))

    def _colour_source(self, src):
        """The arguments both colour calls share, from the dict ``check_colour_args`` returns and the device addresses added to it."""
        fill = np.ascontiguousarray(src["fill"], dtype=np.float64)
        return (src["K"].shape[0], src["width"], src["height"], self._ptr(src["K"]), self._ptr(src["P"]), self._addr(src["d_images"]), int(src["pitch"]), src["channels"],
                IMAP_DTYPE_IDS[src["image_dtype"]], self._addr(src.get("d_visibility")), int(bool(src.get("visibility_f32", True))), float(src["occlusion_tol"]),
                float(src["cos_min"]), COLOUR_MODE_IDS[src["mode"]], self._ptr(fill), self._addr(src["d_colour"]), IMAP_DTYPE_IDS[src["dtype"]], self._addr(src.get("d_weight")),
                self._addr(src.get("d_count")), self._addr(src.get("d_best")))

    def colour_points(self, n, d_points, point_f32, d_normals, src, stream=None):
        """The thin call of ``pcs_tsdf_colour_points``; ``src``: see ``_colour_source``."""
        self._call("pcs_tsdf_colour_points", self._h, int(n), self._addr(d_points), int(bool(point_f32)), self._addr(d_normals), *self._colour_source(src), _stream_arg(stream))

    def colour_views(self, width, height, K, P, d_depth, depth_f32, d_normal, src, stream=None):
        """The thin call of ``pcs_tsdf_colour_views``: the render views ``K`` (R, 4), ``P`` (R, 12) on the host."""
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_tsdf_colour_views", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P), self._addr(d_depth), int(bool(depth_f32)), self._addr(d_normal),
                   *self._colour_source(src), _stream_arg(stream))

    def colour_last_kernel_ms(self):
        """-> (point normals, colour) in ms; NaN for a part that has not run."""
        out = []
        for k in range(2):
            ms = self._ct.c_float(0.0)
            args = [None, None]
            args[k] = self._ct.byref(ms)
            rc = getattr(self._capi.lib(), "pcs_tsdf_colour_last_kernel_ms")(self._h, *args)
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


def _dtype_name(a):
    return str(getattr(a, "dtype", "")).replace("torch.", "")


def check_colour_args(images, K, ext, *, normals=None, n_points=None, visibility=None, occlusion_tol=None, cos_min=0.0, mode="blend", fill=None, dtype=None):
    """The checks of pcs_tsdf_colour_points / pcs_tsdf_colour_views on the source side, on the host; the ValueError names the argument.
    Only shapes and dtypes of ``images``, ``normals`` and ``visibility`` are looked at (NumPy arrays or tensors).  -> dict(K (V, 4), P (V, 12),
    width, height, channels, image_dtype, occlusion_tol, cos_min, mode, fill (channels,) float64, dtype: 'uint8' or 'float32')."""
    shape = tuple(int(n) for n in getattr(images, "shape", ()))
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] not in (1, 3, 4)):
        raise ValueError(f"images: expected (V, H, W) or (V, H, W, C) with C of 1, 3 or 4, got shape {shape}")
    image_dtype = _dtype_name(images)
    if image_dtype not in ("uint8", "float32"):
        raise ValueError(f"images: expected uint8 or float32, got {image_dtype or type(images).__name__}")
    V, H, W = shape[:3]
    C = shape[3] if len(shape) == 4 else 1
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"images: between 1 and {MAX_VIEWS} views per call, got {V}")
    if not (2 <= W <= MAX_SIDE and 2 <= H <= MAX_SIDE):
        raise ValueError(f"images: width and height must be in [2, {MAX_SIDE}], got {W} x {H}")
    Ka = np.asarray(K, dtype=np.float64)
    if Ka.shape != (V, 4):
        raise ValueError(f"K: expected ({V}, 4) rows [fx, cx, fy, cy], one per image, got shape {np.shape(K)}")
    if not np.all(np.isfinite(Ka)) or np.any(Ka[:, 0] == 0) or np.any(Ka[:, 2] == 0):
        raise ValueError("K: every entry must be finite and the focal lengths non-zero")
    P = check_ext(ext, V)
    if P is None or not np.all(np.isfinite(P)):
        raise ValueError(f"ext: expected finite ({V}, 3, 4) world -> view")
    if normals is not None:
        nshape = tuple(int(n) for n in getattr(normals, "shape", ()))
        if len(nshape) < 2 or nshape[-1] != 3 or (n_points is not None and int(np.prod(nshape[:-1])) != n_points):
            raise ValueError(f"normals: expected ({'N' if n_points is None else n_points}, 3), one per point, got shape {nshape}")
        if _dtype_name(normals) not in ("float32", "float64"):
            raise ValueError(f"normals: expected float32 or float64, got {_dtype_name(normals) or type(normals).__name__}")
    if visibility is not None:
        if tuple(int(n) for n in getattr(visibility, "shape", ())) != (V, H, W):
            raise ValueError(f"visibility: expected ({V}, {H}, {W}), one depth map per image, got shape {tuple(getattr(visibility, 'shape', ()))}")
        if _dtype_name(visibility) not in ("float32", "float64"):
            raise ValueError(f"visibility: expected float32 or float64, got {_dtype_name(visibility)}")
        if occlusion_tol is None:
            raise ValueError("occlusion_tol: must be given with visibility maps (world units; sqrt(3) voxel for a model's own depth)")
    if occlusion_tol is not None:
        occlusion_tol = _number(occlusion_tol, "occlusion_tol", positive=False)
        if occlusion_tol < 0:
            raise ValueError(f"occlusion_tol: expected a finite number >= 0, got {occlusion_tol!r}")
    else:
        occlusion_tol = 0.0
    cos_min = _number(cos_min, "cos_min", positive=False)
    if not 0.0 <= cos_min < 1.0:
        raise ValueError(f"cos_min: expected a number in [0, 1), got {cos_min!r}")
    if mode not in COLOUR_MODE_IDS:
        raise ValueError(f"mode: expected one of {sorted(COLOUR_MODE_IDS)}, got {mode!r}")
    try:
        fl = np.zeros(C) if fill is None else np.broadcast_to(np.asarray(fill, dtype=np.float64), (C,)).copy()
    except (TypeError, ValueError):
        fl = None
    if fl is None or np.any(np.isinf(fl)):
        raise ValueError(f"fill: expected a number or {C} numbers, none infinite, got {fill!r}")
    try:
        out = image_dtype if dtype is None else np.dtype(dtype).name
    except TypeError:
        out = ""
    if out not in ("uint8", "float32"):
        raise ValueError(f"dtype: expected uint8 or float32, got {dtype!r}")
    return dict(K=np.ascontiguousarray(Ka), P=P, width=W, height=H, channels=C, image_dtype=image_dtype, occlusion_tol=occlusion_tol, cos_min=cos_min, mode=mode, fill=fl, dtype=out)


def _check_points(points, name="points"):
    shape = tuple(int(n) for n in getattr(points, "shape", ()))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{name}: expected (N, 3), got shape {shape}")
    if _dtype_name(points) not in ("float32", "float64"):
        raise ValueError(f"{name}: expected float32 or float64, got {_dtype_name(points) or type(points).__name__}")
    return shape[0], _dtype_name(points) == "float32"


def _colour_run(a, dev, images, visibility, out_shape, launch):
    """Copies what is on the host to the device, allocates the outputs of shape ``out_shape`` + (...), runs ``launch(src)`` and waits.
    -> (colour, weight, count, best) tensors on the device."""
    torch = _torch()
    device = torch.device("cuda", dev)
    img = _to_device(images, getattr(torch, a["image_dtype"]), dev)
    vis = None if visibility is None else _to_device(visibility, getattr(torch, _dtype_name(visibility)), dev)
    colour = torch.empty(tuple(out_shape) + (a["channels"],), dtype=getattr(torch, a["dtype"]), device=device)
    weight = torch.empty(tuple(out_shape), dtype=torch.float32, device=device)
    count = torch.empty(tuple(out_shape), dtype=torch.uint16, device=device)
    best = torch.empty(tuple(out_shape), dtype=torch.int32, device=device)
    src = dict(a, d_images=img.data_ptr(), pitch=a["width"] * a["channels"] * img.element_size(), d_visibility=None if vis is None else vis.data_ptr(),
               visibility_f32=vis is None or vis.dtype == torch.float32, d_colour=colour.data_ptr() if colour.numel() else 1, d_weight=weight.data_ptr(), d_count=count.data_ptr(),
               d_best=best.data_ptr())
    launch(src)
    torch.cuda.current_stream(dev).synchronize()   # img and vis may be temporary copies: the kernel has read them before they go
    return colour, weight, count, best


def _colour_out(outs, as_tensor, info):
    outs = tuple(_result(t, as_tensor) for t in outs)
    return outs if info else outs[0]


def vertex_normals(volume, vertices, min_weight=2, status=False):
    """The ray-cast's normal rule at arbitrary points of a volume, e.g. the vertices of ``extract_surface``: central differences of the
    distance field one node apart, in the world frame, pointing from inside to outside.  -> normals (N, 3) float32, NaN where one of the
    six samples leaves the box or meets a node fewer than ``min_weight`` views saw; with ``status=True`` also the uint8 status (0 with a
    normal, 1 without).  Tensors on the device when ``vertices`` is one, NumPy otherwise."""
    torch = _torch()
    if not isinstance(volume, TsdfVolume) or volume.dims is None:
        raise ValueError("volume: expected a TsdfVolume with a grid")
    n, f32 = _check_points(vertices, "vertices")
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, np.integer)) or not 1 <= min_weight <= TSDF_MAX_WEIGHT:
        raise ValueError(f"min_weight: expected an integer in [1, {TSDF_MAX_WEIGHT}], got {min_weight!r}")
    as_tensor = _is_tensor(vertices) and vertices.is_cuda
    dev = volume.device
    X = _to_device(vertices, torch.float32 if f32 else torch.float64, dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=X.device)
    stat = torch.empty((n,), dtype=torch.uint8, device=X.device)
    volume.point_normals(n, X.data_ptr() if n else None, f32, int(min_weight), normals.data_ptr() if n else None, stat.data_ptr() if n else None, stream=_stream(dev))
    torch.cuda.current_stream(dev).synchronize()
    return (_result(normals, as_tensor), _result(stat, as_tensor)) if status else _result(normals, as_tensor)


def colour_points(points, images, K, ext, *, normals=None, visibility=None, occlusion_tol=None, cos_min=0.0, mode="blend", fill=None, dtype=None, info=False, volume=None,
                  device=None):
    """The colour of ``points`` (N, 3) from the source ``images`` (V, H, W) or (V, H, W, C), C of 1, 3 or 4, uint8 or float32, of the
    distortion-free views ``K`` (V, 4) = [fx, cx, fy, cy], ``ext`` (V, 3, 4) world -> view (the rule of include/pcs_hip.h).  A view
    contributes when the point lies in front of it and projects into its image, when it is not occluded — ``visibility`` (V, H, W): a
    depth map per view, the point's depth may exceed it by ``occlusion_tol`` at most — and when it faces the view: with ``normals``
    (N, 3) the cosine c between the normal and the direction to the camera must exceed ``cos_min``.  ``mode`` "blend": the mean of the
    bilinear samples weighted by c; "best": the sample of the view with the largest c.  ``fill``: the colour of a point no view
    contributes to.  ``dtype``: uint8 or float32, default that of the images.  ``volume``: a ``TsdfVolume`` whose handle is used (default:
    a temporary one; no grid is needed).  -> colour (N, C); with ``info=True`` (colour, weight (N) float32, count (N) uint16, best (N)
    int32: the sum of the c, the number of contributing views, the view with the largest c or -1).  Tensors on the device when ``points``
    is one, NumPy otherwise."""
    torch = _torch()
    n, f32 = _check_points(points)
    a = check_colour_args(images, K, ext, normals=normals, n_points=n, visibility=visibility, occlusion_tol=occlusion_tol, cos_min=cos_min, mode=mode, fill=fill, dtype=dtype)
    if volume is not None and not isinstance(volume, TsdfVolume):
        raise ValueError("volume: expected a TsdfVolume or None")
    as_tensor = _is_tensor(points) and points.is_cuda
    dev = volume.device if volume is not None else _device_of(points, images, device=device)
    X = _to_device(points, torch.float32 if f32 else torch.float64, dev)
    nrm = None if normals is None else _to_device(normals, torch.float32, dev).reshape(-1, 3)
    vol = TsdfVolume(dev) if volume is None else volume
    try:
        outs = _colour_run(a, dev, images, visibility, (n,),
                           lambda src: vol.colour_points(n, X.data_ptr() if n else None, f32, None if nrm is None or not n else nrm.data_ptr(), src, stream=_stream(dev)))
    finally:
        if volume is None:
            vol.close()
    return _colour_out(outs, as_tensor, info)


def _cast_on_device(volume, K, ext, width, height, **kw):
    """``raycast_views`` with tensors on the device as the result, whatever the volume was integrated from."""
    as_tensor = volume.as_tensor
    try:
        volume.as_tensor = True
        return raycast_views(volume, K, ext, width, height, **kw)
    finally:
        volume.as_tensor = as_tensor


def colour_surface(volume, vertices, images, K, ext, *, min_weight=2, step=None, occlusion_tol=None, cos_min=0.0, mode="blend", fill=None, dtype=None, info=False):
    """The colour of mesh ``vertices`` (N, 3) of a volume from the images of its source views: ``vertex_normals`` for the weights, the
    model's own depth in every source view (``raycast_views`` with ``min_weight`` and ``step``) for the occlusion, then ``colour_points``
    with its remaining arguments; ``occlusion_tol`` defaults to sqrt(3) voxel, the diagonal of a cell.  A vertex without a normal takes
    the fill.  -> colours (N, C), or (colours, weight, count, best) with ``info=True``."""
    if not isinstance(volume, TsdfVolume) or volume.dims is None:
        raise ValueError("volume: expected a TsdfVolume with a grid")
    n, _ = _check_points(vertices, "vertices")
    tol = np.sqrt(3.0) * volume.voxel if occlusion_tol is None else occlusion_tol
    a = check_colour_args(images, K, ext, occlusion_tol=tol, cos_min=cos_min, mode=mode, fill=fill, dtype=dtype)
    torch = _torch()
    as_tensor = _is_tensor(vertices) and vertices.is_cuda
    X = _to_device(vertices, torch.float32 if _dtype_name(vertices) == "float32" else torch.float64, volume.device)
    normals = vertex_normals(volume, X, min_weight)
    model, _ = _cast_on_device(volume, a["K"], a["P"].reshape(-1, 3, 4), a["width"], a["height"], min_weight=min_weight, step=step, normals=False)
    outs = colour_points(X, images, K, ext, normals=normals, visibility=model, occlusion_tol=tol, cos_min=cos_min, mode=mode, fill=fill, dtype=dtype, info=True, volume=volume)
    return _colour_out(outs, as_tensor, info)


def colour_views(volume, K_render, ext_render, width, height, images, K, ext, *, min_weight=2, step=None, z_near=0.0, z_far=np.inf, occlusion_tol=None, cos_min=0.0,
                 mode="blend", fill=None, dtype=None, info=False):
    """The coloured rendering of a volume from any pinhole pose: ``raycast_views`` into the render views ``K_render`` (R, 4),
    ``ext_render`` (R, 3, 4) of ``width`` x ``height`` pixels, the model's own depth in every source view for the occlusion, then the
    rule of ``colour_points`` with the surface point of every pixel as the point and its normal for the weights.  A pixel whose ray
    meets no surface takes the fill.  -> (colour (R, H, W, C), depth (R, H, W) float32), with ``info=True`` also weight, count and best
    (R, H, W).  Tensors on the device when the volume was integrated from tensors on the device, NumPy otherwise."""
    if not isinstance(volume, TsdfVolume) or volume.dims is None:
        raise ValueError("volume: expected a TsdfVolume with a grid")
    Kr, Pr, min_weight, step, z_near, z_far, _ = check_raycast_args(_n_views(K_render), width, height, K_render, ext_render, volume.voxel, min_weight, step, z_near, z_far)
    tol = np.sqrt(3.0) * volume.voxel if occlusion_tol is None else occlusion_tol
    a = check_colour_args(images, K, ext, occlusion_tol=tol, cos_min=cos_min, mode=mode, fill=fill, dtype=dtype)
    R, W, H = len(Kr), int(width), int(height)
    dev = volume.device
    depth, normal = _cast_on_device(volume, Kr, Pr.reshape(-1, 3, 4), W, H, min_weight=min_weight, step=step, z_near=z_near, z_far=z_far)
    model, _ = _cast_on_device(volume, a["K"], a["P"].reshape(-1, 3, 4), a["width"], a["height"], min_weight=min_weight, step=step, normals=False)
    outs = _colour_run(a, dev, images, model, (R, H, W),
                       lambda src: volume.colour_views(W, H, Kr, Pr, depth.data_ptr(), True, normal.data_ptr(), src, stream=_stream(dev)))
    outs = (outs[0], depth) + outs[1:]
    return tuple(_result(t, volume.as_tensor) for t in (outs if info else outs[:2]))


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


def mesh_views(depth, K, ext, bounds, voxel, *, trunc=None, views=None, min_weight=2, dtype=np.float32, triangles=False, device=None, images=None, **colour_arguments):
    """One call from depth maps to a mesh: ``integrate_depth_maps`` on the grid that covers ``bounds`` (two corners, (2, 3)) in steps of
    ``voxel``, then ``extract_surface``.  -> (vertices, faces).  With ``images`` (V, H, W[, C]), the images of the views of ``depth``,
    -> (vertices, faces, colours): ``colour_surface`` on the vertices, with its keyword arguments."""
    if images is None and colour_arguments:
        raise ValueError(f"images: {sorted(colour_arguments)} are arguments of colour_surface and need images")
    origin, dims = grid_from_bounds(bounds, voxel)
    vol = integrate_depth_maps(depth, K, ext, origin, voxel, dims, trunc=trunc, views=views, device=device)
    try:
        mesh = extract_surface(vol, min_weight=min_weight, dtype=dtype, triangles=triangles)
        if images is None:
            return mesh
        return mesh + (colour_surface(vol, mesh[0], images, K, ext, min_weight=min_weight, **colour_arguments),)
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


def write_ply(path, vertices, faces, colours=None, normals=None):
    """An ASCII PLY of a mesh: ``vertices`` (n, 3), ``faces`` (m, 3) or (m, 4) vertex numbers.  ``normals`` (n, 3) are written as nx, ny, nz
    and ``colours`` (n,), (n, 1), (n, 3) or (n, 4) as uchar red, green, blue[, alpha] (one channel: grey on all three; float colours
    are rounded half-to-even and saturated)."""
    host = lambda a: a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)
    v, f = np.asarray(host(vertices), dtype=np.float64).reshape(-1, 3), np.asarray(host(faces), dtype=np.int64)
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError(f"faces: expected (m, 3) or (m, 4), got shape {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces: a vertex number outside the vertices")
    extra, columns = "", []
    if normals is not None:
        n = np.asarray(host(normals), dtype=np.float64)
        if n.shape != v.shape:
            raise ValueError(f"normals: expected {v.shape}, got shape {n.shape}")
        extra += "property float nx\nproperty float ny\nproperty float nz\n"
        columns.append([" ".join(f"{c:.9g}" for c in row) for row in n])
    if colours is not None:
        c = host(colours)
        c = c.reshape(len(c), -1) if c.ndim in (1, 2) else c
        if c.ndim != 2 or c.shape[0] != len(v) or c.shape[1] not in (1, 3, 4):
            raise ValueError(f"colours: expected ({len(v)},) or ({len(v)}, 1 | 3 | 4), got shape {np.shape(colours)}")
        if c.dtype != np.uint8:
            with np.errstate(invalid="ignore"):
                c = np.clip(np.nan_to_num(np.rint(c.astype(np.float64)), nan=0.0), 0, 255).astype(np.uint8)
        if c.shape[1] == 1:
            c = np.repeat(c, 3, axis=1)
        extra += "".join(f"property uchar {name}\n" for name in ("red", "green", "blue", "alpha")[:c.shape[1]])
        columns.append([" ".join(str(int(x)) for x in row) for row in c])
    with open(path, "w") as out:
        out.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n{extra}"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for i, (x, y, z) in enumerate(v):
            out.write(" ".join([f"{x:.9g} {y:.9g} {z:.9g}"] + [col[i] for col in columns]) + "\n")
        for row in f:
            out.write(f"{len(row)} " + " ".join(str(int(i)) for i in row) + "\n")
