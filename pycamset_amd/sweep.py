"""Plane-sweep multi-view depth on the device: from the images of a rig to one z-depth map per view (include/pcs_hip.h pcs_sweep_*,
csrc/ba_sweep.hpp).

For a dense reconstruction of a camera ring the reference leaves the library, and what it hands over is not rectified pairs: it is a
rig, per-view neighbour lists of up to nine views and a depth range cut into steps — ``ReconParams(mindist, maxdist, steps=192,
max_n_view=9)`` (reconstruction/acmmp_utils.py:6-21), the last line ``Camera.to_MVSnet_txt`` writes, ``depth_min interval steps
depth_max`` (cameras/camera.py:158-159), and ``calc_pairs``.  Those are the inputs of a plane sweep: for every pixel of a view and every
depth hypothesis, look the pixel up in all neighbours at once, score photo-consistency, keep the best depth.  The rule is the
library's own (stated in full in include/pcs_hip.h, restated in NumPy in tests/sweep_reference.py); MVSNet / ACMMP are not reproduced.
The depth maps are what ``fusion.fuse_depth_maps`` takes.

Conventions follow ``fusion.py``: views are DISTORTION-FREE pinholes ``K = [fx, cx, fy, cy]`` with ``[R | t]`` world -> view, i.e. the
images are undistorted ones.  NumPy arrays are copied to the device and results come back as NumPy arrays; torch tensors on the device
are used in place and the results are torch tensors.  There is no CPU fallback; the argument checks raise ValueError before anything
touches the device."""
from __future__ import annotations

import numpy as np

from ._capi import SWEEP_MAX_NEIGHBOURS, SWEEP_MAX_PLANES, SWEEP_NO_VIEW, SWEEP_NOT_STRICT, SWEEP_UNIQUENESS  # noqa: F401  (re-exported)
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg
from .fusion import MAX_SIDE, MAX_VIEWS, _csr, fuse_depth_maps, view_neighbours
from .imaging import _device_of, _is_tensor, _result, _stream, _torch, check_ext, check_intr, undistort_images
from .stereo import SGM_MAX_BITS, _u8_on_device

MAX_BOX = 4


def depth_planes(depth_range, steps, spacing="depth"):
    """The hypothesis set of the line ``Camera.to_MVSnet_txt`` writes for ``depth_range`` = (depth_min, depth_max) and ``steps``:
    ``depth_min + k * interval`` for k < steps, interval = (depth_max - depth_min) / steps.  ``spacing="inverse"``: the same count
    uniform in 1 / z between the same ends, 1 / (1 / depth_min + k (1 / z_last - 1 / depth_min) / (steps - 1)) with z_last the last
    plane of the "depth" spacing.  -> (steps,) float64."""
    try:
        lo, hi = (float(v) for v in depth_range)
    except (TypeError, ValueError):
        raise ValueError(f"depth_range: expected (depth_min, depth_max), got {depth_range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"depth_range: expected finite 0 < depth_min < depth_max, got {depth_range!r}")
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= SWEEP_MAX_PLANES:
        raise ValueError(f"steps: expected an integer in [1, {SWEEP_MAX_PLANES}], got {steps!r}")
    if spacing not in ("depth", "inverse"):
        raise ValueError(f"spacing: expected 'depth' or 'inverse', got {spacing!r}")
    k = np.arange(int(steps), dtype=np.float64)
    interval = (hi - lo) / int(steps)
    z = lo + k * interval
    if spacing == "inverse" and steps > 1:
        z = 1.0 / (1.0 / lo + k * ((1.0 / z[-1] - 1.0 / lo) / (int(steps) - 1)))
    return z


def default_truncate(census, box):
    """A quarter of the full scale of a neighbour's cost: (cw ch - 1)(2 r + 1)^2 // 4."""
    return (int(census[0]) * int(census[1]) - 1) * (2 * int(box) + 1) ** 2 // 4


def check_sweep_args(n_views, width, height, pitch, K, ext, neighbours, planes, census=(5, 5), box=2, truncate=None, uniqueness_ratio=0, dtype=np.float32):
    """The checks of pcs_sweep_set_views, pcs_sweep_set_neighbours and pcs_sweep_run on the host; the ValueError names the argument.
    -> (K (V, 4), P (V, 12), nbr_start int32, nbr int32, z (n_z, D) float64, cw, ch, box, truncate, uniqueness_ratio, f32)."""
    def integer(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: expected an integer, got {v!r}")
        return int(v)

    if not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"images: between 1 and {MAX_VIEWS} views per call, got {n_views}")
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"images: width and height must be in [1, {MAX_SIDE}], got {width} x {height}")
    if pitch < width:
        raise ValueError(f"pitch: {pitch} bytes is below the row size {width}")
    Ka = np.asarray(K, dtype=np.float64)
    if Ka.shape != (n_views, 4):
        raise ValueError(f"K: expected ({n_views}, 4) rows [fx, cx, fy, cy], got shape {np.shape(K)}")
    if not np.all(np.isfinite(Ka)) or np.any(Ka[:, 0] == 0) or np.any(Ka[:, 2] == 0):
        raise ValueError("K: every entry must be finite and the focal lengths non-zero")
    P = check_ext(ext, n_views)
    if P is None:
        raise ValueError(f"ext: expected ({n_views}, 3, 4) world -> view")
    start, nbr = _csr(neighbours, n_views)
    if start[0] != 0 or len(nbr) != start[-1] or np.any(np.diff(start) < 0):
        raise ValueError("neighbours: nbr_start must run from 0 to len(nbr) and never decrease")
    for v in range(n_views):
        l = nbr[start[v]:start[v + 1]]
        if len(l) > SWEEP_MAX_NEIGHBOURS:
            raise ValueError(f"neighbours: view {v} has {len(l)} neighbours, more than {SWEEP_MAX_NEIGHBOURS}")
        if np.any(l < 0) or np.any(l >= n_views):
            raise ValueError(f"neighbours: view {v} lists an index outside [0, {n_views})")
        if np.any(l == v):
            raise ValueError(f"neighbours: view {v} lists itself")
        if len(np.unique(l)) != len(l):
            raise ValueError(f"neighbours: view {v} lists a view twice")
    try:
        z = np.asarray(planes, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"planes: expected (D,) or (n_z, D) depths, got {type(planes).__name__}") from None
    if z.ndim == 1:
        z = z[None]
    if z.ndim != 2 or z.shape[0] not in (1, n_views) or not 1 <= z.shape[1] <= SWEEP_MAX_PLANES:
        raise ValueError(f"planes: expected (D,) or (n_z, D) with n_z = 1 or {n_views} and D in [1, {SWEEP_MAX_PLANES}], got shape {np.shape(planes)}")
    if not np.all(np.isfinite(z)) or np.any(z <= 0):
        raise ValueError("planes: every depth must be finite and > 0")
    d = np.diff(z, axis=1)
    if d.size and not all(np.all(row > 0) or np.all(row < 0) for row in d):
        raise ValueError("planes: every row must be strictly monotone")
    try:
        cw, ch = census
    except (TypeError, ValueError):
        raise ValueError(f"census: expected (width, height), got {census!r}") from None
    cw, ch = integer(cw, "census"), integer(ch, "census")
    if cw < 3 or ch < 3 or cw % 2 == 0 or ch % 2 == 0 or cw * ch - 1 > SGM_MAX_BITS:
        raise ValueError(f"census: expected odd sides >= 3 with width * height - 1 <= {SGM_MAX_BITS}, got {cw} x {ch}")
    box = integer(box, "box")
    if not 0 <= box <= MAX_BOX:
        raise ValueError(f"box: expected a radius in [0, {MAX_BOX}], got {box}")
    full = (cw * ch - 1) * (2 * box + 1) ** 2
    truncate = default_truncate((cw, ch), box) if truncate is None else integer(truncate, "truncate")
    if not 1 <= truncate <= full:
        raise ValueError(f"truncate: expected an integer in [1, {full}], got {truncate}")
    uniq = integer(uniqueness_ratio, "uniqueness_ratio")
    if not 0 <= uniq <= 100:
        raise ValueError(f"uniqueness_ratio: expected an integer in [0, 100], got {uniq}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    return (np.ascontiguousarray(Ka), P, np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(nbr, dtype=np.int32), np.ascontiguousarray(z), cw, ch, box, truncate,
            uniq, np.dtype(dtype) == np.dtype(np.float32))


class PlaneSweeper(_Handle):
    """Owner of one ``pcs_plane_sweeper`` handle (include/pcs_hip.h): the neighbour lists, the warp table and the plane table stay on
    the device across calls; images and outputs are raw device addresses used in place."""

    _create, _destroy = "pcs_sweep_create", "pcs_sweep_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)

    def set_views(self, width, height, K, P):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_sweep_set_views", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P))

    def set_neighbours(self, nbr_start, nbr):
        nbr_start, nbr = np.ascontiguousarray(nbr_start, dtype=np.int32), np.ascontiguousarray(nbr, dtype=np.int32)
        self._call("pcs_sweep_set_neighbours", self._h, self._ptr(nbr_start), self._ptr(nbr) if nbr.size else None, len(nbr_start) - 1)

    def run(self, d_images, pitch, z, d_depth, *, census=(5, 5), box=2, truncate=None, uniqueness_ratio=0, f32=True, d_level=None, d_cost=None, d_status=None, stream=None):
        z = np.ascontiguousarray(z, dtype=np.float64)
        z = z[None] if z.ndim == 1 else z
        truncate = default_truncate(census, box) if truncate is None else truncate
        self._call("pcs_sweep_run", self._h, self._addr(d_images), int(pitch), self._ptr(z), z.shape[0], z.shape[1], int(census[0]), int(census[1]), int(box), int(truncate),
                   int(uniqueness_ratio), self._addr(d_depth), int(bool(f32)), self._addr(d_level), self._addr(d_cost), self._addr(d_status), _stream_arg(stream))

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_sweep_last_kernel_ms")


_sweeper_cache: dict = {}


def _sweeper(device: int) -> PlaneSweeper:
    return _cached_handle(_sweeper_cache, int(device), lambda: PlaneSweeper(device))


def sweep_depth_maps(images, K, ext, neighbours, planes, *, census=(5, 5), box=2, truncate=None, uniqueness_ratio=0, dtype=np.float32, return_level=False, return_cost=False,
                     return_status=False, device=None):
    """One z-depth map per view by a plane sweep over its neighbours (the rule of include/pcs_hip.h).  ``images`` (V, H, W) uint8, the
    undistorted images; ``K`` (V, 4) = [fx, cx, fy, cy]; ``ext`` (V, 3, 4) world -> view; ``neighbours``: a list of index sequences,
    one per view, or a CSR pair — at most 16 per view (``fusion.view_neighbours`` makes them); ``planes``: (D,) depths for every view
    or (V, D) per view (``depth_planes`` makes them), D <= 1024.  The cost of a plane is the Hamming distance of ``census`` = (width,
    height) descriptors of the reference image and of each neighbour warped onto the plane, summed over a box of radius ``box``,
    truncated at ``truncate`` per neighbour (default: a quarter of the full scale) and added over the neighbours; the plane of the
    smallest cost wins, refined between planes by the block matcher's parabola.  ``uniqueness_ratio`` > 0 rejects a winner that a plane
    two or more steps away comes within that many percent of.
    -> depth (V, H, W) of ``dtype``, NaN where nothing was accepted[, level int32 = 16 k* + offset (-16 outside the strict rectangle)
    (``return_level``)][, cost int32 (-1 there) (``return_cost``)][, status uint8, bits SWEEP_* (``return_status``)]; a tuple when
    any of the three is asked for."""
    torch = _torch()
    if getattr(images, "ndim", None) != 3:
        raise ValueError(f"images: expected (V, H, W) uint8, got shape {tuple(getattr(images, 'shape', ()))}")
    V, H, W = (int(v) for v in images.shape)
    as_tensor = _is_tensor(images) and images.is_cuda
    if str(images.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"images: expected uint8, got {images.dtype}")
    Ka, P, start, nbr, z, cw, ch, box, truncate, uniq, f32 = check_sweep_args(V, W, H, W, K, ext, neighbours, planes, census, box, truncate, uniqueness_ratio, dtype)
    dev = _device_of(images, device=device)
    I, pitch = _u8_on_device(images, "images", dev)
    sw = _sweeper(dev)
    sw.set_views(W, H, Ka, P)
    sw.set_neighbours(start, nbr)
    depth = torch.empty((V, H, W), dtype=torch.float32 if f32 else torch.float64, device=I.device)
    level = torch.empty((V, H, W), dtype=torch.int32, device=I.device) if return_level else None
    cost = torch.empty((V, H, W), dtype=torch.int32, device=I.device) if return_cost else None
    status = torch.empty((V, H, W), dtype=torch.uint8, device=I.device) if return_status else None
    ptr = lambda t: None if t is None else t.data_ptr()
    sw.run(I.data_ptr(), pitch, z, depth.data_ptr(), census=(cw, ch), box=box, truncate=truncate, uniqueness_ratio=uniq, f32=f32, d_level=ptr(level), d_cost=ptr(cost),
           d_status=ptr(status), stream=_stream(dev))
    outs = [_result(o, as_tensor) for o in (depth, level, cost, status) if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def reconstruct_views(images, intr, ext, depth_range, steps=192, *, spacing="depth", neighbours=None, min_angle=3.0, max_angle=45.0, max_views=9, census=(5, 5), box=2,
                      truncate=None, uniqueness_ratio=15, interpolation: str = "bilinear", px_tol=1.0, rel_tol=0.01, min_views=2, unique=False, transform=None,
                      dtype=np.float32, device=None, refine_iterations=0):
    """From the images of a calibrated rig to one cloud: ``undistort_images`` -> ``view_neighbours`` -> ``sweep_depth_maps`` ->
    ``fuse_depth_maps(values=, compact=True)``.  ``refine_iterations`` > 0: the sweep's depth maps pass through that many iterations of
    ``patchmatch.refine_depth_maps`` in front of the fusion: its defaults, the search bounded by ``depth_range``, and ``max_slant`` =
    90 - ``max_angle`` degrees (at most its default 70, at least 10) — a surface seen at slant s from one view is seen at up to s +
    ``max_angle`` from a neighbour, and past 90 degrees there is nothing to match.  A thin composition: no kernel of its own.  ``images`` (C, H, W) uint8, one per camera;
    ``intr`` (C, 9); ``ext`` (C, 3, 4) world -> camera; ``depth_range`` = (depth_min, depth_max) and ``steps`` as ``ReconParams`` /
    ``to_MVSnet_txt`` hand them over.  ``neighbours`` defaults to ``view_neighbours(ext, min_angle, max_angle, max_views)``.  Every view
    keeps its own consistent pixels; ``unique=True`` leaves a surface element to the lowest view that sees it (``fuse_depth_maps``).
    -> (points (M, 3) in the world frame, or in ``transform``'s, grey values (M,) uint8), the views concatenated in order.
    ``reconstruct_views.last`` holds (K, neighbours, planes, depth maps, per-view counts)."""
    Kc = check_intr(intr)
    C = int(images.shape[0])
    E = check_ext(ext, C).reshape(C, 3, 4)
    dev = _device_of(images, device=device)
    und = undistort_images(images, np.arange(C), Kc, interpolation=interpolation, device=dev)
    und = und.reshape(images.shape)
    Kv = np.ascontiguousarray(Kc[:, :4])
    nb = view_neighbours(E, min_angle, max_angle, min(int(max_views), SWEEP_MAX_NEIGHBOURS)) if neighbours is None else neighbours
    planes = depth_planes(depth_range, steps, spacing)
    depth = sweep_depth_maps(und, Kv, E, nb, planes, census=census, box=box, truncate=truncate, uniqueness_ratio=uniqueness_ratio, dtype=np.float64, device=dev)
    if refine_iterations:
        from .patchmatch import refine_depth_maps

        depth = refine_depth_maps(und, Kv, E, nb, depth_range, depth, iterations=refine_iterations, max_slant=min(70.0, max(10.0, 90.0 - float(max_angle))), dtype=np.float64,
                                  device=dev)
    clouds = fuse_depth_maps(depth, Kv, E, nb, px_tol=px_tol, rel_tol=rel_tol, min_views=min_views, unique=unique, transform=transform, values=und, compact=True, dtype=dtype,
                             device=dev)
    cat = _torch().cat if _is_tensor(clouds[0][0]) else np.concatenate
    reconstruct_views.last = (Kv, nb, planes, depth, [len(c[0]) for c in clouds])
    return cat([c[0] for c in clouds]), cat([c[1] for c in clouds])
