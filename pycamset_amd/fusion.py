"""Depth-map fusion across views on the device: the geometric consistency filter and the merged cloud (include/pcs_hip.h pcs_fuse_*,
csrc/ba_fusion.hpp).

The reference does not fuse the clouds of a camera ring itself.  It writes the rig out for an external multi-view program and reads
that program's fused cloud back: ``CameraSet.write_to_txt`` (cameras/camera_set.py:235-272), ``Camera.to_MVSnet_txt`` (cameras/
camera.py:130-160), ``calc_pairs`` / ``write_pair_file`` (reconstruction/acmmp_utils.py:24-83).  The step that program adds over
per-view depth maps — keep a depth only where enough neighbouring views agree with it, merge the agreeing observations into one
point — is what this module does, by the library's own rule (stated in full in include/pcs_hip.h, restated in NumPy in
tests/fusion_reference.py), in the spirit of MVSNet's ``filter_depth``.

Conventions follow ``stereo.py``.  Views are DISTORTION-FREE pinholes ``K = [fx, cx, fy, cy]`` with ``[R | t]`` world -> view, i.e. the
depth maps are those of undistorted or rectified images; depths are z-depths, float32 or float64, invalid where NaN, +-inf or <= 0.
NumPy arrays are copied to the device and results come back as NumPy arrays; torch tensors on the device are used in place and the
results are torch tensors.  There is no CPU fallback; the argument checks raise ValueError before anything touches the device."""
from __future__ import annotations

import numpy as np

from ._capi import FUSE_DUPLICATE, FUSE_FEW_VIEWS, FUSE_INVALID_DEPTH, FUSE_MAX_NEIGHBOURS  # noqa: F401  (re-exported)
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg
from .imaging import _device_of, _is_tensor, _result, _stream, _to_device, _torch, check_ext, rectify_images
from .stereo import _matcher, _plane_stack, _u8_on_device, disparity_to_points, stereo_match

MAX_VIEWS, MAX_SIDE = 32767, 65535


def _csr(neighbours, n_views):
    """A list of index sequences or a (nbr_start, nbr) pair -> (nbr_start (V + 1), nbr) as Python-int arrays (int64, unchecked)."""
    try:
        if isinstance(neighbours, tuple) and len(neighbours) == 2 and np.ndim(neighbours[0]) == 1 and len(neighbours[0]) == n_views + 1 and np.ndim(neighbours[1]) == 1:
            start, nbr = np.asarray(neighbours[0]), np.asarray(neighbours[1])   # a TUPLE of two arrays, the first V + 1 long, is the CSR pair
        else:
            lists = [np.asarray(l).reshape(-1) if len(l) else np.zeros(0, dtype=np.int64) for l in neighbours]
            if len(lists) != n_views:
                raise ValueError(f"neighbours: expected one list per view ({n_views}) or a CSR pair (nbr_start ({n_views + 1},), nbr), got {len(lists)} lists")
            start = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
            nbr = np.concatenate(lists + [np.zeros(0, dtype=np.int64)])
    except TypeError:
        raise ValueError(f"neighbours: expected a list of index sequences or a CSR pair, got {type(neighbours).__name__}") from None
    for a in (start, nbr):
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"neighbours: expected integer indices, got {a.dtype}")
    return start.astype(np.int64), nbr.astype(np.int64)


def check_fuse_args(n_views, width, height, K, ext, neighbours, px_tol=1.0, rel_tol=0.01, min_views=2, transform=None, dtype=np.float32):
    """The checks of pcs_fuse_set_views, pcs_fuse_set_neighbours and pcs_fuse_run on the host; the ValueError names the argument.
    -> (K (V, 4), P (V, 12), nbr_start int32, nbr int32, px_tol, rel_tol, min_views, T (12,) or None, f32)."""
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
    if P is None:
        raise ValueError(f"ext: expected ({n_views}, 3, 4) world -> view")
    start, nbr = _csr(neighbours, n_views)
    if start[0] != 0 or len(nbr) != start[-1] or np.any(np.diff(start) < 0):
        raise ValueError("neighbours: nbr_start must run from 0 to len(nbr) and never decrease")
    for v in range(n_views):
        l = nbr[start[v]:start[v + 1]]
        if len(l) > FUSE_MAX_NEIGHBOURS:
            raise ValueError(f"neighbours: view {v} has {len(l)} neighbours, more than {FUSE_MAX_NEIGHBOURS}")
        if np.any(l < 0) or np.any(l >= n_views):
            raise ValueError(f"neighbours: view {v} lists an index outside [0, {n_views})")
        if np.any(l == v):
            raise ValueError(f"neighbours: view {v} lists itself")
        if len(np.unique(l)) != len(l):
            raise ValueError(f"neighbours: view {v} lists a view twice")
    for val, name in ((px_tol, "px_tol"), (rel_tol, "rel_tol")):
        if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) or not np.isfinite(val) or not val > 0:
            raise ValueError(f"{name}: expected a finite number > 0, got {val!r}")
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or not 1 <= min_views <= FUSE_MAX_NEIGHBOURS:
        raise ValueError(f"min_views: expected an integer in [1, {FUSE_MAX_NEIGHBOURS}], got {min_views!r}")
    T = None
    if transform is not None:
        T = np.asarray(transform, dtype=np.float64)
        if T.shape == (4, 4):
            T = T[:3]
        if T.shape != (3, 4) or not np.all(np.isfinite(T)):
            raise ValueError(f"transform: expected a finite (3, 4) or (4, 4), got shape {np.shape(transform)}")
        T = np.ascontiguousarray(T).reshape(12)
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    return (np.ascontiguousarray(Ka), P, np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(nbr, dtype=np.int32), float(px_tol), float(rel_tol),
            int(min_views), T, np.dtype(dtype) == np.dtype(np.float32))


class DepthFuser(_Handle):
    """Owner of one ``pcs_depth_fuser`` handle (include/pcs_hip.h): the view table, the neighbour lists and the workspace (the support
    words, the block counts) stay on the device across calls; depth maps and outputs are raw device addresses used in place."""

    _create, _destroy = "pcs_fuse_create", "pcs_fuse_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)

    def set_views(self, width, height, K, P):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 12)
        self._call("pcs_fuse_set_views", self._h, K.shape[0], int(width), int(height), self._ptr(K), self._ptr(P))

    def set_neighbours(self, nbr_start, nbr):
        nbr_start, nbr = np.ascontiguousarray(nbr_start, dtype=np.int32), np.ascontiguousarray(nbr, dtype=np.int32)
        self._call("pcs_fuse_set_neighbours", self._h, self._ptr(nbr_start), self._ptr(nbr) if nbr.size else None, len(nbr_start) - 1)

    def run(self, d_depth, depth_f32, d_points, d_mask, *, px_tol=1.0, rel_tol=0.01, min_views=2, unique=False, T=None, f32=True, d_count=None, d_support=None,
            d_status=None, d_fused_depth=None, fused_f32=True, d_counts=None, stream=None):
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(12)
        self._call("pcs_fuse_run", self._h, self._addr(d_depth), int(bool(depth_f32)), float(px_tol), float(rel_tol), int(min_views), int(bool(unique)), self._ptr(T),
                   self._addr(d_points), int(bool(f32)), self._addr(d_mask), self._addr(d_count), self._addr(d_support), self._addr(d_status), self._addr(d_fused_depth),
                   int(bool(fused_f32)), self._addr(d_counts), _stream_arg(stream))

    def last_kernel_ms(self):
        """-> (check kernel, duplicate kernel (0 without ``unique``), the whole call) in ms."""
        ms = [self._ct.c_float(0.0) for _ in range(3)]
        self._call("pcs_fuse_last_kernel_ms", self._h, *(self._ct.byref(m) for m in ms))
        return tuple(float(m.value) for m in ms)


_fuser_cache: dict = {}


def _fuser(device: int) -> DepthFuser:
    return _cached_handle(_fuser_cache, int(device), lambda: DepthFuser(device))


def fuse_depth_maps(depth, K, ext, neighbours, *, px_tol=1.0, rel_tol=0.01, min_views=2, unique=False, transform=None, values=None, compact=False, dtype=np.float32,
                    return_support=False, return_status=False, return_depth=False, device=None):
    """Keep a depth only where at least ``min_views`` neighbouring views agree with it and merge the agreeing observations into one
    point (the rule of include/pcs_hip.h).  ``depth`` (V, H, W) float32 / float64 z-depths; ``K`` (V, 4) = [fx, cx, fy, cy]; ``ext``
    (V, 3, 4) world -> view; ``neighbours``: a list of index sequences, one per view in the order that counts, or a CSR pair
    (nbr_start (V + 1,), nbr) — at most 32 per view (``view_neighbours`` makes them).  A neighbour agrees when the pixel's surface point,
    seen in the neighbour and taken back with the neighbour's depth, returns within ``px_tol`` pixels and ``rel_tol`` relative depth.
    ``unique``: of the kept pixels that agree with one another only the one of the lowest view stays.  ``transform`` (3, 4): world ->
    the caller's frame, applied to the points.
    -> (points (V, H, W, 3) of ``dtype`` with NaN where the mask is 0, mask uint8, count uint8[, support uint32 (``return_support``)]
    [, status uint8, bits FUSE_* (``return_status``)][, fused_depth (V, H, W) of ``dtype``: the fused point's z in its own view
    (``return_depth``)]).  With ``compact``: a list with one entry per view, the masked points (M_i, 3) in row-major pixel order, or
    (points, values (M_i,)) with ``values`` (V, H, W) uint8."""
    torch = _torch()
    if getattr(depth, "ndim", None) != 3:
        raise ValueError(f"depth: expected (V, H, W), got shape {tuple(getattr(depth, 'shape', ()))}")
    name = str(depth.dtype).replace("torch.", "")
    if name not in ("float32", "float64"):
        raise ValueError(f"depth: expected float32 or float64, got {name}")
    V, H, W = (int(v) for v in depth.shape)
    Ka, P, start, nbr, px_tol, rel_tol, min_views, T, f32 = check_fuse_args(V, W, H, K, ext, neighbours, px_tol, rel_tol, min_views, transform, dtype)
    as_tensor = _is_tensor(depth) and depth.is_cuda
    dev = _device_of(depth, values, device=device)
    dv = None
    if values is not None:
        Vs, _ = _plane_stack(values, "values")
        if tuple(Vs.shape) != (V, H, W):
            raise ValueError(f"values: expected the shape of depth, {(V, H, W)}, got {tuple(values.shape)}")
        dv, pv = _u8_on_device(Vs, "values", dev)
    D = _to_device(depth, getattr(torch, name), dev)
    fz = _fuser(dev)
    fz.set_views(W, H, Ka, P)
    fz.set_neighbours(start, nbr)
    ft = torch.float32 if f32 else torch.float64
    pts = torch.empty((V, H, W, 3), dtype=ft, device=D.device)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=D.device)
    count = torch.empty((V, H, W), dtype=torch.uint8, device=D.device)
    support = torch.empty((V, H, W), dtype=torch.int32, device=D.device) if return_support else None   # the bits of a uint32
    status = torch.empty((V, H, W), dtype=torch.uint8, device=D.device) if return_status else None
    fused = torch.empty((V, H, W), dtype=ft, device=D.device) if return_depth else None
    counts = torch.zeros((V,), dtype=torch.int64, device=D.device) if compact else None
    ptr = lambda t: None if t is None else t.data_ptr()
    fz.run(D.data_ptr(), name == "float32", pts.data_ptr(), mask.data_ptr(), px_tol=px_tol, rel_tol=rel_tol, min_views=min_views, unique=unique, T=T, f32=f32,
           d_count=count.data_ptr(), d_support=ptr(support), d_status=ptr(status), d_fused_depth=ptr(fused), fused_f32=f32, d_counts=ptr(counts), stream=_stream(dev))
    if not compact:
        outs = [pts, mask, count]
        if support is not None:
            outs.append(support if as_tensor else support.cpu().numpy().view(np.uint32))
        outs += [o for o in (status, fused) if o is not None]
        return tuple(o if isinstance(o, np.ndarray) else _result(o, as_tensor) for o in outs)
    out_pts = torch.empty((V * H * W, 3), dtype=ft, device=D.device)
    out_val = torch.empty((V * H * W,), dtype=torch.uint8, device=D.device) if dv is not None else None
    _matcher(dev).compact(V, W, H, pts.data_ptr(), f32, mask.data_ptr(), out_pts.data_ptr(), counts.data_ptr(), d_values=ptr(dv), values_pitch=0 if dv is None else pv,
                          d_out_values=ptr(out_val), stream=_stream(dev))
    ends = np.cumsum(counts.cpu().numpy())
    clouds = []
    for i in range(V):
        a, b = int(ends[i - 1]) if i else 0, int(ends[i])
        p = _result(out_pts[a:b], as_tensor)
        clouds.append(p if out_val is None else (p, _result(out_val[a:b], as_tensor)))
    return clouds


def view_neighbours(ext, min_angle=3.0, max_angle=45.0, max_views=9):
    """Neighbour lists from the viewing directions: the deterministic form of the reference's ``calc_pairs(c_vec, ReconParams(minangle,
    maxangle, max_n_view), pick_closest=True)`` (reconstruction/acmmp_utils.py:47-83).  Host NumPy.  ``ext`` (V, 3, 4) world -> view; the
    viewing direction of such an extrinsic is the third ROW of R, R^T e_z.  The reference's ``cam.view`` (cameras/camera.py:419) is
    ``cam_to_world @ [0, 0, 1, 0]``, the third column of the camera -> world rotation: the same vector.  (``get_v_vec`` (:39-45), the
    third COLUMN of whatever extrinsic it is given, equals it only for a camera -> world matrix.)
    A view j is a candidate of view i when the angle between the two directions, in degrees, lies strictly inside (``min_angle``,
    ``max_angle``).  With fewer than ``max_views`` candidates the list is the candidates in index order, as the reference returns them;
    otherwise the ``max_views`` closest in angle, nearest first, ties broken to the lower index (the reference's ``argsort`` leaves ties
    to chance).  -> a list of V int32 arrays."""
    E = np.asarray(ext, dtype=np.float64)
    if E.ndim != 3 or E.shape[1:] not in ((3, 4), (4, 4)) or not np.all(np.isfinite(E)):
        raise ValueError(f"ext: expected finite (V, 3, 4) world -> view, got shape {np.shape(ext)}")
    if not (np.isfinite(min_angle) and np.isfinite(max_angle) and 0.0 <= min_angle < max_angle):
        raise ValueError(f"min_angle: expected 0 <= min_angle < max_angle, got {min_angle!r}, {max_angle!r}")
    if isinstance(max_views, bool) or not isinstance(max_views, (int, np.integer)) or not 1 <= max_views <= FUSE_MAX_NEIGHBOURS:
        raise ValueError(f"max_views: expected an integer in [1, {FUSE_MAX_NEIGHBOURS}], got {max_views!r}")
    return neighbours_of_directions(E[:, 2, :3], min_angle, max_angle, max_views)


def neighbours_of_directions(view_vectors, min_angle=3.0, max_angle=45.0, max_views=9):
    """``view_neighbours`` on the viewing directions themselves (V, 3), the argument of the reference's ``calc_pairs``."""
    v = np.asarray(view_vectors, dtype=np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(v @ v.T, -1.0, 1.0)))
    out = []
    for i in range(len(v)):
        ok = (ang[i] > min_angle) & (ang[i] < max_angle)
        ok[i] = False
        cand = np.flatnonzero(ok)
        if len(cand) >= max_views:
            cand = cand[np.argsort(ang[i, cand], kind="stable")][:max_views]
        out.append(cand.astype(np.int32))
    return out


def rectified_view(ext_a, R_a, K_new):
    """The pinhole view in which ``disparity_to_points(...)[..., 2]`` of a rectified pair is a z-depth map (NaN where masked): camera
    a's rectified frame.  ``ext_a`` (3, 4) world -> camera a, ``R_a`` (3, 3) camera -> rectified and ``K_new`` = [fx, cx, fy, cy] of
    ``imaging.rectify_pair``.  -> (K (4,), [R_a E_a] (3, 4) world -> rectified)."""
    E = check_ext(ext_a, 1)[0].reshape(3, 4)
    R = np.asarray(R_a, dtype=np.float64)
    Kn = np.asarray(K_new, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or Kn.shape != (4,):
        raise ValueError(f"R_a / K_new: expected (3, 3) and [fx, cx, fy, cy], got {R.shape} and {Kn.shape}")
    return Kn.copy(), R @ E


def fuse_stereo_pairs(images, intr, ext, pairs, num_disp, *, method="block", match_options=None, depth_range=(0.0, 2.0), neighbours=None, alpha: float = 1.0,
                      interpolation: str = "bicubic", px_tol=1.0, rel_tol=0.01, min_views=2, unique=True, transform=None, dtype=np.float32, device=None):
    """One cloud of a rig from several stereo pairs: per pair (a, b) ``rectify_images`` -> ``stereo_match`` -> ``disparity_to_points
    (compact=False)``, whose z in camera a's rectified frame is that pair's depth map; each pair's camera a becomes one fusion view
    (``rectified_view``); then ``fuse_depth_maps(values=rectified a, compact=True)``.  A thin composition: no kernel of its own.
    ``images`` (C, H, W) uint8, one per camera; ``intr`` (C, 9); ``ext`` (C, 3, 4) world -> camera; ``pairs``: (a, b) index pairs.
    ``neighbours`` defaults to ``view_neighbours`` of the fusion views; ``match_options`` go to ``stereo_match`` (``block`` defaults to
    the reference's 25).  The pairs' rectified images must share one size.  -> (points (M, 3) in the world frame, or in ``transform``'s,
    grey values (M,) uint8), the views concatenated in pair order.  ``fuse_stereo_pairs.last`` holds (K, P, neighbours, depth maps,
    per-view counts, per-pair mask sums)."""
    opts = dict(match_options or {})
    min_disp0 = int(opts.pop("min_disp", 0))
    if method == "block" and "block" not in opts:
        opts["block"] = 25
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise ValueError("pairs: expected at least one (a, b)")
    C = int(images.shape[0])
    if any(not (0 <= a < C and 0 <= b < C and a != b) for a, b in pairs):
        raise ValueError(f"pairs: expected index pairs of two different cameras in [0, {C})")
    E = check_ext(ext, C).reshape(C, 3, 4)
    dev = _device_of(images, device=device)
    Ks, Ps, depths, greys, sums = [], [], [], [], []
    for a, b in pairs:
        ra, rb, Q, va, vb = rectify_images(images[a], images[b], intr[a], E[a], intr[b], E[b], alpha, interpolation=interpolation, return_valid=True, device=dev)
        R_a, _, K_new, _ = rectify_images.last
        min_disp = -(min_disp0 + int(num_disp) - 1) if Q[3, 2] < 0 else min_disp0   # as stereo_reconstruct: camera a the right-hand one
        disp = stereo_match(ra, rb, num_disp, min_disp=min_disp, valid=(va, vb), device=dev, method=method, **opts)
        pts, mask = disparity_to_points(disp, Q, depth_range=depth_range, dtype=np.float64, invalid=16 * (min_disp - 1), device=dev)
        if depths and tuple(pts.shape) != tuple(depths[0].shape) + (3,):
            raise ValueError(f"pairs: the rectified images of pair {(a, b)} are {tuple(pts.shape[:2])}, those of pair {pairs[0]} {tuple(depths[0].shape)}")
        Kv, Pv = rectified_view(E[a], R_a, K_new)
        Ks.append(Kv), Ps.append(Pv), depths.append(pts[..., 2]), greys.append(ra.reshape(pts.shape[:2])), sums.append(int(mask.sum()))
    stack = _torch().stack if _is_tensor(depths[0]) else np.stack
    D, G = stack(depths), stack(greys)
    Ks, Ps = np.stack(Ks), np.stack(Ps)
    nb = view_neighbours(Ps) if neighbours is None else neighbours
    clouds = fuse_depth_maps(D, Ks, Ps, nb, px_tol=px_tol, rel_tol=rel_tol, min_views=min_views, unique=unique, transform=transform, values=G, compact=True, dtype=dtype,
                             device=dev)
    cat = _torch().cat if _is_tensor(clouds[0][0]) else np.concatenate
    fuse_stereo_pairs.last = (Ks, Ps, nb, D, [len(c[0]) for c in clouds], sums)
    return cat([c[0] for c in clouds]), cat([c[1] for c in clouds])
