"""Mirror of the legacy cost entry points and of the batched triangulation
(row f4: ``nb_triangulate_full``, ch:609-643, with the grouping of
``CameraSet.multi_cam_triangulate``, cameras/camera_set.py:371-378) of
pyCamSet/optimisation/compiled_helpers.py, evaluated by the HIP engine:

    bundle_adjustment_costfn(dct, im_points, projection_matrixes, intrinsics, dists) -> (2N,)   ch:518-549
    bundle_adj_parrallel_solver(dct (T, L, 5), ...) -> (T, 2L)                                  ch:493-516

Row f5, ``estimate_view_poses``: the per-view target pose the reference gets from cv2.solvePnPGeneric
(calibration_targets/abstract_target.py:345-405) in front of ``calc_initial_params``.
Row f6, ``estimate_intrinsics``: the per-camera intrinsics the reference gets from cv2.calibrateCamera
(``AbstractTarget.initial_calibration``, abstract_target.py:263-343), from planar views in closed form, optionally refined.

The reference calls them with the detection table on every call (template_handler.py:537-543,
:586-592); the table is uploaded once and cached by content.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _capi
from .engine import Engine, _stream_arg

_cache: dict = {}


def _engine_for(dct: np.ndarray, n_imgs: int, n_keys: int, n_cams: int, device: int) -> Engine:
    dct = np.ascontiguousarray(dct, dtype=np.float64)
    key = (dct.shape, hash(dct.tobytes()), n_imgs, n_keys, n_cams, device)
    if key not in _cache:
        _cache.clear()  # one table at a time, like the reference's single closure
        eng = Engine("template", n_cams, n_imgs, n_keys, device=device)
        eng.set_detections_table(dct)
        _cache[key] = eng
    return _cache[key]


def bundle_adjustment_costfn(dct, im_points, projection_matrixes, intrinsics, dists, device: int = 0) -> np.ndarray:
    im = np.ascontiguousarray(im_points, dtype=np.float64)
    n_imgs = im.shape[0]
    n_keys = int(np.prod(im.shape[1:-1]))
    P = np.ascontiguousarray(projection_matrixes, dtype=np.float64)
    eng = _engine_for(dct, n_imgs, n_keys, P.shape[0], device)
    return eng.legacy_cost(im.reshape(n_imgs, n_keys, 3), P, intrinsics, np.asarray(dists, dtype=np.float64).reshape(P.shape[0], 5))


numpy_bundle_adjustment_costfn = bundle_adjustment_costfn


def bundle_adj_parrallel_solver(dct, im_points, projection_matrixes, intrinsics, dists, device: int = 0) -> np.ndarray:
    dct = np.asarray(dct, dtype=np.float64)
    t, l = dct.shape[0], dct.shape[1]
    flat = bundle_adjustment_costfn(dct.reshape(t * l, dct.shape[2]), im_points, projection_matrixes, intrinsics, dists, device)
    return flat.reshape(t, 2 * l)


last_triangulate_kernel_ms = None

# Defaults of the triangulation refinement (include/pcs_hip.h pcs_tri_refine).  max_iter counts LM trials (one pass over a point's
# views each; a DLT start converges in 2-4).  ftol / xtol stop at a relative cost decrease / a step relative to |X| of 1e-10: far below
# the noise of any measurement, and a step that small moves the point by less than its own rounding after one more GN step.
# gtol (max |J'r| <= gtol) is off: J'r carries pixel^2 per world unit, so no absolute threshold suits every rig.
REFINE_DEFAULTS = {"max_iter": 10, "ftol": 1e-10, "xtol": 1e-10, "gtol": 0.0}
# per-point status of the refinement (include/pcs_hip.h PCS_TRI_REFINE_*)
TRI_NOT_REFINED, TRI_CONVERGED, TRI_MAX_ITER, TRI_NO_DECREASE = 0, 1, 2, 3


def check_refine_options(max_iter, ftol, xtol, gtol):
    """Validate the refinement options on the host (ValueError) before anything is queued."""
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 0 <= int(max_iter) < 2 ** 31:
        raise ValueError(f"max_iter must be an integer >= 0, got {max_iter!r}")
    out = [int(max_iter)]
    for name, v in (("ftol", ftol), ("xtol", xtol), ("gtol", gtol)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}") from None
        if not (np.isfinite(f) and f >= 0.0):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        out.append(f)
    return tuple(out)


def check_loss(loss, f_scale):
    """Validate ``loss`` / ``f_scale`` the way ``device_solver.lm_solve`` does (ValueError) -> (name, float(f_scale))."""
    if loss not in _capi.LOSS_IDS:
        raise ValueError(f"unknown loss {loss!r}: expected one of {sorted(_capi.LOSS_IDS)}")
    try:
        fs = float(f_scale)
    except (TypeError, ValueError):
        raise ValueError(f"f_scale must be finite and > 0, got {f_scale!r}") from None
    if not (np.isfinite(fs) and fs > 0.0):
        raise ValueError(f"f_scale must be finite and > 0, got {f_scale}")
    return loss, fs


@dataclass
class TriangulationResult:
    """Refined triangulation (``refine_triangulation``, ``multi_cam_triangulate(return_result=True)``, ``Triangulator.refined``).

    points, points_dlt: (n, 3) refined and DLT points; rms, rms_dlt: (n,) RMS reprojection error sqrt(sum_v |r_v|^2 / n_v) in pixels at
    them (rms <= rms_dlt without a loss); n_views, iterations (LM trials), status (TRI_*): (n,) int32; residuals: (n_obs, 2)
    uv - pi(points) in the observation order, or None; cost: (n,) scipy's 0.5 sum rho0 of the refinement's loss at the points (half
    the sum of squares without one), or None for a result that was not fetched with it.  With the consensus stage (``consensus`` > 0):
    inliers (n_obs,) bool, the rows the points were computed from; n_inliers (n,) int32; consensus_used (n,) bool (False: fewer than
    three views, the plain path); score (n,) the winner's sum min(e^2, inlier_px^2); rms is over the inliers, n_views the full count
    and residuals cover every row.  All four are None when the stage was off."""
    points: np.ndarray
    points_dlt: np.ndarray
    rms: np.ndarray
    rms_dlt: np.ndarray
    n_views: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    residuals: np.ndarray | None = None
    cost: np.ndarray | None = None
    inliers: np.ndarray | None = None
    n_inliers: np.ndarray | None = None
    consensus_used: np.ndarray | None = None
    score: np.ndarray | None = None


TRI_CONSENSUS_MAX = 256   # hypotheses per point that pcs_tri_set_consensus takes


def check_tri_consensus_options(consensus, inlier_px, seed):
    """Validate the consensus options of the triangulation on the host (ValueError) before anything is queued: the checks of
    pcs_tri_set_consensus (``check_consensus_options`` with its own hypothesis limit and no sample size: a sample is a pair of views)."""
    if isinstance(consensus, bool) or not isinstance(consensus, (int, np.integer)) or not 0 <= int(consensus) <= TRI_CONSENSUS_MAX:
        raise ValueError(f"consensus must be an integer in [0, {TRI_CONSENSUS_MAX}], got {consensus!r}")
    _, _, px, sd = check_consensus_options(0, 4, inlier_px, seed)
    return int(consensus), px, sd


def _cached_handle(cache: dict, key, factory):
    """One handle at a time per cache: a new key replaces the old handle."""
    h = cache.get(key)
    if h is None:
        cache.clear()
        h = cache[key] = factory()
    return h


class _Handle:
    """What the owners of a batched C-ABI handle share: creation and destruction through the named entry points, the call-and-check,
    the ``last_*_ms`` getters and the ctypes pointer casts."""
    _create = _destroy = ""

    def __init__(self, device: int, *sizes: int):
        self._capi, self._ct = _capi, ctypes
        self._h = ctypes.c_void_p()
        self._call(self._create, ctypes.byref(self._h), int(device), *(int(n) for n in sizes))

    def _call(self, name: str, *args):
        self._capi.check(getattr(self._capi.lib(), name)(*args))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self._capi.lib(), self._destroy)(self._h)
            self._h = self._ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ms(self, getter: str) -> float:
        ms = self._ct.c_float(0.0)
        self._call(getter, self._h, self._ct.byref(ms))
        return float(ms.value)

    def _ptr(self, a):
        return None if a is None else a.ctypes.data_as(self._ct.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))

    def _addr(self, d):
        return self._ct.c_void_p(d or 0)


class Triangulator(_Handle):
    """Owner of one ``pcs_triangulator`` handle (include/pcs_hip.h): the camera table, device copies of the
    observations, the kernel's scratch and the output live on the device across calls, so repeated
    triangulations with the same cameras (``CameraSet.multi_cam_triangulate`` per set of frames,
    cameras/camera_set.py:343-402) allocate nothing and — with device-resident inputs — copy nothing."""

    _create, _destroy = "pcs_tri_create", "pcs_tri_destroy"

    def __init__(self, n_cams: int, device: int = 0):
        super().__init__(device, n_cams)
        self.n_cams, self.device, self.n_pts = int(n_cams), int(device), 0
        self._cam_key = None
        self._n_obs = 0

    def set_cameras(self, proj, intr, dist):
        P = np.ascontiguousarray(proj, dtype=np.float64)
        K = np.ascontiguousarray(intr, dtype=np.float64)
        D = np.ascontiguousarray(np.asarray(dist, dtype=np.float64).reshape(P.shape[0], -1))
        if P.shape != (self.n_cams, 3, 4) or K.shape != (self.n_cams, 3, 3) or D.shape != (self.n_cams, 5):
            raise ValueError("expected proj (C,3,4), intr (C,3,3), dist (C,5)")
        key = hash(P.tobytes() + K.tobytes() + D.tobytes())
        if key != self._cam_key:   # the same cameras across calls: nothing to upload
            self._call("pcs_tri_set_cameras", self._h, self._ptr(P), self._ptr(K), self._ptr(D))
            self._cam_key = key

    def set_observations(self, cam, uv, start_inds):
        """Host arrays (copied to handle-owned device buffers): cam (n_obs,) int, uv (n_obs, 2), start_inds (n_pts + 1,)."""
        cam = np.ascontiguousarray(cam, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        self._call("pcs_tri_set_observations", self._h, cam.shape[0], self._ptr(cam), self._ptr(uv), start.shape[0] - 1, self._ptr(start))
        self.n_pts = start.shape[0] - 1
        self._n_obs = cam.shape[0]

    def set_observations_device(self, n_obs: int, d_cam: int, d_uv: int, n_pts: int, d_start: int):
        """Raw device addresses (e.g. ``tensor.data_ptr()``) of int32 cam, float64 uv, int64 start_inds: used in place."""
        self._call("pcs_tri_set_observations_device", self._h, int(n_obs), self._addr(d_cam), self._addr(d_uv), int(n_pts), self._addr(d_start))
        self.n_pts = int(n_pts)
        self._n_obs = int(n_obs)

    def group_table_device(self, n: int, d_cam: int, d_feat: int, d_uv: int, n_features: int, stream: int | None = None):
        """The grouping of ``multi_cam_triangulate`` (cameras/camera_set.py:371-378) on the device: raw device addresses of int32
        camera indices, int32 dense feature ids (< ``n_features``) and float64 measurements of ``n`` table rows grouped by feature.
        -> (n_pts, n_kept, grouped); with ``grouped`` the handle's current observations are the rows of the features seen by at least
        two cameras (``run`` next); not grouped: nothing was set (group on the host: ``group_reconstructable``)."""
        ct = self._ct
        n_pts, n_kept, grouped = ct.c_int64(), ct.c_int64(), ct.c_int32()
        self._call("pcs_tri_group_device", self._h, int(n), self._addr(d_cam), self._addr(d_feat), self._addr(d_uv), int(n_features),
                   ct.byref(n_pts), ct.byref(n_kept), ct.byref(grouped), _stream_arg(stream))
        if grouped.value:
            self.n_pts = int(n_pts.value)
            self._n_obs = int(n_kept.value)
        return int(n_pts.value), int(n_kept.value), bool(grouped.value)

    def run(self, d_pts: int | None = None, stream: int | None = None):
        """Queue the kernel (asynchronous).  ``d_pts`` = device address of an (n_pts, 3) float64 buffer, or None for the
        handle-owned output (fetch it with ``points()``)."""
        self._call("pcs_tri_run", self._h, self._addr(d_pts), _stream_arg(stream))

    def launch_config(self) -> tuple:
        """What ``run`` launches for this handle (include/pcs_hip.h pcs_tri_launch_config): (lanes per point, register views per lane —
        0 for the scratch kernel —, 1 for the register kernel, 1 for points visited in order of their view count)."""
        out = (self._ct.c_int32 * 4)()
        self._call("pcs_tri_launch_config", self._h, out)
        return tuple(int(v) for v in out)

    def synchronize(self, stream: int | None = None):
        self._call("pcs_tri_synchronize", self._h, _stream_arg(stream))

    def points(self) -> np.ndarray:
        pts = np.empty((max(self.n_pts, 0), 3))
        if self.n_pts > 0:
            self._call("pcs_tri_points", self._h, self._ptr(pts))
        return pts

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_tri_last_kernel_ms")

    def refine(self, max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"],
               gtol: float = REFINE_DEFAULTS["gtol"], residuals: bool = False, d_pts: int | None = None, d_rms: int | None = None,
               d_info: int | None = None, d_resid: int | None = None, stream: int | None = None):
        """Queue the reprojection-error refinement of the last ``run``'s points (asynchronous, like ``run``; include/pcs_hip.h
        pcs_tri_refine).  Device addresses: ``d_pts`` (n_pts, 3) float64, ``d_rms`` (n_pts, 2) float64 [rms, rms at the DLT point],
        ``d_info`` (n_pts, 3) int32 [trials, status, views], ``d_resid`` (n_obs, 2) float64 (with ``residuals``); None = handle-owned
        (fetch them with ``refined()``)."""
        max_iter, ftol, xtol, gtol = check_refine_options(max_iter, ftol, xtol, gtol)
        self._call("pcs_tri_refine", self._h, max_iter, ftol, xtol, gtol, self._capi.TRI_REFINE_RESIDUALS if residuals else 0,
                   self._addr(d_pts), self._addr(d_rms), self._addr(d_info), self._addr(d_resid), _stream_arg(stream))
        self._refined_residuals = bool(residuals) and not d_resid

    def set_refine_loss(self, loss: str = "linear", f_scale: float = 1.0):
        """The robust loss of ``refine`` (include/pcs_hip.h pcs_tri_set_refine_loss): scipy's 'linear' (the default), 'huber',
        'soft_l1', 'cauchy', 'arctan' on each scalar residual, ``f_scale`` in pixels.  It stays with the handle until it is set again."""
        loss, f_scale = check_loss(loss, f_scale)
        self._call("pcs_tri_set_refine_loss", self._h, self._capi.LOSS_IDS[loss], f_scale)

    def get_refine_loss(self):
        """The current (loss, f_scale) of ``set_refine_loss``."""
        k, fs = self._ct.c_int(), self._ct.c_double()
        self._call("pcs_tri_get_refine_loss", self._h, self._ct.byref(k), self._ct.byref(fs))
        return {v: n for n, v in self._capi.LOSS_IDS.items()}[k.value], fs.value

    def refine_costs(self) -> np.ndarray:
        """Wait for the last ``refine``: (n_pts, 2) scipy's cost 0.5 sum rho0 at the refined point and at the DLT point."""
        cost = np.empty((max(self.n_pts, 0), 2))
        self._call("pcs_tri_refine_costs", self._h, self._ptr(cost))
        return cost

    def refined(self, points_dlt: np.ndarray | None = None) -> "TriangulationResult":
        """Wait for the last ``refine`` and return its handle-owned outputs.  ``points_dlt``: the start points, when the run wrote
        them to a caller buffer (otherwise they are fetched from the handle)."""
        n = max(self.n_pts, 0)
        pts, rms, info = np.empty((n, 3)), np.empty((n, 2)), np.empty((n, 3), dtype=np.int32)
        resid = np.empty((self._n_obs, 2)) if getattr(self, "_refined_residuals", False) else None
        self._call("pcs_tri_refined", self._h, self._ptr(pts), self._ptr(rms), self._ptr(info), self._ptr(resid))
        start = self.points() if points_dlt is None else np.asarray(points_dlt, dtype=np.float64).reshape(n, 3)
        return TriangulationResult(points=pts, points_dlt=start, rms=rms[:, 0].copy(), rms_dlt=rms[:, 1].copy(), n_views=info[:, 2].copy(),
                                   iterations=info[:, 0].copy(), status=info[:, 1].copy(), residuals=resid, cost=self.refine_costs()[:, 0].copy())

    def last_refine_ms(self) -> float:
        return self._ms("pcs_tri_last_refine_ms")

    def set_consensus(self, n_hypotheses: int = 0, inlier_px: float = 8.0, seed: int = 0):
        """The consensus stage of the runs that follow (pcs_tri_set_consensus): ``n_hypotheses`` view pairs per point are triangulated
        and scored on all views of the point, DLT and refinement work on the views within ``inlier_px`` of the best.  0 = off (the
        default).  It stays with the handle until it is set again."""
        self._call("pcs_tri_set_consensus", self._h, *check_tri_consensus_options(n_hypotheses, inlier_px, seed))

    def get_consensus(self):
        """The current (n_hypotheses, inlier_px, seed) of ``set_consensus``."""
        h, px, seed = self._ct.c_int(), self._ct.c_double(), self._ct.c_uint64()
        self._call("pcs_tri_get_consensus", self._h, self._ct.byref(h), self._ct.byref(px), self._ct.byref(seed))
        return h.value, px.value, seed.value

    def consensus_results(self):
        """Wait for the last ``run`` with a consensus stage: (inlier (n_obs,) bool, cinfo (n_pts, 4) int32 = [inliers, winning
        hypothesis, finite hypotheses, consensus used], score (n_pts,))."""
        n = max(self.n_pts, 0)
        inlier, cinfo, score = np.empty(self._n_obs, dtype=np.uint8), np.empty((n, 4), dtype=np.int32), np.empty(n)
        self._call("pcs_tri_consensus_results", self._h, self._ptr(inlier), self._ptr(cinfo), self._ptr(score))
        return inlier.astype(bool), cinfo, score

    def with_consensus(self, res: "TriangulationResult") -> "TriangulationResult":
        """``res`` with what the stage of the last ``run`` found (nothing when that run had none)."""
        if self.get_consensus()[0] > 0:
            inl, cinfo, score = self.consensus_results()
            res.inliers, res.n_inliers, res.consensus_used, res.score = inl, cinfo[:, 0].copy(), cinfo[:, 3] != 0, score
        return res


_tri_cache: dict = {}


def _triangulator(device: int, n_cams: int) -> Triangulator:
    return _cached_handle(_tri_cache, (int(device), int(n_cams)), lambda: Triangulator(n_cams, device))


def nb_triangulate_full(data, proj, start_inds, intr, dist, device: int = 0, *, consensus: int = 0, inlier_px: float = 8.0, seed: int = 0) -> np.ndarray:
    """``data`` rows = [cam, ..., u, v] sorted by point; ``start_inds`` (n_pts + 1) like the reference
    (compiled_helpers.py:609-643).  Returns (n_pts, 3).  A ``Triangulator`` per (device, camera count) is kept
    across calls: camera table and buffers are reused.  ``consensus`` > 0 puts the view-pair consensus in front
    (``Triangulator.set_consensus``; 64 is a good value): the points come from the views within ``inlier_px`` of the best pair."""
    global last_triangulate_kernel_ms
    cons = check_tri_consensus_options(consensus, inlier_px, seed)
    data = np.asarray(data, dtype=np.float64)
    P = np.asarray(proj, dtype=np.float64)
    start = np.asarray(start_inds, dtype=np.int64)
    if start.shape[0] <= 1:
        return np.empty((0, 3))
    tri = _triangulator(device, P.shape[0])
    tri.set_cameras(P, intr, dist)
    tri.set_observations(data[:, 0].astype(np.int32), data[:, -2:], start)
    tri.set_consensus(*cons)   # the handle is shared: every call states its setting
    tri.run()
    pts = tri.points()
    last_triangulate_kernel_ms = tri.last_kernel_ms()
    return pts


def _empty_result(return_residuals: bool) -> TriangulationResult:
    z, i = np.empty((0, 3)), np.empty(0, dtype=np.int32)
    return TriangulationResult(points=z, points_dlt=z.copy(), rms=np.empty(0), rms_dlt=np.empty(0), n_views=i, iterations=i.copy(), status=i.copy(),
                               residuals=np.empty((0, 2)) if return_residuals else None, cost=np.empty(0))


def refine_triangulation(data, proj, start_inds, intr, dist, *, max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"],
                         xtol: float = REFINE_DEFAULTS["xtol"], gtol: float = REFINE_DEFAULTS["gtol"], return_residuals: bool = False,
                         device: int = 0, loss: str = "linear", f_scale: float = 1.0, consensus: int = 0, inlier_px: float = 8.0,
                         seed: int = 0) -> TriangulationResult:
    """``nb_triangulate_full`` followed by the per-point refinement of the reprojection error in the measured (distorted) pixels
    (include/pcs_hip.h pcs_tri_refine): DLT and refinement are queued back to back on the device, one synchronisation at the end.
    ``data`` rows = [cam, ..., u, v] sorted by point, ``start_inds`` (n_pts + 1).  Returns a ``TriangulationResult``; with
    ``return_residuals`` its ``residuals`` are (n_obs, 2) in the rows' order.  ``loss`` / ``f_scale``: a robust loss on each scalar
    residual (``Triangulator.set_refine_loss``); the DLT start is the plain one, ``rms`` stays the plain pixel RMS and ``residuals`` the
    raw ones (``diagnostics.robust_weights`` lists what was down-weighted).  ``consensus`` > 0 (64 is a good value) puts the view-pair
    consensus in front of the DLT (``Triangulator.set_consensus``, with ``inlier_px`` and ``seed``): a loss only helps while the start
    is in the right basin, the stage keeps a mismatched view out of the start.  The result then carries ``inliers``, ``n_inliers``,
    ``consensus_used`` and ``score``; two calls agree bit for bit, and a table without outliers gives the bits of ``consensus=0``."""
    global last_triangulate_kernel_ms
    opts = check_refine_options(max_iter, ftol, xtol, gtol)
    loss, f_scale = check_loss(loss, f_scale)
    cons = check_tri_consensus_options(consensus, inlier_px, seed)
    data = np.asarray(data, dtype=np.float64)
    P = np.asarray(proj, dtype=np.float64)
    start = np.asarray(start_inds, dtype=np.int64)
    if data.ndim != 2 or data.shape[1] < 3 or start.ndim != 1 or start.shape[0] < 1:
        raise ValueError("expected data (n_obs, >= 3) and start_inds (n_pts + 1,)")
    if start.shape[0] <= 1:
        return _empty_result(return_residuals)
    tri = _triangulator(device, P.shape[0])
    tri.set_cameras(P, intr, dist)
    tri.set_observations(data[:, 0].astype(np.int32), data[:, -2:], start)
    tri.set_consensus(*cons)             # the handle is shared between calls: every call states its setting
    tri.run()
    tri.set_refine_loss(loss, f_scale)   # ... and its loss
    tri.refine(*opts, residuals=return_residuals)
    res = tri.with_consensus(tri.refined())
    last_triangulate_kernel_ms = tri.last_kernel_ms()
    return res


def multi_cam_triangulate(data, proj, intr, dist, distort: bool = True, device: int = 0, *, refine: bool = False, return_result: bool = False,
                          max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"],
                          gtol: float = REFINE_DEFAULTS["gtol"], return_residuals: bool = False, loss: str = "linear", f_scale: float = 1.0,
                          consensus: int = 0, inlier_px: float = 8.0, seed: int = 0):
    """``CameraSet.multi_cam_triangulate`` for a detection table (cameras/camera_set.py:343-402, the array branch): ``data`` rows =
    [cam, image, key..., u, v] as ``TargetDetection.get_data`` returns them; the features seen by more than one camera are
    triangulated, in order of first appearance.  Grouping (``np.unique`` twice in the reference: 0.37 s for 1e6 rows) AND
    triangulation run on the device; a table whose features are not stored consecutively takes the host grouping
    (``group_reconstructable``: the reference's semantics for any table).  ``distort=False`` zeroes the distortion (camera_set.py:384-385).

    ``refine=True``: the DLT points are refined to the minimum of the reprojection error (``refine_triangulation``; options max_iter,
    ftol, xtol, gtol), grouping, DLT and refinement queued back to back, one synchronisation at the end.  ``return_result=True``
    returns the ``TriangulationResult`` (points, RMS errors, status, with ``return_residuals`` the residuals in the order of the kept
    rows) instead of the points; without ``refine`` it carries the DLT points and their RMS (a refinement with max_iter = 0).  The
    default returns the DLT points, as before.  ``loss`` / ``f_scale``: the robust loss of the refinement (``refine_triangulation``).
    ``consensus`` / ``inlier_px`` / ``seed``: the view-pair consensus in front of the DLT (``refine_triangulation``), on both grouping
    paths; the result carries its ``inliers`` (in the order of the kept rows), ``n_inliers``, ``consensus_used`` and ``score``."""
    global last_triangulate_kernel_ms
    loss, f_scale = check_loss(loss, f_scale)
    cons = check_tri_consensus_options(consensus, inlier_px, seed)
    with_result = refine or return_result
    if with_result:
        opts = check_refine_options(max_iter if refine else 0, ftol, xtol, gtol)
    table = np.asarray(data, dtype=np.float64)
    P = np.asarray(proj, dtype=np.float64)
    D = np.zeros_like(np.asarray(dist, dtype=np.float64)) if not distort else np.asarray(dist, dtype=np.float64)

    def out(res: TriangulationResult):
        return res if return_result else res.points

    empty = (lambda: out(_empty_result(return_residuals))) if with_result else (lambda: np.empty((0, 3)))
    if table.shape[0] == 0:
        return empty()
    tri, n_pts = _group_on_device(table, P, intr, D, device)
    if tri is None:                                                         # host grouping
        rec, start = group_reconstructable(table)
        if not with_result:
            return nb_triangulate_full(rec, P, start, intr, D, device=device, consensus=cons[0], inlier_px=cons[1], seed=cons[2])
        return out(refine_triangulation(rec, P, start, intr, D, max_iter=opts[0], ftol=opts[1], xtol=opts[2], gtol=opts[3],
                                        return_residuals=return_residuals, device=device, loss=loss, f_scale=f_scale, consensus=cons[0],
                                        inlier_px=cons[1], seed=cons[2]))
    if n_pts == 0:
        return empty()
    tri.set_consensus(*cons)   # the handle is shared: every call states its setting
    tri.run()
    if not with_result:
        pts = tri.points()
        last_triangulate_kernel_ms = tri.last_kernel_ms()
        return pts
    tri.set_refine_loss(loss, f_scale)
    tri.refine(*opts, residuals=return_residuals)
    res = tri.with_consensus(tri.refined())
    last_triangulate_kernel_ms = tri.last_kernel_ms()
    return out(res)


def _group_on_device(table: np.ndarray, P: np.ndarray, intr, D: np.ndarray, device: int):
    """The grouping of ``multi_cam_triangulate`` on the device for a non-empty table: (the cached Triangulator holding the kept rows,
    n_pts), or (None, 0) when the table needs the host grouping."""
    import torch

    ids = table[:, 1:-2].astype(np.int64)                                   # (image, key...) columns
    dims = ids.max(axis=0) + 1
    n_features = int(np.prod(dims))
    if n_features >= 2 ** 31 or ids.min() < 0:
        return None, 0
    feat = np.ravel_multi_index(ids.T, dims).astype(np.int32)               # a dense id per feature: no sort needed
    tri = _triangulator(device, P.shape[0])
    tri.set_cameras(P, intr, D)
    dev = torch.device("cuda", device)
    d_cam = torch.from_numpy(table[:, 0].astype(np.int32)).to(dev)
    d_feat = torch.from_numpy(feat).to(dev)
    d_uv = torch.from_numpy(np.ascontiguousarray(table[:, -2:])).to(dev)
    torch.cuda.synchronize(dev)                                             # the uploads ran on torch's stream, the grouping runs on the handle's
    n_pts, _, grouped = tri.group_table_device(table.shape[0], d_cam.data_ptr(), d_feat.data_ptr(), d_uv.data_ptr(), n_features)
    return (tri, n_pts) if grouped else (None, 0)


def group_reconstructable(data: np.ndarray):
    """The grouping CameraSet.multi_cam_triangulate does before calling nb_triangulate_full
    (cameras/camera_set.py:371-378): keep (image, key) groups seen by more than one camera, in the
    table's order, and return (reconstructable_data, start_ind)."""
    table = np.asarray(data, dtype=np.float64)
    if table.shape[0] == 0:
        return table, np.zeros(1, dtype=np.int64)
    # one id per (image, key...) feature; how many cameras saw it; where it first appears in the table
    _, feature = np.unique(table[:, 1:-2], axis=0, return_inverse=True)
    feature = feature.reshape(-1)
    seen_by = np.bincount(feature)
    keep = seen_by[feature] >= 2                    # one view cannot be triangulated
    kept = table[keep]
    kept_feature = feature[keep]
    first_row = np.full(seen_by.shape[0], kept.shape[0], dtype=np.int64)
    np.minimum.at(first_row, kept_feature, np.arange(kept.shape[0]))
    in_table_order = np.argsort(first_row[seen_by >= 2], kind="stable")
    sizes = seen_by[seen_by >= 2][in_table_order]
    starts = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    np.cumsum(sizes, out=starts[1:])
    return kept, starts


# ---- batched target-pose estimation (row f5: the PnP in front of calc_initial_params) -------------------------------------------------
# per-view status of the pose estimation (include/pcs_hip.h PCS_PNP_*)
PNP_NOT_ESTIMATED, PNP_CONVERGED, PNP_MAX_ITER, PNP_NO_DECREASE = 0, 1, 2, 3
last_pnp_kernel_ms = None


@dataclass
class ViewPoses:
    """Target poses per (camera, image) view (``estimate_view_poses``): ``poses`` (C, I, 6) = [rotvec, t] with
    X_cam = R(rotvec) X_target + t, |rotvec| <= pi; ``poses_init`` the linear start, ``poses_alt`` the second start of a planar view (NaN
    for 3-D views); ``rms`` / ``rms_init`` (C, I) RMS reprojection error in pixels at the pose / at the start (rms <= rms_init);
    ``status`` (PNP_*), ``iterations`` (LM trials), ``n_points`` (C, I) int32; ``residuals`` (N, 2) uv - projection in the table's row
    order, or None.  Views without detections or with fewer than ``min_points``: NaN, status 0 (the reference's mode="nan")."""
    poses: np.ndarray
    poses_init: np.ndarray
    poses_alt: np.ndarray
    rms: np.ndarray
    rms_init: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    n_points: np.ndarray
    residuals: np.ndarray | None = None
    inliers: np.ndarray | None = None
    n_inliers: np.ndarray | None = None
    hypothesis: np.ndarray | None = None


def check_consensus_options(consensus, sample_size, inlier_px, seed):
    """Validate the consensus options on the host (ValueError) before anything is queued: the checks of pcs_pnp_set_consensus."""
    for name, v, lo, hi in (("consensus", consensus, 0, 4096), ("sample_size", sample_size, 4, 16), ("seed", seed, 0, 2 ** 64 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    try:
        px = float(inlier_px)
    except (TypeError, ValueError):
        raise ValueError(f"inlier_px must be a finite number > 0, got {inlier_px!r}") from None
    if not (np.isfinite(px) and px > 0.0):
        raise ValueError(f"inlier_px must be a finite number > 0, got {inlier_px!r}")
    return int(consensus), int(sample_size), px, int(seed)


class PoseEstimator(_Handle):
    """Owner of one ``pcs_pose_estimator`` handle (include/pcs_hip.h): camera table, template, observation copies and outputs stay on
    the device across calls."""

    _create, _destroy = "pcs_pnp_create", "pcs_pnp_destroy"

    def __init__(self, n_cams: int, n_keys: int, device: int = 0):
        super().__init__(device, n_cams, n_keys)
        self.n_cams, self.n_keys, self.device = int(n_cams), int(n_keys), int(device)
        self.n_views, self.n_obs = 0, 0
        self._residuals = False

    def set_cameras(self, intr):
        K = np.ascontiguousarray(intr, dtype=np.float64)
        if K.shape != (self.n_cams, 9):
            raise ValueError(f"expected intr ({self.n_cams}, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]")
        self._call("pcs_pnp_set_cameras", self._h, self._ptr(K))

    def set_template(self, points):
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        if pts.shape[0] != self.n_keys:
            raise ValueError(f"expected {self.n_keys} template points")
        self._call("pcs_pnp_set_template", self._h, self._ptr(pts))

    def set_observations(self, key, uv, start_inds, view_cam):
        """Host arrays sorted by view: key (n_obs,) int, uv (n_obs, 2), start_inds (n_views + 1,), view_cam (n_views,) int."""
        key = np.ascontiguousarray(key, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        vcam = np.ascontiguousarray(view_cam, dtype=np.int32)
        if start.ndim != 1 or start.shape[0] < 1 or vcam.shape != (start.shape[0] - 1,) or uv.shape != (key.shape[0], 2):
            raise ValueError("expected key (n_obs,), uv (n_obs, 2), start_inds (n_views + 1,), view_cam (n_views,)")
        self._call("pcs_pnp_set_observations", self._h, key.shape[0], self._ptr(key), self._ptr(uv), start.shape[0] - 1, self._ptr(start), self._ptr(vcam))
        self.n_views, self.n_obs = start.shape[0] - 1, key.shape[0]

    def run(self, max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"],
            gtol: float = REFINE_DEFAULTS["gtol"], min_points: int = 6, residuals: bool = False, stream: int | None = None):
        """Queue the start and LM kernels (asynchronous; handle-owned outputs, fetched with ``results()``)."""
        max_iter, ftol, xtol, gtol = check_refine_options(max_iter, ftol, xtol, gtol)
        min_points = check_min_points(min_points)
        self._call("pcs_pnp_run", self._h, max_iter, ftol, xtol, gtol, min_points, self._capi.PNP_RESIDUALS if residuals else 0,
                   None, None, None, None, None, None, _stream_arg(stream))
        self._residuals = bool(residuals)

    def results(self):
        """Wait for the last ``run``: (pose (n_views, 6), pose_init, pose_alt, rms (n_views, 2), info (n_views, 3) int32, residuals or None)."""
        n = self.n_views
        pose, init, alt, rms, info = np.empty((n, 6)), np.empty((n, 6)), np.empty((n, 6)), np.empty((n, 2)), np.empty((n, 3), dtype=np.int32)
        resid = np.empty((self.n_obs, 2)) if self._residuals else None
        self._call("pcs_pnp_results", self._h, self._ptr(pose), self._ptr(init), self._ptr(alt), self._ptr(rms), self._ptr(info), self._ptr(resid))
        return pose, init, alt, rms, info, resid

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_pnp_last_kernel_ms")

    def set_consensus(self, n_hypotheses: int = 0, sample_size: int = 6, inlier_px: float = 8.0, seed: int = 0):
        """The consensus stage of the runs that follow (pcs_pnp_set_consensus: cv2.solvePnPRansac's iterationsCount, minimal sample,
        reprojectionError and seed); ``n_hypotheses = 0`` turns it off."""
        self._call("pcs_pnp_set_consensus", self._h, *check_consensus_options(n_hypotheses, sample_size, inlier_px, seed))

    def get_consensus(self):
        """(n_hypotheses, sample_size, inlier_px, seed) in force."""
        h, s, px, seed = self._ct.c_int(0), self._ct.c_int(0), self._ct.c_double(0.0), self._ct.c_uint64(0)
        self._call("pcs_pnp_get_consensus", self._h, self._ct.byref(h), self._ct.byref(s), self._ct.byref(px), self._ct.byref(seed))
        return int(h.value), int(s.value), float(px.value), int(seed.value)

    def consensus_results(self):
        """Wait for the last ``run`` with a consensus stage: (inlier (n_obs,) bool, cinfo (n_views, 4) int32 = [inliers, winning
        hypothesis, finite hypotheses, consensus used], score (n_views,))."""
        inlier, cinfo, score = np.zeros(self.n_obs, dtype=np.uint8), np.zeros((self.n_views, 4), dtype=np.int32), np.empty(self.n_views)
        self._call("pcs_pnp_consensus_results", self._h, self._ptr(inlier), self._ptr(cinfo), self._ptr(score))
        return inlier.astype(bool), cinfo, score


def check_min_points(min_points) -> int:
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 1 <= int(min_points) < 2 ** 31:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points!r}")
    return int(min_points)


def group_by_view(dct, n_imgs: int):
    """The host grouping of ``estimate_view_poses``: one stable sort on (cam * n_imgs + im, key), skipped when the table is already
    ordered.  The key takes part so that a view's observations reach the device in one order whatever the order of the table: the
    same table shuffled gives the same bits.  -> (order or None, view ids (n_views,), start (n_views + 1,))."""
    d = np.asarray(dct, dtype=np.float64)
    vid = d[:, 0].astype(np.int64) * int(n_imgs) + d[:, 1].astype(np.int64)
    key = d[:, 2].astype(np.int64)
    span = int(key.max()) + 1 if key.shape[0] else 1
    rank = vid * span + key if key.shape[0] and key.min() >= 0 else vid   # keys out of range are refused by the handle later
    order = None
    if rank.shape[0] > 1 and np.any(rank[1:] < rank[:-1]):
        order = np.argsort(rank, kind="stable")
        vid = vid[order]
    head = np.ones(vid.shape[0], dtype=bool)
    head[1:] = vid[1:] != vid[:-1]
    first = np.nonzero(head)[0]
    return order, vid[first], np.concatenate([first, [vid.shape[0]]]).astype(np.int64)


_pnp_cache: dict = {}


def _pose_estimator(device: int, n_cams: int, n_keys: int) -> PoseEstimator:
    return _cached_handle(_pnp_cache, (int(device), int(n_cams), int(n_keys)), lambda: PoseEstimator(n_cams, n_keys, device))


def estimate_view_poses(dct, points, intr, *, n_imgs: int | None = None, min_points: int = 6, max_iter: int = REFINE_DEFAULTS["max_iter"],
                        ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"], gtol: float = REFINE_DEFAULTS["gtol"],
                        return_residuals: bool = False, device: int = 0, consensus: int = 0, sample_size: int = 6, inlier_px: float = 8.0,
                        seed: int = 0) -> ViewPoses:
    """The pose of the known target in every (camera, image) view, on the device (include/pcs_hip.h pcs_pnp_run): what the reference's
    ``target_pose_in_cam_image`` (calibration_targets/abstract_target.py:345-405, cv2.solvePnPGeneric and the solution of lowest error)
    gives ``estimate_camera_relative_poses`` (optimisation/template_handler.py:484-491) per camera and image.

    ``dct``: the flattened (N, 5) table [cam, im, key, u, v] in any order; ``points``: the template (K, 3) (or ``target.point_data``);
    ``intr``: (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2]; ``n_imgs``: images of the result (default: largest image index + 1).

    ``consensus`` > 0 puts consensus sampling in front (pcs_pnp_set_consensus; cv2.solvePnPRansac in place of cv2.solvePnPGeneric):
    that many hypotheses per view, each the linear start of ``sample_size`` random detections, are scored on all detections of the view
    by sum min(e^2, inlier_px^2); start and LM then use the detections within ``inlier_px`` of the best one, and the result gains
    ``inliers``, ``n_inliers`` and ``hypothesis``.  A detection with a wrong id (tens to hundreds of pixels off) then no longer bends
    its view.  Where the defaults come from: 8 px is OpenCV's ``solvePnPRansac`` default ``reprojectionError``; 6 is the fewest points the
    3-D DLT takes and the default of ``min_points``; a good value of ``consensus`` is 64, log(1 - 0.999) / log(1 - 0.7^6) = 55 rounded up:
    three nines of confidence at 30 % outliers.  ``seed`` keys the counter-based sampler; the hypothesis count is fixed (no early
    exit), so two calls agree bit for bit, and a table without outliers gives the bits of ``consensus=0``.  The cached handle is
    shared: every call states its setting."""
    global last_pnp_kernel_ms
    opts = check_refine_options(max_iter, ftol, xtol, gtol)
    min_points = check_min_points(min_points)
    cons = check_consensus_options(consensus, sample_size, inlier_px, seed)
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    K = np.asarray(intr, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 5 or K.ndim != 2 or K.shape[1] != 9:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v] and intr (C, 9)")
    C = K.shape[0]
    if n_imgs is None:
        n_imgs = int(d[:, 1].max()) + 1 if d.shape[0] else 0
    I = int(n_imgs)
    if d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 1].min() < 0 or d[:, 1].max() >= I):
        raise ValueError("camera or image index of the table outside the intrinsics / n_imgs")
    out = ViewPoses(poses=np.full((C, I, 6), np.nan), poses_init=np.full((C, I, 6), np.nan), poses_alt=np.full((C, I, 6), np.nan),
                    rms=np.full((C, I), np.nan), rms_init=np.full((C, I), np.nan), status=np.zeros((C, I), dtype=np.int32),
                    iterations=np.zeros((C, I), dtype=np.int32), n_points=np.zeros((C, I), dtype=np.int32),
                    residuals=np.empty((d.shape[0], 2)) if return_residuals else None)
    if cons[0] > 0:
        out.inliers = np.zeros(d.shape[0], dtype=bool)
        out.n_inliers, out.hypothesis = np.zeros((C, I), dtype=np.int32), np.full((C, I), -1, dtype=np.int32)
    if d.shape[0] == 0:
        return out
    order, ids, start = group_by_view(d, I)
    ds = d if order is None else d[order]
    est = _pose_estimator(device, C, pts.shape[0])
    est.set_cameras(K)
    est.set_template(pts)
    est.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (ids // I).astype(np.int32))
    est.set_consensus(*cons)   # the handle is shared: every call states its setting
    est.run(*opts, min_points=min_points, residuals=return_residuals)
    pose, init, alt, rms, info, resid = est.results()
    last_pnp_kernel_ms = est.last_kernel_ms()
    c, i = ids // I, ids % I
    if cons[0] > 0:
        inl, cinfo, _ = est.consensus_results()
        if order is None:
            out.inliers = inl
        else:
            out.inliers[order] = inl
        out.n_inliers[c, i], out.hypothesis[c, i] = cinfo[:, 0], cinfo[:, 1]
    out.poses[c, i], out.poses_init[c, i], out.poses_alt[c, i] = pose, init, alt
    out.rms[c, i], out.rms_init[c, i] = rms[:, 0], rms[:, 1]
    out.iterations[c, i], out.status[c, i], out.n_points[c, i] = info[:, 0], info[:, 1], info[:, 2]
    if return_residuals:
        if order is None:
            out.residuals = resid
        else:
            out.residuals[order] = resid
    return out


# ---- two-view relative pose by consensus (row f10: the first estimate of a target-free seed) -------------------------------------------
from ._capi import TWOVIEW_DEGENERATE, TWOVIEW_NO_CHEIRALITY, TWOVIEW_OK, TWOVIEW_TOO_FEW  # noqa: E402,F401
last_twoview_kernel_ms = None
TWOVIEW_STAGES = ("undistort", "hypotheses", "scores", "selection", "final")
TWOVIEW_SOLVERS = {"eight-point": 0, "five-point": 1}   # include/pcs_hip.h PCS_TWOVIEW_EIGHT_POINT / PCS_TWOVIEW_FIVE_POINT
TWOVIEW_MAX_REFINE = 50


def check_twoview_solver(solver, refine_iters):
    """Validate the solver options on the host (ValueError): the checks of pcs_twoview_set_solver.  -> (code, refine_iters)."""
    if solver not in TWOVIEW_SOLVERS:
        raise ValueError(f"solver must be one of {sorted(TWOVIEW_SOLVERS)}, got {solver!r}")
    if isinstance(refine_iters, bool) or not isinstance(refine_iters, (int, np.integer)) or not 0 <= int(refine_iters) <= TWOVIEW_MAX_REFINE:
        raise ValueError(f"refine_iters must be an integer in [0, {TWOVIEW_MAX_REFINE}], got {refine_iters!r}")
    return TWOVIEW_SOLVERS[solver], int(refine_iters)


@dataclass
class TwoViewResult:
    """Relative poses of camera pairs (``estimate_two_view``).  ``pairs`` (P, 2) cameras (a, b), a < b; ``T`` (P, 3, 4) = [R | t] with
    X_b = R X_a + t and |t| = 1, NaN unless ``status`` is TWOVIEW_OK; ``n``, ``n_inliers``, ``n_front`` (inliers in front of both
    cameras), ``status`` (TWOVIEW_*), ``hypothesis`` (the winner, -1: none) (P,) int32; ``score`` the winner's sum min(e^2, inlier_px^2),
    ``rms`` the RMS Sampson distance over the inliers in undistorted pixels, ``parallax`` the RMS angle between the two rays of the front
    inliers in radians (P,).  The correspondence table: pair p owns rows ``start[p]:start[p + 1]`` of ``keys``, ``uv_a``, ``uv_b`` and
    ``inliers`` (n_corr,), ascending in the key."""
    pairs: np.ndarray
    T: np.ndarray
    n: np.ndarray
    n_inliers: np.ndarray
    n_front: np.ndarray
    status: np.ndarray
    hypothesis: np.ndarray
    score: np.ndarray
    rms: np.ndarray
    parallax: np.ndarray
    start: np.ndarray
    keys: np.ndarray
    uv_a: np.ndarray
    uv_b: np.ndarray
    inliers: np.ndarray


def check_twoview_options(consensus, inlier_px, seed, min_points, group_lanes=0):
    """Validate the options of the two-view consensus on the host (ValueError) before anything is queued: the checks of
    pcs_twoview_set_consensus and pcs_twoview_run."""
    for name, v, lo, hi in (("consensus", consensus, 1, 256), ("seed", seed, 0, 2 ** 64 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    try:
        px = float(inlier_px)
    except (TypeError, ValueError):
        raise ValueError(f"inlier_px must be a finite number > 0, got {inlier_px!r}") from None
    if not (np.isfinite(px) and px > 0.0):
        raise ValueError(f"inlier_px must be a finite number > 0, got {inlier_px!r}")
    if isinstance(group_lanes, bool) or group_lanes not in (0, 16, 64):
        raise ValueError(f"group_lanes must be 0 (by size), 16 or 64, got {group_lanes!r}")
    return int(consensus), px, int(seed), check_min_points(min_points), int(group_lanes)


class TwoViewEstimator(_Handle):
    """Owner of one ``pcs_two_view`` handle (include/pcs_hip.h): camera table, correspondence copies, stage buffers and outputs stay on
    the device across calls."""

    _create, _destroy = "pcs_twoview_create", "pcs_twoview_destroy"

    def __init__(self, n_cams: int, device: int = 0):
        super().__init__(device, n_cams)
        self.n_cams, self.device = int(n_cams), int(device)
        self.n_pairs, self.n_corr = 0, 0

    def set_cameras(self, intr):
        K = np.ascontiguousarray(intr, dtype=np.float64)
        if K.shape != (self.n_cams, 9):
            raise ValueError(f"expected intr ({self.n_cams}, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]")
        self._call("pcs_twoview_set_cameras", self._h, self._ptr(K))

    def set_correspondences(self, uv_a, uv_b, start_inds, pair_cams):
        """Host arrays sorted by pair: uv_a, uv_b (n_corr, 2) measured pixels, start_inds (n_pairs + 1,), pair_cams (n_pairs, 2) int with
        a < b.  Shapes raise ValueError; values are checked by the handle (PcsError) without touching the device."""
        ua = np.ascontiguousarray(uv_a, dtype=np.float64)
        ub = np.ascontiguousarray(uv_b, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        pc = np.ascontiguousarray(pair_cams, dtype=np.int32)
        if start.ndim != 1 or start.shape[0] < 1 or pc.shape != (start.shape[0] - 1, 2) or ua.ndim != 2 or ua.shape[1] != 2 or ub.shape != ua.shape:
            raise ValueError("expected uv_a, uv_b (n_corr, 2), start_inds (n_pairs + 1,), pair_cams (n_pairs, 2)")
        self._call("pcs_twoview_set_correspondences", self._h, ua.shape[0], self._ptr(ua), self._ptr(ub), start.shape[0] - 1, self._ptr(start), self._ptr(pc))
        self.n_pairs, self.n_corr = start.shape[0] - 1, ua.shape[0]

    def set_consensus(self, n_hypotheses: int = 64, inlier_px: float = 2.0, seed: int = 0):
        """Hypotheses per pair, inlier threshold in undistorted pixels and the seed of the sampler, for the runs that follow."""
        self._call("pcs_twoview_set_consensus", self._h, int(n_hypotheses), float(inlier_px), int(seed))

    def get_consensus(self):
        """(n_hypotheses, inlier_px, seed) in force."""
        h, px, seed = self._ct.c_int(0), self._ct.c_double(0.0), self._ct.c_uint64(0)
        self._call("pcs_twoview_get_consensus", self._h, self._ct.byref(h), self._ct.byref(px), self._ct.byref(seed))
        return int(h.value), float(px.value), int(seed.value)

    def set_solver(self, solver: str = "eight-point", refine_iters: int = 0):
        """The hypothesis solver ("eight-point", or "five-point" for scenes that are mostly one plane) and the number of LM trials that
        refine the final pose on the essential manifold (0: none), for the runs that follow."""
        code, iters = check_twoview_solver(solver, refine_iters)
        self._call("pcs_twoview_set_solver", self._h, code, iters)

    def get_solver(self):
        """(solver name, refine_iters) in force."""
        code, iters = self._ct.c_int(0), self._ct.c_int(0)
        self._call("pcs_twoview_get_solver", self._h, self._ct.byref(code), self._ct.byref(iters))
        return {v: k for k, v in TWOVIEW_SOLVERS.items()}[int(code.value)], int(iters.value)

    def run(self, min_points: int = 16, group_lanes: int = 0, d_T: int | None = None, stream: int | None = None):
        """Queue the five stages (asynchronous; handle-owned outputs, fetched with ``results()``)."""
        self._call("pcs_twoview_run", self._h, int(min_points), int(group_lanes), 0, self._addr(d_T), _stream_arg(stream))
        self._own_T = d_T is None

    def results(self):
        """Wait for the last ``run``: (T (n_pairs, 3, 4) or None when the run wrote it to a caller buffer, info (n_pairs, 5) int32 =
        [n, inliers, front, status, winning hypothesis], stats (n_pairs, 3) = [score, rms, parallax], inlier (n_corr,) bool)."""
        n = self.n_pairs
        T = np.empty((n, 3, 4)) if getattr(self, "_own_T", True) else None
        info, stats, inl = np.empty((n, 5), dtype=np.int32), np.empty((n, 3)), np.zeros(self.n_corr, dtype=np.uint8)
        self._call("pcs_twoview_results", self._h, self._ptr(T), self._ptr(info), self._ptr(stats), self._ptr(inl))
        return T, info, stats, inl.astype(bool)

    def last_kernel_ms(self) -> dict:
        """Device time of every stage of the last run, milliseconds by stage name (TWOVIEW_STAGES)."""
        ms = (self._ct.c_float * len(TWOVIEW_STAGES))()
        self._call("pcs_twoview_last_kernel_ms", self._h, ms)
        return dict(zip(TWOVIEW_STAGES, (float(v) for v in ms)))


def shared_keys(dct, n_cams: int):
    """Per camera the pixel of every key it sees, that of the lowest image where a camera sees a key in several:
    (keys (n,) ascending, uv (n, 2)) per camera."""
    d = np.asarray(dct, dtype=np.float64)
    out = []
    for c in range(int(n_cams)):
        rows = d[d[:, 0] == c]
        rows = rows[np.lexsort((rows[:, 1], rows[:, 2]))]   # by key, then image
        first = np.ones(rows.shape[0], dtype=bool)
        first[1:] = rows[1:, 2] != rows[:-1, 2]
        out.append((rows[first, 2].astype(np.int64), rows[first, 3:5]))
    return out


_twoview_cache: dict = {}


def _twoview_estimator(device: int, n_cams: int) -> TwoViewEstimator:
    return _cached_handle(_twoview_cache, (int(device), int(n_cams)), lambda: TwoViewEstimator(n_cams, device))


def estimate_two_view(dct, intr, *, pairs=None, consensus: int = 64, inlier_px: float = 2.0, seed: int = 0, min_points: int = 16,
                      group_lanes: int = 0, device: int = 0, solver: str = "eight-point", refine_iters: int = 0) -> TwoViewResult:
    """The relative pose of camera pairs from their shared image points alone, on the device (include/pcs_hip.h pcs_twoview_run): what
    cv2.findEssentialMat(..., RANSAC) + cv2.recoverPose give on the host, and the first step of a target-free seed (``seed_scene``).

    ``dct``: the flat (N, 5) table [cam, im, key, u, v] in any order — a point is a key, two cameras correspond where both see it, and
    a camera that sees a key in several images contributes the lowest; ``intr``: (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2];
    ``pairs``: (P, 2) cameras with a < b (default: every pair with at least ``min_points`` shared keys).  ``consensus`` hypotheses of
    eight correspondences each (64: log(1 - 0.999) / log(1 - 0.75^8) = 66 draws give three nines at 25 % wrong matches) are scored by
    sum min(e^2, inlier_px^2) of the Sampson distance in undistorted pixels; the winner's inliers are refitted.  The hypothesis
    count is fixed and the sampler counter-based (``seed``): two calls agree bit for bit.  A pair with fewer than max(8, min_points)
    correspondences, a degenerate one (coplanar points, no baseline) or one without a point in front of both cameras keeps NaN in
    ``T``; ``status``, ``n_front`` and ``parallax`` say why.

    ``solver="five-point"`` is for scenes that are (mostly) one plane — boards, walls, floors — where the eight-point method degenerates:
    every hypothesis is Nister's five-point solver on five rows, scored with a cheirality term over its four (R, +-t), and the winner's
    pose is the model (TOO_FEW below max(5, min_points) rows, DEGENERATE below 6 inliers).  ``refine_iters`` > 0, with either solver,
    refines the final pose by that many LM trials at most over the Sampson residuals of the inliers, on the essential manifold."""
    global last_twoview_kernel_ms
    H, px, seed, min_points, lanes = check_twoview_options(consensus, inlier_px, seed, min_points, group_lanes)
    check_twoview_solver(solver, refine_iters)
    d = np.asarray(dct, dtype=np.float64)
    K = np.asarray(intr, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 5 or K.ndim != 2 or K.shape[1] != 9 or K.shape[0] < 2:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v] and intr (C, 9) of at least two cameras")
    C = K.shape[0]
    if not np.all(np.isfinite(d)) or not np.all(np.isfinite(K)):
        raise ValueError("dct and intr must be finite")
    if d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 2].min() < 0):
        raise ValueError("camera index of the table outside the intrinsics, or a negative key")
    seen = shared_keys(d, C)
    if pairs is None:
        pc = np.array([(a, b) for a in range(C) for b in range(a + 1, C)
                       if np.intersect1d(seen[a][0], seen[b][0], assume_unique=True).shape[0] >= min_points], dtype=np.int32).reshape(-1, 2)
    else:
        pc = np.asarray(pairs)
        if pc.ndim != 2 or pc.shape[1] != 2 or not np.issubdtype(pc.dtype, np.integer):
            raise ValueError("pairs must be an integer array (P, 2)")
        if pc.shape[0] and (pc.min() < 0 or pc.max() >= C or np.any(pc[:, 0] >= pc[:, 1])):
            raise ValueError(f"pairs must hold cameras in [0, {C}) with a < b")
        pc = pc.astype(np.int32)
    keys, ua, ub, start = [], [], [], [0]
    for a, b in pc:
        common, ia, ib = np.intersect1d(seen[a][0], seen[b][0], assume_unique=True, return_indices=True)
        keys.append(common)
        ua.append(seen[a][1][ia])
        ub.append(seen[b][1][ib])
        start.append(start[-1] + common.shape[0])
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    ua = np.concatenate(ua).reshape(-1, 2) if ua else np.zeros((0, 2))
    ub = np.concatenate(ub).reshape(-1, 2) if ub else np.zeros((0, 2))
    start = np.array(start, dtype=np.int64)
    est = _twoview_estimator(device, C)
    est.set_cameras(K)
    est.set_correspondences(ua, ub, start, pc)
    est.set_consensus(H, px, seed)   # the handle is shared: every call states its setting
    est.set_solver(solver, refine_iters)
    est.run(min_points=min_points, group_lanes=lanes)
    T, info, stats, inl = est.results()
    last_twoview_kernel_ms = est.last_kernel_ms() if pc.shape[0] else None
    return TwoViewResult(pairs=pc, T=T, n=info[:, 0], n_inliers=info[:, 1], n_front=info[:, 2], status=info[:, 3], hypothesis=info[:, 4],
                         score=stats[:, 0], rms=stats[:, 1], parallax=stats[:, 2], start=start, keys=keys, uv_a=ua, uv_b=ub, inliers=inl)


# ---- intrinsics from planar views (row f6: the rough intrinsics calc_initial_params starts from) -------------------------------------
# per-camera and per-group status of the estimate (include/pcs_hip.h PCS_INTR_*, PCS_INTR_GROUP_*)
from ._capi import (INTR_FOCAL, INTR_FOCAL_FALLBACK, INTR_FULL, INTR_GROUP_FIT_FAILED, INTR_GROUP_NOT_FINITE,  # noqa: E402,F401
                    INTR_GROUP_NOT_PLANAR, INTR_GROUP_TOO_FEW, INTR_GROUP_USED, INTR_NOT_ESTIMATED)
last_intrinsics_kernel_ms = None


@dataclass
class IntrinsicsEstimate:
    """Intrinsics per camera from planar target views (``estimate_intrinsics``).  ``intr`` (C, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]
    (the closed form has zero distortion; NaN rows where ``status`` is INTR_NOT_ESTIMATED); ``status`` (INTR_*), ``n_groups`` (groups
    used) (C,) int32; ``eig_ratio`` (C,) smallest / second smallest eigenvalue of the constraint matrix (near 1: the views do not
    constrain the model).  Per (camera, image, board) group: ``homographies`` (G, 3, 3) pixels <- metric plane frame, ``plane_frames``
    (G, 9) = [centroid, e1, e2] of that frame in template coordinates, ``group_status`` (INTR_GROUP_*), ``group_counts``,
    ``group_index`` (G, 3) = [cam, im, board].  With ``refine=True``: ``intr_init`` the closed form, ``intr`` the refined rows,
    ``rms_init`` / ``rms`` (C,) RMS reprojection error in pixels before and after, ``lm`` the ``DeviceLMResult``.  With the consensus
    stage (``consensus`` > 0): ``inliers`` (N,) bool in the order of the caller's table, the rows the homographies (and the refinement)
    were computed from; per group ``group_inliers`` (G,) int32, ``group_hypothesis`` (G,) int32 the winning hypothesis (-1: none),
    ``group_consensus_used`` (G,) bool (False: fewer observations than max(sample_size, min_points), the plain path) and
    ``group_score`` (G,) the winner's sum min(e^2, inlier_px^2) (+inf: no finite hypothesis, NaN: not used); ``group_counts`` stays the
    observation count.  All five are None without the stage."""
    intr: np.ndarray
    status: np.ndarray
    n_groups: np.ndarray
    eig_ratio: np.ndarray
    homographies: np.ndarray
    plane_frames: np.ndarray
    group_status: np.ndarray
    group_counts: np.ndarray
    group_index: np.ndarray
    intr_init: np.ndarray | None = None
    rms_init: np.ndarray | None = None
    rms: np.ndarray | None = None
    lm: object | None = None
    inliers: np.ndarray | None = None
    group_inliers: np.ndarray | None = None
    group_hypothesis: np.ndarray | None = None
    group_consensus_used: np.ndarray | None = None
    group_score: np.ndarray | None = None


class IntrinsicsEstimator(_Handle):
    """Owner of one ``pcs_intrinsics_estimator`` handle (include/pcs_hip.h): template, observation copies and outputs stay on the
    device across calls."""

    _create, _destroy = "pcs_intr_create", "pcs_intr_destroy"

    def __init__(self, n_cams: int, n_keys: int, device: int = 0):
        super().__init__(device, n_cams, n_keys)
        self.n_cams, self.n_keys, self.device = int(n_cams), int(n_keys), int(device)
        self.n_groups, self.n_obs = 0, 0

    def set_template(self, points):
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        if pts.shape[0] != self.n_keys:
            raise ValueError(f"expected {self.n_keys} template points")
        self._call("pcs_intr_set_template", self._h, self._ptr(pts))

    def set_observations(self, key, uv, start_inds, group_cam):
        """Host arrays sorted by group, the groups sorted by camera: key (n_obs,) int, uv (n_obs, 2), start_inds (n_groups + 1,),
        group_cam (n_groups,) int."""
        key = np.ascontiguousarray(key, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        gcam = np.ascontiguousarray(group_cam, dtype=np.int32)
        if start.ndim != 1 or start.shape[0] < 1 or gcam.shape != (start.shape[0] - 1,) or uv.shape != (key.shape[0], 2):
            raise ValueError("expected key (n_obs,), uv (n_obs, 2), start_inds (n_groups + 1,), group_cam (n_groups,)")
        self._call("pcs_intr_set_observations", self._h, key.shape[0], self._ptr(key), self._ptr(uv), start.shape[0] - 1, self._ptr(start), self._ptr(gcam))
        self.n_groups, self.n_obs = start.shape[0] - 1, key.shape[0]

    def run(self, model: str = "auto", min_points: int = 13, res=None, stream: int | None = None):
        """Queue the two kernels, behind the consensus stage when ``set_consensus`` turned it on (asynchronous; handle-owned outputs, fetched with ``results()``).  ``res``: (n_cams, 2) = (h, w) or None."""
        model_id, min_points = check_intrinsics_options(model, min_points)
        r = None if res is None else check_res(res, self.n_cams)
        self._call("pcs_intr_run", self._h, model_id, min_points, self._ptr(r), None, None, None, None, None, None, None, _stream_arg(stream))

    def results(self):
        """Wait for the last ``run``: (intr (n_cams, 9), cam_info (n_cams, 2) int32 [status, groups used], eig_ratio (n_cams,),
        homographies (n_groups, 9), frames (n_groups, 9), group_info (n_groups, 2) int32 [status, observations], pixel_stats (n_groups, 3))."""
        c, n = self.n_cams, self.n_groups
        out = (np.empty((c, 9)), np.empty((c, 2), dtype=np.int32), np.empty(c), np.empty((n, 9)), np.empty((n, 9)), np.empty((n, 2), dtype=np.int32),
               np.empty((n, 3)))
        self._call("pcs_intr_results", self._h, *(self._ptr(a) for a in out))
        return out

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_intr_last_kernel_ms")

    def set_consensus(self, n_hypotheses: int = 0, sample_size: int = 6, inlier_px: float = 8.0, seed: int = 0):
        """The consensus stage of the runs that follow (pcs_intr_set_consensus: cv2.findHomography's maxIters, the sample,
        ransacReprojThreshold and a seed); ``n_hypotheses = 0`` turns it off."""
        self._call("pcs_intr_set_consensus", self._h, *check_consensus_options(n_hypotheses, sample_size, inlier_px, seed))

    def get_consensus(self):
        """(n_hypotheses, sample_size, inlier_px, seed) in force."""
        h, s, px, seed = self._ct.c_int(0), self._ct.c_int(0), self._ct.c_double(0.0), self._ct.c_uint64(0)
        self._call("pcs_intr_get_consensus", self._h, self._ct.byref(h), self._ct.byref(s), self._ct.byref(px), self._ct.byref(seed))
        return int(h.value), int(s.value), float(px.value), int(seed.value)

    def consensus_results(self):
        """Wait for the last ``run`` with a consensus stage: (inlier (n_obs,) bool, cinfo (n_groups, 4) int32 = [inliers, winning
        hypothesis, finite hypotheses, consensus used], score (n_groups,))."""
        inlier, cinfo, score = np.zeros(self.n_obs, dtype=np.uint8), np.zeros((self.n_groups, 4), dtype=np.int32), np.empty(self.n_groups)
        self._call("pcs_intr_consensus_results", self._h, self._ptr(inlier), self._ptr(cinfo), self._ptr(score))
        return inlier.astype(bool), cinfo, score


def check_intrinsics_options(model, min_points):
    """-> (model id, min_points); ValueError before anything is queued.  A homography needs four points."""
    if model not in _capi.INTR_MODEL_IDS:
        raise ValueError(f"model must be one of {sorted(_capi.INTR_MODEL_IDS)}, got {model!r}")
    if check_min_points(min_points) < 4:
        raise ValueError(f"min_points must be at least 4 (a homography has eight unknowns), got {min_points!r}")
    return _capi.INTR_MODEL_IDS[model], int(min_points)


def check_res(res, n_cams: int) -> np.ndarray:
    """``res`` = (h, w) or (n_cams, 2) -> contiguous (n_cams, 2) float64; ValueError unless finite and positive."""
    r = np.asarray(res, dtype=np.float64)
    if r.shape not in ((2,), (n_cams, 2)):
        raise ValueError(f"res must be (h, w) or ({n_cams}, 2), got shape {r.shape}")
    r = np.ascontiguousarray(np.broadcast_to(r, (n_cams, 2)))
    if not (np.all(np.isfinite(r)) and np.all(r > 0)):
        raise ValueError("res must be finite and positive")
    return r


def group_by_board(dct, n_imgs: int, board_of_key, n_boards: int):
    """The host grouping of ``estimate_intrinsics``: one stable sort on (cam, im, board, key), as ``group_by_view`` does it (the same
    table shuffled reaches the device in the same order).  -> (order or None, group ids (cam * n_imgs + im) * n_boards + board, start)."""
    d = np.asarray(dct, dtype=np.float64)
    key = d[:, 2].astype(np.int64)
    gid = (d[:, 0].astype(np.int64) * int(n_imgs) + d[:, 1].astype(np.int64)) * int(n_boards) + np.asarray(board_of_key, dtype=np.int64)[key]
    rank = gid * (int(key.max()) + 1 if key.shape[0] else 1) + key
    order = None
    if rank.shape[0] > 1 and np.any(rank[1:] < rank[:-1]):
        order = np.argsort(rank, kind="stable")
        gid = gid[order]
    head = np.ones(gid.shape[0], dtype=bool)
    head[1:] = gid[1:] != gid[:-1]
    first = np.nonzero(head)[0]
    return order, gid[first], np.concatenate([first, [gid.shape[0]]]).astype(np.int64)


_intr_cache: dict = {}


def _intrinsics_estimator(device: int, n_cams: int, n_keys: int) -> IntrinsicsEstimator:
    return _cached_handle(_intr_cache, (int(device), int(n_cams), int(n_keys)), lambda: IntrinsicsEstimator(n_cams, n_keys, device))


def estimate_intrinsics(dct, points, *, n_cams: int | None = None, n_imgs: int | None = None, board_of_key=None, res=None, model: str = "auto",
                        min_points: int = 13, refine: bool = False, device: int = 0, consensus: int = 0, sample_size: int = 6,
                        inlier_px: float = 8.0, seed: int = 0, **lm_opts) -> IntrinsicsEstimate:
    """Camera intrinsics from the detections of a target made of planar boards, on the device (include/pcs_hip.h pcs_intr_run): what the
    reference's ``AbstractTarget.initial_calibration`` (calibration_targets/abstract_target.py:263-343) gets from cv2.calibrateCamera,
    as Zhang's closed form with zero skew (``model="full"``) or OpenCV's initCameraMatrix2D form (``"focal"``: the principal point
    at the image centre).  ``"auto"`` takes the focal model when ``res`` is given, as OpenCV does, and the full model otherwise.

    ``dct``: the flattened (N, 5) table [cam, im, key, u, v] in any order; ``points``: the template (K, 3); ``board_of_key`` (K,) int:
    the planar board of every key (default: one board; for a Ccube the face); ``res``: (h, w) or (C, 2); a group is used when it has at
    least ``min_points`` observations (the reference: more than 12).

    ``refine=True`` runs the device LM (``device_solver.lm_solve``, options ``lm_opts``) on projection + extrinsic3D + template
    points with every extrinsic fixed at identity, one free pose per (camera, image) view (started by ``estimate_view_poses`` at the
    closed form) and all nine intrinsics of every estimated camera free.  Cameras and views without an estimate stay out of it.

    ``consensus`` > 0 puts consensus sampling in front of the homographies (pcs_intr_set_consensus; cv2.findHomography's RANSAC in place
    of the plain fit): that many hypotheses per group, each the homography of ``sample_size`` random detections, are scored on all
    detections of the group by sum min(e^2, inlier_px^2); the closed form then uses the detections within ``inlier_px`` of the best one,
    and the result gains ``inliers``, ``group_inliers``, ``group_hypothesis``, ``group_consensus_used`` and ``group_score``.  A detection
    with a wrong id (tens to hundreds of pixels off) then no longer costs its camera the estimate.  64 is a good value (see
    ``estimate_view_poses``); ``seed`` keys the counter-based sampler and the hypothesis count is fixed, so two calls agree bit for bit,
    and a table without outliers gives the bits of ``consensus=0``.  A homography cannot model lens distortion: ``inlier_px`` must
    cover what the lens moves a detection by, or good rows at the image's edge are lost.  With ``refine=True`` the per-view poses and
    the LM run on the inlier rows only: rows beyond ``inlier_px`` are kept out of the refinement too.  The cached handle is shared:
    every call states its setting."""
    global last_intrinsics_kernel_ms
    check_intrinsics_options(model, min_points)
    cons = check_consensus_options(consensus, sample_size, inlier_px, seed)
    if lm_opts and not refine:
        raise ValueError(f"options {sorted(lm_opts)} belong to the refinement: pass refine=True")
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if d.ndim != 2 or d.shape[1] != 5:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v]")
    K = pts.shape[0]
    bok = np.zeros(K, dtype=np.int64) if board_of_key is None else np.asarray(board_of_key)
    if bok.shape != (K,) or bok.dtype.kind not in "iu" or (K and bok.min() < 0):
        raise ValueError(f"board_of_key must be ({K},) non-negative integers")
    n_boards = int(bok.max()) + 1 if K else 1
    C = (int(d[:, 0].max()) + 1 if d.shape[0] else 0) if n_cams is None else int(n_cams)
    I = (int(d[:, 1].max()) + 1 if d.shape[0] else 0) if n_imgs is None else int(n_imgs)
    if d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 1].min() < 0 or d[:, 1].max() >= I or d[:, 2].min() < 0 or d[:, 2].max() >= K):
        raise ValueError("camera, image or key index of the table outside n_cams / n_imgs / the template")
    r = None if res is None else check_res(res, C)
    if d.shape[0] == 0 or C == 0:
        z = np.zeros(C, dtype=np.int32)
        out = IntrinsicsEstimate(intr=np.full((C, 9), np.nan), status=z, n_groups=z.copy(), eig_ratio=np.full(C, np.nan), homographies=np.empty((0, 3, 3)),
                                 plane_frames=np.empty((0, 9)), group_status=np.empty(0, dtype=np.int32), group_counts=np.empty(0, dtype=np.int32),
                                 group_index=np.empty((0, 3), dtype=np.int64))
        if cons[0] > 0:
            out.inliers, out.group_inliers, out.group_hypothesis = np.zeros(d.shape[0], dtype=bool), z[:0].copy(), z[:0].copy()
            out.group_consensus_used, out.group_score = np.zeros(0, dtype=bool), np.empty(0)
    else:
        order, gid, start = group_by_board(d, I, bok, n_boards)
        ds = d if order is None else d[order]
        index = np.stack([gid // (I * n_boards), (gid // n_boards) % I, gid % n_boards], axis=1)
        est = _intrinsics_estimator(device, C, K)
        est.set_template(pts)
        est.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, index[:, 0].astype(np.int32))
        est.set_consensus(*cons)   # the handle is shared: every call states its setting
        est.run(model, min_points, r)
        intr, cinfo, eig, H, frames, ginfo, _ = est.results()
        last_intrinsics_kernel_ms = est.last_kernel_ms()
        out = IntrinsicsEstimate(intr=intr, status=cinfo[:, 0].copy(), n_groups=cinfo[:, 1].copy(), eig_ratio=eig, homographies=H.reshape(-1, 3, 3),
                                 plane_frames=frames, group_status=ginfo[:, 0].copy(), group_counts=ginfo[:, 1].copy(), group_index=index)
        if cons[0] > 0:
            inl, gc, out.group_score = est.consensus_results()
            if order is None:
                out.inliers = inl
            else:
                out.inliers = np.zeros(d.shape[0], dtype=bool)
                out.inliers[order] = inl
            out.group_inliers, out.group_hypothesis, out.group_consensus_used = gc[:, 0].copy(), gc[:, 1].copy(), gc[:, 3] != 0
    if refine:
        _refine_intrinsics(out, d if out.inliers is None else d[out.inliers], pts, I, device, lm_opts)
    return out


def _refine_intrinsics(est: IntrinsicsEstimate, d: np.ndarray, pts: np.ndarray, n_imgs: int, device: int, lm_opts: dict) -> None:
    """The refinement of ``estimate_intrinsics``: fills ``intr_init``, ``intr``, ``rms_init``, ``rms`` and ``lm`` in place."""
    from . import function_blocks as fb
    from .device_solver import lm_solve
    from .handlers import ChainProblem

    C, I = est.intr.shape[0], int(n_imgs)
    est.intr_init = est.intr.copy()
    est.rms_init, est.rms = np.full(C, np.nan), np.full(C, np.nan)
    have = est.status != INTR_NOT_ESTIMATED
    if not have.any():
        return
    cam, im = d[:, 0].astype(np.int64), d[:, 1].astype(np.int64)
    start = np.where(have[:, None], est.intr, np.array([1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]))   # rows of cameras that stay out: never read
    vp = estimate_view_poses(d[have[cam]], pts, start, n_imgs=I, device=device)
    seen = vp.status != PNP_NOT_ESTIMATED                                   # (C, I) views with a pose
    rows = have[cam] & seen[cam, im]
    if not rows.any():
        return
    det = np.ascontiguousarray(np.column_stack([cam[rows], cam[rows] * I + im[rows], d[rows, 2], d[rows, 3:5]]))
    poses = np.where(seen[:, :, None], vp.poses, 0.0).reshape(C * I, 6)
    free_cam = np.zeros(C, dtype=bool)
    free_cam[np.unique(cam[rows])] = True
    unfixed = [np.repeat(free_cam[:, None], 9, axis=1), np.zeros((C, 6), dtype=bool), np.repeat(seen.reshape(-1, 1), 6, axis=1)]
    op = fb.optimisation_function([fb.projection(), fb.extrinsic3D(), fb.template_points()], device=device, counts=(C, C * I, pts.shape[0]))
    prob = ChainProblem(op, det, [start, np.zeros((C, 6)), poses], template=pts, unfixed=unfixed)
    loss = prob.make_loss_fun()
    n_rows = np.bincount(det[:, 0].astype(np.int64), minlength=C)

    def rms_per_camera(x):
        r2 = np.sum(np.asarray(loss(x)).reshape(-1, 2) ** 2, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(free_cam, np.sqrt(np.bincount(det[:, 0].astype(np.int64), weights=r2, minlength=C) / n_rows), np.nan)

    est.rms_init = rms_per_camera(prob.x0)
    est.lm = lm_solve(prob, prob.x0, **lm_opts)
    refined = prob.get_bundle_adjustment_inputs(est.lm.x)[0]
    est.intr = np.where(free_cam[:, None], refined, est.intr_init)
    est.rms = rms_per_camera(est.lm.x)


# ---- view-graph seeding (row f7: extrinsics along a tree through the co-visibility graph, candidates scored in one pass) ------------
last_rig_kernel_ms = None


@dataclass
class EdgeConsensus:
    """Relative camera transforms by consensus (``rig_edge_consensus``), per pair a < b in lexicographic order: ``pairs`` (P, 2);
    ``n`` (P,) images both cameras have a pose for; ``medoid`` (P,) the image whose candidate M[a, i] inv(M[b, i]) was chosen (-1 for
    n = 0); ``T`` (P, 3, 4) that transform, camera b -> camera a (NaN for n = 0); ``sigma`` (P,) mean distance of the medoid from the
    other candidates in length units (0 for n = 1, NaN for n = 0); ``score`` / ``runner_up`` (P,) the summed distances of the medoid and
    of the second-best candidate (+inf for n < 2); ``centroid`` (3,), ``rho``: the template's centroid and RMS radius."""
    pairs: np.ndarray
    n: np.ndarray
    medoid: np.ndarray
    T: np.ndarray
    sigma: np.ndarray
    score: np.ndarray
    runner_up: np.ndarray
    centroid: np.ndarray
    rho: float


def camera_pairs(n_cams: int) -> np.ndarray:
    """(P, 2): the pairs a < b in the order of the device's edge outputs; pair (a, b) is row a (2 C - a - 1) / 2 + b - a - 1."""
    a, b = np.triu_indices(int(n_cams), k=1)
    return np.stack([a, b], axis=1)


class RigGraph(_Handle):
    """Owner of one ``pcs_rig_graph`` handle (include/pcs_hip.h): cameras, template, observation copies, view poses, extrinsics and the
    outputs of the two runs (edges, scores) stay on the device across calls."""

    _create, _destroy = "pcs_rig_create", "pcs_rig_destroy"

    def __init__(self, n_cams: int, n_imgs: int, n_keys: int, device: int = 0):
        super().__init__(device, n_cams, n_imgs, n_keys)
        self.n_cams, self.n_imgs, self.n_keys, self.device = int(n_cams), int(n_imgs), int(n_keys), int(device)
        self.n_pairs = self.n_cams * (self.n_cams - 1) // 2
        self.n_views = 0
        self.centroid, self.rho = None, None

    def set_cameras(self, intr):
        K = np.ascontiguousarray(intr, dtype=np.float64)
        if K.shape != (self.n_cams, 9):
            raise ValueError(f"expected intr ({self.n_cams}, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]")
        self._call("pcs_rig_set_cameras", self._h, self._ptr(K))

    def set_template(self, points):
        """-> (centroid (3,), rho): the template's centroid and the RMS distance of its points from it."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        if pts.shape[0] != self.n_keys:
            raise ValueError(f"expected {self.n_keys} template points")
        frame = np.empty(4)
        self._call("pcs_rig_set_template", self._h, self._ptr(pts), self._ptr(frame))
        self.centroid, self.rho = frame[:3].copy(), float(frame[3])
        return self.centroid, self.rho

    def set_observations(self, key, uv, start_inds, view_cam, view_im):
        """Host arrays sorted by view, the views sorted by (camera, image) — ``group_by_view``'s order: key (n_obs,) int, uv (n_obs, 2),
        start_inds (n_views + 1,), view_cam, view_im (n_views,) int."""
        key = np.ascontiguousarray(key, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        vcam = np.ascontiguousarray(view_cam, dtype=np.int32)
        vim = np.ascontiguousarray(view_im, dtype=np.int32)
        if start.ndim != 1 or start.shape[0] < 1 or vcam.shape != (start.shape[0] - 1,) or vim.shape != vcam.shape or uv.shape != (key.shape[0], 2):
            raise ValueError("expected key (n_obs,), uv (n_obs, 2), start_inds (n_views + 1,), view_cam and view_im (n_views,)")
        self._call("pcs_rig_set_observations", self._h, key.shape[0], self._ptr(key), self._ptr(uv), start.shape[0] - 1, self._ptr(start), self._ptr(vcam),
                   self._ptr(vim))
        self.n_views = start.shape[0] - 1

    def set_view_poses(self, poses):
        p = np.ascontiguousarray(poses, dtype=np.float64)
        if p.shape != (self.n_cams, self.n_imgs, 6):
            raise ValueError(f"expected view poses ({self.n_cams}, {self.n_imgs}, 6)")
        self._call("pcs_rig_set_view_poses", self._h, self._ptr(p))

    def run_edges(self, stream: int | None = None):
        """Queue the edge consensus (asynchronous; fetch with ``edges()``)."""
        self._call("pcs_rig_run_edges", self._h, _stream_arg(stream))

    def edges(self):
        """Wait for the last ``run_edges``: (info (P, 2) int32 [n, medoid image], T (P, 12), stats (P, 3) [sigma, S, runner-up S])."""
        n = self.n_pairs
        info, T, stats = np.empty((n, 2), dtype=np.int32), np.empty((n, 12)), np.empty((n, 3))
        self._call("pcs_rig_edges", self._h, self._ptr(info), self._ptr(T), self._ptr(stats))
        return info, T, stats

    def set_extrinsics(self, ext):
        E = np.ascontiguousarray(np.asarray(ext, dtype=np.float64).reshape(-1, 12))
        if E.shape != (self.n_cams, 12):
            raise ValueError(f"expected extrinsics ({self.n_cams}, 3, 4), world -> camera")
        self._call("pcs_rig_set_extrinsics", self._h, self._ptr(E))

    def run_scores(self, stream: int | None = None):
        """Queue preparation, scoring and the per-image sums (asynchronous; fetch with ``results()``)."""
        self._call("pcs_rig_run_scores", self._h, _stream_arg(stream))

    def results(self, partial: bool = False):
        """Wait for the last ``run_scores``: (W (C, I, 3, 4), errors (C, I)[, partial (C, n_views)])."""
        W, err = np.empty((self.n_cams, self.n_imgs, 3, 4)), np.empty((self.n_cams, self.n_imgs))
        part = np.empty((self.n_cams, self.n_views)) if partial else None
        self._call("pcs_rig_results", self._h, self._ptr(W), self._ptr(err), self._ptr(part))
        return (W, err, part) if partial else (W, err)

    def last_edges_ms(self) -> float:
        ms = self._ct.c_float(0.0)
        self._call("pcs_rig_last_kernel_ms", self._h, self._ct.byref(ms), None, None)
        return float(ms.value)

    def last_scores_ms(self):
        """-> (preparation, scoring) device times of the last ``run_scores``."""
        a, b = self._ct.c_float(0.0), self._ct.c_float(0.0)
        self._call("pcs_rig_last_kernel_ms", self._h, None, self._ct.byref(a), self._ct.byref(b))
        return float(a.value), float(b.value)


_rig_cache: dict = {}


def _rig_graph(device: int, n_cams: int, n_imgs: int, n_keys: int) -> RigGraph:
    return _cached_handle(_rig_cache, (int(device), int(n_cams), int(n_imgs), int(n_keys)), lambda: RigGraph(n_cams, n_imgs, n_keys, device))


def rig_edge_consensus(view_poses, points, device: int = 0) -> EdgeConsensus:
    """Per camera pair the medoid of the relative transforms M[a, i] inv(M[b, i]) over the images both cameras have a pose for, on the
    device (include/pcs_hip.h pcs_rig_run_edges).  ``view_poses`` (C, I, 6) as ``estimate_view_poses`` returns them (NaN = no pose);
    ``points`` the template (K, 3)."""
    global last_rig_kernel_ms
    vp = np.asarray(view_poses, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if vp.ndim != 3 or vp.shape[2] != 6 or vp.shape[0] < 1 or vp.shape[1] < 1:
        raise ValueError("expected view poses (C, I, 6)")
    C, I = vp.shape[:2]
    g = _rig_graph(device, C, I, pts.shape[0])
    centroid, rho = g.set_template(pts)
    g.set_view_poses(vp)
    g.run_edges()
    info, T, stats = g.edges()
    last_rig_kernel_ms = g.last_edges_ms()
    return EdgeConsensus(pairs=camera_pairs(C), n=info[:, 0].copy(), medoid=info[:, 1].copy(), T=T.reshape(-1, 3, 4), sigma=stats[:, 0].copy(),
                         score=stats[:, 1].copy(), runner_up=stats[:, 2].copy(), centroid=centroid, rho=rho)


def rig_candidate_scores(dct, points, intr, view_poses, ext, n_imgs: int, device: int = 0):
    """Every camera's estimate of every image's target pose, W[c', i] = inv(E_c') M[c', i], and its summed reprojection error over ALL
    detections of the image, errors[c', i], in one pass over the table on the device (include/pcs_hip.h pcs_rig_run_scores).
    ``dct`` (N, 5) in any order; ``ext`` (C, 3, 4) world -> camera.  -> (W (C, I, 3, 4), errors (C, I)), NaN where camera c' has no pose
    for image i."""
    global last_rig_kernel_ms
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    vp = np.asarray(view_poses, dtype=np.float64)
    C, I = vp.shape[0], int(n_imgs)
    if d.ndim != 2 or d.shape[1] != 5 or vp.shape != (C, I, 6):
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v] and view poses (C, n_imgs, 6)")
    if d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 1].min() < 0 or d[:, 1].max() >= I):
        raise ValueError("camera or image index of the table outside the view poses")
    order, ids, start = group_by_view(d, I)
    ds = d if order is None else d[order]
    g = _rig_graph(device, C, I, pts.shape[0])
    g.set_cameras(intr)
    g.set_template(pts)
    g.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (ids // I).astype(np.int32), (ids % I).astype(np.int32))
    g.set_view_poses(vp)
    g.set_extrinsics(ext)
    g.run_scores()
    W, errors = g.results()
    last_rig_kernel_ms = sum(g.last_scores_ms())
    return W, errors


# ---- the target pose per image in a calibrated rig (row f9: optimisation/find_target.py) -----------------------------------------------
# per-image status of the localisation (include/pcs_hip.h PCS_RIGPOSE_*: the meanings of PCS_PNP_*)
from ._capi import RIGPOSE_CONVERGED, RIGPOSE_MAX_ITER, RIGPOSE_NO_DECREASE, RIGPOSE_NOT_ESTIMATED  # noqa: E402,F401
last_rigpose_kernel_ms = None
# a scaled J'J whose smallest eigenvalue is below this fraction of its largest leaves no digit of the covariance: the image is reported NaN
COVARIANCE_RANK_TOL = 1e-12


def unpack_hessian(packed) -> np.ndarray:
    """(n, 21) packed upper triangles by rows (00 01 .. 05 11 .. 55) -> (n, 6, 6) symmetric."""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1, 21)
    H = np.empty((packed.shape[0], 6, 6))
    iu = np.triu_indices(6)
    H[:, iu[0], iu[1]] = packed
    H[:, iu[1], iu[0]] = packed
    return H


@dataclass
class ImagePoses:
    """Target poses per image in a rig of fixed cameras (``localise_target``): ``poses`` (I, 6) = [rotvec, t], target -> world,
    X_cam = E_c (R(rotvec) X_target + t); ``poses_init`` the start; ``rms`` / ``rms_init`` (I,) RMS reprojection error in pixels over all
    detections of the image at the pose / at the start (rms <= rms_init); ``status`` (RIGPOSE_*), ``iterations`` (LM trials),
    ``n_points`` (detections), ``n_cams`` (cameras that contributed): (I,) int32; ``hessian`` (I, 6, 6) = J'J at the pose for the update
    R <- exp([d omega]x) R, t <- t + d t; ``residuals`` (N, 2) uv - projection in the table's row order, or None.  Images without
    detections, with fewer than ``min_points`` or without a usable start: NaN, status 0.

    ``loss`` / ``f_scale``: the robust loss the poses minimise (``localise_target``); ``cost`` / ``cost_init`` (I,) scipy's
    0.5 sum rho0 at the pose / at the start (half the sum of squares for 'linear'; cost <= cost_init).  Under a loss ``hessian`` is the
    robust sum s^2 J'J, ``rms`` stays the plain pixel RMS (it may exceed ``rms_init``) and ``residuals`` the raw ones."""
    poses: np.ndarray
    poses_init: np.ndarray
    rms: np.ndarray
    rms_init: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    n_points: np.ndarray
    n_cams: np.ndarray
    hessian: np.ndarray
    residuals: np.ndarray | None = None
    cost: np.ndarray | None = None
    cost_init: np.ndarray | None = None
    loss: str = "linear"
    f_scale: float = 1.0

    def covariance(self, absolute_sigma: bool = False) -> np.ndarray:
        """(I, 6, 6) = sigma^2 inv(H) in the coordinates (d omega, d t) of the update, sigma^2 = sum r^2 / (2 n - 6), or 1 with
        ``absolute_sigma`` (the meanings of ``device_solver.parameter_covariance``).  Under a loss H is the returned robust H and
        sigma^2 = 2 cost / (2 n - 6).  NaN for an image that was not estimated, has no degree of freedom left (2 n <= 6) or a singular H
        (a NumPy batch inverse on the host; nothing raises)."""
        I = self.hessian.shape[0]
        out = np.full((I, 6, 6), np.nan)
        n = self.n_points.astype(np.float64)
        for i in range(I):
            H = self.hessian[i]
            dof = 2.0 * n[i] - 6.0
            if not np.all(np.isfinite(H)) or (dof <= 0 and not absolute_sigma):
                continue
            d = np.sqrt(np.diag(H))
            if not np.all(d > 0):
                continue
            lam = np.linalg.eigvalsh(H / np.outer(d, d))
            if not lam[0] > COVARIANCE_RANK_TOL * lam[-1]:
                continue
            try:
                inv = np.linalg.inv(H)
            except np.linalg.LinAlgError:
                continue
            if absolute_sigma:
                s2 = 1.0
            elif self.loss != "linear":
                s2 = 2.0 * self.cost[i] / dof
            else:
                s2 = self.rms[i] ** 2 * n[i] / dof
            out[i] = s2 * inv
        return out


class RigLocaliser(_Handle):
    """Owner of one ``pcs_rig_localiser`` handle (include/pcs_hip.h): camera and extrinsic tables, template, observation copies, start
    poses and outputs stay on the device across calls."""

    _create, _destroy = "pcs_rigpose_create", "pcs_rigpose_destroy"

    def __init__(self, n_cams: int, n_keys: int, device: int = 0):
        super().__init__(device, n_cams, n_keys)
        self.n_cams, self.n_keys, self.device = int(n_cams), int(n_keys), int(device)
        self.n_groups, self.n_obs = 0, 0
        self._residuals = False

    def set_cameras(self, intr):
        K = np.ascontiguousarray(intr, dtype=np.float64)
        if K.shape != (self.n_cams, 9):
            raise ValueError(f"expected intr ({self.n_cams}, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]")
        self._call("pcs_rigpose_set_cameras", self._h, self._ptr(K))

    def set_extrinsics(self, ext):
        E = np.ascontiguousarray(ext, dtype=np.float64)
        if E.shape != (self.n_cams, 3, 4):
            raise ValueError(f"expected ext ({self.n_cams}, 3, 4) world -> camera")
        self._call("pcs_rigpose_set_extrinsics", self._h, self._ptr(E))

    def set_template(self, points):
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        if pts.shape[0] != self.n_keys:
            raise ValueError(f"expected {self.n_keys} template points")
        self._call("pcs_rigpose_set_template", self._h, self._ptr(pts))

    def set_observations(self, key, cam, uv, start_inds):
        """Host arrays sorted by (image, camera, key): key, cam (n_obs,) int, uv (n_obs, 2), start_inds (n_groups + 1,)."""
        key = np.ascontiguousarray(key, dtype=np.int32)
        cam = np.ascontiguousarray(cam, dtype=np.int32)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        if start.ndim != 1 or start.shape[0] < 1 or key.ndim != 1 or cam.shape != key.shape or uv.shape != (key.shape[0], 2):
            raise ValueError("expected key (n_obs,), cam (n_obs,), uv (n_obs, 2), start_inds (n_groups + 1,)")
        self._call("pcs_rigpose_set_observations", self._h, key.shape[0], self._ptr(key), self._ptr(cam), self._ptr(uv), start.shape[0] - 1, self._ptr(start))
        self.n_groups, self.n_obs = start.shape[0] - 1, key.shape[0]

    def set_start(self, poses):
        p = np.ascontiguousarray(poses, dtype=np.float64)
        if p.shape != (self.n_groups, 6):
            raise ValueError(f"expected start poses ({self.n_groups}, 6)")
        self._call("pcs_rigpose_set_start", self._h, self._ptr(p))

    def run(self, max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"],
            gtol: float = REFINE_DEFAULTS["gtol"], min_points: int = 6, group_lanes: int | None = None, residuals: bool = False,
            stream: int | None = None):
        """Queue the kernel (asynchronous; handle-owned outputs, fetched with ``results()``)."""
        max_iter, ftol, xtol, gtol = check_refine_options(max_iter, ftol, xtol, gtol)
        min_points = check_min_points(min_points)
        lanes = check_group_lanes(group_lanes)
        self._call("pcs_rigpose_run", self._h, max_iter, ftol, xtol, gtol, min_points, lanes, self._capi.RIGPOSE_RESIDUALS if residuals else 0,
                   None, None, None, None, None, _stream_arg(stream))
        self._residuals = bool(residuals)

    def set_loss(self, loss: str = "linear", f_scale: float = 1.0):
        """The robust loss of ``run`` (include/pcs_hip.h pcs_rigpose_set_loss): scipy's 'linear' (the default), 'huber', 'soft_l1',
        'cauchy', 'arctan' on each scalar residual, ``f_scale`` in pixels.  It stays with the handle until it is set again."""
        loss, f_scale = check_loss(loss, f_scale)
        self._call("pcs_rigpose_set_loss", self._h, self._capi.LOSS_IDS[loss], f_scale)

    def get_loss(self):
        """The current (loss, f_scale) of ``set_loss``."""
        k, fs = self._ct.c_int(), self._ct.c_double()
        self._call("pcs_rigpose_get_loss", self._h, self._ct.byref(k), self._ct.byref(fs))
        return {v: n for n, v in self._capi.LOSS_IDS.items()}[k.value], fs.value

    def costs(self) -> np.ndarray:
        """Wait for the last ``run``: (n, 2) scipy's cost 0.5 sum rho0 at the returned pose and at the start (NaN: not estimated)."""
        cost = np.empty((self.n_groups, 2))
        self._call("pcs_rigpose_costs", self._h, self._ptr(cost))
        return cost

    def results(self):
        """Wait for the last ``run``: (pose (n, 6), rms (n, 2), info (n, 4) int32, hessian (n, 21), residuals or None)."""
        n = self.n_groups
        pose, rms, info, hess = np.empty((n, 6)), np.empty((n, 2)), np.empty((n, 4), dtype=np.int32), np.empty((n, 21))
        resid = np.empty((self.n_obs, 2)) if self._residuals else None
        self._call("pcs_rigpose_results", self._h, self._ptr(pose), self._ptr(rms), self._ptr(info), self._ptr(hess), self._ptr(resid))
        return pose, rms, info, hess, resid

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_rigpose_last_kernel_ms")


def check_group_lanes(group_lanes) -> int:
    """None (the width rule of include/pcs_hip.h pcs_rigpose_run decides), 16 or 64 -> the C argument."""
    if group_lanes is None:
        return 0
    if isinstance(group_lanes, bool) or not isinstance(group_lanes, (int, np.integer)) or int(group_lanes) not in (16, 64):
        raise ValueError(f"group_lanes must be None, 16 or 64, got {group_lanes!r}")
    return int(group_lanes)


def group_by_image(dct):
    """The host grouping of ``localise_target``: one stable sort on (im, cam, key), skipped when the table is already ordered, so that
    an image's observations reach the device in one order whatever the order of the table.  ``dct`` holds valid camera indices.
    -> (order or None, image ids (n_groups,), start (n_groups + 1,))."""
    d = np.asarray(dct, dtype=np.float64)
    im, cam, key = d[:, 1].astype(np.int64), d[:, 0].astype(np.int64), d[:, 2].astype(np.int64)
    n = d.shape[0]
    cspan = int(cam.max()) + 1 if n else 1
    kspan = int(key.max()) + 1 if n else 1
    rank = (im * cspan + cam) * kspan + key if n and key.min() >= 0 else im * cspan + cam   # keys out of range are refused by the handle later
    order = None
    if n > 1 and np.any(rank[1:] < rank[:-1]):
        order = np.argsort(rank, kind="stable")
        im = im[order]
    head = np.ones(n, dtype=bool)
    head[1:] = im[1:] != im[:-1]
    first = np.nonzero(head)[0]
    return order, im[first], np.concatenate([first, [n]]).astype(np.int64)


_rigpose_cache: dict = {}


def _rig_localiser(device: int, n_cams: int, n_keys: int) -> RigLocaliser:
    return _cached_handle(_rigpose_cache, (int(device), int(n_cams), int(n_keys)), lambda: RigLocaliser(n_cams, n_keys, device))


def rig_pose_start(dct, points, intr, ext, n_imgs: int, min_points: int = 6, device: int = 0, consensus: int = 0, sample_size: int = 6,
                   inlier_px: float = 8.0, seed: int = 0) -> np.ndarray:
    """A start (I, 6) for ``localise_target`` from the existing pieces: the per-view poses of ``estimate_view_poses``, every camera's
    estimate W[c', i] = inv(E_c') M[c', i] of the image's pose and its error over ALL detections of the image
    (``rig_candidate_scores``); the image takes the finite candidate of lowest error, ties to the lowest camera.  NaN where there is none.
    The start is linear whatever loss ``localise_target`` runs with: the PnP and the scores take no loss, an outlier moves the start
    and the robust solve works from there — unless ``consensus`` > 0 puts consensus sampling in front of the per-view poses
    (``estimate_view_poses``: ``consensus``, ``sample_size``, ``inlier_px``, ``seed``), which keeps gross outliers out of the candidates."""
    from .pose_seeding import pose_from_4x4, to_4x4

    vp = estimate_view_poses(dct, points, intr, n_imgs=n_imgs, min_points=min_points, device=device, consensus=consensus, sample_size=sample_size,
                             inlier_px=inlier_px, seed=seed)
    W, errors = rig_candidate_scores(dct, points, intr, vp.poses, ext, n_imgs, device=device)
    W, errors = np.asarray(W, dtype=np.float64).reshape(-1, n_imgs, 3, 4), np.asarray(errors, dtype=np.float64).reshape(-1, n_imgs)
    finite = np.isfinite(errors) & np.isfinite(W.reshape(W.shape[0], n_imgs, 12)).all(axis=-1)
    best = np.argmin(np.where(finite, errors, np.inf), axis=0)   # the first of equal minima: the lowest camera
    start = pose_from_4x4(to_4x4(W[best, np.arange(n_imgs)]))
    start[~finite.any(axis=0)] = np.nan
    return start


def check_localise_arguments(dct, points, intr, ext, n_imgs, poses_init, min_points, max_iter, ftol, xtol, gtol, group_lanes):
    """Everything ``localise_target`` can refuse on the host (ValueError), before a device is touched."""
    opts = check_refine_options(max_iter, ftol, xtol, gtol)
    min_points = check_min_points(min_points)
    lanes = check_group_lanes(group_lanes)
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64)
    K = np.asarray(intr, dtype=np.float64)
    E = np.asarray(ext, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 5 or K.ndim != 2 or K.shape[1] != 9:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v] and intr (C, 9)")
    if pts.size == 0 or pts.size % 3:
        raise ValueError("expected template points (K, 3)")
    pts = pts.reshape(-1, 3)
    C = K.shape[0]
    if E.shape != (C, 3, 4):
        raise ValueError(f"expected ext ({C}, 3, 4) world -> camera, got {E.shape}")
    if not (np.all(np.isfinite(K)) and np.all(np.isfinite(E))):
        raise ValueError("intr and ext must be finite: every camera is held fixed")
    if n_imgs is None:
        n_imgs = int(d[:, 1].max()) + 1 if d.shape[0] else 0
    if isinstance(n_imgs, bool) or not isinstance(n_imgs, (int, np.integer)) or n_imgs < 0:
        raise ValueError(f"n_imgs must be an integer >= 0, got {n_imgs!r}")
    I = int(n_imgs)
    if d.shape[0]:
        if d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 1].min() < 0 or d[:, 1].max() >= I:
            raise ValueError("camera or image index of the table outside the intrinsics / n_imgs")
        if d[:, 2].min() < 0 or d[:, 2].max() >= pts.shape[0]:
            raise ValueError("key of the table outside the template")
    if poses_init is not None:
        poses_init = np.array(poses_init, dtype=np.float64)
        if poses_init.shape != (I, 6):
            raise ValueError(f"expected poses_init ({I}, 6), got {poses_init.shape}")
    return d, pts, K, E, I, poses_init, min_points, opts, lanes


def localise_target(dct, points, intr, ext, *, n_imgs: int | None = None, poses_init=None, min_points: int = 6,
                    max_iter: int = REFINE_DEFAULTS["max_iter"], ftol: float = REFINE_DEFAULTS["ftol"], xtol: float = REFINE_DEFAULTS["xtol"],
                    gtol: float = REFINE_DEFAULTS["gtol"], group_lanes: int | None = None, return_residuals: bool = False,
                    device: int = 0, loss: str = "linear", f_scale: float = 1.0, start_consensus: int = 0) -> ImagePoses:
    """The pose of the known target in every image of a rig whose cameras are held fixed, on the device (include/pcs_hip.h
    pcs_rigpose_run): what the reference's ``find_target_poses`` (optimisation/find_target.py:9-82) gets from a bundle adjustment with
    every camera's "ext" / "int" / "dst" fixed, as one independent 6-parameter problem per image.

    ``dct``: the flattened (N, 5) table [cam, im, key, u, v] in any order (the same table shuffled gives the same bits); ``points``: the
    template (K, 3); ``intr``: (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2]; ``ext``: (C, 3, 4) world -> camera, the convention of
    ``rig_candidate_scores``; ``n_imgs``: images of the result (default: largest image index + 1); ``poses_init``: (I, 6) starts (NaN
    rows are not estimated), default ``rig_pose_start``; ``group_lanes``: 16 or 64 lanes per image, default by the mean number of
    detections per image (include/pcs_hip.h).

    ``loss`` / ``f_scale``: scipy ``least_squares``'s robust losses ('linear', 'huber', 'soft_l1', 'cauchy', 'arctan') on each scalar
    residual, ``f_scale`` in pixels (include/pcs_hip.h pcs_rigpose_set_loss; the reference's commented ``loss = "cauchy"``).  The
    default start stays the linear one (``rig_pose_start``); ``start_consensus`` > 0 (64 is a good value) gives its per-view poses that
    many consensus hypotheses (``estimate_view_poses(consensus=...)``), so that a wrong id cannot put every residual of an image beyond
    ``f_scale`` before the robust solve begins.  ``diagnostics.robust_weights(res.residuals, loss, f_scale)`` lists what was
    down-weighted."""
    global last_rigpose_kernel_ms
    loss, f_scale = check_loss(loss, f_scale)
    d, pts, K, E, I, start, min_points, opts, lanes = check_localise_arguments(dct, points, intr, ext, n_imgs, poses_init, min_points, max_iter, ftol, xtol,
                                                                               gtol, group_lanes)
    out = ImagePoses(poses=np.full((I, 6), np.nan), poses_init=np.full((I, 6), np.nan), rms=np.full(I, np.nan), rms_init=np.full(I, np.nan),
                     status=np.zeros(I, dtype=np.int32), iterations=np.zeros(I, dtype=np.int32), n_points=np.zeros(I, dtype=np.int32),
                     n_cams=np.zeros(I, dtype=np.int32), hessian=np.full((I, 6, 6), np.nan),
                     residuals=np.empty((d.shape[0], 2)) if return_residuals else None, cost=np.full(I, np.nan), cost_init=np.full(I, np.nan),
                     loss=loss, f_scale=f_scale)
    if start is not None:
        out.poses_init[:] = start
    if d.shape[0] == 0:
        return out
    order, ids, first = group_by_image(d)
    ds = d if order is None else d[order]
    if start is None:
        start = rig_pose_start(ds, pts, K, E, I, min_points=min_points, device=device, consensus=check_consensus_options(start_consensus, 6, 8.0, 0)[0])
        out.poses_init[:] = start
    loc = _rig_localiser(device, K.shape[0], pts.shape[0])
    loc.set_cameras(K)
    loc.set_extrinsics(E)
    loc.set_template(pts)
    loc.set_observations(ds[:, 2].astype(np.int32), ds[:, 0].astype(np.int32), ds[:, 3:5], first)
    loc.set_start(start[ids])
    loc.set_loss(loss, f_scale)   # the handle is shared between calls: every call states its loss
    loc.run(*opts, min_points=min_points, group_lanes=lanes or None, residuals=return_residuals)
    pose, rms, info, hess, resid = loc.results()
    cost = loc.costs()
    out.cost[ids], out.cost_init[ids] = cost[:, 0], cost[:, 1]
    last_rigpose_kernel_ms = loc.last_kernel_ms()
    out.poses[ids] = pose
    out.rms[ids], out.rms_init[ids] = rms[:, 0], rms[:, 1]
    out.iterations[ids], out.status[ids], out.n_points[ids], out.n_cams[ids] = info[:, 0], info[:, 1], info[:, 2], info[:, 3]
    out.hessian[ids] = unpack_hessian(hess)
    if return_residuals:
        if order is None:
            out.residuals = resid
        else:
            out.residuals[order] = resid
    return out


# ---- registration of 3-D point sets (row f11: n_estimate_rigid_transform, ch:727-762, batched) ----------------------------------------
# per-problem status of the registration (include/pcs_hip.h PCS_ALIGN_*)
from ._capi import ALIGN_DEGENERATE, ALIGN_MODEL_IDS, ALIGN_NO_CONSENSUS, ALIGN_NONFINITE, ALIGN_OK, ALIGN_TOO_FEW  # noqa: E402,F401

ALIGN_STAGES = ("hypotheses", "scores", "selection", "fit")
ALIGN_CONSENSUS_MAX = 256   # hypotheses per problem that pcs_align_set_consensus takes
last_align_kernel_ms = None


@dataclass
class Alignment:
    """Registrations of P point-set problems (``align_points``): ``dst ~ scale * R @ src + t``.  ``R`` (P, 3, 3), ``t`` (P, 3),
    ``scale`` (P,) (1 for the rigid model) and ``rms`` (P,), the weighted RMS distance over the rows used, are NaN unless ``status``
    (ALIGN_*) is ALIGN_OK; ``n_used`` rows entered the fit, ``n_inliers`` of them by consensus (= ``n_used`` without), ``hypothesis``
    the winner (-1: none) and ``score`` its sum min(d^2, inlier_dist^2) (NaN without consensus); ``conditioning`` (P,) in [0, 1], 0 for
    collinear points (NaN where no fit was tried).  Per row of the table: ``inliers`` (n,) bool, the row entered the fit, and
    ``distances`` (n,), |dst - scale R src - t|; problem p owns rows ``start[p]:start[p + 1]``."""
    R: np.ndarray
    t: np.ndarray
    scale: np.ndarray
    rms: np.ndarray
    status: np.ndarray
    n_used: np.ndarray
    n_inliers: np.ndarray
    inliers: np.ndarray
    conditioning: np.ndarray
    hypothesis: np.ndarray
    score: np.ndarray
    distances: np.ndarray
    start: np.ndarray

    def matrix(self) -> np.ndarray:
        """(P, 4, 4) homogeneous transforms with scale * R in the upper left block."""
        M = np.zeros((self.R.shape[0], 4, 4))
        M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = self.scale[:, None, None] * self.R, self.t, 1.0
        return M

    def apply(self, points) -> np.ndarray:
        """scale * R @ x + t: ``points`` (n, 3) in the table's layout (every problem's rows by its own transform), or (P, K, 3)."""
        X = np.asarray(points, dtype=np.float64)
        if X.ndim == 3 and X.shape[0] == self.R.shape[0] and X.shape[2] == 3:
            return np.einsum("p,pij,pkj->pki", self.scale, self.R, X) + self.t[:, None, :]
        if X.ndim != 2 or X.shape != (int(self.start[-1]), 3):
            raise ValueError(f"expected points ({int(self.start[-1])}, 3) in the table's rows or ({self.R.shape[0]}, K, 3)")
        prob = np.repeat(np.arange(self.R.shape[0]), np.diff(self.start))
        return np.einsum("n,nij,nj->ni", self.scale[prob], self.R[prob], X) + self.t[prob]


def check_align_options(model, consensus, inlier_dist, seed, min_points, rank_tol, group_lanes=0):
    """Validate the options of the registration on the host (ValueError) before anything is queued: the checks of
    pcs_align_set_consensus and pcs_align_run.  -> (model code, consensus, inlier_dist, seed, min_points, rank_tol, group_lanes)."""
    if model not in ALIGN_MODEL_IDS:
        raise ValueError(f"model must be one of {sorted(ALIGN_MODEL_IDS)}, got {model!r}")
    for name, v, lo, hi in (("consensus", consensus, 0, ALIGN_CONSENSUS_MAX), ("seed", seed, 0, 2 ** 64 - 1), ("min_points", min_points, 3, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    dist = 0.0
    if int(consensus) > 0:
        if inlier_dist is None:
            raise ValueError("consensus > 0 needs inlier_dist, the largest distance of an inlier in the units of dst")
        try:
            dist = float(inlier_dist)
        except (TypeError, ValueError):
            raise ValueError(f"inlier_dist must be a finite number > 0, got {inlier_dist!r}") from None
        if not (np.isfinite(dist) and dist > 0.0):
            raise ValueError(f"inlier_dist must be a finite number > 0, got {inlier_dist!r}")
    try:
        tol = float(rank_tol)
    except (TypeError, ValueError):
        raise ValueError(f"rank_tol must be a number in [0, 1), got {rank_tol!r}") from None
    if not 0.0 <= tol < 1.0:
        raise ValueError(f"rank_tol must be a number in [0, 1), got {rank_tol!r}")
    if isinstance(group_lanes, bool) or group_lanes not in (0, 16, 64):
        raise ValueError(f"group_lanes must be 0 (by size), 16 or 64, got {group_lanes!r}")
    return ALIGN_MODEL_IDS[model], int(consensus), dist, int(seed), int(min_points), tol, int(group_lanes)


class PointAligner(_Handle):
    """Owner of one ``pcs_point_aligner`` handle (include/pcs_hip.h): the point table, the stage buffers and the outputs stay on the
    device across calls."""

    _create, _destroy = "pcs_align_create", "pcs_align_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device = int(device)
        self.n_problems, self.n_rows = 0, 0

    def set_points(self, src, dst, start_inds, weights=None):
        """Host arrays sorted by problem: src, dst (n, 3), start_inds (P + 1,), weights (n,) >= 0 or None.  Shapes raise ValueError;
        values are checked by the handle (PcsError) without touching the device.  Non-finite coordinates are data: the row is skipped."""
        x = np.ascontiguousarray(src, dtype=np.float64)
        y = np.ascontiguousarray(dst, dtype=np.float64)
        start = np.ascontiguousarray(start_inds, dtype=np.int64)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if start.ndim != 1 or start.shape[0] < 1 or x.ndim != 2 or x.shape[1] != 3 or y.shape != x.shape or (w is not None and w.shape != (x.shape[0],)):
            raise ValueError("expected src, dst (n, 3), start_inds (P + 1,) and weights (n,) or None")
        self._call("pcs_align_set_points", self._h, x.shape[0], self._ptr(x), self._ptr(y), self._ptr(w), start.shape[0] - 1, self._ptr(start))
        self.n_problems, self.n_rows = start.shape[0] - 1, x.shape[0]

    def set_consensus(self, n_hypotheses: int = 0, inlier_dist: float = 0.0, seed: int = 0):
        """Hypotheses per problem (0: no consensus stage), inlier distance in the units of dst and the seed of the sampler, for the runs
        that follow."""
        self._call("pcs_align_set_consensus", self._h, int(n_hypotheses), float(inlier_dist), int(seed))

    def get_consensus(self):
        """(n_hypotheses, inlier_dist, seed) in force."""
        h, d, seed = self._ct.c_int(0), self._ct.c_double(0.0), self._ct.c_uint64(0)
        self._call("pcs_align_get_consensus", self._h, self._ct.byref(h), self._ct.byref(d), self._ct.byref(seed))
        return int(h.value), float(d.value), int(seed.value)

    def run(self, model: str = "rigid", min_points: int = 3, rank_tol: float = 1e-10, group_lanes: int = 0, d_T: int | None = None,
            stream: int | None = None):
        """Queue the stages (asynchronous; handle-owned outputs, fetched with ``results()``)."""
        self._call("pcs_align_run", self._h, ALIGN_MODEL_IDS[model], int(min_points), float(rank_tol), int(group_lanes), 0, self._addr(d_T), _stream_arg(stream))
        self._own_T = d_T is None

    def results(self):
        """Wait for the last ``run``: (T (P, 3, 4) or None when the run wrote it to a caller buffer, scale (P,), info (P, 4) int32 =
        [rows used, inliers, status, winning hypothesis], stats (P, 3) = [rms, score, conditioning], inlier (n,) bool, dist (n,))."""
        n = self.n_problems
        T = np.empty((n, 3, 4)) if getattr(self, "_own_T", True) else None
        scale, info, stats = np.empty(n), np.empty((n, 4), dtype=np.int32), np.empty((n, 3))
        inl, dist = np.zeros(self.n_rows, dtype=np.uint8), np.empty(self.n_rows)
        self._call("pcs_align_results", self._h, self._ptr(T), self._ptr(scale), self._ptr(info), self._ptr(stats), self._ptr(inl), self._ptr(dist))
        return T, scale, info, stats, inl.astype(bool), dist

    def last_kernel_ms(self) -> dict:
        """Device time of every stage of the last run, milliseconds by stage name (ALIGN_STAGES)."""
        ms = (self._ct.c_float * len(ALIGN_STAGES))()
        self._call("pcs_align_last_kernel_ms", self._h, ms)
        return dict(zip(ALIGN_STAGES, (float(v) for v in ms)))


_align_cache: dict = {}


def _point_aligner(device: int) -> PointAligner:
    return _cached_handle(_align_cache, int(device), lambda: PointAligner(device))


def align_points(src, dst, start_inds=None, *, weights=None, model: str = "rigid", consensus: int = 0, inlier_dist=None, seed: int = 0,
                 min_points: int = 3, rank_tol: float = 1e-10, group_lanes: int = 0, device: int = 0) -> Alignment:
    """Register 3-D point sets on the device (include/pcs_hip.h pcs_align_run): per problem the rotation, translation and, for
    ``model="similarity"``, scale with ``dst ~ scale * R @ src + t`` in the weighted least-squares sense — the reference's
    ``n_estimate_rigid_transform`` (ch:727-762), batched, by Horn's unit-quaternion closed form.

    ``src``, ``dst``: (n, 3) rows sorted by problem with ``start_inds`` (P + 1,), or (P, K, 3) stacks, or one (K, 3) problem
    (``start_inds`` None).  A row with a non-finite coordinate or with weight 0 takes no part.  Planar sets and mirrored destinations
    give proper rotations; collinear ones are refused (``status`` ALIGN_DEGENERATE, ``conditioning`` <= ``rank_tol``).

    ``consensus`` > 0: that many hypotheses of three rows each per problem, scored by sum min(d^2, inlier_dist^2); the fit runs on the
    rows within ``inlier_dist`` (units of dst, required) of the winner.  64 hypotheses find an all-inlier triple at 30 % outliers but for
    a chance of (1 - 0.7^3)^64 = 2e-12.  The sampler is counter-based (``seed``): two calls agree bit for bit."""
    global last_align_kernel_ms
    code, H, dist, seed, min_points, tol, lanes = check_align_options(model, consensus, inlier_dist, seed, min_points, rank_tol, group_lanes)
    x, y = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if x.shape != y.shape or x.ndim not in (2, 3) or x.shape[-1] != 3:
        raise ValueError("expected src and dst of one shape, (n, 3) or (P, K, 3)")
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    if start_inds is None:
        P, K = (1, x.shape[0]) if x.ndim == 2 else x.shape[:2]
        start = np.arange(P + 1, dtype=np.int64) * K
    else:
        if x.ndim != 2:
            raise ValueError("start_inds goes with src and dst (n, 3)")
        start = np.asarray(start_inds, dtype=np.int64)
        if start.ndim != 1 or start.shape[0] < 1 or start[0] != 0 or start[-1] != x.shape[0] or np.any(np.diff(start) < 0):
            raise ValueError("start_inds must run from 0 to n without decreasing")
    x, y = x.reshape(-1, 3), y.reshape(-1, 3)
    if w is not None:
        if w.size != x.shape[0]:
            raise ValueError(f"expected {x.shape[0]} weights, one per row")
        w = w.reshape(-1)
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("weights must be finite and >= 0")
    al = _point_aligner(device)
    al.set_points(x, y, start, w)
    al.set_consensus(H, dist, seed)   # the handle is shared: every call states its setting
    al.run(model=model, min_points=min_points, rank_tol=tol, group_lanes=lanes)
    T, scale, info, stats, inl, d = al.results()
    last_align_kernel_ms = al.last_kernel_ms() if start.shape[0] > 1 else None
    return Alignment(R=T[:, :, :3].copy(), t=T[:, :, 3].copy(), scale=scale, rms=stats[:, 0], status=info[:, 2], n_used=info[:, 0], n_inliers=info[:, 1],
                     inliers=inl, conditioning=stats[:, 2], hypothesis=info[:, 3], score=stats[:, 1], distances=d, start=start)


def register_target(points_by_image, template, **opts):
    """The pose of a known target in every image from 3-D points of its features: ``points_by_image`` (I, K, 3), NaN where a feature
    was not reconstructed, ``template`` (K, 3).  One registration per image over the finite rows (``align_points``; ``opts`` are its
    options: weights (I, K), consensus, inlier_dist, min_points, ...), template -> image points.  -> poses (I, 6) = [rotvec, t], NaN
    where the image's status is not ALIGN_OK.  ``register_target.last`` holds the ``Alignment`` of the last call."""
    from .pose_seeding import pose_from_4x4, to_4x4

    pts, tmpl = np.asarray(points_by_image, dtype=np.float64), np.asarray(template, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[2] != 3 or tmpl.shape != pts.shape[1:]:
        raise ValueError("expected points_by_image (I, K, 3) and template (K, 3)")
    if opts.get("model", "rigid") != "rigid":
        raise ValueError("a target pose is rigid: model must be 'rigid'")
    res = align_points(np.broadcast_to(tmpl, pts.shape), pts, **opts)
    register_target.last = res
    poses = np.full((pts.shape[0], 6), np.nan)
    ok = res.status == ALIGN_OK
    if np.any(ok):
        poses[ok] = pose_from_4x4(to_4x4(np.concatenate([res.R[ok], res.t[ok][:, :, None]], axis=2)))
    return poses


def rig_pose_start_3d(dct, points, intr, ext, n_imgs: int, min_points: int = 6, device: int = 0, consensus: int = 0, inlier_dist=None,
                      seed: int = 0) -> np.ndarray:
    """A start (I, 6) for ``localise_target`` with the signature of ``rig_pose_start``, from 3-D points: every (image, key) feature that
    two or more cameras of the rig see is triangulated (the grouping of ``multi_cam_triangulate``, ``nb_triangulate_full`` with the rig's
    projection matrices), and every image's pose is one registration of the template onto its points (``register_target``): no
    per-view PnP and no planar ambiguity.  NaN where an image has fewer than ``min_points`` triangulated features.  ``consensus`` /
    ``inlier_dist`` (units of the template) / ``seed``: the consensus stage of ``align_points``."""
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    K, E = np.asarray(intr, dtype=np.float64), np.asarray(ext, dtype=np.float64)
    C = K.shape[0]
    Kmat = np.zeros((C, 3, 3))
    Kmat[:, 0, 0], Kmat[:, 0, 2], Kmat[:, 1, 1], Kmat[:, 1, 2], Kmat[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1.0
    by_image = np.full((int(n_imgs), pts.shape[0], 3), np.nan)
    if d.shape[0]:
        rec, start = group_reconstructable(d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))])   # a feature's rows side by side, by camera
        if start.shape[0] > 1:
            X = nb_triangulate_full(rec, Kmat @ E, start, Kmat, K[:, 4:9], device=device)
            head = rec[start[:-1]]
            by_image[head[:, 1].astype(np.int64), head[:, 2].astype(np.int64)] = X
    return register_target(by_image, pts, min_points=max(3, int(min_points)), device=device, consensus=consensus, inlier_dist=inlier_dist, seed=seed)
