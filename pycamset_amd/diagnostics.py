"""After the solve: which camera, image, key or view is bad.

The reference judges a result on the host from a read-back residual vector: one mean (optimisation/optimisation_handling.py:66-70), and,
while seeding, a MAD test on the per-image error (optimisation/template_handler.py:242-279 with utils/general_utils.py:108-133).  Here the
residual stays where the engine wrote it: ``reprojection_report`` evaluates it on the device and runs the per-group statistics of
include/pcs_hip.h ``pcs_stats_*`` (csrc/ba_groupstats.hpp) on that buffer — per camera, per image, per key, per view = (camera, image) and
overall: count, mean, RMS, bias, the worst detection, the exact median and MAD.  ``per_view.rms`` is the counterpart of the
``perViewErrors`` of OpenCV's ``calibrateCameraExtended``, next to the ``stdDeviations*`` that ``device_solver.parameter_covariance`` mirrors.

There is no fallback: without a device the calls raise (``_capi.PcsError``)."""
from __future__ import annotations

import weakref
from dataclasses import dataclass

import numpy as np

from . import _capi
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg

GROUPINGS = tuple(_capi.STATS_GROUPINGS)   # in the order of the device's outputs


def mad_outliers(values, out_thresh: float = 3):
    """The MAD test of utils/general_utils.py:108-133: the indices where ``|v - median| / MAD > out_thresh`` with
    ``MAD = median(|v - median|)``, or ``None`` when there are none.  Two differences from the reference, on purpose: NaN entries are
    ignored (they are neither counted in the medians nor returned); ``MAD == 0`` — more than half of the values equal — returns
    ``None`` where the reference divides by zero and calls every other value an outlier.  Nothing is drawn."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(v)
    if not ok.any():
        return None
    mdn = np.median(v[ok])
    mad = np.median(np.abs(v[ok] - mdn))
    if not mad > 0:
        return None
    with np.errstate(invalid="ignore"):
        found = np.nonzero(ok & (np.abs(v - mdn) / mad > out_thresh))[0]
    return found if found.size else None


def robust_weights(residuals, loss: str = "linear", f_scale: float = 1.0) -> np.ndarray:
    """rho'(z), z = (f / f_scale)^2, per scalar residual f: the weight a robust loss of ``lm_solve``, ``localise_target`` or
    ``refine_triangulation`` gives that residual in J' rho1 f (1 = full weight; scipy ``least_squares``'s rho[1]).  Same shape as
    ``residuals``; NaN stays NaN.  Thresholding it (say < 0.5) lists the detections a solve down-weighted."""
    from .compiled_helpers import check_loss

    loss, f_scale = check_loss(loss, f_scale)
    f = np.asarray(residuals, dtype=np.float64)
    z = (f / f_scale) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "huber":
            w = np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(z))
        elif loss == "soft_l1":
            w = 1.0 / np.sqrt(1.0 + z)
        elif loss == "cauchy":
            w = 1.0 / (1.0 + z)
        elif loss == "arctan":
            w = 1.0 / (1.0 + z * z)
        else:
            w = np.ones_like(z)
    return np.where(np.isnan(f), np.nan, w)


@dataclass
class GroupStats:
    """The statistics of one grouping, one entry per group (``per_view``: shaped (C, I)).  ``count``: detections with a finite error;
    ``n_nonfinite``: the others, which take no part in anything else; ``mean`` / ``rms`` of the error e = |(ru, rv)|; ``bias_u`` /
    ``bias_v``: the mean signed residual; ``max`` and ``argmax``: the worst detection and its table row (-1: none); ``median`` / ``mad``
    of e, exact.  The sums they come from are kept (``sum_e``, ``sum_e2``, ``sum_ru``, ``sum_rv``).  A group without finite detections
    has count 0, argmax -1 and NaN everywhere else."""
    count: np.ndarray
    n_nonfinite: np.ndarray
    mean: np.ndarray
    rms: np.ndarray
    bias_u: np.ndarray
    bias_v: np.ndarray
    max: np.ndarray
    argmax: np.ndarray
    median: np.ndarray
    mad: np.ndarray
    sum_e: np.ndarray
    sum_e2: np.ndarray
    sum_ru: np.ndarray
    sum_rv: np.ndarray

    @classmethod
    def from_sums(cls, count, n_nonfinite, argmax, sum_e, sum_e2, sum_ru, sum_rv, max_e, median, mad, shape=None):
        n = np.where(count > 0, count, 1).astype(np.float64)
        per = lambda s: np.where(count > 0, s / n, np.nan)   # noqa: E731
        out = cls(count=count, n_nonfinite=n_nonfinite, mean=per(sum_e), rms=np.sqrt(per(sum_e2)), bias_u=per(sum_ru), bias_v=per(sum_rv), max=max_e,
                  argmax=argmax, median=median, mad=mad, sum_e=sum_e, sum_e2=sum_e2, sum_ru=sum_ru, sum_rv=sum_rv)
        if shape is not None:
            for name in cls.__dataclass_fields__:
                setattr(out, name, getattr(out, name).reshape(shape))
        return out


class ResidualStats(_Handle):
    """Owner of one ``pcs_residual_stats`` handle (include/pcs_hip.h): the group index of one detection table, built on the device and
    kept across runs, and the outputs of the last run."""

    _create, _destroy = "pcs_stats_create", "pcs_stats_destroy"

    def __init__(self, n_cams: int, n_imgs: int, n_keys: int, device: int = 0):
        super().__init__(device, n_cams, n_imgs, n_keys)
        self.n_cams, self.n_imgs, self.n_keys, self.device = int(n_cams), int(n_imgs), int(n_keys), int(device)
        self.counts = (self.n_cams, self.n_imgs, self.n_keys, self.n_cams * self.n_imgs, 1)
        self.n_groups = sum(self.counts)
        self.n = None          # rows of the table the index was built for
        self.runs = 0          # how many runs this handle has queued: a report knows whether its run is still the last one
        self._table = None     # what reprojection_report bound (see _bind_table)

    def set_groups(self, cam, img, key):
        """Host id columns (n,) of the detection table, in table order; builds the group index on the device."""
        ids = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (cam, img, key)]
        if not ids[0].shape == ids[1].shape == ids[2].shape:
            raise ValueError("cam, img and key must have one entry per detection")
        self.n, self._table = None, None
        self._call("pcs_stats_set_groups", self._h, ids[0].shape[0], *(self._ptr(a) for a in ids))
        self.n = ids[0].shape[0]

    def set_groups_device(self, n: int, d_cam: int, d_img: int, d_key: int):
        """The same from raw device addresses of int32 arrays (n,)."""
        self.n, self._table = None, None
        self._call("pcs_stats_set_groups_device", self._h, int(n), self._addr(d_cam), self._addr(d_img), self._addr(d_key))
        self.n = int(n)

    def run(self, d_resid: int, *, order_statistics: bool = True, d_errors: int | None = None, d_counts: int | None = None, d_values: int | None = None,
            stream: int | None = None):
        """Queue the statistics of the residual buffer at the raw device address ``d_resid`` (2 n float64, [u0, v0, u1, v1, ...]);
        asynchronous, fetch with ``results`` / ``errors``.  ``d_errors`` (n) float64, ``d_counts`` (3, G) int32, ``d_values`` (7, G)
        float64: raw device addresses of the caller's, or None = handle-owned."""
        self._call("pcs_stats_run", self._h, self._addr(d_resid), 0 if order_statistics else _capi.STATS_NO_ORDER_STATISTICS, self._addr(d_errors),
                   self._addr(d_counts), self._addr(d_values), _stream_arg(stream))
        self.runs += 1

    def results(self, grouping: str) -> GroupStats:
        """Wait for the last run and fetch one grouping: 'camera', 'image', 'key', 'view' (shaped (C, I)) or 'overall'."""
        if grouping not in _capi.STATS_GROUPINGS:
            raise ValueError(f"grouping must be one of {list(_capi.STATS_GROUPINGS)}")
        g = _capi.STATS_GROUPINGS[grouping]
        ints = [np.empty(self.counts[g], dtype=np.int32) for _ in range(3)]
        vals = [np.empty(self.counts[g]) for _ in range(7)]
        self._call("pcs_stats_results", self._h, g, *(self._ptr(a) for a in ints + vals))
        return GroupStats.from_sums(*ints, *vals, shape=(self.n_cams, self.n_imgs) if grouping == "view" else None)

    def errors(self) -> np.ndarray:
        """Wait for the last run and fetch the per-detection error e (n,)."""
        e = np.empty(self.n)
        if self.n:
            self._call("pcs_stats_errors", self._h, self._ptr(e))
        return e

    def last_kernel_ms(self):
        """-> (index build, error kernel, statistics) device times of the last ``set_groups*`` and the last ``run``."""
        ms = [self._ct.c_float(0.0) for _ in range(3)]
        self._call("pcs_stats_last_kernel_ms", self._h, *(self._ct.byref(m) for m in ms))
        return tuple(float(m.value) for m in ms)

    # -- which table the index holds (reprojection_report) -------------------------------------------------------------------------
    def _bind_table(self, det: np.ndarray):
        """Build the index for the id columns of ``det`` (N, 5) unless it is the table the index already holds: the same array object
        (a live weak reference) with the same sampled rows, or equal id columns."""
        sample = det[:: max(1, det.shape[0] // 256), :3].tobytes()
        held = self._table
        if held is not None and held[0]() is det and held[1] == sample:
            return
        ids = np.ascontiguousarray(det[:, :3].T, dtype=np.int32)
        digest = hash(ids.tobytes())
        if held is None or held[2] != digest or self.n != det.shape[0]:
            self.set_groups(ids[0], ids[1], ids[2])
        try:
            ref = weakref.ref(det)
        except TypeError:
            ref = lambda: None   # noqa: E731
        self._table = (ref, sample, digest)


_stats_cache: dict = {}


def _residual_stats(device: int, n_cams: int, n_imgs: int, n_keys: int) -> ResidualStats:
    return _cached_handle(_stats_cache, (int(device), int(n_cams), int(n_imgs), int(n_keys)), lambda: ResidualStats(n_cams, n_imgs, n_keys, device))


class CalibrationReport:
    """What ``reprojection_report`` returns: ``overall``, ``per_camera``, ``per_image``, ``per_key`` and ``per_view`` (shaped (C, I), NaN
    where a view has no detection) are ``GroupStats``; ``n`` is the number of detections.  ``per_view.rms`` is the counterpart of OpenCV's
    ``perViewErrors``, ``overall.mean`` that of ``optimisation_handling.mean_reprojection_error``."""

    def __init__(self, stats: ResidualStats):
        self._stats, self._run, self._errors = stats, stats.runs, None
        self.n = stats.n
        self.per_camera, self.per_image, self.per_key, self.per_view, self.overall = (stats.results(g) for g in GROUPINGS)
        self.kernel_ms = dict(zip(("index", "error", "statistics"), stats.last_kernel_ms()))

    def errors(self) -> np.ndarray:
        """The per-detection error e (n,) in table order, fetched from the device on first use — which has to happen before the next
        report of the same table sizes reuses the handle."""
        if self._errors is None:
            if self._stats.runs != self._run:
                raise RuntimeError("the device buffer of this report's errors has been reused by a later report: call errors() before the next one")
            self._errors = self._stats.errors()
        return self._errors

    def worst(self, n: int = 10) -> np.ndarray:
        """The table rows of the ``n`` detections of largest finite error, worst first (equal errors: the lower row first)."""
        e = self.errors()
        rows = np.nonzero(np.isfinite(e))[0]
        return rows[np.argsort(-e[rows], kind="stable")[: max(0, int(n))]]

    def outlier_images(self, out_thresh: float = 20):
        """The images whose mean error fails the MAD test (``mad_outliers``) at the threshold of template_handler.py:262, or None.
        Images without detections are ignored.  The reference tests the per-image SUM of the errors while seeding
        (template_handler.py:535-560), which grows with the number of detections of an image; this is the mean."""
        return mad_outliers(self.per_image.mean, out_thresh)

    def outlier_views(self, out_thresh: float = 20):
        """The views (k, 2) = [camera, image] whose mean error fails the MAD test over all views with detections, or None."""
        found = mad_outliers(self.per_view.mean, out_thresh)
        return None if found is None else np.stack(np.unravel_index(found, self.per_view.mean.shape), axis=1)


def reprojection_report(handler, x, *, device: int | None = None) -> CalibrationReport:
    """The reprojection statistics of ``handler`` (a bundle handler or a ``ChainProblem``) at the free vector ``x``: the residual is
    evaluated on the device into the engine's own buffer and the statistics run on that buffer — no residual is read back.  The engine
    has to compute in float64 (``dtype='f64'``).  ``device``: the handler's (the default); naming another one is an error, the residual
    lives where the engine is."""
    op = handler.op_fun
    det = handler._flat_detections()
    eng = op._engine_for(det)
    if device is not None and int(device) != int(eng.device):
        raise ValueError(f"the handler's engine is on device {eng.device}, not {device}")
    if eng.dtype != "f64":
        raise ValueError("reprojection_report needs float64 residuals on the device: build the handler with dtype='f64'")
    op._bind_template(eng, handler._template_arg())
    p = eng._check_params(op._leading(op.build_param_list(*handler.get_bundle_adjustment_inputs(np.asarray(x, dtype=np.float64))), eng))
    d_resid = _capi.c_void_p()
    if hasattr(eng, "spec"):   # a generated chain: its evaluation takes the parameter string on the device
        import torch

        _capi.check(_capi.lib().pcs_genchain_device_buffers(eng._h, _capi.ctypes.byref(d_resid), None))
        d_param = torch.from_numpy(p).to(f"cuda:{int(eng.device)}")
        eng.eval_device(d_param.data_ptr(), d_resid.value, None)
    else:
        _capi.check(_capi.lib().pcs_device_buffers(eng._h, _capi.ctypes.byref(d_resid), None))
        eng.eval_device(p, d_resid.value, None)
    eng.synchronize()   # the statistics run on their own stream
    det = np.asarray(det)
    # the free chain's engine has no image group: there the images are counted off the table
    n_imgs = eng.n_imgs or (int(det[:, 1].max()) + 1 if det.shape[0] else 1)
    stats = _residual_stats(eng.device, eng.n_cams, n_imgs, eng.n_keys)
    stats._bind_table(det)
    stats.run(d_resid.value)
    return CalibrationReport(stats)
