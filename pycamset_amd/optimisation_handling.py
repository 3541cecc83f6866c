"""The caller of the path, kept in Python like the reference
(pyCamSet optimisation/optimisation_handling.py:24-117).

``make_optimisation_function`` returns the handler's two closures plus the start vector;
``run_bundle_adjustment`` feeds them to ``scipy.optimize.least_squares`` with the reference's
keyword arguments (jac = the CSR closure, ``x_scale='jac'``, ``max_nfev`` and ``verbose`` from the
handler's options, oh:88-98).  The reference finishes by rebuilding a ``CameraSet`` (oh:109); that
data model is outside the accelerated path, so the full parameter slabs at the solution are
returned instead.  ``solver='device'`` swaps scipy for ``device_solver.lm_solve`` (the Jacobian never
leaves the GPU).
"""
from __future__ import annotations

import logging
import time

import numpy as np
from scipy.optimize import least_squares

log = logging.getLogger(__name__)


def mean_reprojection_error(residuals: np.ndarray) -> float:
    """Mean Euclidean pixel error of a flat residual vector [u0, v0, u1, v1, ...] (the figure the
    reference logs before and after the solve, oh:66-70, oh:101-103)."""
    uv = np.asarray(residuals, dtype=np.float64).reshape(-1, 2)
    return float(np.hypot(uv[:, 0], uv[:, 1]).mean())


def make_optimisation_function(param_handler, threads: int = 1):
    """(loss_fn, jac_fn | None, x0) — oh:24-49."""
    x0 = param_handler.get_initial_params()
    loss_fn = param_handler.make_loss_fun(threads)
    jac_fn = param_handler.make_loss_jac(threads) if param_handler.can_make_jac() else None
    return loss_fn, jac_fn, x0


def _with_prior_rows(loss_fn, jac_fn, prior):
    """The closures of the augmented problem: residual rows ``w (x - mean)`` behind the detections' and the matching diagonal rows
    behind the Jacobian's, for the entries with w = 1 / sigma > 0."""
    from scipy.sparse import csr_array, vstack

    mean, w = prior
    idx = np.flatnonzero(w > 0.0)
    rows = csr_array((w[idx], (np.arange(idx.shape[0]), idx)), shape=(idx.shape[0], w.shape[0]))

    def fun(x):
        return np.concatenate([loss_fn(x), w[idx] * (x[idx] - mean[idx])])

    def jac(x):
        return vstack([jac_fn(x), rows], format="csr")

    return fun, (jac if jac_fn is not None else None)


def run_bundle_adjustment(param_handler, threads: int = 1, solver: str = "scipy", linear_solver: str = "auto"):
    """Solve the handler's problem; returns (result, parameter slabs at the solution) — oh:52-117.
    ``solver='device'`` runs device_solver.lm_solve with ``linear_solver`` in {'auto', 'cholesky', 'pcg'}.
    Optional ``problem_opts['loss']`` / ``['f_scale']`` (scipy's names, default 'linear' / 1.0 — the reference's call carries the
    commented ``# loss = "cauchy"``, oh:96) go to whichever solver runs.  Optional ``problem_opts['prior'] = (mean, sigma)``: a
    Gaussian prior on the free vector (``device_solver.lm_solve``'s ``prior_mean`` / ``prior_sigma``; ``handlers.slab_prior`` builds
    one).  The device solver takes it as it is; for scipy the rows ``(x - mean) / sigma`` are appended to the residual closure and the
    matching diagonal rows to the Jacobian closure, so both solvers minimise the same function — with the linear loss: scipy's robust
    losses would apply to the appended rows too.  Optional ``problem_opts['bounds']``: box bounds on the free vector in scipy's forms
    (``(lo, hi)`` or a ``scipy.optimize.Bounds``; ``handlers.slab_bounds`` builds the arrays), handed to whichever solver runs:
    ``lm_solve(bounds=)`` or ``least_squares(bounds=)``."""
    loss_fn, jac_fn, x0 = make_optimisation_function(param_handler, threads)
    opts = param_handler.problem_opts
    loss, f_scale = opts.get("loss", "linear"), opts.get("f_scale", 1.0)
    prior = None
    if opts.get("prior") is not None:
        from .device_solver import _free_prior

        prior_mean, prior_sigma = opts["prior"]
        prior = _free_prior(x0, prior_mean, prior_sigma)
    bounds = opts.get("bounds")
    if bounds is not None:
        from .device_solver import _free_bounds

        _free_bounds(x0, bounds)   # shapes, values and the start, checked the same way for both solvers
    n_rows = 2 * param_handler._flat_detections().shape[0]
    start_error = mean_reprojection_error(loss_fn(x0))
    log.info("%d parameters, %d residuals, start error %.2f px", len(x0), 2 * param_handler._flat_detections().shape[0], start_error)
    if not np.isfinite(start_error) or start_error > 150:  # the reference's sanity threshold (oh:80-83)
        log.critical("start error is very high or not finite: check the initial parameters")
    tic = time.perf_counter()
    if solver == "device":
        from .device_solver import lm_solve

        result = lm_solve(param_handler, x0, max_iter=opts["max_nfev"], linear_solver=linear_solver, loss=loss, f_scale=f_scale,
                          **({} if prior is None else {"prior_mean": prior_mean, "prior_sigma": prior_sigma}),
                          **({} if bounds is None else {"bounds": bounds}))
        end_error = mean_reprojection_error(loss_fn(result.x))
    else:
        fun, jac = loss_fn, jac_fn
        if prior is not None:
            if loss != "linear":
                raise NotImplementedError("problem_opts['prior'] with solver='scipy' and a robust loss: scipy would pass the prior rows "
                                          "through the loss (solver='device' keeps them outside it)")
            fun, jac = _with_prior_rows(loss_fn, jac_fn, prior)
        result = least_squares(fun, x0, jac=jac if jac is not None else "2-point", x_scale="jac",
                               max_nfev=opts["max_nfev"], verbose=opts["verbosity"], loss=loss, f_scale=f_scale,
                               **({} if bounds is None else {"bounds": bounds}))
        end_error = mean_reprojection_error(result.fun[:n_rows])
    log.info("solved in %.2f s, final error %.2f px", time.perf_counter() - tic, end_error)
    if end_error > 5:  # oh:105-107
        log.critical("remaining error is very large: check the result")
    slabs = tuple(np.array(a) for a in param_handler.get_bundle_adjustment_inputs(result.x))
    return result, slabs
