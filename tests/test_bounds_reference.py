"""tests/bounds_reference.py pinned on the CPU: its two pieces on small cases by hand, the whole loop against scipy's bounded
least_squares on the oracle closures of ring-4 with the boxes the GPU tests use, and the CPU side of lm_solve(bounds=): argument
checking, handlers.slab_bounds and the hand-over of problem_opts["bounds"] to scipy."""
import numpy as np
import pytest
from scipy.optimize import Bounds, least_squares

from tests import bounds_reference as BR


def test_active_set_by_hand():
    x = np.array([0.0, 0.0, 1.0, 1.0, 0.5, 2.0, 0.0])
    lo = np.array([0.0, 0.0, -np.inf, -np.inf, 0.0, 2.0, 0.0])
    hi = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0])
    g = np.array([1.0, -1.0, -1.0, 1.0, 5.0, 0.0, 1.0])
    fixed = np.array([0, 0, 0, 0, 0, 0, 1], bool)
    eff, n = BR.active_set(x, g, lo, hi, fixed)
    # lower bound + gradient out | lower + in | upper + out | upper + in | interior | lo == hi | user-fixed and on a bound
    assert eff.tolist() == [True, False, True, False, False, True, True] and n == 3
    eff, n = BR.active_set(x, g, lo, hi, fixed, pin=np.array([0, 1, 0, 0, 1, 0, 0], bool))
    assert eff.tolist() == [True, True, True, False, False, True, True] and n == 4      # a pin holds an entry ON a bound only


def test_truncate_by_hand():
    x = np.array([0.0, 0.0, 0.0, 1.0])
    lo, hi = np.full(4, -1.0), np.array([np.inf, 0.25, 0.5, 1.0])
    alpha, hit, xn, delta = BR.truncate(x, np.array([1.0, 1.0, 2.0, 0.0]), lo, hi)
    assert alpha == 0.25 and hit == 1                                                    # 0.25 / 1 and 0.5 / 2 tie: the lower index
    assert xn.tolist() == [0.25, 0.25, 0.5, 1.0] and delta.tolist() == [0.25, 0.25, 0.5, 0.0]
    alpha, hit, xn, delta = BR.truncate(x, np.array([1.0, 0.125, -0.5, 0.5]), lo, hi)    # the last entry sits on its bound and steps out: pinned
    assert alpha == 1.0 and hit == -1 and xn.tolist() == [1.0, 0.125, -0.5, 1.0] and delta.tolist() == [1.0, 0.125, -0.5, 0.0]
    d = np.array([0.3, -0.7, 0.1, -0.2])
    alpha, hit, xn, delta = BR.truncate(x, d, np.full(4, -np.inf), np.full(4, np.inf))
    assert alpha == 1.0 and np.array_equal(delta, d) and np.array_equal(xn, x + d)


def test_predicted_reduction_is_the_model_decrease_of_the_cut_step():
    rng = np.random.default_rng(0)
    J = rng.standard_normal((30, 6))
    H, g = J.T @ J, J.T @ rng.standard_normal(30)
    lam, D = 0.3, np.diag(J.T @ J)
    d = np.linalg.solve(H + lam * np.diag(D), -g)
    for alpha in (1.0, 0.4, 0.01):
        delta = alpha * d
        model = -(g @ delta) - 0.5 * delta @ H @ delta
        assert abs(BR.predicted_reduction(lam, D, g, delta, alpha) - model) <= 1e-12 * abs(model)
    from tests import lm_reference as LR
    assert BR.predicted_reduction(lam, D, g, d, 1.0) == pytest.approx(LR.predicted_reduction(lam, D, g, d), rel=1e-15)


@pytest.mark.parametrize("chain", BR.CHAINS)
def test_reference_loop_matches_scipy_with_the_designed_active_set(chain):
    p = BR.problem(chain)
    assert np.all(p.x0 >= p.lo) and np.all(p.x0 <= p.hi)
    ref = least_squares(p.fun, p.x0_interior, jac=p.jac, bounds=(p.lo, p.hi), x_scale="jac", method="trf", max_nfev=BR.SCIPY_NFEV)
    res = BR.solve(p.fun, p.jac, p.x0, p.lo, p.hi, max_iter=BR.SOLVE_ITERS)
    print(chain, ref.status, ref.cost, ref.nfev, res.status, res.cost, len(res.trials), res.n_truncated)
    assert ref.status > 0 and res.status in (1, 3, 4)
    assert np.array_equal(ref.active_mask, p.designed_mask) and np.array_equal(res.active_mask, p.designed_mask)
    assert res.cost <= ref.cost * (1 + 1e-3), (res.cost, ref.cost)
    assert np.all(res.x >= p.lo) and np.all(res.x <= p.hi)
    assert res.n_truncated >= 1 and res.history == sorted(res.history, reverse=True)
    # the bounds bind clearly: the gradient on either of them, in units of its column's norm, is far above the loop's tolerances
    J = p.jac(res.x).toarray()
    k = np.flatnonzero(p.designed_mask)
    assert np.all(np.abs(res.grad[k]) / np.linalg.norm(J[:, k], axis=0) > 1e-3)
    short = BR.solve(p.fun, p.jac, p.x0, p.lo, p.hi, max_iter=BR.TRIAL_ITERS, lam0=p.lam0)
    assert any(t["alpha"] < 1.0 for t in short.trials) and any(t["n_active"] > 0 for t in short.trials)   # what the trial-by-trial GPU test compares


def test_lm_solve_checks_bounds_before_any_device_work():
    from pycamset_amd.device_solver import _free_bounds, _string_bounds
    x0 = np.array([0.0, 1.0, 2.0])
    assert _free_bounds(x0, None) is None and _free_bounds(x0, (-np.inf, np.inf)) is None
    lo, hi = _free_bounds(x0, (-1.0, [1.0, np.inf, 3.0]))
    assert lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0, np.inf, 3.0]
    lo, hi = _free_bounds(x0, Bounds([-1, -1, -1], [5, 5, 5]))
    assert hi.tolist() == [5.0] * 3
    with pytest.raises(ValueError, match=r"`x0` is infeasible: x0\[2\]"):
        _free_bounds(x0, (-1.0, 1.5))
    with pytest.raises(ValueError, match="index 1"):
        _free_bounds(x0, ([-1, 3, -1], [5, 2, 5]))
    with pytest.raises(ValueError, match="NaN at index 0"):
        _free_bounds(x0, ([np.nan, 0, 0], 5.0))
    with pytest.raises(ValueError, match="2 values for 3"):
        _free_bounds(x0, ([0.0, 0.0], 5.0))
    with pytest.raises(ValueError, match="bounds must be"):
        _free_bounds(x0, 3.0)
    mask = np.array([True, False, True, True, False])
    slo, shi = _string_bounds(mask, (np.array([-1.0, -2.0, -3.0]), np.array([1.0, 2.0, 3.0])))
    assert slo.tolist() == [-1.0, -np.inf, -2.0, -3.0, -np.inf] and shi.tolist() == [1.0, np.inf, 2.0, 3.0, np.inf]
    with pytest.raises(ValueError, match="free parameters"):
        _string_bounds(mask, (np.zeros(2), np.ones(2)))


def test_slab_bounds_per_group():
    from pycamset_amd import handlers
    from tests import weights_reference as W
    rig, h, x0 = W.ring4_handler("template")
    h.bundlePrimitive.intr[:] = rig.intr                     # ("rel", width) is measured around the handler's current slab
    lo, hi = handlers.slab_bounds(h, {"intr": np.r_[900.0, np.full(8, -np.inf)], "pose": None}, {"intr": ("rel", 0.1), "extr": 10.0})
    assert lo.shape == hi.shape == x0.shape
    C = rig.n_cams
    assert np.all(lo[0: 9 * C: 9] == 900.0) and np.all(np.isinf(lo[1: 9 * C: 9]))
    start = h.bundlePrimitive.intr[h.bundlePrimitive.intr_unfixed].ravel()
    assert np.allclose(hi[: 9 * C], start + 0.1 * np.abs(start))
    assert np.all(hi[9 * C: 9 * C + 6 * (C - 1)] == 10.0) and np.all(np.isinf(hi[9 * C + 6 * (C - 1):])) and np.all(np.isinf(lo[9 * C:]))
    with pytest.raises(ValueError, match="unknown parameter groups"):
        handlers.slab_bounds(h, {"lens": 0.0}, None)


def test_problem_opts_bounds_reach_scipy(monkeypatch):
    from pycamset_amd import optimisation_handling as oh
    from tests import weights_reference as W
    rig, h, x0 = W.ring4_handler("template")
    fun, jac = W.oracle_closures(h, "template", rig.points)            # (the handler's own closures run on the device)
    monkeypatch.setattr(oh, "make_optimisation_function", lambda handler, threads: (fun, jac, x0))
    n = x0.shape[0]
    seen = {}
    real = oh.least_squares

    def spy(fun, x0, **kw):
        seen.update(kw)
        return real(fun, x0, **kw)

    monkeypatch.setattr(oh, "least_squares", spy)
    hi = np.full(n, np.inf)
    hi[0] = 1e6
    h.problem_opts = dict(h.problem_opts, max_nfev=2, bounds=(-np.inf, hi))
    res, _ = oh.run_bundle_adjustment(h, solver="scipy")
    assert seen["bounds"][0] == -np.inf and np.array_equal(seen["bounds"][1], hi) and res.x[0] <= 1e6
    h.problem_opts = dict(h.problem_opts, bounds=(-np.inf, -1e6))
    with pytest.raises(ValueError, match="infeasible"):
        oh.run_bundle_adjustment(h, solver="scipy")
