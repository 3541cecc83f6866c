"""The Gaussian parameter prior (include/pcs_hip.h pcs_set_prior; lm_solve(prior_mean=, prior_sigma=)) as far as it is decided without a
device: the C ABI's symbols and NULL-handle checks, the argument checks of the Python layer, the host-operator paths of lm_solve against
scipy on the augmented closures of tests/prior_reference.py, handlers.slab_prior, the gauge option of SelfBundleHandler and the scipy
branch of run_bundle_adjustment."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import least_squares

from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests import prior_reference as PR
from tests import weights_reference as W
from tests.test_capi_symbols import declared_symbols
from tests.test_host_logic import DuckCamset, DuckTarget
from tests.test_robust_loss import _Untouchable, _cpu_problem

PRIOR_SYMBOLS = ("pcs_set_prior", "pcs_get_prior", "pcs_prior_add_device", "pcs_genchain_set_prior", "pcs_genchain_get_prior", "pcs_genchain_prior_add_device")


def test_prior_symbols_and_null_handles():
    lib = _capi.lib()
    for name in PRIOR_SYMBOLS:
        assert name in declared_symbols() and name in _capi.SYMBOLS and hasattr(lib, name), name
    assert lib.pcs_version() >= 114
    v = np.ones(3)
    dp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    n = ctypes.c_int64(0)
    for prefix in ("pcs_", "pcs_genchain_"):
        assert getattr(lib, prefix + "set_prior")(None, dp, dp, 3) == _capi.PCS_ERR_ARG
        assert (prefix + "set_prior").encode() in lib.pcs_last_error()
        assert getattr(lib, prefix + "set_prior")(None, None, None, 0) == _capi.PCS_ERR_ARG
        assert getattr(lib, prefix + "get_prior")(None, dp, dp, 3, ctypes.byref(n)) == _capi.PCS_ERR_ARG
        assert getattr(lib, prefix + "prior_add_device")(None, None, None, None) == _capi.PCS_ERR_ARG
        assert (prefix + "prior_add_device").encode() in lib.pcs_last_error()


def test_bad_priors_raise_before_any_device_work():
    from pycamset_amd.device_solver import lm_solve, parameter_covariance
    from pycamset_amd.engine import prior_arrays
    x0 = np.zeros(5)
    bad = [dict(prior_sigma=np.ones(4)),                                   # a wrong length
           dict(prior_sigma=np.ones(5), prior_mean=np.zeros(6)),
           dict(prior_sigma=np.array([1.0, 1.0, 0.0, 1.0, 1.0])),          # sigma <= 0
           dict(prior_sigma=np.array([1.0, -2.0, 1.0, 1.0, 1.0])),
           dict(prior_sigma=np.array([1.0, np.nan, 1.0, 1.0, 1.0])),       # NaN
           dict(prior_sigma=np.ones(5), prior_mean=np.array([0.0, np.nan, 0.0, 0.0, 0.0])),
           dict(prior_mean=np.zeros(5))]                                   # a mean without sigma
    for kw in bad:
        with pytest.raises(ValueError, match="prior"):
            lm_solve(_Untouchable(), x0, **kw)
        with pytest.raises(ValueError, match="prior"):
            lm_solve(_Untouchable(), x0, operator=_Untouchable(), linear_solver="pcg", **kw)
        with pytest.raises(ValueError, match="prior"):
            parameter_covariance(_Untouchable(), x0, **kw)
    with pytest.raises(ValueError, match="prior_mean"):                    # the covariance's variance of unit weight needs the mean
        parameter_covariance(_Untouchable(), x0, prior_sigma=np.ones(5))
    # a NaN mean is fine where sigma is inf: no prior there
    assert PR.weights_of([np.inf, 2.0])[0] == 0.0
    m, w = prior_arrays(3, [np.nan, 1.0, 2.0], sigma=[np.inf, 0.5, np.inf])
    assert np.array_equal(w, [0.0, 2.0, 0.0]) and np.array_equal(m, [0.0, 1.0, 0.0])
    assert prior_arrays(3, None) == (None, None)
    for kw in (dict(sigma=np.ones(2)), dict(sigma=[1.0, 0.0, 1.0]), dict(inv_sigma=[1.0, -1.0, 1.0]), dict(inv_sigma=[1.0, np.inf, 1.0]),
               dict(sigma=np.ones(3), inv_sigma=np.ones(3))):
        with pytest.raises(ValueError):
            prior_arrays(3, np.zeros(3), **kw)
    with pytest.raises(ValueError):
        prior_arrays(3, [0.0, np.inf, 0.0], sigma=np.ones(3))


@pytest.fixture(scope="module")
def cpu_problem():
    """ring-4, template chain, a CPU operator (test_robust_loss._cpu_problem), the oracle's closures, a prior on the intrinsics' distortion
    terms and on every pose translation (the rest: np.inf), and scipy's solution of the augmented problem — computed once."""
    h, x0, op = _cpu_problem()
    rig = W.ring4()
    fun, jac = W.oracle_closures(h, "template", rig.points)
    sig = {"intr": np.r_[np.full(4, np.inf), np.full(5, 0.02)], "pose": np.r_[np.full(3, np.inf), np.full(3, 5.0)]}
    mean, sigma = handlers.slab_prior(h, sig)
    rng = np.random.default_rng(4)
    mean = mean + np.where(np.isinf(sigma), 0.0, sigma) * rng.standard_normal(mean.shape)      # the knowledge is off by about one sigma
    w = PR.weights_of(sigma)
    fa, ja, n_prior = PR.augmented_closures(fun, jac, mean, w)
    ref = least_squares(fa, x0.copy(), jac=ja, x_scale="jac", max_nfev=60)
    return dict(h=h, x0=x0, op=op, fun=fun, jac=jac, mean=mean, sigma=sigma, w=w, fa=fa, ja=ja, n_prior=n_prior, ref=ref, rig=rig)


def _check_against_scipy(res, p):
    """The rule of the existing solve tests (test_lm_solve_reaches_the_scipy_solution_on_the_reduced_parameters)."""
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost <= p["ref"].cost * (1 + 1e-3), (res.cost, p["ref"].cost)
    assert abs(0.5 * np.sum(p["fa"](res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    assert abs(res.prior_cost - PR.prior_half_sum(res.x, p["mean"], p["w"])) <= 1e-12 * max(res.prior_cost, 1e-300)
    assert 0.0 < res.prior_cost < res.cost


def test_pcg_through_a_host_operator_matches_scipy_on_the_augmented_closures(cpu_problem):
    from pycamset_amd.device_solver import lm_solve
    p = cpu_problem
    assert p["n_prior"] == 5 * 4 + 3 * 5 and p["ref"].cost > 0
    res = lm_solve(p["h"], p["x0"].copy(), max_iter=40, operator=p["op"], linear_solver="pcg", prior_mean=p["mean"], prior_sigma=p["sigma"])
    _check_against_scipy(res, p)
    g = p["ja"](res.x).T @ p["fa"](res.x)
    assert np.max(np.abs(res.grad - g)) <= 1e-9 * np.max(np.abs(p["ja"](res.x)).T @ np.abs(p["fa"](res.x)))
    # without the prior the same operator solves the plain problem: another minimum, no prior cost
    plain = lm_solve(p["h"], p["x0"].copy(), max_iter=40, operator=p["op"], linear_solver="pcg")
    assert plain.prior_cost == 0.0 and abs(0.5 * np.sum(p["fun"](plain.x) ** 2) - plain.cost) <= 1e-9 * plain.cost
    assert plain.cost < res.cost - res.prior_cost + 1e-9 * res.cost          # the prior can only raise the data term
    # prior_mean defaults to x0
    pull = lm_solve(p["h"], p["x0"].copy(), max_iter=3, operator=p["op"], linear_solver="pcg", prior_sigma=p["sigma"])
    assert abs(pull.prior_cost - PR.prior_half_sum(pull.x, p["x0"], p["w"])) <= 1e-12 * pull.prior_cost


def test_cholesky_through_a_host_operator_matches_scipy_on_the_augmented_closures(cpu_problem):
    import torch
    from pycamset_amd.device_solver import lm_solve
    from tools.library_solver import cholesky_step
    p = cpu_problem
    mask = np.asarray(p["h"]._jac_mask(), bool)
    eng = p["op"].eng

    class CpuNormal:
        free = np.flatnonzero(mask)

        def build(self, ps):
            eng.linearize(ps)
            Jf = eng.J[:, self.free]
            return torch.from_numpy((Jf.T @ Jf).toarray()), torch.from_numpy(Jf.T @ eng.r), float(eng.r @ eng.r)

        solve = staticmethod(cholesky_step)

    res = lm_solve(p["h"], p["x0"].copy(), max_iter=40, operator=CpuNormal(), prior_mean=p["mean"], prior_sigma=p["sigma"])
    assert res.n_jtjv <= res.nfev + 12                                       # factorisations, not CG products ("auto" saw build())
    _check_against_scipy(res, p)
    # the normal system the wrapped operator hands the step is prior_system of the plain one
    from pycamset_amd.device_solver import _PriorOperator
    ps = p["h"].op_fun.build_param_list(*p["h"].get_bundle_adjustment_inputs(p["x0"]))
    H0, g0, c0 = CpuNormal().build(ps)
    H1, g1, c1 = _PriorOperator(CpuNormal(), CpuNormal.free, (p["mean"], p["w"])).build(ps)
    Hr, gr, cr = PR.prior_system(H0.numpy(), g0.numpy(), c0, p["x0"], p["mean"], p["w"])
    assert np.array_equal(H1.numpy(), Hr) and np.allclose(g1.numpy(), gr, rtol=1e-15, atol=0) and abs(c1 - cr) <= 1e-15 * cr
    with pytest.raises(ValueError, match="free parameters"):
        lm_solve(p["h"], p["x0"][:-1].copy(), max_iter=2, operator=CpuNormal(), prior_sigma=np.ones(p["x0"].shape[0] - 1))


def _self_handler(options=None, det=None):
    rig = W.ring4()
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    return rig, handlers.SelfBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections if det is None else det),
                                           fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options=dict({"verbosity": 0}, **(options or {})))


def test_slab_prior_follows_the_masks():
    rig, h, x0 = W.ring4_handler("template")
    bp = h.bundlePrimitive
    C, I = rig.n_cams, rig.n_imgs
    assert not bp.extr_unfixed[0] and not bp.poses_unfixed[0]                # the fixed camera, the fixed pose
    row = np.arange(1.0, 10.0)
    per_pose = 10.0 * np.arange(1, I + 1)[:, None]
    mean, sigma = handlers.slab_prior(h, {"intr": row, "extr": 0.5, "pose": per_pose})
    assert mean.shape == sigma.shape == x0.shape
    assert np.array_equal(sigma[: 9 * C].reshape(C, 9), np.tile(row, (C, 1)))
    assert np.array_equal(sigma[9 * C: 9 * C + 6 * (C - 1)], np.full(6 * (C - 1), 0.5))       # camera 0 has no row
    assert np.array_equal(sigma[9 * C + 6 * (C - 1):].reshape(I - 1, 6), np.repeat(per_pose[1:], 6, axis=1))   # nor pose 0
    # the mean defaults to the handler's current slabs, in free-vector order
    cur = np.concatenate([bp.intr[bp.intr_unfixed].ravel(), bp.extr[bp.extr_unfixed].ravel(), bp.poses[bp.poses_unfixed].ravel()])
    assert np.array_equal(mean, cur)
    m2, s2 = handlers.slab_prior(h, {"intr": 1.0}, {"intr": rig.intr})
    assert np.array_equal(m2[: 9 * C], rig.intr.ravel()) and np.all(np.isinf(s2[9 * C:])) and np.all(s2[: 9 * C] == 1.0)
    with pytest.raises(ValueError, match="bdpt"):
        handlers.slab_prior(h, {"bdpt": 1.0})                                 # the template chain has no free points
    with pytest.raises(ValueError, match="broadcast"):
        handlers.slab_prior(h, {"intr": np.ones(4)})
    with pytest.raises(ValueError, match="> 0"):
        handlers.slab_prior(h, {"intr": 0.0})

    rig, hs = _self_handler()
    bps = hs.bundlePrimitive
    n_pt = int(bps.bdpt_unfixed.sum())
    assert n_pt < 3 * rig.n_keys                                              # the gauge scalars (and unseen features) are fixed
    per_coord = np.tile([0.05, 0.05, 0.2], rig.n_keys)
    mean, sigma = handlers.slab_prior(hs, {"bdpt": per_coord.reshape(-1, 3)})
    assert np.all(np.isinf(sigma[:-n_pt])) and np.array_equal(sigma[-n_pt:], per_coord[bps.bdpt_unfixed])     # the per-scalar mask
    assert np.array_equal(mean[-n_pt:], rig.points.ravel()[bps.bdpt_unfixed])                                # the nominal target
    hs.get_bundle_adjustment_inputs(np.full(mean.shape, 7.0))                 # a solve scatters its iterates into the primitive's slabs ...
    assert np.array_equal(handlers.slab_prior(hs, {"bdpt": 0.05})[0][-n_pt:], rig.points.ravel()[bps.bdpt_unfixed])   # ... the nominal mean stays

    # a ChainProblem: a list per slab
    from pycamset_amd import function_blocks as fb
    op = fb.projection() + fb.extrinsic3D() + fb.template_points()
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, rig.poses], template=rig.points, unfixed=[None, fix_ext, None])
    mean, sigma = handlers.slab_prior(prob, [row, None, 2.0])
    assert np.array_equal(mean, prob.x0) and sigma.shape == prob.x0.shape
    assert np.array_equal(sigma[: 9 * C].reshape(C, 9), np.tile(row, (C, 1))) and np.all(np.isinf(sigma[9 * C: 9 * C + 6 * (C - 1)]))
    assert np.all(sigma[9 * C + 6 * (C - 1):] == 2.0)
    with pytest.raises(ValueError, match="per slab"):
        handlers.slab_prior(prob, [row, None])


def test_gauge_free_frees_exactly_the_seven_gauge_scalars():
    rig, fixed = _self_handler()
    _, explicit = _self_handler({"gauge": "fixed"})
    _, free = _self_handler({"gauge": "free"})
    assert np.array_equal(fixed.bundlePrimitive.bdpt_unfixed, explicit.bundlePrimitive.bdpt_unfixed)
    assert np.array_equal(fixed._jac_mask(), explicit._jac_mask())
    i0, i1, i2 = fixed.fixed_inds
    gauge = np.r_[3 * i0 + np.arange(3), 3 * i1 + np.arange(3), 3 * i2]
    # today's mask: the seven scalars and the unseen features, nothing else
    expect = np.ones(3 * rig.n_keys, bool)
    expect[gauge] = False
    expect[np.repeat(~fixed.visible_feature_mask, 3)] = False
    assert np.array_equal(fixed.bundlePrimitive.bdpt_unfixed, expect)
    diff = np.flatnonzero(free.bundlePrimitive.bdpt_unfixed != fixed.bundlePrimitive.bdpt_unfixed)
    seen_gauge = gauge[np.repeat(fixed.visible_feature_mask, 3)[gauge]]
    assert np.array_equal(diff, np.sort(seen_gauge)) and diff.size == 7 and np.all(free.bundlePrimitive.bdpt_unfixed[diff])
    assert free._jac_mask().sum() == fixed._jac_mask().sum() + 7
    # unseen features stay fixed: drop every detection of two keys
    det = rig.detections[~np.isin(rig.detections[:, 2], [5, 11])]
    _, part = _self_handler({"gauge": "free"}, det)
    m = part.bundlePrimitive.bdpt_unfixed.reshape(-1, 3)
    assert not m[5].any() and not m[11].any() and m[np.setdiff1d(np.arange(rig.n_keys), [5, 11])].all()
    with pytest.raises(ValueError, match="gauge"):
        _self_handler({"gauge": "loose"})


def test_run_bundle_adjustment_with_scipy_minimises_the_augmented_function(cpu_problem):
    from pycamset_amd.optimisation_handling import run_bundle_adjustment
    p = cpu_problem
    h = p["h"]
    h.make_loss_fun = lambda threads=None: p["fun"]          # the oracle's closures in place of the device's
    h.make_loss_jac = lambda threads=None: p["jac"]
    h.set_initial_params(p["x0"].copy())
    h.problem_opts.update({"prior": (p["mean"], p["sigma"]), "max_nfev": 60})
    try:
        res, slabs = run_bundle_adjustment(h, solver="scipy")
        assert res.fun.shape[0] == 2 * h._flat_detections().shape[0] + p["n_prior"]
        assert res.cost == p["ref"].cost and np.array_equal(res.x, p["ref"].x)       # the same call: the same bits
        assert np.array_equal(res.fun, p["fa"](res.x))
        h.problem_opts["loss"] = "huber"
        with pytest.raises(NotImplementedError, match="prior"):
            run_bundle_adjustment(h, solver="scipy")
        h.problem_opts.update({"loss": "linear", "prior": (p["mean"], p["sigma"][:-1])})
        with pytest.raises(ValueError, match="prior_sigma"):
            run_bundle_adjustment(h, solver="scipy")
    finally:
        for k in ("prior", "loss"):
            h.problem_opts.pop(k, None)
        del h.make_loss_fun, h.make_loss_jac
