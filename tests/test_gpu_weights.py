"""Noise weights on the device (include/pcs_hip.h pcs_set_weights, lm_solve(sigma=), parameter_covariance(sigma=)): the weighted normal
equations against the whitened oracle system of tests/weights_reference.py and against a table with repeated detections, what stays
bit-identical, the weighted solve against scipy on the whitened closures, the weighted covariance, and the refusals.  Everything
runs on the ring-4 rig of the robust-loss tests."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.optimize._lsq.least_squares import construct_loss_function

from pycamset_amd import _capi
from tests import weights_reference as W

pytestmark = pytest.mark.gpu
CHAINS = ["template", "self", "free"]


def _engine(chain, rig, det, tm):
    from pycamset_amd.engine import Engine
    e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys)
    e.set_detections_table(det)
    if tm is not None:
        e.set_template(tm)
    return e


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- 1. the build against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_weighted_normal_equations_match_the_whitened_oracle(chain):
    """Linear and huber, atomic and ordered contraction, in table order, from a shuffled table (every pass reads a sorted copy of the
    weights) and with the sorted copies switched off (the weights are read through the visiting order)."""
    rig, det, ps, tm = W.chain_inputs(chain)
    w = W.log_uniform_weights(det.shape[0], 11)
    e = _engine(chain, rig, det, tm)
    assert e.weights() is None
    e.set_weights(1.0 / w)
    assert np.allclose(e.weights(), w, rtol=1e-15, atol=0)
    perm = np.random.default_rng(2).permutation(det.shape[0])
    shuffled = _engine(chain, rig, det[perm], tm)
    shuffled.set_weights(inv_sigma=w[perm])
    unsorted = _engine(chain, rig, det[perm], tm)
    unsorted.set_option("normal_sort_tables", 0)
    unsorted.set_weights({"detection": 1.0 / w[perm]})
    for loss in ("linear", "huber"):
        Href, gref, cref, slack = W.weighted_system(chain, det, ps, tm, w, loss, 1.0)
        for eng in (e, shuffled, unsorted):
            eng.set_loss(loss, 1.0)
            for det_mode in (0, 1):
                eng.set_option("deterministic", det_mode)
                Hu, g, cost = eng.normal_equations(ps, symmetric=False)
                W.check(Hu, g, cost, Href, gref, cref, slack)
    # a per-camera sigma is the per-detection one it expands to
    per_cam = np.array([0.5, 1.0, 2.0, 4.0])
    e.set_loss("linear", 1.0)
    e.set_weights(per_cam)
    Href, gref, cref, _ = W.weighted_system(chain, det, ps, tm, 1.0 / per_cam[det[:, 0].astype(int)])
    W.check(*e.normal_equations(ps, symmetric=False), Href, gref, cref)


# ---- 2. the duplication identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_weight_two_is_four_copies_of_the_detection(chain):
    """Independent of the oracle: under the linear loss 1 / sigma = 2 on a detection is that detection four times in the table.  Every
    third detection is repeated, its copies side by side, so that tile boundaries (64 rows) fall inside a run of copies."""
    rig, det, ps, tm = W.chain_inputs(chain)
    n = det.shape[0]
    sel = np.arange(n) % 3 == 0
    reps = np.where(sel, 4, 1)
    src = np.repeat(np.arange(n), reps)
    cut = np.arange(64, src.shape[0], 64)
    assert np.any(src[cut] == src[cut - 1])                   # a tile of the shared pass ends between two copies of one detection
    dup = _engine(chain, rig, det[src], tm)
    wtd = _engine(chain, rig, det, tm)
    wtd.set_weights(inv_sigma=np.where(sel, 2.0, 1.0))
    for det_mode in (0, 1):
        for eng in (dup, wtd):
            eng.set_option("deterministic", det_mode)
        Hd, gd, cd = dup.normal_equations(ps, symmetric=True)
        Hw, gw, cw = wtd.normal_equations(ps, symmetric=False)
        W.check(Hw, gw, cw, Hd, gd, cd)


# ---- 3. nothing changes when unset -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_cleared_weights_and_a_new_table_leave_the_build_bit_identical(chain):
    rig, det, ps, tm = W.chain_inputs(chain)
    w = W.log_uniform_weights(det.shape[0], 5)
    plain, touched = _engine(chain, rig, det, tm), _engine(chain, rig, det, tm)
    for e in (plain, touched):
        e.set_option("deterministic", 1)
    a = plain.normal_equations(ps, symmetric=False)
    touched.set_weights(inv_sigma=w)
    weighted = touched.normal_equations(ps, symmetric=False)
    assert not _same(a, weighted)
    touched.set_weights(None)
    assert touched.weights() is None
    assert _same(a, touched.normal_equations(ps, symmetric=False))
    touched.set_weights(inv_sigma=w)
    assert _same(weighted, touched.normal_equations(ps, symmetric=False))
    touched.set_detections_table(det)                         # a new table has no weights
    assert touched.weights() is None
    assert _same(a, touched.normal_equations(ps, symmetric=False))
    # a robust loss without weights keeps its bits as well (the weight the kernels then multiply by is exactly 1)
    for e in (plain, touched):
        e.set_loss("cauchy", 2.0)
    touched.set_weights(inv_sigma=w)
    touched.normal_equations(ps)
    touched.set_weights(None)
    assert _same(plain.normal_equations(ps, symmetric=False), touched.normal_equations(ps, symmetric=False))


# ---- 4. deterministic mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_ordered_weighted_builds_repeat_bit_for_bit(chain):
    rig, det, ps, tm = W.chain_inputs(chain)
    e = _engine(chain, rig, det, tm)
    e.set_option("deterministic", 1)
    e.set_weights(inv_sigma=W.log_uniform_weights(det.shape[0], 7))
    for loss in ("linear", "cauchy"):
        e.set_loss(loss, 1.5)
        assert _same(e.normal_equations(ps, symmetric=False), e.normal_equations(ps, symmetric=False)), loss


# ---- 5. the solve ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["template", "self"])
def test_weighted_solve_matches_scipy_on_the_whitened_closures(chain):
    """Device-steered and host-steered loops, linear and huber, against least_squares on (w f, diag(w) J) with the tolerances of
    test_robust_solve_matches_scipy_and_resists_outliers and test_robust_solve_through_every_loop; afterwards the handler solves
    unweighted exactly as a fresh one does."""
    from pycamset_amd.device_solver import lm_solve
    rig, h, x0 = W.ring4_handler(chain)
    tm = rig.points if chain == "template" else None
    fun, jac = W.oracle_closures(h, chain, tm)
    det = h._flat_detections()
    per_cam = np.array([0.5, 1.0, 2.0, 4.0])                  # pixels: the four cameras differ by a factor of eight
    w = 1.0 / per_cam[det[:, 0].astype(int)]
    wf, wj = W.whitened_closures(fun, jac, w)
    start = x0
    for loss in ("linear", "huber"):
        # the huber solves start where the weighted linear one ended, as in test_robust_solve_matches_scipy_and_resists_outliers (from the
        # far start most residuals lie beyond f_scale, where scipy's trf needs hundreds of evaluations)
        res = lm_solve(h, start.copy(), max_iter=200, loss=loss, f_scale=1.0, sigma=per_cam)
        ref = least_squares(wf, start.copy(), jac=wj, x_scale="jac", loss=loss, f_scale=1.0, max_nfev=300)
        f = wf(res.x)
        rho = construct_loss_function(f.size, loss, 1.0)(f, cost_only=False) if loss != "linear" else np.stack([f * f, np.ones_like(f)])
        assert abs(res.cost - 0.5 * np.sum(rho[0])) <= 1e-9 * res.cost
        assert res.cost <= ref.cost * (1 + 1e-6), (loss, res.cost, ref.cost)
        g_ref = wj(res.x).T @ (rho[1] * f)
        assert np.max(np.abs(res.grad - g_ref)) <= 1e-9 * max(np.max(np.abs(wj(res.x).T @ np.abs(rho[1] * f))), 1.0)
        # the per-detection form of the same sigma, and the host-steered loop
        same = lm_solve(h, start.copy(), max_iter=200, loss=loss, f_scale=1.0, sigma=1.0 / w)
        assert abs(same.cost - res.cost) <= 1e-9 * res.cost, (loss, same.cost, res.cost)
        host = lm_solve(h, start.copy(), max_iter=200, reduce_fn=lambda v: v, loss=loss, f_scale=1.0, sigma=per_cam)
        assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (loss, host.cost, res.cost)
        start = res.x
    eng = h.op_fun.engine if hasattr(h.op_fun, "engine") else h.op_fun._engine
    assert eng.weights() is None and eng.loss() == ("linear", 1.0)           # both restored after the solve
    # the cached solver state keeps nothing of the weights
    after = lm_solve(h, x0.copy(), max_iter=30)
    _, hf, _ = W.ring4_handler(chain)
    fresh = lm_solve(hf, x0.copy(), max_iter=30)
    assert abs(after.cost - fresh.cost) <= 1e-9 * fresh.cost and np.max(np.abs(after.x - fresh.x)) <= 1e-7 * np.max(np.abs(fresh.x))
    weighted = lm_solve(h, x0.copy(), max_iter=30, sigma=per_cam)
    assert weighted.cost != after.cost


# ---- 6. the covariance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["template", "self"])
def test_weighted_covariance_matches_the_whitened_oracle(chain):
    from scipy.sparse import csr_array, diags
    from pycamset_amd.device_solver import parameter_covariance
    from tests.test_gpu_covariance import _compare, _oracle_jac, _reference
    rig, h, x = W.ring4_handler(chain)
    mask = h._jac_mask()
    det = h._flat_detections()
    w = W.log_uniform_weights(det.shape[0], 13)
    J, r = _oracle_jac(h, x)
    wr = W.rows_of(w)
    Jw, rw = csr_array(diags(wr) @ J), wr * r
    slabs = h.get_bundle_adjustment_inputs(x)
    full, s2, kappa = _reference(Jw, rw, mask)
    cov = parameter_covariance(h, x, sigma=1.0 / w)
    assert cov.dof == 2 * det.shape[0] - mask.sum()
    assert abs(cov.sigma2 - s2) <= 1e-10 * s2 and abs(cov.cost - 0.5 * float(rw @ rw)) <= 1e-10 * cov.cost
    _compare(cov, slabs, full, mask, kappa, f"{chain} weighted")
    full_abs, _, _ = _reference(Jw, rw, mask, absolute_sigma=True)
    ab = parameter_covariance(h, x, sigma=1.0 / w, absolute_sigma=True)
    assert ab.sigma2 == 1.0
    _compare(ab, slabs, full_abs, mask, kappa, f"{chain} weighted, absolute")
    # and without sigma the raw system again, on the same cached state
    full_raw, s2_raw, kappa_raw = _reference(J, r, mask)
    raw = parameter_covariance(h, x)
    assert abs(raw.sigma2 - s2_raw) <= 1e-10 * s2_raw
    _compare(raw, slabs, full_raw, mask, kappa_raw, f"{chain} unweighted after weighted")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_weights_leave_the_previous_ones_in_force():
    rig, det, ps, tm = W.chain_inputs("self")
    n = det.shape[0]
    w = W.log_uniform_weights(n, 17)
    e = _engine("self", rig, det, tm)
    e.set_option("deterministic", 1)
    e.set_weights(inv_sigma=w)
    before = e.normal_equations(ps, symmetric=False)
    lib = _capi.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        v = np.ones(n)
        v[n // 2] = bad
        assert lib.pcs_set_weights(e._h, v.ctypes.data_as(dp), n) == _capi.PCS_ERR_ARG
        assert b"finite and > 0" in lib.pcs_last_error()
    v = np.ones(n + 1)
    for m in (n - 1, n + 1, 0):
        assert lib.pcs_set_weights(e._h, v.ctypes.data_as(dp), m) == _capi.PCS_ERR_ARG
    with pytest.raises(ValueError):
        e.set_weights(np.full(n, -2.0))
    assert np.array_equal(e.weights(), w)
    assert _same(before, e.normal_equations(ps, symmetric=False))


def test_weights_where_they_are_not_implemented(monkeypatch):
    from pycamset_amd import device_solver, function_blocks as fb, handlers
    from pycamset_amd.device_solver import lm_solve, parameter_covariance
    rig, h, x0 = W.ring4_handler("template")
    per_cam = np.ones(rig.n_cams)
    with pytest.raises(NotImplementedError, match="pcg"):
        lm_solve(h, x0.copy(), max_iter=3, linear_solver="pcg", sigma=per_cam)
    with pytest.raises(NotImplementedError, match="operator"):
        lm_solve(h, x0.copy(), max_iter=3, operator=object(), sigma=per_cam)
    monkeypatch.setattr(device_solver, "blocked_fits", lambda eng: False)          # a system beyond the blocked normal equations
    with pytest.raises(NotImplementedError, match="too large"):
        lm_solve(h, x0.copy(), max_iter=3, sigma=per_cam)
    monkeypatch.undo()
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()   # not one of the hand-fused chains
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    second = np.zeros((rig.n_imgs, 6))
    fix_second = np.zeros((rig.n_imgs, 6), dtype=bool)
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, second, rig.poses], template=rig.points,
                                 unfixed=[None, fix_ext, fix_second, None])
    with pytest.raises(NotImplementedError, match="generated chains"):
        lm_solve(prob, prob.x0, max_iter=3, sigma=per_cam)
    with pytest.raises(NotImplementedError, match="generated chains"):
        parameter_covariance(prob, prob.x0, sigma=per_cam)
