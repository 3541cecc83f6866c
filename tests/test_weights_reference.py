"""Noise weights of the device solve (include/pcs_hip.h pcs_set_weights, lm_solve(sigma=)): the reference of tests/weights_reference.py
pinned to scipy, and everything that is decided before any device work — the forms sigma may take, its expansion per camera, the
shards of a sharded solve, the combinations this version refuses and the C symbols."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import least_squares

from pycamset_amd import _capi, sharding
from pycamset_amd.engine import expand_sigma
from tests import weights_reference as W
from tests.test_capi_symbols import declared_symbols


@pytest.mark.parametrize("chain", ["template", "self"])
@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_reference_is_what_scipy_builds_on_the_whitened_closures(chain, loss):
    """least_squares on (w f, diag(w) J) stopped after its first evaluation reports the linearised system at the start: its (scaled)
    Jacobian, gradient and cost are the reference's J~^T J~, J~^T r~ and sum rho0."""
    rig, h, x0 = W.ring4_handler(chain)
    tm = rig.points if chain == "template" else None
    fun, jac = W.oracle_closures(h, chain, tm)
    det, mask = h._flat_detections(), np.asarray(h._jac_mask(), bool)
    w = W.log_uniform_weights(det.shape[0], 3)
    wf, wj = W.whitened_closures(fun, jac, w)
    res = least_squares(wf, x0, jac=wj, x_scale="jac", loss=loss, f_scale=1.0, max_nfev=1)
    assert np.array_equal(res.x, x0)
    from oracle import ba_oracle as orc
    ps = orc.build_param_list(*h.get_bundle_adjustment_inputs(x0))
    Href, gref, cref, _ = W.weighted_system(chain, det, ps, tm, w, loss, 1.0)
    free = np.flatnonzero(mask)
    Hs = (res.jac.T @ res.jac).toarray()
    assert np.max(np.abs(Hs - Href[np.ix_(free, free)])) <= 1e-12 * np.max(np.abs(Hs))
    assert np.max(np.abs(res.grad - gref[free])) <= 1e-12 * np.max(np.abs(res.grad))
    assert abs(2.0 * res.cost - cref) <= 1e-12 * cref
    # the weights matter: the unweighted system is another one
    H1, _, c1, _ = W.weighted_system(chain, det, ps, tm, np.ones_like(w), loss, 1.0)
    assert abs(c1 - cref) > 1e-3 * cref and np.max(np.abs(H1 - Href)) > 1e-3 * np.max(np.abs(Href))


def test_sigma_forms_and_validation():
    cam = np.array([0, 0, 1, 2, 2, 2, 1])
    assert expand_sigma(None, cam, 3) is None
    per_det = np.linspace(0.5, 2.0, 7)
    assert np.array_equal(expand_sigma(per_det, cam, 3), per_det)
    assert np.array_equal(expand_sigma({"detection": per_det}, cam, 3), per_det)
    per_cam = np.array([0.5, 1.0, 4.0])
    want = np.array([0.5, 0.5, 1.0, 4.0, 4.0, 4.0, 1.0])
    assert np.array_equal(expand_sigma(per_cam, cam, 3), want)
    assert np.array_equal(expand_sigma({"camera": per_cam}, cam, 3), want)
    assert np.array_equal(expand_sigma(list(per_cam), cam, 3), want)
    for bad_len in (2, 4, 6, 8):
        with pytest.raises(ValueError, match="entries"):
            expand_sigma(np.ones(bad_len), cam, 3)
    with pytest.raises(ValueError, match="entries"):
        expand_sigma({"camera": np.ones(7)}, cam, 3)
    with pytest.raises(ValueError, match="entries"):
        expand_sigma({"detection": np.ones(3)}, cam, 3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for form in (per_det.copy(), per_cam.copy()):
            form[1] = bad
            with pytest.raises(ValueError, match="finite and > 0"):
                expand_sigma(form, cam, 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        expand_sigma(np.ones((7, 2)), cam, 3)
    with pytest.raises(ValueError, match="dict"):
        expand_sigma({"image": np.ones(3)}, cam, 3)
    # N == C: a bare array could be either
    cam3 = np.array([2, 0, 1])
    with pytest.raises(ValueError, match="ambiguous"):
        expand_sigma(per_cam, cam3, 3)
    assert np.array_equal(expand_sigma({"camera": per_cam}, cam3, 3), per_cam[cam3])
    assert np.array_equal(expand_sigma({"detection": per_cam}, cam3, 3), per_cam)


def test_per_camera_sigma_follows_the_camera_column_of_the_handlers_table():
    rig, h, _ = W.ring4_handler("template")
    det = h._flat_detections()
    per_cam = np.array([0.5, 1.0, 2.0, 4.0])
    s = expand_sigma(per_cam, det[:, 0], rig.n_cams)
    assert s.shape == (det.shape[0],) and np.array_equal(s, per_cam[det[:, 0].astype(int)])
    assert set(np.unique(s)) == set(per_cam)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_sigma_follows_the_detection_split(world):
    n = 23
    det = np.arange(5 * n, dtype=np.float64).reshape(n, 5)
    sigma = 1.0 + np.arange(n) / 7.0
    per = sharding.shard_rows(n, world)
    parts = []
    for rank in range(world):
        mine = det[rank * per:(rank + 1) * per]
        s = sharding.shard_sigma(sigma, n, rank, world)
        assert set(s) == {"detection"} and s["detection"].shape[0] == mine.shape[0]
        assert np.array_equal(s["detection"], 1.0 + (mine[:, 0] / 5.0) / 7.0)      # row i of the table carries sigma[i]
        assert np.array_equal(sharding.shard_sigma({"detection": sigma}, n, rank, world)["detection"], s["detection"])
        parts.append(s["detection"])
        per_cam = {"camera": np.array([1.0, 2.0])}
        assert sharding.shard_sigma(per_cam, n, rank, world) is per_cam and sharding.shard_sigma(None, n, rank, world) is None
    assert np.array_equal(np.concatenate(parts), sigma)
    # more ranks than rows leave the last ranks an empty slice, like their shard
    assert sharding.shard_sigma(np.ones(2), 2, 2, 3)["detection"].shape == (0,)
    with pytest.raises(ValueError, match="entries"):
        sharding.shard_sigma({"detection": np.ones(n + 1)}, n, 0, world)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the arguments were checked")


def test_weighted_solve_refuses_pcg_and_caller_operators_before_any_device_work():
    from pycamset_amd.device_solver import lm_solve
    with pytest.raises(NotImplementedError, match="pcg"):
        lm_solve(_Untouchable(), np.zeros(3), linear_solver="pcg", sigma=np.ones(4))
    with pytest.raises(NotImplementedError, match="operator"):
        lm_solve(_Untouchable(), np.zeros(3), operator=object(), sigma=np.ones(4))
    with pytest.raises(NotImplementedError, match="operator"):
        lm_solve(_Untouchable(), np.zeros(3), operator=object(), linear_solver="cholesky", sigma={"camera": np.ones(4)})


def test_bad_sigma_is_refused_before_an_engine_exists():
    """lm_solve and parameter_covariance check sigma against the handler's table first: no engine (and no GPU) is needed to be told."""
    from pycamset_amd.device_solver import lm_solve, parameter_covariance
    rig, h, x0 = W.ring4_handler("template")
    n = h._flat_detections().shape[0]
    bad = np.ones(n)
    bad[5] = 0.0
    for call in (lambda s: lm_solve(h, x0.copy(), max_iter=2, sigma=s), lambda s: parameter_covariance(h, x0.copy(), sigma=s)):
        with pytest.raises(ValueError, match="entries"):
            call(np.ones(n - 1))
        with pytest.raises(ValueError, match="finite and > 0"):
            call(bad)
        with pytest.raises(ValueError, match="finite and > 0"):
            call(np.array([1.0, np.nan, 1.0, 1.0]))
    assert h.op_fun._engine is None


def test_weight_symbols_and_their_argument_checks_without_a_gpu():
    lib = _capi.lib()
    for name in ("pcs_set_weights", "pcs_get_weights"):
        assert name in declared_symbols() and name in _capi.SYMBOLS and hasattr(lib, name)
    w = (ctypes.c_double * 2)(1.0, 2.0)
    assert lib.pcs_set_weights(None, w, 2) == _capi.PCS_ERR_ARG
    assert b"pcs_set_weights" in lib.pcs_last_error()
    n = ctypes.c_int64(-1)
    assert lib.pcs_get_weights(None, None, 0, ctypes.byref(n)) == _capi.PCS_ERR_ARG
    assert b"pcs_get_weights" in lib.pcs_last_error()
    assert lib.pcs_version() >= 112
