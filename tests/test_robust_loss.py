"""Robust losses of the device solve (include/pcs_hip.h pcs_set_loss, device_solver.lm_solve(loss=, f_scale=)): what is decided
before any device work — argument checks of the C ABI, the loss name, and the combinations this version does not support."""
import ctypes

import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests.test_capi_symbols import declared_symbols
from tests.test_host_logic import DuckCamset, DuckTarget


def test_set_loss_checks_its_arguments_without_a_gpu():
    lib = _capi.lib()
    for name in ("pcs_set_loss", "pcs_get_loss"):
        assert name in declared_symbols() and name in _capi.SYMBOLS and hasattr(lib, name)
    assert lib.pcs_set_loss(None, 1, 1.0) == _capi.PCS_ERR_ARG
    assert b"pcs_set_loss" in lib.pcs_last_error()
    k, fs = ctypes.c_int(0), ctypes.c_double(0.0)
    assert lib.pcs_get_loss(None, ctypes.byref(k), ctypes.byref(fs)) == _capi.PCS_ERR_ARG
    assert lib.pcs_version() >= 101
    assert _capi.LOSS_IDS == {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}


class _Untouchable:
    """A handler / operator that fails on any use: the checks must come first."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the arguments were checked")


def test_unknown_loss_and_bad_f_scale_raise_before_any_device_work():
    from pycamset_amd.device_solver import lm_solve
    with pytest.raises(ValueError, match="bogus"):
        lm_solve(_Untouchable(), np.zeros(3), loss="bogus")
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="f_scale"):
            lm_solve(_Untouchable(), np.zeros(3), loss="huber", f_scale=fs)


def _cpu_problem():
    """The ring-4 template problem of test_host_logic's LM driver test, with a CPU operator built from the oracle's Jacobian."""
    from scipy.sparse import csr_array
    from pycamset_amd.device_solver import JacobianOperator

    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                       fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()])
    det, mask = h._flat_detections(), h._jac_mask()
    counts = orc.counts_from_detections(det)

    class CpuEngine:
        n, n_params = det.shape[0], mask.shape[0]

        def linearize(self, ps):
            dense, r = orc.full_jac_dense("template", det, ps, rig.points, with_resid=True, counts=counts)
            idx, ptr, _ = orc.csr_structure("template", det, np.ones(mask.shape[0], bool))
            self.J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], mask.shape[0]))
            self.r = r.reshape(-1)

        def jv(self, v):
            return self.J @ v

        def jtu(self, u):
            return self.J.T @ u

        def jtjv(self, v):
            return self.J.T @ (self.J @ v)

        def jtj_diag(self):
            return np.asarray(self.J.multiply(self.J).sum(axis=0)).ravel()

        def grad(self):
            return self.J.T @ self.r, float(self.r @ self.r)

    return h, x0, JacobianOperator(CpuEngine(), mask)


def test_robust_loss_with_pcg_or_a_caller_operator_is_not_implemented():
    """A host operator's products know nothing of the loss, and neither do the matrix-free products of the PCG step."""
    from pycamset_amd.device_solver import lm_solve
    h, x0, op = _cpu_problem()
    for loss in ("huber", "soft_l1", "cauchy", "arctan"):
        with pytest.raises(NotImplementedError, match="operator"):
            lm_solve(h, x0.copy(), max_iter=3, operator=op, loss=loss)
        with pytest.raises(NotImplementedError, match="operator"):
            lm_solve(h, x0.copy(), max_iter=3, operator=op, linear_solver="cholesky", loss=loss)
        with pytest.raises(NotImplementedError, match="pcg"):
            lm_solve(h, x0.copy(), max_iter=3, linear_solver="pcg", loss=loss)
    # the linear loss is the solve as before
    res = lm_solve(h, x0.copy(), max_iter=3, operator=op, loss="linear")
    ref = lm_solve(h, x0.copy(), max_iter=3, operator=op)
    assert res.cost == ref.cost and np.array_equal(res.x, ref.x)
