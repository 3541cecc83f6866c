"""Parameter covariance (device_solver.parameter_covariance, include/pcs_hip.h pcs_cov_trsm / pcs_cov_block_gram): what is decided
before any device work — argument checks of the C ABI and of the Python entry point."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests.test_capi_symbols import declared_symbols
from tests.test_host_logic import DuckCamset, DuckTarget


def test_covariance_entry_points_check_their_arguments_without_a_gpu():
    lib = _capi.lib()
    for name in ("pcs_cov_trsm", "pcs_cov_block_gram"):
        assert name in declared_symbols() and name in _capi.SYMBOLS and hasattr(lib, name)
    assert lib.pcs_version() >= 102
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below fails its argument check
    null = None
    trsm = lib.pcs_cov_trsm
    assert trsm(0, -1, p, 4, p, 4, 4, 0, null) == _capi.PCS_ERR_ARG
    assert b"pcs_cov_trsm" in lib.pcs_last_error()
    assert trsm(0, 4, p, 4, p, -2, 4, 0, null) == _capi.PCS_ERR_ARG
    assert trsm(0, 4, null, 4, p, 4, 4, 0, null) == _capi.PCS_ERR_ARG
    assert trsm(0, 4, p, 4, null, 4, 4, 0, null) == _capi.PCS_ERR_ARG
    assert trsm(0, 4, p, 3, p, 4, 4, 0, null) == _capi.PCS_ERR_ARG            # ldl < n
    assert trsm(0, 4, p, 4, p, 4, 3, 0, null) == _capi.PCS_ERR_ARG            # ldx < n_rhs
    assert trsm(0, 4, p, 4, p, 3, 4, _capi.COV_TRSM_IDENTITY, null) == _capi.PCS_ERR_ARG   # L^-1 is n x n
    assert trsm(0, 4, p, 4, p, 4, 4, 8, null) == _capi.PCS_ERR_ARG            # unknown flag
    gram = lib.pcs_cov_block_gram
    ok = dict(X=p, ldx=8, rows=8, cols=8, col=p, width=p, row0=null, nb=2, out=p, stride=64, linvt=null, tb=0, fixed=null, off=0, scale_dev=null, scale=1.0)

    def g(**kw):
        a = dict(ok, **kw)
        return gram(0, a["X"], a["ldx"], a["rows"], a["cols"], a["col"], a["width"], a["row0"], a["nb"], a["out"], a["stride"], a["linvt"], a["tb"],
                    a["fixed"], a["off"], a["scale_dev"], a["scale"], null)

    for bad in (dict(rows=-1), dict(cols=-3), dict(ldx=4), dict(nb=-1), dict(stride=0), dict(X=null), dict(col=null), dict(width=null),
                dict(out=null), dict(linvt=p, tb=0), dict(linvt=p, tb=17), dict(off=-1), dict(scale=float("nan"))):
        assert g(**bad) == _capi.PCS_ERR_ARG, bad
        assert b"pcs_cov_block_gram" in lib.pcs_last_error()


class _Untouchable:
    """A handler that fails on any use: the checks must come first."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the arguments were checked")


class _NoDevice(handlers.TemplateBundleHandler):
    """A real handler whose engine may not be created: the checks must come before any device work."""

    @property
    def op_fun(self):
        raise AssertionError("device work before the arguments were checked")

    @op_fun.setter
    def op_fun(self, v):
        self._op = v


def _handler(n_det=None):
    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    det = rig.detections if n_det is None else rig.detections[:n_det]
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = _NoDevice(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, det),
                  fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    return h, np.zeros(int(h._jac_mask().sum()))


def test_parameter_covariance_checks_its_arguments_before_any_device_work():
    from pycamset_amd import parameter_covariance
    from pycamset_amd.device_solver import ParameterCovariance, parameter_covariance as pc
    assert parameter_covariance is pc and "std" in ParameterCovariance.__dataclass_fields__
    with pytest.raises(NotImplementedError, match="reduce_fn"):
        pc(_Untouchable(), np.zeros(3), reduce_fn=lambda buf: buf)
    h, x0 = _handler()
    with pytest.raises(ValueError, match="free parameters"):
        pc(h, x0[:-1])
    with pytest.raises(ValueError, match="free parameters"):
        pc(h, np.concatenate([x0, [0.0]]))
    with pytest.raises(ValueError, match="rcond"):
        pc(h, x0, rcond=-1.0)
    h, x0 = _handler(n_det=20)   # 40 residuals for 54 free parameters
    assert x0.shape[0] == 54
    with pytest.raises(ValueError, match="degrees of freedom"):
        pc(h, x0)
    with pytest.raises(ValueError, match="degrees of freedom"):
        pc(h, x0, absolute_sigma=True)
