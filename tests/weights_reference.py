"""Reference for the noise weights of the device solve (include/pcs_hip.h pcs_set_weights): the CPU oracle's Jacobian and residuals with
each detection's two rows scaled by w = 1 / sigma, then — for a robust loss — scipy's own loss functions and linearisation applied to that
whitened system.  Mirrors ``_oracle_system`` of tests/test_gpu_robust_loss.py."""
import functools

import numpy as np
from scipy.optimize._lsq.common import scale_for_robust_loss_function
from scipy.optimize._lsq.least_squares import construct_loss_function
from scipy.sparse import csr_array, diags

from oracle import ba_oracle as orc
from pycamset_amd import synthetic
from tests import helpers as H

EPS = np.finfo(float).eps


def log_uniform_weights(n, seed, lo=0.25, hi=4.0):
    """n weights 1 / sigma, log-uniform over [lo, hi]."""
    return np.exp(np.random.default_rng(seed).uniform(np.log(lo), np.log(hi), n))


def rows_of(w):
    """One weight per detection -> one per residual row (u and v share it)."""
    return np.repeat(np.asarray(w, dtype=np.float64), 2)


@functools.lru_cache(maxsize=None)
def ring4():
    """The ring-4 rig of the robust-loss tests: 4 cameras, 6 images, a 7-row ChArUco board, visibility 0.9."""
    return synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)


def chain_inputs(chain):
    """(rig, detections, parameter string, template or None) of `chain` on ring-4."""
    rig = ring4()
    return rig, rig.detections, orc.build_param_list(*H.chain_slabs(rig, chain)), (rig.points if chain == "template" else None)


def whitened_jacobian(chain, det, ps, tm, w, counts=None):
    """(J~ = diag(w) J as CSR over the full parameter string, f~ = w f).  ``counts``: the (cameras, images, keys) of the layout when
    ``det`` is a slice of a larger table (a rank's shard) that may not reach the last index of each."""
    dense, r = orc.full_jac_dense(chain, det, ps, tm, with_resid=True, counts=counts)
    idx, ptr, _ = orc.csr_structure(chain, det, np.ones(ps.shape[0], bool), counts=counts)
    J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], ps.shape[0]))
    wr = rows_of(w)
    return csr_array(diags(wr) @ J), wr * r.reshape(-1)


def weighted_system(chain, det, ps, tm, w, loss="linear", f_scale=1.0, counts=None):
    """(J~^T J~, J~^T r~, sum rho0, slack of H) of the whitened system through scipy's loss and scale_for_robust_loss_function; the slack
    is that of ``_oracle_system``: rows where rho1 + 2 rho2 f^2 cancels to rounding level (huber beyond f_scale) carry a weight^2 of
    anything in [EPS, a few EPS], bounded by 16 EPS |J~_i|^T |J~_i| summed over those rows."""
    J, f = whitened_jacobian(chain, det, ps, tm, w, counts)
    if loss == "linear":
        return (J.T @ J).toarray(), J.T @ f, float(f @ f), 0.0
    rho = construct_loss_function(f.size, loss, f_scale)(f, cost_only=False)
    js = rho[1] + 2 * rho[2] * f ** 2
    Jb = abs(J[np.flatnonzero(js < 8 * EPS)])
    Js, fs = scale_for_robust_loss_function(J.tocsr().copy(), f.copy(), rho)
    return (Js.T @ Js).toarray(), Js.T @ fs, float(np.sum(rho[0])), 16 * EPS * (Jb.T @ Jb).toarray()


def check(Hu, g, cost, Href, gref, cref, slack=0.0, tol=1e-10):
    """The rule of ``_check`` in tests/test_gpu_robust_loss.py, unchanged."""
    scale = np.sqrt(np.outer(np.diag(Href), np.diag(Href)))
    up = np.triu(np.ones_like(Href, dtype=bool))
    bound = (tol * scale + slack + 1e-300)[up]
    assert np.all(np.abs(Hu - Href)[up] <= bound), float(np.max(np.abs(Hu - Href)[up] / bound))
    gs = np.sqrt(np.diag(Href) * max(float(gref @ gref), 1e-300) + 1e-300)
    assert np.all(np.abs(g - gref) <= tol * np.maximum(gs, np.max(np.abs(gref)))), float(np.max(np.abs(g - gref)))
    assert abs(cost - cref) <= tol * abs(cref), (cost, cref)


def oracle_closures(h, chain, tm):
    """(fun, jac) of a handler over its free parameters, from the oracle: raw residuals (2N,) and the CSR Jacobian."""
    det, mask = h._flat_detections(), np.asarray(h._jac_mask(), bool)
    counts = orc.counts_from_detections(det)

    def ps_of(x):
        return orc.build_param_list(*h.get_bundle_adjustment_inputs(x))

    def fun(x):
        return orc.full_loss(chain, det, ps_of(x), tm, counts=counts).reshape(-1)

    idx, ptr, _ = orc.csr_structure(chain, det, np.ones(mask.shape[0], bool))

    def jac(x):
        dense = orc.full_jac_dense(chain, det, ps_of(x), tm, counts=counts)
        return csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], mask.shape[0]))[:, np.flatnonzero(mask)]

    return fun, jac


def whitened_closures(fun, jac, w):
    """The closures scipy's least_squares minimises for weights w: x -> w f(x) and x -> diag(w) J(x)."""
    wr = rows_of(w)
    return (lambda x: wr * fun(x)), (lambda x: csr_array(diags(wr) @ jac(x)))


def ring4_handler(chain, det=None):
    """(rig, handler with camera 0's extrinsics fixed, start vector) on ring-4, with `det` in place of the rig's table if given."""
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget
    rig = ring4()
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections if det is None else det),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return rig, h, np.concatenate(parts)
