"""Robust losses on the device (include/pcs_hip.h pcs_set_loss): the normal equations against scipy's own loss functions and
linearisation applied to the CPU oracle's Jacobian, and the LM solve against scipy.optimize.least_squares with the same loss."""
import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.optimize._lsq.common import scale_for_robust_loss_function
from scipy.optimize._lsq.least_squares import construct_loss_function
from scipy.sparse import csr_array

from oracle import ba_oracle as orc
from pycamset_amd import synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu
LOSSES = ["huber", "soft_l1", "cauchy", "arctan"]


def _oracle_system(chain, det, ps, tm, loss, f_scale):
    """(J~^T J~, J~^T r~, sum rho0, slack of H) from the oracle's J and residuals through scipy's loss and scale_for_robust_loss_function.
    Where rho1 + 2 rho2 f^2 cancels to rounding level (huber beyond f_scale: exactly 0 in exact arithmetic) scipy's clamp to EPS meets
    a rounding residue of either sign, computed one way there and another on the device: such a row's weight^2 is anything in
    [EPS, a few EPS].  The slack bounds what that can change in H: 16 EPS |J_i|^T |J_i| summed over those rows."""
    dense, r = orc.full_jac_dense(chain, det, ps, tm, with_resid=True)
    idx, ptr, _ = orc.csr_structure(chain, det, np.ones(ps.shape[0], bool))
    J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], ps.shape[0]))
    f = r.reshape(-1).copy()
    if loss == "linear":
        return (J.T @ J).toarray(), J.T @ f, float(f @ f), 0.0
    rho = construct_loss_function(f.size, loss, f_scale)(f, cost_only=False)
    js = rho[1] + 2 * rho[2] * f ** 2
    Jb = abs(J[np.flatnonzero(js < 8 * np.finfo(float).eps)])
    Js, fs = scale_for_robust_loss_function(J.tocsr().copy(), f.copy(), rho)
    return (Js.T @ Js).toarray(), Js.T @ fs, float(np.sum(rho[0])), 16 * np.finfo(float).eps * (Jb.T @ Jb).toarray()


def _check(Hu, g, cost, Href, gref, cref, slack=0.0, tol=1e-10):
    scale = np.sqrt(np.outer(np.diag(Href), np.diag(Href)))
    up = np.triu(np.ones_like(Href, dtype=bool))
    bound = (tol * scale + slack + 1e-300)[up]
    assert np.all(np.abs(Hu - Href)[up] <= bound), float(np.max(np.abs(Hu - Href)[up] / bound))
    gs = np.sqrt(np.diag(Href) * max(float(gref @ gref), 1e-300) + 1e-300)
    assert np.all(np.abs(g - gref) <= tol * np.maximum(gs, np.max(np.abs(gref)))), float(np.max(np.abs(g - gref)))
    assert abs(cost - cref) <= tol * abs(cref), (cost, cref)


def _engine(chain, rig, det, tm):
    from pycamset_amd.engine import Engine
    e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys)
    e.set_detections_table(det)
    if tm is not None:
        e.set_template(tm)
    return e


def _blocks(e, ps):
    """[A | B | C | g | cost] of pcs_normal_blocks_device, as (A, B, C, g, cost) on the host."""
    import torch
    lay = e.normal_layout()
    nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
    d_ps = torch.from_numpy(ps).cuda()
    pk = torch.empty(lay["packed_len"], dtype=torch.float64, device="cuda")
    e.normal_blocks_device(d_ps.data_ptr(), pk.data_ptr())
    e.synchronize()
    pk = pk.cpu().numpy()
    n = ps.shape[0]
    A = pk[: nl * nl].reshape(nl, nl)
    B = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
    C = pk[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
    return nl, tb, A, B, C, pk[-(n + 1):-1], float(pk[-1])


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_robust_normal_equations_match_scipy_linearisation(chain):
    """Dense and blocked builds, atomic and ordered contraction, every loss and two f_scale: J~^T J~, J~^T r~ and sum rho0 to 1e-10;
    the ordered builds repeat bit for bit."""
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    e = _engine(chain, rig, rig.detections, tm)
    for loss in LOSSES:
        for f_scale in (1.0, 2.5):
            Href, gref, cref, slack = _oracle_system(chain, rig.detections, ps, tm, loss, f_scale)
            e.set_loss(loss, f_scale)
            assert e.loss() == (loss, f_scale)
            for det_mode in (0, 1):
                e.set_option("deterministic", det_mode)
                Hu, g, cost = e.normal_equations(ps, symmetric=False)
                _check(Hu, g, cost, Href, gref, cref, slack)
                nl, tb, A, B, C, gb, cb = _blocks(e, ps)
                Hb = np.zeros_like(Href)
                Hb[:nl, :nl] = A
                Hb[:nl, nl:] = B
                for k in range(C.shape[0]):
                    o = nl + k * tb
                    Hb[o: o + tb, o: o + tb] = C[k]
                blk = np.zeros_like(Href, dtype=bool)   # what the blocked layout stores: A, B and the diagonal blocks of C
                blk[:nl, :] = True
                for k in range(C.shape[0]):
                    o = nl + k * tb
                    blk[o: o + tb, o: o + tb] = True
                _check(np.where(blk, Hb, 0.0), gb, cb, np.where(blk, Href, 0.0), gref, cref, slack)
                if det_mode:
                    Hu2, g2, cost2 = e.normal_equations(ps, symmetric=False)
                    assert np.array_equal(Hu, Hu2) and np.array_equal(g, g2) and cost == cost2
                    gb2 = _blocks(e, ps)
                    assert np.array_equal(gb2[2], A) and np.array_equal(gb2[3], B) and np.array_equal(gb2[5], gb) and gb2[6] == cb
    e.set_option("deterministic", 0)


def test_first_robust_build_on_a_caller_stream():
    """The first robust build of a self-chain engine gathers the measurements into the (image, key) order: that gather must be
    ordered before the pass that reads it on the CALLER's stream (an LM solve builds on its own stream), not on the engine's."""
    import torch
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, "self"))
    Href, gref, cref, slack = _oracle_system("self", rig.detections, ps, None, "cauchy", 1.0)
    e = _engine("self", rig, rig.detections, None)
    e.set_loss("cauchy", 1.0)
    lay = e.normal_layout()
    nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_ps = torch.from_numpy(ps).cuda()
        pk = torch.empty(lay["packed_len"], dtype=torch.float64, device="cuda")
        e.normal_blocks_device(d_ps.data_ptr(), pk.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    pk = pk.cpu().numpy()
    n = ps.shape[0]
    B = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt)    # the pose x point blocks F[i, k] (the (image, key) pass) are in B
    Hb = np.zeros_like(Href)
    Hb[:nl, nl:] = B
    blk = np.zeros_like(Href, dtype=bool)
    blk[:nl, nl:] = True
    scale = np.sqrt(np.outer(np.diag(Href), np.diag(Href)))
    assert np.all(np.abs(np.where(blk, Hb - Href, 0.0)) <= 1e-10 * scale + slack + 1e-300)
    assert np.all(np.abs(pk[-(n + 1):-1] - gref) <= 1e-10 * np.max(np.abs(gref))) and abs(pk[-1] - cref) <= 1e-10 * cref


def test_robust_normal_equations_full_size_template_huber():
    rig = synthetic.config_rig(3)
    ps = orc.build_param_list(*H.chain_slabs(rig, "template"))
    e = _engine("template", rig, rig.detections, rig.points)
    e.set_loss("huber", 1.0)
    Href, gref, cref, slack = _oracle_system("template", rig.detections, ps, rig.points, "huber", 1.0)
    Hu, g, cost = e.normal_equations(ps, symmetric=False)
    _check(Hu, g, cost, Href, gref, cref, slack)


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_linear_loss_leaves_the_build_bit_identical(chain):
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    plain, touched = _engine(chain, rig, rig.detections, tm), _engine(chain, rig, rig.detections, tm)
    for e in (plain, touched):
        e.set_option("deterministic", 1)
    touched.set_loss("cauchy", 3.0)
    touched.normal_equations(ps)
    touched.set_loss("linear", 1.0)
    a, b = plain.normal_equations(ps, symmetric=False), touched.normal_equations(ps, symmetric=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _outlier_problem(chain, seed=5):
    """ring-8-small (0.3 px noise) with ~3 % of the detections moved by 20 - 50 px (the handler of test_gpu_dropin's ring-8 tests)."""
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    det = rig.detections.copy()
    rng = np.random.default_rng(seed)
    bad = rng.choice(det.shape[0], max(1, int(0.03 * det.shape[0])), replace=False)
    ang = rng.uniform(0, 2 * np.pi, bad.size)
    mag = rng.uniform(20.0, 50.0, bad.size)
    det[bad, 3] += mag * np.cos(ang)
    det[bad, 4] += mag * np.sin(ang)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, det),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return rig, h, np.concatenate(parts)


def _oracle_closures(h, chain, tm):
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


def _focal_error(h, x, rig):
    intr = np.asarray(h.get_bundle_adjustment_inputs(x)[0])
    return float(np.max(np.abs(intr[:, [0, 2]] - rig.intr_true[:, [0, 2]])))


@pytest.mark.parametrize("chain", ["template", "self"])
def test_robust_solve_matches_scipy_and_resists_outliers(chain):
    from pycamset_amd.device_solver import lm_solve
    rig, h, x0 = _outlier_problem(chain)
    tm = rig.points if chain == "template" else None
    fun, jac = _oracle_closures(h, chain, tm)
    lin = lm_solve(h, x0.copy(), max_iter=60)
    # the robust solves start where the linear one ended (a calibration's usual refinement; from the far start most residuals lie
    # beyond f_scale, where scipy's trf needs hundreds of evaluations)
    for loss in ("huber", "cauchy"):
        res = lm_solve(h, lin.x.copy(), max_iter=200, loss=loss, f_scale=1.0)
        ref = least_squares(fun, lin.x.copy(), jac=jac, x_scale="jac", loss=loss, f_scale=1.0, max_nfev=300)
        f = fun(res.x)
        rho = construct_loss_function(f.size, loss, 1.0)(f, cost_only=False)
        assert abs(res.cost - 0.5 * np.sum(rho[0])) <= 1e-9 * res.cost
        # scipy's trf creeps on this problem (still ~3 % above the device's cost after 1000 evaluations): the device solve must reach
        # at least its robust cost
        assert res.cost <= ref.cost * (1 + 1e-6), (res.cost, ref.cost)
        g_ref = jac(res.x).T @ (rho[1] * f)
        assert np.max(np.abs(res.grad - g_ref)) <= 1e-9 * max(np.max(np.abs(jac(res.x).T @ np.abs(rho[1] * f))), 1.0)
        assert _focal_error(h, res.x, rig) < 0.5 * _focal_error(h, lin.x, rig), (loss, _focal_error(h, res.x, rig), _focal_error(h, lin.x, rig))
    # the engine's loss is restored after the solve
    assert h.op_fun.engine.loss() == ("linear", 1.0)


@pytest.mark.parametrize("chain", ["template", "self"])
def test_robust_solve_through_every_loop(chain):
    """Host-steered loop (identity reduce_fn, no on_device), the stream-ordered stand-in collective, and ordered mode (two solves,
    the same bits): each agrees with the single-GPU robust solve."""
    import torch
    from pycamset_amd.device_solver import lm_solve
    rig, h, x0 = _outlier_problem(chain)
    one = lm_solve(h, x0.copy(), max_iter=40, loss="huber")

    def host_sum(v):
        return v

    res = lm_solve(h, x0.copy(), max_iter=40, reduce_fn=host_sum, loss="huber")
    assert abs(res.cost - one.cost) <= 1e-9 * one.cost, (res.cost, one.cost)

    def in_stream_sum(t):
        t.mul_(1.0)
        return t

    in_stream_sum.on_device = True
    res = lm_solve(h, x0.copy(), max_iter=40, reduce_fn=in_stream_sum, loss="huber")
    assert abs(res.cost - one.cost) <= 1e-9 * one.cost, (res.cost, one.cost)
    torch.cuda.synchronize()

    eng = h.op_fun.engine
    eng.set_option("deterministic", 1)
    try:
        a = lm_solve(h, x0.copy(), max_iter=40, loss="huber")
        b = lm_solve(h, x0.copy(), max_iter=40, loss="huber")
    finally:
        eng.set_option("deterministic", 0)
    assert a.cost == b.cost and np.array_equal(a.x, b.x) and np.array_equal(a.grad, b.grad)
    assert abs(a.cost - one.cost) <= 1e-9 * one.cost, (a.cost, one.cost)


def test_cached_solver_state_does_not_keep_the_old_loss():
    from pycamset_amd.device_solver import lm_solve
    _, h, x0 = _outlier_problem("template")
    runs = [lm_solve(h, x0.copy(), max_iter=30, loss=loss) for loss in ("huber", "linear", "huber")]
    for loss, res in zip(("huber", "linear", "huber"), runs):
        _, hf, _ = _outlier_problem("template")   # a fresh handler: a fresh engine and solver state
        fresh = lm_solve(hf, x0.copy(), max_iter=30, loss=loss)
        assert abs(res.cost - fresh.cost) <= 1e-9 * fresh.cost and np.max(np.abs(res.x - fresh.x)) <= 1e-7 * np.max(np.abs(fresh.x)), loss
    assert runs[0].cost != runs[1].cost


def test_generated_chain_with_a_robust_loss_is_not_implemented():
    from pycamset_amd import function_blocks as fb
    from pycamset_amd import handlers
    from pycamset_amd.device_solver import lm_solve
    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()   # not one of the hand-fused chains
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    second = np.zeros((rig.n_imgs, 6))
    fix_second = np.zeros((rig.n_imgs, 6), dtype=bool)
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, second, rig.poses], template=rig.points,
                                 unfixed=[None, fix_ext, fix_second, None])
    with pytest.raises(NotImplementedError, match="generated chains"):
        lm_solve(prob, prob.x0, max_iter=3, loss="huber")
