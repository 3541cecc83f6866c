"""tests/lm_reference.py against lm_solve's host loop on CPU operators (no GPU): the reference's decisions must be the loop's, trial by
trial — accepted / rejected, the lambda sequence bit for bit, the stop code and nfev — before any GPU test relies on the reference.
The reference itself is checked on small hand-made inputs first."""
import numpy as np
import pytest
from scipy.sparse import csr_array

from oracle import ba_oracle as orc
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests import lm_reference as R
from tests.test_host_logic import DuckCamset, DuckTarget


def test_reference_step_and_backward_error():
    rng = np.random.default_rng(3)
    J = rng.standard_normal((40, 12))
    H, g = J.T @ J, rng.standard_normal(12)
    mask = np.ones(12, bool)
    mask[[0, 5, 11]] = False
    for lam in (1e-12, 1e-3, 10.0):
        d = R.reference_step(H, g, mask, lam)
        assert np.all(d[~mask] == 0)
        M, rhs = R.masked_system(H, g, mask, lam)
        assert R.backward_error(M, rhs, d) <= 1e-15
        f = np.flatnonzero(mask)
        Mf = H[np.ix_(f, f)] + lam * np.diag(np.diag(H)[f])
        assert np.allclose(Mf @ d[f], -g[f], rtol=0, atol=1e-9 * np.max(np.abs(g)))
        # a perturbed step has a backward error of the perturbation's size, whatever the conditioning
        assert R.backward_error(M, rhs, d * (1 + 1e-9)) > 1e-11
    # the predicted reduction of the damped model
    dvec, gm, delta = np.array([2.0, 0.0, 1.0]), np.array([1.0, 5.0, -2.0]), np.array([1.0, 0.0, 2.0])
    assert R.predicted_reduction(0.5, dvec, gm, delta) == 0.5 * (0.5 * (2.0 + 4.0) - (1.0 - 4.0))


def test_reference_decision_rules():
    C = R.make_ctrl()

    def run(c_old, c_new, pred, ctrl=C, **kw):
        t = dict(c_old=c_old, c_new=c_new, pred=pred, gmax=1.0, delta=np.array([3.0, 4.0]), x_free=np.array([9.5]), lam=1.0)
        t.update(kw)
        return R.decide(R.TrialInputs(**t), ctrl)

    assert run(4.0, 2.0, 1.0).lam_next == 0.1                         # rho = 1 > 0.95: the fast factor
    assert run(4.0, 2.0, 1.0, ctrl=R.make_ctrl(fast=(0.0, 0.1))).lam_next == 1.0 / 3.0
    assert run(4.0, 3.0, 1.0).lam_next == 1.0                          # rho = 0.5
    assert run(4.0, 3.0, 1.0).rho == 0.5
    assert run(3.8, 1.9, 1.0).lam_next == 1.0 / 3.0                    # rho = 0.95 exactly: not above the fast threshold
    assert run(3.8, 1.9, 1.0).near_threshold
    assert run(4.0, 2.0, 0.5).lam_next == 0.1                          # rho = 2
    assert run(1.0, 0.5, 1.0).lam_next == 2.0                          # rho = 0.25 exactly: x 2
    assert run(8.0, 6.0, -1.0).lam_next == 2.0 and run(8.0, 6.0, -1.0).accepted
    d = run(8.0, 9.0, 1.0)
    assert d.branch == "reject" and d.lam_next == 1e3 and d.ctrl[R.REJ] == 1 and d.ctrl[R.TRIALS] == 1
    assert run(8.0, 9.0, 1.0, ctrl=R.make_ctrl(lam_grow0=2.0)).lam_next == 2.0
    assert run(8.0, 9.0, 1.0, ctrl=R.make_ctrl(lam_grow0=1.0)).lam_next == 4.0
    assert run(8.0, 9.0, 1.0, ctrl=C + np.eye(12)[R.ACC]).lam_next == 4.0
    assert run(8.0, np.nan, 1.0).branch == "reject" and run(8.0, 6.0, np.inf).branch == "reject" and run(8.0, 8.0, 1.0).branch == "reject"
    assert run(8.0, 6.0, 1.0, status=2).branch == "reject"
    d = run(8.0, 6.0, 1.0, status=4, ctrl=C + np.eye(12)[R.ACC] * 2)
    assert (d.branch, d.code, d.lam_next, d.ctrl[R.ACC], d.ctrl[R.TRIALS]) == ("void", 9, 1.0, 2.0, 1.0)
    assert run(8.0, 6.0, 1.0, votes=1.0).branch == "void"
    assert run(4.0, 3.0, 1.0, lam=1e-12).lam_next == 1e-12 and run(4.0, 2.0, 1.0, lam=5e-12).lam_next == 1e-12
    # tolerances: rel_drop = 1/4, |step| = 5, |x| = 9.5
    assert run(8.0, 6.0, 1.0, ctrl=R.make_ctrl(ftol=0.25)).code == 3
    assert run(8.0, 6.0, 1.0, ctrl=R.make_ctrl(ftol=np.nextafter(0.25, 0))).code == 0
    assert run(8.0, 6.0, 1.0, ctrl=R.make_ctrl(xtol=0.5)).code == 4
    assert run(8.0, 6.0, 1.0, ctrl=R.make_ctrl(xtol=np.nextafter(0.5, 0))).code == 0
    d = run(8.0, 6.0, 1.0, gmax=2.0, ctrl=R.make_ctrl(gtol=2.0))
    assert (d.branch, d.code, d.lam_next) == ("gtol", 1, 1.0)
    assert run(8.0, 6.0, 1.0, ctrl=R.make_ctrl(max_iter=3) + np.eye(12)[R.ACC] * 2).code == 5
    assert run(8.0, 9.0, 1.0, ctrl=C + np.eye(12)[R.REJ] * 11).code == 2


# ------------------------------------------------------------------------------------------------------------ the host loop replayed

FAR, FAR_LAM0 = 30.0, 1e-6     # a start 30 x the rig's perturbation whose first exact step at this damping is rejected


def _rig_problem(scale=1.0):
    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                       fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    intr = rig.intr_true + scale * (rig.intr - rig.intr_true)
    extr = rig.extr_true + scale * (rig.extr - rig.extr_true)
    poses = rig.poses_true + scale * (rig.poses - rig.poses_true)
    x0 = np.concatenate([intr[bp.intr_unfixed].ravel(), extr[bp.extr_unfixed].ravel(), poses[bp.poses_unfixed].ravel()])
    return rig, h, x0


def _cpu_operators(rig, h):
    """The CPU engine (PCG on matrix-free products) and the CPU normal equations (Cholesky) of test_device_lm_driver_logic_on_cpu_operator."""
    import torch
    from pycamset_amd.device_solver import JacobianOperator
    from tools.library_solver import cholesky_step
    det, mask = h._flat_detections(), h._jac_mask()
    counts = orc.counts_from_detections(det)
    idx, ptr, _ = orc.csr_structure("template", det, np.ones(mask.shape[0], bool))

    class CpuEngine:
        n, n_params = det.shape[0], mask.shape[0]

        def linearize(self, ps):
            dense, r = orc.full_jac_dense("template", det, ps, rig.points, with_resid=True, counts=counts)
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

    class CpuNormal:
        free = np.flatnonzero(mask)

        def build(self, ps):
            e = CpuEngine()
            e.linearize(ps)
            Jf = e.J[:, self.free]
            return torch.from_numpy((Jf.T @ Jf).toarray()), torch.from_numpy(Jf.T @ e.r), float(e.r @ e.r)

        solve = staticmethod(cholesky_step)

    return JacobianOperator(CpuEngine(), mask), CpuNormal()


def _logged_solve(monkeypatch, h, x0, operator, linear_solver, **kw):
    """lm_solve with every evaluation and every step of its host loop logged: ("eval", sumsq, g) / ("step", lam, delta, pred)."""
    from pycamset_amd import device_solver as ds
    log = []
    for cls in (ds._PcgStep, ds._CholeskyStep):
        ev, so = cls.evaluate, cls.solve

        def evaluate(self, ps, need_scale=True, _ev=ev):
            st = _ev(self, ps, need_scale)
            log.append(("eval", st["sumsq"], np.array(st["g"], dtype=np.float64)))
            return st

        def solve(self, st, lam, _so=so):
            out = _so(self, st, lam)
            log.append(("step", lam, None if out[0] is None else np.array(out[0], dtype=np.float64), out[2]))
            return out

        monkeypatch.setattr(cls, "evaluate", evaluate)
        monkeypatch.setattr(cls, "solve", solve)
    res = ds.lm_solve(h, x0.copy(), operator=operator, linear_solver=linear_solver, **kw)
    monkeypatch.undo()
    return res, log


def replay(res, log, x0, ctrl):
    """Walk the logged trials through the reference; every decision and every lambda must be the loop's.  Returns the decisions."""
    assert log[0][0] == "eval"
    c_old, g = log[0][1], log[0][2]
    x = x0.copy()
    decisions = []
    i = 1
    lam_expected = None
    while i < len(log):
        _, lam, delta, pred = log[i]
        if lam_expected is not None:
            assert lam == lam_expected, (len(decisions), lam, lam_expected)          # the lambda sequence, bit for bit
        if delta is None:                                                           # the factorisation failed: rejected, not evaluated
            c_new, i = np.nan, i + 1
            inp = R.TrialInputs(c_old=c_old, c_new=np.nan, pred=np.nan, gmax=float(np.max(np.abs(g))), delta=np.zeros_like(x), x_free=x, lam=lam, status=1)
        else:
            assert log[i + 1][0] == "eval"
            c_new, g_new = log[i + 1][1], log[i + 1][2]
            i += 2
            inp = R.TrialInputs(c_old=c_old, c_new=c_new, pred=pred, gmax=float(np.max(np.abs(g))), delta=delta, x_free=x, lam=lam)
        d = R.decide(inp, ctrl)
        k = len(decisions)
        tr = res.trials[k]
        assert not d.near_threshold, k
        assert tr[0] == (1.0 if d.accepted else 0.0) and tr[8] == d.code and tr[9] == d.ctrl[R.TRIALS], (k, tr, d.branch, d.code)
        assert tr[11] == d.lam_next and tr[7] == lam, (k, tr[11], d.lam_next)
        assert tr[5] == c_new or (np.isnan(tr[5]) and np.isnan(c_new))
        for j in (2, 3, 4):
            assert abs(tr[j] - d.stats[j]) <= 1e-13 * abs(d.stats[j]) or (np.isnan(tr[j]) and np.isnan(d.stats[j])), (k, j, tr[j], d.stats[j])
        decisions.append(d)
        ctrl = d.ctrl
        lam_expected = d.lam_next
        if d.accepted:
            x, c_old, g = x + delta, c_new, g_new
    assert len(decisions) == len(res.trials)
    assert res.nfev == 1 + sum(1 for e in log[1:] if e[0] == "eval")
    final = decisions[-1].code if decisions else 0
    if res.status == 1:                 # the host loop tests gtol before it steps: no trial
        assert final == 0 and np.max(np.abs(g)) <= ctrl[R.GTOL]
    else:
        assert {5: 0}.get(final, final) == res.status, (final, res.status, res.message)
    assert np.array_equal(res.x, x)
    return decisions


@pytest.mark.parametrize("linear_solver", ["pcg", "cholesky"])
@pytest.mark.parametrize("case", ["near", "far30", "max_iter-3", "xtol"])
def test_host_loop_follows_the_reference(monkeypatch, linear_solver, case):
    rig, h, x0 = _rig_problem(FAR if case == "far30" else 1.0)
    pcg_op, chol_op = _cpu_operators(rig, h)
    kw = dict(max_iter=25)
    if case == "far30":
        kw["lam0"] = FAR_LAM0
    if case == "max_iter-3":
        kw.update(max_iter=3, ftol=0.0, xtol=0.0, gtol=0.0)
    if case == "xtol":
        kw.update(ftol=0.0, xtol=1e-5)
    op = pcg_op if linear_solver == "pcg" else chol_op
    res, log = _logged_solve(monkeypatch, h, x0, op, linear_solver, **kw)
    from pycamset_amd.device_solver import LAM_FAST, LAM_GROW0
    ctrl = R.make_ctrl(max_iter=kw["max_iter"], ftol=kw.get("ftol", 1e-8), xtol=kw.get("xtol", 1e-8), gtol=kw.get("gtol", 1e-8), lam_grow0=LAM_GROW0,
                       fast=(0.0, 0.0) if linear_solver == "pcg" else LAM_FAST)
    ds = replay(res, log, x0, ctrl)
    codes = [d.code for d in ds]
    if case == "max_iter-3":
        assert codes[-1] == 5 and sum(d.accepted for d in ds) == 3
    if case == "xtol":
        assert codes[-1] == 4
    if case == "far30" and linear_solver == "cholesky":
        assert ds[0].branch == "reject" and any(d.accepted for d in ds)
        assert res.trials[0][11] == FAR_LAM0 * LAM_GROW0


def test_first_rejection_multiplies_by_lam_grow0(monkeypatch):
    """lm_solve's docstring: a rejection BEFORE the first accepted step multiplies lambda by lam_grow0 — also for 1 < lam_grow0 < 4,
    where the host loop (PCG and Cholesky operators alike) used max(lam_grow0, 4)."""
    rig, h, x0 = _rig_problem(FAR)
    _, chol_op = _cpu_operators(rig, h)
    res, log = _logged_solve(monkeypatch, h, x0, chol_op, "cholesky", max_iter=25, lam0=FAR_LAM0, lam_grow0=2.0)
    from pycamset_amd.device_solver import LAM_FAST
    ctrl = R.make_ctrl(max_iter=25, lam_grow0=2.0, fast=LAM_FAST)
    ds = replay(res, log, x0, ctrl)
    assert ds[0].branch == "reject", "the first trial from this start is rejected"
    assert any(d.accepted for d in ds)
    steps = [e for e in log if e[0] == "step"]
    assert res.trials[0][11] == 2.0 * FAR_LAM0 and steps[1][1] == 2.0 * FAR_LAM0
    first_acc = next(k for k, d in enumerate(ds) if d.accepted)
    assert all(res.trials[k][11] == 2.0 * res.trials[k][7] for k in range(first_acc))
    later = [k for k in range(first_acc + 1, len(ds)) if ds[k].branch == "reject"]
    assert all(res.trials[k][11] == 4.0 * res.trials[k][7] for k in later)
