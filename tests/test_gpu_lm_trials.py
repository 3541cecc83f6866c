"""The device Levenberg-Marquardt loop trial by trial against the plain reference of tests/lm_reference.py.

A: lm_decide_kernel (pcs_lm_trial_finish) on hand-filled inputs, one row per branch, at sizes below, at and well above one workgroup.
B: real solves driven one trial at a time (pcs_lm_trial + a synchronisation): the step against the device's own system (backward
   error) and the oracle's normal equations, the costs and stats against the reference, the decision against ``decide``, the
   hand-off from trial to trial.
C: the real loops (device-steered with speculation, host-steered) reproduce the stepwise drive; the fused and the separate launches of a trial
   (engine option "fused_trial") give the same bits.
D: every stop code on a real problem."""
import numpy as np
import pytest

from oracle import ba_oracle as orc
from pycamset_amd import synthetic
from tests import lm_reference as R
from tests.test_host_logic import DuckCamset, DuckTarget

pytestmark = pytest.mark.gpu
nxt = np.nextafter


def _report(capsys, name, labels, near=0):
    with capsys.disabled():
        print(f"\n[{name}] branches: {', '.join(sorted(labels))}; near-threshold trials: {near}")


def _label(d: R.Decision, ctrl) -> str:
    if d.branch == "accept":
        f = R.gain_factor(d.rho, ctrl)
        band = "fast" if (ctrl[R.FAST_RHO] > 0 and ctrl[R.FAST_FAC] > 0 and d.rho > ctrl[R.FAST_RHO]) else {1.0 / 3.0: "x1/3", 1.0: "x1", 2.0: "x2"}[f]
        return f"accept:{band}" + (":floor" if d.lam_next == R.LAM_FLOOR else "")
    if d.branch == "reject":
        return "reject:grow0" if ctrl[R.ACC] == 0.0 and ctrl[R.GROW0] > 1.0 else "reject:x4"
    return d.branch


# =============================================================================================== A: the decision kernel, crafted rows

def _rig_engine(n_cams, n_keys):
    """A free-point engine (15 per camera + 3 per point) sized through the rig's dimensions; the decision reads no detections."""
    from pycamset_amd.engine import Engine
    return Engine("free", n_cams, 0, n_keys)


SIZES = [(1, 10), (2, 323), (2, 5600)]     # n_params 45, 999, 16 830: below, at and well above 1024 threads / 16 waves


class Table:
    """One engine + solver state; every row fills all inputs, runs pcs_lm_trial_finish and reads every output back."""

    def __init__(self, n_cams, n_keys):
        import torch
        from pycamset_amd.device_solver import BlockedNormalEquations
        self.torch = torch
        self.eng = _rig_engine(n_cams, n_keys)
        n = self.n = self.eng.n_params
        mask = np.ones(n, bool)
        mask[::1024] = False                       # fixed at the start and at 1024-strides ...
        mask[-1] = False                           # ... and at the end
        self.mask = mask
        self.ne = BlockedNormalEquations(self.eng, mask)
        self.free = np.flatnonzero(mask)
        self.np_ = self.ne.n_packed
        # the free entries a row puts its step, its gradient and its x on: far apart, across wave and workgroup-stride boundaries
        f = self.free
        self.i1, self.i2, self.ig, self.ix = int(f[len(f) // 3]), int(f[-1]), int(f[len(f) // 2]), int(f[1])

    def run(self, *, c_old, c_new, g2=-0.5, gmax=1e3, x=9.5, lam=1.0, status=0, vote=0.0, ctrl=None, mode=0, sel=0, stop_raised=False,
            result=True, dvec_step=0.0, rng_seed=0):
        from pycamset_amd._capi import LM_VOTES
        torch = self.torch
        dev = self.ne.dev
        n, npk = self.n, self.np_
        rng = np.random.default_rng(rng_seed)
        ctrl = R.make_ctrl() if ctrl is None else np.array(ctrl, dtype=np.float64)
        # inputs: delta = (3, 4) at two free entries (|step| = 5), gm = g2 under the 4 and gmax elsewhere, dvec positive elsewhere
        delta = np.zeros(n)
        delta[self.i1], delta[self.i2] = 3.0, 4.0
        gm = np.zeros(n)
        gm[self.i2], gm[self.ig] = g2, gmax
        dvec = rng.uniform(0.5, 2.0, n)
        dvec[[self.i1, self.i2]] = dvec_step
        ps = [rng.uniform(-1e3, 1e3, n) for _ in range(2)]
        for p in ps:
            p[self.mask] = 0.0
            p[self.ix] = x                          # |x| over the free entries is |x|; the fixed ones hold large values
        packed = [rng.standard_normal(npk + 1) for _ in range(2)]
        cur = sel
        tri = 1 - cur if not (mode & 1) else 1
        if mode & 1:
            cur = 0
        packed[cur][npk - 1], packed[tri][npk - 1] = c_old, c_new
        packed[tri][npk] = vote
        packed[cur][npk] = 0.0
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for s in range(2):
                self.ne.packed[s].copy_(torch.from_numpy(packed[s]))
            d_ps = [torch.from_numpy(p.copy()).to(dev) for p in ps]
            self.ne.delta.copy_(torch.from_numpy(delta))
            self.ne.gm.copy_(torch.from_numpy(gm))
            self.ne.dvec.copy_(torch.from_numpy(dvec))
            self.ne.status.fill_(status)
            d_lam = torch.full((1,), lam, **f64)
            d_ctrl = torch.from_numpy(ctrl.copy()).to(dev)
            flags = torch.tensor([1 if stop_raised else 0, 0, sel, 0], dtype=torch.int32, device=dev)
            pattern = np.arange(12, dtype=np.float64) + 100.0
            stats = torch.from_numpy(pattern.copy()).to(dev)
            stats_host = torch.full((12,), np.nan, dtype=torch.float64).pin_memory()
            nf = self.free.shape[0]
            result_host = torch.full((2 * nf + 1,), np.nan, dtype=torch.float64).pin_memory() if result else None
            torch.cuda.synchronize()
            b = self.ne.lm_buffers(d_ps, d_lam, d_ctrl, flags, stats, stats_host, result_host, mode=mode)
            self.eng.lm_trial_finish(b, self.ne.stream.cuda_stream)
            self.ne.stream.synchronize()
            out = dict(stats=stats.cpu().numpy(), stats_host=stats_host.numpy().copy(), lam=float(d_lam.item()), ctrl=d_ctrl.cpu().numpy(),
                       flags=flags.cpu().numpy(), status=int(self.ne.status.item()), ps=[p.cpu().numpy() for p in d_ps],
                       packed=[p.cpu().numpy() for p in self.ne.packed], result=result_host.numpy().copy() if result else None)
        inputs = R.TrialInputs(c_old=c_old, c_new=c_new, pred=R.predicted_reduction(lam, dvec, gm, delta), gmax=float(np.nanmax(np.abs(gm))),
                               delta=delta[self.mask], x_free=ps[cur][self.mask], lam=lam, status=status, votes=vote if mode & LM_VOTES else 0.0)
        return out, inputs, ctrl, dict(ps=ps, packed=packed, cur=cur, tri=tri, gm=gm, pattern=pattern)

    def check(self, name, expect=None, **kw):
        out, inp, ctrl, src = self.run(**kw)
        d = R.decide(inp, ctrl)
        if expect is not None:
            assert (d.branch, d.code) == expect[:2], (name, d.branch, d.code, expect)
        mode, cur, tri = kw.get("mode", 0), src["cur"], src["tri"]
        if kw.get("stop_raised") or ctrl[R.STOP] != 0.0:
            assert np.all(out["stats_host"] == -1.0), (name, out["stats_host"])
            want = src["pattern"].copy()
            want[9] = -1.0
            assert np.array_equal(out["stats"], want, equal_nan=True), (name, out["stats"])
            assert out["lam"] == kw.get("lam", 1.0) and np.array_equal(out["ctrl"], ctrl, equal_nan=True), name
            assert out["flags"][1] == 0 and out["flags"][2] == kw.get("sel", 0), name
            assert out["status"] == kw.get("status", 0), name
            for s in range(2):
                assert np.array_equal(out["ps"][s], src["ps"][s], equal_nan=True) and np.array_equal(out["packed"][s], src["packed"][s], equal_nan=True), name
            return d
        acc = d.branch == "accept"
        now = tri if (acc and not (mode & 1)) else cur
        want = d.stats.copy()
        want[10] = now
        st = out["stats"]
        same = (st == want) | (np.isnan(st) & np.isnan(want))
        # the norms are sums in another order: equal to the reference within 1e-13 (exact for the rows' representable values)
        for i in (3, 4):
            same[i] = abs(st[i] - want[i]) <= 1e-13 * abs(want[i])
        assert np.all(same), (name, st, want)
        hs = out["stats_host"]
        assert np.all((hs == st) | (np.isnan(hs) & np.isnan(st))), (name, hs, st)
        assert out["lam"] == d.lam_next, (name, out["lam"], d.lam_next)
        for i in (R.STOP, R.REJ, R.ACC, R.TRIALS):
            assert out["ctrl"][i] == d.ctrl[i], (name, i, out["ctrl"], d.ctrl)
        assert list(out["flags"][:3]) == [int(d.code != 0), int(acc), now], (name, out["flags"], d.code, acc, now)
        assert out["status"] == 0, name
        if mode & 1:                            # fixed trial buffer: an accepted trial is copied over state 0, nothing flips
            if acc:
                assert np.array_equal(out["packed"][0][: self.np_], src["packed"][1][: self.np_], equal_nan=True), name
                assert out["packed"][0][self.np_] == src["packed"][0][self.np_], name           # the vote word is not part of the copy
                assert np.array_equal(out["ps"][0], src["ps"][1], equal_nan=True), name
            else:
                assert np.array_equal(out["packed"][0], src["packed"][0], equal_nan=True) and np.array_equal(out["ps"][0], src["ps"][0], equal_nan=True), name
        else:
            for s in range(2):
                assert np.array_equal(out["packed"][s], src["packed"][s], equal_nan=True) and np.array_equal(out["ps"][s], src["ps"][s], equal_nan=True), name
        if out["result"] is not None:
            if d.code != 0:                     # the final state: g | ps at the free entries | cost of the state the loop ends in
                fin = tri if acc else cur
                g0 = self.np_ - 1 - self.n
                pk = src["packed"][fin]
                want_r = np.concatenate([pk[g0: g0 + self.n][self.mask], src["ps"][fin][self.mask], [pk[self.np_ - 1]]])
                assert np.array_equal(out["result"], want_r, equal_nan=True), name
            else:
                assert np.all(np.isnan(out["result"])), name
        return d


def _table_rows():
    """(name, kwargs, (branch, code) the documented rules give)."""
    C = R.make_ctrl
    rows = []

    def rho_row(name, r, expect=("accept", 0), **kw):    # pred = 1 (gm = -0.5 under delta = 4), actual = r exactly, rel_drop = 1/2
        rows.append((name, dict(c_old=4.0 * r, c_new=2.0 * r, **kw), expect))

    for r in (0.1, 0.25, nxt(0.25, 1.0), 0.5, 0.75, nxt(0.75, 1.0), 0.9, 0.95, nxt(0.95, 1.0), 1.5):
        rho_row(f"rho={r!r}", r)
    rho_row("rho=0.97, fast off", 0.97, ctrl=C(fast=(0.0, 0.1)))
    rho_row("rho=0.97, fast factor 0", 0.97, ctrl=C(fast=(0.95, 0.0)))
    rho_row("rho=0.6, fast threshold 0.5", 0.6, ctrl=C(fast=(0.5, 0.1)))
    rows.append(("pred<0 accepted", dict(c_old=8.0, c_new=6.0, g2=0.5), ("accept", 0)))
    rows.append(("pred=0 accepted", dict(c_old=8.0, c_new=6.0, g2=0.0), ("accept", 0)))
    rows.append(("pred from D", dict(c_old=8.0, c_new=6.0, g2=0.25, dvec_step=0.5, lam=2.0), ("accept", 0)))
    # rejections
    rows.append(("actual=0", dict(c_old=8.0, c_new=8.0), ("reject", 0)))
    rows.append(("actual<0", dict(c_old=8.0, c_new=9.0), ("reject", 0)))
    rows.append(("c_new NaN", dict(c_old=8.0, c_new=np.nan), ("reject", 0)))
    rows.append(("c_new +inf", dict(c_old=8.0, c_new=np.inf), ("reject", 0)))
    rows.append(("c_new -1e300", dict(c_old=8.0, c_new=-1e300), ("reject", 0)))
    rows.append(("pred NaN", dict(c_old=8.0, c_new=6.0, g2=np.nan), ("reject", 0)))
    rows.append(("pred +inf", dict(c_old=8.0, c_new=6.0, g2=-np.inf), ("reject", 0)))
    rows.append(("pred -inf", dict(c_old=8.0, c_new=6.0, g2=np.inf), ("reject", 0)))
    rows.append(("status 1", dict(c_old=8.0, c_new=6.0, status=1), ("reject", 0)))
    rows.append(("status 2", dict(c_old=8.0, c_new=6.0, status=2), ("reject", 0)))
    rows.append(("status 4 void", dict(c_old=8.0, c_new=6.0, status=4, ctrl=C() + np.eye(12)[R.REJ] * 3 + np.eye(12)[R.ACC] * 2), ("void", 9)))
    rows.append(("vote 1 void", dict(c_old=8.0, c_new=6.0, vote=1.0, mode=2), ("void", 9)))
    rows.append(("vote 0", dict(c_old=8.0, c_new=6.0, vote=0.0, mode=2), ("accept", 0)))
    rows.append(("vote ignored without PCS_LM_VOTES", dict(c_old=8.0, c_new=6.0, vote=1.0, mode=0), ("accept", 0)))
    # the first rejection: lam_grow0 while nothing was accepted, x 4 otherwise
    for g0 in (1e3, 2.0, 1.0, 0.5):
        rows.append((f"first rejection, lam_grow0={g0}", dict(c_old=8.0, c_new=9.0, ctrl=C(lam_grow0=g0)), ("reject", 0)))
    rows.append(("rejection after an acceptance, lam_grow0=1e3", dict(c_old=8.0, c_new=9.0, ctrl=C(lam_grow0=1e3) + np.eye(12)[R.ACC]), ("reject", 0)))
    rows.append(("rejection after an acceptance, lam_grow0=2", dict(c_old=8.0, c_new=9.0, ctrl=C(lam_grow0=2.0) + np.eye(12)[R.ACC] * 3), ("reject", 0)))
    # the lambda floor
    rho_row("floor, x1/3", 0.9, lam=1e-12)
    rho_row("floor, fast", 0.99, lam=5e-12)
    rho_row("no floor needed", 0.9, lam=6e-12)
    rho_row("floor not for x2", 0.1, lam=1e-12)
    rows.append(("rejection below the floor", dict(c_old=8.0, c_new=9.0, lam=1e-13, ctrl=C() + np.eye(12)[R.ACC]), ("reject", 0)))
    # tolerances at exact equality and one ulp beyond: rel_drop = 1/4 (c 8 -> 6), |step| = 5, |x| = 9.5, max |g| = 2
    rows.append(("ftol ==", dict(c_old=8.0, c_new=6.0, ctrl=C(ftol=0.25)), ("accept", 3)))
    rows.append(("ftol one ulp below", dict(c_old=8.0, c_new=6.0, ctrl=C(ftol=nxt(0.25, 0.0))), ("accept", 0)))
    rows.append(("xtol ==", dict(c_old=8.0, c_new=6.0, ctrl=C(xtol=0.5)), ("accept", 4)))
    rows.append(("xtol one ulp below", dict(c_old=8.0, c_new=6.0, ctrl=C(xtol=nxt(0.5, 0.0))), ("accept", 0)))
    rows.append(("xtol wins over the iteration limit", dict(c_old=8.0, c_new=6.0, ctrl=C(xtol=0.5, max_iter=1)), ("accept", 4)))
    rows.append(("ftol wins over xtol", dict(c_old=8.0, c_new=6.0, ctrl=C(ftol=0.25, xtol=0.5)), ("accept", 3)))
    rows.append(("gtol ==", dict(c_old=8.0, c_new=6.0, gmax=2.0, ctrl=C(gtol=2.0)), ("gtol", 1)))
    rows.append(("gtol one ulp below", dict(c_old=8.0, c_new=6.0, gmax=2.0, ctrl=C(gtol=nxt(2.0, 0.0))), ("accept", 0)))
    rows.append(("gtol on a rejected trial", dict(c_old=8.0, c_new=9.0, gmax=2.0, ctrl=C(gtol=2.0) + np.eye(12)[R.REJ] * 11), ("gtol", 1)))
    # the limits on their last count
    rows.append(("iteration limit", dict(c_old=8.0, c_new=6.0, ctrl=C(max_iter=5) + np.eye(12)[R.ACC] * 4), ("accept", 5)))
    rows.append(("iteration limit not yet", dict(c_old=8.0, c_new=6.0, ctrl=C(max_iter=5) + np.eye(12)[R.ACC] * 3), ("accept", 0)))
    rows.append(("rejection limit", dict(c_old=8.0, c_new=9.0, ctrl=C() + np.eye(12)[R.REJ] * 11 + np.eye(12)[R.ACC]), ("reject", 2)))
    rows.append(("rejection limit not yet", dict(c_old=8.0, c_new=9.0, ctrl=C() + np.eye(12)[R.REJ] * 10), ("reject", 0)))
    rows.append(("acceptance clears the rejections", dict(c_old=8.0, c_new=6.0, ctrl=C() + np.eye(12)[R.REJ] * 11 + np.eye(12)[R.TRIALS] * 7), ("accept", 0)))
    # the state words: state 1 current; a fixed trial buffer (copy instead of flip)
    rows.append(("sel=1 accepted", dict(c_old=8.0, c_new=6.0, sel=1), ("accept", 0)))
    rows.append(("sel=1 rejected", dict(c_old=8.0, c_new=9.0, sel=1), ("reject", 0)))
    rows.append(("fixed buffer accepted", dict(c_old=8.0, c_new=6.0, mode=1), ("accept", 0)))
    rows.append(("fixed buffer accepted, ends the loop", dict(c_old=8.0, c_new=6.0, mode=1, ctrl=C(ftol=0.25)), ("accept", 3)))
    rows.append(("fixed buffer rejected", dict(c_old=8.0, c_new=9.0, mode=1), ("reject", 0)))
    rows.append(("fixed buffer + votes", dict(c_old=8.0, c_new=6.0, mode=3, vote=0.0), ("accept", 0)))
    rows.append(("rejection limit, state 1 current", dict(c_old=8.0, c_new=9.0, sel=1, ctrl=C() + np.eye(12)[R.REJ] * 11), ("reject", 2)))
    rows.append(("no result buffer", dict(c_old=8.0, c_new=6.0, result=False, ctrl=C(ftol=0.25)), ("accept", 3)))
    # the flag already raised: nothing happens but the -1 read-back
    rows.append(("stop raised", dict(c_old=8.0, c_new=6.0, stop_raised=True, ctrl=C() + np.eye(12)[R.STOP] * 3, sel=1, status=1), None))
    return rows


@pytest.mark.parametrize("size", SIZES, ids=[f"{c}cam-{k}pts" for c, k in SIZES])
def test_decision_kernel_on_crafted_rows(size, capsys):
    t = Table(*size)
    assert t.np_ % 2 == 1, "an odd n_packed: lm_accept_kernel's scalar tail"
    assert t.n > 64 or size == SIZES[0]
    labels, codes = set(), set()
    for name, kw, expect in _table_rows():
        d = t.check(name, expect=expect, **kw)
        ctrl = R.make_ctrl() if kw.get("ctrl") is None else kw["ctrl"]
        if expect is not None:
            labels.add(_label(d, ctrl))
            codes.add(d.code)
    with capsys.disabled():
        print(f"\n[table n_params={t.n}, n_packed={t.np_}] branches: {', '.join(sorted(labels))}; stop codes {sorted(codes)}")
    # every band, code and flag of the rules
    for want in ("accept:x2", "accept:x1", "accept:x1/3", "accept:fast", "accept:x1/3:floor", "accept:fast:floor", "reject:grow0", "reject:x4", "gtol", "void"):
        assert want in labels, (want, labels)
    assert codes == {0, 1, 2, 3, 4, 5, 9}, codes
    t.eng.close()


# ======================================================================================== B: real solves, one trial at a time

def _ring8(chain="template", scale=1.0, outliers=False):
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    det = rig.detections
    if outliers:   # the robust solve starts where the linear one ended (test_robust_solve_matches_scipy_and_resists_outliers)
        from pycamset_amd.device_solver import lm_solve
        from tests.test_gpu_robust_loss import _outlier_problem
        rig, h, x0 = _outlier_problem(chain)
        return rig, h, lm_solve(h, x0.copy(), max_iter=60).x
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, det),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    intr = rig.intr_true + scale * (rig.intr - rig.intr_true)
    extr = rig.extr_true + scale * (rig.extr - rig.extr_true)
    poses = rig.poses_true + scale * (rig.poses - rig.poses_true)
    parts = [intr[bp.intr_unfixed].ravel(), extr[bp.extr_unfixed].ravel(), poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return rig, h, np.concatenate(parts)


def _config1_free():
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    rig = synthetic.config_rig(1)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.FreePointBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                        fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.points.ravel()[bp.bdpt_unfixed]]
    return rig, h, np.concatenate(parts)


def _genchain(dense):
    from pycamset_amd import function_blocks as fb
    from pycamset_amd import handlers
    rig = synthetic.make_rig("gen-lm", 4, 10, synthetic.charuco_points(7, 8.0), seed=61, visibility=0.9)
    det = rig.detections
    rng = np.random.default_rng(5)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()
    second = np.concatenate([rng.normal(0, 0.02, (rig.n_imgs, 3)), rng.normal(0, 0.002, (rig.n_imgs, 3))], axis=1)
    ps_true = op.build_param_list(rig.intr_true, rig.extr_true, second, rig.poses_true)
    uv = op.make_full_loss_fn(det, 1)(ps_true, rig.points) + det[:, 3:]
    det = det.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()
    fix_ext = np.ones((rig.n_cams, 6), dtype=bool)
    fix_ext[0] = False
    fix_second = np.zeros((rig.n_imgs, 6), dtype=bool)
    fix_second[1:] = True
    start = [rig.intr_true * (1 + 1e-2 * rng.standard_normal(rig.intr_true.shape)), rig.extr_true + 1e-2 * rng.standard_normal(rig.extr_true.shape),
             second + 1e-2 * rng.standard_normal(second.shape), rig.poses_true + 1e-2 * rng.standard_normal(rig.poses_true.shape)]
    start[1][0] = rig.extr_true[0]
    start[2][0] = second[0]
    prob = handlers.ChainProblem(op, det, start, template=rig.points, unfixed=[None, fix_ext, fix_second, None])
    eng = op._engine_for(prob._flat_detections())
    eng.set_option("dense_normal", 1 if dense else 0)
    return rig, prob, prob.x0.copy()


class Fixture:
    """A handler's solver state, the oracle's normal equations at any parameter string, and the loop's control block."""

    def __init__(self, h, x0, chain, template=None, loss="linear", f_scale=1.0, deterministic=False):
        from pycamset_amd.device_solver import _blocked_solver
        from pycamset_amd.engine import Engine
        self.h, self.chain, self.template, self.loss, self.f_scale = h, chain, template, loss, f_scale
        op_fun = h.op_fun
        det = h._flat_detections()
        self.det = det
        eng = self.eng = op_fun._engine_for(det)
        op_fun._bind_template(eng, h._template_arg())
        self.mask = np.asarray(h._jac_mask(), dtype=bool)
        self.generated = not isinstance(eng, Engine)
        if not self.generated:
            eng.set_loss(loss, f_scale)
        eng.set_option("deterministic", int(deterministic))
        self.ne = _blocked_solver(eng, self.mask, None, loss, f_scale)
        self.ne.spd_algorithm = "auto"
        self.ps0 = op_fun.build_param_list(*h.get_bundle_adjustment_inputs(np.array(x0, dtype=np.float64)))
        self.lay = eng.normal_layout()
        if self.generated:
            self.loss_fn, self.jac_fn = h.make_loss_fun(), h.make_loss_jac()

    def close(self):
        if not self.generated:
            self.eng.set_loss("linear", 1.0)
        self.eng.set_option("deterministic", 0)

    def oracle(self, ps):
        """(H over the free entries, g over the free entries, cost, slack of H) at the parameter string ps."""
        if self.generated:
            Hf, gf, c = R.reference_normal_closure(self.loss_fn, self.jac_fn, ps[self.mask])
            return Hf, gf, c, 0.0
        Hh, g, c, slack = R.reference_normal(self.chain, self.det, ps, self.template, loss=self.loss, f_scale=self.f_scale, with_slack=True)
        m = self.mask
        return Hh[np.ix_(m, m)], g[m], c, (slack[np.ix_(m, m)] if np.ndim(slack) else slack)

    def oracle_cost(self, ps):
        if self.generated:
            r = self.loss_fn(ps[self.mask])
            return float(r @ r)
        r = orc.full_loss(self.chain, self.det, ps, self.template).reshape(-1)
        if self.loss == "linear":
            return float(r @ r)
        from scipy.optimize._lsq.least_squares import construct_loss_function
        return float(np.sum(construct_loss_function(r.size, self.loss, self.f_scale)(r, cost_only=False)[0]))


def stepwise(fx: Fixture, ctrl, lam0, max_trials=80):
    """Drive fx's solver state with pcs_lm_trial one trial at a time; per trial everything the checks need."""
    import torch
    ne, eng = fx.ne, fx.eng
    npk = ne.n_packed
    recs = []
    with torch.cuda.device(ne.dev), torch.cuda.stream(ne.stream):
        ps = [torch.from_numpy(fx.ps0.copy()).to(ne.dev), None]
        ps[1] = torch.empty_like(ps[0])
        lam = torch.full((1,), float(lam0), dtype=torch.float64, device=ne.dev)
        d_ctrl = torch.from_numpy(np.array(ctrl, dtype=np.float64)).to(ne.dev)
        flags = torch.zeros(4, dtype=torch.int32, device=ne.dev)
        stats = torch.zeros(12, dtype=torch.float64, device=ne.dev)
        ne.build(ps[0], 0)
        ne.stream.synchronize()
        fixed_buffer = bool(getattr(eng, "lm_fixed_trial_buffer", False))
        for _ in range(max_trials):
            cur = int(flags[2].item())
            tri = 1 if fixed_buffer else 1 - cur
            rec = dict(cur=cur, tri=tri, ps_cur=ps[cur].cpu().numpy(), pk_cur=ne.packed[cur][:npk].cpu().numpy(), lam=float(lam.item()),
                       ctrl=d_ctrl.cpu().numpy(), sel=cur)
            eng.lm_trial(ne.lm_buffers(ps, lam, d_ctrl, flags, stats), ne.stream.cuda_stream)
            ne.stream.synchronize()
            rec.update(delta=ne.delta.cpu().numpy(), dvec=ne.dvec.cpu().numpy(), gm=ne.gm.cpu().numpy(), ps_tri=ps[tri].cpu().numpy(),
                       c_new=float(ne.packed[tri][npk - 1].item()), stats=stats.cpu().numpy(), lam_after=float(lam.item()),
                       ctrl_after=d_ctrl.cpu().numpy(), flags=flags.cpu().numpy())
            recs.append(rec)
            if rec["flags"][0]:
                break
    return recs


def check_trials(fx: Fixture, recs, *, with_oracle=True):
    """Every check of part B on every trial; returns (labels reached, near-threshold trials)."""
    m = fx.mask
    labels, near = set(), 0
    fixed_buffer = bool(getattr(fx.eng, "lm_fixed_trial_buffer", False))
    for k, rc in enumerate(recs):
        Hd, gd, c_old = R.unpack_blocks(rc["pk_cur"], fx.lay)
        delta = rc["delta"]
        # the step: exactly 0 where fixed, the trial string is ps + delta bit for bit, backward stable for the device's own system
        assert np.all(delta[~m] == 0.0), k
        assert np.array_equal(rc["ps_tri"], rc["ps_cur"] + delta), k
        assert np.array_equal(rc["dvec"][m], np.maximum(np.diag(Hd)[m], 1e-300)), k
        assert np.array_equal(rc["gm"][m], gd[m]) and np.all(rc["gm"][~m] == 0.0), k
        M, rhs = R.masked_system(Hd, gd, m, rc["lam"])
        eta = R.backward_error(M, rhs, delta)
        assert eta <= 1e-13, (k, eta)
        if with_oracle:
            Hf, gf, cf, slack = fx.oracle(rc["ps_cur"])
            Hdf = Hd[np.ix_(m, m)]
            scale = np.sqrt(np.outer(np.diag(Hf), np.diag(Hf)))
            assert np.all(np.abs(Hdf - Hf) <= 1e-10 * scale + slack + 1e-300), (k, float(np.max(np.abs(Hdf - Hf) / (scale + 1e-300))))
            assert np.max(np.abs(gd[m] - gf)) <= 1e-10 * max(np.max(np.abs(gf)), np.sqrt(np.max(np.diag(Hf)) * max(float(gf @ gf), 1e-300))), k
            assert abs(c_old - cf) <= 1e-10 * cf, (k, c_old, cf)
            if np.isfinite(rc["c_new"]):
                cn = fx.oracle_cost(rc["ps_tri"])
                assert abs(rc["c_new"] - cn) <= 1e-10 * cn, (k, rc["c_new"], cn)
        st = rc["stats"]
        inp = R.TrialInputs(c_old=c_old, c_new=rc["c_new"], pred=R.predicted_reduction(rc["lam"], rc["dvec"], rc["gm"], delta),
                            gmax=float(np.max(np.abs(rc["gm"]))), delta=delta[m], x_free=rc["ps_cur"][m], lam=rc["lam"])
        d = R.decide(inp, rc["ctrl"])
        assert st[6] == c_old and st[5] == rc["c_new"] and st[7] == rc["lam"], k
        for i in (1, 2, 3, 4):
            assert abs(st[i] - d.stats[i]) <= 1e-13 * abs(d.stats[i]) or (np.isnan(st[i]) and np.isnan(d.stats[i])), (k, i, st[i], d.stats[i])
        near += int(d.near_threshold)
        if not d.near_threshold:
            assert st[0] == d.stats[0] and st[8] == d.code and st[9] == d.ctrl[R.TRIALS], (k, st, d.stats, d.branch)
            assert st[11] == d.lam_next == rc["lam_after"], (k, st[11], d.lam_next, rc["lam_after"])
            for i in (R.STOP, R.REJ, R.ACC, R.TRIALS):
                assert rc["ctrl_after"][i] == d.ctrl[i], (k, i)
        acc = st[0] > 0
        flip = acc and not fixed_buffer
        assert rc["flags"][2] == (rc["tri"] if flip else rc["cur"]) and st[10] == rc["flags"][2], k
        labels.add(_label(d, rc["ctrl"]))
        if d.code:
            labels.add(f"stop:{R.CODES[d.code]}")
        if k + 1 < len(recs):
            nx = recs[k + 1]
            _, _, c_next = R.unpack_blocks(nx["pk_cur"], fx.lay)
            assert c_next == (rc["c_new"] if acc else c_old), k
            assert np.array_equal(nx["ps_cur"], rc["ps_tri"] if acc else rc["ps_cur"]), k
            assert nx["lam"] == rc["lam_after"], k
    return labels, near


FIXTURES = {
    # name: (builder, chain, loss, lam0, ctrl overrides, branches it must reach)
    "ring8-template-near": (lambda: _ring8("template"), "template", "linear", 1e-5, {}, [{"accept:fast", "accept:x1/3"}, {"stop:ftol", "stop:xtol"}]),
    # 20 x the rig's perturbation at lambda0 = 1e-9: the first exact steps overshoot (10 x is still accepted at any lambda0)
    "ring8-template-far20": (lambda: _ring8("template", 20.0), "template", "linear", 1e-9, {}, [{"reject:grow0"}, {"accept:fast"}, {"reject:x4"}]),
    "ring8-self-gauge": (lambda: _ring8("self"), "self", "linear", 1e-5, {}, [{"accept:fast", "accept:x1/3", "accept:x1"}]),
    "config1-free": (_config1_free, "free", "linear", 1e-5, {}, [{"accept:fast", "accept:x1/3", "accept:x1"}]),
    "ring8-huber": (lambda: _ring8("template", outliers=True), "template", "huber", 1e-5, {}, [{"accept:fast", "accept:x1/3", "accept:x1"}]),
    "genchain-blocked": (lambda: _genchain(False), "generated", "linear", 1e-5, {}, [{"accept:fast", "accept:x1/3", "accept:x1"}]),
    "genchain-dense": (lambda: _genchain(True), "generated", "linear", 1e-5, {}, [{"accept:fast", "accept:x1/3", "accept:x1"}]),
}


def _fixture(name, deterministic=False):
    build, chain, loss, lam0, over, _ = FIXTURES[name]
    rig, h, x0 = build()
    tm = rig.points if chain == "template" else None
    fx = Fixture(h, x0, chain, tm, loss=loss, deterministic=deterministic)
    return fx, x0, lam0, R.make_ctrl(max_iter=30, **over)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_every_trial_of_a_real_solve(name, capsys):
    fx, x0, lam0, ctrl = _fixture(name)
    try:
        if name == "ring8-self-gauge":
            assert fx.lay["n_trail"] > 0 and fx.lay["tb"] == 3          # the points are the trailing entities
        if name == "genchain-dense":
            assert fx.lay["n_trail"] == 0
        if name == "genchain-blocked":
            assert fx.lay["n_trail"] > 0
        recs = stepwise(fx, ctrl, lam0)
        assert recs[-1]["flags"][0] == 1, "the loop ended"
        labels, near = check_trials(fx, recs)
        _report(capsys, name, labels, near)
        assert near == 0, (name, near)
        for need in FIXTURES[name][5]:
            assert labels & need, (name, need, labels)
    finally:
        fx.close()


# ================================================================================ C: the real loops reproduce the stepwise drive

@pytest.mark.parametrize("name", ["ring8-template-far20", "ring8-self-gauge", "genchain-blocked"])
def test_loops_reproduce_the_stepwise_drive(name):
    from pycamset_amd.device_solver import lm_solve
    fx, x0, lam0, ctrl = _fixture(name, deterministic=True)
    try:
        recs = stepwise(fx, ctrl, lam0)
    finally:
        fx.close()
    want = np.array([r["stats"] for r in recs])
    h = fx.h
    fx.eng.set_option("deterministic", 1)
    try:
        kw = dict(max_iter=30, lam0=lam0, loss=fx.loss) if not fx.generated else dict(max_iter=30, lam0=lam0)
        res = lm_solve(h, x0.copy(), **kw)
    finally:
        fx.eng.set_option("deterministic", 0)
    got = np.array(res.trials)
    assert got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape)
    acc = [r for r in recs if r["stats"][0] > 0]
    hist = [0.5 * recs[0]["stats"][6]] + [0.5 * r["stats"][5] for r in acc]
    assert res.history == hist and res.nit == len(acc) and res.nfev == 1 + len(recs)
    fin = recs[-1]["ps_tri"] if recs[-1]["stats"][0] > 0 else recs[-1]["ps_cur"]
    assert np.array_equal(res.x, fin[fx.mask])
    from pycamset_amd.device_solver import STOP_MESSAGES
    assert res.message == STOP_MESSAGES[int(recs[-1]["stats"][8])]
    if fx.generated:
        return
    # the host-steered loop (one rank, a host-staged identity collective): the same decisions

    def identity(v):
        return v

    host = lm_solve(h, x0.copy(), max_iter=30, lam0=lam0, loss=fx.loss, reduce_fn=identity)
    hs = np.array(host.trials)
    assert hs.shape == want.shape, (hs.shape, want.shape)
    assert np.array_equal(hs[:, 0], want[:, 0]) and np.array_equal(hs[:, 8], want[:, 8])
    for k in range(len(recs)):
        if hs[k, 11] != want[k, 11]:       # only where the host's recomputed gain ratio lies next to a threshold
            rc = recs[k]
            rho = 0.5 * (rc["stats"][6] - rc["stats"][5]) / R.predicted_reduction(rc["lam"], rc["dvec"], rc["gm"], rc["delta"])
            assert R.near_a_threshold(rho, rc["ctrl"]), (k, hs[k], want[k])
    assert host.message == res.message and host.nit == res.nit and host.nfev == res.nfev


@pytest.mark.parametrize("name", ["ring8-template-far20", "ring8-self-gauge"])
def test_fused_and_separate_trial_launches_give_the_same_bits(name):
    """DESIGN section 4 and INTEGRATION.md: ``set_option("fused_trial", 0)`` runs the small kernels of a trial as separate launches and
    returns the same bits.  In deterministic mode (the default mode's atomics reorder the last bits from run to run) every read-back of
    every trial and the solution are compared exactly: no tolerance."""
    from pycamset_amd.device_solver import lm_solve
    build, _, _, lam0, _, _ = FIXTURES[name]
    _, h, x0 = build()
    eng = h.op_fun._engine_for(h._flat_detections())
    eng.set_option("deterministic", 1)
    res = {}
    try:
        for fused in (1, 0):
            eng.set_option("fused_trial", fused)
            res[fused] = lm_solve(h, x0.copy(), max_iter=30, lam0=lam0, linear_solver="cholesky")
    finally:
        eng.set_option("fused_trial", 1)
        eng.set_option("deterministic", 0)

    def bits(v):
        return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)

    assert len(res[1].trials) == len(res[0].trials) > 0
    for k, (fused, separate) in enumerate(zip(res[1].trials, res[0].trials)):
        assert np.array_equal(bits(fused), bits(separate)), (name, k, fused, separate)
    assert np.array_equal(bits(res[1].x), bits(res[0].x)), name


# =================================================================================== D: every stop code on a real problem

def test_every_stop_code_on_a_real_problem():
    rig, h, x0 = _ring8("template")
    eng = h.op_fun._engine_for(h._flat_detections())
    eng.set_option("deterministic", 1)          # the same max |g| on every build: gtol can be set to it exactly
    try:
        _stop_codes(h, x0)
    finally:
        eng.set_option("deterministic", 0)


def _stop_codes(h, x0):
    from pycamset_amd.device_solver import STOP_MESSAGES, lm_solve
    ref = lm_solve(h, x0.copy(), max_iter=30)
    t0 = np.array(ref.trials[0])
    # gtol above the start's max |g|: code 1 at the first trial, nothing moves
    res = lm_solve(h, x0.copy(), max_iter=30, gtol=t0[1] * 1.5)
    tr = np.array(res.trials)
    assert tr.shape[0] == 1 and tr[0, 8] == 1 and tr[0, 0] == 0 and tr[0, 11] == tr[0, 7]
    assert np.array_equal(res.x, x0) and res.nit == 0 and res.nfev == 2 and res.status == 1
    # gtol exactly at the start's max |g|: `<=` fires
    res = lm_solve(h, x0.copy(), max_iter=30, gtol=t0[1])
    assert np.array(res.trials)[0, 8] == 1
    # ftol, and xtol with ftol = 0: the reference agrees with the trial that stopped
    res = lm_solve(h, x0.copy(), max_iter=60, ftol=1e-6, xtol=0.0)
    last = np.array(res.trials[-1])
    assert last[8] == 3 and last[2] <= 1e-6 and res.message == STOP_MESSAGES[3]
    assert all(t[2] > 1e-6 for t in res.trials[:-1] if t[0] > 0)
    res = lm_solve(h, x0.copy(), max_iter=60, ftol=0.0, xtol=1e-7)
    last = np.array(res.trials[-1])
    assert last[8] == 4 and last[3] <= 1e-7 * (1e-7 + last[4]) and res.message == STOP_MESSAGES[4]
    assert all(t[3] > 1e-7 * (1e-7 + t[4]) for t in res.trials[:-1] if t[0] > 0)
    # the iteration limit on exactly that many acceptances
    for n in (1, 2, 3):
        res = lm_solve(h, x0.copy(), max_iter=n, ftol=0.0, xtol=0.0, gtol=0.0)
        tr = np.array(res.trials)
        assert int(np.sum(tr[:, 0] > 0)) == n and tr[-1, 8] == 5 and tr[-1, 0] == 1 and res.nit == n
        assert res.message == STOP_MESSAGES[5]
    res = lm_solve(h, x0.copy(), max_iter=0)
    assert res.trials == [] and res.nfev == 1 and res.nit == 0 and np.array_equal(res.x, x0)
