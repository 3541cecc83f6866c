"""Box bounds in the device LM solve (include/pcs_hip.h pcs_set_bounds, csrc/ba_bounds.hpp, lm_solve(bounds=)): the two kernels alone
against NumPy bit for bit, the device-steered loop trial by trial against tests/bounds_reference.py, solves through every loop against
scipy's bounded least_squares on the oracle closures, the composition with loss, sigma and prior, no effect where none is due, a start
on a bound, the deterministic mode and the refusals.  ring-4 and the four-block generated chain of tests/test_gpu_prior.py."""
import functools

import numpy as np
import pytest
from scipy.optimize import least_squares

from pycamset_amd import _capi
from tests import bounds_reference as BR
from tests import prior_reference as PR
from tests import weights_reference as W

pytestmark = pytest.mark.gpu


def _in_stream_sum(t):
    t.mul_(1.0)
    return t


_in_stream_sum.on_device = True


# ---- 1. the two kernels alone ----------------------------------------------------------------------------------------------------
def _free_engine():
    """A free-point engine of 4 cameras and 343 points: 60 + 1029 = 1089 parameters — more than one stride of the 1 024 threads, not a
    multiple of 64, the points a trailing group of 3.  The kernels read no detections."""
    from pycamset_amd.engine import Engine
    e = Engine("free", 4, 0, 343)
    assert e.n_params == 1089
    return e


def _run_pieces(e, x, g, d, lo, hi, fixed, raw=False, sel=None):
    """(fixed_eff, alpha, x_new, delta) of the two piece entry points on the engine's stream.  ``sel`` = 0 / 1: the two-state entries
    with a selector word, as pcs_lm_trial_build runs the kernels — the current string and gradient in state ``sel``, the other state
    holding a decoy string and gradient that must not be read, and the trial string expected in the OTHER state's string."""
    import ctypes

    import torch
    lay = e.normal_layout()
    n = lay["n_params"]
    if raw:   # all-infinite bounds cannot be set through Engine.set_bounds (it clears them): the C entry takes them as they are
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
        _capi.check(_capi.lib().pcs_set_bounds(e._h, dp(lo), dp(hi), n))
    else:
        e.set_bounds(lo, hi)
    pk = np.zeros(lay["packed_len"])
    g0 = lay["packed_len"] - 1 - n
    pk[g0: g0 + n] = g
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d_x, d_pk, d_fixed, d_delta, d_out = up(x), up(pk), up(fixed.astype(np.uint8)), up(d.copy()), up(x + d)
    d_eff = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_alpha = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    if sel is not None:
        decoy = np.zeros(lay["packed_len"])
        decoy[g0: g0 + n] = -g                                           # every gradient the other way round: a swapped index shows
        d_decoy = up(decoy)
        pks = [d_pk, d_decoy] if sel == 0 else [d_decoy, d_pk]
        pss = [d_x, d_out] if sel == 0 else [d_out, d_x]                 # the trial string lives in the state that is not current
        d_sel = torch.full((1,), sel, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.bounds_active_sel_device(pss[0].data_ptr(), pss[1].data_ptr(), pks[0].data_ptr(), pks[1].data_ptr(), d_fixed.data_ptr(), d_eff.data_ptr(), d_sel.data_ptr())
        e.bounds_truncate_sel_device(pss[0].data_ptr(), pss[1].data_ptr(), d_delta.data_ptr(), d_alpha.data_ptr(), d_sel.data_ptr())
        e.synchronize()
        assert np.array_equal(d_x.cpu().numpy(), x)                      # the current string is read only
        return d_eff.cpu().numpy(), float(d_alpha.cpu().numpy()[0]), d_out.cpu().numpy(), d_delta.cpu().numpy()
    torch.cuda.synchronize()
    e.bounds_active_device(d_x.data_ptr(), d_pk.data_ptr(), d_fixed.data_ptr(), d_eff.data_ptr())
    e.bounds_truncate_device(d_x.data_ptr(), d_delta.data_ptr(), d_out.data_ptr(), d_alpha.data_ptr())
    e.synchronize()
    return d_eff.cpu().numpy(), float(d_alpha.cpu().numpy()[0]), d_out.cpu().numpy(), d_delta.cpu().numpy()


def _synthetic(n, seed, tie):
    """x, g, d, lo, hi, fixed with every case of the issue's list: bounds on the first and the last parameter (a trailing-group entry)
    and on many in between, entries exactly on a bound with the gradient pointing out and in, lo == hi, an entry both user-fixed and
    bounded, d = 0 on a bound, an entry on a bound whose step points out (pinned) — and, with ``tie``, two entries whose fractions are
    the same bits, the higher index first in its stride."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    g = rng.standard_normal(n)
    d = 0.1 * rng.standard_normal(n)
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    pick = rng.choice(np.arange(1, n - 1), 300, replace=False)
    lo[pick[:200]] = x[pick[:200]] - rng.uniform(0.5, 2.0, 200)
    hi[pick[100:]] = x[pick[100:]] + rng.uniform(0.5, 2.0, 200)
    lo[0], hi[0] = x[0] - 1.0, x[0] + 1.0
    lo[n - 1], hi[n - 1] = x[n - 1] - 1.0, x[n - 1] + 1.0
    fixed = np.zeros(n, bool)
    fixed[rng.choice(n, 40, replace=False)] = True
    a, b, c, e_, f, gq, hq = pick[10], pick[120], pick[250], pick[20], pick[130], pick[30], pick[140]
    x[a] = lo[a]; g[a] = 1.0; d[a] = 0.0; fixed[a] = False          # on the lower bound, gradient out: active; d = 0 on a bound
    x[b] = hi[b]; g[b] = -1.0; fixed[b] = False                      # on the upper bound, gradient out: active
    x[c] = hi[c]; g[c] = 1.0; d[c] = -0.05; fixed[c] = False         # on the upper bound, gradient in, step in: free
    x[e_] = lo[e_]; g[e_] = -1.0; d[e_] = -0.05; fixed[e_] = False   # on the lower bound, gradient in, step OUT: pinned
    hi[f] = lo[f] = x[f]; fixed[f] = False                           # lo == hi: acts as fixed
    fixed[gq] = True                                                 # user-fixed and bounded
    fixed[hq] = False
    d[fixed] = 0.0                                                   # what the Schur step writes for fixed entries
    eff, _ = BR.active_set(x, g, lo, hi, fixed)
    d[eff] = 0.0
    if tie:
        # Two entries whose fractions are the SAME BITS but whose x + alpha d both fall short of the bound by rounding: the winner is
        # forced onto its bound, the loser keeps x + alpha d < hi — so x_new tells which index the device took.  70 and 1030 = thread 70's
        # first stride and thread 6's second: a tree that prefers the lower THREAD, or a strided loop with <=, picks 1030.
        pairs = _tie_pairs()
        for k, (xk, dk, hk) in zip((70, 1030), pairs):
            fixed[k] = False
            x[k], d[k], lo[k], hi[k], g[k] = xk, dk, -np.inf, hk, 0.0
        d[(BR.fractions(x, d, lo, hi) <= BR.fractions(x, d, lo, hi)[70]) & (np.arange(n) != 70) & (np.arange(n) != 1030)] *= 1e-3
    else:
        k = int(hq)
        x[k], d[k], lo[k], hi[k], g[k] = 0.0, 1.0, -1.0, 0.25, 0.0   # the one entry that cuts: alpha = 0.25 exactly
        d[(BR.fractions(x, d, lo, hi) < 1.0) & (np.arange(n) != k)] *= 0.01
    return x, g, d, lo, hi, fixed


@functools.lru_cache(maxsize=None)
def _tie_pairs():
    """Two (x, d, hi) with d > 0 and bit-identical (hi - x) / d = f < 1 for which x + f d < hi in double arithmetic."""
    rng = np.random.default_rng(17)
    f0, found = None, []
    for _ in range(200000):
        xk, hk = rng.uniform(-1.0, 1.0), 0.0
        hk = xk + rng.uniform(0.05, 0.5)
        if f0 is None:
            dk = (hk - xk) / 0.3
        else:
            dk = (hk - xk) / f0
        fk = (hk - xk) / dk
        if not (fk < 1.0 and xk + fk * dk < hk):
            continue
        if f0 is None:
            f0, found = fk, [(xk, dk, hk)]
        elif fk == f0:
            found.append((xk, dk, hk))
            return found
    raise AssertionError("no tie found")


@pytest.mark.parametrize("sel", [None, 0, 1])
@pytest.mark.parametrize("case", ["cut", "tie", "whole"])
def test_the_two_kernels_alone_match_numpy_bit_for_bit(case, sel):
    e = _free_engine()
    n = e.n_params
    x, g, d, lo, hi, fixed = _synthetic(n, 3, tie=case == "tie")
    if case == "whole":   # no entry cuts the step: alpha = 1
        d = np.where(BR.fractions(x, d, lo, hi) < 1.0, 0.0, d)
    eff, alpha, x_new, delta = _run_pieces(e, x, g, d, lo, hi, fixed, sel=sel)
    want_eff, n_active = BR.active_set(x, g, lo, hi, fixed)
    assert np.array_equal(eff, want_eff.astype(np.uint8)) and n_active >= 3
    want_alpha, hit, want_x, want_delta = BR.truncate(x, d, lo, hi)
    assert alpha == want_alpha
    assert np.array_equal(x_new, want_x) and np.array_equal(delta, want_delta)
    assert np.all(x_new[np.isfinite(lo)] >= lo[np.isfinite(lo)]) and np.all(x_new[np.isfinite(hi)] <= hi[np.isfinite(hi)])
    if case == "whole":
        assert alpha == 1.0 and hit == -1
        untouched = ~BR.pinned(x, d, lo, hi) & (np.minimum(np.maximum(x + d, lo), hi) == x + d)
        assert np.array_equal(delta[untouched], d[untouched]) and np.array_equal(x_new[untouched], (x + d)[untouched])
    else:
        assert alpha < 1.0 and x_new[hit] == (hi[hit] if d[hit] > 0 else lo[hit])
    if case == "tie":
        f = BR.fractions(x, d, lo, hi)
        assert f[70] == f[1030] == alpha and hit == 70
        # the device's index, read off x_new: the winner exactly on its bound, the loser one rounding short of its own
        assert x_new[70] == hi[70] and x_new[1030] == x[1030] + alpha * d[1030] < hi[1030]
        assert x[70] + alpha * d[70] < hi[70]                       # had 1030 won, x_new[70] would be this, not hi[70]
    e.set_bounds()
    assert e.bounds() is None


def test_all_infinite_bounds_leave_the_step_untouched():
    e = _free_engine()
    n = e.n_params
    rng = np.random.default_rng(8)
    x, g, d = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    fixed = rng.random(n) < 0.1
    d[fixed] = 0.0
    eff, alpha, x_new, delta = _run_pieces(e, x, g, d, np.full(n, -np.inf), np.full(n, np.inf), fixed, raw=True)
    assert alpha == 1.0 and np.array_equal(eff, fixed.astype(np.uint8))
    assert np.array_equal(delta, d) and np.array_equal(x_new, x + d)
    e.set_bounds()


def test_setter_checks_its_arguments():
    e = _free_engine()
    n = e.n_params
    with pytest.raises(ValueError, match="index 5"):
        e.set_bounds(np.r_[np.zeros(5), 2.0, np.zeros(n - 6)], 1.0)
    with pytest.raises(ValueError, match="NaN at index 2"):
        e.set_bounds(np.r_[0.0, 0.0, np.nan, np.zeros(n - 3)], 1.0)
    with pytest.raises(ValueError, match="values for"):
        e.set_bounds(np.zeros(n - 1), 1.0)
    lib = _capi.lib()
    import ctypes
    bad = np.full(n, np.nan)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    assert lib.pcs_set_bounds(e._h, dp(bad), dp(bad), n) == _capi.PCS_ERR_ARG
    assert lib.pcs_set_bounds(e._h, dp(np.ones(n)), dp(np.zeros(n)), n) == _capi.PCS_ERR_ARG
    assert lib.pcs_set_bounds(e._h, dp(np.zeros(n)), dp(np.ones(n)), n - 1) == _capi.PCS_ERR_ARG
    assert e.bounds() is None
    e.set_bounds(0.0, np.r_[0.0, np.ones(n - 1)])                      # lo == hi is allowed
    lo, hi = e.bounds()
    assert lo[0] == hi[0] == 0.0 and hi[1] == 1.0
    e.set_bounds(-np.inf, np.inf)                                      # all infinite: cleared
    assert e.bounds() is None


# ---- 2. trial by trial -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(chain):
    p = BR.problem(chain)
    return p, BR.solve(p.fun, p.jac, p.x0, p.lo, p.hi, max_iter=BR.TRIAL_ITERS, lam0=p.lam0)


@pytest.mark.parametrize("chain", BR.CHAINS)
def test_device_loop_follows_the_reference_trial_by_trial(chain):
    """The device-steered loop against the NumPy loop on the oracle closures: the accepted / rejected sequence, the active count and
    alpha per trial, lambda and both costs.  Costs to 1e-10 and lambda to 1e-13 as tests/test_gpu_lm_trials.py takes them; alpha is a
    quotient of a distance and a step component of the damped solve: 1e-6 relative, the agreement two backward-stable solves of these
    systems give for a component (their conditioning is at most ~1e9 here)."""
    from pycamset_amd.device_solver import lm_solve
    p, ref = _reference(chain)
    res = lm_solve(p.h, p.x0.copy(), max_iter=BR.TRIAL_ITERS, bounds=(p.lo, p.hi), lam0=p.lam0)
    assert len(res.trials) == len(res.bound_trials)
    m = min(len(res.trials), len(ref.trials))
    assert m >= 8
    near = cut = held = 0
    for k in range(m):
        st, (alpha, n_active), want = res.trials[k], res.bound_trials[k], ref.trials[k]
        print(k, st[0], alpha, n_active, st[7], st[6], st[5], "| want", want["accepted"], want["alpha"], want["n_active"], want["lam"], want["c_old"], want["c_new"])
        assert bool(st[0] > 0) == want["accepted"], k
        assert n_active == want["n_active"], k
        assert abs(alpha - want["alpha"]) <= 1e-6 * want["alpha"], (k, alpha, want["alpha"])
        assert abs(st[7] - want["lam"]) <= 1e-13 * want["lam"], (k, st[7], want["lam"])
        assert abs(st[6] - want["c_old"]) <= 1e-10 * want["c_old"] and abs(st[5] - want["c_new"]) <= 1e-10 * want["c_new"], k
        near += bool(want["near"])
        cut += alpha < 1.0
        held += n_active > 0
    # every trial of the shorter list was compared; none sat on a gain-ratio threshold (where either side may be taken); cut trials and
    # trials with a non-empty active set were among them
    assert near == 0 and cut >= 1 and held >= 1, (near, cut, held)
    assert res.n_truncated == sum(1 for a, _ in res.bound_trials if a < 1.0) and res.n_truncated >= 1


# ---- 3. solves through every loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scipy(chain):
    p = BR.problem(chain)
    return least_squares(p.fun, p.x0_interior, jac=p.jac, bounds=(p.lo, p.hi), x_scale="jac", method="trf", max_nfev=BR.SCIPY_NFEV)


def _check_against_scipy(res, ref, p, what):
    print(what, res.cost, ref.cost, res.status, res.nfev, res.n_truncated, np.flatnonzero(res.active_mask), np.flatnonzero(ref.active_mask))
    assert res.cost <= ref.cost * (1 + 1e-3), (what, res.cost, ref.cost)
    assert np.array_equal(res.active_mask, ref.active_mask), (what, np.flatnonzero(res.active_mask != ref.active_mask))
    assert np.all(res.x >= p.lo) and np.all(res.x <= p.hi), what


@pytest.mark.parametrize("chain", BR.CHAINS)
def test_bounded_solves_match_scipy_through_every_loop(chain):
    from pycamset_amd.device_solver import lm_solve
    p, ref = BR.problem(chain), _scipy(chain)
    assert ref.status > 0 and np.array_equal(ref.active_mask, p.designed_mask)
    res = lm_solve(p.h, p.x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(p.lo, p.hi))
    _check_against_scipy(res, ref, p, "device")
    host = lm_solve(p.h, p.x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(p.lo, p.hi), reduce_fn=lambda a: a)
    _check_against_scipy(host, ref, p, "host")
    assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (host.cost, res.cost)
    dev = lm_solve(p.h, p.x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(p.lo, p.hi), reduce_fn=_in_stream_sum)
    _check_against_scipy(dev, ref, p, "in-stream")
    assert abs(dev.cost - res.cost) <= 1e-9 * res.cost, (dev.cost, res.cost)
    assert p.h.op_fun._engine_for(p.h._flat_detections()).bounds() is None


def _genchain_problem():
    from tests.test_gpu_prior import _four_block_problem
    rig, prob = _four_block_problem()
    lo, hi, designed = BR.genchain_box(rig, prob)
    return rig, prob, lo, hi, designed


def test_generated_chain_blocked_and_dense_with_bounds_and_with_a_prior():
    from pycamset_amd import handlers
    from pycamset_amd.device_solver import lm_solve
    rig, prob, lo, hi, designed = _genchain_problem()
    x0 = np.clip(prob.x0, lo, hi)
    fun, jac = prob.make_loss_fun(), prob.make_loss_jac()
    ref = least_squares(fun, BR.interior(x0, lo, hi), jac=jac, bounds=(lo, hi), x_scale="jac", method="trf", max_nfev=BR.SCIPY_NFEV)
    assert ref.status > 0 and np.array_equal(ref.active_mask, designed)
    sig = [np.r_[np.full(4, np.inf), np.full(5, 0.02)], None, None, np.r_[np.full(3, 0.01), np.full(3, 2.0)]]
    mean, sigma = handlers.slab_prior(prob, sig)
    wf = PR.weights_of(sigma)
    fa, ja, _ = PR.augmented_closures(fun, jac, mean, wf)
    refp = least_squares(fa, BR.interior(x0, lo, hi), jac=ja, bounds=(lo, hi), x_scale="jac", method="trf", max_nfev=BR.SCIPY_NFEV)
    eng = prob.op_fun._engine_for(prob.det)
    p = type("P", (), dict(lo=lo, hi=hi))
    for dense in (0, 1):
        eng.set_option("dense_normal", dense)
        res = lm_solve(prob, x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(lo, hi))
        _check_against_scipy(res, ref, p, f"genchain dense={dense}")
        host = lm_solve(prob, x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(lo, hi), reduce_fn=lambda a: a)
        assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (dense, host.cost, res.cost)
        resp = lm_solve(prob, x0.copy(), max_iter=BR.SOLVE_ITERS, bounds=(lo, hi), prior_mean=mean, prior_sigma=sigma)
        assert refp.status > 0
        _check_against_scipy(resp, refp, p, f"genchain + prior dense={dense}")
    eng.set_option("dense_normal", 0)
    assert eng.bounds() is None and eng.prior() is None


# ---- 4. composition --------------------------------------------------------------------------------------------------------------
def test_huber_sigma_prior_and_bounds_together_match_scipy():
    """sigma + prior + bounds with the linear loss from the common start, then huber on top of it from where the linear solve ended (the
    robust solve of a calibration starts there): both against scipy on the whitened, augmented closures with the same bounds.  The prior
    holds the distortion terms (which ring-4 alone determines too poorly for scipy's trf to converge) and the pose translations."""
    from pycamset_amd import handlers
    from pycamset_amd.device_solver import lm_solve
    p = BR.problem("template")
    det = p.h._flat_detections()
    n_rows = 2 * det.shape[0]
    per_cam = np.array([0.5, 1.0, 2.0, 4.0])
    wd = 1.0 / per_cam[det[:, 0].astype(int)]
    groups = {"intr": np.r_[np.full(4, np.inf), np.full(5, 0.02)], "pose": np.r_[np.full(3, np.inf), np.full(3, 5.0)]}
    mean, sigma = handlers.slab_prior(p.h, groups, {"intr": p.rig.intr, "pose": p.rig.poses})
    w = PR.weights_of(sigma)
    f0, j0 = W.whitened_closures(p.fun, p.jac, wd)
    fa, ja, _ = PR.augmented_closures(f0, j0, mean, w)
    kw = dict(bounds=(p.lo, p.hi), sigma=per_cam, prior_mean=mean, prior_sigma=sigma, max_iter=BR.SOLVE_ITERS)
    sk = dict(jac=ja, bounds=(p.lo, p.hi), x_scale="jac", method="trf", max_nfev=BR.SCIPY_NFEV)
    ref = least_squares(fa, p.x0_interior, **sk)
    assert ref.status > 0 and np.array_equal(ref.active_mask, p.designed_mask)
    res = lm_solve(p.h, p.x0.copy(), **kw)
    _check_against_scipy(res, ref, p, "sigma + prior + bounds")
    assert abs(0.5 * np.sum(fa(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    # huber: the box keeps the translation bound only.  With a second bound (fx, or another camera's t_z) scipy's trf under a robust loss
    # ends by ftol 3e-7 .. 7e-4 short of it (257 evaluations; tighter tolerances bring it closer, 2.8e-7 after 600, never onto it) and its
    # active_mask, a closeness test at xtol, then leaves out an entry the device holds exactly on the bound at a lower cost
    # (87.46239 against 87.46421): such a box makes the comparison a matter of scipy's stopping point and is not used.
    # What the device does with the FULL box under huber is checked on its own: both designed entries exactly on their bounds, at a cost
    # no higher than scipy's on the same box.
    full = least_squares(fa, BR.interior(ref.x, p.lo, p.hi, 1e-6), loss=PR.split_loss("huber", n_rows), **sk)
    both = lm_solve(p.h, np.clip(ref.x, p.lo, p.hi), loss="huber", f_scale=1.0, **kw)
    k = np.flatnonzero(p.designed_mask)
    print("huber, full box", both.cost, full.cost, both.x[k] - p.hi[k], full.x[k] - p.hi[k])
    assert np.array_equal(both.active_mask, p.designed_mask) and np.array_equal(both.x[k], p.hi[k]) and both.cost <= full.cost
    assert np.all(both.x >= p.lo) and np.all(both.x <= p.hi)
    hi1 = p.hi.copy()
    hi1[9 * BR.FX_CAM] = np.inf
    one = type("P", (), dict(lo=p.lo, hi=hi1))
    sk["bounds"], kw["bounds"] = (p.lo, hi1), (p.lo, hi1)
    start = least_squares(fa, p.x0_interior, **sk)
    refh = least_squares(fa, BR.interior(start.x, p.lo, hi1, 1e-6), loss=PR.split_loss("huber", n_rows), **sk)
    designed = np.where(np.isfinite(hi1) | np.isfinite(p.lo), p.designed_mask, 0)
    assert refh.status > 0 and np.array_equal(refh.active_mask, designed) and np.count_nonzero(designed) == 1
    resh = lm_solve(p.h, np.clip(start.x, p.lo, hi1), loss="huber", f_scale=1.0, **kw)
    _check_against_scipy(resh, refh, one, "huber + sigma + prior + bounds")


# ---- 5. no effect where none is due ----------------------------------------------------------------------------------------------
def test_no_bounds_and_infinite_bounds_are_the_plain_solve_bit_for_bit():
    from pycamset_amd.device_solver import lm_solve
    p = BR.problem("template")
    eng = p.h.op_fun._engine_for(p.h._flat_detections())
    eng.set_option("deterministic", 1)
    try:
        plain = lm_solve(p.h, p.x0.copy(), max_iter=8)
        for b in (None, (-np.inf, np.inf), (np.full(p.x0.shape, -np.inf), np.full(p.x0.shape, np.inf))):
            r = lm_solve(p.h, p.x0.copy(), max_iter=8, bounds=b)
            assert np.array_equal(r.x, plain.x) and r.history == plain.history and r.nfev == plain.nfev and r.active_mask is None and r.n_truncated == 0
        wide = lm_solve(p.h, p.x0.copy(), max_iter=8, bounds=(p.x0 - 1e6, p.x0 + 1e6))       # finite, never binding: the non-fused path
        assert [t[0] for t in wide.trials] == [t[0] for t in plain.trials]
        assert abs(wide.cost - plain.cost) <= 1e-9 * plain.cost and wide.n_truncated == 0 and not wide.active_mask.any()
        bounded = lm_solve(p.h, p.x0.copy(), max_iter=8, bounds=(p.lo, p.hi))
        assert bounded.n_truncated >= 1 and eng.bounds() is None
        again = lm_solve(p.h, p.x0.copy(), max_iter=8)
        assert np.array_equal(again.x, plain.x) and again.history == plain.history and again.nfev == plain.nfev
    finally:
        eng.set_option("deterministic", 0)


# ---- 6. start on a bound ---------------------------------------------------------------------------------------------------------
def test_start_on_a_bound_with_the_gradient_pointing_out_and_in():
    from pycamset_amd.device_solver import lm_solve
    p = BR.problem("template")
    plain = lm_solve(p.h, p.x0.copy(), max_iter=0)                 # the gradient at the start
    k = 0                                                          # fx of camera 0
    n = p.x0.shape[0]
    for out in (True, False):
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        # gradient > 0: the cost falls towards smaller x — a LOWER bound at x0 holds it (gradient out), an UPPER bound at x0 leaves it free
        if (plain.grad[k] > 0) == out:
            lo[k] = p.x0[k]
        else:
            hi[k] = p.x0[k]
        res = lm_solve(p.h, p.x0.copy(), max_iter=1, bounds=(lo, hi))
        alpha, n_active = res.bound_trials[0]
        print(out, plain.grad[k], alpha, n_active, res.x[k] - p.x0[k])
        assert n_active == (1 if out else 0)
        if out:
            assert alpha == 1.0 and res.x[k] == p.x0[k]


# ---- 7. deterministic mode -------------------------------------------------------------------------------------------------------
def test_two_bounded_solves_in_deterministic_mode_give_the_same_bits():
    from pycamset_amd.device_solver import lm_solve
    p = BR.problem("self")
    eng = p.h.op_fun._engine_for(p.h._flat_detections())
    eng.set_option("deterministic", 1)
    try:
        a = lm_solve(p.h, p.x0.copy(), max_iter=10, bounds=(p.lo, p.hi))
        b = lm_solve(p.h, p.x0.copy(), max_iter=10, bounds=(p.lo, p.hi))
    finally:
        eng.set_option("deterministic", 0)
    assert np.array_equal(a.x, b.x) and a.history == b.history and a.bound_trials == b.bound_trials and a.n_truncated == b.n_truncated >= 1
    assert all(np.array_equal(s, t) for s, t in zip(a.trials, b.trials))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pycamset_amd import device_solver as ds
    from pycamset_amd.device_solver import lm_solve
    p = BR.problem("template")
    k = int(np.flatnonzero(np.isfinite(p.hi))[0])
    bad = p.x0.copy()
    bad[k] = p.hi[k] + 1.0
    with pytest.raises(ValueError, match=rf"`x0` is infeasible: x0\[{k}\]"):
        lm_solve(p.h, bad, bounds=(p.lo, p.hi))
    with pytest.raises(NotImplementedError, match="bounds"):
        lm_solve(p.h, p.x0.copy(), bounds=(p.lo, p.hi), linear_solver="pcg")
    with pytest.raises(NotImplementedError, match="bounds"):
        lm_solve(p.h, p.x0.copy(), bounds=(p.lo, p.hi), operator=object())
    saved = ds.LEAD_LIMIT
    ds.LEAD_LIMIT = 8                                             # "beyond blocked_fits" without a large system
    try:
        with pytest.raises(NotImplementedError, match="bounds"):
            lm_solve(p.h, p.x0.copy(), bounds=(p.lo, p.hi))
    finally:
        ds.LEAD_LIMIT = saved
