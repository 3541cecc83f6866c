"""Gaussian parameter priors on the device (include/pcs_hip.h pcs_set_prior, csrc/ba_prior.hpp, lm_solve(prior_mean=, prior_sigma=),
parameter_covariance(prior_mean=, prior_sigma=)): what the add writes and what it leaves alone, clearing, the combination with loss and
noise weights, generated chains, the solves through every loop against scipy on the augmented closures of tests/prior_reference.py, the
two limits of sigma, gauge-free self-calibration and an entity without detections.  ring-4 unless stated."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.sparse import csr_array, vstack

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests import helpers as H
from tests import prior_reference as PR
from tests import weights_reference as W
from tests.test_host_logic import DuckCamset, DuckTarget

pytestmark = pytest.mark.gpu
CHAINS = ["template", "self", "free"]
PRIOR_PER_WG = 1024          # csrc/ba_prior.hpp: entries one workgroup of prior_add_kernel takes (256 threads x 4)


def _engine(chain, rig, det, tm):
    from pycamset_amd.engine import Engine
    e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys)
    e.set_detections_table(det)
    if tm is not None:
        e.set_template(tm)
    return e


def _packed(e, ps, add_prior, packed_in=None):
    """The packed state of normal_blocks_device (or a copy of ``packed_in``), with prior_add_device behind it when asked; on the host."""
    import torch
    lay = e.normal_layout()
    d_ps = torch.from_numpy(np.ascontiguousarray(ps)).cuda()
    if packed_in is None:
        pk = torch.full((lay["packed_len"],), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.normal_blocks_device(d_ps.data_ptr(), pk.data_ptr())
    else:
        pk = torch.from_numpy(packed_in.copy()).cuda()
        torch.cuda.synchronize()
    if add_prior:
        e.prior_add_device(d_ps.data_ptr(), pk.data_ptr())
    e.synchronize()
    return pk.cpu().numpy()


def _places(lay, idx):
    """Where parameter i's diagonal entry and gradient entry sit in the packed state, and the cost word."""
    nl, nt, tb, n = lay["n_lead"], lay["n_trail"], lay["tb"], lay["n_params"]
    idx = np.asarray(idx, dtype=np.int64)
    t = idx - nl
    diag = np.where(idx < nl, idx * nl + idx, nl * nl + nl * nt + (t // tb) * tb * tb + (t % tb) * tb + (t % tb))
    g0 = nl * nl + nl * nt + nt * tb
    return diag, g0 + idx, g0 + n


def _dense(pk, lay):
    """(upper triangle of H, g, cost) from a packed state."""
    nl, nt, tb, n = lay["n_lead"], lay["n_trail"], lay["tb"], lay["n_params"]
    Hu = np.zeros((n, n))
    Hu[:nl, :nl] = pk[: nl * nl].reshape(nl, nl)
    Hu[:nl, nl:] = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
    C = pk[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
    for e in range(nt // tb):
        Hu[nl + e * tb: nl + (e + 1) * tb, nl + e * tb: nl + (e + 1) * tb] = C[e]
    return np.triu(Hu), pk[-(n + 1):-1].copy(), float(pk[-1])


def _check_add(raw, got, lay, ps, idx, mean, w):
    """The add is the prior and nothing else: every entry outside the prior's places keeps its bits; the diagonals, the gradient entries
    and the cost word are the exactly rounded sums to 2 ulp (1e-14 relative for the cost word, a sum of len(idx) terms).  The gradient
    entry is a sum of two terms of either sign: its ulp is that of the larger of the terms and the result."""
    diag, gi, ci = _places(lay, idx)
    touched = np.zeros(raw.shape[0], bool)
    touched[diag] = touched[gi] = touched[ci] = True
    assert np.array_equal(raw[~touched], got[~touched])
    L = np.longdouble
    d = L(ps[idx]) - L(mean)
    want_diag = L(raw[diag]) + L(w) * L(w)
    assert np.all(np.abs(L(got[diag]) - want_diag) <= 2 * np.spacing(got[diag])), float(np.max(np.abs(L(got[diag]) - want_diag) / np.spacing(got[diag])))
    term = L(w) * L(w) * d
    want_g = L(raw[gi]) + term
    ulp = np.spacing(np.maximum(np.maximum(np.abs(raw[gi]), np.abs(term.astype(np.float64))), np.abs(got[gi])))
    assert np.all(np.abs(L(got[gi]) - want_g) <= 2 * ulp), float(np.max(np.abs(L(got[gi]) - want_g) / ulp))
    want_c = L(raw[ci]) + np.sum((L(w) * d) ** 2)
    assert abs(L(got[ci]) - want_c) <= 1e-14 * float(want_c), (got[ci], float(want_c))


def _prior_entries(chain, rig, n_params, rng, lone):
    """Index 0 and the last index, fx of every camera, and the trailing columns: one pose's t_z for the template chain, every point
    coordinate for the self and free chains — and the entity `lone` that has no detections."""
    C, I, K = rig.n_cams, rig.n_imgs, rig.n_keys
    idx = {0, n_params - 1} | {9 * c for c in range(C)}
    if chain == "template":
        idx |= {15 * C + 6 * 2 + 5, 15 * C + 6 * lone + 5}
    else:
        if chain == "self":
            idx |= {15 * C + 6 * lone + 5}
        idx |= set(range(n_params - 3 * K, n_params))
    idx = np.array(sorted(idx), dtype=np.int64)
    w = np.exp(rng.uniform(np.log(0.1), np.log(50.0), idx.shape[0]))
    return idx, w


# ---- 1. the add is the prior and nothing else ------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_the_add_is_the_prior_and_nothing_else(chain):
    rig, det, ps, tm = W.chain_inputs(chain)
    lone = 3
    det = det[det[:, 2] != lone] if chain == "free" else det[det[:, 1] != lone]     # a key (free chain) / an image without detections
    e = _engine(chain, rig, det, tm)
    e.set_option("deterministic", 1)
    lay = e.normal_layout()
    n = lay["n_params"]
    rng = np.random.default_rng(8)
    idx, w = _prior_entries(chain, rig, n, rng, lone)
    assert idx.shape[0] <= PRIOR_PER_WG                                               # the one-workgroup form
    mean_e = ps[idx] + rng.standard_normal(idx.shape[0]) / w
    mean, inv_sigma = np.zeros(n), np.zeros(n)
    mean[idx], inv_sigma[idx] = mean_e, w
    assert e.prior() is None
    raw = _packed(e, ps, add_prior=True)                                              # no prior set: the add queues nothing
    assert np.array_equal(raw, _packed(e, ps, add_prior=False))
    e.set_prior(mean, inv_sigma=inv_sigma)
    got_mean, got_w = e.prior()
    assert np.array_equal(got_mean, mean) and np.array_equal(got_w, inv_sigma)
    assert np.array_equal(raw, _packed(e, ps, add_prior=False))                       # the raw build does not include the prior
    got = _packed(e, ps, add_prior=True)
    _check_add(raw, got, lay, ps, idx, mean_e, w)
    # the entity without detections: its diagonal is exactly w^2
    k = (n - 3 * rig.n_keys + 3 * lone) if chain == "free" else 15 * rig.n_cams + 6 * lone + 5
    at = int(np.flatnonzero(idx == k)[0])
    assert raw[_places(lay, [k])[0][0]] == 0.0 and got[_places(lay, [k])[0][0]] == w[at] * w[at]
    # two runs, the same bits, in both contraction modes (the add itself has one order)
    for mode in (0, 1):
        e.set_option("deterministic", mode)
        assert np.array_equal(_packed(e, ps, True, packed_in=raw), got)
    e.set_option("deterministic", 1)
    # and the sum is prior_system of the oracle's H
    Href, gref, cref, _ = W.weighted_system(chain, det, ps, tm, np.ones(det.shape[0]))
    Hu, g, cost = _dense(got, lay)
    W.check(Hu, g, cost, *PR.prior_system(Href, gref, cref, ps, mean, inv_sigma))
    # sigma as the Python layer takes it: inf = no entry
    sigma = np.full(n, np.inf)
    sigma[idx] = 1.0 / w
    e.set_prior(mean, sigma)
    assert np.allclose(e.prior()[1], inv_sigma, rtol=1e-15, atol=0)
    e.set_prior()
    assert e.prior() is None


def test_a_prior_longer_than_one_workgroup():
    """The free chain on ring-4-big: 1 083 point coordinates (+ fx of four cameras + index 0) exceed PRIOR_PER_WG = 1 024, the share of
    one workgroup of prior_add_kernel: two workgroups park partial sums and prior_cost_kernel adds them in workgroup order."""
    rig = synthetic.make_rig("ring-4-big", 4, 3, synthetic.charuco_points(20, 8.0), seed=3, visibility=0.9)
    assert rig.n_keys == 361 and rig.detections.shape[0] == 3903
    det, ps = rig.detections, orc.build_param_list(*H.chain_slabs(rig, "free"))
    e = _engine("free", rig, det, None)
    e.set_option("deterministic", 1)
    lay = e.normal_layout()
    n = lay["n_params"]
    rng = np.random.default_rng(9)
    idx, w = _prior_entries("free", rig, n, rng, 3)
    assert idx.shape[0] > PRIOR_PER_WG and idx.shape[0] == 3 * 361 + 4
    mean_e = ps[idx] + rng.standard_normal(idx.shape[0]) / w
    mean, inv_sigma = np.zeros(n), np.zeros(n)
    mean[idx], inv_sigma[idx] = mean_e, w
    raw = _packed(e, ps, add_prior=False)
    e.set_prior(mean, inv_sigma=inv_sigma)
    got = _packed(e, ps, add_prior=True)
    _check_add(raw, got, lay, ps, idx, mean_e, w)
    for mode in (0, 1):
        e.set_option("deterministic", mode)
        assert np.array_equal(_packed(e, ps, True, packed_in=raw), got)


# ---- 2. clearing -----------------------------------------------------------------------------------------------------------------
def test_cleared_prior_new_table_and_refused_calls():
    from pycamset_amd.device_solver import lm_solve
    rig, det, ps, tm = W.chain_inputs("self")
    plain, touched = _engine("self", rig, det, tm), _engine("self", rig, det, tm)
    for e in (plain, touched):
        e.set_option("deterministic", 1)
    n = plain.n_params
    rng = np.random.default_rng(12)
    inv_sigma = np.where(rng.uniform(size=n) < 0.3, rng.uniform(0.5, 5.0, n), 0.0)
    mean = ps + 0.01 * rng.standard_normal(n)
    a = _packed(plain, ps, add_prior=True)
    touched.set_prior(mean, inv_sigma=inv_sigma)
    with_prior = _packed(touched, ps, add_prior=True)
    assert not np.array_equal(a, with_prior)
    touched.set_detections_table(det)                                                 # the prior is the handle's: a new table keeps it
    assert np.array_equal(touched.prior()[1], inv_sigma) and np.array_equal(touched.prior()[0], np.where(inv_sigma > 0, mean, 0.0))
    assert np.array_equal(with_prior, _packed(touched, ps, add_prior=True))
    # refused calls keep the previous prior
    lib = _capi.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    for bad_w, bad_m in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), (1.0, float("inf"))):
        wv, mv = np.ones(n), np.zeros(n)
        wv[n // 2], mv[n // 2] = bad_w, bad_m
        assert lib.pcs_set_prior(touched._h, mv.ctypes.data_as(dp), wv.ctypes.data_as(dp), n) == _capi.PCS_ERR_ARG
        assert b"pcs_set_prior" in lib.pcs_last_error()
    big = np.ones(n + 1)
    for m in (n - 1, n + 1, 0):
        assert lib.pcs_set_prior(touched._h, big.ctypes.data_as(dp), big.ctypes.data_as(dp), m) == _capi.PCS_ERR_ARG
    assert lib.pcs_set_prior(touched._h, None, big.ctypes.data_as(dp), n) == _capi.PCS_ERR_ARG
    nan_mean = np.where(inv_sigma > 0, mean, np.nan)                                  # a mean is only looked at where a weight is set
    with pytest.raises(ValueError):
        touched.set_prior(mean, np.zeros(n))                                          # sigma = 0
    assert np.array_equal(touched.prior()[1], inv_sigma)
    assert np.array_equal(with_prior, _packed(touched, ps, add_prior=True))
    touched.set_prior(nan_mean, inv_sigma=inv_sigma)
    assert np.array_equal(with_prior, _packed(touched, ps, add_prior=True))
    touched.set_prior()                                                               # cleared: the bits of an engine that never had one
    assert touched.prior() is None
    assert np.array_equal(a, _packed(touched, ps, add_prior=True))

    # solves: after a solve with a prior the handler solves exactly as one that never saw a prior (ordered mode: the same bits)
    _, h, x0 = W.ring4_handler("self")
    _, hf, _ = W.ring4_handler("self")
    for hh in (h, hf):
        hh.op_fun._engine_for(hh._flat_detections()).set_option("deterministic", 1)
    pm, psig = handlers.slab_prior(h, {"bdpt": 0.05, "intr": 10.0})
    first = lm_solve(h, x0.copy(), max_iter=6)
    with_p = lm_solve(h, x0.copy(), max_iter=6, prior_mean=pm, prior_sigma=psig)
    assert with_p.prior_cost > 0 and not np.array_equal(with_p.x, first.x)
    assert h.op_fun._engine_for(h._flat_detections()).prior() is None                # restored
    again = lm_solve(h, x0.copy(), max_iter=6)
    fresh = lm_solve(hf, x0.copy(), max_iter=6)
    for r in (again, fresh):
        assert r.cost == first.cost and np.array_equal(r.x, first.x) and np.array_equal(r.grad, first.grad) and r.prior_cost == 0.0


# ---- 3. with loss and weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_prior_with_huber_and_noise_weights(chain):
    rig, det, ps, tm = W.chain_inputs(chain)
    wd = W.log_uniform_weights(det.shape[0], 11)
    e = _engine(chain, rig, det, tm)
    e.set_loss("huber", 2.5)
    e.set_weights(inv_sigma=wd)
    lay = e.normal_layout()
    n = lay["n_params"]
    rng = np.random.default_rng(5)
    idx, w = _prior_entries(chain, rig, n, rng, 1)
    mean, inv_sigma = np.zeros(n), np.zeros(n)
    mean[idx], inv_sigma[idx] = ps[idx] + rng.standard_normal(idx.shape[0]) / w, w
    e.set_prior(mean, inv_sigma=inv_sigma)
    Href, gref, cref, slack = W.weighted_system(chain, det, ps, tm, wd, "huber", 2.5)
    Hp, gp, cp = PR.prior_system(Href, gref, cref, ps, mean, inv_sigma)             # the prior rows: outside the loss, not whitened
    for mode in (0, 1):
        e.set_option("deterministic", mode)
        Hu, g, cost = _dense(_packed(e, ps, add_prior=True), lay)
        W.check(Hu, g, cost, Hp, gp, cp, slack)
    assert e.loss() == ("huber", 2.5) and np.array_equal(e.weights(), wd)


# ---- 4. generated chain ----------------------------------------------------------------------------------------------------------
def _four_block_problem(free_all=False):
    from pycamset_amd import function_blocks as fb
    rig = W.ring4()
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()   # not one of the hand-fused chains
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    second = np.zeros((rig.n_imgs, 6))
    masks = [None, None, None, None] if free_all else [None, fix_ext, np.zeros((rig.n_imgs, 6), dtype=bool), None]
    return rig, handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, second, rig.poses], template=rig.points, unfixed=masks)


def test_generated_chain_build_and_solve_with_a_prior():
    """The four-block chain of the refusal tests, blocked and dense: the prior on a leading group (the intrinsics) and on the trailing
    one (the last poses) against the chain's own read-back J and r contracted on the host plus the prior, with the bounds of
    test_normal_equations_are_the_contracted_unshared_ones; then lm_solve against scipy on the augmented CSR closures."""
    from pycamset_amd.device_solver import lm_solve
    from tests.test_gpu_shared_params import check_normal
    rig, full = _four_block_problem(free_all=True)
    x = full.x0
    J = csr_array(full.make_loss_jac()(x))
    r = full.make_loss_fun()(x)
    ps = full._param_str(x)
    n = ps.shape[0]
    assert J.shape == (2 * rig.detections.shape[0], n)
    rng = np.random.default_rng(6)
    sig = [np.r_[np.full(4, np.inf), np.full(5, 0.02)], None, None, np.r_[np.full(3, 0.01), np.full(3, 2.0)]]
    mean_f, sigma_f = handlers.slab_prior(full, sig)
    mean_f = mean_f + np.where(np.isinf(sigma_f), 0.0, sigma_f) * rng.standard_normal(n)
    w = PR.weights_of(sigma_f)
    want, want_g, want_c = PR.prior_system((J.T @ J).toarray(), J.T @ r, float(r @ r), ps, mean_f, w)
    eng = full.op_fun._engine_for(full.det)
    full.op_fun._bind_template(eng, full.template)
    eng.set_prior(mean_f, sigma_f)
    assert np.array_equal(eng.prior()[1], w)
    for dense in (0, 1):
        eng.set_option("dense_normal", dense)
        lay = eng.normal_layout()
        assert (lay["n_trail"] == 0) == bool(dense) and (dense or lay["tb"] == 6)
        check_normal(_packed(eng, ps, add_prior=True), lay, n, want, want_g, want_c)
        raw = _packed(eng, ps, add_prior=False)
        check_normal(raw, lay, n, (J.T @ J).toarray(), J.T @ r, float(r @ r))             # the raw build stays the sum over the detections
    eng.set_option("dense_normal", 0)
    eng.set_prior()

    rig, prob = _four_block_problem()
    mean, sigma = handlers.slab_prior(prob, sig)
    mean = mean + np.where(np.isinf(sigma), 0.0, sigma) * rng.standard_normal(mean.shape)
    wf = PR.weights_of(sigma)
    fa, ja, n_prior = PR.augmented_closures(prob.make_loss_fun(), prob.make_loss_jac(), mean, wf)
    assert n_prior == 5 * rig.n_cams + 6 * rig.n_imgs
    ref = least_squares(fa, prob.x0.copy(), jac=ja, x_scale="jac", max_nfev=40)
    for dense in (0, 1):
        prob.op_fun._engine_for(prob.det).set_option("dense_normal", dense)
        res = lm_solve(prob, prob.x0.copy(), max_iter=40, prior_mean=mean, prior_sigma=sigma)
        assert res.n_jtjv == res.nfev - 1 and res.history == sorted(res.history, reverse=True)
        assert res.cost <= ref.cost * (1 + 1e-3), (dense, res.cost, ref.cost)
        assert abs(0.5 * np.sum(fa(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
        assert abs(res.prior_cost - PR.prior_half_sum(res.x, mean, wf)) <= 1e-12 * res.prior_cost
        host = lm_solve(prob, prob.x0.copy(), max_iter=40, reduce_fn=lambda a: a, prior_mean=mean, prior_sigma=sigma)
        assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (dense, host.cost, res.cost)
    prob.op_fun._engine_for(prob.det).set_option("dense_normal", 0)
    assert prob.op_fun._engine_for(prob.det).prior() is None
    with pytest.raises(NotImplementedError, match="generated chains"):                    # the refusals that stand
        lm_solve(prob, prob.x0, max_iter=3, loss="huber", prior_sigma=sigma)


# ---- 5. solves -------------------------------------------------------------------------------------------------------------------
def _in_stream_sum(t):
    t.mul_(1.0)
    return t


_in_stream_sum.on_device = True


@pytest.mark.parametrize("chain", ["template", "self"])
def test_solves_with_a_prior_match_scipy_through_every_loop(chain):
    """Linear, linear with sigma, and huber against least_squares on the augmented (whitened) closures — huber through the callable
    loss that leaves the prior rows linear — with the tolerances of test_weighted_solve_matches_scipy_on_the_whitened_closures;
    device-steered, host-steered and in-stream loops agree to 1e-9, PCG to 1e-3
    (test_lm_solve_reaches_the_scipy_solution_on_the_reduced_parameters)."""
    import torch
    from pycamset_amd.device_solver import lm_solve
    rig, h, x0 = W.ring4_handler(chain)
    tm = rig.points if chain == "template" else None
    fun, jac = W.oracle_closures(h, chain, tm)
    det = h._flat_detections()
    n_rows = 2 * det.shape[0]
    groups = {"intr": np.r_[np.full(4, np.inf), np.full(5, 0.02)], "pose": np.r_[np.full(3, np.inf), np.full(3, 5.0)]}
    if chain == "self":
        groups["bdpt"] = 0.05
    mean, sigma = handlers.slab_prior(h, groups)
    mean = mean + np.where(np.isinf(sigma), 0.0, sigma) * np.random.default_rng(4).standard_normal(mean.shape)
    w = PR.weights_of(sigma)
    kw = dict(prior_mean=mean, prior_sigma=sigma)
    per_cam = np.array([0.5, 1.0, 2.0, 4.0])
    wd = 1.0 / per_cam[det[:, 0].astype(int)]
    start = x0
    for name, loss, sig in (("linear", "linear", None), ("weighted", "linear", per_cam), ("huber", "huber", per_cam)):
        f0, j0 = (fun, jac) if sig is None else W.whitened_closures(fun, jac, wd)
        fa, ja, n_prior = PR.augmented_closures(f0, j0, mean, w)
        ref = least_squares(fa, start.copy(), jac=ja, x_scale="jac", max_nfev=300, loss="linear" if loss == "linear" else PR.split_loss(loss, n_rows))
        res = lm_solve(h, start.copy(), max_iter=200, loss=loss, f_scale=1.0, sigma=sig, **kw)
        f = fa(res.x)
        rho = np.stack([f * f, np.ones_like(f)]) if loss == "linear" else PR.split_loss(loss, n_rows)(f * f)
        assert abs(res.cost - 0.5 * np.sum(rho[0])) <= 1e-9 * res.cost, name
        assert res.cost <= ref.cost * (1 + 1e-6), (name, res.cost, ref.cost)
        g_ref = ja(res.x).T @ (rho[1] * f)
        assert np.max(np.abs(res.grad - g_ref)) <= 1e-9 * max(np.max(np.abs(ja(res.x).T @ np.abs(rho[1] * f))), 1.0), name
        assert abs(res.prior_cost - PR.prior_half_sum(res.x, mean, w)) <= 1e-12 * res.prior_cost, name
        assert abs(res.prior_cost - 0.5 * np.sum(f[n_rows:] ** 2)) <= 1e-12 * res.prior_cost, name
        host = lm_solve(h, start.copy(), max_iter=200, reduce_fn=lambda a: a, loss=loss, f_scale=1.0, sigma=sig, **kw)
        assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (name, host.cost, res.cost)
        dev = lm_solve(h, start.copy(), max_iter=200, reduce_fn=_in_stream_sum, loss=loss, f_scale=1.0, sigma=sig, **kw)
        assert abs(dev.cost - res.cost) <= 1e-9 * res.cost, (name, dev.cost, res.cost)
        if name == "linear":
            cg = lm_solve(h, start.copy(), max_iter=200, linear_solver="pcg", **kw)
            assert cg.n_jtjv > cg.nfev and abs(cg.cost - res.cost) <= 1e-3 * res.cost, (cg.cost, res.cost)
            assert abs(cg.prior_cost - PR.prior_half_sum(cg.x, mean, w)) <= 1e-12 * cg.prior_cost
        if name == "weighted":
            start = res.x              # the huber solve starts where the weighted linear one ended, as in the weighted-solve test
    torch.cuda.synchronize()
    eng = h.op_fun.engine
    assert eng.prior() is None and eng.weights() is None and eng.loss() == ("linear", 1.0)
    after = lm_solve(h, x0.copy(), max_iter=30)
    _, hf, _ = W.ring4_handler(chain)
    fresh = lm_solve(hf, x0.copy(), max_iter=30)
    assert after.prior_cost == 0.0
    assert abs(after.cost - fresh.cost) <= 1e-9 * fresh.cost and np.max(np.abs(after.x - fresh.x)) <= 1e-7 * np.max(np.abs(fresh.x))


# ---- 6. limits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["template", "self"])
def test_a_tight_prior_fixes_and_a_loose_one_vanishes(chain):
    """sigma = 1e-9 on every intrinsic reproduces the solve with the intrinsics fixed; sigma = 1e12 the solve without a prior.

    At the minimiser w^2 (x_i - mu_i) = -(J'r)_i, so an intrinsic stays within G / w^2 of its mean, G the largest |J'r| over the
    intrinsics between start and end, plus the rounding of storing it (2 ulp).  scipy's least_squares on the augmented closures with the
    same sigma moved the intrinsics by at most 1.0e-14 (template) / 2.4e-15 (self) and ended within 5.8e-8 / 2.4e-6 of the
    fixed-intrinsics solve in the other parameters, 1.2e-12 / 5.4e-11 in relative cost: those are the bounds here."""
    from pycamset_amd.device_solver import lm_solve
    rig, h, x0 = W.ring4_handler(chain)
    nI = 9 * rig.n_cams
    mean, sigma = handlers.slab_prior(h, {"intr": 1e-9}, {"intr": rig.intr})
    tight = lm_solve(h, x0.copy(), max_iter=100, prior_mean=mean, prior_sigma=sigma)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    fp = {name: {"int": rig.intr[i].copy()} for i, name in enumerate(names)}
    fp["cam_0"]["ext"] = rig.extr_true[0].copy()
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    hfix = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections), fixed_params=fp, options={"verbosity": 0})
    fixed = lm_solve(hfix, x0[nI:].copy(), max_iter=100)
    tm = rig.points if chain == "template" else None
    fun, jac = W.oracle_closures(h, chain, tm)
    G = max(np.max(np.abs((jac(x).T @ fun(x))[:nI])) for x in (x0, tight.x))
    move = np.abs(tight.x[:nI] - x0[:nI])
    print(f"{chain}: intrinsics moved by at most {move.max():.3e} (G / w^2 = {G * 1e-18:.3e}), rest differs by {np.max(np.abs(tight.x[nI:] - fixed.x)):.3e}, "
          f"cost {tight.cost:.12e} vs {fixed.cost:.12e}, prior cost {tight.prior_cost:.3e}")
    assert np.all(move <= G * 1e-18 + 2 * np.spacing(np.abs(x0[:nI])))
    assert np.max(np.abs(tight.x[nI:] - fixed.x)) <= {"template": 5.8e-8, "self": 2.4e-6}[chain]
    assert abs(tight.cost - fixed.cost) <= 1e-9 * fixed.cost
    loose = lm_solve(h, x0.copy(), max_iter=100, prior_sigma=np.full(x0.shape, 1e12))
    none = lm_solve(h, x0.copy(), max_iter=100)
    assert abs(loose.cost - none.cost) <= 1e-9 * none.cost, (loose.cost, none.cost)


# ---- 7. gauge-free self-calibration ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauge_free():
    rig = W.ring4()
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.SelfBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                   fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0, "gauge": "free", "fixed_pose": []})
    bp = h.bundlePrimitive
    assert bp.poses_unfixed.all() and bp.bdpt_unfixed.all() and not bp.extr_unfixed[0]        # camera 0's extrinsics fixed, every point free
    x = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses.ravel(), rig.points.ravel()])
    return rig, h, x


def test_gauge_free_self_calibration_covariance():
    from pycamset_amd.device_solver import parameter_covariance
    from tests.test_gpu_covariance import _compare, _oracle_jac, _reference
    rig, h, x = _gauge_free()
    with pytest.raises(np.linalg.LinAlgError, match="gauge"):
        parameter_covariance(h, x)
    mean, sigma = handlers.slab_prior(h, {"bdpt": 0.05})
    cov = parameter_covariance(h, x, prior_mean=mean, prior_sigma=sigma)
    mask = np.asarray(h._jac_mask(), bool)
    K3 = 3 * rig.n_keys
    assert cov.dof == 2 * rig.detections.shape[0] + K3 - mask.sum()
    J, r = _oracle_jac(h, x)
    n = mask.shape[0]
    free = np.flatnonzero(mask)
    w_str, mean_str = np.zeros(n), np.zeros(n)
    w_str[free], mean_str[free] = PR.weights_of(sigma), mean
    rows = np.flatnonzero(w_str > 0)
    Jp = csr_array((w_str[rows], (np.arange(rows.shape[0]), rows)), shape=(rows.shape[0], n))
    ps = h.op_fun.build_param_list(*h.get_bundle_adjustment_inputs(x))
    Ja, ra = csr_array(vstack([J, Jp])), np.r_[r, w_str[rows] * (ps[rows] - mean_str[rows])]
    full, s2, kappa = _reference(Ja, ra, mask)
    assert abs(cov.sigma2 - s2) <= 1e-10 * s2 and abs(cov.cost - 0.5 * float(ra @ ra)) <= 1e-10 * cov.cost
    _compare(cov, h.get_bundle_adjustment_inputs(x), full, mask, kappa, "gauge free, point prior")
    assert cov.min_pivot > 1e-10
    ab = parameter_covariance(h, x, prior_sigma=sigma, absolute_sigma=True)                  # no mean needed
    full_abs, _, _ = _reference(Ja, ra, mask, absolute_sigma=True)
    _compare(ab, h.get_bundle_adjustment_inputs(x), full_abs, mask, kappa, "gauge free, absolute")


def test_gauge_free_self_calibration_solve_stays_in_the_nominal_frame():
    from pycamset_amd.device_solver import lm_solve
    rig, h, x = _gauge_free()
    sig = 0.05
    mean, sigma = handlers.slab_prior(h, {"bdpt": sig})
    x0 = x * (1 + 1e-3 * np.random.default_rng(2).standard_normal(x.shape))
    res = lm_solve(h, x0, max_iter=100, prior_mean=mean, prior_sigma=sigma)
    assert res.status in (1, 3, 4), (res.status, res.message)
    K = rig.n_keys
    pts, nominal = res.x[-3 * K:].reshape(K, 3), rig.points

    def spread(p):
        d = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=-1)
        return d[np.triu_indices(K, 1)].mean()

    bound = 3 * sig / np.sqrt(K)
    print(f"centroid moved by {np.abs(pts.mean(0) - nominal.mean(0)).max():.3e}, mean pairwise distance by {abs(spread(pts) - spread(nominal)):.3e}, bound {bound:.3e}")
    assert np.all(np.abs(pts.mean(0) - nominal.mean(0)) <= bound)
    assert abs(spread(pts) - spread(nominal)) <= bound


# ---- 8. an entity without detections -------------------------------------------------------------------------------------------------
def test_an_unobserved_pose_has_its_prior_sigma_as_standard_error():
    from pycamset_amd.device_solver import parameter_covariance
    rig = W.ring4()
    lone = 3
    det = rig.detections[rig.detections[:, 1] != lone]
    rig, h, x = W.ring4_handler("template", det=det)
    assert h.bundlePrimitive.poses.shape[0] == rig.n_imgs and h.bundlePrimitive.poses_unfixed[lone]
    pose_sigma = np.full((rig.n_imgs, 6), np.inf)
    pose_sigma[lone] = [0.01, 0.02, 0.03, 1.0, 2.0, 3.0]
    mean, sigma = handlers.slab_prior(h, {"pose": pose_sigma})
    cov = parameter_covariance(h, x, prior_sigma=sigma, absolute_sigma=True)
    at = np.flatnonzero(np.isfinite(sigma))
    assert at.shape[0] == 6
    assert np.all(np.abs(cov.std[at] - pose_sigma[lone]) <= 1e-12 * pose_sigma[lone]), cov.std[at]
    blk = cov.blocks[2][lone]
    assert np.all(np.abs(np.diag(blk) - pose_sigma[lone] ** 2) <= 1e-12 * pose_sigma[lone] ** 2) and np.all(blk[~np.eye(6, dtype=bool)] == 0.0)
