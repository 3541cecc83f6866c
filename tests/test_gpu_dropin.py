"""Drop-in boundary on the GPU: the optimisation_function adapter and the ParamHandler closures
against the goldens produced by the reference's own handlers, and scipy.least_squares driven by
the HIP closures."""
import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.sparse import csr_array

from oracle import ba_oracle as orc
from pycamset_amd import function_blocks as fb
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests import helpers as H
from tests.test_host_logic import R2_CASES, R2_SAME_AS_REFERENCE, DuckCamset, DuckTarget, make_handler, make_handler_r2

pytestmark = pytest.mark.gpu


def chain_op(chain):
    if chain == "template":
        return fb.projection() + fb.extrinsic3D() + fb.template_points()
    if chain == "self":
        return fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.free_point()
    return fb.projection() + fb.extrinsic3D() + fb.free_point()


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_operator_api_on_the_3000_detection_fixture(golden_dir, chain):
    """SURVEY 8c's (4 cams, 20 images, 486 keys, N ~ 3000) block-level case, made by the reference."""
    g = np.load(golden_dir / f"block_{chain}_large.npz")
    det, ps = g["detections"], g["param_str"]
    tm = g["points"] if chain == "template" else None
    op = chain_op(chain)
    P = op.param_line_length
    H.assert_resid_close(op.make_full_loss_fn(det, 5)(ps, tm), g["resid_t5"], det[:, 3:])
    d, c, rp = op.make_jacobean(det, 5)(ps, tm)
    H.assert_jac_close(d.reshape(-1, P), g["data_all_t5"].reshape(-1, P))
    assert np.array_equal(c, g["indices_all_t5"]) and np.array_equal(rp, g["indptr_all_t5"])
    dm, cm, rpm = op.make_jacobean(det, 5, unfixed_params=g["unfixed"])(ps, tm)
    assert np.array_equal(cm, g["indices_masked_t5"]) and np.array_equal(rpm, g["indptr_masked_t5"])
    keep = np.repeat(g["unfixed"][g["block_param_inds"]], 2, axis=0).reshape(-1)
    assert np.array_equal(dm, d[keep])      # device-side compaction = dense[mask], bit for bit


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_operator_api_matches_reference_goldens(golden_dir, chain):
    g = np.load(golden_dir / f"block_{chain}_medium.npz")
    det, ps = g["detections"], g["param_str"]
    tm = g["points"] if chain == "template" else None
    op = chain_op(chain)
    assert op.can_make_jac()
    loss = op.make_full_loss_fn(det, 4)
    r = loss(ps, tm) if tm is not None else loss(ps)
    assert r.shape == (det.shape[0], 2)
    H.assert_resid_close(r, g["resid_t4"], det[:, 3:])
    jac = op.make_jacobean(det, 4)
    d, c, rp = jac(ps, tm) if tm is not None else jac(ps)
    P = op.param_line_length
    H.assert_jac_close(d.reshape(-1, P), g["data_all_t4"].reshape(-1, P))
    assert np.array_equal(c, g["indices_all_t4"]) and np.array_equal(rp, g["indptr_all_t4"])
    jac_m = op.make_jacobean(det, 4, unfixed_params=g["unfixed"])
    dm, cm, rpm = jac_m(ps, tm) if tm is not None else jac_m(ps)
    assert np.array_equal(cm, g["indices_masked_t4"]) and np.array_equal(rpm, g["indptr_masked_t4"])
    assert dm.shape == g["data_masked_t4"].shape
    assert np.max(np.abs(dm - g["data_masked_t4"])) <= 1e-10 * np.max(np.abs(g["data_masked_t4"]))
    # the all-free closure still works after the masked one re-bound the engine
    d2, _, _ = jac(ps, tm) if tm is not None else jac(ps)
    assert np.array_equal(d2, d)
    assert np.array_equal(op.build_param_list(g["intr"], g["extr"]), np.concatenate([g["intr"].ravel(), g["extr"].ravel()]))
    assert np.array_equal(op.get_block_param_inds(det, 4), g["block_param_inds"])


@pytest.mark.parametrize("chain", ["template", "self", "free"])
@pytest.mark.parametrize("tag,fixed", [("tiny", True), ("tiny_nofix", False)])
def test_handler_closures_match_reference_goldens(golden_dir, chain, tag, fixed):
    g = np.load(golden_dir / f"handler_{chain}_{tag}.npz")
    h = make_handler(g, chain, fixed)
    x = g["x"].copy()
    loss_fn = h.make_loss_fun(2)
    jac_fn = h.make_loss_jac(2)
    r = loss_fn(x)
    assert r.shape == g["resid"].shape and r.flags.c_contiguous
    uv = np.repeat(np.max(np.abs(g["detections"][:, 3:]), axis=1), 2)
    assert np.max(np.abs(r - g["resid"]) / np.maximum(np.abs(g["resid"]), 1e-3 * uv)) <= H.RES_RTOL
    J = jac_fn(x)
    assert isinstance(J, csr_array) and tuple(J.shape) == tuple(g["shape"])
    assert np.array_equal(J.indices, g["indices"]) and np.array_equal(J.indptr, g["indptr"])
    ref = csr_array((g["data"], g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    rows = np.repeat(np.max(np.abs(ref).toarray(), axis=1), np.diff(g["indptr"]))
    err = np.max(np.abs(J.data - g["data"]) / np.maximum(np.abs(g["data"]), H.ROW_FLOOR * rows))
    assert err <= H.JAC_RTOL
    # rows of the fixed pose 0 lose their 6 pose columns
    if chain == "template" and not fixed:
        per_row = np.diff(J.indptr)
        on_pose0 = np.repeat(g["detections"][:, 1] == 0, 2)
        assert set(per_row[on_pose0]) == {15} and set(per_row[~on_pose0]) == {21}


def _check_closures(h, g, ref_resid, ref_data, ref_idx, ref_ptr):
    x = g["x"].copy()
    r = h.make_loss_fun(2)(x)
    J = h.make_loss_jac(2)(x)
    assert r.shape == ref_resid.shape and isinstance(J, csr_array) and tuple(J.shape) == (ref_resid.shape[0], x.shape[0])
    det = h._flat_detections()
    uv = np.repeat(np.max(np.abs(det[:, 3:]), axis=1), 2)
    assert np.max(np.abs(r - ref_resid) / np.maximum(np.abs(ref_resid), 1e-3 * uv)) <= H.RES_RTOL
    assert np.array_equal(J.indices, ref_idx) and np.array_equal(J.indptr, ref_ptr)
    ref = csr_array((ref_data, ref_idx, ref_ptr), shape=J.shape)
    rows = np.repeat(np.max(np.abs(ref).toarray(), axis=1), np.diff(ref_ptr))
    assert np.max(np.abs(J.data - ref_data) / np.maximum(np.abs(ref_data), H.ROW_FLOOR * rows)) <= H.JAC_RTOL
    return J


@pytest.mark.parametrize("name", R2_SAME_AS_REFERENCE)
def test_ccube_shaped_and_edge_handler_closures_match_reference_goldens(golden_dir, name):
    """Ccube-shaped targets (point_data (6, 81, 3), multi-dimensional keys, N ~ 1e3), fixed_pose 3 / None, a camera
    with both 'int' and 'ext' fixed, trailing unobserved images / keys: HIP closures vs fixtures made by the
    reference's own handlers (th:157-193, sbh:184-226)."""
    g = np.load(golden_dir / f"{name}.npz")
    h, chain = make_handler_r2(g, name)
    J = _check_closures(h, g, g["resid"], g["data"], g["indices"], g["indptr"])
    assert tuple(J.shape) == tuple(g["shape"])
    if name == "handler_template_ccube":   # rows on the fixed pose 3 / the fully fixed camera 2 are shorter
        det = h._flat_detections()
        per_row = np.diff(J.indptr)[::2]
        expect = 21 - 6 * (det[:, 1] == 3) - 15 * (det[:, 0] == 2) - 6 * (det[:, 0] == 0)
        assert np.array_equal(per_row, expect)


@pytest.mark.parametrize("name", ["quirk_self_last_image_unobserved", "quirk_template_last_cam_unobserved"])
def test_trailing_unobserved_entities_use_the_slab_layout(golden_dir, name):
    """Where the reference's max(index)+1 rule mis-offsets a group (quirk ii, afb:793-795) the engine is laid out
    from the handler's slab sizes: the closures agree with the oracle under those counts (and the CPU test shows
    the fixture is the mis-offset evaluation)."""
    g = np.load(golden_dir / f"{name}.npz")
    h, chain = make_handler_r2(g, name)
    x = g["x"].copy()
    ps = orc.build_param_list(*h.get_bundle_adjustment_inputs(x))
    det, tmpl, mask, counts = h._flat_detections(), h._template_arg(), h._jac_mask(), h.op_fun.counts
    idx, ptr, m = orc.csr_structure(chain, det, mask, counts)
    dense, res = orc.full_jac_dense(chain, det, ps, tmpl, with_resid=True, counts=counts)
    _check_closures(h, g, res.reshape(-1), dense[m], idx, ptr)


@pytest.mark.parametrize("name", sorted(R2_CASES))
def test_reference_layout_rule_reproduces_the_reference_quirks_included(golden_dir, name):
    """counts="reference" = what a reference handler patched with the adapter gets: layout
    from max index + 1 of the detections (afb:793-795), longer strings / masks read by their leading entries.  That is
    bit-compatible with the reference even where its rule mis-offsets a group (quirk ii) — all seven fixtures match."""
    g = np.load(golden_dir / f"{name}.npz")
    h, chain = make_handler_r2(g, name, counts="reference")
    assert h.op_fun.counts is None
    _check_closures(h, g, g["resid"], g["data"], g["indices"], g["indptr"])


def _oracle_closures(h, chain):
    det = h._flat_detections()
    tmpl = h._template_arg()
    mask = h._jac_mask()
    idx, ptr, m = orc.csr_structure(chain, det, mask)

    def loss(x):
        ps = orc.build_param_list(*h.get_bundle_adjustment_inputs(x))
        return orc.full_loss(chain, det, ps, tmpl, threads=8, fast=True).flatten()

    def jac(x):
        ps = orc.build_param_list(*h.get_bundle_adjustment_inputs(x))
        dense = orc.full_jac_dense(chain, det, ps, tmpl, threads=8, fast=True)
        return csr_array((dense[m], idx, ptr), shape=(2 * det.shape[0], x.shape[0]))

    return loss, jac


@pytest.mark.parametrize("chain", ["template", "self"])
def test_least_squares_with_hip_closures_converges_like_the_cpu_path(chain):
    """optimisation_handling.py:88-98: least_squares(loss_fn, x0, jac=jac_fn, x_scale='jac') on a
    synthetic 8-camera ring; the HIP closures and CPU-oracle closures must walk to the same x."""
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    fixed = {"cam_0": {"ext": rig.extr_true[0].copy()}}

    def build():
        return cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                   fixed_params={k: dict(v) for k, v in fixed.items()}, options={"verbosity": 0, "max_nfev": 12})

    h = build()
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    x0 = np.concatenate(parts)
    loss_fn, jac_fn = h.make_loss_fun(1), h.make_loss_jac(1)
    res = least_squares(loss_fn, x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=12, verbose=0)
    h2 = build()
    o_loss, o_jac = _oracle_closures(h2, chain)
    ref = least_squares(o_loss, x0.copy(), jac=o_jac, x_scale="jac", max_nfev=12, verbose=0)
    e0 = np.mean(np.linalg.norm(loss_fn(x0).reshape(-1, 2), axis=1))
    e1 = np.mean(np.linalg.norm(res.fun.reshape(-1, 2), axis=1))
    e_ref = np.mean(np.linalg.norm(ref.fun.reshape(-1, 2), axis=1))
    assert e1 < 0.6 and e1 < e0  # noise floor is 0.3 px per axis
    # trf + lsmr on this rig crawls along nearly flat focal-length / depth directions and amplifies
    # 1e-13 input perturbations to 5e-6 in the cost after 100 evaluations (measured with the CPU
    # closures alone), so the two runs are compared on cost and reprojection error, not on x.
    assert res.nfev == ref.nfev
    assert abs(res.cost - ref.cost) <= 1e-4 * ref.cost
    assert abs(e1 - e_ref) <= 1e-4
    # same first step: one evaluation from the common start must agree to rounding
    assert np.max(np.abs(loss_fn(x0) - o_loss(x0))) <= 1e-9


def test_handler_closures_with_the_mixed_engine():
    """dtype='mixed' through the handler surface: the closures return float64 arrays whose values are the FP64
    results rounded once to FP32 (1.2e-7), the CSR structure is unchanged, and the device solver — which never reads
    the FP32 stream — reaches the FP64 solution."""
    from pycamset_amd.device_solver import lm_solve
    rig = synthetic.make_rig("ring-5-small", 5, 8, synthetic.charuco_points(7, 8.0), seed=29, visibility=0.9)
    names = [f"cam_{i}" for i in range(rig.n_cams)]

    def build(dtype):
        return handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                              fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0}, dtype=dtype)

    h64, hmx = build("f64"), build("mixed")
    bp = h64.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()])
    r64, rmx = h64.make_loss_fun(1)(x0), hmx.make_loss_fun(1)(x0)
    J64, Jmx = h64.make_loss_jac(1)(x0), hmx.make_loss_jac(1)(x0)
    assert rmx.dtype == np.float64 and Jmx.data.dtype == np.float64
    assert np.array_equal(J64.indices, Jmx.indices) and np.array_equal(J64.indptr, Jmx.indptr)
    assert np.max(np.abs(rmx - r64) / np.maximum(np.abs(r64), 1e-3)) <= 1.2e-7
    rowmax = np.repeat(np.abs(J64).max(axis=1).toarray().ravel(), np.diff(J64.indptr))
    assert np.max(np.abs(Jmx.data - J64.data) / np.maximum(np.abs(J64.data), 1e-6 * rowmax)) <= 1.2e-7
    a, b = lm_solve(h64, x0.copy(), max_iter=25), lm_solve(hmx, x0.copy(), max_iter=25)
    assert abs(a.cost - b.cost) <= 1e-6 * a.cost   # atomics reorder the sums: the two runs may stop one step apart


def test_run_bundle_adjustment_caller_with_both_solvers():
    """optimisation_handling.run_bundle_adjustment (the reference's caller, oh:52-117) end to end: scipy on the
    HIP closures and the device solver (block-reduced normal equations + Schur step) reach the same solution
    and hand back the full parameter slabs."""
    from pycamset_amd.optimisation_handling import run_bundle_adjustment
    rig = synthetic.make_rig("ring-6-small", 6, 10, synthetic.charuco_points(9, 8.0), seed=23, visibility=0.85)
    names = [f"cam_{i}" for i in range(rig.n_cams)]

    def build():
        h = handlers.TemplateBundleHandler(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
                                           fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0, "max_nfev": 40})
        bp = h.bundlePrimitive
        h.set_initial_params(np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]))
        return h

    r_scipy, slabs_scipy = run_bundle_adjustment(build())
    out = {}
    for ls in ("cholesky", "pcg"):
        r_dev, slabs = run_bundle_adjustment(build(), solver="device", linear_solver=ls)
        out[ls] = r_dev
        assert r_dev.cost <= r_scipy.cost * (1 + 1e-3), ls
        assert [a.shape for a in slabs] == [a.shape for a in slabs_scipy]
        assert np.array_equal(slabs[1][0], rig.extr_true[0])              # the fixed extrinsic is handed back untouched
    # exact steps (Cholesky) end at least as low as the inexact CG steps, and both sit on the noise floor
    assert out["cholesky"].cost <= out["pcg"].cost * (1 + 1e-6)
    assert abs(out["cholesky"].cost - out["pcg"].cost) <= 1e-3 * out["pcg"].cost


# ---- Jacobian kept on the device -------------------------------------------------------
@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_matrix_free_products_match_sparse_products_of_the_oracle_jacobian(chain):
    """J v, J^T u, J^T J v, diag(J^T J), J^T r and the cost, against scipy.sparse products of the
    oracle's Jacobian.  f64 atomics reorder the sums: |a - b| <= 1e-10 * max|ref|.  tests/test_gpu_matfree.py holds the same
    products to a bound per entry (tests/matfree_reference.py), at every tile shape and in both accumulator forms."""
    from pycamset_amd.engine import Engine
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    dense, r = orc.full_jac_dense(chain, rig.detections, ps, tm, with_resid=True)
    idx, ptr, _ = orc.csr_structure(chain, rig.detections, np.ones(ps.shape[0], bool))
    J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * rig.n_det, ps.shape[0]))
    rng = np.random.default_rng(3)
    v = rng.standard_normal(ps.shape[0])
    u = rng.standard_normal(2 * rig.n_det)
    for order in ("sorted", "shuffled"):  # wave-uniform fast path and per-lane atomic path
        det = rig.detections if order == "sorted" else rig.detections[np.random.default_rng(0).permutation(rig.n_det)]
        Jo = J if order == "sorted" else None
        e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys)
        e.set_detections_table(det)
        if tm is not None:
            e.set_template(tm)
        e.linearize(ps)

        def close(a, b):
            assert a.shape == b.shape
            assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b)), float(np.max(np.abs(a - b)) / np.max(np.abs(b)))

        for tpw in (0, 12, 32):   # 1, 3 and up to 8 tiles per wave: the kernels' two-level tile pipeline (ragged last workgroup)
            e.set_option("tiles_per_wg", tpw)
            if Jo is not None:
                close(e.jv(v), Jo @ v)
                close(e.jtu(u), Jo.T @ u)
            close(e.jtjv(v), J.T @ (J @ v))
            close(e.jtj_diag(), np.asarray(J.multiply(J).sum(axis=0)).ravel())
            g, cost = e.grad()
            close(g, J.T @ r.reshape(-1))
            assert abs(cost - float(np.sum(r * r))) <= 1e-10 * float(np.sum(r * r))
        e.set_option("tiles_per_wg", 0)
        # an evaluation re-linearises too
        e.eval(ps * (1 + 1e-3), want_jac=False)
        e.linearize(ps)
        close(e.jtjv(v), J.T @ (J @ v))
        e.close()


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_blocked_normal_equations_and_schur_step(chain):
    """Round 3: J^T J stored as [A | B | C] (leading x leading, leading x trailing, block-diagonal trailing group) must hold
    exactly the entries of the dense build, and the device Schur step (csrc/ba_schur.hpp + library GEMM / Cholesky) must solve
    (H + lam diag(H)) x = -g with the fixed parameters' rows and columns replaced by the identity — checked against a dense
    NumPy solve of that very system.  Shuffled table too (every pass walks sorted copies)."""
    import torch
    from pycamset_amd.device_solver import BlockedNormalEquations
    from pycamset_amd.engine import Engine
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    rng = np.random.default_rng(4)
    for det in (rig.detections, rig.detections[rng.permutation(rig.n_det)]):
        e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys)
        e.set_detections_table(det)
        if tm is not None:
            e.set_template(tm)
        Hd, g_ref, c_ref = e.normal_equations(ps)
        n = ps.shape[0]
        lay = e.normal_layout()
        nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
        assert nl + nt == n and lay["packed_len"] == nl * nl + nl * nt + nt * tb + n + 1
        mask = rng.random(n) > 0.15
        mask[nl + 1] = False                      # one coordinate of the first trailing entity: a partly fixed block
        ne = BlockedNormalEquations(e, mask)
        d_ps = torch.from_numpy(ps).cuda()
        ne.build(d_ps, 0)
        torch.cuda.synchronize()
        pk = ne.packed[0][: ne.n_packed].cpu().numpy()          # one more word behind it: the ranks' void votes
        A = pk[: nl * nl].reshape(nl, nl)
        B = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
        C = pk[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
        g = pk[-(n + 1):-1]
        scale = np.sqrt(np.outer(np.diag(Hd), np.diag(Hd)))
        scale[scale == 0] = 1.0
        Hb = np.zeros((n, n))
        Hb[:nl, :nl] = np.triu(A)
        assert np.all(np.tril(A, -1) == 0)
        Hb[:nl, nl:] = B
        for k in range(C.shape[0]):
            assert np.all(np.tril(C[k], -1) == 0)
            Hb[nl + k * tb: nl + (k + 1) * tb, nl + k * tb: nl + (k + 1) * tb] = C[k]
        Hb = Hb + np.triu(Hb, 1).T
        assert np.max(np.abs(Hb - Hd) / scale) <= 1e-10            # same entries (atomics reorder the sums)
        assert np.max(np.abs(g - g_ref)) <= 1e-10 * np.max(np.abs(g_ref)) and abs(pk[-1] - c_ref) <= 1e-10 * c_ref
        # the damped, masked system in NumPy
        for lam_v in (1e-3, 10.0):
            lam = torch.full((1,), lam_v, dtype=torch.float64, device="cuda")
            d_trial = torch.empty_like(d_ps)
            torch.cuda.synchronize()              # `lam` is filled on torch's stream, the solver works on its own
            delta = ne.solve(0, lam, d_ps, d_trial)
            pred, ok = ne.predicted_reduction(lam)
            torch.cuda.synchronize()
            assert bool(ok.item())
            assert np.array_equal(d_trial.cpu().numpy(), ps + delta.cpu().numpy())      # the trial parameter string comes with the step
            d = np.maximum(np.diag(Hb), 1e-300) * mask
            M = Hb * np.outer(mask, mask) + np.diag(lam_v * d) + np.diag((~mask).astype(float))
            x_ref = np.linalg.solve(M, -(g * mask))
            x = delta.cpu().numpy()
            assert np.all(x[~mask] == 0)
            assert np.max(np.abs(x - x_ref)) <= 1e-8 * np.max(np.abs(x_ref)), (chain, lam_v, np.max(np.abs(x - x_ref)), np.max(np.abs(x_ref)))
            pred_ref = 0.5 * (lam_v * np.sum(d * x_ref * x_ref) - np.dot(g * mask, x_ref))
            assert abs(float(pred.item()) - pred_ref) <= 1e-8 * abs(pred_ref)
        # deterministic mode: the blocked build and the whole step hold the same bits on every run, and the values of the atomics build
        e.set_option("deterministic", 1)
        lam = torch.full((1,), 1e-3, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            ne.build(d_ps, 1)
            torch.cuda.synchronize()
            built = ne.packed[1][: ne.n_packed].cpu().numpy()      # before the step: the solve masks B in place (fixed rows / columns -> 0)
            delta = ne.solve(1, lam, d_ps, d_trial)
            torch.cuda.synchronize()
            runs.append((built, delta.cpu().numpy().copy()))
        assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:])
        pk1 = runs[0][0]
        nb_ = nl * nl + nl * nt + nt * tb
        Hd1 = np.zeros((n, n))
        Hd1[:nl, :nl] = np.triu(pk1[: nl * nl].reshape(nl, nl))
        Hd1[:nl, nl:] = pk1[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
        C1 = pk1[nl * nl + nl * nt: nb_].reshape(-1, tb, tb)
        for k in range(C1.shape[0]):
            Hd1[nl + k * tb: nl + (k + 1) * tb, nl + k * tb: nl + (k + 1) * tb] = C1[k]
        Hd1 = Hd1 + np.triu(Hd1, 1).T
        assert np.max(np.abs(Hd1 - Hd) / scale) <= 1e-10
        assert np.max(np.abs(pk1[nb_: nb_ + n] - g_ref)) <= 1e-10 * np.max(np.abs(g_ref)) and abs(pk1[nb_ + n] - c_ref) <= 1e-10 * c_ref
        e.set_option("deterministic", 0)
        e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_block_reduced_normal_equations_match_the_oracle_jacobian(chain, dtype):
    """H = J^T J, g = J^T r, cost = r^T r in one pass (no J in memory) against the same products of the
    oracle's Jacobian.  A Gram matrix obeys |H_ij| <= sqrt(H_ii H_jj), so that is the scale of the
    tolerance: |dH_ij| <= 1e-10 sqrt(H_ii H_jj) (atomics reorder the sums; the arithmetic is FP64 for every dtype).  An
    F32 engine holds the measurements as float, so g and the cost — the only outputs that depend on them — agree to 1e-6."""
    from pycamset_amd.engine import Engine
    rig = synthetic.config_rig(1)
    ps = orc.build_param_list(*H.chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    tol = 1e-10
    tol_r = 1e-10 if dtype == "f64" else 1e-6
    rng = np.random.default_rng(0)
    orders = {"sorted": np.arange(rig.n_det), "shuffled": rng.permutation(rig.n_det),
              # runs of 7 detections: every tile mixes several (cam, image) pairs but keeps some run structure
              "runs-of-7": np.concatenate([np.arange(s, min(s + 7, rig.n_det)) for s in rng.permutation(np.arange(0, rig.n_det, 7))]),
              # a third of the table: most (image, key) pairs are left with one or two cameras, so a tile of the pose-point pass
              # holds up to 64 runs (four batches of 16), and some cameras / images / keys lose all their detections
              "thinned": np.sort(rng.choice(rig.n_det, rig.n_det // 3, replace=False))}
    H_ref = None
    for name, perm in orders.items():
        if H_ref is None or name == "thinned":   # the products do not depend on the row order
            det = rig.detections[perm]
            dense, r = orc.full_jac_dense(chain, det, ps, tm, with_resid=True)
            idx, ptr, _ = orc.csr_structure(chain, det, np.ones(ps.shape[0], bool))
            J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], ps.shape[0]))
            H_ref = (J.T @ J).toarray()
            g_ref = J.T @ r.reshape(-1)
            c_ref = float(np.sum(r * r))
            scale = np.sqrt(np.outer(np.diag(H_ref), np.diag(H_ref)))
        e = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys, dtype=dtype)
        e.set_detections_table(rig.detections[perm])
        if tm is not None:
            e.set_template(tm)
        Hu, g, cost = e.normal_equations(ps, symmetric=False)
        assert np.all(np.tril(Hu, -1) == 0), "only the upper triangle is written"
        Hs = Hu + np.triu(Hu, 1).T
        err = np.max(np.abs(Hs - H_ref) / np.where(scale > 0, scale, 1.0))
        assert err <= tol, (name, err)
        assert np.all(Hs[H_ref == 0] == 0), "structural zeros stay zero"
        assert np.max(np.abs(g - g_ref)) <= tol_r * np.max(np.abs(g_ref)), name
        assert abs(cost - c_ref) <= tol_r * c_ref, name
        H2, g2, c2 = e.normal_equations(ps)           # second call: buffers are re-zeroed
        assert np.allclose(H2, Hs, rtol=1e-9, atol=1e-9 * np.max(np.abs(Hs))) and np.allclose(H2, H2.T)
        e.set_option("normal_rows", 32)               # half-tile LDS images: same matrix
        H3, g3, c3 = e.normal_equations(ps)
        assert np.max(np.abs(H3 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, name
        assert np.max(np.abs(g3 - g_ref)) <= tol_r * np.max(np.abs(g_ref)) and abs(c3 - c_ref) <= tol_r * c_ref, name
        e.set_option("normal_rows", 64)
        e.set_option("normal_sort_tables", 0)         # passes walk the original table through their visiting orders (A/B): same matrix
        H5, g5, c5 = e.normal_equations(ps)
        assert np.max(np.abs(H5 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, name
        assert np.max(np.abs(g5 - g_ref)) <= tol_r * np.max(np.abs(g_ref)) and abs(c5 - c_ref) <= tol_r * c_ref, name
        e.set_option("normal_sort_tables", 1)
        if name == "shuffled":                        # three int32 index arrays instead of the packed word: the sorted copies too
            e6 = Engine(chain, rig.n_cams, rig.n_imgs, rig.n_keys, dtype=dtype)
            e6.set_option("pack_indices", 0)
            e6.set_detections_table(rig.detections[perm])
            if tm is not None:
                e6.set_template(tm)
            H6, g6, c6 = e6.normal_equations(ps)
            assert np.max(np.abs(H6 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, name
            assert np.max(np.abs(g6 - g_ref)) <= tol_r * np.max(np.abs(g_ref)) and abs(c6 - c_ref) <= tol_r * c_ref, name
        if name == "sorted":                          # caller-owned device buffers; H on an odd 8-byte boundary takes the memset prologue
            import torch
            n = ps.shape[0]
            buf = torch.full((n * n + 1,), 7.0, dtype=torch.float64, device="cuda")
            gd = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
            cd = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()                  # the fills run on torch's stream, the build on the engine's own
            for off in (0, 1):
                Hd = buf[off: off + n * n]
                e.normal_equations_device(ps, Hd.data_ptr(), gd.data_ptr(), cd.data_ptr())
                e.synchronize()
                Hu7 = Hd.cpu().numpy().reshape(n, n)
                H7 = Hu7 + np.triu(Hu7, 1).T
                assert np.max(np.abs(H7 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, (name, off)
                assert np.max(np.abs(gd.cpu().numpy() - g_ref)) <= tol_r * np.max(np.abs(g_ref)) and abs(float(cd.cpu()[0]) - c_ref) <= tol_r * c_ref
        if chain == "self":                           # pose-point blocks by the boundary-walking pass (kept for A/B): same matrix
            e.set_option("normal_imgkey_product", 0)
            H4, _, _ = e.normal_equations(ps)
            assert np.max(np.abs(H4 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, name
            e.set_option("normal_imgkey_product", 1)
        # deterministic mode (round 5, csrc/ba_reduce.hpp): no sum in arrival order — the same matrix, and the same BITS on every build,
        # for every table order (a scattered table is walked through sorted copies; "runs-of-7" repeats (camera, image) pairs)
        e.set_option("deterministic", 1)
        builds = [e.normal_equations(ps, symmetric=False) for _ in range(3)]
        assert all(np.array_equal(builds[0][0], b[0]) and np.array_equal(builds[0][1], b[1]) and builds[0][2] == b[2] for b in builds[1:]), name
        Hu8, g8, c8 = builds[0]
        assert np.all(np.tril(Hu8, -1) == 0)
        H8 = Hu8 + np.triu(Hu8, 1).T
        assert np.max(np.abs(H8 - H_ref) / np.where(scale > 0, scale, 1.0)) <= tol, name
        assert np.all(H8[H_ref == 0] == 0), "structural zeros stay zero"
        assert np.max(np.abs(g8 - g_ref)) <= tol_r * np.max(np.abs(g_ref)) and abs(c8 - c_ref) <= tol_r * c_ref, name
        e.set_option("deterministic", 0)
        e.close()


@pytest.mark.parametrize("chain", ["template", "self"])
def test_device_lm_reaches_the_scipy_solution(chain):
    from pycamset_amd.device_solver import JacobianOperator, lm_solve
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    x0 = np.concatenate(parts)
    loss_fn, jac_fn = h.make_loss_fun(1), h.make_loss_jac(1)
    ref = least_squares(loss_fn, x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=30, verbose=0)
    e_ref = np.mean(np.linalg.norm(ref.fun.reshape(-1, 2), axis=1))
    for linear_solver in ("pcg", "cholesky"):   # matrix-free CG / block-reduced J^T J + Cholesky
        res = lm_solve(h, x0.copy(), max_iter=30, linear_solver=linear_solver)
        assert res.history == sorted(res.history, reverse=True), linear_solver        # monotone decrease
        assert res.cost <= ref.cost * (1 + 1e-3), linear_solver                       # at least as low as scipy's trf+lsmr
        assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost   # device cost == residual kernel
        e_dev = np.mean(np.linalg.norm(loss_fn(res.x).reshape(-1, 2), axis=1))
        assert e_dev <= e_ref + 1e-3, linear_solver
    # the operator view agrees with the CSR closure
    op = JacobianOperator(h.op_fun.engine, h._jac_mask())
    ps = h.op_fun.build_param_list(*h.get_bundle_adjustment_inputs(res.x))
    op.linearize(ps)
    Jc = jac_fn(res.x)
    v = np.random.default_rng(0).standard_normal(res.x.shape[0])
    assert np.max(np.abs(op.jtjv(v) - Jc.T @ (Jc @ v))) <= 1e-9 * np.max(np.abs(Jc.T @ (Jc @ v)))
    L = op.as_linear_operator()
    assert L.shape == Jc.shape and np.max(np.abs(L @ v - Jc @ v)) <= 1e-9 * np.max(np.abs(Jc @ v))


def _ring8_small_handler(chain="template"):
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return rig, h, np.concatenate(parts)


def test_device_lm_repeats_a_void_trial_with_the_launch_per_column_solve():
    """The recovery path of the one-launch dense solve inside the LM loop: with a 1 us time limit the persistent
    Cholesky gives up in the first trial (status bit 2 -> stop code 9), the loop drains what it queued behind it, switches the
    solver state to the launch-per-column form and repeats the trial — same message, same cost as a run that used that form from
    the start, and the solver state says so afterwards."""
    from pycamset_amd.device_solver import lm_solve
    _, h, x0 = _ring8_small_handler()
    ref = lm_solve(h, x0.copy(), max_iter=30)
    eng = h.op_fun.engine
    ne = next(iter(eng.__dict__["_blocked_solvers"].values()))
    assert ne.spd_algorithm == "auto"
    eng.set_option("spd_timeout_us", 1)
    try:
        res = lm_solve(h, x0.copy(), max_iter=30)
    finally:
        eng.set_option("spd_timeout_us", 250000)
    assert ne.spd_algorithm == "launches"
    assert res.message == ref.message and res.nit == ref.nit and res.nfev == ref.nfev, (res.message, ref.message, res.nfev, ref.nfev)
    assert abs(res.cost - ref.cost) <= 1e-9 * ref.cost and np.max(np.abs(res.x - ref.x)) <= 1e-7 * np.max(np.abs(ref.x))
    again = lm_solve(h, x0.copy(), max_iter=30)          # the next solve starts with the one-launch form again
    assert ne.spd_algorithm == "auto" and abs(again.cost - ref.cost) <= 1e-9 * ref.cost
    assert lm_solve(h, x0.copy(), max_iter=0).nfev == 1  # max_iter = 0: the start is evaluated and returned, no trial is queued


@pytest.mark.parametrize("chain", ["template", "self"])
def test_device_steered_loop_with_a_stream_ordered_collective(chain):
    """The sharded form of the device-steered loop on ONE rank: ``reduce_fn.on_device`` (what RCCL is) makes lm_solve queue
    pcs_lm_trial_build -> the collective on the solver's stream -> pcs_lm_trial_finish per trial, with the trial built into the
    fixed buffer the collective was queued on and the ranks' void votes summed with the blocks.  The stand-in collective is an
    in-stream operation that leaves the sum of ONE rank unchanged, so the solve must reproduce the single-GPU one — and it must never
    synchronise with the host between build and decision (the calls are counted: one per trial + one for the start)."""
    import torch
    from pycamset_amd.device_solver import lm_solve
    _, h, x0 = _ring8_small_handler(chain)
    one = lm_solve(h, x0.copy(), max_iter=30)
    calls = []

    def in_stream_sum(t):
        calls.append((t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream))
        t.mul_(1.0)                                      # stream-ordered, like dist.all_reduce on the current stream
        return t

    in_stream_sum.on_device = True
    res = lm_solve(h, x0.copy(), max_iter=30, reduce_fn=in_stream_sum)
    assert res.message == one.message and res.nit == one.nit, (res.message, one.message)
    assert abs(res.cost - one.cost) <= 1e-9 * one.cost and np.max(np.abs(res.x - one.x)) <= 1e-7 * np.max(np.abs(one.x))
    eng = h.op_fun.engine
    ne = [v for v in eng.__dict__["_blocked_solvers"].values() if v.reduce_fn is in_stream_sum][0]
    # the start state goes into packed[0]; every trial's collective is queued on packed[1] (a fixed address), on the solver's stream
    assert calls[0][0] == ne.packed[0].data_ptr() and {c[0] for c in calls[1:]} == {ne.packed[1].data_ptr()}
    assert all(c[1] == ne.n_packed + 1 and c[2] == ne.stream.cuda_stream for c in calls)
    assert res.nfev <= len(calls) <= res.nfev + 1        # one per evaluation (+ the speculative trial behind the end)


def _config_handler(number, chain):
    rig = synthetic.config_rig(number)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = {"template": handlers.TemplateBundleHandler, "self": handlers.SelfBundleHandler, "free": handlers.FreePointBundleHandler}[chain]
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel()]
    if chain != "free":
        parts.append(rig.poses[bp.poses_unfixed].ravel())
    if chain != "template":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return rig, h, np.concatenate(parts)


@pytest.mark.parametrize("number,chain", [(3, "template"), (2, "template"), (1, "self"), (1, "free")])
def test_deterministic_mode_repeats_a_solve_bit_for_bit(number, chain):
    """with ``set_option('deterministic', 1)`` no sum of the solve is taken in arrival order — the run-boundary
    flush of the normal equations goes through per-segment partials and an ordered second pass (csrc/ba_reduce.hpp), the K split of
    S -= V V' through a workspace — so two solves of the same problem return the same BITS (the reference's path is deterministic
    for a given thread count: afb:281-288, afb:356-387), and the same cost as the atomics build."""
    from pycamset_amd.device_solver import lm_solve
    _, h, x0 = _config_handler(number, chain)
    plain = lm_solve(h, x0.copy(), max_iter=8)
    eng = h.op_fun.engine
    eng.set_option("deterministic", 1)
    try:
        a = lm_solve(h, x0.copy(), max_iter=8)
        b = lm_solve(h, x0.copy(), max_iter=8)
    finally:
        eng.set_option("deterministic", 0)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.grad, b.grad) and a.cost == b.cost and a.history == b.history and (a.nit, a.nfev) == (b.nit, b.nfev)
    assert abs(a.cost - plain.cost) <= 1e-8 * plain.cost and a.message == plain.message, (a.cost, plain.cost, a.message, plain.message)


# ---- round 3: chains as data (pycamset_amd/chain_compiler.py + csrc/ba_generic.hpp) -------------------------------------
@pytest.mark.parametrize("tag", ["proj_rigid_free", "proj_extr_rigid_template", "proj_template", "proj_rigid_extr_free"])
def test_generated_chains_match_the_reference_code_generator(golden_dir, tag):
    """Compositions that are NOT one of the handlers' three chains (make_golden.py GENERIC_CHAINS: a single camera at the origin
    with a moving scene; two per-image transforms; a bare projection of a posed template; per-image BEFORE per-camera), evaluated
    by the reference's own generated loss / Jacobian (afb:290-419, afb:492-652, mm:147-263).  Through the operator API: the
    chain is compiled into a fused kernel on first use; residual, dense data, masked data and both CSR structures must match."""
    from pycamset_amd import function_blocks as fb
    g = np.load(golden_dir / f"generic_{tag}.npz")
    names = [str(n) for n in g["blocks"]]
    op = getattr(fb, names[0])()
    for n in names[1:]:
        op = op + getattr(fb, n)()
    assert op.chain == "generated"
    det, ps = g["detections"], g["param_str"]
    tm = (g["points"],) if names[-1] == "template_points" else ()
    slabs = [g[f"slab_{i}"] for i in range(len(names))]          # one slab per block, in block order
    assert np.array_equal(op.build_param_list(*slabs), ps)
    r = op.make_full_loss_fn(det, 2)(ps, *tm)
    H.assert_resid_close(r, g["resid"].reshape(r.shape), det[:, 3:])
    data, idx, ptr = op.make_jacobean(det, 2)(ps, *tm)
    P = g["block_param_inds"].shape[1]
    ref = g["data_all"].reshape(-1, P)
    H.assert_jac_close(data.reshape(-1, P), ref)
    assert np.array_equal(idx, g["indices_all"]) and np.array_equal(ptr, g["indptr_all"])
    assert np.array_equal(op.get_block_param_inds(det, 1), g["block_param_inds"])
    dm, idx, ptr = op.make_jacobean(det, 2, unfixed_params=g["unfixed"])(ps, *tm)
    assert np.array_equal(idx, g["indices_masked"]) and np.array_equal(ptr, g["indptr_masked"])
    keep = np.repeat(g["unfixed"][g["block_param_inds"]], 2, axis=0)
    rows = np.broadcast_to(np.max(np.abs(ref), axis=1, keepdims=True), ref.shape)[keep]
    assert np.max(np.abs(dm - g["data_masked"]) / np.maximum(np.abs(g["data_masked"]), H.ROW_FLOOR * rows)) <= H.JAC_RTOL
    assert np.array_equal(dm, data.reshape(-1, P)[keep])          # the masked kernel packs at the store what the dense one writes: same values bit for bit
    # explicit structural entries stay stored, like the reference's CSR (mm:231, mm:237-242)
    d = data.reshape(-1, 2, P)
    assert np.all(d[:, 0, 1] == 1) and np.all(d[:, 1, 3] == 1) and np.all(d[:, 0, 2] == 0) and np.all(d[:, 1, 0] == 0)


def test_generated_chain_options_counts_shared_groups_and_errors():
    """The operator API around generated chains: explicit `counts` (slab sizes beyond max index + 1), two blocks of one class
    sharing ONE parameter group (the reference tells groups apart by object identity, afb:160-163: `rigidTform3d + rigidTform3d`
    applies the same pose twice), the float engines refused, and agreement of a generated chain with its own hand-fused twin
    when the extra transform is the identity."""
    from pycamset_amd import function_blocks as fb
    rig = synthetic.tiny_rig(seed=50, n_cams=3, n_imgs=5, n_keys=8, visibility=0.9)
    det = rig.detections
    # (1) projection + rigidTform3d + rigidTform3d + free_point with ONE pose group: R_p (R_p X + t_p) + t_p
    op = fb.projection() + fb.rigidTform3d() + fb.rigidTform3d() + fb.free_point()
    assert op.chain == "generated"
    ps = op.build_param_list(rig.intr, rig.poses, rig.points)
    r = op.make_full_loss_fn(det, 1)(ps)
    data, idx, ptr = op.make_jacobean(det, 1)(ps)
    cols = op.get_block_param_inds(det, 1)
    assert cols.shape == (det.shape[0], 9 + 6 + 6 + 3) and np.array_equal(cols[:, 9:15], cols[:, 15:21])      # the shared group, twice
    # finite differences of the residual (central, per parameter of detection 0's row) against the analytic columns;
    # the two copies of the shared group each hold the partial derivative through THEIR block, the total is their sum
    J = data.reshape(-1, 2, 24)
    d0 = 0
    for col in (0, 4, 9, 12, 14, 21):
        gi = cols[d0, col]
        h = 1e-6 * max(1.0, abs(ps[gi]))
        pp, pm = ps.copy(), ps.copy()
        pp[gi] += h
        pm[gi] -= h
        fd = (op.make_full_loss_fn(det, 1)(pp)[d0] - op.make_full_loss_fn(det, 1)(pm)[d0]) / (2 * h)
        analytic = J[d0, :, [c for c in range(24) if cols[d0, c] == gi]].sum(axis=0)
        assert np.max(np.abs(fd - analytic)) <= 1e-5 * max(1.0, np.max(np.abs(analytic))), (col, fd, analytic)
    # the dense / blocked normal equations of the chain with the SHARED group: the product of its two local columns belongs to the
    # diagonal entry twice (csrc/ba_blockgram.hpp gram_add); scipy's CSR sums the duplicate column entries of a row the same way
    import torch
    from scipy.sparse import csr_array
    eng1 = op._engine_for(det)
    for dense in (0, 1):
        eng1.set_option("dense_normal", dense)
        lay = eng1.normal_layout()
        nl, nt, tb, n1 = lay["n_lead"], lay["n_trail"], lay["tb"], eng1.n_params
        assert (nt > 0) == (dense == 0)
        ps_dev = torch.from_numpy(np.ascontiguousarray(ps[:n1])).cuda()
        packed = torch.empty(lay["packed_len"], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng1.normal_blocks_device(ps_dev.data_ptr(), packed.data_ptr())
        eng1.synchronize()
        out = packed.cpu().numpy()
        Jc = csr_array((np.asarray(data).ravel(), idx, ptr), shape=(2 * det.shape[0], n1))
        want = (Jc.T @ Jc).toarray()
        A = out[: nl * nl].reshape(nl, nl)
        assert np.max(np.abs(np.triu(A) - np.triu(want[:nl, :nl]))) <= 1e-11 * np.max(np.abs(want))
        if nt:
            assert np.max(np.abs(out[nl * nl: nl * nl + nl * nt].reshape(nl, nt) - want[:nl, nl:])) <= 1e-11 * np.max(np.abs(want))
        assert np.max(np.abs(out[-(n1 + 1): -1] - Jc.T @ r.ravel())) <= 1e-11 * np.max(np.abs(Jc.T @ r.ravel()))
    eng1.set_option("dense_normal", 0)
    assert not eng1.deterministic_supported()                               # two local columns per parameter: the ordered sums refuse the chain
    with pytest.raises(NotImplementedError, match="share a parameter group"):
        eng1.set_option("deterministic", 1)
    # (2) explicit counts: a trailing image and key without detections still get their place in the string
    op2 = fb.optimisation_function([fb.projection(), fb.rigidTform3d(), fb.free_point()], counts=(3, 7, 10))
    eng = op2._engine_for(det)
    assert eng.n_params == 27 + 42 + 30
    ps2 = np.concatenate([rig.intr.ravel(), np.concatenate([rig.poses, np.zeros((2, 6))]).ravel(), np.concatenate([rig.points, np.zeros((2, 3))]).ravel()])
    ps1 = op2.build_param_list(rig.intr, rig.poses, rig.points)
    op1 = fb.projection() + fb.rigidTform3d() + fb.free_point()
    assert np.array_equal(op2.make_full_loss_fn(det, 1)(ps2), op1.make_full_loss_fn(det, 1)(ps1))
    # (3) float outputs (FP64 arithmetic, one rounding at the store) for generated chains too: dense and masked
    r64 = op1.make_full_loss_fn(det, 1)(ps1)
    d64, _, _ = op1.make_jacobean(det, 1)(ps1)
    mask = np.random.default_rng(3).random(ps1.shape[0]) > 0.3
    m64, _, _ = op1.make_jacobean(det, 1, unfixed_params=mask)(ps1)
    for dt, res_tol in (("mixed", None), ("f32", H.F32_RES_ATOL)):
        opf = fb.optimisation_function([fb.projection(), fb.rigidTform3d(), fb.free_point()], dtype=dt)
        rf = opf.make_full_loss_fn(det, 1)(ps1)
        df, _, _ = opf.make_jacobean(det, 1)(ps1)
        mf, _, _ = opf.make_jacobean(det, 1, unfixed_params=mask)(ps1)
        assert rf.dtype == np.float32 and df.dtype == np.float32 and mf.dtype == np.float32
        H.assert_jac_close(df.reshape(-1, 18).astype(np.float64), d64.reshape(-1, 18), rtol=H.MIXED_JAC_RTOL)
        assert np.array_equal(mf, df.reshape(-1, 18)[np.repeat(mask[cols1 := opf.get_block_param_inds(det, 1)], 2, axis=0)])
        assert m64.shape == mf.shape
        if res_tol is None:
            H.assert_resid_close(rf.astype(np.float64), r64, det[:, 3:], rtol=H.MIXED_RES_RTOL)
        else:
            assert np.all(np.abs(rf.astype(np.float64) - r64) <= res_tol + 2.4e-7 * np.abs(r64))   # float measurement + one rounding at the store
    # (4) a generated chain with an identity extra transform = the hand-fused self chain on the same inputs
    op3 = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.free_point()          # hand-fused "self"
    ps3 = op3.build_param_list(rig.intr, rig.extr, rig.poses, rig.points)
    r3 = op3.make_full_loss_fn(det, 1)(ps3)
    # per-image BEFORE per-camera is a different function unless the per-image transform is the identity:
    op4 = fb.projection() + fb.rigidTform3d() + fb.extrinsic3D() + fb.free_point()          # generated
    ps4 = op4.build_param_list(rig.intr, np.zeros_like(rig.poses), rig.extr, rig.points)
    ps5 = op3.build_param_list(rig.intr, rig.extr, np.zeros_like(rig.poses), rig.points)
    assert np.max(np.abs(op4.make_full_loss_fn(det, 1)(ps4) - op3.make_full_loss_fn(det, 1)(ps5))) <= 1e-9
    assert r3.shape == (det.shape[0], 2)


@pytest.mark.parametrize("tag", ["user_cam_scale", "user_division", "user_board_flex"])
def test_user_blocks_match_the_reference_code_generator(golden_dir, tag):
    """The reference's extension point on the GPU (afb:689-775): chains with USER-written blocks — a per-camera isotropic scale
    between `projection` and `extrinsic3D`; a division-model projection REPLACING `projection` — evaluated by the reference's
    own generator from blocks written on its ABC (tests/golden/_user_blocks.py, make_golden.py --only round4), against the same
    blocks declared as device code (function_blocks.device_function_block) and compiled into a fused kernel: residual, dense
    data, masked data (packed at the store), both CSR structures."""
    from pycamset_amd import function_blocks as fb
    g = np.load(golden_dir / f"{tag}.npz")
    ub = H.user_blocks(fb)
    names = [str(n) for n in g["blocks"]]
    op = fb.optimisation_function([ub[n]() if n in ub else getattr(fb, n)() for n in names])
    assert op.chain == "generated"
    det, ps = g["detections"], g["param_str"]
    # template[key] goes to whatever block sits last when that block says template = True (afb:138, afb:374-375): the shipped
    # template_points, or — round 5 — a user source (board_flex: one flex model of the board per image)
    tm = (g["points"],) if op.templated else ()
    assert op.templated == (names[-1] in ("template_points", "board_flex"))
    assert np.array_equal(op.build_param_list(*[g[f"slab_{i}"] for i in range(len(names))]), ps)
    r = op.make_full_loss_fn(det, 2)(ps, *tm)
    H.assert_resid_close(r, g["resid"].reshape(r.shape), det[:, 3:])
    data, idx, ptr = op.make_jacobean(det, 2)(ps, *tm)
    P = g["block_param_inds"].shape[1]
    ref = g["data_all"].reshape(-1, P)
    H.assert_jac_close(data.reshape(-1, P), ref)
    assert np.array_equal(idx, g["indices_all"]) and np.array_equal(ptr, g["indptr_all"])
    assert np.array_equal(op.get_block_param_inds(det, 1), g["block_param_inds"])
    dm, idx, ptr = op.make_jacobean(det, 2, unfixed_params=g["unfixed"])(ps, *tm)
    assert np.array_equal(idx, g["indices_masked"]) and np.array_equal(ptr, g["indptr_masked"])
    keep = np.repeat(g["unfixed"][g["block_param_inds"]], 2, axis=0)
    rows = np.broadcast_to(np.max(np.abs(ref), axis=1, keepdims=True), ref.shape)[keep]
    assert np.max(np.abs(dm - g["data_masked"]) / np.maximum(np.abs(g["data_masked"]), H.ROW_FLOOR * rows)) <= H.JAC_RTOL
    assert np.array_equal(dm, data.reshape(-1, P)[keep])
    # the analytic columns of the user block are the derivative of the residual: central differences through the kernel itself
    cols = g["block_param_inds"]
    J = data.reshape(-1, 2, P)
    loss = op.make_full_loss_fn(det, 2)
    for col in range(P):
        gi = cols[0, col]
        h = 1e-6 * max(1.0, abs(ps[gi]))
        pp, pm = ps.copy(), ps.copy()
        pp[gi] += h
        pm[gi] -= h
        fd = (loss(pp, *tm)[0] - loss(pm, *tm)[0]) / (2 * h)
        analytic = J[0][:, [c for c in range(P) if cols[0, c] == gi]].sum(axis=1)
        assert np.max(np.abs(fd - analytic)) <= 2e-5 * max(1.0, np.max(np.abs(analytic))), (col, fd, analytic)


def test_generated_chain_products_and_device_lm_reach_the_scipy_solution(golden_dir):
    """Row f2 for generated chains: with the dense block rows kept on the device (pcs_genchain_linearize) the products J v,
    J^T u, J^T (J v), diag(J^T J), J^T r (csrc/ba_blockrow.hpp) equal the CSR closure's, and `lm_solve` on
    `projection + extrinsic3D + rigidTform3d + template_points` — not one of the handlers' chains — ends where
    scipy.optimize.least_squares on the same closures ends (optimisation_handling.py:88-98)."""
    from pycamset_amd.device_solver import JacobianOperator, lm_solve
    rig = synthetic.make_rig("gen-lm", 4, 10, synthetic.charuco_points(7, 8.0), seed=61, visibility=0.9)
    det = rig.detections
    rng = np.random.default_rng(5)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()
    assert op.chain == "generated"
    second = np.concatenate([rng.normal(0, 0.02, (rig.n_imgs, 3)), rng.normal(0, 0.002, (rig.n_imgs, 3))], axis=1)   # a small second per-image transform
    # truth: (intr, extr, second, poses); measured = exact projection of the truth + noise; start = truth perturbed
    ps_true = op.build_param_list(rig.intr_true, rig.extr_true, second, rig.poses_true)
    uv = op.make_full_loss_fn(det, 1)(ps_true, rig.points) + det[:, 3:]
    det = det.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + fb.template_points()      # a fresh engine on the new table
    fix_ext = np.ones((rig.n_cams, 6), dtype=bool)
    fix_ext[0] = False                                                   # gauge: camera 0 stays where it is,
    fix_second = np.zeros((rig.n_imgs, 6), dtype=bool)
    fix_second[1:] = True                                                # and so does the first image's second transform (it is redundant with its pose)
    start = [rig.intr_true * (1 + 1e-3 * rng.standard_normal(rig.intr_true.shape)), rig.extr_true + 1e-3 * rng.standard_normal(rig.extr_true.shape),
             second + 1e-3 * rng.standard_normal(second.shape), rig.poses_true + 1e-3 * rng.standard_normal(rig.poses_true.shape)]
    start[1][0] = rig.extr_true[0]
    start[2][0] = second[0]
    prob = handlers.ChainProblem(op, det, start, template=rig.points, unfixed=[None, fix_ext, fix_second, None])
    loss_fn, jac_fn = prob.make_loss_fun(), prob.make_loss_jac()
    # (1) products against the CSR closure
    eng = op._engine_for(det)
    opr = JacobianOperator(eng, prob._jac_mask())
    ps0 = op.build_param_list(*prob.get_bundle_adjustment_inputs(prob.x0))
    op._bind_template(eng, rig.points)
    opr.linearize(ps0)
    Jc = jac_fn(prob.x0)
    r0 = loss_fn(prob.x0)
    v = rng.standard_normal(prob.x0.shape[0])
    u = rng.standard_normal(2 * det.shape[0])
    for got, want in ((opr.jv(v), Jc @ v), (opr.jtu(u), Jc.T @ u), (opr.jtjv(v), Jc.T @ (Jc @ v)), (opr.diag(), np.asarray(Jc.multiply(Jc).sum(axis=0)).ravel()),
                      (opr.grad()[0], Jc.T @ r0)):
        assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
    assert abs(opr.grad()[1] - r0 @ r0) <= 1e-12 * (r0 @ r0)
    # (2) the solve
    ref = least_squares(loss_fn, prob.x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=40)
    res = lm_solve(prob, prob.x0.copy(), max_iter=40)
    # round 5: "auto" is the EXACT step on the chain's dense normal equations, steered by the device (csrc/ba_blockgram.hpp +
    # pcs_genchain_lm_trial): one factorisation per evaluated trial, not conjugate gradients on products with the host in between
    assert res.n_jtjv == res.nfev - 1 and res.nfev <= 12, (res.n_jtjv, res.nfev)
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost <= ref.cost * (1 + 1e-3), (res.cost, ref.cost)
    assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    assert res.cost < 0.05 * res.history[0]
    # deterministic mode for a generated chain: two solves, the same bits
    eng.set_option("deterministic", 1)
    d1 = lm_solve(prob, prob.x0.copy(), max_iter=40)
    d2 = lm_solve(prob, prob.x0.copy(), max_iter=40)
    eng.set_option("deterministic", 0)
    assert np.array_equal(d1.x, d2.x) and d1.cost == d2.cost and (d1.nit, d1.nfev) == (d2.nit, d2.nfev)
    assert abs(d1.cost - res.cost) <= 1e-9 * res.cost
    # ... and the inexact path is still there on request, ending at the same cost
    cg = lm_solve(prob, prob.x0.copy(), max_iter=40, linear_solver="pcg")
    assert cg.n_jtjv > cg.nfev and abs(cg.cost - res.cost) <= 1e-3 * res.cost, (cg.cost, res.cost)


@pytest.mark.parametrize("tag", ["generic_proj_rigid_free", "generic_proj_extr_rigid_template", "generic_proj_template", "generic_proj_rigid_extr_free",
                                 "user_cam_scale", "user_division", "user_board_flex"])
def test_generated_chain_dense_normal_equations_match_the_reference_jacobian(golden_dir, tag):
    """Round 5 (csrc/ba_blockgram.hpp): [J^T J | J^T r | sum r^2] of a generated chain, contracted on the device from its block rows,
    against the SAME products of the reference generator's own CSR Jacobian and residual (the fixtures of make_golden.py) — the four
    shipped compositions and the three chains with user blocks; three of the seven have columns linked to the KEY (free points:
    a different global column per detection), whose products are summed in (camera, key) and (image, key) order (passes 1 and 2 of
    the kernel); six of the seven end in a group that makes trailing entities (blocked form), board_flex stays dense."""
    import torch
    from scipy.sparse import csr_array
    from pycamset_amd import function_blocks as fb
    g = np.load(golden_dir / f"{tag}.npz")
    ub = H.user_blocks(fb)
    names = [str(n) for n in g["blocks"]]
    op = fb.optimisation_function([ub[n]() if n in ub else getattr(fb, n)() for n in names])
    assert op.chain == "generated"
    det, ps = g["detections"], g["param_str"]
    eng = op._engine_for(det)
    if op.templated:
        op._bind_template(eng, g["points"])
    n = eng.n_params
    dev = torch.device("cuda", eng.device)
    ps_dev = torch.from_numpy(np.ascontiguousarray(ps[:n])).to(dev)
    Jc = csr_array((g["data_all"], g["indices_all"], g["indptr_all"]), shape=(2 * det.shape[0], n))
    r = g["resid"].ravel()
    want = (Jc.T @ Jc).toarray()
    assert eng.dense_lm_supported()

    def build_and_check(e):
        """[A | B | C | g | cost] of engine `e` against the reference's products, whatever its layout"""
        lay = e.normal_layout()
        nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
        assert nl + nt == n and lay["packed_len"] == nl * nl + nl * nt + nt * tb + n + 1
        packed = torch.full((lay["packed_len"],), np.nan, dtype=torch.float64, device=dev)      # the build zeroes its output itself
        torch.cuda.synchronize()
        e.normal_blocks_device(ps_dev.data_ptr(), packed.data_ptr())
        e.synchronize()
        out = packed.cpu().numpy()
        A = out[: nl * nl].reshape(nl, nl)
        B = out[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
        C = out[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
        grad, cost = out[-(n + 1): -1], out[-1]
        scale = np.max(np.abs(want))
        assert np.max(np.abs(np.triu(A) - np.triu(want[:nl, :nl]))) <= 1e-11 * scale
        assert np.all(np.tril(A, -1) == 0)                                                    # only the upper triangle is written
        if nt:
            assert np.max(np.abs(B - want[:nl, nl:])) <= 1e-11 * scale
            T = want[nl:, nl:].copy()
            for ent in range(nt // tb):                                                       # the trailing part is block diagonal ...
                blk = T[ent * tb: (ent + 1) * tb, ent * tb: (ent + 1) * tb]
                assert np.max(np.abs(np.triu(C[ent]) - np.triu(blk))) <= 1e-11 * scale and np.all(np.tril(C[ent], -1) == 0)
                blk[:] = 0.0
            assert np.all(T == 0.0)                                                           # ... and nothing else: two entities never share a detection
        assert np.max(np.abs(grad - Jc.T @ r)) <= 1e-11 * np.max(np.abs(Jc.T @ r))
        assert abs(cost - r @ r) <= 1e-12 * (r @ r)
        return out, lay

    out, lay = build_and_check(eng)
    # chains whose LAST parameter group is one rigid transform per image / one point per key get the blocked form (Schur step on the
    # leading part only), everything else — the board-flex source: five parameters per image — the dense one
    blocked = {"generic_proj_rigid_free": 3, "generic_proj_extr_rigid_template": 6, "generic_proj_template": 6, "generic_proj_rigid_extr_free": 3,
               "user_cam_scale": 6, "user_division": 3}
    assert (lay["n_trail"] > 0) == (tag in blocked) and (tag not in blocked or lay["tb"] == blocked[tag])
    if tag in blocked:   # the dense form of the same chain on request
        eng.set_option("dense_normal", 1)
        _, lay_d = build_and_check(eng)
        assert lay_d["n_trail"] == 0 and lay_d["n_lead"] == n
        eng.set_option("dense_normal", 0)
    # ORDERED mode (set_option("deterministic", 1)): the segments' matrices go to a workspace and are added group by group in table
    # order — the same matrix, and the same BITS on every build (the default mode's atomics leave the last bits to the schedule)
    assert eng.deterministic_supported()
    eng.set_option("deterministic", 1)
    od1, _ = build_and_check(eng)
    od2, _ = build_and_check(eng)
    assert np.array_equal(od1, od2)
    assert np.max(np.abs(od1 - out)) <= 1e-12 * np.max(np.abs(out))
    eng.set_option("deterministic", 0)
    key_linked = any(str(b) == "free_point" for b in names)
    assert key_linked == (tag in ("generic_proj_rigid_free", "generic_proj_rigid_extr_free", "user_division"))
    # the rows of the table in ANY order: the host cuts it into segments of one (camera, image) pair wherever they lie (a shuffled table
    # degenerates to short segments), the sums are the same
    perm = np.random.default_rng(3).permutation(det.shape[0])
    op2 = fb.optimisation_function([ub[n_]() if n_ in ub else getattr(fb, n_)() for n_ in names])
    eng2 = op2._engine_for(np.ascontiguousarray(det[perm]))
    if op2.templated:
        op2._bind_template(eng2, g["points"])
    Jc = Jc[np.stack([2 * perm, 2 * perm + 1], axis=1).ravel()]
    r = r.reshape(-1, 2)[perm].ravel()
    out2, _ = build_and_check(eng2)
    assert np.max(np.abs(out2 - out)) <= 1e-11 * np.max(np.abs(out))


def test_templated_user_source_through_the_device_lm(golden_dir):
    """a user block as a TEMPLATED source through `lm_solve` (handlers.ChainProblem): the board-flex model of
    tests/golden/_user_blocks.py — `projection + extrinsic3D + rigidTform3d + board_flex`, template[key] as the source's input —
    ends where scipy.optimize.least_squares on the same closures ends, from a start off the truth; a block that says
    template = True anywhere but last, or with inputs, is refused with the reason."""
    from pycamset_amd import function_blocks as fb
    from pycamset_amd.device_solver import lm_solve
    ub = H.user_blocks(fb)
    rig = synthetic.make_rig("flex-lm", 4, 10, synthetic.charuco_points(7, 8.0), seed=62, visibility=0.9)
    det = rig.detections
    rng = np.random.default_rng(6)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + ub["board_flex"]()
    assert op.chain == "generated" and op.templated
    flex = np.concatenate([rng.uniform(0.98, 1.02, (rig.n_imgs, 2)), rng.normal(0, 1e-3, (rig.n_imgs, 2)), rng.normal(0, 0.3, (rig.n_imgs, 1))], axis=1)
    ps_true = op.build_param_list(rig.intr_true, rig.extr_true, rig.poses_true, flex)
    uv = op.make_full_loss_fn(det, 1)(ps_true, rig.points) + det[:, 3:]
    det = det.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + ub["board_flex"]()
    fix_ext = np.ones((rig.n_cams, 6), dtype=bool)
    fix_ext[0] = False                                                   # gauge: camera 0 stays where it is
    free_flex = np.zeros((rig.n_imgs, 5), dtype=bool)
    free_flex[:, 4] = True                                               # the bend of every image is estimated; scale and shift are redundant with the pose
    start = [rig.intr_true * (1 + 1e-3 * rng.standard_normal(rig.intr_true.shape)), rig.extr_true + 1e-3 * rng.standard_normal(rig.extr_true.shape),
             rig.poses_true + 1e-3 * rng.standard_normal(rig.poses_true.shape), flex.copy()]
    start[1][0] = rig.extr_true[0]
    start[3][:, 4] = 0.0                                                 # a flat board as the first guess
    prob = handlers.ChainProblem(op, det, start, template=rig.points, unfixed=[None, fix_ext, None, free_flex])
    loss_fn, jac_fn = prob.make_loss_fun(), prob.make_loss_jac()
    ref = least_squares(loss_fn, prob.x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=40)
    res = lm_solve(prob, prob.x0.copy(), max_iter=40)
    assert res.n_jtjv == res.nfev - 1                                    # the exact step of round 5 (dense normal equations of the generated chain)
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost <= ref.cost * (1 + 1e-3), (res.cost, ref.cost)
    assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    assert res.cost < 0.05 * res.history[0]
    k_est = prob.get_bundle_adjustment_inputs(res.x)[3][:, 4]
    assert np.max(np.abs(k_est - flex[:, 4])) < 0.15, (k_est, flex[:, 4])            # the bends are recovered from a flat start
    with pytest.raises(NotImplementedError, match="template = True"):
        (fb.projection() + ub["board_flex"]() + fb.free_point()).chain


@pytest.mark.parametrize("n_rigid", [2, 5])
def test_normal_equations_of_a_long_generated_chain_with_three_and_four_column_blocks(n_rigid):
    """Block rows of 34 / 52 columns (+ the residual column: three / four column blocks of 16 — the NB = 3 and NB = 4 instances of
    blockrow_gram_kernel, four waves per workgroup): `projection + cam_scale + extrinsic3D + rigidTform3d x n + template_points` — a
    user block, a SHARED pose group (n local column sets for ONE parameter group: every pair of them meets on the group's diagonal
    block twice) and one more per-image transform — against the products of the chain's own CSR closure (scipy sums the duplicate
    column entries of a row)."""
    import torch
    from scipy.sparse import csr_array
    from pycamset_amd import function_blocks as fb
    ub = H.user_blocks(fb)
    rig = synthetic.make_rig("long-chain", 3, 6, synthetic.charuco_points(5, 8.0), seed=64, visibility=0.9)
    det = rig.detections
    rng = np.random.default_rng(8)
    op = fb.optimisation_function([fb.projection(), ub["cam_scale"](), fb.extrinsic3D()] + [fb.rigidTform3d() for _ in range(n_rigid)] + [fb.template_points()])
    assert op.chain == "generated"
    small = np.concatenate([rng.normal(0, 0.02, (rig.n_imgs, 3)), rng.normal(0, 0.002, (rig.n_imgs, 3))], axis=1) / n_rigid
    ps = op.build_param_list(rig.intr, rng.uniform(0.9, 1.1, (rig.n_cams, 1)), rig.extr, small, rig.poses)
    r = op.make_full_loss_fn(det, 1)(ps, rig.points)
    data, idx, ptr = op.make_jacobean(det, 1)(ps, rig.points)
    eng = op._engine_for(det)
    assert eng.P == 9 + 1 + 6 + 6 * n_rigid + 6 and eng.dense_lm_supported()
    n = eng.n_params
    Jc = csr_array((np.asarray(data).ravel(), idx, ptr), shape=(2 * det.shape[0], n))
    want, gwant = (Jc.T @ Jc).toarray(), Jc.T @ np.asarray(r).ravel()
    for dense in (0, 1):
        eng.set_option("dense_normal", dense)
        lay = eng.normal_layout()
        nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
        assert (nt, tb) == ((6 * rig.n_imgs, 6) if not dense else (0, 3))
        ps_dev = torch.from_numpy(np.ascontiguousarray(ps[:n])).cuda()
        packed = torch.empty(lay["packed_len"], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.normal_blocks_device(ps_dev.data_ptr(), packed.data_ptr())
        eng.synchronize()
        out = packed.cpu().numpy()
        scale = np.max(np.abs(want))
        assert np.max(np.abs(np.triu(out[: nl * nl].reshape(nl, nl)) - np.triu(want[:nl, :nl]))) <= 1e-11 * scale
        if nt:
            assert np.max(np.abs(out[nl * nl: nl * nl + nl * nt].reshape(nl, nt) - want[:nl, nl:])) <= 1e-11 * scale
            C = out[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
            for e in range(nt // tb):
                assert np.max(np.abs(np.triu(C[e]) - np.triu(want[nl + e * tb: nl + (e + 1) * tb, nl + e * tb: nl + (e + 1) * tb]))) <= 1e-11 * scale
        assert np.max(np.abs(out[-(n + 1): -1] - gwant)) <= 1e-11 * np.max(np.abs(gwant))
        assert abs(out[-1] - np.sum(np.asarray(r) ** 2)) <= 1e-12 * np.sum(np.asarray(r) ** 2)
    eng.set_option("dense_normal", 0)


@pytest.mark.parametrize("blocks", [("projection", "extrinsic3D", "rigidTform3d", "template_points"), ("projection", "rigidTform3d", "extrinsic3D", "free_point")])
def test_generated_chain_normal_equations_on_ragged_tables(blocks):
    """The contraction on tables that are NOT the reference's tidy product: 1, 2, 63, 64, 65, 129 and all rows drawn at random from a
    sparse rig (cameras and images without any row, runs of one row), in random order, with explicit counts (trailing entities nobody
    observes keep their empty blocks) — against J'J assembled on the host from the chain's own dense block rows."""
    import torch
    from pycamset_amd import function_blocks as fb
    rig = synthetic.make_rig("ragged", 5, 9, synthetic.charuco_points(6, 8.0), seed=65, visibility=0.5)
    counts = (rig.n_cams + 1, rig.n_imgs + 2, rig.n_keys + 3)                  # one camera, two images, three keys nobody sees
    rng = np.random.default_rng(9)
    small = np.concatenate([rng.normal(0, 0.02, (counts[1], 3)), rng.normal(0, 0.002, (counts[1], 3))], axis=1)
    pad = lambda a, n: np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:])])   # noqa: E731
    intr, extr, poses, pts = pad(rig.intr, counts[0]), pad(rig.extr, counts[0]), pad(rig.poses, counts[1]), pad(rig.points, counts[2])
    intr[-1, :4] = [1000.0, 500.0, 1000.0, 500.0]
    for n_rows in (1, 2, 63, 64, 65, 129, rig.detections.shape[0]):
        rows = rng.choice(rig.detections.shape[0], size=n_rows, replace=False)
        det = np.ascontiguousarray(rig.detections[rows])
        op = fb.optimisation_function([getattr(fb, b)() for b in blocks], counts=counts)
        assert op.chain == "generated"
        slabs = [intr, extr, small, poses] if blocks[-1] == "template_points" else [intr, small, extr, pts]
        ps = op.build_param_list(*slabs)
        tm = (pts,) if op.templated else ()
        r = np.asarray(op.make_full_loss_fn(det, 1)(ps, *tm))
        eng = op._engine_for(det)
        _, j = eng.eval(ps[: eng.n_params], want_resid=False, want_jac=True)
        cols = eng.block_param_inds()
        n = eng.n_params
        Jd = np.zeros((2 * n_rows, n))
        for k in range(cols.shape[1]):                                             # duplicates (none here) would add up
            np.add.at(Jd, (2 * np.arange(n_rows), cols[:, k]), j[0::2, k])
            np.add.at(Jd, (2 * np.arange(n_rows) + 1, cols[:, k]), j[1::2, k])
        want, gwant = Jd.T @ Jd, Jd.T @ r.ravel()
        lay = eng.normal_layout()
        nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
        assert nt == (6 * counts[1] if blocks[-1] == "template_points" else 3 * counts[2])
        ps_dev = torch.from_numpy(np.ascontiguousarray(ps[:n])).cuda()
        packed = torch.full((lay["packed_len"],), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.normal_blocks_device(ps_dev.data_ptr(), packed.data_ptr())
        eng.synchronize()
        out = packed.cpu().numpy()
        scale = max(np.max(np.abs(want)), 1e-300)
        assert np.all(np.isfinite(out))
        assert np.max(np.abs(np.triu(out[: nl * nl].reshape(nl, nl)) - np.triu(want[:nl, :nl]))) <= 1e-11 * scale, n_rows
        assert np.max(np.abs(out[nl * nl: nl * nl + nl * nt].reshape(nl, nt) - want[:nl, nl:])) <= 1e-11 * scale, n_rows
        C = out[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
        for e in range(nt // tb):
            assert np.max(np.abs(np.triu(C[e]) - np.triu(want[nl + e * tb: nl + (e + 1) * tb, nl + e * tb: nl + (e + 1) * tb]))) <= 1e-11 * scale, (n_rows, e)
        assert np.max(np.abs(out[-(n + 1): -1] - gwant)) <= 1e-11 * max(np.max(np.abs(gwant)), 1e-300), n_rows
        assert abs(out[-1] - np.sum(r ** 2)) <= 1e-12 * np.sum(r ** 2), n_rows
        op.engine.close()


def test_user_lens_model_with_free_points_through_the_blocked_device_lm():
    """A generated chain whose LAST group is one point per key: `division_projection + extrinsic3D + rigidTform3d + free_point` — a
    user-written lens model AND free points — takes the blocked normal equations with the points as trailing entities (tb = 3: the
    Schur step of the self / free chains, here fed by csrc/ba_blockgram.hpp's per-detection path for key-linked columns).  Poses held at
    their values (they fix the frame), lens, extrinsics and every point free: `lm_solve` ends where scipy's trf on the same closures
    ends, with one factorisation of the LEADING part per evaluation."""
    from pycamset_amd import function_blocks as fb
    from pycamset_amd.device_solver import lm_solve
    ub = H.user_blocks(fb)
    rig = synthetic.make_rig("div-free", 4, 10, synthetic.charuco_points(7, 8.0), seed=63, visibility=0.9)
    det = rig.detections
    rng = np.random.default_rng(7)

    def chain():
        return ub["division_projection"]() + fb.extrinsic3D() + fb.rigidTform3d() + fb.free_point()

    op = chain()
    assert op.chain == "generated"
    div = np.concatenate([rig.intr_true[:, :4], rng.normal(0, 0.05, (rig.n_cams, 1))], axis=1)      # fx, cx, fy, cy, k
    uv = op.make_full_loss_fn(det, 1)(op.build_param_list(div, rig.extr_true, rig.poses_true, rig.points)) + det[:, 3:]
    det = det.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    op = chain()
    start = [div * (1 + 1e-3 * rng.standard_normal(div.shape)), rig.extr_true + 1e-3 * rng.standard_normal(rig.extr_true.shape),
             rig.poses_true.copy(), rig.points + rng.normal(0, 2e-4, rig.points.shape)]
    prob = handlers.ChainProblem(op, det, start, unfixed=[None, None, np.zeros_like(rig.poses_true, dtype=bool), None])
    eng = op._engine_for(prob._flat_detections())
    lay = eng.normal_layout()
    assert (lay["n_lead"], lay["n_trail"], lay["tb"]) == (rig.n_cams * 11 + rig.n_imgs * 6, 3 * rig.n_keys, 3)
    loss_fn, jac_fn = prob.make_loss_fun(), prob.make_loss_jac()
    ref = least_squares(loss_fn, prob.x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=40)
    res = lm_solve(prob, prob.x0.copy(), max_iter=40)
    assert res.n_jtjv == res.nfev - 1 and res.nfev <= 15, (res.n_jtjv, res.nfev)
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost <= ref.cost * (1 + 1e-3), (res.cost, ref.cost)
    assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    assert res.cost < 0.2 * res.history[0], (res.cost, res.history[0])
    # the reference's caller (optimisation_handling.py:52-117) takes the composed problem like a handler: both solvers, the slabs back
    from pycamset_amd.optimisation_handling import run_bundle_adjustment
    prob_c = handlers.ChainProblem(chain(), det, start, unfixed=[None, None, np.zeros_like(rig.poses_true, dtype=bool), None], options={"max_nfev": 40})
    res_c, slabs_c = run_bundle_adjustment(prob_c, solver="device")
    assert abs(res_c.cost - res.cost) <= 1e-9 * res.cost and len(slabs_c) == 4 and slabs_c[3].shape == rig.points.shape
    assert np.array_equal(slabs_c[2], rig.poses_true)                                  # the held poses come back untouched
    # the SHARDED form of the device-steered loop on one rank, for a generated chain: a stream-ordered stand-in for the collective
    # (reduce_fn.on_device, what RCCL is) — lm_solve switches the ordered contraction on and queues build -> collective -> decision per trial
    import torch
    queued = []

    def in_stream_sum(t):
        queued.append((t.data_ptr(), torch.cuda.current_stream().cuda_stream))
        t.mul_(1.0)
        return t

    in_stream_sum.on_device = True
    prob_s = handlers.ChainProblem(chain(), det, start, unfixed=[None, None, np.zeros_like(rig.poses_true, dtype=bool), None])
    res_s = lm_solve(prob_s, prob_s.x0.copy(), max_iter=40, reduce_fn=in_stream_sum)
    eng_s = prob_s.op_fun._engine_for(prob_s._flat_detections())
    ne_s = [v for v in eng_s.__dict__["_blocked_solvers"].values() if v.reduce_fn is in_stream_sum][0]
    assert abs(res_s.cost - res.cost) <= 1e-9 * res.cost and res_s.nit == res.nit, (res_s.cost, res.cost, res_s.nit, res.nit)
    assert queued[0][0] == ne_s.packed[0].data_ptr() and {q[0] for q in queued[1:]} == {ne_s.packed[1].data_ptr()}
    assert all(q[1] == ne_s.stream.cuda_stream for q in queued) and res_s.nfev <= len(queued) <= res_s.nfev + 1
    assert eng_s.option("deterministic", 0) == 0                                      # switched back after the loop
    # the dense form of the same problem walks to the same cost
    op_d = chain()
    prob_d = handlers.ChainProblem(op_d, det, start, unfixed=[None, None, np.zeros_like(rig.poses_true, dtype=bool), None])
    op_d._engine_for(prob_d._flat_detections()).set_option("dense_normal", 1)
    res_d = lm_solve(prob_d, prob_d.x0.copy(), max_iter=40)
    assert abs(res_d.cost - res.cost) <= 1e-6 * res.cost, (res_d.cost, res.cost)


def test_generated_kernel_for_the_template_chain_against_the_hand_fused_one(capsys):
    """The chain compiler applied to `projection + extrinsic3D + template_points` itself (bypassing the hand-fused fast path):
    same function as ba_eval_kernel on the headline rig (N = 1e6) — values to 1e-12 of the row scale, golden parity on the
    reference fixture — and a kernel time within 1.2 x of the hand-fused kernel's."""
    import torch
    from pycamset_amd import function_blocks as fb
    from pycamset_amd.chain_compiler import ChainEngine
    from pycamset_amd.engine import Engine
    rig = synthetic.config_rig(3)
    ps = orc.build_param_list(rig.intr, rig.extr, rig.poses)
    N = rig.n_det
    gen = ChainEngine([fb.projection(), fb.extrinsic3D(), fb.template_points()], rig.n_cams, rig.n_imgs, rig.n_keys)
    gen.set_detections_table(rig.detections)
    gen.set_template(rig.points)
    hand = Engine("template", rig.n_cams, rig.n_imgs, rig.n_keys)
    hand.set_detections_table(rig.detections)
    hand.set_template(rig.points)
    assert gen.n_params == hand.n_params and gen.P == hand.P
    d_p = torch.from_numpy(ps).cuda()
    bufs = [(torch.empty((N, 2), dtype=torch.float64, device="cuda"), torch.empty((2 * N, 21), dtype=torch.float64, device="cuda")) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    t_gen, t_hand = [], []
    for _ in range(12):   # interleaved
        gen.eval_device(d_p.data_ptr(), bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), stream)
        hand.eval_device_resident(d_p.data_ptr(), bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), stream)
        torch.cuda.synchronize()
        t_gen.append(gen.last_kernel_ms()[1])
        t_hand.append(hand.last_kernel_ms()[1])
    rg, jg = bufs[0][0].cpu().numpy(), bufs[0][1].cpu().numpy()
    rh, jh = bufs[1][0].cpu().numpy(), bufs[1][1].cpu().numpy()
    rows = np.max(np.abs(jh), axis=1, keepdims=True)
    assert np.max(np.abs(jg - jh) / np.maximum(np.abs(jh), H.ROW_FLOOR * rows)) <= 1e-11
    assert np.max(np.abs(rg - rh)) <= 1e-9
    # the step of a generated chain is one launch (round 4); with the slab preparation as a launch of its own: same bits, and the times side by side
    gen.set_one_launch(False)
    t_two = []
    for _ in range(8):
        gen.eval_device(d_p.data_ptr(), bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), stream)
        torch.cuda.synchronize()
        t_two.append(sum(gen.last_kernel_ms()))
    assert np.array_equal(bufs[1][1].cpu().numpy(), jg) and np.array_equal(bufs[1][0].cpu().numpy(), rg)
    one, two, hf = float(np.median(t_gen[2:])), float(np.median(t_two[2:])), float(np.median(t_hand[2:]))
    ratio = min(one, two) / hf
    with capsys.disabled():
        print(f"\n[generated vs hand-fused, chain T, N = {N}] kernel time: generated {one * 1e3:.1f} us in one launch, {two * 1e3:.1f} us in two "
              f"(preparation + evaluation; back to back the one-launch step is the faster one up to 5e5 detections, equal at 1e6: "
              f"profiles/r04/genchain_forms.log), hand-fused {hf * 1e3:.1f} us, ratio of the better form {ratio:.3f}")
    assert ratio <= 1.2 and one / hf <= 1.35
    gen.close()
    hand.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_generated_chain_one_launch_and_two_launch_forms_hold_the_same_bits(dtype):
    """ba_generic.hpp's one-launch step (every wave prepares the slabs of its tile's one or two (camera, image) pairs itself and
    broadcasts them from its lanes) against the form with a slab-preparation launch in front: residual, dense block rows and the
    data packed at the store, bit for bit, two rigid groups.  A table whose tiles hold more than two pairs (a shuffled one) takes
    the two-launch form whatever was asked for."""
    from pycamset_amd import function_blocks as fb
    from pycamset_amd.chain_compiler import ChainEngine
    rig = synthetic.config_rig(1)
    rng = np.random.default_rng(5)
    ps = orc.build_param_list(rig.intr, rig.extr, rig.poses, rig.points)
    blocks = [fb.projection(), fb.extrinsic3D(), fb.rigidTform3d(), fb.free_point()]
    for in_order, det in ((True, rig.detections[: 64 * 100 + 11]), (False, rig.detections[rng.permutation(rig.n_det)][: 64 * 37 + 11])):
        eng = ChainEngine(blocks, rig.n_cams, rig.n_imgs, rig.n_keys, dtype=dtype)
        eng.set_detections_table(det)
        unfixed = rng.random(eng.n_params) < 0.7
        eng.set_unfixed(unfixed)
        out = []
        for one in (True, False):
            eng.set_one_launch(one)
            r, j = eng.eval(ps)
            prep_dense, _ = eng.last_kernel_ms()
            rc, d = eng.eval_compact(ps, want_resid=True)
            prep_packed, _ = eng.last_kernel_ms()
            out.append((r.copy(), j.copy(), rc.copy(), d.copy()))
            # last_kernel_ms reports 0 for the preparation when there was no such launch
            assert (prep_dense == 0.0) == (one and in_order) and (prep_packed == 0.0) == (one and in_order)
        for a, b in zip(*out):
            assert np.array_equal(a, b, equal_nan=True)
        if dtype == "f64":
            ref_j, ref_r = orc.full_jac_dense("self", det, ps, None, with_resid=True)
            H.assert_jac_close(out[0][1], ref_j)
            H.assert_resid_close(out[0][0], ref_r.reshape(out[0][0].shape), det[:, 3:])
        eng.close()


@pytest.mark.parametrize("algorithm", ["one_launch", "launches"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 97, 480, 1003, 1680])
def test_dense_spd_solve_against_numpy(n, algorithm):
    """The reduced system of the Schur step: blocked Cholesky + both substitutions on the device — as ONE persistent launch
    (csrc/ba_chol_persist.hpp) and as one launch per block column (csrc/ba_dense_chol.hpp) — against numpy.linalg.solve, ragged
    sizes included; only the lower triangle may be read; a non-positive pivot is flagged."""
    import torch
    from pycamset_amd.engine import dense_spd_solve, dense_spd_work_len
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 5))
    d = 10.0 ** rng.uniform(-2, 2, n)                                     # badly scaled unknowns (focal lengths next to distortion terms);
    S = (G @ G.T + 1e-3 * np.eye(n)) * np.outer(d, d)                     # a congruence keeps the matrix positive definite
    S = 0.5 * (S + S.T)
    rhs = rng.standard_normal(n)
    x_ref = np.linalg.solve(S, rhs)
    dS = torch.from_numpy(np.tril(S) + np.triu(np.full((n, n), np.nan), 1)).cuda()     # the upper triangle must not be touched
    d_rhs, d_x = torch.from_numpy(rhs).cuda(), torch.empty(n, dtype=torch.float64, device="cuda")
    work = torch.empty(dense_spd_work_len(n), dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    dense_spd_solve(0, n, dS.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream,
                    algorithm=algorithm)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    x = d_x.cpu().numpy()
    # the same accuracy class as LAPACK's own Cholesky solve of this matrix (its condition number reaches 1e10)
    import scipy.linalg as sla
    x_lapack = sla.cho_solve(sla.cho_factor(S, lower=True), rhs)
    tol = max(1e-9, 20 * np.max(np.abs(x_lapack - x_ref)) / np.max(np.abs(x_ref)))
    assert np.max(np.abs(x - x_ref)) <= tol * np.max(np.abs(x_ref)), (np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)), tol)
    L = np.tril(dS.cpu().numpy())
    assert np.max(np.abs(L @ L.T - S) / np.sqrt(np.outer(np.diag(S), np.diag(S)))) <= 1e-12
    assert np.all(np.isnan(dS.cpu().numpy()[np.triu_indices(n, 1)]))
    if n > 1:   # an indefinite matrix: flagged, never an exception or a hang
        bad = S.copy()
        bad[n // 2, n // 2] = -abs(S[n // 2, n // 2])
        dB = torch.from_numpy(bad).cuda()
        dense_spd_solve(0, n, dB.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream,
                        algorithm=algorithm)
        torch.cuda.synchronize()
        assert int(status.item()) & 2 and not int(status.item()) & 4
        # and the same buffers solve the good system again (the flags of a launch are reset by the next one)
        status.zero_()
        dS2 = torch.from_numpy(np.tril(S)).cuda()
        dense_spd_solve(0, n, dS2.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream,
                        algorithm=algorithm)
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and np.max(np.abs(d_x.cpu().numpy() - x_ref)) <= tol * np.max(np.abs(x_ref))


@pytest.mark.parametrize("n", [480, 1680])
def test_one_launch_spd_solve_gives_up_and_drains(n):
    """The persistent Cholesky's escape hatch (csrc/ba_chol_persist.hpp "Safety"): with a time limit of 1 us per wait — no hand-over
    between workgroups is that fast — a workgroup abandons the launch, bit 2 of the status is set, EVERY workgroup leaves at its next
    wait (the call returns: the grid has drained), and the same workspace then solves the system with the default limit."""
    import torch
    from pycamset_amd.engine import dense_spd_solve, dense_spd_work_len
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 5))
    S = G @ G.T + 1e-3 * np.eye(n)
    rhs = rng.standard_normal(n)
    x_ref = np.linalg.solve(S, rhs)
    d_rhs, d_x = torch.from_numpy(rhs).cuda(), torch.empty(n, dtype=torch.float64, device="cuda")
    work = torch.empty(dense_spd_work_len(n), dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    dS = torch.from_numpy(np.tril(S)).cuda()
    dense_spd_solve(0, n, dS.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), stream, algorithm="one_launch", timeout_us=1)
    torch.cuda.synchronize()                                               # returns: no workgroup is left spinning
    assert int(status.item()) & 4, int(status.item())
    status.zero_()
    dS = torch.from_numpy(np.tril(S)).cuda()                               # the abandoned launch has overwritten part of the triangle
    dense_spd_solve(0, n, dS.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), stream, algorithm="one_launch")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    import scipy.linalg as sla
    x_lapack = sla.cho_solve(sla.cho_factor(S, lower=True), rhs)
    tol = max(1e-9, 20 * np.max(np.abs(x_lapack - x_ref)) / np.max(np.abs(x_ref)))
    assert np.max(np.abs(d_x.cpu().numpy() - x_ref)) <= tol * np.max(np.abs(x_ref))
    with pytest.raises(Exception):
        dense_spd_solve(0, n, dS.data_ptr(), n, d_rhs.data_ptr(), d_x.data_ptr(), work.data_ptr(), status.data_ptr(), stream, timeout_us=0)


@pytest.mark.parametrize("n_lead,n_trail", [(480, 1200), (45, 18), (100, 7), (180, 20001), (33, 64), (1, 3), (1100, 257), (1680, 1458)])
def test_schur_syrk_and_vtx_against_numpy(n_lead, n_trail):
    """csrc/ba_schur.hpp: S -= V V' on the lower triangle (the upper one must stay as it was), rhs += V u and w = V' x against
    NumPy — K split into 1 .. 25 parts (partial sums meet in atomics), ragged sizes up to rig-32-self's 1 680 x 1 458, a row stride
    larger than the row."""
    import torch
    from pycamset_amd.engine import schur_syrk, schur_vtx
    rng = np.random.default_rng(n_lead * 7 + n_trail)
    ldv = n_trail + 3
    V = rng.standard_normal((n_lead, ldv))
    S0 = rng.standard_normal((n_lead, n_lead))
    u, rhs0, x = rng.standard_normal(n_trail), rng.standard_normal(n_lead), rng.standard_normal(n_lead)
    dV, dS, du, drhs, dx = (torch.from_numpy(a).cuda() for a in (V, S0.copy(), u, rhs0.copy(), x))
    dw = torch.empty(n_trail, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    schur_syrk(0, n_lead, n_trail, dV.data_ptr(), ldv, dS.data_ptr(), n_lead, du.data_ptr(), drhs.data_ptr(), stream)
    schur_vtx(0, n_lead, n_trail, dV.data_ptr(), ldv, dx.data_ptr(), dw.data_ptr(), stream)
    torch.cuda.synchronize()
    Vr = V[:, :n_trail]
    ref = S0 - Vr @ Vr.T
    got = dS.cpu().numpy()
    scale = np.sqrt(np.outer(np.sum(Vr * Vr, axis=1), np.sum(Vr * Vr, axis=1))) + 1.0
    lo = np.tril_indices(n_lead)
    assert np.max(np.abs(got[lo] - ref[lo]) / scale[lo]) <= 1e-13
    up = np.triu_indices(n_lead, 1)
    assert np.array_equal(got[up], S0[up])
    assert np.max(np.abs(drhs.cpu().numpy() - (rhs0 + Vr @ u))) <= 1e-12 * (1.0 + np.max(np.abs(Vr @ u)))
    assert np.max(np.abs(dw.cpu().numpy() - Vr.T @ x)) <= 1e-12 * (1.0 + np.max(np.abs(Vr.T @ x)))
    # the ORDERED form (engine option "deterministic"): the partial products of the K split go through a workspace and are subtracted
    # split by split — same values, and the same BITS every time
    from pycamset_amd.engine import schur_syrk_work_len
    wl = schur_syrk_work_len(n_lead, n_trail)
    work = torch.empty(max(1, wl), dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(3):
        dS2, drhs2 = torch.from_numpy(S0.copy()).cuda(), torch.from_numpy(rhs0.copy()).cuda()
        schur_syrk(0, n_lead, n_trail, dV.data_ptr(), ldv, dS2.data_ptr(), n_lead, du.data_ptr(), drhs2.data_ptr(), stream, work=work.data_ptr(), work_len=wl)
        torch.cuda.synchronize()
        outs.append((dS2.cpu().numpy(), drhs2.cpu().numpy()))
    assert all(np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1]) for o in outs[1:])
    assert np.max(np.abs(outs[0][0][lo] - ref[lo]) / scale[lo]) <= 1e-13 and np.array_equal(outs[0][0][up], S0[up])
    assert np.max(np.abs(outs[0][1] - (rhs0 + Vr @ u))) <= 1e-12 * (1.0 + np.max(np.abs(Vr @ u)))


def test_free_point_chain_with_2e4_points_solves_through_the_schur_path():
    """Classic free-point bundle adjustment (fph:143) beyond the dense-H limits of round 2 (23 170 parameters in the kernel,
    8 192 before lm_solve fell back to CG): 12 cameras x 2e4 points = 60 180 parameters.  The blocked normal equations store
    A (180 x 180), B (180 x 60 000) and 2e4 3 x 3 blocks — 87 MB instead of a 29 GB dense matrix — and the device LM takes
    exact Schur / Cholesky steps."""
    from pycamset_amd.device_solver import blocked_fits, lm_solve
    rng = np.random.default_rng(41)
    pts = rng.uniform(-0.06, 0.06, (20000, 3))
    rig = synthetic.make_rig("free-2e4", 12, 1, pts, seed=41, visibility=0.6, noise_px=0.3)
    start_pts = pts + rng.normal(0, 5e-4, pts.shape)          # half a millimetre off
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.FreePointBundleHandler(DuckCamset(rig.n_cams), DuckTarget(start_pts), TargetDetection(names, rig.detections),
                                        fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}, "cam_1": {"ext": rig.extr_true[1].copy()}},
                                        options={"verbosity": 0})
    bp = h.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), start_pts.ravel()[bp.bdpt_unfixed]])
    loss_fn = h.make_loss_fun(1)
    eng = h.op_fun.engine
    assert eng.n_params == 15 * 12 + 3 * 20000 and blocked_fits(eng)
    lay = eng.normal_layout()
    assert (lay["n_lead"], lay["n_trail"], lay["tb"]) == (180, 60000, 3)
    res = lm_solve(h, x0.copy(), max_iter=25)              # "auto" -> the Schur / Cholesky step
    assert res.n_jtjv == res.nfev - 1                      # one factorisation per evaluated trial: not the CG path
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost < 0.02 * res.history[0], (res.cost, res.history[0], res.message)
    assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    rms = np.sqrt(2 * res.cost / (2 * rig.n_det))
    assert rms < 0.5, rms                                  # back at the 0.3 px measurement noise


def test_free_point_chain_with_1e6_points_past_the_old_region_limit():
    """Round 5: the blocked build addresses A, B and C with 32-bit offsets in DOUBLES (bytes until round 4: a region ended at 2^29
    doubles and `lm_solve` fell back to Jacobi-CG on matrix-free products, ~150 passes over the table per step — VERDICT r4 item 7).
    12 cameras x 1.05e6 points: B = 180 x 3.15e6 = 5.7e8 doubles (4.5 GB) > 2^29.  The exact Schur / Cholesky step handles it:
    one factorisation per trial, back at the measurement noise in a handful of evaluations."""
    from pycamset_amd.device_solver import blocked_fits, lm_solve
    rng = np.random.default_rng(42)
    pts = rng.uniform(-0.06, 0.06, (1050000, 3))
    rig = synthetic.make_rig("free-1e6", 12, 1, pts, seed=42, visibility=0.35, noise_px=0.3)
    start_pts = pts + rng.normal(0, 5e-4, pts.shape)
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    h = handlers.FreePointBundleHandler(DuckCamset(rig.n_cams), DuckTarget(start_pts), TargetDetection(names, rig.detections),
                                        fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}, "cam_1": {"ext": rig.extr_true[1].copy()}},
                                        options={"verbosity": 0})
    bp = h.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), start_pts.ravel()[bp.bdpt_unfixed]])
    h.make_loss_fun(1)
    eng = h.op_fun.engine
    lay = eng.normal_layout()
    assert lay["n_lead"] * lay["n_trail"] >= 2 ** 29 and blocked_fits(eng), lay
    res = lm_solve(h, x0.copy(), max_iter=8)
    assert res.n_jtjv == res.nfev - 1                      # one factorisation per evaluated trial: not the CG path
    assert res.history == sorted(res.history, reverse=True)
    rms = np.sqrt(2 * res.cost / (2 * rig.n_det))
    assert rms < 0.5, (rms, res.message, res.history)      # back at the 0.3 px measurement noise
    h.op_fun.engine.close()


# ---- legacy residual-only cost -----------------------------------------------------------
def test_legacy_cost_kernel(golden_dir):
    from pycamset_amd import compiled_helpers as hip_ch
    g = np.load(golden_dir / "legacy_cost_medium.npz")
    e = hip_ch.bundle_adjustment_costfn(g["detections"], g["im_points"], g["proj"], g["intrinsics"], g["dists"])
    assert e.shape == g["errors"].shape
    assert np.max(np.abs(e - g["errors"])) <= 1e-10 * 1e3          # 1e-10 relative on ~1e3 px projections
    n = (g["detections"].shape[0] // 3) * 3
    par = hip_ch.bundle_adj_parrallel_solver(g["detections"][:n].reshape(3, n // 3, 5), g["im_points"], g["proj"], g["intrinsics"], g["dists"])
    assert par.shape == g["errors_parallel"].shape and np.max(np.abs(par - g["errors_parallel"])) <= 1e-7
    # full size: agrees with the oracle on a sample and with the chain-T residual kernel everywhere
    from pycamset_amd.engine import Engine
    rig = synthetic.config_rig(3)
    im, P, K, D = orc.legacy_inputs(rig.intr, rig.extr, rig.poses, rig.points)
    eng = Engine("template", rig.n_cams, rig.n_imgs, rig.n_keys)
    eng.set_detections_table(rig.detections)
    eng.set_template(rig.points)
    err = eng.legacy_cost(im, P, K, D)
    prep_ms, k_ms = eng.last_kernel_ms()
    idx = np.arange(0, rig.n_det, 97)
    ref = orc.legacy_cost(rig.detections[idx], im, P, K, D, threads=8)
    assert np.max(np.abs(err.reshape(-1, 2)[idx].reshape(-1) - ref)) <= 1e-9
    r, _ = eng.eval(orc.build_param_list(rig.intr, rig.extr, rig.poses), want_jac=False)
    assert np.max(np.abs(r.reshape(-1) - err)) <= 1e-9
    assert 0 < k_ms < 5
    eng.close()


def test_plain_c_program_through_the_c_abi(tmp_path):
    """examples/c_api_demo.c: a C99 program linked only against libpcs_hip.so must reproduce the
    Python-side numbers (same library, no Python in the loop)."""
    import re
    import subprocess
    from pathlib import Path
    from pycamset_amd.engine import Engine
    repo = Path(__file__).resolve().parent.parent
    exe = tmp_path / "c_api_demo"
    subprocess.run(["gcc", "-std=c99", f"-I{repo / 'include'}", str(repo / "examples" / "c_api_demo.c"), "-o", str(exe),
                    f"-L{repo / 'pycamset_amd'}", "-lpcs_hip", f"-Wl,-rpath,{repo / 'pycamset_amd'}", "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "n_params 42, row length 21" in res.stdout and "CSR nnz (all parameters free) 336" in res.stdout
    vals = [float(x) for x in re.findall(r"detection 0: residual \(([-\d.]+), ([-\d.]+)\), du/dfx ([-\d.]+), dv/dfy ([-\d.]+)", res.stdout)[0]]
    # same toy problem through the Python binding
    C, I, K, N = 2, 2, 4, 8
    det = np.array([[n // 4, (n // 2) % 2, n % 4, 500.0 + 3.0 * n, 480.0 - 2.0 * n] for n in range(N)], dtype=np.float64)
    tmpl = np.array([-0.01, -0.01, 0, 0.01, -0.01, 0, 0.01, 0.01, 0, -0.01, 0.01, 0.002]).reshape(4, 3)
    prm = np.zeros(15 * C + 6 * I)
    for c in range(C):
        prm[9 * c: 9 * c + 9] = [1000, 500, 1000, 500, 0.01, 0.001, 1e-4, -1e-4, 1e-5]
        prm[9 * C + 6 * c: 9 * C + 6 * c + 6] = [0.0, 0.3 * c, 0.0, 0.0, 0.0, 0.2]
    prm[15 * C + 6: 15 * C + 12] = [0.01 * (j + 1) for j in range(6)]
    e = Engine("template", C, I, K)
    e.set_detections_table(det)
    e.set_template(tmpl)
    r, j = e.eval(prm)
    ref = [r[0, 0], r[0, 1], j[0, 0], j[1, 2]]
    assert np.allclose(vals, ref, rtol=0, atol=2e-6)      # the demo prints 6 decimals
    ro = orc.full_loss("template", det, prm, tmpl)
    assert np.max(np.abs(r - ro)) <= 1e-9
    e.close()


@pytest.mark.parametrize("chain", ["template", "self"])
@pytest.mark.parametrize("rig_name", ["ring-8-small", "config-1"])
def test_device_lm_from_far_starts(rig_name, chain):
    """the default damping policy away from the 1 % / 7 px starts every other LM test uses.  Starts: 5 x and 10 x
    the rig's perturbation (35-70 px rms) and the near start with the poses of two images exchanged (30-45 px).  The device loop must
    end at least as low as scipy's least_squares on the same closures (the reference's solver, optimisation_handling.py:88-98)
    within the evaluation budget the table in DESIGN section 4 records (tools/lm_far_start.py prints it)."""
    from pycamset_amd.device_solver import lm_solve
    rig = (synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8) if rig_name == "ring-8-small"
           else synthetic.config_rig(1))
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
    h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, rig.detections),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    loss_fn, jac_fn = h.make_loss_fun(1), h.make_loss_jac(1)
    for kind, scale in (("far", 5.0), ("far10", 10.0), ("swap", 1.0)):
        intr = rig.intr_true + scale * (rig.intr - rig.intr_true)
        extr = rig.extr_true + scale * (rig.extr - rig.extr_true)
        poses = rig.poses_true + scale * (rig.poses - rig.poses_true)
        if kind == "swap":
            poses[[1, 2]] = poses[[2, 1]]
        parts = [intr[bp.intr_unfixed].ravel(), extr[bp.extr_unfixed].ravel(), poses[bp.poses_unfixed].ravel()]
        if chain == "self":
            parts.append(rig.points.ravel()[bp.bdpt_unfixed])
        x0 = np.concatenate(parts)
        px = float(np.sqrt(np.mean(loss_fn(x0) ** 2)))
        assert px > 15.0, (kind, px)                                      # far from the 3-7 px of the other tests' starts
        ref = least_squares(loss_fn, x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=100, verbose=0)
        res = lm_solve(h, x0.copy(), max_iter=60)
        # (70 px away there is more than one valley: both solvers may end in a neighbouring minimum a few per cent apart)
        assert res.cost <= ref.cost * (1.03 if kind == "far10" else 1 + 1e-3), (rig_name, chain, kind, res.cost, ref.cost, res.message)
        assert res.nfev <= 16, (rig_name, chain, kind, res.nfev)           # the table: 6-12 evaluations (round 4's 1e-6: up to 21)
        assert res.history == sorted(res.history, reverse=True)
