"""Shared parameter groups on the device: generated chains whose groups are indexed through a table entity -> group index
(param_type's mod_function / key_type.SINGLE) — evaluation, products, normal equations, the LM solve, covariance, the C ABI.

What the checks rest on (tests/shared_blocks.py): a detection has one camera, one image and one key, so with S the 0/1 matrix that
sends group columns to entity columns the shared Jacobian is J_full S entry for entry — the BLOCK ROWS are the un-shared chain's at the
expanded parameters — and the normal equations are S'(J'J)S, S'J'r, r'r.  J_full and r come from the CPU oracle for the compositions it
knows, from the un-shared generated chain (pinned to the reference's goldens by tests/test_gpu_dropin.py) for the chain with a user block.

Chains (tests/shared_blocks.py chain_blocks):
  (a) projection[SINGLE] + extrinsic3D + template_points           (b) projection[cam -> c // 2] + extrinsic3D + rigidTform3d + free_point
  (c) projection + extrinsic3D + template_points[img -> i % 3]     (d) projection + extrinsic3D + rigidTform3d + face_transform[key -> face]
  (e) projection[SINGLE] + extrinsic3D + rigidTform3d + free_point (SINGLE next to key-linked columns)"""
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.sparse import csr_array

from oracle import ba_oracle as orc
from pycamset_amd import _capi, handlers, synthetic
from pycamset_amd import chain_compiler as cc
from pycamset_amd import function_blocks as fb
from tests import helpers as H
from tests import shared_blocks as sb

pytestmark = pytest.mark.gpu
ORACLE_CHAIN = {"a": "template", "b": "self", "c": "template", "e": "self"}
FACE = 9                                      # ccube_points(4): 6 faces x 9 corners
_cache = {}


def rig_of(which):
    """4 cameras; (a)-(c), (e): 7 images of a 13 x 13 board — 144 keys, so a (camera, image) run is longer than GRAM_SEG = 128 detections
    and always spans several segments of the contraction; (d): 6 images of the 54-key cube."""
    key = "cube" if which.lower() == "d" else "board"
    if key not in _cache:
        if key == "cube":
            _cache[key] = synthetic.make_rig("shared-cube", 4, 6, synthetic.ccube_points(4), seed=71, visibility=0.9)
        else:
            _cache[key] = synthetic.make_rig("shared-board", 4, 7, synthetic.charuco_points(13, 8.0), seed=72, visibility=0.95)
    return _cache[key]


def table_of(which, rig):
    w = which.lower()
    return {"a": None, "e": None, "b": np.array([0, 0, 1, 1]), "c": np.arange(rig.n_imgs) % 3, "d": np.arange(rig.n_keys) // FACE}[w]


def shared_slabs(which, rig, rng):
    """Slabs of the SHARED chain (one row per group) near the rig's evaluation point."""
    w = which.lower()
    if w == "a":
        return [rig.intr[:1], rig.extr, rig.poses]
    if w == "e":
        return [rig.intr[:1], rig.extr, rig.poses, rig.points]
    if w == "b":
        return [rig.intr[[0, 2]], rig.extr, rig.poses, rig.points]
    if w == "c":
        return [rig.intr, rig.extr, rig.poses[:3]]
    faces = np.concatenate([rng.normal(0, 0.02, (6, 3)), rng.normal(0, 0.002, (6, 3))], axis=1)
    return [rig.intr, rig.extr, rig.poses, faces]


def engines(which, rig, det=None, dtype="f64", table="default"):
    """(shared engine, un-shared GENERATED engine of the same composition, src with x_full = x_shared[src], S)"""
    det = rig.detections if det is None else det
    counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
    table = table_of(which, rig) if isinstance(table, str) else table
    eng = cc.ChainEngine(sb.chain_blocks(fb, which, table), *counts, dtype=dtype)
    full = cc.ChainEngine(sb.chain_blocks(fb, which.upper()), *counts, dtype=dtype)
    for e in (eng, full):
        e.set_detections_table(det)
        if e.spec.uses_template:
            e.set_template(rig.points)
    src, S = sb.expansion(eng.spec, counts)
    return eng, full, src, S


def reference(which, rig, det, ps_full, full):
    """(J_full block rows (2N, P), r (N, 2)): the CPU oracle for (a)-(c), (e); the un-shared generated chain for (d)."""
    if which in ORACLE_CHAIN:
        tm = rig.points if ORACLE_CHAIN[which] == "template" else None
        return orc.full_jac_dense(ORACLE_CHAIN[which], det, ps_full, tm, with_resid=True)
    r, j = full.eval(ps_full)
    return j, r


# ---- 1. evaluation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["reference", "shuffled"])
@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
def test_evaluation_is_the_unshared_chain_at_the_expanded_parameters(which, order):
    """Residual and dense block rows against the oracle / the un-shared chain (H.JAC_RTOL) and, against the un-shared GENERATED chain
    on the same device, bit for bit; both launch forms; a table in the reference's order and a shuffled one (no uniform tiles: every
    lane looks its groups up itself); the last tile is partial; the compacted data under a mask that fixes one whole shared group
    and single scalars of the others."""
    rig = rig_of(which)
    rng = np.random.default_rng(11)
    det = rig.detections if order == "reference" else np.ascontiguousarray(rig.detections[rng.permutation(rig.n_det)])
    assert det.shape[0] % 64 != 0 and det.shape[0] > 64
    eng, full, src, S = engines(which, rig, det)
    assert eng.spec.has_maps and not full.spec.has_maps and eng.n_params < full.n_params == src.shape[0]
    ps = np.concatenate([s.ravel() for s in shared_slabs(which, rig, rng)])
    assert ps.shape[0] == eng.n_params
    ps_full = ps[src]
    ref_j, ref_r = reference(which, rig, det, ps_full, full)
    out = {}
    for one in (True, False):
        eng.set_one_launch(one)
        full.set_one_launch(one)
        r, j = eng.eval(ps)
        rf, jf = full.eval(ps_full)
        H.assert_resid_close(r, np.asarray(ref_r).reshape(r.shape), det[:, 3:])
        H.assert_jac_close(j, np.asarray(ref_j).reshape(j.shape))
        assert np.array_equal(r, rf) and np.array_equal(j, jf)              # the same arithmetic on the same numbers
        out[one] = (r, j)
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    # compaction at the store: one whole shared group fixed, single scalars of the rest
    lay = eng.lay
    g0 = next(i for i, t in enumerate(lay["tables"]) if t is not None)
    mask = rng.random(eng.n_params) > 0.15
    mask[lay["starts"][g0]: lay["starts"][g0] + eng.spec.groups[g0]["n_params"]] = False
    cols = eng.block_param_inds()
    assert np.array_equal(cols, src[full.block_param_inds()])
    keep = np.repeat(mask[cols], 2, axis=0)
    for one in (True, False):
        eng.set_one_launch(one)
        nnz = eng.set_unfixed(mask)
        r, data = eng.eval_compact(ps, want_resid=True)
        assert nnz == keep.sum() and np.array_equal(data, out[one][1][keep]) and np.array_equal(r, out[one][0])
    idx, ptr = eng.csr_structure(mask)
    idx_f, ptr_f = full.csr_structure(mask[src])
    assert np.array_equal(ptr, ptr_f) and np.array_equal(np.flatnonzero(mask)[idx], src[np.flatnonzero(mask[src])[idx_f]])
    eng.close(), full.close()


@pytest.mark.parametrize("dtype", ["f32", "mixed"])
def test_evaluation_with_float_outputs(dtype):
    """FP64 arithmetic, one rounding at the store: (a) with float outputs against the oracle at H.F32_JAC_RTOL, both launch forms."""
    rig = rig_of("a")
    eng, full, src, _ = engines("a", rig, dtype=dtype)
    ps = np.concatenate([s.ravel() for s in shared_slabs("a", rig, None)])
    ref_j, ref_r = orc.full_jac_dense("template", rig.detections, ps[src], rig.points, with_resid=True)
    for one in (True, False):
        eng.set_one_launch(one)
        full.set_one_launch(one)
        r, j = eng.eval(ps)
        assert r.dtype == np.float32 and j.dtype == np.float32
        H.assert_jac_close(j.astype(np.float64), np.asarray(ref_j).reshape(j.shape), rtol=H.F32_JAC_RTOL)
        rr = np.asarray(ref_r).reshape(r.shape)
        assert np.all(np.abs(r.astype(np.float64) - rr) <= H.F32_RES_ATOL + 2.4e-7 * np.abs(rr))
        rf, jf = full.eval(ps[src])
        assert np.array_equal(r, rf) and np.array_equal(j, jf)
    eng.close(), full.close()


# ---- problems for the products, the solve and the covariance --------------------------------------------------------------------------
def problem(which, shared=True, seed=5):
    """A ChainProblem built like the existing generated-chain LM test: truth with genuinely shared parameters, measurements = the
    exact projection of the truth + 0.3 px noise, start = truth perturbed by 1e-3, the gauge fixed (camera 0; for (d) face 0 too).
    ``shared=False``: the un-shared chain on the SAME data, started from the expanded start."""
    rig = rig_of(which)
    rng = np.random.default_rng(seed)
    counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
    table = table_of(which, rig)
    if which == "a":
        truth = [rig.intr_true[:1], rig.extr_true, rig.poses_true]
    elif which == "c":
        truth = [rig.intr_true, rig.extr_true, rig.poses_true[:3]]
    else:
        truth = [rig.intr_true, rig.extr_true, rig.poses_true, np.concatenate([rng.normal(0, 0.02, (6, 3)), rng.normal(0, 0.002, (6, 3))], axis=1)]
        truth[3][0] = 0.0
    op = fb.optimisation_function(sb.chain_blocks(fb, which, table), counts=counts)
    uv = op.make_full_loss_fn(rig.detections, 1)(op.build_param_list(*truth), rig.points) + rig.detections[:, 3:]
    det = rig.detections.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    start = [t * (1 + 1e-3 * rng.standard_normal(t.shape)) if i == 0 else t + 1e-3 * rng.standard_normal(t.shape) for i, t in enumerate(truth)]
    start[1][0] = truth[1][0]
    masks = [None, np.ones_like(truth[1], dtype=bool)] + [None] * (len(truth) - 2)
    masks[1][0] = False
    if which == "d":
        start[3][0] = truth[3][0]
        masks[3] = np.ones_like(truth[3], dtype=bool)
        masks[3][0] = False
    if not shared:
        spec = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, which, table), counts=counts)
        tabs = spec.layout(*counts)["tables"]
        start = [s if t is None else s[t] for s, t in zip(start, tabs)]
        masks = [m if (t is None or m is None) else m[t] for m, t in zip(masks, tabs)]
        op = fb.optimisation_function(sb.chain_blocks(fb, which.upper()), counts=counts)
    op = fb.optimisation_function(op.function_blocks, counts=counts)            # a fresh engine on the new table
    return handlers.ChainProblem(op, det, start, template=rig.points, unfixed=masks), rig


# ---- 2. products ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "d"])
def test_products_against_the_csr_closure(which):
    """J v, J'u, J'(J v), diag(J'J) and the gradient (csrc/ba_blockrow.hpp: the gather and the scatter go through the table) against
    the CSR closure; the bound of test_generated_chain_products_and_device_lm_reach_the_scipy_solution: 1e-9 of the largest entry."""
    from pycamset_amd.device_solver import JacobianOperator
    prob, rig = problem(which)
    rng = np.random.default_rng(3)
    op = prob.op_fun
    eng = op._engine_for(prob.det)
    assert eng.spec.has_maps
    opr = JacobianOperator(eng, prob._jac_mask())
    op._bind_template(eng, rig.points)
    opr.linearize(op.build_param_list(*prob.get_bundle_adjustment_inputs(prob.x0)))
    Jc, r0 = prob.make_loss_jac()(prob.x0), prob.make_loss_fun()(prob.x0)
    v, u = rng.standard_normal(prob.x0.shape[0]), rng.standard_normal(2 * prob.det.shape[0])
    for got, want in ((opr.jv(v), Jc @ v), (opr.jtu(u), Jc.T @ u), (opr.jtjv(v), Jc.T @ (Jc @ v)), (opr.diag(), np.asarray(Jc.multiply(Jc).sum(axis=0)).ravel()),
                      (opr.grad()[0], Jc.T @ r0)):
        assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
    assert abs(opr.grad()[1] - r0 @ r0) <= 1e-12 * (r0 @ r0)


# ---- 3. normal equations -------------------------------------------------------------------------------------------------------------
def segment_starts(det, waves):
    """The contraction's cutting rule for the table's own order (pcs_genchain.inc genchain_gram_tables): runs of one (camera, image) pair in
    pieces of at most `cap` detections, `waves` consecutive segments per workgroup -> per camera (first segment, last segment)."""
    n = det.shape[0]
    cap = min(128, max(16, (n // 4096 + 15) // 16 * 16))
    pair = det[:, 0].astype(np.int64) * 100000 + det[:, 1].astype(np.int64)
    cut = np.flatnonzero(np.diff(pair)) + 1
    runs = np.diff(np.concatenate([[0], cut, [n]]))
    cams = det[np.concatenate([[0], cut]), 0].astype(int)
    pieces = (runs + cap - 1) // cap
    first = np.concatenate([[0], np.cumsum(pieces)[:-1]])
    return {c: (int(first[cams == c].min()), int((first + pieces - 1)[cams == c].max())) for c in np.unique(cams)}, int(pieces.max())


def normal_blocks(eng, ps):
    import torch
    lay = eng.normal_layout()
    dev = torch.device("cuda", eng.device)
    ps_dev = torch.from_numpy(np.ascontiguousarray(ps)).to(dev)
    packed = torch.full((lay["packed_len"],), np.nan, dtype=torch.float64, device=dev)      # the build zeroes its output itself
    torch.cuda.synchronize()
    eng.normal_blocks_device(ps_dev.data_ptr(), packed.data_ptr())
    eng.synchronize()
    return packed.cpu().numpy(), lay


def check_normal(out, lay, n, want, want_g, want_cost):
    nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
    assert nl + nt == n and lay["packed_len"] == nl * nl + nl * nt + nt * tb + n + 1
    A = out[: nl * nl].reshape(nl, nl)
    B = out[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
    C = out[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
    grad, cost = out[-(n + 1): -1], out[-1]
    scale = np.max(np.abs(want))
    assert np.max(np.abs(np.triu(A) - np.triu(want[:nl, :nl]))) <= 1e-11 * scale and np.all(np.tril(A, -1) == 0)
    if nt:
        assert np.max(np.abs(B - want[:nl, nl:])) <= 1e-11 * scale
        T = want[nl:, nl:].copy()
        for ent in range(nt // tb):
            blk = T[ent * tb: (ent + 1) * tb, ent * tb: (ent + 1) * tb]
            assert np.max(np.abs(np.triu(C[ent]) - np.triu(blk))) <= 1e-11 * scale and np.all(np.tril(C[ent], -1) == 0)
            blk[:] = 0.0
        assert np.all(T == 0.0)
    assert np.max(np.abs(grad - want_g)) <= 1e-11 * np.max(np.abs(want_g))
    assert abs(cost - want_cost) <= 1e-12 * want_cost
    return A, grad


@pytest.mark.parametrize("which,table", [("a", "default"), ("b", "default"), ("c", "default"), ("d", "default"), ("e", "default"), ("b", np.array([1, 0, 1, 3])),
                                          ("d", "shuffled")])
def test_normal_equations_are_the_contracted_unshared_ones(which, table):
    """[A | B | C | g | cost] (csrc/ba_blockgram.hpp) against S'(J'J)S, S'J'r, r'r with the bounds of
    test_generated_chain_dense_normal_equations_match_the_reference_jacobian (1e-11 of the largest entry, the cost 1e-12), in the
    chain's own form and with dense_normal = 1.  Present, each asserted where it occurs: cameras joined across workgroups ((a), (e): SINGLE),
    cameras joined as neighbouring waves of one workgroup ((a), (b), (e)), (camera, image) runs that span several segments (all),
    key-linked shared columns, so passes 1 and 2 run through the sorted orders ((d)), SINGLE next to key-linked columns ((e)), a group
    that nothing maps to ((b) with cameras -> 1, 0, 1, 3), a face table in no order ((d) shuffled)."""
    rig = rig_of(which)
    rng = np.random.default_rng(13)
    det = rig.detections
    if isinstance(table, str) and table == "shuffled":
        table = rng.permutation(table_of(which, rig))
    eng, full, src, S = engines(which, rig, table=table)
    ps = np.concatenate([s.ravel() for s in shared_slabs(which, rig, rng)])
    if which == "b" and not isinstance(table, str):
        ps = np.concatenate([rig.intr.ravel(), ps[18:]])            # four groups, the third without detections
    assert ps.shape[0] == eng.n_params
    ref_j, ref_r = reference(which, rig, det, ps[src], full)
    cols_full = full.block_param_inds()
    P = eng.P
    ptr = np.arange(0, 2 * det.shape[0] * P + 1, P)
    Jf = csr_array((np.asarray(ref_j).ravel(), np.repeat(cols_full, 2, axis=0).ravel(), ptr), shape=(2 * det.shape[0], full.n_params))
    r = np.asarray(ref_r).ravel()
    Js = csr_array(Jf @ csr_array(S))
    want, want_g = (Js.T @ Js).toarray(), Js.T @ r
    # the shapes the flush must get right
    waves = 16 if P + 1 <= 16 else 8 if P + 1 <= 32 else 4
    seg, longest = segment_starts(det, waves)
    assert longest >= 2                                                                  # a (camera, image) run spans several segments
    if which in ("a", "e"):
        assert len({s[0] // waves for s in seg.values()}) == 4                          # SINGLE joins cameras whose segments sit in different workgroups ...
    if which in ("a", "b", "e"):
        assert seg[1][0] % waves != 0 and seg[0][1] // waves == seg[1][0] // waves      # ... and cameras 0 and 1 as neighbouring waves of one workgroup
    dense_only = which in ("c", "d")
    for dense in ((0,) if dense_only else (0, 1)):
        eng.set_option("dense_normal", dense)
        out, lay = normal_blocks(eng, ps)
        if dense_only:
            assert lay["n_trail"] == 0 and lay["n_lead"] == eng.n_params                  # a shared group is never the trailing group: (c) and (d) are dense
        elif not dense:
            assert lay["n_trail"] > 0 and lay["tb"] == (6 if which == "a" else 3)         # (a), (b), (e) keep the blocked form, shared groups leading
        A, grad = check_normal(out, lay, eng.n_params, want, want_g, float(r @ r))
        if which == "b" and not isinstance(table, str):                                   # the group nothing maps to: rows and columns exactly zero
            empty = slice(18, 27)
            assert np.all(A[empty, :] == 0.0) and np.all(A[:, empty] == 0.0) and np.all(grad[empty] == 0.0) and np.any(A[9:18, 9:18] != 0.0)
    # the ordered sums write every destination from one workgroup: refused, with the reason
    assert not eng.deterministic_supported()
    with pytest.raises(NotImplementedError, match="shared"):
        eng.set_option("deterministic", 1)
    assert _capi.lib().pcs_genchain_set_option(eng._h, b"deterministic", 1) == _capi.PCS_ERR_ARG
    eng.close(), full.close()


def test_identity_tables_build_the_unshared_bits_in_ordered_mode():
    rig = rig_of("b")
    eng, full, src, _ = engines("b", rig, table=np.arange(rig.n_cams))
    assert not eng.spec.has_maps and np.array_equal(src, np.arange(full.n_params)) and eng.deterministic_supported()
    ps = np.concatenate([rig.intr.ravel(), rig.extr.ravel(), rig.poses.ravel(), rig.points.ravel()])
    for e in (eng, full):
        e.set_option("deterministic", 1)
    a, b = normal_blocks(eng, ps)[0], normal_blocks(full, ps)[0]
    assert np.array_equal(a, b)
    eng.close(), full.close()


# ---- 4. the solve --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "c", "d"])
def test_lm_solve_reaches_the_scipy_solution_on_the_reduced_parameters(which):
    """lm_solve against scipy.optimize.least_squares(x_scale="jac") on the CSR closures of the REDUCED parameter vector, with the
    conditions of the existing generated-chain test; the host-steered loop (a host reduce_fn), the stand-in collective
    (reduce_fn.on_device) and linear_solver="pcg" end at the same cost.  (a): the un-shared solve of the same data has 9 n_cams
    intrinsic unknowns and cannot end higher."""
    import torch
    from pycamset_amd.device_solver import lm_solve
    prob, rig = problem(which)
    loss_fn, jac_fn = prob.make_loss_fun(), prob.make_loss_jac()
    ref = least_squares(loss_fn, prob.x0.copy(), jac=jac_fn, x_scale="jac", max_nfev=40)
    res = lm_solve(prob, prob.x0.copy(), max_iter=40)
    assert res.n_jtjv == res.nfev - 1, (res.n_jtjv, res.nfev)                     # the exact step, not conjugate gradients
    assert res.history == sorted(res.history, reverse=True)
    assert res.cost <= ref.cost * (1 + 1e-3), (res.cost, ref.cost)
    assert abs(0.5 * np.sum(loss_fn(res.x) ** 2) - res.cost) <= 1e-9 * res.cost
    host = lm_solve(prob, prob.x0.copy(), max_iter=40, reduce_fn=lambda a: a)
    assert abs(host.cost - res.cost) <= 1e-9 * res.cost, (host.cost, res.cost)

    def in_stream_sum(t):
        t.mul_(1.0)
        return t

    in_stream_sum.on_device = True
    dev = lm_solve(prob, prob.x0.copy(), max_iter=40, reduce_fn=in_stream_sum)
    assert abs(dev.cost - res.cost) <= 1e-9 * res.cost, (dev.cost, res.cost)
    assert prob.op_fun._engine_for(prob.det).option("deterministic", 0) == 0
    cg = lm_solve(prob, prob.x0.copy(), max_iter=40, linear_solver="pcg")
    assert cg.n_jtjv > cg.nfev and abs(cg.cost - res.cost) <= 1e-3 * res.cost, (cg.cost, res.cost)
    if which == "a":
        wide, _ = problem(which, shared=False)
        assert wide.x0.shape[0] == prob.x0.shape[0] + 9 * (rig.n_cams - 1)
        res_w = lm_solve(wide, wide.x0.copy(), max_iter=40)
        assert res_w.cost <= res.cost * (1 + 1e-9), (res_w.cost, res.cost)
    torch.cuda.synchronize()


# ---- 5. covariance -------------------------------------------------------------------------------------------------------------------
def test_covariance_of_the_shared_lens_and_an_unobserved_group():
    """parameter_covariance of (a) against sigma^2 inv(S'J'J S) on the free columns, J from the CPU oracle, with the tolerance of
    tests/test_gpu_covariance.py's generated-chain case; a group that nothing maps to and that the mask leaves free is singular."""
    from pycamset_amd.device_solver import parameter_covariance
    from tests.test_gpu_covariance import _compare, _reference
    prob, rig = problem("a")
    x = prob.x0 * (1 + 1e-4 * np.random.default_rng(1).standard_normal(prob.x0.shape))
    mask = prob._jac_mask()
    eng = prob.op_fun._engine_for(prob.det)
    src, S = sb.expansion(eng.spec, (rig.n_cams, rig.n_imgs, rig.n_keys))
    ps = prob._param_str(x)
    dense, r = orc.full_jac_dense("template", prob.det, ps[src], rig.points, with_resid=True)
    idx, ptr, _ = orc.csr_structure("template", prob.det, np.ones(src.shape[0], bool))
    J = (csr_array((np.asarray(dense).reshape(-1), idx, ptr), shape=(2 * prob.det.shape[0], src.shape[0])) @ csr_array(S)).toarray()
    full, s2, kappa = _reference(J, np.asarray(r).reshape(-1), mask)
    cov = parameter_covariance(prob, x)
    assert abs(cov.sigma2 - s2) <= 1e-9 * s2
    _compare(cov, prob.get_bundle_adjustment_inputs(x), full, mask, kappa, "shared lens")
    assert cov.blocks[0].shape == (1, 9, 9)
    # (b) with cameras -> groups 1, 0, 1, 3: group 2 has no detection
    rig_b = rig_of("b")
    op = fb.optimisation_function(sb.chain_blocks(fb, "b", np.array([1, 0, 1, 3])), counts=(rig_b.n_cams, rig_b.n_imgs, rig_b.n_keys))
    fix_ext = np.ones_like(rig_b.extr, dtype=bool)
    fix_ext[0] = False
    slabs = [rig_b.intr, rig_b.extr, rig_b.poses, rig_b.points]
    free = handlers.ChainProblem(op, rig_b.detections, slabs, unfixed=[None, fix_ext, None, np.zeros_like(rig_b.points, dtype=bool)])
    with pytest.raises(np.linalg.LinAlgError):
        parameter_covariance(free, free.x0)
    held = np.ones_like(rig_b.intr, dtype=bool)
    held[2] = False                                                                # it is the caller's to fix it in the mask
    fixed = handlers.ChainProblem(op, rig_b.detections, slabs, unfixed=[held, fix_ext, None, np.zeros_like(rig_b.points, dtype=bool)])
    cov_b = parameter_covariance(fixed, fixed.x0)
    assert np.all(cov_b.blocks[0][2] == 0.0) and np.all(np.isfinite(cov_b.std))


# ---- 6. the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_set_group_maps_refuses_bad_tables_and_late_calls():
    """pcs_genchain_set_group_maps: PCS_ERR_RANGE / PCS_ERR_ARG with a message for a table value out of range, a wrong table length and
    a call after the first evaluation — and the handle evaluates as before afterwards."""
    lib = _capi.lib()
    rig = rig_of("a")
    counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
    spec = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "a"), counts=counts)
    lay = spec.layout(*counts)
    path = cc.compile_chain(spec)
    h = c_void_p()
    off, cnt = (c_int64 * 2)(*lay["rigid_off"]), (c_int32 * 2)(*lay["rigid_count"])
    _capi.check(lib.pcs_genchain_create(byref(h), str(path).encode(), spec.P, 1, 2, off, cnt, 0, (c_int64 * 1)(0), lay["intr_off"], lay["point_off"], lay["n_params"],
                                        *counts, 0, 0))
    link = (c_int32 * 3)(0, 0, 1)
    n_mapped = (c_int32 * 3)(1, 0, 0)

    def call(table, length=None):
        t = np.ascontiguousarray(table, dtype=np.int32)
        ptrs = (c_void_p * 3)(t.ctypes.data, None, None)
        rc = lib.pcs_genchain_set_group_maps(h, 3, link, ptrs, (c_int64 * 3)(t.shape[0] if length is None else length, 0, 0), n_mapped)
        return rc, (lib.pcs_last_error() or b"").decode()

    rc, msg = call([0, 0, 1, 0])
    assert rc == _capi.PCS_ERR_RANGE and "entity 2 -> group 1" in msg
    rc, msg = call([0, 0, -1, 0])
    assert rc == _capi.PCS_ERR_RANGE and "group -1" in msg
    rc, msg = call([0, 0, 0])
    assert rc == _capi.PCS_ERR_ARG and "3 entries" in msg and "4 entities" in msg
    # the code object reads its table unconditionally: without one the handle refuses to launch
    det = np.ascontiguousarray(rig.detections)
    _capi.check(lib.pcs_genchain_set_detections_table(h, det.ctypes.data_as(POINTER(_capi.c_double)), det.shape[0]))
    pts = np.ascontiguousarray(rig.points)
    _capi.check(lib.pcs_genchain_set_template(h, pts.ctypes.data_as(POINTER(_capi.c_double))))
    ps = np.ascontiguousarray(np.concatenate([s.ravel() for s in shared_slabs("a", rig, None)]))
    r = np.empty((det.shape[0], 2))
    assert lib.pcs_genchain_eval(h, ps.ctypes.data_as(POINTER(_capi.c_double)), c_void_p(r.ctypes.data), None) == _capi.PCS_ERR_STATE
    assert "shared parameter groups" in (lib.pcs_last_error() or b"").decode()
    rc, msg = call([0, 0, 0, 0])
    assert rc == _capi.PCS_OK, msg
    col0 = (c_int32 * 3)(0, 9, 15)
    _capi.check(lib.pcs_genchain_set_blocks(h, 3, col0, (c_int32 * 3)(9, 6, 6), link, (c_int64 * 3)(*lay["starts"])))
    _capi.check(lib.pcs_genchain_eval(h, ps.ctypes.data_as(POINTER(_capi.c_double)), c_void_p(r.ctypes.data), None))
    rc, msg = call([0, 0, 0, 0])
    assert rc == _capi.PCS_ERR_ARG and "evaluated" in msg
    r2 = np.empty_like(r)
    _capi.check(lib.pcs_genchain_eval(h, ps.ctypes.data_as(POINTER(_capi.c_double)), c_void_p(r2.ctypes.data), None))
    eng, full, src, _ = engines("a", rig)
    assert np.array_equal(r, r2) and np.array_equal(r, eng.eval(ps, want_jac=False)[0])
    lib.pcs_genchain_destroy(h)
    eng.close(), full.close()
    # blocks of ONE group (the same first column) go through the same table or through none: a shared group must not slip past the
    # "never the trailing group" rule of the blocked form by carrying its table on one of its blocks only
    h2 = c_void_p()
    _capi.check(lib.pcs_genchain_create(byref(h2), str(path).encode(), spec.P, 1, 2, off, cnt, 0, (c_int64 * 1)(0), lay["intr_off"], lay["point_off"], lay["n_params"],
                                        *counts, 0, 0))
    t = np.zeros(rig.n_cams, dtype=np.int32)
    _capi.check(lib.pcs_genchain_set_group_maps(h2, 3, link, (c_void_p * 3)(t.ctypes.data, None, None), (c_int64 * 3)(t.shape[0], 0, 0), n_mapped))
    rc = lib.pcs_genchain_set_blocks(h2, 3, col0, (c_int32 * 3)(9, 6, 6), (c_int32 * 3)(0, 0, 1), (c_int64 * 3)(0, 0, lay["starts"][2]))
    assert rc == _capi.PCS_ERR_ARG and "only one of them has a table" in (lib.pcs_last_error() or b"").decode()
    lib.pcs_genchain_destroy(h2)


def test_face_transform_passes_its_own_jacobian_check():
    """The worked example calls the library's Rodrigues helpers (pcs::rot_terms / pcs::rot_element) from its device bodies: the block
    check unit (csrc/ba_blockcheck.hpp) offers them like a chain's unit does, and the analytic Jacobian agrees with differences."""
    rep = sb.face_transform(fb).test_self(n_points=256)
    assert isinstance(rep, dict)
