"""User blocks with Python bodies on the MI355X: the chains built from them match the reference's generator and their hand-translated
device twins, a Levenberg-Marquardt solve does not tell them apart, and ``test_self`` passes for both kinds and catches corrupted
Jacobians by (output row, column)."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import chain_compiler as cc
from pycamset_amd import function_blocks as fb
from pycamset_amd import handlers, synthetic
from tests import helpers as H
from tests import python_blocks as PB

pytestmark = pytest.mark.gpu

BLOCKS = ["cam_scale", "division_projection", "board_flex"]


@pytest.mark.parametrize("tag", ["user_cam_scale", "user_division", "user_board_flex"])
def test_python_bodied_chains_match_the_reference_generator_and_the_twins(golden_dir, tag):
    g = np.load(golden_dir / f"{tag}.npz")
    names = [str(n) for n in g["blocks"]]
    op = fb.optimisation_function(PB.chain_of(names))
    twin = fb.optimisation_function(PB.chain_of(names, H.user_blocks(fb)))
    assert op.chain == "generated" and op._engine is None
    det, ps = g["detections"], g["param_str"]
    tm = (g["points"],) if op.templated else ()
    r = op.make_full_loss_fn(det, 2)(ps, *tm)
    H.assert_resid_close(r, g["resid"].reshape(r.shape), det[:, 3:])
    data, idx, ptr = op.make_jacobean(det, 2)(ps, *tm)
    P = g["block_param_inds"].shape[1]
    ref = g["data_all"].reshape(-1, P)
    H.assert_jac_close(data.reshape(-1, P), ref)
    assert np.array_equal(idx, g["indices_all"]) and np.array_equal(ptr, g["indptr_all"])
    dm, idx, ptr = op.make_jacobean(det, 2, unfixed_params=g["unfixed"])(ps, *tm)
    assert np.array_equal(idx, g["indices_masked"]) and np.array_equal(ptr, g["indptr_masked"])
    keep = np.repeat(g["unfixed"][g["block_param_inds"]], 2, axis=0)
    rows = np.broadcast_to(np.max(np.abs(ref), axis=1, keepdims=True), ref.shape)[keep]
    assert np.max(np.abs(dm - g["data_masked"]) / np.maximum(np.abs(g["data_masked"]), H.ROW_FLOOR * rows)) <= H.JAC_RTOL
    # the hand-translated twin: the same function to 1e-14 of the row scale (the kernels compile to the same instructions: bitwise)
    rt = twin.make_full_loss_fn(det, 2)(ps, *tm)
    dt, _, _ = twin.make_jacobean(det, 2)(ps, *tm)
    d, t = data.reshape(-1, P), dt.reshape(-1, P)
    assert np.max(np.abs(r - rt) / np.maximum(1.0, np.abs(rt))) <= 1e-14
    assert np.max(np.abs(d - t) / np.maximum(1.0, np.max(np.abs(t), axis=1, keepdims=True))) <= 1e-14
    print(f"{tag}: residual bitwise equal to the twin: {np.array_equal(r, rt)}, Jacobian bitwise equal: {np.array_equal(d, t)}")


def _division_problem(blocks):
    rig = synthetic.make_rig("py-lm", 4, 12, synthetic.charuco_points(7, 8.0), seed=23, visibility=0.9)
    rng = np.random.default_rng(4)
    div = np.concatenate([rig.intr_true[:, :4], rng.normal(0, 0.05, (rig.n_cams, 1))], axis=1)
    truth = [div, rig.extr_true, rig.poses_true]
    start = [div * (1 + 1e-3 * rng.standard_normal(div.shape)), rig.extr_true + 1e-3 * rng.standard_normal(rig.extr_true.shape),
             rig.poses_true + 1e-3 * rng.standard_normal(rig.poses_true.shape)]
    start[1][0] = rig.extr_true[0]
    fix_ext = np.ones((rig.n_cams, 6), dtype=bool)
    fix_ext[0] = False
    det = rig.detections.copy()
    op = fb.optimisation_function(PB.chain_of(["division_projection", "extrinsic3D", "template_points"], blocks))
    uv = op.make_full_loss_fn(det, 1)(op.build_param_list(*truth), rig.points) + det[:, 3:]
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    op = fb.optimisation_function(PB.chain_of(["division_projection", "extrinsic3D", "template_points"], blocks))
    return handlers.ChainProblem(op, det, start, template=rig.points, unfixed=[None, fix_ext, None])


def test_lm_solve_does_not_tell_the_python_block_from_its_twin():
    from pycamset_amd.device_solver import lm_solve

    res = {}
    for kind, blocks in (("python", PB.python_blocks()), ("twin", H.user_blocks(fb))):
        prob = _division_problem(blocks)
        res[kind] = lm_solve(prob, prob.x0.copy(), max_iter=40)
    a, b = res["python"], res["twin"]
    assert a.nfev == b.nfev and a.message == b.message, (a.nfev, b.nfev, a.message, b.message)
    assert np.max(np.abs(a.x - b.x)) <= 1e-10
    assert np.isfinite(a.cost) and abs(a.cost - b.cost) <= 1e-12 * b.cost
    print(f"python-bodied: {a.nfev} evaluations, cost {a.cost:.9e}, {a.message}; bitwise equal x: {np.array_equal(a.x, b.x)}")


@pytest.mark.parametrize("kind", ["python", "twin"])
@pytest.mark.parametrize("name", BLOCKS)
def test_test_self_passes_for_python_and_device_string_blocks(kind, name):
    blk = (PB.python_blocks() if kind == "python" else H.user_blocks(fb))[name]()
    rep = blk.test_self()
    assert rep["n_points"] == 1025
    nc = blk.params.n_params + blk.num_inp
    assert rep["max_error"].shape == (nc,) and rep["worst_ratio"] <= 1.0
    assert (rep["python_max_rel"] is not None) == (kind == "python")
    if kind == "python":
        assert rep["python_max_rel"] <= 1e-12
    # the caller's points: (M, NP) parameters, (M, NIN) inputs (a templated source: the template points)
    rng = np.random.default_rng(1)
    nin = 3
    rep = blk.test_self(rng.uniform(0.8, 1.2, (7, blk.params.n_params)), rng.uniform(0.8, 1.2, (7, nin)))
    assert rep["n_points"] == 7


def _corrupt(name, old, new):
    base = H.user_blocks(fb)[name]
    assert old in base.device_jac, old
    return type(f"{name}_corrupt", (base,), {"device_jac": base.device_jac.replace(old, new)})


CORRUPTIONS = {
    # flipped sign: d u / d fx
    "flipped_sign": ("division_projection", "out[0] = x * d;", "out[0] = -x * d;", {(0, 0)}),
    # two swapped columns: d u / d X and d u / d Y
    "swapped_columns": ("division_projection", "out[5] = ux * iz; out[6] = uy * iz;", "out[5] = uy * iz; out[6] = ux * iz;", {(0, 5), (0, 6)}),
    # a dropped term: d v / d lam loses -fy y r2 d2
    "dropped_term": ("division_projection", "out[8 + 4] = -params[2] * y * r2 * d2;", "out[8 + 4] = 0.0;", {(1, 4)}),
    # a zeroed column of the templated source: d Z / d k
    "zeroed_template_column": ("board_flex", "out[10 + 4] = inp[0] * inp[0] + inp[1] * inp[1];", "out[10 + 4] = 0.0;", {(2, 4)}),
}


@pytest.mark.parametrize("case", sorted(CORRUPTIONS))
def test_test_self_names_the_corrupted_entry(case):
    name, old, new, where = CORRUPTIONS[case]
    blk = _corrupt(name, old, new)()
    with pytest.raises(AssertionError) as e:
        blk.test_self()
    msg = str(e.value)
    assert any(f"output row {o}, column {c}" in msg for o, c in where), msg


def test_block_check_refuses_a_code_object_of_another_shape():
    info = cc.user_block_info(PB.python_blocks()["division_projection"]())
    path = cc.compile_blockcheck(info)
    pts = np.ones((2, 8))
    f, j, d = np.empty(2 * 3), np.empty(2 * 3 * 8), np.empty(2 * 3 * 8)     # sized for the shape asked for (np 5, nin 3, nout 3)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = _capi.lib().pcs_blockcheck(str(path).encode(), 0, 5, 3, 3, 0, pts.ctypes.data_as(dp), 2, f.ctypes.data_as(dp), j.ctypes.data_as(dp), d.ctypes.data_as(dp))
    assert rc == _capi.PCS_ERR_ARG and b"shape" in _capi.lib().pcs_last_error()
