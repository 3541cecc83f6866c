"""The matrix-free J products (csrc/ba_matfree.hpp) at every tile shape the kernel branches on, in both accumulator forms, against the
longdouble reference of tests/matfree_reference.py — entry by entry, within the bound that follows from the suite's own Jacobian and
residual rules.  tests/test_matfree_reference.py proves on the CPU which table reaches which branch and that a branch gone wrong leaves
the bounds by a factor of 1e3 at least.

Every comparison prints ``MATFREE-RATIO <case> <chain> <form> tiles_per_wg=<t> <operator> <error / bound>`` before it asserts: how much
of its bound the honest kernel uses (run with ``-s`` to see the lines)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import matfree_inputs as MI
from tests import matfree_reference as MR
from tests.matfree_reference import CASE_CHAINS, problem

pytestmark = pytest.mark.gpu

TILES_PER_WG = (0, 4, 12)


def make_engine(p, table=None, **options):
    """An engine of the problem's chain and rig shape with ``table`` (default: the problem's) installed, linearised at its string."""
    from pycamset_amd.engine import Engine
    e = Engine(p.chain, *p.case.shape)
    for key, value in options.items():
        e.set_option(key, value)
    e.set_detections_table(p.table if table is None else table)
    if p.template is not None:
        e.set_template(p.template)
    e.linearize(p.ps)
    return e


def run_products(e, p, v=None):
    g, cost = e.grad()
    v = p.v if v is None else v
    return {"jv": e.jv(v), "jtu": e.jtu(p.u), "jtjv": e.jtjv(v), "diag": e.jtj_diag(), "grad": g, "cost": cost}


def check(got, p, form, tpw, ops=MR.OPS + ("cost",), ref=None, bound=None):
    """Every entry of every result within its bound of the reference; entries nothing observed feeds exactly 0.0."""
    ref, bound = p.ref if ref is None else ref, p.bound if bound is None else bound
    for op in ops:
        if op == "cost":
            ratio, k = abs(got[op] - ref[op]) / bound[op], 0
        else:
            assert got[op].shape == ref[op].shape and got[op].dtype == np.float64
            ratio, k = MR.worst_ratio(got[op], ref[op], bound[op])
        print(f"MATFREE-RATIO {p.name} {p.chain} {form} tiles_per_wg={tpw} {op} {ratio:.3e}")
        if ratio > 1.0:
            if op == "jv":
                where = f"row {k} (detection {k // 2}) in tile {k // 128}: {p.tiles[k // 128].label}, {p.tiles[k // 128].n_valid} valid"
            elif op == "cost":
                where = "the cost"
            else:
                where = f"{MI.param_group(p.chain, p.case.shape, k)}, fed by {MI.feeding_tiles(p.J.cols, p.tiles, k) or 'no row'}"
            value = got[op] if op == "cost" else got[op][k]
            expect = ref[op] if op == "cost" else ref[op][k]
            pytest.fail(f"{p.name} / {p.chain} / {form} / tiles_per_wg={tpw} / {op}: error / bound = {ratio:.3e} at {where}: "
                        f"got {value!r}, reference {float(expect)!r}")
        if op in MR.TRANSPOSED:
            assert np.all(got[op][~p.observed] == 0.0), (op, "an unobserved camera, image or key got a contribution")


@pytest.mark.parametrize("name,chain", CASE_CHAINS)
def test_products_match_the_longdouble_reference_entry_by_entry(name, chain):
    """All five products and the cost, LDS accumulators (``matfree_lds`` 1) and wave sums + global atomics (0), ``tiles_per_wg`` 0, 4 and 12.
    The engine rounds the count up to a multiple of 4 (one tile per wave at least) and derives 4 for tables this small, so 0 and 4 give
    the same launch — one tile per wave, a second workgroup from the fifth tile on — and 12 gives three tiles per wave in one workgroup
    (several in the size cases).  One engine per (case, chain) serves the whole option loop."""
    p = problem(name, chain)
    e = make_engine(p)
    try:
        for lds in (1, 0):
            e.set_option("matfree_lds", lds)
            form = "lds" if lds and p.ps.shape[0] <= MI.LDS_PARAM_LIMIT else "global"
            for tpw in TILES_PER_WG:
                e.set_option("tiles_per_wg", tpw)
                check(run_products(e, p), p, form, tpw)
    finally:
        e.close()


THREE_ARRAY_CASES = [(name, MI.CHAINS) for name in ("na-22/image", "na-22/camera", "three-pairs", "aba/image", "aba/camera", "tail-1/new-pair",
                                                   "tail-1/same-pair")]
THREE_ARRAY_CASES += [(f"na-{n}/image", ("free",)) for n in MI.NA_EDGES if n != 22]


@pytest.mark.parametrize("name,chains", THREE_ARRAY_CASES)
def test_products_with_the_three_array_index_form(name, chains):
    """``pack_indices`` 0: camera, image and key in three int32 arrays instead of one packed word per detection.  The free chain's
    image values reach the kernel in this form only (the packed word has no bits for them): an image-only run boundary splits its
    tiles here, so its n_a edges with ONE camera in the tile — both pairs' camera columns are the same entries — run here."""
    for chain in chains:
        p = problem(name, chain)
        e = make_engine(p, pack_indices=0)
        p = SimpleNamespace(**{**vars(p), "tiles": MI.tile_classes(p.table)})     # the failure report's tile classes: image column seen
        try:
            for lds in (1, 0):
                e.set_option("matfree_lds", lds)
                check(run_products(e, p), p, "lds/3-array" if lds else "global/3-array", 0)
        finally:
            e.close()


@pytest.mark.parametrize("name", ["aligned-64", "tail-63", "few-tiles/5", "holes"])
def test_jv_is_bit_repeatable_and_its_two_paths_agree(name):
    """J v has no atomics: two calls return the same bits.  The rows of the table-order table (scalar one- and two-pair forward mode)
    agree with the same rows of a shuffled copy (per-lane slabs, the 2 x P block) within the bound.  The shuffled copy must hold a
    tile on the general path AS THE KERNEL SEES IT: the free chain's packed word carries no image, so with one or two cameras in the
    table its shuffled tiles would all stay scalar — those cases run in the three-array index form, where the images split the tiles."""
    for chain in MI.CASES[name].chains:
        p = problem(name, chain)
        perm = np.random.default_rng(11).permutation(p.table.shape[0])
        shuffled = p.table[perm]
        options = {}
        if chain == "free" and all(t.jv_scalar for t in MI.tile_classes(shuffled, image_column=False)):
            options = {"pack_indices": 0}
        sees_images = chain != "free" or bool(options)
        assert any(t.jv_scalar for t in MI.tile_classes(p.table, sees_images))          # table order: tiles on the scalar paths
        general = [not t.jv_scalar for t in MI.tile_classes(shuffled, sees_images)]
        assert any(general) and (all(general) or chain == "free")
        e, es = make_engine(p, **options), make_engine(p, table=shuffled, **options)
        try:
            a, b, s = e.jv(p.v), e.jv(p.v), es.jv(p.v)
            assert np.array_equal(a, b) and np.array_equal(s, es.jv(p.v))
            rows = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
            check({"jv": a}, p, "jv/table-order", 0, ops=("jv",))
            check({"jv": s}, p, "jv/shuffled", 0, ops=("jv",), ref={"jv": p.ref["jv"][rows]}, bound={"jv": p.bound["jv"][rows]})
            ratio = float(np.max(np.abs(s - a[rows]) / p.bound["jv"][rows]))
            print(f"MATFREE-RATIO {p.name} {p.chain} jv/shuffled-vs-table-order tiles_per_wg=0 jv {ratio:.3e}")
            assert np.all(np.abs(s - a[rows]) <= p.bound["jv"][rows])
        finally:
            e.close()
            es.close()


@pytest.mark.parametrize("chain", MI.CHAINS)
@pytest.mark.parametrize("lds", [1, 0])
def test_one_engine_takes_a_large_a_small_and_the_large_table_again(chain, lds):
    """The engine's input / output vectors grow with the first table and are reused by the second: nothing stale may show."""
    large, small = problem("holes", chain), problem("na-22/image", chain)
    form = "lds/reused" if lds else "global/reused"
    e = make_engine(large, matfree_lds=lds)
    try:
        g, cost = e.grad()
        check({"jtu": e.jtu(large.u), "jv": e.jv(large.v), "grad": g, "cost": cost}, large, form, 0, ops=("jtu", "jv", "grad", "cost"))
        e.set_detections_table(small.table)
        e.linearize(small.ps)
        check(run_products(e, small), small, form, 0)
        e.set_detections_table(large.table)
        e.linearize(large.ps)
        check(run_products(e, large), large, form, 0)
    finally:
        e.close()


@pytest.mark.parametrize("name", MI.SIZE_CASES)
def test_the_accumulator_form_follows_the_parameter_count_on_its_own(name):
    """``matfree_lds`` left alone: 13 740 parameters launch with the full 150 KiB of dynamic LDS, 13 743 take wave sums and global
    atomics without being told to."""
    (chain,) = MI.CASES[name].chains
    p = problem(name, chain)
    e = make_engine(p)
    try:
        check(run_products(e, p), p, "lds/150KiB" if name == "free-lds-edge" else "global/auto", 0)
    finally:
        e.close()


def test_pcg_solve_past_the_lds_limit_reaches_the_cholesky_cost():
    """``lm_solve(linear_solver="pcg")`` with 13 743 parameters — every J^T J v, diagonal and gradient of the solve through the
    LDS_ACC = false kernels — ends where the exact Schur / Cholesky steps end: the two relations of
    test_run_bundle_adjustment_caller_with_both_solvers.  The iterations are capped at 40 (neither solve has met a tolerance by then:
    both creep along flat directions near the noise floor), and the costs are compared after the same number of accepted steps:
    ``history`` gains one entry per accepted step in both loops (asserted)."""
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from pycamset_amd.device_solver import lm_solve
    from tests.test_host_logic import DuckCamset, DuckTarget
    p = problem("free-past-lds", "free")
    rig = p.rig
    start_pts = rig.points + np.random.default_rng(43).normal(0, 5e-4, rig.points.shape)      # half a millimetre off
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    out = {}
    for ls in ("cholesky", "pcg"):
        h = handlers.FreePointBundleHandler(DuckCamset(rig.n_cams), DuckTarget(start_pts), TargetDetection(names, rig.detections),
                                            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}, "cam_1": {"ext": rig.extr_true[1].copy()}},
                                            options={"verbosity": 0})
        bp = h.bundlePrimitive
        x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), start_pts.ravel()[bp.bdpt_unfixed]])
        h.make_loss_fun(1)
        assert h.op_fun.engine.n_params == 13743 > MI.LDS_PARAM_LIMIT
        out[ls] = lm_solve(h, x0.copy(), max_iter=40, linear_solver=ls)
        print(f"MATFREE-SOLVE {ls}: cost {out[ls].cost!r} after {len(out[ls].history) - 1} accepted steps, {out[ls].nfev} evaluations, {out[ls].n_jtjv} "
              f"linear products / factorisations ({out[ls].message})")
        h.op_fun.engine.close()
    assert out["pcg"].n_jtjv > out["pcg"].nfev                 # the CG path: several J^T J v per trial
    assert len(out["pcg"].history) == len(out["cholesky"].history) > 1      # the same number of accepted steps
    assert out["cholesky"].cost <= out["pcg"].cost * (1 + 1e-6)
    assert abs(out["cholesky"].cost - out["pcg"].cost) <= 1e-3 * out["pcg"].cost
    assert np.sqrt(2 * out["pcg"].cost / (2 * rig.n_det)) < 0.5    # at the 0.3 px measurement noise


@pytest.mark.parametrize("chain", MI.CHAINS)
def test_masked_operator_returns_the_free_entries_of_the_unrestricted_products(chain):
    """``JacobianOperator`` with an ``unfixed`` mask on 'three-pairs': J v of the expanded free vector, and the free entries of the
    transposed products, against the reference with the fixed entries of v set to zero."""
    from pycamset_amd.device_solver import JacobianOperator
    p = problem("three-pairs", chain)
    mask = np.random.default_rng(17).random(p.ps.shape[0]) > 0.3
    mask[:9] = False                       # a whole intrinsics block fixed
    vm = np.where(mask, p.v, 0.0)
    ref, bound = MR.products(p.J, p.r, vm, p.u), MR.bounds(p.J, vm, p.u, p.w)
    free = np.flatnonzero(mask)
    for lds in (1, 0):
        e = make_engine(p, matfree_lds=lds)
        try:
            op = JacobianOperator(e, mask)
            assert op.n_free == free.shape[0]
            g, cost = op.grad()
            got = {"jv": op.jv(p.v[free]), "jtu": op.jtu(p.u), "jtjv": op.jtjv(p.v[free]), "diag": op.diag(), "grad": g, "cost": cost}
            for k in MR.OPS:
                assert got[k].shape == ((2 * p.table.shape[0],) if k == "jv" else free.shape)
                sel = slice(None) if k == "jv" else free
                ratio, _ = MR.worst_ratio(got[k], ref[k][sel], bound[k][sel])
                print(f"MATFREE-RATIO {p.name} {chain} {'lds' if lds else 'global'}/masked tiles_per_wg=0 {k} {ratio:.3e}")
                assert ratio <= 1.0, (k, ratio)
            assert abs(cost - ref["cost"]) <= bound["cost"]
        finally:
            e.close()
