"""Shared parameter groups on the host: param_type's mod_function / key_type.SINGLE, the layout and index tables of generated
chains that go through a table entity -> group index, and the slabs of ChainProblem (no GPU needed).

The reference declares both (abstract_function_blocks.py:42-61) and builds neither (`#TODO account for the mod function here`,
afb:803); the layout rule here is its own with the TODO filled in: a group takes n_params x (largest group index + 1) columns."""
import numpy as np
import pytest

from pycamset_amd import chain_compiler as cc
from pycamset_amd import function_blocks as fb
from pycamset_amd import handlers
from tests import shared_blocks as sb

K = fb.key_type


class JitLike:
    """What a numba-jitted function looks like to the table builder: not to be called, its Python body under .py_func."""

    def __init__(self, f):
        self.py_func = f

    def __call__(self, *a):
        raise AssertionError("the dispatcher itself is never called: the table is built from .py_func on the host")


def test_param_type_validation_and_single():
    assert fb.param_type(K.SINGLE, 9).group_table(4).tolist() == [0, 0, 0, 0]
    assert fb.param_type(K.PER_CAM, 9).group_table(4) is None
    with pytest.raises(ValueError, match="SINGLE"):
        fb.param_type(K.SINGLE, 9, lambda i: 0)
    with pytest.raises(ValueError, match="callable int -> int or a one-dimensional integer array"):
        fb.param_type(K.PER_CAM, 9, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="block lens.*negative"):
        fb.param_type(K.PER_CAM, 9, lambda i: i - 1).group_table(3, "lens")
    with pytest.raises(ValueError, match="block lens.*non-integer"):
        fb.param_type(K.PER_CAM, 9, lambda i: i / 2).group_table(3, "lens")
    with pytest.raises(ValueError, match="block lens.*2 entries.*3 entities"):
        fb.param_type(K.PER_CAM, 9, np.array([0, 0])).group_table(3, "lens")
    # a table longer than the entity count is cut; one that sends every entity to itself is no table at all
    assert fb.param_type(K.PER_IMG, 6, np.array([0, 1, 0, 1, 5])).group_table(4).tolist() == [0, 1, 0, 1]
    assert fb.param_type(K.PER_IMG, 6, np.arange(9)).group_table(4) is None
    assert fb.param_type(K.PER_IMG, 6, lambda i: i).group_table(4) is None
    # the refusals of the generator name the block
    blocks = sb.chain_blocks(fb, "c", lambda i: -1)
    with pytest.raises(NotImplementedError, match="template_points.*negative"):
        cc.ChainSpec.from_blocks(blocks, counts=(2, 3, 4))
    bad = sb.with_params(fb.projection(), fb.param_type(K.SINGLE, 9))
    bad.params.mod_function = lambda i: 0          # set behind the constructor's back
    with pytest.raises(NotImplementedError, match="projection.*SINGLE together with a mod_function"):
        cc.ChainSpec.from_blocks([bad, fb.extrinsic3D(), fb.template_points()])
    # a key-linked built-in rigid group is still refused, and the message says what to write instead
    with pytest.raises(NotImplementedError, match="user block"):
        cc.ChainSpec.from_blocks([fb.projection(), sb.with_params(fb.template_points(), fb.param_type(K.PER_KEY, 6, lambda k: k // 9))])


def test_callable_jitted_and_array_give_the_same_table():
    want = np.arange(10) % 3
    tabs = [fb.param_type(K.PER_IMG, 6, m).group_table(10) for m in (lambda i: i % 3, JitLike(lambda i: i % 3), want, want.astype(np.uint8), np.asarray(want.tolist()))]
    for t in tabs:
        assert t.dtype == np.int32 and np.array_equal(t, want)
    specs = [cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "c", m), counts=(4, 10, 16)) for m in (lambda i: i % 3, JitLike(lambda i: i % 3), want)]
    lays = [s.layout(4, 10, 16) for s in specs]
    assert all(l["n_params"] == 36 + 24 + 18 and np.array_equal(l["tables"][2], want) and l["tables"][0] is None for l in lays)
    assert len({cc.emit_source(s) for s in specs}) == 1            # the tables are run-time data: one code object for all of them
    assert cc.code_object_path(specs[0]) == cc.code_object_path(cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "c", lambda i: i // 2), counts=(4, 10, 16)))


def test_a_mod_function_is_evaluated_once_per_engine():
    calls = []

    def turntable(i):
        calls.append(i)
        return i % 3

    spec = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "c", turntable), counts=(4, 10, 16))
    for _ in range(3):
        lay = spec.layout(4, 10, 16)
        cc.block_param_inds(spec, lay, np.zeros((5, 3), dtype=np.int64))
    assert calls == list(range(10)) and lay["tables"][2].tolist() == [i % 3 for i in range(10)]


def test_identity_table_is_the_unmapped_chain():
    plain = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "C"))
    for table in (np.arange(10), lambda i: i, np.arange(30)):
        spec = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "c", table), counts=(4, 10, 16))
        assert not spec.has_maps and spec.groups == plain.groups
        assert cc.emit_source(spec) == cc.emit_source(plain) and cc.code_object_path(spec) == cc.code_object_path(plain)
        assert spec.layout(4, 10, 16)["tables"] == [None, None, None]
    mapped = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "c", lambda i: i % 3), counts=(4, 10, 16))
    assert mapped.has_maps and cc.code_object_path(mapped) != cc.code_object_path(plain)
    assert "c.slab_m(1, pcs::LINK_IMG)" in cc.emit_source(mapped) and "_m(" not in cc.emit_source(plain)
    # SINGLE is a camera-linked group whose table is all zeros; extrinsics stay per camera: the maps are per GROUP, not per link type
    single = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, "a"), counts=(4, 10, 16))
    assert [g["mapped"] for g in single.groups] == [True, False, False] and single.groups[0]["link"] == cc.LINK_CAM
    assert "c.intr_m()" in cc.emit_source(single) and "c.slab(0, pcs::LINK_CAM)" in cc.emit_source(single)
    lay = single.layout(4, 10, 16)
    assert lay["n_params"] == 9 + 24 + 60 and lay["tables"][0].tolist() == [0, 0, 0, 0] and lay["group_count"] == [1, 4, 10]
    # sharing one param_type OBJECT between blocks keeps its meaning (afb:160-163): one group, one table
    pose = fb.param_type(K.PER_IMG, 6, lambda i: i % 3)
    two = cc.ChainSpec.from_blocks([fb.projection(), sb.with_params(fb.rigidTform3d(), pose), sb.with_params(fb.template_points(), pose)], counts=(4, 10, 16))
    assert two.group_of_block == (0, 1, 1) and two.layout(4, 10, 16)["n_params"] == 36 + 18
    # shipped blocks in the order of a hand-fused chain run as a generated chain when they share parameters
    assert fb.optimisation_function(sb.chain_blocks(fb, "a")).chain == "generated" and fb.optimisation_function(sb.chain_blocks(fb, "A")).chain == "template"


@pytest.mark.parametrize("which,table", [("a", None), ("b", [0, 0, 1, 1]), ("b", [1, 0, 1, 3]), ("c", [0, 1, 2, 0, 1, 2, 0]), ("d", np.arange(54) // 9),
                                          ("d", np.random.default_rng(2).permutation(np.arange(54) // 9)), ("e", None)])
def test_layout_index_rows_and_csr_structure_against_the_expansion_matrix(which, table):
    """block_param_inds and csr_structure_of of a shared chain = S applied to the un-shared chain's tables, fixed columns included."""
    counts = (4, 7, 54)
    rng = np.random.default_rng(7)
    n = 300
    det = np.stack([rng.integers(0, counts[0], n), rng.integers(0, counts[1], n), rng.integers(0, counts[2], n)], axis=1)
    table = None if table is None else np.asarray(table)
    spec = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, which, table), counts=counts)
    full = cc.ChainSpec.from_blocks(sb.chain_blocks(fb, which.upper()), counts=counts)
    assert spec.has_maps and not full.has_maps and spec.P == full.P
    lay, lay_full = spec.layout(*counts), full.layout(*counts)
    src, S = sb.expansion(spec, counts)
    assert src.shape[0] == lay_full["n_params"] and S.shape == (lay_full["n_params"], lay["n_params"])
    n_groups = [int(t.max()) + 1 for t in lay["tables"] if t is not None]
    assert lay["n_params"] == lay_full["n_params"] - sum(g["n_params"] * (counts[g["link"]] - (int(t.max()) + 1))
                                                         for g, t in zip(spec.groups, lay["tables"]) if t is not None) and n_groups
    cols, cols_full = cc.block_param_inds(spec, lay, det), cc.block_param_inds(full, lay_full, det)
    assert np.array_equal(cols, src[cols_full])                                   # entry for entry: no sums inside a row
    # a mask that fixes one whole shared group and single scalars elsewhere; the CSR structure is the expanded one's, renumbered
    mask = rng.random(lay["n_params"]) > 0.2
    g0 = next(i for i, t in enumerate(lay["tables"]) if t is not None)
    mask[lay["starts"][g0]: lay["starts"][g0] + spec.groups[g0]["n_params"]] = False
    idx, ptr, keep, off = cc.csr_structure_of(cols, lay["n_params"], mask)
    idx_f, ptr_f, keep_f, off_f = cc.csr_structure_of(cols_full, lay_full["n_params"], mask[src])
    assert np.array_equal(ptr, ptr_f) and np.array_equal(keep, keep_f) and np.array_equal(off, off_f)
    free = np.flatnonzero(mask)
    free_full = np.flatnonzero(mask[src])
    assert np.array_equal(free[idx], src[free_full[idx_f]])


def test_chain_problem_takes_group_slabs():
    """A shared group's slab is (n_groups, n_params), its mask has the same shape, and x <-> slabs round-trips."""
    counts = (4, 6, 16)
    rng = np.random.default_rng(3)
    det = np.concatenate([np.stack([rng.integers(0, c, 50) for c in counts], axis=1).astype(float), rng.random((50, 2))], axis=1)
    op = fb.optimisation_function(sb.chain_blocks(fb, "c", lambda i: i % 3), counts=counts)
    intr, extr, poses = rng.random((4, 9)), rng.random((4, 6)), rng.random((3, 6))
    free_pose = np.ones((3, 6), dtype=bool)
    free_pose[0] = False
    prob = handlers.ChainProblem(op, det, [intr, extr, poses], template=rng.random((16, 3)), unfixed=[None, None, free_pose])
    assert prob.x0.shape == (36 + 24 + 12,) and prob._jac_mask().shape == (36 + 24 + 18,)
    x = rng.random(prob.x0.shape[0])
    back = prob.get_bundle_adjustment_inputs(x)
    assert [s.shape for s in back] == [(4, 9), (4, 6), (3, 6)] and np.array_equal(back[2][0], poses[0])
    assert np.array_equal(np.concatenate([s[m] for s, m in zip(back, prob.unfixed)]), x)
    spec = cc.ChainSpec.from_blocks(op.function_blocks, counts=counts)
    assert prob._param_str(x).shape[0] == spec.layout(*counts)["n_params"]
