"""CPU side of the matrix-free product tests (tests/test_gpu_matfree.py): every table of tests/matfree_inputs.py reaches the tile branch
it is named for, the longdouble reference agrees with scipy.sparse, and the bounds of tests/matfree_reference.py are tight enough to
see a tile branch go wrong — each mutant exceeds them by at least BLIND_FACTOR."""
import functools

import numpy as np
import pytest

from oracle import ba_oracle as orc
from tests import matfree_inputs as MI
from tests import matfree_reference as MR

BLIND_FACTOR = 1e3
CASE_CHAINS, problem = MR.CASE_CHAINS, MR.problem


# ---- every case reaches its branch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MI.RUN_SHAPE_CASES)
def test_every_run_shape_case_reaches_the_tile_class_it_is_named_for(name):
    case = MI.CASES[name]
    _, table = MI.case_table(name)
    tiles = MI.tile_classes(table)
    print(f"{name}: n = {table.shape[0]}, tiles = {[t.label for t in tiles]}, last tile {tiles[-1].n_valid} valid")
    assert len(tiles) == (table.shape[0] + 63) // 64
    if case.tiles is not None:
        assert tuple(t.label for t in tiles) == case.tiles
    assert tiles[-1].n_valid == case.last_valid and all(t.n_valid == 64 for t in tiles[:-1])
    bnd = MI.run_boundaries(table)
    if name.startswith("na-"):
        n_a = int(name.split("-")[1].split("/")[0])
        assert tiles[0].kind == "two_pair" and tiles[0].n_a == n_a and bnd.tolist() == [n_a]
        a, b = table[n_a - 1, :2], table[n_a, :2]
        assert (a[0] == b[0] and a[1] != b[1]) if name.endswith("image") else (a[0] != b[0] and a[1] != b[1] and b[1] == 0)
        assert tiles[0].uniform_cam == name.endswith("image") and not tiles[0].uniform_img and tiles[0].jv_scalar and not tiles[0].one_slab
    if name == "aligned-64":
        assert all(t.kind == "one_pair" and t.one_slab for t in tiles) and np.all(bnd % 64 == 0) and bnd.size == len(tiles) - 1
        assert np.any(table[bnd, 0] != table[bnd - 1, 0]) and np.any(table[bnd, 0] == table[bnd - 1, 0])
    if name in ("three-pairs", "runs-of-8", "runs-of-1"):
        pairs = len({tuple(x) for x in table[:64, :2]})
        assert tiles[0].kind == "other" and not tiles[0].jv_scalar and pairs == {"three-pairs": 3, "runs-of-8": 8, "runs-of-1": 64}[name]
        assert np.all(np.lexsort((table[:, 2], table[:, 1], table[:, 0])) == np.arange(table.shape[0]))   # table order: no shuffle needed
    if name.startswith("aba/"):
        assert tiles[0].kind == "other" and not tiles[0].jv_scalar and len({tuple(x) for x in table[:64, :2]}) == 2
        assert tiles[0].uniform_cam == name.endswith("image") and tiles[0].uniform_img == name.endswith("camera")
    if name == "abab":
        assert tiles[0].kind == "other" and tiles[0].jv_scalar     # the scalar J v path with pair A's lanes not a prefix
    if name == "tail-1/new-pair":
        assert tuple(table[-1, :2]) != tuple(table[-2, :2])
    if name in ("tail-1/same-pair", "n-65"):
        assert tuple(table[-1, :2]) == tuple(table[-2, :2])
    if name == "tail-63":
        assert tiles[-1].kind == "two_pair" and tiles[-1].n_a == 30      # the invalid lane sits on the SECOND pair
    if name.startswith("few-tiles"):
        assert len(tiles) == int(name.split("/")[1])
    if name == "holes":
        cam, img, key = (set(table[:, j].astype(int)) for j in range(3))
        assert not cam & set(MI.HOLES["cams"]) and not img & set(MI.HOLES["imgs"]) and not key & set(MI.HOLES["keys"])
        for chain in MI.CHAINS:
            seen = problem(name, chain).observed
            n_holes = 15 * 1 + (6 * 17 if chain != "free" else 0) + (3 * 61 if chain != "template" else 0)   # images 2 and 6 .. 21
            assert int(np.sum(~seen)) == n_holes


@pytest.mark.parametrize("image_column", [True, False])
def test_the_run_shape_cases_cover_every_class_and_every_group_edge_in_table_order(image_column):
    """With the image column (chains with poses; the free chain in the three-array index form) and without it (the free chain in the
    packed form, where only a camera change ends a run: the 'camera' group of the n_a cases is the one that splits a tile there)."""
    seen, n_as = set(), set()
    for name in MI.RUN_SHAPE_CASES:
        if name.startswith(("aba", "abab")):
            continue                       # not table order
        tiles = MI.tile_classes(MI.case_table(name)[1], image_column)
        for t in tiles:
            seen.add(t.kind)
            if t.kind == "two_pair":
                n_as.add(t.n_a)
        if name.startswith("na-") and not image_column:
            n_a = int(name.split("-")[1].split("/")[0])
            assert (tiles[0].kind, tiles[0].n_a) == (("two_pair", n_a) if name.endswith("camera") else ("one_pair", 64))
    assert seen == {"one_pair", "two_pair", "other"} and set(MI.NA_EDGES) <= n_as
    if not image_column:
        assert MI.tile_classes(MI.case_table("runs-of-1")[1], False)[0].kind == "other"     # three cameras in tile 0


@pytest.mark.parametrize("name", MI.SIZE_CASES)
def test_the_size_cases_sit_on_both_sides_of_the_lds_limit(name):
    case = MI.CASES[name]
    (chain,) = case.chains
    p = problem(name, chain)
    lds_bytes = 8 * ((p.ps.shape[0] + 1) & ~1) + 8 * 4 * 21 * 65
    print(f"{name}: n = {p.table.shape[0]}, n_params = {p.ps.shape[0]}, LDS form needs {lds_bytes} B of {150 * 1024}")
    assert p.ps.shape[0] == case.n_params[chain]
    assert (lds_bytes <= 150 * 1024) == (p.ps.shape[0] <= MI.LDS_PARAM_LIMIT) == (name == "free-lds-edge")
    if name == "free-lds-edge":
        assert p.ps.shape[0] == MI.LDS_PARAM_LIMIT and lds_bytes == 150 * 1024
    if name == "template-past-lds":      # eight pairs in every full tile; the last tile holds the last run alone
        assert all(t.kind == "other" for t in p.tiles[:-1]) and (p.tiles[-1].kind, p.tiles[-1].n_valid) == ("one_pair", 8)
    else:
        assert {t.kind for t in p.tiles} == {"one_pair", "two_pair"}
    if name == "template-past-lds":
        assert p.table.shape[0] == 3 * 2283 * 8 and np.all(np.diff(np.concatenate([[0], MI.run_boundaries(p.table)])) == 8)
    assert np.all(p.observed)


# ---- the references agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,chain", CASE_CHAINS)
def test_longdouble_products_match_scipy_sparse_products_within_the_bounds(name, chain):
    p = problem(name, chain)
    Js = p.J.to_csr()
    got = {"jv": Js @ p.v, "jtu": Js.T @ p.u, "jtjv": Js.T @ (Js @ p.v), "diag": np.asarray(Js.multiply(Js).sum(axis=0)).ravel(),
           "grad": Js.T @ p.r.reshape(-1)}
    for op in MR.OPS:
        ratio, k = MR.worst_ratio(got[op], p.ref[op], p.bound[op])
        assert ratio <= 1.0, (op, k, ratio)
        assert np.all(np.asarray(got[op])[p.bound[op] == 0] == 0.0)
    assert abs(float(np.sum(p.r * p.r)) - p.ref["cost"]) <= p.bound["cost"]
    assert np.array_equal(p.bound["jtu"] == 0, ~p.observed) and np.all(p.bound["jv"] > 0) and p.bound["cost"] > 0


# ---- the cases are not blind -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blind_factors(name, chain):
    """{(operator, mutant): max |wrong - exact| / bound} of every wrong result that exists for the problem's table; computed once."""
    p = problem(name, chain)
    bnd = MI.run_boundaries(p.table)
    moves = p.table[bnd, 0] != p.table[bnd - 1, 0]
    if p.chain != "free":
        moves = moves | (p.table[bnd, 1] != p.table[bnd - 1, 1])
    pbnd = bnd[moves]
    out = {}
    for op in MR.TRANSPOSED:
        for mutant, delta in MR.wrong_transposed(p.J, p.chain, op, bnd, pbnd, p.r, p.v, p.u).items():
            assert np.all(p.bound[op][delta != 0] > 0)
            out[op, mutant] = float(np.max(np.abs(delta[p.observed]).astype(np.float64) / p.bound[op][p.observed]))
    if pbnd.size:
        rows = pbnd - 1
        moved = p.table[rows].copy()
        moved[:, :2] = p.table[pbnd, :2]          # the row's key and measurement with the next pair's camera and image
        dense = orc.full_jac_dense(p.chain, moved, p.ps, p.template, counts=p.case.shape)
        Jn = MR.BlockJacobian(dense, orc.block_param_inds(p.chain, moved, p.case.shape), p.ps.shape[0])
        delta = MR.wrong_jv(Jn, rows, p.v, p.ref["jv"])
        out["jv", "neighbour"] = float(np.max(np.abs(delta).astype(np.float64) / p.bound["jv"].reshape(-1, 2)[rows]))
    return out


@pytest.mark.parametrize("name,chain", CASE_CHAINS)
def test_a_wrong_tile_branch_exceeds_the_bounds_by_a_factor_of_1e3(name, chain):
    """Rows lost at a run boundary, a boundary row credited to the neighbouring pair, clamped tail lanes added again, a J v row taken
    from the neighbouring pair's slabs: each leaves the bound by BLIND_FACTOR at least.  A mutant needs something to act on: the
    boundary mutants a run boundary ('n-1', 'n-63', 'n-65' have none), 'credited' and the J v one a boundary at which the pair's
    parameters change (the free chain has no pose columns, so an image-only boundary moves nothing), 'tail' a part-filled last tile."""
    p = problem(name, chain)
    f = blind_factors(name, chain)
    has_boundary = MI.run_boundaries(p.table).size > 0
    has_tail = p.table.shape[0] % 64 != 0
    assert has_boundary or has_tail
    for op in MR.TRANSPOSED:
        assert ((op, "dropped") in f) == has_boundary and ((op, "tail") in f) == has_tail
    if has_boundary and (chain != "free" or len(set(p.table[:, 0])) > 1):
        assert ("jv", "neighbour") in f and all((op, "credited") in f for op in MR.TRANSPOSED)
    worst = min(f, key=f.get)
    print(f"MATFREE-BLIND {name} {chain}: smallest factor {f[worst]:.3e} ({worst[0]}, {worst[1]}) of {len(f)} wrong results")
    assert f[worst] >= BLIND_FACTOR, {k: f"{x:.2e}" for k, x in f.items()}


def test_smallest_blind_spot_factor_over_all_cases():
    """The one figure the summary of this family quotes: the smallest factor over every case, chain, operator and mutant."""
    best = None
    for name, chain in CASE_CHAINS:
        f = blind_factors(name, chain)
        k = min(f, key=f.get)
        if best is None or f[k] < best[0]:
            best = (f[k], name, chain, k)
    print(f"MATFREE-BLIND smallest factor over all cases: {best[0]:.3e} ({best[1]}, {best[2]}, {best[3][0]}, {best[3][1]})")
    assert best[0] >= BLIND_FACTOR
