"""Detection tables for the tests of the matrix-free J products (csrc/ba_matfree.hpp), shared by tests/test_matfree_reference.py
(CPU) and tests/test_gpu_matfree.py: one table per tile shape the kernel branches on, a restatement of those branches
(``tile_classes``) that proves which table reaches which, and the three sizes around the 13 740-parameter LDS limit.  NumPy only.

The run-shape cases are cut from ONE full-visibility rig (3 cameras x 22 images x 128 keys, 0.3 px noise): ``table_with_runs`` takes
the first keys of the named (camera, image) pairs in the given order, so that a run boundary falls on any row wanted.  66 pairs let a
tile hold 64 different ones.  The size cases are whole tables of rigs of their own."""
import functools
from dataclasses import dataclass

import numpy as np

from pycamset_amd import synthetic

TILE = 64                    # detections per wave and tile (csrc/ba_device.hpp TILE)
LDS_PARAM_LIMIT = 13740      # 150 KiB = 8 * (n_params rounded up to even) + 4 panels of 21 x 65 doubles  ->  n_params <= 13 740
CHAINS = ("template", "self", "free")
SMALL_SHAPE = (3, 22, 128)   # cameras, images, keys of the rig the run-shape cases are cut from


@dataclass(frozen=True)
class Tile:
    """What the kernel's conditions evaluate to on one 64-row tile (invalid lanes clamped to row n - 1, as in the kernel)."""
    kind: str             # transposed products with LDS accumulators: "one_pair" | "two_pair" | "other"
    n_a: int              # lanes (clamped ones included) on the first lane's (camera, image) pair: the ballot's popcount
    n_valid: int          # rows of the tile below n
    jv_scalar: bool       # J v: forward mode with scalar slab loads (every lane on the first or on the last lane's pair)
    one_slab: bool        # the general path's eval_detection takes scalar slab loads (one camera and one image in the tile)
    uniform_cam: bool     # LDS_ACC = false: accumulate_group's wave-sum form for the camera columns (valid lanes share the camera) ...
    uniform_img: bool     # ... and for the pose columns

    @property
    def label(self):
        return f"{self.kind}(n_a={self.n_a})" if self.kind == "two_pair" else self.kind


def tile_classes(table, image_column=True):
    """One ``Tile`` per 64 rows of an (N, 5) table: the branch conditions of ba_matfree_kernel, restated.
         in_a     = lane's (c, im) == lane 0's          in_b = lane's (c, im) == lane 63's
         two-pair form  <=>  all(in_a | in_b)  and  the in_a lanes are lanes 0 .. n_a - 1      (n_a == 64: one pair, the plain sum)
         J v scalar path <=> all(in_a | in_b)                                                   (no prefix condition).
    ``image_column=False``: what the kernel sees of a FREE-chain table in the packed index form — that chain has no image column, the
    packed word gives it no bits and every lane decodes image 0, so only a camera change ends a run there.  (The three-array index form
    hands the kernel the image values as they are: ``image_column=True`` for every chain.)"""
    table = np.asarray(table)
    n = table.shape[0]
    cam, img = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64)
    if not image_column:
        img = np.zeros_like(img)
    out = []
    for t in range((n + TILE - 1) // TILE):
        lane_row = t * TILE + np.arange(TILE)
        valid = lane_row < n
        rows = np.where(valid, lane_row, n - 1)
        c, im = cam[rows], img[rows]
        in_a = (c == c[0]) & (im == im[0])
        in_b = (c == c[-1]) & (im == im[-1])
        n_a = int(in_a.sum())
        both = bool(np.all(in_a | in_b))
        prefix = bool(np.all(in_a[:n_a]))
        kind = "other" if not (both and prefix) else "one_pair" if n_a == TILE else "two_pair"
        out.append(Tile(kind, n_a, int(valid.sum()), both, n_a == TILE,
                        bool(np.all(c[valid] == c[0])), bool(np.all(im[valid] == im[0]))))
    return out


def run_boundaries(table):
    """Rows i >= 1 whose (camera, image) pair differs from row i - 1's: the first row of every run but the first."""
    table = np.asarray(table)
    return 1 + np.flatnonzero(np.any(table[1:, :2] != table[:-1, :2], axis=1))


@functools.lru_cache(maxsize=None)
def rig_of(shape, seed=77):
    """Full-visibility rig of (cameras, images, keys); random points in a 6 cm cube, 0.3 px noise, parameters 1 % off the truth."""
    n_cams, n_imgs, n_keys = shape
    pts = np.random.default_rng(seed + 1000).uniform(-0.03, 0.03, (n_keys, 3))
    rig = synthetic.make_rig(f"matfree-{n_cams}x{n_imgs}x{n_keys}", n_cams, n_imgs, pts, seed=seed, visibility=1.0, noise_px=0.3)
    rig.detections.setflags(write=False)
    return rig


def table_with_runs(rig, runs):
    """The (N, 5) table of the runs ``(cam, image, length[, first_key])`` in the given order: ``length`` keys of that pair, from
    ``first_key`` (default 0) on.  ``rig`` has every (camera, image, key) once, in table order."""
    n_imgs, n_keys = rig.n_imgs, rig.n_keys
    assert rig.n_det == rig.n_cams * n_imgs * n_keys, "table_with_runs needs a full-visibility rig"
    rows = []
    for cam, img, length, *first in runs:
        k0 = first[0] if first else 0
        assert 0 <= cam < rig.n_cams and 0 <= img < n_imgs and length >= 1 and k0 + length <= n_keys, (cam, img, length, k0)
        rows.append((cam * n_imgs + img) * n_keys + k0 + np.arange(length))
    table = rig.detections[np.concatenate(rows)].copy()
    return table


@dataclass(frozen=True)
class Case:
    """One table recipe.  ``tiles``: the labels ``tile_classes`` must report, tile by tile (run-shape cases) — what the name promises;
    ``last_valid``: the valid rows of the last tile; ``n_params``: per chain, for the size cases."""
    shape: tuple                      # (cameras, images, keys) of the rig
    runs: tuple = None                # None: the rig's whole table
    drop_keys: tuple = ()             # keys removed from the table afterwards
    chains: tuple = CHAINS
    tiles: tuple = None
    last_valid: int = None
    n_params: dict = None


def _two(n_a):
    return f"two_pair(n_a={n_a})"


def _na_case(n_a, change):
    # image: (0, 0) -> (0, 1);  camera: (0, 5) -> (1, 0): the image falls back to 0, both fields change
    a, b = ((0, 0), (0, 1)) if change == "image" else ((0, 5), (1, 0))
    return Case(SMALL_SHAPE, runs=((*a, n_a), (*b, 128 - n_a)), tiles=(_two(n_a), "one_pair"), last_valid=64)


def _runs_of(length, n_rows):
    """Runs of ``length`` rows over the pairs in table order (camera -> image) until ``n_rows`` rows are there."""
    runs, left, pair = [], n_rows, 0
    while left > 0:
        runs.append((pair // SMALL_SHAPE[1], pair % SMALL_SHAPE[1], min(length, left)))
        left -= length
        pair += 1
    return tuple(runs)


NA_EDGES = (1, 21, 22, 23, 43, 44, 45, 63)   # around the starts of the three summing groups (rows 0, 22, 44) and the tile's ends

CASES = {}
for _n in NA_EDGES:
    CASES[f"na-{_n}/image"] = _na_case(_n, "image")
    CASES[f"na-{_n}/camera"] = _na_case(_n, "camera")
CASES.update({
    # every tile inside one run, every run boundary on a tile boundary (image and camera changes)
    "aligned-64": Case(SMALL_SHAPE, runs=((0, 0, 64), (0, 1, 64), (0, 2, 64), (1, 0, 64), (1, 1, 64), (2, 0, 64)),
                       tiles=("one_pair",) * 6, last_valid=64),
    # three pairs per tile, in table order; the last tile part-filled
    "three-pairs": Case(SMALL_SHAPE, runs=((0, 0, 20), (0, 1, 20), (0, 2, 24), (0, 3, 20), (1, 0, 20), (1, 1, 24), (2, 0, 20), (2, 1, 20), (2, 2, 10)),
                        tiles=("other", "other", "other"), last_valid=50),
    "runs-of-8": Case(SMALL_SHAPE, runs=_runs_of(8, 200), tiles=("other", "other", "other", "one_pair"), last_valid=8),   # 25 pairs, two cameras
    # 66 pairs of one row each: 64 different pairs in tile 0
    "runs-of-1": Case(SMALL_SHAPE, runs=_runs_of(1, 66), tiles=("other", _two(1)), last_valid=2),
    # pair A, pair B, pair A again inside one tile: two pairs, but A's lanes are no prefix (not the reference's order)
    "aba/image": Case(SMALL_SHAPE, runs=((0, 0, 20), (0, 1, 24), (0, 0, 20, 20), (0, 2, 10)), tiles=("other", "one_pair"), last_valid=10),
    "aba/camera": Case(SMALL_SHAPE, runs=((0, 0, 20), (1, 0, 24), (0, 0, 20, 20), (1, 1, 10)), tiles=("other", "one_pair"), last_valid=10),
    # A B A B: first lane on A, last lane on B — J v takes the scalar two-pair path, the transposed products the lane-by-lane one
    "abab": Case(SMALL_SHAPE, runs=((0, 0, 16), (1, 1, 16), (0, 0, 16, 16), (1, 1, 16, 16)), tiles=("other",), last_valid=64),
    # last tiles with one valid row: it starts a new pair / it continues the previous pair
    "tail-1/new-pair": Case(SMALL_SHAPE, runs=((0, 0, 40), (0, 1, 88), (1, 0, 1)), tiles=(_two(40), "one_pair", "one_pair"), last_valid=1),
    "tail-1/same-pair": Case(SMALL_SHAPE, runs=((0, 0, 40), (0, 1, 89)), tiles=(_two(40), "one_pair", "one_pair"), last_valid=1),
    # 63 valid rows across a boundary: the invalid lane belongs to the second pair
    "tail-63": Case(SMALL_SHAPE, runs=((0, 0, 64), (0, 1, 30), (1, 2, 33)), tiles=("one_pair", _two(30)), last_valid=63),
    "n-1": Case(SMALL_SHAPE, runs=((1, 3, 1),), tiles=("one_pair",), last_valid=1),
    "n-63": Case(SMALL_SHAPE, runs=((1, 3, 63),), tiles=("one_pair",), last_valid=63),
    "n-65": Case(SMALL_SHAPE, runs=((1, 3, 65),), tiles=("one_pair", "one_pair"), last_valid=1),
    # 1, 2, 3 tiles: waves of the only workgroup without a tile; 5 tiles: a second workgroup with one tile (4 tiles per workgroup at least)
    "few-tiles/1": Case(SMALL_SHAPE, runs=_runs_of(40, 60), tiles=(_two(40),), last_valid=60),
    "few-tiles/2": Case(SMALL_SHAPE, runs=_runs_of(40, 120), tiles=(_two(40), _two(16)), last_valid=56),
    "few-tiles/3": Case(SMALL_SHAPE, runs=_runs_of(40, 180), tiles=(_two(40), "other", _two(32)), last_valid=52),
    "few-tiles/5": Case(SMALL_SHAPE, runs=_runs_of(40, 300), tiles=(_two(40), "other", _two(32), "other", _two(24)), last_valid=44),
    # camera 1, image 2, keys 3, 17, 50 and every key from 70 on have no row: their entries of the transposed products stay 0.0
    "holes": Case(SMALL_SHAPE, runs=((0, 0, 70), (0, 1, 70), (0, 3, 70), (2, 0, 70), (2, 4, 70), (2, 5, 70)), drop_keys=(3, 17, 50), last_valid=18),
    # the last size that takes the LDS form (a 150 KiB dynamic allocation) and the first sizes that cannot
    "free-lds-edge": Case((3, 1, 4565), chains=("free",), n_params={"free": 13740}),
    "free-past-lds": Case((3, 1, 4566), chains=("free",), n_params={"free": 13743}),
    "template-past-lds": Case((3, 2283, 8), chains=("template",), n_params={"template": 13743}),
})
HOLES = dict(cams=(1,), imgs=(2,), keys=(3, 17, 50) + tuple(range(70, 128)))
RUN_SHAPE_CASES = tuple(k for k, c in CASES.items() if c.n_params is None)
SIZE_CASES = tuple(k for k, c in CASES.items() if c.n_params is not None)


def n_params_of(chain, shape):
    n_cams, n_imgs, n_keys = shape
    return 15 * n_cams + (6 * n_imgs if chain != "free" else 0) + (3 * n_keys if chain != "template" else 0)


@functools.lru_cache(maxsize=None)
def case_table(name):
    """-> (rig, table (N, 5), read-only) of the case."""
    case = CASES[name]
    rig = rig_of(case.shape)
    table = rig.detections if case.runs is None else table_with_runs(rig, case.runs)
    if case.drop_keys:
        table = table[~np.isin(table[:, 2].astype(np.int64), case.drop_keys)]
    table = np.ascontiguousarray(table)
    table.setflags(write=False)
    return rig, table


def param_group(chain, shape, j):
    """'intrinsics of camera 2 [4]'-style name of parameter ``j`` of the string (include/pcs_hip.h layout)."""
    n_cams, n_imgs, n_keys = shape
    groups = [("intrinsics of camera", 9, n_cams), ("extrinsics of camera", 6, n_cams)]
    if chain != "free":
        groups.append(("pose of image", 6, n_imgs))
    if chain != "template":
        groups.append(("point of key", 3, n_keys))
    for what, width, count in groups:
        if j < width * count:
            return f"{what} {j // width} [{j % width}]"
        j -= width * count
    raise IndexError(j)


def feeding_tiles(cols, tiles, j):
    """Labels of the tiles whose rows have parameter ``j`` among their columns (``cols``: (N, P) global columns per detection)."""
    rows = np.flatnonzero(np.any(cols == j, axis=1))
    return sorted({f"tile {t}: {tiles[t].label}, {tiles[t].n_valid} valid" for t in np.unique(rows // TILE)})
