"""PatchMatch depth on the device (pycamset_amd/patchmatch.py, csrc/ba_patchmatch.hpp) against the NumPy restatement
(tests/patchmatch_reference.py).

``plane`` (float64), ``cost``, ``status``, the float64 ``depth`` and ``normal`` must be IDENTICAL to the restatement, NaN matching NaN:
the random numbers are exact, the plane arithmetic is plain IEEE in a fixed order, and behind the rounding of a warped coordinate to a
sixteenth the rule is all integers; tests/test_patchmatch_reference.py asserts for every input set used here
(tests/patchmatch_inputs.py ``CASES``) that no such rounding, and no sign of n_2 or omega, lies within MARGIN x the restatement's own
float64-versus-longdouble gap of its threshold.  A float32 depth is the float64 one rounded once."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import patchmatch as pm
from pycamset_amd import sweep
from tests import fusion_inputs as fi
from tests import patchmatch_inputs as inp
from tests import patchmatch_reference as ref
from tests import sweep_inputs as si

pytestmark = pytest.mark.gpu
KEYS = ("depth", "normal", "plane", "cost", "status")


@functools.lru_cache(maxsize=None)
def reference(name):
    a, o = inp.CASES[name]()
    r = ref.patchmatch(**a, **o)
    for v in r.values():
        v.setflags(write=False)
    return r


def device(name, dtype=np.float64, **more):
    a, o = inp.CASES[name]()
    o = dict(o, **more)
    return dict(zip(KEYS, pm.refine_depth_maps(**a, **o, dtype=dtype, return_normal=True, return_plane=True, return_cost=True, return_status=True)))


def compare(got, want, what="", keys=KEYS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        same = (g == w) | ((g != g) & (w != w))
        bad = np.argwhere(~same)
        assert bad.size == 0, (what, k, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert np.array_equal(np.isnan(got["depth"]), got["status"] != 0) and np.array_equal(np.isnan(got["normal"][..., 0]), got["status"] != 0)
    assert np.array_equal(got["status"] == ref.NOT_STRICT, got["cost"] == -1) and np.array_equal(got["cost"] == -1, np.isnan(got["plane"][..., 0]))


@pytest.mark.parametrize("name", list(inp.CASES))
def test_every_case_against_the_restatement(name):
    """The 5 x 96 x 64 ring at one iteration; 48 x 40 crops at two: a permuted list; widths and heights one below and one above a tile
    edge, an image smaller than a tile, images narrower and lower than the footprint, one of exactly the footprint and one whose
    strict rectangle is 5 x 5; a random start, a start depth with holes, a start plane map; 0 and 3 iterations; 0, 1, 4 and 16
    neighbours; a facing pair; views without overlap; census 3 x 3, 5 x 5 and 9 x 7, stride 1 and 3; truncation 1 and full scale; a
    range per view; a tight slant bound; two seeds (tests/patchmatch_inputs.py CASES)."""
    got = device(name)
    assert got["depth"].dtype == np.float64
    compare(got, reference(name), name)


def test_cases_cover_what_the_kernel_branches_on():
    shapes = {n: inp.CASES[n]()[0]["images"].shape for n in inp.CASES}
    assert shapes["ring"] == (5, 64, 96)                                       # 3 x 4 tiles of 32 x 16 per view
    assert shapes["shape_31x33"][1:] == (33, 31) and shapes["shape_33x31"][1:] == (31, 33) and shapes["shape_65x33"][1:] == (33, 65)
    assert shapes["shape_20x14"][1] < 16 and shapes["shape_20x14"][2] < 32     # smaller than one tile
    strict = lambda n: reference(n)["status"] != ref.NOT_STRICT
    assert not strict("narrower_than_footprint").any() and not strict("lower_than_footprint").any()
    assert strict("footprint_exactly")[0].sum() == 1 and strict("strict_5x5")[0].sum() == 25   # the offsets of 5 leave it on both sides
    r = reference("no_overlap")
    assert strict("no_overlap").any() and np.all(r["status"][strict("no_overlap")] == ref.NO_VIEW)
    assert [len(l) for l in inp.CASES["nbr_0_and_1"]()[0]["neighbours"]] == [1, 1, 0, 1, 1] and shapes["nbr_16"][0] == 17
    r = reference("nbr_0_and_1")
    assert np.all(r["status"][2][strict("nbr_0_and_1")[2]] == ref.NO_VIEW) and np.all(r["cost"][2][strict("nbr_0_and_1")[2]] == 0)
    assert (reference("facing")["status"] == 0).any()
    # the start: invalid start depths fall back to the draw, spoiled start planes are redrawn, the others continue
    a, o = inp.CASES["start_depth_holes"]()
    assert np.isnan(o["depth"]).any() and (o["depth"] <= 0).any() and np.isinf(o["depth"]).any()
    a, o = inp.CASES["start_planes"]()
    assert np.isnan(o["planes"][0, 10, 10, 0]) and o["first_iteration"] == 1
    # candidates of every kind are taken somewhere, and the tight slant bound refuses most slopes
    two, zero = reference("base"), reference("iterations_0")
    assert (two["cost"] < zero["cost"]).any() and not np.array_equal(reference("seed_1")["plane"], two["plane"], equal_nan=True)
    slope = lambda r: np.nanmax(np.abs(r["plane"][..., 1]) / r["plane"][..., 0])
    assert slope(reference("tight_slant")) < 0.1 * slope(two)
    assert np.all(reference("truncate_1")["cost"][strict("truncate_1")] <= 4)


def test_a_permuted_list_gives_the_same_bits():
    a, b = device("base"), device("base_permuted")
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_two_and_one_iterations_equal_three():
    first = device("iterations_3", iterations=2)
    a, o = inp.CASES["iterations_3"]()
    o = dict(o, planes=first["plane"], first_iteration=2, iterations=1)
    got = dict(zip(KEYS, pm.refine_depth_maps(**a, **o, dtype=np.float64, return_normal=True, return_plane=True, return_cost=True, return_status=True)))
    compare(got, reference("iterations_3"), "2 + 1 iterations")


@pytest.mark.parametrize("name", ["base", "wrange_per_view"])
def test_float32_depth_is_the_float64_one_rounded_once(name):
    d64, d32 = device(name), device(name, dtype=np.float32)
    for k in KEYS[2:]:
        assert np.array_equal(d32[k], d64[k], equal_nan=True), k
    assert d32["depth"].dtype == d32["normal"].dtype == np.float32
    assert np.array_equal(d32["depth"], d64["depth"].astype(np.float32), equal_nan=True) and np.array_equal(d32["normal"], d64["normal"].astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("name", ["base", "shape_33x31", "shape_65x33", "stride_3"])
def test_two_runs_and_every_tile_give_the_same_bits(name, monkeypatch):
    first = device(name)
    compare(device(name), first, name)
    for columns in (8, 16, 64):   # tiles of 8 x 64, 16 x 32 and 64 x 8 instead of 32 x 16
        monkeypatch.setenv("PCS_PM_TILE_COLUMNS", str(columns))
        compare(device(name), first, f"{name} at {columns} columns")
    monkeypatch.delenv("PCS_PM_TILE_COLUMNS")
    compare(device(name), reference(name), name)


def test_device_tensors_are_used_in_place_and_a_pitch_may_exceed_the_width():
    a, o = inp.CASES["shape_33x31"]()
    V, H, W = a["images"].shape
    wide = torch.full((V, H, W + 13), 255, dtype=torch.uint8, device="cuda")
    wide[:, :, :W] = torch.from_numpy(a["images"]).cuda()
    view = wide[:, :, :W]
    assert not view.is_contiguous()
    out = pm.refine_depth_maps(view, a["K"], a["ext"], a["neighbours"], a["depth_range"], **o, dtype=np.float64, return_normal=True, return_plane=True, return_cost=True,
                               return_status=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out)
    compare(dict(zip(KEYS, (t.cpu().numpy() for t in out))), reference("shape_33x31"), "pitched tensor")
    only = pm.refine_depth_maps(view, a["K"], a["ext"], a["neighbours"], a["depth_range"], **o, dtype=np.float64)
    assert isinstance(only, torch.Tensor) and torch.equal(torch.nan_to_num(only), torch.nan_to_num(out[0]))
    planes = out[2].clone()   # a start plane map on the device is read, never changed
    pm.refine_depth_maps(view, a["K"], a["ext"], a["neighbours"], a["depth_range"], planes=planes, **dict(o, first_iteration=2, iterations=1))
    assert torch.equal(torch.nan_to_num(planes), torch.nan_to_num(out[2]))


def test_handle_reports_its_kernel_time_and_refuses_a_run_before_its_tables():
    from pycamset_amd import _capi

    a, o = inp.CASES["shape_20x14"]()
    h = pm.PatchMatcher(0)
    with pytest.raises(_capi.PcsError, match="nothing has run yet"):
        h.last_kernel_ms()
    img = torch.from_numpy(a["images"]).cuda()
    plane, cost = torch.empty((5, 14, 20, 3), dtype=torch.float64, device="cuda"), torch.empty((5, 14, 20), dtype=torch.int32, device="cuda")
    depth = torch.empty((5, 14, 20), dtype=torch.float64, device="cuda")
    wr, slope = np.array([[1 / 1.2, 1 / 0.8]]), np.full(5, 0.02)
    kw = dict(census=(3, 3), stride=1, truncate=2)
    with pytest.raises(_capi.PcsError, match="come first"):
        h.init(img.data_ptr(), 20, wr, slope, plane.data_ptr(), cost.data_ptr(), **kw)
    h.set_views(20, 14, a["K"], a["ext"].reshape(5, 12))
    with pytest.raises(_capi.PcsError, match="come first"):
        h.iterate(0, 1, img.data_ptr(), 20, wr, slope, plane.data_ptr(), cost.data_ptr(), **kw)
    start, nbr = np.array([0, 1, 2, 3, 4, 5]), np.array([1, 0, 1, 2, 3])
    h.set_neighbours(start, nbr)
    with pytest.raises(_capi.PcsError, match="pcs_pm_init or pcs_pm_iterate comes first"):
        h.finish(plane.data_ptr(), cost.data_ptr(), depth.data_ptr(), f32=False, **kw)
    with pytest.raises(_capi.PcsError, match="pitch"):
        h.init(img.data_ptr(), 19, wr, slope, plane.data_ptr(), cost.data_ptr(), **kw)
    with pytest.raises(_capi.PcsError, match="n_w"):
        h.init(img.data_ptr(), 20, np.tile(wr, (2, 1)), slope, plane.data_ptr(), cost.data_ptr(), **kw)
    h.init(img.data_ptr(), 20, wr, slope, plane.data_ptr(), cost.data_ptr(), **kw)
    assert h.last_kernel_ms() > 0.0
    h.iterate(0, 1, img.data_ptr(), 20, wr, slope, plane.data_ptr(), cost.data_ptr(), **kw)
    assert h.last_kernel_ms() > 0.0
    h.finish(plane.data_ptr(), cost.data_ptr(), depth.data_ptr(), f32=False, **kw)
    assert h.last_kernel_ms() > 0.0
    S = ref.Setup(a["images"], a["K"], a["ext"], (start, nbr), (0.8, 1.2), (3, 3), 1, 2)
    S.sigma = slope
    P, C = ref.initialise(S)
    ref.half_iteration(S, P, C, 0, 0)
    ref.half_iteration(S, P, C, 0, 1)
    assert np.array_equal(plane.cpu().numpy(), P, equal_nan=True) and np.array_equal(cost.cpu().numpy(), C)
    assert np.array_equal(depth.cpu().numpy(), ref.finish(S, P, C)[0], equal_nan=True)
    h.close()


def test_reconstruct_views_refined_keeps_the_ring_on_its_plane():
    """``refine_iterations=2``: every fused point within one plane step of the plane; ``refine_iterations=0`` returns exactly what the
    function returns without the keyword.  Measured on the restatement chain (sweep_reference -> patchmatch_reference ->
    fusion_reference, which the device equals): 20 264 fused points, the largest distance 0.79 steps, the median 0.054 (0.026 and a
    largest 0.57 without refinement).  The slant bound ``reconstruct_views`` passes (90 - max_angle = 45 degrees) matters: at the
    refinement's own default of 70 degrees six points lie 1.14 to 1.35 steps away, steep planes near the edge of the strict rectangle on
    which two views agree.  It is no guarantee of the rule: at 3 iterations two points lie up to 2.6 steps away (DESIGN.md,
    "PatchMatch depth")."""
    images, intr, ext = fi.stereo_ring(5)
    plain = sweep.reconstruct_views(np.array(images), intr, ext, si.RING_RANGE, si.RING_STEPS, dtype=np.float64)
    zero = sweep.reconstruct_views(np.array(images), intr, ext, si.RING_RANGE, si.RING_STEPS, dtype=np.float64, refine_iterations=0)
    assert np.array_equal(plain[0], zero[0]) and np.array_equal(plain[1], zero[1])
    pts, grey = sweep.reconstruct_views(np.array(images), intr, ext, si.RING_RANGE, si.RING_STEPS, dtype=np.float64, refine_iterations=2)
    counts = sweep.reconstruct_views.last[4]
    step = (si.RING_RANGE[1] - si.RING_RANGE[0]) / si.RING_STEPS
    off, off0 = np.abs(pts[:, 2] - fi.STEREO_Z0), np.abs(plain[0][:, 2] - fi.STEREO_Z0)
    print("fused points", len(pts), "per view", counts, "without refinement", len(plain[0]), "largest distance from the plane", float(off.max()) / step, "steps, median",
          float(np.median(off)) / step, "; without refinement", float(off0.max()) / step, float(np.median(off0)) / step)
    assert pts.shape == (sum(counts), 3) and grey.shape == (len(pts),) and grey.dtype == np.uint8 and len(pts) > 0
    assert off.max() <= step
