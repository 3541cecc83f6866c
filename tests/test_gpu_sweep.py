"""The plane sweep on the device (pycamset_amd/sweep.py, csrc/ba_sweep.hpp) against the NumPy restatement (tests/sweep_reference.py).

``level``, ``cost`` and ``status`` must be IDENTICAL to the restatement and ``depth`` in float64 bit-equal: behind the rounding of a
warped coordinate to a sixteenth the rule is all integers, and tests/test_sweep_reference.py asserts for every input set used here
(tests/sweep_inputs.py ``CASES``) that no such rounding, and no sign of n_2, lies within MARGIN x the restatement's own
float64-versus-longdouble gap of its threshold.  A float32 depth is the float64 one rounded once.

No golden from the reference exists for the sweep itself: the reference hands this step to an external program.  The plane table does
have one (tests/golden/mvsnet_depth_lines.npz, checked without a GPU)."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import sweep
from tests import fusion_inputs as fi
from tests import sweep_inputs as inp
from tests import sweep_reference as ref

pytestmark = pytest.mark.gpu
KEYS = ("depth", "level", "cost", "status")


@functools.lru_cache(maxsize=None)
def reference(name):
    a, o = inp.CASES[name]()
    r = ref.sweep(**a, **o)
    for v in r.values():
        v.setflags(write=False)
    return r


def device(name, dtype=np.float64):
    a, o = inp.CASES[name]()
    return dict(zip(KEYS, sweep.sweep_depth_maps(**a, **o, dtype=dtype, return_level=True, return_cost=True, return_status=True)))


def compare(got, want, what=""):
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        same = (g == w) | ((g != g) & (w != w))
        bad = np.argwhere(~same)
        assert bad.size == 0, (what, k, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert np.array_equal(np.isnan(got["depth"]), got["status"] != 0)
    assert np.array_equal(got["status"] == ref.NOT_STRICT, got["level"] == -16) and np.array_equal(got["level"] == -16, got["cost"] == -1)


@pytest.mark.parametrize("name", list(inp.CASES))
def test_every_case_against_the_restatement(name):
    """The 5 x 96 x 64 ring (u = 0 and 15, a permuted list); widths and heights one below and one above a tile edge, an image smaller
    than a tile, images narrower and lower than the footprint and one of exactly the footprint; 1, 2 and 3 planes, a falling table, one
    row of planes per view, inverse spacing; 0, 1, 4 and 16 neighbours; a facing pair; views without overlap; census 3 x 3, 5 x 5 and
    9 x 7; box radius 0, 2 and 4; truncation 1 and full scale (tests/sweep_inputs.py CASES)."""
    got = device(name)
    assert got["depth"].dtype == np.float64
    compare(got, reference(name), name)


def test_cases_cover_what_the_kernel_branches_on():
    shapes = {n: inp.CASES[n]()[0]["images"].shape for n in inp.CASES}
    assert shapes["ring"] == (5, 64, 96)                                       # 3 x 2 tiles of 32 x 32 per view
    assert shapes["shape_31x33"][1:] == (33, 31) and shapes["shape_33x31"][1:] == (31, 33) and shapes["shape_65x33"][1:] == (33, 65)
    assert shapes["shape_20x14"][1] < 32 and shapes["shape_20x14"][2] < 32     # smaller than one tile
    assert shapes["narrower_than_footprint"][2] == 8 and shapes["lower_than_footprint"][1] == 8 and shapes["footprint_exactly"][1:] == (9, 9)
    assert np.all(reference("narrower_than_footprint")["status"] == ref.NOT_STRICT) and np.all(reference("lower_than_footprint")["status"] == ref.NOT_STRICT)
    strict = reference("no_overlap")["status"] != ref.NOT_STRICT
    assert strict.any() and np.all(reference("no_overlap")["status"][strict] == ref.NO_VIEW)
    assert [len(l) for l in inp.CASES["nbr_0_and_1"]()[0]["neighbours"]] == [1, 1, 0, 1, 1] and shapes["nbr_16"][0] == 17
    assert (reference("ring_u15")["status"] == ref.UNIQUENESS).any() and (reference("facing")["status"] == 0).any()


def test_a_permuted_list_gives_the_same_bits():
    a, b = device("ring"), device("ring_permuted")
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["ring_u15", "planes_per_view"])
def test_float32_depth_is_the_float64_one_rounded_once(name):
    d64, d32 = device(name), device(name, dtype=np.float32)
    for k in KEYS[1:]:
        assert np.array_equal(d32[k], d64[k]), k
    assert d32["depth"].dtype == np.float32 and np.array_equal(d32["depth"], d64["depth"].astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("name", ["ring_u15", "shape_33x31", "census_9x7", "box_4"])
def test_two_runs_and_every_tile_give_the_same_bits(name, monkeypatch):
    first = device(name)
    compare(device(name), first, name)
    for columns in (8, 16, 64):   # tiles of 8 x 128, 16 x 64 and 64 x 16 instead of 32 x 32
        monkeypatch.setenv("PCS_SWEEP_TILE_COLUMNS", str(columns))
        compare(device(name), first, f"{name} at {columns} columns")
    monkeypatch.delenv("PCS_SWEEP_TILE_COLUMNS")
    compare(device(name), reference(name), name)


def test_device_tensors_are_used_in_place_and_a_pitch_may_exceed_the_width():
    a, o = inp.CASES["shape_33x31"]()
    V, H, W = a["images"].shape
    wide = torch.full((V, H, W + 13), 255, dtype=torch.uint8, device="cuda")
    wide[:, :, :W] = torch.from_numpy(a["images"]).cuda()
    view = wide[:, :, :W]
    assert not view.is_contiguous()
    out = sweep.sweep_depth_maps(view, a["K"], a["ext"], a["neighbours"], a["planes"], **o, dtype=np.float64, return_level=True, return_cost=True, return_status=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out)
    compare(dict(zip(KEYS, (t.cpu().numpy() for t in out))), reference("shape_33x31"), "pitched tensor")
    only = sweep.sweep_depth_maps(view, a["K"], a["ext"], a["neighbours"], a["planes"], **o, dtype=np.float64)
    assert isinstance(only, torch.Tensor) and torch.equal(torch.nan_to_num(only), torch.nan_to_num(out[0]))


def test_handle_reports_its_kernel_time_and_refuses_a_run_before_its_tables():
    from pycamset_amd import _capi

    a, _ = inp.CASES["shape_20x14"]()
    h = sweep.PlaneSweeper(0)
    with pytest.raises(_capi.PcsError, match="nothing has run yet"):
        h.last_kernel_ms()
    img, out = torch.from_numpy(a["images"]).cuda(), torch.empty(a["images"].shape, dtype=torch.float32, device="cuda")
    with pytest.raises(_capi.PcsError, match="come first"):
        h.run(img.data_ptr(), 20, a["planes"], out.data_ptr())
    h.set_views(20, 14, a["K"], a["ext"].reshape(5, 12))
    start, nbr = np.array([0, 1, 2, 3, 4, 5]), np.array([1, 0, 1, 2, 3])
    h.set_neighbours(start, nbr)
    with pytest.raises(_capi.PcsError, match="pitch"):
        h.run(img.data_ptr(), 19, a["planes"], out.data_ptr())
    with pytest.raises(_capi.PcsError, match="n_z"):
        h.run(img.data_ptr(), 20, np.ones((2, 1)), out.data_ptr())
    h.run(img.data_ptr(), 20, a["planes"], out.data_ptr(), census=(3, 3), box=1)
    assert h.last_kernel_ms() > 0.0
    want = ref.sweep(a["images"], a["K"], a["ext"], (start, nbr), a["planes"], census=(3, 3), box=1)["depth"].astype(np.float32)
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    h.close()


def test_reconstruct_views_puts_the_ring_on_its_plane():
    """From the images of the ring to one cloud: every fused point within one plane step of the plane, and at least half of the
    strict pixels of the middle view kept (the same conditions hold on the restatement chain: tests/test_sweep_reference.py)."""
    images, intr, ext = fi.stereo_ring(5)
    pts, grey = sweep.reconstruct_views(np.array(images), intr, ext, inp.RING_RANGE, inp.RING_STEPS, dtype=np.float64)
    K, nb, planes, depth, counts = sweep.reconstruct_views.last
    step = (inp.RING_RANGE[1] - inp.RING_RANGE[0]) / inp.RING_STEPS
    strict = ref.strict_mask(96, 64, 5, 5, 2)
    off = np.abs(pts[:, 2] - fi.STEREO_Z0)
    print("fused points", len(pts), "per view", counts, "largest distance from the plane", float(off.max()) / step, "steps; strict pixels", int(strict.sum()))
    assert pts.shape == (sum(counts), 3) and grey.shape == (len(pts),) and grey.dtype == np.uint8
    assert off.max() <= step and counts[2] >= 0.5 * strict.sum()
    assert np.array_equal(planes, sweep.depth_planes(inp.RING_RANGE, inp.RING_STEPS)) and [list(l) for l in nb] == [[j for j in range(5) if j != i] for i in range(5)]
