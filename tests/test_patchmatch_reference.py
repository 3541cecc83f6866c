"""The PatchMatch rule on the CPU (tests/patchmatch_reference.py restates include/pcs_hip.h): the two forms of the restatement agree
exactly; no input set of the device tests has a floating-point decision near its threshold; a propagated plane is the same plane; a
permuted list and a split of the iterations change no bit; what the rule does on a plane seen obliquely; every argument error is raised
without a GPU."""
import functools

import numpy as np
import pytest

from pycamset_amd import patchmatch as pm
from pycamset_amd import sweep
from tests import fusion_inputs as fi
from tests import patchmatch_inputs as inp
from tests import patchmatch_reference as ref
from tests import sweep_reference as sref

KEYS = ("depth", "normal", "plane", "cost", "status")


@functools.lru_cache(maxsize=None)
def reference(name):
    a, o = inp.CASES[name]()
    r = ref.patchmatch(**a, **o)
    for v in r.values():
        v.setflags(write=False)
    return r


def same(a, b, what=""):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _tiny(name, **more):
    a, o = inp.CASES[name]()
    return a, dict(o, **more)


@pytest.mark.parametrize("name,more", [("shape_20x14", dict(iterations=1)), ("strict_5x5", {}), ("footprint_exactly", {}),
                                       ("shape_20x14", dict(iterations=1, census=(3, 5), stride=2, truncate=3, seed=5, max_slant=30.0))])
def test_loop_and_vectorised_forms_agree_exactly(name, more):
    a, o = _tiny(name, **more)
    same(ref.patchmatch_loops(**a, **o), ref.patchmatch(**a, **o), name)


def test_loop_and_vectorised_forms_agree_on_every_start():
    a, o = _tiny("shape_20x14", iterations=1)
    truth = fi.render(a["K"], a["ext"], 20, 14, plane=(np.array([0.0, 0.0, 1.0]), fi.STEREO_Z0), sphere=None)
    d = fi.add_invalid(truth * 1.01, 5).astype(np.float32)
    same(ref.patchmatch_loops(**a, **o, depth=d), ref.patchmatch(**a, **o, depth=d), "start depth")
    p = ref.patchmatch(**a, **o)["plane"].copy()
    p[1, 5, 5:9] = np.nan
    p[2, 6, 5:9, 2] = 1.0
    o = dict(o, first_iteration=1)
    same(ref.patchmatch_loops(**a, **o, planes=p), ref.patchmatch(**a, **o, planes=p), "start planes")


@functools.lru_cache(maxsize=None)
def margins(name):
    a, o = inp.CASES[name]()
    return ref.decision_margins(**a, **o)


def test_patchmatch_gaps_are_the_pinned_ones():
    g = {k: max(margins(n)[k] for n in inp.CASES) for k in ("gap_t", "gap_n2", "gap_om")}
    print("PM_GAP measured", g["gap_t"], "PM_N2_GAP measured", g["gap_n2"], "PM_OMEGA_GAP measured", g["gap_om"])
    assert 0.5 * inp.PM_GAP <= g["gap_t"] <= inp.PM_GAP
    assert 0.5 * inp.PM_N2_GAP <= g["gap_n2"] <= inp.PM_N2_GAP
    assert 0.5 * inp.PM_OMEGA_GAP <= g["gap_om"] <= inp.PM_OMEGA_GAP


@pytest.mark.parametrize("name", list(inp.CASES))
def test_no_decision_of_a_device_input_sits_near_its_threshold(name):
    """The device's licence to exact equality: over every sample the run evaluates, no 16 u + 0.5 or 16 v + 0.5 that can decide anything
    lies within MARGIN x PM_GAP of an integer, no n_2 within MARGIN x PM_N2_GAP of 0 and no omega within MARGIN x PM_OMEGA_GAP of 0.
    A case that fails this is replaced in tests/patchmatch_inputs.py; the margin stays."""
    m = margins(name)
    print(name, "samples", m["samples"], "closest rounding", m["closest_t"], "needed", inp.MARGIN * inp.PM_GAP, "closest n_2", m["closest_n2"], "needed",
          inp.MARGIN * inp.PM_N2_GAP, "closest omega", m["closest_om"], "needed", inp.MARGIN * inp.PM_OMEGA_GAP)
    assert m["closest_t"] >= inp.MARGIN * inp.PM_GAP and m["closest_n2"] >= inp.MARGIN * inp.PM_N2_GAP and m["closest_om"] >= inp.MARGIN * inp.PM_OMEGA_GAP


def test_a_propagated_plane_is_the_same_plane():
    """The plane identity: the plane of the pixel at offset (ox, oy), read at p as ((w_q - a_q ox) - b_q oy, a_q, b_q), has at every
    window position of p the omega — and so the sample — the source plane has at the same image position.  With dyadic planes every
    operation is exact, so the two are equal to the bit."""
    a, o = inp.CASES["base"]()
    S = ref.Setup(a["images"], a["K"], a["ext"], a["neighbours"], a["depth_range"], (5, 5), 1)
    ys, xs = np.nonzero(S.strict)
    n = len(xs)
    wq, aq, bq = np.full(n, 1.0) + (xs % 4) * 2.0 ** -6, np.full(n, 2.0 ** -7), np.full(n, -(2.0 ** -8))
    sx = np.array([0] + [dx for dx, _ in S.window])[:, None]
    sy = np.array([0] + [dy for _, dy in S.window])[:, None]
    for ox, oy in ref.OFFSETS:
        wp = (wq - aq * float(ox)) - bq * float(oy)
        keep = (xs - ox >= 2) & (xs - ox < S.W - 2) & (ys - oy >= 2) & (ys - oy < S.H - 2)   # p = q - (ox, oy) with its window inside
        for slot in range(len(S.lists[2])):
            at_p = ref._sample(S, 2, slot, wp[keep], aq[keep], bq[keep], xs[keep] - ox, ys[keep] - oy, sx, sy)
            at_q = ref._sample(S, 2, slot, wq[keep], aq[keep], bq[keep], xs[keep], ys[keep], sx - ox, sy - oy)
            assert np.array_equal(at_p[0], at_q[0]) and np.array_equal(at_p[1], at_q[1]) and at_p[1].any()


def test_a_permuted_list_gives_the_same_bits():
    same(reference("base"), reference("base_permuted"))   # an integer sum: the order of a list does not change a bit


def test_a_split_of_the_iterations_equals_one_call():
    a, o = inp.CASES["iterations_3"]()
    first = ref.patchmatch(**a, **dict(o, iterations=2))
    same(ref.patchmatch(**a, **dict(o, iterations=1, first_iteration=2, planes=first["plane"])), reference("iterations_3"), "2 + 1")
    first = ref.patchmatch(**a, **dict(o, iterations=0))
    same(ref.patchmatch(**a, **dict(o, iterations=3, planes=first["plane"])), reference("iterations_3"), "0 + 3")


def test_cases_reach_what_they_are_for():
    strict = lambda n: reference(n)["status"] != ref.NOT_STRICT
    assert not strict("narrower_than_footprint").any() and not strict("lower_than_footprint").any()
    assert strict("footprint_exactly").sum() == 5 and strict("strict_5x5").sum() == 125
    r = reference("no_overlap")
    assert np.all(r["status"][strict("no_overlap")] == ref.NO_VIEW) and np.all(np.isnan(r["depth"])) and np.all(np.isnan(r["normal"]))
    r = reference("nbr_0_and_1")   # the view with an empty list: NO_VIEW at cost 0, the plane of the initialisation kept
    s = strict("nbr_0_and_1")[2]
    a, o = inp.CASES["nbr_0_and_1"]()
    assert np.all(r["status"][2][s] == ref.NO_VIEW) and np.all(r["cost"][2][s] == 0) and (r["status"][1] == 0).any()
    assert np.array_equal(r["plane"][2], ref.patchmatch(**a, **dict(o, iterations=0))["plane"][2], equal_nan=True)
    assert max(len(l) for l in inp.CASES["nbr_16"]()[0]["neighbours"]) == 16 == pm.PM_MAX_NEIGHBOURS
    two, zero = reference("base"), reference("iterations_0")
    assert np.all(two["cost"] <= zero["cost"]) and (two["cost"] < zero["cost"]).sum() > 0.5 * strict("base").sum()   # a cost never rises
    n = reference("base")["normal"]
    ok = reference("base")["status"] == 0
    K = inp.CASES["base"]()[0]["K"]
    xs, ys = np.meshgrid(np.arange(48.0), np.arange(40.0))
    ray = np.stack([np.stack([(xs - k[1]) / k[0], (ys - k[3]) / k[2], np.ones_like(xs)], axis=-1) for k in K])
    assert np.allclose(np.linalg.norm(n[ok], axis=-1), 1.0, rtol=0, atol=1e-15) and np.all(np.sum(n * ray, axis=-1)[ok] < 0)   # unit, facing the camera along the pixel's ray
    a, o = inp.CASES["start_depth_holes"]()   # a valid start depth inside the range is the start plane, flat
    init = ref.patchmatch(**a, **dict(o, iterations=0))["plane"]
    d = o["depth"]
    inside = strict("start_depth_holes") & np.isfinite(d) & (d > 0.8) & (d < 1.2)
    assert inside.sum() > 1000 and np.array_equal(init[inside][:, 0], 1.0 / d[inside]) and np.all(init[inside][:, 1:] == 0)
    a, o = inp.CASES["start_planes"]()   # the spoiled entries are redrawn, the others are kept by the initialisation
    init = ref.patchmatch(**a, **dict(o, iterations=0))["plane"]
    assert np.all(np.isfinite(init[0, 10:14, 10:20])) and np.all(init[1, 20:24, 8:12, 0] <= 1 / 0.8) and np.array_equal(init[3], o["planes"][3], equal_nan=True)
    slope = lambda r: np.nanmax(np.abs(r["plane"][..., 1:]) / r["plane"][..., :1])
    S = ref.Setup(a["images"], a["K"], a["ext"], a["neighbours"], a["depth_range"], max_slant=5.0)
    assert slope(reference("tight_slant")) <= S.sigma.max() < 0.05 * slope(reference("base"))
    assert np.all(reference("truncate_1")["cost"][strict("truncate_1")] <= 4)
    assert not np.array_equal(reference("seed_1")["plane"], reference("base")["plane"], equal_nan=True)
    assert not np.array_equal(reference("wrange_per_view")["plane"], reference("base")["plane"], equal_nan=True)


# ---- what the rule does on a plane seen obliquely --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oblique_scene():
    """fusion_inputs.stereo_ring(5, 12.0): 96 x 64, a textured plane one metre away, five views 12 degrees apart: the outer views see it at
    about 24 degrees.  The reference view is the outer view 0 and its neighbours are the two views FARTHEST from it, 36 and 48 degrees
    away: a fronto-parallel window of radius r is wrong by (baseline / depth) r tan(slant) pixels of disparity at its edge, so the
    sweep's bias on a slanted surface grows with the baseline — 0.37 px at the adjacent view for the sweep's radius of 4, 1.1 and 1.45 px
    at these two.  The start: the restated sweep, 32 planes over (0.8, 1.2), census 5 x 5, box 2.  Then 3 iterations of the restated
    PatchMatch with the defaults of ``refine_depth_maps`` but ``max_slant`` = 45 degrees, what ``reconstruct_views`` passes for its
    default ``max_angle`` (a view's state depends on no other view's, so only view 0 has a list)."""
    images, intr, ext = fi.stereo_ring(5, 12.0)
    images, K = np.array(images), np.ascontiguousarray(intr[:, :4])
    lists = [[3, 4], [], [], [], []]
    s = sref.sweep(images, K, ext, lists, sweep.depth_planes((0.8, 1.2), 32), census=(5, 5), box=2)
    p = ref.patchmatch(images, K, ext, lists, (0.8, 1.2), depth=s["depth"], iterations=3, max_slant=45.0)
    truth = fi.render(K, ext, 96, 64, plane=(np.array([0.0, 0.0, 1.0]), fi.STEREO_Z0), sphere=None)
    strict = ref.Setup(images, K, ext, lists, (0.8, 1.2)).strict
    return s["depth"][0], p, truth[0], strict, ext[0][:, :3] @ np.array([0.0, 0.0, -1.0])


def test_refinement_keeps_most_of_an_oblique_plane_and_finds_its_normal():
    """At least half of the strict pixels of the outer view end with status 0, and the median angle between the normal and the true
    one stays below twice the figure measured on this restatement, 4.49 degrees (the scene is one seed; the true slant is 24 degrees,
    which is also what the flat start planes are off by)."""
    _, p, _, strict, n_true = oblique_scene()
    ok = p["status"][0] == 0
    angle = np.degrees(np.arccos(np.clip(p["normal"][0][ok] @ n_true, -1.0, 1.0)))
    print("status 0 on", int(ok.sum()), "of", int(strict.sum()), "strict pixels; median angle to the true normal", float(np.median(angle)), "degrees")
    assert ok.sum() >= 0.5 * strict.sum()
    assert np.median(angle) <= 2 * 4.49


def test_refinement_beats_the_sweep_on_an_oblique_plane():
    """After 3 iterations the median absolute depth error of the outer view over the pixels of status 0 is strictly below the sweep's
    own median error on the same pixels.  Measured: PatchMatch 0.00147, the sweep 0.00191, over 3812 pixels of status 0 of 4368 strict
    ones.  WHERE this holds, measured on the same ring ("PatchMatch depth"): the sweep's error on the outer view grows with
    the baseline of its neighbours (0.00144 with the adjacent views 1 and 2, 0.00160 with views 2, 3, 4, 0.00191 with views 3, 4),
    while the refinement stays near 0.0015 at a slant bound of 45 degrees (0.00198, 0.00149, 0.00147) and near 0.0021 at the default
    70 degrees (0.00236, 0.00210, 0.00210).  On adjacent views a 5 x 5 window is wrong by a third of a pixel only; there the sweep's
    box sum resolves depth better than one descriptor per pixel, and the refinement does NOT beat it."""
    d_sweep, p, truth, _, _ = oblique_scene()
    ok = p["status"][0] == 0
    e_pm, e_sweep = np.abs(p["depth"][0] - truth)[ok], np.abs(d_sweep - truth)[ok]
    print("median |z - z_true| over", int(ok.sum()), "pixels: PatchMatch", float(np.median(e_pm)), "sweep", float(np.nanmedian(e_sweep)))
    assert np.median(e_pm) < np.nanmedian(e_sweep)


# ---- argument errors: none of them needs a GPU ----------------------------------------------------------------------------------------------
def good():
    K, E = fi.ring_views(3, 8, 6, 8.0)
    return dict(n_views=3, width=8, height=6, pitch=8, K=K, ext=E, neighbours=[[1, 2], [0], []], depth_range=(1.0, 2.0))


@pytest.mark.parametrize("change,name", [
    (dict(n_views=0), "images"), (dict(width=0), "images"), (dict(pitch=7), "pitch"), (dict(K=np.ones((2, 4))), "K"), (dict(K=np.full((3, 4), np.inf)), "K"),
    (dict(ext=np.zeros((2, 3, 4))), "ext"), (dict(neighbours=[[1], [0]]), "neighbours"), (dict(neighbours=[[0], [0], []]), "neighbours"),
    (dict(neighbours=[[1, 1], [0], []]), "neighbours"),
    (dict(depth_range=(1.0,)), "depth_range"), (dict(depth_range=(0.0, 1.0)), "depth_range"), (dict(depth_range=(2.0, 1.0)), "depth_range"),
    (dict(depth_range=(1.0, np.inf)), "depth_range"), (dict(depth_range=(1.0, np.nan)), "depth_range"), (dict(depth_range=np.ones((2, 2))), "depth_range"),
    (dict(depth_range="ab"), "depth_range"), (dict(depth_range=np.array([[1.0, 2.0], [1.0, 2.0], [3.0, 2.0]])), "depth_range"),
    (dict(census=5), "census"), (dict(census=(4, 5)), "census"), (dict(census=(9, 9)), "census"),
    (dict(stride=0), "stride"), (dict(stride=5), "stride"), (dict(stride=1.0), "stride"), (dict(stride=True), "stride"),
    (dict(truncate=0), "truncate"), (dict(truncate=49), "truncate"), (dict(truncate=2.5), "truncate"),
    (dict(max_slant=0.0), "max_slant"), (dict(max_slant=90.0), "max_slant"), (dict(max_slant=np.nan), "max_slant"), (dict(max_slant="steep"), "max_slant"),
    (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=1.5), "seed"),
    (dict(iterations=-1), "iterations"), (dict(iterations=1001), "iterations"), (dict(iterations=2.0), "iterations"), (dict(first_iteration=-1), "first_iteration"),
    (dict(first_iteration=1001), "first_iteration"), (dict(first_iteration=999, iterations=2), "iterations"),
    (dict(dtype=np.float16), "dtype"), (dict(dtype=np.int32), "dtype"),
])
def test_check_patchmatch_args_names_the_argument(change, name):
    with pytest.raises(ValueError, match=rf"^{name}\b"):
        pm.check_patchmatch_args(**dict(good(), **change))


def test_check_patchmatch_args_accepts_and_normalises():
    K, P, start, nbr, wrange, slope, cw, ch, stride, tau, seed, iterations, first, f32 = pm.check_patchmatch_args(**good())
    assert K.shape == (3, 4) and P.shape == (3, 12) and start.dtype == nbr.dtype == np.int32 and list(start) == [0, 2, 3, 3] and list(nbr) == [1, 2, 0]
    assert wrange.shape == (1, 2) and wrange.dtype == np.float64 and np.array_equal(wrange, [[0.5, 1.0]])
    assert slope.shape == (3,) and np.array_equal(slope, np.tan(np.radians(70.0)) / np.minimum(K[:, 0], K[:, 2]))
    assert (cw, ch, stride, tau, seed, iterations, first, f32) == (7, 7, 2, 12, 0, 3, 0, True)
    per_view = pm.check_patchmatch_args(**dict(good(), depth_range=[[1.0, 2.0], [1.5, 4.0], [0.5, 8.0]], census=(9, 7), truncate=62, seed=2 ** 64 - 1, dtype=np.float64))
    assert np.array_equal(per_view[4], [[0.5, 1.0], [0.25, 1 / 1.5], [0.125, 2.0]]) and per_view[9] == 62 and per_view[10] == 2 ** 64 - 1 and per_view[13] is False


def test_refine_depth_maps_refuses_bad_inputs_before_the_device():
    a, o = inp.CASES["shape_20x14"]()
    I, K, E, nb, zr = a["images"], a["K"], a["ext"], a["neighbours"], a["depth_range"]
    d, p = np.ones(I.shape, dtype=np.float32), np.ones(I.shape + (3,))
    for args, kw, name in (((I[0], K, E, nb, zr), {}, "images"), ((I.astype(np.int16), K, E, nb, zr), {}, "images"), ((I, K[:4], E, nb, zr), {}, "K"),
                           ((I, K, E, nb, (1.0, 0.5)), {}, "depth_range"), ((I, K, E, nb, zr, d[:, :5]), {}, "depth"), ((I, K, E, nb, zr, d.astype(np.int32)), {}, "depth"),
                           ((I, K, E, nb, zr), dict(planes=p[..., :2]), "planes"), ((I, K, E, nb, zr), dict(planes=p.astype(np.float32)), "planes"),
                           ((I, K, E, nb, zr, d), dict(planes=p), "planes"), ((I, K, E, nb, zr), dict(stride=9), "stride"), ((I, K, E, nb, zr), dict(dtype=np.int8), "dtype")):
        with pytest.raises(ValueError, match=rf"^{name}\b"):
            pm.refine_depth_maps(*args, **kw)
