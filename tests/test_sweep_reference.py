"""The plane sweep's rule on the CPU (tests/sweep_reference.py restates include/pcs_hip.h): the two forms of the restatement agree
exactly; no input set of the device tests has a floating-point decision near its threshold; the rule itself recovers a textured plane;
``depth_planes`` is the hypothesis set of the line the reference writes; every argument error is raised without a GPU."""
import ctypes
import functools
from pathlib import Path

import numpy as np
import pytest

from pycamset_amd import _capi, sweep
from tests import fusion_inputs as fi
from tests import fusion_reference as fref
from tests import sweep_inputs as inp
from tests import sweep_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "mvsnet_depth_lines.npz"


@functools.lru_cache(maxsize=None)
def reference(name):
    a, o = inp.CASES[name]()
    r = ref.sweep(**a, **o)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("name,extra", [("shape_20x14", dict(uniqueness_ratio=15)), ("footprint_exactly", {}), ("facing", dict(uniqueness_ratio=40)),
                                        ("planes_3", {}), ("nbr_0_and_1", dict(census=(3, 3), box=1, truncate=5))])
def test_loop_and_vectorised_forms_agree_exactly(name, extra):
    a, o = inp.CASES[name]()
    o = dict(o, **extra)
    L, R = ref.sweep_loops(**a, **o), ref.sweep(**a, **o)
    for k in ("level", "cost", "status", "depth"):
        assert L[k].dtype == R[k].dtype and np.array_equal(L[k], R[k], equal_nan=True), k


@functools.lru_cache(maxsize=None)
def margins(name):
    return ref.decision_margins(**inp.CASES[name]()[0])


def test_sweep_gaps_are_the_pinned_ones():
    gt = max(margins(n)["gap_t"] for n in inp.CASES)
    gn = max(margins(n)["gap_n2"] for n in inp.CASES)
    print("SWEEP_GAP measured", gt, "SWEEP_N2_GAP measured", gn)
    assert 0.5 * inp.SWEEP_GAP <= gt <= inp.SWEEP_GAP
    assert 0.5 * inp.SWEEP_N2_GAP <= gn <= inp.SWEEP_N2_GAP


@pytest.mark.parametrize("name", list(inp.CASES))
def test_no_rounding_of_a_device_input_sits_near_its_threshold(name):
    """The device's licence to exact equality: no 16 u + 0.5 or 16 v + 0.5 of a sample with n_2 > 0 lies within MARGIN x SWEEP_GAP of an
    integer, and no n_2 within MARGIN x SWEEP_N2_GAP of 0.  A case that fails this is replaced HERE."""
    m = margins(name)
    print(name, "closest rounding", m["closest_t"], "needed", inp.MARGIN * inp.SWEEP_GAP, "closest n_2", m["closest_n2"], "needed", inp.MARGIN * inp.SWEEP_N2_GAP)
    assert m["closest_t"] >= inp.MARGIN * inp.SWEEP_GAP and m["closest_n2"] >= inp.MARGIN * inp.SWEEP_N2_GAP


def test_cases_reach_what_they_are_for():
    strict = lambda n: reference(n)["status"] != ref.NOT_STRICT
    assert not strict("narrower_than_footprint").any() and not strict("lower_than_footprint").any()
    assert strict("footprint_exactly").sum() == 5 and strict("shape_20x14").any()
    r = reference("no_overlap")
    assert np.all(r["status"][strict("no_overlap")] == ref.NO_VIEW) and np.all(np.isnan(r["depth"]))
    a, _ = inp.CASES["facing"]()
    A, b = ref.warp_table(a["K"][0], a["ext"][0].reshape(12), a["K"][1], a["ext"][1].reshape(12))
    xs, ys = np.meshgrid(np.arange(64.0), np.arange(48.0))
    n2 = np.stack([ref.project(A, b, z, xs, ys)[0] for z in a["planes"]])
    assert (n2 <= 0).any() and (n2 > 0).any()   # planes behind and in front of the camera that faces the reference view
    for name in ("ring_u15", "planes_3", "census_9x7", "truncate_full", "inverse_spacing"):
        assert (reference(name)["status"] == ref.UNIQUENESS).any(), name
    for k in ("level", "cost", "status", "depth"):   # an integer sum: the order of a list does not change a bit
        assert np.array_equal(reference("ring_permuted")[k], reference("ring")[k], equal_nan=True)
    assert max(len(l) for l in inp.CASES["nbr_16"]()[0]["neighbours"]) == 16 == sweep.SWEEP_MAX_NEIGHBOURS
    r = reference("nbr_0_and_1")   # the view with an empty list: every strict pixel NO_VIEW at level 0 and cost 0
    s = strict("nbr_0_and_1")[2]
    assert np.all(r["status"][2][s] == ref.NO_VIEW) and np.all(r["level"][2][s] == 0) and np.all(r["cost"][2][s] == 0) and (r["status"][1] == 0).any()
    for name, D in (("planes_1", 1), ("planes_2", 2), ("planes_3", 3)):   # the ends of the table: no offset
        lv = reference(name)["level"][strict(name)]
        assert lv.min() >= 0 and lv.max() <= 16 * (D - 1) and np.all((lv % 16 == 0) | ((D == 3) & (lv >= 8) & (lv <= 24)))
    assert np.all(reference("truncate_1")["cost"][strict("truncate_1")] <= 4)
    z = inp.CASES["planes_per_view"]()[0]["planes"]
    assert z.shape == (5, 6) and not np.array_equal(z[0], z[1])
    z = inp.CASES["inverse_spacing"]()[0]["planes"]
    assert np.allclose(np.diff(1.0 / z), np.diff(1.0 / z)[0], rtol=1e-9) and not np.allclose(np.diff(z), np.diff(z)[0], rtol=1e-3)
    shapes = {n: inp.CASES[n]()[0]["images"].shape[1:] for n in inp.CASES}
    assert shapes["shape_31x33"] == (33, 31) and shapes["shape_33x31"] == (31, 33) and shapes["shape_20x14"] == (14, 20) and shapes["shape_65x33"] == (33, 65)
    assert shapes["ring"] == (64, 96)   # 3 x 2 tiles of 32 x 32


@pytest.mark.parametrize("uniq", [0, 15])
def test_the_rule_recovers_a_textured_plane(uniq):
    """fusion_inputs.stereo_ring(5): 96 x 64, a textured plane one metre away; planes depth_planes((0.8, 1.2), 32); neighbours (i - 1,
    i + 1, i - 2, i + 2); census 5 x 5, box 2, default truncation.  Per view: at least 85 % of the strict pixels kept, the median
    |z - z_true| at most 0.25 plane steps, the 95th percentile at most 0.5 — half a step is what the right plane alone guarantees
    without interpolation.  Measured over the five views: kept >= 93.8 % (u = 0) / 92.1 % (u = 15), median <= 0.100 / 0.099, 95th
    percentile <= 0.370 / 0.336 steps."""
    a, _ = inp.CASES["ring"]()
    r = reference("ring_u15" if uniq else "ring")
    V, H, W = a["images"].shape
    truth = fi.render(a["K"], a["ext"], W, H, plane=(np.array([0.0, 0.0, 1.0]), fi.STEREO_Z0), sphere=None)
    step = (inp.RING_RANGE[1] - inp.RING_RANGE[0]) / inp.RING_STEPS
    strict = ref.strict_mask(W, H, 5, 5, 2)
    for v in range(V):
        kept = strict & (r["status"][v] == 0)
        err = np.abs(r["depth"][v][kept] - truth[v][kept]) / step
        print(f"u = {uniq}, view {v}: kept {kept.sum() / strict.sum():.3f}, median {np.median(err):.3f}, 95th percentile {np.percentile(err, 95):.3f} steps")
        assert kept.sum() >= 0.85 * strict.sum() and np.median(err) <= 0.25 and np.percentile(err, 95) <= 0.5


def test_the_restatement_chain_of_reconstruct_views_keeps_the_plane():
    """What tests/test_gpu_sweep.py asks of ``reconstruct_views`` on the ring, on the restatements first (sweep_reference ->
    fusion_reference, with that function's defaults): every fused point within one plane step of the plane, and at least half of the
    strict pixels of the middle view kept."""
    a, _ = inp.CASES["ring"]()
    V, H, W = a["images"].shape
    nb = sweep.view_neighbours(a["ext"])
    r = ref.sweep(a["images"], a["K"], a["ext"], nb, a["planes"], uniqueness_ratio=15)
    f = fref.fuse(r["depth"], a["K"], a["ext"], nb, unique=False)
    step = (inp.RING_RANGE[1] - inp.RING_RANGE[0]) / inp.RING_STEPS
    m = f["mask"].astype(bool)
    off = np.abs(f["points"][m][:, 2] - fi.STEREO_Z0)
    strict = ref.strict_mask(W, H, 5, 5, 2)
    print("fused points", int(m.sum()), "largest distance from the plane", float(off.max()), "steps", float(off.max()) / step, "middle view kept", int(m[V // 2].sum()), "of", int(strict.sum()))
    assert off.max() <= step and m[V // 2].sum() >= 0.5 * strict.sum()


def test_depth_planes_is_the_hypothesis_set_of_the_line_the_reference_writes():
    """tests/golden/mvsnet_depth_lines.npz holds the numbers of the last line ``Camera.to_MVSnet_txt`` wrote (make_mvsnet_golden.py)."""
    g = np.load(GOLDEN)
    for (lo, hi, steps), (d0, interval, n, d1) in zip(g["sets"], g["lines"]):
        z = sweep.depth_planes((lo, hi), int(steps))
        assert (d0, n, d1) == (lo, steps, hi) and z.dtype == np.float64 and np.array_equal(z, d0 + np.arange(int(n)) * interval)
        zi = sweep.depth_planes((lo, hi), int(steps), "inverse")
        assert len(zi) == len(z) and np.isclose(zi[0], z[0], rtol=1e-14) and np.isclose(zi[-1], z[-1], rtol=1e-14) and np.all(np.diff(zi) > 0)
        if steps > 2:
            assert np.allclose(np.diff(1.0 / zi), np.diff(1.0 / zi)[0], rtol=1e-7)
    for bad, name in (((1.0,), "depth_range"), ((0.0, 1.0), "depth_range"), ((1.0, 1.0), "depth_range"), ((1.0, np.inf), "depth_range"), ("ab", "depth_range")):
        with pytest.raises(ValueError, match=rf"^{name}\b"):
            sweep.depth_planes(bad, 4)
    for steps in (0, 1025, 4.0, True):
        with pytest.raises(ValueError, match=r"^steps\b"):
            sweep.depth_planes((1.0, 2.0), steps)
    with pytest.raises(ValueError, match=r"^spacing\b"):
        sweep.depth_planes((1.0, 2.0), 4, "log")


# ---- argument errors: none of them needs a GPU ----------------------------------------------------------------------------------------------
def good():
    K, E = fi.ring_views(3, 8, 6, 8.0)
    return dict(n_views=3, width=8, height=6, pitch=8, K=K, ext=E, neighbours=[[1, 2], [0], []], planes=[1.0, 1.5, 2.0])


@pytest.mark.parametrize("change,name", [
    (dict(n_views=0), "images"), (dict(width=0), "images"), (dict(height=65536), "images"), (dict(pitch=7), "pitch"),
    (dict(K=np.ones((2, 4))), "K"), (dict(K=np.array([[1.0, 0, 0.0, 0]] * 3)), "K"), (dict(K=np.full((3, 4), np.inf)), "K"),
    (dict(ext=np.zeros((2, 3, 4))), "ext"), (dict(ext=np.full((3, 3, 4), np.nan)), "ext"), (dict(ext=None), "ext"),
    (dict(neighbours=[[1], [0]]), "neighbours"), (dict(neighbours=[[1], [0], [3]]), "neighbours"), (dict(neighbours=[[1], [0], [-1]]), "neighbours"),
    (dict(neighbours=[[0], [0], []]), "neighbours"), (dict(neighbours=[[1, 1], [0], []]), "neighbours"), (dict(neighbours=[[1.5], [0], []]), "neighbours"),
    (dict(neighbours=(np.array([0, 2, 1, 3]), np.array([1, 2, 0]))), "neighbours"), (dict(neighbours=(np.array([1, 2, 3, 3]), np.array([1, 2, 0]))), "neighbours"),
    (dict(neighbours=5), "neighbours"),
    (dict(planes=[]), "planes"), (dict(planes=np.ones((2, 3))), "planes"), (dict(planes=np.ones((1, 1, 3))), "planes"), (dict(planes=np.linspace(1, 2, 1025)), "planes"),
    (dict(planes=[1.0, np.nan]), "planes"), (dict(planes=[0.0, 1.0]), "planes"), (dict(planes=[-1.0, 1.0]), "planes"), (dict(planes=[1.0, np.inf]), "planes"),
    (dict(planes=[1.0, 1.0, 2.0]), "planes"), (dict(planes=[1.0, 2.0, 1.5]), "planes"), (dict(planes="abc"), "planes"),
    (dict(census=5), "census"), (dict(census=(4, 5)), "census"), (dict(census=(5, 1)), "census"), (dict(census=(9, 9)), "census"), (dict(census=(5.0, 5)), "census"),
    (dict(box=-1), "box"), (dict(box=5), "box"), (dict(box=1.0), "box"), (dict(box=True), "box"),
    (dict(truncate=0), "truncate"), (dict(truncate=24 * 25 + 1), "truncate"), (dict(truncate=2.5), "truncate"),
    (dict(uniqueness_ratio=-1), "uniqueness_ratio"), (dict(uniqueness_ratio=101), "uniqueness_ratio"), (dict(uniqueness_ratio=1.5), "uniqueness_ratio"),
    (dict(dtype=np.float16), "dtype"), (dict(dtype=np.int32), "dtype"),
])
def test_check_sweep_args_names_the_argument(change, name):
    with pytest.raises(ValueError, match=rf"^{name}\b"):
        sweep.check_sweep_args(**dict(good(), **change))


def test_check_sweep_args_accepts_and_normalises():
    K, P, start, nbr, z, cw, ch, box, tau, uniq, f32 = sweep.check_sweep_args(**good())
    assert K.shape == (3, 4) and P.shape == (3, 12) and start.dtype == nbr.dtype == np.int32 and list(start) == [0, 2, 3, 3] and list(nbr) == [1, 2, 0]
    assert z.shape == (1, 3) and z.dtype == np.float64 and (cw, ch, box, tau, uniq, f32) == (5, 5, 2, 24 * 25 // 4, 0, True)
    assert sweep.check_sweep_args(**dict(good(), planes=np.array([[3.0, 2.0], [1.0, 2.0], [5.0, 1.0]])))[4].shape == (3, 2)   # a row may fall
    assert sweep.check_sweep_args(**dict(good(), census=(9, 7), box=0, truncate=62))[8] == 62
    K18, E18 = fi.ring_views(18, 8, 6, 1.0)
    many = [[j for j in range(18) if j != i][:16] for i in range(18)]
    assert len(sweep.check_sweep_args(18, 8, 6, 8, K18, E18, many, [1.0])[3]) == 18 * 16
    many[5] = [j for j in range(18) if j != 5]
    with pytest.raises(ValueError, match="^neighbours.*17"):
        sweep.check_sweep_args(18, 8, 6, 8, K18, E18, many, [1.0])


def test_sweep_depth_maps_refuses_bad_inputs_before_the_device():
    a, _ = inp.CASES["shape_20x14"]()
    I, K, E, nb, z = a["images"], a["K"], a["ext"], a["neighbours"], a["planes"]
    for args, kw, name in (((I[0], K, E, nb, z), {}, "images"), ((I.astype(np.int16), K, E, nb, z), {}, "images"), ((I, K[:4], E, nb, z), {}, "K"),
                           ((I, K, E, nb, z[::-1] * 0), {}, "planes"), ((I, K, E, nb, z), dict(box=9), "box"), ((I, K, E, nb, z), dict(dtype=np.int8), "dtype")):
        with pytest.raises(ValueError, match=rf"^{name}\b"):
            sweep.sweep_depth_maps(*args, **kw)


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 126
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    K, E = fi.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    ARG = _capi.PCS_ERR_ARG
    assert lib.pcs_sweep_create(None, 0) == ARG and lib.pcs_sweep_destroy(None) == _capi.PCS_OK
    bad_K, bad_P = K.copy(), P.copy()
    bad_K[1, 2], bad_P[0, 7] = 0.0, np.nan
    for args, word in (((0, 8, 6, dp(K), dp(P)), "n_views"), ((3, 0, 6, dp(K), dp(P)), "width"), ((3, 8, 65536, dp(K), dp(P)), "height"), ((3, 8, 6, None, dp(P)), "K"),
                       ((3, 8, 6, dp(K), None), "P"), ((3, 8, 6, dp(bad_K), dp(P)), "K of view 1"), ((3, 8, 6, dp(K), dp(bad_P)), "P of view 0"),
                       ((3, 8, 6, dp(K), dp(P)), "NULL handle")):
        assert lib.pcs_sweep_set_views(None, *args) == ARG and "pcs_sweep_set_views" in _err() and word in _err(), (word, _err())
    too_many = np.concatenate([[0], np.full(3, 17)])
    for start, nbr, n, word in (([0, 1, 2, 3], [1, 0, 0], 0, "n 0"), (None, [1], 3, "nbr_start"), ([0, 2, 1, 3], [1, 2, 0], 3, "non-decreasing"),
                                (too_many, np.arange(17) % 3, 3, "more than 16"), ([0, 1, 2, 3], None, 3, "nbr must be given"), ([0, 1, 2, 3], [1, 0, 3], 3, "outside"),
                                ([0, 1, 2, 3], [1, 1, 0], 3, "own neighbour"), ([0, 2, 2, 3], [1, 1, 0], 3, "twice"), ([0, 1, 2, 3], [1, 0, 0], 3, "NULL handle")):
        rc = lib.pcs_sweep_set_neighbours(None, None if start is None else ip(start), None if nbr is None else ip(nbr), n)
        assert rc == ARG and "pcs_sweep_set_neighbours" in _err() and word in _err(), (word, _err())
    # pcs_sweep_run: (d_images, pitch, z, n_z, D, census_w, census_h, box_radius, truncate, uniqueness_ratio, d_depth, depth_dtype, d_level, d_cost, d_status, stream)
    z3 = np.array([1.0, 1.5, 2.0])
    ok = dict(d_images=64, pitch=8, z=dp(z3), n_z=1, D=3, census_w=5, census_h=5, box_radius=2, truncate=150, uniqueness_ratio=0, d_depth=64, depth_dtype=1, d_level=None,
              d_cost=None, d_status=None, stream=None)
    for change, word in ((dict(d_images=None), "d_images"), (dict(n_z=0), "n_z"), (dict(D=0), "D 0"), (dict(D=1025), "D 1025"), (dict(z=None), "z (n_z, D)"),
                         (dict(z=dp([1.0, np.nan, 2.0])), "finite"), (dict(z=dp([1.0, 0.0, 2.0])), "finite and > 0"), (dict(z=dp([1.0, 1.0, 2.0])), "monotone"),
                         (dict(z=dp([1.0, 2.0, 1.5])), "monotone"), (dict(census_w=4), "census_w"), (dict(census_h=1), "census_h"), (dict(census_w=9, census_h=9), "bits"),
                         (dict(box_radius=-1), "box_radius"), (dict(box_radius=5), "box_radius"), (dict(truncate=0), "truncate"), (dict(truncate=601), "truncate"),
                         (dict(uniqueness_ratio=101), "uniqueness_ratio"), (dict(depth_dtype=2), "depth_dtype"), (dict(d_depth=None), "d_depth"), (dict(), "NULL handle")):
        a = dict(ok, **change)
        assert lib.pcs_sweep_run(None, *a.values()) == ARG and "pcs_sweep_run" in _err() and word in _err(), (word, _err())
    f = ctypes.c_float()
    assert lib.pcs_sweep_last_kernel_ms(None, ctypes.byref(f)) == ARG
    if lib.pcs_device_count() == 0:   # no device: no handle, and never a CPU fallback
        with pytest.raises(_capi.PcsError) as e:
            sweep.PlaneSweeper(0)
        assert e.value.code == _capi.PCS_ERR_NODEVICE
