"""The ray-cast rule without a GPU: the two forms of the NumPy restatement (tests/raycast_reference.py) against each other, the margins of
every input set of the device tests (tests/raycast_inputs.py), the properties that make the rule a rendering of the surface (a plane
comes back at its depth with its normal, a sphere near the analytic depth with radial normals, a spurious depth is seen through, an
integrated view is reproduced, the step does not matter), and the host-side argument checks of pycamset_amd/volume.py and the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

from pycamset_amd import _capi, volume
from tests import fusion_inputs as fi
from tests import raycast_inputs as inp
from tests import raycast_reference as ray
from tests import tsdf_inputs as ti

MARGIN = inp.MARGIN
ALL = list(inp.CASES) + ["translated_plane"]
DIAGONAL = np.sqrt(3.0) * 0.04   # of a cell of the sphere grid: 0.0693

# The restatement's own median angle (degrees) between the normal and the radial direction over the hits with a normal, per sphere
# case and render view (generic, inside), as test_the_sphere_comes_back_near_the_analytic_depth_with_radial_normals printed them; the
# test asserts twice these ("Ray-cast of the TSDF volume").
MEDIAN_ANGLE = {("sphere_008", 0): 1.02, ("sphere_008", 1): 1.04, ("sphere_012", 0): 1.14, ("sphere_012", 1): 0.95}


def get(name):
    return inp.translated_plane()[0] if name == "translated_plane" else inp.CASES[name]()


@functools.lru_cache(maxsize=None)
def cast(name, k):
    case = get(name)
    return inp.cast_reference(case, inp.integrated(name), case["views"][k])


def rays(view):
    """World centre and direction (per unit z-depth) of every pixel: (3,), (H, W, 3)."""
    K, E = view["K"][0], view["ext"][0]
    xs, ys = np.meshgrid(np.arange(view["width"], dtype=np.float64), np.arange(view["height"], dtype=np.float64))
    r = np.stack([(xs - K[1]) / K[0], (ys - K[3]) / K[2], np.ones_like(xs)], axis=-1)
    return -E[:, :3].T @ E[:, 3], r @ E[:, :3]


@pytest.mark.parametrize("name", ALL)
def test_the_two_forms_agree_exactly(name):
    """Every pixel of the small views; every seventh pixel of the 40 x 30 views (7 and 40 share no factor: all columns are met)."""
    case, vol = get(name), inp.integrated(name)
    for k, view in enumerate(case["views"]):
        want = cast(name, k)
        rows = ray.render_rows(view["K"], view["ext"])
        W, H = view["width"], view["height"]
        picked = range(0, W * H, 7 if W * H > 200 else 1)
        for p in picked:
            y, x = divmod(p, W)
            d, n, st, closest = ray.raycast_pixel(vol, rows[0], x, y, case["min_weight"], case["step"], case["z_near"], case["z_far"])
            assert st == want["status"][0, y, x], (name, k, x, y)
            assert np.array_equal(np.array([d, *n]), np.array([want["depth"][0, y, x], *want["normal"][0, y, x]]), equal_nan=True), (name, k, x, y)
            assert closest == want["closest"][0, y, x], (name, k, x, y)


@pytest.mark.parametrize("name", ALL)
def test_no_decision_of_an_input_set_sits_near_its_threshold(name):
    case = get(name)
    worst = min(float(cast(name, k)["closest"].min()) for k in range(len(case["views"])))
    print(f"{name}: closest call {worst:.2e} (needed {MARGIN * inp.RAY_DECISION_GAP:.2e})")
    assert worst >= MARGIN * inp.RAY_DECISION_GAP


def test_the_gaps_are_the_restatements_own():
    g, ng, dg = inp.measure_gaps()
    print(f"RAY_GAP measured {g[0]:.2e} ({g[1]}), recorded {inp.RAY_GAP:.2e}; RAY_NORMAL_GAP measured {ng[0]:.2e} ({ng[1]}), recorded {inp.RAY_NORMAL_GAP:.2e}; "
          f"RAY_DECISION_GAP measured {dg[0]:.2e} ({dg[1]}), recorded {inp.RAY_DECISION_GAP:.2e}")
    assert g[0] <= inp.RAY_GAP <= 2 * g[0] and ng[0] <= inp.RAY_NORMAL_GAP <= 2 * ng[0] and dg[0] <= inp.RAY_DECISION_GAP <= 2 * dg[0]


def test_cases_cover_what_the_kernel_branches_on():
    assert set(inp.VOLUMES) <= set(ti.CASES) and inp.CASES["noisy"]()["volume"]["sum_dtype"] == np.float32 and inp.CASES["noisy_sum_f64"]()["volume"]["sum_dtype"] == np.float64
    seen = np.zeros(4, dtype=np.int64)
    for name in ALL:
        case = get(name)
        assert [(v["width"], v["height"]) for v in case["views"]][:3] == [(40, 30), (13, 7), (1, 1)]   # no width a multiple of 8; 40 x 30 is six workgroups
        for k in range(len(case["views"])):
            seen += np.bincount(cast(name, k)["status"].reshape(-1), minlength=4)
        o, s, d = np.array(case["volume"]["origin"]), case["volume"]["voxel"], np.array(case["volume"]["dims"])
        C, _ = rays(case["views"][1])
        assert np.all(C > o) and np.all(C < o + s * (d - 1)) or min(d) < 2   # the second view starts inside the box
    assert np.all(seen > 100)   # every status, often
    assert all((cast("dims_1x9x9", k)["status"] == ray.MISSED).all() for k in range(3))                                  # no cells
    assert all(np.isin(cast("empty_list", k)["status"], (ray.NO_CROSSING, ray.MISSED)).all() for k in range(3))          # an empty volume
    assert (cast("empty_list", 1)["status"] == ray.NO_CROSSING).all()
    assert get("dims_2x2x2")["volume"]["dims"] == (2, 2, 2) and (cast("dims_2x2x2", 1)["status"] == ray.NO_NORMAL).any()   # one cell: a hit, never a normal
    assert {get(n)["step"] is None for n in ALL} == {True, False} and get("plane")["z_near"] > 0 and np.isfinite(get("plane")["z_far"])
    assert get("dims_33x17x5")["step"] == get("dims_33x17x5")["volume"]["voxel"] / 64.0   # the smallest step the host admits
    # the axis view of the translated plane: the column x = cx runs in a plane x = const
    case = get("translated_plane")
    view = case["views"][3]
    _, w = rays(view)
    assert np.array_equal(view["ext"][0][:, :3], np.eye(3)) and np.all(w[:, 20, 0] == 0.0) and np.all(w[:, 19, 0] != 0.0)
    assert (cast("translated_plane", 3)["status"][:, 20] == ray.HIT).sum() >= 5


def test_a_translated_plane_comes_back_at_its_depth_with_its_normal():
    """min_weight 4 on the float64 volume of four purely translated cameras.  In the R = I view the z-depth of a hit IS the world z: it
    must be c; in the rotated views the hit point's world z must be.  The blend of a field that is linear in z is linear, so the only
    error is rounding.  Normals are (0, 0, -1): outside is where the cameras are."""
    case, c = inp.translated_plane()
    assert case["min_weight"] == 4 and case["volume"]["sum_dtype"] == np.float64
    hits = 0
    for k, view in enumerate(case["views"]):
        r = cast("translated_plane", k)
        hit = r["status"][0] <= ray.NO_NORMAL
        C, w = rays(view)
        z = C[2] + r["depth"][0][hit] * w[hit][:, 2]
        worst = float(np.max(np.abs(z - c)) / c) if hit.any() else 0.0
        got = r["normal"][0][r["status"][0] == ray.HIT]
        worst_n = float(np.max(np.abs(got - (0.0, 0.0, -1.0)))) if len(got) else 0.0
        print(f"view {k}: {int(hit.sum())} hits, worst |z - c| / c {worst:.2e} (bound {MARGIN * inp.RAY_GAP:.2e}), {len(got)} normals, worst deviation {worst_n:.2e} (bound {MARGIN * inp.RAY_NORMAL_GAP:.2e})")
        assert worst <= MARGIN * inp.RAY_GAP and worst_n <= MARGIN * inp.RAY_NORMAL_GAP
        if k == 3:
            assert np.max(np.abs(r["depth"][0][hit] - c)) <= MARGIN * inp.RAY_GAP * c and hit.sum() >= 88
        hits += int(hit.sum())
    assert hits >= 300


@pytest.mark.parametrize("name", ["sphere_008", "sphere_012"])
def test_the_sphere_comes_back_near_the_analytic_depth_with_radial_normals(name):
    case = get(name)
    centre, _ = fi.SPHERE
    for k, view in enumerate(case["views"]):
        r = cast(name, k)
        truth = fi.render(view["K"], view["ext"], view["width"], view["height"], plane=None)[0]
        hit = r["status"][0] <= ray.NO_NORMAL
        assert hit.any() and np.all(np.isfinite(truth[hit]))
        err = float(np.max(np.abs(r["depth"][0][hit] - truth[hit])))
        C, w = rays(view)
        full = r["status"][0] == ray.HIT
        X = C + r["depth"][0][full][:, None] * w[full]
        radial = (X - centre) / np.linalg.norm(X - centre, axis=1, keepdims=True)
        dots = np.sum(r["normal"][0][full] * radial, axis=1)
        angle = np.degrees(np.arccos(np.clip(dots, -1.0, 1.0)))
        med = float(np.median(angle)) if len(angle) else 0.0
        print(f"{name} view {k}: {int(hit.sum())} hits, worst depth error {err:.4f} (bound {DIAGONAL:.4f}); {len(angle)} normals, median angle {med:.2f} deg, max {float(angle.max()) if len(angle) else 0.0:.2f} deg")
        assert err <= DIAGONAL and np.all(dots > 0)
        if (name, k) in MEDIAN_ANGLE:
            assert len(angle) >= 20 and med <= 2.0 * MEDIAN_ANGLE[(name, k)]


@functools.lru_cache(maxsize=None)
def free_space_scene():
    """The ray of the centre pixel of view 2's patch (tests/fusion_inputs.py PATCHES: its depths are 0.75 of the true ones), and a grid
    of 0.03 around the stretch of that ray from the spurious surface to the true one."""
    case, _, v = ti.free_space_node()
    D, K, E = case["depth"], case["K"], case["ext"]
    _, y0, y1, x0, x1, factor = fi.PATCHES[1]
    x, y = (x0 + x1) // 2, (y0 + y1) // 2
    view = dict(width=64, height=48, K=K[v:v + 1], ext=E[v:v + 1])
    C, w = rays(view)
    ends = np.stack([C + D[v, y, x] * w[y, x], C + D[v, y, x] / factor * w[y, x]])
    voxel = 0.03
    origin, dims = volume.grid_from_bounds([ends.min(axis=0) - 4.3 * voxel, ends.max(axis=0) + 4.3 * voxel], voxel)
    return dict(case, origin=tuple(origin), voxel=voxel, dims=dims, trunc=0.09), v, x, y, D[v, y, x], D[v, y, x] / factor


def test_views_that_see_through_a_spurious_depth_show_the_true_surface():
    """Cast from the patch's own view: with all ten views integrated (min_weight 2) the centre pixel's ray passes the spurious surface,
    which the other views see through, and hits the true one; with that view alone (min_weight 1) it hits the spurious one."""
    case, v, x, y, spurious, true = free_space_scene()
    assert max(case["dims"]) <= 33 and true - spurious > 10 * case["voxel"]
    row = ray.render_rows(case["K"][v:v + 1], case["ext"][v:v + 1])[0]
    diagonal = np.sqrt(3.0) * case["voxel"]
    vol, _ = ti.run_reference(case)
    d_all, _, st_all, closest_all = ray.raycast_pixel(vol, row, x, y, 2)
    vol1, _ = ti.run_reference(dict(case, views=(v,)))
    d_one, _, st_one, closest_one = ray.raycast_pixel(vol1, row, x, y, 1)
    print(f"spurious {spurious:.4f}, true {true:.4f}; all views: {d_all:.4f} (status {st_all}); view {v} alone: {d_one:.4f} (status {st_one})")
    assert st_all <= ray.NO_NORMAL and abs(d_all - true) <= diagonal
    assert st_one <= ray.NO_NORMAL and abs(d_one - spurious) <= diagonal
    assert min(closest_all, closest_one) >= MARGIN * inp.RAY_DECISION_GAP


def test_casting_an_integrated_view_reproduces_its_depth_map():
    """The noise-free sphere ring: every hit of view v is within one cell diagonal of D_v."""
    case = get("sphere_008")
    D, K, E = case["volume"]["depth"], case["volume"]["K"], case["volume"]["ext"]
    V, H, W = D.shape
    r = ray.raycast(inp.integrated("sphere_008"), K, E, W, H, 2)
    hit = r["status"] <= ray.NO_NORMAL
    err = np.abs(r["depth"][hit] - D[hit])
    print(f"{int(hit.sum())} hits over {V} views, worst |model - D| {err.max():.4f} (bound {DIAGONAL:.4f}), median {np.median(err):.4f}")
    assert np.all(hit.sum(axis=(1, 2)) >= 300) and np.all(np.isfinite(D[hit])) and err.max() <= DIAGONAL


@pytest.mark.parametrize("name", ["sphere_008", "sphere_012"])
def test_halving_the_step_moves_no_hit_by_a_cell_diagonal(name):
    """On the noise-free sphere, whose band of negative values is everywhere thicker than the step.  (On the noisy ring a grazing ray can
    step over a sliver thinner than the step and hit the plane behind it: a property of any fixed step, not held here.)"""
    case, vol = get(name), inp.integrated(name)
    diagonal = np.sqrt(3.0) * case["volume"]["voxel"]
    for k, view in enumerate(case["views"][:2]):
        a = cast(name, k)
        b = inp.cast_reference(dict(case, step=0.5 * (case["step"] or case["volume"]["voxel"])), vol, view)
        both = (a["status"] <= ray.NO_NORMAL) & (b["status"] <= ray.NO_NORMAL)
        moved = np.abs(a["depth"][both] - b["depth"][both])
        print(f"{name} view {k}: {int(both.sum())} hits in both, moved by at most {moved.max():.5f} (bound {diagonal:.4f})")
        assert both.sum() >= 40 and moved.max() <= diagonal


def test_check_raycast_args_refuses_each_bad_argument_by_name():
    K, E = fi.ring_views(3, 8, 6, 8.0)
    ok = dict(n_views=3, width=8, height=6, K=K, ext=E, voxel=0.04)
    Ka, P, mw, step, zn, zf, f32 = volume.check_raycast_args(**ok)
    assert Ka.shape == (3, 4) and P.shape == (3, 12) and (mw, step, zn, zf, f32) == (2, 0.04, 0.0, np.inf, True)
    assert volume.check_raycast_args(**ok, dtype=np.float64)[6] is False and volume.check_raycast_args(**ok, step=0.04 / 64.0)[3] == 0.04 / 64.0
    bad_K = K.copy()
    bad_K[1, 2] = 0.0
    for change, word in ((dict(n_views=0, K=K[:0], ext=E[:0]), "K"), (dict(width=0), "width"), (dict(width=65536), "width"), (dict(height=0), "height"), (dict(height=2.0), "height"),
                         (dict(K=bad_K), "K"), (dict(K=K[:, :3]), "K"), (dict(K=np.where(K > 0, np.nan, K)), "K"), (dict(ext=E[:2]), "ext"), (dict(min_weight=0), "min_weight"),
                         (dict(min_weight=65536), "min_weight"), (dict(min_weight=1.5), "min_weight"), (dict(min_weight=True), "min_weight"), (dict(step=0.0), "step"),
                         (dict(step=-0.01), "step"), (dict(step=np.nan), "step"), (dict(step=np.inf), "step"), (dict(step=0.04 / 65.0), "step"), (dict(z_near=-0.1), "z_near"),
                         (dict(z_near=np.nan), "z_near"), (dict(z_near=1.0, z_far=1.0), "z_near"), (dict(z_near=2.0, z_far=1.0), "z_near"), (dict(z_near=np.inf), "z_near"),
                         (dict(z_far=np.nan), "z_far"), (dict(z_far="far"), "z_far"), (dict(dtype=np.float16), "dtype"), (dict(voxel=0.0), "voxel")):
        with pytest.raises(ValueError) as e:
            volume.check_raycast_args(**dict(ok, **change))
        assert word in str(e.value), (change, str(e.value))
    for f in (lambda: volume.raycast_views(None, K, E, 8, 6), lambda: volume.depth_residuals(None, np.ones((3, 6, 8)), K, E)):
        with pytest.raises(ValueError) as e:
            f()
        assert "volume" in str(e.value)   # the volume is looked at first: without one nothing touches the device
    with pytest.raises(ValueError) as e:
        volume.depth_residuals(None, np.ones((6, 8)), K, E)
    assert "depth" in str(e.value)


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 128
    assert (_capi.TSDF_RAY_HIT, _capi.TSDF_RAY_NO_NORMAL, _capi.TSDF_RAY_NO_CROSSING, _capi.TSDF_RAY_MISSED) == (ray.HIT, ray.NO_NORMAL, ray.NO_CROSSING, ray.MISSED)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    K, E = fi.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    bad_K = K.copy()
    bad_K[1, 2] = 0.0
    bad_P = P.copy()
    bad_P[2, 5] = np.inf
    ARG = _capi.PCS_ERR_ARG
    good = dict(n=3, w=8, h=6, K=dp(K), P=dp(P), mw=2, step=0.04, zn=0.0, zf=np.inf, depth=64, dt=1, normal=64, status=64, flags=0)
    for change, word in ((dict(n=0), "n_views"), (dict(n=32768), "n"), (dict(w=0), "width"), (dict(h=65536), "height"), (dict(K=None), "K"), (dict(K=dp(bad_K)), "K of view 1"),
                         (dict(P=None), "P"), (dict(P=dp(bad_P)), "P of view 2"), (dict(mw=0), "min_weight"), (dict(mw=65536), "min_weight"), (dict(step=0.0), "step"),
                         (dict(step=np.nan), "step"), (dict(step=np.inf), "step"), (dict(zn=-1.0), "z_near"), (dict(zn=np.nan), "z_near"), (dict(zn=1.0, zf=1.0), "z_near"),
                         (dict(zf=np.nan), "z_far"), (dict(depth=None), "d_depth"), (dict(dt=2), "depth_dtype"), (dict(flags=2), "flags"), (dict(), "NULL handle"),
                         (dict(normal=None, status=None, flags=1), "NULL handle")):
        a = dict(good, **change)
        rc = lib.pcs_tsdf_raycast(None, a["n"], a["w"], a["h"], a["K"], a["P"], a["mw"], a["step"], a["zn"], a["zf"], a["depth"], a["dt"], a["normal"], a["status"], a["flags"], None)
        assert rc == ARG and word in _err(), (change, word, _err())
    f = ctypes.c_float()
    assert lib.pcs_tsdf_raycast_last_kernel_ms(None, ctypes.byref(f), ctypes.byref(f)) == ARG
