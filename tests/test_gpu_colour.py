"""The colour of surface points on the device (pycamset_amd/volume.py, csrc/ba_tsdf_colour.hpp) against the NumPy restatement
(tests/colour_reference.py).

``count`` and ``best`` and the uint8 colours must be IDENTICAL to the restatement's: tests/test_colour_reference.py asserts for every
input set used here (tests/colour_inputs.py) that no decision of the rule, the rounding to uint8 included, lies within MARGIN x
COLOUR_DECISION_GAP of its threshold.  Float32 colours and weights are held to MARGIN x COLOUR_GAP relative to the case's largest value
(the restatement's own float64-versus-longdouble gap) plus one rounding to float32 (2^-24 of the value); point normals to MARGIN x
COLOUR_NORMAL_GAP + 2^-24.  With contraction off the expectation is bit equality with the restatement's value rounded once, and the
number of values that differ from it is printed."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, volume
from tests import colour_inputs as inp
from tests import colour_reference as col
from tests import fusion_inputs as fi
from tests import raycast_inputs as ri
from tests import tsdf_reference as tref

pytestmark = pytest.mark.gpu
MARGIN = inp.MARGIN
F32 = 2.0 ** -24
ALL = list(inp.CASES)
OUT = (np.uint8, np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    r = inp.run_reference(inp.get(name), mode)
    for key in ("colour", "weight", "count", "best"):
        r[key].setflags(write=False)
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run(case, mode, dtype, **kw):
    a = dict(normals=case["normals"], visibility=case["visibility"], occlusion_tol=case["occlusion_tol"] if case["visibility"] is not None else None, cos_min=case["cos_min"], mode=mode,
             fill=case["fill"], dtype=dtype, info=True)
    a.update(kw)
    return volume.colour_points(case["points"], case["images"], case["K"], case["ext"], **a)


def compare(got, want, dtype, what):
    colour, weight, count, best = got
    shape = want["count"].shape
    assert colour.dtype == dtype and weight.dtype == np.float32 and count.dtype == np.uint16 and best.dtype == np.int32
    assert colour.shape == want["colour"].shape and weight.shape == count.shape == best.shape == shape, what
    assert np.array_equal(count, want["count"]) and np.array_equal(best, want["best"]), (what, int((count != want["count"]).sum()), int((best != want["best"]).sum()))
    ref = col.to_output(want["colour"], dtype)
    big_w = float(np.max(np.abs(want["weight"]))) if want["weight"].size else 0.0
    wgap = np.abs(weight.astype(np.float64) - want["weight"])
    assert np.all(wgap <= MARGIN * inp.COLOUR_GAP * big_w + F32 * np.abs(want["weight"])), what
    if dtype == np.uint8:
        assert np.array_equal(colour, ref), (what, int((colour != ref).sum()))
        differ = 0
    else:
        finite = np.isfinite(want["colour"])
        assert np.array_equal(np.isnan(colour), np.isnan(ref)), what
        big = float(np.max(np.abs(want["colour"][finite]))) if finite.any() else 0.0
        gap = np.abs(colour.astype(np.float64)[finite] - want["colour"][finite])
        assert np.all(gap <= MARGIN * inp.COLOUR_GAP * big + F32 * np.abs(want["colour"][finite])), (what, float(gap.max()))
        differ = int((bits(colour).reshape(-1, 4) != bits(ref).reshape(-1, 4)).any(axis=1).sum())
    differ_w = int((bits(weight).reshape(-1, 4) != bits(want["weight"].astype(np.float32)).reshape(-1, 4)).any(axis=1).sum())
    print(f"{what}: {count.size} points, {int((count > 0).sum())} coloured; values that are not the restatement's rounded once: colour {differ}, weight {differ_w}")


@pytest.mark.parametrize("name", ALL)
def test_every_case_mode_and_dtype_against_the_restatement(name):
    """The textured plane's mesh, the plane and sphere with and without maps and normals, float32 maps, NaN points, NaN normals and
    every kind of invalid map entry, the facing pair, the views that share nothing, one view, 40 views, images of 2 x 2, channels 1, 3
    and 4 of uint8 and float32, float32 points, N = 0, 1, 63, 64, 65 and 257; both modes; uint8 and float32 out."""
    case = inp.get(name)
    for mode in col.MODES:
        want = reference(name, mode)
        for dtype in OUT:
            compare(run(case, mode, dtype), want, dtype, f"{name} {mode} {np.dtype(dtype).name}")
    only = run(case, "blend", np.uint8, info=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, col.to_output(reference(name, "blend")["colour"], np.uint8))


def source(case, images, colour, **ptrs):
    """The ``src`` of the thin calls for a case: ``images`` and ``colour`` tensors on the device."""
    a = volume.check_colour_args(case["images"], case["K"], case["ext"], occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], fill=case["fill"],
                                 dtype=str(colour.dtype).replace("torch.", ""))
    return dict(a, d_images=images.data_ptr(), pitch=images.stride(1) * images.element_size(), d_colour=colour.data_ptr(), **ptrs)


@pytest.mark.parametrize("name", ["views_40", "views_40_c1_float32", "image_2x2"])
def test_a_pitch_larger_than_the_row_and_optional_outputs(name):
    """The images inside a wider buffer whose padding holds other values: the same bits; weight, count and best may each be NULL."""
    case = inp.get(name)
    V, H, W, C = case["images"].shape
    wide = torch.from_numpy(np.full((V, H, W + 5, C), 77, dtype=case["images"].dtype)).cuda()
    wide[:, :, :W] = torch.from_numpy(case["images"]).cuda()
    X, n = torch.from_numpy(case["points"]).cuda(), torch.from_numpy(case["normals"]).cuda()
    want = run(case, "blend", np.float32, visibility=None, occlusion_tol=None)
    vol = volume.TsdfVolume(0)
    N = len(X)
    for skip in (None, "d_weight", "d_count", "d_best"):
        out = dict(colour=torch.zeros((N, C), dtype=torch.float32, device="cuda"), d_weight=torch.zeros(N, dtype=torch.float32, device="cuda"),
                   d_count=torch.zeros(N, dtype=torch.uint16, device="cuda"), d_best=torch.zeros(N, dtype=torch.int32, device="cuda"))
        src = source(case, wide[:, :, :W], out["colour"], **{k: (None if k == skip else t.data_ptr()) for k, t in out.items() if k != "colour"})
        assert src["pitch"] == (W + 5) * C * wide.element_size()
        vol.colour_points(N, X.data_ptr(), False, n.data_ptr(), src)
        torch.cuda.synchronize()
        for key, w in zip(("colour", "d_weight", "d_count", "d_best"), want):
            assert np.array_equal(bits(out[key].cpu().numpy()), bits(w if key != skip else np.zeros_like(w))), (name, skip, key)
    ms = vol.colour_last_kernel_ms()
    assert np.isnan(ms[0]) and ms[1] > 0
    vol.close()


def device_volume(name):
    """A handle whose volume holds the bits of the restatement's."""
    case, want = inp.get(name), inp.integrated(inp.get(name))
    vc = case["volume"]
    vol = volume.TsdfVolume(0)
    vol.set_grid(vc["origin"], vc["voxel"], vc["dims"], want.sum.dtype == np.float32)
    s, w = vol.volume()
    s.copy_(torch.from_numpy(want.sum.copy()))
    w.view(torch.int16).copy_(torch.from_numpy(want.weight.copy().view(np.int16)))
    torch.cuda.synchronize()
    return case, vol


@pytest.mark.parametrize("name", inp.VOLUME_CASES)
def test_point_normals_against_the_restatement(name):
    """Mesh vertices, surface points, points outside the box and a NaN point; float64 and float32 points."""
    case, vol = device_volume(name)
    X = inp.normal_points(name)
    for dtype in (np.float64, np.float32):
        P = X.astype(dtype)
        want = col.point_normals(inp.integrated(case), P, 2)
        normals, status = volume.vertex_normals(vol, P, 2, status=True)
        assert normals.dtype == np.float32 and normals.shape == (len(X), 3) and status.dtype == np.uint8
        assert np.array_equal(status, want["status"]) and np.array_equal(np.isnan(normals), np.isnan(want["normal"])) and np.array_equal(np.isnan(normals[:, 0]), status == 1)
        has = status == 0
        gap = float(np.max(np.abs(normals[has].astype(np.float64) - want["normal"][has])))
        differ = int((bits(normals[has]) != bits(want["normal"][has].astype(np.float32))).any(axis=1).sum())
        print(f"{name} {np.dtype(dtype).name}: {int(has.sum())} of {len(X)} with a normal, gap {gap:.2e} (bound {MARGIN * inp.COLOUR_NORMAL_GAP + F32:.2e}), {differ} not the restatement's rounded once")
        assert has.sum() >= 100 and gap <= MARGIN * inp.COLOUR_NORMAL_GAP + F32
    assert np.array_equal(bits(volume.vertex_normals(vol, X, 2)), bits(volume.vertex_normals(vol, X, 2, status=True)[0]))
    assert volume.vertex_normals(vol, X[:0], 2).shape == (0, 3)
    assert np.isnan(volume.vertex_normals(vol, X, 60000)).all()   # no node was seen that often
    vol.close()


@pytest.mark.parametrize("name", ["sphere_008", "noisy"])
def test_point_normals_at_the_hit_points_of_a_cast_are_the_casts_normals(name):
    """Both go through the same T(g).  The cast takes g = gc + z gw and the point normals g = ((C + z w) - o) / s, which can differ in the
    last place of a double; the normals are stored as float32."""
    case, want = ri.CASES[name](), ri.integrated(name)
    vol = volume.TsdfVolume(0)
    vol.set_grid(case["volume"]["origin"], case["volume"]["voxel"], case["volume"]["dims"], want.sum.dtype == np.float32)
    s, w = vol.volume()
    s.copy_(torch.from_numpy(want.sum.copy()))
    w.view(torch.int16).copy_(torch.from_numpy(want.weight.copy().view(np.int16)))
    torch.cuda.synchronize()
    hits = 0
    for view in case["views"][:2]:
        depth, normal, status = volume.raycast_views(vol, view["K"], view["ext"], view["width"], view["height"], min_weight=case["min_weight"], step=case["step"], z_near=case["z_near"],
                                                     z_far=case["z_far"], dtype=np.float64, status=True)
        X, live = col.view_points(view["K"], view["ext"], view["width"], view["height"], depth)
        got, st = volume.vertex_normals(vol, X[live], case["min_weight"], status=True)
        assert np.array_equal(st, status[live]) and np.array_equal(bits(got), bits(normal[live]))
        hits += int((st == 0).sum())
    assert hits >= 100
    vol.close()


def views_call(case, vol, name, k, mode, dtype, depth=None, normal=None):
    view = case["render"][k]
    d, n = inp.render_inputs(name, k)
    d, n = (d if depth is None else depth), (n if normal is None else normal)
    R, H, W, C = 1, view["height"], view["width"], case["images"].shape[3]
    dev = dict(depth=torch.from_numpy(np.ascontiguousarray(d)).cuda(), normal=torch.from_numpy(np.ascontiguousarray(n)).cuda(), images=torch.from_numpy(case["images"]).cuda(),
               vis=torch.from_numpy(np.array(inp.model_depth(case["volume_key"]))).cuda())
    out = dict(colour=torch.zeros((R, H, W, C), dtype=getattr(torch, np.dtype(dtype).name), device="cuda"), d_weight=torch.zeros((R, H, W), dtype=torch.float32, device="cuda"),
               d_count=torch.zeros((R, H, W), dtype=torch.uint16, device="cuda"), d_best=torch.zeros((R, H, W), dtype=torch.int32, device="cuda"))
    src = source(case, dev["images"], out["colour"], d_visibility=dev["vis"].data_ptr(), visibility_f32=True, **{k_: t.data_ptr() for k_, t in out.items() if k_ != "colour"})
    src["mode"] = mode
    vol.colour_views(W, H, view["K"], view["ext"].reshape(1, 12), dev["depth"].data_ptr(), dev["depth"].dtype == torch.float32, dev["normal"].data_ptr(), src)
    torch.cuda.synchronize()
    return tuple(out[key].cpu().numpy() for key in ("colour", "d_weight", "d_count", "d_best"))


@pytest.mark.parametrize("name", inp.VOLUME_CASES)
def test_colour_views_against_the_restatement_and_against_colour_points(name):
    """Render views of 40 x 30 (six workgroups, no side a multiple of the tile), 13 x 7 from inside the box and 1 x 1; the depth and
    normal maps are the restatement's cast, the visibility the model's own depth.  The same call on the points C + z w of the
    restatement through ``colour_points`` returns the same bits; a float64 depth map gives the rule's value for it."""
    case = inp.get(name)
    vol = volume.TsdfVolume(0)
    for k, view in enumerate(case["render"]):
        depth, normal = inp.render_inputs(name, k)
        X, live = col.view_points(view["K"], view["ext"], view["width"], view["height"], depth)
        X = np.where(live[..., None], X, np.nan).reshape(-1, 3)
        for mode in col.MODES:
            want = inp.run_views_reference(case, name, k, mode)
            for dtype in OUT:
                got = views_call(case, vol, name, k, mode, dtype)
                compare(got, want, dtype, f"{name} render view {k} {mode} {np.dtype(dtype).name}")
                pts = volume.colour_points(X, case["images"], case["K"], case["ext"], normals=normal.reshape(-1, 3), visibility=np.array(inp.model_depth(case["volume_key"])),
                                           occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], mode=mode, fill=case["fill"], dtype=dtype, info=True)
                for a, b in zip(got, pts):
                    assert np.array_equal(bits(a.reshape(b.shape)), bits(b)), (name, k, mode)
        d64 = depth.astype(np.float64) * (1.0 + 2.0 ** -30)   # not a float32: the float64 map is read as it is
        got = views_call(case, vol, name, k, "blend", np.float32, depth=d64)
        want = col.colour_views(view["K"], view["ext"], view["width"], view["height"], d64, case["K"], case["ext"], case["width"], case["height"], case["images"], normal_map=normal,
                                visibility=inp.model_depth(case["volume_key"]), occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], fill=case["fill"])
        assert np.array_equal(got[2], want["count"]) and np.array_equal(got[3], want["best"])
    vol.close()


@pytest.mark.parametrize("name", ["plane_sphere", "views_40_c4_float32"])
def test_two_runs_and_the_numpy_and_tensor_routes_return_identical_bits(name):
    case = inp.get(name)
    for mode in col.MODES:
        a, b = run(case, mode, np.float32), run(case, mode, np.float32)
        dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
        t = volume.colour_points(dev(case["points"]), dev(case["images"]), case["K"], case["ext"], normals=dev(case["normals"]), visibility=dev(case["visibility"]),
                                 occlusion_tol=case["occlusion_tol"], cos_min=case["cos_min"], mode=mode, fill=case["fill"], dtype=np.float32, info=True)
        assert all(isinstance(x, np.ndarray) for x in a) and all(isinstance(x, torch.Tensor) and x.is_cuda for x in t)
        for x, y, z in zip(a, b, t):
            assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z.cpu().numpy()))


def test_the_colour_calls_leave_the_volume_and_a_count_valid_for_the_write():
    case, vol = device_volume("plane_sphere")
    want = tref.extract(inp.integrated(case), 2)
    nv, nq = vol.extract_count(2)
    assert (nv, nq) == (len(want["vertices"]), len(want["quads"])) and nv > 100
    before = [t.clone() for t in vol.volume()]
    X = want["vertices"]
    normals = volume.vertex_normals(vol, X, 2)
    colours = volume.colour_points(X, case["images"], case["K"], case["ext"], normals=normals, visibility=np.array(inp.model_depth("plane_sphere")), occlusion_tol=case["occlusion_tol"],
                                   volume=vol)
    views_call(case, vol, "plane_sphere", 1, "best", np.uint8)
    assert colours.shape == (nv, 3) and colours.dtype == np.uint8
    V, Q = torch.empty((nv, 3), dtype=torch.float64, device="cuda"), torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    vol.extract_write(V.data_ptr(), False, Q.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Q.cpu().numpy(), want["quads"]) and np.max(np.abs(V.cpu().numpy() - want["vertices"])) <= 1e-12
    after = vol.volume()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1].view(torch.int16), after[1].view(torch.int16))
    normals_ms, colour_ms = vol.colour_last_kernel_ms()
    assert np.isfinite(normals_ms) and normals_ms > 0 and np.isfinite(colour_ms) and colour_ms > 0
    vol.close()


def test_the_host_refuses_bad_arguments_with_the_outputs_untouched():
    case = inp.get("views_40")
    N, C = len(case["points"]), 3
    X, n, im = torch.from_numpy(case["points"]).cuda(), torch.from_numpy(case["normals"]).cuda(), torch.from_numpy(case["images"]).cuda()
    colour, count = torch.full((N, C), 5, dtype=torch.uint8, device="cuda"), torch.full((N,), 7, dtype=torch.uint16, device="cuda")
    vol = volume.TsdfVolume(0)
    for change, word in ((dict(cos_min=1.0), "cos_min"), (dict(channels=2), "channels"), (dict(pitch=24 * 3 - 1), "pitch"), (dict(width=1), "width"), (dict(occlusion_tol=-1.0), "occlusion_tol")):
        src = dict(source(case, im, colour, d_count=count.data_ptr(), d_visibility=X.data_ptr()), **change)
        with pytest.raises(_capi.PcsError) as e:
            vol.colour_points(N, X.data_ptr(), False, n.data_ptr(), src)
        assert e.value.code == _capi.PCS_ERR_ARG and word in str(e.value)
    with pytest.raises(_capi.PcsError) as e:
        vol.point_normals(N, X.data_ptr(), False, 2, colour.data_ptr())
    assert e.value.code == _capi.PCS_ERR_ARG and "grid" in str(e.value)
    with pytest.raises(_capi.PcsError) as e:
        vol._call("pcs_tsdf_colour_last_kernel_ms", vol._h, None, None)
    assert e.value.code == _capi.PCS_ERR_ARG
    torch.cuda.synchronize()
    assert bool((colour == 5).all()) and bool((count.view(torch.int16) == 7).all())
    vol.close()


def test_mesh_views_with_images_and_colour_surface_end_to_end():
    """On a volume the DEVICE integrated from the textured plane's depth maps: the vertex colours are the texture at the vertex within
    twice the restatement's median error, from NumPy and from tensors alike."""
    case = inp.get("textured_plane")
    vc = case["volume"]
    bounds = [vc["origin"], np.array(vc["origin"]) + vc["voxel"] * (np.array(vc["dims"]) - 1)]
    plain = volume.mesh_views(vc["depth"], vc["K"], vc["ext"], bounds, vc["voxel"], trunc=vc["trunc"])
    V, Q, colours = volume.mesh_views(vc["depth"], vc["K"], vc["ext"], bounds, vc["voxel"], trunc=vc["trunc"], images=case["images"], cos_min=0.1, fill=17.0)
    assert len(plain) == 2 and np.array_equal(bits(plain[0]), bits(V)) and np.array_equal(plain[1], Q)
    assert colours.shape == (len(V), 1) and colours.dtype == np.uint8 and len(V) >= 100
    vol = volume.integrate_depth_maps(vc["depth"], vc["K"], vc["ext"], vc["origin"], vc["voxel"], vc["dims"], trunc=vc["trunc"])
    c2, weight, count, best = volume.colour_surface(vol, V, case["images"], vc["K"], vc["ext"], cos_min=0.1, fill=17.0, info=True)
    assert np.array_equal(colours, c2) and count.dtype == np.uint16 and best.dtype == np.int32 and weight.dtype == np.float32
    some = count > 0
    err = np.abs(c2[some, 0].astype(np.float64) - fi.texture(V[some, 0].astype(np.float64), V[some, 1].astype(np.float64)))
    print(f"{int(some.sum())} of {len(V)} vertices coloured, |colour - texture| median {np.median(err):.2f}, max {err.max():.2f} grey levels")
    assert some.sum() >= 60 and np.median(err) <= 2.0 * inp.MEDIAN_TEXTURE_ERROR["blend"] + 0.5   # + 0.5: the colour is rounded to uint8
    assert np.all(c2[~some, 0] == 17) and np.all(best[~some] == -1) and np.all(weight[~some] == 0)
    t = volume.colour_surface(vol, torch.from_numpy(V).cuda(), torch.from_numpy(case["images"]).cuda(), vc["K"], vc["ext"], cos_min=0.1, fill=17.0, mode="best")
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == c2.shape
    view = case["render"][0]
    img, depth = volume.colour_views(vol, view["K"], view["ext"], view["width"], view["height"], case["images"], vc["K"], vc["ext"], fill=3.0)
    assert img.shape == (1, 30, 40, 1) and img.dtype == np.uint8 and depth.shape == (1, 30, 40) and depth.dtype == np.float32
    hit = np.isfinite(depth)
    assert hit.sum() >= 10 and np.all(img[~hit] == 3) and len(np.unique(img[hit])) > 3
    full = volume.colour_views(vol, view["K"], view["ext"], view["width"], view["height"], case["images"], vc["K"], vc["ext"], fill=3.0, info=True)
    assert len(full) == 5 and np.array_equal(full[0], img) and np.array_equal(bits(full[1]), bits(depth)) and np.all(full[3][~hit] == 0) and full[3][hit].max() == 6
    vol.close()
