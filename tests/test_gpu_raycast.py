"""The ray-cast of the TSDF volume on the device (pycamset_amd/volume.py, csrc/ba_tsdf_raycast.hpp) against the NumPy restatement
(tests/raycast_reference.py).

The status must be IDENTICAL to the restatement's: tests/test_raycast_reference.py asserts for every input set used here
(tests/raycast_inputs.py) that no decision of the rule lies within MARGIN = 8 x RAY_DECISION_GAP of its threshold.  Depths are held to
MARGIN x RAY_GAP relative to the view's largest depth and normals to MARGIN x RAY_NORMAL_GAP (the restatement's own float64-versus-longdouble
gaps), the float32 outputs with one rounding to float32 (2^-24 relative) on top; with contraction off the expectation is bit equality,
and the gaps found are printed.  The volume under the cast is the restatement's own, copied into the handle, so that nothing but the
cast is held here; the cast of a volume the device integrated is covered through ``raycast_views`` below."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, volume
from tests import raycast_inputs as inp
from tests import raycast_reference as ray
from tests import tsdf_reference as tref

pytestmark = pytest.mark.gpu
MARGIN = inp.MARGIN
ALL = list(inp.CASES) + ["translated_plane"]
F32 = 2.0 ** -24


def get(name):
    return inp.translated_plane()[0] if name == "translated_plane" else inp.CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, k):
    case = get(name)
    r = inp.cast_reference(case, inp.integrated(name), case["views"][k])
    for key in ("depth", "normal", "status"):
        r[key].setflags(write=False)
    return r


def device_volume(name):
    """A handle whose volume holds the bits of the restatement's."""
    case, want = get(name), inp.integrated(name)
    vol = volume.TsdfVolume(0)
    vol.set_grid(case["volume"]["origin"], case["volume"]["voxel"], case["volume"]["dims"], want.sum.dtype == np.float32)
    s, w = vol.volume()
    s.copy_(torch.from_numpy(want.sum.copy()))
    w.view(torch.int16).copy_(torch.from_numpy(want.weight.copy().view(np.int16)))
    torch.cuda.synchronize()
    return case, vol


def cast(case, vol, view, dtype=np.float64, normals=True, status=True, skip=True):
    return volume.raycast_views(vol, view["K"], view["ext"], view["width"], view["height"], min_weight=case["min_weight"], step=case["step"], z_near=case["z_near"], z_far=case["z_far"],
                                dtype=dtype, normals=normals, status=status, skip=skip)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def compare(got, want, dtype, what):
    depth, normal, status = got
    assert depth.dtype == dtype and normal.dtype == np.float32 and status.dtype == np.uint8
    assert depth.shape == want["depth"].shape and normal.shape == want["normal"].shape and np.array_equal(status, want["status"]), (what, int((status != want["status"]).sum()))
    assert np.array_equal(np.isnan(depth), np.isnan(want["depth"])) and np.array_equal(np.isnan(depth), status > ray.NO_NORMAL), what
    assert np.array_equal(np.isnan(normal), np.isnan(want["normal"])) and np.array_equal(np.isnan(normal[..., 0]), status != ray.HIT), what
    hit, full = status <= ray.NO_NORMAL, status == ray.HIT
    extra = F32 if dtype == np.float32 else 0.0
    gap = float(np.max(np.abs(depth[hit].astype(np.float64) - want["depth"][hit])) / np.max(want["depth"][hit])) if hit.any() else 0.0
    ngap = float(np.max(np.abs(normal[full].astype(np.float64) - want["normal"][full]))) if full.any() else 0.0
    print(f"{what}: {int(hit.sum())} hits, depth gap {gap:.2e} (bound {MARGIN * inp.RAY_GAP + extra:.2e}); {int(full.sum())} normals, gap {ngap:.2e} (bound {MARGIN * inp.RAY_NORMAL_GAP + F32:.2e})")
    assert gap <= MARGIN * inp.RAY_GAP + extra and ngap <= MARGIN * inp.RAY_NORMAL_GAP + F32


@pytest.mark.parametrize("name", ALL)
def test_every_case_and_view_against_the_restatement(name):
    """The sphere and plane rings, the noisy ring with a float32 and a float64 sum, a subset of its views, an empty volume, a grid partly
    behind the cameras, dims (33, 17, 5), one cell, no cells, the translated plane with its axis-parallel column; views of 40 x 30
    (six workgroups, no side a multiple of the tile), 13 x 7 from inside the box and 1 x 1; depth in float32 and float64; with and
    without skipping: the same bits."""
    case, vol = device_volume(name)
    for k, view in enumerate(case["views"]):
        want = reference(name, k)
        for dtype in (np.float64, np.float32):
            got = cast(case, vol, view, dtype)
            compare(got, want, dtype, f"{name} view {k} {np.dtype(dtype).name}")
            plain = cast(case, vol, view, dtype, skip=False)
            for a, b in zip(got, plain):
                assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (name, k, "skipping changed a bit")
        d64, d32 = cast(case, vol, view, np.float64)[0], cast(case, vol, view, np.float32)[0]
        assert np.array_equal(bits(d64.astype(np.float32)), bits(d32))   # the float32 depth is the float64 one rounded once
    vol.close()


@pytest.mark.parametrize("name", ["sphere_012", "noisy", "dims_33x17x5"])
def test_two_runs_return_identical_bits(name):
    runs = []
    for _ in range(2):
        case, vol = device_volume(name)
        runs.append([a for view in case["views"] for a in cast(case, vol, view)])
        vol.close()
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["sphere_008", "behind", "dims_2x2x2"])
def test_without_normals_the_depth_is_the_same_and_status_1_reads_0(name):
    case, vol = device_volume(name)
    ones = 0
    for view in case["views"]:
        depth, normal, status = cast(case, vol, view)
        d2, n2, s2 = cast(case, vol, view, normals=False)
        assert n2 is None and np.array_equal(bits(depth), bits(d2)) and np.array_equal(s2, np.where(status == ray.NO_NORMAL, ray.HIT, status))
        d3, n3 = cast(case, vol, view, status=False)   # no status either way: the call runs and gives the same maps
        assert np.array_equal(bits(depth), bits(d3)) and np.array_equal(bits(normal), bits(n3))
        d4, n4 = cast(case, vol, view, normals=False, status=False)
        assert n4 is None and np.array_equal(bits(depth), bits(d4))
        ones += int((status == ray.NO_NORMAL).sum())
    assert ones > 0
    vol.close()


def test_a_cast_leaves_a_count_valid_for_the_write():
    case, vol = device_volume("sphere_008")
    mesh = tref.extract(inp.integrated("sphere_008"), 2)
    nv, nq = vol.extract_count(2)
    assert (nv, nq) == (len(mesh["vertices"]), len(mesh["quads"])) and nv > 100
    before = [t.clone() for t in vol.volume()]
    for view in case["views"]:
        cast(case, vol, view)
    V, Q = torch.empty((nv, 3), dtype=torch.float64, device="cuda"), torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    vol.extract_write(V.data_ptr(), False, Q.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Q.cpu().numpy(), mesh["quads"]) and np.max(np.abs(V.cpu().numpy() - mesh["vertices"])) <= 1e-12
    after = vol.volume()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1].view(torch.int16), after[1].view(torch.int16))   # the cast reads the volume only
    mask_ms, cast_ms = vol.raycast_last_kernel_ms()
    assert np.isfinite(mask_ms) and mask_ms > 0 and np.isfinite(cast_ms) and cast_ms > 0
    view = case["views"][0]
    cast(case, vol, view, skip=False)
    mask_ms, cast_ms = vol.raycast_last_kernel_ms()
    assert np.isnan(mask_ms) and cast_ms > 0   # no mask was made
    vol.close()


@pytest.mark.parametrize("name", ["sphere_008", "noisy_sum_f64"])
def test_the_counting_launch_counts_the_samples_of_the_restatement(name):
    """Without skipping and without normals every sample of the march is evaluated: the restatement's count.  With the mask there are
    fewer, and with the normals up to six more per hit."""
    case, vol = device_volume(name)
    with pytest.raises(_capi.PcsError) as e:
        vol.raycast_count_samples(torch.empty(1, dtype=torch.int32, device="cuda").data_ptr())
    assert e.value.code == _capi.PCS_ERR_STATE
    view = case["views"][0]
    n = torch.zeros((1, view["height"], view["width"]), dtype=torch.int32, device="cuda")
    counts = {}
    for normals, skip in ((False, False), (False, True), (True, False)):
        got = cast(case, vol, view, normals=normals, skip=skip)
        vol.raycast_count_samples(n.data_ptr())
        torch.cuda.synchronize()
        counts[(normals, skip)] = int(n.sum())
        assert np.array_equal(got[-1], reference(name, 0)["status"]) or not normals
    hits = int((reference(name, 0)["status"] <= ray.NO_NORMAL).sum())
    print(f"{name}: {counts}, the restatement's march {reference(name, 0)['samples']}, {hits} hits")
    assert counts[(False, False)] == reference(name, 0)["samples"]
    assert 0 < counts[(False, True)] < counts[(False, False)] < counts[(True, False)] <= counts[(False, False)] + 6 * hits
    vol.close()


def test_the_host_refuses_bad_arguments_before_the_device_is_touched():
    case, vol = device_volume("dims_2x2x2")
    view = case["views"][1]
    K, P = np.ascontiguousarray(view["K"]), np.ascontiguousarray(view["ext"].reshape(1, 12))
    out = torch.full((7, 13), 5.0, dtype=torch.float64, device="cuda")
    for kw, word in ((dict(step=case["volume"]["voxel"] / 65.0), "step"), (dict(min_weight=0), "min_weight"), (dict(z_near=1.0, z_far=0.5), "z_near")):
        a = dict(min_weight=1, step=case["volume"]["voxel"], z_near=0.0, z_far=np.inf)
        a.update(kw)
        with pytest.raises(_capi.PcsError) as e:
            vol.raycast(13, 7, K, P, a["min_weight"], a["step"], a["z_near"], a["z_far"], out.data_ptr(), False)
        assert e.value.code == _capi.PCS_ERR_ARG and word in str(e.value)
    fresh = volume.TsdfVolume(0)
    with pytest.raises(_capi.PcsError) as e:
        fresh.raycast(13, 7, K, P, 1, 0.04, 0.0, np.inf, out.data_ptr(), False)
    assert e.value.code == _capi.PCS_ERR_ARG and "grid" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    fresh.close(), vol.close()


@pytest.mark.parametrize("name", ["sphere_008", "noisy"])
def test_raycast_views_and_depth_residuals_from_tensors_and_from_numpy(name):
    """On a volume the DEVICE integrated: the views that were integrated are cast back and held against their depth maps."""
    case = get(name)
    v = case["volume"]
    kw = dict(trunc=v["trunc"], dtype=v["sum_dtype"])
    host = volume.integrate_depth_maps(v["depth"], v["K"], v["ext"], v["origin"], v["voxel"], v["dims"], **kw)
    D = torch.from_numpy(np.ascontiguousarray(v["depth"])).cuda()
    dev = volume.integrate_depth_maps(D, v["K"], v["ext"], v["origin"], v["voxel"], v["dims"], **kw)
    H, W = v["depth"].shape[1:]
    a = volume.raycast_views(host, v["K"], v["ext"], W, H, status=True)
    b = volume.raycast_views(dev, v["K"], v["ext"], W, H, status=True)
    assert all(isinstance(x, np.ndarray) for x in a) and all(isinstance(x, torch.Tensor) and x.is_cuda for x in b)
    assert a[0].dtype == np.float32 and a[0].shape == v["depth"].shape and a[1].shape == v["depth"].shape + (3,)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y.cpu().numpy()))
    assert (a[2] == ray.HIT).sum() > 1000
    res_h, stats_h = volume.depth_residuals(host, v["depth"], v["K"], v["ext"], dtype=np.float64)
    res_d, stats_d = volume.depth_residuals(dev, D, v["K"], v["ext"], dtype=np.float64)
    assert isinstance(res_h, np.ndarray) and isinstance(stats_h, np.ndarray) and res_d.is_cuda and stats_d.is_cuda and stats_h.shape == (len(D), 3)
    assert np.array_equal(bits(res_h), bits(res_d.cpu().numpy())) and np.array_equal(bits(stats_h), bits(stats_d.cpu().numpy()))
    valid = np.isfinite(v["depth"]) & (v["depth"] > 0)
    model = volume.raycast_views(host, v["K"], v["ext"], W, H, dtype=np.float64, normals=False)[0]
    both = np.isfinite(model) & valid
    assert np.array_equal(np.isfinite(res_h), both) and np.array_equal(res_h[both], (model - v["depth"])[both])
    for k in range(len(D)):
        r = res_h[k][both[k]]
        assert stats_h[k, 0] == r.size and r.size > 300
        med = np.sort(r)[(r.size - 1) // 2]   # torch's median: the lower of the two middle values
        assert stats_h[k, 1] == med and stats_h[k, 2] == np.sort(np.abs(r - med))[(r.size - 1) // 2]
    print(f"{name}: per-view (count, median, MAD) of model - depth:\n{stats_h}")
    assert np.all(np.abs(stats_h[:, 1]) <= np.sqrt(3.0) * v["voxel"])
    host.close(), dev.close()
