"""The TSDF volume and the surface-nets extraction on the device (pycamset_amd/volume.py, csrc/ba_tsdf.hpp) against the NumPy restatement
(tests/tsdf_reference.py).

``weight``, the vertex and quad counts and ``quads`` must be IDENTICAL to the restatement: tests/test_tsdf_reference.py asserts for every
input set used here (tests/tsdf_inputs.py ``CASES``) that no decision of the rule lies within MARGIN = 8 x TSDF_DECISION_GAP of its
threshold.  ``sum`` and ``vertices`` are held to MARGIN x TSDF_GAP relative to the largest magnitude (TSDF_GAP: the restatement's own
float64-versus-longdouble gap); with contraction off the expectation is bit equality, and the gaps found are printed."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, volume
from tests import tsdf_inputs as inp
from tests import tsdf_reference as ref

pytestmark = pytest.mark.gpu
MARGIN = inp.MARGIN


@functools.lru_cache(maxsize=None)
def reference(name):
    case = inp.CASES[name]()
    vol, _ = inp.run_reference(case)
    meshes = {mw: ref.extract(vol, mw) for mw in case["min_weights"]}
    for a in [vol.sum, vol.weight] + [m[k] for m in meshes.values() for k in ("vertices", "quads")]:
        a.setflags(write=False)
    return vol, meshes


def integrate(case, depth=None, **kw):
    a = dict(trunc=case["trunc"], views=None if case["views"] is None else list(case["views"]), dtype=case["sum_dtype"])
    a.update(kw)
    return volume.integrate_depth_maps(case["depth"] if depth is None else depth, case["K"], case["ext"], case["origin"], case["voxel"], case["dims"], **a)


def stored(vol):
    s, w = vol.volume()
    return s.cpu().numpy(), w.cpu().numpy()


def compare_volume(got_sum, got_weight, want, what):
    assert got_weight.dtype == np.uint16 and got_weight.shape == want.weight.shape and np.array_equal(got_weight, want.weight), (what, int((got_weight != want.weight).sum()))
    assert got_sum.dtype == want.sum.dtype and got_sum.shape == want.sum.shape
    big = float(np.max(np.abs(want.sum))) or 1.0
    gap = float(np.max(np.abs(got_sum.astype(np.float64) - want.sum.astype(np.float64)))) / big
    print(f"{what}: sum gap {gap:.2e} (bound {MARGIN * inp.TSDF_GAP:.2e}), weights up to {int(got_weight.max())}")
    assert gap <= MARGIN * inp.TSDF_GAP


def compare_mesh(V, Q, want, what, dtype=np.float64):
    assert V.dtype == dtype and Q.dtype == np.int32 and V.shape == want["vertices"].shape and Q.shape == want["quads"].shape, (what, V.shape, Q.shape, want["vertices"].shape, want["quads"].shape)
    assert np.array_equal(Q, want["quads"]), what
    if len(V):
        gap = float(np.max(np.abs(V - want["vertices"]))) / float(np.max(np.abs(want["vertices"])))
        print(f"{what}: {len(V)} vertices, {len(Q)} quads, vertex gap {gap:.2e} (bound {MARGIN * inp.TSDF_GAP:.2e})")
        assert gap <= MARGIN * inp.TSDF_GAP


@pytest.mark.parametrize("name", list(inp.CASES))
def test_every_case_against_the_restatement(name):
    """The sphere and plane rings; the noisy ring with patches and every kind of invalid depth; float32 and float64 depths and sums; a
    permuted subset of the views; an empty list; a grid partly behind the cameras and partly outside every image; dims (26, 26, 26),
    (33, 17, 5), (2, 2, 2) and (1, 9, 9); min_weight 1, 2 and V (tests/tsdf_inputs.py CASES)."""
    case = inp.CASES[name]()
    want, meshes = reference(name)
    vol = integrate(case)
    compare_volume(*stored(vol), want, name)
    for mw, w in meshes.items():
        V, Q = volume.extract_surface(vol, min_weight=mw, dtype=np.float64)
        compare_mesh(V, Q, w, f"{name} min_weight {mw}")
    if name == "empty_list":
        assert not stored(vol)[0].any() and not stored(vol)[1].any() and vol.n_integrated == 0
    vol.close()


@pytest.mark.parametrize("name", ["sphere_008", "noisy_sum_f64"])
def test_float32_vertices_are_the_float64_ones_rounded_once(name):
    case = inp.CASES[name]()
    vol = integrate(case)
    V64, Q64 = volume.extract_surface(vol, min_weight=2, dtype=np.float64)
    V32, Q32 = volume.extract_surface(vol, min_weight=2)
    assert V32.dtype == np.float32 and len(V32) > 100 and np.array_equal(V32, V64.astype(np.float32)) and np.array_equal(Q32, Q64)
    T = volume.extract_surface(vol, min_weight=2, triangles=True)[1]
    assert np.array_equal(T, volume.quads_to_triangles(Q64)) and T.shape == (2 * len(Q64), 3)
    vol.close()


@pytest.mark.parametrize("name", ["sphere_012", "noisy", "dims_33x17x5"])
def test_two_runs_return_identical_bits(name):
    case = inp.CASES[name]()
    runs = []
    for _ in range(2):
        vol = integrate(case)
        runs.append(stored(vol) + volume.extract_surface(vol, min_weight=2, dtype=np.float64))
        vol.close()
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name,m", [("noisy", 4), ("noisy_depth_f32", 9), ("sphere_012", 1)])
def test_two_calls_continue_from_the_stored_values(name, m):
    """[0, m) then [m, V): with a float64 sum bit for bit one call over all views; with a float32 sum the restatement doing the same two
    calls (the sum is rounded between them)."""
    case = inp.CASES[name]()
    V = len(case["depth"])
    for sum_dtype in (np.float64, np.float32):
        vol = integrate(case, views=list(range(m)), dtype=sum_dtype)
        again =volume.integrate_depth_maps(case["depth"], case["K"], case["ext"], None, None, None, trunc=case["trunc"], views=list(range(m, V)), dtype=None, volume=vol)
        assert again is vol and vol.n_integrated == V
        s2, w2 = stored(vol)
        want = ref.Volume(case["origin"], case["voxel"], case["dims"], sum_dtype)
        ref.integrate(want, case["depth"], case["K"], case["ext"], case["trunc"], range(m))
        ref.integrate(want, case["depth"], case["K"], case["ext"], case["trunc"], range(m, V))
        compare_volume(s2, w2, want, f"{name} two calls {np.dtype(sum_dtype).name}")
        if sum_dtype == np.float64:
            one = integrate(case, dtype=sum_dtype)
            s1, w1 = stored(one)
            assert np.array_equal(s1.view(np.uint8), s2.view(np.uint8)) and np.array_equal(w1, w2)
            one.close()
        vol.close()


def test_a_write_needs_a_count_on_the_volume_as_it_stands():
    case = inp.CASES["sphere_008"]()
    vol = integrate(case)
    buf_v, buf_q = torch.empty((1000, 3), dtype=torch.float64, device="cuda"), torch.empty((1000, 4), dtype=torch.int32, device="cuda")

    def refused():
        with pytest.raises(_capi.PcsError) as e:
            vol.extract_write(buf_v.data_ptr(), False, buf_q.data_ptr())
        assert e.value.code == _capi.PCS_ERR_ARG and "pcs_tsdf_extract_count" in str(e.value)

    refused()                                  # no count yet
    nv, nq = vol.extract_count(2)
    assert (nv, nq) == tuple(len(reference("sphere_008")[1][2][k]) for k in ("vertices", "quads")) and nv <= 1000 and nq <= 1000
    vol.extract_write(buf_v.data_ptr(), False, buf_q.data_ptr())
    torch.cuda.synchronize()
    compare_mesh(buf_v[:nv].cpu().numpy(), buf_q[:nq].cpu().numpy(), reference("sphere_008")[1][2], "count then write")
    D = torch.from_numpy(case["depth"]).cuda()
    vol.integrate(D.data_ptr(), False, len(D), case["trunc"], [0])   # the volume changes: the count no longer stands
    refused()
    vol.extract_count(2)
    vol.reset()
    refused()
    assert not stored(vol)[1].any() and vol.n_integrated == 0
    ms = vol.last_kernel_ms()
    assert all(np.isfinite(m) and m > 0 for m in ms)
    vol.close()


def test_the_host_refuses_a_weight_past_the_limit_before_the_device_is_touched():
    case = inp.CASES["dims_2x2x2"]()
    vol = integrate(case, views=[0] * 65535, dtype=np.float64)
    s, w = stored(vol)
    assert vol.n_integrated == 65535 and w.max() == 65535
    D = torch.from_numpy(case["depth"]).cuda()
    with pytest.raises(_capi.PcsError) as e:
        vol.integrate(D.data_ptr(), False, len(D), case["trunc"], [1])
    assert e.value.code == _capi.PCS_ERR_ARG and "weight" in str(e.value)
    with pytest.raises(ValueError) as e2:
        volume.integrate_depth_maps(case["depth"], case["K"], case["ext"], None, None, None, trunc=case["trunc"], views=[1], dtype=None, volume=vol)
    assert "weight" in str(e2.value)
    s2, w2 = stored(vol)
    assert np.array_equal(s, s2) and np.array_equal(w, w2)
    vol.close()


@pytest.mark.parametrize("name", ["noisy_depth_f32", "sphere_008"])
def test_device_tensors_are_used_in_place_and_give_the_same_bits(name):
    case = inp.CASES[name]()
    D = torch.from_numpy(np.ascontiguousarray(case["depth"])).cuda()
    before = D.clone()
    vol = integrate(case, depth=D)
    V, Q = volume.extract_surface(vol, min_weight=2)
    T = volume.extract_surface(vol, min_weight=2, triangles=True)[1]
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (V, Q, T)) and V.dtype == torch.float32 and Q.dtype == torch.int32
    ints = torch.int64 if D.dtype == torch.float64 else torch.int32
    assert torch.equal(D.view(ints), before.view(ints))
    host = integrate(case)
    Vh, Qh = volume.extract_surface(host, min_weight=2)
    assert isinstance(Vh, np.ndarray) and np.array_equal(V.cpu().numpy(), Vh) and np.array_equal(Q.cpu().numpy(), Qh) and np.array_equal(T.cpu().numpy(), volume.quads_to_triangles(Qh))
    vol.close(), host.close()


def test_mesh_views_is_the_two_steps_in_one_call():
    case = inp.CASES["sphere_008"]()
    lo = np.array(case["origin"])
    hi = lo + case["voxel"] * (np.array(case["dims"]) - 1)
    origin, dims = volume.grid_from_bounds([lo, hi], case["voxel"])
    assert dims == case["dims"] and np.array_equal(origin, lo)
    V, Q = volume.mesh_views(case["depth"], case["K"], case["ext"], [lo, hi], case["voxel"], trunc=case["trunc"], min_weight=2, dtype=np.float64)
    compare_mesh(V, Q, reference("sphere_008")[1][2], "mesh_views", np.float64)
    b = volume.volume_from_points(V, case["voxel"])
    V2, Q2 = volume.mesh_views(case["depth"], case["K"], case["ext"], b, case["voxel"], min_weight=2)   # trunc = 3 voxels on the box of the cloud
    assert len(Q2) >= 100 and V2.dtype == np.float32
