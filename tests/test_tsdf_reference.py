"""The TSDF volume and surface-nets rule without a GPU: the two forms of the NumPy restatement (tests/tsdf_reference.py) against each
other, the properties that make the rule a surface reconstruction (a plane comes back as that plane, a sphere as a closed, outward
oriented quad mesh near the sphere, a spurious depth is out-voted), the margins of every input set of the device tests
(tests/tsdf_inputs.py), and the host-side argument checks, the triangle split and the PLY writer of pycamset_amd/volume.py."""
import ctypes
import functools

import numpy as np
import pytest

from pycamset_amd import _capi, volume
from tests import fusion_inputs as fi
from tests import tsdf_inputs as inp
from tests import tsdf_reference as ref

MARGIN = inp.MARGIN


@functools.lru_cache(maxsize=None)
def integrated(name):
    case = inp.CASES[name]()
    vol, r = inp.run_reference(case)
    return case, vol, r["closest"]


@pytest.mark.parametrize("name", list(inp.CASES))
def test_the_two_forms_agree_exactly(name):
    case, vol, closest = integrated(name)
    vl, rl = inp.run_reference(case, loop=True)
    assert vl.sum.dtype == vol.sum.dtype and np.array_equal(vl.sum, vol.sum) and np.array_equal(vl.weight, vol.weight) and np.array_equal(vl.scale, vol.scale)
    assert rl["closest"] == closest
    for mw in case["min_weights"]:
        a, b = ref.extract(vol, mw), ref.extract_loop(vol, mw)
        assert a["vertices"].shape == b["vertices"].shape and np.array_equal(a["vertices"], b["vertices"]), (name, mw)
        assert a["quads"].dtype == b["quads"].dtype == np.int32 and np.array_equal(a["quads"], b["quads"]), (name, mw)
        assert a["closest"] == b["closest"]
        assert len(a["vertices"]) == int(a["active"].sum()) and (a["quads"].size == 0 or (a["quads"].min() >= 0 and a["quads"].max() < len(a["vertices"])))


@pytest.mark.parametrize("name", list(inp.CASES))
def test_no_decision_of_an_input_set_sits_near_its_threshold(name):
    case, vol, closest = integrated(name)
    worst = min([closest] + [ref.extract(vol, mw)["closest"] for mw in case["min_weights"]])
    print(f"{name}: closest call {worst:.2e} (needed {MARGIN * inp.TSDF_DECISION_GAP:.2e})")
    assert worst >= MARGIN * inp.TSDF_DECISION_GAP


def test_the_gaps_are_the_restatements_own():
    g, gn, d, dn = inp.measure_gaps()
    print(f"TSDF_GAP measured {g:.2e} ({gn}), recorded {inp.TSDF_GAP:.2e}; TSDF_DECISION_GAP measured {d:.2e} ({dn}), recorded {inp.TSDF_DECISION_GAP:.2e}")
    assert g <= inp.TSDF_GAP <= 2 * g and d <= inp.TSDF_DECISION_GAP <= 2 * d


def test_cases_cover_what_the_kernels_branch_on():
    c = {n: inp.CASES[n]() for n in inp.CASES}
    assert c["sphere_008"]["dims"] == (26, 26, 26) and c["dims_33x17x5"]["dims"] == (33, 17, 5) and c["dims_2x2x2"]["dims"] == (2, 2, 2) and c["dims_1x9x9"]["dims"] == (1, 9, 9)
    assert all(max(v["dims"]) <= 33 and v["depth"].shape[1:] == (48, 64) for v in c.values())
    assert c["noisy_depth_f32"]["depth"].dtype == np.float32 and c["noisy_sum_f64"]["sum_dtype"] == np.float64 and c["noisy"]["sum_dtype"] == np.float32
    assert c["subset"]["views"] == (7, 2, 5, 0, 3) and c["empty_list"]["views"] == ()
    D = c["noisy"]["depth"]
    assert np.isnan(D).any() and np.isposinf(D).any() and np.isneginf(D).any() and (D == 0).any() and (D < 0).any()   # every kind of invalid depth
    assert sorted({max(v["min_weights"]) == len(v["depth"]) for v in c.values()}) == [False, True] and all(min(v["min_weights"]) == 1 for v in c.values())
    # "behind": nodes behind every camera and nodes in front of one but outside its image, beside observed ones
    b = c["behind"]
    vol, _ = inp.run_reference(b)
    nx, ny, nz = b["dims"]
    X = np.stack(np.meshgrid(*(b["origin"][a] + b["voxel"] * np.arange(n) for a, n in zip(range(3), (nx, ny, nz))), indexing="ij"), axis=-1).reshape(-1, 3)
    Yz = np.stack([X @ E[2, :3] + E[2, 3] for E in b["ext"]])
    assert (Yz <= 0).all(axis=0).any() and (Yz > 0).all(axis=0).any() and (vol.weight == 0).any() and (vol.weight == len(b["depth"])).any()


def test_a_translated_plane_comes_back_as_that_plane():
    """Four purely translated cameras, depth maps constant at z = c.  The per-node sum is float64 here: a float32 sum rounds D on store,
    2e-11 of c in the vertex, which is the format's precision and not the rule's."""
    case, c = inp.translated_plane()
    assert np.all(case["ext"][:, :, :3] == np.eye(3)) and np.all(case["depth"] == c) and case["sum_dtype"] == np.float64
    vol, r = inp.run_reference(case)
    assert r["closest"] >= MARGIN * inp.TSDF_DECISION_GAP
    for mw in case["min_weights"]:
        x = ref.extract(vol, mw)
        assert len(x["vertices"]) >= 50 and len(x["quads"]) >= 30 and x["closest"] >= MARGIN * inp.TSDF_DECISION_GAP
        dev = float(np.max(np.abs(x["vertices"][:, 2] - c)))
        print(f"min_weight {mw}: {len(x['vertices'])} vertices, worst |z - c| {dev:.2e} (bound {MARGIN * inp.TSDF_GAP * abs(c):.2e})")
        assert dev <= MARGIN * inp.TSDF_GAP * abs(c)


def quad_edges(quads):
    e = np.concatenate([quads[:, [a, (a + 1) % 4]] for a in range(4)])
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


@pytest.mark.parametrize("trunc", [0.08, 0.12])
@pytest.mark.parametrize("min_weight", [1, 2, 6])
def test_the_sphere_comes_back_as_a_closed_outward_mesh(trunc, min_weight):
    """sphere_ring() on 26^3 nodes of 0.04 from (-0.5, -0.5, -0.6).  Measured over the six settings: 234 to 624 vertices, 186 to 537
    quads, the farthest vertex 0.0133 from the sphere (the cell diagonal is 0.069)."""
    case, vol, _ = integrated("sphere_008" if trunc == 0.08 else "sphere_012")
    assert case["trunc"] == trunc and case["origin"] == (-0.5, -0.5, -0.6) and case["voxel"] == 0.04 and case["dims"] == (26, 26, 26)
    x = ref.extract(vol, min_weight)
    V, Q = x["vertices"], x["quads"]
    centre, radius = fi.SPHERE
    dist = np.abs(np.linalg.norm(V - centre, axis=1) - radius)
    print(f"trunc {trunc}, min_weight {min_weight}: {len(V)} vertices, {len(Q)} quads, farthest vertex {dist.max():.4f} (mean {dist.mean():.4f}) of the bound {np.sqrt(3) * 0.04:.4f}")
    assert len(Q) >= 100
    assert dist.max() <= np.sqrt(3.0) * case["voxel"]
    _, uses = quad_edges(Q)
    assert uses.max() <= 2
    P = V[Q]
    normal = np.cross(P[:, 1] - P[:, 0], P[:, 3] - P[:, 0])
    assert np.all(np.sum(normal * (P.mean(axis=1) - centre), axis=1) > 0)


def test_views_that_see_through_a_spurious_depth_out_vote_it():
    """ring(patches=True): view 2's patch claims a surface at 0.75 of the true depth.  The node half a truncation behind that surface
    is INSIDE for view 2 alone; with all views and min_weight = 2 it is observed and not inside."""
    case, (i, j, k), v = inp.free_space_node()
    vol, r = inp.run_reference(dict(case, views=(v,)))
    alone = ref.extract(vol, 1)
    assert r["closest"] >= MARGIN * inp.TSDF_DECISION_GAP and vol.weight[k, j, i] == 1 and alone["inside"][k, j, i] and -0.6 < alone["D"][k, j, i] < -0.4
    vol, r = inp.run_reference(case)
    x = ref.extract(vol, 2)
    assert r["closest"] >= MARGIN * inp.TSDF_DECISION_GAP and x["closest"] >= MARGIN * inp.TSDF_DECISION_GAP
    others = ref.Volume(case["origin"], case["voxel"], case["dims"])
    ref.integrate(others, case["depth"], case["K"], case["ext"], case["trunc"], [w for w in range(len(case["depth"])) if w != v])
    assert others.weight[k, j, i] >= 2 and others.sum[k, j, i] == others.weight[k, j, i]   # at least two other views see through the node: +1 each
    assert x["observed"][k, j, i] and not x["inside"][k, j, i] and x["D"][k, j, i] > 0


@pytest.mark.parametrize("name,m", [("noisy", 4), ("sphere_012", 1), ("noisy_depth_f32", 9)])
def test_two_calls_equal_one_call(name, m):
    """integrate [0, m) then [m, V): bit for bit one call over all views with a float64 sum; with a float32 sum the sum is rounded
    between the calls, so the weights agree and the sums differ by float32 roundings only (the device is held to the restatement doing
    the same two calls)."""
    case = inp.CASES[name]()
    V = len(case["depth"])
    for sum_dtype in (np.float64, np.float32):
        one = ref.Volume(case["origin"], case["voxel"], case["dims"], sum_dtype)
        ref.integrate(one, case["depth"], case["K"], case["ext"], case["trunc"])
        two, loop = one.copy(), None
        two.sum[:], two.weight[:], two.scale[:], two.n_integrated = 0, 0, 1, 0
        loop = two.copy()
        for vol, f in ((two, ref.integrate), (loop, ref.integrate_loop)):
            f(vol, case["depth"], case["K"], case["ext"], case["trunc"], range(m))
            f(vol, case["depth"], case["K"], case["ext"], case["trunc"], range(m, V))
        assert two.n_integrated == one.n_integrated == V and np.array_equal(two.weight, one.weight)
        assert np.array_equal(two.sum, loop.sum) and np.array_equal(two.weight, loop.weight)
        if sum_dtype == np.float64:
            assert np.array_equal(two.sum, one.sum)
        else:
            assert np.max(np.abs(two.sum.astype(np.float64) - one.sum)) <= 2 * np.finfo(np.float32).eps * V


def test_check_tsdf_args_refuses_each_bad_argument_by_name():
    D, K, E = fi.sphere_ring()
    V, H, W = D.shape
    ok = dict(n_views=V, width=W, height=H, K=K, ext=E, origin=(-0.5, -0.5, -0.6), voxel=0.04, dims=(26, 26, 26), trunc=0.08)
    Ka, P, o, voxel, dims, trunc, lst, f32 = volume.check_tsdf_args(**ok)
    assert Ka.shape == (V, 4) and P.shape == (V, 12) and o.tolist() == [-0.5, -0.5, -0.6] and (voxel, dims, trunc, lst, f32) == (0.04, (26, 26, 26), 0.08, None, True)
    assert volume.check_tsdf_args(**ok, dtype=np.float64)[7] is False
    lst = volume.check_tsdf_args(**ok, views=[3, 0, 3])[6]
    assert lst.dtype == np.int32 and lst.tolist() == [3, 0, 3]
    assert len(volume.check_tsdf_args(**ok, views=[])[6]) == 0
    bad_K = K.copy()
    bad_K[1, 0] = 0.0
    for change, word in ((dict(origin=(0.0, np.nan, 0.0)), "origin"), (dict(origin=(0.0, np.inf, 0.0)), "origin"), (dict(origin=(0.0, 0.0)), "origin"), (dict(voxel=0.0), "voxel"),
                         (dict(voxel=-0.04), "voxel"), (dict(voxel=np.nan), "voxel"), (dict(dims=(26, 0, 26)), "dims"), (dict(dims=(1025, 26, 26)), "dims"),
                         (dict(dims=(26, 26)), "dims"), (dict(dims=(26, 26, 2.5)), "dims"), (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=np.inf), "trunc"),
                         (dict(views=[0, V]), "views"), (dict(views=[-1]), "views"), (dict(views=[0.5]), "views"), (dict(n_integrated=65535 - V + 1), "weight"),
                         (dict(views=[0, 1], n_integrated=65534), "weight"), (dict(K=bad_K), "K"), (dict(K=K[:, :3]), "K"), (dict(dtype=np.float16), "dtype"),
                         (dict(width=0), "depth"), (dict(n_views=0, K=K[:0], ext=E[:0]), "depth")):
        with pytest.raises(ValueError) as e:
            volume.check_tsdf_args(**dict(ok, **change))
        assert word in str(e.value), (change, str(e.value))
    assert volume.check_tsdf_args(**dict(ok, n_integrated=65535 - V))[4] == (26, 26, 26)   # exactly to the limit
    for change, word in ((dict(min_weight=0), "min_weight"), (dict(min_weight=65536), "min_weight"), (dict(min_weight=1.5), "min_weight")):
        with pytest.raises(ValueError) as e:
            volume.extract_surface(None, **change)
        assert "volume" in str(e.value)   # the volume is looked at first: without one nothing else is checked


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 127
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    K, E = fi.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    ARG = _capi.PCS_ERR_ARG
    assert lib.pcs_tsdf_create(None, 0) == ARG and lib.pcs_tsdf_destroy(None) == _capi.PCS_OK
    bad_K = K.copy()
    bad_K[1, 2] = 0.0
    for args, word in (((0, 8, 6, dp(K), dp(P)), "n_views"), ((3, 0, 6, dp(K), dp(P)), "width"), ((3, 8, 6, None, dp(P)), "K"), ((3, 8, 6, dp(bad_K), dp(P)), "K of view 1"),
                       ((3, 8, 6, dp(K), dp(P)), "NULL handle")):
        assert lib.pcs_tsdf_set_views(None, *args) == ARG and word in _err(), (word, _err())
    o = (0.0, 0.0, 0.0)
    for args, word in (((None, 0.1, 4, 4, 4, 1), "origin"), ((dp((0.0, np.nan, 0.0)), 0.1, 4, 4, 4, 1), "origin"), ((dp(o), 0.0, 4, 4, 4, 1), "voxel"), ((dp(o), np.inf, 4, 4, 4, 1), "voxel"),
                       ((dp(o), 0.1, 0, 4, 4, 1), "nx"), ((dp(o), 0.1, 4, 1025, 4, 1), "ny"), ((dp(o), 0.1, 4, 4, -1, 1), "nz"), ((dp(o), 0.1, 4, 4, 4, 2), "sum_dtype"),
                       ((dp(o), 0.1, 4, 4, 4, 0), "NULL handle")):
        assert lib.pcs_tsdf_set_grid(None, *args) == ARG and word in _err(), (word, _err())
    for args, word in (((64, 2, None, 0, 0.1, None), "depth_dtype"), ((64, 1, None, 0, 0.0, None), "trunc"), ((64, 1, None, 0, np.nan, None), "trunc"),
                       ((64, 0, ip([0]), -1, 0.1, None), "n_list"), ((64, 0, ip([0]), 65536, 0.1, None), "n_list"), ((None, 1, None, 0, 0.1, None), "d_depth"),
                       ((64, 1, None, 0, 0.1, None), "NULL handle")):
        assert lib.pcs_tsdf_integrate(None, *args) == ARG and word in _err(), (word, _err())
    n = ctypes.c_int64()
    for args, word in (((0, ctypes.byref(n), ctypes.byref(n), None), "min_weight"), ((65536, ctypes.byref(n), ctypes.byref(n), None), "min_weight"), ((2, None, ctypes.byref(n), None), "n_vertices"),
                       ((2, ctypes.byref(n), ctypes.byref(n), None), "NULL handle")):
        assert lib.pcs_tsdf_extract_count(None, *args) == ARG and word in _err(), (word, _err())
    assert lib.pcs_tsdf_extract_write(None, 64, 2, 64, None) == ARG and "vertex_dtype" in _err()
    assert lib.pcs_tsdf_extract_write(None, 64, 1, 64, None) == ARG and "NULL handle" in _err()
    assert lib.pcs_tsdf_reset(None) == ARG and lib.pcs_tsdf_volume_ptrs(None, None, None) == ARG
    f = ctypes.c_float()
    assert lib.pcs_tsdf_last_kernel_ms(None, ctypes.byref(f), None, None) == ARG
    if lib.pcs_device_count() == 0:   # no device: no handle, and never a CPU fallback
        with pytest.raises(_capi.PcsError) as e:
            volume.TsdfVolume(0)
        assert e.value.code == _capi.PCS_ERR_NODEVICE


def read_ply(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    end = lines.index("end_header")
    nv = int([l for l in lines[:end] if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines[:end] if l.startswith("element face")][0].split()[-1])
    body = [l for l in lines[end + 1:] if l]
    assert len(body) == nv + nf
    V = np.array([[float(t) for t in l.split()] for l in body[:nv]]).reshape(-1, 3)
    F = [[int(t) for t in l.split()] for l in body[nv:]]
    assert all(f[0] == len(f) - 1 for f in F)
    return V, np.array([f[1:] for f in F])


def test_triangles_and_the_ply_writer(tmp_path):
    case, vol, _ = integrated("sphere_008")
    x = ref.extract(vol, 2)
    V, Q = x["vertices"].astype(np.float32), x["quads"]
    T = volume.quads_to_triangles(Q)
    assert T.shape == (2 * len(Q), 3) and T.dtype == np.int32
    assert np.array_equal(T[0::2], Q[:, [0, 1, 2]]) and np.array_equal(T[1::2], Q[:, [0, 2, 3]])
    for faces, name in ((Q, "quads.ply"), (T, "triangles.ply")):
        volume.write_ply(tmp_path / name, V, faces)
        Vr, Fr = read_ply(tmp_path / name)
        assert Vr.shape == V.shape and np.array_equal(Vr.astype(np.float32), V) and np.array_equal(Fr, faces)
    volume.write_ply(tmp_path / "empty.ply", V[:0], Q[:0])
    Vr, Fr = read_ply(tmp_path / "empty.ply")
    assert len(Vr) == 0 and len(Fr) == 0
    with pytest.raises(ValueError):
        volume.write_ply(tmp_path / "bad.ply", V[:3], Q)
    b = volume.volume_from_points(np.concatenate([V, [[np.nan, 0, 0]]]), 0.04)
    assert b.shape == (2, 3) and np.allclose(b[0], V.min(axis=0) - 0.16) and np.allclose(b[1], V.max(axis=0) + 0.16)
    origin, dims = volume.grid_from_bounds(b, 0.04)
    assert np.array_equal(origin, b[0]) and all(origin[a] + 0.04 * (dims[a] - 1) >= b[1][a] - 1e-9 > origin[a] + 0.04 * (dims[a] - 2) for a in range(3))
