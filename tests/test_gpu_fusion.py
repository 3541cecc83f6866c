"""The depth-map fusion on the device (pycamset_amd/fusion.py, csrc/ba_fusion.hpp) against the NumPy restatement (tests/fusion_reference.py).

``mask``, ``count``, ``support``, ``status`` and the per-view counts must be IDENTICAL to the restatement: tests/test_fusion_reference.py
asserts for every input set used here (tests/fusion_inputs.py ``CASES``) that no decision of the rule lies within MARGIN = 8 x
FUSE_DECISION_GAP of its threshold.  The points and the fused depth are held to MARGIN x FUSE_GAP, relative to the largest coordinate
(FUSE_GAP: the restatement's own float64-versus-longdouble gap); a float32 output is the float64 one rounded once.

No golden from the reference exists for the fusion itself: the reference hands this step to an external program.  The neighbour lists
do have one (tests/golden/view_pairs.npz, checked without a GPU)."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, fusion
from tests import fusion_inputs as inp
from tests import fusion_reference as ref

pytestmark = pytest.mark.gpu
MARGIN = 8.0
EXACT = ("mask", "count", "support", "status")


@functools.lru_cache(maxsize=None)
def reference(name):
    a, o = inp.CASES[name]()
    r = ref.fuse(**a, **o)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def device(name, dtype=np.float64, **kw):
    a, o = inp.CASES[name]()
    got = fusion.fuse_depth_maps(**a, **o, dtype=dtype, return_support=True, return_status=True, return_depth=True, **kw)
    return dict(zip(("points", "mask", "count", "support", "status", "fused_depth"), got))


def compare(got, want, what=""):
    for k in EXACT:
        g, w = got[k], want[k]
        bad = np.argwhere(g != w)
        assert g.dtype == w.dtype and g.shape == w.shape and bad.size == 0, (what, k, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    m = want["mask"].astype(bool)
    assert np.array_equal(got["mask"] == 1, got["status"] == 0)
    assert np.all(np.isnan(got["points"][~m])) and np.all(np.isfinite(got["points"][m])) and np.array_equal(np.isnan(got["fused_depth"]), ~m)
    if m.any():
        big = float(np.max(np.abs(want["points"][m])))
        gp = float(np.max(np.abs(got["points"][m] - want["points"][m]))) / big
        gd = float(np.max(np.abs(got["fused_depth"][m] - want["fused_depth"][m]))) / big
        print(f"{what}: points gap {gp:.2e}, fused depth gap {gd:.2e} (bound {MARGIN * inp.FUSE_GAP:.2e}), kept {int(m.sum())} of {m.size}")
        assert gp <= MARGIN * inp.FUSE_GAP and gd <= MARGIN * inp.FUSE_GAP


@pytest.mark.parametrize("name", list(inp.CASES))
def test_every_case_against_the_restatement(name):
    """Neighbour counts 1, 2, 9 and 32; an empty list; a list in descending order; ragged and degenerate shapes; min_views 1, 2 and the
    list length; tight and loose tolerances; float32 and float64 depths; with and without transform and unique; every kind of invalid
    depth; the facing pair; views without overlap (tests/fusion_inputs.py CASES)."""
    a, o = inp.CASES[name]()
    want = reference(name)
    got = device(name)
    assert got["points"].dtype == np.float64 and got["fused_depth"].dtype == np.float64
    compare(got, want, name)
    clouds = fusion.fuse_depth_maps(**a, **o, dtype=np.float64, compact=True)   # the per-view counts, as the compaction reads them
    assert [len(c) for c in clouds] == want["counts"].tolist()
    for c, w in zip(clouds, ref.compact(got["points"], want["mask"])):
        assert c.dtype == np.float64 and np.array_equal(c, w)


def test_cases_cover_what_the_kernels_branch_on():
    shapes = {n: inp.CASES[n]()[0]["depth"].shape for n in inp.CASES}
    assert shapes["shape_67x45"][1:] == (45, 67) and shapes["shape_w_below_tile"][2] < 32 and shapes["shape_h_below_tile"][1] < 8
    assert shapes["shape_h1"][1] == 1 and shapes["shape_1x1"][1:] == (1, 1) and shapes["nbr32"] == (33, 16, 24)
    assert shapes["nbr2"][2] > 32 and shapes["nbr2"][1] > 8   # more than one workgroup in x and in y
    assert reference("nbr32")["count"].max() == 32 and reference("unique")["status"].max() == ref.DUPLICATE
    assert inp.CASES["depth_f32"]()[0]["depth"].dtype == np.float32 and inp.CASES["unique_f32"]()[0]["depth"].dtype == np.float32


@pytest.mark.parametrize("name", ["nbr2", "transform", "unique_f32"])
def test_float32_points_are_the_float64_ones_rounded_once(name):
    p64, p32 = device(name), device(name, dtype=np.float32)
    for k in EXACT:
        assert np.array_equal(p32[k], p64[k])
    for k in ("points", "fused_depth"):
        assert p32[k].dtype == np.float32 and np.array_equal(p32[k], p64[k].astype(np.float32), equal_nan=True), k


@pytest.mark.parametrize("name", ["nbr9", "unique", "nbr32"])
def test_two_runs_return_identical_bits(name):
    a, b = device(name), device(name)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["nbr2", "unique_f32"])
def test_device_tensors_are_used_in_place_and_give_the_same_bits(name):
    a, o = inp.CASES[name]()
    host = device(name, dtype=np.float32)
    D = torch.from_numpy(np.ascontiguousarray(a["depth"])).cuda()
    before = D.clone()
    got = fusion.fuse_depth_maps(D, a["K"], a["ext"], a["neighbours"], **o, dtype=np.float32, return_support=True, return_status=True, return_depth=True)
    assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got) and torch.equal(D.view(torch.int64 if D.dtype == torch.float64 else torch.int32),
                                                                                     before.view(torch.int64 if D.dtype == torch.float64 else torch.int32))
    for g, k in zip(got, ("points", "mask", "count", "support", "status", "fused_depth")):
        g = g.cpu().numpy()
        assert np.array_equal(g.view(np.uint32) if k == "support" else g, host[k], equal_nan=True), k
    start, nbr = ref.as_csr(a["neighbours"])   # the CSR pair in place of the lists
    csr = fusion.fuse_depth_maps(a["depth"], a["K"], a["ext"], (start, nbr), **o, dtype=np.float32)
    assert len(csr) == 3 and np.array_equal(csr[0], host["points"], equal_nan=True) and np.array_equal(csr[1], host["mask"]) and np.array_equal(csr[2], host["count"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compact_is_the_masked_points_in_view_and_pixel_order_with_the_grey_values(dtype):
    a, o = inp.CASES["unique"]()
    want = reference("unique")
    values = (np.arange(a["depth"].size, dtype=np.int64).reshape(a["depth"].shape) * 7 % 251).astype(np.uint8)
    full = fusion.fuse_depth_maps(**a, **o, dtype=dtype)
    clouds = fusion.fuse_depth_maps(**a, **o, dtype=dtype, values=values, compact=True)
    assert [len(c[0]) for c in clouds] == want["counts"].tolist() and 0 < want["counts"].min()
    for (p, v), (pw, vw), (pr, _) in zip(clouds, ref.compact(full[0], want["mask"], values), ref.compact(want["points"], want["mask"], values)):
        assert p.dtype == np.dtype(dtype) and p.shape == pw.shape and np.array_equal(p, pw) and v.dtype == np.uint8 and np.array_equal(v, vw)
        if dtype == np.float64:
            assert float(np.max(np.abs(p - pr))) <= MARGIN * inp.FUSE_GAP * float(np.max(np.abs(want["points"][want["mask"] == 1])))


def test_the_handle_on_raw_addresses():
    """Optional outputs left out, the timers, another shape on the same handle, and the refusals that need a handle."""
    a, o = inp.CASES["nbr2"]()
    want = reference("nbr2")
    V, H, W = a["depth"].shape
    start, nbr = ref.as_csr(a["neighbours"])
    f = fusion.DepthFuser(0)
    D = torch.from_numpy(np.ascontiguousarray(a["depth"])).cuda()
    pts = torch.empty((V, H, W, 3), dtype=torch.float64, device="cuda")
    mask = torch.empty((V, H, W), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((V,), dtype=torch.int64, device="cuda")
    with pytest.raises(_capi.PcsError) as e:
        f.run(D.data_ptr(), False, pts.data_ptr(), mask.data_ptr(), f32=False)
    assert e.value.code == _capi.PCS_ERR_STATE
    with pytest.raises(_capi.PcsError) as e:
        f.set_neighbours(start, nbr)
    assert e.value.code == _capi.PCS_ERR_STATE
    f.set_views(W, H, a["K"], a["ext"].reshape(V, 12))
    with pytest.raises(_capi.PcsError) as e:
        f.set_neighbours(np.append(start, start[-1]), nbr)   # valid lists, for one view more
    assert e.value.code == _capi.PCS_ERR_ARG and "differs" in str(e.value)
    f.set_neighbours(start, nbr)
    f.run(D.data_ptr(), False, pts.data_ptr(), mask.data_ptr(), f32=False, d_counts=counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy(), want["mask"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
    check_ms, unique_ms, total_ms = f.last_kernel_ms()
    assert check_ms > 0 and unique_ms == 0 and total_ms >= check_ms
    f.run(D.data_ptr(), False, pts.data_ptr(), mask.data_ptr(), f32=False, unique=True, d_counts=counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    uniq = ref.fuse(**a, **dict(o, unique=True))
    assert np.array_equal(mask.cpu().numpy(), uniq["mask"]) and np.array_equal(counts.cpu().numpy(), uniq["counts"]) and f.last_kernel_ms()[1] > 0
    f.set_views(W, H, a["K"], a["ext"].reshape(V, 12))   # new views drop the neighbour lists
    with pytest.raises(_capi.PcsError) as e:
        f.run(D.data_ptr(), False, pts.data_ptr(), mask.data_ptr(), f32=False)
    assert e.value.code == _capi.PCS_ERR_STATE
    f.close()


# ---- stereo pairs of a ring to one cloud ----------------------------------------------------------------------------------------------------
def test_fuse_stereo_pairs_on_a_ring():
    """Five cameras on an arc look at a textured plane; the four adjacent pairs are matched and fused.

    The scale.  One quantum of disparity, 1/16 px, moves a point at depth Z by Z^2 / (f B) / 16 along its ray, and no further from the
    plane than that: q = Zmax^2 / (f_min B_min) / 16, Zmax (and Zmin below) the depth of the plane over the corners of the rectified
    views, f and B those of the pairs.

    MEDIAN distance <= q: "within the disparity quantisation", as the issue words it.
    95 % of the distances <= e q, e derived per observation, in quanta, from what a right match of this matcher can be off by:
      0.5                         the disparity is stored rounded to a sixteenth;
      16 r B_max tan(t) / Zmin    the window is matched as if fronto-parallel, but the plane is tilted by up to t against the rectified
                                  views, so the disparities inside a window of radius r differ from the centre's by up to r B tan(t) / Z
                                  px, and the answer lies among them;
      16 (3 - 2 sqrt 2) / 2       the parabola through three values of a V-shaped sum of absolute differences C(d) = |d - s| puts its
                                  minimum at s / (2 (1 - |s|)) for a true offset s in [-1/2, 1/2]; the largest error over s, at
                                  s = 1 - 1 / sqrt 2, is (3 - 2 sqrt 2) / 2 = 0.0858 px.
    A fused point is a mean of observations that each carry the bound, so it carries it too.  A bound for EVERY point is not
    attainable and not asked: the images are rounded to 8 bits, which moves a cost minimum by an amount no formula of f, B and 1/16 px
    gives, and wrong matches of several pairs can agree with one another by chance; the largest distance is printed.
    The fused median must also be no worse than the median of any one pair's own cloud.
    First measured (MI355X): q 6.59e-3, e = 3.48; median 3.73e-3 = 0.57 q; 95 % 1.39e-2 = 2.12 q; largest 2.81e-2; per-pair medians 4.8e-3 .. 7.8e-3."""
    images, intr, ext = inp.stereo_ring()
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4)]
    block = 9
    opts = dict(match_options=dict(block=block, lr_max_diff=1), depth_range=(0.2, 3.0), rel_tol=0.02, dtype=np.float64)
    pts, grey = fusion.fuse_stereo_pairs(images, intr, ext, pairs, 32, **opts)
    Ks, Ps, nb, D, counts, sums = fusion.fuse_stereo_pairs.last
    assert pts.dtype == np.float64 and pts.shape == (sum(counts), 3) and grey.dtype == np.uint8 and grey.shape == (len(pts),)
    assert [list(l) for l in nb] == [list(l) for l in fusion.view_neighbours(Ps)] and all(len(l) == 3 for l in nb)
    W, H = inp.STEREO_RES
    assert D.shape == (4, H, W)
    zs = []
    for K, P in zip(Ks, Ps):
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            d, o = P[:, :3].T @ np.array([(x - K[1]) / K[0], (y - K[3]) / K[2], 1.0]), -P[:, :3].T @ P[:, 3]
            zs.append((inp.STEREO_Z0 - o[2]) / d[2])
    zmin, zmax = min(zs), max(zs)
    assert zmin > 0
    centres = np.stack([-E[:, :3].T @ E[:, 3] for E in ext])
    bases = [float(np.linalg.norm(centres[a] - centres[b])) for a, b in pairs]
    quantum = zmax * zmax / (float(Ks[:, 0].min()) * min(bases)) / 16.0
    cos_t = min(abs(float(P[2, 2])) for P in Ps)   # the view's axis (third row of R) against the plane's normal e_z
    tan_t = np.sqrt(1.0 - cos_t * cos_t) / cos_t
    e95 = 0.5 + 16.0 * (block // 2) * max(bases) * tan_t / zmin + 16.0 * (3.0 - 2.0 * np.sqrt(2.0)) / 2.0
    dist = np.abs(pts[:, 2] - inp.STEREO_Z0)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    per_pair = [float(np.nanmedian(np.abs(ref.to_world(K, P.reshape(12), xs, ys, z)[2] - inp.STEREO_Z0))) for K, P, z in zip(Ks, Ps, D)]
    print(f"fused cloud {len(pts)} points (per view {counts}), per-pair clouds {sums}; one quantum of 1/16 px {quantum:.3e}; distance from the plane: median "
          f"{np.median(dist):.3e} = {np.median(dist) / quantum:.2f} q (bound 1 q), 95 % {np.quantile(dist, 0.95):.3e} = {np.quantile(dist, 0.95) / quantum:.2f} q "
          f"(bound {e95:.2f} q, tilt {np.degrees(np.arctan(tan_t)):.1f} deg, depths {zmin:.3f} .. {zmax:.3f}), largest {dist.max():.3e}; per-pair medians {per_pair}")
    assert len(pts) > 2000
    assert len(pts) < sum(sums)                      # fewer points than the concatenation of the per-pair clouds
    assert np.median(dist) <= quantum
    assert np.quantile(dist, 0.95) <= e95 * quantum
    assert np.median(dist) <= min(per_pair)
    # the composition, step by step: the same depth maps through fuse_depth_maps and the restatement
    r = ref.fuse(D, Ks, Ps, nb, rel_tol=0.02, unique=True)
    assert r["counts"].tolist() == counts
    want = np.concatenate(ref.compact(r["points"], r["mask"]))
    assert float(np.max(np.abs(pts - want))) <= MARGIN * inp.FUSE_GAP * float(np.max(np.abs(want)))
    tr = fusion.fuse_stereo_pairs(images, intr, ext, pairs, 32, transform=inp.TRANSFORM, **opts)[0]
    assert np.allclose(tr, pts @ inp.TRANSFORM[:, :3].T + inp.TRANSFORM[:, 3], atol=1e-12)
    with pytest.raises(ValueError, match="^pairs"):
        fusion.fuse_stereo_pairs(images, intr, ext, [(0, 0)], 32)
