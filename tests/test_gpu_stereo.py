"""The stereo matcher on the device (pycamset_amd/stereo.py, csrc/ba_stereo.hpp) against the NumPy restatement (tests/stereo_reference.py).

The matcher is integer arithmetic from end to end: ``disp``, ``cost`` and ``status`` must be BIT-IDENTICAL to the restatement.  The
reprojection is FP64: it is held to MARGIN = 8 x STEREO_GAP (tests/stereo_inputs.py: the restatement's own float64-versus-longdouble gap,
relative to the largest coordinate), the margin the other suites give a different operation order and fused multiply-adds; its mask,
NaN pattern and the compaction's order must be identical (tests/test_stereo_reference.py asserts that no depth sits near a bound).

No golden from the reference exists for this row: its reconstruction_utils.py imports cv2 and pyvista at module level, neither is
available where goldens are made, and OpenCV's StereoBM is not reproduced bit for bit; the rule is the library's own (include/pcs_hip.h)."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import imaging, stereo
from tests import stereo_inputs as inp
from tests import stereo_reference as ref

pytestmark = pytest.mark.gpu
MARGIN = 8.0
STAGES = {"none": dict(texture_threshold=0, uniqueness_ratio=0, lr_max_diff=-1), "texture": dict(texture_threshold=10, uniqueness_ratio=0, lr_max_diff=-1),
          "uniqueness": dict(texture_threshold=0, uniqueness_ratio=15, lr_max_diff=-1), "left_right": dict(texture_threshold=0, uniqueness_ratio=0, lr_max_diff=1),
          "all": dict(texture_threshold=10, uniqueness_ratio=15, lr_max_diff=1)}


@functools.lru_cache(maxsize=None)
def pair():
    return inp.textured_pair()


def check(L, R, D, block, valid=None, what="", **kw):
    """One pair or a stack through the device and the restatement: all three outputs bit for bit.  -> the device's (disp, cost, status)."""
    got = stereo.stereo_match(L, R, D, block, valid=valid, return_cost=True, return_status=True, **kw)
    if L.ndim == 2:
        o = ref.match(L, R, D, block, valid=valid, **kw)
        want = (o["disp"], o["cost"], o["status"])
    else:
        want = ref.match_stack(L, R, D, block, valid=valid, **kw)
    for g, w, name in zip(got, want, ("disp", "cost", "status")):
        bad = np.argwhere(g != w)
        assert g.dtype == w.dtype and g.shape == w.shape and bad.size == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


@pytest.mark.parametrize("min_disp,D,block", [(0, 32, 7), (0, 24, 5), (-3, 21, 9), (2, 17, 3), (0, 1, 5), (-20, 16, 5)])
@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("cap", [31, 0])
def test_textured_pair(min_disp, D, block, stage, cap):
    L, R = pair()
    kw = dict(STAGES[stage], min_disp=min_disp, prefilter_cap=cap)
    if cap == 0:
        kw["texture_threshold"] = 0
    _, _, status = check(L, R, D, block, **kw)
    assert (status != ref.NOT_STRICT).any()


@pytest.mark.parametrize("D,block", [(16, 7), (8, 3)])
@pytest.mark.parametrize("min_disp", [1, 0, -4])
def test_exactly_one_strict_column_and_none(D, block, min_disp):
    """The strict columns are r + max(d_max, 0) .. W - 1 - r + min(min_disp, 0).  With the disparities 1 .. D that is one column at
    W = D + 2r + 1 and none at W = D + 2r; with another min_disp the two widths move with it.  With none the call is valid, everything
    comes back invalid and only the fill is launched."""
    L, R = pair()
    r = block // 2
    one = 2 * r + 1 + max(min_disp + D - 1, 0) - min(min_disp, 0)
    assert min_disp != 1 or one == D + 2 * r + 1
    for W in (one, one - 1):
        disp, cost, status = check(L[:, :W].copy(), R[:, :W].copy(), D, block, min_disp=min_disp, lr_max_diff=1, what=f"W={W}")
        strict = status != ref.NOT_STRICT
        assert strict.any(axis=0).sum() == (1 if W == one else 0)
        if W == one - 1:
            assert np.all(disp == 16 * (min_disp - 1)) and np.all(cost == -1)


@pytest.mark.parametrize("W", [63, 64, 65, 129])
@pytest.mark.parametrize("H", ["2r+1", "2r+2", 33])
def test_ragged_shapes(W, H):
    L, R = pair()
    block, D = 5, 12
    H = {"2r+1": block, "2r+2": block + 1}.get(H, H)
    check(L[:H, :W].copy(), R[:H, :W].copy(), D, block, lr_max_diff=1, what=f"{H}x{W}")
    check(L[3:3 + H, 11:11 + W].copy(), R[3:3 + H, 11:11 + W].copy(), D, block, min_disp=-5, lr_max_diff=0, what=f"{H}x{W} negative")


def test_row_pitch_inside_a_larger_tensor():
    L, R = pair()
    H, W = L.shape
    bufL = torch.full((2, H, W + 23), 7, dtype=torch.uint8, device="cuda")
    bufR = torch.full((2, H, W + 23), 201, dtype=torch.uint8, device="cuda")   # the bytes past W differ between the two
    Ls, Rs = np.stack([L, L[::-1]]), np.stack([R, R[::-1]])
    bufL[:, :, :W] = torch.from_numpy(Ls.copy()).cuda()
    bufR[:, :, :W] = torch.from_numpy(Rs.copy()).cuda()
    vL, vR = bufL[:, :, :W], bufR[:, :, :W]
    assert imaging._pitched(vL[..., None]) == W + 23
    got = stereo.stereo_match(vL, vR, 32, 7, lr_max_diff=1, return_cost=True, return_status=True)
    want = ref.match_stack(Ls, Rs, 32, 7, lr_max_diff=1)
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and np.array_equal(g.cpu().numpy(), w)


def test_three_pairs_with_different_contents():
    L, R = pair()
    L2, R2 = inp.textured_pair(seed=777)
    Ls, Rs = np.stack([L, L2, R]), np.stack([R, R2, L])   # the third pair swapped: its true disparities are negative
    check(Ls, Rs, 32, 7, min_disp=-16, lr_max_diff=1)


def test_constant_pair_takes_the_smallest_disparity():
    L, R = inp.constant_pair()
    for min_disp in (0, -2):
        disp, cost, status = check(L, R, 8, 5, min_disp=min_disp, texture_threshold=0, uniqueness_ratio=0)
        strict = status != ref.NOT_STRICT
        assert strict.any() and np.all(disp[strict] == 16 * min_disp) and np.all(cost[strict] == 0)
    _, _, status = check(L, R, 8, 5, lr_max_diff=0)   # with the defaults a constant image has no texture and no unique winner
    strict = status != ref.NOT_STRICT
    assert np.all(status[strict] & ref.TEXTURE) and np.all(status[strict] & ref.UNIQUENESS)


def test_the_references_parameters():
    """block 25 and 256 disparities (stereo_reconstruct's defaults) on a 48 x 352 generated pair."""
    L, R = inp.wide_pair()
    assert L.shape == (48, 352)
    disp, _, status = check(L, R, 256, 25, lr_max_diff=1)
    ok = status == 0
    assert ok.sum() > 100 and 16 * 20 <= np.median(disp[ok]) <= 16 * 60


@pytest.mark.parametrize("tw,sh", [(1, 1), (7, 3), (32, 16), (64, 4096)])
def test_any_tiling_gives_the_same_bits(monkeypatch, tw, sh):
    """The tile width and the strip length are the library's choice (an occupancy model); the environment overrides them."""
    monkeypatch.setenv("PCS_STEREO_TILE_COLUMNS", str(tw))
    monkeypatch.setenv("PCS_STEREO_STRIP_ROWS", str(sh))
    L, R = pair()
    vL, vR = inp.holes(L.shape)
    check(L, R, 32, 7, valid=(vL, vR), lr_max_diff=1)
    check(L[:, :70].copy(), R[:, :70].copy(), 9, 5, min_disp=-4, lr_max_diff=0)
    if tw == 7:
        check(*inp.wide_pair(), 256, 25, lr_max_diff=1)


def test_validity_planes_with_holes():
    L, R = pair()
    vL, vR = inp.holes(L.shape)
    _, _, status = check(L, R, 32, 7, valid=(vL, vR), lr_max_diff=1)
    assert (status & ref.VALIDITY).any() and (status[status != ref.NOT_STRICT] & ref.VALIDITY == 0).any()
    Ls, Rs = np.stack([L, L]), np.stack([R, R])
    check(Ls, Rs, 32, 7, valid=(np.stack([vL, np.ones_like(vL)]), np.stack([vR, vR])))


def test_as_float_and_integer_shift():
    L, R = inp.shifted_pair(5)
    d16 = stereo.stereo_match(L, R, 16, 7, lr_max_diff=1)
    f = stereo.stereo_match(L, R, 16, 7, lr_max_diff=1, as_float=True)
    ok = d16 != -16
    assert f.dtype == np.float32 and np.array_equal(np.isnan(f), ~ok) and np.array_equal(f[ok], d16[ok].astype(np.float32) / 16)
    assert ok.sum() > 100 and np.max(np.abs(d16[ok].astype(int) - 80)) <= 8


# ---- reprojection and compaction --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud():
    disp, Q, T, invalid = inp.cloud_inputs()
    return disp, Q, T, invalid, {t: ref.reproject(disp, Q, inp.DEPTH_RANGE, T if t else None, invalid) for t in (False, True)}


@pytest.mark.parametrize("with_T", [False, True])
def test_reprojection(with_T):
    disp, Q, T, invalid, refs = cloud()
    want, mask_r, _ = refs[with_T]
    p64, m64 = stereo.disparity_to_points(disp, Q, inp.DEPTH_RANGE, transform=T if with_T else None, invalid=invalid, dtype=np.float64)
    p32, m32 = stereo.disparity_to_points(disp, Q, inp.DEPTH_RANGE, transform=T if with_T else None, invalid=invalid, dtype=np.float32)
    assert np.array_equal(m64, mask_r) and np.array_equal(m32, mask_r) and m64.dtype == np.uint8
    m = mask_r.astype(bool)
    assert np.all(np.isnan(p64[~m])) and np.all(np.isfinite(p64[m])) and np.array_equal(np.isnan(p32), np.isnan(p64))
    gap = float(np.max(np.abs(p64[m] - want[m]))) / float(np.max(np.abs(want[m])))
    print(f"reprojection transform={with_T}: gap {gap:.2e} (bound {MARGIN * inp.STEREO_GAP:.2e})")
    assert gap <= MARGIN * inp.STEREO_GAP
    assert p32.dtype == np.float32 and np.array_equal(p32[m], p64[m].astype(np.float32))   # rounded once
    one, _ = stereo.disparity_to_points(disp[2], Q[2], inp.DEPTH_RANGE, dtype=np.float64)   # a single plane with its own Q
    if not with_T:
        assert one.shape == disp[2].shape + (3,) and np.array_equal(one, p64[2])
    f, _ = stereo.disparity_to_points(np.where(disp == invalid, np.nan, disp / 16.0), Q, inp.DEPTH_RANGE, transform=T if with_T else None, dtype=np.float64)
    assert np.array_equal(f, p64, equal_nan=True)   # float disparities with NaN where rejected: the same points


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compaction_order_counts_and_values(dtype):
    disp, Q, T, invalid, refs = cloud()
    _, mask_r, _ = refs[False]
    values = (np.arange(disp.size, dtype=np.int64).reshape(disp.shape) * 7 % 251).astype(np.uint8)
    pts, mask = stereo.disparity_to_points(disp, Q, inp.DEPTH_RANGE, invalid=invalid, dtype=dtype)
    clouds = stereo.disparity_to_points(disp, Q, inp.DEPTH_RANGE, invalid=invalid, dtype=dtype, values=values, compact=True)
    want = ref.compact(pts, mask_r, values)
    counts = [len(c[0]) for c in clouds]
    assert counts == [int(m.sum()) for m in mask_r] and counts[1] == 0 and counts[2] == mask_r[2].size and 0 < counts[0] < mask_r[0].size
    for (p, v), (pw, vw) in zip(clouds, want):
        assert p.dtype == np.dtype(dtype) and p.shape == pw.shape and np.array_equal(p, pw) and np.array_equal(v, vw)
    bare = stereo.disparity_to_points(disp, Q, inp.DEPTH_RANGE, invalid=invalid, dtype=dtype, compact=True)
    assert all(np.array_equal(b, c[0]) for b, c in zip(bare, clouds))
    big = np.tile(disp[0], (2, 45, 9))   # several thousand blocks: the scan's carry across its chunks of 1024
    assert big.size // 256 > 2048
    pb, mb = stereo.disparity_to_points(big, Q[0], inp.DEPTH_RANGE, invalid=invalid, dtype=dtype)
    cb = stereo.disparity_to_points(big, Q[0], inp.DEPTH_RANGE, invalid=invalid, dtype=dtype, compact=True)
    for i in range(2):
        assert np.array_equal(cb[i], pb[i].reshape(-1, 3)[np.flatnonzero(mb[i])])


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
Z0, RES = 1.0, (96, 64)
INTR_A = np.array([118.0, 47.1, 119.0, 31.6, -0.06, 0.015, 0.0008, -0.0006, 0.0])
INTR_B = np.array([121.0, 48.3, 120.5, 32.2, -0.05, 0.01, -0.0005, 0.0007, 0.0])


def _ext():
    from scipy.spatial.transform import Rotation

    Ra = Rotation.from_rotvec([0.01, -0.015, 0.005]).as_matrix()
    Rb = Rotation.from_rotvec([-0.012, 0.02, -0.008]).as_matrix()
    ca, cb = np.array([-0.06, 0.002, 0.0]), np.array([0.06, -0.001, 0.004])
    return np.concatenate([Ra, (-Ra @ ca)[:, None]], axis=1), np.concatenate([Rb, (-Rb @ cb)[:, None]], axis=1)


def _texture(X, Y):
    return 127.5 + 45.0 * np.sin(61.0 * X + 2.0 * np.sin(23.0 * Y)) + 40.0 * np.sin(47.0 * Y + 13.0 * X * X) + 35.0 * np.sin(29.0 * (X + Y) + 5.0 * np.cos(37.0 * X))


@functools.lru_cache(maxsize=None)
def scene():
    """A noise-free analytically textured plane Z = Z0 of the world, seen by two distorted cameras: each pixel's ray meets the plane."""
    W, H = RES
    ext = _ext()
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack([xs, ys], axis=-1).reshape(-1, 2)
    images = []
    for K, E in zip((INTR_A, INTR_B), ext):
        rays = imaging.pixel_rays(pix, K, ext=E[None], world=True)
        c = -E[:, :3].T @ E[:, 3]
        s = (Z0 - c[2]) / rays[:, 2]
        P = c[None, :] + s[:, None] * rays
        images.append(np.clip(np.rint(_texture(P[:, 0], P[:, 1])), 0, 255).astype(np.uint8).reshape(H, W))
    return images[0], images[1], ext[0], ext[1]


def test_end_to_end_plane():
    A, B, Ea, Eb = scene()
    opts = dict(num_disp=32, block=9, depth_range=(0.2, 3.0), lr_max_diff=1)
    clouds = stereo.stereo_reconstruct(A, B, INTR_A, Ea, INTR_B, Eb, frame="rectified", dtype=np.float64, **opts)
    ra, rb, Q, disp, min_disp = stereo.stereo_reconstruct.last
    assert min_disp == 0
    # the separate device calls, bit for bit
    ra2, rb2, Q2, va, vb = imaging.rectify_images(A, B, INTR_A, Ea, INTR_B, Eb, return_valid=True)
    R_a = imaging.rectify_images.last[0]
    disp2 = stereo.stereo_match(ra2, rb2, 32, 9, valid=(va, vb), lr_max_diff=1)
    sep = stereo.disparity_to_points(disp2, Q2, (0.2, 3.0), values=ra2, compact=True, dtype=np.float64, invalid=-16)
    assert np.array_equal(ra, ra2) and np.array_equal(rb, rb2) and np.array_equal(Q, Q2) and np.array_equal(disp, disp2)
    assert len(clouds) == 1 and np.array_equal(clouds[0][0], sep[0][0]) and np.array_equal(clouds[0][1], sep[0][1])
    # the disparities against the restatement on the rectified images read back
    o = ref.match(ra2, rb2, 32, 9, valid=(va[0], vb[0]), lr_max_diff=1)
    assert np.array_equal(disp2, o["disp"])
    # the plane: in camera a's rectified frame the world's plane Z = Z0 is n . X = h
    M, t = R_a @ Ea[:, :3], R_a @ Ea[:, 3]       # X_r = M X_w + t
    normal = M[:, 2]                             # M e_z
    h = Z0 + normal @ t
    f, base = Q[2, 3], 1.0 / abs(Q[3, 2])
    step = Z0 * Z0 / (f * base)
    pts_r, mask_r, _ = ref.reproject(o["disp"][None], Q, (0.2, 3.0), None, -16)
    dist_r = np.abs(pts_r[0][mask_r[0].astype(bool)] @ normal - h)
    print("surviving", int(mask_r.sum()), "of", mask_r.size, "median distance: restatement", np.median(dist_r), "one disparity step", step)
    assert mask_r.sum() > 500 and np.median(dist_r) <= step   # the input is fit for the demand
    dist = np.abs(clouds[0][0] @ normal - h)
    assert len(dist) == mask_r.sum() and np.median(dist) <= step
    # both orders of the pair, in the world
    w_ab = stereo.stereo_reconstruct(A, B, INTR_A, Ea, INTR_B, Eb, frame="world", dtype=np.float64, **opts)[0][0]
    w_ba = stereo.stereo_reconstruct(B, A, INTR_B, Eb, INTR_A, Ea, frame="world", dtype=np.float64, **opts)[0][0]
    assert stereo.stereo_reconstruct.last[4] == -31   # camera b is the right-hand one: the range is mirrored
    for w in (w_ab, w_ba):
        print("world cloud", len(w), "median |z - Z0|", np.median(np.abs(w[:, 2] - Z0)))
        assert len(w) > 500 and np.median(np.abs(w[:, 2] - Z0)) <= step
    assert np.allclose(w_ab, (clouds[0][0] - t) @ M, atol=1e-12)
