"""The semi-global matcher on the device (pycamset_amd/stereo.py method="sgm", csrc/ba_stereo_sgm.hpp) against the NumPy restatement
(tests/sgm_reference.py).

The matcher is integer arithmetic from end to end: ``disp``, ``cost`` and ``status`` must be BIT-IDENTICAL to the restatement, for every
disparity range (one disparity, a full wave, one past a wave, two and four disparities per lane), every penalty pair up to the width
limits of L_r and S, every census window, every rejection stage, ragged shapes, and any chunking of a batch.  The reprojection behind
``stereo_reconstruct(method="sgm")`` is held to MARGIN x STEREO_GAP as in tests/test_gpu_stereo.py.

No golden from the reference exists for this row: its matlab_stereo needs a MATLAB engine, and the rule is the library's own."""
import functools

import numpy as np
import pytest
import torch

from pycamset_amd import _capi, imaging, stereo
from tests import sgm_reference as sgm
from tests import stereo_inputs as inp
from tests import stereo_reference as ref
from tests.test_gpu_stereo import INTR_A, INTR_B, MARGIN, scene

pytestmark = pytest.mark.gpu
STAGES = {"none": dict(uniqueness_ratio=0, lr_max_diff=-1), "uniqueness": dict(uniqueness_ratio=15, lr_max_diff=-1), "left_right_0": dict(uniqueness_ratio=0, lr_max_diff=0),
          "left_right_1": dict(uniqueness_ratio=0, lr_max_diff=1), "all": dict(uniqueness_ratio=15, lr_max_diff=1)}
RANGES = [(0, 32), (0, 24), (-3, 21), (2, 17), (0, 1), (-20, 16), (0, 16), (0, 64), (0, 65), (0, 128)]
PENALTIES = [(0, 0), (1, 1), (8, 32), (10, 120), (1023, 1023), (0, 1023)]


@functools.lru_cache(maxsize=None)
def pair():
    return inp.textured_pair()


@functools.lru_cache(maxsize=None)
def wide():
    return inp.wide_pair()


@functools.lru_cache(maxsize=None)
def stack5():
    L, R = pair()
    L2, R2 = inp.textured_pair(seed=777)
    L3, R3 = inp.textured_pair(seed=778, noise=4.0)
    return np.stack([L, L2, R, L3, L[::-1]]), np.stack([R, R2, L, R3, R[::-1]])   # the third pair swapped: its true disparities are negative


def check(L, R, D, valid=None, what="", **kw):
    """One pair or a stack through the device and the restatement: all three outputs bit for bit.  -> the device's (disp, cost, status)."""
    got = stereo.stereo_match(L, R, D, valid=valid, return_cost=True, return_status=True, method="sgm", **kw)
    if L.ndim == 2:
        o = sgm.match(L, R, D, valid=valid, **kw)
        want = (o["disp"], o["cost"], o["status"])
    else:
        want = sgm.match_stack(L, R, D, valid=valid, **kw)
    for g, w, name in zip(got, want, ("disp", "cost", "status")):
        bad = np.argwhere(g != w)
        assert g.dtype == w.dtype and g.shape == w.shape and bad.size == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


@pytest.mark.parametrize("min_disp,D", RANGES)
@pytest.mark.parametrize("paths", [4, 8])
def test_disparity_ranges(min_disp, D, paths):
    L, R = pair()
    _, _, status = check(L, R, D, min_disp=min_disp, paths=paths, uniqueness_ratio=15, lr_max_diff=1)
    assert (status != ref.NOT_STRICT).any() and not (status & ref.TEXTURE).any()


@pytest.mark.parametrize("min_disp,D", [(0, 256), (128, 128)])
def test_four_disparities_per_lane_and_the_references_range(min_disp, D):
    """wide_pair() (48 x 352): 256 disparities, and the reference's own call, the range (num_disp - 128, num_disp) at num_disp = 256."""
    L, R = wide()
    assert L.shape == (48, 352)
    disp, _, status = check(L, R, D, min_disp=min_disp, lr_max_diff=1)
    ok = status == 0
    assert (status != ref.NOT_STRICT).sum() > 100
    if min_disp == 0:
        assert ok.sum() > 100 and 16 * 20 <= np.median(disp[ok]) <= 16 * 60


@pytest.mark.parametrize("p1,p2", PENALTIES)
@pytest.mark.parametrize("paths", [4, 8])
def test_penalties(p1, p2, paths):
    L, R = pair()
    _, cost, _ = check(L, R, 32, p1=p1, p2=p2, paths=paths, lr_max_diff=1)
    check(L[:, :120].copy(), R[:, :120].copy(), 65, p1=p1, p2=p2, paths=paths)   # two disparities per lane
    assert cost.max() <= paths * (62 + p2)


@pytest.mark.parametrize("census", [(3, 3), (5, 5), (7, 5), (9, 7)])
def test_census_windows(census):
    L, R = pair()
    check(L, R, 32, census=census, lr_max_diff=1)
    check(L, R, 21, census=census, min_disp=-3, paths=4)


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("holes", [False, True])
def test_stages_and_validity_planes(stage, holes):
    L, R = pair()
    valid = inp.holes(L.shape) if holes else None
    _, _, status = check(L, R, 32, valid=valid, **STAGES[stage])
    strict = status != ref.NOT_STRICT
    for bit, on in ((ref.UNIQUENESS, STAGES[stage]["uniqueness_ratio"] > 0), (ref.LEFT_RIGHT, STAGES[stage]["lr_max_diff"] >= 0), (ref.VALIDITY, holes)):
        assert (status[strict] & bit).any() == on
    assert (status[strict] == 0).any()


@pytest.mark.parametrize("W", [63, 64, 65, 129])
@pytest.mark.parametrize("H", ["ch", "ch+1", 33])
def test_ragged_shapes(W, H):
    """H = ch: one strict row, every vertical and diagonal path has length one."""
    L, R = pair()
    census, D = (7, 5), 12
    H = {"ch": census[1], "ch+1": census[1] + 1}.get(H, H)
    check(L[:H, :W].copy(), R[:H, :W].copy(), D, census=census, lr_max_diff=1, what=f"{H}x{W}")
    check(L[3:3 + H, 11:11 + W].copy(), R[3:3 + H, 11:11 + W].copy(), D, census=census, min_disp=-5, lr_max_diff=0, what=f"{H}x{W} negative")


@pytest.mark.parametrize("min_disp,D,census", [(1, 16, (9, 7)), (0, 8, (3, 3)), (-4, 8, (5, 5))])
def test_exactly_one_strict_column_and_none(min_disp, D, census):
    L, R = pair()
    one = census[0] + max(min_disp + D - 1, 0) - min(min_disp, 0)
    for W in (one, one - 1):
        disp, cost, status = check(L[:, :W].copy(), R[:, :W].copy(), D, census=census, min_disp=min_disp, lr_max_diff=1, what=f"W={W}")
        strict = status != ref.NOT_STRICT
        assert strict.any(axis=0).sum() == (1 if W == one else 0)
        if W == one - 1:
            assert np.all(disp == 16 * (min_disp - 1)) and np.all(cost == -1)


def test_crops_taller_than_wide_and_wider_than_tall():
    """Strict rectangles of 34 x 9 and 6 x 139: the diagonal lines start on both edges, and most of them on the longer one."""
    L, R = pair()
    tall = check(L[:, 20:20 + 24].copy(), R[:, 20:20 + 24].copy(), 8, census=(9, 7), lr_max_diff=1, what="tall")
    assert (tall[2] != ref.NOT_STRICT).sum() == 34 * 9
    flat = check(L[:12].copy(), R[:12].copy(), 14, census=(9, 7), lr_max_diff=1, what="wide")
    assert (flat[2] != ref.NOT_STRICT).sum() == 6 * 139


def test_batch_chunks_give_the_same_bits():
    """Five different pairs with the workspace limit set for chunks of one, two and all five pairs; a limit below one pair's need raises
    and names the byte count."""
    Ls, Rs = stack5()
    n, H, W = Ls.shape
    D = 40
    per = stereo.sgm_pair_bytes(W, H, D)
    m = stereo._matcher(0)
    want = sgm.match_stack(Ls, Rs, D, min_disp=-16, lr_max_diff=1)
    try:
        for pairs in (1, 2, 5):
            m.set_sgm_workspace(pairs * per + (per // 2 if pairs < 5 else 0))
            got = stereo.stereo_match(Ls, Rs, D, min_disp=-16, lr_max_diff=1, return_cost=True, return_status=True, method="sgm")
            for g, w, name in zip(got, want, ("disp", "cost", "status")):
                assert np.array_equal(g, w), (pairs, name)
        m.set_sgm_workspace(per - 1)
        with pytest.raises(_capi.PcsError, match=str(per)) as e:
            stereo.stereo_match(Ls[0], Rs[0], D, method="sgm")
        assert e.value.code == _capi.PCS_ERR_ARG
        stereo.stereo_match(Ls[0, :, :20], Rs[0, :, :20], D, method="sgm")   # no strict pixel: only the fill runs, no workspace is needed
    finally:
        m.set_sgm_workspace(0)
    check(Ls[0], Rs[0], D)   # the default again


def test_row_pitch_inside_a_larger_tensor_on_another_stream():
    L, R = pair()
    H, W = L.shape
    bufL = torch.full((2, H, W + 23), 7, dtype=torch.uint8, device="cuda")
    bufR = torch.full((2, H, W + 23), 201, dtype=torch.uint8, device="cuda")   # the bytes past W differ between the two
    Ls, Rs = np.stack([L, L[::-1]]), np.stack([R, R[::-1]])
    bufL[:, :, :W] = torch.from_numpy(Ls.copy()).cuda()
    bufR[:, :, :W] = torch.from_numpy(Rs.copy()).cuda()
    vL, vR = bufL[:, :, :W], bufR[:, :, :W]
    assert imaging._pitched(vL[..., None]) == W + 23
    want = sgm.match_stack(Ls, Rs, 32, lr_max_diff=1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = stereo.stereo_match(vL, vR, 32, lr_max_diff=1, return_cost=True, return_status=True, method="sgm")
    side.synchronize()
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and np.array_equal(g.cpu().numpy(), w)


def test_two_runs_give_the_same_bits():
    L, R = wide()
    a = stereo.stereo_match(L, R, 128, lr_max_diff=1, return_cost=True, return_status=True, method="sgm")
    b = stereo.stereo_match(L, R, 128, lr_max_diff=1, return_cost=True, return_status=True, method="sgm")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_matcher_handle_times_the_call():
    L, R = pair()
    check(L, R, 32)
    assert stereo._matcher(0).last_kernel_ms() > 0.0


def test_end_to_end_plane():
    """stereo_reconstruct(method="sgm") on the synthetic rig of tests/test_gpu_stereo.py equals rectify + the restated match + the restated
    reprojection and compaction: disparity, mask and order identical, points within MARGIN x STEREO_GAP."""
    A, B, Ea, Eb = scene()
    opts = dict(num_disp=32, depth_range=(0.2, 3.0), lr_max_diff=1, method="sgm", census=(7, 5), p1=6, p2=40)
    clouds = stereo.stereo_reconstruct(A, B, INTR_A, Ea, INTR_B, Eb, frame="rectified", dtype=np.float64, **opts)
    ra, rb, Q, disp, min_disp = stereo.stereo_reconstruct.last
    assert min_disp == 0
    ra2, rb2, Q2, va, vb = imaging.rectify_images(A, B, INTR_A, Ea, INTR_B, Eb, return_valid=True)
    assert np.array_equal(ra, ra2) and np.array_equal(rb, rb2) and np.array_equal(Q, Q2)
    o = sgm.match(ra2, rb2, 32, census=(7, 5), p1=6, p2=40, valid=(va[0], vb[0]), lr_max_diff=1)   # one pair comes back as planes
    assert np.array_equal(disp, o["disp"])
    pts_r, mask_r, _ = ref.reproject(o["disp"][None], Q, (0.2, 3.0), None, -16)
    want = ref.compact(pts_r, mask_r, ra2[None])
    assert len(clouds) == 1 and mask_r.sum() > 500
    pts, grey = clouds[0]
    assert pts.shape == want[0][0].shape and np.array_equal(grey, want[0][1])   # the same pixels in the same order
    gap = float(np.max(np.abs(pts - want[0][0]))) / float(np.max(np.abs(want[0][0])))
    print(f"sgm end to end: {len(pts)} points, gap {gap:.2e} (bound {MARGIN * inp.STEREO_GAP:.2e})")
    assert gap <= MARGIN * inp.STEREO_GAP
    # camera b as the left-hand one: the range is mirrored, as for the block matcher
    stereo.stereo_reconstruct(B, A, INTR_B, Eb, INTR_A, Ea, frame="world", dtype=np.float64, **opts)
    assert stereo.stereo_reconstruct.last[4] == -31
