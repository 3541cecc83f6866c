"""The semi-global restatement against itself (CPU): the loop form against the vectorised form, the properties that follow from the rule
(include/pcs_hip.h, pcs_stereo_sgm), the argument checks of the Python layer and of the C ABI without a device, and the measurement
behind the claim that aggregation carries a disparity into untextured and repetitive regions.

No golden from the reference exists for this row: its matlab_stereo needs a MATLAB engine, and disparitySGM is not what the library
computes anyway.

One statement of the row's issue cannot hold as written and is replaced by what the rule does give: on a noise-free integer shift d0
"every strict pixel comes back as 16 d0".  S(d0) = 0 there, so d* = d0 and the status is 0, but the sub-pixel offset is the parabola
through S(d0 - 1), 0, S(d0 + 1), round(8 (m - p) / (m + p)), which is 0 only where the two neighbours are nearly equal (measured: offsets
-6 .. 6 occur).  The test asserts S(d0) = 0, d* = d0, status 0 and the offset formula on every strict pixel, hence |disp - 16 d0| <= 8."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi, stereo

from tests import sgm_reference as sgm
from tests import stereo_inputs as inp
from tests import stereo_reference as ref

CROP = (slice(0, 14), slice(60, 100))


@pytest.mark.parametrize("min_disp,D,census,paths,p1,p2,lr,uniq", [
    (0, 8, (5, 5), 8, 8, 32, 1, 15), (0, 8, (5, 5), 4, 8, 32, -1, 15), (-3, 9, (3, 3), 8, 3, 20, 0, 0), (2, 6, (9, 7), 4, 10, 120, 1, 30),
    (3, 1, (5, 3), 8, 1, 1, 1, 15), (-6, 5, (3, 5), 8, 0, 1023, 2, 100)])
def test_loop_form_equals_vectorised_form(min_disp, D, census, paths, p1, p2, lr, uniq):
    L, R = inp.textured_pair()
    L, R = L[CROP], R[CROP]
    assert L.shape == (14, 40)
    vL, vR = inp.holes(L.shape)
    for valid in (None, (vL, vR)):
        kw = dict(census=census, min_disp=min_disp, p1=p1, p2=p2, paths=paths, uniqueness_ratio=uniq, lr_max_diff=lr, valid=valid)
        a = sgm.match_loops(L, R, D, **kw)
        b = sgm.match(L, R, D, **kw)
        assert b["strict"].sum() > 0
        for x, k in zip(a, ("disp", "cost", "status")):
            assert np.array_equal(x, b[k]), k
        for (y, x), s in a[3].items():
            assert b["S"][:, y, x].tolist() == s


@pytest.mark.parametrize("paths", [4, 8])
def test_zero_penalties_sum_the_matching_cost(paths):
    L, R = inp.textured_pair()
    o = sgm.match(L, R, 24, census=(7, 5), min_disp=-3, p1=0, p2=0, paths=paths)
    s = o["strict"]
    assert s.sum() > 1000 and np.array_equal(o["S"][:, s], paths * o["C"][:, s])
    assert o["C"].max() <= 7 * 5 - 1 and o["C"][:, s].max() > 10


@pytest.mark.parametrize("d0,min_disp", [(5, 0), (-4, -8)])
def test_integer_shift(d0, min_disp):
    """Module docstring: S(d0) = 0 on every strict pixel, so d* = d0 with status 0; the offset is the rule's parabola."""
    L, R = inp.shifted_pair(d0)
    o = sgm.match(L, R, 16, min_disp=min_disp, uniqueness_ratio=0)
    s = o["strict"]
    k = d0 - min_disp
    assert s.sum() > 1000
    assert np.all(o["S"][k][s] == 0) and np.all(o["d_star"][s] == d0) and np.all(o["status"][s] == 0) and np.all(o["cost"][s] == 0)
    m, p = o["S"][k - 1][s], o["S"][k + 1][s]
    assert np.all(m > 0) and np.all(p > 0)   # no exact repeat in the seeded scene: the winner is the only zero
    want = np.floor_divide(32 * (m - p) + 2 * (m + p), 4 * (m + p))
    assert np.array_equal(o["disp"][s].astype(int) - 16 * d0, want) and np.max(np.abs(want)) <= 8


@pytest.mark.parametrize("min_disp,D,census", [(1, 16, (9, 7)), (0, 8, (3, 3)), (-4, 8, (5, 3)), (-12, 6, (7, 5)), (3, 1, (3, 9))])
def test_strict_rectangle(min_disp, D, census):
    """Rows rh .. H - 1 - rh, columns rw + max(d_max, 0) .. W - 1 - rw + min(min_disp, 0): exactly one strict column at
    W = cw + max(d_max, 0) - min(min_disp, 0) and none one narrower."""
    L, R = inp.textured_pair()
    cw, ch = census
    rw, rh = cw // 2, ch // 2
    d_max = min_disp + D - 1
    one = cw + max(d_max, 0) - min(min_disp, 0)
    for W in (one + 9, one, one - 1):
        for H in (ch + 2, ch, ch - 1):
            o = sgm.match(L[:H, :W], R[:H, :W], D, census=census, min_disp=min_disp)
            want = np.zeros((H, W), dtype=bool)
            want[rh:max(H - rh, rh), rw + max(d_max, 0):max(W - rw + min(min_disp, 0), 0)] = True
            assert np.array_equal(o["strict"], want)
            assert o["strict"].any(axis=0).sum() == (0 if H < ch else {one + 9: 10, one: 1, one - 1: 0}[W])
            assert np.all(o["status"][~want] == ref.NOT_STRICT) and np.all(o["disp"][~want] == 16 * (min_disp - 1)) and np.all(o["cost"][~want] == -1)
            assert np.all(o["status"][want] & ref.NOT_STRICT == 0) and np.all(o["status"] & ref.TEXTURE == 0)


BAD = [(dict(census=(4, 5)), "census"), (dict(census=(5, 6)), "census"), (dict(census=(9, 9)), "census"), (dict(census=(11, 7)), "census"), (dict(census=(1, 3)), "census"), (dict(p1=9, p2=8), "p1"),
       (dict(p1=-1), "p1"), (dict(p2=1024), "p2"), (dict(paths=6), "paths"), (dict(num_disp=0), "num_disp"), (dict(num_disp=257), "num_disp"),
       (dict(uniqueness_ratio=101), "uniqueness_ratio"), (dict(lr_max_diff=-2), "lr_max_diff"), (dict(min_disp=1025), "min_disp")]


@pytest.mark.parametrize("over,word", BAD)
def test_check_sgm_args_names_the_argument(over, word):
    kw = dict(num_disp=16, census=(9, 7), min_disp=0, p1=8, p2=32, paths=8, uniqueness_ratio=15, lr_max_diff=-1)
    assert stereo.check_sgm_args(1, 64, 32, 64, 64, **kw) == (16, 9, 7, 0, 8, 32, 8, 15, -1)
    assert stereo.check_sgm_args(1, 64, 32, 64, 64, **{**kw, "census": (13, 5), "num_disp": 256, "p1": 0, "p2": 1023, "paths": 4})   # 64 bits: the limits themselves
    kw.update(over)
    with pytest.raises(ValueError, match=word):
        stereo.check_sgm_args(1, 64, 32, 64, 64, **kw)
    L, R = inp.constant_pair()
    with pytest.raises(ValueError, match=word):   # refused before anything touches a device
        stereo.stereo_match(L, R, method="sgm", **kw)


def test_python_layer_keeps_the_two_methods_apart():
    L, R = inp.constant_pair()
    for kw, word in ((dict(block=7), "block"), (dict(prefilter_cap=31), "prefilter_cap"), (dict(texture_threshold=0), "texture_threshold")):
        with pytest.raises(ValueError, match=word):
            stereo.stereo_match(L, R, 8, method="sgm", **kw)
    with pytest.raises(ValueError, match="method"):
        stereo.stereo_match(L, R, 8, 5, method="sgbm")
    with pytest.raises(ValueError, match="block"):
        stereo.stereo_match(L, R, 8)
    assert stereo.sgm_pair_bytes(160, 40, 30) == 2 * 40 * 160 * 32 + 16 * 40 * 160


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------
def _sgm(lib, **over):
    a = dict(n=1, width=64, height=32, left=1, left_pitch=64, right=1, right_pitch=64, min_disp=0, num_disp=16, cw=9, ch=7, p1=8, p2=32, paths=8, uniq=15, lr=-1, disp=1)
    a.update(over)
    p = ctypes.c_void_p
    return lib.pcs_stereo_sgm(None, a["n"], a["width"], a["height"], p(a["left"]), a["left_pitch"], p(a["right"]), a["right_pitch"], a["min_disp"], a["num_disp"], a["cw"],
                              a["ch"], a["p1"], a["p2"], a["paths"], a["uniq"], a["lr"], None, None, p(a["disp"]), None, None, None)


@pytest.mark.parametrize("over,word", [
    (dict(cw=4), b"census_w"), (dict(ch=6), b"census_h"), (dict(cw=1), b"census_w"), (dict(cw=9, ch=9), b"bits"), (dict(cw=13, ch=7), b"bits"), (dict(p1=33), b"p1"),
    (dict(p1=-1), b"p1"), (dict(p2=1024), b"p2"), (dict(paths=6), b"paths"), (dict(num_disp=0), b"num_disp"), (dict(num_disp=257), b"num_disp"),
    (dict(min_disp=-1025), b"min_disp"), (dict(uniq=101), b"uniqueness_ratio"), (dict(lr=-2), b"lr_max_diff"), (dict(left_pitch=63), b"left_pitch"),
    (dict(right_pitch=10), b"right_pitch"), (dict(left=0), b"d_left"), (dict(disp=0), b"d_disp"), (dict(width=0), b"width"), (dict(), b"handle"),
    (dict(cw=13, ch=5, num_disp=256, p1=0, p2=1023, paths=4), b"handle")])
def test_sgm_argument_errors_need_no_gpu(over, word):
    lib = _capi.lib()
    assert lib.pcs_version() >= 124
    assert _sgm(lib, **over) == _capi.PCS_ERR_ARG
    assert word in lib.pcs_last_error(), lib.pcs_last_error()


def test_workspace_limit_argument_errors_need_no_gpu():
    lib = _capi.lib()
    assert lib.pcs_stereo_set_sgm_workspace(None, -1) == _capi.PCS_ERR_ARG and b"bytes" in lib.pcs_last_error()
    assert lib.pcs_stereo_set_sgm_workspace(None, 1 << 20) == _capi.PCS_ERR_ARG and b"handle" in lib.pcs_last_error()


# ---- what the aggregation is for -------------------------------------------------------------------------------------------------------------
def test_flat_patch_and_stripes_measured():
    """A measurement, not a threshold fixed in advance: on textured_pair() (40 x 160, 32 disparities from 0), the pixels of the noise-free
    flat patch and of the period-8 stripes, both in the 6 px plane, whose disparity comes back within 1 px of 6 px with every rejection
    off.  Restated SGM (census 9 x 7, P1 = 8, P2 = 32, 8 paths) against the restated block matcher at block 7 (prefilter cap 31):

        flat patch (520 px, 220 / 240 of them strict):   SGM 220, block matching 168
        stripes    (840 px, all strict):                 SGM 808, block matching 589

    Only that SGM's count is not below block matching's is asserted."""
    L, R = inp.textured_pair()
    H, W = L.shape
    y0, y1, x0, x1 = H // 4, 3 * H // 4, W // 8, W // 8 + 26   # as tests/stereo_inputs.textured_pair lays them out
    sx0, sx1 = W // 4 + 8, W // 4 + 38
    o = sgm.match(L, R, 32, census=(9, 7), p1=8, p2=32, paths=8, uniqueness_ratio=0)
    b = ref.match(L, R, 32, 7, texture_threshold=0, uniqueness_ratio=0)
    for name, (ya, yb, xa, xb) in (("flat patch", (y0, y1, x0, x1)), ("stripes", (y0 - 4, y1 + 4, sx0, sx1))):
        count = {}
        for who, out in (("sgm", o), ("block", b)):
            d, st = out["disp"][ya:yb, xa:xb].astype(int), out["status"][ya:yb, xa:xb]
            count[who] = int(((st == 0) & (np.abs(d - 16 * 6) <= 16)).sum())
        print(f"{name}: within 1 px of 6 px: SGM {count['sgm']}, block matching {count['block']}, of {(yb - ya) * (xb - xa)} pixels")
        assert count["sgm"] >= count["block"]
