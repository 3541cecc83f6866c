"""The stereo restatement against itself (CPU): the loop form against the vectorised form, and the conditions that make the device test
(tests/test_gpu_stereo.py) a fair demand, asserted on the restatement alone.

No golden from the reference exists for this row: its reconstruction_utils.py imports cv2 and pyvista at module level and neither is
available where the goldens are made, and OpenCV's StereoBM is not what the library computes anyway (its NORMALIZED_RESPONSE prefilter,
SIMD rounding and dispDescale formula are its own).  The rule is the library's, stated exactly in include/pcs_hip.h and restated in
tests/stereo_reference.py.

One condition of the issue cannot hold and is replaced by its proof: "a den = 0 case occurs".  den = 2 (m + p - 2 C*) with m, p >= C*,
so den = 0 needs m = C*, and then d* - 1 — a smaller disparity of the same cost — would have been the winner.  den > 0 on every
interior winner is asserted instead, together with the other zero-offset branch (the winner at an end of the range)."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi

from tests import stereo_inputs as inp
from tests import stereo_reference as ref

CROP = (slice(0, 14), slice(60, 100))


@pytest.mark.parametrize("min_disp,D,block,cap,lr,uniq", [
    (0, 8, 5, 31, 1, 15), (3, 8, 5, 31, -1, 15), (-3, 9, 3, 31, 0, 0), (0, 6, 7, 0, 1, 30), (2, 1, 5, 31, 1, 15), (-6, 5, 3, 8, 2, 100)])
def test_loop_form_equals_vectorised_form(min_disp, D, block, cap, lr, uniq):
    L, R = inp.textured_pair()
    L, R = L[CROP], R[CROP]
    vL, vR = inp.holes(L.shape)
    for valid in (None, (vL, vR)):
        kw = dict(min_disp=min_disp, prefilter_cap=cap, texture_threshold=10 if cap else 0, uniqueness_ratio=uniq, lr_max_diff=lr, valid=valid)
        a = ref.match_loops(L, R, D, block, **kw)
        b = ref.match(L, R, D, block, **kw)
        assert b["strict"].sum() > 0
        for x, k in zip(a, ("disp", "cost", "status")):
            assert np.array_equal(x, b[k]), k


def test_textured_pair_exercises_every_stage():
    L, R = inp.textured_pair()
    assert L.shape == (40, 160)
    o = ref.match(L, R, **inp.DEFAULTS, lr_max_diff=1)
    s = o["strict"]
    st = o["status"][s]
    frac = {b: float(np.mean((st & b) != 0)) for b in (ref.TEXTURE, ref.UNIQUENESS, ref.LEFT_RIGHT)}
    survive = float(np.mean(st == 0))
    print("strict", int(s.sum()), "flagged", frac, "surviving", survive)
    assert all(f >= 0.01 for f in frac.values()), frac
    assert survive >= 0.5
    Cm = np.where(o["ok"], o["C"], ref.BIG)
    ties = ((Cm == Cm.min(axis=0)[None]).sum(axis=0) > 1) & s
    print("tied minima", int(ties.sum()))
    assert ties.any()
    offs = set(np.unique(o["offset"][s]).tolist())
    print("offsets", sorted(offs))
    assert {-8, 8, 0} <= offs and any(v < 0 for v in offs) and any(v > 0 for v in offs)
    D = inp.DEFAULTS["num_disp"]
    k = o["d_star"] - inp.DEFAULTS["min_disp"]
    interior = s & (k > 0) & (k < D - 1)
    den = 2 * (o["m"] + o["p"] - 2 * o["cost"].astype(np.int64))
    assert interior.any() and np.all(den[interior] > 0)   # den = 0 cannot occur (module docstring)
    assert (s & ~interior).any()                           # the other zero-offset branch: the winner at an end of the range


@pytest.mark.parametrize("d0,min_disp", [(5, 0), (-4, -8), (0, -2)])
def test_integer_shift(d0, min_disp):
    L, R = inp.shifted_pair(d0)
    o = ref.match(L, R, 16, 7, min_disp=min_disp, lr_max_diff=1)
    ok = o["status"] == 0
    assert ok.sum() > 100
    assert np.all(o["d_star"][ok] == d0) and np.max(np.abs(o["disp"][ok].astype(int) - 16 * d0)) <= 8


def test_constant_pair_takes_the_smallest_disparity():
    L, R = inp.constant_pair()
    o = ref.match(L, R, 8, 5, min_disp=-2, texture_threshold=0, uniqueness_ratio=0)
    assert o["strict"].any() and np.all(o["d_star"][o["strict"]] == -2) and np.all(o["disp"][o["strict"]] == -32)


def measured_gap():
    disp, Q, T, invalid = inp.cloud_inputs()
    gap = 0.0
    for transform in (None, T):
        a, ma, _ = ref.reproject(disp, Q, inp.DEPTH_RANGE, transform, invalid)
        b, mb, _ = ref.reproject(disp, Q, inp.DEPTH_RANGE, transform, invalid, real=np.longdouble)
        assert np.array_equal(ma, mb)
        m = ma.astype(bool)
        gap = max(gap, float(np.max(np.abs(a[m] - b[m]))) / float(np.max(np.abs(a[m]))))
    return gap


def test_stereo_gap_is_the_pinned_one():
    gap = measured_gap()
    print("STEREO_GAP measured", gap)
    assert 0.5 * inp.STEREO_GAP <= gap <= inp.STEREO_GAP


def test_no_cloud_depth_sits_at_a_bound():
    """Then the mask, and with it the compaction's order, must be identical on the device: no z lies within the device's error bound
    (8 x STEREO_GAP x the largest coordinate) of lo or hi; the counts per pair are the three cases of the device test."""
    disp, Q, T, invalid = inp.cloud_inputs()
    pts, mask, z = ref.reproject(disp, Q, inp.DEPTH_RANGE, None, invalid)
    fin = np.isfinite(z)
    bound = 8.0 * inp.STEREO_GAP * float(np.max(np.abs(z[fin])))
    dist = min(np.min(np.abs(z[fin] - inp.DEPTH_RANGE[0])), np.min(np.abs(z[fin] - inp.DEPTH_RANGE[1])))
    print("nearest depth to a bound", dist, "device bound", bound)
    assert dist > 1e6 * bound
    counts = mask.reshape(mask.shape[0], -1).sum(axis=1)
    assert 0 < counts[0] < mask[0].size and counts[1] == 0 and counts[2] == mask[2].size
    assert not np.all(fin)   # a point at infinity is among the inputs


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------
def _match(lib, **over):
    a = dict(n=1, width=64, height=32, left=1, left_pitch=64, right=1, right_pitch=64, min_disp=0, num_disp=16, block=7, cap=31, tex=10, uniq=15, lr=-1)
    a.update(over)
    p = ctypes.c_void_p
    return lib.pcs_stereo_match(None, a["n"], a["width"], a["height"], p(a["left"]), a["left_pitch"], p(a["right"]), a["right_pitch"], a["min_disp"], a["num_disp"], a["block"],
                                a["cap"], a["tex"], a["uniq"], a["lr"], None, None, p(1), None, None, None)


@pytest.mark.parametrize("over,word", [
    (dict(block=8), b"block"), (dict(block=33), b"block"), (dict(num_disp=0), b"num_disp"), (dict(cap=0, tex=10), b"texture_threshold"),
    (dict(left_pitch=63), b"left_pitch"), (dict(right_pitch=10), b"right_pitch"), (dict(left=0), b"d_left"), (dict(right=0), b"d_right"),
    (dict(min_disp=1025), b"min_disp"), (dict(num_disp=1025), b"num_disp"), (dict(cap=64), b"prefilter_cap"), (dict(uniq=101), b"uniqueness_ratio"),
    (dict(lr=-2), b"lr_max_diff"), (dict(width=0), b"width"), (dict(), b"handle")])
def test_match_argument_errors_need_no_gpu(over, word):
    lib = _capi.lib()
    assert lib.pcs_version() >= 123
    assert _match(lib, **over) == _capi.PCS_ERR_ARG
    assert word in lib.pcs_last_error(), lib.pcs_last_error()


def test_reproject_and_compact_argument_errors_need_no_gpu():
    lib = _capi.lib()
    p = ctypes.c_void_p
    Q = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    bad = (ctypes.c_double * 16)(*([np.nan] + [0.0] * 15))
    inf = float("inf")
    assert lib.pcs_stereo_reproject(None, 1, 8, 8, p(1), 0, None, 1, -inf, inf, None, p(1), 1, p(1), None, None) == _capi.PCS_ERR_ARG and b"Q" in lib.pcs_last_error()
    assert lib.pcs_stereo_reproject(None, 1, 8, 8, p(1), 0, bad, 1, -inf, inf, None, p(1), 1, p(1), None, None) == _capi.PCS_ERR_ARG and b"not finite" in lib.pcs_last_error()
    assert lib.pcs_stereo_reproject(None, 2, 8, 8, p(1), 0, Q, 3, -inf, inf, None, p(1), 1, p(1), None, None) == _capi.PCS_ERR_ARG and b"n_Q" in lib.pcs_last_error()
    assert lib.pcs_stereo_reproject(None, 1, 8, 8, p(1), 0, Q, 1, -inf, inf, None, p(1), 7, p(1), None, None) == _capi.PCS_ERR_ARG and b"dtype" in lib.pcs_last_error()
    assert lib.pcs_stereo_reproject(None, 1, 8, 8, p(1), 0, Q, 1, -inf, inf, None, None, 1, p(1), None, None) == _capi.PCS_ERR_ARG and b"d_points" in lib.pcs_last_error()
    assert lib.pcs_stereo_reproject(None, 1, 8, 8, p(1), 0, Q, 1, -inf, inf, None, p(1), 1, p(1), None, None) == _capi.PCS_ERR_ARG and b"handle" in lib.pcs_last_error()
    assert lib.pcs_stereo_compact(None, 1, 8, 8, p(1), 1, p(1), p(1), 4, p(1), p(1), p(1), None) == _capi.PCS_ERR_ARG and b"values_pitch" in lib.pcs_last_error()
    assert lib.pcs_stereo_compact(None, 1, 8, 8, p(1), 1, p(1), p(1), 8, p(1), None, p(1), None) == _capi.PCS_ERR_ARG and b"d_out_values" in lib.pcs_last_error()
    assert lib.pcs_stereo_compact(None, 1, 8, 8, p(1), 1, p(1), None, 0, p(1), None, None, None) == _capi.PCS_ERR_ARG and b"d_counts" in lib.pcs_last_error()
    assert lib.pcs_stereo_compact(None, 1, 8, 8, p(1), 1, p(1), None, 0, p(1), None, p(1), None) == _capi.PCS_ERR_ARG and b"handle" in lib.pcs_last_error()
    assert lib.pcs_stereo_destroy(None) == _capi.PCS_OK
    ms = ctypes.c_float()
    assert lib.pcs_stereo_last_kernel_ms(None, ctypes.byref(ms)) == _capi.PCS_ERR_ARG


def test_python_checks_name_the_argument():
    from pycamset_amd import stereo

    L, R = inp.constant_pair()
    for kw, word in ((dict(block=8), "block"), (dict(num_disp=0), "num_disp"), (dict(prefilter_cap=0), "texture_threshold"), (dict(uniqueness_ratio=-1), "uniqueness_ratio")):
        with pytest.raises(ValueError, match=word):
            stereo.stereo_match(L, R, **{**dict(num_disp=8, block=5), **kw})
    with pytest.raises(ValueError, match="right"):
        stereo.stereo_match(L, R[:, :-1], 8, 5)
    with pytest.raises(ValueError, match="uint8"):
        stereo.stereo_match(L.astype(np.float32), R.astype(np.float32), 8, 5)
    with pytest.raises(ValueError, match="Q"):
        stereo.disparity_to_points(np.zeros((4, 4), dtype=np.int16), np.eye(3))
