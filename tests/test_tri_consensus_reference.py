"""The view-pair consensus of the triangulation without a GPU: the sampler of the NumPy restatement (tests/tri_consensus_reference.py),
the restatement on the corrupted rigs of tests/tri_consensus_inputs.py, and the argument checks of the C entry points and of the Python
front end."""
import ctypes

import numpy as np
import pytest

from pycamset_amd import _capi
from pycamset_amd import compiled_helpers as hip_ch
from tests import tri_consensus_inputs as inp
from tests import tri_consensus_reference as cref


def test_sampler_pairs_are_distinct_in_range_and_reproducible():
    for V in (3, 4, 6, 7, 11, 12, 23, 24, 33, 200):
        for H in (1, 15, 64, 256):
            used = cref.n_used(V, H)
            assert used == min(H, V * (V - 1) // 2)
            pr = cref.pairs(5, 17, V, H)
            assert len(pr) == used and all(0 <= a < b < V for a, b in pr)
            assert pr == cref.pairs(5, 17, V, H)
            assert cref.pair(5, 17, V, H, used) is None
            all_pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
            if V * (V - 1) // 2 <= H:   # exhaustive exactly then: every pair once, in lexicographic order
                assert pr == all_pairs
            else:
                assert len(pr) == H
                if H >= 15:   # 15 draws and more: a coincidence of all of them is out of the question; keyed by the seed and the point
                    assert pr != all_pairs[:H] and pr != cref.pairs(6, 17, V, H) and pr != cref.pairs(5, 18, V, H)
    assert cref.n_used(2, 64) == 0 and cref.n_used(0, 64) == 0 and cref.pairs(0, 0, 2, 64) == []
    assert cref.exhaustive(6, 15) and not cref.exhaustive(7, 15)
    # the generator: splitmix64's first outputs for the state 0 (the published test vector of the finaliser on multiples of the increment)
    assert cref.mix64(cref.GOLDEN) == 0xE220A8397B1DCDAF and cref.mix64(2 * cref.GOLDEN) == 0x6E789E6AA1B965F4


def test_sampled_pairs_cover_the_views_evenly():
    """Every view position of a 24-view point is drawn: 256 pairs, 21.3 expected per position; none below 8."""
    cnt = np.zeros(24, dtype=int)
    for a, b in cref.pairs(0, 3, 24, 256):
        cnt[a] += 1
        cnt[b] += 1
    assert cnt.min() >= 8, cnt


@pytest.mark.parametrize("name", inp.RIGS)
def test_corruption_seeds_need_no_exception(name):
    """On the corrupted rigs the restatement's inliers are exactly the unmoved rows of every point with at least 4 views, and the best two
    scores of distinct pairs are more than 1e-9 apart, relative: no point needs the parity exception of the GPU test."""
    rec, start = inp.clean_rig(name)[:2]
    _, clean = inp.corrupted_rig(name)
    inlier, cinfo, score, gap = inp.restated(name)
    views = np.diff(start)
    many = views >= inp.MIN_VIEWS_CHECKED
    rows = inp.many_views(start)
    assert many.sum() == {"tri-perm": 491, "tri-refine": 288}[name]
    assert np.array_equal(inlier[rows], clean[rows])
    assert np.all(cinfo[many, 3] == 1) and np.all(cinfo[many, 1] >= 0) and np.all(np.isfinite(score[many]))
    assert np.array_equal(cinfo[many, 0], views[many] - np.where(views[many] < 8, 1, 2))
    print(name, "smallest relative gap between the best two scores:", gap[many].min())
    assert gap[many].min() > 1e-9
    # tri-perm is exhaustive for every point (at most 11 views with 64 hypotheses), tri-refine sampled for some
    exh = np.array([cref.exhaustive(int(v), inp.CONSENSUS["n_hypotheses"]) for v in views[many]])
    assert exh.all() if name == "tri-perm" else not exh.all()


def test_restatement_on_a_clean_table_flags_every_row():
    inlier, cinfo, _, _ = inp.restated("tri-perm", corrupted=False)
    start = inp.clean_rig("tri-perm")[1]
    assert inlier.all() and np.array_equal(cinfo[:, 0], np.diff(start))
    assert np.array_equal(cinfo[:, 3] == 1, np.diff(start) >= 3)


def test_consensus_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    assert lib.pcs_version() >= 116
    vp = ctypes.c_void_p
    assert lib.pcs_tri_set_consensus(None, 64, 8.0, 0) == _capi.PCS_ERR_ARG
    assert b"NULL handle" in lib.pcs_last_error()
    for bad in ((-1, 8.0, 0), (257, 8.0, 0), (64, 0.0, 0), (64, -1.0, 0), (64, float("nan"), 0), (64, float("inf"), 0)):
        # a (dummy) handle: the arguments are refused before the handle is touched
        assert lib.pcs_tri_set_consensus(vp(1), *bad) == _capi.PCS_ERR_ARG
        assert b"bad arguments" in lib.pcs_last_error()
    assert lib.pcs_tri_get_consensus(None, None, None, None) == _capi.PCS_ERR_ARG
    assert lib.pcs_tri_consensus_results(None, None, None, None) == _capi.PCS_ERR_ARG


def test_python_front_end_validates_consensus_options():
    rec, start, P, K, D, _ = inp.clean_rig("tri-perm")
    for kw in ({"consensus": -1}, {"consensus": 257}, {"consensus": 2.5}, {"consensus": True}, {"inlier_px": 0.0}, {"inlier_px": float("nan")},
               {"inlier_px": "x"}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5}):
        with pytest.raises(ValueError):
            hip_ch.nb_triangulate_full(rec, P, start, K, D, **kw)
        with pytest.raises(ValueError):
            hip_ch.refine_triangulation(rec, P, start, K, D, **kw)
        with pytest.raises(ValueError):
            hip_ch.multi_cam_triangulate(rec, P, K, D, refine=True, **kw)
    assert hip_ch.check_tri_consensus_options(64, 8, 2 ** 64 - 1) == (64, 8.0, 2 ** 64 - 1)
    assert hip_ch.check_tri_consensus_options(0, 0.5, 0) == (0, 0.5, 0)
    assert hip_ch.TRI_CONSENSUS_MAX == 256
