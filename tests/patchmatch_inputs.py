"""Fixed inputs of the PatchMatch tests, from the seeded generators and analytic scenes of tests/fusion_inputs.py and
tests/sweep_inputs.py: nothing is committed but this code.  ``CASES`` names every input set the device tests use;
tests/test_patchmatch_reference.py asserts for each of them that no floating-point decision of the rule sits near its threshold, which
is the device's licence to exact equality."""
import functools

import numpy as np

from tests import fusion_inputs as fi
from tests import sweep_inputs as si

# The float64-versus-longdouble gap of the restatement (tests/patchmatch_reference.py decision_margins) over every case below: PM_GAP
# the largest |float64 - longdouble| of 16 u + 0.5 and 16 v + 0.5 (in sixteenths of a pixel) over the samples whose rounding can decide
# anything, PM_N2_GAP the same for n_2 and PM_OMEGA_GAP for omega.  tests/test_patchmatch_reference.py recomputes all three.
PM_GAP = 8.0e-12
PM_N2_GAP = 5.0e-16
PM_OMEGA_GAP = 2.5e-16
MARGIN = 8.0

RING_RANGE = (0.8, 1.2)


def _case(images, K, ext, nb, depth_range, **opts):
    return dict(images=np.array(images), K=K, ext=ext, neighbours=nb, depth_range=depth_range), opts


def _ring_case(crop=(48, 40), C=5, step=7.0, lists=None, depth_range=RING_RANGE, **opts):
    images, K, ext = si.ring(C, step, crop)
    o = dict(iterations=2, census=(5, 5), stride=1)
    o.update(opts)
    return _case(images, K, ext, si.ring_lists(C) if lists is None else lists, depth_range, **o)


@functools.lru_cache(maxsize=None)
def ring_truth(crop=(48, 40)):
    """The true z-depth of the ring's textured plane in every view."""
    images, K, ext = si.ring(5, 7.0, crop)
    d = fi.render(K, ext, images.shape[2], images.shape[1], plane=(np.array([0.0, 0.0, 1.0]), fi.STEREO_Z0), sphere=None)
    d.setflags(write=False)
    return d


def _start_depth_with_holes():
    """A start a sweep could have made: the truth off by up to 2 %, every kind of invalid depth in about 2 % of the pixels each."""
    d = ring_truth() * (1.0 + 0.02 * np.sin(np.arange(48)[None, None, :] * 0.7 + np.arange(40)[None, :, None] * 0.3))
    return _ring_case(depth=fi.add_invalid(d, 303))


@functools.lru_cache(maxsize=None)
def _first_iteration_planes():
    from tests import patchmatch_reference as ref

    a, o = _ring_case(iterations=1)
    p = ref.patchmatch(**a, **o)["plane"].copy()
    p[0, 10:14, 10:20] = np.nan            # entries a caller spoiled: redrawn
    p[1, 20:24, 8:12, 0] = 5.0             # outside the range
    p[2, 6:9, 30:34, 1] = 1.0              # steeper than the bound
    p.setflags(write=False)
    return p


def _facing():
    _, K, E = fi.facing_pair()
    return _case(si.noise_images(3, 64, 48, 11), K, E, [[1, 2], [0, 2], [1, 0]], (5.0, 7.0), iterations=1, census=(3, 3), stride=1)


def _no_overlap():
    _, K, E = fi.no_overlap()
    return _case(si.noise_images(4, 64, 48, 12), K, E, [[2, 3], [3], [0, 1], [1]], (2.0, 3.2), iterations=1, census=(3, 3), stride=1)


# name -> () -> (inputs of refine_depth_maps, options): every input set of tests/test_gpu_patchmatch.py.  The device's tile is 32 x 16
# (8 x 64, 16 x 32 and 64 x 8 by override); crops are 48 x 40, census 5 x 5 at stride 1 and 2 iterations unless the case says otherwise.
CASES = {
    "ring": lambda: _ring_case(crop=None, iterations=1),
    "base": lambda: _ring_case(),
    "base_permuted": lambda: _ring_case(lists=si.ring_lists(5, order=(2, -1, -2, 1))),
    "shape_31x33": lambda: _ring_case(crop=(31, 33)),
    "shape_33x31": lambda: _ring_case(crop=(33, 31)),
    "shape_65x33": lambda: _ring_case(crop=(65, 33), census=(3, 3)),
    "shape_20x14": lambda: _ring_case(crop=(20, 14), census=(3, 3)),
    "narrower_than_footprint": lambda: _ring_case(crop=(4, 40)),
    "lower_than_footprint": lambda: _ring_case(crop=(40, 4)),
    "footprint_exactly": lambda: _ring_case(crop=(5, 5)),
    "strict_5x5": lambda: _ring_case(crop=(9, 9)),
    "start_depth_holes": _start_depth_with_holes,
    "start_planes": lambda: _ring_case(planes=np.array(_first_iteration_planes()), first_iteration=1, iterations=1),
    "iterations_0": lambda: _ring_case(iterations=0),
    "iterations_3": lambda: _ring_case(crop=(33, 31), iterations=3),
    "nbr_0_and_1": lambda: _ring_case(lists=[[1], [0], [], [4], [3]]),
    "nbr_16": lambda: _ring_case(C=17, step=2.0, crop=(24, 20), lists=[[j for j in range(17) if j != i] for i in range(17)], iterations=1),
    "facing": _facing,
    "no_overlap": _no_overlap,
    "census_3x3": lambda: _ring_case(census=(3, 3)),
    "census_9x7": lambda: _ring_case(census=(9, 7), iterations=1),
    "stride_3": lambda: _ring_case(stride=3),
    "truncate_1": lambda: _ring_case(truncate=1),
    "truncate_full": lambda: _ring_case(truncate=24),
    "wrange_per_view": lambda: _ring_case(depth_range=np.array([[0.8 + 0.01 * v, 1.2 - 0.008 * v] for v in range(5)])),
    "tight_slant": lambda: _ring_case(max_slant=5.0),
    "seed_1": lambda: _ring_case(seed=0x9e3779b97f4a7c15),
}
