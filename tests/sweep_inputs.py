"""Fixed inputs of the plane-sweep tests, from the seeded generators and analytic scenes of tests/fusion_inputs.py: nothing is committed
but this code.  ``CASES`` names every input set the device tests use; tests/test_sweep_reference.py asserts for each of them that no
floating-point decision of the rule sits near its threshold, which is the device's licence to exact equality."""
import functools

import numpy as np

from tests import fusion_inputs as fi

# The float64-versus-longdouble gap of the restatement (tests/sweep_reference.py decision_margins) over every case below: SWEEP_GAP the
# largest |float64 - longdouble| of 16 u + 0.5 and 16 v + 0.5 (in sixteenths of a pixel) over the samples whose rounding can decide
# anything, SWEEP_N2_GAP the same for n_2.  tests/test_sweep_reference.py recomputes both.
SWEEP_GAP = 3.6e-12
SWEEP_N2_GAP = 2.5e-15
MARGIN = 8.0

RING_RANGE, RING_STEPS = (0.8, 1.2), 32


def planes_of(depth_range, steps, spacing="depth"):
    from pycamset_amd.sweep import depth_planes   # host NumPy

    return depth_planes(depth_range, steps, spacing)


def ring_lists(V, order=(-1, 1, -2, 2)):
    """View i's neighbours: those of (i - 1, i + 1, i - 2, i + 2) that exist, in that order."""
    return [[i + d for d in order if 0 <= i + d < V] for i in range(V)]


@functools.lru_cache(maxsize=None)
def ring(C=5, step=7.0, crop=None):
    """-> (images (C, H, W) uint8, K (C, 4), ext (C, 3, 4)) of fusion_inputs.stereo_ring; ``crop`` = (w, h): the top-left part of every
    image, the same views with a smaller sensor."""
    images, intr, ext = fi.stereo_ring(C, step)
    if crop is not None:
        images = np.ascontiguousarray(images[:, :crop[1], :crop[0]])
    K = np.ascontiguousarray(intr[:, :4])
    for a in (images, K):
        a.setflags(write=False)
    return images, K, ext


def noise_images(V, W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(V, H, W), dtype=np.uint8)


def _case(images, K, ext, nb, planes, **opts):
    return dict(images=np.array(images), K=K, ext=ext, neighbours=nb, planes=planes), opts


def _ring_case(crop=(48, 40), C=5, step=7.0, lists=None, depth_range=(0.9, 1.1), steps=6, spacing="depth", planes=None, **opts):
    images, K, ext = ring(C, step, crop)
    z = planes_of(depth_range, steps, spacing) if planes is None else planes
    return _case(images, K, ext, ring_lists(C) if lists is None else lists, z, **opts)


def _per_view_planes():
    return np.stack([planes_of((0.9 + 0.004 * v, 1.1 - 0.003 * v), 6) for v in range(5)])


def _lists_with_an_empty_one():
    return [[1], [0], [], [4], [3]]


def _facing():
    _, K, E = fi.facing_pair()
    return _case(noise_images(3, 64, 48, 11), K, E, [[1, 2], [0, 2], [1, 0]], planes_of((5.0, 7.0), 5), census=(3, 3), box=1)


def _no_overlap():
    _, K, E = fi.no_overlap()
    return _case(noise_images(4, 64, 48, 12), K, E, [[2, 3], [3], [0, 1], [1]], planes_of((2.0, 3.2), 5), census=(3, 3), box=1)


# name -> () -> (inputs of sweep_depth_maps, options): every input set of tests/test_gpu_sweep.py.  The device's tile is 32 x 32 (8 x 128,
# 16 x 64 and 64 x 16 by override); it takes the planes one at a time, so no number of planes crosses a batch.
CASES = {
    "ring": lambda: _ring_case(crop=None, depth_range=RING_RANGE, steps=RING_STEPS),
    "ring_u15": lambda: _ring_case(crop=None, depth_range=RING_RANGE, steps=RING_STEPS, uniqueness_ratio=15),
    "ring_permuted": lambda: _ring_case(crop=None, depth_range=RING_RANGE, steps=RING_STEPS, lists=ring_lists(5, order=(2, -1, -2, 1))),
    "shape_31x33": lambda: _ring_case(crop=(31, 33)),
    "shape_33x31": lambda: _ring_case(crop=(33, 31)),
    "shape_20x14": lambda: _ring_case(crop=(20, 14), census=(3, 3), box=1),
    "shape_65x33": lambda: _ring_case(crop=(65, 33), census=(3, 3), box=0),
    "narrower_than_footprint": lambda: _ring_case(crop=(8, 40)),
    "lower_than_footprint": lambda: _ring_case(crop=(40, 8)),
    "footprint_exactly": lambda: _ring_case(crop=(9, 9)),
    "planes_1": lambda: _ring_case(planes=np.array([1.0])),
    "planes_2": lambda: _ring_case(planes=np.array([0.97, 1.02])),
    "planes_3": lambda: _ring_case(planes=np.array([0.95, 1.0, 1.05]), uniqueness_ratio=15),
    "planes_descending": lambda: _ring_case(planes=planes_of((0.9, 1.1), 7)[::-1].copy()),
    "nbr_0_and_1": lambda: _ring_case(lists=_lists_with_an_empty_one()),
    "nbr_16": lambda: _ring_case(C=17, step=2.0, crop=(40, 36), lists=[[j for j in range(17) if j != i] for i in range(17)], steps=4),
    "facing": _facing,
    "no_overlap": _no_overlap,
    "census_3x3": lambda: _ring_case(census=(3, 3)),
    "census_9x7": lambda: _ring_case(census=(9, 7), box=0, uniqueness_ratio=15),
    "box_0": lambda: _ring_case(box=0),
    "box_4": lambda: _ring_case(box=4),
    "truncate_1": lambda: _ring_case(truncate=1),
    "truncate_full": lambda: _ring_case(truncate=24 * 25, uniqueness_ratio=15),
    "planes_per_view": lambda: _ring_case(planes=_per_view_planes()),
    "inverse_spacing": lambda: _ring_case(spacing="inverse", steps=9, uniqueness_ratio=15),
}


def margin_inputs():
    """The input sets SWEEP_GAP and SWEEP_N2_GAP are measured over: every case of the device tests."""
    return [make()[0] for make in CASES.values()]
