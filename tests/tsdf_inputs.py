"""Fixed inputs of the TSDF volume and surface-nets tests, built from the rendered rings of tests/fusion_inputs.py: nothing is committed
but this code.  ``CASES`` names every input set the device tests use (tests/test_gpu_tsdf.py); tests/test_tsdf_reference.py asserts for
each of them that no decision of the rule sits near its threshold.

TSDF_GAP and TSDF_DECISION_GAP are the float64-versus-longdouble gaps of the restatement (tests/tsdf_reference.py) over ``CASES``, with a
sum that is not rounded on store in either arithmetic.  TSDF_GAP: the largest |float64 - longdouble| of the per-node sums and of the
vertex coordinates, each relative to the largest magnitude of its array.  TSDF_DECISION_GAP: the same for the decision quantities (Y_z,
u + 0.5, v + 0.5, sdf + trunc, D), each relative to its scale.  Measured on the CPU with

    python -m tests.tsdf_inputs

which printed ``TSDF_GAP 1.1e-14 (subset)  TSDF_DECISION_GAP 8.6e-15 (behind)``.  Both are some tens of units in the last place, not one: sdf
is the difference of two numbers of about 2 (d and Y_z) divided by a truncation of about 0.1, so one rounding of Y_z is 2e-15 of a term
of the sum.  tests/test_tsdf_reference.py recomputes both and holds the constants below to be no smaller."""
import functools

import numpy as np

from tests import fusion_inputs as fi
from tests import tsdf_reference as ref

TSDF_GAP = 1.1e-14
TSDF_DECISION_GAP = 8.6e-15
MARGIN = 8.0

SPHERE_GRID = dict(origin=(-0.5, -0.5, -0.6), voxel=0.04, dims=(26, 26, 26))


def _case(ring, origin, voxel, dims, trunc, views=None, depth_dtype=np.float64, sum_dtype=np.float32, min_weights=(2,)):
    D, K, E = ring
    return dict(depth=np.array(D).astype(depth_dtype), K=K, ext=E, origin=tuple(origin), voxel=voxel, dims=tuple(dims), trunc=trunc, views=views, sum_dtype=sum_dtype,
                min_weights=tuple(min_weights))


def _noisy(**kw):
    """The noisy ring of ten views with patches and every kind of invalid depth, on a grid that holds the sphere and a part of the plane."""
    a = dict(origin=(-0.47, -0.52, -0.61), voxel=0.06, dims=(19, 18, 23), trunc=0.15, min_weights=(1, 2, 10))
    a.update(kw)
    return _case(fi.ring(10, 64, 48, 8.0, 101, True, 202), **a)


# name -> () -> the inputs: every input set of tests/test_gpu_tsdf.py
CASES = {
    "sphere_008": lambda: _case(fi.sphere_ring(), trunc=0.08, min_weights=(1, 2, 6), **SPHERE_GRID),                     # dims (26, 26, 26); min_weight 1, 2 and V
    "sphere_012": lambda: _case(fi.sphere_ring(), trunc=0.12, min_weights=(1, 2, 6), **SPHERE_GRID),
    "plane": lambda: _case(fi.plane_ring(), (-0.41, -0.33, 0.33), 0.05, (17, 13, 11), 0.12, min_weights=(1, 6)),
    "noisy": _noisy,
    "noisy_depth_f32": lambda: _noisy(depth_dtype=np.float32),
    "noisy_sum_f64": lambda: _noisy(sum_dtype=np.float64),
    "noisy_both_f64_f32": lambda: _noisy(depth_dtype=np.float32, sum_dtype=np.float64),
    "subset": lambda: _noisy(views=(7, 2, 5, 0, 3), min_weights=(1, 3)),                                                # a permuted subset
    "empty_list": lambda: _noisy(views=(), min_weights=(1,)),                                                           # the volume stays 0: an empty mesh
    "behind": lambda: _case(fi.sphere_ring(), (-1.63, -0.42, -2.61), 0.1, (33, 9, 30), 0.2, min_weights=(1, 2)),       # partly behind the cameras, partly outside every image
    "dims_33x17x5": lambda: _case(fi.sphere_ring(), (-0.37, -0.21, -0.553), 0.03, (33, 17, 5), 0.09, min_weights=(1, 2, 6)),   # the near cap of the sphere
    "dims_2x2x2": lambda: _case(fi.sphere_ring(), (0.093, 0.017, -0.523), 0.04, (2, 2, 2), 0.08, min_weights=(1, 6)),   # one cell across the sphere's nearest point
    "dims_1x9x9": lambda: _case(fi.sphere_ring(), (0.1, -0.13, -0.61), 0.04, (1, 9, 9), 0.08, min_weights=(1,)),        # no cells: an empty mesh
}


@functools.lru_cache(maxsize=None)
def translated_plane(c=0.613, W=64, H=48):
    """Four purely translated cameras (R = I, centres in the plane z = 0) whose depth maps are constant at c: the plane z = c.
    -> the inputs of a case."""
    K = np.array([[60.0, 31.3, 60.5, 23.6]] * 4)
    E = np.zeros((4, 3, 4))
    for v, (x, y) in enumerate(((0.1, 0.08), (-0.09, 0.1), (-0.1, -0.07), (0.08, -0.1))):
        E[v, :, :3] = np.eye(3)
        E[v, :, 3] = (-x, -y, 0.0)
    D = np.full((4, H, W), c)
    return _case((D, K, E), (-0.1013, -0.0807, 0.5009), 0.02, (11, 9, 11), 0.06, sum_dtype=np.float64, min_weights=(1, 4)), c


def free_space_node():
    """The grid of the free-space test: 5^3 nodes whose centre node sits half a truncation behind the SPURIOUS surface of view 2's patch
    (tests/fusion_inputs.py PATCHES: its depths are 0.75 of the true ones), on the ray of the patch's centre pixel.  Views 1 and 3 see
    through that point to the true surface.  -> (the inputs of a case, the centre node (i, j, k), the patch's view)."""
    D, K, E = fi.ring(10, 64, 48, 8.0, None, True, None)
    v, y0, y1, x0, x1, _ = fi.PATCHES[1]
    x, y = (x0 + x1) // 2, (y0 + y1) // 2
    trunc, voxel = 0.09, 0.03
    z = D[v, y, x] + 0.5 * trunc
    R, t = E[v][:, :3], E[v][:, 3]
    X = R.T @ (z * np.array([(x - K[v, 1]) / K[v, 0], (y - K[v, 3]) / K[v, 2], 1.0]) - t)
    return _case((D, K, E), np.round(X - 2 * voxel, 4) + 0.00013, voxel, (5, 5, 5), trunc), (2, 2, 2), v


def run_reference(case, dtype=np.float64, sum_dtype=None, loop=False):
    """Integrate a case into a fresh volume.  -> (volume, the dict of ``integrate``)."""
    vol = ref.Volume(case["origin"], case["voxel"], case["dims"], case["sum_dtype"] if sum_dtype is None else sum_dtype)
    if loop:
        return vol, ref.integrate_loop(vol, case["depth"], case["K"], case["ext"], case["trunc"], case["views"])
    return vol, ref.integrate(vol, case["depth"], case["K"], case["ext"], case["trunc"], case["views"], dtype=dtype)


def _rel(a, b):
    both = np.isfinite(a.astype(np.float64)) & np.isfinite(b.astype(np.float64))
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def measure_gaps(cases=None):
    """-> (TSDF_GAP, its case, TSDF_DECISION_GAP, its case) over ``cases`` (default: every case), float64 against longdouble."""
    L = np.longdouble
    gap, dgap = (0.0, None), (0.0, None)
    for name, make in (CASES.items() if cases is None else cases):
        c = make()
        v64, r64 = run_reference(c, np.float64, np.float64)
        vL, rL = run_reference(c, L, L)
        assert np.array_equal(v64.weight, vL.weight), name
        big = float(np.max(np.abs(vL.sum))) or 1.0
        g, d = _rel(v64.sum.astype(L), vL.sum) / big, _rel(r64["decisions"].astype(L), rL["decisions"])
        for mw in c["min_weights"]:
            x64, xL = ref.extract(v64, mw, np.float64), ref.extract(vL, mw, L)
            assert np.array_equal(x64["quads"], xL["quads"]) and x64["vertices"].shape == xL["vertices"].shape, (name, mw)
            if len(xL["vertices"]):
                g = max(g, _rel(x64["vertices"].astype(L), xL["vertices"]) / float(np.max(np.abs(xL["vertices"]))))
            d = max(d, _rel(x64["decision"].astype(L), xL["decision"]))
        gap, dgap = max(gap, (g, name)), max(dgap, (d, name))
    return gap[0], gap[1], dgap[0], dgap[1]


if __name__ == "__main__":
    g, gn, d, dn = measure_gaps()
    print(f"TSDF_GAP {g:.1e} ({gn})  TSDF_DECISION_GAP {d:.1e} ({dn})")
