"""Fixed inputs of the ray-cast tests: the volumes of tests/tsdf_inputs.py (imported, not copied) and, per volume, the render views they
are cast into.  Nothing is committed but this code.  ``CASES`` names every input set the device tests use (tests/test_gpu_raycast.py);
tests/test_raycast_reference.py asserts for each of them that no decision of the rule sits near its threshold.

Render views per volume: a generic pose between the ring's cameras at 40 x 30, a camera INSIDE the box at 13 x 7 and one view of 1 x 1
(widths that are no multiple of the 8 x 8 tile; rays that start inside; rays that miss the box).  ``translated_plane`` adds a view with
R = I and an integer cx: the pixel column x = cx has gw_x == 0 exactly.

RAY_GAP, RAY_NORMAL_GAP and RAY_DECISION_GAP are the float64-versus-longdouble gaps of the restatement (tests/raycast_reference.py) over
``CASES`` and the translated plane.  RAY_GAP: the largest |float64 - longdouble| hit depth of a view, relative to the view's largest
depth.  RAY_NORMAL_GAP: the same for the normals' components (unit vectors: absolute).  RAY_DECISION_GAP: the same for the decision
quantities, each relative to its scale.  Measured on the CPU with

    python -m tests.raycast_inputs

which printed ``RAY_GAP 1.9e-15 (noisy)  RAY_NORMAL_GAP 3.7e-14 (subset)  RAY_DECISION_GAP 2.7e-14 (sphere_012)``; the constants below are
those figures rounded up in the second digit.  The normals' gap is the largest: G is a difference of blends of about 1 that can be as small
as a few hundredths, so one rounding of a blend is some 1e-14 of a component.  The decisions' gap is a few tens of units in the last place
because g_a = gc_a + z gw_a is a sum of terms of up to about 50 cells that is held against an integer.  tests/test_raycast_reference.py
recomputes all three and holds the constants below to be no smaller."""
import functools

import numpy as np

from tests import fusion_inputs as fi
from tests import raycast_reference as ray
from tests import tsdf_inputs as ti

RAY_GAP = 2.0e-15
RAY_NORMAL_GAP = 3.8e-14
RAY_DECISION_GAP = 2.8e-14
MARGIN = ti.MARGIN

VOLUMES = ("sphere_008", "sphere_012", "plane", "noisy", "noisy_sum_f64", "subset", "empty_list", "behind", "dims_33x17x5", "dims_2x2x2", "dims_1x9x9")
# what differs from the defaults (step = voxel, z_near = 0, z_far = inf) per volume
OPTIONS = {"sphere_012": dict(step_voxels=0.6), "plane": dict(z_near=0.3, z_far=2.4), "noisy_sum_f64": dict(step_voxels=1.7), "dims_33x17x5": dict(step_voxels=1.0 / 64.0)}


def _view(width, height, f, cx, cy, ext):
    return dict(width=width, height=height, K=np.array([[f, cx, f * 1.004, cy]]), ext=np.asarray(ext, dtype=np.float64)[None])


def render_views(case):
    """The three render views of a volume: generic (40 x 30), inside (13 x 7), one pixel (1 x 1)."""
    o, s, d = np.array(case["origin"]), case["voxel"], np.array(case["dims"])
    span = s * (d - 1)
    centre = o + 0.5 * span
    a = np.radians(2.7)
    generic = fi.look_at(centre + 1.9 * np.array([np.sin(a), 0.067, -np.cos(a)]) + (0.0213, 0.0117, 0.0), target=centre + (0.011, -0.006, 0.004), roll=0.031)
    eye = o + span * (0.313, 0.471, 0.127)
    inside = fi.look_at(eye, target=eye + (0.083, -0.041, 1.0), roll=-0.052)
    pixel = fi.look_at(centre + (0.217, -0.113, -1.7), target=centre + (0.0031, 0.0017, 0.0), roll=0.011)
    return [_view(40, 30, 37.3, 19.3, 14.6, generic), _view(13, 7, 9.1, 6.2, 3.3, inside), _view(1, 1, 50.0, 0.2, -0.1, pixel)]


def _settings(case, name):
    opt = OPTIONS.get(name, {})
    mw = 2 if 2 in case["min_weights"] else min(case["min_weights"])
    step = None if "step_voxels" not in opt else opt["step_voxels"] * case["voxel"]
    return dict(min_weight=mw, step=step, z_near=opt.get("z_near", 0.0), z_far=opt.get("z_far", np.inf))


def _make(name):
    case = ti.CASES[name]()
    return dict(volume=case, views=render_views(case), **_settings(case, name))


# name -> () -> dict(volume: the inputs of a tsdf case, views: the render views, min_weight, step, z_near, z_far)
CASES = {name: functools.partial(_make, name) for name in VOLUMES}


@functools.lru_cache(maxsize=None)
def translated_plane():
    """The plane z = c of tests/tsdf_inputs.py at min_weight 4, its three views and a fourth with R = I and cx = 20: the rays of the
    pixel column x = 20 run in a plane x = const, gw_x == 0 exactly.  -> (the inputs of a case, c)."""
    case, c = ti.translated_plane()
    E = np.concatenate([np.eye(3), -np.array([[0.0131], [-0.0113], [0.0]])], axis=1)
    axis = dict(width=40, height=30, K=np.array([[60.0, 20.0, 60.5, 14.6]]), ext=E[None])
    return dict(volume=case, views=render_views(case) + [axis], min_weight=4, step=None, z_near=0.0, z_far=np.inf), c


def all_cases():
    return [(n, make()) for n, make in CASES.items()] + [("translated_plane", translated_plane()[0])]


@functools.lru_cache(maxsize=None)
def integrated(name):
    """The volume of a case from the restatement of the integration (tests/tsdf_reference.py), read-only."""
    case = translated_plane()[0] if name == "translated_plane" else CASES[name]()
    vol, _ = ti.run_reference(case["volume"])
    for a in (vol.sum, vol.weight):
        a.setflags(write=False)
    return vol


def cast_reference(case, vol, view, dtype=np.float64, normals=True):
    return ray.raycast(vol, view["K"], view["ext"], view["width"], view["height"], case["min_weight"], case["step"], case["z_near"], case["z_far"], dtype=dtype, normals=normals)


def _gap(a, b):
    both = np.isfinite(a.astype(np.float64)) & np.isfinite(b.astype(np.float64))
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def measure_gaps():
    """-> ((RAY_GAP, case), (RAY_NORMAL_GAP, case), (RAY_DECISION_GAP, case)), float64 against longdouble."""
    L = np.longdouble
    g, ng, dg = (0.0, None), (0.0, None), (0.0, None)
    for name, case in all_cases():
        vol = integrated(name)
        for k, view in enumerate(case["views"]):
            r64, rL = cast_reference(case, vol, view), cast_reference(case, vol, view, L)
            assert np.array_equal(r64["status"], rL["status"]), (name, k)
            if np.isfinite(rL["depth"]).any():
                g = max(g, (_gap(r64["depth"].astype(L), rL["depth"]) / float(np.nanmax(rL["depth"])), name))
            ng = max(ng, (_gap(r64["normal"].astype(L), rL["normal"]), name))
            for key, q in rL["decisions"].items():
                assert q.shape == r64["decisions"][key].shape and np.array_equal(np.isnan(q), np.isnan(r64["decisions"][key])), (name, k, key)
                dg = max(dg, (_gap(r64["decisions"][key].astype(L), q), name))
    return g, ng, dg


if __name__ == "__main__":
    g, ng, dg = measure_gaps()
    print(f"RAY_GAP {g[0]:.1e} ({g[1]})  RAY_NORMAL_GAP {ng[0]:.1e} ({ng[1]})  RAY_DECISION_GAP {dg[0]:.1e} ({dg[1]})")
    for name, case in all_cases():
        vol = integrated(name)
        for k, view in enumerate(case["views"]):
            r = cast_reference(case, vol, view)
            st = np.bincount(r["status"].reshape(-1), minlength=4)
            print(f"{name} view {k}: status counts {st.tolist()}, closest call {r['closest'].min():.2e}, {r['samples']} samples")
