#!/usr/bin/env python3
"""Box bounds in the device solve: ring-4 (4 cameras, 6 images, a 36-corner board), the template chain, camera 0's extrinsics fixed.

The board covers only the centre of each image, so the data say little about the higher distortion terms: left free, k2 and k3 run off
to values no lens has while the reprojection error barely moves.  A box holds them — hard limits, not the pull of a prior: where the
data keep a parameter inside its box the estimate is not biased at all.

  1. ``lm_solve(h, x0)``: the free solve, and where k2, k3 end up;
  2. ``handlers.slab_bounds``: |k2| <= 0.5, |k3| <= 0.5 on every camera, focal lengths within 10 % of their start;
  3. ``lm_solve(h, x0, bounds=(lo, hi))``: the bounded solve, ``active_mask`` and ``n_truncated``.

    python examples/bounded_solve.py

Needs an MI355X.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from pycamset_amd.device_solver import lm_solve


class Camset:
    def __init__(self, n):
        self.names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self.names)

    def get_n_cams(self):
        return len(self.names)


class Target:
    def __init__(self, pts):
        self.point_data = np.asarray(pts)[None]


def main():
    rig = synthetic.make_rig("ring-4", 4, 6, synthetic.charuco_points(7, 8.0), seed=31, visibility=0.9)
    cs = Camset(rig.n_cams)
    h = handlers.TemplateBundleHandler(cs, Target(rig.points), TargetDetection(cs.get_names(), rig.detections),
                                       fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    bp.intr[:] = rig.intr                                        # slab_bounds measures ("rel", width) around the handler's slabs
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()])
    C = rig.n_cams
    k23 = np.r_[np.arange(5, 9 * C, 9), np.arange(8, 9 * C, 9)]   # k2 and k3 of every camera in the free vector

    free = lm_solve(h, x0.copy(), max_iter=100)
    print(f"free:    {free.message} after {free.nfev} evaluations, cost {free.cost:.4f}")
    print("         k2:", np.round(free.x[5:9 * C:9], 2), " k3:", np.round(free.x[8:9 * C:9], 1), " (true: |k2| ~ 0.01, |k3| ~ 0.001)")

    dist = np.r_[np.full(5, np.inf), 0.5, np.inf, np.inf, 0.5]   # [fx cx fy cy k1 k2 p1 p2 k3]
    focal = ("rel", np.r_[0.1, np.inf, 0.1, np.full(6, np.inf)])
    lo_d, hi_d = handlers.slab_bounds(h, {"intr": -dist}, {"intr": dist})
    lo_f, hi_f = handlers.slab_bounds(h, {"intr": focal}, {"intr": focal})
    lo, hi = np.maximum(lo_d, lo_f), np.minimum(hi_d, hi_f)
    res = lm_solve(h, x0.copy(), max_iter=100, bounds=(lo, hi))
    print(f"bounded: {res.message} after {res.nfev} evaluations, cost {res.cost:.4f}, {res.n_truncated} trials cut at a bound")
    print("         k2:", np.round(res.x[5:9 * C:9], 3), " k3:", np.round(res.x[8:9 * C:9], 3))
    print("         active_mask over k2, k3 (-1 lower, +1 upper):", res.active_mask[k23], "; elsewhere:", int(np.count_nonzero(np.delete(res.active_mask, k23))))
    print(f"         the box costs {100 * (res.cost / free.cost - 1):.2f} % of the free cost")


if __name__ == "__main__":
    main()
