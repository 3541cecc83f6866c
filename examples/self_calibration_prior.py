#!/usr/bin/env python3
"""Gauge-free self-calibration with a prior on the target's points: ring-4 (4 cameras, 6 images, a 36-corner board), the self chain,
camera 0's extrinsics fixed and EVERY point coordinate free.

The reference pins 3 + 3 + 1 point coordinates to fix the 7-DoF gauge (frame and scale of the target) and afterwards rescales and
aligns the result to the nominal target.  Here the board's manufacturing tolerance does that job: a Gaussian prior on the points at
their nominal positions (``handlers.slab_prior(h, {"bdpt": tolerance})``).

  1. ``options={"gauge": "free", "fixed_pose": []}``: nothing of the target or its poses is pinned;
  2. without a prior ``parameter_covariance`` can only raise: H has a seven-dimensional null space;
  3. ``lm_solve(prior_mean=, prior_sigma=)`` solves in the nominal frame and scale;
  4. ``parameter_covariance(prior_mean=, prior_sigma=)``: standard errors of everything, the points included.

    python examples/self_calibration_prior.py

Needs an MI355X.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from pycamset_amd.device_solver import lm_solve, parameter_covariance


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
    h = handlers.SelfBundleHandler(cs, Target(rig.points), TargetDetection(cs.get_names(), rig.detections),
                                   fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}},
                                   options={"verbosity": 0, "gauge": "free", "fixed_pose": []})
    bp = h.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel(),
                         rig.points.ravel()[bp.bdpt_unfixed]])
    K = rig.n_keys
    print(f"{rig.detections.shape[0]} detections, {x0.shape[0]} free parameters, {int(bp.bdpt_unfixed.sum())} of {3 * K} point coordinates free")
    try:
        parameter_covariance(h, x0)
    except np.linalg.LinAlgError as e:
        print("without a prior:", e)

    tolerance = 0.05                                             # of the board, in its own units, per coordinate
    mean, sigma = handlers.slab_prior(h, {"bdpt": tolerance})    # the mean defaults to the nominal target
    res = lm_solve(h, x0.copy(), max_iter=100, prior_mean=mean, prior_sigma=sigma)
    print(f"with the point prior: {res.message} after {res.nfev} evaluations, cost {res.cost:.3f} of which the prior {res.prior_cost:.3e}")
    pts = res.x[-int(bp.bdpt_unfixed.sum()):].reshape(-1, 3)
    print("centroid of the solved points - nominal centroid:", np.round(pts.mean(0) - rig.points.mean(0), 6))
    cov = parameter_covariance(h, res.x, prior_mean=mean, prior_sigma=sigma)
    print(f"variance of unit weight {cov.sigma2:.3f} over {cov.dof} degrees of freedom, min L_ii^2 / H_ii = {cov.min_pivot:.2e}")
    print("standard errors of camera 1's [fx, cx, fy, cy]:", np.round(np.sqrt(np.diagonal(cov.blocks[0][1]))[:4], 3))
    print("standard errors of point 0 (prior: %.3f):" % tolerance, np.round(np.sqrt(np.diagonal(cov.blocks[3][0])), 5))


if __name__ == "__main__":
    main()
