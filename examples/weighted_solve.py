#!/usr/bin/env python3
"""Weight detections by their pixel noise: a ring of eight cameras in which every second one is four times as noisy as the others
(a soft lens, a low resolution, a far camera).

  1. solve with every detection counting the same, in pixels;
  2. measure the noise the solve left per camera: ``diagnostics.reprojection_report`` gives the RMS of the error e = |(ru, rv)| per
     camera, and for isotropic noise sigma per axis is RMS / sqrt(2);
  3. solve again with ``lm_solve(sigma=per_camera_sigma)``: each detection's residual and Jacobian rows are whitened by 1 / sigma on
     the device, which is the maximum-likelihood estimate for that noise;
  4. ``parameter_covariance(sigma=..., absolute_sigma=True)``: standard errors for noise of exactly that size.

    python examples/weighted_solve.py

Needs an MI355X.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from pycamset_amd.device_solver import lm_solve, parameter_covariance
from pycamset_amd.diagnostics import reprojection_report


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
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)   # 0.3 px noise
    det = rig.detections.copy()
    noisy = det[:, 0].astype(int) % 2 == 1
    det[noisy, 3:] += np.random.default_rng(1).normal(0.0, np.sqrt(1.2 ** 2 - 0.3 ** 2), (int(noisy.sum()), 2))     # 1.2 px in all
    cs = Camset(rig.n_cams)
    h = handlers.TemplateBundleHandler(cs, Target(rig.points), TargetDetection(cs.get_names(), det),
                                       fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()])

    def focal_error(x):
        intr = np.asarray(h.get_bundle_adjustment_inputs(x)[0])
        return float(np.max(np.abs(intr[:, [0, 2]] - rig.intr_true[:, [0, 2]])))

    plain = lm_solve(h, x0.copy(), max_iter=60)
    sigma = reprojection_report(h, plain.x).per_camera.rms / np.sqrt(2.0)
    print("sigma per camera from the unweighted solve [px]:", np.round(sigma, 2))
    weighted = lm_solve(h, plain.x.copy(), max_iter=60, sigma=sigma)          # (C,) = one sigma per camera
    cov = parameter_covariance(h, weighted.x, sigma=sigma, absolute_sigma=True)
    check = parameter_covariance(h, weighted.x, sigma=sigma)
    print(f"unweighted: worst focal length error {focal_error(plain.x):.3f} px")
    print(f"weighted  : worst focal length error {focal_error(weighted.x):.3f} px, whitened cost {weighted.cost:.1f}, "
          f"variance of unit weight {check.sigma2:.3f} (1 = the sigmas are right)")
    print("standard errors of camera 1's intrinsics [fx, cx, fy, cy]:", np.round(np.sqrt(np.diagonal(cov.blocks[0][1]))[:4], 3))


if __name__ == "__main__":
    main()
