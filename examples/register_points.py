#!/usr/bin/env python3
"""Registering 3-D point sets on the device: ``compiled_helpers.align_points`` and the front ends built on it.

1. One rigid fit, the reference's ``n_estimate_rigid_transform``: a planar board measured in another frame.
2. A batch with wrong matches: per-image registration of a target with the consensus stage switched on.
3. A seeded scene brought into the frame and scale of a few surveyed control points (``pose_seeding.align_scene``).

    python examples/register_points.py          (needs the built library and a HIP device)
"""
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import pose_seeding, synthetic  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    # 1. a planar board in another frame: the polar-factor route divides by the smallest singular value (0 for a plane); Horn's does not
    board = synthetic.charuco_points(10, 8.0)
    R, t = Rotation.from_rotvec([0.4, -0.3, 0.9]).as_matrix(), np.array([0.05, -0.02, 0.6])
    seen = board @ R.T + t + rng.normal(0.0, 2e-5, board.shape)
    fit = ch.align_points(board, seen)
    print(f"1. board of {board.shape[0]} corners: status {fit.status[0]}, RMS {fit.rms[0] * 1e6:.1f} um, conditioning {fit.conditioning[0]:.3f}, "
          f"|R - R_true| {np.max(np.abs(fit.R[0] - R)):.1e}, det R {np.linalg.det(fit.R[0]):+.12f}")

    # 2. 200 images of a cube target, 20 % of the features of every image matched to the wrong point
    cube = synthetic.ccube_points(6, 40.0)
    poses = np.concatenate([rng.normal(0.0, 0.5, (200, 3)), rng.normal(0.0, 0.05, (200, 3))], axis=1)
    pts = np.einsum("iab,kb->ika", Rotation.from_rotvec(poses[:, :3]).as_matrix(), cube) + poses[:, None, 3:] + rng.normal(0.0, 2e-5, (200, cube.shape[0], 3))
    wrong = rng.random(pts.shape[:2]) < 0.2
    pts[wrong] = rng.uniform(-0.1, 0.1, (int(wrong.sum()), 3))
    plain = ch.register_target(pts, cube)
    robust = ch.register_target(pts, cube, consensus=64, inlier_dist=2e-4)
    res = ch.register_target.last
    print(f"2. 200 images x {cube.shape[0]} features, 20 % wrong: largest pose error {np.max(np.abs(plain - poses)):.2e} plain, "
          f"{np.max(np.abs(robust - poses)):.2e} with consensus; flags are the right rows: {np.array_equal(res.inliers, ~wrong.ravel())}; "
          f"stage times {ch.last_align_kernel_ms}")

    # 3. a scene seeded from detections alone has a camera's frame and a free scale; twelve surveyed points give it the surveyor's
    from tests import twoview_inputs as ti

    rig = ti.chain_rig(0.0)
    seed = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, consensus=16)
    control = np.full_like(rig["points"], np.nan)
    control[:12] = rig["points"][:12]
    world = pose_seeding.align_scene(seed, control)
    print(f"3. seeded scene: frame camera {seed.frame_cam} -> {world.frame_cam}, scale {world.alignment.scale[0]:.4f}, "
          f"largest point error after alignment {np.max(np.abs(world.points - rig['points'])):.2e} (scene size {np.ptp(rig['points'], axis=0).max():.1f})")


if __name__ == "__main__":
    main()
