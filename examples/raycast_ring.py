#!/usr/bin/env python3
"""Look at a reconstruction through its own cameras and through one no camera had: the ring of examples/mesh_ring.py is carried from its
images to per-view depth maps and integrated into a truncated signed distance volume; the volume is then RAY-CAST
(``volume.raycast_views``) from a pose half-way between two cameras, and ``volume.depth_residuals`` holds the model's depth in each of
the six input views against that view's measured depth map: the dense counterpart of the reprojection statistics.

The scene is an analytically textured plane one metre in front of six distorted cameras on an arc, so the cast depth of the new pose
has to be that of the plane Z = 1 and its normals (0, 0, -1).

    python examples/raycast_ring.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from fuse_ring_stereo import C, H, W, Z0, cameras, render  # noqa: E402

from pycamset_amd import sweep, volume  # noqa: E402

DEPTH_RANGE, STEPS, VOXEL = (0.8, 1.2), 64, 0.01


def between(ext, a, b):
    """A pose half-way between views a and b: the mean centre, the rotation of the mean rotation vector."""
    from scipy.spatial.transform import Rotation

    Ra, Rb = ext[a][:, :3], ext[b][:, :3]
    centre = 0.5 * (-Ra.T @ ext[a][:, 3] - Rb.T @ ext[b][:, 3])
    R = (Rotation.from_rotvec(0.5 * Rotation.from_matrix(Rb @ Ra.T).as_rotvec()) * Rotation.from_matrix(Ra)).as_matrix()
    return np.concatenate([R, (-R @ centre)[:, None]], axis=1)


def main():
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    points, _ = sweep.reconstruct_views(images, intr, ext, DEPTH_RANGE, STEPS)
    K, _, _, depth, _ = sweep.reconstruct_views.last
    origin, dims = volume.grid_from_bounds(volume.volume_from_points(points, VOXEL), VOXEL)
    vol = volume.integrate_depth_maps(depth, K, ext, origin, VOXEL, dims)
    Kn = 0.5 * (np.asarray(K)[2:3] + np.asarray(K)[3:4])
    En = between(np.asarray(ext, dtype=np.float64).reshape(C, 3, 4), 2, 3)[None]
    z, normal, status = volume.raycast_views(vol, Kn, En, W, H, dtype=np.float64, status=True)
    hit = status[0] == 0
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(xs - Kn[0, 1]) / Kn[0, 0], (ys - Kn[0, 3]) / Kn[0, 2], np.ones((H, W))], axis=-1) @ En[0][:, :3]
    world_z = (-En[0][:, :3].T @ En[0][:, 3])[2] + z[0] * ray[..., 2]
    err = np.abs(world_z[hit] - Z0)
    tilt = np.degrees(np.arccos(np.clip(-normal[0][hit][:, 2], -1.0, 1.0)))
    print(f"volume of {dims[0]} x {dims[1]} x {dims[2]} nodes of {VOXEL}; a pose between cameras 2 and 3 at {W} x {H}: {int(hit.sum())} of {W * H} pixels hit the surface "
          f"(status counts {np.bincount(status.reshape(-1), minlength=4).tolist()})")
    print(f"distance of the hit points from the plane Z = {Z0}: median {np.median(err):.5f}, 95 % {np.quantile(err, 0.95):.5f}; angle of the normals to (0, 0, -1): "
          f"median {np.median(tilt):.2f} deg, 95 % {np.quantile(tilt, 0.95):.2f} deg")
    residual, stats = volume.depth_residuals(vol, depth, K, ext)
    print("model depth minus measured depth per input view (count, median, MAD):")
    for c in range(C):
        print(f"  view {c}: {int(stats[c, 0]):6d} pixels, median {stats[c, 1]:+.5f}, MAD {stats[c, 2]:.5f}")
    vol.close()
    if not (hit.sum() > 0.2 * W * H and np.median(err) <= VOXEL and np.all(np.abs(stats[:, 1]) <= VOXEL)):
        raise SystemExit("the cast does not lie on the plane")


if __name__ == "__main__":
    main()
