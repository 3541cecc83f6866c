#!/usr/bin/env python3
"""A ring of calibrated cameras to a surface MESH on the device: the ring of examples/sweep_ring.py is carried from its images to per-view
depth maps (``sweep.reconstruct_views``), the depth maps are integrated into a truncated signed distance volume around the fused cloud
(``volume.volume_from_points`` -> ``volume.mesh_views``) and the quad mesh of its surface is written as an ASCII PLY.

The scene is an analytically textured plane one metre in front of six distorted cameras on an arc, so the mesh has to lie on Z = 1.

    python examples/mesh_ring.py [out.ply]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from fuse_ring_stereo import C, H, W, Z0, cameras, render  # noqa: E402

from pycamset_amd import sweep, volume  # noqa: E402

DEPTH_RANGE, STEPS, VOXEL = (0.8, 1.2), 64, 0.01


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("mesh_ring.ply")
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    points, _ = sweep.reconstruct_views(images, intr, ext, DEPTH_RANGE, STEPS)
    K, _, _, depth, counts = sweep.reconstruct_views.last
    bounds = volume.volume_from_points(points, VOXEL)
    origin, dims = volume.grid_from_bounds(bounds, VOXEL)
    vertices, quads = volume.mesh_views(depth, K, ext, bounds, VOXEL, min_weight=2)
    volume.write_ply(out, vertices, quads)
    err = np.abs(vertices[:, 2] - Z0)
    print(f"{C} cameras of {W} x {H}: {len(points)} fused points (per view {counts}); volume of {dims[0]} x {dims[1]} x {dims[2]} nodes of {VOXEL} from {np.round(origin, 3).tolist()}")
    print(f"mesh: {len(vertices)} vertices, {len(quads)} quads -> {out}; distance of the vertices from the plane Z = {Z0}: median {np.median(err):.5f}, "
          f"95 % {np.quantile(err, 0.95):.5f}" if len(vertices) else f"mesh: 0 vertices, 0 quads -> {out}")
    if not (len(quads) > 0 and np.median(err) <= VOXEL):
        raise SystemExit("the mesh does not lie on the plane")


if __name__ == "__main__":
    main()
