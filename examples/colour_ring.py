#!/usr/bin/env python3
"""Bring the images back onto the reconstruction: the ring of examples/mesh_ring.py is carried from its images to per-view depth maps and
integrated into a truncated signed distance volume; the mesh of its surface is COLOURED from the undistorted images
(``volume.colour_surface``: vertex normals for the weights, the model's own depth in every source view for the occlusion) and written as
a PLY with colours and normals, and the volume is rendered in colour from a pose half-way between two cameras
(``volume.colour_views``), written as a PGM.

The scene is the analytically textured plane of the ring, one metre in front of six distorted cameras on an arc, so a vertex at (X, Y)
has to take the grey level ``texture(X, Y)``.

    python examples/colour_ring.py [out.ply [out.pgm]]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from fuse_ring_stereo import C, H, W, cameras, render, texture  # noqa: E402
from raycast_ring import between  # noqa: E402

from pycamset_amd import imaging, sweep, volume  # noqa: E402

DEPTH_RANGE, STEPS, VOXEL = (0.8, 1.2), 64, 0.01


def main():
    ply = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("colour_ring.ply")
    pgm = Path(sys.argv[2]) if len(sys.argv) > 2 else Path("colour_ring.pgm")
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    points, _ = sweep.reconstruct_views(images, intr, ext, DEPTH_RANGE, STEPS)
    K, _, _, depth, _ = sweep.reconstruct_views.last
    undistorted = imaging.undistort_images(images, np.arange(C), intr).reshape(images.shape)   # the pinhole images K belongs to
    origin, dims = volume.grid_from_bounds(volume.volume_from_points(points, VOXEL), VOXEL)
    vol = volume.integrate_depth_maps(depth, K, ext, origin, VOXEL, dims)
    vertices, quads = volume.extract_surface(vol)
    normals = volume.vertex_normals(vol, vertices)
    colours, weight, count, best = volume.colour_surface(vol, vertices, undistorted, K, ext, cos_min=0.2, info=True)
    volume.write_ply(ply, vertices, quads, colours=colours, normals=np.nan_to_num(normals))
    some = count > 0
    err = np.abs(colours[some, 0].astype(np.float64) - texture(vertices[some, 0].astype(np.float64), vertices[some, 1].astype(np.float64)))
    print(f"{C} cameras of {W} x {H}; volume of {dims[0]} x {dims[1]} x {dims[2]} nodes of {VOXEL}; mesh: {len(vertices)} vertices, {len(quads)} quads -> {ply}")
    print(f"{int(some.sum())} vertices coloured (views per vertex: {np.bincount(count, minlength=C + 1).tolist()}), {int((~some).sum())} without a normal or a view; "
          f"|colour - texture| in grey levels: median {np.median(err):.2f}, 95 % {np.quantile(err, 0.95):.2f}")
    Kn = 0.5 * (np.asarray(K)[2:3] + np.asarray(K)[3:4])
    En = between(np.asarray(ext, dtype=np.float64).reshape(C, 3, 4), 2, 3)[None]
    image, z, _, vcount, _ = volume.colour_views(vol, Kn, En, W, H, undistorted, K, ext, cos_min=0.2, info=True)
    pgm.write_bytes(f"P5\n{W} {H}\n255\n".encode() + image[0, :, :, 0].tobytes())
    seen = vcount[0] > 0
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(xs - Kn[0, 1]) / Kn[0, 0], (ys - Kn[0, 3]) / Kn[0, 2], np.ones((H, W))], axis=-1) @ En[0][:, :3]
    X = (-En[0][:, :3].T @ En[0][:, 3]) + z[0][..., None].astype(np.float64) * ray
    rerr = np.abs(image[0, :, :, 0][seen].astype(np.float64) - texture(X[..., 0][seen], X[..., 1][seen]))
    print(f"a pose between cameras 2 and 3 at {W} x {H}: {int(np.isfinite(z).sum())} pixels hit the surface, {int(seen.sum())} coloured -> {pgm}; "
          f"|colour - texture|: median {np.median(rerr):.2f}, 95 % {np.quantile(rerr, 0.95):.2f}")
    kernel_ms = vol.colour_last_kernel_ms()
    print(f"device time of the last point-normals kernel {kernel_ms[0]:.3f} ms, of the last colour kernel {kernel_ms[1]:.3f} ms")
    vol.close()
    if not (some.sum() > 0.5 * len(vertices) and np.median(err) <= 10.0 and seen.sum() > 0.2 * W * H and np.median(rerr) <= 10.0):
        raise SystemExit("the colours are not the texture's")


if __name__ == "__main__":
    main()
