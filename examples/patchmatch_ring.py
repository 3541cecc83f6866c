#!/usr/bin/env python3
"""A ring of calibrated cameras to depth maps WITH NORMALS and one point cloud on the device: the plane sweep localises the depth
(``sweep.sweep_depth_maps``), PatchMatch refines it with a slanted plane per pixel (``patchmatch.refine_depth_maps``), and the fusion
keeps what the views agree on — ``sweep.reconstruct_views(refine_iterations=)`` in one call.  This is the step the reference exports its
rig for (``ReconParams``, ``Camera.to_MVSnet_txt``: the inputs of ACMMP, a PatchMatch method).

Printed: per view the depth error of the sweep and of the refined maps against the plane and the angle of the refined normals to the
plane's normal; then the fused clouds with and without refinement.

The scene is that of examples/sweep_ring.py: an analytically textured plane one metre in front of six distorted cameras on an arc,
7 degrees apart.

    python examples/patchmatch_ring.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from fuse_ring_stereo import C, H, W, Z0, cameras, render  # noqa: E402

from pycamset_amd import imaging, patchmatch, sweep  # noqa: E402

DEPTH_RANGE, STEPS, ITERATIONS = (0.8, 1.2), 64, 3


def main():
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    step = (DEPTH_RANGE[1] - DEPTH_RANGE[0]) / STEPS
    clouds = {}
    for it in (0, ITERATIONS):
        points, _ = sweep.reconstruct_views(images, intr, ext, DEPTH_RANGE, STEPS, refine_iterations=it)
        clouds[it] = (points, sweep.reconstruct_views.last)
    K, neighbours, planes, depth0, _ = clouds[0][1]
    # the same refinement by hand, to look at the maps: undistorted images, the sweep's depth as the start, normals asked for
    und = imaging.undistort_images(images, np.arange(C), imaging.check_intr(intr)).reshape(images.shape)
    depth, normal, status = patchmatch.refine_depth_maps(und, K, ext, neighbours, DEPTH_RANGE, depth0, iterations=ITERATIONS, dtype=np.float64, return_normal=True,
                                                         return_status=True)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    print(f"{C} cameras of {W} x {H}, {STEPS} planes {step:.5f} apart, {ITERATIONS} iterations of PatchMatch behind the sweep")
    for c in range(C):
        R, t = ext[c][:, :3], ext[c][:, 3]
        ray = np.stack([(xs - K[c, 1]) / K[c, 0], (ys - K[c, 3]) / K[c, 2], np.ones_like(xs)], axis=-1)
        truth = (Z0 - (-R.T @ t)[2]) / (ray @ R)[..., 2]
        ok = (status[c] == 0) & np.isfinite(depth0[c])
        n_true = R @ np.array([0.0, 0.0, -1.0])
        angle = np.degrees(np.arccos(np.clip(normal[c][ok] @ n_true, -1.0, 1.0)))
        print(f"view {c}: {int(ok.sum())} pixels; median |z - z_true| sweep {np.median(np.abs(depth0[c] - truth)[ok]):.5f}, refined {np.median(np.abs(depth[c] - truth)[ok]):.5f}; "
              f"median angle of the normal to the plane's {np.median(angle):.1f} degrees (the view sees the plane at {np.degrees(np.arccos(-n_true[2])):.1f})")
    for it, (points, _) in clouds.items():
        err = np.abs(points[:, 2] - Z0)
        print(f"fused cloud with {it} iterations of refinement: {len(points)} points; distance from the plane Z = {Z0}: median {np.median(err):.5f}, "
              f"95 % {np.quantile(err, 0.95):.5f}, largest {err.max():.5f}")
    if not (len(clouds[ITERATIONS][0]) > 0 and np.median(np.abs(clouds[ITERATIONS][0][:, 2] - Z0)) <= 0.5 * step):
        raise SystemExit("the refined cloud does not lie on the plane")


if __name__ == "__main__":
    main()
