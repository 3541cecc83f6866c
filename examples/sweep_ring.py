#!/usr/bin/env python3
"""A ring of calibrated cameras to ONE point cloud on the device by a plane sweep (``sweep.reconstruct_views``): the images are
undistorted, every view gets its neighbours from the viewing directions, a depth map per view comes from sweeping ``steps`` planes
through the depth range and scoring every plane in all neighbours at once, and the depth maps are fused.  These are the inputs the
reference hands to an external multi-view program (``ReconParams``, ``Camera.to_MVSnet_txt``, ``calc_pairs``).

The same ring goes through ``fusion.fuse_stereo_pairs`` at its defaults for comparison: the time from the images to the cloud and the
points kept, both as host wall time around calls that end with the results on the host (the second call of each, so that neither pays
for loading its kernels).

The scene is that of examples/fuse_ring_stereo.py: an analytically textured plane one metre in front of six distorted cameras on an
arc, 7 degrees apart.

    python examples/sweep_ring.py
"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from fuse_ring_stereo import C, STEP, H, W, Z0, cameras, render  # noqa: E402

from pycamset_amd import fusion, sweep  # noqa: E402

DEPTH_RANGE, STEPS = (0.8, 1.2), 64


def timed(f):
    f()
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def main():
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    (points, grey), t_sweep = timed(lambda: sweep.reconstruct_views(images, intr, ext, DEPTH_RANGE, STEPS))
    K, neighbours, planes, depth, counts = sweep.reconstruct_views.last
    err = np.abs(points[:, 2] - Z0)
    step = (DEPTH_RANGE[1] - DEPTH_RANGE[0]) / STEPS
    print(f"{C} cameras of {W} x {H}, {STEPS} planes {step:.5f} apart, neighbours {[[int(j) for j in l] for l in neighbours]}")
    print(f"plane sweep: {len(points)} points (per view {counts}) in {1e3 * t_sweep:.1f} ms; distance from the plane Z = {Z0}: median {np.median(err):.5f}, "
          f"95 % {np.quantile(err, 0.95):.5f}; grey values {grey.min()} .. {grey.max()}")
    pairs = [(c, c + 1) for c in range(C - 1)]
    (p2, _), t_pairs = timed(lambda: fusion.fuse_stereo_pairs(images, intr, ext, pairs, 64))
    e2 = np.abs(p2[:, 2] - Z0)
    print(f"fuse_stereo_pairs at its defaults on the same ring: {len(p2)} points in {1e3 * t_pairs:.1f} ms; median {np.median(e2):.5f}, 95 % {np.quantile(e2, 0.95):.5f}"
          if len(p2) else f"fuse_stereo_pairs at its defaults on the same ring: 0 points in {1e3 * t_pairs:.1f} ms")
    if not (len(points) > 0 and np.median(err) <= 0.5 * step):
        raise SystemExit("the swept cloud does not lie on the plane")


if __name__ == "__main__":
    main()
