#!/usr/bin/env python3
"""A ring of calibrated cameras to ONE point cloud on the device: every adjacent pair is rectified, matched and reprojected
(``stereo.py``), and the per-pair depth maps are fused (``fusion.fuse_stereo_pairs``): a depth stays only where at least two other
pairs agree with it, the agreeing observations are merged into one point, and of the pixels that describe one surface element only the
lowest view's stays.  This is the step the reference leaves to an external multi-view program (``CameraSet.write_to_txt``,
``calc_pairs`` / ``write_pair_file``).

The scene is synthetic so that the example needs no files: an analytically textured plane one metre in front of six distorted cameras
on an arc, 7 degrees apart.  Every pixel's ray (``imaging.pixel_rays``) is intersected with the plane and the texture is evaluated there.

    python examples/fuse_ring_stereo.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pycamset_amd import fusion, imaging  # noqa: E402

W, H, Z0, C, STEP = 320, 240, 1.0, 6, 7.0


def cameras():
    intr, ext = np.zeros((C, 9)), np.zeros((C, 3, 4))
    for c in range(C):
        a = np.radians(STEP) * (c - 0.5 * (C - 1))
        centre = np.array([np.sin(a), 0.004 * np.sin(2.0 * c), Z0 - np.cos(a)])
        fwd = (np.array([0.0, 0.0, Z0]) - centre) / np.linalg.norm(np.array([0.0, 0.0, Z0]) - centre)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        ext[c] = np.concatenate([R, (-R @ centre)[:, None]], axis=1)
        intr[c] = [395.0 + 2.0 * c, 158.3 + 0.4 * c, 396.0 + 1.5 * c, 121.2 - 0.3 * c, -0.06 + 0.004 * c, 0.015, 0.0008, -0.0006, 0.0]
    return intr, ext


def texture(X, Y):
    return 127.5 + 45.0 * np.sin(61.0 * X + 2.0 * np.sin(23.0 * Y)) + 40.0 * np.sin(47.0 * Y + 13.0 * X * X) + 35.0 * np.sin(29.0 * (X + Y) + 5.0 * np.cos(37.0 * X))


def render(K, E):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = imaging.pixel_rays(np.stack([xs, ys], axis=-1).reshape(-1, 2), K, ext=E[None], world=True)
    c = -E[:, :3].T @ E[:, 3]
    P = c[None, :] + ((Z0 - c[2]) / rays[:, 2])[:, None] * rays
    return np.clip(np.rint(texture(P[:, 0], P[:, 1])), 0, 255).astype(np.uint8).reshape(H, W)


def main():
    intr, ext = cameras()
    images = np.stack([render(intr[c], ext[c]) for c in range(C)])
    pairs = [(c, c + 1) for c in range(C - 1)]
    points, grey = fusion.fuse_stereo_pairs(images, intr, ext, pairs, 64, match_options=dict(block=15, lr_max_diff=1), depth_range=(0.2, 3.0), rel_tol=0.02)
    K, P, neighbours, depth, counts, per_pair = fusion.fuse_stereo_pairs.last
    print(f"{C} cameras, {len(pairs)} pairs of {W} x {H}: per-pair clouds {per_pair} ({sum(per_pair)} points), neighbours {[[int(j) for j in l] for l in neighbours]}")
    err = np.abs(points[:, 2] - Z0)
    print(f"fused cloud: {len(points)} points (per view {counts}); distance from the plane Z = {Z0}: median {np.median(err):.5f}, 95 % {np.quantile(err, 0.95):.5f}; "
          f"grey values {grey.min()} .. {grey.max()}")
    step = Z0 * Z0 / (K[0, 0] * 2.0 * np.sin(np.radians(STEP) / 2.0))
    if not (len(points) < sum(per_pair) and np.median(err) <= 0.5 * step):
        raise SystemExit("the fused cloud does not lie on the plane")


if __name__ == "__main__":
    main()
