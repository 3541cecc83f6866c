#!/usr/bin/env python3
"""Apply a calibration to images on the device: undistort a rig's frames in one launch, look at the ray of a pixel, rectify a pair.

Synthetic checkerboard images, no files read.  Needs the device (there is no CPU fallback).

    python examples/undistort_rig_images.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pycamset_amd import imaging  # noqa: E402


def checkerboard(n, H, W, square=32):
    yy, xx = np.mgrid[0:H, 0:W]
    board = (((xx // square) + (yy // square)) % 2).astype(np.uint8) * 200 + 30
    return np.stack([np.roll(board, 3 * i, axis=1) for i in range(n)])


def main():
    n_cams, W, H = 4, 640, 480
    rng = np.random.default_rng(0)
    intr = np.stack([[560.0 + 10 * c, W / 2 + 3 * c, 558.0 + 10 * c, H / 2 - 2 * c, -0.22, 0.06, 1e-3, -5e-4, -0.005] for c in range(n_cams)])
    ext = np.concatenate([np.broadcast_to(np.eye(3), (n_cams, 3, 3)), np.stack([[-0.12 * c, 0.0, 0.0] for c in range(n_cams)])[:, :, None]], axis=2)
    frames = checkerboard(n_cams, H, W)

    # every camera's frame through its own model, one launch; no map is written or read
    flat, valid = imaging.undistort_images(frames, np.arange(n_cams), intr, interpolation="bicubic", return_valid=True)
    print(f"undistorted {flat.shape} {flat.dtype}; {valid.mean():.1%} of the pixels have every tap inside the source")

    # the classical two-step form gives the same picture within one grey level
    two_step = imaging.undistort_images(frames, np.arange(n_cams), intr, interpolation="bicubic", method="mapped")
    print("fused against mapped: largest difference", int(np.max(np.abs(flat.astype(int) - two_step.astype(int)))), "grey level(s)")

    # rays: of a few detections, and of the whole sensor (image order, float32)
    px = rng.uniform([0, 0], [W - 1, H - 1], size=(5, 2))
    print("world rays of 5 pixels of camera 2:\n", imaging.pixel_rays(px, intr, cams=2, ext=ext, mode="normalised", world=True))
    smap = imaging.sensor_map(intr, (W, H), mode="linear", ext=ext, cam=1, dtype=np.float32)
    print("sensor map of camera 1:", smap.shape, smap.dtype, "centre ray", smap[H // 2, W // 2])

    # undistort and distort are inverse to the level five fixed-point steps give
    back = imaging.distort_points(imaging.undistort_points(px, intr, cams=0), intr, cams=0)
    print(f"distort(undistort(p)) - p: {np.max(np.abs(back - px)):.2e} px")

    # rectify cameras 0 and 1: rows of the results correspond
    ra, rb, Q = imaging.rectify_images(frames[0:1], frames[1:2], intr[0], ext[0], intr[1], ext[1], alpha=0.0)
    R_a, R_b, K_new, _ = imaging.rectify_images.last
    print(f"rectified pair {ra.shape}, new focal length {K_new[0]:.1f} px, baseline {-1.0 / Q[3, 2]:.3f}")


if __name__ == "__main__":
    main()
