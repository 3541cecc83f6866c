#!/usr/bin/env python3
"""A calibrated pair to a point cloud on the device: the reference's ``stereo_reconstruct`` (reconstruction/reconstruction_utils.py:
170-223) with pycamset_amd — rectify both images in one fused remap each, match blocks (or, with ``--method sgm``, the reference's
``matlab=True`` branch: semi-global matching on a census cost), reproject, mask by depth, compact.

The scene is synthetic so that the example needs no files: an analytically textured plane one metre in front of two distorted cameras
12 cm apart.  Every pixel's ray (``imaging.pixel_rays``) is intersected with the plane and the texture is evaluated there.

    python examples/stereo_reconstruct.py [--method sgm]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pycamset_amd import imaging, stereo  # noqa: E402

W, H, Z0 = 320, 240, 1.0
INTR = np.array([[395.0, 158.3, 396.0, 121.2, -0.06, 0.015, 0.0008, -0.0006, 0.0], [402.0, 161.1, 401.0, 118.9, -0.05, 0.01, -0.0005, 0.0007, 0.0]])


def extrinsics():
    out = []
    for w, c in (([0.01, -0.015, 0.005], [-0.06, 0.002, 0.0]), ([-0.012, 0.02, -0.008], [0.06, -0.001, 0.004])):
        R = Rotation.from_rotvec(w).as_matrix()
        out.append(np.concatenate([R, (-R @ np.array(c))[:, None]], axis=1))
    return out


def texture(X, Y):
    return 127.5 + 45.0 * np.sin(61.0 * X + 2.0 * np.sin(23.0 * Y)) + 40.0 * np.sin(47.0 * Y + 13.0 * X * X) + 35.0 * np.sin(29.0 * (X + Y) + 5.0 * np.cos(37.0 * X))


def render(K, E):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = imaging.pixel_rays(np.stack([xs, ys], axis=-1).reshape(-1, 2), K, ext=E[None], world=True)
    c = -E[:, :3].T @ E[:, 3]
    P = c[None, :] + ((Z0 - c[2]) / rays[:, 2])[:, None] * rays
    return np.clip(np.rint(texture(P[:, 0], P[:, 1])), 0, 255).astype(np.uint8).reshape(H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=("block", "sgm"), default="block")
    method = ap.parse_args().method
    Ea, Eb = extrinsics()
    A, B = render(INTR[0], Ea), render(INTR[1], Eb)
    options = dict(block=15) if method == "block" else dict(census=(9, 7), p1=8, p2=32, paths=8)
    (points, grey), = stereo.stereo_reconstruct(A, B, INTR[0], Ea, INTR[1], Eb, num_disp=64, depth_range=(0.2, 3.0), frame="world", lr_max_diff=1, method=method, **options)
    _, _, Q, disp, min_disp = stereo.stereo_reconstruct.last
    ok = disp != 16 * (min_disp - 1)
    print(f"{W} x {H} pair, {method}: {int(ok.sum())} of {ok.size} pixels matched, median disparity {np.median(disp[ok]) / 16:.2f} px")
    step = Z0 * Z0 / (Q[2, 3] / abs(Q[3, 2]))
    err = np.abs(points[:, 2] - Z0)
    print(f"{len(points)} points in the world; distance from the plane Z = {Z0}: median {np.median(err):.5f}, 95 % {np.quantile(err, 0.95):.5f} "
          f"(one disparity step at this depth: {step:.5f}); grey values {grey.min()} .. {grey.max()}")
    if not np.median(err) <= step:
        raise SystemExit("the cloud does not lie on the plane")


if __name__ == "__main__":
    main()
