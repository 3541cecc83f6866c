#!/usr/bin/env python3
"""The relative pose of two cameras that look at a wall: eight-point against five-point hypotheses.

Two cameras see 60 points of an unknown scene with 0.2 px noise; ``--on-plane`` of them (default: all) lie on one plane that faces the
cameras, the common scene of a calibration (a board, a wall, a floor).  The eight-point hypotheses of ``estimate_two_view`` degenerate
there: the pair is refused, or worse, accepted with a wrong rotation.  ``solver="five-point"`` does not, and ``refine_iters`` polishes the
pose on the essential manifold.  Printed per solver: status, inliers, RMS Sampson distance and the error against the truth; then the
scene seed (``pose_seeding.seed_scene(two_view_solver="five-point")``) of five cameras whose shared points are mostly on the plane.

    python examples/planar_scene_seeding.py [--on-plane 60] [--consensus 64] [--refine 10]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import pose_seeding  # noqa: E402


def look_at(centre, target):
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ centre


def scene(n_cams, n_keys, n_plane, noise_px, rng, visible=None):
    """Cameras on an arc of radius 3 around points in a unit box, the first ``n_plane`` of them moved onto the plane y = 0.3 x."""
    pts = rng.uniform(-1.0, 1.0, (n_keys, 3))
    pts[:n_plane, 1] = 0.3 * pts[:n_plane, 0]
    intr = np.zeros((n_cams, 9))
    intr[:, 0] = intr[:, 2] = 1200.0
    intr[:, 1], intr[:, 3], intr[:, 4] = 640.0, 480.0, -0.05
    rows, poses = [], []
    for c in range(n_cams):
        ang = 0.45 * (c - 0.5 * (n_cams - 1))
        R, t = look_at(3.0 * np.array([np.sin(ang), -np.cos(ang), 0.15 * ((c % 3) - 1)]), np.zeros(3))
        poses.append((R, t))
        X = pts @ R.T + t
        x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
        k = 1.0 + intr[c, 4] * (x * x + y * y)
        uv = np.stack([intr[c, 0] * x * k + intr[c, 1], intr[c, 2] * y * k + intr[c, 3]], axis=1) + noise_px * rng.standard_normal((n_keys, 2))
        rows += [[c, 0, key, uv[key, 0], uv[key, 1]] for key in range(n_keys) if visible is None or visible(c, key)]
    return np.array(rows), intr, poses, pts


def pose_error(T, Ra, ta, Rb, tb):
    R = Rb @ Ra.T
    t = tb - R @ ta
    rot = np.arccos(np.clip((np.trace(T[:, :3] @ R.T) - 1.0) / 2.0, -1.0, 1.0))
    return rot, np.arccos(np.clip(T[:, 3] @ t / np.linalg.norm(t), -1.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--on-plane", type=int, default=60)
    ap.add_argument("--consensus", type=int, default=64)
    ap.add_argument("--refine", type=int, default=10)
    a = ap.parse_args()
    det, intr, poses, _ = scene(2, 60, a.on_plane, 0.2, np.random.default_rng(5))
    print(f"two cameras, 60 points, {a.on_plane} of them on one plane, 0.2 px noise")
    for solver, refine in (("eight-point", 0), ("five-point", 0), ("five-point", a.refine)):
        r = ch.estimate_two_view(det, intr, consensus=a.consensus, solver=solver, refine_iters=refine)
        line = f"  {solver:11s} refine {refine:2d}: status {int(r.status[0])}, {int(r.n_inliers[0])} inliers"
        if r.status[0] == ch.TWOVIEW_OK:
            rot, tra = pose_error(r.T[0], *poses[0], *poses[1])
            line += f", RMS {r.rms[0]:.3f} px, rotation {rot:.2e} rad and translation direction {tra:.2e} rad off"
        print(line)
    det, intr, poses, pts = scene(5, 60, 48, 0.2, np.random.default_rng(7), visible=lambda c, k: k % 3 <= c <= k % 3 + 2)
    seed = pose_seeding.seed_scene(det, intr, 5, consensus=a.consensus, two_view_solver="five-point", two_view_refine=a.refine)
    print(f"five cameras, 48 of 60 points on the plane: placed in round {seed.round_of_camera.tolist()}, first pair {seed.first_pair}, "
          f"{int(np.all(np.isfinite(seed.points), axis=1).sum())} points triangulated")


if __name__ == "__main__":
    main()
