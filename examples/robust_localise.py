#!/usr/bin/env python3
"""Locate the target in tracked frames of a calibrated rig when a camera misreads a few corners.

A 4-camera rig sees the cube in 6 frames (0.3 px noise).  In every frame three detections are displaced by 25-60 px: misread marker
corners.  ``localise_target`` is run three times from the same start: on the clean table, on the contaminated table with the
default linear loss, and on the contaminated table with ``loss="cauchy"``.  The plain sum of squares lets the outliers drag every
pose; under the loss the poses return to those of the clean table, the reported ``rms`` stays the plain pixel RMS (so it shows that
something is off), and ``diagnostics.robust_weights`` on the returned residuals lists the detections that were down-weighted.

    python examples/robust_localise.py [--loss cauchy] [--f-scale 1.0]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import diagnostics, pose_seeding, synthetic  # noqa: E402


def pose_error(a, b):
    ang = (Rotation.from_rotvec(a[:, :3]).inv() * Rotation.from_rotvec(b[:, :3])).magnitude()
    return np.degrees(ang), 1e3 * np.linalg.norm(a[:, 3:] - b[:, 3:], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", default="cauchy")
    ap.add_argument("--f-scale", type=float, default=1.0, help="pixels: residuals well beyond this are treated as outliers")
    a = ap.parse_args()
    rig = synthetic.make_rig("robust-example", 4, 6, synthetic.ccube_points(5, 30.0), seed=5, noise_px=0.3, visibility=0.5)
    E = pose_seeding.pose_to_4x4(rig.extr_true)[:, :3, :]
    clean = rig.detections
    dirty = clean.copy()
    rng = np.random.default_rng(0)
    bad = np.concatenate([rng.choice(np.nonzero(clean[:, 1] == i)[0], 3, replace=False) for i in range(rig.n_imgs)])
    ang = rng.uniform(0, 2 * np.pi, bad.shape[0])
    dirty[bad, 3:5] += rng.uniform(25.0, 60.0, bad.shape[0])[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)

    args = (rig.points, rig.intr_true, E)
    ref = ch.localise_target(clean, *args)                                   # the default start (rig_pose_start) is linear in every call
    lin = ch.localise_target(dirty, *args, poses_init=ref.poses_init)
    rob = ch.localise_target(dirty, *args, poses_init=lin.poses, loss=a.loss, f_scale=a.f_scale, return_residuals=True)
    print("frame  detections | linear: deg    mm   rms px | %-8s deg    mm   rms px   cost" % (a.loss + ":"))
    for i, (dl, tl, dr, tr) in enumerate(zip(*pose_error(lin.poses, ref.poses), *pose_error(rob.poses, ref.poses))):
        print(f"{i:5d}  {rob.n_points[i]:10d} | {dl:11.4f} {tl:5.2f} {lin.rms[i]:8.3f} | {dr:12.4f} {tr:5.2f} {rob.rms[i]:8.3f} {rob.cost[i]:6.2f}")
    w = diagnostics.robust_weights(rob.residuals, a.loss, a.f_scale).min(axis=1)
    flagged = np.nonzero(w < 0.1)[0]
    print(f"down-weighted below 0.1: {len(flagged)} detections, {len(np.intersect1d(flagged, bad))} of the {len(bad)} displaced ones among them")
    sd = np.sqrt(np.diagonal(rob.covariance(), axis1=1, axis2=2))
    print("standard errors of frame 0 under the loss (rad, rad, rad, m, m, m):", np.array2string(sd[0], precision=2))


if __name__ == "__main__":
    main()
