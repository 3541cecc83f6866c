#!/usr/bin/env python3
"""Seed a calibration from detections of which a few carry a wrong id.

A ring of 8 cameras sees a ChArUco board in 12 images (0.3 px noise); 3 % of the detections are moved by 20-50 px, what a misread
marker does.  ``calc_initial_params`` seeds the calibration twice: with the plain per-view poses (every detection of a view enters its
linear start) and with ``view_consensus=64`` (64 hypotheses of 6 detections per view, scored on all of them; start and LM use the
detections within 8 px of the best one — cv2.solvePnPRansac in place of cv2.solvePnPGeneric).  Both starts are then solved with
``lm_solve(loss="cauchy")``.  Printed: how far each seed's camera and image poses are from the truth, what the consensus flagged, and
the focal errors after the solve.  The intrinsics are given here; where they have to be estimated from the same detections first, the
stage in front needs its own consensus: ``examples/outlier_intrinsics.py`` (``intrinsics_consensus=64``).

    python examples/outlier_seeding.py [--hypotheses 64] [--moved 0.03]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import handlers, synthetic  # noqa: E402
from pycamset_amd.detections import TargetDetection  # noqa: E402
from pycamset_amd.device_solver import lm_solve  # noqa: E402


class Camset:   # the two methods of a CameraSet that the handler asks for
    def __init__(self, n):
        self.names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self.names)

    def get_n_cams(self):
        return len(self.names)


class Target:
    def __init__(self, points):
        self.point_data = np.array(points, dtype=np.float64)[None]


def pose_error(a, b):
    ang = (Rotation.from_rotvec(a[:, :3]).inv() * Rotation.from_rotvec(b[:, :3])).magnitude()
    return np.degrees(ang).max(), 1e3 * np.linalg.norm(a[:, 3:] - b[:, 3:], axis=1).max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--moved", type=float, default=0.03)
    a = ap.parse_args()
    rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
    det = rig.detections.copy()
    rng = np.random.default_rng(5)
    bad = rng.choice(det.shape[0], max(1, int(a.moved * det.shape[0])), replace=False)
    ang = rng.uniform(0, 2 * np.pi, bad.size)
    det[bad, 3:5] += rng.uniform(20.0, 50.0, bad.size)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)

    vp = ch.estimate_view_poses(det, rig.points, rig.intr, n_imgs=rig.n_imgs, consensus=a.hypotheses)
    moved = np.zeros(det.shape[0], dtype=bool)
    moved[bad] = True
    print(f"{det.shape[0]} detections, {bad.size} moved by 20-50 px; consensus of {a.hypotheses} hypotheses per view: "
          f"{int((~vp.inliers).sum())} flagged, {int((~vp.inliers & moved).sum())} of the moved ones among them")
    print("seed        cameras: deg     mm | images: deg     mm | after cauchy: focal error px   cost   trials")
    for name, n_hyp in (("plain", 0), ("consensus", a.hypotheses)):
        h = handlers.TemplateBundleHandler(Camset(rig.n_cams), Target(rig.points), TargetDetection(Camset(rig.n_cams).names, det), options={"verbosity": 0})
        x0 = h.calc_initial_params(rig.intr, view_consensus=n_hyp)
        _, extr, poses = h.get_bundle_adjustment_inputs(x0)[:3]
        (de, te), (dp, tp) = pose_error(extr, rig.extr_true), pose_error(poses, rig.poses_true)
        h.set_initial_params(x0)
        res = lm_solve(h, h.get_initial_params(), max_iter=200, loss="cauchy", f_scale=1.0)
        intr = np.asarray(h.get_bundle_adjustment_inputs(res.x)[0])
        focal = np.max(np.abs(intr[:, [0, 2]] - rig.intr_true[:, [0, 2]]))
        print(f"{name:10s} {de:13.4f} {te:6.2f} | {dp:11.4f} {tp:6.2f} | {focal:27.4f} {res.cost:8.2f} {res.nit:6d}")


if __name__ == "__main__":
    main()
