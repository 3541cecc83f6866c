#!/usr/bin/env python3
"""Calibrate from detections of which some carry a wrong id, WITHOUT known intrinsics.

Three cameras see the calibration cube in six images (config 1; 0.3 px noise); a fraction of the detections of every (camera, image,
face) group is moved by 30-200 px, what a misread marker does.  ``calc_initial_params()`` has to estimate the intrinsics from the planar
views first (``compiled_helpers.estimate_intrinsics``): without ``intrinsics_consensus`` the bent homographies cost the cameras their
estimate and it raises; with ``intrinsics_consensus=64`` (64 hypotheses of 6 detections per group, scored on all of them; the closed
form and the refinement use the detections within 8 px of the best one — cv2.findHomography's RANSAC in place of the plain fit) and
``view_consensus=64`` behind it the seed exists, and ``lm_solve(loss="huber")`` finishes the calibration.  Printed: what the plain stage
returns, what the consensus flagged, and the intrinsics of the seed and of the solve against the truth.

    python examples/outlier_intrinsics.py [--hypotheses 64] [--moved 0.15]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import handlers, synthetic  # noqa: E402
from pycamset_amd.detections import TargetDetection  # noqa: E402
from pycamset_amd.device_solver import lm_solve  # noqa: E402


class Camset:   # the two methods of a CameraSet that the handler asks for; it holds no intrinsics
    def __init__(self, n):
        self.names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self.names)

    def get_n_cams(self):
        return len(self.names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--moved", type=float, default=0.15)
    a = ap.parse_args()
    rig = synthetic.config_rig(1, n_imgs=6)
    det = rig.detections.copy()
    per_face = rig.n_keys // 6
    face = np.arange(rig.n_keys) // per_face
    gid = (det[:, 0].astype(int) * rig.n_imgs + det[:, 1].astype(int)) * 6 + face[det[:, 2].astype(int)]
    rng = np.random.default_rng(3)
    moved = np.zeros(det.shape[0], dtype=bool)
    for g in np.unique(gid):
        rows = np.nonzero(gid == g)[0]
        moved[rng.permutation(rows)[: int(round(a.moved * rows.shape[0]))]] = True
    ang = rng.uniform(0, 2 * np.pi, int(moved.sum()))
    det[moved, 3:5] += rng.uniform(30.0, 200.0, ang.size)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)

    class Target:
        point_data = rig.points.reshape(6, per_face, 3).copy()

    kw = dict(n_cams=rig.n_cams, n_imgs=rig.n_imgs, board_of_key=face)
    plain = ch.estimate_intrinsics(det, rig.points, **kw)
    cons = ch.estimate_intrinsics(det, rig.points, consensus=a.hypotheses, **kw)
    print(f"{det.shape[0]} detections in {len(np.unique(gid))} groups, {int(moved.sum())} moved by 30-200 px")
    print(f"plain closed form: camera status {plain.status.tolist()} (0 = not estimated)")
    print(f"consensus of {a.hypotheses} hypotheses per group: camera status {cons.status.tolist()}, {int((~cons.inliers).sum())} rows flagged, "
          f"{int((~cons.inliers & moved).sum())} of the moved ones among them, {int((~cons.inliers & ~moved).sum())} others")

    def handler(**options):
        return handlers.TemplateBundleHandler(Camset(rig.n_cams), Target(), TargetDetection(Camset(rig.n_cams).names, det), options=dict({"verbosity": 0}, **options))

    try:
        handler().calc_initial_params()
    except ValueError as e:
        print(f"calc_initial_params() without the option: ValueError: {e}")
    h = handler(intrinsics_consensus=a.hypotheses, view_consensus=a.hypotheses)
    x0 = h.calc_initial_params()
    h.set_initial_params(x0)
    res = lm_solve(h, h.get_initial_params(), max_iter=200, loss="huber")

    def rel(x):
        K = np.asarray(h.get_bundle_adjustment_inputs(x)[0])
        return np.max(np.abs(K[:, :4] - rig.intr_true[:, :4]) / rig.intr_true[:, [0, 0, 2, 2]])

    print(f"with intrinsics_consensus and view_consensus: fx, cx, fy, cy of the seed off by {rel(x0):.2e} of the focal length, "
          f"after the huber solve {rel(res.x):.2e} (cost {res.cost:.2f}, {res.nit} trials)")


if __name__ == "__main__":
    main()
