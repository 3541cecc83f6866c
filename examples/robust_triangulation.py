#!/usr/bin/env python3
"""Triangulate features of which some were matched to the wrong place.

Twelve calibrated cameras see 750 features in 6 frames (0.3 px noise); in every feature seen by at least four cameras one view is moved
by 30-200 px (two views from eight cameras on), what a mismatched feature does.  ``refine_triangulation`` runs three times: as it is
(every view enters the DLT start), with a robust loss on the refinement (the start is still the plain one), and with ``consensus=64``
(view pairs are triangulated and scored on all views of the feature; DLT and refinement use the views within 8 px of the best pair —
the two-view RANSAC that COLMAP and OpenCV's sfm module put in front of their n-view triangulation).  Printed: the distance of the points
from the truth, the RMS reprojection error, and what the consensus flagged.

    python examples/robust_triangulation.py [--hypotheses 64] [--inlier-px 8]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--inlier-px", type=float, default=8.0)
    a = ap.parse_args()
    rig = synthetic.make_rig("tri-perm", 12, 6, synthetic.ccube_points(5, 30.0), seed=21, visibility=0.45, n_rings=2)
    it = rig.intr_true
    K = np.zeros((rig.n_cams, 3, 3))
    K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = it[:, 0], it[:, 1], it[:, 2], it[:, 3], 1.0
    P = np.stack([K[c] @ np.concatenate([Rotation.from_rotvec(rig.extr_true[c, :3]).as_matrix(), rig.extr_true[c, 3:, None]], axis=1)
                  for c in range(rig.n_cams)])
    D = np.ascontiguousarray(it[:, 4:9])
    d = rig.detections
    rec, start = ch.group_reconstructable(d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))])
    # the true point of every feature: the target point in the frame's pose
    truth = np.empty((len(start) - 1, 3))
    for j, row in enumerate(rec[start[:-1]]):
        pose = rig.poses_true[int(row[1])]
        truth[j] = Rotation.from_rotvec(pose[:3]).apply(rig.points[int(row[2])]) + pose[3:]

    rng = np.random.default_rng(3)
    moved = np.zeros(rec.shape[0], dtype=bool)
    for j in range(len(start) - 1):
        V = int(start[j + 1] - start[j])
        if V >= 4:
            moved[start[j] + rng.permutation(V)[: 1 if V < 8 else 2]] = True
    ang, mag = rng.uniform(0, 2 * np.pi, moved.sum()), rng.uniform(30.0, 200.0, moved.sum())
    rec[moved, -2:] += mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    hit = np.add.reduceat(moved.astype(int), start[:-1]) > 0

    print(f"{rec.shape[0]} views of {len(start) - 1} features, {int(moved.sum())} views moved by 30-200 px in {int(hit.sum())} features")
    print("run                      distance to the truth, features with a moved view [mm]: median     max | RMS of the kept views [px]: median")
    for name, kw in (("plain", {}), ("cauchy loss", dict(loss="cauchy", f_scale=1.0)),
                     (f"consensus of {a.hypotheses}", dict(consensus=a.hypotheses, inlier_px=a.inlier_px))):
        res = ch.refine_triangulation(rec, P, start, K, D, **kw)
        e = 1e3 * np.linalg.norm(res.points - truth, axis=1)[hit]
        print(f"{name:24s} {np.median(e):73.3f} {e.max():7.3f} | {np.median(res.rms[hit]):34.3f}")
    print(f"consensus: {int((~res.inliers).sum())} views flagged, {int((~res.inliers & moved).sum())} of the moved ones among them; "
          f"used at {int(res.consensus_used.sum())} features (three views and more)")


if __name__ == "__main__":
    main()
