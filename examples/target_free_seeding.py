#!/usr/bin/env python3
"""Bundle adjustment of a scene nobody measured: from a table of matched image points to a solved calibration.

Six cameras on an arc see 120 points of an unknown scene (0.3 px noise); 5 % of the detections are wrong matches, moved to random
pixels.  Nothing is known but the intrinsics.  ``FreePointBundleHandler.calc_initial_params(seeding="scene")`` seeds the problem on the
device (``pose_seeding.seed_scene``): two-view consensus on every camera pair, the best pair fixes the frame and the scale, the rest
follows by triangulation and resection in rounds; ``lm_solve(loss="cauchy")`` then refines cameras and points together.  Printed: what
the seed placed in which round, and how far seed and solution are from the truth after a similarity alignment.

    python examples/target_free_seeding.py [--consensus 64] [--moved 0.05]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
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


def aligned_error(points, truth):
    """RMS distance to the truth after the best similarity, relative to the size of the scene."""
    ok = np.all(np.isfinite(points), axis=1)
    X, Y = points[ok], truth[ok]
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    U, S, Vt = np.linalg.svd((Y - my).T @ (X - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = np.trace(np.diag(S) @ D) / np.sum((X - mx) ** 2)
    err = (X - mx) @ (s * U @ D @ Vt).T + my - Y
    return float(np.sqrt(np.mean(np.sum(err ** 2, axis=1))) / np.linalg.norm(Y.max(axis=0) - Y.min(axis=0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--consensus", type=int, default=64)
    ap.add_argument("--moved", type=float, default=0.05)
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    C, K = 6, 120
    points = rng.uniform(-0.05, 0.05, (K, 3))
    rig = synthetic.make_rig("scene-6", C, 1, points, seed=3, visibility=1.0, noise_px=0.3)
    det = rig.detections.copy()
    bad = rng.choice(det.shape[0], int(a.moved * det.shape[0]), replace=False)
    det[bad, 3:5] = rng.uniform([0.0, 0.0], 2.0 * rig.intr_true[det[bad, 0].astype(int)][:, [1, 3]])
    names = Camset(C).names
    fixed = {n: {"int": rig.intr_true[i].copy()} for i, n in enumerate(names)}
    fixed["cam_0"]["ext"] = np.zeros(6)   # the gauge of the seed: camera 0 is the world
    h = handlers.FreePointBundleHandler(Camset(C), Target(np.zeros((K, 3))), TargetDetection(names, det), fixed_params=fixed, options={"verbosity": 0})
    opts = {"consensus": a.consensus, "resect_opts": {"consensus": a.consensus}, "tri_opts": {"consensus": a.consensus}}
    x0 = h.calc_initial_params(rig.intr_true, seeding="scene", scene_opts=opts)
    seed = h.scene_seed
    tv = seed.two_view
    print(f"{det.shape[0]} detections of {K} points in {C} cameras, {bad.size} of them wrong matches")
    print(f"two-view: {tv.pairs.shape[0]} pairs, {int((tv.status == 0).sum())} OK; first pair {seed.first_pair} "
          f"(parallax {np.degrees(tv.parallax[np.all(tv.pairs == seed.first_pair, axis=1)][0]):.1f} deg)")
    print(f"placed in round: {seed.round_of_camera.tolist()}; {int(np.all(np.isfinite(seed.points), axis=1).sum())} points triangulated")
    res = lm_solve(h, x0, max_iter=100, loss="cauchy", f_scale=1.0)
    solved = np.asarray(h.get_bundle_adjustment_inputs(res.x)[2]).reshape(-1, 3)
    print(f"seed:     points {aligned_error(seed.points, points):.2e} of the scene size off")
    print(f"solution: points {aligned_error(solved, points):.2e} of the scene size off, cost {res.cost:.2f} after {res.nit} steps ({res.message})")


if __name__ == "__main__":
    main()
