#!/usr/bin/env python3
"""Times the per-image target pose in a calibrated rig (compiled_helpers.RigLocaliser, include/pcs_hip.h pcs_rigpose_run) at both group
widths, and the only other way to the same answer: device_solver.lm_solve through a handler with every camera in ``fixed_params``.

    python tools/rigpose_bench.py --shape tracking|rig32|sweep:CAMS:VIS [--images N] [--reps 7] [--loss KIND] [--f-scale F] [--joint] [--seed-eval]
                                  [--out FILE]

tracking: 8 cameras x 1e5 images of the 25-point board at visibility 0.2 (~40 detections per image); rig32: BASELINE config 3
(32 cameras x 200 images, ~5 000 detections per image); sweep:CAMS:VIS: CAMS cameras x 2 000 images of the 96-point cube at visibility VIS
(96 CAMS VIS detections per image), the shapes between the two that place the width rule's threshold.  Kernel time is the handle's event pair (``last_kernel_ms``: ordering of the
images + the LM kernel); host time is a host clock around run() + results(), which ends in a device synchronise.  The widths are
timed alternately after two warm-up calls each; median, minimum and maximum of ``--reps`` calls are printed as one JSON line per case.
``--loss`` runs the robust instantiation of the kernel (RigLocaliser.set_loss; linear, the default, is the kernel without a loss)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import pose_seeding, synthetic  # noqa: E402


def make(shape, images):
    if shape == "tracking":
        return synthetic.make_rig("tracking", 8, images or 100000, synthetic.charuco_points(6), seed=91, visibility=0.2, order="im")
    if shape.startswith("sweep:"):
        _, cams, vis = shape.split(":")
        return synthetic.make_rig(shape, int(cams), images or 2000, synthetic.ccube_points(5, 30.0), seed=92, visibility=float(vis), order="im")
    return synthetic.config_rig(3, order="im", n_imgs=images or None)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


class Names:
    def __init__(self, n):
        self.names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self.names)

    def get_n_cams(self):
        return len(self.names)


class Target:
    def __init__(self, points):
        self.point_data = np.array(points, dtype=np.float64)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, help="tracking, rig32 or sweep:CAMS:VIS")
    ap.add_argument("--images", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loss", default="linear", help="linear (default), huber, soft_l1, cauchy or arctan")
    ap.add_argument("--f-scale", type=float, default=1.0)
    ap.add_argument("--joint", action="store_true", help="also time lm_solve with every camera fixed on the same table")
    ap.add_argument("--seed-eval", action="store_true", help="LM evaluations of the joint solve from a seed with and without refine_poses")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    rig = make(a.shape, a.images)
    det = rig.detections
    I, C = rig.n_imgs, rig.n_cams
    E = pose_seeding.pose_to_4x4(rig.extr_true)[:, :3, :]
    order, ids, first = ch.group_by_image(det)
    ds = det if order is None else det[order]
    start = rig.poses.copy()          # the truth jiggled by 1 %
    start[0] = rig.poses_true[0]
    loc = ch.RigLocaliser(C, rig.n_keys)
    loc.set_cameras(rig.intr_true)
    loc.set_extrinsics(E)
    loc.set_template(rig.points)
    if a.loss != "linear":   # a library without the robust kernels still runs the linear case
        loc.set_loss(a.loss, a.f_scale)
    t0 = time.perf_counter()
    loc.set_observations(ds[:, 2].astype(np.int32), ds[:, 0].astype(np.int32), ds[:, 3:5], first)
    loc.set_start(start[ids])
    upload_s = time.perf_counter() - t0
    emit(case="table", shape=a.shape, cams=C, images=int(len(ids)), observations=int(det.shape[0]), mean_per_image=det.shape[0] / len(ids), upload_s=upload_s)
    kernel, host, out = {16: [], 64: []}, {16: [], 64: []}, {}
    for rep in range(-2, a.reps):
        for lanes in (16, 64):
            t0 = time.perf_counter()
            loc.run(group_lanes=lanes)
            out[lanes] = loc.results()
            dt = time.perf_counter() - t0
            if rep >= 0:
                host[lanes].append(dt * 1e3)
                kernel[lanes].append(loc.last_kernel_ms())
    for lanes in (16, 64):
        pose, rms, info, hess, _ = out[lanes]
        cost = float(np.nansum(rms[:, 0] ** 2 * info[:, 2]))
        emit(case="localise", shape=a.shape, lanes=lanes, loss=a.loss, f_scale=a.f_scale, kernel_ms=summary(kernel[lanes]), host_ms=summary(host[lanes]), sum_r2=cost,
             sum_r2_start=float(np.nansum(rms[:, 1] ** 2 * info[:, 2])), trials_mean=float(info[:, 0].mean()), trials_max=int(info[:, 0].max()),
             status_counts=np.bincount(info[:, 1], minlength=4).tolist())
    d = np.abs(out[16][0] - out[64][0])
    emit(case="widths", shape=a.shape, max_pose_difference=float(np.nanmax(d)))
    if a.joint:
        from pycamset_amd import device_solver, handlers
        from pycamset_amd.detections import TargetDetection

        names = Names(C)
        fixed = {n: {"ext": rig.extr_true[c].copy(), "int": rig.intr_true[c].copy()} for c, n in enumerate(names.names)}
        try:
            t0 = time.perf_counter()
            h = handlers.TemplateBundleHandler(names, Target(rig.points), TargetDetection(names.names, det, max_ims=I), fixed_params=fixed)
            x0 = start[1:].ravel()
            device_solver.lm_solve(h, x0, max_iter=1)     # warm-up: uploads the table, builds the structure
            setup_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            sol = device_solver.lm_solve(h, x0, max_iter=50, ftol=1e-10, xtol=1e-10, gtol=0.0)
            emit(case="joint", shape=a.shape, setup_s=setup_s, solve_ms=(time.perf_counter() - t0) * 1e3, sum_r2=2.0 * float(sol.cost), nfev=int(sol.nfev),
                 nit=int(sol.nit), status=int(sol.status), message=sol.message)
        except Exception as e:   # a measurement, not a test: what the joint path cannot do at this shape is a result too
            emit(case="joint", shape=a.shape, error=f"{type(e).__name__}: {e}"[:400])
    if a.seed_eval:
        from pycamset_amd import device_solver, handlers
        from pycamset_amd.detections import TargetDetection

        names = Names(C)
        for refine in (False, True):
            h = handlers.TemplateBundleHandler(names, Target(rig.points), TargetDetection(names.names, det, max_ims=I))
            t0 = time.perf_counter()
            x0 = h.calc_initial_params(rig.intr, seeding="graph", refine_poses=refine)
            seed_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            sol = device_solver.lm_solve(h, x0)
            emit(case="seed", shape=a.shape, refine_poses=refine, seed_s=seed_s, solve_s=time.perf_counter() - t0, nfev=int(sol.nfev), nit=int(sol.nit),
                 cost=float(sol.cost), status=int(sol.status))
    loc.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
