#!/usr/bin/env python3
"""Triangulation refinement (pcs_tri_refine) at config 3 (the rig of tools/tri_bench.py): DLT alone against DLT + refinement as
device-event kernel times, the iteration histogram, RMS before and after, and the work the refinement did (view evaluations).

    python tools/tri_refine_bench.py [--reps 20] [--residuals] [--loss KIND] [--f-scale F] [--consensus H] [--inlier-px PX]
``--loss`` runs the robust instantiation of the refinement kernel (Triangulator.set_refine_loss; linear, the default, is the kernel without a loss).
``--consensus H`` puts the view-pair consensus in front (Triangulator.set_consensus; 0, the default, is the run without the stage): "DLT" is then
the stage and the DLT on the inliers, "refinement" the refinement of the inliers with the finish step.
Kernel times from rocprofv3 in a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o tri_refine -- python tools/tri_refine_bench.py --reps 5
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import synthetic  # noqa: E402
from pycamset_amd import compiled_helpers as hc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--residuals", action="store_true", help="also write the per-observation residuals")
ap.add_argument("--loss", default="linear", help="linear (default), huber, soft_l1, cauchy or arctan")
ap.add_argument("--f-scale", type=float, default=1.0)
ap.add_argument("--consensus", type=int, default=0, help="hypotheses per point of the view-pair consensus (0: off)")
ap.add_argument("--inlier-px", type=float, default=8.0)
args = ap.parse_args()

rig = synthetic.config_rig(3)
Kc = np.zeros((rig.n_cams, 3, 3)); it = rig.intr_true
Kc[:, 0, 0], Kc[:, 0, 2], Kc[:, 1, 1], Kc[:, 1, 2], Kc[:, 2, 2] = it[:, 0], it[:, 1], it[:, 2], it[:, 3], 1.0
from scipy.spatial.transform import Rotation  # noqa: E402
P = np.stack([Kc[c] @ np.concatenate([Rotation.from_rotvec(rig.extr_true[c, :3]).as_matrix(), rig.extr_true[c, 3:, None]], axis=1) for c in range(rig.n_cams)])
D = np.ascontiguousarray(it[:, 4:9])
d = rig.detections
d = d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))]
rec, start = hc.group_reconstructable(d)
n_pts, n_obs = len(start) - 1, rec.shape[0]
views = np.diff(start)
print(f"config 3: {n_obs} observations, {n_pts} points, views/point {views.min()}..{views.max()} (mean {views.mean():.1f})")

tri = hc.Triangulator(rig.n_cams)
tri.set_cameras(P, Kc, D)
tri.set_observations(rec[:, 0].astype(np.int32), rec[:, -2:], start)
if args.loss != "linear":   # a library without the robust kernel still runs the linear case
    tri.set_refine_loss(args.loss, args.f_scale)
if args.consensus > 0:      # ... and one without the stage the plain run
    tri.set_consensus(args.consensus, args.inlier_px, 0)
for _ in range(3):   # warm-up: code objects, visiting order, buffers
    tri.run(); tri.refine(residuals=args.residuals); tri.refined()
dlt_alone, dlt, ref = [], [], []
for _ in range(args.reps):   # DLT alone
    tri.run(); tri.synchronize(); dlt_alone.append(tri.last_kernel_ms())
for _ in range(args.reps):   # DLT + refinement, back to back on the handle's stream
    tri.run(); tri.refine(residuals=args.residuals); tri.synchronize()
    dlt.append(tri.last_kernel_ms()); ref.append(tri.last_refine_ms())
res = tri.refined()
med = lambda x: float(np.median(x)) * 1e3   # noqa: E731  (us)
print(f"device events, median of {args.reps}:  DLT alone {med(dlt_alone):7.1f} us   |   DLT {med(dlt):7.1f} us + refinement {med(ref):7.1f} us "
      f"= {med(dlt) + med(ref):7.1f} us   (refinement / DLT = {np.median(ref) / np.median(dlt):.2f}){'  [with residuals]' if args.residuals else ''}"
      f"  [loss {args.loss}, f_scale {args.f_scale:g}; consensus {args.consensus}; refinement min {min(ref) * 1e3:.1f} max {max(ref) * 1e3:.1f} us]")

if args.consensus > 0:
    inl, cinfo, _ = tri.consensus_results()
    used = cinfo[:, 3] != 0
    print(f"consensus: {args.consensus} hypotheses, inlier_px {args.inlier_px:g}: used at {int(used.sum())} of {n_pts} points, {int(inl.sum())} inliers of {n_obs} "
          f"observations, {int(np.sum(used & (cinfo[:, 0] == 0)))} points without a kept row; DLT min {min(dlt) * 1e3:.1f} max {max(dlt) * 1e3:.1f} us")
its = res.iterations
hist = np.bincount(its, minlength=hc.REFINE_DEFAULTS["max_iter"] + 1)
print("iterations (LM trials) histogram: " + "  ".join(f"{k}:{v}" for k, v in enumerate(hist) if v))
names = {hc.TRI_NOT_REFINED: "not refined", hc.TRI_CONVERGED: "converged", hc.TRI_MAX_ITER: "max_iter", hc.TRI_NO_DECREASE: "no decrease"}
print("status: " + "  ".join(f"{names[k]}:{v}" for k, v in enumerate(np.bincount(res.status, minlength=4)) if v))
print(f"RMS reprojection error [px]: DLT mean {res.rms_dlt.mean():.6f} median {np.median(res.rms_dlt):.6f}  ->  refined mean {res.rms.mean():.6f} "
      f"median {np.median(res.rms):.6f};  never worse: {bool(np.all(res.rms <= res.rms_dlt))}" + (" (the plain RMS may rise under a loss)" if args.loss != "linear" else ""))
print(f"point moved by the refinement [m]: median {np.median(np.linalg.norm(res.points - res.points_dlt, axis=1)):.3e}, "
      f"max {np.max(np.linalg.norm(res.points - res.points_dlt, axis=1)):.3e}")
# work: one pass over a point's views at the start and one per trial
evals = int(np.sum(views * (its + 1)))
t = np.median(ref) * 1e-3
print(f"view evaluations: {evals} ({evals / n_obs:.2f} per observation) -> {t / evals * 1e12:.1f} ps each, {evals / t:.3e} per second")
