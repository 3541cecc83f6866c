#!/usr/bin/env python3
"""Batched target-pose estimation (pcs_pnp_run) at config 1, ring-8, rig-32 (6 400 views, about 1e6 observations) and a ChArUco rig of
the rig-32 shape: device time of a run (ordering of the views + start + LM kernels, device events), the iteration histogram, the
statuses and the RMS at the start and at the returned pose.

    python tools/pnp_bench.py [--reps 10] [--configs 1,2,3,charuco] [--consensus H [--moved 0.03]]
--consensus H puts the consensus stage in front (pcs_pnp_set_consensus: H hypotheses of 6 detections per view, 8 px); --moved F first moves
that fraction of the detections by 20 - 50 px, so that there is something to find.  Without --consensus the runs are the plain ones.
Kernel times from rocprofv3 in a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o pnp -- python tools/pnp_bench.py --reps 3 --configs 3
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import synthetic  # noqa: E402
from pycamset_amd import compiled_helpers as hc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--configs", default="1,2,3,charuco")
ap.add_argument("--consensus", type=int, default=0, help="hypotheses per view of the consensus stage (0: off)")
ap.add_argument("--moved", type=float, default=0.0, help="fraction of the detections moved by 20 - 50 px before the run")
args = ap.parse_args()


def rig_of(name):
    if name == "charuco":   # planar target on the two-ring rig: every view takes the homography start and both planar candidates
        return synthetic.make_rig("charuco-32", 32, 200, synthetic.charuco_points(17, 4.0), seed=13, visibility=0.6, n_rings=2)
    return synthetic.config_rig(int(name))


names = {hc.PNP_NOT_ESTIMATED: "not estimated", hc.PNP_CONVERGED: "converged", hc.PNP_MAX_ITER: "max_iter", hc.PNP_NO_DECREASE: "no decrease"}
for cfg in args.configs.split(","):
    rig = rig_of(cfg)
    d = rig.detections
    moved = np.zeros(d.shape[0], dtype=bool)
    if args.moved > 0.0:
        rng = np.random.default_rng(5)
        d = d.copy()
        bad = rng.choice(d.shape[0], max(1, int(args.moved * d.shape[0])), replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, bad.size), rng.uniform(20.0, 50.0, bad.size)
        d[bad, 3] += mag * np.cos(ang)
        d[bad, 4] += mag * np.sin(ang)
        moved[bad] = True
    order, ids, start = hc.group_by_view(d, rig.n_imgs)
    ds = d if order is None else d[order]
    n = np.diff(start)
    est = hc.PoseEstimator(rig.n_cams, rig.n_keys)
    est.set_cameras(rig.intr)   # the jiggled intrinsics: what a calibration starts from
    est.set_template(rig.points)
    est.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (ids // rig.n_imgs).astype(np.int32))
    if args.consensus:
        est.set_consensus(args.consensus)
    for _ in range(2):   # warm-up: code objects, visiting order, buffers
        est.run(); est.results()
    ms = []
    for _ in range(args.reps):
        est.run(); est.results(); ms.append(est.last_kernel_ms())
    pose, init, alt, rms, info, _ = est.results()
    ok = info[:, 1] != hc.PNP_NOT_ESTIMATED
    print(f"{rig.name}: {d.shape[0]} observations, {len(n)} views, observations/view {n.min()}..{n.max()} (mean {n.mean():.1f}), "
          f"planar views {int(np.isfinite(alt[:, 0]).sum())}")
    print(f"  device time of a run, median of {args.reps}: {np.median(ms) * 1e3:9.1f} us (min {np.min(ms) * 1e3:.1f})")
    print("  iterations (LM trials of the kept candidate): " + "  ".join(f"{k}:{v}" for k, v in enumerate(np.bincount(info[:, 0])) if v))
    print("  status: " + "  ".join(f"{names[k]}:{v}" for k, v in enumerate(np.bincount(info[:, 1], minlength=4)) if v))
    print(f"  RMS [px]: start mean {rms[ok, 1].mean():.4f} median {np.median(rms[ok, 1]):.4f} max {rms[ok, 1].max():.3f}  ->  "
          f"returned mean {rms[ok, 0].mean():.4f} median {np.median(rms[ok, 0]):.4f} max {rms[ok, 0].max():.3f};  never worse: {bool(np.all(rms[ok, 0] <= rms[ok, 1]))}")
    if args.consensus:
        flags, cinfo, score = est.consensus_results()
        ms_moved = moved if order is None else moved[order]
        print(f"  consensus, {args.consensus} hypotheses: {int(flags.sum())} inliers of {d.shape[0]}; moved detections flagged as inliers {int((flags & ms_moved).sum())} "
              f"of {int(ms_moved.sum())}, others dropped {int((~flags & ~ms_moved).sum())}; views using it {int(cinfo[:, 3].sum())}, "
              f"finite hypotheses per view min {cinfo[:, 2].min()} mean {cinfo[:, 2].mean():.1f}")
    evals = int(np.sum(n[ok] * (info[ok, 0] + 1)))
    print(f"  observation evaluations of the kept candidates: {evals} ({evals / max(1, d.shape[0]):.2f} per observation)")
    est.close()
