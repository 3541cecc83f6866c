#!/usr/bin/env python3
"""Intrinsics from planar views (pcs_intr_run) at config 1 and rig-32 (cube faces as boards), ring-8 and a ChArUco rig of the rig-32
shape (one board): device time of a run (homography + camera kernels, device events), the group and camera statuses, the error of
the closed form against the rig's true intrinsics, and with --refine the wall time and result of the refinement.

    python tools/intrinsics_bench.py [--reps 10] [--configs 1,2,3,charuco] [--model auto|full|focal] [--res] [--refine] [--consensus H [--moved 0.15]]
--consensus H puts the consensus stage in front (pcs_intr_set_consensus: H hypotheses of 6 detections per group, 8 px); --moved F first moves
that fraction of the detections by 30 - 200 px, so that there is something to find.  Without --consensus the runs are the plain ones.
Kernel times from rocprofv3 in a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o intr -- python tools/intrinsics_bench.py --reps 3 --configs 3
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import synthetic  # noqa: E402
from pycamset_amd import compiled_helpers as hc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--configs", default="1,2,3,charuco")
ap.add_argument("--model", default="auto")
ap.add_argument("--res", action="store_true", help="pass res = (1000, 1000): the rigs' principal points are 500 +- 20")
ap.add_argument("--refine", action="store_true")
ap.add_argument("--consensus", type=int, default=0, help="hypotheses per group of the consensus stage (0: off)")
ap.add_argument("--moved", type=float, default=0.0, help="fraction of the detections moved by 30 - 200 px before the run")
args = ap.parse_args()


def rig_of(name):
    if name == "charuco":
        return synthetic.make_rig("charuco-32", 32, 200, synthetic.charuco_points(17, 4.0), seed=13, visibility=0.6, n_rings=2)
    return synthetic.config_rig(int(name))


for cfg in args.configs.split(","):
    rig = rig_of(cfg)
    d = rig.detections
    moved = np.zeros(d.shape[0], dtype=bool)
    if args.moved > 0.0:
        d = d.copy()
        rng = np.random.default_rng(5)
        bad = rng.choice(d.shape[0], max(1, int(args.moved * d.shape[0])), replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, bad.size), rng.uniform(30.0, 200.0, bad.size)
        d[bad, 3] += mag * np.cos(ang)
        d[bad, 4] += mag * np.sin(ang)
        moved[bad] = True
    cube = rig.n_keys == 486
    bok = np.repeat(np.arange(6), 81) if cube else np.zeros(rig.n_keys, dtype=np.int64)
    n_boards = 6 if cube else 1
    order, gid, start = hc.group_by_board(d, rig.n_imgs, bok, n_boards)
    ds = d if order is None else d[order]
    n = np.diff(start)
    est = hc.IntrinsicsEstimator(rig.n_cams, rig.n_keys)
    est.set_template(rig.points)
    est.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (gid // (rig.n_imgs * n_boards)).astype(np.int32))
    res = np.full((rig.n_cams, 2), 1000.0) if args.res else None
    if args.consensus:
        est.set_consensus(args.consensus)
    for _ in range(2):   # warm-up: code objects, buffers
        est.run(args.model, 13, res); est.results()
    ms = []
    for _ in range(args.reps):
        est.run(args.model, 13, res); est.results(); ms.append(est.last_kernel_ms())
    K, cinfo, eig, H, frames, ginfo, pix = est.results()
    ok = cinfo[:, 0] != hc.INTR_NOT_ESTIMATED
    print(f"{rig.name}: {d.shape[0]} observations, {len(n)} groups, observations/group {n.min()}..{n.max()} (mean {n.mean():.1f}), {rig.n_cams} cameras")
    print(f"  device time of a run, median of {args.reps}: {np.median(ms) * 1e3:9.1f} us (min {np.min(ms) * 1e3:.1f})")
    print("  group status [too few, used, not planar, not finite, fit failed]: " + " ".join(str(v) for v in np.bincount(ginfo[:, 0], minlength=5)))
    print("  camera status [not estimated, full, focal, fallback]: " + " ".join(str(v) for v in np.bincount(cinfo[:, 0], minlength=4)))
    if args.consensus:
        flags, gc, score = est.consensus_results()
        ms_moved = moved if order is None else moved[order]
        print(f"  consensus, {args.consensus} hypotheses: {int(flags.sum())} inliers of {d.shape[0]}; moved detections flagged as inliers {int((flags & ms_moved).sum())} "
              f"of {int(ms_moved.sum())}, others dropped {int((~flags & ~ms_moved).sum())}; groups using it {int(gc[:, 3].sum())}, "
              f"without a finite hypothesis {int(((gc[:, 3] != 0) & (gc[:, 1] < 0)).sum())}; finite hypotheses per group, median {np.median(gc[:, 2]):.0f}")
    if ok.any():
        rel = np.abs(K[ok, :4] - rig.intr_true[ok, :4]) / np.abs(rig.intr_true[ok][:, [0, 0, 2, 2]])
        print(f"  closed form against the truth (distorted, 0.3 px noise), relative to the focal length: median {np.median(rel):.3e} max {rel.max():.3e}; "
              f"eigenvalue ratio median {np.nanmedian(eig):.1e} max {np.nanmax(eig):.1e}")
    est.close()
    if args.refine:
        t0 = time.perf_counter()
        r = hc.estimate_intrinsics(d, rig.points, n_cams=rig.n_cams, n_imgs=rig.n_imgs, board_of_key=bok, model=args.model, res=res, refine=True,
                                   consensus=args.consensus)
        wall = time.perf_counter() - t0
        good = r.status != hc.INTR_NOT_ESTIMATED
        rel = np.abs(r.intr[good] - rig.intr_true[good])[:, :4] / np.abs(rig.intr_true[good][:, [0, 0, 2, 2]])
        print(f"  refine=True: {wall * 1e3:.1f} ms wall (grouping, closed form, PnP, LM with {r.lm.nit} iterations, status {r.lm.status}); RMS "
              f"{np.nanmedian(r.rms_init):.3f} -> {np.nanmedian(r.rms):.3f} px; fx, cx, fy, cy against the truth: median {np.median(rel):.3e} max {rel.max():.3e}")
