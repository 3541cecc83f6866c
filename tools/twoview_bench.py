#!/usr/bin/env python3
"""Stage times of the two-view consensus (include/pcs_hip.h pcs_twoview_run) on the rig-32 free-chain table.

The rig-32 table (32 cameras on two rings, 200 poses of the Ccube target) read as a scene nobody measured: every (image, key) is one
free point, key' = image * K + key.  Every camera pair with at least ``--min-points`` shared points is one pair of the handle.  Printed
per hypothesis count: the device time of every stage (events around the launches), their sum, and what came out.

    python tools/twoview_bench.py [--imgs 200] [--hypotheses 16 64 256] [--solver five-point] [--refine 10] [--repeat 5] [--json out.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import synthetic  # noqa: E402


def free_chain_table(rig):
    det = rig.detections.copy()
    det[:, 2] = det[:, 1] * rig.n_keys + det[:, 2]
    det[:, 1] = 0
    return det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imgs", type=int, default=200)
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--min-points", type=int, default=16)
    ap.add_argument("--inlier-px", type=float, default=2.0)
    ap.add_argument("--solver", choices=sorted(ch.TWOVIEW_SOLVERS), default="eight-point")
    ap.add_argument("--refine", type=int, default=0, help="LM trials that refine the final pose (0: none)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    rig = synthetic.config_rig(3, n_imgs=a.imgs)
    det = free_chain_table(rig)
    t0 = time.perf_counter()
    first = ch.estimate_two_view(det, rig.intr, consensus=a.hypotheses[0], inlier_px=a.inlier_px, min_points=a.min_points, solver=a.solver,
                                 refine_iters=a.refine)
    host_s = time.perf_counter() - t0
    n_pairs, n_corr = first.pairs.shape[0], first.uv_a.shape[0]
    print(f"rig-32 free-chain table: {det.shape[0]} detections, {n_pairs} pairs, {n_corr} correspondences "
          f"(mean {n_corr / max(1, n_pairs):.0f} per pair); first call with table building {host_s:.2f} s")
    est = ch.TwoViewEstimator(rig.n_cams)
    est.set_cameras(rig.intr)
    est.set_correspondences(first.uv_a, first.uv_b, first.start, first.pairs)
    est.set_solver(a.solver, a.refine)
    print(f"solver {a.solver}, {a.refine} refinement trials")
    out = []
    for H in a.hypotheses:
        est.set_consensus(H, a.inlier_px, 0)
        runs = []
        for _ in range(a.repeat + 1):   # the first run grows the buffers
            est.run(min_points=a.min_points)
            T, info, stats, inl = est.results()
            runs.append(est.last_kernel_ms())
        ms = {k: float(np.median([r[k] for r in runs[1:]])) for k in ch.TWOVIEW_STAGES}
        ok = info[:, 3] == ch.TWOVIEW_OK
        row = {"hypotheses": H, "stage_ms": ms, "total_ms": sum(ms.values()), "pairs_ok": int(ok.sum()), "inlier_fraction": float(inl.mean()),
               "median_rms_px": float(np.median(stats[ok, 1])) if ok.any() else None}
        out.append(row)
        print(f"H = {H:3d}: " + "  ".join(f"{k} {v:8.3f} ms" for k, v in ms.items()) + f"  | total {row['total_ms']:8.3f} ms, "
              f"{row['pairs_ok']} / {n_pairs} pairs OK, inliers {row['inlier_fraction']:.3f}, median RMS {row['median_rms_px']} px")
    est.close()
    if a.json:
        Path(a.json).write_text(json.dumps({"detections": int(det.shape[0]), "pairs": n_pairs, "correspondences": n_corr, "solver": a.solver, "refine_iters": a.refine,
                                              "runs": out}, indent=1))


if __name__ == "__main__":
    main()
