#!/usr/bin/env python3
"""Stage times of the batched point-set registration (include/pcs_hip.h pcs_align_run).

One problem per image: a target of ``--keys`` features whose 3-D points were measured in ``--images`` images (noise ``--noise``, a
fraction ``--outliers`` of every image's rows replaced by points anywhere around the target), registered onto the template.  Printed
per hypothesis count and group width: the device time of every stage (events around the launches), their sum, and what came out.

    python tools/align_bench.py [--images 2000] [--keys 486] [--consensus 0 64] [--model rigid] [--lanes 16 64] [--repeat 5] [--json out.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import compiled_helpers as ch  # noqa: E402
from pycamset_amd import synthetic  # noqa: E402


def make_table(n_imgs, n_keys, noise, outliers, seed=0):
    """-> (src, dst (I K, 3), start (I + 1,), outlier (I K,) bool, true poses (I, 6))."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_keys / 6.0))) + 1
    tmpl = synthetic.ccube_points(side, 40.0)[:n_keys]
    if tmpl.shape[0] < n_keys:
        raise SystemExit(f"--keys {n_keys}: the cube target of this tool has {tmpl.shape[0]} features at most")
    poses = np.concatenate([rng.normal(0.0, 0.5, (n_imgs, 3)), rng.normal(0.0, 0.05, (n_imgs, 3))], axis=1)
    R = Rotation.from_rotvec(poses[:, :3]).as_matrix()
    dst = np.einsum("iab,kb->ika", R, tmpl) + poses[:, None, 3:] + rng.normal(0.0, noise, (n_imgs, n_keys, 3))
    bad = rng.random((n_imgs, n_keys)) < outliers
    dst[bad] = rng.uniform(-0.1, 0.1, (int(bad.sum()), 3))
    return np.broadcast_to(tmpl, dst.shape).reshape(-1, 3).copy(), dst.reshape(-1, 3), np.arange(n_imgs + 1, dtype=np.int64) * n_keys, bad.ravel(), poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--keys", type=int, default=486)
    ap.add_argument("--consensus", type=int, nargs="+", default=[0, 64])
    ap.add_argument("--model", choices=sorted(ch.ALIGN_MODEL_IDS), default="rigid")
    ap.add_argument("--lanes", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--noise", type=float, default=5e-5, help="noise of a measured coordinate, metres")
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--inlier-dist", type=float, default=5e-4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    src, dst, start, bad, poses = make_table(a.images, a.keys, a.noise, a.outliers)
    print(f"{a.images} images x {a.keys} keys = {src.shape[0]} rows, model {a.model}, {bad.mean():.3f} outliers, noise {a.noise} m, inlier distance {a.inlier_dist} m")
    al = ch.PointAligner()
    al.set_points(src, dst, start)
    R_true = Rotation.from_rotvec(poses[:, :3]).as_matrix()
    out = []
    for H in a.consensus:
        al.set_consensus(H, a.inlier_dist if H else 0.0, 0)
        for lanes in a.lanes:
            runs = []
            for _ in range(a.repeat + 1):   # the first run grows the buffers
                al.run(model=a.model, group_lanes=lanes)
                T, scale, info, stats, inl, dist = al.results()
                runs.append(al.last_kernel_ms())
            ms = {k: float(np.median([r[k] for r in runs[1:]])) for k in ch.ALIGN_STAGES}
            ok = info[:, 2] == ch.ALIGN_OK
            row = {"hypotheses": H, "lanes": lanes, "stage_ms": ms, "total_ms": sum(ms.values()), "problems_ok": int(ok.sum()),
                   "inlier_fraction": float(inl.mean()), "flags_are_the_clean_rows": bool(np.array_equal(inl, ~bad)),
                   "median_rms_m": float(np.median(stats[ok, 0])) if ok.any() else None,
                   "largest_rotation_error": float(np.max(np.abs(T[ok, :, :3] - R_true[ok]))) if ok.any() else None}
            out.append(row)
            print(f"H = {H:3d}, {lanes} lanes: " + "  ".join(f"{k} {v:8.3f} ms" for k, v in ms.items()) + f"  | total {row['total_ms']:8.3f} ms, "
                  f"{row['problems_ok']} / {a.images} OK, inliers {row['inlier_fraction']:.3f} (the clean rows: {row['flags_are_the_clean_rows']}), "
                  f"median RMS {row['median_rms_m']:.3e} m, largest |R - R_true| {row['largest_rotation_error']:.2e}")
    al.close()
    if a.json:
        Path(a.json).write_text(json.dumps({"images": a.images, "keys": a.keys, "model": a.model, "runs": out}, indent=1))


if __name__ == "__main__":
    main()
