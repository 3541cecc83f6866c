#!/usr/bin/env python3
"""Times the depth-map fusion (pycamset_amd/fusion.py, csrc/ba_fusion.hpp) on one device at a rig's size: 32 views of 2448 x 2048 float32
depth maps with 4 and 8 neighbours per view, without and with the duplicate marking (``unique``).

The maps are rendered on the device: a ring of views 3 degrees apart looks at a plane, each pixel's ray is intersected with it, and a
seeded relative noise of 0.2 % is added, so that the gathers land where they would in use and some neighbours agree and some do not.

Every row: ``runs`` calls after ``warmup`` calls of the same shape; per call the handle's own device times (``last_kernel_ms``: the check
kernel, the duplicate kernel, the whole call with the per-view counts); medians with the smallest and largest run.  Beside each kernel's
time stand the ALGORITHMIC bytes — what the rule has to move, not what the caches moved — and the rate they give:
  check      per pixel the depth (4 B) and the outputs (points 12 B, mask 1 B, count 1 B, support 4 B); per (pixel, neighbour) one depth
             of the neighbour's map (4 B)
  duplicate  per pixel the support word (4 B) and the depth (4 B); per (pixel, neighbour j < i of the list) one support word (4 B)

    python tools/fusion_bench.py --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--neighbours", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--step", type=float, default=3.0, help="degrees between adjacent views of the ring")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from pycamset_amd import fusion

    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    V, W, H = a.views, a.width, a.height
    # the ring: view v at angle step (v - (V - 1) / 2) on a circle of radius 2 about the origin, looking at it; the plane z = 0.6 behind it
    K, E = np.zeros((V, 4)), np.zeros((V, 3, 4))
    for v in range(V):
        ang = np.radians(a.step) * (v - 0.5 * (V - 1))
        c = 2.0 * np.array([np.sin(ang), 0.05 * np.sin(2.3 * v), -np.cos(ang)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        E[v] = np.concatenate([R, (-R @ c)[:, None]], axis=1)
        K[v] = [0.93 * W, 0.5 * (W - 1) + 0.3 * np.sin(v), 0.93 * W, 0.5 * (H - 1) - 0.3 * np.cos(v)]
    g = torch.Generator(device=dev).manual_seed(7)
    D = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    n, h = np.array([0.05, -0.03, -1.0]) / np.linalg.norm([0.05, -0.03, -1.0]), -0.6
    for v in range(V):
        R, t = E[v][:, :3], E[v][:, 3]
        o = -R.T @ t
        m = R @ n   # n . (R^T ray) = (R n) . ray
        den = float(m[0]) * (xs - float(K[v, 1])) / float(K[v, 0]) + float(m[1]) * (ys - float(K[v, 3])) / float(K[v, 2]) + float(m[2])
        z = float(h - n @ o) / den
        D[v] = (z * (1.0 + 0.002 * torch.randn((H, W), dtype=torch.float64, device=dev, generator=g))).to(torch.float32)
    pts = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    count = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    support = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    counts = torch.zeros((V,), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(0).cuda_stream
    f = fusion.DepthFuser(0)
    f.set_views(W, H, K, E.reshape(V, 12))
    npix = V * H * W
    rows = []
    for nn in a.neighbours:
        lists = [[j for k in range(1, V) for j in (i - k, i + k) if 0 <= j < V][:nn] for i in range(V)]
        _, _, start, nbr, *_ = fusion.check_fuse_args(V, W, H, K, E, lists)
        f.set_neighbours(start, nbr)
        pairs = int(start[-1]) * H * W
        lower = sum(1 for i, l in enumerate(lists) for j in l if j < i) * H * W
        for unique in (False, True):
            def call():
                f.run(D.data_ptr(), True, pts.data_ptr(), mask.data_ptr(), px_tol=1.0, rel_tol=0.01, min_views=2, unique=unique, f32=True, d_count=count.data_ptr(),
                      d_support=support.data_ptr(), d_counts=counts.data_ptr(), stream=stream)
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.runs):
                call()
                ms.append(f.last_kernel_ms())
            kept = int(counts.sum())
            check, uniq, total = ([m[k] for m in ms] for k in range(3))
            b_check, b_uniq = npix * (4 + 12 + 1 + 1 + 4) + pairs * 4, npix * 8 + lower * 4
            row = {"row": f"{V} x {W}x{H} float32, {nn} neighbours, unique {'on' if unique else 'off'}", "neighbours": nn, "unique": unique, "kept": kept, "pixels": npix,
                   "pixel_neighbour_pairs": pairs, "check_ms_median": statistics.median(check), "check_ms_min": min(check), "check_ms_max": max(check),
                   "unique_ms_median": statistics.median(uniq), "unique_ms_min": min(uniq), "unique_ms_max": max(uniq), "total_ms_median": statistics.median(total),
                   "check_algorithmic_bytes": b_check, "check_TB_per_s": b_check / statistics.median(check) / 1e9,
                   "unique_algorithmic_bytes": b_uniq if unique else 0, "unique_TB_per_s": b_uniq / statistics.median(uniq) / 1e9 if unique else None}
            rows.append(row)
            print(f"{row['row']:62s} check {row['check_ms_median']:8.3f} ms [{min(check):.3f} .. {max(check):.3f}] {b_check / 1e9:6.2f} GB = {row['check_TB_per_s']:.3f} TB/s"
                  + (f";  duplicate {row['unique_ms_median']:7.3f} ms [{min(uniq):.3f} .. {max(uniq):.3f}] {b_uniq / 1e9:5.2f} GB = {row['unique_TB_per_s']:.3f} TB/s" if unique else "")
                  + f";  call {row['total_ms_median']:8.3f} ms;  kept {kept} of {npix}", flush=True)
    result = {"tool": "fusion_bench", "views": V, "width": W, "height": H, "step_deg": a.step, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
