#!/usr/bin/env python3
"""Times the plane sweep (pycamset_amd/sweep.py, csrc/ba_sweep.hpp) on one device at a rig's size: 1 and 32 reference views of
2448 x 2048, 64 and 192 planes, 4 and 8 neighbours per view, census 5 x 5 with box radius 2 and census 9 x 7 with box radius 0.

The images are rendered on the device: a ring of views ``--step`` degrees apart looks at an analytically textured plane one metre away;
the planes span 0.8 .. 1.2 m.  A row with ONE reference view is a rig of (neighbours + 1) views of which only the middle one has a
neighbour list: the others leave the kernel without a sample.

Every row: ``runs`` calls after ``warmup`` calls of the same shape; per call the handle's own device time of the kernel
(``last_kernel_ms``, a pair of events around the launch); the median with the smallest and largest run.  Beside it stand the (pixel,
plane, neighbour) triples of the call — pixels of the views that have a list x planes x list length — and their rate, the share of
the staged samples that are halo (the tile is 32 x 32 and is staged with box radius + census radius on every side), and the FP64
operations of the warp per staged sample (18 multiply / add and 2 divisions) as a rate.

    python tools/sweep_bench.py --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

TILE = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--planes", type=int, nargs="+", default=[64, 192])
    ap.add_argument("--neighbours", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--settings", nargs="+", default=["5x5+2", "9x7+0"], help="census width x height + box radius")
    ap.add_argument("--step", type=float, default=3.0, help="degrees between adjacent views of the ring")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from pycamset_amd import sweep

    if not torch.cuda.is_available():
        raise SystemExit("sweep_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    Vmax = max(max(a.views), max(a.neighbours) + 1)
    K, E = np.zeros((Vmax, 4)), np.zeros((Vmax, 3, 4))
    images = torch.empty((Vmax, H, W), dtype=torch.uint8, device=dev)
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    for v in range(Vmax):   # view v on a circle of radius 1 about (0, 0, 1), looking at it; the plane Z = 1 carries the texture
        ang = np.radians(a.step) * (v - 0.5 * (Vmax - 1))
        c = np.array([np.sin(ang), 0.004 * np.sin(2.0 * v), 1.0 - np.cos(ang)])
        fwd = (np.array([0.0, 0.0, 1.0]) - c) / np.linalg.norm(np.array([0.0, 0.0, 1.0]) - c)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        E[v] = np.concatenate([R, (-R @ c)[:, None]], axis=1)
        K[v] = [1.2 * W, 0.5 * (W - 1) + 0.3 * np.sin(v), 1.2 * W, 0.5 * (H - 1) - 0.3 * np.cos(v)]
        rx, ry = (xs - float(K[v, 1])) / float(K[v, 0]), (ys - float(K[v, 3])) / float(K[v, 2])
        d = [float(R[0, k]) * rx + float(R[1, k]) * ry + float(R[2, k]) for k in range(3)]   # R^T ray
        s = (1.0 - float(c[2])) / d[2]
        X, Y = float(c[0]) + s * d[0], float(c[1]) + s * d[1]
        tex = (127.5 + 45.0 * torch.sin(61.0 * X + 2.0 * torch.sin(23.0 * Y)) + 40.0 * torch.sin(47.0 * Y + 13.0 * X * X)
               + 35.0 * torch.sin(29.0 * (X + Y) + 5.0 * torch.cos(37.0 * X)))
        images[v] = torch.clamp(torch.round(tex), 0, 255).to(torch.uint8)
    depth = torch.empty((Vmax, H, W), dtype=torch.float32, device=dev)
    status = torch.empty((Vmax, H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(0).cuda_stream
    rows = []
    for nv in a.views:
        for setting in a.settings:
            census, box = setting.split("+")
            cw, ch = (int(t) for t in census.split("x"))
            box = int(box)
            for nn in a.neighbours:
                V = nv if nv > 1 else nn + 1
                lists = [[j for k in range(1, V) for j in (i - k, i + k) if 0 <= j < V][:nn] for i in range(V)]
                if nv == 1:
                    lists = [l if i == V // 2 else [] for i, l in enumerate(lists)]
                h = sweep.PlaneSweeper(0)
                h.set_views(W, H, K[:V], E[:V].reshape(V, 12))
                start = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
                h.set_neighbours(start, np.concatenate([np.asarray(l, dtype=np.int32) for l in lists]))
                for D in a.planes:
                    z = sweep.depth_planes((0.8, 1.2), D)

                    def call():
                        h.run(images.data_ptr(), W, z, depth.data_ptr(), census=(cw, ch), box=box, f32=True, d_status=status.data_ptr(), stream=stream)
                    for _ in range(a.warmup):
                        call()
                    torch.cuda.synchronize()
                    ms = []
                    for _ in range(a.runs):
                        call()
                        ms.append(h.last_kernel_ms())
                    med = statistics.median(ms)
                    with_list = [i for i, l in enumerate(lists) if l]
                    kept = int((status[with_list] == 0).sum())
                    triples = int(start[-1]) * H * W * D
                    staged = (TILE + 2 * (box + cw // 2)) * (TILE + 2 * (box + ch // 2))
                    halo = 1.0 - TILE * TILE / staged
                    flop = triples * (staged / (TILE * TILE)) * 20
                    row = {"row": f"{nv} view(s) of {W}x{H}, census {cw}x{ch}, box {box}, {nn} neighbours, {D} planes", "reference_views": len(with_list), "neighbours": nn,
                           "planes": D, "census": [cw, ch], "box": box, "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "triples": triples,
                           "triples_per_s": triples / med * 1e3, "halo_share_of_staged_samples": halo, "warp_fp64_ops_per_s": flop / med * 1e3,
                           "kept": kept, "pixels": len(with_list) * H * W}
                    rows.append(row)
                    print(f"{row['row']:78s} kernel {med:10.2f} ms [{min(ms):.2f} .. {max(ms):.2f}]  {triples:.3e} triples = {row['triples_per_s']:.3e} / s;  halo {100 * halo:.0f} % of the "
                          f"staged samples;  warp {row['warp_fp64_ops_per_s'] / 1e12:.2f} T FP64 op/s;  kept {kept} of {row['pixels']}", flush=True)
                h.close()
    result = {"tool": "sweep_bench", "width": W, "height": H, "step_deg": a.step, "runs": a.runs, "warmup": a.warmup, "tile": [TILE, TILE],
              "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
