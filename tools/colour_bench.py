#!/usr/bin/env python3
"""Times the colour stage (pycamset_amd/volume.py, csrc/ba_tsdf_colour.hpp) on one device at a rig's size: the scene of tools/tsdf_bench.py
— 32 views of 2448 x 2048 float32 depth maps integrated into grids of 256^3 and 512^3 nodes (``tools/raycast_bench.scene``) — with a
synthetic uint8 x 3 image per view.

Per grid: the mesh is extracted, its vertices get normals (``point_normals``) and are coloured from 1 and from 32 views, with and
without the visibility maps and the normals; then ``colour_views`` renders one view of 2448 x 2048 in colour from all source views.
The visibility maps are the model's own depth in the source views: that ray-cast is timed on its own (mask pass + cast kernel) and is
NOT part of the colour kernel's time.  Every row: ``runs`` calls after ``warmup`` calls of the same shape, the handle's own device times
(``colour_last_kernel_ms``, ``raycast_last_kernel_ms``); medians with the smallest and largest run.

    python tools/colour_bench.py --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--step", type=float, default=3.0, help="degrees between adjacent views of the ring")
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from raycast_bench import scene

    from pycamset_amd import volume

    if not torch.cuda.is_available():
        raise SystemExit("colour_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    V, W, H = a.views, a.width, a.height
    K, E, D = scene(V, W, H, a.step, dev)
    P = E.reshape(V, 12)
    g = torch.Generator(device=dev).manual_seed(11)
    images = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    stream = torch.cuda.current_stream(0).cuda_stream
    med = statistics.median
    rows = []

    def timed(call, read):
        t = []
        for r in range(a.warmup + a.runs):
            call()
            torch.cuda.synchronize()
            if r >= a.warmup:
                t.append(read())
        return t

    def add(row, t, n, unit):
        row.update(ms_median=med(t), ms_min=min(t), ms_max=max(t), items=n, items_per_s=n / med(t) * 1e3)
        rows.append(row)
        print(f"{row['row']:78s} {row['ms_median']:9.3f} ms [{min(t):.3f} .. {max(t):.3f}]  {row['items_per_s'] / 1e9:7.3f} G {unit}/s", flush=True)

    for N in a.grids:
        voxel = 2.0 / (N - 1)
        tol = float(np.sqrt(3.0) * voxel)
        vol = volume.TsdfVolume(0)
        vol.set_views(W, H, K, P)
        vol.set_grid((-1.0, -1.0, -0.6), voxel, (N, N, N), True)
        vol.integrate(D.data_ptr(), True, V, 3 * voxel, stream=stream)
        nv, nq = vol.extract_count(a.min_weight, stream=stream)
        verts, quads = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nq, 4), dtype=torch.int32, device=dev)
        vol.extract_write(verts.data_ptr(), True, quads.data_ptr(), stream=stream)
        del quads
        normals, nstat = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nv,), dtype=torch.uint8, device=dev)
        t = timed(lambda: vol.point_normals(nv, verts.data_ptr(), True, a.min_weight, normals.data_ptr(), nstat.data_ptr(), stream=stream), lambda: vol.colour_last_kernel_ms()[0])
        add({"row": f"{N}^3 nodes: point normals of {nv} vertices", "grid": N, "stage": "point_normals", "with_normal": int((nstat == 0).sum())}, t, nv, "vertices")
        model = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        for k in (1, V):   # the visibility ray-cast, on its own
            t = timed(lambda: vol.raycast(W, H, K[:k], P[:k], a.min_weight, voxel, 0.0, np.inf, model.data_ptr(), True, None, None, stream=stream), lambda: sum(vol.raycast_last_kernel_ms()))
            add({"row": f"{N}^3 nodes: visibility ray-cast of {k} x {W}x{H} (mask + cast, no normals)", "grid": N, "stage": "visibility_raycast", "views": k}, t, k * H * W, "rays")
        colour = torch.empty((nv, 3), dtype=torch.uint8, device=dev)
        weight, count, best = torch.empty((nv,), dtype=torch.float32, device=dev), torch.empty((nv,), dtype=torch.uint16, device=dev), torch.empty((nv,), dtype=torch.int32, device=dev)
        src = dict(volume.check_colour_args(images, K, E, occlusion_tol=tol), d_images=images.data_ptr(), pitch=W * 3, d_colour=colour.data_ptr(), d_weight=weight.data_ptr(),
                   d_count=count.data_ptr(), d_best=best.data_ptr())
        for k in (1, V):
            for vis in (True, False):
                for nrm in (True, False):
                    s = dict(src, K=src["K"][:k], P=src["P"][:k], d_visibility=model.data_ptr() if vis else None, visibility_f32=True)
                    t = timed(lambda: vol.colour_points(nv, verts.data_ptr(), True, normals.data_ptr() if nrm else None, s, stream=stream), lambda: vol.colour_last_kernel_ms()[1])
                    add({"row": f"{N}^3 nodes: colour {nv} vertices from {k} view(s), visibility {'yes' if vis else 'no'}, normals {'yes' if nrm else 'no'}", "grid": N,
                         "stage": "colour_points", "views": k, "visibility": vis, "normals": nrm, "coloured": int((count.to(torch.int32) > 0).sum()),
                         "pairs_contributing": int(count.to(torch.int64).sum())}, t, nv * k, "(vertex, view) pairs")
        del colour, weight, count, best
        depth, nmap = torch.empty((1, H, W), dtype=torch.float32, device=dev), torch.empty((1, H, W, 3), dtype=torch.float32, device=dev)
        vol.raycast(W, H, K[V // 2:V // 2 + 1], P[V // 2:V // 2 + 1], a.min_weight, voxel, 0.0, np.inf, depth.data_ptr(), True, nmap.data_ptr(), None, stream=stream)
        vol.raycast(W, H, K, P, a.min_weight, voxel, 0.0, np.inf, model.data_ptr(), True, None, None, stream=stream)
        image, vcount = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((1, H, W), dtype=torch.uint16, device=dev)
        s = dict(src, d_visibility=model.data_ptr(), visibility_f32=True, d_colour=image.data_ptr(), d_weight=None, d_count=vcount.data_ptr(), d_best=None)
        t = timed(lambda: vol.colour_views(W, H, K[V // 2:V // 2 + 1], P[V // 2:V // 2 + 1], depth.data_ptr(), True, nmap.data_ptr(), s, stream=stream), lambda: vol.colour_last_kernel_ms()[1])
        add({"row": f"{N}^3 nodes: colour_views 1 x {W}x{H} from {V} views, visibility yes, normals yes", "grid": N, "stage": "colour_views", "views": V,
             "coloured": int((vcount.to(torch.int32) > 0).sum()), "pairs_contributing": int(vcount.to(torch.int64).sum())}, t, H * W * V, "(pixel, view) pairs")
        vol.close()
        del verts, normals, nstat, model, depth, nmap, image, vcount
    result = {"tool": "colour_bench", "views": V, "width": W, "height": H, "step_deg": a.step, "min_weight": a.min_weight, "runs": a.runs, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
