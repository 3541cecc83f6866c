#!/usr/bin/env python3
"""Times the TSDF integration and the surface-nets extraction (pycamset_amd/volume.py, csrc/ba_tsdf.hpp) on one device at a rig's size:
32 views of 2448 x 2048 float32 depth maps into grids of 256^3 and 512^3 nodes around the scene.

The maps are rendered on the device: a ring of views 3 degrees apart looks at a sphere of radius 0.4 in front of a plane, each pixel's
ray is intersected with both, and a seeded relative noise of 0.2 % is added.  The grid is the cube of side 2 from (-1, -1, -0.6), which
holds the sphere and the part of the plane behind it; trunc is three voxels.

Every row: ``runs`` calls after ``warmup`` calls of the same shape, the volume zeroed before each; per call the handle's own device times
(``last_kernel_ms``: the integration, the count — classification, numbering, quad flags and both scans — and the write); medians with
the smallest and largest run.  Beside the integration stand its ALGORITHMIC bytes — what the rule has to move, not what the caches moved:
per node the sum and weight read and written (12 B with a float32 sum), per (node, view) test one gathered depth (4 B) — and the rate they
give against the streaming-copy rate of DESIGN.md's fusion section.

    python tools/tsdf_bench.py --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

STREAM_COPY_TB_S = 6.29   # DESIGN.md, "Depth-map fusion": what a streaming copy reaches on this part


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

    from pycamset_amd import volume

    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    V, W, H = a.views, a.width, a.height
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
    n, h, radius = np.array([0.05, -0.03, -1.0]) / np.linalg.norm([0.05, -0.03, -1.0]), -0.6, 0.4
    for v in range(V):
        R, t = E[v][:, :3], E[v][:, 3]
        o = -R.T @ t
        rx, ry = (xs - float(K[v, 1])) / float(K[v, 0]), (ys - float(K[v, 3])) / float(K[v, 2])
        m = R @ n   # n . (R^T ray) = (R n) . ray
        z = float(h - n @ o) / (float(m[0]) * rx + float(m[1]) * ry + float(m[2]))
        oc = R @ o   # the sphere about the world origin: |z ray + R o|^2 = radius^2 in the view's frame (R o = -t)
        A, B, Cq = rx * rx + ry * ry + 1.0, rx * float(oc[0]) + ry * float(oc[1]) + float(oc[2]), float(oc @ oc) - radius * radius
        disc = B * B - A * Cq
        zs = (-B - torch.sqrt(disc.clamp_min(0.0))) / A
        z = torch.where((disc > 0) & (zs > 0), torch.minimum(z, zs), z)
        D[v] = (z * (1.0 + 0.002 * torch.randn((H, W), dtype=torch.float64, device=dev, generator=g))).to(torch.float32)
    stream = torch.cuda.current_stream(0).cuda_stream
    rows = []
    for N in a.grids:
        voxel = 2.0 / (N - 1)
        trunc = 3 * voxel
        vol = volume.TsdfVolume(0)
        vol.set_views(W, H, K, E.reshape(V, 12))
        vol.set_grid((-1.0, -1.0, -0.6), voxel, (N, N, N), True)
        t_int, t_cnt, t_wr = [], [], []
        nv = nq = 0
        for r in range(a.warmup + a.runs):
            vol.reset()
            vol.integrate(D.data_ptr(), True, V, trunc, stream=stream)
            nv, nq = vol.extract_count(a.min_weight, stream=stream)
            verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            quads = torch.empty((nq, 4), dtype=torch.int32, device=dev)
            vol.extract_write(verts.data_ptr() if nv else None, True, quads.data_ptr() if nq else None, stream=stream)
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms = vol.last_kernel_ms()
                t_int.append(ms[0]), t_cnt.append(ms[1]), t_wr.append(ms[2])
        s, w = vol.volume()
        observed = int((w.to(torch.int32) >= a.min_weight).sum())   # torch compares no uint16
        nodes, tests = N ** 3, N ** 3 * V
        b_int = nodes * 12 + tests * 4
        med = statistics.median
        row = {"row": f"{N}^3 nodes, {V} x {W}x{H} float32, float32 sum", "grid": N, "voxel": voxel, "trunc": trunc, "nodes": nodes, "node_view_tests": tests,
               "integrate_ms_median": med(t_int), "integrate_ms_min": min(t_int), "integrate_ms_max": max(t_int), "tests_per_s": tests / med(t_int) * 1e3,
               "integrate_algorithmic_bytes": b_int, "integrate_TB_per_s": b_int / med(t_int) / 1e9, "share_of_streaming_copy": b_int / med(t_int) / 1e9 / STREAM_COPY_TB_S,
               "count_ms_median": med(t_cnt), "count_ms_min": min(t_cnt), "count_ms_max": max(t_cnt), "write_ms_median": med(t_wr), "write_ms_min": min(t_wr),
               "write_ms_max": max(t_wr), "min_weight": a.min_weight, "observed_nodes": observed, "vertices": nv, "quads": nq}
        rows.append(row)
        print(f"{row['row']:52s} integrate {row['integrate_ms_median']:8.3f} ms [{min(t_int):.3f} .. {max(t_int):.3f}] = {row['tests_per_s'] / 1e9:.1f} G tests/s, "
              f"{b_int / 1e9:.2f} GB = {row['integrate_TB_per_s']:.3f} TB/s ({100 * row['share_of_streaming_copy']:.1f} % of a streaming copy);  count {row['count_ms_median']:8.3f} ms "
              f"[{min(t_cnt):.3f} .. {max(t_cnt):.3f}];  write {row['write_ms_median']:7.3f} ms [{min(t_wr):.3f} .. {max(t_wr):.3f}];  {nv} vertices, {nq} quads, "
              f"{observed} of {nodes} nodes observed", flush=True)
        del s, w
        vol.close()
    result = {"tool": "tsdf_bench", "views": V, "width": W, "height": H, "step_deg": a.step, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "streaming_copy_TB_per_s": STREAM_COPY_TB_S, "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
