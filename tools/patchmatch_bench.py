#!/usr/bin/env python3
"""Times the PatchMatch depth (pycamset_amd/patchmatch.py, csrc/ba_patchmatch.hpp) on one device at a rig's size: 1 and 32 reference
views of 2448 x 2048, 4 and 8 neighbours per view, census 7 x 7 at stride 2 and census 5 x 5 at stride 1.

The scene is that of tools/sweep_bench.py, rendered on the device: a ring of views ``--step`` degrees apart looks at an analytically
textured plane one metre away; the search spans 0.8 .. 1.2 m.  The start is the true depth of the plane, flat (what a sweep hands over).
A row with ONE reference view is a rig of (neighbours + 1) views of which only the middle one has a neighbour list: the pixels of the
others leave the kernels at once.

Every row: ``runs`` calls after ``warmup`` calls of the same shape, a call being initialise, ``--iterations`` iterations, finish; per
call the handle's own device time of the iterations (``last_kernel_ms``, a pair of events around the 2 x iterations launches) and of
the initialisation; the median with the smallest and largest run.  Beside it stand the nominal (pixel, candidate, neighbour, sample)
evaluations of an iteration — strict pixels of the views that have a list x 12 candidates x list length x cw ch window positions; a
candidate that is inadmissible, whose source is not strict, or whose window meets an invalid sample costs less — and their rate.

    python tools/patchmatch_bench.py --out result.json
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
    ap.add_argument("--views", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--neighbours", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--settings", nargs="+", default=["7x7s2", "5x5s1"], help="census width x height s stride")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--step", type=float, default=3.0, help="degrees between adjacent views of the ring")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from pycamset_amd import patchmatch

    if not torch.cuda.is_available():
        raise SystemExit("patchmatch_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    Vmax = max(max(a.views), max(a.neighbours) + 1)
    K, E = np.zeros((Vmax, 4)), np.zeros((Vmax, 3, 4))
    images = torch.empty((Vmax, H, W), dtype=torch.uint8, device=dev)
    start_depth = torch.empty((Vmax, H, W), dtype=torch.float32, device=dev)
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
        s = (1.0 - float(c[2])) / d[2]   # the ray has z = 1 in the view's frame: s is the z-depth
        X, Y = float(c[0]) + s * d[0], float(c[1]) + s * d[1]
        tex = (127.5 + 45.0 * torch.sin(61.0 * X + 2.0 * torch.sin(23.0 * Y)) + 40.0 * torch.sin(47.0 * Y + 13.0 * X * X)
               + 35.0 * torch.sin(29.0 * (X + Y) + 5.0 * torch.cos(37.0 * X)))
        images[v] = torch.clamp(torch.round(tex), 0, 255).to(torch.uint8)
        start_depth[v] = s.to(torch.float32)
    plane = torch.empty((Vmax, H, W, 3), dtype=torch.float64, device=dev)
    cost = torch.empty((Vmax, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((Vmax, H, W), dtype=torch.float32, device=dev)
    status = torch.empty((Vmax, H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(0).cuda_stream
    wrange = np.array([[1 / 1.2, 1 / 0.8]])
    rows = []
    for nv in a.views:
        for setting in a.settings:
            census, stride = setting.split("s")
            cw, ch = (int(t) for t in census.split("x"))
            stride = int(stride)
            for nn in a.neighbours:
                V = nv if nv > 1 else nn + 1
                lists = [[j for k in range(1, V) for j in (i - k, i + k) if 0 <= j < V][:nn] for i in range(V)]
                if nv == 1:
                    lists = [l if i == V // 2 else [] for i, l in enumerate(lists)]
                h = patchmatch.PatchMatcher(0)
                h.set_views(W, H, K[:V], E[:V].reshape(V, 12))
                start = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
                h.set_neighbours(start, np.concatenate([np.asarray(l, dtype=np.int32) for l in lists]))
                slope = np.tan(np.radians(70.0)) / np.minimum(K[:V, 0], K[:V, 2])
                kw = dict(census=(cw, ch), stride=stride, stream=stream)
                ms_init, ms_iter = [], []
                for run in range(a.warmup + a.runs):
                    h.init(images.data_ptr(), W, wrange, slope, plane.data_ptr(), cost.data_ptr(), d_start_depth=start_depth.data_ptr(), start_f32=True, **kw)
                    t_init = h.last_kernel_ms()
                    h.iterate(0, a.iterations, images.data_ptr(), W, wrange, slope, plane.data_ptr(), cost.data_ptr(), **kw)
                    t_iter = h.last_kernel_ms()
                    h.finish(plane.data_ptr(), cost.data_ptr(), depth.data_ptr(), f32=True, d_status=status.data_ptr(), **kw)
                    if run >= a.warmup:
                        ms_init.append(t_init), ms_iter.append(t_iter)
                with_list = [i for i, l in enumerate(lists) if l]
                kept = int((status[with_list] == 0).sum())
                strict = max(0, W - 2 * (cw // 2) * stride) * max(0, H - 2 * (ch // 2) * stride)
                evals = int(start[-1]) * strict * 12 * cw * ch
                med = statistics.median(ms_iter)
                row = {"row": f"{nv} view(s) of {W}x{H}, census {cw}x{ch}, stride {stride}, {nn} neighbours", "reference_views": len(with_list), "neighbours": nn,
                       "census": [cw, ch], "stride": stride, "iterations": a.iterations, "iterate_ms_median": med, "iterate_ms_min": min(ms_iter), "iterate_ms_max": max(ms_iter),
                       "ms_per_iteration": med / max(1, a.iterations), "init_ms_median": statistics.median(ms_init), "evaluations_per_iteration": evals,
                       "evaluations_per_s": evals * a.iterations / med * 1e3 if med > 0 else 0.0, "kept": kept, "strict_pixels": len(with_list) * strict}
                rows.append(row)
                print(f"{row['row']:72s} {a.iterations} iterations {med:10.2f} ms [{min(ms_iter):.2f} .. {max(ms_iter):.2f}] = {row['ms_per_iteration']:.2f} ms each;  init "
                      f"{row['init_ms_median']:.2f} ms;  {evals:.3e} nominal evaluations per iteration = {row['evaluations_per_s']:.3e} / s;  kept {kept} of {row['strict_pixels']}",
                      flush=True)
                h.close()
    result = {"tool": "patchmatch_bench", "width": W, "height": H, "step_deg": a.step, "runs": a.runs, "warmup": a.warmup, "tile": [32, 16],
              "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
