#!/usr/bin/env python3
"""Times the ray-cast of the TSDF volume (pycamset_amd/volume.py, csrc/ba_tsdf_raycast.hpp) on one device at a rig's size: the scene of
tools/tsdf_bench.py — 32 views of 2448 x 2048 float32 depth maps integrated into grids of 256^3 and 512^3 nodes — cast back into its own
views at 2448 x 2048, float32 depth, step = one voxel.

Every row: ``runs`` calls after ``warmup`` calls of the same shape; per call the handle's own device times (``raycast_last_kernel_ms``:
the mask pass — memset and mask kernel — and the cast kernel); medians with the smallest and largest run.  Rows: one view and all
views, with the normals and without, with the empty-space mask and with PCS_TSDF_RAYCAST_NO_SKIP.  Beside the times stand rays / s and
evaluated samples / s over the cast kernel's time.  The samples are counted by a SEPARATE launch (``raycast_count_samples``: the last
cast over again, writing a count per pixel); the timed cast counts nothing.  Every row also checks that skipping changed no bit of any
output.

    python tools/raycast_bench.py --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def scene(V, W, H, step_deg, dev):
    """The ring, the sphere in front of a plane and the noise of tools/tsdf_bench.py: -> (K, E, depth (V, H, W) float32 on the device)."""
    import numpy as np
    import torch

    K, E = np.zeros((V, 4)), np.zeros((V, 3, 4))
    for v in range(V):
        ang = np.radians(step_deg) * (v - 0.5 * (V - 1))
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
        m = R @ n
        z = float(h - n @ o) / (float(m[0]) * rx + float(m[1]) * ry + float(m[2]))
        oc = R @ o
        A, B, Cq = rx * rx + ry * ry + 1.0, rx * float(oc[0]) + ry * float(oc[1]) + float(oc[2]), float(oc @ oc) - radius * radius
        disc = B * B - A * Cq
        zs = (-B - torch.sqrt(disc.clamp_min(0.0))) / A
        z = torch.where((disc > 0) & (zs > 0), torch.minimum(z, zs), z)
        D[v] = (z * (1.0 + 0.002 * torch.randn((H, W), dtype=torch.float64, device=dev, generator=g))).to(torch.float32)
    return K, E, D


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
        raise SystemExit("raycast_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    V, W, H = a.views, a.width, a.height
    K, E, D = scene(V, W, H, a.step, dev)
    P = E.reshape(V, 12)
    stream = torch.cuda.current_stream(0).cuda_stream
    med = statistics.median
    rows = []
    for N in a.grids:
        voxel = 2.0 / (N - 1)
        vol = volume.TsdfVolume(0)
        vol.set_views(W, H, K, P)
        vol.set_grid((-1.0, -1.0, -0.6), voxel, (N, N, N), True)
        vol.integrate(D.data_ptr(), True, V, 3 * voxel, stream=stream)
        torch.cuda.synchronize()
        for nv in (1, V):
            depth = torch.empty((nv, H, W), dtype=torch.float32, device=dev)
            normal = torch.empty((nv, H, W, 3), dtype=torch.float32, device=dev)
            status = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            samples = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
            for with_normals in (True, False):
                kept = {}
                for skip in (True, False):
                    t_mask, t_cast = [], []
                    for r in range(a.warmup + a.runs):
                        vol.raycast(W, H, K[:nv], P[:nv], a.min_weight, voxel, 0.0, np.inf, depth.data_ptr(), True, normal.data_ptr() if with_normals else None, status.data_ptr(),
                                    skip=skip, stream=stream)
                        torch.cuda.synchronize()
                        if r >= a.warmup:
                            ms = vol.raycast_last_kernel_ms()
                            t_mask.append(ms[0] if skip else 0.0), t_cast.append(ms[1])
                    vol.raycast_count_samples(samples.data_ptr(), stream=stream)
                    torch.cuda.synchronize()
                    n_samples, rays = int(samples.sum(dtype=torch.int64)), nv * H * W
                    kept[skip] = (depth.clone(), normal.clone() if with_normals else None, status.clone())
                    hits = int((status <= 1).sum())
                    row = {"row": f"{N}^3 nodes, {nv} x {W}x{H}, normals {'yes' if with_normals else 'no'}, {'mask' if skip else 'NO_SKIP'}", "grid": N, "voxel": voxel, "views": nv,
                           "normals": with_normals, "skip": skip, "mask_ms_median": med(t_mask), "mask_ms_min": min(t_mask), "mask_ms_max": max(t_mask), "cast_ms_median": med(t_cast),
                           "cast_ms_min": min(t_cast), "cast_ms_max": max(t_cast), "total_ms_median": med([m + c for m, c in zip(t_mask, t_cast)]), "rays": rays, "hits": hits,
                           "samples_evaluated": n_samples, "rays_per_s": rays / med(t_cast) * 1e3, "samples_per_s": n_samples / med(t_cast) * 1e3}
                    rows.append(row)
                    print(f"{row['row']:62s} mask {row['mask_ms_median']:7.3f} ms [{min(t_mask):.3f} .. {max(t_mask):.3f}]  cast {row['cast_ms_median']:9.3f} ms [{min(t_cast):.3f} .. "
                          f"{max(t_cast):.3f}]  {row['rays_per_s'] / 1e9:6.2f} G rays/s, {n_samples / rays:7.1f} samples/ray, {row['samples_per_s'] / 1e9:6.2f} G samples/s, {hits} hits", flush=True)
                same = all(x is None or torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(kept[True], kept[False]))
                rows[-1]["identical_to_mask_row"] = rows[-2]["identical_to_no_skip_row"] = same
                if not same:
                    raise SystemExit("skipping changed a bit of an output")
        vol.close()
    result = {"tool": "raycast_bench", "views": V, "width": W, "height": H, "step_deg": a.step, "min_weight": a.min_weight, "runs": a.runs, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
