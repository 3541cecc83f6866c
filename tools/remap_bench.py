#!/usr/bin/env python3
"""Times the image mapper (pycamset_amd/imaging.py, csrc/ba_imagemap.hpp) on one device at a rig's size: ray maps, map build, the fused
remap, the mapped remap with and without its map build, against two comparators that are not the code under test: a device-to-device
copy of the same source + destination bytes (the floor) and torch's grid_sample on a precomputed grid.

Every row: `reps` back-to-back launches between two device events, after a warm-up of the same shape, repeated `runs` times; the
median per-launch time with the smallest and largest run, and the bytes the algorithm must move (source read once, destination written
once, plus 8 B of float32 map per pixel where a map is read or written) over that time.

    python tools/remap_bench.py --cams 32 --width 2448 --height 2048 --out result.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def rig(n, W, H, seed=1):
    rng = np.random.default_rng(seed)
    f = 0.9 * W * rng.uniform(0.95, 1.05, size=(n, 1))
    return np.concatenate([f, W / 2 + rng.uniform(-20, 20, (n, 1)), f * rng.uniform(0.99, 1.01, (n, 1)), H / 2 + rng.uniform(-20, 20, (n, 1)),
                           rng.uniform(-0.15, -0.05, (n, 1)), rng.uniform(0.0, 0.05, (n, 1)), rng.uniform(-1e-3, 1e-3, (n, 2)), rng.uniform(-0.01, 0.01, (n, 1))], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from pycamset_amd import imaging

    if not torch.cuda.is_available():
        raise SystemExit("remap_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    n, W, H = a.cams, a.width, a.height
    m = imaging.ImageMapper(0)
    m.set_cameras(rig(n, W, H))
    stream = torch.cuda.current_stream(0).cuda_stream
    cams = list(range(n))
    rows = []

    def timed(name, fn, bytes_moved, note=""):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        med = statistics.median(ms)
        row = {"row": name, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes": int(bytes_moved), "GBps": bytes_moved / med / 1e6, "note": note}
        rows.append(row)
        print(f"{name:46s} {med:9.4f} ms  [{min(ms):.4f} .. {max(ms):.4f}]  {row['GBps']:9.1f} GB/s of {bytes_moved / 1e6:9.1f} MB  {note}", flush=True)

    plane = W * H
    # ray maps and the map build: one camera per launch
    for dt, size in ((torch.float32, 4), (torch.float64, 8)):
        out = torch.empty((H, W, 3), dtype=dt, device=dev)
        timed(f"ray map {str(dt)[6:]} (1 camera)", lambda: m.rays(0, W, H, out.data_ptr(), out_f32=dt == torch.float32, stream=stream), plane * 3 * size)
    maps = torch.empty((n, 2, H, W), dtype=torch.float32, device=dev)

    def build_all():
        for c in range(n):
            m.build_maps(c, W, H, maps[c].data_ptr(), out_f32=True, stream=stream)

    timed(f"map build float32 ({n} cameras)", build_all, n * plane * 8)
    for name, tdt, C, item in (("uint8 mono", torch.uint8, 1, 1), ("float32 RGB", torch.float32, 3, 4)):
        g = torch.Generator(device=dev).manual_seed(5)
        if tdt == torch.uint8:
            src = torch.randint(0, 256, (n, H, W, C), dtype=tdt, device=dev, generator=g)
        else:
            src = torch.rand((n, H, W, C), dtype=tdt, device=dev, generator=g)
        dst = torch.empty_like(src)
        pitch = W * C * item
        img_bytes = 2 * n * plane * C * item
        dname = "uint8" if tdt == torch.uint8 else "float32"

        def remap(interp, mapped):
            kw = dict(d_map=maps.data_ptr(), map_f32=True, n_maps=n) if mapped else {}
            m.remap(cams, src.data_ptr(), (W, H), C, dname, pitch, dst.data_ptr(), (W, H), pitch, interpolation=interp, stream=stream, **kw)

        timed(f"{name}: device-to-device copy (floor)", lambda: dst.copy_(src), img_bytes)
        for interp in ("bilinear", "bicubic"):
            timed(f"{name}: fused {interp}", lambda: remap(interp, False), img_bytes)
            timed(f"{name}: mapped {interp}, map resident", lambda: remap(interp, True), img_bytes + n * plane * 8)
            timed(f"{name}: mapped {interp} + map build", lambda: (build_all(), remap(interp, True)), img_bytes + 2 * n * plane * 8)
        # torch's sampler on a precomputed normalised grid (float input; for the 8-bit workload its float32 twin: grid_sample takes no uint8)
        fsrc = src.permute(0, 3, 1, 2).float().contiguous()
        grid = torch.stack([2.0 * maps[:, 0] / (W - 1) - 1.0, 2.0 * maps[:, 1] / (H - 1) - 1.0], dim=-1).contiguous()
        for interp in ("bilinear", "bicubic"):
            timed(f"{name}: grid_sample {interp} (float32 NCHW)", lambda: torch.nn.functional.grid_sample(fsrc, grid, mode=interp, padding_mode="zeros", align_corners=True),
                  2 * n * plane * C * 4 + n * plane * 8, "comparator")
        del fsrc, grid, src, dst
    result = {"tool": "remap_bench", "cams": n, "width": W, "height": H, "reps": a.reps, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
