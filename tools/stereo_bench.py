#!/usr/bin/env python3
"""Times the stereo matcher (pycamset_amd/stereo.py, csrc/ba_stereo.hpp) on one device at a rig's size: one and sixteen 2448 x 2048 pairs,
256 and 64 disparities, blocks 5, 15 and 25, with and without the left-right pass; then the reprojection and the compaction.  With --sgm:
semi-global matching (csrc/ba_stereo_sgm.hpp) at 64, 128 and 256 disparities and 4 and 8 paths, stage by stage, with the traffic of the
aggregated volume against the time of the path kernels.

Every row: `reps` back-to-back calls between two device events after a warm-up of the same shape, repeated `runs` times; the median
per-call time with the smallest and largest run, and the (pixel, disparity) window costs per second, counting the strict pixels times
the disparities (twice that with the left-right pass, whose second sweep is anchored in the right image).

    python tools/stereo_bench.py --out result.json
    python tools/stereo_bench.py --sgm --blocks 15 --out sgm.json
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
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--width", type=int, default=2448)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--disparities", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--blocks", type=int, nargs="+", default=[5, 15, 25])
    ap.add_argument("--tile-columns", type=int, nargs="+", default=[0], help="PCS_STEREO_TILE_COLUMNS per row; 0: the library's own choice")
    ap.add_argument("--strip-rows", type=int, nargs="+", default=[0], help="PCS_STEREO_STRIP_ROWS per row; 0: the library's own choice")
    ap.add_argument("--no-cloud", action="store_true", help="skip the reprojection and compaction rows")
    ap.add_argument("--sgm", action="store_true", help="time semi-global matching stage by stage instead, next to the block matcher at the first of --blocks")
    ap.add_argument("--sgm-disparities", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--paths", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--census", type=int, nargs=2, default=[9, 7], help="census window, width height")
    ap.add_argument("--p1", type=int, default=8)
    ap.add_argument("--p2", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import os

    import torch

    from pycamset_amd import stereo

    if not torch.cuda.is_available():
        raise SystemExit("stereo_bench needs the device: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    m = stereo.StereoMatcher(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    rows = []

    def timed(name, fn, work, unit, note=""):
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
        row = {"row": name, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "work": int(work), "unit": unit, "G_per_s": work / med / 1e6, "note": note}
        rows.append(row)
        print(f"{name:58s} {med:10.3f} ms  [{min(ms):.3f} .. {max(ms):.3f}]  {row['G_per_s']:8.2f} G {unit}/s", flush=True)

    def sgm_rows(n, left, right, disp):
        """--sgm: per (D, paths) the call cut off after the census, after the paths, complete without and with the left-right check
        (PCS_SGM_LAST_STAGE); the stage times are the differences of the medians.  Traffic model of the paths: every direction reads and
        writes S on the strict rectangle, 2 Hs Ws Dpad bytes each way, and the first one only writes."""
        for D in a.sgm_disparities:
            rw, rh = a.census[0] // 2, a.census[1] // 2
            Ws, Hs, Dpad = max(W - 2 * rw - (D - 1), 0), max(H - 2 * rh, 0), (D + 3) & ~3
            for block in a.blocks[:1]:
                for lr in (-1, 1):
                    timed(f"block match {n:2d} x {W}x{H}  D={D:3d} block={block:2d} {'left-right' if lr >= 0 else 'one pass  '}",
                          lambda: m.match(n, W, H, left.data_ptr(), W, right.data_ptr(), W, disp.data_ptr(), num_disp=D, block=block, lr_max_diff=lr, stream=stream),
                          max(W - 2 * (block // 2) - (D - 1), 0) * max(H - 2 * (block // 2), 0) * n * D * (2 if lr >= 0 else 1), "(pixel, disparity)")
            for paths in a.paths:
                med = {}
                for stage, lr, name in ((1, -1, "census"), (2, -1, "census + paths"), (4, -1, "complete, one pass"), (4, 1, "complete, left-right")):
                    os.environ["PCS_SGM_LAST_STAGE"] = str(stage)
                    timed(f"sgm {n:2d} x {W}x{H}  D={D:3d} paths={paths} {name}",
                          lambda: m.match_sgm(n, W, H, left.data_ptr(), W, right.data_ptr(), W, disp.data_ptr(), num_disp=D, census=tuple(a.census), p1=a.p1, p2=a.p2, paths=paths,
                                              lr_max_diff=lr, stream=stream), Ws * Hs * n * D * paths, "(pixel, disparity, path)")
                    med[(stage, lr)] = rows[-1]["ms_median"]
                os.environ.pop("PCS_SGM_LAST_STAGE", None)
                t_paths = med[(2, -1)] - med[(1, -1)]
                s_bytes = (2 * paths - 1) * 2 * Hs * Ws * Dpad * n
                stages = {"census_ms": med[(1, -1)], "paths_ms": t_paths, "select_ms": med[(4, -1)] - med[(2, -1)], "right_ms": med[(4, 1)] - med[(4, -1)],
                          "complete_one_pass_ms": med[(4, -1)], "complete_left_right_ms": med[(4, 1)], "S_bytes_moved": s_bytes,
                          "S_TB_per_s": s_bytes / t_paths / 1e9 if t_paths > 0 else None, "share_of_8_TB_per_s": s_bytes / t_paths / 1e9 / 8.0 if t_paths > 0 else None}
                rows.append({"row": f"sgm stages {n} pairs D={D} paths={paths}", **stages})
                print(f"    stages: census {stages['census_ms']:.3f}  paths {t_paths:.3f} ({t_paths / paths:.3f} per direction)  select {stages['select_ms']:.3f}  "
                      f"right {stages['right_ms']:.3f} ms;  S traffic {s_bytes / 1e9:.2f} GB at {stages['S_TB_per_s']:.3f} TB/s = {100 * stages['share_of_8_TB_per_s']:.1f} % of 8 TB/s",
                      flush=True)

    for n in a.pairs:
        g = torch.Generator(device=dev).manual_seed(5)
        # smoothed noise; the right image is the left one shifted by 20 px, with its own noise
        base = torch.rand((n, H, W + 32), device=dev, generator=g)
        base = (base + base.roll(1, 2) + base.roll(1, 1) + base.roll(-1, 2)) / 4.0
        left = (base[:, :, 32:] * 255).to(torch.uint8).contiguous()
        right = ((base[:, :, 12:W + 12] + 0.02 * torch.rand((n, H, W), device=dev, generator=g)).clamp(0, 1) * 255).to(torch.uint8).contiguous()
        disp = torch.empty((n, H, W), dtype=torch.int16, device=dev)
        if a.sgm:
            sgm_rows(n, left, right, disp)
            continue
        for D in a.disparities:
            for block in a.blocks:
                for lr in (-1, 1):
                    for tw, sh in ((t, s) for t in a.tile_columns for s in a.strip_rows):
                        for key, v in (("PCS_STEREO_TILE_COLUMNS", tw), ("PCS_STEREO_STRIP_ROWS", sh)):
                            os.environ.pop(key, None)
                            if v > 0:
                                os.environ[key] = str(v)
                        r = block // 2
                        strict = max(W - 2 * r - (D - 1), 0) * max(H - 2 * r, 0) * n
                        work = strict * D * (2 if lr >= 0 else 1)
                        timed(f"match {n:2d} x {W}x{H}  D={D:3d} block={block:2d} {'left-right' if lr >= 0 else 'one pass  '}" + (f" tile {tw}" if tw else "") + (f" strip {sh}" if sh else ""),
                              lambda: m.match(n, W, H, left.data_ptr(), W, right.data_ptr(), W, disp.data_ptr(), num_disp=D, block=block, lr_max_diff=lr, stream=stream),
                              work, "(pixel, disparity)")
        os.environ.pop("PCS_STEREO_TILE_COLUMNS", None)
        os.environ.pop("PCS_STEREO_STRIP_ROWS", None)
        if a.no_cloud:
            continue
        import numpy as np

        Q = np.array([[1.0, 0, 0, -W / 2], [0, 1.0, 0, -H / 2], [0, 0, 0, 2200.0], [0, 0, 1 / 0.12, 0]])
        for f32 in (True, False):
            pts = torch.empty((n, H, W, 3), dtype=torch.float32 if f32 else torch.float64, device=dev)
            out = torch.empty_like(pts)
            mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            vals = torch.empty((n * H * W,), dtype=torch.uint8, device=dev)
            counts = torch.zeros((n,), dtype=torch.int64, device=dev)
            name = "float32" if f32 else "float64"
            timed(f"reproject {n:2d} pairs to {name}, with counts", lambda: m.reproject(n, W, H, disp.data_ptr(), Q, pts.data_ptr(), mask.data_ptr(), invalid=-16,
                                                                                          z_range=(0.0, 50.0), f32=f32, d_counts=counts.data_ptr(), stream=stream), n * H * W, "pixel")
            timed(f"compact {n:2d} pairs of {name} with grey values", lambda: m.compact(n, W, H, pts.data_ptr(), f32, mask.data_ptr(), out.data_ptr(), counts.data_ptr(),
                                                                                         d_values=left.data_ptr(), values_pitch=W, d_out_values=vals.data_ptr(), stream=stream),
                  n * H * W, "pixel", f"{int(counts.sum())} survivors")
            del pts, out
    result = {"tool": "stereo_bench", "width": W, "height": H, "reps": a.reps, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
