#!/usr/bin/env python3
"""Per-group residual statistics (pcs_stats_run) at rig-32 (about 1e6 detections) and ring-8: device time of the index build, of the
error kernel and of the statistics (gather + statistics kernel, device events), the whole ``diagnostics.reprojection_report`` call on
the host clock, and what the call replaces: the NumPy restatement of tests/stats_reference.py on a read-back residual (read-back
included), also on the host clock.

    python tools/stats_bench.py [--reps 10] [--configs 3,2]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from pycamset_amd import _capi, diagnostics, function_blocks as fb, handlers, synthetic  # noqa: E402
from tests import stats_reference as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--configs", default="3,2")
args = ap.parse_args()


def spread(ms):
    return f"{np.median(ms):10.3f} ms (min {np.min(ms):.3f}, max {np.max(ms):.3f})"


for cfg in args.configs.split(","):
    rig = synthetic.config_rig(int(cfg))
    op = fb.projection() + fb.extrinsic3D() + fb.template_points()
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, rig.poses], template=rig.points)
    counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
    x = prob.x0
    for _ in range(2):   # warm-up: engine, code objects, the index
        report = diagnostics.reprojection_report(prob, x)
    stats = report._stats
    whole, parts = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        report = diagnostics.reprojection_report(prob, x)
        whole.append((time.perf_counter() - t0) * 1e3)
        parts.append(stats.last_kernel_ms())
    e = report.errors()   # before the handle runs again
    index = []
    ids = [np.ascontiguousarray(rig.detections[:, k], dtype=np.int32) for k in range(3)]
    for _ in range(max(2, args.reps // 3)):
        stats.set_groups(*ids)
        index.append(stats.last_kernel_ms()[0])
    stats._table = None   # the index was rebuilt behind reprojection_report's back
    d_resid = _capi.c_void_p()   # the engine's residual buffer, still holding the residual at x
    _capi.check(_capi.lib().pcs_device_buffers(op.engine._h, _capi.ctypes.byref(d_resid), None))
    sums_only = []
    for _ in range(args.reps):
        stats.run(d_resid.value, order_statistics=False)
        stats.results("overall")
        sums_only.append(stats.last_kernel_ms()[2])
    loss = prob.make_loss_fun()
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        ref.all_group_stats(loss(x), *(rig.detections[:, k] for k in range(3)), counts)
        host.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(getattr(g, f), np.asarray(ref.all_group_stats(loss(x), *(rig.detections[:, k] for k in range(3)), counts, e=e)[name][f]).reshape(
        np.shape(getattr(g, f))), equal_nan=True) for name, g in (("camera", report.per_camera), ("image", report.per_image)) for f in ("median", "mad", "count"))
    n_groups = stats.n_groups
    sizes = {name: (int(g.count.min()), int(g.count.max())) for name, g in (("camera", report.per_camera), ("image", report.per_image), ("key", report.per_key),
                                                                          ("view", report.per_view))}
    print(f"{rig.name}: {rig.n_det} detections, {n_groups} groups (rows per group: " + ", ".join(f"{k} {a}..{b}" for k, (a, b) in sizes.items()) + ")")
    print(f"  index build (once per table), device events:          {spread(index)}")
    print(f"  error kernel, device events:                          {spread([p[1] for p in parts])}")
    print(f"  statistics (gather + kernel), device events:          {spread([p[2] for p in parts])}")
    print(f"  statistics without median and MAD, device events:     {spread(sums_only)}")
    print(f"  reprojection_report, whole call, host clock:          {spread(whole)}")
    print(f"  NumPy restatement on a read-back residual, host clock:{spread(host)}")
    print(f"  ratio restatement / reprojection_report: {np.median(host) / np.median(whole):.1f} x; medians, MADs and counts per camera and image equal to the restatement's: {same}")
    print(f"  overall: mean {report.overall.mean[0]:.4f} px, rms {report.overall.rms[0]:.4f}, median {report.overall.median[0]:.4f}, mad {report.overall.mad[0]:.4f}, "
          f"worst row {report.overall.argmax[0]} at {report.overall.max[0]:.3f} px")
