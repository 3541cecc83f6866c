#!/usr/bin/env python3
"""Per-trial time of the device-steered LM loop with and without box bounds (developer tool, one MI355X; profiles/r25).  One process
builds the rig of a BASELINE config, warms the solver up and then alternates whole solves `lm_solve(h, x0, max_iter=30)` without
bounds and with the bounds asked for; the figure is host wall time per evaluation (a trial), median and range over the rounds.

    python tools/bounds_bench.py --config 3 --chain template --bounds wide          # a few bounds set, none binding: the non-fused path
    python tools/bounds_bench.py --root <another checkout> --config 3 --chain template      # a tree without bounds: the plain solve only

Run under `rocprofv3 --kernel-trace --stats` with `--rounds 1` for the launches per trial."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="the checkout to import pycamset_amd from")
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--chain", default="template")
    ap.add_argument("--bounds", default="", help="comma-separated: wide (every focal length and principal point within +- 50 % of its start: set, never binding), "
                                                 "tight (every focal length at most 0.5 % above its start: binding)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--perturb", type=float, default=0.0, help="relative Gaussian perturbation of the start (seed 0): a farther start takes more trials per solve, "
                                                               "so the per-solve cost of setting and restoring the bounds weighs less in the figure")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    from pycamset_amd import handlers, synthetic
    from pycamset_amd.detections import TargetDetection
    from pycamset_amd.device_solver import lm_solve

    class Camset:
        def __init__(self, n):
            self.names = [f"cam_{i}" for i in range(n)]

        def get_names(self):
            return list(self.names)

        def get_n_cams(self):
            return len(self.names)

    class Target:
        def __init__(self, pts):
            self.point_data = np.asarray(pts)[None]

    rig = synthetic.config_rig(a.config)
    cs = Camset(rig.n_cams)
    cls = {"template": handlers.TemplateBundleHandler, "self": handlers.SelfBundleHandler, "free": handlers.FreePointBundleHandler}[a.chain]
    h = cls(cs, Target(rig.points), TargetDetection(cs.get_names(), rig.detections), fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}},
            options={"verbosity": 0, "max_nfev": a.max_iter})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel()]
    if a.chain != "free":
        parts.append(rig.poses[bp.poses_unfixed].ravel())
    if a.chain != "template":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    x0 = np.concatenate(parts)
    if a.perturb:
        x0 = x0 * (1.0 + a.perturb * np.random.default_rng(0).standard_normal(x0.shape))
    variants = {"none": {}}
    for name in [p for p in a.bounds.split(",") if p]:
        lo, hi = np.full(x0.shape, -np.inf), np.full(x0.shape, np.inf)
        n_intr = 9 * int(np.count_nonzero(bp.intr_unfixed))
        if name == "wide":
            for j in range(4):
                lo[j:n_intr:9], hi[j:n_intr:9] = 0.5 * x0[j:n_intr:9], 1.5 * x0[j:n_intr:9]
        elif name == "tight":
            hi[0:n_intr:9] = 1.005 * x0[0:n_intr:9]
        else:
            raise SystemExit(f"unknown bounds '{name}'")
        variants[name] = {"bounds": (lo, hi)}
    print(f"# {a.root}: {rig.name} chain {a.chain}, N = {rig.n_det}, {x0.shape[0]} free parameters; ms per evaluation over whole solves of at most {a.max_iter} iterations")
    times = {k: [] for k in variants}
    solves = {k: [] for k in variants}
    last = {}
    for rnd in range(a.rounds + 1):                      # round 0 warms every variant's solver state up and is not counted
        for k, kw in variants.items():
            lm_solve(h, x0.copy(), max_iter=2, **kw)     # the cache holds one solver state: the variant's own, allocated outside the timing
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = lm_solve(h, x0.copy(), max_iter=a.max_iter, **kw)
            dt = time.perf_counter() - t0
            if rnd:
                times[k].append(dt / res.nfev * 1e3)
                solves[k].append(dt * 1e3)
            last[k] = res
    for k, t in times.items():
        t = np.sort(t)
        n_finite = 0 if k == "none" else int(np.isfinite(variants[k]["bounds"][0]).sum() + np.isfinite(variants[k]["bounds"][1]).sum())
        print(f"  bounds {k:7s} ({n_finite:7d} finite): median {np.median(t):.4f} ms per evaluation, range {t[0]:.4f} - {t[-1]:.4f} over {len(t)} solves "
              f"(median {np.median(solves[k]):.3f} ms per solve); {last[k].nfev} evaluations, cost {last[k].cost:.6e}, {last[k].message}"
              + (f", {last[k].n_truncated} cut trials, {int(np.count_nonzero(last[k].active_mask))} active" if k != "none" else ""))


if __name__ == "__main__":
    main()
