#!/usr/bin/env python3
"""Per-trial time of the device-steered LM loop with and without a Gaussian parameter prior (developer tool, one MI355X;
profiles/r21).  One process builds the rig of a BASELINE config, warms the solver up and then alternates whole solves
`lm_solve(h, x0, max_iter=30)` without a prior and with each prior asked for; the figure is host wall time per evaluation (a
trial), median and range over the rounds.

    python tools/prior_bench.py --config 3 --chain template --prior intr
    python tools/prior_bench.py --config 4 --chain self --prior intr,points
    python tools/prior_bench.py --root <another checkout> --config 3 --chain template      # a tree without priors: the plain solve only

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
    ap.add_argument("--prior", default="", help="comma-separated: intr (every intrinsic, sigma = 10 % of its size or 0.01), points (every free point coordinate, sigma 0.05)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--perturb", type=float, default=0.0, help="relative Gaussian perturbation of the start (seed 0): a farther start takes more trials per solve, "
                                                               "so the per-solve cost of setting and restoring the prior weighs less in the figure")
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
    for name in [p for p in a.prior.split(",") if p]:
        if name == "intr":
            mean, sigma = handlers.slab_prior(h, {"intr": np.maximum(0.1 * np.abs(rig.intr), 0.01)}, {"intr": rig.intr})
        elif name == "points":
            mean, sigma = handlers.slab_prior(h, {"bdpt": 0.05})
        else:
            raise SystemExit(f"unknown prior '{name}'")
        variants[name] = {"prior_mean": mean, "prior_sigma": sigma}
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
        n_prior = 0 if k == "none" else int(np.isfinite(variants[k]["prior_sigma"]).sum())
        print(f"  prior {k:7s} ({n_prior:7d} entries): median {np.median(t):.4f} ms per evaluation, range {t[0]:.4f} - {t[-1]:.4f} over {len(t)} solves "
              f"(median {np.median(solves[k]):.3f} ms per solve); {last[k].nfev} evaluations, cost {last[k].cost:.6e}, {last[k].message}")


if __name__ == "__main__":
    main()
