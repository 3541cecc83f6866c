#!/usr/bin/env python3
"""Time device_solver.parameter_covariance (build + Schur reduction + dense Cholesky + L^-1 / Z = L^-1 V + block Grams, blocks read
back) on configs 1 / 3 / 4 and on the dense generated chain projection + extrinsic3D + rigidTform3d + board_flex over rig-32
(n_params = 2 680), against what a user can do today: download the packed normal equations [A | B | C] and form the same blocks with
numpy (S = A - B C^-1 B', inv(S), C_e^-1 + C_e^-1 B_e' S^-1 B_e C_e^-1).  Wall-clock medians of --reps calls after one warm-up.

    python tools/covariance_bench.py [--reps 5] [--only 1,3,4,flex]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from pycamset_amd import function_blocks as fb, handlers, synthetic  # noqa: E402
from pycamset_amd.detections import TargetDetection  # noqa: E402
from pycamset_amd.device_solver import parameter_covariance  # noqa: E402


class _Camset:
    def __init__(self, n):
        self.n = n

    def get_names(self):
        return [f"cam_{i}" for i in range(self.n)]

    def get_n_cams(self):
        return self.n


class _Target:
    def __init__(self, points):
        self.point_data = np.asarray(points, dtype=np.float64)[None]


def bundle_problem(cfg, chain):
    rig = synthetic.config_rig(cfg)
    cls = {"template": handlers.TemplateBundleHandler, "self": handlers.SelfBundleHandler}[chain]
    h = cls(_Camset(rig.n_cams), _Target(rig.points), TargetDetection([f"cam_{i}" for i in range(rig.n_cams)], rig.detections),
            fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
    bp = h.bundlePrimitive
    parts = [rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()]
    if chain == "self":
        parts.append(rig.points.ravel()[bp.bdpt_unfixed])
    return f"config {cfg} ({rig.name}, {chain})", h, np.concatenate(parts)


def flex_problem():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    from helpers import user_blocks
    rig = synthetic.config_rig(3)
    op = fb.projection() + fb.extrinsic3D() + fb.rigidTform3d() + user_blocks(fb)["board_flex"]()
    flex = np.concatenate([np.ones((rig.n_imgs, 2)), np.zeros((rig.n_imgs, 2)), np.full((rig.n_imgs, 1), 0.01)], axis=1)
    fix_ext = np.ones_like(rig.extr, dtype=bool)
    fix_ext[0] = False
    free_flex = np.zeros((rig.n_imgs, 5), dtype=bool)
    free_flex[:, 4] = True
    prob = handlers.ChainProblem(op, rig.detections, [rig.intr, rig.extr, rig.poses, flex], template=rig.points, unfixed=[None, fix_ext, None, free_flex])
    return "rig-32 board_flex (dense chain)", prob, prob.x0.copy()


def host_blocks(h, x):
    """The host alternative: the packed blocks to the host, the covariance blocks with numpy."""
    eng = h.op_fun._engine_for(h._flat_detections())
    lay = eng.normal_layout()
    nl, nt, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
    ps = torch.from_numpy(h.op_fun.build_param_list(*h.get_bundle_adjustment_inputs(x))).cuda()
    pk = torch.empty(lay["packed_len"], dtype=torch.float64, device="cuda")
    eng.normal_blocks_device(ps.data_ptr(), pk.data_ptr())
    torch.cuda.synchronize()
    pk = pk.cpu().numpy()
    fx = ~h._jac_mask()
    A = pk[: nl * nl].reshape(nl, nl)
    A = np.triu(A) + np.triu(A, 1).T
    fl = fx[:nl]
    A[fl, :] = 0.0
    A[:, fl] = 0.0
    A[np.flatnonzero(fl), np.flatnonzero(fl)] = 1.0
    if not nt:
        return np.linalg.inv(A)
    B = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt).copy()
    C = pk[nl * nl + nl * nt: nl * nl + nl * nt + nt * tb].reshape(-1, tb, tb)
    C = np.triu(C) + np.transpose(np.triu(C, 1), (0, 2, 1))
    ft = fx[nl:].reshape(-1, tb)
    B[fl, :] = 0.0
    B[:, fx[nl:]] = 0.0
    for e in np.flatnonzero(ft.any(axis=1)):
        C[e][ft[e], :] = 0.0
        C[e][:, ft[e]] = 0.0
        C[e][ft[e], ft[e]] = 1.0
    Ci = np.linalg.inv(C)
    Bb = B.reshape(nl, -1, tb)
    W = np.einsum("ieb,ebc->iec", Bb, Ci)                # B_e C_e^-1
    Si = np.linalg.inv(A - W.reshape(nl, -1) @ B.T)
    M = np.einsum("iec,ij,jed->ecd", W, Si, W, optimize=True)
    return Si, Ci + M


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="1,3,4,flex")
    args = ap.parse_args()
    which = args.only.split(",")
    probs = [bundle_problem(c, ch) for c, ch in ((1, "template"), (3, "template"), (4, "self")) if str(c) in which]
    if "flex" in which:
        probs.append(flex_problem())
    for name, h, x in probs:
        eng = h.op_fun._engine_for(h._flat_detections())
        h.op_fun._bind_template(eng, h._template_arg())
        lay = eng.normal_layout()
        cov = parameter_covariance(h, x)
        dev_ms = timed(lambda: parameter_covariance(h, x), args.reps)
        host_ms = timed(lambda: host_blocks(h, x), max(1, min(args.reps, 3)))
        print(f"{name}: N={h._flat_detections().shape[0]} n_lead={lay['n_lead']} n_trail={lay['n_trail']} sigma2={cov.sigma2:.4f} "
              f"min_pivot={cov.min_pivot:.3e}  device {dev_ms:.2f} ms  host (download + numpy) {host_ms:.2f} ms  ratio {host_ms / dev_ms:.2f}", flush=True)


if __name__ == "__main__":
    main()
