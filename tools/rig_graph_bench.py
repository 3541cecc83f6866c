#!/usr/bin/env python3
"""View-graph seeding (pcs_rig_*) on rig-32 (config 3: 32 cameras, 200 images, about 1e6 observations), fully visible and cut to
neighbour visibility (camera c keeps the images in which one of its two ring neighbours is the lowest camera, see ``cut_to_neighbours``),
after the device PnP: the existing ``estimate_camera_relative_poses`` (C passes of the legacy cost; fully visible rig only, it raises on
the cut one) against the new path split into edge kernel, preparation, scoring (device events) and host tree + selection + re-basing
(host clock).  Warm-up runs, then ``--reps`` repeats: median and min .. max.

    python tools/rig_graph_bench.py [--reps 10] [--warmup 2] [--config 3] [--n-imgs N]
Kernel times from rocprofv3 in a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rig -- python tools/rig_graph_bench.py --reps 3
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import pose_seeding, synthetic  # noqa: E402
from pycamset_amd import compiled_helpers as hc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--n-imgs", type=int, default=None)
args = ap.parse_args()


def cut_to_neighbours(det, n_cams):
    """Image i is kept by the cameras i mod C and (i + 1) mod C only: the co-visibility graph is a ring, no image is seen by all."""
    cam, im = det[:, 0].astype(np.int64), det[:, 1].astype(np.int64)
    return det[(cam == im % n_cams) | (cam == (im + 1) % n_cams)]


def stats(xs, unit="us", scale=1e3):
    xs = np.asarray(xs) * scale
    return f"median {np.median(xs):10.1f} {unit} (min {xs.min():.1f}, max {xs.max():.1f})"


rig = synthetic.config_rig(args.config, n_imgs=args.n_imgs)
C, I = rig.n_cams, rig.n_imgs
for name, det in (("fully visible", rig.detections), ("neighbours only", cut_to_neighbours(rig.detections, C))):
    vp = hc.estimate_view_poses(det, rig.points, rig.intr, n_imgs=I)
    have = np.isfinite(vp.poses[:, :, 0])
    shared = (have[:, None, :] & have[None, :, :]).sum(axis=2)[np.triu_indices(C, 1)]
    print(f"{rig.name}, {name}: {det.shape[0]} observations, {int(have.sum())} views with a pose, pairs with shared images {int((shared > 0).sum())} of "
          f"{shared.size}, distance evaluations {int((shared.astype(np.int64) ** 2).sum())}")
    fixed = lambda *a, **k: vp  # noqa: E731
    # the existing path: everything after the PnP, host clock around calls that end in device synchronisations
    try:
        t = []
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            pose_seeding.estimate_camera_relative_poses(det, rig.points, rig.intr, C, I, view_pose_fn=fixed)
            t.append((time.perf_counter() - t0) * 1e3)
        print(f"  existing estimate_camera_relative_poses after the PnP (host clock):   {stats(t[args.warmup:], 'ms', 1.0)}")
    except ValueError as e:
        print(f"  existing estimate_camera_relative_poses: ValueError({e})")
    # the new path, whole (host clock) and split (device events / host clock)
    t = []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = pose_seeding.estimate_camera_relative_poses_graph(det, rig.points, rig.intr, C, I, view_pose_fn=fixed, return_graph=True)
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"  estimate_camera_relative_poses_graph after the PnP (host clock):      {stats(t[args.warmup:], 'ms', 1.0)}")
    info = out[4]
    print(f"    sigma of the usable edges: median {np.median(info.sigma[np.isfinite(info.edge_cost)]):.3e} m; missing images {int(out[3].sum())}")
    order, ids, start = hc.group_by_view(det, I)
    ds = det if order is None else det[order]
    g = hc.RigGraph(C, I, rig.n_keys)
    g.set_cameras(rig.intr)
    _, rho = g.set_template(rig.points)
    g.set_observations(ds[:, 2].astype(np.int32), ds[:, 3:5], start, (ids // I).astype(np.int32), (ids % I).astype(np.int32))
    g.set_view_poses(vp.poses)
    edges_ms, prep_ms, score_ms, tree_ms, select_ms = [], [], [], [], []
    for r in range(args.warmup + args.reps):
        g.run_edges()
        e_info, e_T, e_stats = g.edges()
        t0 = time.perf_counter()
        n, sigma = e_info[:, 0].astype(np.int64), e_stats[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = np.where((n > 0) & np.isfinite(sigma), sigma + rho / np.maximum(n, 1), np.inf)
        pairs = hc.camera_pairs(C)
        parents, settled = pose_seeding.shortest_path_tree(C, pairs, cost, 0)
        T = pose_seeding.to_4x4(e_T.reshape(-1, 3, 4))
        E = np.zeros((C, 4, 4))
        E[0] = np.eye(4)
        for c in settled[1:]:
            p = int(parents[c])
            a, b = min(c, p), max(c, p)
            T_ab = T[a * (2 * C - a - 1) // 2 + b - a - 1]
            E[c] = (T_ab if c == a else pose_seeding.rigid_inverse(T_ab)) @ E[p]
        tree_ms.append((time.perf_counter() - t0) * 1e3)
        g.set_extrinsics(E[:, :3, :])
        g.run_scores()
        W, errors = g.results()
        t0 = time.perf_counter()
        fin = np.isfinite(errors)
        best = np.argmin(np.where(fin, errors, np.inf), axis=0)
        pose = pose_seeding.to_4x4(W)[best, np.arange(I)]
        ok = fin.any(axis=0)
        P_ref = pose[int(np.argmax(ok))]
        pose_seeding.pose_from_4x4(pose_seeding.rigid_inverse(P_ref) @ pose[ok])
        pose_seeding.pose_from_4x4(E @ P_ref)
        select_ms.append((time.perf_counter() - t0) * 1e3)
        edges_ms.append(g.last_edges_ms())
        a, b = g.last_scores_ms()
        prep_ms.append(a)
        score_ms.append(b)
    w = args.warmup
    print(f"    edge kernel (view matrices + consensus, device events):            {stats(edges_ms[w:])}")
    print(f"    preparation (W and projections, device events):                    {stats(prep_ms[w:])}")
    print(f"    scoring (score + per-image sums, device events):                   {stats(score_ms[w:])}")
    print(f"    host tree and composition of the extrinsics (host clock):          {stats(tree_ms[w:])}")
    print(f"    host selection and re-basing (host clock):                         {stats(select_ms[w:])}")
    g.close()
