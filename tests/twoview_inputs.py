"""Inputs of the two-view tests: small synthetic rigs looking at a cloud of free points, as flat (N, 5) tables [cam, im, key, u, v], with
their true poses; shared by tests/test_twoview_reference.py (CPU) and tests/test_gpu_twoview.py."""
from __future__ import annotations

import numpy as np

from tests import pnp_reference as pref

PARITY_HYPOTHESES = (1, 16, 17)
INLIER_PX = 2.0
# How closely a noise-free pair at radius 5 recovers the true (R, t / |t|).  The only error above rounding is the residual of the five
# fixed-point undistortion steps: the distortion moves a normalised point by at most |k0| r^2 |x| = 0.08 * 0.11 * 0.33 = 3e-3 there, each step
# contracts by at most 3 |k0| r^2 = 0.026, so 3e-3 * 0.026^5 = 3.5e-11, or 4e-8 px at f = 1200.  The same rig with 0.2 px of noise ends
# 4e-3 off (test_twoview_reference prints it): 2e-2 per pixel.  4e-8 px * 2e-2 / px = 8e-10.
CLEAN_POSE_BOUND = 1e-9


def intrinsics(n_cams, rng):
    """(C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2]: mildly different cameras with a little distortion."""
    K = np.zeros((n_cams, 9))
    K[:, 0] = 1200.0 + rng.uniform(-40, 40, n_cams)
    K[:, 2] = K[:, 0] * (1.0 + rng.uniform(-0.01, 0.01, n_cams))
    K[:, 1] = 640.0 + rng.uniform(-15, 15, n_cams)
    K[:, 3] = 480.0 + rng.uniform(-15, 15, n_cams)
    K[:, 4] = rng.uniform(-0.08, -0.02, n_cams)
    K[:, 5] = rng.uniform(0.0, 0.02, n_cams)
    K[:, 6:8] = rng.uniform(-5e-4, 5e-4, (n_cams, 2))
    return K


def look_at(centre, target):
    """(R, t) of a camera at ``centre`` looking at ``target``: X_cam = R X + t, z forward, y roughly down."""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def arc_rig(n_cams, n_keys, noise_px, seed, radius=3.0, spread=0.45, visible=None, depth=1.0):
    """Cameras on an arc around a cloud of ``n_keys`` points in a box of half size (1, 1, depth).  visible(c, k) -> bool restricts which
    camera sees which key.  -> dict(dct, intr, R (C, 3, 3), t (C, 3), points (K, 3))."""
    rng = np.random.default_rng(seed)
    K = intrinsics(n_cams, rng)
    pts = rng.uniform(-1.0, 1.0, (n_keys, 3)) * np.array([1.0, 1.0, depth])
    Rs, ts, rows = [], [], []
    for c in range(n_cams):
        ang = spread * (c - 0.5 * (n_cams - 1))
        centre = radius * np.array([np.sin(ang), -np.cos(ang), 0.15 * ((c % 3) - 1)])
        R, t = look_at(centre, rng.uniform(-0.1, 0.1, 3))
        Rs.append(R)
        ts.append(t)
        uv = pref.project(R, t, pts, K[c])[0] + noise_px * rng.standard_normal((n_keys, 2))
        rows += [[c, 0, k, uv[k, 0], uv[k, 1]] for k in range(n_keys) if visible is None or visible(c, k)]
    return {"dct": np.array(rows, dtype=np.float64), "intr": K, "R": np.array(Rs), "t": np.array(ts), "points": pts}


def relative_pose(rig, a, b):
    """The true (R, t / |t|) of camera a -> camera b."""
    R = rig["R"][b] @ rig["R"][a].T
    t = rig["t"][b] - R @ rig["t"][a]
    return R, t / np.linalg.norm(t)


def parity_rig():
    """The parity input of both test files: 3 cameras, 40 keys, 0.2 px noise."""
    return arc_rig(3, 40, 0.2, seed=11)


def one_pair(n, noise_px=0.2, seed=5):
    """One pair of n correspondences."""
    return arc_rig(2, n, noise_px, seed=seed + n)


def corrupt(uv, fraction, rng):
    """Replace ``fraction`` of the rows by uniformly random pixels: (corrupted copy, moved (n,) bool)."""
    n = uv.shape[0]
    moved = np.zeros(n, dtype=bool)
    moved[rng.choice(n, int(round(fraction * n)), replace=False)] = True
    out = uv.copy()
    out[moved] = rng.uniform([0.0, 0.0], [1280.0, 960.0], (int(moved.sum()), 2))
    return out, moved


def outlier_pair(n=60, seed=3):
    """A noise-free pair of n rows (its clean table) and the same with 30 % of camera b's pixels replaced."""
    rig = arc_rig(2, n, 0.0, seed=seed, radius=5.0)
    d = rig["dct"]
    uv_a, uv_b = d[d[:, 0] == 0][:, 3:5], d[d[:, 0] == 1][:, 3:5]
    bad, moved = corrupt(uv_b, 0.3, np.random.default_rng(seed + 100))
    return rig, uv_a, uv_b, bad, moved


def coplanar_pair(n=40, seed=9):
    """Two cameras looking at points of one plane: the eight-point method's degenerate case."""
    return arc_rig(2, n, 0.0, seed=seed, depth=0.0)


def identical_cameras(n=40, seed=9):
    """Two cameras with the same pose (no baseline) and the same pixels."""
    rig = arc_rig(2, n, 0.0, seed=seed)
    d = rig["dct"]
    second = d[d[:, 0] == 0].copy()
    second[:, 0] = 1
    rig["dct"] = np.concatenate([d[d[:, 0] == 0], second])
    rig["intr"][1] = rig["intr"][0]
    rig["R"][1], rig["t"][1] = rig["R"][0], rig["t"][0]
    return rig


BOUNDARY_N = (8, 15, 16, 17, 33, 64, 65, 257)   # the sample is the whole pair; around the lane stride 16 and 2 x 16 + 1; around a wave; past 256


def table_of(rig, n_cams, min_points):
    """The grouped correspondence table of a rig, as ``twoview_reference.correspondences`` builds it."""
    from tests import twoview_reference as tv

    pairs, start, _, ua, ub = tv.correspondences(rig["dct"], n_cams, min_points=min_points)
    return {"uv_a": ua, "uv_b": ub, "start": start, "pairs": pairs, "intr": rig["intr"]}


def parity_inputs():
    """name -> (table, options): the 3-camera rig at H = 1, 16, 17 and one pair at every boundary size (H = 16, min_points = 8)."""
    rig = table_of(parity_rig(), 3, 16)
    out = {f"rig3-H{H}": (rig, {"n_hypotheses": H, "inlier_px": INLIER_PX, "seed": 0, "min_points": 16}) for H in PARITY_HYPOTHESES}
    for n in BOUNDARY_N:
        out[f"pair-n{n}"] = (table_of(one_pair(n), 2, 8), {"n_hypotheses": 16, "inlier_px": INLIER_PX, "seed": 0, "min_points": 8})
    return out


def chain_rig(noise_px, seed=21):
    """Five cameras on an arc, 60 keys, key k seen by the three cameras k % 3 .. k % 3 + 2: camera i shares keys only with i +- 1 and
    i +- 2 (20 or 40 of them), so that a seed needs two rounds of resection after its first pair."""
    return arc_rig(5, 60, noise_px, seed=seed, radius=5.0, visible=lambda c, k: k % 3 <= c <= k % 3 + 2)


SCENE_HYPOTHESES = 16
# What the restatement pipeline (tests/twoview_reference.py seed_scene) reaches on chain_rig(0.0) after a similarity alignment to truth, the
# largest of point error / scene size, camera-centre error / scene size and rotation error in radians: 5.6e-12, measured and pinned by
# tests/test_twoview_reference.py test_scene_seed_of_the_restatement.  The device pipeline is held to 8 x this.
SCENE_GAP = 5.6e-12


def in_camera_frame(rig, cam=0):
    """The truth of a rig with the world moved to a camera's frame: (extr (C, 6) = [rotvec, t], points (K, 3))."""
    from scipy.spatial.transform import Rotation

    R0, t0 = rig["R"][cam], rig["t"][cam]
    extr = np.zeros((rig["R"].shape[0], 6))
    for c in range(extr.shape[0]):
        Rc = rig["R"][c] @ R0.T
        extr[c, :3], extr[c, 3:] = Rotation.from_matrix(Rc).as_rotvec(), rig["t"][c] - Rc @ t0
    return extr, rig["points"] @ R0.T + t0
