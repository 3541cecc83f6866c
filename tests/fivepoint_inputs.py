"""Inputs of the five-point tests, on top of tests/twoview_inputs.py: rigs whose points lie on (or mostly on) a plane that faces the arc
of cameras; shared by tests/test_fivepoint_reference.py (CPU) and tests/test_gpu_fivepoint.py."""
from __future__ import annotations

import numpy as np

from tests import pnp_reference as pref
from tests import twoview_inputs as ti

INLIER_PX = ti.INLIER_PX
PARITY_HYPOTHESES = (1, 16, 17)
BOUNDARY_N = (5, 6, 15, 16, 17, 33, 64, 65, 257)   # the sample is the whole pair; around the lane stride; around a wave; past 256
CAPABILITY_SEEDS = tuple(range(8))
CAPABILITY_OPTS = {"n_hypotheses": 16, "inlier_px": INLIER_PX, "seed": 0, "min_points": 16, "solver": "five-point", "refine_iters": 10}
CAPABILITY_SCENES = {"planar": (40, 0), "dominant": (48, 12)}


def replan(rig, n_plane, tilt, n_cams, noise_px, rng):
    """Move the first ``n_plane`` points of a rig onto y = tilt * x and project them again (fresh noise from ``rng``)."""
    pts = rig["points"].copy()
    pts[:n_plane, 1] = tilt * pts[:n_plane, 0]
    rig["points"] = pts
    d = rig["dct"]
    for c in range(n_cams):
        uv = pref.project(rig["R"][c], rig["t"][c], pts, rig["intr"][c])[0] + noise_px * rng.standard_normal((pts.shape[0], 2))
        rows = d[:, 0] == c
        d[rows, 3:5] = uv[d[rows, 2].astype(np.int64)]
    return rig


def planar_rig(n_plane, n_off, noise, seed, tilt=0.3):
    """Two cameras of ``arc_rig`` and n_plane + n_off keys; the first ``n_plane`` points are moved onto y = tilt * x, a plane that faces
    the arc (both cameras see it as a plane, not as a line)."""
    rig = ti.arc_rig(2, n_plane + n_off, noise, seed=seed)
    return replan(rig, n_plane, tilt, 2, noise, np.random.default_rng(seed + 1000))


def pair_table(rig, min_points=1):
    return ti.table_of(rig, 2, min_points)


def parity_inputs(refine_iters=0, solver="five-point"):
    """name -> (table, options): the 3-camera rig at H = 1, 16, 17 and one pair at every boundary size (H = 16, min_points = 5)."""
    rig = ti.table_of(ti.parity_rig(), 3, 16)
    base = {"inlier_px": INLIER_PX, "seed": 0, "solver": solver, "refine_iters": refine_iters}
    out = {f"rig3-H{H}": (rig, {**base, "n_hypotheses": H, "min_points": 16}) for H in PARITY_HYPOTHESES}
    for n in BOUNDARY_N:
        out[f"pair-n{n}"] = (ti.table_of(ti.one_pair(n), 2, 5), {**base, "n_hypotheses": 16, "min_points": 5})
    return out


def eight_point_refined_input():
    """``arc_rig(2, 40, 0.2, seed=11)`` for the eight-point solver with ten refinement trials."""
    return (ti.table_of(ti.arc_rig(2, 40, 0.2, seed=11), 2, 16),
            {"n_hypotheses": 16, "inlier_px": INLIER_PX, "seed": 0, "min_points": 16, "solver": "eight-point", "refine_iters": 10})


def capability_table(scene, noise, seed):
    n_plane, n_off = CAPABILITY_SCENES[scene]
    rig = planar_rig(n_plane, n_off, noise, seed)
    return rig, pair_table(rig, 16)


def planar_outlier_pair(n=60, seed=3):
    """``planar_rig(60, 0, 0.0, 3)`` and the same with 30 % of camera b's pixels replaced."""
    rig = planar_rig(n, 0, 0.0, seed)
    d = rig["dct"]
    uv_a, uv_b = d[d[:, 0] == 0][:, 3:5], d[d[:, 0] == 1][:, 3:5]
    bad, moved = ti.corrupt(uv_b, 0.3, np.random.default_rng(seed + 100))
    return rig, uv_a, uv_b, bad, moved


def planar_chain_rig(noise_px, seed=21, tilt=0.3):
    """``twoview_inputs.chain_rig`` with 80 % of its 60 keys (the first 48) on the facing plane."""
    return replan(ti.chain_rig(noise_px, seed), 48, tilt, 5, noise_px, np.random.default_rng(seed + 1000))


# ---- figures measured by tests/test_fivepoint_reference.py (it prints them and checks that they still hold) and used by the device tests ----
# float64 against extended precision of the restatement over the parity inputs at 0 and at 10 refinement trials and over the refined
# eight-point input: d_T = 2.1e-10 (the pair of 64 rows at 10 trials: the trial count of the LM is a discrete decision inside), d_s =
# 1.2e-7 (one hypothesis of the pair of 64 rows: a root of its polynomial is close to a double root).  The device is held to 8 x these.
D_T, D_S = 2.1e-10, 1.2e-7
# The largest rotation / translation-direction error in radians of the restatement over planar_rig(40, 0, 0.2, seed) and
# planar_rig(48, 12, 0.2, seed), seeds 0 .. 7, none left out (H = 16, tau = 2 px, 10 refinement trials): 5.2e-3 (planar, seed 5,
# translation direction).  The device is held to 2 x this.
CAPABILITY_POSE_ERROR = 5.2e-3
# Noise-free scenes: the only error above rounding is the residual of the five fixed-point undistortion steps, which the test measures on
# the fixture (largest |undistorted - ideal pinhole pixel|, up to 1.1e-6 px at radius 3).  A bias b px common to the rows moves the pose by
# b x the sensitivity to noise x sqrt(rows), because independent noise averages over the rows and a bias does not: 0.2 px of noise on 40
# rows cost 5.2e-3 rad, so 5.2e-3 / 0.2 x sqrt(40) = 0.16 rad / px.  The rounding of the solver itself (D_T) comes on top.
CLEAN_SENSITIVITY = 0.16


def clean_pose_bound(residual_px):
    return CLEAN_SENSITIVITY * residual_px + D_T


# What the restatement pipeline (pose_seeding.seed_scene on the restated entry points, five-point solver with 10 refinement trials)
# reaches on planar_chain_rig(0.0) after a similarity alignment to truth, the largest of point error / scene size, camera-centre error /
# scene size and rotation error in radians: 4.2e-13.  The device pipeline is held to 8 x this.
SCENE_GAP = 4.2e-13


def undistortion_residual(rig, cams=(0, 1)):
    """Largest |undistort(measured) - ideal pinhole pixel| in pixels over the noise-free rows of the cameras."""
    from tests import twoview_reference as tv

    worst = 0.0
    for c in cams:
        d = rig["dct"][rig["dct"][:, 0] == c]
        K0 = rig["intr"][c].copy()
        K0[4:] = 0.0
        ideal = pref.project(rig["R"][c], rig["t"][c], rig["points"][d[:, 2].astype(np.int64)], K0)[0]
        worst = max(worst, float(np.abs(tv.undistort(d[:, 3:5], rig["intr"][c]) - ideal).max()))
    return worst


def restated_two_view(d, K, *, consensus, inlier_px, seed, min_points, solver="eight-point", refine_iters=0):
    """``compiled_helpers.estimate_two_view`` on the restatement, with the device's signature (for ``pose_seeding.seed_scene``)."""
    from pycamset_amd import compiled_helpers as ch
    from tests import fivepoint_reference as fp
    from tests import twoview_reference as tv

    pairs, start, keys, ua, ub = tv.correspondences(d, K.shape[0], min_points=min_points)
    T, info, stats, inl, _ = fp.estimate_pairs(ua, ub, start, pairs, K, n_hypotheses=consensus, inlier_px=inlier_px, seed=seed, min_points=min_points,
                                               solver=solver, refine_iters=refine_iters)
    return ch.TwoViewResult(pairs=pairs, T=T, n=info[:, 0], n_inliers=info[:, 1], n_front=info[:, 2], status=info[:, 3], hypothesis=info[:, 4],
                            score=stats[:, 0], rms=stats[:, 1], parallax=stats[:, 2], start=start, keys=keys, uv_a=ua, uv_b=ub, inliers=inl)
