"""Inputs shared by tests/test_rig_graph_reference.py (CPU: the tie condition of every noisy input) and tests/test_gpu_rig_graph.py."""
import numpy as np
from scipy.spatial.transform import Rotation

from pycamset_amd import synthetic
from tests.test_pnp_reference import CUBE, true_view_poses, truth_rig

TILE = 64   # candidates the edge kernel stages through LDS at a time (csrc/ba_riggraph.hpp RIG_TILE)
G = 16      # lanes per (view, candidate) group of the scoring kernel (csrc/pcs_rig.inc RIG_G)
NOISE_PX = 0.3
SEED = 21
# (kind, visibility) of the noisy 3 x 3 rigs of the parity test
PARITY_RIGS = [("cube", 1.0), ("planar", 1.0), ("cube", 0.5), ("planar", 0.5)]
TILE_IMAGES = [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def parity_rig(kind, vis):
    return truth_rig(kind, noise_px=NOISE_PX, seed=SEED, visibility=vis)


def chain_rig(noise_px=NOISE_PX, seed=SEED):
    """5 cameras x 8 images of the cube; camera c keeps the images 2 c - 2 .. 2 c + 1, so it shares images (two of them) only with
    c - 1 and c + 1 and no image is seen by more than two cameras."""
    rig = synthetic.make_rig("rig-chain", 5, 8, CUBE, seed=seed, noise_px=noise_px)
    det = rig.detections
    cam, pair = det[:, 0].astype(np.int64), det[:, 1].astype(np.int64) // 2
    return rig, det[(pair == cam) | (pair == cam - 1)]


def ring_rig(n_cams=8, n_imgs=6, neighbours_only=False, noise_px=NOISE_PX, seed=SEED):
    """A ring of cameras around the cube.  ``neighbours_only``: image i is kept by the cameras i mod C and (i + 1) mod C only, so that
    the co-visibility graph is the ring itself and no image is seen by every camera."""
    rig = synthetic.make_rig("rig-ring", n_cams, n_imgs, CUBE, seed=seed, noise_px=noise_px)
    det = rig.detections
    if neighbours_only:
        cam, im = det[:, 0].astype(np.int64), det[:, 1].astype(np.int64)
        det = det[(cam == im % n_cams) | (cam == (im + 1) % n_cams)]
    return rig, det


def perturbed_view_poses(n_cams, n_imgs, seed=SEED, rot=1e-3, trans=1e-4):
    """(rig, (C, I, 6)): the true view poses of a seeded rig with a seeded perturbation of the size 0.3 px of noise gives a PnP
    (rotation ``rot`` rad, translation ``trans`` m): view poses for the edge kernel without running a PnP."""
    rig = synthetic.make_rig("rig-poses", n_cams, n_imgs, CUBE[:8], seed=seed, noise_px=0.0)
    rng = np.random.default_rng(seed + 1)
    T = true_view_poses(rig)
    out = np.empty_like(T)
    for c in range(n_cams):
        for i in range(n_imgs):
            out[c, i, :3] = (Rotation.from_rotvec(rng.normal(0, rot, 3)) * Rotation.from_rotvec(T[c, i, :3])).as_rotvec()
            out[c, i, 3:] = T[c, i, 3:] + rng.normal(0, trans, 3)
    return rig, out
