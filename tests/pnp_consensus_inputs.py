"""Inputs shared by tests/test_pnp_consensus_reference.py (CPU) and tests/test_gpu_pnp_consensus.py: the rigs of
``test_pnp_reference.truth_rig`` (3 cameras x 3 images, 16 to 54 detections per view, 0.3 px noise, seed 21) with 15 % of the
detections of EVERY view moved by 30 to 200 px in a random direction — what a wrong ChArUco id does to a detection."""
import numpy as np

from tests.test_pnp_reference import truth_rig

KINDS = ("cube", "planar", "face")
FRACTION = 0.15
# Chosen on the CPU (test_pnp_consensus_reference.test_corruption_seed_needs_no_exception): with this seed the restatement finds exactly the
# uncorrupted set in every view of every kind, and its best two scores are never closer than 1e-9 relative.
CORRUPTION_SEED = 3
CONSENSUS = dict(n_hypotheses=64, sample_size=6, inlier_px=8.0, seed=0)


def corrupted_rig(kind, fraction=FRACTION, seed=CORRUPTION_SEED):
    """-> (rig, corrupted table, clean (N,) bool: rows that were not moved)."""
    rig, det = truth_rig(kind, noise_px=0.3, seed=21)
    det = det.copy()
    rng = np.random.default_rng(seed)
    clean = np.ones(det.shape[0], dtype=bool)
    vid = det[:, 0].astype(np.int64) * 3 + det[:, 1].astype(np.int64)
    for v in np.unique(vid):
        rows = np.nonzero(vid == v)[0]
        hit = rng.permutation(rows)[: int(round(fraction * rows.shape[0]))]
        ang, mag = rng.uniform(0.0, 2.0 * np.pi, hit.shape[0]), rng.uniform(30.0, 200.0, hit.shape[0])
        det[hit, 3] += mag * np.cos(ang)
        det[hit, 4] += mag * np.sin(ang)
        clean[hit] = False
    return rig, det, clean
