"""Inputs shared by tests/test_tri_consensus_reference.py (CPU) and tests/test_gpu_tri_consensus.py: the rigs of
tests/test_gpu_tri_refine.py (``tri-perm``: 12 cameras, 6 images; ``tri-refine``: 32 cameras, 3 images; 0.3 px noise) with views moved by
30 to 200 px in a random direction — what a mismatched feature does to a view.  Every point with at least 4 views is hit: one view
when it has fewer than 8, two views when it has 8 or more.  Points with fewer views stay as they are."""
import functools

import numpy as np

from oracle import ba_oracle as orc
from pycamset_amd import compiled_helpers as hip_ch
from pycamset_amd import synthetic
from tests import tri_consensus_reference as cref

RIGS = ("tri-perm", "tri-refine")
# Chosen on the CPU (test_tri_consensus_reference.test_corruption_seeds_need_no_exception): with these seeds the restatement's inliers are
# exactly the unmoved rows of every point with at least 4 views, and its best two scores of distinct pairs are never within 1e-9 relative.
CORRUPTION_SEED = {"tri-perm": 3, "tri-refine": 3}
CONSENSUS = dict(n_hypotheses=64, inlier_px=8.0, seed=0)
MIN_VIEWS_CHECKED = 4


@functools.lru_cache(maxsize=None)
def clean_rig(name):
    """-> (rec, start, P, K, D, truth (n_pts, 3)): the grouped table of the rig (read-only) and the true points in its order."""
    if name == "tri-perm":
        rig = synthetic.make_rig("tri-perm", 12, 6, synthetic.ccube_points(5, 30.0), seed=21, visibility=0.45, n_rings=2)
    else:
        rig = synthetic.make_rig("tri-refine", 32, 3, synthetic.ccube_points(5, 30.0), seed=122, visibility=0.5, n_rings=2)
    im, P, K, D = orc.legacy_inputs(rig.intr_true, rig.extr_true, rig.poses_true, rig.points)
    d = rig.detections
    d = d[np.lexsort((d[:, 0], d[:, 2], d[:, 1]))]
    rec, start = hip_ch.group_reconstructable(d)
    truth = im[rec[start[:-1], 1].astype(int), rec[start[:-1], 2].astype(int)]
    for a in (rec, start, P, K, D, truth):
        a.setflags(write=False)
    return rec, start, P, K, D, truth


@functools.lru_cache(maxsize=None)
def corrupted_rig(name, seed=None):
    """-> (corrupted table, clean (n_obs,) bool: rows that were not moved)."""
    rec, start = clean_rig(name)[:2]
    rec = rec.copy()
    rng = np.random.default_rng(CORRUPTION_SEED[name] if seed is None else seed)
    clean = np.ones(rec.shape[0], dtype=bool)
    for j in range(len(start) - 1):
        V = int(start[j + 1] - start[j])
        if V < MIN_VIEWS_CHECKED:
            continue
        hit = start[j] + rng.permutation(V)[: 1 if V < 8 else 2]
        ang, mag = rng.uniform(0.0, 2.0 * np.pi, hit.shape[0]), rng.uniform(30.0, 200.0, hit.shape[0])
        rec[hit, -2] += mag * np.cos(ang)
        rec[hit, -1] += mag * np.sin(ang)
        clean[hit] = False
    rec.setflags(write=False)
    clean.setflags(write=False)
    return rec, clean


def deleted_table(rec, start, keep):
    """The table without the rows where ``keep`` is False -> (rows, start)."""
    n = len(start) - 1
    point = np.repeat(np.arange(n), np.diff(start))
    return rec[keep], np.append(0, np.cumsum(np.bincount(point[keep], minlength=n)))


@functools.lru_cache(maxsize=None)
def restated(name, corrupted=True, seed=None):
    """The restatement on the (corrupted) rig with CONSENSUS: (inlier, cinfo, score, gap).  Computed once, shared, read-only."""
    _, start, P, K, D, _ = clean_rig(name)
    rec = corrupted_rig(name, seed)[0] if corrupted else clean_rig(name)[0]
    out = cref.consensus_table(rec, start, P, K, D, CONSENSUS["n_hypotheses"], CONSENSUS["inlier_px"], CONSENSUS["seed"])
    for a in out:
        a.setflags(write=False)
    return out


def many_views(rows):
    """(n_obs,) bool: rows of points with at least MIN_VIEWS_CHECKED views, for a start array ``rows`` = start."""
    v = np.diff(rows)
    return np.repeat(v >= MIN_VIEWS_CHECKED, v)
