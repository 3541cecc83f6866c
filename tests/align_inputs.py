"""Inputs and pinned constants of the point-set registration tests (tests/test_align_reference.py on the CPU, tests/test_gpu_align.py on
the device).  Everything is drawn from fixed seeds; nothing here touches a device."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

# Problem sizes of the parity table: below, at and above both group widths (16, 64), more than one stride of either, the smallest
# problem the fit takes (3), and empty problems between full ones.  37 problems: not a multiple of the 16 or 4 groups of a workgroup.
SIZES = [3, 0, 4, 15, 16, 0, 17, 33, 63, 64, 65, 257]
N_PROBLEMS = 37
NOISE = 1e-3

# Largest float64-versus-extended difference of the restatement (tests/align_reference.py) over parity_inputs() x both models x
# with / without weights, as (|dR|, |dt| / scene size, |ds| / s).  Measured: (7.35e-15, 1.147e-9, 1.246e-15);
# tests/test_align_reference.py::test_align_gap_is_the_pinned_one recomputes it.  The three-point planar problem sets the rotation
# figure and the offset-by-1e6 table the translation figure (1e6 x 2^-53 x a few roundings, against a scene of a few units).  The
# device is held to 8 x these.
ALIGN_GAP = (7.35e-15, 1.15e-9, 1.25e-15)

# The larger of the two distances to the extended-precision restatement on the golden sets (tests/golden/rigid_transform.npz), as
# (|dR|, |dt|): the restatement in float64 and the reference's n_estimate_rigid_transform.  The two agree within 4 x these.
GOLDEN_GAP = (1.46e-15, 8.7e-16)   # measured: (1.460e-15, 8.613e-16), both on the mirrored set

# The change of a handler's residual vector that the restatement's own gauge transform causes through the same closure (pixels).
GAUGE_CLOSURE_GAP = 2.3e-13   # measured: 2.27e-13 for both scales, one unit in the last place of a pixel coordinate near 1e3


def random_transform(rng, scale_range=(0.5, 2.0)):
    return float(rng.uniform(*scale_range)), Rotation.from_rotvec(rng.normal(size=3) * 0.8).as_matrix(), rng.normal(size=3) * 3.0


def make_problem(rng, n, planar=False, mirrored=False, offset=0.0, noise=NOISE, scale_range=(0.5, 2.0)):
    """n rows: src in a box of a few units, dst = s R src + t + noise."""
    s, R, t = random_transform(rng, scale_range)
    x = rng.uniform(-1.0, 1.0, size=(n, 3)) * np.array([1.0, 0.7, 0.4])
    if planar:
        x[:, 2] = 0.0
    y = s * x @ R.T + t
    if mirrored:
        y = y * np.array([1.0, 1.0, -1.0])
    y = y + rng.normal(size=(n, 3)) * noise
    return x + offset, y - 0.7 * offset, (s, R, t)


def make_table(seed, sizes, weighted_zero_every=11, **kw):
    """-> dict(src, dst, start, weights, size (P,) the diagonal of every problem's dst box (1 for an empty one), truth)."""
    rng = np.random.default_rng(seed)
    src, dst, truth, size = [], [], [], []
    for n in sizes:
        x, y, tr = make_problem(rng, n, **kw)
        src.append(x), dst.append(y), truth.append(tr)
        size.append(float(np.linalg.norm(y.max(axis=0) - y.min(axis=0))) if n else 1.0)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    w = rng.uniform(0.5, 2.0, size=int(start[-1]))
    w[::weighted_zero_every] = 0.0          # weight 0: the row takes no part
    for j, n in enumerate(sizes):           # ... but every problem keeps three rows
        if n and np.sum(w[start[j]:start[j + 1]] > 0) < 3:
            w[start[j]:start[j + 1]] = 1.0
    return {"src": np.concatenate(src).reshape(-1, 3), "dst": np.concatenate(dst).reshape(-1, 3), "start": start, "weights": w,
            "size": np.array(size), "truth": truth}


def parity_inputs():
    """name -> table.  'batch': 37 problems of every size; 'single': one problem; 'planar', 'mirrored', 'offset': the special sets."""
    sizes = [SIZES[i % len(SIZES)] for i in range(N_PROBLEMS)]
    special = [3, 16, 65, 257]
    return {"batch": make_table(11, sizes), "single": make_table(12, [65]), "planar": make_table(13, special, planar=True),
            "mirrored": make_table(14, special, mirrored=True), "offset": make_table(15, special, offset=1e6)}


# ---- consensus ------------------------------------------------------------------------------------------------------------------------
CONSENSUS_SIZES = [3, 20, 0, 40, 64, 100, 257]
INLIER_DIST = 0.02     # 20 sigma of the noise: no clean row comes near it
OUTLIER_FRACTION = 0.3
HYPOTHESES = (1, 16, 17, 64)
SEED = 5


def consensus_inputs():
    """name -> table.  'clean': every row an inlier; 'outliers': 30 % of the rows of every problem of 20 rows or more replaced by
    points anywhere in a box three times the scene (``outlier`` (n,) bool says which)."""
    clean = make_table(21, CONSENSUS_SIZES, scale_range=(1.0, 1.0))   # scale 1: both models fit within INLIER_DIST
    dirty = make_table(22, CONSENSUS_SIZES, scale_range=(1.0, 1.0))
    rng = np.random.default_rng(23)
    bad = np.zeros(dirty["src"].shape[0], dtype=bool)
    for j, n in enumerate(CONSENSUS_SIZES):
        if n >= 20:
            a = int(dirty["start"][j])
            pick = rng.choice(n, size=int(round(OUTLIER_FRACTION * n)), replace=False)
            bad[a + pick] = True
            centre = dirty["dst"][a:a + n].mean(axis=0)
            dirty["dst"][a + pick] = centre + rng.uniform(-3.0, 3.0, size=(pick.shape[0], 3)) * dirty["size"][j]
    clean["outlier"], dirty["outlier"] = np.zeros(clean["src"].shape[0], dtype=bool), bad
    return {"clean": clean, "outliers": dirty}


# ---- statuses -------------------------------------------------------------------------------------------------------------------------
def status_inputs():
    """A table whose problems are, in order: good, 0 rows, 1 row, 2 rows, good, collinear, good with one NaN row, NaN only, good;
    ``expected`` their statuses (align_reference codes) and ``good`` the indices of the good ones."""
    from tests import align_reference as ref

    rng = np.random.default_rng(31)
    parts, expected = [], []

    def good(n):
        x, y, _ = make_problem(rng, n)
        parts.append((x, y)), expected.append(ref.OK)

    def few(n):
        x, y, _ = make_problem(rng, n)
        parts.append((x, y)), expected.append(ref.TOO_FEW)

    good(17), few(0), few(1), few(2), good(5)
    s, R, t = random_transform(rng)
    line = np.array([0.3, -0.2, 0.5]) + np.arange(9)[:, None] * np.array([0.25, 0.5, -0.125])   # exactly collinear in binary
    parts.append((line, s * line @ R.T + t)), expected.append(ref.DEGENERATE)
    x, y, _ = make_problem(rng, 33)
    x[7, 1] = np.nan
    parts.append((x, y)), expected.append(ref.OK)
    parts.append((np.full((6, 3), np.nan), np.full((6, 3), np.nan))), expected.append(ref.NONFINITE)
    good(64)
    sizes = [p[0].shape[0] for p in parts]
    return {"src": np.concatenate([p[0] for p in parts]).reshape(-1, 3), "dst": np.concatenate([p[1] for p in parts]).reshape(-1, 3),
            "start": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), "expected": np.array(expected, dtype=np.int32),
            "good": [0, 4, 6, 8], "nan_row_problem": 6}


def sub_table(table, problems):
    """The table of the listed problems only (src, dst, start)."""
    rows = np.concatenate([np.arange(table["start"][j], table["start"][j + 1]) for j in problems]).astype(np.int64)
    sizes = [int(table["start"][j + 1] - table["start"][j]) for j in problems]
    return table["src"][rows], table["dst"][rows], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- the fixed sets of the reference golden (tests/golden/make_align_golden.py) ---------------------------------------------------------
def golden_sets():
    """name -> (v0, v1): general, planar and mirrored sets of 12 points for n_estimate_rigid_transform (rigid, unweighted, all finite)."""
    rng = np.random.default_rng(41)
    out = {}
    for name, kw in (("general", {}), ("planar", {"planar": True}), ("mirrored", {"mirrored": True})):
        x, y, (s, R, t) = make_problem(rng, 12, **kw)
        out[name] = (x, (y - t) / s + t)   # the rigid part of the motion: scale taken out about t
    return out


# ---- the front ends -------------------------------------------------------------------------------------------------------------------
def overlap_rig(noise_px=0.0):
    """Four ring cameras that all see a cube target of 96 features in six images: every feature of every image is triangulated."""
    from pycamset_amd import synthetic

    return synthetic.make_rig("align-rig", 4, 6, synthetic.ccube_points(5, 30.0), seed=71, noise_px=noise_px)


def gauge_state():
    """A self-calibration that sits away from its nominal target: the rig's true cameras and poses (pose 0 the identity) with the target's
    features scaled by 1.05, turned by 0.05 rad, shifted by 2 mm and moved by 10 um of noise each.  The residuals of such a state are
    not small; the gauge transform has to leave them as they are all the same.  -> (rig, extr, poses, points)."""
    from pycamset_amd import synthetic

    rig = synthetic.make_rig("align-gauge", 4, 6, synthetic.charuco_points(7, 8.0), seed=81, noise_px=0.3)
    rng = np.random.default_rng(82)
    R0 = Rotation.from_rotvec([0.03, -0.02, 0.035]).as_matrix()
    pts = 1.05 * rig.points_true @ R0.T + np.array([0.002, -0.001, 0.0015]) + rng.normal(size=rig.points_true.shape) * 1e-5
    return rig, rig.extr_true.copy(), rig.poses_true.copy(), pts


def oracle_residuals(rig, extr, poses, points):
    """The self chain's residual vector of a state through the NumPy oracle: the CPU closure of the gauge test."""
    from oracle import ba_oracle as orc
    from oracle import ba_oracle_np as onp

    ps = orc.build_param_list(rig.intr_true, extr, poses, points)
    return onp.evaluate("self", rig.detections, ps, None, counts=(rig.n_cams, rig.n_imgs, rig.n_keys), want_jac=False)[0]
