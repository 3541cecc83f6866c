#!/usr/bin/env python3
"""Generate tests/golden/view_pairs.npz from the reference itself: ``calc_pairs(c_vec, ReconParams(...), pick_closest=True)``
(reconstruction/acmmp_utils.py:47-83) on a few seeded sets of view vectors and limits.

TEST INFRASTRUCTURE (build container only: it needs the reference checkout that ``_refload`` finds; nothing under tests/ -m gpu,
smoke() or bench.py runs this).  The reference's module is imported from the temporary copy ``_refload.reference_modules`` makes and
only its inputs and outputs are stored: a few KB.  ``acmmp_utils`` needs nothing but NumPy; it is loaded from its file in that copy, so
that the ``reconstruction`` package's own imports (cv2, pyvista) are not needed.

The reference's ``argsort`` is not stable, so tied angles would leave its answer to chance: every set is checked to have no two
candidate angles of one view closer than 1e-9 degrees and no angle that close to a limit.

Run:  python tests/golden/make_pairs_golden.py
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _refload  # noqa: E402

# (seed, views, spread of the directions about +z in degrees, min angle, max angle, max views)
SETS = ((41, 12, 30.0, 3.0, 45.0, 9), (42, 24, 25.0, 3.0, 45.0, 9), (43, 16, 60.0, 5.0, 40.0, 4), (44, 9, 15.0, 2.0, 20.0, 32), (45, 20, 8.0, 3.0, 45.0, 6))


def view_vectors(seed, n, spread):
    """Seeded directions about +z, NOT normalised (calc_pairs normalises its argument in place)."""
    rng = np.random.default_rng(seed)
    a = np.radians(spread) * np.sqrt(rng.uniform(size=n))
    b = rng.uniform(0.0, 2.0 * np.pi, size=n)
    v = np.stack([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)], axis=1)
    return v * rng.uniform(0.5, 2.0, size=(n, 1))


def check_no_ties(v, lo, hi):
    u = v / np.linalg.norm(v, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(u @ u.T, -1.0, 1.0)))
    for i in range(len(u)):
        a = np.sort(np.delete(ang[i], i))
        assert np.all(np.diff(a) > 1e-9), "tied angles"
        assert np.all(np.abs(a - lo) > 1e-9) and np.all(np.abs(a - hi) > 1e-9), "an angle at a limit"


def main() -> None:
    out = {"sets": np.array(SETS, dtype=np.float64)}
    with _refload.reference_modules() as ref:
        spec = importlib.util.spec_from_file_location("_pcs_ref_acmmp_utils", ref.root / "pyCamSet" / "reconstruction" / "acmmp_utils.py")
        acmmp = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(acmmp)
        for s, (seed, n, spread, lo, hi, mv) in enumerate(SETS):
            v = view_vectors(seed, n, spread)
            check_no_ties(v, lo, hi)
            lists = acmmp.calc_pairs(v.copy(), acmmp.ReconParams(minangle=lo, maxangle=hi, max_n_view=mv), pick_closest=True)
            padded = np.full((n, mv), -1, dtype=np.int32)
            for i, l in enumerate(lists):
                padded[i, :len(l)] = l
            out[f"vectors_{s}"], out[f"lists_{s}"] = v, padded
            print(f"set {s}: {n} views, list lengths {[len(l) for l in lists]}")
    path = HERE / "view_pairs.npz"
    np.savez(path, **out)
    print(f"{path}: {sorted(out)} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
