#!/usr/bin/env python3
"""Generate tests/golden/undistort_points.npz from the reference itself: ``nb_undistort_arr`` and ``nb_distort``
(optimisation/compiled_helpers.py:373-490) on the fixed points of ``tests/imagemap_inputs.points`` for its three cameras.

TEST INFRASTRUCTURE (build container only: it needs the reference checkout that ``_refload`` finds; nothing under tests/ -m gpu,
smoke() or bench.py runs this).  The reference's module is imported from a temporary copy (``_refload.reference_modules``) and only
its inputs and outputs are stored: a few KB.

``vector_cam_points`` lives in pyCamSet/utils/general_utils.py, which imports cv2 at module level; cv2 is not installed, so it cannot
be reached through the loaded modules and its rays are NOT part of the golden.  The ray kernels are checked against the restatement
and, through it, against the undistortion stored here.

Run:  python tests/golden/make_imagemap_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

import _refload  # noqa: E402

from tests import imagemap_inputs as inp  # noqa: E402


def main() -> None:
    pts = inp.points()
    out = {"points": pts, "intr": inp.INTR}
    with _refload.reference_modules() as ref:
        for c, row in enumerate(inp.INTR):
            K = np.array([[row[0], 0.0, row[1]], [0.0, row[2], row[3]], [0.0, 0.0, 1.0]])
            dist = np.array(row[4:9])
            out[f"undistort_{c}"] = np.asarray(ref.ch.nb_undistort_arr(pts.copy(), K, dist))
            out[f"distort_{c}"] = np.stack([np.asarray(ref.ch.nb_distort(p.copy(), K, dist)) for p in pts])   # it takes one point at a time
    path = HERE / "undistort_points.npz"
    np.savez(path, **out)
    print(f"{path}: {sorted(out)} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
