#!/usr/bin/env python3
"""Generate tests/golden/mvsnet_depth_lines.npz from the reference itself: the last line ``Camera.to_MVSnet_txt`` writes,
``depth_min interval steps depth_max`` (cameras/camera.py:158-159), for a few depth ranges and step counts.

TEST INFRASTRUCTURE (build container only: it needs the reference checkout that ``_refload`` finds; nothing under tests/ -m gpu,
smoke() or bench.py runs this).  The reference's ``Camera`` is imported from the temporary copy ``_refload.reference_modules`` makes
and only the numbers of the written line are stored (Python prints a float so that it reads back exactly): a few hundred bytes.

Run:  python tests/golden/make_mvsnet_golden.py
"""
from __future__ import annotations

import importlib
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _refload  # noqa: E402

# (depth_min, depth_max, steps): the reference's default step count, the accuracy test's range, and ranges whose interval is inexact
SETS = ((0.8, 1.2, 32), (0.5, 2.0, 192), (0.3, 1.7, 7), (1.0, 1.1, 3), (2.0, 3.2, 1), (0.123, 4.567, 1024))


def main() -> None:
    lines = []
    with _refload.reference_modules():
        camera = importlib.import_module("pyCamSet.cameras.camera")
        cam = camera.Camera(extrinsic=np.eye(4), intrinsic=np.array([[100.0, 0.0, 50.0], [0.0, 100.0, 40.0], [0.0, 0.0, 1.0]]), res=np.array([96, 64]))
        with tempfile.TemporaryDirectory() as tmp:
            for lo, hi, steps in SETS:
                path = Path(tmp) / "cam.txt"
                cam.to_MVSnet_txt(path, (lo, hi), steps)
                last = path.read_text().strip().splitlines()[-1].split()
                assert len(last) == 4 and int(last[2]) == steps, last
                lines.append([float(v) for v in last])
                print(lo, hi, steps, "->", last)
    out = HERE / "mvsnet_depth_lines.npz"
    np.savez(out, sets=np.array(SETS, dtype=np.float64), lines=np.array(lines, dtype=np.float64))
    print(f"{out}: {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
