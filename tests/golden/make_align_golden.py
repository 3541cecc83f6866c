#!/usr/bin/env python3
"""Generate tests/golden/rigid_transform.npz from the reference itself: ``n_estimate_rigid_transform``
(optimisation/compiled_helpers.py:727-762) on the fixed general, planar and mirrored sets of ``tests/align_inputs.golden_sets``.

TEST INFRASTRUCTURE (build container only: it needs the reference checkout that ``_refload`` finds; nothing under tests/ -m gpu,
smoke() or bench.py runs this).  The reference's module is imported from a temporary copy (``_refload.reference_modules``) and only its
inputs and outputs, (v0, v1) and (R, t), are stored: a few KB.

Run:  python tests/golden/make_align_golden.py
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

from tests.align_inputs import golden_sets  # noqa: E402


def main() -> None:
    out = {}
    with _refload.reference_modules() as ref:
        for name, (v0, v1) in golden_sets().items():
            R, t = ref.ch.n_estimate_rigid_transform(np.array(v0), np.array(v1))
            out[f"{name}_v0"], out[f"{name}_v1"], out[f"{name}_R"], out[f"{name}_t"] = v0, v1, np.asarray(R), np.asarray(t)
    path = HERE / "rigid_transform.npz"
    np.savez(path, **out)
    print(f"{path}: {sorted(out)} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
