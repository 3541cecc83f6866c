#!/usr/bin/env python3
"""Parameters shared across cameras, images or keys in generated chains (param_type's mod_function / key_type.SINGLE):

  (1) ONE lens model for every camera        projection[SINGLE] + extrinsic3D + template_points
  (2) a turntable: image i has the pose of position i mod n
                                              projection + extrinsic3D + template_points[img -> i % n]
  (3) a target made of rigid boards — the six faces of the reference's Ccube (calibration_targets/shape_by_faces.py): one small
      transform per FACE between the rigid template and free points, as a user block whose key-linked group is shared per face
                                              projection + extrinsic3D + rigidTform3d + face_transform[key -> k // points_per_face]

Each is solved with pycamset_amd.device_solver.lm_solve from a start near the truth of a synthetic rig whose parameters are
genuinely shared.  The tables are evaluated on the host, once per engine; the kernels look the group up per detection.

    python examples/shared_parameters.py

Needs an MI355X."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pycamset_amd import function_blocks as fb
from pycamset_amd import handlers, synthetic
from pycamset_amd.device_solver import lm_solve, parameter_covariance


def face_transform(points_per_face):
    class face_transform(fb.device_function_block):
        """out = R(params[0:3]) inp + params[3:6]: a rigid transform of the template point, one set of six per FACE."""
        template = True                     # the last block of the chain: `inp` is the detection's template point
        num_inp, num_out, array_memory = 0, 3, 0
        params = fb.param_type(fb.key_type.PER_KEY, 6, lambda k: k // points_per_face)
        # pcs::rot_terms / pcs::rot_element: the library's Rodrigues rotation (csrc/ba_device.hpp) — element q < 9 of R, 9 + 9 a + 3 row + col of dR / dr_a
        device_fun = """const pcs::RotTerms t = pcs::rot_terms(params[0], params[1], params[2]);
        for (int r = 0; r < 3; ++r)
            out[r] = pcs::rot_element(t, 3 * r) * inp[0] + pcs::rot_element(t, 3 * r + 1) * inp[1] + pcs::rot_element(t, 3 * r + 2) * inp[2] + params[3 + r];"""
        device_jac = """const pcs::RotTerms t = pcs::rot_terms(params[0], params[1], params[2]);
        for (int r = 0; r < 3; ++r)
            for (int a = 0; a < 3; ++a) {
                out[6 * r + a] = pcs::rot_element(t, 9 + 9 * a + 3 * r) * inp[0] + pcs::rot_element(t, 10 + 9 * a + 3 * r) * inp[1]
                                 + pcs::rot_element(t, 11 + 9 * a + 3 * r) * inp[2];
                out[6 * r + 3 + a] = r == a ? 1.0 : 0.0;
            }"""

    return face_transform()


def solve(title, blocks, rig, truth, masks, rng):
    """Measurements = the exact projection of `truth` + 0.3 px noise; start = truth perturbed by 1e-3; then lm_solve."""
    counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
    op = fb.optimisation_function(blocks, counts=counts)
    uv = op.make_full_loss_fn(rig.detections, 1)(op.build_param_list(*truth), rig.points) + rig.detections[:, 3:]
    det = rig.detections.copy()
    det[:, 3:] = uv + rng.normal(0, 0.3, uv.shape)
    start = [t + 1e-3 * rng.standard_normal(t.shape) * (np.abs(t) if i == 0 else 1.0) for i, t in enumerate(truth)]
    for s, t, m in zip(start, truth, masks):
        if m is not None:
            s[~m] = t[~m]
    prob = handlers.ChainProblem(fb.optimisation_function(blocks, counts=counts), det, start, template=rig.points, unfixed=masks)
    res = lm_solve(prob, prob.x0.copy(), max_iter=40)
    cov = parameter_covariance(prob, res.x)
    rms = np.sqrt(2 * res.cost / det.shape[0])
    print(f"{title}: {prob.x0.size} unknowns, {det.shape[0]} detections, {res.nfev} evaluations, rms {rms:.3f} px, largest standard error {cov.std.max():.2e}")
    return prob.get_bundle_adjustment_inputs(res.x)


def main():
    rng = np.random.default_rng(1)
    board = synthetic.make_rig("board", 4, 12, synthetic.charuco_points(9, 8.0), seed=3, visibility=0.9)
    gauge = np.ones((4, 6), dtype=bool)
    gauge[0] = False                                                   # camera 0 stays where it is
    # (1) four identical cameras: nine intrinsics for all of them, extrinsics per camera
    lens = fb.projection()
    lens.params = fb.param_type(fb.key_type.SINGLE, 9)
    solve("one lens for four cameras ", [lens, fb.extrinsic3D(), fb.template_points()], board,
          [board.intr_true[:1], board.extr_true, board.poses_true], [None, gauge, None], rng)
    # (2) a turntable with four positions, photographed three times round
    table = fb.template_points()
    table.params = fb.param_type(fb.key_type.PER_IMG, 6, lambda i: i % 4)
    solve("turntable, 12 images of 4  ", [fb.projection(), fb.extrinsic3D(), table], board,
          [board.intr_true, board.extr_true, board.poses_true[:4]], [None, gauge, None], rng)
    # (3) the cube as six rigid faces: 36 unknowns for the target (30 free: face 0 is the gauge against the pose) instead of three per corner
    n = 6
    cube = synthetic.make_rig("cube", 4, 10, synthetic.ccube_points(n), seed=4, visibility=0.9)
    faces = np.concatenate([rng.normal(0, 0.01, (6, 3)), rng.normal(0, 0.0005, (6, 3))], axis=1)
    faces[0] = 0.0
    free_face = np.ones((6, 6), dtype=bool)
    free_face[0] = False
    out = solve("cube of six rigid faces    ", [fb.projection(), fb.extrinsic3D(), fb.rigidTform3d(), face_transform((n - 1) ** 2)], cube,
                [cube.intr_true, cube.extr_true, cube.poses_true, faces], [None, gauge, None, free_face], rng)
    print(f"    face transforms recovered to {np.max(np.abs(out[3] - faces)):.2e} (rotation vector / metres)")


if __name__ == "__main__":
    main()
