"""Chains with SHARED parameter groups (param_type's mod_function / key_type.SINGLE) for tests/test_shared_params.py and
tests/test_gpu_shared_params.py, and the 0/1 matrix S that sends the columns of a shared group to the columns of its entities.

The expected values need no oracle of their own: a detection has one camera, one image and one key, so the Jacobian of the shared
chain is, entry for entry, J_full S (no sums inside a row), and its residual is the un-shared chain's at the expanded parameters."""
import numpy as np

FACE_FUN = """const pcs::RotTerms t = pcs::rot_terms(params[0], params[1], params[2]);
        for (int r = 0; r < 3; ++r)
            out[r] = pcs::rot_element(t, 3 * r) * inp[0] + pcs::rot_element(t, 3 * r + 1) * inp[1] + pcs::rot_element(t, 3 * r + 2) * inp[2] + params[3 + r];"""
FACE_JAC = """const pcs::RotTerms t = pcs::rot_terms(params[0], params[1], params[2]);
        for (int r = 0; r < 3; ++r)
            for (int a = 0; a < 3; ++a) {
                out[6 * r + a] = pcs::rot_element(t, 9 + 9 * a + 3 * r) * inp[0] + pcs::rot_element(t, 10 + 9 * a + 3 * r) * inp[1]
                                 + pcs::rot_element(t, 11 + 9 * a + 3 * r) * inp[2];
                out[6 * r + 3 + a] = r == a ? 1.0 : 0.0;
            }"""


def face_transform(fb, table=None):
    """The worked example of function_blocks.device_function_block: a rigid transform of the template point, PER_KEY, shared per
    face through ``table`` (None: one transform per key, the un-mapped chain the shared one is compared with)."""

    class face_transform(fb.device_function_block):
        template = True
        num_inp, num_out, array_memory = 0, 3, 0
        params = fb.param_type(fb.key_type.PER_KEY, 6, table)
        device_fun = FACE_FUN
        device_jac = FACE_JAC

    return face_transform()


def with_params(block, params):
    block.params = params          # shipped blocks take their sharing by instance
    return block


def chain_blocks(fb, which, table=None):
    """(a) projection[SINGLE] + extrinsic3D + template_points          (b) projection[cam -> table] + extrinsic3D + rigidTform3d + free_point
    (c) projection + extrinsic3D + template_points[img -> table]       (d) projection + extrinsic3D + rigidTform3d + face_transform[key -> table]
    (e) projection[SINGLE] + extrinsic3D + rigidTform3d + free_point: SINGLE next to key-linked columns.
    ``which`` in upper case: the same composition without sharing."""
    K = fb.key_type
    shared = which.islower()
    w = which.lower()
    if w in ("a", "e"):
        p = with_params(fb.projection(), fb.param_type(K.SINGLE, 9)) if shared else fb.projection()
        return [p, fb.extrinsic3D(), fb.template_points()] if w == "a" else [p, fb.extrinsic3D(), fb.rigidTform3d(), fb.free_point()]
    if w == "b":
        p = with_params(fb.projection(), fb.param_type(K.PER_CAM, 9, table)) if shared else fb.projection()
        return [p, fb.extrinsic3D(), fb.rigidTform3d(), fb.free_point()]
    if w == "c":
        t = with_params(fb.template_points(), fb.param_type(K.PER_IMG, 6, table)) if shared else fb.template_points()
        return [fb.projection(), fb.extrinsic3D(), t]
    if w == "d":
        return [fb.projection(), fb.extrinsic3D(), fb.rigidTform3d(), face_transform(fb, table if shared else None)]
    raise ValueError(which)


def expansion(spec, counts):
    """``src`` (n_full,) with x_full = x_shared[src], and S (n_full x n_shared, 0/1) = the matrix that sends group columns to entity
    columns, for a ChainSpec with shared groups and the entity counts (n_cams, n_imgs, n_keys)."""
    lay = spec.layout(*counts)
    src = []
    for g, start, table in zip(spec.groups, lay["starts"], lay["tables"]):
        n = counts[g["link"]]
        t = np.arange(n) if table is None else np.asarray(table, dtype=np.int64)
        src.append((start + g["n_params"] * t[:, None] + np.arange(g["n_params"])[None, :]).ravel())
    src = np.concatenate(src)
    S = np.zeros((src.shape[0], lay["n_params"]))
    S[np.arange(src.shape[0]), src] = 1.0
    return src, S
