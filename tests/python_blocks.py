"""The user blocks of tests/golden/_user_blocks.py with PYTHON bodies, declared on pycamset_amd's own ABC.

tests/golden/_user_blocks.py writes these three blocks on the reference's ABC (with numba decorators) for the golden generator;
tests/helpers.py declares hand-translated twins as device strings.  Here the same bodies are plain Python, as a pyCamSet user's
block would be after dropping the numba import: pycamset_amd/block_translate.py turns them into device code.
"""
import numpy as np

from pycamset_amd.function_blocks import abstract_function_block, key_type, param_type


class cam_scale(abstract_function_block):
    """One isotropic scale per camera, applied to the camera-frame point (between `projection` and `extrinsic3D`)."""
    num_inp = 3
    num_out = 3
    params = param_type(key_type.PER_CAM, 1)
    array_memory = 0

    @staticmethod
    def compute_fun(params, inp, output, memory=0):
        output[0] = params[0] * inp[0]
        output[1] = params[0] * inp[1]
        output[2] = params[0] * inp[2]

    @staticmethod
    def compute_jac(params, inp, output, memory=0):
        output[:12] = 0
        output[0] = inp[0]
        output[4] = inp[1]
        output[8] = inp[2]
        output[1] = params[0]
        output[6] = params[0]
        output[11] = params[0]


class division_projection(abstract_function_block):
    """Pinhole with the one-parameter division model of lens distortion, params = [fx, px, fy, py, lam]:
    (x, y) = (X / Z, Y / Z), d = 1 / (1 + lam (x^2 + y^2)), (u, v) = (fx x d + px, fy y d + py).  Replaces `projection`."""
    num_inp = 3
    num_out = 2
    params = param_type(key_type.PER_CAM, 5)
    array_memory = 0

    @staticmethod
    def compute_fun(params, inp, output, memory=0):
        iz = 1 / inp[2]
        x = inp[0] * iz
        y = inp[1] * iz
        d = 1 / (1 + params[4] * (x * x + y * y))
        output[0] = params[0] * x * d + params[1]
        output[1] = params[2] * y * d + params[3]

    @staticmethod
    def compute_jac(params, inp, output, memory=0):
        iz = 1 / inp[2]
        x = inp[0] * iz
        y = inp[1] * iz
        r2 = x * x + y * y
        d = 1 / (1 + params[4] * r2)
        d2 = d * d
        output[:16] = 0
        # row u: [fx, px, fy, py, lam | X, Y, Z]
        output[0] = x * d
        output[1] = 1
        output[4] = -params[0] * x * r2 * d2
        ux = params[0] * (d - 2 * params[4] * x * x * d2)
        uy = -2 * params[0] * params[4] * x * y * d2
        output[5] = ux * iz
        output[6] = uy * iz
        output[7] = -(x * ux + y * uy) * iz
        # row v
        output[8 + 2] = y * d
        output[8 + 3] = 1
        output[8 + 4] = -params[2] * y * r2 * d2
        vx = -2 * params[2] * params[4] * x * y * d2
        vy = params[2] * (d - 2 * params[4] * y * y * d2)
        output[8 + 5] = vx * iz
        output[8 + 6] = vy * iz
        output[8 + 7] = -(x * vx + y * vy) * iz


class board_flex(abstract_function_block):
    """A TEMPLATED user source: one flex model of the calibration board per image, params = [sx, sy, tx, ty, k]:
    out = [sx X + tx, sy Y + ty, Z + k (X^2 + Y^2)]  with (X, Y, Z) the template point."""
    template = True
    num_inp = 0
    num_out = 3
    params = param_type(key_type.PER_IMG, 5)
    array_memory = 0

    @staticmethod
    def compute_fun(params, inp, output, memory):
        output[0] = params[0] * inp[0] + params[2]
        output[1] = params[1] * inp[1] + params[3]
        output[2] = inp[2] + params[4] * (inp[0] * inp[0] + inp[1] * inp[1])

    @staticmethod
    def compute_jac(params, inp, output, memory):
        output[:15] = 0
        output[0] = inp[0]
        output[2] = 1
        output[5 + 1] = inp[1]
        output[5 + 3] = 1
        output[10 + 4] = inp[0] * inp[0] + inp[1] * inp[1]


def python_blocks():
    return {"cam_scale": cam_scale, "division_projection": division_projection, "board_flex": board_flex}


def chain_of(names, blocks=None):
    """Instances of a block-name list: user names from ``blocks`` (default: the Python-bodied ones), the rest shipped."""
    from pycamset_amd import function_blocks as fb

    blocks = python_blocks() if blocks is None else blocks
    return [blocks[n]() if n in blocks else getattr(fb, n)() for n in names]
