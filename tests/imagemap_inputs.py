"""Fixed inputs and pinned constants of the image-mapping tests (tests/test_imagemap_reference.py on the CPU, tests/test_gpu_imagemap.py
on the device).  Everything is fixed or drawn from fixed seeds; nothing here touches a device."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

# Three cameras, rows [fx, cx, fy, cy, k0, k1, p0, p1, k2]: mild distortion; strong barrel with tangential terms; none.  Camera 2 has
# dyadic intrinsics (powers of two and quarters), so that with it the identity properties hold exactly in binary floating point:
# (u - cx) / fx * fx + cx is u itself, on the device as in the restatement.
INTR = np.array([
    [58.3, 31.7, 57.1, 20.4, -0.08, 0.02, 0.001, -0.0015, -0.003],
    [41.0, 27.9, 43.5, 23.6, -0.28, 0.07, 0.012, -0.009, -0.008],
    [64.0, 29.25, 32.0, 20.5, 0.0, 0.0, 0.0, 0.0, 0.0],
])
N_CAMS = 3
# world -> camera [R | t], (3, 3, 4)
_POSES = np.array([[0.10, -0.20, 0.05, 0.3, -0.1, 1.2], [-0.25, 0.15, 0.30, -0.4, 0.2, 0.9], [0.05, 0.40, -0.10, 0.1, 0.5, 1.5]])
EXT = np.concatenate([Rotation.from_rotvec(_POSES[:, :3]).as_matrix(), _POSES[:, 3:, None]], axis=2)

SENSOR = (61, 43)                                   # (W, H) of every source image
DESTS = [(67, 45), (64, 4), (5, 3), (1, 1)]         # (Wd, Hd): widths 3, 0, 1, 1 mod 4, below and above 64, larger than the source
BATCH_CAMS = [2, 0, 2, 1, 0]                        # camera of every image of the batch
CHANNELS = (1, 3)
DTYPES = ("uint8", "float32")
PITCH_PAD = (0, 5)                                  # bytes (uint8) or elements (float32) added to every row; 5 leaves odd rows off the dword


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    return Rotation.from_rotvec(a / np.linalg.norm(a) * np.deg2rad(deg)).as_matrix()


def views():
    """name -> (R_new (3, 3, 3) or None, K_new (3, 4) or None), per camera.
    identity: the camera itself (cv2.undistort).  shift_zoom: 0.6 of the focal length and a shifted centre, so that source coordinates fall
    below 0, in (-1, 0), in (Ws - 2, Ws - 1] and wholly outside.  rot7: 7 degrees about an oblique axis.  past90: 75 degrees about an axis
    near y, which with the half field of view of the cameras puts one side of the image behind the source camera (Z <= 0)."""
    K = INTR[:, :4]
    zoom = K * np.array([0.6, 1.0, 0.6, 1.0]) + np.array([0.0, 3.37, 0.0, 1.73])
    r7 = np.stack([_rot([0.6, -0.7, 0.41], 7.0)] * N_CAMS)
    r75 = np.stack([_rot([0.1, 1.0, 0.05], 75.0)] * N_CAMS)
    return {"identity": (None, None), "shift_zoom": (None, zoom), "rot7": (r7, None), "past90": (r75, None)}


def images(dtype: str, C: int):
    """(5, H, W, C): a fixed pseudo-random field plus a ramp (a smooth image hides tap-order mistakes).  uint8 in [0, 255]; float32 in
    about [-1, 3], not on any coarse grid."""
    W, H = SENSOR
    rng = np.random.default_rng(20260 + C)
    n = len(BATCH_CAMS)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (xx / (W - 1) + 0.5 * yy / (H - 1))[None, :, :, None] + 0.1 * np.arange(n)[:, None, None, None] + 0.05 * np.arange(C)[None, None, None, :]
    field = rng.uniform(0.0, 1.0, size=(n, H, W, C))
    img = 0.6 * field + 0.4 * ramp / 1.7
    if dtype == "uint8":
        return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
    return (4.0 * img - 1.0).astype(np.float32)


def image_range(dtype: str) -> float:
    return 255.0 if dtype == "uint8" else 4.0


BORDER = {"uint8": (37.0, 201.0, 90.0), "float32": (0.625, -0.3, 2.2)}


def points():
    """(n, 2) pixels for the point kernels: a grid over the sensor and its margin plus a few fixed off-grid ones."""
    W, H = SENSOR
    gx, gy = np.meshgrid(np.linspace(-2.0, W + 1.0, 9), np.linspace(-1.5, H + 0.5, 7))
    rng = np.random.default_rng(77)
    extra = rng.uniform([0, 0], [W - 1, H - 1], size=(37, 2))
    return np.concatenate([np.stack([gx.ravel(), gy.ravel()], axis=1), extra])   # 100 points


def depth_image():
    """(H, W) depths with a NaN, an inf and a negative value."""
    W, H = SENSOR
    d = np.random.default_rng(5).uniform(0.5, 3.0, size=(H, W))
    d[3, 7], d[10, 2], d[20, 40] = np.nan, np.inf, -1.25
    return d


# Largest float64-versus-extended difference of the restatement (tests/imagemap_reference.py) over these inputs, per output kind:
# (point in px, ray component, map coordinate in px, interpolated value relative to the image's range).  A map coordinate far outside
# the source (the view turned past 90 degrees sends some to 1e15) is measured relative to its own size: see map_scale.
# tests/test_imagemap_reference.py::test_imagemap_gap_is_the_pinned_one recomputes it.  The device is held to 8 x these.
# Measured: (4.517e-14, 1.556e-15, 5.595e-11, 1.220e-13).  The point figure comes from the strong barrel camera after one step, the map
# figure from the view turned past 90 degrees, where the radial polynomial is steep; the other views stay below 3e-14 px.
IMAGEMAP_GAP = (4.6e-14, 1.6e-15, 5.6e-11, 1.3e-13)

# Largest difference between torch's grid_sample on the CPU (float32 arithmetic on normalised coordinates, align_corners=True, zero
# padding) and the restatement's remap of the float32 images over the restatement's float64 maps, relative to the image's range, as
# (bilinear, bicubic).  tests/test_imagemap_reference.py::test_grid_sample_agrees_with_the_restatement recomputes it.
# Measured: (5.30e-6, 5.72e-6): a float32 coordinate near 60 px has an ulp of 4e-6 px, and neighbouring pixels differ by the range.
GRID_SAMPLE_GAP = (5.4e-6, 5.8e-6)


def map_scale(coord):
    """What a map coordinate's error is measured in: pixels within a few sensor sizes, and in units of |coordinate| / 64 beyond."""
    with np.errstate(invalid="ignore"):
        return np.maximum(1.0, np.abs(np.asarray(coord, dtype=np.float64)) / 64.0)


def near_tie_mask(raw, gap_value: float):
    """Where an unrounded 8-bit value lies within ``gap_value`` of a half-integer: the only pixels on which two correct float64
    evaluations may round to different grey levels (and then by one)."""
    r = np.asarray(raw, dtype=np.float64)
    return np.abs(r - np.floor(r) - 0.5) <= gap_value


def flip_values(interpolation: str, size: int):
    """The source coordinates along one axis of ``size`` pixels at which a tap enters or leaves the source: where the validity flag
    and the border's share flip."""
    if interpolation == "nearest":
        return (-0.5, size - 0.5)
    if interpolation == "bilinear":
        return (-1.0, 0.0, size - 1.0, float(size))
    return (-2.0, -1.0, 0.0, 1.0, size - 2.0, size - 1.0, float(size), size + 1.0)
