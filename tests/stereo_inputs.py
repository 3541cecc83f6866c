"""Fixed inputs of the stereo tests, from seeded generators: nothing is committed but this code."""
import numpy as np

DEFAULTS = dict(num_disp=32, block=7, min_disp=0, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=15)
# The float64-versus-longdouble gap of the reprojection over cloud_inputs(): the largest |float64 - longdouble| coordinate over the
# masked points, relative to the largest coordinate.  tests/test_stereo_reference.py recomputes it.
STEREO_GAP = 1.6e-16
DEPTH_RANGE = (0.5, 2.0)


def _smooth_noise(rng, H, W):
    a = rng.uniform(0.0, 255.0, size=(H + 2, W + 2))
    a = (a[:-2] + 2.0 * a[1:-1] + a[2:]) / 4.0
    a = (a[:, :-2] + 2.0 * a[:, 1:-1] + a[:, 2:]) / 4.0
    return np.clip((a - 127.5) * 2.0 + 127.5, 0.0, 255.0)


def _disparity_map(H, W):
    """Two planes, 6 px and 13.5 px, and inside the near plane a band 4 px nearer still: its edge occludes."""
    d = np.full((H, W), 6.0)
    d[:, W // 2:] = 13.5
    d[H // 4:3 * H // 4, 5 * W // 8:6 * W // 8] = 17.5
    return d


def textured_pair(H=40, W=160, seed=20261, noise=2.0):
    """-> (L, R) uint8 (H, W): the left image is the right one seen through the disparity map, sensor noise on both; a noise-free flat
    patch and a patch of period-8 stripes lie in the 6 px plane."""
    rng = np.random.default_rng(seed)
    pad = 32
    scene = _smooth_noise(rng, H, W + pad)   # the right image, with room to the left of column 0
    y0, y1, x0, x1 = H // 4, 3 * H // 4, W // 8, W // 8 + 26
    scene[y0:y1, pad + x0 - 6:pad + x1 - 6] = 128.0                                            # the flat patch, as the right image sees it
    sx0, sx1 = W // 4 + 8, W // 4 + 38
    scene[y0 - 4:y1 + 4, pad + sx0 - 6:pad + sx1 - 6] = np.where((np.arange(sx0, sx1) // 4) % 2 == 0, 60.0, 200.0)[None, :]   # period 8
    d = _disparity_map(H, W)
    xs = np.arange(W)[None, :] + pad - d
    i0 = np.floor(xs).astype(int)
    f = xs - i0
    rows = np.arange(H)[:, None]
    Lf = scene[rows, i0] * (1.0 - f) + scene[rows, i0 + 1] * f
    Rf = scene[:, pad:].copy()
    nL, nR = rng.normal(0.0, noise, size=(H, W)), rng.normal(0.0, noise, size=(H, W))
    nL[y0:y1, x0:x1] = 0.0
    nR[y0:y1, x0 - 6:x1 - 6] = 0.0
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to8(Lf + nL), to8(Rf + nR)


def wide_pair(H=48, W=352, seed=20262):
    """A wider generated pair for the reference's own parameters (block 25, 256 disparities): disparities between 20 and 60 px."""
    rng = np.random.default_rng(seed)
    pad = 80
    scene = _smooth_noise(rng, H, W + pad)
    d = 20.0 + 40.0 * (np.arange(W)[None, :] / (W - 1.0)) * np.ones((H, 1))
    xs = np.arange(W)[None, :] + pad - d
    i0 = np.floor(xs).astype(int)
    f = xs - i0
    rows = np.arange(H)[:, None]
    Lf = scene[rows, i0] * (1.0 - f) + scene[rows, i0 + 1] * f
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to8(Lf + rng.normal(0.0, 1.5, size=(H, W))), to8(scene[:, pad:] + rng.normal(0.0, 1.5, size=(H, W)))


def constant_pair(H=12, W=48, value=97):
    return np.full((H, W), value, dtype=np.uint8), np.full((H, W), value, dtype=np.uint8)


def shifted_pair(d0, H=24, W=96, seed=20263):
    """Noise-free: R(x) = L(x + d0)."""
    rng = np.random.default_rng(seed)
    scene = np.rint(_smooth_noise(rng, H, W + abs(d0))).astype(np.uint8)
    if d0 >= 0:
        return scene[:, :W].copy(), scene[:, d0:d0 + W].copy()
    return scene[:, -d0:-d0 + W].copy(), scene[:, :W].copy()


def holes(shape, seed=20264, frac=0.08):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=shape) >= frac).astype(np.uint8), (rng.uniform(size=shape) >= frac).astype(np.uint8)


def cloud_inputs(n=3, H=21, W=37, seed=20265):
    """-> (disp (n, H, W) int16, Q (n, 4, 4), T (3, 4), invalid): disparity planes whose depths Z = f B / d straddle DEPTH_RANGE, pair 0
    with invalid pixels sprinkled in, pair 1 entirely outside the range (no survivor), pair 2 entirely inside (all survive)."""
    rng = np.random.default_rng(seed)
    f, B = 400.0, 0.1
    Q = np.zeros((n, 4, 4))
    for i in range(n):
        cx, cy = (W - 1) / 2.0 + 0.25 * i, (H - 1) / 2.0 - 0.5 * i
        Q[i] = [[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f + i], [0.0, 0.0, 1.0 / B, 0.0]]
    invalid = 16 * -1
    disp = np.zeros((n, H, W), dtype=np.int16)
    xs, ys = np.arange(W)[None, :], np.arange(H)[:, None]
    # pair 0: Z from 0.3 to 3: d = f B / Z between 13 and 133 px, in sixteenths, a tilted plane
    d0 = 13.4 + (133.0 - 13.4) * (xs + 0.37 * ys) / (W - 1 + 0.37 * (H - 1))
    disp[0] = np.rint(16.0 * d0).astype(np.int16)
    disp[0][rng.uniform(size=(H, W)) < 0.1] = invalid
    disp[0][0, 0] = 0   # Wh = 0: a point at infinity
    disp[1] = np.rint(16.0 * (5.0 + 0.05 * xs + 0.0 * ys)).astype(np.int16)     # Z about 6 to 8: beyond the range
    disp[2] = np.rint(16.0 * (30.0 + 0.5 * xs + 0.25 * ys)).astype(np.int16)    # Z about 0.75 to 1.35: inside
    a = 0.3
    T = np.array([[np.cos(a), 0.0, np.sin(a), 0.2], [0.0, 1.0, 0.0, -0.1], [-np.sin(a), 0.0, np.cos(a), 1.5]])
    return disp, Q, T, invalid
