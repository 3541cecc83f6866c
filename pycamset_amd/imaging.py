"""A finished calibration applied to points and images on the device: rays, undistortion and rectified remap (include/pcs_hip.h
pcs_imap_*, csrc/ba_imagemap.hpp).

What the reference does with OpenCV and a full-resolution float64 sensor map per call — ``Camera._make_sensormap`` / ``undistort`` /
``im_to_world_ray`` (cameras/camera.py), ``nb_undistort_arr`` / ``nb_distort`` (optimisation/compiled_helpers.py), ``undistort_im`` /
``remap_im`` / ``rectify_camera_pair`` / ``rectify_camera_images`` (reconstruction/reconstruction_utils.py) — as kernels over the
library's own camera slabs: ``intr`` (C, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2] and ``ext`` (C, 3, 4) world -> camera (or (C, 6) =
[rotvec, t]).

Conventions.  Pixel coordinates are (x, y) = (column, row), the pixel centre at the integer.  Images are (n, H, W) or (n, H, W, C)
stacks (a single (H, W) image is taken as n = 1), C in {1, 3, 4}, uint8 or float32.  NumPy arrays are copied to the device and the
result comes back as a NumPy array; torch tensors on the device are used in place (a padded row pitch included) and the result is a
torch tensor on that device, or the ``out=`` tensor.  Maps are (2, Hd, Wd): plane 0 the source x, plane 1 the source y.

There is no CPU fallback: every function here needs the device, except ``rectify_pair`` with a caller-supplied ``undistort`` and the
argument checks, which raise ValueError before anything touches it."""
from __future__ import annotations

import numpy as np

from ._capi import IMAP_DISTORT, IMAP_DTYPE_IDS, IMAP_INTERP_IDS, IMAP_NO_DISTORT, IMAP_NORMALISED, IMAP_RAY, IMAP_UNDISTORT, IMAP_WORLD
from .compiled_helpers import _cached_handle, _Handle
from .engine import _stream_arg

CHANNELS = (1, 3, 4)
MAX_ITERS = 100
# undistort_images(method="auto"): the fused kernel.  Measured on the MI355X at 32 x 2448 x 2048 (profiles/r29): the fused form is
# never slower than reading a resident float32 map for 8-bit mono, and it needs no 8 B of map per pixel per camera to stay resident.
DEFAULT_METHOD = "fused"


# ---- argument checks (host only; ValueError names the offending argument) ------------------------------------------------------------
def check_intr(intr) -> np.ndarray:
    K = np.asarray(intr, dtype=np.float64)
    if K.ndim == 1:
        K = K[None, :]
    if K.ndim != 2 or K.shape[1] != 9 or K.shape[0] < 1:
        raise ValueError(f"intr: expected (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2], got shape {np.shape(intr)}")
    if not np.all(np.isfinite(K)) or np.any(K[:, 0] == 0) or np.any(K[:, 2] == 0):
        raise ValueError("intr: every entry must be finite and the focal lengths non-zero")
    return np.ascontiguousarray(K)


def check_ext(ext, n_cams: int):
    """-> (C, 12) rows [R | t] world -> camera, or None."""
    if ext is None:
        return None
    E = np.asarray(ext, dtype=np.float64)
    if E.ndim == 1 and n_cams == 1:
        E = E[None, :]
    if E.shape == (n_cams, 6):
        from scipy.spatial.transform import Rotation

        E = np.concatenate([Rotation.from_rotvec(E[:, :3]).as_matrix(), E[:, 3:, None]], axis=2)
    elif E.shape == (n_cams, 4, 4):
        E = E[:, :3, :]
    elif n_cams == 1 and E.shape in ((3, 4), (4, 4)):
        E = E[None, :3, :]
    if E.shape not in ((n_cams, 3, 4), (n_cams, 12)):
        raise ValueError(f"ext: expected ({n_cams}, 3, 4) world -> camera, ({n_cams}, 4, 4) or ({n_cams}, 6) = [rotvec, t], got shape {np.shape(ext)}")
    if not np.all(np.isfinite(E)):
        raise ValueError("ext: every entry must be finite")
    return np.ascontiguousarray(E.reshape(n_cams, 12))


def check_view(R_new, K_new, n_cams: int):
    R = K = None
    if R_new is not None:
        R = np.asarray(R_new, dtype=np.float64)
        if R.shape == (3, 3):
            R = np.broadcast_to(R, (n_cams, 3, 3))
        if R.shape != (n_cams, 3, 3) or not np.all(np.isfinite(R)):
            raise ValueError(f"R_new: expected finite ({n_cams}, 3, 3) or (3, 3), got shape {np.shape(R_new)}")
        R = np.ascontiguousarray(R.reshape(n_cams, 9))
    if K_new is not None:
        K = np.asarray(K_new, dtype=np.float64)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[0, 2], K[1, 1], K[1, 2]])
        if K.shape == (4,):
            K = np.broadcast_to(K, (n_cams, 4))
        if K.shape != (n_cams, 4) or not np.all(np.isfinite(K)) or np.any(K[:, 0] == 0) or np.any(K[:, 2] == 0):
            raise ValueError(f"K_new: expected finite ({n_cams}, 4) rows [fx, cx, fy, cy] with non-zero focal lengths (or (4,), or a 3 x 3 matrix), got shape {np.shape(K_new)}")
        K = np.ascontiguousarray(K)
    return R, K


def check_cams(cams, n: int, limit: int, name: str = "cams") -> np.ndarray:
    """One camera (or map) index per row: an int for all rows, or n of them, each in [0, limit)."""
    c = np.asarray(cams)
    if c.ndim == 0:
        c = np.full(n, c)
    if c.shape != (n,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"{name}: expected {n} integer indices (or one for all), got shape {np.shape(cams)} of {c.dtype}")
    if n and (c.min() < 0 or c.max() >= limit):
        bad = int(np.nonzero((c < 0) | (c >= limit))[0][0])
        raise ValueError(f"{name}: index {int(c[bad])} at position {bad} outside [0, {limit})")
    return np.ascontiguousarray(c, dtype=np.int32)


def check_interpolation(interpolation) -> int:
    if interpolation not in IMAP_INTERP_IDS:
        raise ValueError(f"interpolation: expected one of {sorted(IMAP_INTERP_IDS)}, got {interpolation!r}")
    return IMAP_INTERP_IDS[interpolation]


def check_size(size, name: str = "size"):
    try:
        W, H = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected (width, height), got {size!r}") from None
    if W < 1 or H < 1:
        raise ValueError(f"{name}: width and height must be >= 1, got {size!r}")
    return W, H


def check_remap_args(n_img: int, channels: int, dtype, src_size, src_pitch: int, dst_size, dst_pitch: int, interpolation):
    """The checks of pcs_imap_remap on the host: -> (dtype id, interpolation id).  Pitches are in bytes."""
    if channels not in CHANNELS:
        raise ValueError(f"channels (C): expected one of {CHANNELS}, got {channels}")
    name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
    if name not in IMAP_DTYPE_IDS:
        raise ValueError(f"dtype: images must be uint8 or float32, got {name}")
    item = 1 if name == "uint8" else 4
    (Ws, Hs), (Wd, Hd) = check_size(src_size, "src_size"), check_size(dst_size, "dst_size")
    if src_pitch < Ws * channels * item:
        raise ValueError(f"src_pitch: {src_pitch} bytes is below the row size {Ws * channels * item}")
    if dst_pitch < Wd * channels * item:
        raise ValueError(f"dst_pitch: {dst_pitch} bytes is below the row size {Wd * channels * item}")
    if item == 4 and (src_pitch % 4 or dst_pitch % 4):
        raise ValueError("src_pitch / dst_pitch: float32 rows must start on a multiple of 4 bytes")
    if not 0 <= n_img <= 65535:
        raise ValueError(f"images: at most 65535 per call, got {n_img}")
    return IMAP_DTYPE_IDS[name], check_interpolation(interpolation)


def _check_iters(iters) -> int:
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"iters: expected an integer in [0, {MAX_ITERS}], got {iters!r}")
    return int(iters)


def _ray_flags(mode: str, world: bool, distort: bool) -> int:
    if mode not in ("linear", "normalised"):
        raise ValueError(f"mode: expected 'linear' or 'normalised', got {mode!r}")   # the reference's "Invalid sensor map type"
    return (IMAP_NORMALISED if mode == "normalised" else 0) | (IMAP_WORLD if world else 0) | (0 if distort else IMAP_NO_DISTORT)


# ---- the handle ----------------------------------------------------------------------------------------------------------------------
class ImageMapper(_Handle):
    """Owner of one ``pcs_image_mapper`` handle (include/pcs_hip.h): the camera table stays on the device across calls; points, maps
    and images are raw device addresses (``tensor.data_ptr()``) used in place."""

    _create, _destroy = "pcs_imap_create", "pcs_imap_destroy"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.device, self.n_cams, self.have_ext = int(device), 0, False
        self._cam_key = self._view_key = None

    def set_cameras(self, intr, ext=None):
        K = check_intr(intr)
        E = check_ext(ext, K.shape[0])
        key = (K.tobytes(), None if E is None else E.tobytes())
        if key != self._cam_key:   # the same cameras across calls: nothing to upload
            self._call("pcs_imap_set_cameras", self._h, K.shape[0], self._ptr(K), self._ptr(E))
            self._cam_key, self._view_key = key, (None, None)
            self.n_cams, self.have_ext = K.shape[0], E is not None

    def set_view(self, R_new=None, K_new=None):
        R, K = check_view(R_new, K_new, self.n_cams)
        key = (None if R is None else R.tobytes(), None if K is None else K.tobytes())
        if key != self._view_key:
            self._call("pcs_imap_set_view", self._h, self._ptr(R), self._ptr(K))
            self._view_key = key

    def points(self, mode: int, n: int, d_in: int, d_out: int, d_cam: int | None = None, cam_all: int = 0, iters: int = 5, flags: int = 0, stream=None):
        self._call("pcs_imap_points", self._h, int(mode), int(n), self._addr(d_cam), int(cam_all), self._addr(d_in), int(iters), int(flags), self._addr(d_out),
                   _stream_arg(stream))

    def rays(self, cam: int, width: int, height: int, d_out: int, out_f32: bool = False, flags: int = 0, iters: int = 5, d_depth: int | None = None,
             depth_f32: bool = False, stream=None):
        self._call("pcs_imap_rays", self._h, int(cam), int(width), int(height), int(flags), int(iters), self._addr(d_depth), int(depth_f32), self._addr(d_out),
                   int(out_f32), _stream_arg(stream))

    def build_maps(self, cam: int, width: int, height: int, d_out: int, out_f32: bool = True, stream=None):
        self._call("pcs_imap_build_maps", self._h, int(cam), int(width), int(height), self._addr(d_out), int(out_f32), _stream_arg(stream))

    def remap(self, cams, d_src: int, src_size, channels: int, dtype, src_pitch: int, d_dst: int, dst_size, dst_pitch: int, *, d_map: int | None = None,
              map_f32: bool = True, n_maps: int = 0, interpolation: str = "bilinear", border=None, d_valid: int | None = None, stream=None):
        """One launch over all images.  ``cams``: host indices, the camera (fused, ``d_map`` None) or the map of every image.  Sizes are
        (width, height), pitches bytes.  Every argument is checked on the host first (ValueError)."""
        n = len(cams)
        dt, ip = check_remap_args(n, channels, dtype, src_size, src_pitch, dst_size, dst_pitch, interpolation)
        c = check_cams(cams, n, n_maps if d_map else self.n_cams)
        b = np.zeros(4)
        if border is not None:
            bb = np.asarray(border, dtype=np.float64).reshape(-1)
            if bb.size not in (1, channels):
                raise ValueError(f"border: expected one value or {channels}, got {bb.size}")
            b[:channels] = bb
        self._call("pcs_imap_remap", self._h, n, self._ptr(c), self._addr(d_src), int(src_size[0]), int(src_size[1]), int(channels), dt, int(src_pitch), self._addr(d_dst),
                   int(dst_size[0]), int(dst_size[1]), int(dst_pitch), self._addr(d_map), int(map_f32), int(n_maps), ip, self._ptr(b), self._addr(d_valid),
                   _stream_arg(stream))

    def last_kernel_ms(self) -> float:
        return self._ms("pcs_imap_last_kernel_ms")


_mapper_cache: dict = {}


def _mapper(device: int) -> ImageMapper:
    return _cached_handle(_mapper_cache, int(device), lambda: ImageMapper(device))


# ---- device plumbing (torch) -----------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    return torch


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _device_of(*arrays, device=None) -> int:
    for a in arrays:
        if _is_tensor(a) and a.is_cuda:
            return a.device.index if a.device.index is not None else _torch().cuda.current_device()
    return 0 if device is None else int(device)


def _stream(device: int) -> int:
    return _torch().cuda.current_stream(device).cuda_stream


def _to_device(a, dtype, device: int):
    torch = _torch()
    if _is_tensor(a):
        return a.to(device=torch.device("cuda", device), dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=torch.device("cuda", device), dtype=dtype)


def _result(t, as_tensor: bool):
    return t if as_tensor else t.cpu().numpy()


def _points_call(mode, pts, intr, cams, ext, iters, flags, device):
    torch = _torch()
    K = check_intr(intr)
    E = check_ext(ext, K.shape[0])
    iters = _check_iters(iters)
    as_tensor = _is_tensor(pts) and pts.is_cuda
    shape = tuple(pts.shape)
    if len(shape) < 1 or shape[-1] != 2:
        raise ValueError(f"pts: expected (..., 2) pixels, got shape {shape}")
    n = int(np.prod(shape[:-1]))
    c_host = None
    if not (_is_tensor(cams) and cams.is_cuda):
        c_host = check_cams(0 if cams is None else cams, n, K.shape[0])
    elif tuple(cams.shape) != shape[:-1]:
        raise ValueError(f"cams: expected one index per point, shape {shape[:-1]}, got {tuple(cams.shape)}")
    elif n and (int(cams.min()) < 0 or int(cams.max()) >= K.shape[0]):
        raise ValueError(f"cams: an index lies outside [0, {K.shape[0]})")
    if (flags & IMAP_WORLD) and E is None:
        raise ValueError("ext: the world frame needs the cameras' extrinsics")
    dev = _device_of(pts, cams, device=device)
    m = _mapper(dev)
    m.set_cameras(K, E)
    d_in = _to_device(pts, torch.float64, dev).reshape(n, 2)
    d_cam = _to_device(cams if c_host is None else c_host, torch.int32, dev).reshape(n)
    out = torch.empty((n, 3 if mode == IMAP_RAY else 2), dtype=torch.float64, device=d_in.device)
    m.points(mode, n, d_in.data_ptr(), out.data_ptr(), d_cam=d_cam.data_ptr(), iters=iters, flags=flags, stream=_stream(dev))
    return _result(out.reshape(shape[:-1] + (out.shape[1],)), as_tensor)


def undistort_points(pts, intr, cams=None, iters: int = 5, device=None):
    """Detected pixels -> the ideal pinhole's pixels: ``nb_undistort_arr`` (optimisation/compiled_helpers.py:373-406), ``iters`` steps of
    its fixed point (the reference takes 5).  ``pts`` (..., 2); ``cams``: the camera of every point, one index for all, or None = 0."""
    return _points_call(IMAP_UNDISTORT, pts, intr, cams, None, iters, 0, device)


def distort_points(pts, intr, cams=None, device=None):
    """Ideal pixels -> detected pixels: ``nb_distort`` (optimisation/compiled_helpers.py:463-490)."""
    return _points_call(IMAP_DISTORT, pts, intr, cams, None, 5, 0, device)


def pixel_rays(pts, intr, cams=None, ext=None, mode: str = "linear", world: bool = False, distort: bool = True, iters: int = 5, device=None):
    """The ray of every pixel (..., 3): undistort (``distort``), K^-1, z = 1 (``linear``) or unit length (``normalised``), in the camera
    frame or rotated into the world by the camera's extrinsic — ``vector_cam_points`` (utils/general_utils.py:432-454) behind
    ``nb_undistort_arr``, the ``use_vector`` path of ``Camera.im_to_world_ray``."""
    return _points_call(IMAP_RAY, pts, intr, cams, ext, iters, _ray_flags(mode, world, distort), device)


def sensor_map(intr, res, mode: str = "linear", distort: bool = True, ext=None, dtype=np.float64, cam: int = 0, iters: int = 5, depth=None, device=None,
               as_tensor: bool = False):
    """The ray of every pixel of camera ``cam`` as an (H, W, 3) array in IMAGE order, ``res`` = (W, H): ``sensor_map``
    (utils/general_utils.py:456-483) in the camera frame, or with ``ext`` the rays rotated into the world, which is
    ``Camera.world_sensor_map`` (cameras/camera.py:162-177: the map as an offset from the camera position).

    The reference's arrays are (res[0], res[1], 3), indexed [x, y]; this one is indexed [y, x]: it equals the reference's transposed
    by (1, 0, 2), which is exactly what ``Camera.get_image_cord_sensor_map`` returns.  ``distort=False`` skips the undistortion
    (``_make_sensormap(distort=False)``).  ``dtype`` float64 or float32 (the FP64 result rounded once).  ``depth`` (H, W): see
    ``depth_to_points``."""
    torch = _torch()
    K = check_intr(intr)
    E = check_ext(ext, K.shape[0])
    W, H = check_size(res, "res")
    c = int(check_cams(cam, 1, K.shape[0], "cam")[0])
    flags, iters = _ray_flags(mode, E is not None, distort), _check_iters(iters)
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float64 or float32, got {dtype!r}")
    if depth is not None and tuple(depth.shape) != (H, W):
        raise ValueError(f"depth: expected ({H}, {W}), got {tuple(depth.shape)}")
    as_tensor = as_tensor or (_is_tensor(depth) and depth.is_cuda)
    dev = _device_of(depth, device=device)
    m = _mapper(dev)
    m.set_cameras(K, E)
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    out = torch.empty((H, W, 3), dtype=torch.float32 if f32 else torch.float64, device=torch.device("cuda", dev))
    d_depth, depth_f32 = None, False
    if depth is not None:
        depth_f32 = (depth.dtype == torch.float32) if _is_tensor(depth) else (np.asarray(depth).dtype == np.float32)
        d_depth = _to_device(depth, torch.float32 if depth_f32 else torch.float64, dev)
    m.rays(c, W, H, out.data_ptr(), out_f32=f32, flags=flags, iters=iters, d_depth=None if d_depth is None else d_depth.data_ptr(), depth_f32=depth_f32,
           stream=_stream(dev))
    return _result(out, as_tensor)


def depth_to_points(depth, intr, ext=None, cam: int = 0, mode: str = "linear", distort: bool = True, dtype=np.float64, iters: int = 5, device=None):
    """A depth image (H, W) to 3-D points (H, W, 3): position + ray * depth per pixel, ``Camera.im_to_world_ray(depth_im=)``
    (cameras/camera.py:460-493) for the whole image in one launch, without building the sensor map.  With ``ext`` the points are in
    the world, without it in the camera frame.  A depth that is not finite gives a NaN point."""
    H, W = tuple(depth.shape)
    return sensor_map(intr, (W, H), mode=mode, distort=distort, ext=ext, dtype=dtype, cam=cam, iters=iters, depth=depth, device=device)


def undistort_rectify_map(intr, size, R_new=None, K_new=None, cams=None, dtype=np.float32, device=None, as_tensor: bool = False):
    """``cv2.initUndistortRectifyMap`` per camera: for every pixel of the new ``size`` = (Wd, Hd) image the source pixel it shows.
    ``R_new`` (C, 3, 3) rectifying rotations (None: identity), ``K_new`` (C, 4) = [fx, cx, fy, cy] of the new cameras (None: their own,
    the map of ``cv2.undistort``).  -> (len(cams), 2, Hd, Wd) for a list of cameras (default: all), (2, Hd, Wd) for one index.  NaN
    where the pixel looks behind the source camera."""
    torch = _torch()
    K = check_intr(intr)
    Wd, Hd = check_size(size)
    check_view(R_new, K_new, K.shape[0])
    single = cams is not None and np.ndim(cams) == 0
    idx = np.arange(K.shape[0], dtype=np.int32) if cams is None else check_cams(np.atleast_1d(cams), np.atleast_1d(cams).shape[0], K.shape[0])
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype: expected float32 or float64, got {dtype!r}")
    dev = _device_of(device=device)
    m = _mapper(dev)
    m.set_cameras(K)
    m.set_view(R_new, K_new)
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    out = torch.empty((len(idx), 2, Hd, Wd), dtype=torch.float32 if f32 else torch.float64, device=torch.device("cuda", dev))
    for k, c in enumerate(idx):
        m.build_maps(int(c), Wd, Hd, out[k].data_ptr(), out_f32=f32, stream=_stream(dev))
    return _result(out[0] if single else out, as_tensor)


def _image_stack(images, name="images"):
    """-> (a 4-D (n, H, W, C) view, restore(result 4-D) -> the caller's layout)."""
    nd = images.ndim
    if nd == 2:
        return images[None, :, :, None], lambda r: r[0, :, :, 0]
    if nd == 3:
        return images[:, :, :, None], lambda r: r[:, :, :, 0]
    if nd == 4:
        return images, lambda r: r
    raise ValueError(f"{name}: expected (H, W), (n, H, W) or (n, H, W, C), got shape {tuple(images.shape)}")


def _pitched(t):
    """A device tensor (n, H, W, C) usable in place: interleaved channels, dense pixels, one row pitch.  -> pitch in elements or None."""
    n, H, W, C = t.shape
    s = t.stride()
    pitch = s[1] if H > 1 else W * C   # the stride of an axis of length 1 says nothing
    if (C == 1 or s[3] == 1) and (W == 1 or s[2] == C) and pitch >= W * C and (n == 1 or s[0] == H * pitch):
        return pitch
    return None


def remap_images(images, maps=None, map_index=None, *, interpolation: str = "bilinear", border=None, return_valid: bool = False, out=None, device=None, _fused=None):
    """``cv2.remap`` with BORDER_CONSTANT over a stack of images in one launch.  ``maps``: (2, Hd, Wd) for all images, or (M, 2, Hd, Wd)
    with ``map_index`` (n,) choosing each image's map (default: image i takes map i when M == n); float32 or float64, from
    ``undistort_rectify_map`` or the caller's own.  ``interpolation``: 'nearest', 'bilinear', 'bicubic' (a = -0.75, cv2.INTER_CUBIC).
    ``border``: one value or one per channel.  uint8 results are the exact FP64 interpolant rounded half-to-even and saturated.
    ``return_valid``: also a uint8 (n, Hd, Wd) plane, 1 where every tap lay inside the source.  ``out``: a device tensor to write."""
    torch = _torch()
    stack, restore = _image_stack(images)
    n, Hs, Ws, C = (int(v) for v in stack.shape)
    name = str(stack.dtype).replace("torch.", "")
    if _fused is None:
        if maps is None:
            raise ValueError("maps: expected (2, Hd, Wd) or (M, 2, Hd, Wd)")
        mp = maps if maps.ndim == 4 else maps[None]
        if mp.ndim != 4 or mp.shape[1] != 2:
            raise ValueError(f"maps: expected (2, Hd, Wd) or (M, 2, Hd, Wd), got shape {tuple(maps.shape)}")
        M, Hd, Wd = int(mp.shape[0]), int(mp.shape[2]), int(mp.shape[3])
        if map_index is None:
            if M not in (1, n):
                raise ValueError(f"map_index: needed to pair {n} images with {M} maps")
            map_index = np.zeros(n, dtype=np.int32) if M == 1 else np.arange(n, dtype=np.int32)
        index, limit = check_cams(map_index, n, M, "map_index"), M
    else:
        index, (Wd, Hd), limit = _fused
    out_stack = None
    if out is not None:
        if not (_is_tensor(out) and out.is_cuda):
            raise ValueError("out: expected a torch tensor on the device")
        out_stack, _ = _image_stack(out, "out")
        if tuple(out_stack.shape) != (n, Hd, Wd, C) or out_stack.dtype != getattr(torch, name, None) or _pitched(out_stack) is None:
            raise ValueError(f"out: expected ({n}, {Hd}, {Wd}, {C}) of {name} with dense pixels and one row pitch, got {tuple(out.shape)} of {out.dtype}")
    item = 1 if name == "uint8" else 4
    check_remap_args(n, C, name, (Ws, Hs), Ws * C * item, (Wd, Hd), Wd * C * item, interpolation)
    as_tensor = _is_tensor(images) and images.is_cuda
    dev = _device_of(images, out, maps, device=device)
    m = _mapper(dev)
    src = stack if as_tensor and _pitched(stack) is not None else _to_device(stack, getattr(torch, name), dev)
    if out_stack is None:
        out_stack = torch.empty((n, Hd, Wd, C), dtype=src.dtype, device=src.device)
    valid = torch.empty((n, Hd, Wd), dtype=torch.uint8, device=src.device) if return_valid else None
    kw = {}
    if _fused is None:
        f32 = (mp.dtype == torch.float32) if _is_tensor(mp) else (np.asarray(mp).dtype == np.float32)
        d_map = _to_device(mp, torch.float32 if f32 else torch.float64, dev)
        kw = dict(d_map=d_map.data_ptr(), map_f32=f32, n_maps=limit)
    m.remap(index, src.data_ptr(), (Ws, Hs), C, name, _pitched(src) * item, out_stack.data_ptr(), (Wd, Hd), _pitched(out_stack) * item, interpolation=interpolation,
            border=border, d_valid=None if valid is None else valid.data_ptr(), stream=_stream(dev), **kw)
    res = out if out is not None else _result(restore(out_stack), as_tensor)
    return (res, _result(valid, as_tensor)) if return_valid else res


def undistort_images(images, cams, intr, R_new=None, K_new=None, size=None, *, interpolation: str = "bilinear", border=None, method: str = "auto",
                     return_valid: bool = False, out=None, device=None):
    """Undistort (and, with ``R_new`` / ``K_new``, rectify) a stack of images, image i by camera ``cams[i]``: ``Camera.undistort`` /
    ``undistort_im`` (cv2.undistort(img, K, d, None, K)) with the defaults, ``remap_im`` (cv2.initUndistortRectifyMap + cv2.remap) with
    a view.  ``size`` = (Wd, Hd) of the results (default: the source's).

    ``method``: 'fused' computes every source coordinate in registers from the camera table, so that the only memory traffic is the
    images' own; 'mapped' builds float32 maps (``undistort_rectify_map``) and reads them back, the classical two-step form, 8 B of map
    per pixel; 'auto' is 'fused' (see DEFAULT_METHOD)."""
    K = check_intr(intr)
    stack, _ = _image_stack(images)
    n, Hs, Ws = int(stack.shape[0]), int(stack.shape[1]), int(stack.shape[2])
    index = check_cams(cams, n, K.shape[0])
    check_view(R_new, K_new, K.shape[0])
    Wd, Hd = (Ws, Hs) if size is None else check_size(size)
    if method not in ("auto", "fused", "mapped"):
        raise ValueError(f"method: expected 'auto', 'fused' or 'mapped', got {method!r}")
    if int(stack.shape[3]) not in CHANNELS:
        raise ValueError(f"channels (C): expected one of {CHANNELS}, got {int(stack.shape[3])}")
    check_interpolation(interpolation)
    dev = _device_of(images, out, device=device)
    if (DEFAULT_METHOD if method == "auto" else method) == "mapped":
        maps = undistort_rectify_map(K, (Wd, Hd), R_new, K_new, device=dev, as_tensor=True)
        return remap_images(images, maps, index, interpolation=interpolation, border=border, return_valid=return_valid, out=out, device=dev)
    m = _mapper(dev)
    m.set_cameras(K)
    m.set_view(R_new, K_new)
    return remap_images(images, interpolation=interpolation, border=border, return_valid=return_valid, out=out, device=dev, _fused=(index, (Wd, Hd), K.shape[0]))


# ---- stereo rectification (host) -------------------------------------------------------------------------------------------------------
def _rodrigues(w):
    from scipy.spatial.transform import Rotation

    return Rotation.from_rotvec(w).as_matrix()


def _outline(res):
    """The border pixels of a W x H sensor as four edges (left, right, top, bottom), each (k, 2)."""
    W, H = res
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    return [np.stack([np.zeros(H), ys], axis=1), np.stack([np.full(H, W - 1.0), ys], axis=1), np.stack([xs, np.zeros(W)], axis=1), np.stack([xs, np.full(W, H - 1.0)], axis=1)]


def rectify_pair(intr_a, ext_a, intr_b, ext_b, res, alpha: float = 1.0, zero_distortion: bool = False, new_size=None, undistort=None):
    """Rectifying rotations and the common new camera of a stereo pair: ``rectify_camera_pair`` (reconstruction/reconstruction_utils.py:
    85-107, cv2.stereoRectify with CALIB_ZERO_DISPARITY).  ``intr_*`` (9,), ``ext_*`` (3, 4) world -> camera, ``res`` = (W, H) of both
    sensors, ``new_size`` (default ``res``).  -> ``R_a, R_b`` (3, 3) camera frame -> rectified frame, ``K_new`` = [fx, cx, fy, cy]
    (one for both: zero disparity at infinity), ``Q`` (4, 4) with Q (u, v, d, 1)^T ~ (X, Y, Z, 1) in the rectified frame of camera a,
    d = u_a - u_b.  Host NumPy; only the outline goes through ``undistort`` (default: ``undistort_points`` on the device).

    The rule, exactly.  (1) Bouguet: with X_b = R X_a + T the relative pose, r = exp(-log(R) / 2) and t = r T; W is the rotation
    about t x e with the smallest angle that turns t onto e = sign(t_x) e_x; R_a = W r^T, R_b = W r.  Then X_b' = X_a' + (+-|T|, 0, 0).
    (2) Outline: the border pixels of each source are undistorted (``zero_distortion``: taken as they are), normalised by the source's
    K and rotated by its R_*, p = (X / Z, Y / Z).  A source pixel reaches half a pixel beyond its centre, h = 0.5 / min(fx, fy) in
    these units.  (3) Inner rectangle: per camera [max over the left edge of p_x + h, min over the right edge of p_x - h] x the same
    for top and bottom, intersected over both cameras; its centre m becomes the image centre.  (4) Scales: f_cover = max((Wn - 1) /
    inner width, (Hn - 1) / inner height): the new image just stays inside both sources; f_fit = min over both axes of ((Wn - 1) / 2)
    / (max over all outline points of |p_x - m_x| + h): every source pixel just fits inside.  (5) f = (1 - alpha) f_cover + alpha
    f_fit, fx = fy = f, (cx, cy) = ((Wn - 1) / 2, (Hn - 1) / 2) - f m."""
    Ka, Kb = check_intr(intr_a)[0], check_intr(intr_b)[0]
    Ea, Eb = check_ext(ext_a, 1)[0].reshape(3, 4), check_ext(ext_b, 1)[0].reshape(3, 4)
    W, H = check_size(res, "res")
    Wn, Hn = (W, H) if new_size is None else check_size(new_size, "new_size")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha: expected a number in [0, 1], got {alpha!r}")
    from scipy.spatial.transform import Rotation

    R = Eb[:, :3] @ Ea[:, :3].T
    T = Eb[:, 3] - R @ Ea[:, 3]
    if not np.linalg.norm(T) > 0:
        raise ValueError("ext_a / ext_b: the cameras share a centre, there is no baseline to rectify along")
    r = _rodrigues(-0.5 * Rotation.from_matrix(R).as_rotvec())
    t = r @ T
    e = np.array([1.0 if t[0] >= 0 else -1.0, 0.0, 0.0])
    axis = np.cross(t, e)
    s = np.linalg.norm(axis)
    Wr = np.eye(3) if s < 1e-300 else _rodrigues(axis / s * np.arctan2(s, float(t @ e)))
    R_a, R_b = Wr @ r.T, Wr @ r
    und = undistort or (lambda pts, intr: undistort_points(pts, intr))
    inner = [-np.inf, np.inf, -np.inf, np.inf]   # x low, x high, y low, y high
    pts_all = []
    h = 0.5 / min(abs(Ka[0]), abs(Ka[2]), abs(Kb[0]), abs(Kb[2]))
    for K, Rc in ((Ka, R_a), (Kb, R_b)):
        edges = []
        for edge in _outline((W, H)):
            u = edge if zero_distortion else np.asarray(und(edge, K), dtype=np.float64)
            X = np.stack([(u[:, 0] - K[1]) / K[0], (u[:, 1] - K[3]) / K[2], np.ones(u.shape[0])], axis=1) @ Rc.T
            edges.append(X[:, :2] / X[:, 2:3])
        left, right, top, bottom = edges
        inner = [max(inner[0], left[:, 0].max() + h), min(inner[1], right[:, 0].min() - h), max(inner[2], top[:, 1].max() + h), min(inner[3], bottom[:, 1].min() - h)]
        pts_all.append(np.concatenate(edges))
    if not (inner[1] > inner[0] and inner[3] > inner[2]):
        raise ValueError("the two views share no rectangle after rectification")
    m = np.array([0.5 * (inner[0] + inner[1]), 0.5 * (inner[2] + inner[3])])
    f_cover = max((Wn - 1) / (inner[1] - inner[0]), (Hn - 1) / (inner[3] - inner[2]))
    p = np.concatenate(pts_all)
    f_fit = min(0.5 * (Wn - 1) / (np.abs(p[:, 0] - m[0]).max() + h), 0.5 * (Hn - 1) / (np.abs(p[:, 1] - m[1]).max() + h))
    f = (1.0 - float(alpha)) * f_cover + float(alpha) * f_fit
    cx, cy = 0.5 * (Wn - 1) - f * m[0], 0.5 * (Hn - 1) - f * m[1]
    tx = float((Wr @ t)[0])   # X_b' = X_a' + (tx, 0, 0)
    Q = np.array([[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / tx, 0.0]])
    return R_a, R_b, np.array([f, cx, f, cy]), Q


def rectify_images(images_a, images_b, intr_a, ext_a, intr_b, ext_b, alpha: float = 1.0, *, interpolation: str = "bicubic", border=None, new_size=None,
                   return_valid: bool = False, device=None):
    """Rectify the images of a stereo pair: ``rectify_camera_images`` (reconstruction/reconstruction_utils.py:61-82) as ONE fused remap
    from the distorted sources (the reference undistorts first and remaps the result: two interpolations).  ``images_a`` / ``images_b``:
    stacks of one shape.  -> (rectified a, rectified b, Q[, valid a, valid b]); ``rectify_images.last`` holds (R_a, R_b, K_new, Q)."""
    sa, _ = _image_stack(images_a, "images_a")
    sb, _ = _image_stack(images_b, "images_b")
    if tuple(sa.shape) != tuple(sb.shape) or sa.dtype != sb.dtype:
        raise ValueError(f"images_b: expected the shape and type of images_a, {tuple(images_a.shape)}, got {tuple(images_b.shape)}")
    n, H, W = int(sa.shape[0]), int(sa.shape[1]), int(sa.shape[2])
    dev = _device_of(images_a, images_b, device=device)
    intr = np.stack([check_intr(intr_a)[0], check_intr(intr_b)[0]])
    R_a, R_b, K_new, Q = rectify_pair(intr_a, ext_a, intr_b, ext_b, (W, H), alpha=alpha, new_size=new_size,
                                      undistort=lambda pts, K: undistort_points(pts, K, device=dev))
    rectify_images.last = (R_a, R_b, K_new, Q)
    size = (W, H) if new_size is None else check_size(new_size, "new_size")
    outs = []
    for img, cam in ((images_a, 0), (images_b, 1)):
        outs.append(undistort_images(img, np.full(n, cam), intr, np.stack([R_a, R_b]), K_new, size, interpolation=interpolation, border=border, method="fused",
                                     return_valid=return_valid, device=dev))
    if return_valid:
        return outs[0][0], outs[1][0], Q, outs[0][1], outs[1][1]
    return outs[0], outs[1], Q
