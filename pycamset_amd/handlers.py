"""ParamHandler surface of the path — the drop-in boundary.

For the cost/Jacobian path only, this provides what pyCamSet's
  ``TemplateBundleHandler``   optimisation/template_handler.py:80-240          (chain T)
  ``SelfBundleHandler``       optimisation/standard_bundle_handler.py:109-260  (chain S)
  ``FreePointBundleHandler``  optimisation/free_point_handler.py:102-201       (chain F)
and their ``*BundlePrimitive`` helpers (th:32-78, sbh:46-107, fph:47-100) provide: the same constructor
arguments and attribute names, the same free-vector layout
``x = [9 * F_intr | 6 * F_extr | 6 * F_pose | F_pointscalar]`` and the same closures

    loss_fn = handler.make_loss_fun(threads)   # x -> (2N,) float64
    jac_fn  = handler.make_loss_jac(threads)   # x -> scipy.sparse.csr_array (2N, len(x))

so ``scipy.optimize.least_squares(loss_fn, x0, jac=jac_fn, x_scale='jac', ...)``
(optimisation_handling.py:88-98) runs unchanged.  The three reference handlers differ only in which
parameter groups exist, so here ONE table (``_CHAIN_GROUPS``) drives one primitive and one handler core.

``camset`` only needs ``get_names()`` / ``get_n_cams()`` and ``target`` only needs ``point_data`` — the
attributes the reference touches on this path (th:116-129, th:160-163).  ``calc_initial_params`` (th:302-346) computes a
start vector from the detections with the device's batched PnP (``pose_seeding``) and, where the camset holds no intrinsics, with
the device's intrinsics estimate (``compiled_helpers.estimate_intrinsics``); the outlier prompt's decision is the option
``"outliers"`` (``find_and_exclude_transform_outliers``); CameraSet reconstruction is outside the path.  ``get_initial_params`` returns what ``set_initial_params`` was given.

Differences from the reference, on purpose:
  * The engine lays the parameter string out from the SLAB sizes (n_cams, max_ims, number of target
    points), not from ``max(index) + 1`` of the detections (afb:793-795).  When the last camera / image /
    key has no detection the two rules differ; trailing unused entries (template chain: last images; self
    chain: last keys) give identical results, and where the reference's rule mis-offsets a later group
    (SURVEY 8a quirk ii: last image unobserved in the self chain, last camera unobserved in any chain) this
    package evaluates the slabs the handler actually built.  tests/test_host_logic.py pins both facts against
    fixtures made by the reference.
  * ``options={'fixed_pose': None}``: NumPy reads a ``None`` index as ``newaxis``, so the reference fixes and
    zeroes EVERY pose (th:134-137).  Reproduced as is (same expression).
"""
from __future__ import annotations

import logging
from copy import deepcopy

import numpy as np
from scipy.sparse import csr_array

from . import function_blocks as fb
from .detections import TargetDetection  # noqa: F401  (re-exported: the handlers' input type)

log = logging.getLogger(__name__)

DEFAULT_OPTIONS = {  # th:24-31
    "verbosity": 2,
    "fixed_pose": 0,
    "ref_cam": 0,
    "ref_pose": 0,
    "outliers": "ask",
    "max_nfev": 100,
}

# parameter groups in free-vector / parameter-string order: (slab attribute, mask attribute, scalars per free unit)
_GROUP = {
    "intr": ("intr", "intr_unfixed", 9),
    "extr": ("extr", "extr_unfixed", 6),
    "pose": ("poses", "poses_unfixed", 6),
    "bdpt": ("bundle_pts", "bdpt_unfixed", 1),   # points are fixed per scalar (sbh:83-86)
}
_CHAIN_GROUPS = {"template": ("intr", "extr", "pose"), "self": ("intr", "extr", "pose", "bdpt"), "free": ("intr", "extr", "bdpt")}


def fill_flat(src: np.ndarray, dst: np.ndarray, dst_unfixed: np.ndarray) -> None:
    """compiled_helpers.py:155-177: scatter the free rows / scalars of ``src`` into ``dst``."""
    dst[np.asarray(dst_unfixed, dtype=bool)] = src


def _list_dict_to_np_array(d):
    """Lists inside a (nested) ``fixed_params`` dict become arrays, in place — the normalisation the reference applies to
    the dict before reading 'int' / 'ext' entries out of it (utils/general_utils.py:21-30)."""
    pending = [d] if isinstance(d, dict) else []
    while pending:
        level = pending.pop()
        for name in list(level):
            entry = level[name]
            if isinstance(entry, list):
                level[name] = np.asarray(entry)
            elif isinstance(entry, dict):
                pending.append(entry)
    return d


class BundlePrimitive:
    """Free vector ``x`` -> full parameter slabs for one chain (th:32-78, sbh:46-107, fph:47-100).

    Holds persistent full slabs (``intr`` (C,9), ``extr`` (C,6), ``poses`` (I,6), ``bundle_pts`` (3K,)) and one
    boolean "unfixed" mask per slab; ``return_bundle_primitives(x)`` scatters the free entries into them and
    returns the slabs in block order.  ``intr_end`` / ``extr_end`` / ``pose_end`` / ``bdpt_end`` are the
    cumulative ends of the groups inside ``x``, ``free_intr`` … the free unit counts, as in the reference."""

    def __init__(self, chain: str, slabs: dict, unfixed: dict):
        self.chain = chain
        self.groups = _CHAIN_GROUPS[chain]
        for g in self.groups:
            slab_name, mask_name, _ = _GROUP[g]
            slab = slabs[g]
            mask = unfixed.get(g)
            setattr(self, slab_name, slab)
            setattr(self, mask_name, np.ones(slab.shape[0], dtype=bool) if mask is None else mask)
        self.correct_gauge = True
        self.calc_type_inds()

    def calc_type_inds(self):
        end = 0
        for g in self.groups:
            _, mask_name, width = _GROUP[g]
            n_free = int(np.sum(getattr(self, mask_name)))
            end += width * n_free
            setattr(self, f"free_{g}", n_free)
            setattr(self, f"{g}_end", end)
        if "pose" in self.groups:
            self.free_poses = self.free_pose   # both spellings exist in the reference (th:52, sbh:77)

    calc_free_poses = calc_type_inds  # th:50

    def return_bundle_primitives(self, params):
        start, out = 0, []
        for g in self.groups:
            slab_name, mask_name, width = _GROUP[g]
            slab, mask, end = getattr(self, slab_name), getattr(self, mask_name), getattr(self, f"{g}_end")
            part = params[start:end]
            fill_flat(part.reshape((-1, width)) if width > 1 else part, slab, mask)
            out.append(slab.reshape((-1, 3)) if g == "bdpt" else slab)
            start = end
        return tuple(out)


def TemplateBundlePrimitive(poses, extr, intr, poses_unfixed=None, extr_unfixed=None, intr_unfixed=None):  # th:32-47
    return BundlePrimitive("template", {"intr": intr, "extr": extr, "pose": poses},
                           {"intr": intr_unfixed, "extr": extr_unfixed, "pose": poses_unfixed})


def StandardBundlePrimitive(poses, bundle_points, extr, intr, poses_unfixed=None, bundle_points_unfixed=None,
                            extr_unfixed=None, intr_unfixed=None, always_correct_gauge=False):  # sbh:46-75
    return BundlePrimitive("self", {"intr": intr, "extr": extr, "pose": poses, "bdpt": bundle_points},
                           {"intr": intr_unfixed, "extr": extr_unfixed, "pose": poses_unfixed, "bdpt": bundle_points_unfixed})


def FreePointPrimitive(bundle_points, extr, intr, bundle_points_unfixed=None, extr_unfixed=None, intr_unfixed=None):  # fph:47-69
    return BundlePrimitive("free", {"intr": intr, "extr": extr, "bdpt": bundle_points},
                           {"intr": intr_unfixed, "extr": extr_unfixed, "bdpt": bundle_points_unfixed})


def find_not_colinear_pts(points):
    """Indices of three points that span a plane: point 0 and the first pair (i, j), 1 <= i < j in lexicographic order,
    whose triangle with it has a cross product longer than 1e-8 (the gauge points of sbh:30-44, same search order)."""
    pts = np.asarray(points, dtype=np.float64)
    legs = pts[1:] - pts[0]
    for i in range(legs.shape[0]):
        areas = np.linalg.norm(np.cross(legs[i], legs[i + 1:]), axis=-1)
        hit = np.nonzero(areas > 1e-8)[0]
        if hit.size:
            return 0, i + 1, i + 2 + int(hit[0])
    raise ValueError("No set of values that were not colinear were found in the provided data.")


class TemplateBundleHandler:  # th:80-240
    """Target-pose based bundle adjustment against a constant template (chain T).  The subclasses only
    change ``chain`` and the point masks; everything on the path lives here."""

    chain = "template"
    _BLOCKS = {"template": (fb.projection, fb.extrinsic3D, fb.template_points),                  # th:152
               "self": (fb.projection, fb.extrinsic3D, fb.rigidTform3d, fb.free_point),          # sbh:182
               "free": (fb.projection, fb.extrinsic3D, fb.free_point)}                           # fph:143

    def __init__(self, camset, target, detection, fixed_params: dict | None = None, options: dict | None = None,
                 missing_poses: list | None = None, *, dtype: str = "f64", device: int = 0, pinned_ring: int | None = None,
                 counts=None, visible_feature_mask=None):
        """Keyword-only extensions: ``dtype`` / ``device`` / ``pinned_ring`` go to the engine
        (function_blocks.optimisation_function); ``counts`` = (n_cams, n_imgs, n_keys) overrides the slab sizes of
        the parameter-string layout (a rank that holds a shard of the detections must lay out the GLOBAL string);
        ``counts="reference"`` selects the reference's own rule, max index + 1 of the detections (afb:793-795) —
        what a reference handler patched with ``pycamset_amd.function_blocks`` gets, quirk ii included;
        ``visible_feature_mask`` (self chain): which features are seen by ANY rank — the reference derives it from
        the handler's own detections (sbh:160-169), and ranks holding shards must fix the same features."""
        self.problem_opts = dict(DEFAULT_OPTIONS)  # the reference aliases and mutates the module global (th:108-110)
        if options is not None:
            self.problem_opts.update(options)
        self.fixed_params = _list_dict_to_np_array(fixed_params)
        if fixed_params is None:
            self.fixed_params = {}
        self.camset = camset
        self.cam_names = camset.get_names()
        self.detection = deepcopy(detection)
        self.target = target
        self.point_data = deepcopy(target.point_data)
        self.target_point_shape = np.array(target.point_data.shape)
        self.initial_params = None
        self.param_len = None
        self.jac_mask = None
        self.missing_poses = missing_poses
        self.initial_intrinsics = None   # the IntrinsicsEstimate of calc_initial_params, where it had to make one

        n_poses = detection.max_ims
        n_cams = camset.get_n_cams()
        slabs = {"intr": np.zeros((n_cams, 9)), "extr": np.zeros((n_cams, 6)), "pose": np.zeros((n_poses, 6))}
        unfixed = {"extr": np.array(["ext" not in self.fixed_params.get(name, {}) for name in self.cam_names]),
                   "intr": np.array(["int" not in self.fixed_params.get(name, {}) for name in self.cam_names]),
                   "pose": np.ones(n_poses, dtype=bool)}
        if "fixed_pose" in self.problem_opts:  # th:134-137 (a None index selects every pose, see module docstring)
            fixed_pose = self.problem_opts["fixed_pose"]
            unfixed["pose"][fixed_pose] = False
            slabs["pose"][fixed_pose, :] = [0, 0, 0, 0, 0, 0]
        if self.chain != "template":
            self.flat_point_data = np.copy(self.point_data.reshape((-1)))
            slabs["bdpt"] = self.flat_point_data
            unfixed["bdpt"] = self.feat_unfixed = self._point_mask(visible_feature_mask)
        if self.chain == "free":
            self.super_primitive = TemplateBundlePrimitive(slabs["pose"], slabs["extr"], slabs["intr"], unfixed["pose"],
                                                           unfixed["extr"], unfixed["intr"])  # fph:131
        self.bundlePrimitive = BundlePrimitive(self.chain, slabs, unfixed)
        self.populate_self_from_fixed_params()
        n_keys = int(np.prod(self.point_data.shape[:-1]))
        self.op_fun = fb.optimisation_function(
            [b() for b in self._BLOCKS[self.chain]], dtype=dtype, device=device, pinned_ring=pinned_ring,
            counts=None if counts == "reference" else counts if counts is not None else (n_cams, n_poses, n_keys))

    def _point_mask(self, visible_feature_mask):
        return None

    # -- the path ------------------------------------------------------------------------------
    def can_make_jac(self):  # th:154-155
        return self.op_fun.can_make_jac()

    def _flat_detections(self) -> np.ndarray:
        return self.detection.return_flattened_keys(self.target.point_data.shape[:-1]).get_data()  # th:162-163

    def _jac_mask(self) -> np.ndarray:  # th:177-183, sbh:211-218, fph:172-178
        bp = self.bundlePrimitive
        return np.concatenate([np.repeat(getattr(bp, _GROUP[g][1]), _GROUP[g][2]) for g in bp.groups], axis=0)

    def _template_arg(self):
        # th:160; the self / free closures call the generated functions without a template (sbh:198, fph:159)
        return self.target.point_data.reshape((-1, 3)) if self.chain == "template" else None

    def make_loss_fun(self, threads=None):  # th:157-170, sbh:184-198, fph:145-159
        obj_data = self._template_arg()
        temp_loss = self.op_fun.make_full_loss_fn(self._flat_detections(), threads)

        def loss_fun(params):
            param_str = self.op_fun.build_param_list(*self.get_bundle_adjustment_inputs(params))
            return temp_loss(param_str, obj_data).flatten()

        return loss_fun

    def make_loss_jac(self, threads=None):  # th:172-193, sbh:200-226, fph:161-186
        obj_data = self._template_arg()
        dd = self._flat_detections()
        temp_loss = self.op_fun.make_jacobean(dd, threads, unfixed_params=self._jac_mask())

        def jac_fn(params):
            param_str = self.op_fun.build_param_list(*self.get_bundle_adjustment_inputs(params))
            d, c, rp = temp_loss(param_str, obj_data)
            return csr_array((d, c, rp), shape=(2 * dd.shape[0], params.shape[0]))

        return jac_fn

    def populate_self_from_fixed_params(self):  # th:204-213
        for idx, cam_name in enumerate(self.cam_names):
            fixed = self.fixed_params.get(cam_name, {})
            if "ext" in fixed:
                self.bundlePrimitive.extr[idx] = fixed["ext"]
            if "int" in fixed:
                self.bundlePrimitive.intr[idx] = fixed["int"]

    def get_bundle_adjustment_inputs(self, x, make_points=False):  # th:215-240
        if make_points:
            raise NotImplementedError("make_points is a visualisation helper outside the cost/Jacobian path")
        return self.bundlePrimitive.return_bundle_primitives(x)

    # -- parameters ----------------------------------------------------------------------------
    def set_initial_params(self, x: np.ndarray):  # th:281-288
        self.initial_params = x

    def get_initial_params(self) -> np.ndarray:  # th:290-300
        if self.initial_params is not None:
            return self.initial_params
        raise NotImplementedError(
            "no start vector has been set: compute one from the detections with calc_initial_params() (template_handler.py:302-346, "
            "device PnP) and hand it to set_initial_params(), or supply your own")

    def calc_initial_params(self, intr=None, *, seeding: str = "reference", refine_poses: bool = False,
                            view_consensus: int | None = None, intrinsics_consensus: int | None = None) -> np.ndarray:  # th:302-346
        """A start vector from the detections: per-view target poses on the device (``compiled_helpers.estimate_view_poses``), the view
        graph of ``pose_seeding.estimate_camera_relative_poses`` (th:468-601), then the free entries in slab order — unfixed intrinsics,
        extrinsics and poses (plus, for the self and free chains, the free point scalars of the template).  ``intr``: (C, 9) rows
        [fx, cx, fy, cy, k0, k1, p0, p1, k2]; default: ``camset[idc].intrinsic`` / ``.distortion_coefs`` (th:321-329) and, where the
        camset holds none, the device's estimate from the planar views of the detections (``compiled_helpers.estimate_intrinsics`` with
        ``refine=True`` and ``camset[idc].res`` where present — the reference's ``initial_calibration``, abstract_target.py:263-343),
        kept on ``initial_intrinsics``.  Sets ``missing_poses`` and runs ``find_and_exclude_transform_outliers`` on the per-image error of the
        seeding (th:319), which excludes images only under ``options["outliers"] == "y"``; returns the vector without storing it.

        ``seeding``: ``"reference"`` (default) is the reference's view graph, which needs an image that every camera sees and raises
        ValueError without one; ``"graph"`` is ``pose_seeding.estimate_camera_relative_poses_graph``, which needs only a connected
        co-visibility graph; ``"auto"`` takes the reference's and falls back to the graph on exactly that error.

        ``refine_poses``: the seeded pose of an image is ONE camera's estimate, the candidate of lowest error.  When true, every image's
        pose is refined over the detections of all cameras with the seeded extrinsics and intrinsics held fixed
        (``compiled_helpers.localise_target``) before the vector is assembled; an image that could not be refined keeps its seeded pose
        and the reference image, whose pose is exactly 0 and fixed, is left alone.  Off by default.

        ``view_consensus``: hypotheses per view of the consensus sampling in front of the per-view poses
        (``compiled_helpers.estimate_view_poses(consensus=...)``; 64 is a good value), so that detections with a wrong id do not bend
        the start; default ``options["view_consensus"]``, else 0 (off).

        ``intrinsics_consensus``: hypotheses per (camera, image, board) group of the consensus sampling in front of the planar
        homographies (``compiled_helpers.estimate_intrinsics(consensus=...)``; 64 is a good value), used where the intrinsics are
        estimated from the detections: without it a few wrong ids cost a camera its estimate before ``view_consensus`` is ever
        reached; default ``options["intrinsics_consensus"]``, else 0 (off)."""
        from .pose_seeding import estimate_camera_relative_poses, estimate_camera_relative_poses_graph

        if view_consensus is None:
            view_consensus = self.problem_opts.get("view_consensus", 0)
        if intrinsics_consensus is None:
            intrinsics_consensus = self.problem_opts.get("intrinsics_consensus", 0)

        if seeding not in ("reference", "graph", "auto"):
            raise ValueError(f"seeding must be 'reference', 'graph' or 'auto', got {seeding!r}")

        bp = self.bundlePrimitive
        n_cams = bp.intr.shape[0]
        intr = self._initial_intrinsics(intr, intrinsics_consensus)
        n_imgs = bp.poses.shape[0] if "pose" in bp.groups else self.detection.max_ims
        args = (self._flat_detections(), self.point_data.reshape((-1, 3)), intr, n_cams, n_imgs)
        refs = {"ref_cam": self.problem_opts.get("ref_cam", 0), "ref_pose": self.problem_opts.get("ref_pose", 0), "view_consensus": view_consensus}
        if seeding == "graph":
            seeded = estimate_camera_relative_poses_graph(*args, **refs)
        else:
            try:
                seeded = estimate_camera_relative_poses(*args, **refs)
            except ValueError as e:
                if seeding != "auto" or "Couldn't find an initial pose" not in str(e):
                    raise
                seeded = estimate_camera_relative_poses_graph(*args, **refs)
        extr, poses, self.initial_per_im_error, missing = seeded
        self.missing_poses = missing
        self.find_and_exclude_transform_outliers(self.initial_per_im_error)   # th:319
        if refine_poses:
            poses = self._refine_seeded_poses(args[0], args[1], intr, extr, poses)
        parts = [intr[bp.intr_unfixed].ravel(), extr[bp.extr_unfixed].ravel()]
        if "pose" in bp.groups:
            parts.append(poses[bp.poses_unfixed].ravel())
        if "bdpt" in bp.groups:
            parts.append(self.flat_point_data[bp.bdpt_unfixed])
        return np.concatenate(parts)

    def _initial_intrinsics(self, intr, intrinsics_consensus: int) -> np.ndarray:
        """The (C, 9) intrinsics a seeding starts from: the caller's, else the camset's (th:321-329), else the device's estimate from
        the planar views; a fixed camera's are the fixed ones."""
        n_cams = self.bundlePrimitive.intr.shape[0]
        if intr is None:
            try:
                intr = np.stack([np.concatenate((np.asarray(self.camset[idc].intrinsic)[[0, 0, 1, 1], [0, 2, 1, 2]].squeeze(),
                                                 np.asarray(self.camset[idc].distortion_coefs).squeeze()), axis=0) for idc in range(n_cams)])
            except (TypeError, AttributeError, KeyError, IndexError):
                intr = self._estimate_initial_intrinsics(n_cams, intrinsics_consensus)
        intr = np.array(intr, dtype=np.float64)
        if intr.shape != (n_cams, 9):
            raise ValueError(f"intr must be ({n_cams}, 9), got {intr.shape}")
        for idc, name in enumerate(self.cam_names):   # a fixed camera's intrinsics are the fixed ones
            if "int" in self.fixed_params.get(name, {}):
                intr[idc] = self.fixed_params[name]["int"]
        return intr

    def _refine_seeded_poses(self, dct, points, intr, extr, poses) -> np.ndarray:
        """``calc_initial_params(refine_poses=True)``: the seeded image poses refined per image with every camera fixed at its seeded
        extrinsics.  The accept rule only ever lowers an image's cost, so no image gets worse."""
        from . import compiled_helpers as ch
        from .pose_seeding import pose_to_4x4

        poses = np.array(poses, dtype=np.float64)
        res = ch.localise_target(dct, points, intr, pose_to_4x4(extr)[:, :3, :], n_imgs=poses.shape[0], poses_init=poses,
                                 device=self.op_fun.device)
        take = (res.status != ch.RIGPOSE_NOT_ESTIMATED) & np.all(np.isfinite(res.poses), axis=1) & ~np.all(poses == 0.0, axis=1)
        poses[take] = res.poses[take]
        return poses

    def find_and_exclude_transform_outliers(self, per_im_error):  # th:242-279
        """The MAD test (``diagnostics.mad_outliers``, threshold 20) on the per-image error over the images that are not missing yet,
        for at most 10 rounds; a round without outliers ends the loop.  The reference asks at a prompt whether to exclude what it found
        (th:268-270); here ``options["outliers"]`` holds the answer: ``"y"`` marks the images found as missing poses and tests the rest
        again, ``"n"`` logs them and stops, and ``"ask"`` (the default: there is nobody to ask) does what ``"n"`` does.  Returns the
        images found in all rounds (excluded only under ``"y"``)."""
        from . import diagnostics

        if self.missing_poses is None:
            raise ValueError("missing poses should be initialised before calling this function")
        answer = self.problem_opts.get("outliers", "ask")
        per_im_error = np.asarray(per_im_error, dtype=np.float64)
        found_all = []
        for round_no in range(10):
            not_missing = np.where(~np.asarray(self.missing_poses, dtype=bool))[0]
            found = diagnostics.mad_outliers(per_im_error[not_missing], out_thresh=20)
            if found is None:
                log.info("no outlier images in round %d", round_no)
                break
            images = not_missing[found]
            found_all.extend(int(i) for i in images)
            log.critical("outlier images %s in round %d: these may prevent the calibration from converging", images.tolist(), round_no)
            if answer != "y":
                log.critical('not excluded (options["outliers"] is %r; "y" excludes them)', answer)
                break
            self.missing_poses = np.array(self.missing_poses, dtype=bool)
            self.missing_poses[images] = True
        return np.array(found_all, dtype=np.int64)

    def _estimate_initial_intrinsics(self, n_cams: int, consensus: int = 0) -> np.ndarray:
        """(C, 9) from the detections alone.  A key's board is its index along the FIRST key axis of ``target.point_data`` — the face of a
        Ccube, whether its points are laid out (faces, n, 3) or (faces, rows, cols, 3) — and a target with one key axis, (n, 3), is
        one board.  A free camera without an estimate raises: its rows would be NaN."""
        from . import compiled_helpers as ch

        shape = tuple(int(n) for n in self.target_point_shape[:-1])
        n_keys = int(np.prod(shape))
        try:
            res = np.array([np.asarray(self.camset[idc].res, dtype=np.float64).reshape(2) for idc in range(n_cams)])
        except (TypeError, AttributeError, KeyError, IndexError, ValueError):
            res = None
        n_imgs = self.bundlePrimitive.poses.shape[0] if "pose" in self.bundlePrimitive.groups else self.detection.max_ims
        per_board = int(np.prod(shape[1:])) if len(shape) > 1 else n_keys
        board_of_key = np.arange(n_keys) // per_board
        no_intr = "calc_initial_params: the camset holds no intrinsics (camset[idc].intrinsic / .distortion_coefs)"
        try:
            est = ch.estimate_intrinsics(self._flat_detections(), self.point_data.reshape((-1, 3)), n_cams=n_cams, n_imgs=n_imgs,
                                         board_of_key=board_of_key, res=res, refine=True, device=self.op_fun.device,
                                         consensus=consensus)
        except ch._capi.PcsError as e:
            if e.code != ch._capi.PCS_ERR_NODEVICE:
                raise
            raise ValueError(f"{no_intr} and no device is visible to estimate them: pass intr (C, 9)") from e
        self.initial_intrinsics = est
        lost = [name for idc, name in enumerate(self.cam_names)
                if est.status[idc] == ch.INTR_NOT_ESTIMATED and "int" not in self.fixed_params.get(name, {})]
        if lost:
            raise ValueError(f"{no_intr} and the planar views of {lost} do not give an estimate: pass intr (C, 9)")
        return np.where(np.isfinite(est.intr), est.intr, 0.0)   # rows of fixed cameras without an estimate are replaced below

    def get_detection_data(self, flatten=False) -> np.ndarray:  # th:387-406
        detection = self.detection
        if self.missing_poses is not None and np.any(self.missing_poses):
            detection = self.detection.delete_row(im_num=np.where(self.missing_poses)[0])
        if flatten:
            return detection.return_flattened_keys(self.target_point_shape[:-1]).get_data()
        return detection.get_data()

    def gauge_fixes(self):  # th:417-423
        return None


class SelfBundleHandler(TemplateBundleHandler):  # sbh:109-260
    """Self-calibration: the 3-D target points are free too (chain S), 7-DoF gauge fixed.

    ``options={"gauge": "free"}`` leaves the seven gauge scalars free (unseen features stay fixed): the gauge is then held by a prior
    on the points at their nominal positions — ``slab_prior(handler, {"bdpt": tolerance})`` handed to ``lm_solve`` /
    ``parameter_covariance`` — instead of pinned coordinates; the result stays in the nominal frame and scale.  The default,
    ``"fixed"``, is the reference's mask."""

    chain = "self"

    def _point_mask(self, visible_feature_mask):
        gauge = self.problem_opts.get("gauge", "fixed")
        if gauge not in ("fixed", "free"):
            raise ValueError(f'options["gauge"] must be "fixed" or "free", got {gauge!r}')
        pts = self.flat_point_data.reshape((-1, 3))
        self.fixed_inds = find_not_colinear_pts(pts)  # sbh:153-158: 3 + 3 + 1 coordinates fix the 7-DoF gauge
        i0, i1, i2 = self.fixed_inds
        feat_unfixed = np.ones(self.flat_point_data.shape[0], dtype=bool)
        if gauge == "fixed":
            feat_unfixed[3 * i0 : 3 * i0 + 3] = False
            feat_unfixed[3 * i1 : 3 * i1 + 3] = False
            feat_unfixed[3 * i2] = False
        n_points = int(np.prod(self.point_data.shape[:2]))  # sbh:161
        if visible_feature_mask is not None:
            self.visible_feature_mask = np.asarray(visible_feature_mask, dtype=bool)
            if self.visible_feature_mask.shape[0] != n_points:
                raise ValueError("visible_feature_mask must have one entry per target point")
        else:
            self.visible_feature_mask = np.isin(np.arange(n_points), self._flat_detections()[:, 2])  # sbh:166
        feat_unfixed[: 3 * n_points][np.repeat(~self.visible_feature_mask, 3)] = False  # sbh:167-169: unseen features are fixed
        return feat_unfixed

    def gauge_distance_scale(self, point_estimate) -> float:  # sbh:359-377
        """The reference's scale of a self-calibrated target: the mean ratio of nominal to estimated distance over the pairs of
        ``target.valid_map`` (n, 2), or, for ``valid_map`` True, over all pairs of visible features whose nominal distance is
        ``target.square_size``.  (The reference's array branch calls a function it does not define, sbh:373; the pairs it names are taken.)"""
        pts = np.asarray(point_estimate, dtype=np.float64).reshape((-1, 3))
        ref = np.asarray(self.target.point_data, dtype=np.float64).reshape((-1, 3))
        valid_map = getattr(self.target, "valid_map", True)
        if isinstance(valid_map, (bool, np.bool_)):
            if not valid_map:
                raise ValueError("Target has given a valid map of False, which indicates no distance comparisons are valid.")
            vis = np.nonzero(self.visible_feature_mask)[0]
            a, b = np.triu_indices(vis.shape[0], k=1)
            a, b = vis[a], vis[b]
            keep = np.isclose(np.linalg.norm(ref[a] - ref[b], axis=1), self.target.square_size)
            a, b = a[keep], b[keep]
        elif isinstance(valid_map, np.ndarray) and valid_map.ndim == 2 and valid_map.shape[1] >= 2:
            a, b = valid_map[:, 0].astype(np.int64), valid_map[:, 1].astype(np.int64)
        else:
            raise ValueError("The target.valid_map property either needs to be true, for all comparisons being valid, or a nx2 list of index pairs.")
        if a.shape[0] == 0:
            raise ValueError("no pair of features to compare distances over")
        return float(np.mean(np.linalg.norm(ref[a] - ref[b], axis=1) / np.linalg.norm(pts[a] - pts[b], axis=1)))

    def apply_gauge_transform(self, proj, extr, poses, point_estimate, *, scale: str = "similarity", consensus: int = 0, inlier_dist=None,
                              seed: int = 0, device: int = 0):  # sbh:339-410
        """Bring a self-calibration back to the nominal frame and scale of the target: the similarity that best fits the estimated
        features to ``target.point_data`` over the visible ones, applied so that the calibration is preserved — points X' = U (s X),
        poses U P U^-1 and extrinsics E U^-1 with their translations times s (sbh:378-409), intrinsics untouched — so every residual
        stays what it was, and a first pose that is the identity stays the identity.

        ``scale="similarity"``: s, R and t from one registration on the device (``compiled_helpers.align_points``, the Umeyama scale);
        ``"distances"``: the reference's s (``gauge_distance_scale``) and a rigid registration of the scaled points.  ``consensus`` /
        ``inlier_dist`` / ``seed``: the consensus stage of the registration, against a few features that moved.  Returns new arrays
        (proj, extr (C, 6), poses (I, 6), points (K, 3)); ValueError when the registration is refused, where the reference logs and
        returns the identity."""
        from . import compiled_helpers as ch
        from .pose_seeding import pose_from_4x4, pose_to_4x4, rigid_inverse

        if scale not in ("similarity", "distances"):
            raise ValueError(f"scale must be 'similarity' or 'distances', got {scale!r}")
        pts = np.array(point_estimate, dtype=np.float64).reshape((-1, 3))
        ref = np.asarray(self.target.point_data, dtype=np.float64).reshape((-1, 3))
        vm = np.asarray(self.visible_feature_mask, dtype=bool)
        opts = {"consensus": consensus, "inlier_dist": inlier_dist, "seed": seed, "device": device}
        if scale == "distances":
            s = self.gauge_distance_scale(pts)
            al = ch.align_points(s * pts[vm], ref[vm], model="rigid", **opts)
        else:
            al = ch.align_points(pts[vm], ref[vm], model="similarity", **opts)
            s = float(al.scale[0])
        if al.status[0] != ch.ALIGN_OK:
            raise ValueError(f"apply_gauge_transform: the registration onto the nominal target was refused (status {int(al.status[0])}, "
                             f"{int(al.n_used[0])} features used)")
        self.gauge_alignment = al
        U = np.eye(4)
        U[:3, :3], U[:3, 3] = al.R[0], al.t[0]
        Ui = rigid_inverse(U)
        P, E = pose_to_4x4(np.asarray(poses, dtype=np.float64)), pose_to_4x4(np.asarray(extr, dtype=np.float64))
        P[..., :3, 3] *= s
        E[..., :3, 3] *= s
        return proj, pose_from_4x4(E @ Ui), pose_from_4x4(U @ P @ Ui), s * pts @ U[:3, :3].T + U[:3, 3]


class FreePointBundleHandler(TemplateBundleHandler):  # fph:102-201
    """Classic bundle adjustment of world points without a target pose (chain F)."""

    chain = "free"

    def _point_mask(self, visible_feature_mask):
        return np.ones(self.flat_point_data.shape[0], dtype=bool)  # fph:130

    def calc_initial_params(self, intr=None, *, seeding: str = "reference", scene_opts: dict | None = None, **kw) -> np.ndarray:
        """``seeding="scene"``: the start vector of a scene nobody measured, from the detections alone
        (``pose_seeding.seed_scene``: two-view consensus, triangulation, resection in rounds; the reference has no such start,
        fph:235).  Intrinsics are found as for the other seedings (``intr``, the camset's, or the planar estimate); ``scene_opts``
        reach ``seed_scene`` (``baseline``, ``consensus``, ``inlier_px``, ``seed``, ``min_points``, ``resect_opts``, ``tri_opts``, and
        ``two_view_solver="five-point"`` / ``two_view_refine`` for a scene that is mostly one plane); ``scene_opts["control_points"]``
        (K, 3), NaN where unknown, brings the seed into the frame and scale of those points (``pose_seeding.align_scene``, with
        ``scene_opts["align_opts"]`` as its options): fixed extrinsics must then be given in THAT frame;
        ``ref_cam`` comes from ``options["ref_cam"]``.  The world is ``ref_cam``'s camera frame and the first pair's baseline has
        length ``baseline``: fixed extrinsics must be given in that gauge.  The seed is kept on ``scene_seed``.  ValueError names the
        cameras and keys with a free entry that got no seed.  Every other ``seeding`` is ``TemplateBundleHandler.calc_initial_params``,
        which starts the points at ``flat_point_data``."""
        if seeding != "scene":
            if scene_opts is not None:
                raise ValueError("scene_opts belongs to seeding='scene'")
            return super().calc_initial_params(intr, seeding=seeding, **kw)
        from .pose_seeding import align_scene, seed_scene

        scene_opts = dict(scene_opts or {})
        control_points, align_opts = scene_opts.pop("control_points", None), scene_opts.pop("align_opts", None)
        if align_opts is not None and control_points is None:
            raise ValueError("scene_opts['align_opts'] belongs to scene_opts['control_points']")
        unknown = set(kw) - {"intrinsics_consensus"}
        if unknown:
            raise ValueError(f"seeding='scene' takes intr, scene_opts and intrinsics_consensus, not {sorted(unknown)}")
        cons = kw.get("intrinsics_consensus")
        bp = self.bundlePrimitive
        n_cams = bp.intr.shape[0]
        intr = self._initial_intrinsics(intr, self.problem_opts.get("intrinsics_consensus", 0) if cons is None else cons)
        seed = seed_scene(self._flat_detections(), intr, n_cams, ref_cam=self.problem_opts.get("ref_cam", 0), **scene_opts)
        if control_points is not None:
            seed = align_scene(seed, control_points, **dict(align_opts or {}))
        self.scene_seed = seed
        points = np.full((self.flat_point_data.shape[0] // 3, 3), np.nan)
        points[: seed.points.shape[0]] = seed.points
        flat = points.ravel()
        no_cam = [self.cam_names[c] for c in np.nonzero(np.asarray(bp.extr_unfixed, dtype=bool) & ~seed.placed)[0]]
        no_key = np.unique(np.nonzero(np.asarray(bp.bdpt_unfixed, dtype=bool) & ~np.isfinite(flat))[0] // 3)
        if no_cam or no_key.shape[0]:
            shown = ", ".join(str(k) for k in no_key[:20]) + (", ..." if no_key.shape[0] > 20 else "")
            raise ValueError(f"seeding='scene' left free entries without a seed: cameras {no_cam} were not placed, "
                             f"{no_key.shape[0]} keys were not triangulated ({shown})")
        self.missing_poses = np.zeros(self.detection.max_ims, dtype=bool)
        return np.concatenate([intr[bp.intr_unfixed].ravel(), seed.extr[bp.extr_unfixed].ravel(), flat[bp.bdpt_unfixed]])


def slab_prior(handler, sigmas, means=None):
    """(prior_mean, prior_sigma) on the handler's FREE vector — what ``lm_solve`` / ``parameter_covariance`` /
    ``problem_opts["prior"]`` take — from per-group values.

    Bundle handlers: ``sigmas`` is a dict over the groups ``"intr"`` (C, 9), ``"extr"`` (C, 6), ``"pose"`` (I, 6) and ``"bdpt"`` (the
    point scalars; (K, 3) or flat); a ``ChainProblem``: a list with one entry per slab.  Each entry is anything that broadcasts to its
    slab — a scalar, a row, the full array; ``None``, a missing group or ``np.inf`` mean no prior there.  Only the free entries (the
    per-row masks, the per-scalar point mask) reach the result, in free-vector order.  ``means``: the same structure; a group without
    one takes the handler's current slab — for ``"bdpt"`` the nominal ``point_data``."""
    if isinstance(handler, ChainProblem):
        slabs = [(i, s, m) for i, (s, m) in enumerate(zip(handler.slabs, handler.unfixed))]
        if isinstance(sigmas, dict) or len(sigmas) != len(slabs):
            raise ValueError(f"sigmas: one entry (or None) per slab of the ChainProblem, {len(slabs)} in all")
        if means is not None and len(means) != len(slabs):
            raise ValueError(f"means: one entry (or None) per slab of the ChainProblem, {len(slabs)} in all")
        pick = lambda d, k: None if d is None else d[k]   # noqa: E731
    else:
        bp = handler.bundlePrimitive
        unknown = set(sigmas) - set(bp.groups) | (set(means or {}) - set(bp.groups))
        if unknown:
            raise ValueError(f"unknown parameter groups {sorted(unknown)}: this handler has {list(bp.groups)}")
        slabs = []
        for g in bp.groups:
            slab_name, mask_name, width = _GROUP[g]
            slab, mask = getattr(bp, slab_name), np.asarray(getattr(bp, mask_name), dtype=bool)
            if g == "bdpt":   # the nominal target, not the primitive's working copy (a solve scatters its iterates into that)
                slab = np.asarray(handler.point_data, dtype=np.float64).reshape(-1)
            slabs.append((g, slab, mask if width == 1 else np.repeat(mask[:, None], width, axis=1)))
        pick = lambda d, k: None if d is None else d.get(k)   # noqa: E731
    mean_parts, sigma_parts = [], []
    for key, slab, mask in slabs:
        slab = np.asarray(slab, dtype=np.float64)

        def spread(v, what):
            v = np.asarray(v, dtype=np.float64)
            if v.size == slab.size:
                return v.reshape(slab.shape)
            try:
                return np.broadcast_to(v, slab.shape)
            except ValueError:
                raise ValueError(f"{what}[{key!r}] of shape {v.shape} does not broadcast to the slab {slab.shape}") from None

        sg, mu = pick(sigmas, key), pick(means, key)
        sg = np.full(slab.shape, np.inf) if sg is None else spread(sg, "sigmas")
        mu = slab if mu is None else spread(mu, "means")
        if np.any(np.isnan(sg)) or not np.all(sg > 0.0):
            raise ValueError(f"sigmas[{key!r}]: every value must be > 0 (np.inf: no prior)")
        mean_parts.append(np.asarray(mu)[mask])
        sigma_parts.append(np.asarray(sg)[mask])
    return np.concatenate(mean_parts).astype(np.float64), np.concatenate(sigma_parts).astype(np.float64)


def slab_bounds(handler, lo_per_group, hi_per_group):
    """(lo, hi) on the handler's FREE vector — what ``lm_solve(bounds=)`` / ``problem_opts["bounds"]`` take — from per-group values;
    the mirror of ``slab_prior``.

    Bundle handlers: each argument is a dict over the groups ``"intr"`` (C, 9), ``"extr"`` (C, 6), ``"pose"`` (I, 6) and ``"bdpt"``, or
    ``None``; a ``ChainProblem``: a list with one entry per slab, or ``None``.  Each entry is anything that broadcasts to its slab — a
    scalar, a row, the full array — with ``-np.inf`` / ``np.inf`` for no bound; ``None`` or a missing group means no bound there; or
    ``("rel", width)``: the handler's current slab minus (``lo``) or plus (``hi``) ``width * |slab|``, ``width`` broadcasting likewise.
    Only the free entries reach the result, in free-vector order."""
    if isinstance(handler, ChainProblem):
        slabs = [(i, s, m) for i, (s, m) in enumerate(zip(handler.slabs, handler.unfixed))]
        for name, d in (("lo_per_group", lo_per_group), ("hi_per_group", hi_per_group)):
            if d is not None and (isinstance(d, dict) or len(d) != len(slabs)):
                raise ValueError(f"{name}: one entry (or None) per slab of the ChainProblem, {len(slabs)} in all")
        pick = lambda d, k: None if d is None else d[k]   # noqa: E731
    else:
        bp = handler.bundlePrimitive
        unknown = (set(lo_per_group or {}) | set(hi_per_group or {})) - set(bp.groups)
        if unknown:
            raise ValueError(f"unknown parameter groups {sorted(unknown)}: this handler has {list(bp.groups)}")
        slabs = []
        for g in bp.groups:
            slab_name, mask_name, width = _GROUP[g]
            slab, mask = getattr(bp, slab_name), np.asarray(getattr(bp, mask_name), dtype=bool)
            if g == "bdpt":
                slab = np.asarray(handler.point_data, dtype=np.float64).reshape(-1)
            slabs.append((g, slab, mask if width == 1 else np.repeat(mask[:, None], width, axis=1)))
        pick = lambda d, k: None if d is None else d.get(k)   # noqa: E731
    lo_parts, hi_parts = [], []
    for key, slab, mask in slabs:
        slab = np.asarray(slab, dtype=np.float64)
        mask = np.ones(slab.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)

        def side(v, sign, what):
            if v is None:
                return np.full(slab.shape, sign * np.inf)
            rel = isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str)
            if rel and v[0] != "rel":
                raise ValueError(f"{what}[{key!r}]: expected ('rel', width), got {v[0]!r}")
            a = np.asarray(v[1] if rel else v, dtype=np.float64)
            try:
                a = a.reshape(slab.shape) if a.size == slab.size else np.broadcast_to(a, slab.shape)
            except ValueError:
                raise ValueError(f"{what}[{key!r}] of shape {a.shape} does not broadcast to the slab {slab.shape}") from None
            if np.any(np.isnan(a)) or (rel and np.any(a < 0.0)):
                raise ValueError(f"{what}[{key!r}]: NaN or a negative relative width")
            return slab + sign * a * np.abs(slab) if rel else np.array(a)

        lo_parts.append(side(pick(lo_per_group, key), -1.0, "lo_per_group")[mask])
        hi_parts.append(side(pick(hi_per_group, key), 1.0, "hi_per_group")[mask])
    lo, hi = np.concatenate(lo_parts).astype(np.float64), np.concatenate(hi_parts).astype(np.float64)
    if np.any(lo > hi):
        k = int(np.flatnonzero(lo > hi)[0])
        raise ValueError(f"slab_bounds: lower bound {lo[k]} > upper bound {hi[k]} at free index {k}")
    return lo, hi


class ChainProblem:
    """The handler protocol for ANY chain of function blocks — what ``device_solver.lm_solve`` and a scipy caller need from a
    handler (template_handler.py:154-240: ``op_fun``, ``make_loss_fun``, ``make_loss_jac``, ``get_bundle_adjustment_inputs``) without
    the target / camera-set model around it.  The three bundle handlers above are tied to the reference's three chains; a chain
    the user composes (generated kernels, user blocks) brings its own parameter groups, so this class takes them as they are:

        op   = projection() + extrinsic3D() + rigidTform3d() + template_points()
        prob = ChainProblem(op, detections, [intr, extr, poses_a, poses_b], template=points,
                            unfixed=[None, None, None, mask_b])            # one array per block, like build_param_list
        res  = lm_solve(prob, prob.x0)                                     # J stays on the device
        res, slabs = run_bundle_adjustment(prob, solver="device")          # the reference's caller (optimisation_handling.py:52-117)
        scipy.optimize.least_squares(prob.make_loss_fun(), prob.x0, jac=prob.make_loss_jac(), x_scale='jac')

    ``slabs``: one array per argument of ``build_param_list`` (afb:669-681), i.e. per parameter GROUP in string order (blocks that
    share a parameter object share one array); ``unfixed``: a boolean array per slab (None = all free).  The free vector ``x`` is the
    concatenation of the slabs' free entries in string order."""

    def __init__(self, op_fun, detections, slabs, *, template=None, unfixed=None, options=None):
        # what optimisation_handling.run_bundle_adjustment reads from a handler (oh:52-117): the reference's option names and defaults
        # (template_handler.py:110-118)
        self.problem_opts = {"verbosity": 0, "max_nfev": 100}
        self.problem_opts.update(options or {})
        self.op_fun = op_fun
        self.det = np.ascontiguousarray(detections, dtype=np.float64)
        self.slabs = [np.array(s, dtype=np.float64) for s in slabs]
        masks = unfixed if unfixed is not None else [None] * len(self.slabs)
        if len(masks) != len(self.slabs):
            raise ValueError("one unfixed mask (or None) per slab")
        self.unfixed = [np.ones(s.shape, dtype=bool) if m is None else np.broadcast_to(np.asarray(m, dtype=bool), s.shape).copy() for s, m in zip(self.slabs, masks)]
        self.template = None if template is None else np.ascontiguousarray(template, dtype=np.float64).reshape(-1, 3)
        self.x0 = np.concatenate([s[m] for s, m in zip(self.slabs, self.unfixed)])

    # -- what run_bundle_adjustment asks of a handler (oh:24-49) ------------------------------------------------------------------------
    def get_initial_params(self):
        return self.x0.copy()

    def can_make_jac(self):
        return True

    # -- what lm_solve asks of a handler ---------------------------------------------------------------------------------------------
    def _flat_detections(self):
        return self.det

    def _template_arg(self):
        return self.template

    def _jac_mask(self):
        return np.concatenate([m.ravel() for m in self.unfixed])

    def get_bundle_adjustment_inputs(self, x):
        x = np.asarray(x, dtype=np.float64)
        out, at = [], 0
        for s, m in zip(self.slabs, self.unfixed):
            k = int(m.sum())
            t = s.copy()
            t[m] = x[at: at + k]
            at += k
            out.append(t)
        if at != x.shape[0]:
            raise ValueError(f"x has {x.shape[0]} entries, the problem has {at} free parameters")
        return out

    # -- the closures scipy takes (th:157-193) -------------------------------------------------------------------------------------
    def _param_str(self, x):
        return self.op_fun.build_param_list(*self.get_bundle_adjustment_inputs(x))

    def make_loss_fun(self, threads=1):
        loss = self.op_fun.make_full_loss_fn(self.det, threads)
        tm = () if self.template is None else (self.template,)
        return lambda x: np.asarray(loss(self._param_str(x), *tm)).reshape(-1)

    def make_loss_jac(self, threads=1):
        from scipy.sparse import csr_array

        jac = self.op_fun.make_jacobean(self.det, threads, unfixed_params=self._jac_mask())
        tm = () if self.template is None else (self.template,)
        shape = (2 * self.det.shape[0], int(self._jac_mask().sum()))

        def jac_fn(x):
            data, indices, indptr = jac(self._param_str(x), *tm)
            return csr_array((data, indices, indptr), shape=shape)

        return jac_fn
