"""The INTEGRATION.md "two-line patch": a handler's ``self.op_fun`` replaced by the adapter of ``pycamset_amd.function_blocks``.

The handler is ``pycamset_amd.handlers``' restatement of the reference's ``TemplateBundleHandler`` / ``SelfBundleHandler`` /
``FreePointBundleHandler``, rebuilt from the inputs stored beside the reference's own outputs (tests/golden/patch_*.npz,
made by tests/golden/make_golden.py from the UNPATCHED reference handlers: ``op_fun`` at template_handler.py:152,
standard_bundle_handler.py:182, free_point_handler.py:143; ``make_loss_fun`` / ``make_loss_jac`` at th:157-193).  Then:

  1. with the real engine: every attribute the handler touches exists on the adapter and the only failure in a
     GPU-less container is ``PcsError(PCS_ERR_NODEVICE)`` out of ``pcs_create`` (there is no CPU fallback to hide it);
  2. with a test-only stand-in for ``Engine`` (arithmetic by the CPU oracle — test infrastructure, never the product):
     the closures built around the adapter return what the unpatched reference returned.
"""
import numpy as np
import pytest
from scipy.sparse import csr_array

from oracle import ba_oracle as orc
from pycamset_amd import _capi
from pycamset_amd import function_blocks as hip_fb
from pycamset_amd.detections import TargetDetection
from tests.test_host_logic import HANDLERS, DuckCamset, DuckTargetND
from tests.test_oracle_golden import assert_close


def hip_chain(chain):
    if chain == "template":
        return hip_fb.projection() + hip_fb.extrinsic3D() + hip_fb.template_points()
    if chain == "self":
        return hip_fb.projection() + hip_fb.extrinsic3D() + hip_fb.rigidTform3d() + hip_fb.free_point()
    return hip_fb.projection() + hip_fb.extrinsic3D() + hip_fb.free_point()


class OracleEngine:
    """TEST-ONLY stand-in for pycamset_amd.engine.Engine (same methods the adapter calls), CPU oracle inside."""

    def __init__(self, chain, n_cams, n_imgs, n_keys, *, dtype="f64", device=0):
        self.chain, self.counts = chain, (int(n_cams), int(n_imgs), int(n_keys))
        self.P = orc.CHAIN_P[chain]
        self.n_keys = int(n_keys)
        self.mask_key = self.nnz = self.template = None

    def set_detections_table(self, det):
        self.det = np.array(det, dtype=np.float64)
        self.n = self.det.shape[0]
        self.n_params = int(orc.param_struct(self.chain, self.det, self.counts)[2])

    def set_template(self, t):
        self.template = np.array(t, dtype=np.float64).reshape(-1, 3)

    def eval(self, ps, want_resid=True, want_jac=True, pinned_ring=0):
        assert ps.shape[0] == self.n_params
        r = orc.full_loss(self.chain, self.det, ps, self.template, counts=self.counts) if want_resid else None
        j = orc.full_jac_dense(self.chain, self.det, ps, self.template, counts=self.counts) if want_jac else None
        return r, j

    def csr_structure(self, unfixed):
        return orc.csr_structure(self.chain, self.det, unfixed, self.counts)[:2]

    def set_unfixed(self, unfixed):
        self.mask = np.asarray(unfixed, dtype=bool)
        self.mask_key = hash(self.mask.tobytes())
        self.keep = orc.csr_structure(self.chain, self.det, self.mask, self.counts)[2]
        self.nnz = int(self.keep.sum())
        return self.nnz

    def eval_compact(self, ps, want_resid=False, pinned_ring=0):
        return None, self.eval(ps, False, True)[1][self.keep]

    def block_param_inds(self):
        return orc.block_param_inds(self.chain, self.det, self.counts)


def _problem(golden_dir, chain, max_ims=0):
    """-> (handler, x, fixture): the handler of the fixture's problem, with the reference's layout rule (max index + 1,
    afb:793-795) like the reference handler the fixture was made with, and the fixture's free vector."""
    g = np.load(golden_dir / f"patch_{chain}_ims{max_ims}.npz")
    n_cams = int(g["n_cams"])
    names = [f"cam_{i}" for i in range(n_cams)]
    fixed = {}
    for c in range(n_cams):
        if not g["intr_unfixed"][c]:
            fixed.setdefault(names[c], {})["int"] = g["intr_slab"][c].copy()
        if not g["extr_unfixed"][c]:
            fixed.setdefault(names[c], {})["ext"] = g["extr_slab"][c].copy()
    det = TargetDetection(names, g["detections"], max_ims=max_ims)
    target = DuckTargetND(g["points"], tuple(int(k) for k in g["keydims"]))
    h = HANDLERS[chain](DuckCamset(n_cams), target, det, fixed_params=fixed, options={"verbosity": 0, "fixed_pose": 0},
                        counts="reference")
    bp = h.bundlePrimitive
    masks = ["intr_unfixed", "extr_unfixed"] + (["poses_unfixed"] if chain != "free" else []) + (["bdpt_unfixed"] if chain != "template" else [])
    for m in masks:   # the free vector of the fixture means the same parameters here
        assert np.array_equal(getattr(bp, m), g[m]), m
    return h, g["x"].copy(), g


@pytest.mark.parametrize("chain", ["template", "self", "free"])
def test_patched_reference_handler_reaches_pcs_create(golden_dir, chain):
    h, x, _ = _problem(golden_dir, chain)
    h.op_fun = hip_chain(chain)                      # <- the patch
    assert h.can_make_jac() is True                  # th:154-155
    if _capi.lib().pcs_device_count() > 0:
        pytest.skip("a GPU is visible: the closure tests in test_gpu_dropin.py cover the live path")
    for make in (h.make_loss_fun, h.make_loss_jac):
        with pytest.raises(_capi.PcsError) as err:
            make(4)
        assert err.value.code == _capi.PCS_ERR_NODEVICE, "every step up to pcs_create must succeed on the host"


@pytest.mark.parametrize("chain,max_ims", [("template", 0), ("self", 0), ("free", 0), ("template", 6), ("self", 6)])
def test_patched_reference_handler_returns_what_the_reference_returns(golden_dir, chain, max_ims, monkeypatch):
    """max_ims = 6 > 4 images: the handler's pose slab (and mask) is longer than the string the detections index —
    the reference reads only the leading entries (afb:363) and, in the self chain, mis-offsets the point block
    (quirk ii); the patched handler must do exactly the same."""
    h, x, g = _problem(golden_dir, chain, max_ims)
    r_ref, J_ref = g["resid"], csr_array((g["data"], g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    monkeypatch.setattr(hip_fb, "Engine", OracleEngine)      # test-only: no GPU in the build container
    h.op_fun = hip_chain(chain)                               # <- the patch
    r = h.make_loss_fun(3)(x.copy())
    J = h.make_loss_jac(3)(x.copy())
    assert r.shape == r_ref.shape and J.shape == J_ref.shape
    assert np.array_equal(J.indices, J_ref.indices) and np.array_equal(J.indptr, J_ref.indptr)
    assert_close(r, r_ref, rtol=1e-11, rows=1e3 * np.repeat(np.max(np.abs(g["detections"][:, -2:]), axis=1), 2))
    dense_rows = np.repeat(np.max(np.abs(J_ref).toarray(), axis=1), np.diff(J_ref.indptr))
    assert_close(J.data, J_ref.data, rows=dense_rows)
