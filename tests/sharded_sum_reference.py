"""Reference side of the sharded-sum tests (tests/test_gpu_sharded_sum.py, tests/test_sharded_sum_reference.py): one detection table, the
row ranges the ranks hold, the per-solve settings (loss, noise weights, prior) and the oracle of the WHOLE table with the whole weight
vector, the loss, and the prior added once — what every rank of a sharded solve must hold after the sum over the ranks.

    p = problem("ring4", "template", "prior+weights+huber")     the table, the handler's mask and start, the settings
    p.parts("empty")                                            one slice per rank
    H, g, c, slack = p.system(ps)                               over the whole string: weights_reference.weighted_system + the prior once
    H, g, c, slack = p.shard_sum(ps, parts)                     the same from the ranks' own systems, the prior behind the sum

No device work here: the module is imported by the host test too."""
import numpy as np

from oracle import ba_oracle as orc
from pycamset_amd import handlers, synthetic
from pycamset_amd.detections import TargetDetection
from tests import prior_reference as PR
from tests import weights_reference as W
from tests.test_host_logic import DuckCamset, DuckTarget

PER_CAMERA_SIGMA = np.array([0.5, 1.0, 2.0, 4.0])
# name: (loss, f_scale, weights: None | "detection" (log-uniform per detection) | "camera" (per-camera sigma), planted outliers, prior)
SETTINGS = {
    "linear": ("linear", 1.0, None, False, False),
    "weights": ("linear", 1.0, "detection", False, False),
    "weights+huber": ("huber", 2.5, "detection", True, False),
    "huber": ("huber", 2.5, "camera", True, False),
    "cauchy": ("cauchy", 1.0, "camera", True, False),
    "prior": ("linear", 1.0, None, False, True),
    "prior+huber": ("huber", 2.5, "camera", True, True),
    "prior+weights+huber": ("huber", 2.5, "detection", True, True),
}
SPLITS = ("two", "empty", "onecam")


def rig_of(name):
    """ring4: weights_reference.ring4(); ring8: the ring-8-small rig of tests/test_gpu_lm_trials.py ``_ring8``."""
    if name == "ring4":
        return W.ring4()
    assert name == "ring8", name
    return synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)


def plant_outliers(det, seed=5):
    """~3 % of the detections moved by 20 - 50 px (tests/test_gpu_robust_loss.py ``_outlier_problem``)."""
    det = det.copy()
    rng = np.random.default_rng(seed)
    bad = rng.choice(det.shape[0], max(1, int(0.03 * det.shape[0])), replace=False)
    ang, mag = rng.uniform(0, 2 * np.pi, bad.size), rng.uniform(20.0, 50.0, bad.size)
    det[bad, 3] += mag * np.cos(ang)
    det[bad, 4] += mag * np.sin(ang)
    return det


def split(det, name):
    """One slice of the table per rank.  two: 60 % / 40 % of the rows in table order; empty: the same with a third, empty rank;
    onecam: three ranks, the middle one holds only the rows of the last camera (the table is ordered camera -> image -> key), so every
    block of its state that belongs to another camera is zero."""
    n = det.shape[0]
    a = (6 * n) // 10
    if name == "two":
        return [slice(0, a), slice(a, n)]
    if name == "empty":
        return [slice(0, a), slice(a, n), slice(n, n)]
    assert name == "onecam", name
    cam = det[:, 0].astype(np.int64)
    assert np.all(np.diff(cam) >= 0), "the table is ordered by camera"
    c0 = int(np.searchsorted(cam, cam[-1]))
    assert 0 < c0 < n
    return [slice(0, c0 // 2), slice(c0, n), slice(c0 // 2, c0)]


def string_prior(h, chain, seed=4):
    """(mean, inv_sigma) over the parameter string: the prior of test_solves_with_a_prior_match_scipy_through_every_loop (tests/test_gpu_prior.py)
    — the distortion terms of every camera, the translations of every pose and, for the self chain, every free point coordinate; the
    other entries np.inf — and (mean, sigma) over the free vector, as ``lm_solve`` takes it."""
    groups = {"intr": np.r_[np.full(4, np.inf), np.full(5, 0.02)], "pose": np.r_[np.full(3, np.inf), np.full(3, 5.0)]}
    if chain == "self":
        groups["bdpt"] = 0.05
    mean, sigma = handlers.slab_prior(h, groups)
    mean = mean + np.where(np.isinf(sigma), 0.0, sigma) * np.random.default_rng(seed).standard_normal(mean.shape)
    w = PR.weights_of(sigma)
    mask = np.asarray(h._jac_mask(), dtype=bool)
    free = np.flatnonzero(mask)
    mean_s, w_s = np.zeros(mask.shape[0]), np.zeros(mask.shape[0])
    mean_s[free], w_s[free] = np.where(w > 0.0, mean, 0.0), w
    assert np.any(w > 0.0) and np.any(w == 0.0)
    return (mean_s, w_s), (mean, sigma)


class Problem:
    """One table, one chain, one setting."""

    def __init__(self, rig_name, chain, setting, scale=1.0):
        self.rig_name, self.chain, self.setting = rig_name, chain, setting
        self.loss, self.f_scale, weights, outliers, with_prior = SETTINGS[setting]
        rig = self.rig = rig_of(rig_name)
        det = self.det = plant_outliers(rig.detections) if outliers else rig.detections
        self.counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
        self.tm = rig.points if chain == "template" else None
        names = [f"cam_{i}" for i in range(rig.n_cams)]
        cls = handlers.TemplateBundleHandler if chain == "template" else handlers.SelfBundleHandler
        h = self.h = cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, det),
                         fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})
        assert np.array_equal(h._flat_detections(), det)
        bp = h.bundlePrimitive
        # the start: `scale` times the rig's perturbation away from the truth (tests/test_gpu_lm_trials.py ``_ring8``)
        intr, extr, poses = (t + scale * (p - t) for t, p in ((rig.intr_true, rig.intr), (rig.extr_true, rig.extr), (rig.poses_true, rig.poses)))
        parts = [intr[bp.intr_unfixed].ravel(), extr[bp.extr_unfixed].ravel(), poses[bp.poses_unfixed].ravel()]
        if chain == "self":
            parts.append(rig.points.ravel()[bp.bdpt_unfixed])
        self.x0 = np.concatenate(parts)
        self.mask = np.asarray(h._jac_mask(), dtype=bool)
        self.ps0 = h.op_fun.build_param_list(*h.get_bundle_adjustment_inputs(self.x0.copy()))
        n = det.shape[0]
        self.sigma = None           # as lm_solve(sigma=) takes it for the whole table
        if weights == "detection":
            self.w = W.log_uniform_weights(n, 11)
            self.sigma = {"detection": 1.0 / self.w}
        elif weights == "camera":
            per_cam = PER_CAMERA_SIGMA[np.arange(rig.n_cams) % 4]
            self.w = 1.0 / per_cam[det[:, 0].astype(np.int64)]
            self.sigma = {"camera": per_cam}
        else:
            self.w = None
        self.prior, self.free_prior = string_prior(h, chain) if with_prior else (None, None)

    def parts(self, name):
        return split(self.det, name)

    def weights_of(self, rows=slice(None)):
        return (np.ones(self.det.shape[0]) if self.w is None else self.w)[rows]

    def detections_system(self, ps, rows=slice(None)):
        """(H, g, sum rho, slack of H) over the whole string from the rows ``rows`` of the table with their own weights: no prior."""
        return W.weighted_system(self.chain, self.det[rows], ps, self.tm, self.weights_of(rows), self.loss, self.f_scale, counts=self.counts)

    def add_prior(self, H, g, c, ps):
        """The prior's diagonal w^2, gradient w^2 (p - mean) and cost sum (w (p - mean))^2 (prior_reference.prior_system): once."""
        return (H, g, c) if self.prior is None else PR.prior_system(H, g, c, ps, *self.prior)

    def system(self, ps):
        H, g, c, slack = self.detections_system(ps)
        return self.add_prior(H, g, c, ps) + (slack,)

    def shard_sum(self, ps, parts, prior_per_rank=False):
        """The ranks' own systems summed in rank order, the prior behind the sum — or, ``prior_per_rank``, in front of it on every rank:
        the mistake the sharded tests are there to catch."""
        n = ps.shape[0]
        H, g, c, slack = np.zeros((n, n)), np.zeros(n), 0.0, 0.0
        for rows in parts:
            if self.det[rows].shape[0] == 0:
                Hr, gr, cr, sr = np.zeros((n, n)), np.zeros(n), 0.0, 0.0
            else:
                Hr, gr, cr, sr = self.detections_system(ps, rows)
            if prior_per_rank:
                Hr, gr, cr = self.add_prior(Hr, gr, cr, ps)
            H, g, c, slack = H + Hr, g + gr, c + cr, slack + sr
        return ((H, g, c) if prior_per_rank else self.add_prior(H, g, c, ps)) + (slack,)

    # ---- what tests/test_gpu_lm_trials.py check_trials asks of its fixture
    def oracle(self, ps):
        """(H, g over the free entries, cost, slack of H) at the parameter string ps."""
        H, g, c, slack = self.system(ps)
        m = self.mask
        return H[np.ix_(m, m)], g[m], c, (slack[np.ix_(m, m)] if np.ndim(slack) else slack)

    def oracle_cost(self, ps):
        f = W.rows_of(self.weights_of()) * orc.full_loss(self.chain, self.det, ps, self.tm, counts=self.counts).reshape(-1)
        if self.loss == "linear":
            c = float(f @ f)
        else:
            from scipy.optimize._lsq.least_squares import construct_loss_function
            c = float(np.sum(construct_loss_function(f.size, self.loss, self.f_scale)(f, cost_only=False)[0]))
        return c if self.prior is None else c + 2.0 * PR.prior_half_sum(ps, *self.prior)


def problem(rig_name, chain, setting, scale=1.0):
    return Problem(rig_name, chain, setting, scale)
