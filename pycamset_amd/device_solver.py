"""Levenberg-Marquardt with the Jacobian kept on the device.

The reference hands a 2N x n_free CSR matrix to ``scipy.optimize.least_squares``
(optimisation_handling.py:88-98), which scales its columns (x_scale='jac'), forms J^T f and runs
lsmr mat-vecs on the host.  Here J only exists as matrix-free products on the GPU
(csrc/ba_matfree.hpp): per LM iteration the host sees n_params-sized vectors only, so neither the
PCIe copy of J (335 MB at N = 1e6) nor — when sharded — an all-gather of J is needed: ranks
all-reduce J^T J v, diag(J^T J) and J^T r (a few KB).

    op  = JacobianOperator(engine, unfixed_mask)          # products in the FREE parameter space
    res = lm_solve(handler, x0)                           # drop-in for run_bundle_adjustment's solve
    res = lm_solve(handler, x0, linear_solver="cholesky") # block-reduced J^T J per step + dense Cholesky

Two ways to get the LM step from the GPU: ``"pcg"`` — Jacobi-preconditioned CG on matrix-free
J^T (J v) products (~150 passes over the detections per step, parameter-sized traffic only); and
``"cholesky"`` — one pass of csrc/ba_normal.hpp builds J^T J, J^T r and the cost in BLOCKED form
([A | B | C]: leading x leading, leading x trailing, block-diagonal trailing group) and the damped system is
reduced by the Schur complement of the trailing group (csrc/ba_schur.hpp: the block parts and both products on the FP64
matrix cores; csrc/ba_chol_persist.hpp: the dense Cholesky of the leading size in one persistent launch) — HIP kernels only; the
vendor-library variants kept for A/B until round 4 live in tools/library_solver.py.  That loop is device-resident: parameter
string, step, damping, gain ratio, the accept / reject decision AND the termination rules live in HBM, the host reads ONE small
vector per trial to follow it.  The sharded form all-reduces the packed [A | B | C | g | cost | votes] once per trial — on the
solver's stream between the two halves of a trial when the collective is RCCL (no host synchronisation), through the host for gloo.

``as_linear_operator()`` exposes J as a scipy LinearOperator (matvec / rmatvec) for callers that
want scipy's own solvers without materialising J.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field

import time

import numpy as np

from ._capi import LOSS_IDS
from .engine import Engine, bounds_arrays, expand_sigma


class JacobianOperator:
    """J(x) restricted to the free parameters, at the engine's current linearisation point.

    ``reduce_fn`` (optional) sums an n-vector across ranks (sharded detections): it is applied to every
    parameter-space result and to the cost.
    """

    def __init__(self, engine, unfixed=None, reduce_fn=None):
        self.eng = engine
        mask = np.ones(engine.n_params, dtype=bool) if unfixed is None else np.asarray(unfixed, dtype=bool)
        if mask.shape[0] != engine.n_params:
            raise ValueError("mask must have one entry per parameter")
        self.free = np.flatnonzero(mask)
        self.n_free = self.free.shape[0]
        self.reduce_fn = reduce_fn
        self._full = np.zeros(engine.n_params)

    def _expand(self, v_free):
        self._full[:] = 0.0
        self._full[self.free] = v_free
        return self._full

    def _red(self, v):
        return self.reduce_fn(v) if self.reduce_fn is not None else v

    # A rank whose shard is EMPTY (ceil(N / world) rows per rank can leave the last ranks without any: N = 9, world = 4)
    # contributes zeros and still takes part in every collective — raising there would leave the other ranks blocked
    # in their all-reduce.
    @property
    def _empty(self) -> bool:
        return self.eng.n == 0

    def linearize(self, param_str):
        if not self._empty:
            self.eng.linearize(param_str)

    def jv(self, v_free):          # (2N_local,) — stays per rank
        return np.zeros(0) if self._empty else self.eng.jv(self._expand(v_free))

    def jtu(self, u):
        return self._red(np.zeros(self.n_free) if self._empty else self.eng.jtu(u)[self.free])

    def jtjv(self, v_free):
        return self._red(np.zeros(self.n_free) if self._empty else self.eng.jtjv(self._expand(v_free))[self.free])

    def diag(self):
        return self._red(np.zeros(self.n_free) if self._empty else self.eng.jtj_diag()[self.free])

    def grad(self):
        g, c = (np.zeros(self.eng.n_params), 0.0) if self._empty else self.eng.grad()
        if self.reduce_fn is not None:
            packed = self.reduce_fn(np.concatenate([g[self.free], [c]]))
            return packed[:-1], float(packed[-1])
        return g[self.free], c

    def as_linear_operator(self):
        from scipy.sparse.linalg import LinearOperator

        return LinearOperator((2 * self.eng.n, self.n_free), matvec=self.jv, rmatvec=self.jtu, dtype=np.float64)


def pcg(apply_a, b, m_inv, tol: float, max_iter: int):
    """Jacobi-preconditioned conjugate gradients for the SPD damped normal equations."""
    x = np.zeros_like(b)
    r = b.copy()
    z = m_inv * r
    p = z.copy()
    rz = float(r @ z)
    b_norm = float(np.sqrt(b @ (m_inv * b))) or 1.0
    it = 0
    for it in range(1, max_iter + 1):
        ap = apply_a(p)
        pap = float(p @ ap)
        if pap <= 0:
            break
        alpha = rz / pap
        x += alpha * p
        r -= alpha * ap
        z = m_inv * r
        rz_new = float(r @ z)
        if np.sqrt(max(rz_new, 0.0)) <= tol * b_norm:
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it


LAM0_EXACT = 1e-5           # initial damping of the exact (Cholesky) step; 1e-3 for the inexact PCG step (lm_solve's docstring has the why)
LAM_GROW0 = 1e3             # factor a rejected trial applies to lambda before the first accepted step (lm_solve)
LAM_FAST = (0.95, 0.1)      # a gain ratio above 0.95 multiplies lambda by 0.1 instead of 1/3: a model THAT accurate lets the damping go quickly
LEAD_LIMIT = 16384          # leading parameters up to which lm_solve(linear_solver="auto") takes the Schur / Cholesky step (S: 2 GB)
BLOCKED_BYTES_LIMIT = 96e9  # and total bytes of the two packed buffers + V + S (a third of the part's 288 GB)


REGION_LIMIT = 2 ** 32     # doubles per region of the packed buffer: the build addresses A, B and C with 32-bit offsets in doubles (pcs_engine.hip enqueue_normal; 2^29 until round 4)


def blocked_fits(engine) -> bool:
    """Can ``linear_solver='auto'`` take the blocked normal equations + Schur / Cholesky step on this engine?  False for leading
    groups beyond LEAD_LIMIT, for buffers beyond BLOCKED_BYTES_LIMIT and for any single region A / B / C of 2^32 doubles or more (the
    build would refuse it).  A generated chain has the DENSE form of the same state (every parameter leading, csrc/ba_blockgram.hpp):
    the same limits apply to its n_params, plus the contraction's own (FP64 block rows of at most 63 columns)."""
    if not hasattr(engine, "normal_layout"):
        return False
    if hasattr(engine, "dense_lm_supported") and not engine.dense_lm_supported():
        return False
    lay = engine.normal_layout()
    n_lead, n_trail, tb = lay["n_lead"], lay["n_trail"], lay["tb"]
    if max(n_lead * n_lead, n_lead * n_trail, n_trail * tb) >= REGION_LIMIT:
        return False
    return n_lead <= LEAD_LIMIT and 8.0 * (2 * lay["packed_len"] + n_lead * n_trail + n_lead ** 2) <= BLOCKED_BYTES_LIMIT


class BlockedNormalEquations:
    """J^T J in blocked form + the Schur-complement step, all on the device (engine.normal_blocks_device,
    engine.schur_prepare / schur_finish; include/pcs_hip.h).  Two packed states (current, trial): in the device-steered loop a
    device word says which is which and an accepted trial flips it (include/pcs_hip.h pcs_lm_buffers)."""

    def __init__(self, engine, unfixed=None, reduce_fn=None):
        import torch

        self.torch, self.eng, self.reduce_fn = torch, engine, reduce_fn
        lay = engine.normal_layout()
        self.n_lead, self.n_trail, self.tb, self.n_params = lay["n_lead"], lay["n_trail"], lay["tb"], lay["n_params"]
        self.n_ent = self.n_trail // self.tb
        self.n_packed = lay["packed_len"]            # [A | B | C | g | cost]; one more word behind it: the ranks' void votes
        mask = np.ones(self.n_params, dtype=bool) if unfixed is None else np.asarray(unfixed, dtype=bool)
        if mask.shape[0] != self.n_params:
            raise ValueError("mask must have one entry per parameter")
        self.free = np.flatnonzero(mask)
        self.n_free = self.free.shape[0]
        dev = self.dev = torch.device("cuda", engine.device)
        f64 = dict(dtype=torch.float64, device=dev)
        n_alloc = self.n_packed + 1 + ((self.n_packed + 1) & 1)     # an even number of doubles: both states 16-byte aligned in any allocator
        self.packed = [torch.zeros(n_alloc, **f64)[: self.n_packed + 1] for _ in range(2)]
        self.fixed = torch.from_numpy((~mask).astype(np.uint8)).to(dev)
        self.free_idx = torch.from_numpy(self.free).to(dev)
        self.linvt = torch.empty(max(1, self.n_ent * self.tb * self.tb), **f64)
        self.u = torch.empty(max(1, self.n_trail), **f64)
        self.V = torch.empty((self.n_lead, max(1, self.n_trail)), **f64)
        self.S = torch.empty((self.n_lead, self.n_lead), **f64)
        self.rhs = torch.empty(self.n_lead, **f64)
        self.dvec = torch.empty(self.n_params, **f64)
        self.gm = torch.empty(self.n_params, **f64)
        self.delta = torch.empty(self.n_params, **f64)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        from .engine import dense_spd_work_len

        self.xl = torch.empty(self.n_lead, **f64)
        self.w = torch.empty(max(1, self.n_trail), **f64)
        self.chol_work = torch.empty(dense_spd_work_len(self.n_lead), **f64)
        from .engine import schur_syrk_work_len

        # the ordered S -= V V' of the engine's deterministic mode parks the partial products of its K split here (0: not split)
        self.syrk_work_len = schur_syrk_work_len(self.n_lead, self.n_trail) if self.n_trail else 0
        self.syrk_work = torch.empty(max(1, self.syrk_work_len), **f64)
        self._cons = None   # sharded host-steered loop only: the ranks' consensus step (n_params + 2)
        # box bounds (engine.set_bounds) in the host-steered pieces: the effective mask of the last `solve` and the fraction of its step
        # that `truncate` kept.  (The device-steered loop keeps both in the handle.)
        self.fixed_eff = torch.zeros_like(self.fixed)
        self.alpha = torch.ones(1, **f64)
        self.bounded = False   # set by lm_solve: the engine carries bounds for this solve
        self.spd_algorithm = "auto"   # 'launches' after a one-launch solve ran out of time (another process held the compute units)

    def cost(self, slot):
        return self.packed[slot][self.n_packed - 1]

    @contextlib.contextmanager
    def on_stream(self):
        """Kernels launched through the C ABI and the few torch operations around them (copies, the collective of a sharded loop)
        must land on ONE stream handle.  torch's default stream is the NULL handle, which the C ABI can only name as
        ``hipStreamLegacy`` — two spellings the runtime is not guaranteed to order against each other in both directions.  So
        whenever the caller is on the default stream the work moves to a stream of this object (ordered after what the caller
        queued, and the caller's later work after ours); a caller that already runs on a real stream keeps it."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream != 0:
            yield cur.cuda_stream
            return
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield self.stream.cuda_stream
        cur.wait_stream(self.stream)

    def reduce(self, buf):
        """Sum ``buf`` (a packed state incl. its vote word) over the ranks, in place: stream-ordered on the device when the
        callable says ``on_device`` (RCCL), through the host otherwise (gloo)."""
        if self.reduce_fn is None:
            return
        if getattr(self.reduce_fn, "on_device", False):
            self.reduce_fn(buf)
        else:
            buf.copy_(self.torch.from_numpy(np.asarray(self.reduce_fn(buf.cpu().numpy()), dtype=np.float64)))

    def build(self, ps, slot: int):
        """packed[slot] <- [A | B | C | g | cost] at the device parameter string ``ps`` (+ the sum over the ranks)."""
        buf = self.packed[slot]
        with self.on_stream() as stream:
            if self.eng.n == 0:   # empty shard: zeros, but the all-reduce below still happens (see JacobianOperator)
                buf[: self.n_packed].zero_()
            else:
                self.eng.normal_blocks_device(ps.data_ptr(), buf.data_ptr(), stream)
            self.reduce(buf)
            # the engine's parameter prior (set_prior) enters ONCE, behind the sum over the ranks, with the same bits on every rank;
            # nothing is queued when none is set.  (The trials of the device-steered loop get it from lm_trial_finish.)
            self.eng.prior_add_device(ps.data_ptr(), buf.data_ptr(), stream)

    def solve(self, slot: int, lam, ps=None, ps_out=None, truncate=True):
        """Enqueue the damped step (H + lam diag(H)) delta = -g for the state in packed[slot]: ``self.delta`` (n_params,
        parameter-string order, 0 where fixed) and — given the current parameter string ``ps`` — the trial string
        ``ps_out = ps + delta``.  Device work only; ``self.status`` becomes non-zero when a factorisation fails.
        With ``self.bounded`` (needs ``ps``): the active set of the state takes the place of the mask (``self.fixed_eff``), and — unless
        ``truncate=False``: the caller calls ``truncate`` itself — the step is cut at the first bound (``self.alpha``)."""
        fixed = self.fixed
        if self.bounded:
            if ps is None:
                raise ValueError("a bounded step needs the current parameter string")
            fixed = self.fixed_eff
        with self.on_stream() as stream:
            if self.bounded:
                self.eng.bounds_active_device(ps.data_ptr(), self.packed[slot].data_ptr(), self.fixed.data_ptr(), fixed.data_ptr(), stream)
            self.eng.schur_prepare(self.packed[slot].data_ptr(), fixed.data_ptr(), lam.data_ptr(), self.linvt.data_ptr(), self.u.data_ptr(),
                                   self.V.data_ptr(), self.S.data_ptr(), self.rhs.data_ptr(), self.dvec.data_ptr(), self.gm.data_ptr(),
                                   self.status.data_ptr(), stream)
            ldv = self.V.shape[1]
            # S = A + lam D - V V' (lower triangle), rhs = -g_l + V u: MFMA kernel of csrc/ba_schur.hpp; S x_l = rhs: blocked
            # Cholesky + substitutions (csrc/ba_chol_persist.hpp / ba_dense_chol.hpp); w = V' x_l
            from .engine import dense_spd_solve, schur_syrk, schur_vtx

            xl = self.xl
            if self.n_trail:
                det = bool(self.eng.option("deterministic", 0))
                schur_syrk(self.eng.device, self.n_lead, self.n_trail, self.V.data_ptr(), ldv, self.S.data_ptr(), self.n_lead,
                           self.u.data_ptr(), self.rhs.data_ptr(), stream, work=self.syrk_work.data_ptr() if det else None, work_len=self.syrk_work_len)
            dense_spd_solve(self.eng.device, self.n_lead, self.S.data_ptr(), self.n_lead, self.rhs.data_ptr(), xl.data_ptr(),
                            self.chol_work.data_ptr(), self.status.data_ptr(), stream, algorithm=self.spd_algorithm,
                            timeout_us=self.eng.option("spd_timeout_us", None))
            if self.n_trail:
                schur_vtx(self.eng.device, self.n_lead, self.n_trail, self.V.data_ptr(), ldv, xl.data_ptr(), self.w.data_ptr(), stream)
                w = self.w
            else:
                w = self.u
            self.eng.schur_finish(self.linvt.data_ptr(), self.u.data_ptr(), w.data_ptr(), xl.data_ptr(), fixed.data_ptr(), self.delta.data_ptr(),
                                  ps.data_ptr() if ps is not None else 0, ps_out.data_ptr() if ps is not None else 0, stream)
        if self.bounded and truncate:
            self.truncate(ps, ps_out)
        return self.delta

    def truncate(self, ps, ps_out):
        """The step of the last ``solve`` cut at the first bound: ``self.delta`` and ``ps_out`` in place, ``self.alpha``."""
        with self.on_stream() as stream:
            self.eng.bounds_truncate_device(ps.data_ptr(), self.delta.data_ptr(), ps_out.data_ptr(), self.alpha.data_ptr(), stream)

    def _consensus_step(self, ps, ps_out):
        """Sharded host-steered loop WITHOUT the engine's deterministic mode: every rank has solved the SAME all-reduced system, but
        schur_syrk_kernel sums its K splits with f64 atomics in arrival order (csrc/ba_schur.hpp), so the steps agree to the last
        bits only — enough for one rank to meet xtol, or to take the other branch of the gain-ratio rule, while its peers enter the
        next all-reduce (a hang).  The ranks therefore adopt ONE step: the mean of theirs, from one more all-reduce of
        n_params + 1 doubles (the extra entry counts the ranks; an all-reduce delivers the same bits to every rank).  With
        ``set_option('deterministic', 1)`` the steps are bit-identical and this collective is not needed."""
        torch = self.torch
        if self._cons is None:
            self._cons = torch.empty(self.n_params + 1, dtype=torch.float64, device=self.dev)
        buf = self._cons
        buf[:-1].copy_(self.delta)
        buf[-1] = 1.0
        self.reduce(buf)
        torch.div(buf[:-1], buf[-1], out=self.delta)
        torch.add(ps, self.delta, out=ps_out)

    def decide(self, cur: int, new: int, ps, lam, stats):
        """The accept / reject decision of the trial state packed[new] against packed[cur] on the device (pcs_lm_decide):
        updates ``lam`` in place, clears ``status`` and fills ``stats`` (12 doubles) — what the host reads once per trial."""
        last = 8 * (self.n_packed - 1)
        with self.on_stream() as stream:
            if self.bounded:
                self.eng.lm_decide_bounded(self.packed[cur].data_ptr() + last, self.packed[new].data_ptr() + last, self.dvec.data_ptr(), self.gm.data_ptr(),
                                           self.delta.data_ptr(), ps.data_ptr(), self.fixed_eff.data_ptr(), self.alpha.data_ptr(), self.status.data_ptr(),
                                           lam.data_ptr(), stats.data_ptr(), stream=stream)
                return
            self.eng.lm_decide(self.packed[cur].data_ptr() + last, self.packed[new].data_ptr() + last, self.dvec.data_ptr(), self.gm.data_ptr(),
                               self.delta.data_ptr(), ps.data_ptr(), self.fixed.data_ptr(), self.status.data_ptr(), lam.data_ptr(), stats.data_ptr(),
                               stream)

    def lm_buffers(self, ps, lam, ctrl, flags, stats, stats_host=None, result_host=None, mode=None):
        """include/pcs_hip.h pcs_lm_buffers of one trial on this state — what the device-steered loop hands pcs_lm_trial*.  ``ps``: the
        two parameter strings; ``lam``, ``ctrl`` (12 doubles), ``flags`` (4 int32), ``stats`` (12 doubles): device tensors;
        ``stats_host`` / ``result_host``: page-locked tensors or None.  ``mode`` (PCS_LM_* bits) defaults to the loop's: a fixed trial
        buffer where a collective is queued on it (sharded) or the build reads its string from a fixed address (generated chains),
        votes when sharded."""
        from ._capi import LM_FIXED_TRIAL_BUFFER, LM_VOTES, LmBuffers
        from .engine import SPD_ALGORITHMS

        if mode is None:
            sharded = self.reduce_fn is not None
            mode = (LM_FIXED_TRIAL_BUFFER | LM_VOTES) if sharded else LM_FIXED_TRIAL_BUFFER if getattr(self.eng, "lm_fixed_trial_buffer", False) else 0
        b = LmBuffers()
        b.packed[0], b.packed[1] = self.packed[0].data_ptr(), self.packed[1].data_ptr()
        b.ps[0], b.ps[1] = ps[0].data_ptr(), ps[1].data_ptr()
        b.flags, b.fixed, b.lam = flags.data_ptr(), self.fixed.data_ptr(), lam.data_ptr()
        b.linvt, b.u, b.V, b.S, b.rhs, b.dvec, b.gm = (t.data_ptr() for t in (self.linvt, self.u, self.V, self.S, self.rhs, self.dvec, self.gm))
        b.status, b.xlead, b.w, b.spd_work = self.status.data_ptr(), self.xl.data_ptr(), self.w.data_ptr(), self.chol_work.data_ptr()
        b.delta, b.ctrl = self.delta.data_ptr(), ctrl.data_ptr()
        b.stats = stats.data_ptr()
        if stats_host is not None:
            b.stats_host = stats_host.data_ptr()
        b.spd_algorithm = SPD_ALGORITHMS[self.spd_algorithm]
        b.mode = mode
        if result_host is not None:
            b.free_idx, b.n_free, b.result_host = self.free_idx.data_ptr(), int(self.free_idx.numel()), result_host.data_ptr()
        b.syrk_work, b.syrk_work_len = self.syrk_work.data_ptr(), self.syrk_work_len
        return b

    def predicted_reduction(self, lam):
        """(0.5 (lam d'D d - g'd), step is valid) of the last ``solve`` as device tensors (tests; the loop uses ``decide``)."""
        torch = self.torch
        if self.bounded:
            pred = 0.5 * lam[0] * torch.dot(self.dvec, self.delta * self.delta) - (1.0 - 0.5 * self.alpha[0]) * torch.dot(self.gm, self.delta)
        else:
            pred = 0.5 * (lam[0] * torch.dot(self.dvec, self.delta * self.delta) - torch.dot(self.gm, self.delta))
        return pred, (self.status[0] == 0) & torch.isfinite(pred)

    def gradient(self, slot: int, lam=None):
        """masked J^T r of the state in packed[slot] (free entries), as NumPy — one read-back, used once at the end.  g sits in the
        packed buffer right behind the blocks ([A | B | C | g | cost]); no solve is needed to read it."""
        g0 = self.n_packed - 1 - self.n_params
        return self.packed[slot][g0: g0 + self.n_params][self.free_idx].cpu().numpy()


def _lm_solve_blocked(ne: BlockedNormalEquations, ps0: np.ndarray, *, max_iter, ftol, xtol, gtol, lam0, lam_grow0, verbose):
    """The device-resident loop behind ``lm_solve(..., linear_solver='cholesky')``.  Per trial step the host enqueues
    step (+ trial parameter string) -> build -> decision and then reads ONE small vector
        [accepted, max |g| before the step, relative cost drop, |step|, |x|, new sum r^2, old sum r^2, lambda used, ...]
    to follow the loop; x, lambda, the gain ratio and both states stay in HBM."""
    # For the duration of the loop the engine records neither the start / stop events of every build (pcs_last_kernel_ms) nor its
    # ordering event after every enqueue on this solver's stream (the stream lives as long as `ne`; "lazy_done_event" = 2 records
    # when somebody waits): each record is a packet between two launches, three of them cost a trial ~17 us (rocprofv3 trace).
    eng = ne.eng
    saved = (eng.option("timing_every", 1), eng.option("lazy_done_event", 1))
    eng.set_option("timing_every", 0)
    eng.set_option("lazy_done_event", 2)
    try:
        # The device steers the loop wherever the collective (if any) is stream-ordered: one GPU, or RCCL on the solver's stream.
        # A host-staged collective (gloo) needs the host between build and decision anyway: host-steered loop.
        # A sharded loop runs in the engine's deterministic mode — every rank computes the same bits from the all-reduced blocks, so
        # no rank can take another branch than its peers — unless the engine cannot (the (image, key) pass of the self chain with more
        # than 64 cameras keeps its atomics, csrc/ba_reduce.hpp): then the ranks adopt one consensus step per trial, host-steered.
        sharded = ne.reduce_fn is not None
        # (generated chains: the ordered contraction of csrc/ba_blockgram.hpp, unless two blocks share a parameter group)
        det_ok = not (eng.chain == "self" and eng.n_cams > DET_SELF_CAM_LIMIT) and getattr(eng, "deterministic_supported", lambda: True)()
        device_steered = not sharded or (getattr(ne.reduce_fn, "on_device", False) and det_ok)
        loop = _lm_loop_device if device_steered else _lm_loop_blocked
        saved_det = eng.option("deterministic", 0)
        if sharded and det_ok and not saved_det:
            eng.set_option("deterministic", 1)
        try:
            return loop(ne, ps0, max_iter=max_iter, ftol=ftol, xtol=xtol, gtol=gtol, lam0=lam0, lam_grow0=lam_grow0, verbose=verbose)
        finally:
            if sharded and det_ok and not saved_det:
                eng.set_option("deterministic", 0)
    finally:
        eng.set_option("lazy_done_event", saved[1])   # flushes the pending record while the stream exists
        eng.set_option("timing_every", saved[0])


STOP_MESSAGES = {0: "maximum number of iterations reached", 1: "gtol reached", 2: "no further decrease (damping exhausted)", 3: "ftol reached", 4: "xtol reached",
                 5: "maximum number of iterations reached"}
STOP_STATUS = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 0}
DET_SELF_CAM_LIMIT = 64          # the self chain's (image, key) pass is order-deterministic up to this many cameras (csrc/ba_reduce.hpp)
REJECTION_LIMIT = 12      # consecutive rejected trials before the loop gives up ("damping exhausted")
LM_SENTINEL = np.uint64(0x7FF8DEAD00000001)   # what a read-back slot holds until the device has written it (csrc/ba_schur.hpp lm_decide_kernel)


def _lm_loop_device(ne: BlockedNormalEquations, ps0: np.ndarray, *, max_iter, ftol, xtol, gtol, lam0, lam_grow0, verbose):
    """The loop the DEVICE steers: one trial = the step, the build at the trial string, the decision WITH the termination rules and
    the state flip of an accepted trial, a 12-double read-back into page-locked memory — and every kernel of it starts by reading a
    stop word.  The host therefore queues trial t + 1 BEFORE it reads the verdict of trial t: the GPU never idles between trials
    (38-53 us per trial on rig-32 in the host-steered form, profiles/r04/lm_trace_rig32.log), and when the loop ends the one
    speculative trial behind it drains as empty launches.

    Sharded over ranks with a stream-ordered collective (RCCL; ``reduce_fn.on_device``): the same loop with the all-reduce of the
    trial state queued between the two halves of a trial (pcs_lm_trial_build / pcs_lm_trial_finish) — no host synchronisation
    either.  The collective is queued on a fixed address, so the trial is always built into packed[1] and an accepted one is copied
    over packed[0] (PCS_LM_FIXED_TRIAL_BUFFER); the ranks decide on identical all-reduced blocks with order-deterministic kernels
    (`_lm_solve_blocked` switches the engine's deterministic mode on for a sharded loop), so every rank walks the same path without a consensus
    collective, and a dense solve that gives up on ONE rank voids the trial on all of them (PCS_LM_VOTES)."""
    from ._capi import LM_STATS

    torch = ne.torch
    dev = ne.dev
    sharded = ne.reduce_fn is not None
    eng = ne.eng
    with torch.cuda.device(dev), torch.cuda.stream(ne.stream):
        stream = ne.stream.cuda_stream
        ps = [torch.from_numpy(np.ascontiguousarray(ps0, dtype=np.float64)).to(dev), None]
        ps[1] = torch.empty_like(ps[0])
        lam = torch.full((1,), float(lam0), dtype=torch.float64, device=dev)
        ctrl = torch.tensor([0.0, 0.0, 0.0, float(max_iter), ftol, xtol, gtol, float(REJECTION_LIMIT), 0.0, float(lam_grow0), LAM_FAST[0], LAM_FAST[1]],
                            dtype=torch.float64, device=dev)
        flags = torch.zeros(4, dtype=torch.int32, device=dev)          # [stop, accepted, current state, -]
        stats_dev = torch.zeros(LM_STATS, dtype=torch.float64, device=dev)
        ring = 4
        # page-locked, allocated once per solver state, not per solve (hipHostMalloc costs ~0.2 ms) — and not shared between states: a
        # speculative trial one solve leaves behind still writes its read-back while the next solve may already run
        stats_host = ne.__dict__.get("_stats_host")
        if stats_host is None:
            stats_host = ne._stats_host = [torch.zeros(LM_STATS, dtype=torch.float64).pin_memory() for _ in range(ring)]
        # the final state (gradient | solution | sum r^2) is written into this page-locked buffer by the trial that ends the loop, before
        # that trial's read-back: the host returns without a copy of its own and without waiting for the speculative trial to drain
        n_free = int(ne.free_idx.numel())
        result_host = ne.__dict__.get("_result_host")
        if result_host is None or result_host.numel() != 2 * n_free + 1:
            result_host = ne._result_host = torch.zeros(2 * n_free + 1, dtype=torch.float64).pin_memory()
        result_view = result_host.numpy()
        result_view[-1] = np.nan
        pending = ne.__dict__.pop("_drain_event", None)
        if pending is not None:
            pending.synchronize()              # the speculative trial the previous solve left behind has written its (void) read-back
        ne.build(ps[0], 0)
        history = []                       # the first entry — the starting cost — comes with the first trial's read-back (no sync of its own)

        def buffers(k):
            return ne.lm_buffers(ps, lam, ctrl, flags, stats_dev, stats_host[k % ring], result_host)

        # The read-back of trial k lands in page-locked memory the device writes directly (lm_decide_kernel; all twelve words are -1 for
        # a launch that found the stop flag raised).  The host waits for THOSE words instead of an event — an event record between two
        # trials cost the GPU 5.6 us of idling per trial (the one gap in profiles/r04/lm_trace_*.log) — and the device needs no fence
        # between them: the host fills the slot with a NaN pattern no arithmetic produces and waits until none of it is left.
        views = [t.numpy() for t in stats_host]
        raw = [v.view(np.uint64) for v in views]

        def enqueue(k):
            raw[k % ring][:] = LM_SENTINEL
            b = buffers(k)
            if sharded:   # the trial state is all-reduced between the two halves, on this stream: nothing waits for the host
                eng.lm_trial_build(b, stream)
                ne.reduce(ne.packed[1])
                eng.lm_trial_finish(b, stream)
            else:
                eng.lm_trial(b, stream)

        def wait_for(k):
            v, u = views[k % ring], raw[k % ring]
            t_end = time.perf_counter() + 30.0
            spins = 0
            while (u == LM_SENTINEL).any():
                spins += 1
                if spins & 1023 == 0:
                    if time.perf_counter() > t_end:
                        raise RuntimeError("device LM loop: no read-back within 30 s")
                    time.sleep(0)
            return v.copy()

        code, nfev, n_lin, it = 0, 1, 0, 0
        trials = []                        # every decided trial's read-back, void ones included
        limit = REJECTION_LIMIT * max_iter + 16          # every accepted step is preceded by fewer than REJECTION_LIMIT rejections
        queued = read = 0
        if max_iter > 0:
            enqueue(queued)
            queued += 1
        else:
            code = 5
        while code == 0 and read < limit:
            if queued < limit:                 # speculate: the next trial goes out before this one's verdict is read
                enqueue(queued)
                queued += 1
            st = wait_for(read)
            read += 1
            if st[9] < 0:                       # a launch that found the flag raised: nothing happened
                if read >= queued:
                    break
                continue
            trials.append(st)
            n_lin += 1
            nfev += 1
            if not history:
                history.append(0.5 * float(st[6]))
            if verbose:
                print(f"  trial {int(st[9])}: lam {st[7]:.2e} cost {0.5 * st[6]:.6e} -> {0.5 * st[5]:.6e} accepted {bool(st[0] > 0)} stop {int(st[8])}")
            if st[0] > 0:
                it += 1
                history.append(0.5 * float(st[5]))
            code = int(st[8])
            if code == 9:   # the one-launch dense solve gave up waiting (on this rank or on a peer): repeat the trial with the launch-per-column form
                torch.cuda.current_stream().synchronize()      # whatever was queued behind it has drained as no-ops
                ne.spd_algorithm = "launches"
                ctrl[0] = 0.0
                flags[:2].zero_()                               # stop and accept; the current-state word stays
                nfev -= 1
                n_lin -= 1
                code = 0
                read = queued                                   # forget the drained launches
                if queued < limit:
                    enqueue(queued)
                    queued += 1
        if read < queued:                           # the speculative trial behind the end drains on its own (empty launches) ...
            ne._drain_event = torch.cuda.Event()    # ... and the next solve on this state waits for that before it reuses the read-back ring
            ne._drain_event.record()
        if code not in (0, 9) and max_iter > 0 and not np.isnan(result_view[-1]):
            out = result_view.copy()           # written by the trial that raised the stop code (lm_decide_kernel), complete before its read-back
        else:
            # gradient, solution and cost in ONE read-back (g and the cost sit behind the blocks of the packed state: [A | B | C | g | cost])
            torch.cuda.current_stream().synchronize()
            cur = int(flags[2].item())
            g0 = ne.n_packed - 1 - ne.n_params
            out = torch.cat([ne.packed[cur][g0: g0 + ne.n_params][ne.free_idx], ps[cur][ne.free_idx], ne.packed[cur][ne.n_packed - 1: ne.n_packed]]).cpu().numpy()
        g, x, cost = out[:n_free].copy(), out[n_free: 2 * n_free].copy(), 0.5 * float(out[-1])
        if not history:
            history.append(cost)
        bound_trials, n_truncated = [], 0
        if ne.bounded:   # alpha and the active count of every decided trial, kept by the handle (one read-back, behind the loop)
            torch.cuda.current_stream().synchronize()
            log, n_truncated = eng.bounds_trials(len(trials))
            bound_trials = [(float(a), int(n)) if a == a else (float("nan"), -1) for a, n in log]
    return DeviceLMResult(x=x, cost=cost, grad=g, optimality=float(np.max(np.abs(g))) if g.size else 0.0, nit=it, nfev=nfev,
                          n_jtjv=n_lin, status=STOP_STATUS.get(code, 0), message=STOP_MESSAGES.get(code, f"stopped ({code})"), history=history,
                          trials=trials, bound_trials=bound_trials, n_truncated=n_truncated)


def _gain_ratio(ne: BlockedNormalEquations, stats) -> float:
    """actual / predicted reduction of the trial `stats` describes (host-steered loop; the device-steered one has it in the kernel)."""
    torch = ne.torch
    lam_used = float(stats[7])
    if ne.bounded:
        pred = float((0.5 * lam_used * torch.dot(ne.dvec, ne.delta * ne.delta) - (1.0 - 0.5 * ne.alpha[0]) * torch.dot(ne.gm, ne.delta)).item())
    else:
        pred = 0.5 * float((lam_used * torch.dot(ne.dvec, ne.delta * ne.delta) - torch.dot(ne.gm, ne.delta)).item())
    return 0.5 * (float(stats[6]) - float(stats[5])) / pred if pred > 0 else -1.0


def _lm_loop_blocked(ne: BlockedNormalEquations, ps0: np.ndarray, *, max_iter, ftol, xtol, gtol, lam0, lam_grow0, verbose):
    """The host-steered loop: what a sharded solve takes when its collective goes through the host (gloo).  Same rules as the
    device-steered loop (the decision itself is pcs_lm_decide on the device).  Every rank decides on the same all-reduced blocks;
    whether a rank's one-launch dense solve gave up is all-reduced with them (the word behind the packed state), so the ranks repeat
    a void trial TOGETHER.  `_lm_solve_blocked` runs the loop in the engine's deterministic mode, where the ranks compute identical
    steps; only where that mode is not available (self chain beyond 64 cameras) do they adopt one consensus step per trial."""
    torch = ne.torch
    dev = ne.dev
    deterministic = bool(ne.eng.option("deterministic", 0))
    with torch.cuda.device(dev), torch.cuda.stream(ne.stream):     # one real stream for torch operations and C-ABI kernels alike
        ps = torch.from_numpy(np.ascontiguousarray(ps0, dtype=np.float64)).to(dev)
        ps_new = torch.empty_like(ps)
        lam = torch.full((1,), float(lam0), dtype=torch.float64, device=dev)
        stats_dev = torch.zeros(12, dtype=torch.float64, device=dev)
        stats_host = torch.zeros(12, dtype=torch.float64).pin_memory()
        verdict = torch.cuda.Event()
        cur, new = 0, 1
        ne.build(ps, cur)
        sumsq = float(ne.cost(cur).item())
        history = [0.5 * sumsq]
        nfev, n_lin = 1, 0
        status, message = 0, "maximum number of iterations reached"
        it = 0
        any_accepted = False
        trials = []
        bound_trials, n_truncated = [], 0
        truncated = False
        for it in range(1, max_iter + 1):
            accepted = False
            stop = False
            retry = 0
            while retry < REJECTION_LIMIT:   # damping retries
                consensus = ne.reduce_fn is not None and not deterministic
                ne.solve(cur, lam, ps, ps_new, truncate=not consensus)
                if ne.reduce_fn is not None:
                    if consensus:
                        ne._consensus_step(ps, ps_new)
                        if ne.bounded:   # the ranks' ONE step is what the bounds cut
                            ne.truncate(ps, ps_new)
                    ne.packed[new][ne.n_packed] = (ne.status[0] & 4).to(torch.float64)     # this rank's vote: "my dense solve gave up"
                n_lin += 1
                ne.build(ps_new, new)                                                        # the all-reduce sums the votes with the blocks
                if ne.reduce_fn is not None:
                    ne.status.bitwise_or_((ne.packed[new][ne.n_packed: ne.n_packed + 1] > 0).to(torch.int32) * 4)
                nfev += 1
                ne.decide(cur, new, ps, lam, stats_dev)
                stats_host.copy_(stats_dev, non_blocking=True)   # the ONE read-back of the trial: 96 bytes into page-locked memory
                verdict.record()
                verdict.synchronize()
                stats = stats_host.numpy().copy()
                # the trial's record in the device-steered loop's layout: pcs_lm_decide leaves [8] .. [10] to the loop, and [11] is
                # completed below where this loop's own rules change lambda
                trials.append(stats)
                stats[9], stats[10] = len(trials), cur
                if ne.bounded:   # alpha and the entries the bounds added to the mask (the device-steered loop: pcs_bounds_trials)
                    ab = torch.stack([ne.alpha[0], ((ne.fixed_eff != 0) & (ne.fixed == 0)).sum().to(torch.float64)]).cpu().numpy()
                    bound_trials.append((float(ab[0]), int(ab[1])))
                    truncated = ab[0] < 1.0
                if stats[0] < 0:   # the one-launch dense solve gave up waiting on SOME rank (status bit 2): nothing of this trial is valid —
                    stats[8] = 9
                    ne.spd_algorithm = "launches"   # every rank repeats it with the launch-per-column form (the decision left the damping alone)
                    nfev -= 1
                    n_lin -= 1
                    continue
                stats[8] = 0
                retry += 1
                n_truncated += 1 if truncated else 0
                gmax = float(stats[1])
                if verbose:
                    print(f"  it {it}: lam {stats[7]:.2e} cost {0.5 * stats[6]:.6e} -> {0.5 * stats[5]:.6e} accepted {bool(stats[0])}")
                if gmax <= gtol:   # the state BEFORE this step was already stationary: the step is dropped
                    status, message, stop = 1, "gtol reached", True
                    stats[0], stats[8], stats[11] = 0, 1, stats[7]
                    break
                if stats[0] > 0:
                    accepted = any_accepted = True
                    # pcs_lm_decide applied the classic 1/3; a gain ratio above LAM_FAST[0] earns LAM_FAST[1] (the device-steered loop's rule)
                    # (not for a step cut at a bound: pcs_lm_decide_bounded left lambda alone, and so does this rule)
                    if not truncated and _gain_ratio(ne, stats) > LAM_FAST[0]:
                        stats[11] = max(float(stats[7]) * LAM_FAST[1], 1e-12)
                        lam.fill_(stats[11])
                    ps, ps_new = ps_new, ps
                    cur, new = new, cur
                    stats[10] = cur
                    history.append(0.5 * float(stats[5]))
                    rel_drop, step_norm, x_norm = float(stats[2]), float(stats[3]), float(stats[4])
                    break
                if not any_accepted and lam_grow0 > 1.0:   # a rejection before the first accepted step: the device rule multiplied by 4
                    lam.mul_(lam_grow0 / 4.0)
                    stats[11] *= lam_grow0 / 4.0
                if retry == REJECTION_LIMIT:
                    stats[8] = 2
            if stop:
                break
            if not accepted:
                status, message = 2, "no further decrease (damping exhausted)"
                break
            if not truncated and rel_drop <= ftol:       # (a truncated trial's small drop and small step say nothing about convergence)
                status, message = 3, "ftol reached"
                trials[-1][8] = 3
                break
            if not truncated and step_norm <= xtol * (xtol + x_norm):
                status, message = 4, "xtol reached"
                trials[-1][8] = 4
                break
            if it == max_iter:
                trials[-1][8] = 5
        g = ne.gradient(cur, lam)
        x = ps[ne.free_idx].cpu().numpy()
        cost = 0.5 * float(ne.cost(cur).item())
    return DeviceLMResult(x=x, cost=cost, grad=g, optimality=float(np.max(np.abs(g))) if g.size else 0.0, nit=it, nfev=nfev,
                          n_jtjv=n_lin, status=status, message=message, history=history, trials=trials, bound_trials=bound_trials, n_truncated=n_truncated)


@dataclass
class DeviceLMResult:
    x: np.ndarray
    cost: float                 # 0.5 * sum rho0 (0.5 * sum r^2 for the linear loss), like scipy's OptimizeResult.cost; with a prior: of the augmented objective
    grad: np.ndarray
    optimality: float
    nit: int
    nfev: int
    n_jtjv: int                 # matrix-free J^T J v products ("pcg") / factorisations ("cholesky")
    status: int
    message: str
    history: list = field(default_factory=list)
    # one float64 array per decided trial (void ones included), in the read-back layout of include/pcs_hip.h (pcs_lm_trial stats):
    # accepted (1 / 0, -1 void), max |g|, relative cost drop, |step|, |x|, new and old sum r^2, lambda used, stop code after the trial,
    # trial number, current state after it, lambda for the next trial.  The PCG / host loop puts NaN where it has no such number.
    # With a prior the two sums are those of the augmented objective (the prior's sum included).
    trials: list = field(default_factory=list)
    prior_cost: float = 0.0     # 0.5 * sum (((x - prior_mean) / prior_sigma)^2) at x: the prior's share of ``cost`` (0.0 without a prior)
    # box bounds (lm_solve(bounds=)); None / 0 / empty without them
    active_mask: np.ndarray | None = None   # scipy's convention over the free vector: -1 at the lower bound, +1 at the upper, 0 otherwise
    n_truncated: int = 0                    # decided trials whose step was cut at a bound (alpha < 1)
    bound_trials: list = field(default_factory=list)   # per decided trial, parallel to ``trials``: (alpha, entries the bounds added to the mask)


def _free_bounds(x0, bounds):
    """``lm_solve``'s ``bounds`` on the FREE vector -> (lo, hi) as float64 arrays of x0's length, or None for ``None`` and for bounds that
    are all infinite.  scipy's forms: ``(lo, hi)`` with scalars or arrays, or an object with ``lb`` / ``ub`` (``scipy.optimize.Bounds``).
    ValueError for wrong shapes, NaN, ``lo > hi`` or an ``x0`` outside the box, naming the first offending index — nothing else is touched."""
    if bounds is None:
        return None
    if hasattr(bounds, "lb") and hasattr(bounds, "ub"):
        lo, hi = bounds.lb, bounds.ub
    else:
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise ValueError("bounds must be (lo, hi) or a scipy.optimize.Bounds") from None
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    fb = bounds_arrays(x0.shape[0], lo, hi, "bounds")
    if fb is None:
        return None
    bad = (x0 < fb[0]) | (x0 > fb[1])
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"`x0` is infeasible: x0[{k}] = {x0[k]} lies outside [{fb[0][k]}, {fb[1][k]}]")
    return fb


def _string_bounds(mask, fb):
    """The free-vector bounds as (lo, hi) over the parameter string (``_string_prior``'s indexing); fixed parameters get none."""
    if fb is None:
        return None
    free = np.flatnonzero(mask)
    if free.shape[0] != fb[0].shape[0]:
        raise ValueError(f"the bounds have {fb[0].shape[0]} entries, the handler has {free.shape[0]} free parameters")
    lo, hi = np.full(mask.shape[0], -np.inf), np.full(mask.shape[0], np.inf)
    lo[free], hi[free] = fb
    return lo, hi


def _bound_result(res, fb):
    """``active_mask`` of a bounded solve: the active set of the FINAL state — on a bound with the gradient pointing out of the box, what
    bounds_active_kernel computes for a trial —, and the optimality as the projected gradient."""
    lo, hi = fb
    am = np.zeros(res.x.shape[0], dtype=np.int64)
    am[(res.x <= lo) & ((res.grad > 0.0) | (lo == hi))] = -1
    am[(res.x >= hi) & (res.grad < 0.0)] = 1
    res.active_mask = am
    res.optimality = float(np.max(np.abs(res.grad[am == 0]))) if np.any(am == 0) else 0.0
    return res


def _free_prior(x0, prior_mean, prior_sigma):
    """``lm_solve`` / ``parameter_covariance``'s prior on the FREE vector -> (mean, weight = 1 / sigma) as float64 arrays of x0's
    length, or None without one.  ``np.inf`` in ``prior_sigma`` = no prior on that entry; every other value finite and > 0.
    ``prior_mean=None`` = ``x0``.  ValueError for wrong shapes or values — nothing else is touched."""
    if prior_sigma is None:
        if prior_mean is not None:
            raise ValueError("prior_mean without prior_sigma: a prior needs its standard deviations")
        return None
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    sig = np.asarray(prior_sigma, dtype=np.float64)
    sig = np.full(x0.shape, float(sig)) if sig.ndim == 0 else sig
    if sig.shape != x0.shape:
        raise ValueError(f"prior_sigma has shape {sig.shape}: expected one value per free parameter, {x0.shape}")
    if np.any(np.isnan(sig)) or not np.all(sig > 0.0):
        raise ValueError("every prior_sigma must be > 0 (np.inf: no prior on that entry)")
    mu = x0.copy() if prior_mean is None else np.asarray(prior_mean, dtype=np.float64)
    mu = np.full(x0.shape, float(mu)) if mu.ndim == 0 else mu
    if mu.shape != x0.shape:
        raise ValueError(f"prior_mean has shape {mu.shape}: expected one value per free parameter, {x0.shape}")
    w = np.where(np.isinf(sig), 0.0, 1.0 / sig)
    if not np.all(np.isfinite(mu[w > 0.0])):
        raise ValueError("prior_mean must be finite wherever prior_sigma is finite")
    return np.where(w > 0.0, mu, 0.0), w


def _string_prior(mask, prior):
    """The free-vector prior as (mean, inv_sigma) over the parameter string: free entry k is string entry ``np.flatnonzero(mask)[k]`` —
    the index the loop's result read-back uses.  Fixed parameters get no entry."""
    if prior is None:
        return None
    free = np.flatnonzero(mask)
    if free.shape[0] != prior[0].shape[0]:
        raise ValueError(f"the prior has {prior[0].shape[0]} entries, the handler has {free.shape[0]} free parameters")
    mean, w = np.zeros(mask.shape[0]), np.zeros(mask.shape[0])
    mean[free], w[free] = prior
    return mean, w


def _prior_half_sum(prior, x) -> float:
    return 0.0 if prior is None else 0.5 * float(np.sum((prior[1] * (np.asarray(x, dtype=np.float64) - prior[0])) ** 2))


class _PriorOperator:
    """A host operator (JacobianOperator, or one with ``build`` / ``solve``) plus a prior on the free vector: gradient, diagonal,
    ``jtjv``, the normal matrix and the sum of squares each gain their prior term.  The free vector is read off the parameter string
    (``free``: the string indices of the free parameters)."""

    def __init__(self, op, free, prior):
        self._op, self._free = op, np.asarray(free)
        self._mu, self._w = prior
        self._d = np.zeros_like(self._w)

    def __getattr__(self, name):   # jv, jtu, solve, as_linear_operator, ...: the operator's own
        return getattr(self.__dict__["_op"], name)

    def _at(self, ps):
        self._d = self._w * (np.asarray(ps, dtype=np.float64).ravel()[self._free] - self._mu)

    def linearize(self, ps):
        self._at(ps)
        self._op.linearize(ps)

    def grad(self):
        g, c = self._op.grad()
        return g + self._w * self._d, c + float(self._d @ self._d)

    def diag(self):
        return self._op.diag() + self._w ** 2

    def jtjv(self, v):
        return self._op.jtjv(v) + self._w ** 2 * v

    def build(self, ps):
        import torch

        self._at(ps)
        H, g, c = self._op.build(ps)
        H = H.clone()
        torch.diagonal(H).add_(torch.from_numpy(self._w ** 2).to(H.device))
        return H, g + torch.from_numpy(self._w * self._d).to(g.device), c + float(self._d @ self._d)


class _PcgStep:
    """LM linear algebra from matrix-free products (JacobianOperator)."""

    def __init__(self, op, cg_tol, cg_max_iter):
        self.op, self.cg_tol, self.cg_max_iter = op, cg_tol, cg_max_iter

    def evaluate(self, ps, need_scale=True):
        self.op.linearize(ps)
        g, sumsq = self.op.grad()
        return {"ps": ps, "g": g, "sumsq": sumsq, "d": None}

    def scale(self, st):
        if st["d"] is None:
            st["d"] = np.maximum(self.op.diag(), 1e-300)   # refers to the current linearisation = st
        return st["d"]

    def restore(self, st):
        self.op.linearize(st["ps"])   # the slabs hold a rejected trial point

    def solve(self, st, lam):
        dd = self.scale(st)
        delta, k = pcg(lambda v: self.op.jtjv(v) + lam * dd * v, -st["g"], 1.0 / ((1.0 + lam) * dd), self.cg_tol, self.cg_max_iter)
        return delta, k, 0.5 * float(-(st["g"] @ delta) + lam * (delta @ (dd * delta)))


class _CholeskyStep:
    """LM linear algebra from the block-reduced normal equations (NormalEquations)."""

    def __init__(self, ne):
        self.ne = ne

    def evaluate(self, ps, need_scale=True):
        Hs, g, sumsq = self.ne.build(ps)
        return {"ps": ps, "H": Hs, "g_dev": g, "g": g.cpu().numpy(), "sumsq": sumsq, "d": None}

    def scale(self, st):
        if st["d"] is None:
            import torch

            st["d"] = torch.clamp(torch.diagonal(st["H"]).clone(), min=1e-300)
        return st["d"]

    def restore(self, st):
        pass   # the state carries H: nothing refers to the engine's slabs

    def solve(self, st, lam):
        dd = self.scale(st)
        delta = self.ne.solve(st["H"], st["g_dev"], lam, dd)
        if delta is None:
            return None, 1, 0.0
        pred = 0.5 * float((-(st["g_dev"] @ delta) + lam * (delta @ (dd * delta))).item())
        return delta.cpu().numpy(), 1, pred


def _n_cams_of(op_fun, dd) -> int:
    """Cameras of the layout ``op_fun._engine_for(dd)`` creates: what a per-camera ``sigma`` is measured against, known before any device work."""
    seen = int(dd[:, 0].max()) + 1 if dd.shape[0] else 0
    counts = getattr(op_fun, "counts", None)
    return seen if counts is None else int(counts[0]) if dd.shape[0] == 0 else max(int(counts[0]), seen)


@contextlib.contextmanager
def _engine_settings(eng, loss, f_scale, inv_sigma, prior=None, bounds=None):
    """The engine's loss, noise weights, parameter prior (``(mean, inv_sigma)`` over the string, or None) and box bounds (``(lo, hi)`` over
    the string, or None) for one solve; all are restored afterwards (a failed solve included).  A generated chain has no loss and no
    weights to set: the prior and the bounds only."""
    fused = isinstance(eng, Engine)
    saved_loss, saved_w = (eng.loss(), eng.weights()) if fused else (None, None)
    saved_prior = eng.prior()
    saved_bounds = eng.bounds()
    if fused:
        eng.set_loss(loss, f_scale)
    try:
        if fused:
            eng.set_weights(inv_sigma=inv_sigma)
        if prior is None:
            eng.set_prior()
        else:
            eng.set_prior(prior[0], inv_sigma=prior[1])
        if bounds is not None:
            eng.set_bounds(*bounds)
        elif saved_bounds is not None:
            eng.set_bounds()
        yield
    finally:
        if saved_bounds is not None:
            eng.set_bounds(*saved_bounds)
        elif bounds is not None:
            eng.set_bounds()
        if fused:
            eng.set_loss(*saved_loss)
            eng.set_weights(inv_sigma=saved_w)
        if saved_prior is None:
            eng.set_prior()
        else:
            eng.set_prior(saved_prior[0], inv_sigma=saved_prior[1])


def _blocked_solver(eng, mask, reduce_fn, loss, f_scale, inv_sigma=None, prior=None, bounds=None) -> BlockedNormalEquations:
    """The engine's cached solver state for this mask, collective, layout, loss, noise weights, prior and bounds (one state per engine: a
    miss drops the previous one)."""
    key = (hash(mask.tobytes()), id(reduce_fn), tuple(sorted(eng.normal_layout().items())), loss, f_scale,
           None if inv_sigma is None else hash(inv_sigma.tobytes()), None if prior is None else hash(prior[0].tobytes() + prior[1].tobytes()))
    if bounds is not None:   # (appended: a solve without bounds keeps the key it had)
        key += (hash(bounds[0].tobytes() + bounds[1].tobytes()),)
    cache = eng.__dict__.setdefault("_blocked_solvers", {})
    ne = cache.get(key)
    if ne is None:
        for old in cache.values():   # a speculative trial of the solver state being dropped may still be draining: its buffers go back to the allocator after that
            old.stream.synchronize()
        cache.clear()
        ne = cache[key] = BlockedNormalEquations(eng, mask, reduce_fn=reduce_fn)
    return ne


def lm_solve(handler, x0, *, max_iter: int = 50, ftol: float = 1e-8, xtol: float = 1e-8, gtol: float = 1e-8,
             cg_tol: float = 1e-3, cg_max_iter: int = 200, lam0: float | None = None, lam_grow0: float | None = None, reduce_fn=None, verbose: int = 0,
             operator=None, linear_solver: str = "auto", loss: str = "linear", f_scale: float = 1.0, sigma=None,
             prior_mean=None, prior_sigma=None, bounds=None) -> DeviceLMResult:
    """Levenberg-Marquardt (Marquardt scaling D = diag(J^T J)) for a pycamset_amd handler.  The damped
    normal equations are solved by Jacobi-PCG on matrix-free J^T J products (``linear_solver='pcg'``) or
    by a Cholesky factorisation of the block-reduced J^T J (``'cholesky'``).  Every quantity that depends
    on the detections is computed by the HIP engine.  ``operator`` replaces the engine-backed
    JacobianOperator (used by the CPU tests of this driver).

    ``lam0``: the initial damping (Nielsen's tau: lambda multiplies D).  ``None`` = LAM0_EXACT = 1e-5 with the exact (Cholesky)
    step, 1e-3 with PCG.  The reference's solver — scipy ``least_squares(method='trf')``, optimisation_handling.py:88-98 — starts with
    the plain Gauss-Newton step whenever that lies inside its first trust region, which it does from a calibration's starting values;
    round 3's 1e-3 with the update lambda <- lambda / 3 needs nine accepted steps on rig-32 to get the damping out of the way.  The
    policy since round 5 (DESIGN section 4 has the table: near starts, 5 x / 10 x farther starts, two poses swapped, chains T and S):
    start at 1e-5 and let an ACCURATE model shed damping fast — a gain ratio above LAM_FAST[0] = 0.95 multiplies lambda by 0.1, above
    0.75 by 1/3, above 0.25 by 1, below by 2; every rejected trial multiplies it by 4 (host and device rule alike; at most
    REJECTION_LIMIT = 12 in a row), a rejection BEFORE the first accepted step by ``lam_grow0`` (default LAM_GROW0 = 1e3).  1e-6 (round
    4) is one evaluation faster from a near start and up to twice as slow from a far one: a nearly undamped step from 70 px away
    overshoots into a region where five to eight trials are rejected in a row.  ``max_iter <= 0`` evaluates the start and returns it.

    ``loss`` / ``f_scale``: scipy ``least_squares``'s robust losses ('linear', 'huber', 'soft_l1', 'cauchy', 'arctan'), applied to each
    scalar residual with scipy's linearisation (include/pcs_hip.h pcs_set_loss): the result's ``cost`` is scipy's ``0.5 * sum rho0`` and
    ``grad`` is J^T (rho1 f).  The engine's loss is set for the solve and restored afterwards.  Hand-fused chains with the blocked step
    only: a robust loss with ``linear_solver='pcg'``, with a caller's ``operator`` or with a generated chain raises NotImplementedError.

    ``sigma``: the detections' pixel noise — ``None``, an (N,) array per detection of ``handler._flat_detections()``, a (C,) array per
    camera, or ``{"camera": arr}`` (``engine.expand_sigma``; a bare array is refused when N == C).  Each detection's residual and
    Jacobian rows are whitened by 1 / sigma in front of the loss: the solve minimises ``sum rho(((f / sigma) / f_scale)^2) f_scale^2``,
    scipy's ``least_squares(loss=, f_scale=)`` on the whitened closures; ``cost`` and ``grad`` are those of the whitened system.  A
    sharded solve gives every rank the sigmas of its own detections (``sharding.shard_sigma``).  The engine's weights are set for the
    solve and restored afterwards; the same combinations as for a robust loss raise NotImplementedError.

    ``prior_mean`` / ``prior_sigma``: a Gaussian prior on the free vector, in the order of ``x0`` (scipy's ``result.x`` order): the
    solve minimises the objective above plus ``sum (((x - prior_mean) / prior_sigma)^2)`` — scipy's extra rows ``(x - mu) / sigma``,
    outside the loss and the detections' sigma.  ``np.inf`` in ``prior_sigma`` puts no prior on that entry, every other value must
    be finite and > 0; ``prior_mean=None`` is ``x0`` (a Tikhonov pull to the start).  ``handlers.slab_prior`` builds the two arrays
    from per-group values.  Works on every path: the blocked loops add the prior on the device (include/pcs_hip.h pcs_set_prior; set
    for the solve and restored afterwards), ``linear_solver='pcg'`` and a caller's ``operator`` add it on the host; with ``loss`` and
    ``sigma`` on hand-fused chains, with the linear loss on generated chains.  The result's ``cost`` and ``grad`` are those of the
    augmented objective, ``prior_cost`` is the prior's half sum at ``x``.  ValueError for wrong shapes or values, before any device work.

    ``bounds``: box bounds on the free vector in the order of ``x0``, in scipy ``least_squares``'s forms — ``(lo, hi)`` with scalars or
    arrays, or a ``scipy.optimize.Bounds``; ``-np.inf`` / ``np.inf`` = no bound.  ``handlers.slab_bounds`` builds the two arrays from
    per-group values.  The method ("Parameter bounds"; include/pcs_hip.h pcs_set_bounds): per trial an active set — on a
    bound with the gradient pointing out — joins the fixed parameters of the step, the step is cut at the first bound it meets, and the
    decision uses the cut step's predicted reduction; gtol tests the projected gradient, a cut trial triggers neither ftol nor xtol and
    never lowers the damping.
    Every blocked loop takes it (device- and host-steered, sharded, generated chains), with ``loss``, ``sigma`` and the prior; the
    engine's bounds are set for the solve and restored afterwards.  ``bounds=None`` or all infinite sets nothing: the launches and the
    bits of a solve without the argument.  The result's ``active_mask`` follows scipy (-1 lower, +1 upper, 0 free), ``n_truncated``
    counts the cut trials, ``optimality`` is the projected gradient's maximum.  ValueError before any device work for wrong shapes,
    NaN, ``lo > hi`` or an infeasible ``x0``; NotImplementedError for ``linear_solver='pcg'``, a caller's ``operator`` and systems
    beyond ``blocked_fits``."""
    prior = _free_prior(x0, prior_mean, prior_sigma)
    fbounds = _free_bounds(x0, bounds)
    if fbounds is not None and linear_solver == "pcg":
        raise NotImplementedError("bounds: the matrix-free step of linear_solver='pcg' has no active set; "
                                  "bounds need the blocked normal equations (linear_solver='cholesky' or 'auto')")
    if fbounds is not None and operator is not None:
        raise NotImplementedError("bounds with a caller-supplied operator: the host loop knows nothing of bounds")
    if loss not in LOSS_IDS:
        raise ValueError(f"unknown loss {loss!r}: expected one of {sorted(LOSS_IDS)}")
    f_scale = float(f_scale)
    if not (np.isfinite(f_scale) and f_scale > 0.0):
        raise ValueError(f"f_scale must be finite and > 0, got {f_scale}")
    if linear_solver not in ("auto", "pcg", "cholesky"):
        raise ValueError("linear_solver must be 'auto', 'pcg' or 'cholesky'")
    robust = loss != "linear"
    if robust and linear_solver == "pcg":
        raise NotImplementedError(f"loss={loss!r}: the matrix-free products of linear_solver='pcg' use the raw Jacobian; "
                                  "a robust loss needs the blocked normal equations (linear_solver='cholesky' or 'auto')")
    if robust and operator is not None:
        raise NotImplementedError(f"loss={loss!r} with a caller-supplied operator: the operator's products know nothing of the loss")
    weighted = sigma is not None
    if weighted and linear_solver == "pcg":
        raise NotImplementedError("sigma: the matrix-free products of linear_solver='pcg' use the raw Jacobian; "
                                  "noise weights need the blocked normal equations (linear_solver='cholesky' or 'auto')")
    if weighted and operator is not None:
        raise NotImplementedError("sigma with a caller-supplied operator: the operator's products know nothing of the weights")
    op_fun = handler.op_fun
    lam0_exact, lam0_pcg = (LAM0_EXACT, 1e-3) if lam0 is None else (float(lam0), float(lam0))
    grow0 = LAM_GROW0 if lam_grow0 is None else float(lam_grow0)
    if operator is None:
        dd = handler._flat_detections()
        inv_sigma = 1.0 / expand_sigma(sigma, dd[:, 0], _n_cams_of(op_fun, dd)) if weighted else None   # checked before any device work
        eng = op_fun._engine_for(dd)
        op_fun._bind_template(eng, handler._template_arg())
        if robust and not isinstance(eng, Engine):
            raise NotImplementedError(f"loss={loss!r}: generated chains (ChainProblem) build their normal equations without a robust loss")
        if weighted and not isinstance(eng, Engine):
            raise NotImplementedError("sigma: generated chains (ChainProblem) build their normal equations without noise weights")
        if linear_solver == "auto":   # blocked J^T J while its regions fit comfortably; beyond that matrix-free CG
            linear_solver = "cholesky" if blocked_fits(eng) else "pcg"
        if robust and linear_solver == "pcg":
            raise NotImplementedError(f"loss={loss!r}: this system is too large for the blocked normal equations (linear_solver='auto' chose "
                                      "'pcg', whose matrix-free products use the raw Jacobian)")
        if weighted and linear_solver == "pcg":
            raise NotImplementedError("sigma: this system is too large for the blocked normal equations (linear_solver='auto' chose "
                                      "'pcg', whose matrix-free products use the raw Jacobian)")
        if fbounds is not None and linear_solver == "pcg":
            raise NotImplementedError("bounds: this system is too large for the blocked normal equations (linear_solver='auto' chose "
                                      "'pcg', whose matrix-free step has no active set)")
        if fbounds is not None and not blocked_fits(eng):
            raise NotImplementedError("bounds: this system is too large for the blocked normal equations (device_solver.blocked_fits)")
        if linear_solver == "cholesky":
            # the solver's device workspace (two packed states, V, S, a stream) lives with the engine: a second solve on the same
            # table and mask — the usual case: a calibration re-run with other start values or tolerances — allocates nothing
            mask = np.asarray(handler._jac_mask(), dtype=bool)
            # (... and layout: a generated chain changes it with set_option("dense_normal", ...) — buffers sized for the other form would be overrun)
            # (... and the loss: nothing in the state depends on it — the engine's loss is set per solve below — but a state is never
            # carried from one loss to another.  The cache holds ONE state: a miss drops the previous one, so a sweep over f_scale
            # re-allocates per value instead of accumulating workspaces)
            # (... and the noise weights, in the same way: the engine's weights are set per solve below, and a state is never carried
            # from one set of weights to another, or from a weighted solve to an unweighted one)
            # (... and the prior, likewise: set per solve below, never carried from one solve's prior to another's)
            # (... and the bounds, likewise)
            sprior = _string_prior(mask, prior)
            sbounds = _string_bounds(mask, fbounds)
            ne = _blocked_solver(eng, mask, reduce_fn, loss, f_scale, inv_sigma, sprior, sbounds)
            ne.spd_algorithm = "auto"
            ne.bounded = sbounds is not None   # the loops' pieces consult the engine's bounds (set below) only then
            ps0 = op_fun.build_param_list(*handler.get_bundle_adjustment_inputs(np.array(x0, dtype=np.float64)))
            # generated chains: linear only (checked above); no prior and no bounds, here or left on the engine by its owner
            # (ChainEngine.set_bounds is public; the settings below set them aside for the solve): nothing to set
            if not isinstance(eng, Engine) and sprior is None and sbounds is None and eng.bounds() is None:
                return _lm_solve_blocked(ne, ps0, max_iter=max_iter, ftol=ftol, xtol=xtol, gtol=gtol, lam0=lam0_exact, lam_grow0=grow0, verbose=verbose)
            with _engine_settings(eng, loss, f_scale, inv_sigma, sprior, sbounds):
                res = _lm_solve_blocked(ne, ps0, max_iter=max_iter, ftol=ftol, xtol=xtol, gtol=gtol, lam0=lam0_exact, lam_grow0=grow0, verbose=verbose)
            res.prior_cost = _prior_half_sum(prior, res.x)
            return res if fbounds is None else _bound_result(res, fbounds)
        operator = JacobianOperator(eng, handler._jac_mask(), reduce_fn=reduce_fn)
    elif linear_solver == "auto":
        linear_solver = "cholesky" if hasattr(operator, "build") else "pcg"
    if prior is not None:   # the host paths: the operator's products gain the prior terms
        free = np.flatnonzero(np.asarray(handler._jac_mask(), dtype=bool))
        if free.shape[0] != prior[0].shape[0]:
            raise ValueError(f"the prior has {prior[0].shape[0]} entries, the handler has {free.shape[0]} free parameters")
        operator = _PriorOperator(operator, free, prior)
    step = _PcgStep(operator, cg_tol, cg_max_iter) if linear_solver == "pcg" else _CholeskyStep(operator)

    def param_str(x):
        return op_fun.build_param_list(*handler.get_bundle_adjustment_inputs(x))

    x = np.array(x0, dtype=np.float64)
    st = step.evaluate(param_str(x))
    nfev, n_lin, lam = 1, 0, (lam0_pcg if linear_solver == "pcg" else lam0_exact)
    history = [0.5 * st["sumsq"]]
    status, message = 0, "maximum number of iterations reached"
    it = 0
    any_accepted = False
    trials = []

    def record(accepted, gmax, sumsq_new, step_norm, x_norm, lam_used, lam_next):
        rel = 0.5 * (st["sumsq"] - sumsq_new) / (0.5 * st["sumsq"])
        trials.append(np.array([1.0 if accepted else 0.0, gmax, rel, step_norm, x_norm, sumsq_new, st["sumsq"], lam_used, 0.0, len(trials) + 1.0,
                                np.nan, lam_next]))

    for it in range(1, max_iter + 1):
        gmax = float(np.max(np.abs(st["g"])))
        if gmax <= gtol:
            status, message = 1, "gtol reached"
            break
        accepted = False
        x_norm = float(np.linalg.norm(x))
        for retry in range(REJECTION_LIMIT):  # damping retries
            if retry:
                step.restore(st)
            delta, k, pred = step.solve(st, lam)
            n_lin += k
            # a rejection before the first accepted step multiplies lambda by lam_grow0 (when that is > 1), every other one by 4
            grow = grow0 if not any_accepted and grow0 > 1.0 else 4.0
            if delta is None:   # damped matrix not positive definite: more damping
                record(False, gmax, np.nan, np.nan, x_norm, lam, lam * grow)
                lam *= grow
                continue
            x_new = x + delta
            st_new = step.evaluate(param_str(x_new))
            nfev += 1
            actual = 0.5 * (st["sumsq"] - st_new["sumsq"])
            rho = actual / pred if pred > 0 else -1.0
            step_norm = float(np.linalg.norm(delta))
            if verbose:
                print(f"  it {it}: lam {lam:.2e} lin {k} cost {0.5 * st['sumsq']:.6e} -> {0.5 * st_new['sumsq']:.6e} rho {rho:.3f}")
            if np.isfinite(st_new["sumsq"]) and actual > 0:
                accepted = any_accepted = True
                rel_drop = actual / (0.5 * st["sumsq"])
                fast = linear_solver != "pcg" and rho > LAM_FAST[0]    # exact steps only: less damping costs an inexact (CG) step iterations
                lam_next = max(lam * (LAM_FAST[1] if fast else 1.0 / 3.0 if rho > 0.75 else 1.0 if rho > 0.25 else 2.0), 1e-12)
                record(True, gmax, st_new["sumsq"], step_norm, x_norm, lam, lam_next)
                x, st, lam = x_new, st_new, lam_next
                history.append(0.5 * st["sumsq"])
                break
            record(False, gmax, st_new["sumsq"], step_norm, x_norm, lam, lam * grow)
            lam *= grow
        if not accepted:
            step.restore(st)
            status, message = 2, "no further decrease (damping exhausted)"
            trials[-1][8] = 2
            break
        if rel_drop <= ftol:
            status, message = 3, "ftol reached"
            trials[-1][8] = 3
            break
        if step_norm <= xtol * (xtol + x_norm):
            status, message = 4, "xtol reached"
            trials[-1][8] = 4
            break
        if it == max_iter:
            trials[-1][8] = 5
    return DeviceLMResult(x=x, cost=0.5 * st["sumsq"], grad=st["g"], optimality=float(np.max(np.abs(st["g"]))), nit=it, nfev=nfev,
                          n_jtjv=n_lin, status=status, message=message, history=history, trials=trials, prior_cost=_prior_half_sum(prior, x))


@dataclass
class ParameterCovariance:
    std: np.ndarray          # (n_free,) standard errors, in the order of x
    blocks: list             # one array per slab of handler.get_bundle_adjustment_inputs(x): (rows, w, w); 0 at fixed entries
    sigma2: float            # the residual variance used (1.0 with absolute_sigma)
    dof: int                 # 2N - n_free (+ the number of prior entries)
    cost: float              # 0.5 sum r^2 at x (+ the prior's half sum)
    min_pivot: float = 0.0   # smallest L_ii^2 / H_ii over the free parameters (the rank test against rcond)


def _slab_layout(slabs):
    """(offset, rows, width) of every slab in the parameter string (the slabs' concatenation, build_param_list's order)."""
    out, off = [], 0
    for s in slabs:
        s = np.asarray(s)
        rows = s.shape[0] if s.ndim else 1
        w = s.size // rows if rows else 0
        out.append((off, rows, w))
        off += s.size
    return out, off


def _covariance_plan(ne: BlockedNormalEquations, layout):
    """Device descriptors of the block Gram launches: leading slabs read column blocks of L^-1 (rows from the block's first column
    on: L^-1 is lower triangular), the trailing group is one tb x tb block per entity of Z = L^-1 V, finished with L_e^-T."""
    torch = ne.torch
    plan = []
    for off, rows, w in layout:
        if rows == 0 or w == 0:
            plan.append(("empty", off, rows, w, None))
        elif off + rows * w <= ne.n_lead:
            if w > 16:
                raise NotImplementedError(f"slab rows of {w} parameters: the block Gram kernel takes at most 16 columns")
            cols = (off + w * np.arange(rows)).astype(np.int32)
            d = torch.from_numpy(np.stack([cols, np.full(rows, w, np.int32), cols])).to(ne.dev)
            plan.append(("lead", off, rows, w, d))
        elif off >= ne.n_params - ne.n_trail:
            o = off - (ne.n_params - ne.n_trail) + w * np.arange(rows)
            if np.any(o % ne.tb + w > ne.tb):
                raise NotImplementedError(f"slab rows of {w} parameters straddle the trailing entities of {ne.tb}")
            plan.append(("trail", off, rows, w, (o // ne.tb, o % ne.tb)))
        else:
            raise NotImplementedError("a slab straddles the leading and the trailing parameters")
    trail = None
    if ne.n_trail:
        cols = (ne.tb * np.arange(ne.n_ent)).astype(np.int32)
        trail = torch.from_numpy(np.stack([cols, np.full(ne.n_ent, ne.tb, np.int32)])).to(ne.dev)
    return plan, trail


def parameter_covariance(handler, x, *, absolute_sigma: bool = False, rcond: float = 1e-10, reduce_fn=None, sigma=None,
                         prior_mean=None, prior_sigma=None) -> ParameterCovariance:
    """Marginal covariance blocks and standard errors of the parameters at ``x`` (the free vector, scipy's ``result.x`` order), from
    the blocked normal equations on the device: H = J'J with the linear loss and no damping, fixed parameters
    as identity rows and columns; sigma^2 = sum r^2 / (2N - n_free), or 1 with ``absolute_sigma`` (scipy curve_fit's meaning);
    the leading blocks are sigma^2 S^-1 (S = A - V V' = L L', column blocks of L^-1), the trailing ones
    sigma^2 L_e^-T (I + Z_e' Z_e) L_e^-1 with Z = L^-1 V formed in place of V.  Only the blocks come back to the host.

    ``sigma``: the detections' pixel noise, as ``lm_solve(sigma=)`` takes it.  H then comes from the weighted build, H = J~'J~ with the
    rows of J and the residuals divided by sigma; sigma^2 = sum (f / sigma)^2 / (2N - n_free), the variance of unit weight, and ``cost``
    is half that sum; ``absolute_sigma=True`` — the sigmas ARE the noise — gives inv(H) as it stands.  Hand-fused chains only.

    ``prior_mean`` / ``prior_sigma``: the Gaussian prior of ``lm_solve`` on the free vector.  H then includes the prior's diagonal
    1 / sigma^2 — what makes a gauge-free self-calibration or an unobserved entity invertible —, the prior rows count as observations:
    sigma^2 = (sum r^2 + sum ((x - mean) / sigma)^2) / (2N + n_prior - n_free), and the degrees-of-freedom test uses the same count.
    ``prior_mean`` is required unless ``absolute_sigma=True``, where the mean plays no part.  Generated chains included.

    Box bounds (``lm_solve(bounds=)``) are not known here: a parameter that ended on a bound is not free to vary, so fix the parameters
    of the solve's ``active_mask`` through the handler's mask before asking for the covariance of the others.

    Raises np.linalg.LinAlgError when H is singular or nearly so (a non-positive pivot, a trailing block that is not positive
    definite, or min L_ii^2 / H_ii below ``rcond``): a free gauge or an unobserved parameter.  ValueError for a wrong ``len(x)``
    or 2N - n_free <= 0, NotImplementedError for sharded systems (``reduce_fn``)."""
    if reduce_fn is not None:
        raise NotImplementedError("parameter_covariance of a sharded system (reduce_fn) is not supported: run it on one rank with all detections")
    rcond = float(rcond)
    if not (np.isfinite(rcond) and rcond >= 0.0):
        raise ValueError(f"rcond must be finite and >= 0, got {rcond}")
    x = np.asarray(x, dtype=np.float64).ravel()
    if prior_sigma is not None and prior_mean is None and not absolute_sigma:
        raise ValueError("prior_sigma without prior_mean: the variance of unit weight needs the prior's residuals (or pass absolute_sigma=True)")
    prior = _free_prior(x, prior_mean, prior_sigma)   # shapes and values, before the handler is touched
    n_prior = 0 if prior is None else int(np.count_nonzero(prior[1]))
    mask = np.asarray(handler._jac_mask(), dtype=bool)
    n_free = int(mask.sum())
    if x.shape[0] != n_free:
        raise ValueError(f"x has {x.shape[0]} entries, the handler has {n_free} free parameters")
    dd = handler._flat_detections()
    inv_sigma = None if sigma is None else 1.0 / expand_sigma(sigma, dd[:, 0], _n_cams_of(handler.op_fun, dd))
    dof = 2 * int(dd.shape[0]) + n_prior - n_free
    if dof <= 0:
        raise ValueError(f"no degrees of freedom left: 2N = {2 * int(dd.shape[0])} residuals and {n_prior} prior rows for {n_free} free parameters")
    slabs = handler.get_bundle_adjustment_inputs(x)
    layout, n_str = _slab_layout(slabs)
    if n_str != mask.shape[0]:
        raise ValueError(f"the slabs hold {n_str} parameters, the mask {mask.shape[0]}")

    op_fun = handler.op_fun
    eng = op_fun._engine_for(dd)
    op_fun._bind_template(eng, handler._template_arg())
    if not blocked_fits(eng):
        raise NotImplementedError("this system is too large for the blocked normal equations (device_solver.blocked_fits)")
    if inv_sigma is not None and not isinstance(eng, Engine):
        raise NotImplementedError("sigma: generated chains (ChainProblem) build their normal equations without noise weights")
    sprior = _string_prior(mask, prior)
    ne = _blocked_solver(eng, mask, None, "linear", 1.0, inv_sigma, sprior)
    ne.stream.synchronize()   # a speculative trial of the last solve may still be draining on this state
    torch = ne.torch
    from .engine import cov_block_gram, cov_trsm, dense_spd_solve, schur_syrk

    plan_key = tuple(layout)
    if getattr(ne, "_cov_plan", (None,))[0] != plan_key:
        ne._cov_plan = (plan_key,) + _covariance_plan(ne, layout)
    _, plan, trail_desc = ne._cov_plan
    nl, nt, dev = ne.n_lead, ne.n_trail, eng.device
    try:
        # hand-fused chains: the linear loss and these weights (none: the raw build) for the build below, the engine's own restored afterwards
        # (a generated chain: the prior only)
        settings = _engine_settings(eng, "linear", 1.0, inv_sigma, sprior)
        with settings, torch.cuda.device(ne.dev), torch.cuda.stream(ne.stream):
            stream = ne.stream.cuda_stream
            ps = torch.from_numpy(np.ascontiguousarray(op_fun.build_param_list(*slabs), dtype=np.float64)).to(ne.dev)
            ne.build(ps, 0)
            lam = torch.zeros(1, dtype=torch.float64, device=ne.dev)
            det = bool(eng.option("deterministic", 0))
            for algorithm in ("auto", "launches"):
                ne.status.zero_()
                eng.schur_prepare(ne.packed[0].data_ptr(), ne.fixed.data_ptr(), lam.data_ptr(), ne.linvt.data_ptr(), ne.u.data_ptr(), ne.V.data_ptr(),
                                  ne.S.data_ptr(), ne.rhs.data_ptr(), ne.dvec.data_ptr(), ne.gm.data_ptr(), ne.status.data_ptr(), stream)
                if nt:
                    schur_syrk(dev, nl, nt, ne.V.data_ptr(), ne.V.shape[1], ne.S.data_ptr(), nl, ne.u.data_ptr(), ne.rhs.data_ptr(), stream,
                               work=ne.syrk_work.data_ptr() if det else None, work_len=ne.syrk_work_len)
                dense_spd_solve(dev, nl, ne.S.data_ptr(), nl, ne.rhs.data_ptr(), ne.xl.data_ptr(), ne.chol_work.data_ptr(), ne.status.data_ptr(), stream,
                                algorithm=algorithm, timeout_us=eng.option("spd_timeout_us", None))
                status = int(ne.status.item())
                if not status & 4:   # bit 2: the one-launch solve gave up waiting; S is rebuilt and factored launch by launch
                    break
            if status & 4:
                raise RuntimeError("the dense factorisation did not complete")
            names = _param_names(layout)
            # rank test: L_ii^2 / H_ii over the free parameters (leading: the factor of S; trailing: 1 / diag(L_e^-T)), reduced here;
            # a failed factorisation leaves NaN behind its first non-positive pivot: counted as 0
            piv = torch.empty(ne.n_params, dtype=torch.float64, device=ne.dev)
            piv[:nl] = torch.diagonal(ne.S) ** 2
            if nt:
                piv[nl:] = 1.0 / torch.diagonal(ne.linvt[: ne.n_ent * ne.tb * ne.tb].view(ne.n_ent, ne.tb, ne.tb), dim1=1, dim2=2).reshape(-1) ** 2
            ratio = torch.where(ne.fixed.bool(), torch.full_like(piv, float("inf")), piv / ne.dvec)
            ratio = torch.where(torch.isnan(ratio), torch.zeros_like(ratio), ratio)
            k = int(torch.argmin(ratio).item())
            min_pivot = float(ratio[k].item()) if n_free else float("inf")
            hint = "a free gauge (fix a reference camera or pose) or an unobserved parameter"
            if status & 1:
                raise np.linalg.LinAlgError(f"H is singular: a trailing block (one pose or point) is not positive definite — {hint}")
            if status & 2:
                raise np.linalg.LinAlgError(f"H is singular: a non-positive pivot in the reduced system (min L_ii^2 / H_ii = {min_pivot:.3e}) — {hint}")
            if min_pivot < rcond:
                raise np.linalg.LinAlgError(f"H is rank deficient at parameter {k} ({names(k)}): L_ii^2 / H_ii = {min_pivot:.3e} < rcond = {rcond:.1e} — {hint}")
            # L^-1 (zeros above the diagonal skipped) and Z = L^-1 V in place of V
            linv = torch.empty((nl, nl), dtype=torch.float64, device=ne.dev)
            cov_trsm(dev, nl, ne.S.data_ptr(), nl, linv.data_ptr(), nl, nl, identity=True, stream=stream)
            if nt:
                cov_trsm(dev, nl, ne.S.data_ptr(), nl, ne.V.data_ptr(), nt, ne.V.shape[1], stream=stream)
            d_cost = 0 if absolute_sigma else ne.packed[0].data_ptr() + 8 * (ne.n_packed - 1)
            scale = 1.0 if absolute_sigma else 1.0 / dof
            outs = []
            for kind, off, rows, w, d in plan:
                if kind != "lead":
                    outs.append(None)
                    continue
                o = torch.empty(rows * w * w, dtype=torch.float64, device=ne.dev)
                cov_block_gram(dev, linv.data_ptr(), nl, nl, nl, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rows, o.data_ptr(), w * w,
                               d_fixed=ne.fixed.data_ptr(), fixed_off=0, d_scale=d_cost or None, scale=scale, stream=stream)
                outs.append(o)
            ent = None
            if nt:
                ent = torch.empty(ne.n_ent * ne.tb * ne.tb, dtype=torch.float64, device=ne.dev)
                cov_block_gram(dev, ne.V.data_ptr(), ne.V.shape[1], nl, nt, trail_desc[0].data_ptr(), trail_desc[1].data_ptr(), None, ne.n_ent,
                               ent.data_ptr(), ne.tb * ne.tb, d_linvt=ne.linvt.data_ptr(), tb=ne.tb, d_fixed=ne.fixed.data_ptr(), fixed_off=nl,
                               d_scale=d_cost or None, scale=scale, stream=stream)
            parts = [o for o in outs if o is not None] + ([ent] if ent is not None else [])
            host = torch.cat(parts + [ne.cost(0).reshape(1)]).cpu().numpy() if parts else ne.cost(0).reshape(1).cpu().numpy()
    finally:
        ne.status.zero_()
        ne.stream.synchronize()
    sumsq = float(host[-1])
    at = 0
    chunks = []
    for o in outs:
        if o is not None:
            chunks.append(host[at: at + o.numel()])
            at += o.numel()
    ent_h = host[at: at + ne.n_ent * ne.tb * ne.tb].reshape(ne.n_ent, ne.tb, ne.tb) if nt else None
    blocks, diag = [], np.zeros(ne.n_params)
    it = iter(chunks)
    for kind, off, rows, w, d in plan:
        if kind == "lead":
            b = next(it).reshape(rows, w, w)
        elif kind == "trail":
            e, o = d
            idx = o[:, None] + np.arange(w)[None, :]
            b = ent_h[e[:, None, None], idx[:, :, None], idx[:, None, :]]
        else:
            b = np.zeros((rows, w, w))
        blocks.append(b)
        if rows and w:
            diag[off: off + rows * w] = np.diagonal(b, axis1=1, axis2=2).reshape(-1)
    sigma2 = 1.0 if absolute_sigma else sumsq / dof
    return ParameterCovariance(std=np.sqrt(diag[mask]), blocks=blocks, sigma2=sigma2, dof=dof, cost=0.5 * sumsq, min_pivot=min_pivot)


def _param_names(layout):
    def name(k):
        for i, (off, rows, w) in enumerate(layout):
            if off <= k < off + rows * w:
                return f"slab {i}, row {(k - off) // w}, column {(k - off) % w}"
        return "?"
    return name
