"""A plain reference of one Levenberg-Marquardt trial, written from the documented rules (device_solver.lm_solve's docstring, the
pcs_lm_decide / pcs_lm_trial comments and the ``ctrl`` layout in include/pcs_hip.h, DESIGN section 4 "damping policy"), not from
the kernel.  The tests replay a loop's trials through it: tests/test_lm_reference.py against the host loop on CPU operators,
tests/test_gpu_lm_trials.py against lm_decide_kernel and the device-steered loop.

    M, rhs = masked_system(H, g, mask, lam)       the damped, masked system a step solves
    delta  = reference_step(H, g, mask, lam)
    eta    = backward_error(M, rhs, delta)        ||M d - rhs||_inf / (||M||_inf ||d||_inf + ||rhs||_inf), in long double
    out    = decide(TrialInputs(...), ctrl)       the branch, the stop code, lambda_next, the updated counters, the twelve stats words
    H, g, c = reference_normal(...)               the normal equations at a parameter string, from the CPU oracle
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
THRESHOLDS = (0.25, 0.75)   # gain-ratio bands: <= 0.25 x2, (0.25, 0.75] x1, above 0.75 x1/3
LAM_FLOOR = 1e-12           # an accepted trial never takes lambda below this
FINITE = 1e300              # |pred| and |c_new| at or above this count as overflowed (not finite)
NEAR = 1e-12                # a gain ratio within this (relative) of a threshold may take either side
# ctrl words (include/pcs_hip.h pcs_lm_buffers)
STOP, REJ, ACC, MAXIT, FTOL, XTOL, GTOL, REJLIM, TRIALS, GROW0, FAST_RHO, FAST_FAC = range(12)
CODES = {0: "running", 1: "gtol", 2: "rejection limit", 3: "ftol", 4: "xtol", 5: "iteration limit", 9: "void"}


def make_ctrl(*, max_iter=50, ftol=1e-8, xtol=1e-8, gtol=1e-8, rejection_limit=12, lam_grow0=1e3, fast=(0.95, 0.1)) -> np.ndarray:
    """A fresh control block: nothing decided yet."""
    c = np.zeros(12)
    c[MAXIT], c[FTOL], c[XTOL], c[GTOL], c[REJLIM], c[GROW0] = max_iter, ftol, xtol, gtol, rejection_limit, lam_grow0
    c[FAST_RHO], c[FAST_FAC] = fast
    return c


# ------------------------------------------------------------------------------------------------------------------------- the step

def masked_system(H, g, mask, lam):
    """(M, rhs) of the damped step: H on the free rows and columns + lam diag(D), D = max(diag H, 1e-300) on free entries; identity
    rows and columns at fixed entries; rhs = -g on free entries, 0 at fixed ones."""
    H = np.asarray(H, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    d = np.maximum(np.diag(H), 1e-300)
    M = np.where(np.outer(mask, mask), H, 0.0)
    M[np.diag_indices_from(M)] += np.where(mask, lam * d, 1.0)
    rhs = np.where(mask, -np.asarray(g, dtype=np.float64), 0.0)
    return M, rhs


def reference_step(H, g, mask, lam):
    M, rhs = masked_system(H, g, mask, lam)
    return np.linalg.solve(M, rhs)


def backward_error(M, rhs, delta) -> float:
    """Normwise backward error of ``delta`` as a solution of M delta = rhs (long double residual).  Independent of the conditioning:
    a backward-stable solve gives a few units of rounding whatever M is."""
    M, rhs, delta = (np.asarray(a, dtype=LD) for a in (M, rhs, delta))
    res = M @ delta - rhs
    den = np.max(np.sum(np.abs(M), axis=1)) * np.max(np.abs(delta)) + np.max(np.abs(rhs))
    return float(np.max(np.abs(res)) / den) if den > 0 else 0.0


def predicted_reduction(lam, dvec, gm, delta) -> float:
    """0.5 (lam delta' D delta - g' delta) of the damped model, in long double, rounded once."""
    dvec, gm, delta = (np.asarray(a, dtype=LD) for a in (dvec, gm, delta))
    return float(LD(0.5) * (LD(lam) * np.sum(dvec * delta * delta) - np.sum(gm * delta)))


# --------------------------------------------------------------------------------------------------------------------- the decision

@dataclass
class TrialInputs:
    c_old: float                 # sum r^2 (sum rho0) of the current state
    c_new: float                 # ... of the trial state
    pred: float                  # predicted reduction of the damped model
    gmax: float                  # max |g_m| of the current state (masked gradient)
    delta: np.ndarray            # the step, free entries (fixed ones are 0 and add nothing)
    x_free: np.ndarray           # the current parameter string at the free entries
    lam: float                   # the damping the step was computed with
    status: int = 0              # bit 1 / 2: a factorisation failed (rejected); bit 4: the dense solve gave up (void)
    votes: float = 0.0           # PCS_LM_VOTES: the ranks' "my dense solve gave up", summed


@dataclass
class Decision:
    branch: str                  # "accept" | "reject" | "void" | "gtol"
    code: int
    lam_next: float
    ctrl: np.ndarray             # the control block after the trial
    stats: np.ndarray            # the twelve read-back words ([10], the current state, is left to the caller: NaN)
    rho: float
    near_threshold: bool = False
    notes: list = field(default_factory=list)

    @property
    def accepted(self) -> bool:
        return self.branch == "accept"


def _finite(v) -> bool:
    return v == v and abs(v) < FINITE


def gain_factor(rho: float, ctrl) -> float:
    """lambda's factor after an accepted trial: x ctrl[11] above ctrl[10] (both > 0, else off), x 1/3 above 0.75, x 1 above 0.25,
    x 2 otherwise (rho = -1 when the model predicted no decrease)."""
    if ctrl[FAST_RHO] > 0.0 and ctrl[FAST_FAC] > 0.0 and rho > ctrl[FAST_RHO]:
        return float(ctrl[FAST_FAC])
    return 1.0 / 3.0 if rho > 0.75 else 1.0 if rho > 0.25 else 2.0


def near_a_threshold(rho: float, ctrl) -> bool:
    ts = list(THRESHOLDS) + ([float(ctrl[FAST_RHO])] if ctrl[FAST_RHO] > 0.0 and ctrl[FAST_FAC] > 0.0 else [])
    return rho == rho and any(abs(rho - t) <= NEAR * t for t in ts)


def decide(t: TrialInputs, ctrl) -> Decision:
    """One trial by the documented rules.  ``ctrl`` is not modified; the updated block is returned."""
    c = np.array(ctrl, dtype=np.float64)
    lam = float(t.lam)
    actual = 0.5 * (t.c_old - t.c_new)
    pred = float(t.pred)
    rho = actual / pred if pred > 0.0 else -1.0
    valid_step = t.status == 0 and _finite(pred)
    decrease = valid_step and _finite(t.c_new) and actual > 0.0
    delta = np.asarray(t.delta, dtype=LD)
    x = np.asarray(t.x_free, dtype=LD)
    step_norm = float(np.sqrt(np.sum(delta * delta)))
    x_norm = float(np.sqrt(np.sum(x * x)))
    rel_drop = actual / (0.5 * t.c_old)
    void = (t.status & 4) != 0 or t.votes > 0.0
    code = 0
    if void:                                   # nothing of the trial is valid: the host repeats it; damping and counters stay
        branch = "void"
        code = 9
    elif t.gmax <= c[GTOL]:                    # the state before the step was already stationary: the step is dropped
        branch = "gtol"
        code = 1
    elif decrease:
        branch = "accept"
        c[REJ] = 0.0
        c[ACC] = ctrl[ACC] + 1.0
        if rel_drop <= c[FTOL]:
            code = 3
        elif step_norm <= c[XTOL] * (c[XTOL] + x_norm):
            code = 4
        elif c[ACC] >= c[MAXIT]:
            code = 5
    else:
        branch = "reject"
        c[REJ] = ctrl[REJ] + 1.0
        if c[REJ] >= c[REJLIM]:
            code = 2
    if branch == "accept":
        lam_next = max(lam * gain_factor(rho, ctrl), LAM_FLOOR)
    elif branch == "reject":
        # a rejection before the first accepted step multiplies by lam_grow0 (when that is > 1), every other one by 4
        grow = float(ctrl[GROW0]) if ctrl[ACC] == 0.0 and ctrl[GROW0] > 1.0 else 4.0
        lam_next = lam * grow
    else:
        lam_next = lam
    c[TRIALS] = ctrl[TRIALS] + 1.0
    c[STOP] = code
    stats = np.array([-1.0 if void else 1.0 if branch == "accept" else 0.0, t.gmax, rel_drop, step_norm, x_norm, t.c_new, t.c_old, lam,
                      float(code), c[TRIALS], np.nan, lam_next])
    near = branch == "accept" and near_a_threshold(rho, ctrl)
    return Decision(branch=branch, code=code, lam_next=lam_next, ctrl=c, stats=stats, rho=rho, near_threshold=near)


# ----------------------------------------------------------------------------------------------------- normal equations from the oracle

def reference_normal(chain, det, ps, template=None, *, loss="linear", f_scale=1.0, with_slack=False):
    """(H, g, sum rho0) over the whole parameter string at ``ps`` from the CPU oracle's Jacobian (hand-fused chains); a robust loss
    goes through scipy's least_squares loss and its row scaling (scale_for_robust_loss_function).  ``with_slack`` adds what H may
    differ by where scipy clamps rho1 + 2 rho2 f^2 to EPS (tests/test_gpu_robust_loss.py _oracle_system): 16 EPS |J_i|^T |J_i| over
    those rows (0 for the linear loss)."""
    from scipy.sparse import csr_array

    from oracle import ba_oracle as orc

    dense, r = orc.full_jac_dense(chain, det, ps, template, with_resid=True)
    idx, ptr, _ = orc.csr_structure(chain, det, np.ones(ps.shape[0], bool))
    J = csr_array((dense.reshape(-1), idx, ptr), shape=(2 * det.shape[0], ps.shape[0]))
    f = r.reshape(-1).copy()
    if loss == "linear":
        out = (J.T @ J).toarray(), J.T @ f, float(f @ f)
        return out + (0.0,) if with_slack else out
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from scipy.optimize._lsq.least_squares import construct_loss_function

    rho = construct_loss_function(f.size, loss, f_scale)(f, cost_only=False)
    js = rho[1] + 2 * rho[2] * f ** 2
    Jb = abs(J[np.flatnonzero(js < 8 * np.finfo(float).eps)])
    Js, fs = scale_for_robust_loss_function(J.tocsr().copy(), f.copy(), rho)
    out = (Js.T @ Js).toarray(), Js.T @ fs, float(np.sum(rho[0]))
    return out + (16 * np.finfo(float).eps * (Jb.T @ Jb).toarray(),) if with_slack else out


def reference_normal_closure(loss_fn, jac_fn, x):
    """(H, g, sum r^2) over the FREE parameters from a handler's CSR closures (generated chains: ChainProblem)."""
    J = jac_fn(x)
    r = loss_fn(x)
    return (J.T @ J).toarray(), J.T @ r, float(r @ r)


def unpack_blocks(pk, lay):
    """The symmetric H, g and cost of a packed state [A | B | C | g | cost] (A, C upper triangles)."""
    nl, nt, tb, n = lay["n_lead"], lay["n_trail"], lay["tb"], lay["n_params"]
    A = pk[: nl * nl].reshape(nl, nl)
    B = pk[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
    nb = nl * nl + nl * nt + nt * tb
    C = pk[nl * nl + nl * nt: nb].reshape(-1, tb, tb) if nt else np.zeros((0, tb, tb))
    Hb = np.zeros((n, n))
    Hb[:nl, :nl] = np.triu(A)
    Hb[:nl, nl:] = B
    for k in range(C.shape[0]):
        Hb[nl + k * tb: nl + (k + 1) * tb, nl + k * tb: nl + (k + 1) * tb] = np.triu(C[k])
    Hb = Hb + np.triu(Hb, 1).T
    return Hb, pk[nb: nb + n].copy(), float(pk[nb + n])
