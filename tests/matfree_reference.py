"""Reference for the matrix-free J products (csrc/ba_matfree.hpp): the five products and the cost in ``np.longdouble``, the per-entry
error bound each may use, and the wrong results a faulty tile branch would give — NumPy only —, and ``problem``, which puts a case of
tests/matfree_inputs.py, the committed oracle's Jacobian and those together once for both test files.

``BlockJacobian`` holds J as the oracle's dense (2N, P) block rows with the global column of every local one: a row of J has P
structural entries, so the 2N x n_params matrix is never formed (110 000 x 13 743 in the largest case).

The bounds invent no tolerance.  The suite accepts a device Jacobian entry within JAC_RTOL * max(|ref|, ROW_FLOOR * ||row||_inf) of the
oracle's and a residual within RES_RTOL * max(|ref|, 1e-3 * max(|u|, |v|)) (tests/helpers.py).  With
        Jhat_ij = |J_ij| + ROW_FLOOR * max_j |J_ij|            (>= the max() of the rule)
        s_i     = max(|r_i|, 1e-3 * max(|u|, |v|) of the detection)
a product formed from such a Jacobian differs from the exact one, to first order, by at most
        J v      row i      JAC_RTOL * sum_j Jhat_ij |v_j|
        J^T u    column j   JAC_RTOL * sum_i Jhat_ij |u_i|
        J^T r    column j   JAC_RTOL * sum_i Jhat_ij |r_i|  +  RES_RTOL * sum_i |J_ij| s_i
        J^T J v  column j   JAC_RTOL * sum_i Jhat_ij |(J v)_i|  +  sum_i |J_ij| bound(J v)_i
        diag     column j   2 JAC_RTOL * sum_i Jhat_ij |J_ij|
        cost                2 RES_RTOL * sum_i |r_i| s_i
FP64 summation in any order stays far inside: its error is n * 2^-53 of the same absolute sums."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from tests import matfree_inputs as MI
from tests.helpers import JAC_RTOL, RES_RTOL, ROW_FLOOR, chain_slabs

LD = np.longdouble
OPS = ("jv", "jtu", "jtjv", "diag", "grad")
TRANSPOSED = ("jtu", "jtjv", "diag", "grad")
Residual = namedtuple("Residual", "r scale")     # both (N, 2)


def residual(r, uv):
    """The residual with the scale ``helpers.resid_rel_err`` measures its error against."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    return Residual(r, np.maximum(np.abs(r), 1e-3 * np.max(np.abs(uv), axis=1, keepdims=True)))


class BlockJacobian:
    def __init__(self, dense, cols, n_params):
        """``dense`` (2N, P): rows 2i, 2i + 1 of detection i;  ``cols`` (N, P): global column of each local column."""
        cols = np.asarray(cols, dtype=np.int64)
        self.n, self.P = cols.shape
        self.n_params = int(n_params)
        self.cols = cols
        self.data = np.asarray(dense, dtype=np.float64).reshape(self.n, 2, self.P)

    def take(self, rows):
        return BlockJacobian(self.data[rows].reshape(-1, self.P), self.cols[rows], self.n_params)

    def scatter(self, contrib):
        """sum over detections of (N, P) per-detection column contributions -> (n_params,), in the dtype of ``contrib``."""
        out = np.zeros(self.n_params, dtype=contrib.dtype)
        np.add.at(out, self.cols, contrib)
        return out

    def matvec(self, v, data=None):
        """J v as (N, 2)."""
        data = self.data if data is None else data
        return np.sum(data * np.asarray(v)[self.cols][:, None, :], axis=2)

    def rmatvec_terms(self, u, data=None):
        """Per-detection terms of J^T u, (N, P): J_i^T u_i."""
        data = self.data if data is None else data
        return np.sum(data * np.asarray(u).reshape(self.n, 2, 1), axis=1)

    def observed(self):
        """(n_params,) bool: columns at least one detection refers to."""
        seen = np.zeros(self.n_params, dtype=bool)
        seen[self.cols.ravel()] = True
        return seen

    def to_csr(self):
        from scipy.sparse import csr_array
        indptr = self.P * np.arange(2 * self.n + 1)
        return csr_array((self.data.reshape(-1), np.repeat(self.cols, 2, axis=0).reshape(-1), indptr), shape=(2 * self.n, self.n_params))


def terms(J, op, r=None, v=None, u=None, dtype=LD):
    """Per-detection (N, P) contributions to the transposed product ``op``: what one lane of the kernel adds."""
    data = J.data.astype(dtype)
    if op == "diag":
        return np.sum(data * data, axis=1)
    w = {"jtu": lambda: np.asarray(u, dtype=dtype), "grad": lambda: np.asarray(r, dtype=dtype),
         "jtjv": lambda: J.matvec(np.asarray(v, dtype=dtype), data)}[op]()
    return J.rmatvec_terms(w, data)


def products(J, r, v, u):
    """{'jv' (2N,), 'jtu', 'jtjv', 'diag', 'grad' (n_params,), 'cost'} in np.longdouble."""
    out = {"jv": J.matvec(np.asarray(v, dtype=LD), J.data.astype(LD)).reshape(-1)}
    for op in TRANSPOSED:
        out[op] = J.scatter(terms(J, op, r=r, v=v, u=u))
    rl = np.asarray(r, dtype=LD)
    out["cost"] = np.sum(rl * rl)
    return out


def bounds(J, v, u, w):
    """Per-entry error bounds of the six results (module docstring); ``w`` is the ``Residual`` (``residual(r, uv)``)."""
    a = np.abs(J.data)
    hat = a + ROW_FLOOR * np.max(a, axis=2, keepdims=True)
    absv = np.abs(np.asarray(v, dtype=np.float64))
    b_jv = JAC_RTOL * J.matvec(absv, hat)                                                  # (N, 2)
    jv = np.abs(J.matvec(np.asarray(v, dtype=np.float64)))
    out = {"jv": b_jv.reshape(-1),
           "jtu": JAC_RTOL * J.scatter(J.rmatvec_terms(np.abs(u), hat)),
           "grad": J.scatter(JAC_RTOL * J.rmatvec_terms(np.abs(w.r), hat) + RES_RTOL * J.rmatvec_terms(w.scale, a)),
           "jtjv": J.scatter(JAC_RTOL * J.rmatvec_terms(jv, hat) + J.rmatvec_terms(b_jv, a)),
           "diag": 2.0 * JAC_RTOL * J.scatter(np.sum(hat * a, axis=1)),
           "cost": 2.0 * RES_RTOL * float(np.sum(np.abs(w.r) * w.scale))}
    return out


def worst_ratio(result, ref, bound):
    """-> (max |result - ref| / bound, its index).  An entry whose bound is 0 (nothing observed feeds it) must be exactly 0.0:
    its ratio is 0 when it is, inf when it is not."""
    err = np.abs(np.asarray(result, dtype=LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    return float(ratio[k]), k


# ---- wrong results: what a faulty tile branch would return ---------------------------------------------------------------------
def _n_lead(chain):
    return 15 if chain == "free" else 21      # camera (+ pose) columns: the ones summed per tile and sent to a PAIR's entries


def wrong_transposed(J, chain, op, boundaries, param_boundaries, r, v, u):
    """{'dropped' | 'credited' | 'tail': wrong - exact, (n_params,) longdouble} for the transposed product ``op``.
       dropped   the contributions of one row on each side of every run boundary are lost (a summing group that skips its edge row)
       credited  the row in front of every boundary adds its camera / pose columns to the NEXT pair's entries (an n_a off by one)
       tail      every lane of the last tile beyond n adds row n - 1 once more (clamped lanes that are not masked)
    ``boundaries``: first rows of the runs after the first; ``param_boundaries``: those at which the pair's PARAMETERS change (the free
    chain has no pose: an image-only boundary moves nothing there).  A mutant that does not exist for the table is left out."""
    t = terms(J, op, r=r, v=v, u=u)
    out = {}
    if boundaries.size:
        rows = np.unique(np.concatenate([boundaries - 1, boundaries]))
        out["dropped"] = -J.take(rows).scatter(t[rows])
    if param_boundaries.size:
        nl = _n_lead(chain)
        rows = param_boundaries - 1
        d = np.zeros(J.n_params, dtype=LD)
        np.add.at(d, J.cols[rows, :nl], -t[rows, :nl])
        np.add.at(d, J.cols[rows + 1, :nl], t[rows, :nl])
        out["credited"] = d
    extra = -J.n % 64
    if extra:
        last = np.array([J.n - 1])
        out["tail"] = extra * J.take(last).scatter(t[last])
    return out


def wrong_jv(J_neighbour, rows, v, exact_jv):
    """wrong - exact of J v where each of ``rows`` (the row in front of a boundary) is computed from the NEXT pair's slabs and its
    entries of v: ``J_neighbour`` is the Jacobian of those rows with the next row's camera and image.  -> (len(rows), 2)."""
    return J_neighbour.matvec(np.asarray(v, dtype=LD), J_neighbour.data.astype(LD)) - exact_jv.reshape(-1, 2)[rows]


# ---- one (case, chain) with everything its tests compare against ------------------------------------------------------------------
CASE_CHAINS = [(name, chain) for name, case in MI.CASES.items() for chain in case.chains]


@functools.lru_cache(maxsize=None)
def problem(name, chain):
    """Everything a test of (case, chain) compares against, computed once: table, parameter string, the oracle's Jacobian and
    residual, fixed-seed v and u (no zero in u), the longdouble products and their bounds.  Read-only."""
    from oracle import ba_oracle as orc
    case = MI.CASES[name]
    rig, table = MI.case_table(name)
    ps = orc.build_param_list(*chain_slabs(rig, chain))
    tm = rig.points if chain == "template" else None
    dense, r = orc.full_jac_dense(chain, table, ps, tm, with_resid=True, counts=case.shape)
    cols = orc.block_param_inds(chain, table, case.shape)
    assert ps.shape[0] == MI.n_params_of(chain, case.shape) and np.all(r != 0.0)
    J = BlockJacobian(dense, cols, ps.shape[0])
    rng = np.random.default_rng(5)
    v = rng.standard_normal(ps.shape[0])
    u = rng.standard_normal(2 * table.shape[0])
    u = np.where(u < 0, -1.0, 1.0) * (0.25 + np.abs(u))
    w = residual(r, table[:, 3:])
    # tiles: as the kernel sees them in the default (packed) index form
    p = SimpleNamespace(name=name, chain=chain, case=case, rig=rig, table=table, ps=ps, template=tm, J=J, r=r, v=v, u=u, w=w,
                        tiles=MI.tile_classes(table, image_column=chain != "free"), ref=products(J, r, v, u), bound=bounds(J, v, u, w),
                        observed=J.observed())
    for a in (ps, v, u, r, J.data, J.cols):
        a.setflags(write=False)
    return p
