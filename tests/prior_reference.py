"""Reference for the Gaussian parameter prior of the device solve (include/pcs_hip.h pcs_set_prior, lm_solve(prior_mean=, prior_sigma=)):
scipy's extra rows.  On top of tests/weights_reference.py: the augmented closures

    fun_aug(x) = [w_det f(x); w (x - mu)]      jac_aug(x) = vstack([diag(w_det) J(x); diag(w) rows])

over the prior entries with w = 1 / sigma > 0, the prior's share of a normal system, and — for a robust solve — a callable scipy
``loss`` that applies the named loss to the first 2N rows and the identity to the prior rows."""
import numpy as np
from scipy.optimize._lsq.least_squares import IMPLEMENTED_LOSSES
from scipy.sparse import csr_array, vstack


def weights_of(sigma):
    """1 / sigma with np.inf -> 0 (no prior on that entry)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    return np.where(np.isinf(sigma), 0.0, 1.0 / sigma)


def augmented_closures(fun, jac, mean, w):
    """(fun_aug, jac_aug, n_prior) for closures over the free vector x; ``mean`` and ``w`` have x's length, rows exist where w > 0."""
    mean, w = np.asarray(mean, dtype=np.float64), np.asarray(w, dtype=np.float64)
    idx = np.flatnonzero(w > 0.0)
    rows = csr_array((w[idx], (np.arange(idx.shape[0]), idx)), shape=(idx.shape[0], w.shape[0]))

    def fun_aug(x):
        return np.concatenate([fun(x), w[idx] * (x[idx] - mean[idx])])

    def jac_aug(x):
        return csr_array(vstack([csr_array(jac(x)), rows], format="csr"))

    return fun_aug, jac_aug, idx.shape[0]


def prior_system(H, g, cost, p, mean, w):
    """(H + diag(w^2), g + w^2 (p - mean), cost + sum (w (p - mean))^2): the normal system of the augmented rows at p.  Everything over
    the same index set (the parameter string, or the free vector)."""
    p, mean, w = (np.asarray(a, dtype=np.float64) for a in (p, mean, w))
    d = np.where(w > 0.0, w * (p - np.where(w > 0.0, mean, 0.0)), 0.0)
    return np.asarray(H) + np.diag(w * w), np.asarray(g) + w * d, float(cost) + float(d @ d)


def prior_half_sum(x, mean, w):
    w = np.asarray(w, dtype=np.float64)
    d = np.where(w > 0.0, w * (np.asarray(x) - np.where(w > 0.0, mean, 0.0)), 0.0)
    return 0.5 * float(d @ d)


def split_loss(name, n_rows):
    """scipy's callable ``loss``: the named loss on the first ``n_rows`` residuals, rho0 = z, rho1 = 1, rho2 = 0 on the rest.  scipy
    calls it with z = (f / f_scale)^2, multiplies rho0 by f_scale^2 and divides rho2 by it, so the prior rows come out exactly as
    under the linear loss whatever f_scale is."""
    def loss(z):
        rho = np.empty((3, z.shape[0]))
        rho[0], rho[1], rho[2] = z, 1.0, 0.0
        head = rho[:, :n_rows]            # a view: the implemented losses fill it in place
        IMPLEMENTED_LOSSES[name](z[:n_rows], head, False)
        return rho

    return loss
