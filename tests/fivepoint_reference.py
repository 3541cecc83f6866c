"""NumPy restatement of the five-point solver and of the on-manifold refinement of the two-view consensus (include/pcs_hip.h
pcs_twoview_set_solver, csrc/ba_fivepoint.hpp), one pair at a time and generic in the dtype (float64 and ``np.longdouble``), on top of
``tests/twoview_reference.py``: the same sampler with a sample of five, the null space from the same cyclic Jacobi (the four columns of the
smallest eigenvalues, in column order), the ten cubic constraints in Nister's column order, Gauss-Jordan with partial pivoting, the
degree-10 polynomial, its Sturm chain, one bisection per real root with a fixed step count and fixed Newton steps, the
cheirality score over the four (R, +-t) of every root, the selection rules, and the 5-parameter LM with the group LM's rules.

Sums run in row order here and in lane order on the device; everything else is the device's formula.  The basis of the null space is
fixed by rounding noise (its four eigenvalues are zero), so the roots z of two precisions differ while their essential matrices agree:
hypotheses are compared through their best score, never root by root."""
from __future__ import annotations

import numpy as np

from tests import twoview_reference as tv
from tests.pnp_consensus_reference import sample_positions

OK, TOO_FEW, DEGENERATE, NO_CHEIRALITY = tv.OK, tv.TOO_FEW, tv.DEGENERATE, tv.NO_CHEIRALITY
SAMPLE, MIN_INLIERS, SLOTS = 5, 6, 10
BISECTIONS, POLISH = 56, 4
LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, FTOL, XTOL = 1e-4, 1e10, 1e-15, 1e-10, 1e-10
# column of the monomial x^a y^b z^c in the 10 x 20 constraint matrix (Nister's order: x and y are eliminated, z is kept)
COLUMN = {(3, 0, 0): 0, (0, 3, 0): 1, (2, 1, 0): 2, (1, 2, 0): 3, (2, 0, 1): 4, (2, 0, 0): 5, (0, 2, 1): 6, (0, 2, 0): 7, (1, 1, 1): 8,
          (1, 1, 0): 9, (1, 0, 2): 10, (1, 0, 1): 11, (1, 0, 0): 12, (0, 1, 2): 13, (0, 1, 1): 14, (0, 1, 0): 15, (0, 0, 3): 16,
          (0, 0, 2): 17, (0, 0, 1): 18, (0, 0, 0): 19}


# ---- polynomials in (x, y, z) of total degree <= 3 as (..., 4, 4, 4) arrays of coefficients -------------------------------------------
def pmul(a, b):
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape), dtype=a.dtype)
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - i - j):
                c = a[..., i, j, k]
                if np.any(c != 0):
                    out[..., i:, j:, k:] += c[..., None, None, None] * b[..., :4 - i, :4 - j, :4 - k]
    return out


def null_space(rays_a, rays_b, dtype):
    """(ok, basis (4, 3, 3)): the four eigenvectors of the smallest eigenvalues of the 9 x 9 moment matrix of the five constraint rows,
    in column order; ok: the fifth smallest eigenvalue is above RANK_RATIO x the largest."""
    xa, ya, xb, yb = rays_a[:, 0], rays_a[:, 1], rays_b[:, 0], rays_b[:, 1]
    rows = np.stack([xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, np.ones_like(xa)], axis=1)
    d, V = tv.jacobi_eigh(rows.T @ rows, tv.SWEEPS, dtype)
    if not np.all(np.isfinite(d)):
        return False, np.zeros((4, 3, 3), dtype=dtype)
    rank = np.array([sum(1 for j in range(9) if d[j] < d[c] or (d[j] == d[c] and j < c)) for c in range(9)])
    cols = [c for c in range(9) if rank[c] < 4]
    fifth = d[int(np.nonzero(rank == 4)[0][0])]
    ok = bool(np.max(d) > 0 and fifth > dtype(tv.RANK_RATIO) * np.max(d))
    return ok, np.stack([V[:, c].reshape(3, 3) for c in cols])


def constraints(basis, dtype):
    """The 10 x 20 matrix of det E = 0 (row 0) and 2 E E' E - tr(E E') E = 0 (rows 1 + 3 i + j), E = x B0 + y B1 + z B2 + B3."""
    E = np.zeros((3, 3, 4, 4, 4), dtype=dtype)
    E[:, :, 1, 0, 0], E[:, :, 0, 1, 0], E[:, :, 0, 0, 1], E[:, :, 0, 0, 0] = basis[0], basis[1], basis[2], basis[3]
    det = (pmul(E[0, 0], pmul(E[1, 1], E[2, 2]) - pmul(E[1, 2], E[2, 1])) + pmul(E[0, 1], pmul(E[1, 2], E[2, 0]) - pmul(E[1, 0], E[2, 2]))
           + pmul(E[0, 2], pmul(E[1, 0], E[2, 1]) - pmul(E[1, 1], E[2, 0])))
    EEt = sum(pmul(E[:, None, m], E[None, :, m]) for m in range(3))                 # (3, 3) of quadratics
    trace = EEt[0, 0] + EEt[1, 1] + EEt[2, 2]
    cub = 2 * sum(pmul(EEt[:, k, None], E[None, k, :]) for k in range(3)) - pmul(trace[None, None], E)
    M = np.zeros((10, 20), dtype=dtype)
    for (a, b, c), col in COLUMN.items():
        M[0, col] = det[a, b, c]
        M[1:, col] = cub[:, :, a, b, c].ravel()
    return M


def gauss_jordan(M):
    """[I | B] of the 10 x 20 with partial pivoting (the largest |entry| of the column at or below the diagonal, ties to the lower row);
    ok False when a pivot is zero or not finite."""
    M = M.copy()
    for c in range(10):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if not (np.isfinite(M[piv, c]) and M[piv, c] != 0):
            return False, M
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] * (1 / M[c, c])
        for r in range(10):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return True, M


def upoly_mul(a, b):
    out = np.zeros(len(a) + len(b) - 1, dtype=a.dtype)
    for i, ai in enumerate(a):
        out[i:i + len(b)] += ai * b
    return out


def hidden_variable(M):
    """From rows e .. j of the eliminated system: (n, p1, p2, p3), ascending coefficients in z of the degree-10 polynomial and of the
    cofactors with x = p1 / p3, y = p2 / p3."""
    def row_pair(e, f):
        kx = np.array([e[12], e[11] - f[12], e[10] - f[11], -f[10]])
        ky = np.array([e[15], e[14] - f[15], e[13] - f[14], -f[13]])
        k1 = np.array([e[19], e[18] - f[19], e[17] - f[18], e[16] - f[17], -f[16]])
        return kx, ky, k1
    kx, ky, k1 = row_pair(M[4], M[5])
    lx, ly, l1 = row_pair(M[6], M[7])
    mx, my, m1 = row_pair(M[8], M[9])
    p1 = upoly_mul(ky, l1) - upoly_mul(k1, ly)
    p2 = upoly_mul(k1, lx) - upoly_mul(kx, l1)
    p3 = upoly_mul(kx, ly) - upoly_mul(ky, lx)
    n = upoly_mul(p1, mx) + upoly_mul(p2, my) + upoly_mul(p3, m1)
    return n, p1, p2, p3


def horner(c, x):
    v = c[-1] + 0 * x
    for k in range(len(c) - 2, -1, -1):
        v = v * x + c[k]
    return v


def sturm_chain(n):
    """The Sturm chain f0 = n, f1 = n', f(i+1) = -rem(f(i-1), f(i)), every remainder scaled to a largest |coefficient| of 1 (a positive
    factor changes no sign): eleven polynomials of degrees 10 .. 0, ascending coefficients."""
    dtype = n.dtype.type
    f0, f1 = n.copy(), np.array([k * n[k] for k in range(1, len(n))], dtype=n.dtype)
    chain = [f0, f1]
    with np.errstate(all="ignore"):
        for _ in range(9):
            d = len(f1) - 1
            inv = dtype(1) / f1[d]
            qa = f0[d + 1] * inv
            qb = (f0[d] - qa * f1[d - 1]) * inv
            rem = np.zeros(d, dtype=n.dtype)        # (qa x + qb) f1 - f0, degree d - 1
            for k in range(d):
                rem[k] = qb * f1[k] + (qa * f1[k - 1] if k > 0 else 0) - f0[k]
            rem = rem * (1 / np.max(np.abs(rem)))
            chain.append(rem)
            f0, f1 = f1, rem
    return chain


def sign_changes(chain, x):
    """Sign changes of the chain at every x (zeros skipped)."""
    last, cnt = None, np.zeros(x.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for f in chain:
            s = np.sign(horner(f, x))
            s = np.where(np.isnan(s), 0, s)
            if last is None:
                last = s
                continue
            cnt = cnt + ((s != 0) & (last != 0) & (s != last))
            last = np.where(s != 0, s, last)
    return cnt


def real_roots(n):
    """(roots (10,), usable (10,)): slot k holds the k-th smallest real root of the degree-10 polynomial: BISECTIONS halvings of the
    Cauchy interval on the root count of the Sturm chain, then POLISH Newton steps that may not leave the bracket."""
    dtype = n.dtype.type
    with np.errstate(all="ignore"):
        n = n * (1 / np.max(np.abs(n)))
        bound = 1 + np.max(np.abs(n[:10] * (1 / n[10])))
        dn = np.array([k * n[k] for k in range(1, 11)], dtype=n.dtype)
        chain = sturm_chain(n)
        if not (np.isfinite(bound) and all(np.all(np.isfinite(f)) for f in chain)):
            return np.full(10, np.nan, dtype=n.dtype), np.zeros(10, dtype=bool)
        k = np.arange(10)
        lo, hi = np.full(10, -bound, dtype=n.dtype), np.full(10, bound, dtype=n.dtype)
        at_lo = sign_changes(chain, lo)
        total = at_lo[0] - sign_changes(chain, hi)[0]
        for _ in range(BISECTIONS):
            mid = (lo + hi) / 2
            above = at_lo - sign_changes(chain, mid) >= k + 1     # at least k + 1 roots at or below mid
            lo, hi = np.where(above, lo, mid), np.where(above, mid, hi)
        z = (lo + hi) / 2
        for _ in range(POLISH):
            zn = z - horner(n, z) / horner(dn, z)
            z = np.where(np.isfinite(zn) & (zn >= lo) & (zn <= hi), zn, z)
    return z.astype(n.dtype), (k < total) & np.isfinite(z)


def five_point(rays_a, rays_b, dtype=np.float64, details=False):
    """Up to ten essential matrices of five rays: (E (10, 3, 3) of unit Frobenius norm, usable (10,))."""
    E, usable = np.full((SLOTS, 3, 3), np.nan, dtype=dtype), np.zeros(SLOTS, dtype=bool)
    with np.errstate(all="ignore"):
        ok, basis = null_space(rays_a, rays_b, dtype)
        if ok:
            ok, M = gauss_jordan(constraints(basis, dtype))
        if not ok:
            return (E, usable, None) if details else (E, usable)
        n, p1, p2, p3 = hidden_variable(M)
        z, usable = real_roots(n)
        inv = 1 / horner(p3, z)
        x, y = horner(p1, z) * inv, horner(p2, z) * inv
        for k in range(SLOTS):
            Ek = x[k] * basis[0] + y[k] * basis[1] + z[k] * basis[2] + basis[3]
            Ek = Ek * (1 / np.sqrt(np.sum(Ek * Ek)))
            E[k] = Ek
            usable[k] = usable[k] and bool(np.all(np.isfinite(Ek)))
    return (E, usable, {"M": M, "n": n, "z": z, "x": x, "y": y, "basis": basis}) if details else (E, usable)


def action_matrix_roots(M):
    """The real z of the solutions by another route (float64 LAPACK): eigenvalues of the 10 x 10 matrix of the multiplication by z on the
    quotient ring's basis [xz^2, xz, x, yz^2, yz, y, z^3, z^2, z, 1], from the same eliminated system."""
    B = np.asarray(M[:, 10:], dtype=np.float64)
    A = np.zeros((10, 10))
    # z * [xz^2, xz, x, yz^2, yz, y, z^3, z^2, z, 1]: xz^3, yz^3 and z^4 are reduced through combinations of the eliminated rows
    # k = e - z f, l = g - z h, m = i - z j hold only x z^(0..3), y z^(0..3), z^(0..4): three relations linear in (x z^3, y z^3, z^4).
    def pair(e, f):
        kx = np.array([e[2], e[1] - f[2], e[0] - f[1], -f[0]])
        ky = np.array([e[5], e[4] - f[5], e[3] - f[4], -f[3]])
        k1 = np.array([e[9], e[8] - f[9], e[7] - f[8], e[6] - f[7], -f[6]])
        return kx, ky, k1
    rel = [pair(B[4], B[5]), pair(B[6], B[7]), pair(B[8], B[9])]
    lead = np.array([[kx[3], ky[3], k1[4]] for kx, ky, k1 in rel])                                    # of x z^3, y z^3, z^4
    rest = np.array([[kx[2], kx[1], kx[0], ky[2], ky[1], ky[0], k1[3], k1[2], k1[1], k1[0]] for kx, ky, k1 in rel])
    red = -np.linalg.solve(lead, rest)                                                              # (x z^3, y z^3, z^4) in the basis
    A[0], A[3], A[6] = red[0], red[1], red[2]
    A[1, 0] = A[2, 1] = A[4, 3] = A[5, 4] = A[7, 6] = A[8, 7] = A[9, 8] = 1.0
    w = np.linalg.eigvals(A)
    return w


# ---- decomposition, cheirality score --------------------------------------------------------------------------------------------------
def decompose(E, dtype):
    """(R1, R2, u3) of an essential matrix, by the formulas of the final stage of the eight-point path."""
    with np.errstate(all="ignore"):
        e, W = tv.jacobi_eigh(E.T @ E, 8, dtype)
        k3 = 0 if e[0] <= e[1] and e[0] <= e[2] else (1 if e[1] <= e[2] else 2)
        sg = np.sqrt(np.maximum(e, 0))
        s1, s2 = (sg[1] if k3 == 0 else sg[0]), (sg[1] if k3 == 2 else sg[2])
        v1, v2 = W[:, 1 if k3 == 0 else 0].copy(), W[:, 1 if k3 == 2 else 2].copy()
        u1, u2 = E @ v1 / s1, E @ v2 / s2
        u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
        u3 = u3 * (1 / np.sqrt(u3 @ u3))
        D, Cm = np.outer(u2, v1) - np.outer(u1, v2), np.outer(u3, v3)
    return Cm + D, Cm - D, u3


def rays_of(und, cam_a, cam_b, dtype):
    ia, ib = tv.inverse_pinhole(cam_a, dtype), tv.inverse_pinhole(cam_b, dtype)
    one = np.ones(und.shape[0], dtype=dtype)
    A = np.stack([ia[0, 0] * und[:, 0] + ia[0, 2], ia[1, 1] * und[:, 1] + ia[1, 2], one], axis=1)
    B = np.stack([ib[0, 0] * und[:, 2] + ib[0, 2], ib[1, 1] * und[:, 3] + ib[1, 2], one], axis=1)
    return A, B


def depths(R, t, A, B):
    """(pos, neg, angle): in front of both cameras under (R, t) and under (R, -t), and the angle between the two rays."""
    with np.errstate(all="ignore"):
        r = A @ R.T
        bb, bt = np.sum(B * B, axis=1), B @ t
        rr, rb, rt = np.sum(r * r, axis=1), np.sum(r * B, axis=1), r @ t
        det, la, lb = rr * bb - rb * rb, rb * bt - rt * bb, rr * bt - rb * rt
        cr = np.cross(r, B)
        a = np.arctan2(np.sqrt(np.sum(cr * cr, axis=1)), rb)
    return (det > 0) & (la > 0) & (lb > 0), (det > 0) & (la < 0) & (lb < 0), a


def slot_score(E, F, und, A, B, tau2, dtype):
    """(score, candidate, R, t): the four sums min(e^2, tau^2) with tau^2 for a row not in front, the smallest (ties: lower candidate)."""
    R1, R2, u3 = decompose(E, dtype)
    e2 = tv.sampson(F, und)
    with np.errstate(invalid="ignore"):
        capped = np.where(e2 <= tau2, e2, tau2)
    sums = []
    for R in (R1, R2):
        pos, neg, _ = depths(R, u3, A, B)
        sums += [np.sum(np.where(pos, capped, tau2)), np.sum(np.where(neg, capped, tau2))]
    best = 0
    for c in range(1, 4):
        if sums[c] < sums[best]:
            best = c
    if not sums[best] < np.inf:
        return dtype(np.inf), 0, R1, u3
    return sums[best], best, (R1 if best < 2 else R2), (-u3 if best & 1 else u3)


# ---- statistics of a pose and the refinement -----------------------------------------------------------------------------------------
def cross_matrix(t, dtype):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dtype=dtype)


def pose_stats(R, t, und, A, B, cam_a, cam_b, dtype):
    """(n_front, rms Sampson, parallax) of the rows at (R, t)."""
    F = tv.fundamental(cross_matrix(t, dtype) @ R, cam_a, cam_b, dtype)
    pos, _, a = depths(R, t, A, B)
    n_front = int(np.sum(pos))
    with np.errstate(all="ignore"):
        rms = np.sqrt(np.sum(tv.sampson(F, und)) / dtype(und.shape[0]))
        parallax = np.sqrt(np.sum(np.where(pos, a * a, 0)) / dtype(n_front))
    return n_front, rms, parallax


def rodrigues(w, dtype):
    th2 = w @ w
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1 - th2 / 6, dtype(0.5) - th2 / 24
    else:
        sh = np.sin(th / 2)
        a, b = np.sin(th) / th, 2 * sh * sh / th2
    K = cross_matrix(w, dtype)
    return np.eye(3, dtype=dtype) + a * K + b * (K @ K)


def tangent_basis(t, dtype):
    k = 0 if abs(t[0]) <= abs(t[1]) and abs(t[0]) <= abs(t[2]) else (1 if abs(t[1]) <= abs(t[2]) else 2)
    e = np.zeros(3, dtype=dtype)
    e[k] = 1
    b1 = np.cross(e, t)
    b1 = b1 * (1 / np.sqrt(b1 @ b1))
    return b1, np.cross(t, b1)


def refine_sums(R, t, und, cam_a, cam_b, dtype):
    """(H (5, 5), g (5,) = -J' r, cost): the signed Sampson residual of every row and its Jacobian in (omega, nu) at zero, R <- exp(omega) R,
    t <- exp(nu1 b1 + nu2 b2) t."""
    ia, ib = tv.inverse_pinhole(cam_a, dtype), tv.inverse_pinhole(cam_b, dtype)
    b1, b2 = tangent_basis(t, dtype)
    tx = cross_matrix(t, dtype)
    dE = [tx @ cross_matrix(np.eye(3, dtype=dtype)[k], dtype) @ R for k in range(3)]
    dE += [cross_matrix(np.cross(b, t), dtype) @ R for b in (b1, b2)]
    F = ib.T @ (tx @ R) @ ia
    dF = [ib.T @ d @ ia for d in dE]
    xa, ya, xb, yb = und[:, 0], und[:, 1], und[:, 2], und[:, 3]

    def parts(G):
        l0, l1, l2 = G[0, 0] * xa + G[0, 1] * ya + G[0, 2], G[1, 0] * xa + G[1, 1] * ya + G[1, 2], G[2, 0] * xa + G[2, 1] * ya + G[2, 2]
        r0, r1 = G[0, 0] * xb + G[1, 0] * yb + G[2, 0], G[0, 1] * xb + G[1, 1] * yb + G[2, 1]
        return l0, l1, r0, r1, xb * l0 + yb * l1 + l2
    with np.errstate(all="ignore"):
        l0, l1, r0, r1, num = parts(F)
        s = l0 * l0 + l1 * l1 + r0 * r0 + r1 * r1
        inv = 1 / np.sqrt(s)
        res = num * inv
        J = []
        for G in dF:
            d0, d1, e0, e1, dnum = parts(G)
            J.append(dnum * inv - res * ((l0 * d0 + l1 * d1 + r0 * e0 + r1 * e1) / s))
        J = np.stack(J, axis=1)
        return J.T @ J, -(J.T @ res), np.sum(res * res)


def solve5(H, g, lam):
    """(H + lam diag(H)) d = g by LDL'; None when a pivot is not positive or the step not finite."""
    n = 5
    A = H.copy()
    for i in range(n):
        A[i, i] = H[i, i] * (1 + lam)
    L, D = np.eye(n, dtype=H.dtype), np.zeros(n, dtype=H.dtype)
    with np.errstate(all="ignore"):
        for j in range(n):
            D[j] = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / D[j]
        if not (np.all(D > 0) and np.all(D < np.inf)):
            return None
        y = np.zeros(n, dtype=H.dtype)
        for i in range(n):
            y[i] = g[i] - sum(L[i, k] * y[k] for k in range(i))
        d = np.zeros(n, dtype=H.dtype)
        for i in range(n - 1, -1, -1):
            d[i] = y[i] / D[i] - sum(L[k, i] * d[k] for k in range(i + 1, n))
    return d if np.all(np.isfinite(d)) else None


def refine_pose(R, t, und, cam_a, cam_b, iters, dtype):
    """At most ``iters`` LM trials with the group LM's rules (damping 1e-4, x 0.1 on an accepted and x 10 on a refused trial, Marquardt
    scaling, ftol = xtol = 1e-10): (R, t, trials)."""
    H, g, cost = refine_sums(R, t, und, cam_a, cam_b, dtype)
    lam, it = dtype(LAMBDA0), 0
    if not np.isfinite(cost):
        return R, t, 0
    while it < iters:
        d = solve5(H, g, lam)
        if d is None:
            break
        b1, b2 = tangent_basis(t, dtype)
        Rt = rodrigues(d[:3], dtype) @ R
        tt = rodrigues(d[3] * b1 + d[4] * b2, dtype) @ t
        tt = tt * (1 / np.sqrt(tt @ tt))
        Ht, gt, ct = refine_sums(Rt, tt, und, cam_a, cam_b, dtype)
        it += 1
        step = np.sqrt(d @ d)
        small = step <= dtype(XTOL) * (dtype(XTOL) + 1)
        if ct < cost:
            flat = cost - ct <= dtype(FTOL) * cost
            R, t, H, g, cost = Rt, tt, Ht, gt, ct
            lam = max(lam * dtype(0.1), dtype(LAMBDA_MIN))
            if flat or small:
                break
        else:
            lam = lam * 10
            if small or lam > LAMBDA_MAX:
                break
    return R, t, it


# ---- one pair ------------------------------------------------------------------------------------------------------------------------
def refine_result(out, und, cam_a, cam_b, refine_iters, dtype):
    """The refinement stage on an OK result: T, n_front, rms and parallax at the refined pose; the unrefined result stays when the refined
    one is not finite or has no row in front."""
    if out["info"][3] != OK or refine_iters <= 0:
        return out
    ui = und[out["inlier"]]
    A, B = rays_of(ui, cam_a, cam_b, dtype)
    R, t, it = refine_pose(out["T"][:, :3], out["T"][:, 3], ui, cam_a, cam_b, refine_iters, dtype)
    n_front, rms, parallax = pose_stats(R, t, ui, A, B, cam_a, cam_b, dtype)
    out["trials"] = it
    if n_front > 0 and np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.isfinite(rms) and np.isfinite(parallax):
        out["T"] = np.concatenate([R, t[:, None]], axis=1)
        out["info"][2] = n_front
        out["stats"][1], out["stats"][2] = rms, parallax
    return out


def two_view_pair(uv_a, uv_b, cam_a, cam_b, pair_index, n_hypotheses=64, inlier_px=2.0, seed=0, min_points=16, solver="five-point",
                  refine_iters=0, dtype=np.float64):
    """One pair, the outputs of ``twoview_reference.two_view_pair``; ``scores`` (H,) is every hypothesis' best slot score."""
    und = np.concatenate([tv.undistort(uv_a, cam_a, dtype), tv.undistort(uv_b, cam_b, dtype)], axis=1)
    if solver == "eight-point":
        out = tv.two_view_pair(uv_a, uv_b, cam_a, cam_b, pair_index, n_hypotheses, inlier_px, seed, min_points, dtype)
        return refine_result(out, und, cam_a, cam_b, refine_iters, dtype)
    n = int(und.shape[0])
    nan = dtype(np.nan)
    out = {"T": np.full((3, 4), nan, dtype=dtype), "info": np.array([n, 0, 0, TOO_FEW, -1], dtype=np.int32),
           "stats": np.full(3, nan, dtype=dtype), "inlier": np.zeros(n, dtype=bool), "scores": None, "slot_scores": None, "e2": None}
    if n < max(SAMPLE, int(min_points)):
        return out
    tau2 = dtype(inlier_px) * dtype(inlier_px)
    A, B = rays_of(und, cam_a, cam_b, dtype)
    slot_scores = np.full((n_hypotheses, SLOTS), np.inf, dtype=dtype)
    poses = {}
    for h in range(n_hypotheses):
        pick = sample_positions(seed, pair_index, n, h, SAMPLE)
        Es, usable = five_point(A[pick], B[pick], dtype)
        for k in range(SLOTS):
            if not usable[k]:
                continue
            F = tv.fundamental(Es[k], cam_a, cam_b, dtype)
            if not np.all(np.isfinite(F)):
                continue
            s, cand, R, t = slot_score(Es[k], F, und, A, B, tau2, dtype)
            if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
                slot_scores[h, k] = s
                poses[(h, k)] = (F, R, t)
    out["slot_scores"], out["scores"] = slot_scores, np.min(slot_scores, axis=1)
    win = int(np.argmin(slot_scores.ravel()))     # ties go to the lower hypothesis, then to the lower root
    out["info"][3] = DEGENERATE
    out["stats"][0] = slot_scores.ravel()[win]
    if not slot_scores.ravel()[win] < np.inf:
        return out
    F, R, t = poses[(win // SLOTS, win % SLOTS)]
    pos, _, _ = depths(R, t, A, B)
    with np.errstate(invalid="ignore"):
        inl = (tv.sampson(F, und) <= tau2) & pos
    n_inl = int(np.sum(inl))
    out["inlier"], out["e2"] = inl, tv.sampson(F, und)
    out["info"][1], out["info"][4] = n_inl, win // SLOTS
    if n_inl < MIN_INLIERS:
        return out
    n_front, rms, parallax = pose_stats(R, t, und[inl], A[inl], B[inl], cam_a, cam_b, dtype)
    out["info"][2] = n_front
    if n_front == 0:
        out["info"][3] = NO_CHEIRALITY
        return out
    if not (np.isfinite(rms) and np.isfinite(parallax)):
        return out
    out["T"], out["info"][3] = np.concatenate([R, t[:, None]], axis=1), OK
    out["stats"][1], out["stats"][2] = rms, parallax
    return refine_result(out, und, cam_a, cam_b, refine_iters, dtype)


def estimate_pairs(uv_a, uv_b, start, pairs, intr, dtype=np.float64, **opts):
    res = [two_view_pair(uv_a[start[p]:start[p + 1]], uv_b[start[p]:start[p + 1]], intr[a], intr[b], p, dtype=dtype, **opts)
           for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2))]
    P = len(res)
    return (np.array([r["T"] for r in res], dtype=dtype).reshape(P, 3, 4), np.array([r["info"] for r in res], dtype=np.int32).reshape(P, 5),
            np.array([r["stats"] for r in res], dtype=dtype).reshape(P, 3),
            np.concatenate([r["inlier"] for r in res]) if P else np.zeros(0, dtype=bool), res)


def run_table(table, opts, dtype=np.float64):
    return estimate_pairs(table["uv_a"], table["uv_b"], table["start"], table["pairs"], table["intr"], dtype=dtype, **opts)


SCORE_FLOOR = 1e-12   # px^2: a score or an RMS below it is the rounding of an exact fit (a pair of five rows fits every root), not a figure


def stats_gap(a, b):
    """max |a - b| / max(|b|, SCORE_FLOOR) over the finite entries of b; entries that are not finite must be the same in both."""
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b)), "non-finite entries differ"
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), SCORE_FLOOR))) if np.any(fin) else 0.0


def rounding(inputs):
    """float64 against extended precision on every input: name -> (d_T, d_s, float64 result); d_T over the entries of T against
    max(|entry|, 1), d_s relative (``stats_gap``) over the best score of every hypothesis and the stats.  The discrete outputs must
    agree."""
    out = {}
    for name, (table, opts) in inputs.items():
        r64, rld = run_table(table, opts), run_table(table, opts, np.longdouble)
        assert np.array_equal(r64[1], rld[1]) and np.array_equal(r64[3], rld[3]), name
        d_s = stats_gap(r64[2], rld[2])
        for a, b in zip(r64[4], rld[4]):
            if a["scores"] is not None:
                d_s = max(d_s, stats_gap(a["scores"], b["scores"]))
        out[name] = (tv.pose_gap(r64[0], rld[0]), d_s, r64)
    return out


def pose_error(T, R_true, t_true):
    """(rotation error, translation-direction error) in radians."""
    T = np.asarray(T, dtype=np.float64)
    c = (np.trace(T[:, :3] @ R_true.T) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1))), float(np.arccos(np.clip(T[:, 3] @ t_true / np.linalg.norm(T[:, 3]), -1, 1)))
